"""Summaries and scores of sample paths on the GPU (include/bnf.h bnf_sample_summaries / bnf_sample_energy_score) against
the brute-force float64 references of tests/totals_ref.py, at the bars stated there (each from float64 rounding: pit exact,
a quantile 4 eps of its neighbours, the mean S eps max|x|, the CRPS S eps max|x - y|, the energy score
(G + 2 S + 64) eps (T1 + T2)).  LDS is poisoned before every call; every test prints what it measured (-s shows it)."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

from bayesnf_amd import BayesianNeuralFieldMAP, BayesianNeuralFieldVI
from bayesnf_amd.engine import Engine
from tests import totals_ref as T
from tests import util
from tests.test_gpu_sampling import MODEL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
  net, _, _, _ = util.make_problem(n_rows=16, width=64, depth=1, observation_model='NORMAL')
  e = Engine(net, members=1, forward_only=True, row_capacity=128, compute_dtype='fp32')
  yield e
  e.close()


def _summ(eng, x, y=None, q=T.LEVELS):
  eng.debug_poison_lds()
  dev = lambda a: None if a is None else torch.from_numpy(np.array(a, dtype=np.float64)).to(eng.device)   # (a copy)
  out = eng.sample_summaries(dev(x), dev(y), q)
  G = x.shape[1]
  assert set(out) == ({'mean', 'quantiles'} if y is None else {'mean', 'quantiles', 'crps', 'pit'})
  assert out['mean'].shape == (G,) and out['quantiles'].shape == (len(q), G)
  assert all(v.dtype == torch.float64 for v in out.values())
  return {k: v.cpu().numpy() for k, v in out.items()}


def _energy(eng, x, y):
  eng.debug_poison_lds()
  dev = lambda a: torch.from_numpy(np.array(a, dtype=np.float64)).to(eng.device)
  return eng.sample_energy_score(dev(x), dev(y))


def _same_bits(a, b):
  return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


@pytest.mark.parametrize('kind', T.KINDS)
def test_summaries_grid(eng, kind):
  """S in {1, 2, 63, 64, 65, 1000} x n_cols in {1, 9, 65}; y by column: a tied sample value, below every sample, above
  every sample, NaN, between.  With the NaN columns left out of the call the other columns keep their bits."""
  worst = {}
  for S in T.SUMMARY_S:
    for G in T.SUMMARY_G:
      x, y, ref = T.summary_case(S, G, kind)
      got = _summ(eng, x, y)
      w = T.check_summaries(f'{kind} S={S} G={G} device', got, x, y, T.LEVELS, ref)
      for k, v in w.items():
        worst[k] = max(worst.get(k, 0.0), v)
      keep = np.isfinite(y)
      if not keep.all():
        assert np.isnan(got['crps'][~keep]).all() and np.isfinite(got['mean'][~keep]).all()
        alone = _summ(eng, x[:, keep], y[keep])
        for k in got:
          assert _same_bits(got[k][..., keep], alone[k]), (kind, S, G, k)
  print(f'{kind}: worst device error / bar {worst}')


def test_a_total_of_1e9_with_a_spread_of_10(eng):
  x, y, ref = T.summary_case(65, 9, 'big')
  got = _summ(eng, x, y)
  T.check_summaries('1e9 + small integers, device', got, x, y, T.LEVELS, ref)
  scored = np.isfinite(y)
  assert np.array_equal(got['crps'][scored], ref['crps'][scored])      # every term is an exact integer on x - y


def test_a_column_with_one_nan_sample(eng):
  x, y, ref = T.summary_case(65, 9, 'normal')
  xn = np.array(x)
  xn[17, 4] = np.nan
  got, clean = _summ(eng, xn, y), _summ(eng, x, y)
  for k in got:
    assert np.isnan(got[k][..., 4]).all(), k
    others = np.arange(9) != 4
    assert _same_bits(got[k][..., others], clean[k][..., others]), k
  T.check_summaries('NaN sample, device', got, xn, y, T.LEVELS, ref)


def test_the_cap(eng):
  """One column at S = 16,384 (128 KiB of LDS); one path more is the library's error."""
  S = T.MAX_SAMPLES
  rng = np.random.default_rng(16384)
  x = T.make_x(S, 1, 'normal', rng)
  y = np.asarray([float(x[5, 0])])
  ref = dict(mean=np.asarray([np.sum(np.sort(x[:, 0])) / S]), quantiles=T.quantiles_ref(x, T.LEVELS), crps=T.crps_ref(x, y),
             pit=T.pit_ref(x, y))
  got = _summ(eng, x, y)
  T.check_summaries(f'S={S} G=1 device', got, x, y, T.LEVELS, ref)
  two = np.concatenate([x, x[::-1]], axis=1)         # two columns with the same multiset: the slab does not matter
  both = _summ(eng, two, np.repeat(y, 2))
  for k in got:
    assert _same_bits(both[k][..., 0], got[k][..., 0]) and _same_bits(both[k][..., 1], got[k][..., 0]), k
  with pytest.raises(ValueError, match='at most 16384'):
    eng.sample_summaries(torch.zeros((S + 1, 1), dtype=torch.float64, device=eng.device))
  with pytest.raises(ValueError, match='at most 16384'):
    eng.sample_energy_score(torch.zeros((S + 1, 1), dtype=torch.float64, device=eng.device), np.zeros(1))


def test_two_calls_give_equal_bits_and_a_pure_summary(eng):
  x, y, ref = T.summary_case(1000, 65, 'normal')
  a, b = _summ(eng, x, y), _summ(eng, x, y)
  for k in a:
    assert _same_bits(a[k], b[k]), k
  pure = _summ(eng, x, None)
  assert _same_bits(pure['mean'], a['mean']) and _same_bits(pure['quantiles'], a['quantiles'])
  none = _summ(eng, x, y, q=())
  assert none['quantiles'].shape == (0, 65) and _same_bits(none['crps'], a['crps'])
  levels = tuple(np.linspace(0.0, 1.0, 70))          # more levels than one call takes
  many = _summ(eng, x, y, q=levels)
  err, bars = np.abs(many['quantiles'] - T.quantiles_ref(x, levels)), T.quantile_bars(x, levels)
  print(f'70 levels: worst quantile error {err.max():.2e}, cells over the bar {(err > bars).sum()}')
  assert np.all(err <= bars) and _same_bits(many['crps'], a['crps']) and _same_bits(many['mean'], a['mean'])
  with pytest.raises(ValueError, match=r'outside \[0, 1\]'):
    eng.sample_summaries(torch.zeros((4, 2), dtype=torch.float64, device=eng.device), q=(0.5, 1.01))
  with pytest.raises(ValueError, match='shape'):
    eng.sample_summaries(torch.zeros((4, 2), dtype=torch.float64, device=eng.device), np.zeros(3))


@pytest.mark.parametrize('S,G', T.ENERGY_SHAPES)
def test_energy_score(eng, S, G):
  x, y, (ref, t1, t2) = T.energy_case(S, G)
  got, again = _energy(eng, x, y), _energy(eng, x, y)
  bar = T.energy_bar(S, G, t1, t2)
  print(f'S={S} G={G}: energy {ref:.9f} device error {abs(got - ref):.2e} bar {bar:.2e} ({abs(got - ref) / bar:.3f})')
  assert abs(got - ref) <= bar
  assert _same_bits(got, again)
  # NaN columns are skipped: the score on the kept columns alone
  yn = np.array(y)
  yn[::3] = np.nan
  keep = np.isfinite(yn)
  if keep.any():
    kept_ref, k1, k2 = T.energy_ref(x[:, keep], y[keep])
    with_nan, alone = _energy(eng, x, yn), _energy(eng, x[:, keep], y[keep])
    kbar = T.energy_bar(S, int(keep.sum()), k1, k2)
    print(f'  {int((~keep).sum())} NaN columns: error {abs(with_nan - kept_ref):.2e}, alone {abs(alone - kept_ref):.2e}, bar {kbar:.2e}')
    assert abs(with_nan - kept_ref) <= kbar and abs(alone - kept_ref) <= kbar
  assert np.isnan(_energy(eng, x, np.full(G, np.nan)))


def test_energy_of_identical_paths_is_the_first_term(eng):
  """Every pair distance is exactly 0.  With differences (3, 4, 0, ...) from y the norm is exactly 5 and so is the score;
  for a generic path the score is the one norm within its own roundings (G / 2 + 2 S of them)."""
  S, G = 65, 130
  y = np.arange(G, dtype=np.float64)
  row = y.copy()
  row[7] += 3.0
  row[101] -= 4.0
  got = _energy(eng, np.tile(row, (S, 1)), y)
  print(f'identical integer paths: {got!r}')
  assert got == 5.0
  x, yy, _ = T.energy_case(S, G)
  one = np.tile(x[3], (S, 1))
  ref, t1, t2 = T.energy_ref(one, yy)
  got = _energy(eng, one, yy)
  print(f'identical paths: error {abs(got - ref):.2e} bar {T.energy_bar(S, G, t1, 0.0):.2e}')
  assert t2 == 0.0 and abs(got - ref) <= T.energy_bar(S, G, t1, 0.0)
  assert abs(got - _energy(eng, x[3:4], yy)) <= T.energy_bar(S, G, t1, 0.0)


# ---- end to end ----------------------------------------------------------------------------------------------------------
def _frame(golden_dir):
  return pd.read_csv(os.path.join(golden_dir, 'chickenpox.8.train.csv'), index_col=0, parse_dates=['datetime'])


def _fit(kind, df):
  if kind == 'map':
    return BayesianNeuralFieldMAP(**MODEL, observation_model='NB', compute_dtype='fp32').fit(
        df, seed=3, ensemble_size=4, num_epochs=5, learning_rate=0.01)
  return BayesianNeuralFieldVI(**MODEL, observation_model='NORMAL', compute_dtype='fp32').fit(
      df, seed=1, ensemble_size=2, num_epochs=10, learning_rate=0.01, sample_size_posterior=5)


@pytest.mark.parametrize('kind', ['map', 'vi'])
def test_estimator_totals(golden_dir, kind):
  """score_totals(df, 'datetime', num_samples=300, seed=3) == the reference functions applied to the totals
  predict_samples(df, 300, 3, group_by='datetime') returns, observed from a pandas groupby; predict_totals gives the same
  mean and quantiles."""
  df = _frame(golden_dir)
  est = _fit(kind, df)
  levels = (0.025, 0.5, 0.975)
  res = est.score_totals(df, 'datetime', num_samples=300, seed=3)
  assert set(res) == {'keys', 'observed', 'mean', 'quantiles', 'crps', 'pit', 'n', 'mean_crps', 'energy_score'}
  totals, keys = est.predict_samples(df, 300, 3, group_by='datetime')
  G = len(keys)
  assert totals.shape == (300, G) and res['keys'].equals(keys)
  observed = df.groupby('datetime')['chickenpox'].sum().reindex(keys).to_numpy(dtype=np.float64)
  assert np.array_equal(res['observed'], observed) and res['n'] == G
  ref = dict(mean=totals.mean(axis=0), quantiles=T.quantiles_ref(totals, levels), crps=T.crps_ref(totals, observed),
             pit=T.pit_ref(totals, observed))
  T.check_summaries(f'{kind} chickenpox weeks (G={G})', res, totals, observed, levels, ref)
  es, t1, t2 = T.energy_ref(totals, observed)
  bar = T.energy_bar(300, G, t1, t2)
  print(f'{kind}: energy score {es:.6f} device error {abs(res["energy_score"] - es):.2e} bar {bar:.2e}; '
        f'mean crps {res["mean_crps"]:.4f}')
  assert abs(res['energy_score'] - es) <= bar
  assert abs(res['mean_crps'] - ref['crps'].mean()) <= T.crps_bars(totals, observed).max()
  mean, q, keys2 = est.predict_totals(df, 'datetime', quantiles=levels, num_samples=300, seed=3)
  assert keys2.equals(keys) and len(q) == 3
  assert _same_bits(mean, res['mean']) and _same_bits(np.stack(q), res['quantiles'])
  # groups with a NaN target row are not scored, in the per-group scores and in the energy score
  d = df.copy()
  d.loc[d.index[[1, 5]], 'chickenpox'] = np.nan
  res2 = est.score_totals(d, 'datetime', num_samples=300, seed=3, energy=False)
  gone = np.isnan(res2['observed'])
  assert 1 <= gone.sum() <= 2 and res2['n'] == G - gone.sum() and 'energy_score' not in res2
  assert np.array_equal(np.isnan(res2['crps']), gone) and _same_bits(res2['crps'][~gone], res['crps'][~gone])
  assert _same_bits(res2['mean'], res['mean'])
