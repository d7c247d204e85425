"""The ranking of the columns of sample paths on the GPU (include/bnf.h bnf_sample_ranks / bnf_rank_probabilities) against
the brute-force references of tests/ranking_ref.py: above, ties and the mid-rank exact, a rank probability within
(S + 8) eps of itself and, as expected of correctly rounded float64 adds and divides, bit for bit the numpy restatement of
the kernel's form.  LDS is poisoned before every call; every test prints what it measured (-s shows it)."""
import copy
import ctypes as C
import os

import numpy as np
import pandas as pd
import pytest
import torch

from bayesnf_amd import BayesianNeuralFieldMAP, BayesianNeuralFieldVI, _native
from bayesnf_amd.engine import Engine
from tests import ranking_ref as R
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


def _dev(eng, a, dtype=np.float64):
  return None if a is None else torch.from_numpy(np.array(a, dtype=dtype)).to(eng.device)      # (a copy)


def _ranks(eng, x, scale=None):
  eng.debug_poison_lds()
  out = eng.sample_ranks(_dev(eng, x), _dev(eng, scale))
  assert set(out) == {'rank', 'above', 'ties'} and all(v.shape == tuple(x.shape) for v in out.values())
  assert out['rank'].dtype == torch.float64 and out['above'].dtype == torch.int32 and out['ties'].dtype == torch.int32
  return {k: v.cpu().numpy() for k, v in out.items()}


def _prob(eng, above, ties, K):
  eng.debug_poison_lds()
  out = eng.rank_probabilities(_dev(eng, above, np.int32), _dev(eng, ties, np.int32), K)
  assert out.shape == (K, above.shape[1]) and out.dtype == torch.float64
  return out.cpu().numpy()


@pytest.mark.parametrize('scaled', [False, True])
@pytest.mark.parametrize('kind', R.KINDS)
def test_grid(eng, kind, scaled):
  """G at 1, 2, 3, around a wave (64), around a workgroup's first pass (256) and a non-power-of-two above 1,024; S at the
  edges of the path chunk and 257; with and without a divisor.  The integers and mid-ranks exact, every path's ranks add up
  to G (G + 1) / 2, rank_prob for K in {1, 2, G} within its bar and bit for bit the restatement."""
  worst, differ, cells = 0.0, 0, 0
  for G in R.GRID_G:
    for S in R.GRID_S:
      x, scale, ref = R.ranking_case(S, G, kind, scaled)
      tag = f'{kind} S={S} G={G}{" scaled" if scaled else ""}'
      got = _ranks(eng, x, scale)
      R.check_ranks(tag, got, ref)
      for K in sorted({1, min(2, G), G}):
        exact, form = R.prob_case(S, G, kind, scaled, K)
        p = _prob(eng, got['above'], got['ties'], K)
        w, d = R.check_prob(f'{tag} K={K}', p, S, exact, form)
        worst, differ, cells = max(worst, w), differ + d, cells + p.size
        assert np.all(np.abs(p.sum(axis=1) - 1.0) <= (S + 8) * R.EPS + G * R.EPS), (tag, K, 'rows sum to 1')
  print(f'{kind}{" scaled" if scaled else ""}: worst rank_prob error / bar {worst:.3f}; {differ} of {cells} cells differ '
        'in bits from the restatement')
  assert differ == 0


def test_the_lds_ceiling(eng):
  """G = 16,384 (128 KiB of keys), S = 2, Poisson totals: the reference by a sort on the host (cross-checked against the
  brute force in tests/test_ranking_host.py); one column more is refused."""
  S, G = 2, R.MAX_COLS
  rng = np.random.default_rng(16384)
  x = R.make_x(S, G, 'count', rng)
  rank, above, ties = R.ranks_sorted(x)
  got = _ranks(eng, x)
  R.check_ranks(f'count S={S} G={G}', got, dict(rank=rank, above=above, ties=ties))
  scale = rng.integers(1, 4, G).astype(np.float64)
  rank, above, ties = R.ranks_sorted(x, scale)
  R.check_ranks(f'count S={S} G={G} scaled', _ranks(eng, x, scale), dict(rank=rank, above=above, ties=ties))
  for K in (1, 2, 33):
    p = _prob(eng, above, ties, K)
    w, d = R.check_prob(f'G={G} K={K}', p, S, *R.rank_prob_both(above, ties, K))
    assert d == 0
  full = _prob(eng, above, ties, R.MAX_CELLS // G)     # the most cells of a call: 1,024 rows
  assert R.same_bits(full[:33], p) and np.all(np.abs(full.sum(axis=1) - 1.0) <= (S + 8 + G) * R.EPS)
  wide = torch.zeros((1, G + 1), dtype=torch.float64, device=eng.device)
  with pytest.raises(ValueError, match='at most 16384'):
    eng.sample_ranks(wide)
  ptr = lambda t: C.c_void_p(t.data_ptr())
  out = torch.zeros((1, G + 1), dtype=torch.float64, device=eng.device)
  assert eng.lib.bnf_sample_ranks(eng.handle, ptr(wide), 1, G + 1, None, ptr(out), None, None) == -1
  assert 'at most 16384' in _native.last_error()
  i32 = torch.ones((1, G), dtype=torch.int32, device=eng.device)
  with pytest.raises(ValueError, match='at most 16777216'):
    eng.rank_probabilities(i32, i32, R.MAX_CELLS // G + 1)


def test_bit_identity(eng):
  """Two calls; the columns permuted (an index-dependent tie-break would show); top_k = 2 against the first rows of
  top_k = G; identical columns; the paths cut into two calls."""
  for kind in R.KINDS:
    S, G = 33, 257
    x, scale, ref = R.ranking_case(S, G, kind, True)
    x, scale = np.array(x), np.array(scale)
    x[:, 200], scale[200] = x[:, 7], scale[7]         # identical columns, far apart
    x[:, 8], scale[8] = x[:, 7], scale[7]             # and next to each other
    a, b = _ranks(eng, x, scale), _ranks(eng, x, scale)
    pa, pb = _prob(eng, a['above'], a['ties'], G), _prob(eng, b['above'], b['ties'], G)
    for k in a:
      assert np.array_equal(a[k], b[k]) and R.same_bits(a['rank'], b['rank']), (kind, k)
    assert R.same_bits(pa, pb)
    for k in a:
      assert np.array_equal(a[k][:, 200], a[k][:, 7]) and np.array_equal(a[k][:, 8], a[k][:, 7]), (kind, k)
    assert R.same_bits(pa[:, 200], pa[:, 7]) and R.same_bits(pa[:, 8], pa[:, 7])
    assert np.all(a['ties'][:, [7, 8, 200]] >= 3)
    perm = np.random.default_rng(3).permutation(G)
    c = _ranks(eng, x[:, perm], scale[perm])
    for k in a:
      assert np.array_equal(c[k], a[k][:, perm]), (kind, k, 'columns permuted')
    assert R.same_bits(_prob(eng, c['above'], c['ties'], G), pa[:, perm])
    assert R.same_bits(_prob(eng, a['above'], a['ties'], 2), pa[:2])
    assert R.same_bits(_prob(eng, a['above'], a['ties'], 17), pa[:17])      # a second block of k, ragged
    first, rest = _ranks(eng, x[:20], scale), _ranks(eng, x[20:], scale)
    for k in a:
      assert np.array_equal(np.concatenate([first[k], rest[k]]), a[k]), (kind, k, 'paths cut in two')
    plain = _ranks(eng, R.values(x, scale))           # the division on the host: the same IEEE quotient
    for k in a:
      assert np.array_equal(plain[k], a[k]), (kind, k, 'scale')


def test_outputs_alone_and_the_library_errors(eng):
  x, _, ref = R.ranking_case(33, 65, 'count')
  xd = _dev(eng, x)
  ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
  S, G = x.shape
  rank = torch.zeros((S, G), dtype=torch.float64, device=eng.device)
  above, ties = (torch.zeros((S, G), dtype=torch.int32, device=eng.device) for _ in range(2))
  call = lambda **k: eng.lib.bnf_sample_ranks(eng.handle, k.get('x', ptr(xd)), k.get('S', S), k.get('G', G), None,
                                               k.get('rank', ptr(rank)), k.get('above', ptr(above)), k.get('ties', ptr(ties)))
  eng.debug_poison_lds()
  assert call(rank=None, above=None) == 0 and call(ties=None, above=None) == 0 and call(rank=None, ties=None) == 0
  torch.cuda.synchronize()
  assert np.array_equal(rank.cpu().numpy(), ref['rank']) and np.array_equal(above.cpu().numpy(), ref['above'])
  assert np.array_equal(ties.cpu().numpy(), ref['ties'])
  assert call(rank=None, above=None, ties=None) == -1 and 'no output' in _native.last_error()
  assert call(S=0) == -1 and call(G=0) == -1 and call(x=None) == -1
  out = torch.zeros((G, G), dtype=torch.float64, device=eng.device)
  prob = lambda **k: eng.lib.bnf_rank_probabilities(eng.handle, k.get('above', ptr(above)), ptr(ties), k.get('S', S),
                                                    k.get('G', G), k.get('K', 3), k.get('out', ptr(out)))
  assert prob() == 0
  torch.cuda.synchronize()
  assert prob(K=0) == -1 and 'top_k = 0' in _native.last_error()
  assert prob(K=G + 1) == -1 and prob(S=0) == -1 and prob(G=0) == -1 and prob(above=None) == -1 and prob(out=None) == -1
  for bad in (0, G + 1):
    with pytest.raises(ValueError, match=f'top_k={bad}'):
      eng.rank_probabilities(above, ties, bad)
  with pytest.raises(ValueError, match='int32'):
    eng.rank_probabilities(above.to(torch.int64), ties, 1)
  with pytest.raises(ValueError, match='n_samples, n_cols'):
    eng.sample_ranks(torch.zeros(4, dtype=torch.float64, device=eng.device))
  with pytest.raises(ValueError, match='shape'):
    eng.sample_ranks(xd, np.ones(G + 1))


def test_the_score_sees_the_ranking_on_the_device(eng):
  """The inputs of tests/test_ranking_host.py: the mid-ranks of the graded groups summarised by bnf_sample_summaries
  against the observed ranks; with the columns reversed the mean rank CRPS is at least 4 times as large."""
  x, y = R.graded_case(0)
  obs = _ranks(eng, y[None, :])['rank'][0]
  assert np.array_equal(obs, R.ranks_brute(y[None, :])[0][0])
  crps = []
  for v in (x, x[:, ::-1]):
    rank = _ranks(eng, np.ascontiguousarray(v))['rank']
    eng.debug_poison_lds()
    crps.append(float(eng.sample_summaries(_dev(eng, rank), _dev(eng, obs))['crps'].cpu().numpy().mean()))
  ref = R.mean_rank_crps(x, y)
  print(f'mean rank CRPS {crps[0]:.4f} (reference {ref:.4f}), columns reversed {crps[1]:.4f}, ratio {crps[1] / crps[0]:.1f}')
  assert crps[1] >= 4 * crps[0] and abs(crps[0] - ref) <= 1e-12 * ref


# ---- end to end ----------------------------------------------------------------------------------------------------------
def _fit(golden_dir, kind, obs):
  df = pd.read_csv(os.path.join(golden_dir, 'chickenpox.8.train.csv'), index_col=0, parse_dates=['datetime'])
  if kind == 'map':
    est = BayesianNeuralFieldMAP(**MODEL, observation_model=obs, compute_dtype='fp32').fit(
        df, seed=3, ensemble_size=4, num_epochs=5, learning_rate=0.01)
  else:
    est = BayesianNeuralFieldVI(**MODEL, observation_model=obs, compute_dtype='fp32').fit(
        df, seed=1, ensemble_size=2, num_epochs=10, learning_rate=0.01, sample_size_posterior=5)
  return df, est


def _table(df):
  """5 places x 6 weeks around the fixture's county, with a population per place."""
  weeks = df['datetime'].iloc[:6].to_numpy()
  rng = np.random.default_rng(9)
  places = ['p0', 'p1', 'p2', 'p3', 'p4']
  t = pd.DataFrame({'location': np.repeat(places, 6), 'datetime': np.tile(weeks, 5),
                    'latitude': np.repeat(df['latitude'].iloc[0] + np.linspace(-0.5, 0.5, 5), 6),
                    'longitude': np.repeat(df['longitude'].iloc[0] + np.linspace(0.4, -0.4, 5), 6),
                    'chickenpox': rng.poisson(20.0, 30).astype(np.float64),
                    'people': np.repeat([1000.0, 250.0, 4000.0, 500.0, 2000.0], 6)})
  return t.sample(frac=1.0, random_state=2).reset_index(drop=True)


def _reference(totals, scale, K, levels, observed=None):
  """Everything predict_ranking / score_ranking report, from the host copy of the totals."""
  rank, above, ties = R.ranks_brute(totals, scale)
  ref = dict(rank=rank, prob=R.rank_prob_ref(above, ties, K), mean=rank.mean(axis=0), quantiles=T.quantiles_ref(rank, levels))
  if observed is not None:
    o_rank, o_above, o_ties = R.ranks_brute(observed[None, :], scale)
    ref.update(observed_rank=o_rank[0], above=o_above[0], ties=o_ties[0], crps=T.crps_ref(rank, o_rank[0]),
               pit=T.pit_ref(rank, o_rank[0]))
  return ref


def _check_forecast(tag, res, ref, S, levels, y=None):
  got = dict(mean=res['rank_mean'], quantiles=res['rank_quantiles'])
  if y is not None:
    got.update(crps=res['rank_crps'], pit=res['rank_pit'])
  T.check_summaries(tag, got, ref['rank'], y, levels, ref)
  w, _ = R.check_prob(tag, res['rank_probability'], S, ref['prob'])
  assert R.same_bits(res['top_probability'], np.cumsum(res['rank_probability'], axis=0))
  print(f'{tag}: rank_prob error / bar {w:.3f}; P(top 1) {np.round(res["rank_probability"][0], 3).tolist()}')


@pytest.mark.parametrize('kind,obs', [('map', 'NORMAL'), ('map', 'ZINB'), ('vi', 'NORMAL'), ('vi', 'ZINB')])
def test_estimator_ranking(golden_dir, kind, obs):
  """predict_ranking / score_ranking on 5 places x 6 weeks == the reference ranking of the host copy
  predict_samples(table, S, seed, group_by='location'): rank_mean / rank_quantiles / rank_crps / rank_pit at the bars
  tests/test_gpu_totals.py holds bnf_sample_summaries to, the probabilities at theirs."""
  df, est = _fit(golden_dir, kind, obs)
  table = _table(df)
  S, seed, K, levels = 300, 3, 3, (0.025, 0.5, 0.975)
  totals, keys = est.predict_samples(table, S, seed, group_by='location')
  G = len(keys)
  assert totals.shape == (S, 5)
  ref = _reference(totals, None, K, levels)
  pred = est.predict_ranking(table, 'location', top_k=K, quantiles=levels, num_samples=S, seed=seed)
  assert set(pred) == {'keys', 'rank_mean', 'rank_quantiles', 'rank_probability', 'top_probability', 'most_likely_top'}
  assert pred['keys'].equals(keys) and pred['rank_probability'].shape == (K, G)
  _check_forecast(f'{kind} {obs} predict', pred, ref, S, levels)
  assert pred['most_likely_top'] == keys[int(np.argmax(ref['prob'][0]))]
  assert np.all(np.abs(pred['rank_probability'].sum(axis=1) - 1.0) <= (S + 16) * R.EPS)

  # all groups observed: the scored forecast is the plain one
  observed = table.groupby('location')['chickenpox'].sum().reindex(keys).to_numpy(dtype=np.float64)
  ref = _reference(totals, None, K, levels, observed)
  res = est.score_ranking(table, 'location', top_k=K, quantiles=levels, num_samples=S, seed=seed)
  assert res['n'] == G and np.array_equal(res['observed'], observed) and np.array_equal(res['observed_rank'], ref['observed_rank'])
  _check_forecast(f'{kind} {obs} score', res, ref, S, levels, ref['observed_rank'])
  for k in ('rank_mean', 'rank_quantiles', 'rank_probability'):
    assert R.same_bits(res[k], pred[k]), k
  kk = np.arange(1, K + 1)[:, None]
  assert np.array_equal(res['observed_top'], np.clip((kk - ref['above'][None, :]) / ref['ties'][None, :], 0.0, 1.0))
  assert np.allclose(res['top_brier'], np.mean((res['top_probability'] - res['observed_top']) ** 2, axis=1), rtol=1e-14)
  assert res['mean_rank_crps'] == float(np.mean(res['rank_crps']))

  # weights that sit on one member: that member alone
  lead = np.shape(est.score(table)['member_log_prob'])
  onehot = np.zeros(lead)
  onehot.reshape(-1)[1] = 1.0
  idx = tuple(slice(i, i + 1) for i in np.unravel_index(1, lead))
  alone = copy.copy(est)
  alone.params_ = tuple(np.asarray(p)[idx] for p in est.params_)
  one = est.predict_ranking(table, 'location', top_k=K, quantiles=levels, num_samples=S, seed=seed, weights=onehot)
  solo = alone.predict_ranking(table, 'location', top_k=K, quantiles=levels, num_samples=S, seed=seed)
  for k in ('rank_mean', 'rank_quantiles', 'rank_probability'):
    assert R.same_bits(one[k], solo[k]), ('one member', k)
  assert not R.same_bits(one['rank_probability'], pred['rank_probability'])
  tw, _ = est.predict_samples(table, S, seed, group_by='location', weights=onehot)
  _check_forecast(f'{kind} {obs} one member', one, _reference(tw, None, K, levels), S, levels)

  # a NaN target in one group: its columns are NaN, n = 4, the rest is the reference on the four scored groups
  d = table.copy()
  d.loc[d.index[d['location'] == 'p2'][0], 'chickenpox'] = np.nan
  res2 = est.score_ranking(d, 'location', top_k=K, quantiles=levels, num_samples=S, seed=seed)
  gone = np.asarray(keys == 'p2')
  assert res2['n'] == 4 and np.array_equal(np.isnan(res2['observed']), gone)
  for k in ('rank_mean', 'rank_crps', 'observed_rank', 'observed_rank_probability'):
    assert np.isnan(res2[k][gone]).all() and (k == 'observed_rank_probability' or not np.isnan(res2[k][~gone]).any()), k
  for k in ('rank_quantiles', 'rank_probability', 'top_probability', 'rank_pit', 'observed_top'):
    assert np.isnan(res2[k][:, gone]).all() and not np.isnan(res2[k][:, ~gone]).any(), k
  ref4 = _reference(totals[:, ~gone], None, K, levels, observed[~gone])
  sub = {k: (v[..., ~gone] if isinstance(v, np.ndarray) and v.ndim and v.shape[-1] == G else v) for k, v in res2.items()}
  _check_forecast(f'{kind} {obs} four scored groups', sub, ref4, S, levels, ref4['observed_rank'])
  assert np.array_equal(sub['observed_rank'], ref4['observed_rank'])
  assert np.allclose(res2['top_brier'], np.mean((sub['top_probability'] - sub['observed_top']) ** 2, axis=1), rtol=1e-14)
  block = np.asarray([sub['rank_probability'][a:min(a + t, K), g].sum() if a < K else np.nan
                      for g, (a, t) in enumerate(zip(ref4['above'], ref4['ties']))])
  assert np.allclose(sub['observed_rank_probability'], block, rtol=1e-14, equal_nan=True)

  # per as a column == the divisor applied by hand
  scale = table.groupby('location')['people'].first().reindex(keys).to_numpy(dtype=np.float64)
  per = est.score_ranking(table, 'location', top_k=G, per='people', quantiles=levels, num_samples=S, seed=seed)
  refp = _reference(totals, scale, G, levels, observed)
  _check_forecast(f'{kind} {obs} per head', per, refp, S, levels, refp['observed_rank'])
  assert np.array_equal(per['observed_rank'], refp['observed_rank']) and not np.array_equal(per['observed_rank'], res['observed_rank'])
  assert np.all(np.abs(per['rank_probability'].sum(axis=0) - 1.0) <= (S + 16) * R.EPS)        # top_k = G: columns too
  by_row = est.predict_ranking(table, 'location', top_k=G, per=table['people'].to_numpy(), quantiles=levels, num_samples=S,
                               seed=seed)
  assert R.same_bits(by_row['rank_probability'], per['rank_probability'])
