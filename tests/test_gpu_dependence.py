"""Covariance, variogram and variogram score of sample paths on the GPU (include/bnf.h bnf_sample_pair_moments) against the
brute-force float64 references of tests/dependence_ref.py, at the bars stated there (each from float64 rounding: the mean
S eps max|x|, a variogram cell (S + 8) eps of itself, a covariance cell (S + 8) eps A_ij + (S eps)^2 max|x_i| max|x_j|, the
score the propagated cell bars + (n_pairs + 8) eps of itself).  LDS is poisoned before every call; every test prints what
it measured (-s shows it)."""
import ctypes as C
import os

import numpy as np
import pandas as pd
import pytest
import torch

from bayesnf_amd import BayesianNeuralFieldMAP, BayesianNeuralFieldVI, _native, inference
from bayesnf_amd.engine import Engine
from tests import dependence_ref as D
from tests import util
from tests.test_gpu_sampling import MODEL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
  net, _, _, _ = util.make_problem(n_rows=16, width=64, depth=1, observation_model='NORMAL')
  e = Engine(net, members=1, forward_only=True, row_capacity=128, compute_dtype='fp32')
  yield e
  e.close()


def _moments(eng, x, p, y=None, w=None, matrices=True):
  eng.debug_poison_lds()
  dev = lambda a: None if a is None else torch.from_numpy(np.array(a, dtype=np.float64)).to(eng.device)   # (a copy)
  out = eng.sample_pair_moments(dev(x), p, dev(y), dev(w), matrices=matrices)
  G = x.shape[1]
  want = {'mean'} | ({'covariance', 'variogram'} if matrices else set()) | ({'variogram_score'} if y is not None else set())
  assert set(out) == want
  assert out['mean'].shape == (G,) and all(out[k].shape == (G, G) for k in ('covariance', 'variogram') if k in out)
  assert all(v.dtype == torch.float64 for v in out.values() if isinstance(v, torch.Tensor))
  return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def _same_bits(a, b):
  return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


def _whole_and_symmetric(got):
  for k in ('covariance', 'variogram'):
    assert _same_bits(got[k], got[k].T), k
  assert _same_bits(np.diagonal(got['variogram']), np.zeros(len(got['mean'])))      # +0.0 exactly


@pytest.mark.parametrize('kind', D.KINDS)
def test_grid(eng, kind):
  """S at the edges of the path chunk and 1000, G at the edges of the column tile and 2 tile + 2 (three tiles a side, a
  ragged last one, off-diagonal tiles; at S = 2 and chunk + 1 only: its fsum reference takes seconds at S = 1000), every p,
  y with NaN in the columns 3 (mod 5).  matrices=False gives the same score bits."""
  worst = {}
  for S in D.GRID_S:
    for G in D.GRID_G:
      if G == D.GRID_G[-1] and S not in D.GRID_S_AT_LARGEST_G:
        continue
      x, y, ref = D.dependence_case(S, G, kind)
      for p in D.ORDERS:
        got = _moments(eng, x, p, y)
        w = D.check_moments(f'{kind} S={S} G={G} p={p} device', got, x, y, p, ref)
        for k, v in w.items():
          worst[k] = max(worst.get(k, 0.0), v)
        _whole_and_symmetric(got)
        assert np.isnan(got['variogram_score']) == (np.isfinite(y).sum() < 2)
        alone = _moments(eng, x, p, y, matrices=False)
        assert _same_bits(alone['variogram_score'], got['variogram_score']) and _same_bits(alone['mean'], got['mean'])
      pure = _moments(eng, x, 1.0)
      assert _same_bits(pure['covariance'], got['covariance']) and 'variogram_score' not in pure
  print(f'{kind}: worst device error / bar {worst}')


def test_bit_identity(eng):
  """Two calls; a duplicated column; a call on a subset of the columns (other tiles, other neighbours, another G)."""
  S, G = 65, 130
  x = np.array(D.dependence_case(D.CHUNK + 1, G, 'normal')[0])
  x = np.concatenate([x, x[::-1][:S - x.shape[0]] * 1.5 + 0.25], axis=0)
  x[:, 70] = x[:, 3]                               # identical columns, in different tiles
  x[:, 9] = x[:, 8]                                # and within one thread's neighbourhood
  y = np.array(D.make_y(x, 'normal', np.random.default_rng(5)))
  keep = np.ones(G, dtype=bool)
  keep[[1, 64, 100]] = False
  for p in D.ORDERS:
    a, b = _moments(eng, x, p, y), _moments(eng, x, p, y)
    for k in a:
      assert _same_bits(a[k], b[k]), (p, k)
    _whole_and_symmetric(a)
    assert a['variogram'][3, 70] == 0.0 and a['variogram'][70, 3] == 0.0 and a['variogram'][8, 9] == 0.0
    assert _same_bits(a['covariance'][3], a['covariance'][70]) and _same_bits(a['variogram'][:, 8], a['variogram'][:, 9])
    sub = _moments(eng, x[:, keep], p, y[keep])
    assert _same_bits(sub['mean'], a['mean'][keep])
    for k in ('covariance', 'variogram'):
      assert _same_bits(sub[k], a[k][np.ix_(keep, keep)]), (p, k)
    alone = _moments(eng, x, p, y, matrices=False)
    assert _same_bits(alone['variogram_score'], a['variogram_score'])
    few = _moments(eng, x[:7], p, y)               # one ragged chunk
    one = _moments(eng, x[:7, 5:6], p)
    assert _same_bits(one['covariance'][0, 0], few['covariance'][5, 5]) and one['variogram'][0, 0] == 0.0


def test_a_total_of_1e9_with_a_spread_of_10(eng):
  """Centred products: the covariance within its bar; integer differences: the variogram at p = 1 and 2 bit for bit."""
  for S, G in ((65, 9), (D.CHUNK + 1, D.TILE + 2)):
    x, y, ref = D.dependence_case(S, G, 'big')
    for p in D.ORDERS:
      got = _moments(eng, x, p, y)
      D.check_moments(f'1e9 + small integers S={S} G={G} p={p} device', got, x, y, p, ref)
      _whole_and_symmetric(got)
      if p != 0.5:
        assert _same_bits(got['variogram'], ref['vario'][p])
    naive = np.abs((x * x).mean(axis=0) - x.mean(axis=0) ** 2 - np.diagonal(ref['cov']))
    print(f'  E[xx] - E[x]^2 would be off by {naive.max():.3g} on variances of {np.diagonal(ref["cov"]).mean():.3g}')


def test_a_column_with_one_nan_sample(eng):
  S, G, c = D.CHUNK + 1, D.TILE + 1, 4
  x, y, ref = D.dependence_case(S, G, 'normal')
  xn = np.array(x)
  xn[17, c] = np.nan
  others = np.arange(G) != c
  y_out = np.array(y)
  y_out[c] = np.nan
  assert np.isfinite(y[c])
  for p in D.ORDERS:
    got, clean = _moments(eng, xn, p, y), _moments(eng, x, p, y)
    for k in ('covariance', 'variogram'):
      assert np.isnan(got[k][c]).all() and np.isnan(got[k][:, c]).all(), (p, k)
      assert _same_bits(got[k][np.ix_(others, others)], clean[k][np.ix_(others, others)]), (p, k)
    assert np.isnan(got['mean'][c]) and _same_bits(got['mean'][others], clean['mean'][others])
    assert np.isnan(got['variogram_score'])         # the column is scored
    left = _moments(eng, xn, p, y_out)
    score, e, wt = D.score_ref(ref['vario'][p], y_out, p)
    bar = D.score_bar(S, ref['vario'][p], y_out, p, score, e, wt)
    err = abs(left['variogram_score'] - score)
    print(f'p={p}: NaN column left out by its y: score {score:.6g} device error {err:.2e} bar {bar:.2e} ({err / bar:.3f})')
    assert err <= bar
    assert _same_bits(left['variogram_score'], _moments(eng, x, p, y_out)['variogram_score'])


def test_pair_weights(eng):
  S, G = D.CHUNK + 1, D.TILE + 1
  x, y, ref = D.dependence_case(S, G, 'normal')
  rng = np.random.default_rng(3)
  w = rng.uniform(0.0, 3.0, (G, G))
  w = w + w.T
  w[:20, 40:] = w[40:, :20] = 0.0                  # a block of pairs switched off
  gone = np.zeros(G, dtype=bool)
  gone[10:30] = True
  w_cols = np.where(gone[:, None] | gone[None, :], 0.0, 1.0)      # every pair of the columns 10..29 switched off
  y_cols = np.where(gone, np.nan, y)
  for p in D.ORDERS:
    for tag, weights, y_ref, w_ref in (('random weights, a zero block', w, y, w), ('columns 10..29 at weight 0', w_cols, y_cols, None)):
      got = _moments(eng, x, p, y, weights)
      D.check_moments(f'p={p} {tag}', got, x, y_ref, p, ref, ref_score=D.score_ref(ref['vario'][p], y_ref, p, w_ref))
    one = _moments(eng, x, p, y, matrices=False)['variogram_score']
    two = _moments(eng, x, p, y, np.full((G, G), 2.0), matrices=False)['variogram_score']
    n_pairs = len(D.scored_pairs(y)[0])
    print(f'p={p}: weights 2: {two!r} against 2 x {one!r}; relative difference {abs(two - 2 * one) / (2 * one):.2e}')
    assert abs(two - 2 * one) <= (n_pairs + 8) * D.EPS * 2 * one
  with pytest.raises(ValueError, match='need y'):
    eng.sample_pair_moments(torch.zeros((4, 2), dtype=torch.float64, device=eng.device), pair_weights=np.ones((2, 2)))
  with pytest.raises(ValueError, match='shape'):
    eng.sample_pair_moments(torch.zeros((4, 2), dtype=torch.float64, device=eng.device), y=np.zeros(2), pair_weights=np.ones((2, 3)))


def test_the_score_sees_dependence_on_the_device(eng):
  """The inputs and the factor of tests/test_dependence_host.py: every column permuted over the paths keeps the marginals
  and loses the shared factor; the device's score at p = 0.5 is at least 5 times as large."""
  x, shuffled, y = D.shared_factor_case(0)
  good, bad = _moments(eng, x, 0.5, y), _moments(eng, shuffled, 0.5, y)
  ref = D.score_ref(D.vario_ref(x, 0.5), y, 0.5)[0]
  print(f'score {good["variogram_score"]:.4f} (reference {ref:.4f}), columns permuted {bad["variogram_score"]:.4f}, '
        f'ratio {bad["variogram_score"] / good["variogram_score"]:.1f}')
  assert bad['variogram_score'] >= 5 * good['variogram_score']
  assert np.allclose(np.diagonal(good['covariance']), np.diagonal(bad['covariance']), rtol=1e-12)      # the same marginals
  off = ~np.eye(12, dtype=bool)
  assert D.correlation(good['covariance'])[off].min() > 0.9 and np.abs(D.correlation(bad['covariance'])[off]).max() < 0.3


def test_the_caps_and_the_library_errors(eng):
  """More columns than a pair matrix takes: the score alone still runs (identical integer paths x_sc = c against y_c = 2 c at
  p = 1: every term is (j - i)^2, the sum exact in any order); the library's refusals arrive as ValueError."""
  G = _native.PAIR_MATRIX_MAX_COLS + 1
  cols = np.arange(G, dtype=np.float64)
  x = np.tile(cols, (3, 1))
  got = _moments(eng, x, 1.0, 2.0 * cols, matrices=False)
  d = np.arange(1, G, dtype=np.float64)
  assert got['variogram_score'] == float(np.sum((G - d) * d * d)) and _same_bits(got['mean'], cols)
  xd = torch.from_numpy(x).to(eng.device)
  with pytest.raises(ValueError, match='at most 4096'):
    eng.sample_pair_moments(xd)
  with pytest.raises(ValueError, match='at most 4096'):
    eng.sample_pair_moments(xd, y=cols, pair_weights=np.ones((2, 2)), matrices=False)
  small = torch.zeros((4, 70), dtype=torch.float64, device=eng.device)
  with pytest.raises(ValueError, match=r'p = 0.75.*code -1'):
    eng.sample_pair_moments(small, p=0.75)
  with pytest.raises(ValueError, match='shape'):
    eng.sample_pair_moments(small, y=np.zeros(3))
  with pytest.raises(ValueError, match='n_samples, n_cols'):
    eng.sample_pair_moments(torch.zeros(4, dtype=torch.float64, device=eng.device))
  ptr = lambda t: C.c_void_p(t.data_ptr())
  f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=eng.device)
  mean, mat, work, score, yd = f64(70), f64(70, 70), f64(3), f64(1), f64(70)
  call = lambda **k: eng.lib.bnf_sample_pair_moments(
      eng.handle, ptr(small), k.get('S', 4), k.get('G', 70), C.c_double(k.get('p', 0.5)), k.get('y', ptr(yd)), None,
      k.get('mean', ptr(mean)), k.get('cov', ptr(mat)), None, ptr(work), C.c_size_t(k.get('nbytes', 24)), k.get('score', ptr(score)))
  assert call() == 0
  torch.cuda.synchronize()
  assert call(nbytes=16) == -1 and 'work buffer' in _native.last_error()      # 70 columns: 2 tiles a side, 3 partial sums
  assert call(y=None) == -1 and 'needs the observations' in _native.last_error()
  assert call(mean=None) == -1 and 'cov needs mean' in _native.last_error()
  assert call(S=0) == -1 and call(G=0) == -1 and call(p=3.0) == -1
  assert call(y=None, score=None, nbytes=0) == 0 and call(y=None, score=None, mean=None, cov=None) == 0
  torch.cuda.synchronize()


# ---- end to end ----------------------------------------------------------------------------------------------------------
def _frame(golden_dir):
  return pd.read_csv(os.path.join(golden_dir, 'chickenpox.8.train.csv'), index_col=0, parse_dates=['datetime'])


def _fit(kind, df):
  if kind == 'map':
    return BayesianNeuralFieldMAP(**MODEL, observation_model='NORMAL', compute_dtype='fp32').fit(
        df, seed=3, ensemble_size=4, num_epochs=5, learning_rate=0.01)
  return BayesianNeuralFieldVI(**MODEL, observation_model='NB', compute_dtype='fp32').fit(
      df, seed=1, ensemble_size=2, num_epochs=10, learning_rate=0.01, sample_size_posterior=5)


@pytest.mark.parametrize('kind', ['map', 'vi'])
def test_estimator_dependence(golden_dir, kind, monkeypatch):
  """predict_dependence / score_dependence(df, 'datetime', num_samples=300, seed=3) == the reference functions applied to
  the totals predict_samples(df, 300, 3, group_by='datetime') returns (the same matrix: only the bars apply), observed from
  a pandas groupby; with equal weights and with the weights of stacking_weights."""
  df = _frame(golden_dir)
  est = _fit(kind, df)
  S, seed, p = 300, 3, 0.5
  stacked = est.stacking_weights(df, max_iter=50)['weights']
  for tag, kw in (('equal weights', {}), ('stacked', {'weights': stacked})):
    totals, keys = est.predict_samples(df, S, seed, group_by='datetime', **kw)
    G = len(keys)
    observed = df.groupby('datetime')['chickenpox'].sum().reindex(keys).to_numpy(dtype=np.float64)
    ref = D.reference(totals, observed)
    res = est.score_dependence(df, 'datetime', p=p, num_samples=S, seed=seed, **kw)
    assert set(res) == {'keys', 'mean', 'std', 'covariance', 'correlation', 'observed', 'variogram', 'observed_variogram',
                        'variogram_score', 'n', 'n_pairs', 'mean_variogram_score'}
    assert res['keys'].equals(keys) and np.array_equal(res['observed'], observed)
    assert (res['n'], res['n_pairs']) == (G, G * (G - 1) // 2)
    D.check_moments(f'{kind} {tag}: chickenpox weeks (G={G})', res, totals, observed, p, ref)
    assert _same_bits(res['std'], np.sqrt(np.diagonal(res['covariance']))) and np.all(res['std'] > 0)
    assert np.array_equal(res['observed_variogram'], np.sqrt(np.abs(observed[:, None] - observed[None, :])))
    assert res['mean_variogram_score'] == res['variogram_score'] / res['n_pairs']
    want, bars = D.correlation(ref['cov']), D.correlation_bars(ref['cov'], D.cov_bars(totals, ref['A']))
    err = np.abs(res['correlation'] - want)
    off = ~np.eye(G, dtype=bool)
    print(f'{kind} {tag}: correlation error / bar {np.max(err / bars):.3f}; off-diagonal correlations '
          f'{want[off].min():.3f} .. {want[off].max():.3f}; score {res["variogram_score"]:.6g}')
    assert np.all(err <= bars) and np.all(np.abs(np.diagonal(res['correlation']) - 1.0) <= 4 * D.EPS)
    pred = est.predict_dependence(df, 'datetime', num_samples=S, seed=seed, **kw)
    assert set(pred) == {'keys', 'mean', 'std', 'covariance', 'correlation'} and pred['keys'].equals(keys)
    for k in ('mean', 'std', 'covariance', 'correlation'):
      assert _same_bits(pred[k], res[k]), k
    alone = est.score_dependence(df, 'datetime', p=p, matrices=False, num_samples=S, seed=seed, **kw)
    assert set(alone) == {'keys', 'mean', 'observed', 'variogram_score', 'n', 'n_pairs', 'mean_variogram_score'}
    assert _same_bits(alone['variogram_score'], res['variogram_score'])
  assert not np.array_equal(res['mean'], est.predict_dependence(df, 'datetime', num_samples=S, seed=seed)['mean'])
  # a group with a NaN target row is in no scored pair; the forecast does not change
  d = df.copy()
  d.loc[d.index[[1, 5]], 'chickenpox'] = np.nan
  res2 = est.score_dependence(d, 'datetime', p=p, num_samples=S, seed=seed, weights=stacked)
  gone = np.isnan(res2['observed'])
  assert gone.sum() == 2 and (res2['n'], res2['n_pairs']) == (G - 2, (G - 2) * (G - 3) // 2)
  assert np.array_equal(np.isnan(res2['observed_variogram']), gone[:, None] | gone[None, :])
  assert _same_bits(res2['covariance'], res['covariance']) and _same_bits(res2['variogram'], res['variogram'])
  score, e, wt = D.score_ref(ref['vario'][p], res2['observed'], p)
  bar = D.score_bar(S, ref['vario'][p], res2['observed'], p, score, e, wt)
  print(f'{kind}: two groups not scored: score {score:.6g} device error {abs(res2["variogram_score"] - score):.2e} bar {bar:.2e}')
  assert abs(res2['variogram_score'] - score) <= bar and res2['variogram_score'] != res['variogram_score']
  # an error raised by the library (an order the host check is made to let through) comes back as ValueError
  monkeypatch.setattr(inference, 'VARIOGRAM_ORDERS', inference.VARIOGRAM_ORDERS + (0.75,))
  with pytest.raises(ValueError, match=r'bnf_sample_pair_moments: p = 0.75.*code -1'):
    est.score_dependence(df, 'datetime', p=0.75, num_samples=S, seed=seed)
  monkeypatch.undo()
  # several group columns: MultiIndex keys; pair weights
  dy = df.assign(year=df['datetime'].dt.year)
  by = est.score_dependence(dy, ['location', 'year'], p=1, pair_weights=np.full((2, 2), 0.5), num_samples=S, seed=seed)
  assert isinstance(by['keys'], pd.MultiIndex) and list(by['keys'].names) == ['location', 'year'] and len(by['keys']) == 2
  assert by['covariance'].shape == (2, 2) and by['n_pairs'] == 1
  assert by['mean_variogram_score'] == by['variogram_score'] / 0.5
  assert by['variogram_score'] == 0.5 * (by['observed_variogram'][0, 1] - by['variogram'][0, 1]) ** 2
