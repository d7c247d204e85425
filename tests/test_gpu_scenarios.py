"""Scenario reduction of sample paths on the GPU (include/bnf.h bnf_sample_distances / bnf_scenario_select) against the
brute-force float64 references of tests/scenarios_ref.py, at the bars stated there (a distance cell (C + 8) eps of itself,
the objective (C + S + 16) eps of itself, eps = 2^-53; everything else exact given the selection; the reference's exact
selection wherever its gaps are at least 1e-9, every step greedy-valid in any case; counts with the 1-norm bit for bit).
LDS is poisoned before every call; every test prints what it measured (-s shows it)."""
import ctypes as C
import itertools
import os

import numpy as np
import pandas as pd
import pytest
import torch

from bayesnf_amd import BayesianNeuralFieldMAP, BayesianNeuralFieldVI, _native
from bayesnf_amd.engine import Engine
from tests import scenarios_ref as R
from tests import util
from tests.test_gpu_sampling import MODEL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
  net, _, _, _ = util.make_problem(n_rows=16, width=64, depth=1, observation_model='NORMAL')
  e = Engine(net, members=1, forward_only=True, row_capacity=128, compute_dtype='fp32')
  yield e
  e.close()


def _dev(eng, a):
  return None if a is None else torch.from_numpy(np.array(a, dtype=np.float64)).to(eng.device)   # (a copy)


def _distances(eng, x, p, scale=None, y=None):
  eng.debug_poison_lds()
  dist, ydist = eng.sample_distances(_dev(eng, x), p, _dev(eng, scale), _dev(eng, y))
  S = x.shape[0]
  assert dist.shape == (S, S) and dist.dtype == torch.float64 and (ydist is None) == (y is None)
  assert ydist is None or (ydist.shape == (S,) and ydist.dtype == torch.float64)
  return dist.cpu().numpy(), None if ydist is None else ydist.cpu().numpy()


def _select(eng, dist, k, ydist=None):
  eng.debug_poison_lds()
  out = eng.scenario_select(_dev(eng, dist), k, _dev(eng, ydist))
  S = dist.shape[0]
  want = {'chosen': ((k,), torch.int32), 'objective': ((k,), torch.float64), 'prob': ((k,), torch.float64),
          'assign': ((S,), torch.int32), 'nearest': ((S,), torch.float64)}
  if ydist is not None:
    want.update(obs_nearest=((1,), torch.int32), obs=((3,), torch.float64))
  assert {key: (tuple(v.shape), v.dtype) for key, v in out.items()} == want
  out = {key: v.cpu().numpy() for key, v in out.items()}
  if ydist is not None:
    out['obs_nearest'] = int(out['obs_nearest'][0])
  return out


def _same_bits(a, b):
  return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


def _whole_and_symmetric(dist):
  assert _same_bits(dist, dist.T)
  assert _same_bits(np.diagonal(dist), np.zeros(dist.shape[0]))      # +0.0 exactly


@pytest.mark.parametrize('kind', R.KINDS)
def test_distances_grid(eng, kind):
  """S at the edges of the 64-path tile (three tiles a side at 129, a ragged last one), C at the edges of the 32-column
  chunk, both norms, scale on and off, y (NaN in the columns 3 mod 5) on and off."""
  worst = 0.0
  for S, Cc in itertools.product(R.GRID_S, R.GRID_C):
    for p, scaled, with_y in itertools.product(R.NORMS, (False, True), (False, True)):
      x, y, scale, ref = R.distance_case(S, Cc, kind, p, scaled, with_y)
      dist, ydist = _distances(eng, x, p, scale, y)
      worst = max(worst, R.check_distances(f'{kind} S={S} C={Cc} p={p} scale={scaled} y={with_y} device', dist, ydist, x, p,
                                           scale, y, ref))
      _whole_and_symmetric(dist)
      if kind == 'counts' and p == 1 and not scaled:
        assert _same_bits(dist, ref[0]) and (ydist is None or _same_bits(ydist, ref[1]))     # integers: exact
  print(f'{kind}: worst device error / bar {worst:.3f}')


def test_distance_bits_depend_on_the_two_paths_and_the_columns_alone(eng):
  """Two calls; a call on a subset of the paths (another S, other tiles, other neighbours); a y equal to a path; a column
  y leaves out may hold anything; no participating column."""
  S, Cc = 129, 33
  for p, scaled in itertools.product(R.NORMS, (False, True)):
    x, y, scale, _ = R.distance_case(S, Cc, 'normal', p, scaled, True)
    a, ay = _distances(eng, x, p, scale, y)
    b, by = _distances(eng, x, p, scale, y)
    assert _same_bits(a, b) and _same_bits(ay, by)
    keep = np.ones(S, dtype=bool)
    keep[[0, 5, 63, 64, 100, 128]] = False
    sub, suby = _distances(eng, x[keep], p, scale, y)
    assert _same_bits(sub, a[np.ix_(keep, keep)]) and _same_bits(suby, ay[keep])
    few, _ = _distances(eng, x[[7, 70]], p, scale, y)
    assert _same_bits(few[0, 1], a[7, 70])
    yp = np.where(np.isfinite(y), x[70], np.nan)       # the observed vector IS path 70 on the participating columns
    _, on_path = _distances(eng, x, p, scale, yp)
    assert _same_bits(on_path, a[:, 70]) and on_path[70] == 0.0
    junk = np.array(x)
    junk[:, 3] = np.nan                                # y[3] is NaN: the column takes no part
    junk[5, 8] = np.inf
    c, cy = _distances(eng, junk, p, scale, y)
    assert np.isnan(y[3]) and np.isnan(y[8]) and _same_bits(c, a) and _same_bits(cy, ay)
    none, ny = _distances(eng, x, p, scale, np.full(Cc, np.nan))
    assert _same_bits(none, np.zeros((S, S))) and _same_bits(ny, np.zeros(S))
    full, _ = _distances(eng, x, p, scale)             # without y every column takes part
    assert not _same_bits(full, a)
    print(f'p={p} scale={scaled}: two calls, a subset of the paths, a y on a path, junk in a skipped column: same bits')


def test_a_path_with_one_nan_sample(eng):
  S, Cc, s = 129, 33, 70
  for p, scaled in itertools.product(R.NORMS, (False, True)):
    x, y, scale, _ = R.distance_case(S, Cc, 'normal', p, scaled, True)
    xn = np.array(x)
    xn[s, 1] = np.nan
    assert np.isfinite(y[1])
    clean, cy = _distances(eng, x, p, scale, y)
    got, gy = _distances(eng, xn, p, scale, y)
    others = np.arange(S) != s
    assert np.isnan(got[s]).all() and np.isnan(got[:, s]).all() and np.isnan(gy[s])
    assert _same_bits(got[np.ix_(others, others)], clean[np.ix_(others, others)]) and _same_bits(gy[others], cy[others])
    sel = _select(eng, got, 3, gy)
    assert (sel['chosen'] == -1).all() and (sel['assign'] == -1).all() and sel['obs_nearest'] == -1
    assert all(np.isnan(sel[key]).all() for key in ('objective', 'prob', 'nearest', 'obs'))
  print('a NaN sample: its row and column NaN, nothing else; the selection reports -1 / NaN')


@pytest.mark.parametrize('kind', ('normal', 'big', 'clusters'))
def test_selection_on_generated_cases(eng, kind):
  """The device's distances, then its selection on them, against the brute force: the reference's exact scenarios (its
  gaps are >= 1e-9 on every one of these cases: the host test asserts it, and so does this), the objective within r, every
  step greedy-valid, and assign / nearest / prob / the observed outputs exactly what follows on the device's own matrix."""
  for (S, Cc), p in itertools.product(R.SELECT_SHAPES, R.NORMS):
    x, y, ref, sel = R.selection_case(S, Cc, kind, p)
    k = len(sel['chosen'])
    dist, ydist = _distances(eng, x, p, None, y)
    R.check_distances(f'{kind} S={S} C={Cc} p={p} device', dist, ydist, x, p, None, y, ref)
    got = _select(eng, dist, k, ydist)
    R.check_selection(f'{kind} S={S} C={Cc} p={p} device', got, ref[0], k, Cc, ref[1], ref=sel, need_gaps=True,
                      own=(dist, ydist))
    again = _select(eng, dist, k, ydist)
    assert all(_same_bits(got[key], again[key]) for key in got)
    alone = _select(eng, dist, k)                      # without the observed vector: the same selection
    assert set(alone) == set(got) - {'obs_nearest', 'obs'} and all(_same_bits(alone[key], got[key]) for key in alone)
    # an observed vector that IS the third scenario: distance 0, nothing strictly nearer
    on = _select(eng, dist, k, dist[:, got['chosen'][2]])
    assert on['obs_nearest'] == 2 and on['obs'][0] == 0.0 and on['obs'][2] == 0.0
    assert on['obs'][1] == np.sum(got['nearest'] == 0) / float(S)


def test_counts_with_the_1_norm_are_exact(eng):
  for S, Cc in ((65, 2), (257, 2), (129, 3)):
    x, y, ref, sel = R.selection_case(S, Cc, 'counts', 1, k=12)
    dist, ydist = _distances(eng, x, 1, None, y)
    assert _same_bits(dist, ref[0]) and _same_bits(ydist, ref[1])
    got = _select(eng, dist, 12, ydist)
    R.check_selection(f'counts S={S} C={Cc} device', got, ref[0], 12, Cc, ref[1], exact=True, ref=sel)


@pytest.mark.parametrize('S', (1, 2, 65, 257))
def test_selection_on_integer_matrices(eng, S):
  """Hand-made integer matrices: every sum is exact, so everything equals the brute force, ties included."""
  for kind in ('random', 'duplicates', 'equal', 'zero'):
    d = R.integer_matrix(S, kind)
    yd = R.integer_matrix(S, 'random', seed=1)[0] + 1.0
    for k in sorted({1, min(2, S), S}):
      got = _select(eng, d, k, yd)
      ref = R.select_ref(d, k, yd)
      R.check_selection(f'{kind} S={S} k={k}', got, d, k, 0, yd, exact=True, ref=ref)
      if kind in ('equal', 'zero'):
        assert got['chosen'].tolist() == list(range(k))   # every candidate ties at every step: the lowest index
      if k == S:
        assert sorted(got['chosen'].tolist()) == list(range(S)) and got['objective'][-1] == 0.0


def test_at_the_cap(eng):
  """S = 4096 paths of three counts, k = 4, the 1-norm: exact against the reference; 4097 is refused; one NaN cell."""
  S, Cc, k = _native.SCENARIO_MAX_SAMPLES, 3, 4
  x, y, _ = R.scenario_case(S, Cc, 'counts')
  yf = np.array(y)
  yf[np.isnan(yf)] = 1.0
  ref = R.distances_ref(x, 1, None, yf)
  dist, ydist = _distances(eng, x, 1, None, yf)
  assert _same_bits(dist, ref[0]) and _same_bits(ydist, ref[1])
  got = _select(eng, dist, k, ydist)
  R.check_selection(f'counts S={S} C={Cc} k={k}', got, ref[0], k, Cc, ref[1], exact=True)
  bad = np.array(dist)
  bad[S - 1, 17] = np.nan
  sel = _select(eng, bad, k, ydist)
  assert (sel['chosen'] == -1).all() and (sel['assign'] == -1).all() and sel['obs_nearest'] == -1
  assert all(np.isnan(sel[key]).all() for key in ('objective', 'prob', 'nearest', 'obs'))
  over = torch.zeros((S + 1, 2), dtype=torch.float64, device=eng.device)
  with pytest.raises(ValueError, match='at most 4096'):
    eng.sample_distances(over, 2)
  ptr = lambda t: C.c_void_p(t.data_ptr())
  out = torch.zeros((8,), dtype=torch.float64, device=eng.device)
  assert eng.lib.bnf_sample_distances(eng.handle, ptr(over), S + 1, 2, None, None, 2, ptr(out), None) == -1
  assert 'at most 4096' in _native.last_error()
  assert eng.lib.bnf_scenario_select(eng.handle, ptr(out), S + 1, 2, None, ptr(out), C.c_size_t(1 << 20), ptr(out), ptr(out),
                                     ptr(out), None, None, None, None) == -1
  assert 'at most 4096' in _native.last_error()


def test_the_library_errors(eng):
  ptr = lambda t: C.c_void_p(t.data_ptr())
  f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=eng.device)
  i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=eng.device)
  x, dist, yv, yd = f64(4, 3), f64(4, 4), f64(3), f64(4)
  call = lambda **k: eng.lib.bnf_sample_distances(
      eng.handle, k.get('x', ptr(x)), k.get('S', 4), k.get('C', 3), None, k.get('y', ptr(yv)), k.get('p', 2),
      k.get('dist', ptr(dist)), k.get('ydist', ptr(yd)))
  assert call() == 0 and call(y=None, ydist=None) == 0
  assert call(y=None) == -1 and 'go together' in _native.last_error()
  assert call(ydist=None) == -1 and 'go together' in _native.last_error()
  assert call(p=0) == -1 and call(p=3) == -1 and 'p = 3' in _native.last_error()
  assert call(S=0) == -1 and call(C=0) == -1 and call(x=None) == -1 and call(dist=None) == -1
  work, chosen, obj, prob, obs, on = f64(13), i32(2), f64(2), f64(2), f64(3), i32(1)       # 20 * 4 + 16 = 96 bytes
  sel = lambda **k: eng.lib.bnf_scenario_select(
      eng.handle, k.get('dist', ptr(dist)), k.get('S', 4), k.get('k', 2), k.get('ydist', None), k.get('work', ptr(work)),
      C.c_size_t(k.get('nbytes', 96)), k.get('chosen', ptr(chosen)), k.get('obj', ptr(obj)), k.get('prob', ptr(prob)), None,
      None, k.get('on', None), k.get('obs', None))
  assert sel() == 0 and sel(ydist=ptr(yd), on=ptr(on), obs=ptr(obs)) == 0
  torch.cuda.synchronize()
  assert chosen.cpu().tolist() == [0, 1] and prob.cpu().tolist() == [1.0, 0.0] and obj.cpu().tolist() == [0.0, 0.0]
  assert sel(nbytes=95) == -1 and 'work buffer' in _native.last_error()
  assert sel(work=None) == -1 and sel(k=0) == -1 and sel(k=5) == -1 and 'k = 5' in _native.last_error()
  assert sel(S=0) == -1 and sel(dist=None) == -1 and sel(chosen=None) == -1 and sel(obj=None) == -1 and sel(prob=None) == -1
  assert sel(ydist=ptr(yd)) == -1 and 'needs obs_nearest and obs' in _native.last_error()
  with pytest.raises(ValueError, match=r'bnf_sample_distances: p = 3.*code -1'):
    eng.sample_distances(x, 3)
  with pytest.raises(ValueError, match='k=5'):
    eng.scenario_select(dist, 5)
  with pytest.raises(ValueError, match='shape'):
    eng.sample_distances(x, 2, scale=np.ones(2))
  with pytest.raises(ValueError, match='n_samples, n_samples'):
    eng.scenario_select(x, 2)
  torch.cuda.synchronize()


# ---- end to end ----------------------------------------------------------------------------------------------------------
def _frame(golden_dir):
  return pd.read_csv(os.path.join(golden_dir, 'chickenpox.8.train.csv'), index_col=0, parse_dates=['datetime'])


def _fit(kind, df):
  if kind == 'normal':
    return BayesianNeuralFieldMAP(**MODEL, observation_model='NORMAL', compute_dtype='fp32').fit(
        df, seed=3, ensemble_size=4, num_epochs=5, learning_rate=0.01)
  return BayesianNeuralFieldVI(**MODEL, observation_model='NB', compute_dtype='fp32').fit(
      df, seed=1, ensemble_size=2, num_epochs=10, learning_rate=0.01, sample_size_posterior=5)


def _as_selection(res):
  out = {'chosen': res['path'], 'objective': res['distance'], 'prob': res['probability'], 'assign': res['assignment']}
  if 'nearest' in res:
    out.update(obs_nearest=res['nearest'], obs=np.array([res['nearest_distance'], res['pit'][0], res['pit'][1]]))
  return out


@pytest.mark.parametrize('kind', ['normal', 'counts'])
def test_estimator_scenarios(eng, golden_dir, kind):
  """predict_scenarios / score_scenarios(df, 'datetime', k=5, num_samples=129, seed=3) against the reference run on the
  totals predict_samples(df, 129, 3, group_by='datetime') returns: the scenarios are rows of that matrix bit for bit; the
  selection under the conditions of tests/scenarios_ref.py (counts with the 1-norm: bit for bit); with equal weights and
  with all weight on one member; one NaN target leaves its group out of every distance."""
  df = _frame(golden_dir)
  est = _fit(kind, df)
  S, seed, k = 129, 3, 5
  shape = np.shape(est.score(df)['member_log_prob'])
  one = np.zeros(shape)
  one.reshape(-1)[1] = 1.0
  d = df.copy()
  d.loc[d.index[[1]], 'chickenpox'] = np.nan
  for (tag, kw), norm, scaled in itertools.product((('equal weights', {}), ('one member', {'weights': one})), R.NORMS,
                                                   (False, True)):
    totals, keys = est.predict_samples(df, S, seed, group_by='datetime', **kw)
    G = len(keys)
    scale = np.maximum(totals.std(axis=0), 1.0) if scaled else None
    res = est.predict_scenarios(df, 'datetime', k=k, norm=norm, scale=scale, num_samples=S, seed=seed, **kw)
    assert set(res) == {'keys', 'scenarios', 'probability', 'path', 'distance', 'assignment'} and res['keys'].equals(keys)
    assert res['scenarios'].shape == (k, G) and res['scenarios'].dtype == np.float64
    assert _same_bits(res['scenarios'], totals[res['path']])
    assert np.array_equal(np.bincount(res['assignment'], minlength=k) / S, res['probability'])
    assert res['assignment'].shape == (S,) and np.all(np.diff(res['distance']) <= 0)
    exact = kind == 'counts' and norm == 1 and not scaled
    label = f'{kind} {tag} norm={norm} scale={scaled} (G={G})'
    ref = R.distances_ref(totals, norm, scale)
    dist, _ = _distances(eng, totals, norm, scale)
    R.check_distances(label, dist, None, totals, norm, scale, None, ref)
    R.check_selection(label, _as_selection(res), ref[0], k, G, exact=exact, own=(dist, None))
    # scored: the observed totals from a pandas groupby, one group left out by its NaN target
    observed = d.groupby('datetime')['chickenpox'].sum(min_count=1).reindex(keys).to_numpy(dtype=np.float64)
    gone = d.groupby('datetime')['chickenpox'].apply(lambda v: v.isna().any()).reindex(keys).to_numpy()
    observed[gone] = np.nan
    assert gone.sum() == 1
    sc = est.score_scenarios(d, 'datetime', k=k, norm=norm, scale=scale, num_samples=S, seed=seed, **kw)
    assert set(sc) == set(res) | {'observed', 'n', 'nearest', 'nearest_distance', 'pit'}
    assert np.array_equal(sc['observed'], observed, equal_nan=True) and sc['n'] == G - 1 and sc['pit'].shape == (2,)
    assert _same_bits(sc['scenarios'], totals[sc['path']])
    ref = R.distances_ref(totals, norm, scale, observed)
    dist, ydist = _distances(eng, totals, norm, scale, observed)
    R.check_distances(label + ' scored', dist, ydist, totals, norm, scale, observed, ref)
    R.check_selection(label + ' scored', _as_selection(sc), ref[0], k, G, ref[1], exact=exact, own=(dist, ydist))
    left_out = R.distances_ref(np.delete(totals, np.flatnonzero(gone), axis=1), norm,
                               None if scale is None else scale[~gone])[0]
    assert np.array_equal(left_out, ref[0])            # the group is in no distance
  plain = est.predict_scenarios(df, 'datetime', k=k, num_samples=S, seed=seed)
  assert not np.array_equal(plain['scenarios'], res['scenarios'])             # the weights are taken
  rows = est.predict_samples(df, S, seed)[plain['path']]                      # the scenarios row by row
  assert rows.shape == (k, len(df))
  by_week = pd.DataFrame(rows.T.astype(np.float64), index=df['datetime'].to_numpy()).groupby(level=0).sum().reindex(plain['keys'])
  assert np.allclose(by_week.to_numpy().T, plain['scenarios'], rtol=1e-6, atol=1e-3)
