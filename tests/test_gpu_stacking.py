"""Stacking of the ensemble members on the GPU (include/bnf.h bnf_member_log_density, bnf_stacking_weights,
bnf_predictive_samples_weighted, bnf_predictive_group_sums_weighted) against the float64 restatement of
tests/stacking_ref.py.

Bars, none tuned on the code under test: the matrix L at max(1e-5, 4 x the float32 restatement's own error)
(tests/scoring_ref.py `bar`); f64 sums of the same f32 terms in another order 1e-12; weights after k updates 1e-12 relative
(f64 exp / log differ from numpy's by ulps, the sums have <= 1025 terms); the closed form of the block case 1e-14.  The
convergence test needs no reference optimum: gap = max_m g_m - 1, recomputed on the host from the downloaded L, bounds the
distance of the objective from its optimum.

Every test prints the errors it measured next to its bar (-s shows them)."""
import ctypes as C
import os

import numpy as np
import pandas as pd
import pytest
import torch

from bayesnf_amd import BayesianNeuralFieldMAP, BayesianNeuralFieldVI, _native, inference
from bayesnf_amd.engine import Engine
from tests import scoring_ref as S
from tests import stacking_ref as K
from tests import util
from tests.test_gpu_sampling import EPS, MODEL, TCS, _mixed_inputs
from tests.test_gpu_sampling import S as N_PATHS

pytestmark = pytest.mark.gpu


def _engine(obs='NORMAL'):
  net, _, _, _ = util.make_problem(n_rows=16, width=64, depth=1, observation_model=obs)
  eng = Engine(net, members=1, forward_only=True, row_capacity=128, compute_dtype='fp32')
  eng.debug_poison_lds()
  return eng


def _dev(eng, a):
  return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(eng.device)


def _stack(eng, L, **kw):
  """L: numpy (rounded to float32 on the way) or a device tensor -> the engine's dict with numpy arrays."""
  res = eng.stacking_weights(L if isinstance(L, torch.Tensor) else _dev(eng, L), **kw)
  return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in res.items()}


def _rel(v, ref):
  v, ref = np.asarray(v, dtype=np.float64), np.asarray(ref, dtype=np.float64)
  return float(np.max(np.abs(v - ref) / np.abs(ref)))


def _uniform(M):
  return np.full(M, 1.0 / M)


# ------------------------------------------------------------------------------------------------------ (a) the matrix L
def _check_L(tag, eng, obs, loc, aux, y, lp_f32):
  want = K.logdens_ref(obs, loc, aux, y)
  L_d = eng.member_log_density(_dev(eng, loc), _dev(eng, aux), _dev(eng, y))
  L = L_d.cpu().numpy()
  M, R = loc.shape
  assert L.shape == (M, R) and L.dtype == np.float32
  rest = S.rel1(lp_f32, want)
  err, bar = S.rel1(L, want), S.bar(rest)
  sc = {k: v.cpu().numpy() for k, v in eng.predictive_scores(_dev(eng, loc), _dev(eng, aux), _dev(eng, y), crps=False,
                                                             pit=False).items()}
  fin = np.isfinite(y)
  sums = L.astype(np.float64)[:, fin].sum(axis=1)
  e_sum = S.rel1(sums, sc['member_ll'])
  lpd = _stack(eng, L_d, max_iter=0)['lpd']
  e_lpd = S.rel1(lpd, sc['lpd'])
  print(f'{tag} L {err:.2e} (f32 {rest:.1e}, bar {bar:.0e}); row sums vs member_ll {e_sum:.2e} (bar 1e-12); '
        f'lpd at uniform weights vs predictive_scores {e_lpd:.2e} (bar {S.GATE:.0e})')
  assert err <= bar and e_sum <= 1e-12 and e_lpd <= S.GATE, (tag, err, e_sum, e_lpd)


@pytest.mark.parametrize('M', [1, 2, 7, 65])
def test_log_density_matrix_normal(M):
  eng = _engine('NORMAL')
  for R in (1, 63, 64, 65, K.ROW_TILE + 1):
    loc, sigma, y = S.normal_case(M, R)
    _check_L(f'NORMAL M={M} R={R}:', eng, 'NORMAL', loc, S.normal_aux(sigma), y, S.normal_f32(loc, sigma, y)['lp'])
  eng.close()


@pytest.mark.parametrize('obs', ['NB', 'ZINB'])
def test_log_density_matrix_counts(obs):
  eng = _engine(obs)
  for tc in TCS:
    loc, aux, y, ref, f32 = S.count_grid_case(obs, tc, 7)
    _check_L(f'{obs} M=7 tc={tc:g}:', eng, obs, loc, aux, y, f32['lp'])
  eng.close()


# -------------------------------------------------------------------------------------------------- (b) the block case
def test_block_case_reaches_its_closed_form_in_one_update():
  eng = _engine()
  sizes = np.asarray(K.BLOCK_SIZES, dtype=np.float64)
  L = K.block_case(K.BLOCK_SIZES, dead=1)
  one = _stack(eng, L, max_iter=1, tol=0.0)
  want = sizes / sizes.sum()
  err = _rel(one['weights'][:5], want)
  print(f'block case: weights after one update {err:.2e} (bar 1e-14), sixth weight {one["weights"][5]!r}, gap {one["gap"]:.2e}')
  assert err <= 1e-14 and one['weights'][5] == 0.0 and one['iterations'] == 1 and one['dropped'] == 0
  assert one['objective_start'] == pytest.approx(np.log(1.0 / 6.0), rel=1e-14)
  two = _stack(eng, L, w_init=one['weights'], max_iter=5, tol=1e-12)
  print(f'block case: a second call from those weights: gap {two["gap"]:.2e} (bar 1e-14), {two["iterations"]} updates')
  assert two['gap'] <= 1e-14 and two['iterations'] == 0 and two['dropped'] == 0 and two['converged']
  assert np.array_equal(two['weights'], one['weights'])
  hot = _stack(eng, L, w_init=np.eye(6)[0], max_iter=0)
  assert hot['dropped'] == 1025 - 3 and hot['objective'] == 0.0
  assert np.array_equal(np.isneginf(hot['lpd']), np.arange(1025) >= 3) and np.all(hot['lpd'][:3] == 0.0)
  dead = _stack(eng, L, w_init=np.eye(6)[5], max_iter=3)      # no scored row
  assert np.isnan(dead['objective']) and np.isnan(dead['gap']) and dead['iterations'] == 0 and dead['dropped'] == 1025
  assert np.array_equal(dead['weights'], np.eye(6)[5]) and not dead['converged']
  eng.close()


# -------------------------------------------------------------------------------------------------- (c) the update rule
@pytest.mark.parametrize('k', [1, 2, 17])
def test_k_updates_equal_the_host_em(k):
  eng = _engine()
  L = K.normal_L(*K.normal_case(7, 1025))
  got = _stack(eng, L, max_iter=k, tol=0.0)
  want = K.em(L, _uniform(7), k, 0.0)
  err = _rel(got['weights'], want['weights'])
  print(f'{k} updates: weights {err:.2e} (bar 1e-12); objective {got["objective"]:.9f} host {want["objective"]:.9f}; '
        f'gap {got["gap"]:.3e} host {want["gap"]:.3e}')
  assert got['iterations'] == k == want['iterations'] and err <= 1e-12
  assert abs(got['objective'] - want['objective']) <= 1e-12 * max(1.0, abs(want['objective']))
  assert abs(got['objective_start'] - want['objective_start']) <= 1e-12 * max(1.0, abs(want['objective_start']))
  assert abs(got['gap'] - want['gap']) <= 1e-9
  eng.close()


# ------------------------------------------------------------------------------ (d) convergence and its own certificate
@pytest.mark.parametrize('M,R', K.CONVERGENCE_SHAPES)
def test_convergence_and_the_certificate(M, R):
  eng = _engine('NORMAL')
  loc, sigma, y = K.normal_case(M, R)
  L_d = eng.member_log_density(_dev(eng, loc), _dev(eng, S.normal_aux(sigma)), _dev(eng, y))
  res = _stack(eng, L_d, tol=1e-5, max_iter=5000)
  eng.close()
  L = L_d.cpu().numpy().astype(np.float64)
  w = res['weights']
  f, g = K.objective(L, w), K.gap(L, w)
  e_f, e_g = abs(res['objective'] - f), abs(res['gap'] - g)
  print(f'M={M} R={R}: {res["iterations"]} updates, gap {res["gap"]:.3e} (tol 1e-5); objective {res["objective_start"]:.6f} -> '
        f'{res["objective"]:.6f}; host recomputation: objective {e_f:.2e} (bar {1e-12 * max(1.0, abs(f)):.0e}), gap {e_g:.2e} '
        f'(bar 1e-9); sum w - 1 = {w.sum() - 1.0:.1e}; {int((w > 1e-6).sum())} members above 1e-6')
  assert res['converged'] and res['gap'] <= 1e-5 and res['iterations'] <= 5000
  assert e_f <= 1e-12 * max(1.0, abs(f)) and e_g <= 1e-9
  assert np.all(w >= 0) and abs(w.sum() - 1.0) <= 1e-12
  assert res['objective'] > res['objective_start']
  assert abs(res['objective_start'] - K.objective(L, _uniform(M))) <= 1e-12 * max(1.0, abs(f))
  assert res['dropped'] == 0


# ------------------------------------------------------------------------------------------------------ (e) max_iter = 0
def test_pure_evaluation_of_given_weights():
  eng = _engine()
  M, R = 7, 1025
  L = K.normal_L(*K.normal_case(M, R))
  w0 = np.random.default_rng(3).dirichlet(np.ones(M))
  res = _stack(eng, L, w_init=w0, max_iter=0)
  assert np.array_equal(res['weights'].view(np.int64), w0.view(np.int64)) and res['iterations'] == 0
  e = S.rel1(res['lpd'], K.lse(L, w0))
  print(f'max_iter = 0: lpd vs host logsumexp {e:.2e} (bar {S.GATE:.0e})')
  assert e <= S.GATE
  assert abs(res['objective'] - K.objective(L, w0)) <= 1e-12 * max(1.0, abs(res['objective']))
  assert res['objective'] == res['objective_start'] and abs(res['gap'] - K.gap(L, w0)) <= 1e-9
  for k in range(M):
    hot = _stack(eng, L, w_init=np.eye(M)[k], max_iter=0)
    assert np.array_equal(hot['lpd'], L[k].astype(np.float32)), k
  eng.close()


# ---------------------------------------------------------------------------------------------------------- (f) NaN rows
def test_nan_rows_are_left_out():
  eng = _engine('NORMAL')
  loc, sigma, y = K.normal_case(7, 1025)
  y = y.copy()
  gone = [0, 17, 64, 1024]
  y[gone] = np.nan
  keep = np.isfinite(y)
  aux = S.normal_aux(sigma)
  L_d = eng.member_log_density(_dev(eng, loc), _dev(eng, aux), _dev(eng, y))
  L = L_d.cpu().numpy()
  assert np.array_equal(np.isnan(L), np.broadcast_to(~keep, L.shape))
  res = _stack(eng, L_d, max_iter=20, tol=0.0)
  assert np.array_equal(np.isnan(res['lpd']), ~keep) and res['dropped'] == 0
  alone = _stack(eng, L[:, keep], max_iter=20, tol=0.0)
  err = _rel(res['weights'], alone['weights'])
  print(f'NaN rows: weights against the kept rows alone {err:.2e} (bar 1e-12)')
  assert err <= 1e-12 and res['iterations'] == alone['iterations'] == 20
  assert abs(res['objective'] - alone['objective']) <= 1e-12 * max(1.0, abs(alone['objective']))
  eng.close()


# ------------------------------------------------------------------------------------------- (g) determinism, arguments
def test_two_calls_give_the_same_bits_and_bad_arguments_are_refused():
  eng = _engine()
  M, R = 64, 2 * K.ROW_TILE + 1
  L_d = _dev(eng, K.normal_L(*K.normal_case(M, R)))
  a = _stack(eng, L_d, max_iter=40, tol=0.0)
  eng.debug_poison_lds()
  b = _stack(eng, L_d, max_iter=40, tol=0.0)
  assert np.array_equal(a['weights'].view(np.int64), b['weights'].view(np.int64))
  assert np.array_equal(a['lpd'].view(np.int32), b['lpd'].view(np.int32))
  for k in ('objective', 'objective_start', 'gap', 'iterations', 'dropped'):
    assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), k
  n_work = _native.stacking_work_doubles(M, R)
  assert n_work == 8 + (M + 3) * 3
  work = torch.empty(n_work, dtype=torch.float64, device=eng.device)
  w = torch.empty(M, dtype=torch.float64, device=eng.device)
  info = torch.empty(5, dtype=torch.float64, device=eng.device)
  p = lambda t: C.c_void_p(t.data_ptr())
  call = lambda m, r, iters, tol, nbytes: eng.lib.bnf_stacking_weights(
      eng.handle, p(L_d), m, r, None, iters, C.c_double(tol), p(work), C.c_size_t(nbytes), p(w), None, p(info))
  assert call(M, R, 40, 0.0, 8 * n_work) == 0
  torch.cuda.synchronize()
  assert np.array_equal(w.cpu().numpy().view(np.int64), a['weights'].view(np.int64))
  for args in ((M, R, 40, 0.0, 8 * n_work - 1), (0, R, 40, 0.0, 1 << 20), (M, 0, 40, 0.0, 1 << 20), (M, R, -1, 0.0, 8 * n_work),
               (M, R, 40, float('nan'), 8 * n_work), (M, R, 40, -1e-9, 8 * n_work)):
    assert call(*args) == -1, args
  eng.close()


# --------------------------------------------------------------------------------------------------- (h) weighted sampling
def _cum(w):
  cum = np.cumsum(np.asarray(w, dtype=np.float64))
  cum[-1] = 1.0
  return cum


@pytest.mark.parametrize('obs', ['NORMAL', 'NB', 'ZINB'])
def test_one_hot_weights_give_the_bits_of_that_member_alone(obs):
  eng = _engine(obs)
  M, R, n = 4, 3001, 20
  loc, aux = _mixed_inputs(obs, M, R, 11)
  loc_d, aux_d = _dev(eng, loc), _dev(eng, aux)
  plain = eng.predictive_samples(loc_d, aux_d, n, seed=5).cpu().numpy()
  for k in range(M):
    got = eng.predictive_samples(loc_d, aux_d, n, seed=5, cum_weights=_cum(np.eye(M)[k])).cpu().numpy()
    alone = eng.predictive_samples(loc_d[k:k + 1], aux_d[k:k + 1], n, seed=5).cpu().numpy()
    assert np.array_equal(got.view(np.int32), alone.view(np.int32)), k
  # no weights: the new entry point with NULL gives the bits of the existing call
  out = torch.empty((n, R), dtype=torch.float32, device=eng.device)
  p = lambda t: C.c_void_p(t.data_ptr())
  assert eng.lib.bnf_predictive_samples_weighted(eng.handle, p(loc_d), p(aux_d), M, R, n, C.c_uint64(5), 0, 0, None,
                                                 p(out)) == 0
  torch.cuda.synchronize()
  assert np.array_equal(out.cpu().numpy().view(np.int32), plain.view(np.int32))
  assert np.array_equal(eng.predictive_samples(loc_d, aux_d, n, seed=5, cum_weights=None).cpu().numpy(), plain)
  # chunks of rows and of paths under weights
  cum = _cum([0.1, 0.2, 0.3, 0.4])
  full = eng.predictive_samples(loc_d, aux_d, n, seed=5, cum_weights=cum).cpu().numpy()
  assert not np.array_equal(full, plain)
  for a, b in ((0, 1), (1, 1025), (1023, 2049), (2990, 3001)):
    part = eng.predictive_samples(loc_d[:, a:b], aux_d, n, seed=5, row0=a, cum_weights=cum).cpu().numpy()
    assert np.array_equal(part, full[:, a:b]), (a, b)
  for s0, k in ((0, 1), (7, 9), (19, 1)):
    part = eng.predictive_samples(loc_d, aux_d, k, seed=5, sample0=s0, cum_weights=cum).cpu().numpy()
    assert np.array_equal(part, full[s0:s0 + k]), (s0, k)
  eng.close()


def test_component_law_under_weights():
  """One member per path, drawn with the given probabilities (DKW on the member index), zero weights never."""
  eng = _engine('NORMAL')
  M, R = 8, 64
  w = np.asarray([0.5, 0.25, 0.125, 0.125, 0, 0, 0, 0])
  loc = np.repeat(100.0 * np.arange(M)[:, None], R, axis=1)
  aux = np.stack([np.full(M, 0.01), np.ones(M), np.zeros(M)], axis=1)
  x = eng.predictive_samples(_dev(eng, loc), _dev(eng, aux), N_PATHS, seed=7, cum_weights=_cum(w)).cpu().numpy().astype(np.float64)
  eng.close()
  member = np.rint(x / 100.0).astype(int)
  assert np.abs(x - 100.0 * member).max() < 0.1
  assert np.all(member == member[:, :1]), 'a path mixed members across its rows'
  freq = np.bincount(member[:, 0], minlength=M) / N_PATHS
  d = np.abs(np.cumsum(freq) - np.cumsum(w)).max()
  print(f'member frequencies {freq}; sup |F_n - F| = {d:.4f} (eps {EPS:.4f})')
  assert d <= EPS and np.all(freq[4:] == 0.0) and member.min() >= 0 and member.max() <= 3


@pytest.mark.parametrize('obs', ['NORMAL', 'NB', 'ZINB'])
def test_weighted_group_sums_equal_the_host_sums_of_the_weighted_draws(obs):
  eng = _engine(obs)
  M, R, n = 4, 2500, 24
  loc, aux = _mixed_inputs(obs, M, R, 21)
  sizes = [1024, 1, 0, 999, 476]                              # a segment edge on the 1024-position tile edge
  codes = np.random.default_rng(5).permutation(np.repeat(np.arange(len(sizes)), sizes))
  G = len(sizes)
  off, rows = inference.csr_from_codes(codes, G)
  cum = _cum([0.4, 0.1, 0.2, 0.3])
  loc_d, aux_d = _dev(eng, loc), _dev(eng, aux)
  x = eng.predictive_samples(loc_d, aux_d, n, seed=42, cum_weights=cum).cpu().numpy().astype(np.float64)
  want = np.stack([np.bincount(codes, weights=x[s], minlength=G) for s in range(n)])
  absum = np.stack([np.bincount(codes, weights=np.abs(x[s]), minlength=G) for s in range(n)])
  got = eng.predictive_group_sums(loc_d, aux_d, off, rows, n, seed=42, cum_weights=cum).cpu().numpy()
  plain = eng.predictive_group_sums(loc_d, aux_d, off, rows, n, seed=42).cpu().numpy()
  work = torch.empty(2 * 3 * n, dtype=torch.float64, device=eng.device)
  out = torch.empty((n, G), dtype=torch.float64, device=eng.device)
  p = lambda t: C.c_void_p(t.data_ptr())
  off_d, rows_d = torch.from_numpy(off).to(eng.device), torch.from_numpy(rows).to(eng.device)
  assert eng.lib.bnf_predictive_group_sums_weighted(eng.handle, p(loc_d), p(aux_d), M, R, p(off_d), p(rows_d), G, n,
                                                    C.c_uint64(42), 0, 0, None, p(work), C.c_size_t(work.numel() * 8),
                                                    p(out)) == 0
  torch.cuda.synchronize()
  eng.close()
  assert np.array_equal(out.cpu().numpy().view(np.int64), plain.view(np.int64))      # NULL: the existing call
  err = np.abs(got - want)
  print(f'{obs}: weighted group sums, max |device - host| = {err.max():.3e}, max sum|x| = {absum.max():.3e}')
  assert got.shape == (n, G) and np.all(got[:, 2] == 0.0) and not np.array_equal(got, plain)
  if obs == 'NORMAL':
    assert np.all(err <= 1e-12 * absum), float((err - 1e-12 * absum).max())
  else:
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------------- (i) estimators
def _frame(golden_dir):
  return pd.read_csv(os.path.join(golden_dir, 'chickenpox.8.train.csv'), index_col=0, parse_dates=['datetime'])


def test_estimator_stacking_map_counts(golden_dir):
  df = _frame(golden_dir)
  est = BayesianNeuralFieldMAP(**MODEL, observation_model='NB', compute_dtype='fp32')
  with pytest.raises(ValueError, match='before fit'):
    est.stacking_weights(df)
  est.fit(df, seed=3, ensemble_size=4, num_epochs=20, learning_rate=0.01)
  R = len(df)
  res = est.stacking_weights(df)
  assert set(res) == {'weights', 'log_density', 'mean_log_density', 'equal_weight_mean_log_density', 'gap', 'iterations',
                      'converged', 'n', 'dropped'}
  sc = est.score(df)
  w = res['weights']
  assert w.shape == sc['member_log_prob'].shape == (1, 4) and w.dtype == np.float64
  assert abs(w.sum() - 1.0) <= 1e-12 and np.all(w >= 0)
  assert res['log_density'].shape == (R,) and res['n'] == R and res['dropped'] == 0
  print(f'MAP NB: weights {w.ravel()}, mean log density {res["equal_weight_mean_log_density"]:.5f} -> '
        f'{res["mean_log_density"]:.5f} in {res["iterations"]} updates, gap {res["gap"]:.2e}')
  assert res['mean_log_density'] >= res['equal_weight_mean_log_density']
  assert res['converged'] == (res['gap'] <= 1e-5)
  assert abs(res['equal_weight_mean_log_density'] - sc['mean_log_density']) <= S.GATE * max(1.0, abs(sc['mean_log_density']))
  assert abs(res['mean_log_density'] - np.mean(res['log_density'], dtype=np.float64)) <= S.GATE * max(1.0, abs(res['mean_log_density']))
  uni = est.weighted_log_density(df, np.full((1, 4), 0.25))
  assert set(uni) == {'log_density', 'mean_log_density', 'n'} and uni['n'] == R
  e = S.rel1(uni['log_density'], sc['log_density'])
  print(f'MAP NB: weighted_log_density at equal weights vs score {e:.2e} (bar {S.GATE:.0e})')
  assert e <= S.GATE
  back = est.weighted_log_density(df, w)
  assert np.array_equal(back['log_density'], res['log_density']) and back['mean_log_density'] == res['mean_log_density']
  # the sample-path family takes the weights
  hot = np.zeros((1, 4))
  hot[0, 2] = 1.0
  mean_w, q_w, keys = est.predict_totals(df, 'datetime', num_samples=256, seed=4, weights=hot)
  mean_u, _, _ = est.predict_totals(df, 'datetime', num_samples=256, seed=4)
  mean_w2, q_w2, _ = est.predict_totals(df, 'datetime', num_samples=256, seed=4, weights=hot)
  assert not np.array_equal(mean_w, mean_u)
  assert np.array_equal(mean_w, mean_w2) and np.array_equal(q_w[0], q_w2[0])
  tot, _ = est.predict_samples(df, 256, seed=4, group_by='datetime', weights=hot)
  np.testing.assert_allclose(tot.mean(axis=0), mean_w, rtol=1e-12)
  st = est.score_totals(df, 'datetime', num_samples=256, seed=4, weights=w)
  assert set(st) == {'keys', 'observed', 'mean', 'quantiles', 'crps', 'pit', 'n', 'mean_crps', 'energy_score'}
  with pytest.raises(ValueError, match='shape'):
    est.predict_samples(df, 8, weights=np.full(4, 0.25))
  d = df.copy()
  d.loc[d.index[2], 'chickenpox'] = 2.5
  with pytest.raises(ValueError, match='non-negative integer'):
    est.stacking_weights(d)
  d.loc[d.index[2], 'chickenpox'] = np.nan
  res2 = est.stacking_weights(d)
  assert res2['n'] == R - 1 and np.isnan(res2['log_density'][2]) and np.isnan(res2['log_density']).sum() == 1


def test_estimator_stacking_vi_normal(golden_dir):
  """The posterior draws count as components: weights (1, 5, 2), flattened in the order of member_log_prob."""
  df = _frame(golden_dir)
  est = BayesianNeuralFieldVI(**MODEL, observation_model='NORMAL', compute_dtype='fp32').fit(
      df, seed=1, ensemble_size=2, num_epochs=10, learning_rate=0.01, sample_size_posterior=5)
  res = est.stacking_weights(df, max_iter=2000)
  sc = est.score(df)
  w = res['weights']
  assert w.shape == sc['member_log_prob'].shape == (1, 5, 2) and abs(w.sum() - 1.0) <= 1e-12
  assert res['mean_log_density'] >= res['equal_weight_mean_log_density']
  assert abs(res['equal_weight_mean_log_density'] - sc['mean_log_density']) <= S.GATE * max(1.0, abs(sc['mean_log_density']))
  # one-hot on the component with the best member_log_prob: its mean log density is that member's
  best = np.unravel_index(np.argmax(sc['member_log_prob']), w.shape)
  hot = np.zeros_like(w)
  hot[best] = 1.0
  one = est.weighted_log_density(df, hot)
  want = sc['member_log_prob'][best] / len(df)
  print(f'VI NORMAL: weights {w.ravel()}; one-hot mean log density {one["mean_log_density"]:.6f} vs member_log_prob / n {want:.6f}')
  assert abs(one['mean_log_density'] - want) <= S.GATE * max(1.0, abs(want))
  x = est.predict_samples(df, 16, seed=2, weights=hot)
  assert x.shape == (16, len(df)) and x.dtype == np.float32
