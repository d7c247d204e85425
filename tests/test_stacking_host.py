"""CPU-only checks of the stacking of ensemble members (include/bnf.h bnf_member_log_density / bnf_stacking_weights /
bnf_predictive_*_weighted): the float64 restatement of tests/stacking_ref.py against closed forms and an independent
optimiser; the cap on the iterations the GPU convergence test relies on; the entry points' declaration and export; their
refusal without a device; the weight checks of the estimators, which fire before any engine is created; weights=None
reaching the code path that was there before."""
import ctypes as C
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

from bayesnf_amd import BayesianNeuralFieldMAP, BayesianNeuralFieldVI, _native, inference
from tests import stacking_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = (('bnf_member_log_density', 7), ('bnf_stacking_weights', 12), ('bnf_predictive_samples_weighted', 11),
       ('bnf_predictive_group_sums_weighted', 16))


def test_block_case_closed_form_after_one_step():
  sizes = np.asarray(K.BLOCK_SIZES, dtype=np.float64)
  L = K.block_case(K.BLOCK_SIZES, dead=1)
  uniform = np.full(6, 1.0 / 6.0)
  res = K.em(L, uniform, 1, 0.0)
  want = np.append(sizes / sizes.sum(), 0.0)
  err = np.abs(res['weights'][:5] - want[:5]) / want[:5]
  print(f'one step from uniform: max rel err {err.max():.2e}, gap {res["gap"]:.2e}')
  assert res['iterations'] == 1 and err.max() <= 1e-14 and res['weights'][5] == 0.0 and res['dropped'] == 0
  assert abs(res['gap']) <= 1e-14
  assert res['objective_start'] == pytest.approx(np.log(1.0 / 6.0), rel=1e-15)
  assert res['objective'] == pytest.approx(float((sizes * np.log(sizes / sizes.sum())).sum() / sizes.sum()), rel=1e-14)
  again = K.em(L, res['weights'], 5, 1e-12)
  assert again['iterations'] == 0 and again['gap'] <= 1e-14
  one_hot = np.eye(6)[0]
  ev = K.em(L, one_hot, 0, 0.0)
  assert ev['dropped'] == 1025 - 3 and ev['objective'] == 0.0 and np.array_equal(ev['weights'], one_hot)
  # no scored row at all: NaN objective and gap, the weights untouched
  none = K.em(L, np.eye(6)[5], 3, 1e-5)
  assert np.isnan(none['objective']) and np.isnan(none['gap']) and none['iterations'] == 0 and none['dropped'] == 1025


@pytest.mark.parametrize('M,R', [(3, 65), (7, 1025)])
def test_em_is_monotone_in_the_objective(M, R):
  L = K.normal_L(*K.normal_case(M, R))
  res = K.em(L, np.full(M, 1.0 / M), 60, 0.0, trajectory=True)
  f = np.asarray([K.objective(L, w) for w in res['trajectory']])
  print(f'M={M} R={R}: objective {f[0]:.6f} -> {f[-1]:.6f} over {len(f) - 1} updates')
  assert len(f) == 61 and np.all(np.diff(f) >= -1e-14) and f[-1] > f[0]
  for w in res['trajectory']:
    assert np.all(w >= 0) and abs(w.sum() - 1.0) <= 1e-14


def test_the_gap_bounds_the_distance_to_the_optimum():
  """f(w_opt) - f(w) <= gap(w) along an EM trajectory, w_opt from SLSQP on the simplex (M = 3)."""
  from scipy import optimize
  M, R = 3, 257
  L = K.normal_L(*K.normal_case(M, R))
  cons = [{'type': 'eq', 'fun': lambda w: w.sum() - 1.0}]
  best = optimize.minimize(lambda w: -K.objective(L, np.maximum(w, 1e-300)), np.full(M, 1.0 / M), method='SLSQP',
                           jac=lambda w: -K.grad(L, np.maximum(w, 1e-300)), bounds=[(0.0, 1.0)] * M, constraints=cons,
                           options=dict(ftol=1e-15, maxiter=500))
  assert best.success, best.message
  f_opt = -best.fun
  res = K.em(L, np.full(M, 1.0 / M), 200, 0.0, trajectory=True)
  worst = -np.inf
  for w in res['trajectory']:
    short, g = f_opt - K.objective(L, w), K.gap(L, w)
    worst = max(worst, short - g)
    assert short <= g + 1e-12, (short, g)
  print(f'f_opt {f_opt:.9f}, EM after 200 updates {res["objective"]:.9f} (gap {res["gap"]:.2e}); max (shortfall - gap) {worst:.2e}')
  assert res['objective'] <= f_opt + 1e-9


@pytest.mark.parametrize('M,R', K.CONVERGENCE_SHAPES)
def test_em_reaches_the_tolerance_well_inside_the_gpu_tests_cap(M, R):
  """The GPU convergence test allows 5,000 updates; the float64 restatement needs at most 2,000 from uniform."""
  L = K.normal_L(*K.normal_case(M, R))
  res = K.em(L, np.full(M, 1.0 / M), 2000, 1e-5)
  print(f'M={M} R={R}: {res["iterations"]} updates to gap {res["gap"]:.2e}; objective {res["objective_start"]:.5f} -> '
        f'{res["objective"]:.5f}; {int((res["weights"] > 1e-6).sum())} members above 1e-6')
  assert res['gap'] <= 1e-5 and res['iterations'] <= 2000
  assert res['objective'] > res['objective_start']


def test_nan_rows_and_logdens_ref():
  loc, sigma, y = K.normal_case(4, 70)
  y = y.copy()
  y[[0, 17]] = np.nan
  L = K.logdens_ref('NORMAL', loc, K.S.normal_aux(sigma), y)
  assert np.array_equal(np.isnan(L), np.broadcast_to(np.isnan(y), L.shape))
  keep = np.isfinite(y)
  a, b = K.em(L, np.full(4, 0.25), 10, 0.0), K.em(L[:, keep], np.full(4, 0.25), 10, 0.0)
  assert np.array_equal(a['weights'], b['weights']) and a['objective'] == b['objective'] and a['dropped'] == 0
  assert np.array_equal(np.isnan(K.lse(L, a['weights'])), ~keep)


def test_entry_points_declared_listed_and_exported():
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'bnf.h')).read(), flags=re.S)
  lib = _native.load()
  for name, n_args in NEW:
    assert re.search(r'\bint\s+' + name + r'\s*\(', src), f'{name} is not declared in include/bnf.h'
    assert name in _native.EXPORTS
    fn = getattr(lib, name)
    assert fn.argtypes is not None and len(fn.argtypes) == n_args
  assert _native.ABI_VERSION == 6 and lib.bnf_abi_version() == 6          # purely additive
  for macro, val in (('BNF_STACK_ROW_TILE', _native.STACK_ROW_TILE), ('BNF_STACK_STATE_DOUBLES', _native.STACK_STATE_DOUBLES)):
    assert int(re.search(r'#define\s+' + macro + r'\s+(\d+)', src).group(1)) == val
  assert _native.STACK_ROW_TILE == K.ROW_TILE
  assert _native.stacking_work_doubles(7, 1025) == 8 + 10 * 2
  from bayesnf_amd.engine import Engine
  for name in ('member_log_density', 'stacking_weights'):
    assert callable(getattr(Engine, name, None))


@pytest.mark.skipif(torch.cuda.is_available(), reason='checks the no-GPU failure mode')
def test_every_new_entry_point_refuses_without_a_device():
  lib = _native.load()
  assert lib.bnf_member_log_density(None, None, None, 2, 4, None, None) == -2
  assert 'no CPU fallback' in _native.last_error()
  assert lib.bnf_stacking_weights(None, None, 2, 4, None, 10, 1e-5, None, 0, None, None, None) == -2
  assert 'no CPU fallback' in _native.last_error()
  assert lib.bnf_predictive_samples_weighted(None, None, None, 2, 4, 1, 0, 0, 0, None, None) == -2
  assert 'no CPU fallback' in _native.last_error()
  assert lib.bnf_predictive_group_sums_weighted(None, None, None, 2, 4, None, None, 1, 1, 0, 0, 0, None, None, 0, None) == -2
  assert 'no CPU fallback' in _native.last_error()


def _frame():
  t = pd.date_range('2020-01-06', periods=4, freq='W-MON')
  return pd.DataFrame({'t': np.repeat(t, 3), 'place': np.tile(['a', 'b', 'c'], 4), 'y': np.arange(12.0)})


def _params(lead):
  """What `fit` leaves in params_, as far as the weight checks look: a tuple of leaves with the ensemble dims in front."""
  return (np.zeros(lead + (3,)), np.zeros(lead))


def test_mixture_weights_helper():
  p = _params((1, 4))
  assert inference.mixture_weights(None, p, 2) == (None, None)
  w, cum = inference.mixture_weights([[0.1, 0.2, 0.3, 0.4]], p, 2)
  assert w.dtype == cum.dtype == np.float64 and w.shape == cum.shape == (4,)
  assert np.array_equal(cum[:3], np.cumsum([0.1, 0.2, 0.3])) and cum[-1] == 1.0
  w, cum = inference.mixture_weights(np.full((1, 4), 0.25) + 2e-10, p, 2)      # inside the 1e-9 of the sum
  assert cum[-1] == 1.0 and np.all(np.diff(cum) >= 0)
  # VI: the posterior draws are components, flattened as member_log_prob is
  wv = np.arange(10.0).reshape(1, 5, 2) / 45.0
  w, cum = inference.mixture_weights(wv, _params((1, 5, 2)), 3)
  assert np.array_equal(w, wv.reshape(-1)) and cum[-1] == 1.0
  for bad, msg in (([0.25] * 4, 'shape'), ([[0.5, 0.5]], 'shape'), ([[0.5, 0.5, np.nan, 0.0]], 'finite'),
                   ([[0.5, 0.5, np.inf, 0.0]], 'finite'), ([[0.7, 0.5, -0.2, 0.0]], '>= 0'),
                   ([[0.25, 0.25, 0.25, 0.25 + 1e-8]], 'sum to 1'), ([[0.0] * 4], 'sum to 1'), ('abcd', 'weights')):
    with pytest.raises(ValueError, match=msg):
      inference.mixture_weights(bad, p, 2)


@pytest.mark.parametrize('cls,lead', [(BayesianNeuralFieldMAP, (1, 4)), (BayesianNeuralFieldVI, (1, 5, 2))])
def test_estimators_check_weights_and_targets_before_any_gpu_work(cls, lead, monkeypatch):
  df = _frame()
  est = cls(feature_cols=['t'], target_col='y', freq='W', width=64, observation_model='NB')
  good = np.full(lead, 1.0 / np.prod(lead))
  for call in (lambda: est.stacking_weights(df), lambda: est.weighted_log_density(df, good),
               lambda: est.predict_samples(df, 5, weights=good)):
    with pytest.raises(ValueError, match='before fit'):
      call()

  def no_gpu(*a, **k):
    raise AssertionError('GPU work was reached')
  monkeypatch.setattr(inference, '_ensemble_forecast', no_gpu)
  monkeypatch.setattr(inference, 'Engine', no_gpu)
  est.params_ = _params(lead)
  calls = (lambda w: est.predict_samples(df, 5, weights=w), lambda w: est.predict_samples(df, 5, group_by='t', weights=w),
           lambda w: est.predict_totals(df, 't', num_samples=5, weights=w),
           lambda w: est.score_totals(df, 't', num_samples=5, weights=w), lambda w: est.weighted_log_density(df, w))
  bads = ((good.reshape(-1), 'shape'), (np.where(np.arange(good.size).reshape(lead) == 0, np.nan, good), 'finite'),
          (good - 2.0 * good * (np.arange(good.size).reshape(lead) == 1) + 2.0 * good * (np.arange(good.size).reshape(lead) == 0), '>= 0'),
          (good * 1.001, 'sum to 1'))
  for call in calls:
    for bad, msg in bads:
      with pytest.raises(ValueError, match=msg):
        call(bad)
    with pytest.raises(AssertionError, match='GPU work'):      # good weights pass the checks and reach the GPU seam
      call(good)
  with pytest.raises(ValueError, match='weights are required'):
    est.weighted_log_density(df, None)
  # the target checks of `score`
  for call in (lambda d: est.stacking_weights(d), lambda d: est.weighted_log_density(d, good)):
    with pytest.raises(ValueError, match='target column'):
      call(df.drop(columns='y'))
    d = df.copy()
    d.loc[3, 'y'] = 2.5
    with pytest.raises(ValueError, match='non-negative integer'):
      call(d)
    d.loc[3, 'y'] = np.nan                          # a NaN target is no error: it reaches the GPU seam
    with pytest.raises(AssertionError, match='GPU work'):
      call(d)
  with pytest.raises(ValueError, match='max_iter'):
    inference.stack_members(np.zeros((12, 1)), np.zeros(12), 'NB', est.params_, None, len(lead), max_iter=-1)
  with pytest.raises(ValueError, match='tol'):
    inference.stack_members(np.zeros((12, 1)), np.zeros(12), 'NB', est.params_, None, len(lead), tol=float('nan'))


def test_no_weights_reach_the_calls_that_were_there_before(monkeypatch):
  """weights=None: sample_predictive and total_summaries are called without the keyword, and the engine's equal-weight
  entry points without cum_weights."""
  df = _frame()
  est = BayesianNeuralFieldMAP(feature_cols=['t'], target_col='y', freq='W', width=64, observation_model='NORMAL')
  est.params_ = _params((1, 4))
  seen = []

  def fake_samples(features, observation_model, params, model_args, num_samples, seed, ensemble_dims, groups=None,
                   compute_dtype=None):
    seen.append('samples')
    return np.zeros((num_samples, 12), dtype=np.float32) if groups is None else np.zeros((num_samples, 4))

  def fake_totals(features, observation_model, params, model_args, num_samples, seed, ensemble_dims, groups, observed=None,
                  quantiles=(), energy=True, compute_dtype=None):
    seen.append('totals')
    G = len(groups[0]) - 1
    return dict(mean=np.zeros(G), quantiles=np.zeros((len(quantiles), G)), pit=np.zeros((2, G)), crps=np.zeros(G),
                energy_score=0.0)
  monkeypatch.setattr(inference, 'sample_predictive', fake_samples)
  monkeypatch.setattr(inference, 'total_summaries', fake_totals)
  assert est.predict_samples(df, 3).shape == (3, 12)
  assert est.predict_samples(df, 3, group_by='t', weights=None)[0].shape == (3, 4)
  est.predict_totals(df, 't', num_samples=3)
  est.score_totals(df, 't', num_samples=3, weights=None)
  assert seen == ['samples', 'samples', 'totals', 'totals']
  with pytest.raises(TypeError, match='weights'):                 # and weights do travel when they are given
    est.predict_totals(df, 't', num_samples=3, weights=np.full((1, 4), 0.25))

  class Lib:
    def __getattr__(self, name):
      def f(*a):
        seen.append(name)
        return 0
      return f
  from bayesnf_amd.engine import Engine
  eng = Engine.__new__(Engine)
  eng.lib, eng.handle, eng.device = Lib(), None, torch.device('cpu')
  monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **k: None)
  del seen[:]
  loc, aux = torch.zeros((4, 12)), torch.zeros((4, 3))
  off, rows_ = inference.csr_from_codes(np.arange(12) // 3, 4)
  eng.predictive_samples(loc, aux, 3, seed=1)
  eng.predictive_group_sums(loc, aux, off, rows_, 3, seed=1)
  eng.predictive_samples(loc, aux, 3, seed=1, cum_weights=np.asarray([0.25, 0.5, 0.75, 1.0]))
  eng.predictive_group_sums(loc, aux, off, rows_, 3, seed=1, cum_weights=np.asarray([0.25, 0.5, 0.75, 1.0]))
  assert seen == ['bnf_predictive_samples', 'bnf_predictive_group_sums', 'bnf_predictive_samples_weighted',
                  'bnf_predictive_group_sums_weighted']
  with pytest.raises(ValueError, match='cum_weights'):
    eng.predictive_samples(loc, aux, 3, seed=1, cum_weights=np.asarray([0.5, 1.0]))
