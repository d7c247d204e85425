"""CPU-only checks of the held-out scoring feature (include/bnf.h bnf_predictive_scores): the float64 reference formulas of
tests/scoring_ref.py against independent evaluations (quadrature, scipy.stats), the entry point's declaration and export,
the estimator's argument checks, and the float32 restatement's error table from which the GPU tests take their bars."""
import os
import re

import numpy as np
import pandas as pd
import pytest
from scipy import special as sp
from scipy import stats

from bayesnf_amd import BayesianNeuralFieldMAP, BayesianNeuralFieldVI, _native, inference
from oracle import bnf_oracle as O
from tests import scoring_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _crps_quadrature(loc, sigma, y, n):
  """int (F(x) - 1{x >= y})^2 dx by the trapezoid rule with n steps on either side of the jump at y, over
  [min mu - 12 max s, max mu + 12 max s] (the integrand left out is < Phi(-12)^2 = 3e-66 per unit length)."""
  lo = min(loc.min(), y) - 12.0 * sigma.max()
  hi = max(loc.max(), y) + 12.0 * sigma.max()
  cdf = lambda x: O.mixture_cdf(loc[:, None], sigma, x)
  xl, xr = np.linspace(lo, y, n + 1), np.linspace(y, hi, n + 1)
  trapezoid = lambda f, x: float(np.sum(0.5 * (f[1:] + f[:-1]) * np.diff(x)))
  return trapezoid(cdf(xl) ** 2, xl) + trapezoid((cdf(xr) - 1.0) ** 2, xr)


@pytest.mark.parametrize('M', [1, 3])
def test_crps_closed_form_against_quadrature(M):
  """The bar is the quadrature's own step error: |I_n - I_2n| bounds the error of I_2n (a third of it for the O(h^2)
  trapezoid rule), plus 1e-12 of the value for the rounding of 2n function values."""
  rng = np.random.default_rng(M)
  for _ in range(6):
    sigma = rng.uniform(0.05, 3.0, M)
    loc = 3.0 * rng.standard_normal(M)
    y = float(loc[0] + 2.0 * rng.standard_normal())
    closed, first = S.normal_crps(loc[:, None], sigma, np.asarray([y]))
    coarse, fine = _crps_quadrature(loc, sigma, y, 20000), _crps_quadrature(loc, sigma, y, 40000)
    step = abs(coarse - fine)
    print(f'M={M}: closed {closed[0]:.12f} quadrature {fine:.12f} step error {step:.2e}')
    assert 0.0 < closed[0] <= first[0]
    assert abs(closed[0] - fine) <= step + 1e-12 * fine, (closed[0], fine, step)


@pytest.mark.parametrize('obs', ['NB', 'ZINB'])
def test_count_reference_against_scipy_nbinom(obs):
  """log pmf and both CDF rows of `count_ref` against scipy.stats.nbinom(n = total_count, p = sigmoid(-logits)) with the
  zero inflation applied by hand, on the whole GPU grid: 1e-9 relative for the log pmf (lgamma triples of size y log y =
  3e8 in float64), 1e-10 for the CDF."""
  worst_lp = worst_cdf = 0.0
  for o, tc, M in S.count_grid():
    if o != obs:
      continue
    loc, aux, y, ref, _ = S.count_grid_case(obs, tc, M)
    fc = O.count_forecast(S.count_grid_model(obs), _theta(obs, aux), loc.astype(np.float64))
    p = sp.expit(-fc['logits'])
    n = np.broadcast_to(fc['tc'], p.shape)
    y64 = y.astype(np.float64)[None, :]
    pmf_lp, cdf, cdf_below = stats.nbinom.logpmf(y64, n, p), stats.nbinom.cdf(y64, n, p), stats.nbinom.cdf(y64 - 1.0, n, p)
    if obs == 'ZINB':
      pi = fc['pi']
      pmf_lp = np.where(y64 == 0, np.log(pi + (1 - pi) * np.exp(pmf_lp)), np.log1p(-pi) + pmf_lp)
      cdf, cdf_below = pi + (1 - pi) * cdf, np.where(y64 >= 1, pi + (1 - pi) * cdf_below, 0.0)
    worst_lp = max(worst_lp, float(np.max(np.abs(ref['lp'] - pmf_lp) / np.maximum(1.0, np.abs(pmf_lp)))))
    worst_cdf = max(worst_cdf, float(np.max(np.abs(ref['pit'] - np.stack([cdf.mean(axis=0), cdf_below.mean(axis=0)])))))
    assert np.all(ref['pit'][1][y == 0] == 0.0)
  print(f'{obs}: worst log pmf error {worst_lp:.2e}, worst cdf error {worst_cdf:.2e}')
  assert worst_lp <= 1e-9 and worst_cdf <= 1e-10


def _theta(obs, aux):
  model = S.count_grid_model(obs)
  theta = np.zeros((aux.shape[0], model.P))
  from tests.test_gpu_sampling import inv_softplus
  theta[:, model.leaf['shape'].offset] = inv_softplus(aux[:, 1].astype(np.float64))
  p = aux[:, 2].astype(np.float64)
  theta[:, model.leaf['inflated_loc_probs'].offset] = np.log(p) - np.log1p(-p)
  return theta


def test_lpd_is_the_log_of_the_mean_density_where_that_does_not_underflow():
  loc, sigma, y = S.normal_case(7, 65)
  ref = S.normal_ref(loc, sigma, y)
  with np.errstate(divide='ignore'):
    naive = np.log(np.mean(np.exp(ref['lp']), axis=0))
  ok = np.isfinite(naive) & (naive > -600)
  assert ok.sum() > 30
  np.testing.assert_allclose(ref['lpd'][ok], naive[ok], rtol=1e-12, atol=1e-12)
  # the tails: the naive form is -inf, the reference and the float32 restatement are not
  loc, sigma, y = S.tail_case(5)
  ref, f32 = S.normal_ref(loc, sigma, y), S.normal_f32(loc, sigma, y)
  with np.errstate(divide='ignore'):
    assert np.all(np.isneginf(np.log(np.mean(np.exp(ref['lp'].astype(np.float32)), axis=0))))
  assert np.all(np.isfinite(ref['lpd'])) and np.all(np.isfinite(f32['lpd'])) and ref['lpd'].max() < -700
  assert S.rel1(f32['lpd'], ref['lpd']) <= S.GATE


def test_nan_targets_are_nan_rows_and_leave_the_member_sums():
  loc, sigma, y = S.normal_case(3, 10)
  y = y.copy()
  y[[2, 7]] = np.nan
  keep = np.isfinite(y)
  for out in (S.normal_ref(loc, sigma, y), S.normal_f32(loc, sigma, y)):
    for k in ('lpd', 'crps'):
      assert np.array_equal(np.isnan(out[k]), ~keep)
    assert np.array_equal(np.isnan(out['pit']), np.stack([~keep, ~keep]))
    np.testing.assert_allclose(out['member_ll'], S.normal_ref(loc[:, keep], sigma, y[keep])['member_ll'], rtol=1e-5)


def test_entry_point_declared_listed_and_exported():
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'bnf.h')).read(), flags=re.S)
  lib = _native.load()                       # the library built for gfx950 by build()
  name = 'bnf_predictive_scores'
  assert re.search(r'\bint\s+' + name + r'\s*\(', src), f'{name} is not declared in include/bnf.h'
  assert name in _native.EXPORTS
  fn = getattr(lib, name)
  assert fn.argtypes is not None and len(fn.argtypes) == 12
  assert _native.ABI_VERSION == 6 and lib.bnf_abi_version() == 6          # purely additive
  for macro, val in (('BNF_SCORE_ROW_TILE', _native.SCORE_ROW_TILE), ('BNF_SCORE_MEMBER_CHUNK', _native.SCORE_MEMBER_CHUNK),
                     ('BNF_SCORE_MAX_SLOTS', _native.SCORE_MAX_SLOTS)):
    assert int(re.search(r'#define\s+' + macro + r'\s+(\d+)', src).group(1)) == val
  assert (S.ROW_TILE, S.MEMBER_CHUNK) == (_native.SCORE_ROW_TILE, _native.SCORE_MEMBER_CHUNK)


@pytest.mark.parametrize('cls', [BayesianNeuralFieldMAP, BayesianNeuralFieldVI])
def test_score_refuses_bad_calls_before_any_gpu_work(cls, monkeypatch):
  df = pd.DataFrame({'t': pd.date_range('2020-01-06', periods=8, freq='W-MON'), 'y': np.arange(8.0)})
  est = cls(feature_cols=['t'], target_col='y', freq='W', width=64, observation_model='NB')
  with pytest.raises(ValueError, match='before fit'):
    est.score(df)

  def no_gpu(*a, **k):
    raise AssertionError('GPU work was reached')
  monkeypatch.setattr(inference, 'score_predictive', no_gpu)
  monkeypatch.setattr(inference, '_ensemble_forecast', no_gpu)
  est.params_ = object()                          # "fitted": everything below must fail on its arguments alone
  with pytest.raises(ValueError, match='target column'):
    est.score(df.drop(columns='y'))
  for bad in (0.5, -1.0):
    d = df.copy()
    d.loc[3, 'y'] = bad
    with pytest.raises(ValueError, match='non-negative integer'):
      est.score(d)
  d = df.copy()
  d.loc[3, 'y'] = np.nan                          # a NaN target is no error: it reaches the GPU seam
  with pytest.raises(AssertionError, match='GPU work'):
    est.score(d)


def test_f32_restatement_error_table():
  """The table DESIGN.md quotes and the GPU tests take their bars from (max(1e-5, 4 x these)).  Asserted here: the forms
  keep the float32 restatement under the 1e-5 gate on the whole count grid and on the NORMAL shapes, VI's 1,920
  components included; pit under its absolute 1e-5."""
  worst = {}
  print('obs   M  total_count  lpd       member_ll pit')
  for obs, tc, M in S.count_grid():
    _, _, _, ref, f32 = S.count_grid_case(obs, tc, M)
    e = S.restatement_errors(ref, f32)
    print(f'{obs:5s} {M}  {tc:<11g}  {e["lpd"]:.2e}  {e["member_ll"]:.2e}  {e["pit"]:.2e}')
    for k, v in e.items():
      worst[obs, k] = max(worst.get((obs, k), 0.0), v)
  print('NORMAL  M     R     lpd       member_ll pit       crps')
  for M, R in ((1, 65), (7, 1025), (S.MEMBER_CHUNK + 1, 64), (64, 32), (1920, 4)):
    loc, sigma, y = S.normal_case(M, R)
    e = S.restatement_errors(S.normal_ref(loc, sigma, y), S.normal_f32(loc, sigma, y))
    print(f'        {M:<5d} {R:<5d} {e["lpd"]:.2e}  {e["member_ll"]:.2e}  {e["pit"]:.2e}  {e["crps"]:.2e}')
    for k, v in e.items():
      worst['NORMAL', k] = max(worst.get(('NORMAL', k), 0.0), v)
  loc, sigma, y = S.tail_case(7)
  e = S.restatement_errors(S.normal_ref(loc, sigma, y), S.normal_f32(loc, sigma, y))
  print(f'        tails M=7   {e["lpd"]:.2e}  {e["member_ll"]:.2e}  {e["pit"]:.2e}  {e["crps"]:.2e}')
  print({k: f'{v:.2e}' for k, v in worst.items()})
  for (obs, k), v in worst.items():
    assert v <= (S.PIT_BAR if k == 'pit' else S.GATE), (obs, k, v)
