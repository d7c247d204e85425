"""CPU checks of the weighted-forecast references (tests/weighted_ref.py) the GPU tests of tests/test_gpu_weighted.py
are measured against, and of the Python plumbing that must hold before any GPU work: the references against the
equal-weight ones, against single-member closed forms, against quadrature and against the expectation form of the RPS; the
float32 restatements' own errors (the GPU bars are max(1e-5, 4 x these)); the ABI names; the weight checks of predict /
score."""
import os
import re

import numpy as np
import pandas as pd
import pytest
from scipy import special as sp
from scipy import stats

from bayesnf_amd import BayesianNeuralFieldMAP, BayesianNeuralFieldVI, _native, inference
from oracle import bnf_oracle as O
from tests import rps_ref as P
from tests import scoring_ref as S
from tests import weighted_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = (('bnf_normal_mixture_quantiles_weighted', 10), ('bnf_count_mixture_quantiles_weighted', 10),
       ('bnf_predictive_scores_weighted', 12), ('bnf_count_rps_weighted', 8))


def _close(a, b, tol=1e-12):
  a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
  assert np.array_equal(np.isnan(a), np.isnan(b))
  ok = ~np.isnan(b)
  assert np.all(np.abs(a[ok] - b[ok]) <= tol * np.maximum(1.0, np.abs(b[ok]))), float(np.max(np.abs(a[ok] - b[ok])))


def test_weight_patterns_are_on_the_simplex():
  for M in (1, 2, 7, 65):
    for p in W.PATTERNS:
      w = W.weights(p, M)
      assert w.shape == (M,) and w.dtype == np.float64 and np.all(w >= 0) and abs(w.sum() - 1.0) <= 1e-12, (p, M)
  assert np.count_nonzero(W.weights('one_hot', 7)) == 1 and np.count_nonzero(W.weights('every_second_zero', 7)) == 4
  assert W.weights('tiny_outlier', 7)[-1] == 1e-12 and W.weights('dirichlet', 65).max() > 5.0 / 65


def test_uniform_weights_reproduce_the_equal_weight_references():
  loc, sigma, y = S.normal_case(7, 65)
  y = y.copy()
  y[3] = np.nan
  w = np.full(7, 1.0 / 7)
  got, want = W.normal_ref(loc, sigma, y, w), S.normal_ref(loc, sigma, y)
  for k in ('lpd', 'pit', 'crps', 'crps_first'):
    _close(got[k], want[k])
  _close(W.normal_cdf(loc, sigma, y, w)[np.isfinite(y)], O.mixture_cdf(loc, sigma, y.astype(np.float64))[np.isfinite(y)])
  for obs in ('NB', 'ZINB'):
    loc, aux, yc = P.many_member_case(obs, M=7, R=25)
    fc = P.forecast(S.count_grid_model(obs), loc, aux)
    got, want = W.count_ref(fc, yc, w), S.count_ref(fc, yc)
    for k in ('lpd', 'pit'):
      _close(got[k], want[k])
    _close(W.count_rps_ref(fc, yc, w), P.count_rps_ref(fc, yc))


def test_one_hot_weights_reproduce_the_single_member_closed_forms():
  loc, sigma, y = S.normal_case(7, 65)
  w = W.weights('one_hot', 7)
  m = int(np.argmax(w))
  got = W.normal_ref(loc, sigma, y, w)
  mu, s, yy = loc[m].astype(np.float64), float(sigma[m]), y.astype(np.float64)
  z = (yy - mu) / s
  _close(got['lpd'], stats.norm.logpdf(yy, mu, s))
  _close(got['pit'][0], stats.norm.cdf(z))
  _close(got['crps'], s * (z * (2.0 * stats.norm.cdf(z) - 1.0) + 2.0 * stats.norm.pdf(z) - 1.0 / np.sqrt(np.pi)), 1e-11)
  _close(W.normal_moment_quantile(loc, sigma, 0.975, w), mu + s * sp.ndtri(0.975))
  for obs in ('NB', 'ZINB'):
    loc, aux, yc = P.many_member_case(obs, M=7, R=25)
    fc = P.forecast(S.count_grid_model(obs), loc, aux)
    one = dict(tc=fc['tc'][m:m + 1], logits=fc['logits'][m:m + 1], pi=None if fc['pi'] is None else fc['pi'][m:m + 1])
    got, want = W.count_ref(fc, yc, w), S.count_ref(one, yc)
    for k in ('lpd', 'pit'):
      _close(got[k], want[k])
    _close(W.count_rps_ref(fc, yc, w), P.count_rps_ref(one, yc))


@pytest.mark.parametrize('pattern', ['dirichlet', 'tiny_outlier'])
def test_weighted_normal_crps_against_quadrature(pattern):
  """int (F_w(x) - 1{x >= y})^2 dx by the trapezoid rule on 4e6 points over [-40, 40], M = 7 (sigma from 0.01 to 3: the
  step 2e-5 resolves the narrowest member): within 1e-5 absolute of the closed form (measured 2e-6: the rule's error at the
  jump of the indicator is half a step)."""
  loc, sigma, y, w = W.normal_case(7, 3, pattern)
  ref = W.normal_ref(loc, sigma, y, w)
  x = np.linspace(-40.0, 40.0, 4_000_000)
  worst = 0.0
  for r in range(3):
    Fw = np.zeros_like(x)
    for m in range(7):
      Fw += w[m] * O._ndtr((x - float(loc[m, r])) / float(sigma[m]))   # pylint: disable=protected-access
    g = (Fw - (x >= float(y[r]))) ** 2
    quad = float(np.sum(0.5 * (g[1:] + g[:-1])) * (x[1] - x[0]))
    worst = max(worst, abs(quad - ref['crps'][r]))
  print(f'{pattern}: worst |closed form - quadrature| {worst:.2e}')
  assert worst <= 1e-5


@pytest.mark.parametrize('obs', ['NB', 'ZINB'])
def test_weighted_rps_against_the_expectation_form(obs):
  """rps = E|X - y| - (1 / 2) E|X - X'| under the weighted pmf, on an explicit pmf vector: within 1e-10 relative."""
  rng = np.random.default_rng(5)
  worst = 0.0
  for M in (1, 3, 7):
    for pattern in W.PATTERNS:
      w = W.weights(pattern, M)
      tc = rng.uniform(0.5, 8.0, M)
      mean = rng.uniform(0.5, 40.0, M)
      pi = rng.uniform(0.05, 0.6, M) if obs == 'ZINB' else None
      logits = np.log(mean / tc)[:, None]
      fc = dict(tc=tc[:, None], logits=logits, pi=None if pi is None else pi[:, None])
      k = np.arange(4001.0)
      pmf = stats.nbinom.pmf(k[None, :], tc[:, None], 1.0 / (1.0 + mean / tc)[:, None])
      if pi is not None:
        pmf = (1.0 - pi[:, None]) * pmf
        pmf[:, 0] += pi
      pmf = w @ pmf
      assert abs(pmf.sum() - 1.0) < 1e-12
      ys = np.asarray([0.0, 1.0, np.round(mean.mean()), np.round(mean.max() * 3.0)])
      got = W.count_rps_ref(dict(fc, logits=np.tile(logits, (1, len(ys)))), ys, w)
      want = P.rps_by_expectations(pmf, ys)
      worst = max(worst, float(np.max(np.abs(got - want) / want)))
  print(f'{obs}: worst |ref - identity| / identity {worst:.2e}')
  assert worst <= 1e-10


def test_restatement_error_table_scores():
  """The float32 restatements of lpd / pit / crps against the float64 references on the shapes of the GPU test, every
  weight pattern: every GPU bar max(1e-5, 4 x error) is the 1e-5 gate, i.e. the errors stay under 2.5e-6."""
  worst = dict(lpd=0.0, pit=0.0, crps=0.0)
  print('model   M     R  pattern              lpd      pit      crps')
  for M in W.SCORE_MEMBERS_NORMAL:
    for R in (65, S.ROW_TILE + 1):
      for p in W.PATTERNS:
        loc, sigma, y, w = W.normal_case(M, R, p)
        ref, f32 = W.normal_ref(loc, sigma, y, w), W.normal_f32(loc, sigma, y, w)
        e = dict(lpd=S.rel1(f32['lpd'], ref['lpd']), pit=S.abs_err(f32['pit'], ref['pit']), crps=S.crps_err(f32['crps'], ref))
        print(f'NORMAL {M:3d} {R:5d}  {p:18s} {e["lpd"]:.1e}  {e["pit"]:.1e}  {e["crps"]:.1e}')
        worst = {k: max(worst[k], e[k]) for k in worst}
  for obs in ('NB', 'ZINB'):
    for M in W.SCORE_MEMBERS_COUNT:
      for p in W.PATTERNS:
        loc, aux, y, w = W.count_case_w(obs, M, 65, p)
        fc = P.forecast(S.count_grid_model(obs), loc, aux)
        ref, f32 = W.count_ref(fc, y, w), W.count_f32(loc, aux, y, obs, w)
        e = dict(lpd=S.rel1(f32['lpd'], ref['lpd']), pit=S.abs_err(f32['pit'], ref['pit']))
        print(f'{obs:6s} {M:3d} {65:5d}  {p:18s} {e["lpd"]:.1e}  {e["pit"]:.1e}')
        worst = {k: max(worst[k], e.get(k, 0.0)) for k in worst}
  print('worst', worst)
  for k, v in worst.items():
    assert S.bar(v) == S.GATE, (k, v)
  # the tail case: every density underflows, the weighted lpd stays finite in the restatement as in the reference
  loc, sigma, y = S.tail_case(7)
  w = W.weights('dirichlet', 7)
  ref, f32 = W.normal_ref(loc, sigma, y, w), W.normal_f32(loc, sigma, y, w)
  assert np.all(np.isfinite(f32['lpd'])) and S.bar(S.rel1(f32['lpd'], ref['lpd'])) == S.GATE


def test_restatement_error_table_rps_and_no_capped_row():
  """Every RPS case of the GPU test: the numpy restatement of the kernel's algorithm against the brute-force reference, no
  row capped or NaN (so the GPU test may demand NaN nowhere), every bar the 1e-5 gate."""
  worst = 0.0
  print('kind     obs    key  pattern             restatement  longest window')
  for case in W.rps_cases():
    _, _, y, w, ref, f64, terms = W.rps_get(*case)
    assert np.all(P.valid_target(y)) and np.all(np.isfinite(ref)) and np.all(ref > 0), case
    assert np.all(np.isfinite(f64)) and np.all(terms > 0) and terms.max() < P.MAX_TERMS, case
    e = P.rel_err(f64, ref)
    print(f'{case[0]:8s} {case[1]:5s} {case[2]:5g}  {case[3]:18s}  {e:.1e}  {terms.max()}')
    worst = max(worst, e)
  assert P.bar(worst) == S.GATE, worst


def test_entry_points_declared_listed_and_exported():
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'bnf.h')).read(), flags=re.S)
  lib = _native.load()
  for name, n_args in NEW:
    assert re.search(r'\bint\s+' + name + r'\s*\(', src), f'{name} is not declared in include/bnf.h'
    assert name in _native.EXPORTS
    fn = getattr(lib, name)
    assert fn.argtypes is not None and len(fn.argtypes) == n_args
  assert _native.ABI_VERSION == 6 and lib.bnf_abi_version() == 6          # purely additive
  from bayesnf_amd.engine import Engine
  import inspect
  for name in ('normal_mixture_quantiles', 'count_mixture_quantiles', 'predictive_scores', 'count_rps'):
    assert inspect.signature(getattr(Engine, name)).parameters['weights'].default is None


def _frame():
  t = pd.date_range('2020-01-06', periods=4, freq='W-MON')
  return pd.DataFrame({'t': np.repeat(t, 3), 'place': np.tile(['a', 'b', 'c'], 4), 'y': np.arange(12.0)})


def _params(lead):
  """What `fit` leaves in params_, as far as the weight checks look: a tuple of leaves with the ensemble dims in front."""
  return (np.zeros(lead + (3,)), np.zeros(lead))


@pytest.mark.parametrize('cls,lead', [(BayesianNeuralFieldMAP, (1, 4)), (BayesianNeuralFieldVI, (1, 5, 2))])
def test_predict_and_score_check_weights_before_any_gpu_work(cls, lead, monkeypatch):
  df = _frame()
  est = cls(feature_cols=['t'], target_col='y', freq='W', width=64, observation_model='NB')

  def no_gpu(*a, **k):
    raise AssertionError('GPU work was reached')
  monkeypatch.setattr(inference, '_ensemble_forecast', no_gpu)
  monkeypatch.setattr(inference, 'Engine', no_gpu)
  est.params_ = _params(lead)
  good = np.full(lead, 1.0 / np.prod(lead))
  idx = np.arange(good.size).reshape(lead)
  bads = ((good.reshape(-1), 'shape'), (np.where(idx == 0, np.nan, good), 'finite'),
          (good - 2.0 * good * (idx == 1) + 2.0 * good * (idx == 0), '>= 0'), (good * 1.001, 'sum to 1'))
  calls = (lambda w: est.predict(df, quantiles=(0.1, 0.9), weights=w), lambda w: est.score(df, weights=w),
           lambda w: est.score(df, rps=True, weights=w))
  for call in calls:
    for bad, msg in bads:
      with pytest.raises(ValueError, match=msg):
        call(bad)
    with pytest.raises(AssertionError, match='GPU work'):      # good weights pass the checks and reach the GPU seam
      call(good)
    with pytest.raises(AssertionError, match='GPU work'):
      call(None)


def test_no_weights_reach_the_calls_that_were_there_before(monkeypatch):
  """weights=None: predict_bnf and score_predictive are called without the keyword, and the engine's equal-weight entry
  points are the ones that run; given weights travel, and a member of weight 0 is dropped before the weighted call."""
  import torch
  df = _frame()
  est = BayesianNeuralFieldMAP(feature_cols=['t'], target_col='y', freq='W', width=64, observation_model='NB')
  est.params_ = _params((1, 4))
  seen = []

  def fake_predict(features, observation_model, params, model_args, quantiles, ensemble_dims=2,
                   approximate_quantiles=False, compute_dtype=None):
    seen.append('predict')
    return np.zeros((1, 4, 12)), [np.zeros(12) for _ in quantiles]

  def fake_score(features, target, observation_model, params, model_args, ensemble_dims, compute_dtype=None, rps=False):
    seen.append('score')
    return {'log_density': np.zeros(12, dtype=np.float32), 'pit': np.zeros((2, 12), dtype=np.float32),
            'member_log_prob': np.zeros((1, 4))}
  monkeypatch.setattr(inference, 'predict_bnf', fake_predict)
  monkeypatch.setattr(inference, 'score_predictive', fake_score)
  est.predict(df)
  est.predict(df, weights=None)
  est.score(df)
  est.score(df, weights=None)
  assert seen == ['predict', 'predict', 'score', 'score']
  for call in (lambda w: est.predict(df, weights=w), lambda w: est.score(df, weights=w)):
    with pytest.raises(TypeError, match='weights'):               # and weights do travel when they are given
      call(np.full((1, 4), 0.25))

  class Lib:
    def __getattr__(self, name):
      def f(*a):
        seen.append((name, int(a[4]) if name.endswith('_weighted') else int(a[3])))     # n_members
        return 0
      return f
  from bayesnf_amd.engine import Engine
  eng = Engine.__new__(Engine)
  eng.lib, eng.handle, eng.device = Lib(), None, torch.device('cpu')
  eng.net = type('Net', (), {'observation_model': 'NORMAL'})()
  monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **k: None)
  del seen[:]
  loc, aux, y = torch.zeros((4, 12)), torch.ones((4, 3)), torch.zeros(12)
  w = np.asarray([0.5, 0.0, 0.5, 0.0])
  eng.normal_mixture_quantiles(loc, aux[:, 0], (0.5,))
  eng.count_mixture_quantiles(loc, aux, (0.5,))
  eng.predictive_scores(loc, aux, y)
  eng.count_rps(loc, aux, y)
  assert seen == [('bnf_normal_mixture_quantiles', 4), ('bnf_count_mixture_quantiles', 4), ('bnf_predictive_scores', 4),
                  ('bnf_count_rps', 4)]
  del seen[:]
  eng.normal_mixture_quantiles(loc, aux[:, 0], (0.5,), weights=w)
  means, _ = eng.count_mixture_quantiles(loc, aux, (0.5,), weights=w)
  res = eng.predictive_scores(loc, aux, y, weights=w)
  eng.count_rps(loc, aux, y, weights=torch.from_numpy(w))
  assert means.shape == (4, 12) and res['member_ll'].shape == (4,)
  assert seen == [('bnf_normal_mixture_quantiles_weighted', 2), ('bnf_count_mixture_quantiles', 4),
                  ('bnf_count_mixture_quantiles_weighted', 2), ('bnf_predictive_scores', 4),
                  ('bnf_predictive_scores_weighted', 2), ('bnf_count_rps_weighted', 2)]
  with pytest.raises(ValueError, match='weights'):
    eng.count_rps(loc, aux, y, weights=np.asarray([0.5, 0.5]))
  with pytest.raises(ValueError, match='weight 0'):
    eng.count_rps(loc, aux, y, weights=np.zeros(4))


def test_likelihood_objects_take_weights_on_the_host():
  rng = np.random.default_rng(2)
  loc, scale = rng.standard_normal((1, 4, 9)), rng.uniform(0.5, 2.0, (1, 4))
  lik = inference.EnsembleLikelihood(loc, scale)
  x = rng.standard_normal(9)
  w = np.asarray([[0.1, 0.0, 0.6, 0.3]])
  _close(lik.mixture_cdf(x, weights=w), W.normal_cdf(loc.reshape(4, 9), scale.reshape(4), x, w.reshape(-1)))
  assert np.array_equal(lik.mixture_cdf(x), lik.cdf(x).reshape(4, 9).mean(axis=0))
  _close(lik.mixture_cdf(x, weights=np.full((1, 4), 0.25)), lik.mixture_cdf(x))
  with pytest.raises(ValueError, match='shape'):
    lik.mixture_cdf(x, weights=w.reshape(-1))
  tc, logits = rng.uniform(0.5, 5.0, (1, 4)), rng.standard_normal((1, 4, 9))
  cl = inference.CountEnsembleLikelihood(tc, logits, rng.uniform(0.1, 0.5, (1, 4)))
  k = np.arange(9.0)
  fc = dict(tc=tc.reshape(4, 1), logits=logits.reshape(4, 9), pi=cl.inflated_loc_probs.reshape(4, 1))
  _close(cl.mixture_cdf(k, weights=w), W.count_cdf(fc, k, w.reshape(-1)))
  assert np.array_equal(cl.mixture_cdf(k), cl.cdf(k).reshape(4, 9).mean(axis=0))
