"""CPU-only checks of the ranked probability score (include/bnf.h bnf_count_rps): the brute-force float64 reference of
tests/rps_ref.py against the independent identity E|X - y| - 0.5 E|X - X'|, the numpy restatement of the kernel's window
algorithm against that reference on the GPU tests' grid (the table DESIGN.md quotes), and the entry point's declaration,
binding and Python seam."""
import os
import re

import numpy as np
import pytest
from scipy import stats

from bayesnf_amd import _native, inference
from bayesnf_amd.engine import Engine
from tests import rps_ref as P
from tests import scoring_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('obs', ['NB', 'ZINB'])
@pytest.mark.parametrize('M', [1, 3])
def test_reference_against_the_expectation_identity(obs, M):
  """sum_k (F(k) - 1{k >= y})^2 = E|X - y| - 0.5 E|X - X'| for any law on the integers.  The right-hand side from an
  explicit pmf vector (scipy.stats.nbinom.pmf, zero inflation by hand) on 0 .. 4000: means <= 30 at total_count >= 0.3 leave
  less than 1e-15 of the mass beyond.  1e-10 relative."""
  rng = np.random.default_rng([M, obs == 'ZINB'])
  worst = 0.0
  for _ in range(6):
    tc = rng.choice([0.3, 1.0, 3.0, 40.0], M)
    mean = rng.uniform(0.05, 30.0, M)
    pi = rng.uniform(0.05, 0.6, M) if obs == 'ZINB' else None
    logits = np.log(mean / tc)[:, None]                      # mean = tc e^logits
    fc = dict(tc=tc[:, None], logits=logits, pi=None if pi is None else pi[:, None])
    k = np.arange(4001.0)
    pmf = stats.nbinom.pmf(k[None, :], tc[:, None], 1.0 / (1.0 + mean / tc)[:, None])
    if pi is not None:
      pmf = (1.0 - pi[:, None]) * pmf
      pmf[:, 0] += pi
    pmf = pmf.mean(axis=0)
    assert abs(pmf.sum() - 1.0) < 1e-12
    ys = np.asarray([0.0, 1.0, np.round(mean.mean()), np.round(mean.max() * 3.0)])
    got = P.count_rps_ref(dict(fc, logits=np.tile(logits, (1, len(ys)))), ys)
    want = P.rps_by_expectations(pmf, ys)
    worst = max(worst, float(np.max(np.abs(got - want) / want)))
  print(f'{obs} M={M}: worst |ref - identity| / identity {worst:.2e}')
  assert worst <= 1e-10


def test_restatement_error_table():
  """The kernel's algorithm in numpy against the brute-force reference on the whole grid of the GPU test (total_count
  0.05 .. 1e3 x mean 0.02 .. 400, M 1 and 7, NB and ZINB, four targets per row): within 1e-6, every row finite, every window
  under the cap.  The GPU test's bars are max(1e-5, 4 x these)."""
  worst, longest = 0.0, 0
  print('obs   M  total_count  restatement  longest window')
  for obs, tc, M in P.grid():
    _, _, _, ref, f64, terms = P.grid_case(obs, tc, M)
    assert np.all(np.isfinite(ref)) and np.all(ref > 0) and np.all(np.isfinite(f64)) and np.all(terms > 0)
    e = P.rel_err(f64, ref)
    print(f'{obs:5s} {M}  {tc:<11g}  {e:.2e}     {terms.max()}')
    worst, longest = max(worst, e), max(longest, int(terms.max()))
  print(f'worst {worst:.2e}, longest window {longest} of {P.MAX_TERMS}')
  assert worst <= 1e-6
  assert longest <= P.MAX_TERMS


def test_restatement_edges():
  """Closed-form terms and the NaN rows of the restatement against the reference: y far above the window, y = 0 under a
  window that starts above 0, and the targets that are not counts."""
  from tests.test_gpu_sampling import count_case
  model = S.count_grid_model('ZINB')
  loc7, aux, fc7 = count_case(model, 1e3, 7)
  loc = np.tile(loc7[:, 4:5], (1, 6))                       # mean 400, total_count 1e3
  fc = dict(tc=fc7['tc'], logits=np.tile(fc7['logits'][:, 4:5], (1, 6)), pi=fc7['pi'])
  y = np.asarray([0.0, 5000.0, np.nan, -1.0, 2.5, 400.0])
  ref = P.count_rps_ref(fc, y)
  f64, terms, starts = P.count_rps_f64(loc, aux, y, 'ZINB')
  assert np.array_equal(np.isnan(ref), [False, False, True, True, True, False])
  assert P.rel_err(f64, ref) <= 1e-6
  assert starts[0] > 0 and starts[0] + terms[0] + 1000 <= 5000


def test_entry_point_declared_bound_and_wrapped():
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'bnf.h')).read(), flags=re.S)
  assert re.search(r'\bint\s+bnf_count_rps\s*\(', src), 'bnf_count_rps is not declared in include/bnf.h'
  terms = re.search(r'#define\s+BNF_RPS_MAX_TERMS\s+\(1\s*<<\s*(\d+)\)', src)
  assert terms and 1 << int(terms.group(1)) == _native.RPS_MAX_TERMS == P.MAX_TERMS
  assert int(re.search(r'#define\s+BNF_RPS_MAX_MEMBERS\s+(\d+)', src).group(1)) == _native.RPS_MAX_MEMBERS
  assert 'bnf_count_rps' in _native.EXPORTS
  lib = _native.load()                       # the library built for gfx950 by build()
  assert lib.bnf_count_rps.argtypes is not None and len(lib.bnf_count_rps.argtypes) == 7
  assert _native.ABI_VERSION == 6 and lib.bnf_abi_version() == 6          # purely additive
  assert callable(getattr(Engine, 'count_rps', None))


def test_rps_on_a_normal_model_is_refused_before_any_gpu_work(monkeypatch):
  import pandas as pd
  from bayesnf_amd import BayesianNeuralFieldMAP

  def no_gpu(*a, **k):
    raise AssertionError('GPU work was reached')
  monkeypatch.setattr(inference, '_ensemble_forecast', no_gpu)
  df = pd.DataFrame({'t': pd.date_range('2020-01-06', periods=8, freq='W-MON'), 'y': np.arange(8.0)})
  est = BayesianNeuralFieldMAP(feature_cols=['t'], target_col='y', freq='W', width=64, observation_model='NORMAL')
  est.params_ = object()
  with pytest.raises(ValueError, match="'crps'"):
    est.score(df, rps=True)
  with pytest.raises(ValueError, match="'crps'"):
    inference.score_predictive(np.zeros((8, 1)), np.zeros(8), 'NORMAL', None, None, None, rps=True)
