"""CPU-only checks of the summaries and scores of group totals (include/bnf.h bnf_sample_summaries /
bnf_sample_energy_score): the numpy restatement of the kernels' sorted and centred forms against the brute-force float64
references of tests/totals_ref.py, at the bars the GPU tests use (the restatement's own error is printed: the bars have
slack); the entry points' declaration and export; their refusal without a device; the estimators' argument checks; the
observed totals formed on the host."""
import ctypes as C
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

from bayesnf_amd import BayesianNeuralFieldMAP, BayesianNeuralFieldVI, _native, inference
from bayesnf_amd import spatiotemporal
from tests import totals_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('kind', T.KINDS)
def test_sorted_and_centred_forms_against_the_brute_force(kind):
  worst = {}
  for S in T.SUMMARY_S:
    for G in T.SUMMARY_G:
      x, y, ref = T.summary_case(S, G, kind)
      got = T.summaries_sorted(x, y, T.LEVELS)
      w = T.check_summaries(f'{kind} S={S} G={G} restatement', got, x, y, T.LEVELS, ref)
      for k, v in w.items():
        worst[k] = max(worst.get(k, 0.0), v)
      assert np.array_equal(np.isnan(got['crps']), np.isnan(y))
  print(f'{kind}: worst error / bar of the restatement {worst}')


def test_a_total_of_1e9_with_a_spread_of_10_and_a_nan_sample():
  x, y, ref = T.summary_case(65, 9, 'big')
  got = T.summaries_sorted(x, y, T.LEVELS)
  T.check_summaries('big restatement', got, x, y, T.LEVELS, ref)
  scored = np.isfinite(y)
  assert np.array_equal(got['crps'][scored], ref['crps'][scored])      # integers: every term is exact on x - y
  xn = np.array(x)
  xn[17, 4] = np.nan
  gn = T.summaries_sorted(xn, y, T.LEVELS)
  for k in ('mean', 'crps'):
    assert np.isnan(gn[k][4]) and np.array_equal(np.delete(gn[k], 4), np.delete(got[k], 4), equal_nan=True)
  assert np.isnan(gn['quantiles'][:, 4]).all() and np.isnan(gn['pit'][:, 4]).all()


def test_crps_reference_against_the_quantile_of_a_known_law():
  """The brute-force CRPS of a big sample from N(0, 1) against the closed form for a Normal forecast,
  y (2 Phi(y) - 1) + 2 phi(y) - 1 / sqrt(pi): the ensemble CRPS is that of the empirical law, whose expected excess is
  O(1 / S); 6 standard errors of the two sample means (< 2 / sqrt(S) each) bound the rest."""
  from scipy import stats
  rng = np.random.default_rng(5)
  S = 4000
  x = rng.standard_normal((S, 2))
  y = np.asarray([0.3, -1.7])
  got = T.crps_ref(x, y)
  closed = y * (2 * stats.norm.cdf(y) - 1) + 2 * stats.norm.pdf(y) - 1 / np.sqrt(np.pi)
  print('crps_ref', got, 'closed form', closed)
  assert np.all(np.abs(got - closed) <= 6 * 2 / np.sqrt(S))


@pytest.mark.parametrize('S,G', T.ENERGY_SHAPES)
def test_energy_upper_triangle_against_the_double_sum(S, G):
  x, y, (ref, t1, t2) = T.energy_case(S, G)
  got = T.energy_upper(x, y)
  bar = T.energy_bar(S, G, t1, t2)
  print(f'S={S} G={G}: energy {ref:.6f} restatement error {abs(got - ref):.2e} bar {bar:.2e}')
  assert abs(got - ref) <= bar
  if G == 1:                                        # one column: the energy score is the CRPS
    assert abs(ref - T.crps_ref(x, y)[0]) <= T.crps_bars(x, y)[0]
  yn = np.array(y)
  yn[::3] = np.nan                                  # skipped columns: the score on the kept ones alone
  keep = np.isfinite(yn)
  if keep.any():
    assert T.energy_ref(x, yn)[0] == T.energy_ref(x[:, keep], y[keep])[0]
  assert np.isnan(T.energy_ref(x, np.full(G, np.nan))[0]) and np.isnan(T.energy_upper(x, np.full(G, np.nan)))


def test_entry_points_declared_listed_and_exported():
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'bnf.h')).read(), flags=re.S)
  lib = _native.load()
  for name, n_args in (('bnf_sample_summaries', 11), ('bnf_sample_energy_score', 8)):
    assert re.search(r'\bint\s+' + name + r'\s*\(', src), f'{name} is not declared in include/bnf.h'
    assert name in _native.EXPORTS
    fn = getattr(lib, name)
    assert fn.argtypes is not None and len(fn.argtypes) == n_args
  assert _native.ABI_VERSION == 6 and lib.bnf_abi_version() == 6          # purely additive
  for macro, val in (('BNF_SUMMARY_MAX_SAMPLES', _native.SUMMARY_MAX_SAMPLES),
                     ('BNF_SUMMARY_MAX_QUANTILES', _native.SUMMARY_MAX_QUANTILES),
                     ('BNF_ENERGY_SAMPLE_TILE', _native.ENERGY_SAMPLE_TILE)):
    assert int(re.search(r'#define\s+' + macro + r'\s+(\d+)', src).group(1)) == val
  assert _native.SUMMARY_MAX_SAMPLES == T.MAX_SAMPLES == 16384
  from bayesnf_amd.engine import Engine
  assert callable(getattr(Engine, 'sample_summaries', None)) and callable(getattr(Engine, 'sample_energy_score', None))


@pytest.mark.skipif(torch.cuda.is_available(), reason='checks the no-GPU failure mode')
def test_both_entry_points_refuse_without_a_device():
  lib = _native.load()
  q = (C.c_double * 1)(0.5)
  assert lib.bnf_sample_summaries(None, None, 4, 2, None, q, 1, None, None, None, None) == -2
  assert 'no CPU fallback' in _native.last_error()
  assert lib.bnf_sample_energy_score(None, None, 4, 2, None, None, 0, None) == -2
  assert 'no CPU fallback' in _native.last_error()


def _frame():
  t = pd.date_range('2020-01-06', periods=4, freq='W-MON')
  return pd.DataFrame({'t': np.repeat(t, 3), 'place': np.tile(['a', 'b', 'c'], 4), 'y': np.arange(12.0)})


@pytest.mark.parametrize('cls', [BayesianNeuralFieldMAP, BayesianNeuralFieldVI])
def test_totals_refuse_bad_calls_before_any_gpu_work(cls, monkeypatch):
  df = _frame()
  est = cls(feature_cols=['t'], target_col='y', freq='W', width=64, observation_model='NB')
  with pytest.raises(ValueError, match='before fit'):
    est.score_totals(df, 't')
  with pytest.raises(ValueError, match='before fit'):
    est.predict_totals(df, 't')

  def no_gpu(*a, **k):
    raise AssertionError('GPU work was reached')
  monkeypatch.setattr(inference, '_ensemble_forecast', no_gpu)
  est.params_ = object()                          # "fitted": everything below must fail on its arguments alone
  with pytest.raises(ValueError, match='target column'):
    est.score_totals(df.drop(columns='y'), 't')
  for bad in (0.5, -1.0):
    d = df.copy()
    d.loc[3, 'y'] = bad
    with pytest.raises(ValueError, match='non-negative integer'):
      est.score_totals(d, 't')
  with pytest.raises(ValueError, match='not among the columns'):
    est.score_totals(df, 'week')
  for call in (est.score_totals, est.predict_totals):
    with pytest.raises(ValueError, match='at most 16384'):
      call(df, 't', num_samples=16385)
    with pytest.raises(ValueError, match='at least one sample path'):
      call(df, 't', num_samples=0)
  groups = inference.csr_from_codes(np.arange(12) // 3, 4)
  with pytest.raises(ValueError, match='at most 16384'):
    inference.total_summaries(np.zeros((12, 1)), 'NB', None, None, 16385, 0, 2, groups)
  big = inference.csr_from_codes(np.arange(1 << 15), 1 << 15)
  with pytest.raises(ValueError, match='held whole'):
    inference.total_summaries(np.zeros((1 << 15, 1)), 'NB', None, None, 16384, 0, 2, big)      # 2^29 cells
  with pytest.raises(ValueError, match=r'\[0, 1\]'):
    inference.total_summaries(np.zeros((12, 1)), 'NB', None, None, 10, 0, 2, groups, quantiles=(0.5, 1.5))
  with pytest.raises(ValueError, match='one total per group'):
    inference.total_summaries(np.zeros((12, 1)), 'NB', None, None, 10, 0, 2, groups, observed=np.zeros(3))
  d = df.copy()
  d.loc[3, 'y'] = np.nan                          # a NaN target is no error: it reaches the GPU seam
  with pytest.raises(AssertionError, match='GPU work'):
    est.score_totals(d, 't')


def test_observed_is_nan_exactly_for_the_groups_with_a_nan_target_row(monkeypatch):
  df = _frame()
  df.loc[[4, 9, 10], 'y'] = np.nan                # weeks 1 and 3
  seen = {}

  def fake(features, observation_model, params, model_args, num_samples, seed, ensemble_dims, groups, observed=None,
           quantiles=(), energy=True, compute_dtype=None):
    seen.update(observed=observed, groups=groups, num_samples=num_samples, energy=energy)
    G = len(groups[0]) - 1
    return dict(mean=np.zeros(G), quantiles=np.zeros((len(quantiles), G)), pit=np.zeros((2, G)),
                crps=np.where(np.isnan(observed), np.nan, 2.0), energy_score=1.0)
  monkeypatch.setattr(inference, 'total_summaries', fake)
  est = BayesianNeuralFieldMAP(feature_cols=['t'], target_col='y', freq='W', width=64, observation_model='NORMAL')
  est.params_ = object()
  res = est.score_totals(df, 't', num_samples=7, seed=1)
  want = df.groupby('t')['y'].sum(min_count=3).to_numpy()            # NaN unless all three rows are there
  assert np.array_equal(np.isnan(res['observed']), [False, True, False, True])
  assert np.array_equal(res['observed'], want, equal_nan=True) and res['observed'].dtype == np.float64
  assert np.array_equal(seen['observed'], want, equal_nan=True) and seen['num_samples'] == 7 and seen['energy'] is True
  assert res['n'] == 2 and res['mean_crps'] == 2.0 and list(res['keys']) == list(df['t'].unique())
  assert set(res) == {'keys', 'observed', 'mean', 'quantiles', 'crps', 'pit', 'n', 'mean_crps', 'energy_score'}
  # by several columns, rows in any order
  shuffled = df.sample(frac=1.0, random_state=0)
  res = est.score_totals(shuffled, ['place', 't'], energy=False)
  want = df.set_index(['place', 't'])['y'].sort_index()
  assert np.array_equal(res['observed'], want.to_numpy(), equal_nan=True) and res['n'] == 9
  assert spatiotemporal.group_target_sums([1.0, 2.0, 4.0], [0, 1, 1, 3], [2, 0, 1]).tolist()[::2] == [4.0, 3.0]
