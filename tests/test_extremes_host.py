"""CPU-only checks of the group peaks and threshold exceedances (include/bnf.h bnf_predictive_group_extremes): the
reference's own tie / NaN / empty rules on hand-made arrays; the entry point's declaration and export; the estimators'
argument checks, which fire before any GPU work; the observed peaks formed on the host."""
import os
import re

import numpy as np
import pandas as pd
import pytest

from bayesnf_amd import BayesianNeuralFieldMAP, BayesianNeuralFieldVI, _native, inference, spatiotemporal
from tests import extremes_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'bnf_predictive_group_extremes'


def test_reference_tie_nan_and_empty_rules():
  nan = np.nan
  #               row 0    1    2    3    4    5    6
  x = np.asarray([[1.0, 5.0, 5.0, nan, 2.0, 5.0, nan],
                  [0.0, 0.0, 0.0, nan, 0.0, 0.0, nan],
                  [nan, -3.0, nan, nan, nan, 7.0, nan]], dtype=np.float32)
  codes = np.asarray([0, 2, 0, 3, 2, 0, 3])                  # group 0 = rows {0, 2, 5}, 1 empty, 2 = {1, 4}, 3 = {3, 6}
  thr = np.asarray([0.5, 4.0, 5.0, 0.0, 2.0, -1.0, 0.0], dtype=np.float32)
  got = X.group_extremes(x, codes, 4, thr)
  inf = np.inf
  assert np.array_equal(got['max'], [[5.0, nan, 5.0, -inf], [0.0, nan, 0.0, -inf], [7.0, nan, -3.0, -inf]], equal_nan=True)
  # ties to the lowest table row (path 0 group 0: rows 2 and 5 tie; path 1: everything ties); an all-NaN group: its
  # first row at -inf; the empty group: -1
  assert np.array_equal(got['argmax'], [[2, -1, 1, 3], [0, -1, 1, 3], [5, -1, 1, 3]]) and got['argmax'].dtype == np.int32
  # strict >: 5.0 at row 2 does not exceed 5.0, 2.0 at row 4 does not exceed 2.0; a NaN draw never exceeds
  assert np.array_equal(got['count'], [[2.0, 0.0, 1.0, 0.0], [1.0, 0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]])
  assert np.array_equal(got['exceed_count'], [1, 1, 0, 0, 0, 3, 0])
  assert np.array_equal(got['peak_count'], [1, 3, 1, 3, 0, 1, 0]) and got['peak_count'].sum() == 3 * 3
  plain = X.group_extremes(x, codes, 4)
  assert 'count' not in plain and 'exceed_count' not in plain
  assert np.array_equal(plain['argmax'], got['argmax'])
  # 6 of the 9 (path, non-empty group) cells reach their maximum at more than one row
  assert X.tie_share(x, codes, 4) == pytest.approx(6 / 9)
  assert X.tie_share(np.arange(12.0).reshape(2, 6), [0, 0, 1, 1, 1, 2], 4) == 0.0


def test_entry_point_declared_listed_and_exported():
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'bnf.h')).read(), flags=re.S)
  lib = _native.load()
  assert re.search(r'\bint\s+' + NAME + r'\s*\(', src), f'{NAME} is not declared in include/bnf.h'
  assert NAME in _native.EXPORTS
  fn = getattr(lib, NAME)
  assert fn.argtypes is not None and len(fn.argtypes) == 21
  assert _native.ABI_VERSION == 6 and lib.bnf_abi_version() == 6          # purely additive
  assert int(re.search(r'#define\s+BNF_EXTREMES_WORK_PER_TILE\s+(\d+)', src).group(1)) == _native.EXTREMES_WORK_PER_TILE
  from bayesnf_amd.engine import Engine
  assert callable(getattr(Engine, 'predictive_group_extremes', None))
  assert callable(getattr(inference, 'extreme_summaries', None))
  # an unbound handle is refused with the code bnf_predictive_group_sums gives
  args = (None, None, None, 2, 4, None, None, 1, 1, 0, 0, 0)
  assert lib.bnf_predictive_group_extremes(*args, None, None, None, 0, None, None, None, None, None) == \
      lib.bnf_predictive_group_sums(*args, None, 0, None) != 0


def _frame():
  t = pd.date_range('2020-01-06', periods=4, freq='W-MON')
  return pd.DataFrame({'t': np.repeat(t, 3), 'place': np.tile(['a', 'b', 'c'], 4), 'y': np.arange(12.0)})


def _params(lead):
  return (np.zeros(lead + (3,)), np.zeros(lead))


@pytest.mark.parametrize('cls,lead', [(BayesianNeuralFieldMAP, (1, 4)), (BayesianNeuralFieldVI, (1, 5, 2))])
def test_extremes_refuse_bad_calls_before_any_gpu_work(cls, lead, monkeypatch):
  df = _frame()
  est = cls(feature_cols=['t'], target_col='y', freq='W', width=64, observation_model='NB')
  for call in (est.predict_extremes, est.score_extremes):
    with pytest.raises(ValueError, match='before fit'):
      call(df, 't')

  def no_gpu(*a, **k):
    raise AssertionError('GPU work was reached')
  monkeypatch.setattr(inference, '_ensemble_forecast', no_gpu)
  est.params_ = _params(lead)                      # "fitted": everything below must fail on its arguments alone
  good = np.full(lead, 1.0 / np.prod(lead))
  for call in (est.predict_extremes, est.score_extremes):
    with pytest.raises(ValueError, match='at most 16384'):
      call(df, 't', num_samples=16385)
    for n in (0, -2):
      with pytest.raises(ValueError, match='at least one sample path'):
        call(df, 't', num_samples=n)
    for bad in (np.nan, np.inf, np.where(np.arange(12) == 5, -np.inf, 3.0)):
      with pytest.raises(ValueError, match='finite'):
        call(df, 't', threshold=bad)
    for bad in (np.zeros(11), np.zeros((12, 1)), np.zeros(4)):
      with pytest.raises(ValueError, match='one limit per row'):
        call(df, 't', threshold=bad)
    with pytest.raises(ValueError, match='threshold'):
      call(df, 't', threshold='high')
    for bad, msg in ((good.reshape(-1), 'shape'), (good * 1.001, 'sum to 1'), (-good, '>= 0')):
      with pytest.raises(ValueError, match=msg):
        call(df, 't', weights=bad)
    with pytest.raises(ValueError, match='not among the columns'):
      call(df, 'week')
    with pytest.raises(AssertionError, match='GPU work'):        # a good call passes the checks and reaches the GPU seam
      call(df, 't', threshold=3.0, weights=good, num_samples=5)
    with pytest.raises(AssertionError, match='GPU work'):
      call(df, ['place'], threshold=np.arange(12.0))
  with pytest.raises(ValueError, match='target column'):
    est.score_extremes(df.drop(columns='y'), 't')
  d = df.copy()
  d.loc[3, 'y'] = 2.5
  with pytest.raises(ValueError, match='non-negative integer'):
    est.score_extremes(d, 't')
  d.loc[3, 'y'] = np.nan                            # a NaN target is no error: it reaches the GPU seam
  with pytest.raises(AssertionError, match='GPU work'):
    est.score_extremes(d, 't')
  # the seam's own checks
  groups = inference.csr_from_codes(np.arange(12) // 3, 4)
  seam = lambda *a, **k: inference.extreme_summaries(np.zeros((12, 1)), 'NB', est.params_, None, *a, **k)
  with pytest.raises(ValueError, match='at most 16384'):
    seam(16385, 0, len(lead), groups)
  with pytest.raises(ValueError, match='at least one sample path'):
    seam(0, 0, len(lead), groups)
  big = inference.csr_from_codes(np.arange(1 << 15), 1 << 15)
  with pytest.raises(ValueError, match='held whole'):
    inference.extreme_summaries(np.zeros((1 << 15, 1)), 'NB', est.params_, None, 16384, 0, len(lead), big)
  with pytest.raises(ValueError, match=r'\[0, 1\]'):
    seam(10, 0, len(lead), groups, quantiles=(0.5, 1.5))
  with pytest.raises(ValueError, match='finite'):
    seam(10, 0, len(lead), groups, threshold=np.full(12, np.nan))
  with pytest.raises(ValueError, match='one limit per row'):
    seam(10, 0, len(lead), groups, threshold=np.zeros(3))
  with pytest.raises(ValueError, match='one value per group'):
    seam(10, 0, len(lead), groups, observed_max=np.zeros(3))
  with pytest.raises(ValueError, match='needs a threshold'):
    seam(10, 0, len(lead), groups, observed_count=np.zeros(4))


def test_observed_peaks_follow_pandas_and_skip_groups_with_a_nan_target(monkeypatch):
  df = _frame()
  df['y'] = [3.0, 7.0, 7.0, 0.0, 0.0, 0.0, 5.0, np.nan, 9.0, 2.0, 8.0, 1.0]
  thr = np.asarray([2.0, 7.0, 6.5, 0.0, -1.0, 0.0, 1.0, 1.0, 1.0, 2.0, 2.0, 2.0])
  seen = {}

  def fake(features, observation_model, params, model_args, num_samples, seed, ensemble_dims, groups, threshold=None,
           observed_max=None, observed_count=None, quantiles=(), compute_dtype=None):
    seen.update(threshold=threshold, observed_max=observed_max, observed_count=observed_count, num_samples=num_samples)
    G, R = len(groups[0]) - 1, len(features)
    out = dict(max_mean=np.zeros(G), max_quantiles=np.zeros((len(quantiles), G)), peak_probability=np.arange(R) / 100.0)
    if observed_max is not None:
      out.update(max_pit=np.zeros((2, G)), max_crps=np.where(np.isnan(observed_max), np.nan, 2.0))
    if threshold is not None:
      out.update(count_mean=np.zeros(G), count_quantiles=np.zeros((len(quantiles), G)), exceed_any=np.full(G, 0.25),
                 exceed_probability=np.zeros(R))
    if observed_count is not None:
      out.update(count_pit=np.zeros((2, G)), count_crps=np.where(np.isnan(observed_count), np.nan, 1.0))
    return out
  monkeypatch.setattr(inference, 'extreme_summaries', fake)
  est = BayesianNeuralFieldMAP(feature_cols=['t'], target_col='y', freq='W', width=64, observation_model='NORMAL')
  est.params_ = object()
  res = est.score_extremes(df, 't', threshold=thr, num_samples=7, seed=1)
  by = df.assign(above=(df['y'] > thr).astype(float)).groupby('t')
  want_max = by['y'].max().where(by['y'].count() == 3).to_numpy()              # NaN unless all three rows are there
  want_count = by['above'].sum().where(by['y'].count() == 3).to_numpy()
  assert np.array_equal(res['observed_max'], want_max, equal_nan=True) and np.isnan(want_max).tolist() == [False, False, True, False]
  assert np.array_equal(res['observed_count'], want_count, equal_nan=True) and want_count[:2].tolist() == [2.0, 1.0]
  assert res['observed_peak_row'].tolist() == [1, 3, -1, 10]                   # the FIRST row of the ties 7, 7 and 0, 0, 0
  assert np.array_equal(seen['observed_max'], want_max, equal_nan=True) and seen['num_samples'] == 7
  assert np.array_equal(seen['observed_count'], want_count, equal_nan=True) and np.array_equal(seen['threshold'], thr)
  assert np.array_equal(res['peak_row_probability'], [0.01, 0.03, np.nan, 0.10], equal_nan=True)
  hit = np.asarray([1.0, 1.0, np.nan, 1.0])
  assert np.array_equal(res['brier'], (0.25 - hit) ** 2, equal_nan=True)
  assert res['n'] == 3 and res['mean_max_crps'] == 2.0 and res['mean_count_crps'] == 1.0 and res['mean_brier'] == 0.75 ** 2
  assert list(res['keys']) == list(df['t'].unique())
  assert set(res) == {'keys', 'max_mean', 'max_quantiles', 'peak_probability', 'exceed_any', 'exceed_count_mean',
                      'exceed_count_quantiles', 'exceed_probability', 'observed_max', 'observed_peak_row', 'max_crps',
                      'max_pit', 'peak_row_probability', 'n', 'mean_max_crps', 'mean_peak_row_probability',
                      'observed_count', 'count_crps', 'count_pit', 'brier', 'mean_count_crps', 'mean_brier'}
  # no threshold: none of the exceedance entries; a scalar threshold is spread over the rows; rows in any order
  res = est.score_extremes(df, 't')
  assert seen['threshold'] is None and seen['observed_count'] is None
  assert not any(k.startswith(('exceed', 'count', 'brier', 'observed_count', 'mean_count', 'mean_brier')) for k in res)
  pred = est.predict_extremes(df, 't', threshold=4)
  assert np.array_equal(seen['threshold'], np.full(12, 4.0)) and seen['observed_max'] is None
  assert set(pred) == {'keys', 'max_mean', 'max_quantiles', 'peak_probability', 'exceed_any', 'exceed_count_mean',
                       'exceed_count_quantiles', 'exceed_probability'}
  shuffled = df.sample(frac=1.0, random_state=0)
  res = est.score_extremes(shuffled, 'place', threshold=thr[shuffled.index.to_numpy()])
  want = df.groupby('place')['y'].max().where(df.groupby('place')['y'].count() == 4)
  assert np.array_equal(res['observed_max'], want.to_numpy(), equal_nan=True) and res['n'] == 2
  rows = res['observed_peak_row']
  assert rows[1] == -1 and np.array_equal(shuffled['y'].to_numpy()[rows[[0, 2]]], want.to_numpy()[[0, 2]])
  # empty groups and ties on hand-made CSR input
  peak, row, count = spatiotemporal.group_target_extremes([1.0, 4.0, 4.0, 2.0], [0, 0, 3, 3, 4], [0, 1, 2, 3], [0.0, 9.0, 3.0, 2.0])
  assert np.array_equal(peak, [np.nan, 4.0, np.nan, 2.0], equal_nan=True) and row.tolist() == [-1, 1, -1, 3]
  assert np.array_equal(count, [np.nan, 2.0, np.nan, 0.0], equal_nan=True)
