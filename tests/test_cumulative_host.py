"""CPU-only checks of the running totals (include/bnf.h bnf_predictive_group_cumulative): the observed running totals
and crossings on hand-written cases; the naive reference on hand-worked paths; the per-group level and its error texts;
the entry point's declaration and export; the estimators' argument checks, which fire before any GPU work."""
import os
import re

import numpy as np
import pandas as pd
import pytest

from bayesnf_amd import BayesianNeuralFieldMAP, BayesianNeuralFieldVI, _native, inference, spatiotemporal
from tests import cumulative_ref as Cu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'bnf_predictive_group_cumulative'
nan = np.nan


def test_group_target_cumulative():
  #         row  0    1    2    3    4    5    6    7    8    9   10   11
  target = [5.0, 0.0, 9.0, 9.0, 1.0, 9.0, nan, 2.0, 0.0, 0.0, 7.0, 3.0]
  # group 0: rows 3, 0, 2, 1, 5, 4 in that time order -> 9 14 23 23 32 33   group 1: empty
  # group 2: rows 7, 6, 8 (a NaN target at its second step)   group 3: row 9 -> 0   group 4: rows 11, 10 -> 3 10
  off = [0, 6, 6, 9, 10, 12]
  rows = [3, 0, 2, 1, 5, 4, 7, 6, 8, 9, 11, 10]
  level = [14.0, 0.0, 1.0, 0.0, 2.5]                     # strict >: 14 does not cross at 14; 0 is never > 0
  got = spatiotemporal.group_target_cumulative(target, off, rows, level)
  assert np.array_equal(got['running'], [14.0, 23.0, 23.0, 9.0, 33.0, 32.0, nan, 2.0, nan, 0.0, 10.0, 3.0], equal_nan=True)
  assert np.array_equal(got['total'], [33.0, nan, nan, 0.0, 10.0], equal_nan=True)
  assert np.array_equal(got['cross_step'], [2.0, nan, nan, 1.0, 0.0], equal_nan=True)     # never: censored at the size; step 0
  assert got['cross_row'].tolist() == [2, -1, -1, -1, 11] and got['cross_row'].dtype == np.int64
  bare = spatiotemporal.group_target_cumulative(target, off, rows)
  assert set(bare) == {'running', 'total'} and np.array_equal(bare['running'], got['running'], equal_nan=True)
  # a negative level is crossed at once by a zero total; the naive reference on the target as a single "path" agrees
  neg = spatiotemporal.group_target_cumulative(target, off, rows, [-1.0] * 5)
  assert neg['cross_step'].tolist()[3:] == [0.0, 0.0] and neg['cross_row'].tolist()[3:] == [9, 11]
  t = np.asarray(target, dtype=np.float32)[None, :]
  ref = Cu.group_cumulative(t, off, rows, level)
  for g in (0, 3, 4):
    for k in ('total', 'cross_step', 'cross_row'):
      assert got[k][g] == ref[k][0, g], (g, k)
  by_row = np.empty(12, dtype=np.int64)
  by_row[rows] = np.arange(12)
  assert np.array_equal(ref['running'][0, by_row], got['running'], equal_nan=True)
  # the order by a column: the same rows in another time order give another curve
  df = pd.DataFrame({'g': ['a'] * 3 + ['b'] * 2, 'when': [2, 0, 1, 1, 0], 'y': [1.0, 10.0, 100.0, 5.0, 7.0]})
  keys, o, r = spatiotemporal.group_rows_ordered(df, 'g', 'when')
  res = spatiotemporal.group_target_cumulative(df['y'].to_numpy(), o, r, [10.5, 7.0])
  assert list(keys) == ['a', 'b'] and r.tolist() == [1, 2, 0, 4, 3]
  assert res['running'].tolist() == [111.0, 10.0, 110.0, 12.0, 7.0]
  assert res['cross_step'].tolist() == [1.0, 1.0] and res['cross_row'].tolist() == [2, 3]


def test_reference_on_hand_worked_paths():
  """The naive reference itself: entries of seg_rows outside the table carry the run and are not steps; a NaN draw counts
  as a step and makes the rest NaN; censoring; an empty group; above_count against cross_count."""
  x = np.asarray([[1.0, 2.0, 3.0, -4.0, 5.0, nan],
                  [0.0, 0.0, 9.0, -9.0, 1.0, 1.0]], dtype=np.float32)
  off = [0, 5, 5, 8]
  rows = [-1, 2, 6, 3, 0, 1, 5, 4]                      # group 0: (skip) 3 (skip) -4 1|0 ; group 2: rows 1, 5, 4
  ref = Cu.group_cumulative(x, off, rows, [-0.5, 0.0, 5.5])
  assert ref['running'].tolist()[0][:5] == [0.0, 3.0, 3.0, -1.0, 0.0] and ref['steps'].tolist() == [0, 1, 1, 2, 3, 1, 2, 3]
  assert ref['running'].tolist()[1][:5] == [0.0, 9.0, 9.0, 0.0, 0.0]
  assert np.array_equal(ref['running'][0, 5:], [2.0, nan, nan], equal_nan=True) and ref['running'][1, 5:].tolist() == [0.0, 1.0, 2.0]
  assert np.array_equal(ref['total'], [[0.0, 0.0, nan], [0.0, 0.0, 2.0]], equal_nan=True)
  assert ref['cross_step'].tolist() == [[0.0, 0.0, 3.0], [0.0, 0.0, 3.0]]        # group 2: never (NaN is not above), censored
  assert ref['cross_row'].tolist() == [[2, -1, -1], [2, -1, -1]]
  assert ref['cross_count'].tolist() == [0, 0, 2, 0, 0, 0]
  assert ref['above_count'].tolist() == [2, 0, 2, 1, 0, 0]                       # path 0 comes back under -0.5 at row 3
  own = Cu.crossings_from_running(ref['running'], off, rows, 6, [-0.5, 0.0, 5.5])
  for k in own:
    assert np.array_equal(own[k], ref[k]), k
  b = Cu.normal_bound(x, off, rows)
  assert b[1].tolist()[:5] == [0.0, 9 * 2.0 ** -52, 9 * 2.0 ** -52, 2 * 18 * 2.0 ** -52, 3 * 18 * 2.0 ** -52]


def test_entry_point_declared_listed_and_exported():
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'bnf.h')).read(), flags=re.S)
  lib = _native.load()
  assert re.search(r'\bint\s+' + NAME + r'\s*\(', src), f'{NAME} is not declared in include/bnf.h'
  assert NAME in _native.EXPORTS
  fn = getattr(lib, NAME)
  assert fn.argtypes is not None and len(fn.argtypes) == 20
  assert _native.ABI_VERSION == 6 and lib.bnf_abi_version() == 6          # purely additive
  from bayesnf_amd.engine import Engine
  assert callable(getattr(Engine, 'predictive_group_cumulative', None))
  assert callable(getattr(inference, 'cumulative_summaries', None))
  # an unbound handle is refused with the code bnf_predictive_group_sums gives
  args = (None, None, None, 2, 4, None, None, 1, 1, 0, 0, 0)
  assert fn(*args, None, None, None, None, None, None, None, None) == lib.bnf_predictive_group_sums(*args, None, 0, None) != 0


def _frame():
  t = pd.date_range('2020-01-06', periods=4, freq='W-MON')
  return pd.DataFrame({'t': np.repeat(t, 3), 'place': np.tile(['a', 'b', 'c'], 4), 'y': np.arange(12.0),
                       'cap': np.tile([10.0, -2.0, 30.0], 4)})


def _params(lead):
  return (np.zeros(lead + (3,)), np.zeros(lead))


def test_group_level_and_its_texts():
  df = _frame()
  keys, off, rows = spatiotemporal.group_rows_ordered(df, 'place', 't')
  level = BayesianNeuralFieldMAP._group_level
  assert level('f', df, None, off, rows) is None
  for given in (4.5, np.float32(4.5), np.full(12, 4.5)):
    got = level('f', df, given, off, rows)
    assert got.dtype == np.float64 and got.tolist() == [4.5, 4.5, 4.5]
  assert level('f', df, 'cap', off, rows).tolist() == [10.0, -2.0, 30.0]               # any sign
  assert level('f', df, np.tile([1.0, 2.0, 3.0], 4), off, rows).tolist() == [1.0, 2.0, 3.0]
  with pytest.raises(ValueError, match='f: level must be constant within every group'):
    level('f', df, np.arange(12.0), off, rows)
  with pytest.raises(ValueError, match="f: level: 'limit' is not among the columns of the table"):
    level('f', df, 'limit', off, rows)
  for bad in (np.nan, -np.inf, np.where(np.arange(12) == 5, np.inf, 3.0)):
    with pytest.raises(ValueError, match='f: level must be finite'):
      level('f', df, bad, off, rows)
  for bad in (np.zeros(11), np.zeros((12, 1)), np.zeros(3)):
    with pytest.raises(ValueError, match=r'f: level must be a scalar or hold one value per row \(12,\)'):
      level('f', df, bad, off, rows)
  with pytest.raises(ValueError, match='f: level must be a number, a column of the table or one number per row'):
    level('f', df, [object()] * 12, off, rows)
  # the texts of the divisor `per` are its own
  with pytest.raises(ValueError, match='f: per must be constant within every group'):
    BayesianNeuralFieldMAP._per_group('f', df, np.arange(1.0, 13.0), off, rows)


@pytest.mark.parametrize('cls,lead', [(BayesianNeuralFieldMAP, (1, 4)), (BayesianNeuralFieldVI, (1, 5, 2))])
def test_cumulative_refuses_bad_calls_before_any_gpu_work(cls, lead, monkeypatch):
  df = _frame()
  est = cls(feature_cols=['t'], target_col='y', freq='W', width=64, observation_model='NB')
  for call in (est.predict_cumulative, est.score_cumulative):
    with pytest.raises(ValueError, match='before fit'):
      call(df, 'place', 3.0)

  def no_gpu(*a, **k):
    raise AssertionError('GPU work was reached')
  monkeypatch.setattr(inference, '_ensemble_forecast', no_gpu)
  est.params_ = _params(lead)                      # "fitted": everything below must fail on its arguments alone
  good = np.full(lead, 1.0 / np.prod(lead))
  for call in (est.predict_cumulative, est.score_cumulative):
    with pytest.raises(ValueError, match='running totals are summarised from at most 16384'):
      call(df, 'place', 3.0, num_samples=16385)
    for n in (0, -2):
      with pytest.raises(ValueError, match='at least one sample path'):
        call(df, 'place', 3.0, num_samples=n)
    for bad in (np.nan, np.inf):
      with pytest.raises(ValueError, match='level must be finite'):
        call(df, 'place', bad)
    with pytest.raises(ValueError, match='one value per row'):
      call(df, 'place', np.zeros(3))
    with pytest.raises(ValueError, match='constant within every group'):
      call(df, 'place', np.arange(12.0))
    with pytest.raises(ValueError, match="level: 'high' is not among the columns"):
      call(df, 'place', 'high')
    for bad, msg in ((good.reshape(-1), 'shape'), (good * 1.001, 'sum to 1'), (-good, '>= 0')):
      with pytest.raises(ValueError, match=msg):
        call(df, 'place', 3.0, weights=bad)
    with pytest.raises(ValueError, match='not among the columns'):
      call(df, 'week', 3.0)
    with pytest.raises(ValueError, match='order_by'):
      call(df, 'place', 3.0, order_by='week')
    with pytest.raises(ValueError, match=r'\[0, 1\]'):
      call(df, 'place', 3.0, quantiles=(0.5, 1.5))
    for kw in (dict(level=3.0, weights=good, num_samples=5), dict(level='cap', order_by='y'), dict(), dict(curve=False)):
      with pytest.raises(AssertionError, match='GPU work'):      # a good call passes the checks and reaches the GPU seam
        call(df, ['place'], **kw)
  with pytest.raises(ValueError, match='target column'):
    est.score_cumulative(df.drop(columns='y'), 'place', 3.0)
  d = df.copy()
  d.loc[3, 'y'] = 2.5
  with pytest.raises(ValueError, match='non-negative integer'):
    est.score_cumulative(d, 'place', 3.0)
  d.loc[3, 'y'] = np.nan                            # a NaN target is no error: it reaches the GPU seam
  with pytest.raises(AssertionError, match='GPU work'):
    est.score_cumulative(d, 'place', 3.0)
  # the cell caps: S x G on a table of 2^15 singleton groups, and S x R of curve=True on one group of 2^15 rows
  wide = pd.DataFrame({'t': pd.Timestamp('2020-01-06'), 'place': np.arange(1 << 15), 'one': 0, 'y': 0.0})
  with pytest.raises(ValueError, match='groups: the totals matrix is held whole'):
    est.predict_cumulative(wide, 'place', 3.0, num_samples=16384, curve=False)
  with pytest.raises(ValueError, match='rows: the running totals are held whole'):
    est.predict_cumulative(wide, 'one', 3.0, num_samples=16384)
  with pytest.raises(AssertionError, match='GPU work'):
    est.predict_cumulative(wide, 'one', 3.0, num_samples=16384, curve=False)
  # the seam's own checks
  groups = inference.csr_from_codes(np.arange(12) // 3, 4)
  seam = lambda *a, **k: inference.cumulative_summaries(np.zeros((12, 1)), 'NB', est.params_, None, *a, **k)
  with pytest.raises(ValueError, match='running totals are summarised from at most 16384'):
    seam(16385, 0, len(lead), groups)
  with pytest.raises(ValueError, match='at least one sample path'):
    seam(0, 0, len(lead), groups)
  big = inference.csr_from_codes(np.arange(1 << 15), 1 << 15)
  with pytest.raises(ValueError, match='totals matrix is held whole'):
    inference.cumulative_summaries(np.zeros((1 << 15, 1)), 'NB', est.params_, None, 16384, 0, len(lead), big, curve=False)
  one = inference.csr_from_codes(np.zeros(1 << 15, dtype=np.int64), 1)
  with pytest.raises(ValueError, match='running totals are held whole'):
    inference.cumulative_summaries(np.zeros((1 << 15, 1)), 'NB', est.params_, None, 16384, 0, len(lead), one)
  with pytest.raises(ValueError, match=r'\[0, 1\]'):
    seam(10, 0, len(lead), groups, quantiles=(0.5, 1.5))
  for bad in (np.full(4, np.nan), np.asarray([0.0, 1.0, np.inf, 2.0])):
    with pytest.raises(ValueError, match='level must be finite'):
      seam(10, 0, len(lead), groups, level=bad)
  with pytest.raises(ValueError, match='one level per group'):
    seam(10, 0, len(lead), groups, level=np.zeros(12))
  with pytest.raises(ValueError, match='one value per group'):
    seam(10, 0, len(lead), groups, observed_total=np.zeros(3))
  with pytest.raises(ValueError, match='one value per row'):
    seam(10, 0, len(lead), groups, observed_running=np.zeros(4))
  with pytest.raises(ValueError, match='needs a level'):
    seam(10, 0, len(lead), groups, observed_cross_step=np.zeros(4))
  with pytest.raises(ValueError, match='sum to 1'):
    seam(10, 0, len(lead), groups, weights=good * 2)
  with pytest.raises(AssertionError, match='GPU work'):
    seam(10, 0, len(lead), groups, level=np.zeros(4), observed_total=np.zeros(4), observed_running=np.zeros(12))


def test_score_cumulative_assembles_observed_values_and_crossing_row_probability(monkeypatch):
  df = _frame()                                     # 4 weeks x 3 places, rows in week order
  df['y'] = [3.0, 0.0, 9.0, 7.0, 0.0, np.nan, 7.0, 0.0, 1.0, 0.0, 0.0, 8.0]
  df = df.iloc[::-1].reset_index(drop=True)         # the table in REVERSE time order: the ordering must undo it
  seen = {}

  def fake(features, observation_model, params, model_args, num_samples, seed, ensemble_dims, groups, level=None,
           curve=True, observed_total=None, observed_running=None, observed_cross_step=None, quantiles=(),
           compute_dtype=None):
    seen.update(groups=groups, level=level, curve=curve, total=observed_total, running=observed_running,
                step=observed_cross_step)
    G, R, Q = len(groups[0]) - 1, len(features), len(quantiles)
    out = {}
    for name, n, obs in (('total', G, observed_total), ('cross_step', G, observed_cross_step), ('running', R, observed_running)):
      if (name == 'cross_step' and level is None) or (name == 'running' and not curve):
        continue
      out[f'{name}_mean'], out[f'{name}_quantiles'] = np.zeros(n), np.zeros((Q, n))
      if obs is not None:
        out[f'{name}_pit'], out[f'{name}_crps'] = np.zeros((2, n)), np.where(np.isnan(obs), np.nan, 2.0)
    if level is not None:
      out.update(crossing_probability=np.arange(R) / 100.0, above_probability=np.zeros(R), never=np.full(G, 0.5))
    return out
  monkeypatch.setattr(inference, 'cumulative_summaries', fake)
  est = BayesianNeuralFieldMAP(feature_cols=['t'], target_col='y', freq='W', width=64, observation_model='NORMAL')
  est.params_ = object()
  res = est.score_cumulative(df, 'place', df['cap'].to_numpy(), num_samples=7, seed=1)
  off, rows = seen['groups']
  t = df['t'].to_numpy()
  for g in range(3):
    assert np.all(np.diff(t[rows[off[g]:off[g + 1]]]) > np.timedelta64(0))      # time order inside every group
  # place a (level 10): 3 10 17 17 -> crosses at step 2 ; place b (level -2): 0 -> step 0 ; place c: 9 nan: not scored
  assert seen['level'].tolist() == [10.0, -2.0, 30.0] and seen['curve'] is True
  assert np.array_equal(res['observed_total'], [17.0, 0.0, np.nan], equal_nan=True)
  assert np.array_equal(res['observed_crossing_step'], [2.0, 0.0, np.nan], equal_nan=True)
  row = lambda place, week: int(np.flatnonzero((df['place'] == place) & (df['t'] == np.sort(df['t'].unique())[week]))[0])
  assert res['observed_crossing_row'].tolist() == [row('a', 2), row('b', 0), -1]
  assert np.array_equal(res['crossing_row_probability'], [row('a', 2) / 100.0, row('b', 0) / 100.0, np.nan], equal_nan=True)
  want_running = np.empty(12)
  for place, run in (('a', [3.0, 10.0, 17.0, 17.0]), ('b', [0.0] * 4), ('c', [9.0, np.nan, np.nan, np.nan])):
    for week, v in enumerate(run):
      want_running[row(place, week)] = v
  assert np.array_equal(res['observed_running'], want_running, equal_nan=True)
  assert np.array_equal(seen['running'], want_running, equal_nan=True) and np.array_equal(seen['total'], res['observed_total'], equal_nan=True)
  assert res['n'] == 2 and res['mean_total_crps'] == 2.0 and res['mean_running_crps'] == 2.0
  assert res['mean_crossing_row_probability'] == (row('a', 2) / 100.0 + row('b', 0) / 100.0) / 2
  assert set(res) == {'keys', 'n', 'total_mean', 'total_quantiles', 'observed_total', 'total_crps', 'total_pit', 'mean_total_crps',
                      'running_mean', 'running_quantiles', 'observed_running', 'running_crps', 'running_pit', 'mean_running_crps',
                      'crossing_step_mean', 'crossing_step_quantiles', 'observed_crossing_step', 'crossing_step_crps',
                      'crossing_step_pit', 'mean_crossing_step_crps', 'observed_crossing_row', 'crossing_row_probability',
                      'mean_crossing_row_probability', 'crossing_probability', 'above_probability', 'never'}
  # a path that never crossed is scored by 'never'
  res = est.score_cumulative(df, 'place', 100.0, num_samples=7, seed=1)
  assert res['observed_crossing_row'].tolist() == [-1, -1, -1] and res['observed_crossing_step'].tolist()[:2] == [4.0, 4.0]
  assert np.array_equal(res['crossing_row_probability'], [0.5, 0.5, np.nan], equal_nan=True)
  # without a level and without the curve
  res = est.score_cumulative(df, 'place', curve=False, num_samples=7)
  assert set(res) == {'keys', 'n', 'total_mean', 'total_quantiles', 'observed_total', 'total_crps', 'total_pit', 'mean_total_crps'}
  assert seen['level'] is None and seen['running'] is None and seen['step'] is None and seen['curve'] is False
  yy = np.nan_to_num(df['y'].to_numpy(), nan=99.0)
  pred = est.predict_cumulative(df.assign(y=yy), 'place', 2.0, order_by='y')      # another ordering column
  assert seen['total'] is None and pred['running_quantiles'].shape == (1, 12) and pred['total_quantiles'].shape == (1, 3)
  assert set(pred) == {'keys', 'total_mean', 'total_quantiles', 'running_mean', 'running_quantiles', 'crossing_step_mean',
                       'crossing_step_quantiles', 'crossing_probability', 'above_probability', 'never'}
  off, rows = seen['groups']
  for g in range(3):
    assert np.all(np.diff(yy[rows[off[g]:off[g + 1]]]) >= 0)
  with pytest.raises(ValueError, match='missing values'):
    est.predict_cumulative(df, 'place', 2.0, order_by='y')
