"""CPU-only checks of the moving-window totals (include/bnf.h bnf_predictive_group_windows): the observed window totals
on hand-written cases; the naive reference of tests/windows_ref.py on hand-worked paths and its own invariants; the
window length, the per-group threshold and their error texts; the entry point's declaration and export; the estimators'
argument checks, which fire before any GPU work."""
import os
import re

import numpy as np
import pandas as pd
import pytest

from bayesnf_amd import BayesianNeuralFieldMAP, BayesianNeuralFieldVI, _native, inference, spatiotemporal
from tests import windows_ref as Wi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'bnf_predictive_group_windows'
nan = np.nan


def test_group_target_windows():
  #         row  0    1    2    3    4    5    6    7    8    9   10   11   12
  target = [5.0, 0.0, 9.0, 9.0, 1.0, 9.0, nan, 2.0, 0.0, 0.0, 7.0, 3.0, 4.0]
  # group 0: rows 3, 0, 2, 1, 5, 4 in that time order -> 9 5 9 0 9 1, windows of 2: 14 14 9 9 10   group 1: empty
  # group 2: rows 6, 7, 8, 12 -> nan 2 0 4: the NaN target lies in ONE full-length window (the one ending at row 7)
  # group 3: row 9 alone, shorter than the window: its total   group 4: rows 11, 10 -> 3 7: one window, 10
  off = [0, 6, 6, 10, 11, 13]
  rows = [3, 0, 2, 1, 5, 4, 6, 7, 8, 12, 9, 11, 10]
  thr = [9.5, 0.0, 0.0, 0.0, 9.0]                         # strict >: the total 0 of group 3 is not > 0
  got = spatiotemporal.group_target_windows(target, off, rows, 2, thr)
  assert np.array_equal(got['window'], [14.0, 9.0, 14.0, nan, 10.0, 9.0, nan, nan, 2.0, 0.0, 10.0, nan, 4.0], equal_nan=True)
  assert np.array_equal(got['peak'], [14.0, nan, nan, 0.0, 10.0], equal_nan=True)
  assert got['peak_row'].tolist() == [0, -1, -1, 9, 10] and got['peak_row'].dtype == np.int64    # 14 twice: the earliest
  assert np.array_equal(got['count'], [3.0, nan, nan, 0.0, 1.0], equal_nan=True)
  bare = spatiotemporal.group_target_windows(target, off, rows, 2)
  assert set(bare) == {'window', 'peak', 'peak_row'} and np.array_equal(bare['window'], got['window'], equal_nan=True)
  # a window of 3: group 4 (2 rows) is shorter than it -- one candidate, the whole group, at its last row
  w3 = spatiotemporal.group_target_windows(target, off, rows, 3, thr)
  assert np.array_equal(w3['window'], [nan, 14.0, 23.0, nan, 10.0, 18.0, nan, nan, nan, 0.0, 10.0, nan, 6.0], equal_nan=True)
  assert np.array_equal(w3['peak'], [23.0, nan, nan, 0.0, 10.0], equal_nan=True) and w3['peak_row'].tolist() == [2, -1, -1, 9, 10]
  # window 1: the target itself; a window as long as the table: the totals
  w1 = spatiotemporal.group_target_windows(target, off, rows, 1)
  assert np.array_equal(w1['window'], target, equal_nan=True) and w1['peak_row'].tolist() == [3, -1, -1, 9, 10]   # 9 first at row 3
  tot = spatiotemporal.group_target_windows(target, off, rows, 13)
  assert np.array_equal(tot['peak'], [33.0, nan, nan, 0.0, 10.0], equal_nan=True) and tot['peak_row'].tolist() == [4, -1, -1, 9, 10]
  assert np.array_equal(tot['peak'], spatiotemporal.group_target_cumulative(target, off, rows)['total'], equal_nan=True)
  # the naive reference on the target as a single "path" agrees in the groups that are scored
  t = np.asarray(target, dtype=np.float32)[None, :]
  for w, res in ((2, got), (3, w3)):
    ref = Wi.group_windows(t, off, rows, w, thr)
    for g in (0, 3, 4):
      for k in ('peak', 'peak_row', 'count'):
        assert res[k][g] == ref[k][0, g], (w, g, k)
    by_row = np.empty(13, dtype=np.int64)
    by_row[rows] = np.arange(13)
    full = np.where(ref['candidate'], ref['window'][0], nan)[by_row]
    assert np.array_equal(full, res['window'], equal_nan=True), w
    assert np.array_equal(inference.window_candidates(off, rows, 13, w), ref['candidate'])
  for bad in (0, 1.5, True):
    with pytest.raises(ValueError, match='window'):
      spatiotemporal.group_target_windows(target, off, rows, bad)


def test_reference_on_hand_worked_paths():
  """The naive reference itself: entries of seg_rows outside the table occupy a slot, add nothing and are no candidates; a
  NaN draw makes exactly the windows that hold it NaN; a group shorter than the window; an empty group; ties."""
  x = np.asarray([[1.0, 2.0, 3.0, -4.0, 5.0, nan, 7.0],
                  [0.0, 0.0, 9.0, -9.0, 1.0, 1.0, 1.0]], dtype=np.float32)
  off = [0, 5, 5, 9]
  rows = [-1, 2, 7, 3, 0, 1, 5, 4, 6]                    # group 0: (skip) 3 (skip) -4 1|0 ; group 2: rows 1, 5, 4, 6
  ref = Wi.group_windows(x, off, rows, 2, [-0.5, 0.0, 5.5])
  assert ref['candidate'].tolist() == [False, True, False, True, True, False, True, True, True]
  assert ref['window'][0].tolist()[:5] == [0.0, 3.0, 3.0, -4.0, -3.0]         # the slot of row 7 holds nothing
  assert ref['window'][1].tolist()[:5] == [0.0, 9.0, 9.0, -9.0, -9.0]
  assert np.array_equal(ref['window'][0, 5:], [2.0, nan, nan, 12.0], equal_nan=True)   # finite again 2 positions later
  assert ref['window'][1, 5:].tolist() == [0.0, 1.0, 2.0, 2.0]
  assert ref['peak'].tolist()[0][0] == 3.0 and ref['peak_row'].tolist() == [[2, -1, 6], [2, -1, 4]]   # 2 twice: the earliest
  assert np.array_equal(ref['peak'], [[3.0, nan, 12.0], [9.0, nan, 2.0]], equal_nan=True)
  assert ref['count'].tolist() == [[1.0, 0.0, 1.0], [1.0, 0.0, 0.0]]
  assert ref['peak_count'].tolist() == [0, 0, 2, 0, 1, 0, 1] and ref['exceed_count'].tolist() == [0, 0, 2, 0, 0, 0, 1]
  own = Wi.from_windows(ref['window'], off, rows, 7, 2, [-0.5, 0.0, 5.5])
  for k in own:
    assert np.array_equal(own[k], ref[k], equal_nan=True), k
  # a window longer than both groups: one candidate each, the group's last position when it takes part
  long = Wi.group_windows(x, off, rows, 9)
  assert long['candidate'].tolist() == [False] * 4 + [True] + [False] * 3 + [True]
  assert np.array_equal(long['peak'], [[0.0, nan, nan], [0.0, nan, 3.0]], equal_nan=True)
  # ... and none when that position takes no part
  none = Wi.group_windows(x, [0, 3], [1, 2, -1], 5, [0.0])
  assert np.isnan(none['peak']).all() and (none['peak_row'] == -1).all() and (none['count'] == 0).all()
  assert not Wi.undecided(ref, np.zeros_like(ref['window']), off, [-0.5, 0.0, 5.5]).any()
  und = Wi.undecided(ref, np.full_like(ref['window'], 0.6), off, [-0.5, 0.0, 5.5])
  assert und.tolist() == [[False, False, False], [False, False, True]]         # path 1, group 2: 2 and 2 tie; 5.5 far


@pytest.mark.parametrize('seed', [0, 1])
def test_reference_invariants(seed):
  """w = 1 reproduces x; w >= the group's size reproduces the last value of np.cumsum (and every clipped window the
  running total); any w: the window is the difference of two running totals up to rounding."""
  rng = np.random.default_rng(seed)
  S, R = 3, 60
  x = rng.standard_normal((S, R)).astype(np.float32) * 10
  sizes = [17, 0, 1, 30, 12]
  off = np.concatenate([[0], np.cumsum(sizes)])
  rows = rng.permutation(R)
  one = Wi.group_windows(x, off, rows, 1)
  assert np.array_equal(one['window'], x[:, rows].astype(np.float64)) and one['candidate'].all()
  for w in (30, 31, 1000):
    big = Wi.group_windows(x, off, rows, w)
    for g, n in enumerate(sizes):
      a, b = off[g], off[g + 1]
      if n == 0:
        assert np.isnan(big['peak'][:, g]).all() and (big['peak_row'][:, g] == -1).all()
        continue
      run = np.cumsum(x[:, rows[a:b]].astype(np.float64), axis=1)
      assert np.allclose(big['window'][:, a:b], run, rtol=0, atol=1e-12)
      assert np.allclose(big['peak'][:, g], run[:, -1], rtol=0, atol=1e-12) and np.all(big['peak_row'][:, g] == rows[b - 1])
      assert big['candidate'][a:b].tolist() == [False] * (n - 1) + [True]
  w = 5
  mid = Wi.group_windows(x, off, rows, w)
  for g, n in enumerate(sizes):
    a, b = off[g], off[g + 1]
    run = np.concatenate([np.zeros((S, w)), np.cumsum(x[:, rows[a:b]].astype(np.float64), axis=1)], axis=1)
    assert np.allclose(mid['window'][:, a:b], run[:, w:] - run[:, :n], rtol=0, atol=1e-11)
    assert mid['candidate'][a:b].tolist() == [i + 1 >= min(w, n) for i in range(n)]


def test_entry_point_declared_listed_and_exported():
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'bnf.h')).read(), flags=re.S)
  lib = _native.load()
  assert re.search(r'\bint\s+' + NAME + r'\s*\(', src), f'{NAME} is not declared in include/bnf.h'
  assert NAME in _native.EXPORTS
  fn = getattr(lib, NAME)
  assert fn.argtypes is not None and len(fn.argtypes) == 21
  assert _native.ABI_VERSION == 6 and lib.bnf_abi_version() == 6          # purely additive
  from bayesnf_amd.engine import Engine
  assert callable(getattr(Engine, 'predictive_group_windows', None))
  assert callable(getattr(inference, 'window_summaries', None))
  # an unbound handle is refused with the code bnf_predictive_group_sums gives
  args = (None, None, None, 2, 4, None, None, 1, 1, 0, 0, 0)
  assert fn(*args, None, 7, None, None, None, None, None, None, None) == lib.bnf_predictive_group_sums(*args, None, 0, None) != 0
  # the contract is in the header, above the declaration
  text = open(os.path.join(ROOT, 'include', 'bnf.h')).read()
  doc = text[:text.index('int ' + NAME)].rsplit('/*', 1)[1]
  for word in ('WINDOW SUM', 'CANDIDATE', 'PEAK', 'THRESHOLD', 'NaN DRAWS', 'DETERMINISM', 'BNF_ERR_INVALID'):
    assert word in doc, word


def _frame():
  t = pd.date_range('2020-01-06', periods=4, freq='W-MON')
  return pd.DataFrame({'t': np.repeat(t, 3), 'place': np.tile(['a', 'b', 'c'], 4), 'y': np.arange(12.0),
                       'cap': np.tile([10.0, -2.0, 30.0], 4)})


def _params(lead):
  return (np.zeros(lead + (3,)), np.zeros(lead))


def test_window_length_and_threshold_texts():
  assert inference._window_length(1) == 1 and inference._window_length(np.int64(7)) == 7
  assert inference._window_length(2 ** 31 - 1) == 2 ** 31 - 1
  for bad in (1.5, 2.0, True, np.bool_(True), '3', None):
    with pytest.raises(ValueError, match='window must be an integer number of rows'):
      inference._window_length(bad)
  for bad in (0, -3, 2 ** 31):
    with pytest.raises(ValueError, match=rf'window={bad}: 1\.\.2147483647 rows'):
      inference._window_length(bad)
  # the per-group threshold goes through the level's helper under its own name; the level's texts are unchanged
  df = _frame()
  keys, off, rows = spatiotemporal.group_rows_ordered(df, 'place', 't')
  level = BayesianNeuralFieldMAP._group_level
  assert level('f', df, 'cap', off, rows, name='threshold').tolist() == [10.0, -2.0, 30.0]
  with pytest.raises(ValueError, match='f: threshold must be constant within every group'):
    level('f', df, np.arange(12.0), off, rows, name='threshold')
  with pytest.raises(ValueError, match='f: level must be constant within every group'):
    level('f', df, np.arange(12.0), off, rows)
  with pytest.raises(ValueError, match="f: threshold: 'limit' is not among the columns of the table"):
    level('f', df, 'limit', off, rows, name='threshold')
  with pytest.raises(ValueError, match='f: threshold must be finite'):
    level('f', df, np.inf, off, rows, name='threshold')
  assert inference._group_level(None, 3, name='threshold') is None
  with pytest.raises(ValueError, match='threshold must hold one threshold per group'):
    inference._group_level(np.zeros(4), 3, name='threshold')
  with pytest.raises(ValueError, match='level must hold one level per group'):
    inference._group_level(np.zeros(4), 3)
  with pytest.raises(ValueError, match='^level must be finite$'):
    inference._group_level(np.full(3, np.nan), 3)


@pytest.mark.parametrize('cls,lead', [(BayesianNeuralFieldMAP, (1, 4)), (BayesianNeuralFieldVI, (1, 5, 2))])
def test_windows_refuse_bad_calls_before_any_gpu_work(cls, lead, monkeypatch):
  df = _frame()
  est = cls(feature_cols=['t'], target_col='y', freq='W', width=64, observation_model='NB')
  for call in (est.predict_windows, est.score_windows):
    with pytest.raises(ValueError, match='before fit'):
      call(df, 'place', 2)

  def no_gpu(*a, **k):
    raise AssertionError('GPU work was reached')
  monkeypatch.setattr(inference, '_ensemble_forecast', no_gpu)
  est.params_ = _params(lead)                      # "fitted": everything below must fail on its arguments alone
  good = np.full(lead, 1.0 / np.prod(lead))
  for call in (est.predict_windows, est.score_windows):
    what = call.__name__
    with pytest.raises(ValueError, match='window totals are summarised from at most 16384'):
      call(df, 'place', 2, num_samples=16385)
    for n in (0, -2):
      with pytest.raises(ValueError, match='at least one sample path'):
        call(df, 'place', 2, num_samples=n)
    for bad in (1.5, True, '2', None):
      with pytest.raises(ValueError, match=f'{what}: window must be an integer number of rows'):
        call(df, 'place', bad)
    for bad in (0, -1, 2 ** 31):
      with pytest.raises(ValueError, match=rf'{what}: window={bad}: 1\.\.2147483647 rows'):
        call(df, 'place', bad)
    for bad in (np.nan, np.inf):
      with pytest.raises(ValueError, match='threshold must be finite'):
        call(df, 'place', 2, bad)
    with pytest.raises(ValueError, match='one value per row'):
      call(df, 'place', 2, np.zeros(3))
    with pytest.raises(ValueError, match='threshold must be constant within every group'):
      call(df, 'place', 2, np.arange(12.0))
    with pytest.raises(ValueError, match="threshold: 'high' is not among the columns"):
      call(df, 'place', 2, 'high')
    for bad, msg in ((good.reshape(-1), 'shape'), (good * 1.001, 'sum to 1'), (-good, '>= 0')):
      with pytest.raises(ValueError, match=msg):
        call(df, 'place', 2, weights=bad)
    with pytest.raises(ValueError, match='not among the columns'):
      call(df, 'week', 2)
    with pytest.raises(ValueError, match='order_by'):
      call(df, 'place', 2, order_by='week')
    with pytest.raises(ValueError, match=r'\[0, 1\]'):
      call(df, 'place', 2, quantiles=(0.5, 1.5))
    for kw in (dict(window=2, threshold=3.0, weights=good, num_samples=5), dict(window=1, threshold='cap', order_by='y'),
               dict(window=2 ** 31 - 1), dict(window=np.int32(3), curve=False)):
      with pytest.raises(AssertionError, match='GPU work'):      # a good call passes the checks and reaches the GPU seam
        call(df, ['place'], **kw)
  with pytest.raises(ValueError, match='target column'):
    est.score_windows(df.drop(columns='y'), 'place', 2)
  d = df.copy()
  d.loc[3, 'y'] = 2.5
  with pytest.raises(ValueError, match='non-negative integer'):
    est.score_windows(d, 'place', 2)
  d.loc[3, 'y'] = np.nan                            # a NaN target is no error: it reaches the GPU seam
  with pytest.raises(AssertionError, match='GPU work'):
    est.score_windows(d, 'place', 2, 3.0)
  # the cell caps: S x G on a table of 2^15 singleton groups, and S x R of curve=True on one group of 2^15 rows
  wide = pd.DataFrame({'t': pd.Timestamp('2020-01-06'), 'place': np.arange(1 << 15), 'one': 0, 'y': 0.0})
  with pytest.raises(ValueError, match='groups: the peak matrix is held whole'):
    est.predict_windows(wide, 'place', 2, num_samples=16384, curve=False)
  with pytest.raises(ValueError, match='rows: the window totals are held whole'):
    est.predict_windows(wide, 'one', 2, num_samples=16384)
  with pytest.raises(AssertionError, match='GPU work'):
    est.predict_windows(wide, 'one', 2, num_samples=16384, curve=False)
  # the seam's own checks
  groups = inference.csr_from_codes(np.arange(12) // 3, 4)
  seam = lambda *a, **k: inference.window_summaries(np.zeros((12, 1)), 'NB', est.params_, None, *a, **k)
  with pytest.raises(ValueError, match='window totals are summarised from at most 16384'):
    seam(16385, 0, len(lead), groups, 2)
  with pytest.raises(ValueError, match='at least one sample path'):
    seam(0, 0, len(lead), groups, 2)
  for bad in (1.5, True):
    with pytest.raises(ValueError, match='window must be an integer number of rows'):
      seam(10, 0, len(lead), groups, bad)
  with pytest.raises(ValueError, match=r'window=0: 1\.\.2147483647 rows'):
    seam(10, 0, len(lead), groups, 0)
  big = inference.csr_from_codes(np.arange(1 << 15), 1 << 15)
  with pytest.raises(ValueError, match='peak matrix is held whole'):
    inference.window_summaries(np.zeros((1 << 15, 1)), 'NB', est.params_, None, 16384, 0, len(lead), big, 2, curve=False)
  one = inference.csr_from_codes(np.zeros(1 << 15, dtype=np.int64), 1)
  with pytest.raises(ValueError, match='window totals are held whole'):
    inference.window_summaries(np.zeros((1 << 15, 1)), 'NB', est.params_, None, 16384, 0, len(lead), one, 2)
  with pytest.raises(ValueError, match=r'\[0, 1\]'):
    seam(10, 0, len(lead), groups, 2, quantiles=(0.5, 1.5))
  for bad in (np.full(4, np.nan), np.asarray([0.0, 1.0, np.inf, 2.0])):
    with pytest.raises(ValueError, match='threshold must be finite'):
      seam(10, 0, len(lead), groups, 2, threshold=bad)
  with pytest.raises(ValueError, match='one threshold per group'):
    seam(10, 0, len(lead), groups, 2, threshold=np.zeros(12))
  with pytest.raises(ValueError, match='one value per group'):
    seam(10, 0, len(lead), groups, 2, observed_peak=np.zeros(3))
  with pytest.raises(ValueError, match='one value per row'):
    seam(10, 0, len(lead), groups, 2, observed_window=np.zeros(4))
  with pytest.raises(ValueError, match='needs a threshold'):
    seam(10, 0, len(lead), groups, 2, observed_count=np.zeros(4))
  with pytest.raises(ValueError, match='needs curve=True'):
    seam(10, 0, len(lead), groups, 2, curve=False, observed_window=np.zeros(12))
  with pytest.raises(ValueError, match='sum to 1'):
    seam(10, 0, len(lead), groups, 2, weights=good * 2)
  with pytest.raises(AssertionError, match='GPU work'):
    seam(10, 0, len(lead), groups, 2, threshold=np.zeros(4), observed_peak=np.zeros(4), observed_window=np.zeros(12),
         observed_count=np.zeros(4))


def test_score_windows_assembles_observed_values_and_peak_row_probability(monkeypatch):
  df = _frame()                                     # 4 weeks x 3 places, rows in week order
  df['y'] = [3.0, 0.0, 9.0, 7.0, 0.0, np.nan, 7.0, 0.0, 1.0, 0.0, 0.0, 8.0]
  df = df.iloc[::-1].reset_index(drop=True)         # the table in REVERSE time order: the ordering must undo it
  seen = {}

  def fake(features, observation_model, params, model_args, num_samples, seed, ensemble_dims, groups, window,
           threshold=None, curve=True, observed_peak=None, observed_window=None, observed_count=None, quantiles=(),
           compute_dtype=None):
    seen.update(groups=groups, window=window, threshold=threshold, curve=curve, peak=observed_peak, win=observed_window,
                count=observed_count)
    G, R, Q = len(groups[0]) - 1, len(features), len(quantiles)
    out = {'peak_probability': np.arange(R) / 100.0}
    for name, n, obs in (('peak', G, observed_peak), ('count', G, observed_count), ('window', R, observed_window)):
      if (name == 'count' and threshold is None) or (name == 'window' and not curve):
        continue
      out[f'{name}_mean'], out[f'{name}_quantiles'] = np.zeros(n), np.zeros((Q, n))
      if obs is not None:
        out[f'{name}_pit'], out[f'{name}_crps'] = np.zeros((2, n)), np.where(np.isnan(obs), np.nan, 2.0)
    if threshold is not None:
      out.update(exceed_probability=np.zeros(R), any=np.full(G, 0.5))
    return out
  monkeypatch.setattr(inference, 'window_summaries', fake)
  est = BayesianNeuralFieldMAP(feature_cols=['t'], target_col='y', freq='W', width=64, observation_model='NORMAL')
  est.params_ = object()
  res = est.score_windows(df, 'place', 2, df['cap'].to_numpy(), num_samples=7, seed=1)
  off, rows = seen['groups']
  t = df['t'].to_numpy()
  for g in range(3):
    assert np.all(np.diff(t[rows[off[g]:off[g + 1]]]) > np.timedelta64(0))      # time order inside every group
  # place a (threshold 10): 3 7 7 0 -> windows 10 14 7, peak 14 in week 2, one above; place b (-2): 0 0 0, peak 0 in
  # week 1 (the earliest), three above; place c: 9 nan 1 8 -> windows nan nan 9: not scored
  assert seen['threshold'].tolist() == [10.0, -2.0, 30.0] and seen['curve'] is True and seen['window'] == 2
  assert np.array_equal(res['observed_peak'], [14.0, 0.0, np.nan], equal_nan=True)
  assert np.array_equal(res['observed_count'], [1.0, 3.0, np.nan], equal_nan=True)
  row = lambda place, week: int(np.flatnonzero((df['place'] == place) & (df['t'] == np.sort(df['t'].unique())[week]))[0])
  assert res['observed_peak_row'].tolist() == [row('a', 2), row('b', 1), -1]
  assert np.array_equal(res['peak_row_probability'], [row('a', 2) / 100.0, row('b', 1) / 100.0, np.nan], equal_nan=True)
  want = np.empty(12)
  for place, win in (('a', [nan, 10.0, 14.0, 7.0]), ('b', [nan, 0.0, 0.0, 0.0]), ('c', [nan, nan, nan, 9.0])):
    for week, v in enumerate(win):
      want[row(place, week)] = v
  assert np.array_equal(res['observed_window'], want, equal_nan=True) and np.array_equal(seen['win'], want, equal_nan=True)
  assert np.array_equal(seen['peak'], res['observed_peak'], equal_nan=True)
  assert res['n'] == 2 and res['mean_peak_crps'] == 2.0 and res['mean_window_crps'] == 2.0 and res['mean_count_crps'] == 2.0
  assert res['mean_peak_row_probability'] == (row('a', 2) / 100.0 + row('b', 1) / 100.0) / 2
  assert set(res) == {'keys', 'n', 'peak_mean', 'peak_quantiles', 'peak_probability', 'observed_peak', 'observed_peak_row',
                      'peak_crps', 'peak_pit', 'mean_peak_crps', 'peak_row_probability', 'mean_peak_row_probability',
                      'window_mean', 'window_quantiles', 'observed_window', 'window_crps', 'window_pit', 'mean_window_crps',
                      'count_mean', 'count_quantiles', 'observed_count', 'count_crps', 'count_pit', 'mean_count_crps',
                      'exceed_probability', 'any'}
  # without a threshold and without the curve
  res = est.score_windows(df, 'place', 3, curve=False, num_samples=7)
  assert set(res) == {'keys', 'n', 'peak_mean', 'peak_quantiles', 'peak_probability', 'observed_peak', 'observed_peak_row',
                      'peak_crps', 'peak_pit', 'mean_peak_crps', 'peak_row_probability', 'mean_peak_row_probability'}
  assert seen['threshold'] is None and seen['win'] is None and seen['count'] is None and seen['curve'] is False
  assert np.array_equal(res['observed_peak'], [17.0, 0.0, np.nan], equal_nan=True)       # 3 7 7 | 7 7 0
  yy = np.nan_to_num(df['y'].to_numpy(), nan=99.0)
  pred = est.predict_windows(df.assign(y=yy), 'place', 2, 2.0, order_by='y')      # another ordering column
  assert seen['peak'] is None and pred['window_quantiles'].shape == (1, 12) and pred['peak_quantiles'].shape == (1, 3)
  assert set(pred) == {'keys', 'peak_mean', 'peak_quantiles', 'peak_probability', 'window_mean', 'window_quantiles',
                       'count_mean', 'count_quantiles', 'exceed_probability', 'any'}
  off, rows = seen['groups']
  for g in range(3):
    assert np.all(np.diff(yy[rows[off[g]:off[g + 1]]]) >= 0)
