"""CPU-only checks of the simultaneous bands (include/bnf.h bnf_sample_depths / bnf_depth_levels / bnf_sample_envelope):
the reference of tests/bands_ref.py on hand-worked paths and against the definitions it restates; `inference.band_need`;
the entry points' declaration and export; the estimators' argument checks, which fire before any GPU work."""
import os
import re

import numpy as np
import pandas as pd
import pytest

from bayesnf_amd import BayesianNeuralFieldMAP, BayesianNeuralFieldVI, _native, inference
from tests import bands_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = np.nan, np.inf


def test_reference_on_hand_worked_paths():
  """Five paths, seven columns, three groups (group 2 is empty, column 6 takes no part):
    column 0  1 2 3 4 5     distinct: depths 0 1 2 1 0
    column 1  0 0 0 1 7     ties: the zeros have 3 <= and 5 >=: depth 2; 1 has 4 <= and 2 >=: 1; 7: 0
    column 2  4 4 4 4 4     all equal: everyone has depth S - 1 = 4
    column 3  -0 +0 -1 1 0  the three zeros tie: 4 <=, 4 >=: depth 3; -1 and 1: 0
    column 4  -inf -inf 0 inf inf   infinities of one sign tie: 2 <= and 5 >=: depth 1; 0: 2
    column 5  1 2 NaN 4 5   a NaN column: -1 for everyone
    column 6  9 8 7 6 5     col_group -1"""
  x = np.asarray([[1, 0, 4, -0.0, -INF, 1, 9],
                  [2, 0, 4, 0.0, -INF, 2, 8],
                  [3, 0, 4, -1, 0, NAN, 7],
                  [4, 1, 4, 1, INF, 4, 6],
                  [5, 7, 4, 0.0, INF, 5, 5]], dtype=np.float64)
  d = B.column_depths(x)
  assert d[:, 0].tolist() == [0, 1, 2, 1, 0]
  assert d[:, 1].tolist() == [2, 2, 2, 1, 0]
  assert d[:, 2].tolist() == [4, 4, 4, 4, 4]
  assert d[:, 3].tolist() == [3, 3, 0, 0, 3]
  assert d[:, 4].tolist() == [1, 1, 2, 1, 1]
  assert d[:, 5].tolist() == [-1, -1, -1, -1, -1]
  cg = np.asarray([0, 0, 0, 0, 1, 1, -1])
  D = B.group_depths(x, cg, 3)
  assert D[:, 0].tolist() == [0, 1, 0, 0, 0] and D[:, 1].tolist() == [-1] * 5 and D[:, 2].tolist() == [B.NONE] * 5
  cg2 = np.asarray([0, 0, 0, 0, 1, -1, 3])               # the NaN column takes no part now; 3 is out of range too
  D = B.group_depths(x, cg2, 3)
  assert D[:, 1].tolist() == [1, 1, 2, 1, 1]
  # levels: need 1 -> the largest depth; need 5 -> the smallest; group 2 is empty
  lev = B.depth_levels(D, [1, 2, 5], k_query=[-3, -1, 0, 1, 2, 5])
  assert lev['level'].tolist() == [[1, 2, -1], [0, 1, -1], [0, 1, -1]]
  assert np.array_equal(lev['achieved'], [[0.2, 0.2, NAN], [1.0, 1.0, NAN], [1.0, 1.0, NAN]], equal_nan=True)
  assert np.array_equal(lev['joint'][:, 0], [1.0, 1.0, 1.0, 0.2, 0.0, 0.0])
  assert np.array_equal(lev['joint'][:, 1], [1.0, 1.0, 1.0, 1.0, 0.2, 0.0]) and np.isnan(lev['joint'][:, 2]).all()
  # the poisoned group: level -1, achieved 1
  pois = B.depth_levels(B.group_depths(x, cg, 3), [1, 5])
  assert pois['level'][:, 1].tolist() == [-1, -1] and pois['achieved'][:, 1].tolist() == [1.0, 1.0]
  # envelopes: band 0 is the range, band 1 the second smallest to the second largest; NaN where there is none
  lo, hi = B.envelope(x, cg, np.asarray([[0, 0, 0], [1, 1, 1], [2, -1, 0], [5, 0, 0]]))
  assert np.array_equal(lo[0], [1, 0, 4, -1, -INF, NAN, NAN], equal_nan=True)
  assert np.array_equal(hi[0], [5, 7, 4, 1, INF, NAN, NAN], equal_nan=True)
  assert np.array_equal(lo[1], [2, 0, 4, 0, -INF, NAN, NAN], equal_nan=True)
  assert np.array_equal(hi[1], [4, 1, 4, 0, INF, NAN, NAN], equal_nan=True)
  assert np.array_equal(lo[2], [3, 0, 4, 0, NAN, NAN, NAN], equal_nan=True) and np.array_equal(lo[2], hi[2], equal_nan=True)
  assert np.isnan(lo[3][:4]).all() and lo[3][4] == -INF
  # observed: y equal to a tied block has its depth; outside the range -1; NaN takes no part
  y = np.asarray([3.0, 0.0, 4.0, NAN, 0.0, 3.0, 0.0])
  assert B.observed_depths(x, cg, 3, y).tolist() == [2, -1, B.NONE]         # the NaN column makes group 1's -1
  assert B.observed_depths(x, cg2, 3, y).tolist() == [2, 2, B.NONE]
  y[0] = 0.5                                                                   # below every sample of column 0
  OD = B.observed_depths(x, cg2, 3, y)
  assert OD.tolist() == [-1, 2, B.NONE]
  y[0] = 1.5                                                                   # between the samples: 1 <=, 4 >=
  OD = B.observed_depths(x, cg2, 3, y)
  assert OD.tolist() == [0, 2, B.NONE]
  pit = B.depth_levels(D, [5], OD=OD)['obs_pit']
  assert np.array_equal(pit, [[0.8, 1.0, NAN], [0.0, 0.8, NAN]], equal_nan=True)
  y[:] = NAN
  assert B.observed_depths(x, cg2, 3, y).tolist() == [B.NONE] * 3


@pytest.mark.parametrize('kind', B.KINDS)
@pytest.mark.parametrize('S,C,G', [(1, 5, 2), (2, 9, 3), (10, 19, 5), (63, 27, 4), (200, 50, 1)])
def test_reference_invariants(kind, S, C, G):
  """inside <=> D >= k by the definition of the band; lower <= upper; coverage >= need / S; levels do not rise with
  coverage and the bands nest; coverage = 1 gives k* = min D; the need-th largest is the largest k with ge(k) >= need."""
  x, cg, y = B.band_case(S, C, G, kind)
  cov = (0.5, 0.7, 0.9, 1.0)
  need = [B.need_of(c, S) for c in cov]
  D = B.group_depths(x, cg, G)
  lev = B.depth_levels(D, need, OD=B.observed_depths(x, cg, G, y))
  lower, upper = B.envelope(x, cg, lev['level'])
  for g in range(G):
    cols = np.flatnonzero(cg == g)
    if cols.size == 0:
      assert np.all(D[:, g] == B.NONE) and np.all(lev['level'][:, g] == -1) and np.isnan(lev['achieved'][:, g]).all()
      continue
    if np.isnan(x[:, cols]).any():
      assert np.all(D[:, g] == -1) and np.all(lev['level'][:, g] == -1) and np.all(lev['achieved'][:, g] == 1.0)
      continue
    assert D[:, g].min() >= 0 and D[:, g].max() <= S - 1
    for k in range(0, (S + 1) // 2 + 1):                  # every band, by the definition
      lo, hi = B.envelope(x, cg, np.full((1, G), k))
      if k <= S - 1:
        assert np.array_equal(B.inside(x, lo[0], hi[0], cols), D[:, g] >= k), (g, k)
    for i, n in enumerate(need):
      k = lev['level'][i, g]
      ge = lambda kk: int((D[:, g] >= kk).sum())
      assert ge(k) >= n and ge(k + 1) < n                  # the largest k with ge(k) >= need
      assert lev['achieved'][i, g] == ge(k) / S >= n / S
      assert np.all(lower[i, cols] <= upper[i, cols])
      if i:
        assert k <= lev['level'][i - 1, g]
        assert np.all(lower[i, cols] <= lower[i - 1, cols]) and np.all(upper[i, cols] >= upper[i - 1, cols])
    assert lev['level'][-1, g] == D[:, g].min() and lev['achieved'][-1, g] == 1.0
  out = np.flatnonzero((cg < 0) | (cg >= G))
  assert np.isnan(lower[:, out]).all() and np.isnan(upper[:, out]).all()
  # the observed curve lies inside band k at every scored column exactly when OD >= k
  OD = B.observed_depths(x, cg, G, y)
  for g in range(G):
    cols = np.flatnonzero((cg == g) & ~np.isnan(y))
    if cols.size == 0:
      assert OD[g] == B.NONE and np.isnan(lev['obs_pit'][:, g]).all()
      continue
    if np.isnan(x[:, np.flatnonzero(cg == g)]).any():
      continue
    for k in range(0, (S + 1) // 2 + 1):
      if k <= S - 1:
        lo, hi = B.envelope(x, cg, np.full((1, G), k))
        assert bool(np.all((y[cols] >= lo[0, cols]) & (y[cols] <= hi[0, cols]))) == bool(OD[g] >= k), (g, k)
    assert lev['obs_pit'][1, g] <= lev['obs_pit'][0, g]


def test_the_pointwise_band_against_the_simultaneous_one_with_and_without_ties():
  """Without ties a column holds exactly S - 2 k samples in band k, so k* <= k_pw = floor((S - need) / 2) and the pointwise
  band holds no more whole paths than the simultaneous one.  With ties a band can hold more than S - 2 k samples: in a
  group that is ONE column of 150 zeros and 50 distinct positive counts (S = 200, need = 180) the zeros have depth 149,
  the i-th smallest positive value depth 50 - i; the 180th largest depth is 20, band 20 holds exactly 180 paths (0.9),
  while band k_pw = 10 holds 190 (0.95): there the simultaneous band lies INSIDE the pointwise one.  ge is monotone, so in
  every cell  level <= k_pw  implies  pointwise_joint_coverage <= coverage  and  level >= k_pw  the reverse."""
  S, need = 200, 180
  x = np.concatenate([np.zeros(150), np.arange(1.0, 51.0)])[:, None]
  out = B.band_summaries(x, np.zeros(1, dtype=np.int32), 1, (0.9,))
  assert (S - need) // 2 == 10 and out['level'][0, 0] == 20
  assert out['coverage'][0, 0] == 0.9 and out['pointwise_joint_coverage'][0, 0] == 0.95
  assert out['lower'][0, 0] == 0.0 and out['upper'][0, 0] == 30.0 and out['pointwise_upper'][0, 0] == 40.0
  for kind, G in (('normal', 4), ('count', 4), ('edge', 3)):
    x, cg, _ = B.band_case(200, 40, G, kind)
    cov = (0.5, 0.8, 0.9, 0.99)
    out = B.band_summaries(x, cg, G, cov)
    k_pw = np.asarray([(200 - B.need_of(c, 200)) // 2 for c in cov])[:, None]
    live = ~np.isnan(out['coverage'])
    below, above = live & (out['level'] <= k_pw), live & (out['level'] >= k_pw)
    assert np.all(out['pointwise_joint_coverage'][below] <= out['coverage'][below])
    assert np.all(out['pointwise_joint_coverage'][above] >= out['coverage'][above])
    if kind == 'normal':
      assert np.array_equal(below, live)
      assert np.any(out['pointwise_joint_coverage'][live] < out['coverage'][live])


def test_band_need():
  assert inference.band_need(0.7, 10) == 7
  assert 0.07 * 100 > 7 and inference.band_need(0.07, 100) == 7          # 7.000000000000001: a plain ceil gives 8
  assert 0.57 * 100 < 57 and inference.band_need(0.57, 100) == 57
  assert inference.band_need(0.9, 1000) == 900
  for S in (1, 2, 10, 1000, 16384):
    assert inference.band_need(1.0, S) == S and inference.band_need(1e-12, S) == 1
    for c in (0.05, 0.5, 0.7, 0.9, 0.95, 0.99):
      assert inference.band_need(c, S) == B.need_of(c, S)
  assert inference.band_need(0.701, 10) == 8 and inference.band_need(0.5, 3) == 2
  for bad in (0.0, -0.1, 1.0000001, NAN, 'wide'):
    with pytest.raises(ValueError, match='coverage'):
      inference.band_need(bad, 10)
  with pytest.raises(ValueError, match='at least one sample path'):
    inference.band_need(0.5, 0)


def test_entry_points_declared_listed_and_exported():
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'bnf.h')).read(), flags=re.S)
  lib = _native.load()
  for name, n_args in (('bnf_sample_depths', 9), ('bnf_depth_levels', 13), ('bnf_sample_envelope', 10)):
    m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)', src)
    assert m, f'{name} is not declared in include/bnf.h'
    assert len(m.group(1).split(',')) == n_args and name in _native.EXPORTS
    fn = getattr(lib, name)
    assert fn.argtypes is not None and len(fn.argtypes) == n_args
  assert _native.ABI_VERSION == 6 and lib.bnf_abi_version() == 6          # purely additive
  macro = lambda name: re.search(r'#define\s+' + name + r'\s+(\S+)', src).group(1).strip()
  assert int(macro('BNF_DEPTH_NONE'), 16) == _native.DEPTH_NONE == B.NONE == 0x7fffffff
  assert int(macro('BNF_BAND_MAX_LEVELS')) == _native.BAND_MAX_LEVELS == B.MAX_LEVELS == 64
  from bayesnf_amd.engine import Engine
  for name in ('sample_depths', 'depth_levels', 'sample_envelope'):
    assert callable(getattr(Engine, name, None)), name
  assert callable(getattr(inference, 'band_summaries', None))
  header = open(os.path.join(ROOT, 'bayesnf_amd', 'csrc', 'Makefile')).read()
  assert 'bnf_bands.h' in re.search(r'^HDR\s*:=(.*)$', header, flags=re.M).group(1)


def test_a_null_handle_is_refused_like_the_summaries_refuse_it():
  lib = _native.load()
  want = lib.bnf_sample_energy_score(None, None, 4, 2, None, None, 0, None)
  message = _native.last_error()
  assert want < 0
  assert lib.bnf_sample_depths(None, None, 4, 2, None, 1, None, None, None) == want and _native.last_error() == message
  assert lib.bnf_depth_levels(None, None, 4, 1, None, 0, None, 0, None, None, None, None, None) == want
  assert _native.last_error() == message
  assert lib.bnf_sample_envelope(None, None, 4, 2, None, None, 1, 1, None, None) == want and _native.last_error() == message


def _frame():
  t = pd.date_range('2020-01-06', periods=4, freq='W-MON')
  return pd.DataFrame({'t': np.repeat(t, 3), 'place': np.tile(['a', 'b', 'c'], 4), 'y': np.arange(12.0)})


def _params(lead):
  return (np.zeros(lead + (3,)), np.zeros(lead))


@pytest.mark.parametrize('cls,lead', [(BayesianNeuralFieldMAP, (1, 4)), (BayesianNeuralFieldVI, (1, 5, 2))])
def test_bands_refuse_bad_calls_before_any_gpu_work(cls, lead, monkeypatch):
  df = _frame()
  est = cls(feature_cols=['t'], target_col='y', freq='W', width=64, observation_model='NB')
  for name in ('predict_bands', 'score_bands'):
    with pytest.raises(ValueError, match=f'^{name} before fit$'):
      getattr(est, name)(df, 'place')

  def no_gpu(*a, **k):
    raise AssertionError('GPU work was reached')
  monkeypatch.setattr(inference, '_ensemble_forecast', no_gpu)
  est.params_ = _params(lead)                      # "fitted": everything below must fail on its arguments alone
  good = np.full(lead, 1.0 / np.prod(lead))
  for name in ('predict_bands', 'score_bands'):
    call = getattr(est, name)
    with pytest.raises(ValueError, match=f"^{name}: of='windows': 'rows' \\(the draws at the rows\\) or 'cumulative' "
                                         r"\(their running totals\)$"):
      call(df, 'place', of='windows')
    with pytest.raises(ValueError, match=f"^{name}: order_by orders a running total: it needs of='cumulative'$"):
      call(df, 'place', order_by='t')
    with pytest.raises(ValueError, match=f"^{name}: of='cumulative' needs group_by: a running total runs along the rows "
                                         'of a group$'):
      call(df, None, of='cumulative')
    with pytest.raises(ValueError, match=f'^{name}: num_samples=16385: the bands are summarised from at most 16384 '
                                         'sample paths$'):
      call(df, 'place', num_samples=16385)
    for n in (0, -2):
      with pytest.raises(ValueError, match=f'^{name}: num_samples={n}: need at least one sample path$'):
        call(df, 'place', num_samples=n)
    for bad in ((0.0,), (0.5, 1.5), (-0.1,), (NAN,)):
      with pytest.raises(ValueError, match=f'^{name}: coverage must lie in \\(0, 1\\]; got '):
        call(df, 'place', coverage=bad)
    with pytest.raises(ValueError, match=f'^{name}: coverage: 1..64 levels; got 0$'):
      call(df, 'place', coverage=())
    with pytest.raises(ValueError, match=f'^{name}: coverage: 1..64 levels; got 65$'):
      call(df, 'place', coverage=tuple(np.linspace(0.1, 0.9, 65)))
    with pytest.raises(ValueError, match=f'^{name}: coverage must be a sequence of numbers in \\(0, 1\\]; got 0.9$'):
      call(df, 'place', coverage=0.9)
    with pytest.raises(ValueError, match='not among the columns'):
      call(df, 'week')
    with pytest.raises(ValueError, match="order_by: 'week' is not among the columns"):
      call(df, 'place', of='cumulative', order_by='week')
    for bad, msg in ((good.reshape(-1), 'shape'), (good * 1.001, 'sum to 1'), (-good, '>= 0')):
      with pytest.raises(ValueError, match=msg):
        call(df, 'place', weights=bad)
    for kw in (dict(group_by='place'), dict(group_by=None), dict(group_by='place', of='cumulative'),
               dict(group_by=['place', 't'], coverage=(0.5, 0.9, 1.0), weights=good, num_samples=5),
               dict(group_by='place', of='cumulative', order_by='y')):
      with pytest.raises(AssertionError, match='GPU work'):        # a good call passes the checks and reaches the GPU seam
        call(df, **kw)
  with pytest.raises(ValueError, match='target column'):
    est.score_bands(df.drop(columns='y'), 'place')
  d = df.copy()
  d.loc[3, 'y'] = 2.5
  with pytest.raises(ValueError, match='non-negative integer'):
    est.score_bands(d, 'place')
  d.loc[3, 'y'] = np.nan                            # a NaN target is no error: it reaches the GPU seam
  for of in ('rows', 'cumulative'):
    with pytest.raises(AssertionError, match='GPU work'):
      est.score_bands(d, 'place', of=of)
  # the whole matrix is held: num_samples * rows <= 2^28
  tall = pd.DataFrame({'t': pd.Timestamp('2020-01-06'), 'place': np.arange(16385) % 7, 'y': 0.0})
  with pytest.raises(ValueError, match=r'^predict_bands: 16384 sample paths x 16385 rows: the sample paths are held whole '
                                       r'on the device, at most 268435456 cells$'):
    est.predict_bands(tall, 'place', num_samples=16384)
  with pytest.raises(AssertionError, match='GPU work'):
    est.predict_bands(tall.iloc[:16384], 'place', num_samples=16384)      # 2^28 cells: the cap itself
  # the seam's own checks
  groups = inference.csr_from_codes(np.arange(12) // 3, 4)
  seam = lambda *a, **k: inference.band_summaries(np.zeros((12, 1)), 'NB', est.params_, None, *a, **k)
  with pytest.raises(ValueError, match='^num_samples=16385: the bands are summarised from at most 16384 sample paths$'):
    seam(16385, 0, len(lead), groups)
  with pytest.raises(ValueError, match='at least one sample path'):
    seam(0, 0, len(lead), groups)
  with pytest.raises(ValueError, match=r'^coverage must lie in \(0, 1\]; got \[0.5, 1.01\]$'):
    seam(10, 0, len(lead), groups, coverage=(0.5, 1.01))
  with pytest.raises(ValueError, match=r"^of='window': 'rows' \(the draws at the rows\) or 'cumulative' \(their running "
                                       r'totals\)$'):
    seam(10, 0, len(lead), groups, of='window')
  with pytest.raises(ValueError, match=r'^observed must hold one value per row \(12,\); got \(4,\)$'):
    seam(10, 0, len(lead), groups, observed=np.zeros(4))
  with pytest.raises(ValueError, match=r"^of='cumulative': seg_rows must hold one entry per row \(12\); got 11$"):
    seam(10, 0, len(lead), (groups[0], groups[1][:11]), of='cumulative')
  with pytest.raises(ValueError, match=r'^groups: seg_offsets covers 12 positions, seg_rows holds 11$'):
    seam(10, 0, len(lead), (groups[0], groups[1][:11]))
  with pytest.raises(ValueError, match='held whole on the device, at most 268435456 cells'):
    inference.band_summaries(np.zeros((16385, 1)), 'NB', est.params_, None, 16384, 0, len(lead),
                             inference.csr_from_codes(np.zeros(16385, dtype=np.int64), 1))
  with pytest.raises(AssertionError, match='GPU work'):
    seam(10, 0, len(lead), groups, coverage=(0.5, 1.0), of='cumulative', observed=np.arange(12.0))
