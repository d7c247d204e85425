"""Moving-window totals of the sample paths on the GPU (include/bnf.h bnf_predictive_group_windows) against the naive
loop of tests/windows_ref.py (a direct float64 sum per window) on `Engine.predictive_samples` for the same seed.
NB / ZINB: every sum is an exact integer, every comparison is EXACT.  NORMAL: |window - ref| <= 2 x
cumulative_ref.normal_bound at the position = 2 n 2^-52 sum |x| with n the participating positions of the group so far
and the sum over them: the reference's direct sum errs by at most (n - 1) u sum |x|, a sum of the differences
x[p] - x[p - w] from the group's start by at most 2 n u sum |x|, u = 2^-53; nothing is measured.  (Where a NaN draw
lies among them the bound counts it as a position and adds 0 for it, which is how it enters the device's sum;
cumulative_ref.normal_bound itself turns NaN there.)  The NaN cells coincide exactly.  Peak, row, count and the
counters equal those recomputed on the host from the GPU's own window matrix in every cell, and those of the reference
wherever the reference decides by more than the bound -- and the tests assert that it does so in every cell.  The
engine-level tests use synthetic loc / aux on a forward-only engine with M = 4, as tests/test_gpu_cumulative.py does."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from bayesnf_amd import _native, inference, spatiotemporal
from tests import cumulative_ref as Cu
from tests import windows_ref as Wi
from tests.test_gpu_cumulative import _half_median_level, _summary_check
from tests.test_gpu_extremes import _grouping, _host, _same
from tests.test_gpu_sampling import _dev, _engine, _fit, _mixed_inputs

pytestmark = pytest.mark.gpu

TILE = 1024
DERIVED = ('peak', 'peak_row', 'count', 'peak_count', 'exceed_count')
HUGE = 1e300                                       # a threshold no window total passes


def _bound(x, off, rows):
  """2 x cumulative_ref.normal_bound per (path, position), a NaN draw counted as a position that adds 0."""
  return 2.0 * Cu.normal_bound(np.where(np.isnan(x), np.float32(0), x), off, rows)


def _check(tag, obs, got, x, off, rows, w, thr, ref=None):
  """Everything `got` holds against the reference on the draws x (module docstring) -> the reference."""
  R = x.shape[1]
  off, rows = np.asarray(off), np.asarray(rows)
  if ref is None:
    ref = Wi.group_windows(x, off, rows, w, thr)
  assert got['peak'].dtype == np.float64 and got['peak'].shape == ref['peak'].shape, tag
  assert got['peak_row'].dtype == np.int32 and got['peak_row'].shape == ref['peak_row'].shape, tag
  if thr is None:
    assert 'count' not in got and 'exceed_count' not in got, (tag, 'threshold outputs without a threshold')
  if 'window' in got:
    assert got['window'].dtype == np.float64 and got['window'].shape == ref['window'].shape, tag
    assert np.array_equal(np.isnan(got['window']), np.isnan(ref['window'])), (tag, 'NaN cells')
    own = Wi.from_windows(got['window'], off, rows, R, w, thr)
    for k in DERIVED:
      if k in got:
        assert np.array_equal(got[k], own[k], equal_nan=True), (tag, k, 'against the GPU window totals')
  if obs == 'NORMAL':
    bound = _bound(x, off, rows)
    if 'window' in got:
      ok = ~np.isnan(ref['window'])
      err = np.abs(got['window'] - ref['window'])
      worst = float(np.max(err[ok] / np.maximum(bound[ok], 1e-300))) if ok.any() else 0.0
      print(f'{tag}: window totals: largest error / bound {worst:.3f}')
      assert np.all(err[ok] <= bound[ok]), (tag, 'window', worst)
    und = Wi.undecided(ref, bound, off, thr)
    assert not und.any(), (tag, 'the reference leaves cells undecided: change the seed', int(und.sum()))
    # decided: the peak is reached at the reference's position, its value within the bound there
    pos_of = np.full(R + 1, 0, dtype=np.int64)
    part = (rows >= 0) & (rows < R)
    pos_of[rows[part]] = np.flatnonzero(part)
    assert np.array_equal(np.isnan(got['peak']), np.isnan(ref['peak'])), (tag, 'NaN peaks')
    seen = ~np.isnan(ref['peak'])
    at = pos_of[np.maximum(ref['peak_row'], 0)]
    pb = np.take_along_axis(bound, at, axis=1)
    assert np.all(np.abs(got['peak'] - ref['peak'])[seen] <= pb[seen]), (tag, 'peak')
  else:
    for k in ('window', 'peak'):
      if k in got:
        assert np.array_equal(got[k], ref[k], equal_nan=True), (tag, k, int((got[k] != ref[k]).sum()))
  for k in DERIVED[1:]:
    if k in got:
      assert np.array_equal(got[k], ref[k]), (tag, k, int((got[k] != ref[k]).sum()))
  if 'peak_count' in got:
    hit = got['peak_row'][got['peak_row'] >= 0]
    assert np.array_equal(got['peak_count'], np.bincount(hit, minlength=R)), (tag, 'peak_count')
  return ref


@pytest.mark.parametrize('kind', ['sizes', 'half'])
@pytest.mark.parametrize('obs', ['NORMAL', 'NB', 'ZINB'])
def test_mixed_and_crossing_tiles(obs, kind):
  """Tiles inside one group, mixed tiles and groups that cross tile edges; the rows of every group in a random order
  (time is position order, not row order).  Windows of 1 (inside a thread's 4 positions), 7 (across lanes and tile
  edges), 1024 (exactly a tile), 1500 (reaching back over more than one tile) and R (the totals).  The threshold of a
  group is half the median of its reference peaks.  A few rows carry a NaN location: NORMAL draws NaN there, which makes
  exactly the windows that hold it NaN."""
  eng, _ = _engine(obs)
  M, R, n = 4, 3 * TILE + 37, 16
  rng = np.random.default_rng(5)
  loc, aux = _mixed_inputs(obs, M, R, 21)
  codes, G = _grouping(kind, R, rng)
  big = int(np.argmax(np.bincount(codes, minlength=G)))
  nan_rows = np.concatenate([np.flatnonzero(codes == big)[[3, 4, 200, 700]], [7, 2048]])
  loc[:, nan_rows] = np.nan
  off, rows = inference.csr_ordered(codes, G, rng.permutation(R))
  assert not np.array_equal(rows, inference.csr_from_codes(codes, G)[1])
  loc_d, aux_d = _dev(eng, loc), _dev(eng, aux)
  x = eng.predictive_samples(loc_d, aux_d, n, seed=42).cpu().numpy()
  assert obs != 'NORMAL' or np.isnan(x[:, nan_rows]).all()
  sums = eng.predictive_group_sums(loc_d, aux_d, off, rows, n, 42).cpu().numpy()
  nan_pos = np.flatnonzero(np.isin(rows, nan_rows))
  group_of = np.repeat(np.arange(G), np.diff(off))
  recovered = 0
  for w in (1, 7, TILE, 1500, R):
    thr = _half_median_level(Wi.group_windows(x, off, rows, w)['peak'])
    if w == 1:
      thr = thr.astype(np.float32).astype(np.float64)      # the per-row limits of predictive_group_extremes are float32
    call = lambda **kw: _host(eng.predictive_group_windows(loc_d, aux_d, off, rows, n, 42, w, **kw))
    got = call(threshold=thr, windows=True)
    assert set(got) == {'window'} | set(DERIVED)
    ref = _check(f'{obs} {kind} w={w}', obs, got, x, off, rows, w, thr)
    above = got['count'] > 0
    print(f'{obs} {kind} w={w}: {G} groups, {int(above.sum())} of {above.size} (path, group) with a window above, '
          f'{int(np.isnan(got["window"]).sum())} NaN windows, {int(ref["candidate"].sum())} candidates')
    assert above.sum() > above.size // 4 and (~above).sum() > 0
    if obs == 'NORMAL':
      # a NaN draw leaves its windows: the window ending w positions after it is finite again, the one before it is NaN
      for p in nan_pos:
        b = off[group_of[p] + 1]
        if p + w < b and not np.isin(np.arange(p + 1, p + w + 1), nan_pos).any():
          assert np.isnan(got['window'][:, p + w - 1]).all() and np.isfinite(got['window'][:, p + w]).all(), (w, p)
          recovered += 1
      assert np.isnan(got['window'][:, nan_pos]).all()
    if w == 1:
      # every participating position is a candidate of its own: the extremes of the paths at the same threshold
      ext = _host(eng.predictive_group_extremes(loc_d, aux_d, off, rows, n, 42, threshold=thr[codes].astype(np.float32)))
      real = np.isfinite(ext['max'])                       # extremes: a group of NaN draws alone reports -inf at a row
      if obs == 'NORMAL':                                  # a window of 1 is still summed as differences from the start
        assert np.all(np.abs(got['peak'] - ext['max'])[real] <= _bound(x, off, rows).max())
      else:
        assert np.array_equal(got['peak'][real], ext['max'][real])
      assert np.array_equal(got['peak_row'][real], ext['argmax'][real])
      assert np.isnan(got['peak'][~real]).all() and np.all(got['peak_row'][~real] == -1)
      assert np.array_equal(got['exceed_count'], ext['exceed_count']) and np.array_equal(got['count'], ext['count'])
    if w == R:
      # the only candidate window of every group is its total
      assert np.array_equal(np.isnan(got['peak']), np.isnan(sums) | (np.diff(off) == 0)[None, :])
      full = ~np.isnan(got['peak'])
      if obs == 'NORMAL':
        last = np.maximum(np.asarray(off[1:]) - 1, 0)
        assert np.all(np.abs(got['peak'] - sums)[full] <= _bound(x, off, rows)[:, last][full])
      else:
        assert np.array_equal(got['peak'][full], sums[full]), 'peak against predictive_group_sums'
      assert np.array_equal(got['peak_row'][full], np.broadcast_to(rows[np.maximum(off[1:] - 1, 0)], got['peak'].shape)[full])
  assert obs != 'NORMAL' or recovered >= 4
  eng.close()


def test_scripted_groups():
  """NB, the four members made one.  Eight groups on one position axis (tile = 1024 positions), windows of 7 and 2500:
    A  positions 0 .. 2047 (2 tiles), finished by the block of tile 0 walking on
    F  500 positions: filler, so that B starts mid-tile
    B  3 * 1024 + 424 positions from 2548 on, over the tiles 2 .. 5: with w = 2500 the draw that leaves lies two chunks
       back and is drawn again, and its first candidate lies in its third chunk
    C  5 positions: shorter than both windows -- one candidate, its total, at its last row
    D  6 positions whose last entry of seg_rows is -1: no candidate -- NaN, -1, 0
    E  empty: NaN, -1, 0
    H  100 positions with entries of -1 inside windows: they occupy slots, add nothing and are no candidates
    K  300 positions, threshold 1e300: count 0 and no exceed_count"""
  eng, _ = _engine('NB')
  M, n = 4, 3
  sizes = [2 * TILE, 500, 3 * TILE + 424, 5, 6, 0, 100, 300]
  off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
  R, G = int(off[-1]), len(sizes)
  a, f, b, c, d, e, h, k = (int(v) for v in off[:8])
  assert b == 2548 and c == 6044
  rng = np.random.default_rng(2)
  table_rows = rng.permutation(R).astype(np.int32)        # the table row of every position: not the position itself
  loc, aux = _mixed_inputs('NB', M, R, 4)
  loc[:], aux[:] = loc[3], aux[3]                          # total_count 60: the least spread
  loc_d, aux_d = _dev(eng, loc), _dev(eng, aux)
  x = eng.predictive_samples(loc_d, aux_d, n, seed=1).cpu().numpy()
  rows = table_rows.copy()
  rows[d + 5] = -1
  rows[[h + 3, h + 20, h + 21, h + 99]] = -1
  sums = eng.predictive_group_sums(loc_d, aux_d, off, rows, n, 1).cpu().numpy()
  for w in (7, 2500):
    thr = _half_median_level(Wi.group_windows(x, off, rows, w)['peak'])
    thr[7] = HUGE
    got = _host(eng.predictive_group_windows(loc_d, aux_d, off, rows, n, 1, w, threshold=thr, windows=True))
    ref = _check(f'scripted w={w}', 'NB', got, x, off, rows, w, thr)
    pos_of = {int(r): p for p, r in enumerate(rows) if r >= 0}
    where = np.vectorize(lambda r: pos_of.get(int(r), -1))(got['peak_row'])
    for s in range(n):
      assert a + min(w, 2 * TILE) - 1 <= where[s, 0] < f and f + min(w, 500) - 1 <= where[s, 1] < b
      assert b + w - 1 <= where[s, 2] < c                   # w = 2500: in B's third or fourth chunk
      assert where[s, 3] == c + 4 and got['peak'][s, 3] == sums[s, 3] == x[s, rows[c:c + 5]].astype(np.float64).sum()
      assert got['count'][s, 3] == float(sums[s, 3] > thr[3])
      for g in (4, 5):
        assert np.isnan(got['peak'][s, g]) and got['peak_row'][s, g] == -1 and got['count'][s, g] == 0.0
      assert got['count'][s, 7] == 0.0 and where[s, 7] >= k + min(w, 300) - 1
    assert got['exceed_count'][table_rows[k:k + 300]].sum() == 0 and got['peak_count'].sum() == (6 if w == 7 else 5) * n
    assert got['count'].sum() == got['exceed_count'].sum() > 0
    # the windows of D are written although none is a candidate; entries of -1 occupy a slot and add nothing
    assert np.array_equal(got['window'][:, d + 5], got['window'][:, d + 4]) and not ref['candidate'][d:d + 6].any()
    assert not ref['candidate'][[h + 3, h + 20, h + 21, h + 99]].any()
    if w == 7:
      assert np.array_equal(got['window'][:, h + 3], got['window'][:, h + 2])              # nothing leaves yet
      assert np.array_equal(got['window'][:, h + 20], got['window'][:, h + 19] - x[:, rows[h + 13]])
      assert np.array_equal(got['window'][:, h + 27], got['window'][:, h + 26] + x[:, rows[h + 27]])   # -1 leaves: nothing
      assert np.all(where[:, 6] != h + 99) and ref['candidate'][h + 6:h + 99].sum() == 93 - 2
    else:
      assert np.isnan(got['peak'][:, 6]).all()             # shorter than the window and its last entry is -1
  eng.close()


@pytest.mark.parametrize('obs', ['NORMAL', 'NB'])
def test_one_group_over_66_tiles_and_shifted(obs):
  """One group over 66 tiles and 5 positions, finished by the block of tile 0 walking over 66 further tiles, windows of
  7 and 3000, and the same shifted by a leading singleton, so the tile edges fall elsewhere in the group.  Counts
  identical up to the shift; NORMAL within the bound (the order of its additions follows the tiling)."""
  eng, _ = _engine(obs)
  M, R, n = 4, 66 * TILE + 5, 4
  loc, aux = _mixed_inputs(obs, M, R, 3)
  rng = np.random.default_rng(6)
  order = rng.permutation(R)
  codes = np.zeros(R, dtype=np.int64)
  codes[700] = 1                                       # the singleton's position comes last: the big group starts at 0
  off, rows = inference.csr_ordered(codes, 2, order)
  off2, rows2 = inference.csr_ordered(1 - codes, 2, order)            # the singleton in front
  assert np.array_equal(rows[:R - 1], rows2[1:]) and rows[R - 1] == rows2[0] == 700
  loc_d, aux_d = _dev(eng, loc), _dev(eng, aux)
  x = eng.predictive_samples(loc_d, aux_d, n, seed=9).cpu().numpy()
  for w in (7, 3000):
    ref = Wi.group_windows(x, off, rows, w)
    thr = _half_median_level(ref['peak'])
    ref.update(Wi.from_windows(ref['window'], off, rows, R, w, thr))
    # the reference of the shifted layout: the same direct sums, one position later
    win2 = np.concatenate([ref['window'][:, R - 1:], ref['window'][:, :R - 1]], axis=1)
    thr2 = thr[::-1].copy()
    ref2 = Wi.from_windows(win2, off2, rows2, R, w, thr2)
    ref2.update(window=win2, candidate=Wi.candidates(off2, rows2, R, w))
    got = _host(eng.predictive_group_windows(loc_d, aux_d, off, rows, n, 9, w, threshold=thr, windows=True))
    got2 = _host(eng.predictive_group_windows(loc_d, aux_d, off2, rows2, n, 9, w, threshold=thr2, windows=True))
    _check(f'{obs} 66 tiles w={w}', obs, got, x, off, rows, w, thr, ref)
    _check(f'{obs} 66 tiles w={w}, shifted', obs, got2, x, off2, rows2, w, thr2, ref2)
    assert ref['candidate'].sum() == R - 1 - (w - 1) + 1 and got['count'][:, 0].min() > 0
    if obs == 'NB':
      assert np.array_equal(got['window'][:, :R - 1], got2['window'][:, 1:])
      for k in ('peak', 'peak_row', 'count'):
        assert np.array_equal(got[k][:, 0], got2[k][:, 1]) and np.array_equal(got[k][:, 1], got2[k][:, 0]), k
      assert np.array_equal(got['peak_count'], got2['peak_count']) and np.array_equal(got['exceed_count'], got2['exceed_count'])
  eng.close()


@pytest.mark.parametrize('obs', ['NORMAL', 'ZINB'])
def test_invariance_bit_for_bit(obs):
  """The bits of every output depend on the seed, the path, the rows, the window, the threshold and the CSR arrays only:
  sample0 chunks, row0 against the column slice, the outputs asked for, a second run, and a launch that strides its
  blocks over several paths (grid.y as for the running totals: 3 tiles and 6 groups give 5461, so the call of 5470 paths
  strides 9 blocks over two paths each).  Windows of 300 (inside the tile and its neighbour) and 1100 (the group of 1400
  positions draws again)."""
  eng, _ = _engine(obs)
  M, R, n = 4, 2 * TILE + 500, 16
  rng = np.random.default_rng(13)
  loc, aux = _mixed_inputs(obs, M, R, 11)
  sizes = [900, 200, 1, 0, 1400, 47]                    # 900 + 200 and 1400 cross the two tile edges
  codes = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
  G = len(sizes)
  off, rows = inference.csr_ordered(codes, G, rng.permutation(R))
  loc_d, aux_d = _dev(eng, loc), _dev(eng, aux)
  x = eng.predictive_samples(loc_d, aux_d, n, seed=5).cpu().numpy()
  big_n = 16384 // 3 + 9
  for w in (300, 1100):
    thr = _half_median_level(Wi.group_windows(x, off, rows, w)['peak'])
    call = lambda n_, **kw: _host(eng.predictive_group_windows(loc_d, aux_d, off, rows, n_, 5, w, threshold=thr, **kw))
    full = call(n, windows=True)
    _check(f'{obs} w={w} one call', obs, full, x, off, rows, w, thr)
    # (a) two calls of 8 paths give the rows of the one call of 16; their per-row counters add up; a second run
    halves = [call(8, windows=True, sample0=s0) for s0 in (0, 8)]
    for k in ('peak', 'peak_row', 'window', 'count'):
      assert _same(np.concatenate([halves[0][k], halves[1][k]]), full[k]), ('sample0', w, k)
    for k in ('peak_count', 'exceed_count'):
      assert np.array_equal(halves[0][k] + halves[1][k], full[k]), ('sample0', w, k)
    again = call(n, windows=True)
    for k in full:
      assert _same(again[k], full[k]), ('two runs differ', w, k)
    # (b) more paths than grid.y: blocks stride over the paths; the first 16 are those of the call of 16, and two halves
    # with sample0 give the same matrices
    big = call(big_n)
    for k in ('peak', 'peak_row', 'count'):
      assert _same(big[k][:n], full[k]), ('strided', w, k)
    parts = [call(big_n // 2, sample0=s0) for s0 in (0, big_n // 2)]
    for k in ('peak', 'peak_row', 'count'):
      assert _same(np.concatenate([parts[0][k], parts[1][k]]), big[k]), ('strided, sample0', w, k)
    for k in ('peak_count', 'exceed_count'):
      assert np.array_equal(parts[0][k] + parts[1][k], big[k]), ('strided, sample0', w, k)
    # (c) every subset of the optional outputs: what is asked for does not change what is given
    for with_thr, windows, per_row in itertools.product((False, True), repeat=3):
      some = _host(eng.predictive_group_windows(loc_d, aux_d, off, rows, n, 5, w, threshold=thr if with_thr else None,
                                                windows=windows, per_row=per_row))
      want = {'peak', 'peak_row'} | ({'window'} if windows else set()) | ({'count'} if with_thr else set())
      want |= ({'peak_count'} if per_row else set()) | ({'exceed_count'} if per_row and with_thr else set())
      assert set(some) == want, (with_thr, windows, per_row)
      for k in some:
        assert _same(some[k], full[k]), ('outputs asked for', w, k, with_thr, windows, per_row)
  w, thr = 300, _half_median_level(Wi.group_windows(x, off, rows, 300)['peak'])
  call = lambda n_, **kw: _host(eng.predictive_group_windows(loc_d, aux_d, off, rows, n_, 5, w, threshold=thr, **kw))
  full = call(n, windows=True)
  # (d) row0: the columns a .. b of the table as a table of their own.  Their groups come first on the position axis of
  # the whole table's layout below, so every group lies where it lies in the slice's own layout
  lo, hi = 300, 300 + TILE + 200
  sub_sizes = [700, 1, 523]
  sub_codes = rng.permutation(np.repeat(np.arange(3), sub_sizes))
  sub_off, sub_rows = inference.csr_ordered(sub_codes, 3, rng.permutation(hi - lo))
  rest = np.concatenate([np.arange(lo), np.arange(hi, R)])
  whole_off = np.concatenate([sub_off, [R]]).astype(np.int32)
  whole_rows = np.concatenate([sub_rows + lo, rng.permutation(rest)]).astype(np.int32)
  thr4 = np.asarray([thr[0], thr[4], thr[1], thr[4]])
  whole = _host(eng.predictive_group_windows(loc_d, aux_d, whole_off, whole_rows, n, 5, w, threshold=thr4, windows=True))
  part = _host(eng.predictive_group_windows(loc_d[:, lo:hi].contiguous(), aux_d, sub_off, sub_rows, n, 5, w,
                                            threshold=thr4[:3], windows=True, row0=lo))
  for k in ('peak', 'count'):
    assert _same(part[k], whole[k][:, :3]), ('row0', k)
  assert _same(part['window'], whole['window'][:, :hi - lo]), ('row0', 'window')
  assert np.array_equal(np.where(part['peak_row'] >= 0, part['peak_row'] + lo, -1), whole['peak_row'][:, :3])
  assert np.array_equal(part['exceed_count'], whole['exceed_count'][lo:hi])
  only3 = np.bincount(whole['peak_row'][:, :3].ravel(), minlength=R)[lo:hi]
  assert np.array_equal(part['peak_count'], only3)
  # (e) weights wholly on one member: that member's M = 1 result; NULL weights: the unweighted call
  for m in (0, 2):
    cum = np.cumsum(np.eye(M)[m])
    one = call(n, windows=True, cum_weights=cum)
    alone = _host(eng.predictive_group_windows(loc_d[m:m + 1], aux_d[m:m + 1], off, rows, n, 5, w, threshold=thr, windows=True))
    for k in one:
      assert _same(one[k], alone[k]), ('one member', m, k)
  none = call(n, windows=True, cum_weights=None)
  for k in full:
    assert _same(none[k], full[k]), ('NULL weights', k)
  # general weights: the reference on the weighted draws
  cum = np.cumsum([0.4, 0.1, 0.2, 0.3])
  cum[-1] = 1.0
  xw = eng.predictive_samples(loc_d, aux_d, n, seed=5, cum_weights=cum).cpu().numpy()
  thr_w = _half_median_level(Wi.group_windows(xw, off, rows, w)['peak'])
  wgt = _host(eng.predictive_group_windows(loc_d, aux_d, off, rows, n, 5, w, threshold=thr_w, windows=True, cum_weights=cum))
  eng.close()
  _check(f'{obs} weighted', obs, wgt, xw, off, rows, w, thr_w)
  assert not np.array_equal(wgt['peak'], full['peak'])


def test_errors_write_nothing():
  """BNF_ERR_INVALID for a NULL out_peak, a window below 1 and the threshold outputs without a threshold; the outputs
  keep their bytes.  Then the smallest valid call (out_peak alone) and everything, on the same buffers."""
  eng, _ = _engine('NB')
  M, R, n, G = 4, 300, 2, 3
  loc, aux = _mixed_inputs('NB', M, R, 1)
  loc_d, aux_d = _dev(eng, loc), _dev(eng, aux)
  dev = eng.device
  off_d = torch.tensor([0, 100, 100, 300], dtype=torch.int32, device=dev)
  rows_d = torch.arange(R, dtype=torch.int32, device=dev)
  thr_d = torch.full((G,), 40.0, dtype=torch.float64, device=dev)
  out = {'peak': torch.full((n, G), 7.0, dtype=torch.float64, device=dev),
         'peak_row': torch.full((n, G), 7, dtype=torch.int32, device=dev),
         'window': torch.full((n, R), 7.0, dtype=torch.float64, device=dev),
         'count': torch.full((n, G), 7.0, dtype=torch.float64, device=dev),
         'peak_count': torch.full((R,), 7, dtype=torch.int32, device=dev),
         'exceed_count': torch.full((R,), 7, dtype=torch.int32, device=dev)}
  p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
  names = ('peak', 'peak_row', 'window', 'count', 'peak_count', 'exceed_count')

  def call(w_, thr, sizes=(M, R, G, n), **given):
    ptrs = [p(given.get(k)) for k in names]
    m_, r_, g_, n_ = sizes
    return eng.lib.bnf_predictive_group_windows(eng.handle, p(loc_d), p(aux_d), m_, r_, p(off_d), p(rows_d), g_, n_,
                                                C.c_uint64(3), 0, 0, None, w_, p(thr), *ptrs)

  assert call(5, thr_d, **{k: v for k, v in out.items() if k != 'peak'}) == -1 and 'out_peak' in _native.last_error()
  for bad in (0, -1, -2 ** 31):
    assert call(bad, thr_d, **out) == -1 and 'window' in _native.last_error(), bad
  for k in ('count', 'exceed_count'):
    assert call(5, None, peak=out['peak'], peak_row=out['peak_row'], window=out['window'], **{k: out[k]}) == -1, k
    assert 'threshold' in _native.last_error()
  for sizes in ((0, R, G, n), (M, 0, G, n), (M, R, 0, n), (M, R, G, 0)):
    assert call(5, thr_d, sizes=sizes, **out) == -1, sizes
  torch.cuda.synchronize()
  for k, v in out.items():
    assert torch.all(v == 7), ('written by a refused call', k)
  # the smallest valid call: a peak alone; then everything, on the same buffers
  assert call(5, None, peak=out['peak']) == 0, _native.last_error()
  torch.cuda.synchronize()
  only_peak = out['peak'].cpu().numpy().copy()
  for k in names[1:]:
    assert torch.all(out[k] == 7), ('written without being asked for', k)
  out['peak_count'].zero_()
  out['exceed_count'].zero_()
  assert call(5, thr_d, **out) == 0, _native.last_error()
  torch.cuda.synchronize()
  x = eng.predictive_samples(loc_d, aux_d, n, seed=3).cpu().numpy()
  got = _host(out)
  eng.close()
  assert _same(got['peak'], only_peak)
  _check('raw call', 'NB', got, x, np.asarray([0, 100, 100, 300]), np.arange(R), 5, np.full(G, 40.0))
  assert np.isnan(got['peak'][:, 1]).all() and np.all(got['peak_row'][:, 1] == -1) and np.all(got['count'][:, 1] == 0)


@pytest.mark.parametrize('kind', ['map', 'vi'])
def test_estimator_windows_end_to_end(golden_dir, kind):
  """chickenpox fixture (NB for MAP, NORMAL for VI) with its rows SHUFFLED: predict_windows / score_windows with a window
  of 4 against the same quantities formed on the host from predict_samples(table, S, seed) with the time ordering applied
  there: direct window sums, np.quantile, CRPS and PIT from tests/totals_ref.py.  The per-row shares and 'any' are exact
  (NORMAL: the reference decides every cell by more than the bound); NB: the observed columns and the means are exact
  too; the rest at the bars of tests/totals_ref.py, for NORMAL plus the summation bound of the module docstring."""
  df, est = _fit(golden_dir, kind)
  df = df.assign(year=df['datetime'].dt.year).sample(frac=1.0, random_state=4).reset_index(drop=True)
  assert not df['datetime'].is_monotonic_increasing
  S, seed, levels, w = 300, 3, (0.025, 0.5, 0.975), 4
  R = len(df)
  x = est.predict_samples(df, S, seed)
  y = df['chickenpox'].to_numpy(dtype=np.float64)
  exact = kind == 'map'
  for by in ('location', 'year'):
    keys = np.sort(df[by].unique())
    codes = np.searchsorted(keys, df[by].to_numpy())
    G = len(keys)
    rows = df.assign(_g=codes).sort_values(['_g', 'datetime'], kind='stable').index.to_numpy()
    off = np.concatenate([[0], np.cumsum(np.bincount(codes, minlength=G))])
    thr = _half_median_level(Wi.group_windows(x, off, rows, w)['peak'])
    ref = Wi.group_windows(x, off, rows, w, thr)
    cand = ref['candidate']
    by_row = np.empty(R, dtype=np.int64)
    by_row[rows] = np.arange(R)                              # the position of every table row
    bound = np.zeros((S, R)) if exact else _bound(x, off, rows)
    assert not Wi.undecided(ref, bound, off, thr).any(), 'the reference leaves cells undecided: change the seed'
    delta_pos = bound.max(axis=0)
    delta_g = np.asarray([delta_pos[off[g]:off[g + 1]].max() for g in range(G)])
    res = est.score_windows(df, by, w, threshold=thr[codes], quantiles=levels, num_samples=S, seed=seed)
    assert list(res['keys']) == list(keys) and res['n'] == G
    obs = spatiotemporal.group_target_windows(y, off, rows, w, thr)
    for g in range(G):                                       # the observed columns once more, by hand
      r = rows[off[g]:off[g + 1]]
      win = np.asarray([y[r[i - w + 1:i + 1]].sum() for i in range(w - 1, len(r))])
      assert np.array_equal(obs['window'][r[w - 1:]], win) and np.isnan(obs['window'][r[:w - 1]]).all()
      assert obs['peak'][g] == win.max() and obs['peak_row'][g] == r[w - 1 + int(np.argmax(win))]
      assert obs['count'][g] == (win > thr[g]).sum()
    assert np.array_equal(res['observed_peak'], obs['peak']) and np.array_equal(res['observed_peak_row'], obs['peak_row'])
    assert np.array_equal(res['observed_window'], obs['window'], equal_nan=True)
    assert np.array_equal(res['observed_count'], obs['count'])
    # the probabilities are exact
    assert np.array_equal(res['peak_probability'], ref['peak_count'] / S)
    assert np.array_equal(res['exceed_probability'], ref['exceed_count'] / S)
    assert np.array_equal(res['any'], (ref['count'] > 0).sum(axis=0) / S)
    assert np.array_equal(np.bincount(codes, weights=np.rint(res['peak_probability'] * S), minlength=G), np.full(G, float(S)))
    assert np.array_equal(res['peak_row_probability'], res['peak_probability'][obs['peak_row']])
    # per-row results are NaN exactly where no full-length window ends
    full_rows = rows[cand]
    part_rows = rows[~cand]
    assert cand.sum() == R - (w - 1) * G
    for k in ('window_mean', 'window_crps'):
      assert np.isnan(res[k][part_rows]).all() and not np.isnan(res[k][full_rows]).any(), k
    assert np.isnan(res['window_quantiles'][:, part_rows]).all() and np.isnan(res['window_pit'][:, part_rows]).all()
    win_rows = ref['window'][:, cand]                        # (S, candidates), the columns in the order of full_rows
    if exact:
      assert np.array_equal(res['peak_mean'], ref['peak'].sum(axis=0) / S)
      assert np.array_equal(res['count_mean'], ref['count'].sum(axis=0) / S)
      assert np.array_equal(res['window_mean'][full_rows], win_rows.sum(axis=0) / S)
    for name, m, yy, dl, cols in (('peak', ref['peak'], obs['peak'], delta_g, slice(None)),
                                  ('count', ref['count'], obs['count'], np.zeros(G), slice(None)),
                                  ('window', win_rows, obs['window'][full_rows], delta_pos[cand], full_rows)):
      have = dict(mean=res[f'{name}_mean'][cols], quantiles=res[f'{name}_quantiles'][:, cols],
                  crps=res[f'{name}_crps'][cols], pit=res[f'{name}_pit'][:, cols])
      _summary_check(f'{kind} by {by}: {name}', have, m, yy, levels, dl)
    assert res['mean_peak_crps'] == float(np.mean(res['peak_crps'], dtype=np.float64))
    assert res['mean_count_crps'] == float(np.mean(res['count_crps'], dtype=np.float64))
    assert res['mean_window_crps'] == float(np.mean(res['window_crps'][np.sort(full_rows)], dtype=np.float64))    # in table order
    assert res['mean_peak_row_probability'] == float(np.mean(res['peak_row_probability'], dtype=np.float64))
    print(f'{kind} by {by}: observed peak {obs["peak"]}, forecast mean {res["peak_mean"]}, windows above '
          f'{res["count_mean"]} (observed {obs["count"]}), any {res["any"]}, P(observed peak row) {res["peak_row_probability"]}')
    pred = est.predict_windows(df, by, w, threshold=thr[codes], quantiles=levels, num_samples=S, seed=seed)
    assert set(pred) == {'keys', 'peak_mean', 'peak_quantiles', 'peak_probability', 'window_mean', 'window_quantiles',
                         'count_mean', 'count_quantiles', 'exceed_probability', 'any'}
    for k in set(pred) - {'keys'}:
      assert _same(pred[k], res[k]), k
  # curve=False and no threshold: the same bits for what remains; a scalar threshold and another ordering column
  bare = est.predict_windows(df, 'year', w, curve=False, quantiles=levels, num_samples=S, seed=seed)
  assert set(bare) == {'keys', 'peak_mean', 'peak_quantiles', 'peak_probability'}
  for k in set(bare) - {'keys'}:
    assert _same(bare[k], pred[k]), k
  flat = est.predict_windows(df, 'year', w, threshold=float(thr.mean()), order_by='chickenpox', num_samples=S, seed=seed)
  rows2 = df.assign(_g=codes).sort_values(['_g', 'chickenpox'], kind='stable').index.to_numpy()
  ref2 = Wi.group_windows(x, off, rows2, w, np.full(G, float(thr.mean())))
  if exact:
    assert np.array_equal(flat['exceed_probability'], ref2['exceed_count'] / S)
    assert np.array_equal(flat['peak_probability'], ref2['peak_count'] / S)
  assert flat['window_quantiles'].shape == (1, R) and flat['count_quantiles'].shape == (1, G)
  # a window longer than every group: the peak is the total, reached at the group's last row
  tot = est.predict_windows(df, 'year', R, curve=False, quantiles=levels, num_samples=S, seed=seed)
  sums = est.predict_totals(df, 'year', quantiles=levels, num_samples=S, seed=seed)
  if exact:
    assert np.array_equal(tot['peak_mean'], sums[0])
  assert np.array_equal(np.flatnonzero(tot['peak_probability']), np.sort(rows[off[1:] - 1]))
  # a group with a NaN target row is not scored; the forecast does not change
  d = df.copy()
  d.loc[d.index[[1]], 'chickenpox'] = np.nan
  res2 = est.score_windows(d, 'year', w, threshold=thr[codes], quantiles=levels, num_samples=S, seed=seed)
  gone = codes[1]
  assert res2['n'] == G - 1 and np.isnan(res2['observed_peak'][gone]) and res2['observed_peak_row'][gone] == -1
  for k in ('peak_crps', 'count_crps', 'peak_row_probability'):
    assert np.array_equal(np.isnan(res2[k]), np.arange(G) == gone), k
  assert _same(res2['peak_mean'], res['peak_mean']) and _same(res2['peak_probability'], res['peak_probability'])
  lost = np.isnan(res2['observed_window']) & ~np.isnan(res['observed_window'])
  assert 1 <= lost.sum() <= w and np.all(codes[lost] == gone)
  # weights are passed through: all weight on one member gives another forecast than equal weights
  wts = np.zeros(np.shape(est.params_[0])[:est._ensemble_dims])
  wts.flat[0] = 1.0
  one = est.predict_windows(df, 'year', w, threshold=thr[codes], num_samples=S, seed=seed, weights=wts)
  xw = est.predict_samples(df, S, seed, weights=wts)
  refw = Wi.group_windows(xw, off, rows, w, thr)
  if exact:
    assert np.array_equal(one['peak_mean'], refw['peak'].sum(axis=0) / S)
    assert np.array_equal(one['exceed_probability'], refw['exceed_count'] / S)
  assert not _same(one['peak_mean'], res['peak_mean'])
