"""Running totals of the sample paths and when they pass a level, on the GPU (include/bnf.h
bnf_predictive_group_cumulative) against the naive loop of tests/cumulative_ref.py (np.cumsum in float64) on
`Engine.predictive_samples` for the same seed.  NB / ZINB: every sum is an exact integer, every comparison is EXACT
(a NaN draw, from a NaN parameter, makes the same cells NaN on both sides).
NORMAL: |running - ref| <= n 2^-52 cumsum(|x|) with n the participating positions so far -- twice the standard bound
gamma_{n-1} sum |x| of a float64 sum in any order; nothing is measured -- and the crossing outputs are exactly those
recomputed on the host from the GPU's own running totals.  The engine-level tests use synthetic loc / aux on a
forward-only engine with M = 4, as tests/test_gpu_episodes.py does."""
import ctypes as C

import numpy as np
import pytest
import torch

from bayesnf_amd import _native, inference, spatiotemporal
from tests import cumulative_ref as Cu
from tests import totals_ref as T
from tests.test_gpu_extremes import _grouping, _host, _same
from tests.test_gpu_sampling import _dev, _engine, _fit, _mixed_inputs

pytestmark = pytest.mark.gpu

TILE = 1024
CROSSING = ('cross_step', 'cross_row', 'cross_count', 'above_count')
HUGE = 1e300                                       # a level no running total passes


def _half_median_level(total):
  """Per group: half the median over the paths of the reference total; 0 where every total is NaN."""
  nan = np.isnan(total).all(axis=0)
  return np.where(nan, 0.0, 0.5 * np.nanmedian(np.where(nan[None, :], 0.0, total), axis=0))


def _check(tag, obs, got, x, off, rows, level):
  """Everything `got` holds against the reference on the draws x.  Counts: exact.  NORMAL: the bound of the module
  docstring on 'running' and 'total', the same NaN cells, and the crossing outputs equal to those of the reference AND
  to those recomputed from the GPU's own running totals."""
  R = x.shape[1]
  off = np.asarray(off)
  ref = Cu.group_cumulative(x, off, rows, level)
  last = np.maximum(off[1:] - 1, 0)
  empty = np.diff(off) == 0
  assert got['total'].dtype == np.float64 and got['total'].shape == ref['total'].shape, tag
  if 'running' in got:
    assert got['running'].dtype == np.float64 and got['running'].shape == ref['running'].shape, tag
    # the total is the run at the group's last position, bit for bit
    assert _same(got['total'][:, ~empty], got['running'][:, last[~empty]]), (tag, 'total is not the last run')
  assert np.all(got['total'][:, empty] == 0.0), (tag, 'empty groups')
  if obs == 'NORMAL':
    bound = Cu.normal_bound(x, off, rows)
    if 'running' in got:
      assert np.array_equal(np.isnan(got['running']), np.isnan(ref['running'])), (tag, 'NaN cells')
      err = np.abs(got['running'] - ref['running'])
      ok = ~np.isnan(ref['running'])
      assert np.all(err[ok] <= bound[ok]), (tag, 'running', float(np.max(err[ok] / np.maximum(bound[ok], 1e-300))))
      print(f'{tag}: running totals: largest error / bound {float(np.max(err[ok] / np.maximum(bound[ok], 1e-300))):.3f}')
    tb = np.where(empty[None, :], 0.0, bound[:, last])
    assert np.array_equal(np.isnan(got['total']), np.isnan(ref['total'])), (tag, 'NaN totals')
    ok = ~np.isnan(ref['total'])
    assert np.all(np.abs(got['total'] - ref['total'])[ok] <= tb[ok]), (tag, 'total')
  else:
    for k in ('running', 'total'):
      if k in got:
        assert np.array_equal(got[k], ref[k], equal_nan=True), (tag, k, int((got[k] != ref[k]).sum()))
  if level is None:
    assert not set(CROSSING) & set(got), (tag, 'crossing outputs without a level')
    return ref
  assert got['cross_step'].dtype == np.float64 and got['cross_row'].dtype == np.int32, tag
  assert np.all(got['cross_step'][:, empty] == 0.0) and np.all(got['cross_row'][:, empty] == -1), (tag, 'empty groups')
  if obs == 'NORMAL':
    # no reference running total of a participating position lies within the bound of its level: no cell left out
    part = (np.asarray(rows) >= 0) & (np.asarray(rows) < R)
    lvl_pos = np.repeat(np.asarray(level, dtype=np.float64), np.diff(off))
    gap = np.abs(ref['running'] - lvl_pos[None, :])[:, part]
    assert np.all(np.isnan(gap) | (gap > bound[:, part])), (tag, 'a reference running total within the bound of its level')
    if 'running' in got:
      own = Cu.crossings_from_running(got['running'], off, rows, R, level)
      for k in CROSSING:
        if k in got:
          assert np.array_equal(got[k], own[k]), (tag, k, 'against the GPU running totals')
  for k in CROSSING:
    if k in got:
      assert np.array_equal(got[k], ref[k]), (tag, k, int((got[k] != ref[k]).sum()))
  if 'cross_count' in got:
    hit = got['cross_row'][got['cross_row'] >= 0]
    assert np.array_equal(got['cross_count'], np.bincount(hit, minlength=R)), (tag, 'cross_count')
  return ref


@pytest.mark.parametrize('kind', ['sizes', 'half'])
@pytest.mark.parametrize('obs', ['NORMAL', 'NB', 'ZINB'])
def test_mixed_and_crossing_tiles(obs, kind):
  """Tiles inside one group, mixed tiles and groups that cross tile edges; the rows of every group in a random order
  (time is position order, not row order).  The level of a group is half the median of its reference totals.  A few rows
  carry a NaN location: every model draws NaN there, which makes every later running total of the group NaN."""
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
  assert np.isnan(x[:, nan_rows]).all() and np.isnan(x).sum() == n * len(np.unique(nan_rows))
  level = _half_median_level(Cu.group_cumulative(x, off, rows)['total'])
  call = lambda **kw: _host(eng.predictive_group_cumulative(loc_d, aux_d, off, rows, n, 42, **kw))
  got = call(level=level, running=True)
  again = call(level=level, running=True)
  bare = call(level=level, per_row=False)
  plain = call()
  sums = eng.predictive_group_sums(loc_d, aux_d, off, rows, n, 42).cpu().numpy()
  eng.close()
  assert set(got) == {'total', 'running'} | set(CROSSING) and set(bare) == {'total', 'cross_step', 'cross_row'}
  assert set(plain) == {'total'}
  ref = _check(f'{obs} {kind}', obs, got, x, off, rows, level)
  crossed = got['cross_row'] >= 0
  print(f'{obs} {kind}: {G} groups, {int(crossed.sum())} of {crossed.size} (path, group) cross, '
        f'{int(np.isnan(got["running"]).sum())} NaN running totals')
  assert crossed.sum() > crossed.size // 4 and (~crossed).sum() > 0
  # the participating positions from the crossing one on, over all (path, group): what above_count would sum to if a
  # running total stayed above its level once it is there
  size = np.where(np.diff(off) > 0, ref['steps'][np.maximum(np.asarray(off[1:]) - 1, 0)], 0)
  after = int((size[None, :] - got['cross_step'])[crossed].sum())
  assert np.isnan(got['total'][:, big]).all() and np.isnan(got['running']).sum() > n * 4
  if obs == 'NORMAL':
    assert 0 < got['above_count'].sum() < after, 'NORMAL: running totals come back under the level (or turn NaN)'
  else:
    # in the groups without a NaN row; those with one are held to the reference above, cell by cell
    clean = ~np.isin(np.arange(G), codes[nan_rows])
    after_clean = int((size[None, :] - got['cross_step'])[crossed & clean[None, :]].sum())
    assert clean.sum() >= G - 3 and 0 < after_clean <= after
    assert got['above_count'][clean[codes]].sum() == after_clean, 'counts: a running total never comes back'
    assert got['above_count'][~clean[codes]].sum() <= after - after_clean, 'a NaN running total is not above its level'
    assert np.array_equal(got['total'], sums, equal_nan=True), 'total against predictive_group_sums'
    assert np.array_equal(np.isnan(sums), np.broadcast_to(~clean, (n, G))), 'the totals of the groups with a NaN row'
  for k in got:
    assert _same(got[k], again[k]), ('two runs differ', k)
  for k in bare:
    assert _same(got[k], bare[k]), ('running / per_row change the matrices', k)
  assert _same(got['total'], plain['total']), 'the level changes the totals'


def test_scripted_groups():
  """NB, the four members made one (so that the paths differ by the observation noise alone and the running totals of
  all paths stay close): the levels are set between the running totals of two positions, so where a path crosses follows
  from the structure.  Seven groups on one position axis (tile = 1024 positions):
    A  positions 0 .. 2047 (2 tiles): crosses in its second tile, found by the block of tile 0 walking on
    F  500 positions: filler, so that B starts mid-tile
    B  2548 .. 6043: starts mid-tile in tile 2 and runs over the tiles 3, 4 and 5; crosses in tile 5, so the carry (sum,
       steps, not yet crossed) goes over more than one tile
    C  300 positions, level 1e300: never crosses, censored at its size; the block of tile 5 skips B's positions
    D  50 positions, level -1, first entry of seg_rows -1: the first participating position crosses, step 0
    E  empty: 0, censored 0, -1
    H  100 positions with entries of -1 before the crossing and where it would have been: not steps, the run is carried"""
  eng, _ = _engine('NB')
  M, n = 4, 3
  sizes = [2 * TILE, 500, 3 * TILE + 424, 300, 50, 0, 100]
  off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
  R, G = int(off[-1]), len(sizes)
  a, f, b, c, d, e, h = (int(v) for v in off[:7])
  assert b == 2548 and off[3] == 6044
  rng = np.random.default_rng(2)
  table_rows = rng.permutation(R).astype(np.int32)        # the table row of every position: not the position itself
  loc, aux = _mixed_inputs('NB', M, R, 4)
  loc[:], aux[:] = loc[3], aux[3]                          # total_count 60: the least spread
  loc_d, aux_d = _dev(eng, loc), _dev(eng, aux)
  x = eng.predictive_samples(loc_d, aux_d, n, seed=1).cpu().numpy()
  rows = table_rows.copy()
  rows[d] = -1
  rows[[h + 3, h + 20, h + 21]] = -1
  # H: find the crossing without the entries of -1 at a level between two running totals, then take its position out
  between = lambda run, lo, hi: 0.5 * (run[:, lo].max() + run[:, hi].min())
  free = Cu.group_cumulative(x, off, rows)['running']
  level = np.zeros(G)
  level[6] = between(free, h + 40, h + 60)
  first = Cu.group_cumulative(x, off, rows, level)
  at = int(np.flatnonzero(rows == first['cross_row'][0, 6])[0])
  assert h + 40 < at <= h + 60
  rows[at] = -1                                            # where path 0 would have crossed
  run = Cu.group_cumulative(x, off, rows)['running']
  level[0] = between(run, a + TILE - 1, a + 2 * TILE - 1)
  level[1] = between(run, f + 100, f + 400)
  level[2] = between(run, 5 * TILE - 1, int(off[3]) - 1)
  level[3], level[4], level[5] = HUGE, -1.0, 0.0
  assert run[:, a + TILE - 1].max() < level[0] < run[:, a + 2 * TILE - 1].min()
  assert run[:, 5 * TILE - 1].max() < level[2] < run[:, int(off[3]) - 1].min()
  assert run[:, h + 40].max() < level[6] < run[:, h + 60].min()
  got = _host(eng.predictive_group_cumulative(loc_d, aux_d, off, rows, n, 1, level=level, running=True))
  eng.close()
  ref = _check('scripted', 'NB', got, x, off, rows, level)
  pos_of = {int(r): p for p, r in enumerate(rows) if r >= 0}
  where = np.vectorize(lambda r: pos_of.get(int(r), -1))(got['cross_row'])
  part_before = lambda p, g: int((rows[int(off[g]):p] >= 0).sum())
  for s in range(n):
    assert a + TILE <= where[s, 0] < a + 2 * TILE and got['cross_step'][s, 0] == where[s, 0] - a
    assert 5 * TILE <= where[s, 2] < off[3] and got['cross_step'][s, 2] == where[s, 2] - b > 2 * TILE
    assert got['cross_step'][s, 3] == 300.0 and got['cross_row'][s, 3] == -1
    assert got['cross_step'][s, 4] == 0.0 and got['cross_row'][s, 4] == table_rows[d + 1]
    assert got['total'][s, 5] == 0.0 and got['cross_step'][s, 5] == 0.0 and got['cross_row'][s, 5] == -1
    assert h + 40 < where[s, 6] <= h + 60 and where[s, 6] != at
    assert got['cross_step'][s, 6] == part_before(where[s, 6], 6) < where[s, 6] - h
  # an entry of -1 carries the run: the position after it adds one draw to the run before it
  assert np.array_equal(got['running'][:, d], np.zeros(n)) and np.array_equal(got['running'][:, h + 3], got['running'][:, h + 2])
  assert np.array_equal(got['running'][:, at], got['running'][:, at - 1]) and np.array_equal(got['running'], ref['running'])
  assert got['cross_count'].sum() == 5 * n and got['above_count'][table_rows[c:c + 300]].sum() == 0


@pytest.mark.parametrize('obs', ['NORMAL', 'NB'])
def test_one_group_over_66_tiles_and_shifted(obs):
  """One group over 66 tiles and a piece, finished by the block of tile 0 walking over 66 further tiles, and the same
  shifted by a leading singleton, so the tile edges fall elsewhere in the group.  Counts exact; NORMAL within the bound
  (the order of its additions follows the tiling: the two layouts need not agree bit for bit)."""
  eng, _ = _engine(obs)
  M, R, n = 4, 66 * TILE + 5, 4
  loc, aux = _mixed_inputs(obs, M, R, 3)
  rng = np.random.default_rng(6)
  order = rng.permutation(R)
  codes = np.zeros(R, dtype=np.int64)
  codes[700] = 1                                       # the singleton's position comes last: the big group starts at 0
  off, rows = inference.csr_ordered(codes, 2, order)
  off2, rows2 = inference.csr_ordered(1 - codes, 2, order)            # the singleton in front
  loc_d, aux_d = _dev(eng, loc), _dev(eng, aux)
  x = eng.predictive_samples(loc_d, aux_d, n, seed=9).cpu().numpy()
  level = _half_median_level(Cu.group_cumulative(x, off, rows)['total'])
  got = _host(eng.predictive_group_cumulative(loc_d, aux_d, off, rows, n, 9, level=level, running=True))
  got2 = _host(eng.predictive_group_cumulative(loc_d, aux_d, off2, rows2, n, 9, level=level[::-1].copy(), running=True))
  eng.close()
  _check(f'{obs} 66 tiles', obs, got, x, off, rows, level)
  _check(f'{obs} 66 tiles, shifted', obs, got2, x, off2, rows2, level[::-1].copy())
  if obs == 'NB':
    assert np.array_equal(got['cross_step'][:, 0], got2['cross_step'][:, 1]) and got['cross_step'][:, 0].min() > TILE
    assert np.array_equal(got['running'][:, :R - 1], got2['running'][:, 1:])


@pytest.mark.parametrize('obs', ['NORMAL', 'ZINB'])
def test_invariance_bit_for_bit(obs):
  """The bits of every output depend on the seed, the path, the rows and the CSR arrays only: sample0 chunks, row0
  against the column slice, the outputs asked for, a second run, and a launch that strides its blocks over several paths.
  The launch takes grid.y = min(paths, 65535, max(16384 / tiles, ceil(2048 / min(tiles, groups)))): 3 tiles and 6 groups
  give 5461, so the call of 5470 paths strides 9 blocks over two paths each."""
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
  level = _half_median_level(Cu.group_cumulative(x, off, rows)['total'])
  call = lambda n_, **kw: _host(eng.predictive_group_cumulative(loc_d, aux_d, off, rows, n_, 5, level=level, **kw))
  full = call(n, running=True)
  _check(f'{obs} one call', obs, full, x, off, rows, level)
  # (a) two calls of 8 paths give the rows of the one call of 16; their per-row counters add up
  halves = [call(8, running=True, sample0=s0) for s0 in (0, 8)]
  for k in ('total', 'running', 'cross_step', 'cross_row'):
    assert _same(np.concatenate([halves[0][k], halves[1][k]]), full[k]), ('sample0', k)
  for k in ('cross_count', 'above_count'):
    assert np.array_equal(halves[0][k] + halves[1][k], full[k]), ('sample0', k)
  # (b) more paths than grid.y: blocks stride over the paths; the first 16 are those of the call of 16, and two halves
  # with sample0 give the same matrices
  big_n = 16384 // 3 + 9
  big = call(big_n)
  for k in ('total', 'cross_step', 'cross_row'):
    assert _same(big[k][:n], full[k]), ('strided', k)
  parts = [call(big_n // 2, sample0=s0) for s0 in (0, big_n // 2)]
  for k in ('total', 'cross_step', 'cross_row'):
    assert _same(np.concatenate([parts[0][k], parts[1][k]]), big[k]), ('strided, sample0', k)
  for k in ('cross_count', 'above_count'):
    assert np.array_equal(parts[0][k] + parts[1][k], big[k]), ('strided, sample0', k)
  if obs == 'ZINB':
    sums = eng.predictive_group_sums(loc_d, aux_d, off, rows, big_n, 5).cpu().numpy()
    assert np.array_equal(big['total'], sums)
  # (c) row0: the columns a .. b of the table as a table of their own.  Their groups come first on the position axis of
  # the whole table's layout below, so every group lies where it lies in the slice's own layout
  lo, hi = 300, 300 + TILE + 200
  sub_sizes = [700, 1, 523]
  sub_codes = rng.permutation(np.repeat(np.arange(3), sub_sizes))
  sub_off, sub_rows = inference.csr_ordered(sub_codes, 3, rng.permutation(hi - lo))
  rest = np.concatenate([np.arange(lo), np.arange(hi, R)])
  whole_off = np.concatenate([sub_off, [R]]).astype(np.int32)
  whole_rows = np.concatenate([sub_rows + lo, rng.permutation(rest)]).astype(np.int32)
  lvl4 = np.asarray([level[0], level[2], level[1], level[4]])
  whole = _host(eng.predictive_group_cumulative(loc_d, aux_d, whole_off, whole_rows, n, 5, level=lvl4, running=True))
  part = _host(eng.predictive_group_cumulative(loc_d[:, lo:hi].contiguous(), aux_d, sub_off, sub_rows, n, 5, level=lvl4[:3],
                                               running=True, row0=lo))
  for k in ('total', 'cross_step'):
    assert _same(part[k], whole[k][:, :3]), ('row0', k)
  assert _same(part['running'], whole['running'][:, :hi - lo]), ('row0', 'running')
  assert np.array_equal(np.where(part['cross_row'] >= 0, part['cross_row'] + lo, -1), whole['cross_row'][:, :3])
  assert np.array_equal(part['cross_count'], whole['cross_count'][lo:hi]) and np.array_equal(part['above_count'], whole['above_count'][lo:hi])
  # (d) weights wholly on one member: that member's M = 1 result; NULL weights: the unweighted call
  for m in (0, 2):
    cum = np.cumsum(np.eye(M)[m])
    one = call(n, running=True, cum_weights=cum)
    alone = _host(eng.predictive_group_cumulative(loc_d[m:m + 1], aux_d[m:m + 1], off, rows, n, 5, level=level, running=True))
    for k in one:
      assert _same(one[k], alone[k]), ('one member', m, k)
  none = call(n, running=True, cum_weights=None)
  for k in full:
    assert _same(none[k], full[k]), ('NULL weights', k)
  # general weights: the reference on the weighted draws
  cum = np.cumsum([0.4, 0.1, 0.2, 0.3])
  cum[-1] = 1.0
  xw = eng.predictive_samples(loc_d, aux_d, n, seed=5, cum_weights=cum).cpu().numpy()
  lvl_w = _half_median_level(Cu.group_cumulative(xw, off, rows)['total'])
  wgt = _host(eng.predictive_group_cumulative(loc_d, aux_d, off, rows, n, 5, level=lvl_w, running=True, cum_weights=cum))
  eng.close()
  _check(f'{obs} weighted', obs, wgt, xw, off, rows, lvl_w)
  assert not np.array_equal(wgt['total'], full['total'])


def test_errors_write_nothing():
  """BNF_ERR_INVALID for a NULL out_total and for every crossing output without a level; the outputs keep their bytes."""
  eng, _ = _engine('NB')
  M, R, n, G = 4, 300, 2, 3
  loc, aux = _mixed_inputs('NB', M, R, 1)
  loc_d, aux_d = _dev(eng, loc), _dev(eng, aux)
  dev = eng.device
  off_d = torch.tensor([0, 100, 100, 300], dtype=torch.int32, device=dev)
  rows_d = torch.arange(R, dtype=torch.int32, device=dev)
  lvl_d = torch.zeros(G, dtype=torch.float64, device=dev)
  out = {'total': torch.full((n, G), 7.0, dtype=torch.float64, device=dev),
         'running': torch.full((n, R), 7.0, dtype=torch.float64, device=dev),
         'cross_step': torch.full((n, G), 7.0, dtype=torch.float64, device=dev),
         'cross_row': torch.full((n, G), 7, dtype=torch.int32, device=dev),
         'cross_count': torch.full((R,), 7, dtype=torch.int32, device=dev),
         'above_count': torch.full((R,), 7, dtype=torch.int32, device=dev)}
  p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
  names = ('total', 'running', 'cross_step', 'cross_row', 'cross_count', 'above_count')

  def call(level, **given):
    ptrs = [p(given.get(k)) for k in names]
    return eng.lib.bnf_predictive_group_cumulative(eng.handle, p(loc_d), p(aux_d), M, R, p(off_d), p(rows_d), G, n,
                                                   C.c_uint64(3), 0, 0, None, p(level), *ptrs)

  assert call(lvl_d, **{k: v for k, v in out.items() if k != 'total'}) == -1 and 'out_total' in _native.last_error()
  for k in CROSSING:
    assert call(None, total=out['total'], running=out['running'], **{k: out[k]}) == -1, k
    assert 'level' in _native.last_error()
  torch.cuda.synchronize()
  for k, v in out.items():
    assert torch.all(v == 7), ('written by a refused call', k)
  # the smallest valid call: a total alone; then everything, on the same buffers
  assert call(None, total=out['total']) == 0, _native.last_error()
  torch.cuda.synchronize()
  only_total = out['total'].cpu().numpy().copy()
  out['cross_count'].zero_()
  out['above_count'].zero_()
  assert call(lvl_d, **out) == 0, _native.last_error()
  torch.cuda.synchronize()
  x = eng.predictive_samples(loc_d, aux_d, n, seed=3).cpu().numpy()
  got = _host(out)
  eng.close()
  assert _same(got['total'], only_total)
  _check('raw call', 'NB', got, x, np.asarray([0, 100, 100, 300]), np.arange(R), np.zeros(G))


def _summary_check(tag, have, m, y, levels, delta):
  """`have` (mean, quantiles, crps, pit) against numpy and the helpers of tests/totals_ref.py on the host matrix m (S, C),
  at the bars of that file; delta (C,) >= the largest difference between a cell of the device matrix and of m (0 for
  counts: exact).  Mean and 'linear' quantiles move by at most delta with their inputs, the CRPS by at most 2 delta."""
  clean = ~np.isnan(m).any(axis=0)
  scored = clean & np.isfinite(y)
  assert np.isnan(have['mean'][~clean]).all() and np.isnan(have['crps'][~scored]).all(), (tag, 'NaN pattern')
  mc, yc = m[:, clean], y[clean]
  assert np.all(np.abs(have['mean'][clean] - mc.mean(axis=0)) <= T.mean_bars(mc) + delta[clean]), (tag, 'mean')
  assert np.all(np.abs(have['quantiles'][:, clean] - T.quantiles_ref(mc, levels)) <= T.quantile_bars(mc, levels) + delta[clean]), (tag, 'quantiles')
  ms, ys, ds = m[:, scored], y[scored], delta[scored]
  assert np.all(np.abs(have['crps'][scored] - T.crps_ref(ms, ys)) <= T.crps_bars(ms, ys) + 2 * ds), (tag, 'crps')
  assert np.all(np.abs(ms - ys[None, :]).min(axis=0) > ds) or np.all(ds == 0), (tag, 'an observed value within delta of a path')
  assert np.array_equal(have['pit'][:, scored], T.pit_ref(ms, ys)), (tag, 'pit')


@pytest.mark.parametrize('kind', ['map', 'vi'])
def test_estimator_cumulative_end_to_end(golden_dir, kind):
  """chickenpox fixture (NB for MAP, NORMAL for VI) with its rows SHUFFLED: predict_cumulative / score_cumulative against
  the same quantities formed on the host from predict_samples(table, S, seed) with the time ordering applied there:
  np.cumsum, np.quantile on the cumulative sums, CRPS and PIT from tests/totals_ref.py.  NB: the per-row shares, 'never',
  the observed columns and the means are exact (integers below 2^53 add without rounding), the rest at the bars of
  tests/totals_ref.py.  NORMAL: the same bars plus the summation bound of the module docstring."""
  df, est = _fit(golden_dir, kind)
  df = df.assign(year=df['datetime'].dt.year).sample(frac=1.0, random_state=4).reset_index(drop=True)
  assert not df['datetime'].is_monotonic_increasing
  S, seed, levels = 300, 3, (0.025, 0.5, 0.975)
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
    lvl = _half_median_level(Cu.group_cumulative(x, off, rows)['total'])
    ref = Cu.group_cumulative(x, off, rows, lvl)
    by_row = np.empty(R, dtype=np.int64)
    by_row[rows] = np.arange(R)                              # the position of every table row
    run_rows = ref['running'][:, by_row]                     # (S, R) per table row
    delta_pos = np.zeros(R) if exact else Cu.normal_bound(x, off, rows).max(axis=0)
    delta_row, delta_g = delta_pos[by_row], delta_pos[off[1:] - 1]
    res = est.score_cumulative(df, by, level=lvl[codes], quantiles=levels, num_samples=S, seed=seed)
    assert list(res['keys']) == list(keys) and res['n'] == G
    obs = spatiotemporal.group_target_cumulative(y, off, rows, lvl)
    for g in range(G):                                       # the observed columns once more, by hand
      r = rows[off[g]:off[g + 1]]
      run = np.cumsum(y[r])
      hit = np.flatnonzero(run > lvl[g])
      assert np.array_equal(obs['running'][r], run) and obs['total'][g] == run[-1]
      assert obs['cross_step'][g] == (hit[0] if hit.size else len(r)) and obs['cross_row'][g] == (r[hit[0]] if hit.size else -1)
    assert np.array_equal(res['observed_total'], obs['total']) and np.array_equal(res['observed_running'], obs['running'])
    assert np.array_equal(res['observed_crossing_step'], obs['cross_step'])
    assert np.array_equal(res['observed_crossing_row'], obs['cross_row'])
    if not exact:                                            # no reference running total within the bound of its level
      assert np.all(np.abs(ref['running'] - np.repeat(lvl, np.diff(off))[None, :]) > Cu.normal_bound(x, off, rows))
    assert np.array_equal(res['crossing_probability'], ref['cross_count'] / S)
    assert np.array_equal(res['above_probability'], ref['above_count'] / S)
    assert np.array_equal(res['never'], (ref['cross_row'] < 0).sum(axis=0) / S)
    # never = 1 - the group's sum of crossing_probability, exactly, as counts
    counts = np.rint(res['crossing_probability'] * S).astype(np.int64)
    assert np.array_equal(np.rint(res['never'] * S).astype(np.int64),
                          S - np.bincount(codes, weights=counts, minlength=G).astype(np.int64))
    want_p = np.where(obs['cross_row'] >= 0, res['crossing_probability'][np.maximum(obs['cross_row'], 0)], res['never'])
    assert np.array_equal(res['crossing_row_probability'], want_p)
    if exact:
      assert np.array_equal(res['total_mean'], ref['total'].sum(axis=0) / S)
      assert np.array_equal(res['running_mean'], run_rows.sum(axis=0) / S)
      assert np.array_equal(res['crossing_step_mean'], ref['cross_step'].sum(axis=0) / S)
    for name, out, m, yy, dl in (('total', 'total', ref['total'], obs['total'], delta_g),
                                 ('cross_step', 'crossing_step', ref['cross_step'], obs['cross_step'], np.zeros(G)),
                                 ('running', 'running', run_rows, obs['running'], delta_row)):
      have = dict(mean=res[f'{out}_mean'], quantiles=res[f'{out}_quantiles'], crps=res[f'{out}_crps'], pit=res[f'{out}_pit'])
      _summary_check(f'{kind} by {by}: {name}', have, m, yy, levels, dl)
      assert res[f'mean_{out}_crps'] == float(np.mean(res[f'{out}_crps'], dtype=np.float64))
    # the band of the running total at a group's last row is the band of the total
    last_rows = rows[off[1:] - 1]
    assert _same(res['running_quantiles'][:, last_rows], res['total_quantiles'])
    assert _same(res['running_mean'][last_rows], res['total_mean'])
    print(f'{kind} by {by}: observed total {obs["total"]}, forecast mean {res["total_mean"]}, crossing step '
          f'{res["crossing_step_mean"]} (observed {obs["cross_step"]}), never {res["never"]}, '
          f'P(observed crossing row) {res["crossing_row_probability"]}')
    pred = est.predict_cumulative(df, by, level=lvl[codes], quantiles=levels, num_samples=S, seed=seed)
    assert set(pred) == {'keys', 'total_mean', 'total_quantiles', 'running_mean', 'running_quantiles', 'crossing_step_mean',
                         'crossing_step_quantiles', 'crossing_probability', 'above_probability', 'never'}
    for k in set(pred) - {'keys'}:
      assert _same(pred[k], res[k]), k
  # curve=False and no level: the totals alone, the same bits; a scalar level and another ordering column
  bare = est.predict_cumulative(df, 'year', curve=False, quantiles=levels, num_samples=S, seed=seed)
  assert set(bare) == {'keys', 'total_mean', 'total_quantiles'} and _same(bare['total_mean'], pred['total_mean'])
  flat = est.predict_cumulative(df, 'year', level=float(lvl.mean()), order_by='chickenpox', num_samples=S, seed=seed)
  rows = df.assign(_g=codes).sort_values(['_g', 'chickenpox'], kind='stable').index.to_numpy()
  ref2 = Cu.group_cumulative(x, off, rows, np.full(G, float(lvl.mean())))
  if exact:
    assert np.array_equal(flat['crossing_probability'], ref2['cross_count'] / S)
    assert np.array_equal(flat['above_probability'], ref2['above_count'] / S)
  assert flat['running_quantiles'].shape == (1, R) and flat['crossing_step_quantiles'].shape == (1, G)
  # a group with a NaN target row is not scored; the forecast does not change
  d = df.copy()
  d.loc[d.index[[1]], 'chickenpox'] = np.nan
  res2 = est.score_cumulative(d, 'year', level=lvl[codes], quantiles=levels, num_samples=S, seed=seed)
  gone = codes[1]
  assert res2['n'] == G - 1 and np.isnan(res2['observed_total'][gone]) and res2['observed_crossing_row'][gone] == -1
  for k in ('total_crps', 'crossing_step_crps', 'crossing_row_probability'):
    assert np.array_equal(np.isnan(res2[k]), np.arange(G) == gone), k
  assert _same(res2['total_mean'], res['total_mean']) and _same(res2['crossing_probability'], res['crossing_probability'])
  # weights are passed through: all weight on one member gives another forecast than equal weights, the same twice
  w = np.zeros(np.shape(est.params_[0])[:est._ensemble_dims])
  w.flat[0] = 1.0
  one = est.predict_cumulative(df, 'year', level=lvl[codes], num_samples=S, seed=seed, weights=w)
  xw = est.predict_samples(df, S, seed, weights=w)
  refw = Cu.group_cumulative(xw, off, df.assign(_g=codes).sort_values(['_g', 'datetime'], kind='stable').index.to_numpy(), lvl)
  if exact:
    assert np.array_equal(one['total_mean'], refw['total'].sum(axis=0) / S)
    assert np.array_equal(one['crossing_probability'], refw['cross_count'] / S)
  assert not _same(one['total_mean'], res['total_mean'])
