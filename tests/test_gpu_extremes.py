"""Group peaks and threshold exceedances of the sample paths on the GPU (include/bnf.h bnf_predictive_group_extremes)
against numpy on `Engine.predictive_samples` for the same seed (tests/extremes_ref.py).  Every comparison of max, argmax
and the counts is EXACT, for NORMAL, NB and ZINB alike: none of them rounds.  The engine-level tests use synthetic
loc / aux on a forward-only engine, as tests/test_gpu_sampling.py does."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from bayesnf_amd import _native, inference
from oracle import bnf_oracle as O
from tests import extremes_ref as X
from tests import totals_ref as T
from tests.test_gpu_sampling import PI, _dev, _engine, _fit, _mixed_inputs, dkw_eps, inv_softplus

pytestmark = pytest.mark.gpu

TILE = 1024


def _bits(a):
  a = np.ascontiguousarray(a)
  return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _same(a, b):
  return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _host(res):
  return {k: v.cpu().numpy() for k, v in res.items()}


def _check(tag, got, ref, codes, G):
  """Exact equality of everything `got` holds with the reference; empty groups (NaN, -1, 0)."""
  assert np.array_equal(got['max'], ref['max'], equal_nan=True), (tag, 'max')
  assert got['argmax'].dtype == np.int32 and np.array_equal(got['argmax'], ref['argmax']), (tag, 'argmax')
  empty = np.bincount(codes, minlength=G)[:G] == 0
  assert np.isnan(got['max'][:, empty]).all() and np.all(got['argmax'][:, empty] == -1), (tag, 'empty groups')
  assert not np.isnan(got['max'][:, ~empty]).any(), (tag, 'NaN in a group with rows')
  if 'peak_count' in got:
    hit = got['argmax'][got['argmax'] >= 0]
    assert np.array_equal(got['peak_count'], np.bincount(hit, minlength=len(got['peak_count']))), (tag, 'peak_count')
    assert np.array_equal(got['peak_count'], ref['peak_count']), (tag, 'peak_count against the host')
  if 'count' in ref:
    assert np.array_equal(got['count'], ref['count']) and np.all(got['count'][:, empty] == 0.0), (tag, 'count')
    if 'exceed_count' in got:
      assert np.array_equal(got['exceed_count'], ref['exceed_count']), (tag, 'exceed_count')
  else:
    assert 'count' not in got and 'exceed_count' not in got, (tag, 'count without a threshold')


def _grouping(kind, R, rng):
  """'sizes': singletons, the sizes 2, 3, 7, 300, 1023 and 1024 (segment edges on and off the tile edges) and three
  empty groups; 'half': one group of half the rows that crosses a tile edge, beside 1, 300, 1023, 7, 3 and three empty
  groups.  (Both lists do not fit into 3 * 1024 + 37 rows at once.)  Rows in random order."""
  sizes = {'sizes': [1024, 1, 1023, 3, 0, 2, 7, 300, 0, 1, 1, 0], 'half': [R // 2, 0, 1, 300, 1023, 0, 7, 0, 3]}[kind]
  menu = [1, 1, 1, 2, 3, 7, 40]
  while sum(sizes) < R:
    sizes.append(min(int(rng.choice(menu)), R - sum(sizes)))
  codes = np.repeat(np.arange(len(sizes)), sizes)
  assert len(codes) == R and sizes.count(0) == 3
  return rng.permutation(codes), len(sizes)


@pytest.mark.parametrize('kind', ['sizes', 'half'])
@pytest.mark.parametrize('obs', ['NORMAL', 'NB', 'ZINB'])
def test_mixed_and_crossing_tiles(obs, kind):
  """Tiles inside one group, mixed tiles and groups that cross tile edges, with a threshold per row and without one.
  The threshold is path 0's own draw: that path never exceeds it (strict >), the others do about half the time.  A few
  rows carry a NaN location (one whole group of 3 among them): NORMAL draws NaN there, which must count as -inf."""
  eng, _ = _engine(obs)
  M, R, n = 4, 3 * TILE + 37, 16
  rng = np.random.default_rng(5)
  loc, aux = _mixed_inputs(obs, M, R, 21)
  codes, G = _grouping(kind, R, rng)
  three = np.flatnonzero(codes == int(np.flatnonzero(np.bincount(codes, minlength=G) == 3)[0]))
  loc[:, np.concatenate([three, np.flatnonzero(codes == 0)[[0, 5]], [7, 2048]])] = np.nan
  off, rows = inference.csr_from_codes(codes, G)
  loc_d, aux_d = _dev(eng, loc), _dev(eng, aux)
  x = eng.predictive_samples(loc_d, aux_d, n, seed=42).cpu().numpy()
  assert obs != 'NORMAL' or np.isnan(x[:, three]).all()
  thr = np.where(np.isnan(x[0]), 0.0, x[0]).astype(np.float32)
  got = _host(eng.predictive_group_extremes(loc_d, aux_d, off, rows, n, seed=42, threshold=thr))
  again = _host(eng.predictive_group_extremes(loc_d, aux_d, off, rows, n, seed=42, threshold=thr))
  plain = _host(eng.predictive_group_extremes(loc_d, aux_d, off, rows, n, seed=42))
  bare = _host(eng.predictive_group_extremes(loc_d, aux_d, off, rows, n, seed=42, threshold=thr, per_row=False))
  eng.close()
  assert set(got) == {'max', 'argmax', 'count', 'peak_count', 'exceed_count'} and set(plain) == {'max', 'argmax', 'peak_count'}
  assert set(bare) == {'max', 'argmax', 'count'}
  assert got['max'].shape == got['argmax'].shape == got['count'].shape == (n, G) and got['max'].dtype == np.float64
  ref = X.group_extremes(x, codes, G, thr)
  share = float((got['count'] > 0).mean())
  print(f'{obs} {kind}: {G} groups, {int(np.isnan(x).sum())} NaN draws, cells with an exceedance {share:.2f}')
  _check(f'{obs} {kind}', got, ref, codes, G)
  _check(f'{obs} {kind} no threshold', plain, X.group_extremes(x, codes, G), codes, G)
  assert np.all(got['count'][0] == 0.0) and 0.05 < share < 1.0
  if obs == 'NORMAL':
    g3 = codes[three[0]]
    assert np.all(got['max'][:, g3] == -np.inf) and np.all(got['argmax'][:, g3] == three.min())
  for k in got:
    assert _same(got[k], again[k]), ('two runs differ', k)
  for k in bare:
    assert _same(got[k], bare[k]), ('per_row changes the matrices', k)
  assert _same(got['max'], plain['max']) and _same(got['argmax'], plain['argmax'])


@pytest.mark.parametrize('obs', ['NORMAL', 'NB'])
def test_more_than_64_tiles_in_one_group(obs):
  """One group over 66 tiles and a piece: the combine pass strides its 64 lanes over the tiles."""
  eng, _ = _engine(obs)
  M, R, n = 4, 66 * TILE + 5, 4
  loc, aux = _mixed_inputs(obs, M, R, 3)
  codes = np.zeros(R, dtype=np.int64)
  codes[700] = 1                                       # the singleton's position comes last: the big group starts at 0
  off, rows = inference.csr_from_codes(codes, 2)
  loc_d, aux_d = _dev(eng, loc), _dev(eng, aux)
  x = eng.predictive_samples(loc_d, aux_d, n, seed=9).cpu().numpy()
  thr = np.quantile(x, 0.9, axis=0).astype(np.float32)
  got = _host(eng.predictive_group_extremes(loc_d, aux_d, off, rows, n, seed=9, threshold=thr))
  # the same with the singleton in front: the big group starts one position into tile 0 and ends in tile 66
  codes2 = 1 - codes
  off2, rows2 = inference.csr_from_codes(codes2, 2)
  got2 = _host(eng.predictive_group_extremes(loc_d, aux_d, off2, rows2, n, seed=9, threshold=thr))
  eng.close()
  _check(f'{obs} 66 tiles', got, X.group_extremes(x, codes, 2, thr), codes, 2)
  _check(f'{obs} 66 tiles, shifted', got2, X.group_extremes(x, codes2, 2, thr), codes2, 2)
  assert got['count'][:, 0].min() > 64                 # pieces of many tiles were added up


def test_ties_go_to_the_lowest_table_row():
  """NB with a mean of 0.02 .. 0.05 per row: most draws are 0, the peak of a group is 0, 1 or 2 and is reached at many
  rows, in small groups at all of them.  Group sizes straddle the tile edges."""
  eng, _ = _engine('NB')
  M, R, n = 3, 2 * TILE + 300, 16
  rng = np.random.default_rng(8)
  tcs = np.asarray([0.5, 1.0, 4.0])
  means = rng.uniform(0.02, 0.05, (M, R))
  loc = inv_softplus(tcs[:, None] ** 2 / means).astype(np.float32)
  aux = np.stack([np.ones(M), 1.0 / tcs, np.full(M, PI)], axis=1).astype(np.float32)
  sizes = [1000, 48, 3, 1, 0, 990, 12, 2, 20, 272]       # 1000 + 48 crosses position 1024; 990 + ... crosses 2048
  assert sum(sizes) == R
  codes = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
  G = len(sizes)
  off, rows = inference.csr_from_codes(codes, G)
  loc_d, aux_d = _dev(eng, loc), _dev(eng, aux)
  x = eng.predictive_samples(loc_d, aux_d, n, seed=77).cpu().numpy()
  got = _host(eng.predictive_group_extremes(loc_d, aux_d, off, rows, n, seed=77, threshold=np.zeros(R, dtype=np.float32)))
  eng.close()
  share = X.tie_share(x, codes, G)
  print(f'ties: {share:.2f} of the (path, group) cells reach their maximum at more than one row; mean draw {x.mean():.4f}')
  assert share >= 0.25, share
  ref = X.group_extremes(x, codes, G, np.zeros(R, dtype=np.float32))
  _check('ties', got, ref, codes, G)
  for g in range(G):                                   # said once more without np.argmax: the lowest row of the tied set
    members = np.flatnonzero(codes == g)
    for s in range(n):
      if members.size:
        tied = members[x[s, members] == x[s, members].max()]
        assert got['argmax'][s, g] == tied.min(), (s, g)


def _raw_call(eng, loc_d, aux_d, off, rows, n, seed, thr, work_paths, sample0=0):
  """The C entry point with a work buffer of `work_paths` paths' worth: ceil(n / work_paths) passes."""
  M, R = loc_d.shape
  G = len(off) - 1
  dev = eng.device
  off_d, rows_d = torch.from_numpy(off).to(dev), torch.from_numpy(rows).to(dev)
  thr_d = torch.from_numpy(thr).to(dev)
  per_path = _native.EXTREMES_WORK_PER_TILE * (-(-R // TILE))
  work = torch.empty(per_path * work_paths, dtype=torch.uint8, device=dev)
  out = {'max': torch.empty((n, G), dtype=torch.float64, device=dev), 'argmax': torch.empty((n, G), dtype=torch.int32, device=dev),
         'count': torch.empty((n, G), dtype=torch.float64, device=dev), 'peak_count': torch.zeros(R, dtype=torch.int32, device=dev),
         'exceed_count': torch.zeros(R, dtype=torch.int32, device=dev)}
  p = lambda t: C.c_void_p(t.data_ptr())
  call = lambda nbytes: eng.lib.bnf_predictive_group_extremes(
      eng.handle, p(loc_d), p(aux_d), M, R, p(off_d), p(rows_d), G, n, C.c_uint64(seed), 0, sample0, None, p(thr_d), p(work),
      C.c_size_t(nbytes), p(out['max']), p(out['argmax']), p(out['count']), p(out['peak_count']), p(out['exceed_count']))
  assert call(per_path - 1) == -1 and 'work buffer' in _native.last_error()      # below one path's worth: BNF_ERR_INVALID
  assert call(work.numel()) == 0, _native.last_error()
  torch.cuda.synchronize()
  return _host(out)


@pytest.mark.parametrize('obs', ['NORMAL', 'ZINB'])
def test_invariance_under_passes_offsets_and_weights(obs):
  eng, _ = _engine(obs)
  M, R, n = 4, 2 * TILE + 500, 16
  rng = np.random.default_rng(13)
  loc, aux = _mixed_inputs(obs, M, R, 11)
  sizes = [900, 200, 1, 0, 1400, 47]                    # 900 + 200 and 1400 cross the two tile edges
  codes = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
  G = len(sizes)
  off, rows = inference.csr_from_codes(codes, G)
  loc_d, aux_d = _dev(eng, loc), _dev(eng, aux)
  x = eng.predictive_samples(loc_d, aux_d, n, seed=5).cpu().numpy()
  thr = np.median(x, axis=0).astype(np.float32)
  full = _host(eng.predictive_group_extremes(loc_d, aux_d, off, rows, n, seed=5, threshold=thr))
  _check(f'{obs} one pass', full, X.group_extremes(x, codes, G, thr), codes, G)
  # (a) the samples cut by the work buffer: 16 paths through room for 5 = 4 passes
  cut = _raw_call(eng, loc_d, aux_d, off, rows, n, 5, thr, work_paths=5)
  for k in full:
    assert _same(full[k], cut[k]), ('passes', k)
  # (b) sample0: a slice of the paths; its per-row counters are those of the slice alone
  for s0, k in ((0, 1), (7, 5), (15, 1)):
    part = _host(eng.predictive_group_extremes(loc_d, aux_d, off, rows, k, seed=5, threshold=thr, sample0=s0))
    for name in ('max', 'argmax', 'count'):
      assert _same(part[name], full[name][s0:s0 + k]), ('sample0', s0, name)
    _check(f'{obs} sample0={s0}', part, X.group_extremes(x[s0:s0 + k], codes, G, thr), codes, G)
  # (c) row0: a slice of the rows, grouped on its own, is the reference on that slice of the one big draw
  for a, b in ((1, 1025), (1023, 2300), (2400, 2548)):
    sub = codes[a:b]
    keys, sub = np.unique(sub, return_inverse=True)
    o, r = inference.csr_from_codes(sub, len(keys))
    part = _host(eng.predictive_group_extremes(loc_d[:, a:b], aux_d, o, r, n, seed=5, threshold=thr[a:b], row0=a))
    _check(f'{obs} row0={a}', part, X.group_extremes(x[:, a:b], sub, len(keys), thr[a:b]), sub, len(keys))
  # (d) entries of seg_rows outside [0, R) take no part: the reference with those rows in a group of their own
  gone = np.asarray([0, 899, 900, 1023, 1024, 2547])     # CSR positions, tile edges among them
  rows_cut = rows.copy()
  rows_cut[gone] = np.asarray([-1, R, R + 7, -5, 2 ** 31 - 1, -2 ** 31], dtype=np.int64).astype(np.int32)
  codes_cut = codes.copy()
  codes_cut[rows[gone]] = G
  part = _host(eng.predictive_group_extremes(loc_d, aux_d, off, rows_cut, n, seed=5, threshold=thr))
  ref = X.group_extremes(x, codes_cut, G + 1, thr)
  ref = {k: (v[:, :G] if v.ndim == 2 else v) for k, v in ref.items()}
  ref['peak_count'][rows[gone]] = 0
  ref['exceed_count'][rows[gone]] = 0
  _check(f'{obs} rows outside the table', part, ref, codes_cut, G)
  # (e) weights wholly on one member: that member's M = 1 result
  for m in (0, 2):
    cum = np.cumsum(np.eye(M)[m])
    one = _host(eng.predictive_group_extremes(loc_d, aux_d, off, rows, n, seed=5, threshold=thr, cum_weights=cum))
    alone = _host(eng.predictive_group_extremes(loc_d[m:m + 1], aux_d[m:m + 1], off, rows, n, seed=5, threshold=thr))
    for k in one:
      assert _same(one[k], alone[k]), ('one member', m, k)
  # (f) general weights: the reference on the weighted draws; cum_weights=None: the integer floor(u M) component, which
  # equal explicit weights reproduce where k / M is exact and #{m : (m + 1) / M <= u} = floor(u M) -- M = 4 is such a case
  cum = np.cumsum([0.4, 0.1, 0.2, 0.3])
  cum[-1] = 1.0
  xw = eng.predictive_samples(loc_d, aux_d, n, seed=5, cum_weights=cum).cpu().numpy()
  wgt = _host(eng.predictive_group_extremes(loc_d, aux_d, off, rows, n, seed=5, threshold=thr, cum_weights=cum))
  _check(f'{obs} weighted', wgt, X.group_extremes(xw, codes, G, thr), codes, G)
  assert not np.array_equal(wgt['max'], full['max'], equal_nan=True)
  equal = _host(eng.predictive_group_extremes(loc_d, aux_d, off, rows, n, seed=5, threshold=thr,
                                              cum_weights=np.asarray([0.25, 0.5, 0.75, 1.0])))
  eng.close()
  for k in full:
    assert _same(full[k], equal[k]), ('equal explicit weights, M = 4', k)


@pytest.mark.parametrize('obs', ['NORMAL', 'NB', 'ZINB'])
def test_exceedance_frequency_against_the_closed_form_mixture_cdf(obs):
  """exceed_count / S on 64 rows against 1 - F(threshold), F the oracle's mixture CDF.  The S = 4096 paths are i.i.d.
  draws of the mixture at every row, so |F_n(t) - F(t)| <= dkw_eps(S) = 0.051 at any t, except with probability 1e-9 per
  row (the bound of tests/test_gpu_sampling.py: derived, not measured)."""
  eng, model = _engine(obs)
  M, R, S = 4, 64, 4096
  rng = np.random.default_rng(17)
  if obs == 'NORMAL':
    loc = (30.0 * rng.standard_normal((M, R))).astype(np.float32)
    scales = rng.uniform(0.5, 20.0, M).astype(np.float32)
    aux = np.stack([scales, np.ones(M), np.zeros(M)], axis=1).astype(np.float32)
    thr = (loc.mean(axis=0) + 10.0 * rng.standard_normal(R)).astype(np.float32)
    tail = 1.0 - O.mixture_cdf(loc.astype(np.float64), scales.astype(np.float64), thr.astype(np.float64))
  else:
    tcs = np.asarray([0.3, 1.0, 5.0, 60.0])
    means = np.exp(rng.uniform(np.log(0.05), np.log(3e3), (M, R)))
    loc = inv_softplus(tcs[:, None] ** 2 / means).astype(np.float32)
    aux = np.stack([np.ones(M), 1.0 / tcs, np.full(M, PI)], axis=1).astype(np.float32)
    theta = np.zeros((M, model.P))
    theta[:, model.leaf['shape'].offset] = inv_softplus(aux[:, 1].astype(np.float64))
    p = aux[:, 2].astype(np.float64)
    theta[:, model.leaf['inflated_loc_probs'].offset] = np.log(p) - np.log1p(-p)
    fc = O.count_forecast(model, theta, loc.astype(np.float64))
    thr = np.floor(np.exp(np.log(fc['mean']).mean(axis=0)) * rng.uniform(0.0, 2.0, R)).astype(np.float32)
    tail = 1.0 - O.count_cdf(fc, thr.astype(np.float64)[None, :]).mean(axis=0)      # P(X > k) at the integer k
  codes = np.arange(R) // 16
  off, rows = inference.csr_from_codes(codes, 4)
  res = _host(eng.predictive_group_extremes(_dev(eng, loc), _dev(eng, aux), off, rows, S, seed=2024, threshold=thr))
  eng.close()
  freq = res['exceed_count'] / S
  d = np.abs(freq - tail)
  print(f'{obs}: exceedance frequency against 1 - F(threshold): max {d.max():.4f} (eps {dkw_eps(S):.4f}); '
        f'closed-form tails span {tail.min():.3f} .. {tail.max():.3f}')
  assert tail.min() < 0.25 and tail.max() > 0.45         # the thresholds sit in the body of the laws, not beyond them
  assert np.all(d <= dkw_eps(S)), float(d.max())
  assert np.array_equal(res['count'].sum(axis=1), res['count'].sum(axis=1).round())
  assert res['count'].sum() == res['exceed_count'].sum() and res['peak_count'].sum() == 4 * S


@pytest.mark.parametrize('kind', ['map', 'vi'])
def test_estimator_extremes_end_to_end(golden_dir, kind):
  """chickenpox fixture (NB for MAP, NORMAL for VI): predict_extremes / score_extremes against the same quantities
  formed on the host from predict_samples(table, S, seed).  Exact: the per-row shares, exceed_any, the observed columns
  and the means (the counts are integers; a peak is a float32 of size >= 2^-10 here, a multiple of 2^-33, and 300 of them
  below 2^17 add up without rounding in any order).  Quantiles, CRPS and PIT: the bars of tests/totals_ref.py, as
  tests/test_gpu_totals.py applies them to the same kernel.  By 'location' (one group: the fixture holds one county) and
  by year (two groups)."""
  df, est = _fit(golden_dir, kind)
  df = df.assign(year=df['datetime'].dt.year)
  S, seed, levels = 300, 3, (0.025, 0.5, 0.975)
  R = len(df)
  x = est.predict_samples(df, S, seed)
  y = df['chickenpox'].to_numpy(dtype=np.float64)
  thr = (40.0 + 20.0 * (np.arange(R) % 3)).astype(np.float32)
  for by in ('location', 'year'):
    keys = np.sort(df[by].unique())
    codes = np.searchsorted(keys, df[by].to_numpy())
    G = len(keys)
    ref = X.group_extremes(x, codes, G, thr)
    res = est.score_extremes(df, by, threshold=thr, quantiles=levels, num_samples=S, seed=seed)
    assert list(res['keys']) == list(keys) and res['n'] == G
    # exact: per-row shares, any-exceedance share, integer-valued means
    assert np.array_equal(res['peak_probability'], ref['peak_count'] / S)
    assert np.array_equal(res['exceed_probability'], ref['exceed_count'] / S)
    assert np.array_equal(res['exceed_any'], (ref['count'] > 0).sum(axis=0) / S)
    assert np.array_equal(res['exceed_count_mean'], ref['count'].sum(axis=0) / S)
    assert np.abs(ref['max']).min() >= 2.0 ** -10 and np.abs(ref['max']).sum(axis=0).max() < 2.0 ** 17
    assert np.array_equal(res['max_mean'], np.asarray([math.fsum(ref['max'][:, g].tolist()) for g in range(G)]) / S)
    share = np.bincount(codes, weights=res['peak_probability'], minlength=G)
    assert np.all(np.abs(share - 1.0) <= 1e-12), share          # R roundings of 2^-53 at most
    assert np.array_equal(np.bincount(codes, weights=ref['peak_count'], minlength=G), np.full(G, float(S)))
    # observed columns: pandas on the target column
    grp = df.assign(above=(y > thr).astype(np.float64)).groupby(by)
    obs_max, obs_count = grp['chickenpox'].max().to_numpy(dtype=np.float64), grp['above'].sum().to_numpy()
    assert np.array_equal(res['observed_max'], obs_max) and np.array_equal(res['observed_count'], obs_count)
    first = np.asarray([np.flatnonzero((codes == g) & (y == obs_max[g]))[0] for g in range(G)])
    assert np.array_equal(res['observed_peak_row'], first)
    assert np.array_equal(res['peak_row_probability'], res['peak_probability'][first])
    assert np.array_equal(res['brier'], (res['exceed_any'] - (obs_count > 0)) ** 2)
    # the summaries kernel at its bars
    for name, obs_y, pre in (('max', obs_max, 'max'), ('count', obs_count, 'exceed_count')):
      m = ref[name]
      want = dict(mean=m.mean(axis=0), quantiles=T.quantiles_ref(m, levels), crps=T.crps_ref(m, obs_y), pit=T.pit_ref(m, obs_y))
      got = dict(mean=res[pre + '_mean'], quantiles=res[pre + '_quantiles'], crps=res[name + '_crps'], pit=res[name + '_pit'])
      T.check_summaries(f'{kind} by {by}: {name} (G={G})', got, m, obs_y, levels, want)
      assert abs(res[f'mean_{name}_crps'] - want['crps'].mean()) <= T.crps_bars(m, obs_y).max()
    print(f'{kind} by {by}: observed max {obs_max}, forecast mean of the max {res["max_mean"]}, exceed_any {res["exceed_any"]}, '
          f'brier {res["brier"]}, P(observed peak row) {res["peak_row_probability"]}')
    # predict_extremes: the same forecast without the scores; a scalar threshold; no threshold
    pred = est.predict_extremes(df, by, threshold=thr, quantiles=levels, num_samples=S, seed=seed)
    assert set(pred) == {'keys', 'max_mean', 'max_quantiles', 'peak_probability', 'exceed_any', 'exceed_count_mean',
                         'exceed_count_quantiles', 'exceed_probability'}
    for k in set(pred) - {'keys'}:
      assert _same(pred[k], res[k]), k
  flat = est.predict_extremes(df, 'year', threshold=60, num_samples=S, seed=seed)
  ref60 = X.group_extremes(x, codes, G, np.full(R, 60.0, dtype=np.float32))
  assert np.array_equal(flat['exceed_probability'], ref60['exceed_count'] / S) and flat['max_quantiles'].shape == (1, G)
  assert np.array_equal(flat['exceed_any'], (ref60['count'] > 0).sum(axis=0) / S)
  none = est.predict_extremes(df, 'year', num_samples=S, seed=seed)
  assert set(none) == {'keys', 'max_mean', 'max_quantiles', 'peak_probability'}
  assert _same(none['peak_probability'], flat['peak_probability']) and _same(none['max_mean'], flat['max_mean'])
  # a group with a NaN target row is not scored; the forecast does not change
  d = df.copy()
  d.loc[d.index[[1, 5]], 'chickenpox'] = np.nan
  res2 = est.score_extremes(d, 'year', threshold=thr, quantiles=levels, num_samples=S, seed=seed)
  gone = codes[[1, 5]]
  assert gone[0] == gone[1] and res2['n'] == G - 1 and np.isnan(res2['observed_max'][gone[0]])
  assert res2['observed_peak_row'][gone[0]] == -1 and np.isnan(res2['observed_count'][gone[0]])
  for k in ('max_crps', 'count_crps', 'brier', 'peak_row_probability'):
    assert np.array_equal(np.isnan(res2[k]), np.arange(G) == gone[0]), k
    assert _same(np.delete(res2[k], gone[0]), np.delete(res[k], gone[0])), k
  assert np.isnan(res2['max_pit'][:, gone[0]]).all() and _same(res2['max_mean'], res['max_mean'])
  assert est.score_extremes(d, 'location', num_samples=S, seed=seed)['n'] == 0
