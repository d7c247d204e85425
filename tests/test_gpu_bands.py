"""Simultaneous bands of sample paths on the GPU (include/bnf.h bnf_sample_depths / bnf_depth_levels /
bnf_sample_envelope) against tests/bands_ref.py, a numpy restatement of the definitions.  Every result is an integer, an
integer divided once by S, or a value picked from the input: every comparison is EXACT equality, nothing is measured.
The engine-level tests run on synthetic matrices with LDS poisoned first; the path tests on the real draws of a
forward-only engine with M = 4, as tests/test_gpu_windows.py does; the estimator tests on the chickenpox fixture.

pointwise_joint_coverage against coverage: ge(k) = #{paths of depth >= k} falls with k, so a cell with level <= k_pw has
pointwise_joint_coverage <= coverage and one with level >= k_pw the reverse.  Without ties a column holds exactly S - 2 k
samples in band k, which forces level <= k_pw: NORMAL draws are held to pointwise_joint_coverage <= coverage in EVERY
cell.  With ties (NB / ZINB rows that are mostly zeros) a small group can have level > k_pw -- its simultaneous band lies
inside the pointwise one (tests/test_bands_host.py works one by hand) -- so for the count models the inequality is
asserted in every cell with level <= k_pw, its reverse in the others, and in every cell of every group of 50 rows or more."""
import ctypes as C

import numpy as np
import pytest
import torch

from bayesnf_amd import _native, inference, spatiotemporal
from tests import bands_ref as B
from tests.test_gpu_extremes import _host, _same
from tests.test_gpu_sampling import _dev, _engine, _fit, _mixed_inputs

pytestmark = pytest.mark.gpu

COV = (0.5, 0.9, 1.0)
TILE = 1024


@pytest.fixture(scope='module')
def eng():
  e, _ = _engine('NB')
  yield e
  e.close()


def _queries(S):
  return [-5, -1, 0, 1, S // 4, S - 1, S, 2 ** 31 - 1]


def _run(eng, x, cg, G, y, cov=COV):
  """The three entry points on one matrix -> everything they return, as numpy."""
  S = x.shape[0]
  eng.debug_poison_lds()
  xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(eng.device)
  dep = eng.sample_depths(xd, cg, G, y)
  need = [1] + [B.need_of(c, S) for c in cov]
  lev = eng.depth_levels(dep['depth'], need, _queries(S), dep.get('obs_depth'))
  env = eng.sample_envelope(xd, cg, lev['level'])
  out = _host(dep)
  out.update(_host(lev))
  out.update(_host(env))
  return out


def _reference(x, cg, G, y, cov=COV):
  S = x.shape[0]
  need = [1] + [B.need_of(c, S) for c in cov]
  ref = {'depth': B.group_depths(x, cg, G)}
  if y is not None:
    ref['obs_depth'] = B.observed_depths(x, cg, G, y)
  ref.update(B.depth_levels(ref['depth'], need, _queries(S), ref.get('obs_depth')))
  ref['lower'], ref['upper'] = B.envelope(x, cg, ref['level'])
  return ref


def _equal(tag, got, ref):
  assert set(got) == set(ref), (tag, sorted(got), sorted(ref))
  for k, want in ref.items():
    have = got[k]
    assert have.shape == want.shape, (tag, k, have.shape, want.shape)
    if k in ('depth', 'obs_depth', 'level'):
      assert have.dtype == np.int32, (tag, k, have.dtype)
      assert np.array_equal(have, want), (tag, k, int((have != want).sum()))
    else:
      assert have.dtype == np.float64, (tag, k, have.dtype)
      assert np.array_equal(have, want, equal_nan=True), (tag, k)


@pytest.mark.parametrize('S', [1, 2, 63, 64, 65, 1000, 1024, 1025, 16384])
def test_grid_against_the_reference(eng, S):
  """S at the edges of the wave, of the padded length and of the cap; C = 8 k + 3 (a ragged last slab of the 8 columns a
  workgroup sorts; 16 columns at S = 16,384, where a slab is one column); 5 groups interleaved at random with
  out-of-range entries, so the columns of a group sit in different workgroups; continuous, tie-heavy and edge columns (all
  equal, +-0.0, +-inf, a NaN column); y with NaN entries and values outside the envelope.  Two calls give the same bits;
  two calls over column halves into one pre-filled depth equal the single call."""
  C_, G = (16, 5) if S == 16384 else (8 * 3 + 3, 5)
  for kind in B.KINDS:
    x, cg, y = B.band_case(S, C_, G, kind)
    tag = f'S={S} {kind}'
    ref = _reference(x, cg, G, y)
    got = _run(eng, x, cg, G, y)
    _equal(tag, got, ref)
    again = _run(eng, x, cg, G, y)
    for k in got:
      assert _same(got[k], again[k]), (tag, 'two calls differ', k)
    bare = _run(eng, x, cg, G, None)                       # without observed values: the same depths, no obs outputs
    assert 'obs_depth' not in bare and 'obs_pit' not in bare
    for k in bare:
      assert _same(bare[k], got[k]), (tag, 'without y', k)
    # column halves, the second first: min does not care
    h = C_ // 2 + 1
    xd = torch.from_numpy(x).to(eng.device)
    eng.debug_poison_lds()
    part = eng.sample_depths(xd[:, h:].contiguous(), cg[h:], G, y[h:])
    part = eng.sample_depths(xd[:, :h].contiguous(), cg[:h], G, y[:h], depth=part['depth'], obs_depth=part['obs_depth'])
    assert np.array_equal(part['depth'].cpu().numpy(), ref['depth']), (tag, 'column halves')
    assert np.array_equal(part['obs_depth'].cpu().numpy(), ref['obs_depth']), (tag, 'column halves, observed')
    if kind == 'edge' and S >= 63:
      assert (ref['depth'] == -1).all(axis=0).any(), 'no group is poisoned by the NaN column'
      assert (ref['obs_depth'] == -1).any(), 'no observed curve leaves the envelope'


def test_one_group_many_slabs_and_empty_groups(eng):
  """One group over 203 columns (26 slabs: every workgroup lowers the same S cells), every other group empty; a running
  total, so the columns are strongly dependent and the level is far above a Bonferroni guess."""
  S, C_, G = 500, 203, 3
  x, _, y = B.band_case(S, C_, G, 'normal')
  cg = np.full(C_, 1, dtype=np.int32)
  ref = _reference(x, cg, G, y)
  got = _run(eng, x, cg, G, y)
  _equal('one group', got, ref)
  assert np.all(got['level'][:, [0, 2]] == -1) and np.isnan(got['achieved'][:, [0, 2]]).all()
  assert np.all(got['depth'][:, [0, 2]] == B.NONE) and np.all(got['obs_depth'][[0, 2]] == B.NONE)
  need = B.need_of(0.9, S)
  bonferroni = (S - B.need_of(1 - 0.1 / C_, S)) // 2         # each column at 1 - 0.1 / C: band 0
  assert bonferroni == 0 and got['level'][2, 1] > 0 and got['achieved'][2, 1] >= need / S


def test_depths_that_are_not_ours_make_an_empty_group(eng):
  """bnf_depth_levels on a matrix with depths outside [-1, S - 1]: S, -2, BNF_DEPTH_NONE, INT32_MIN -- level -1 and NaN
  ratios in exactly those groups, the valid groups beside them as the reference has them."""
  S, G = 300, 6
  rng = np.random.default_rng(3)
  D = rng.integers(-1, S, size=(S, G)).astype(np.int32)
  D[:, 0] = rng.integers(0, 5, size=S)
  D[7, 1] = S
  D[299, 2] = -2
  D[:, 3] = B.NONE
  D[150, 4] = -2 ** 31
  OD = np.asarray([2, 3, 4, B.NONE, 0, S], dtype=np.int32)
  need = [1, 150, S]
  ref = B.depth_levels(D, need, _queries(S), OD)
  eng.debug_poison_lds()
  got = _host(eng.depth_levels(torch.from_numpy(D).to(eng.device), need, _queries(S), torch.from_numpy(OD).to(eng.device)))
  _equal('foreign depths', got, ref)
  assert np.all(got['level'][:, 1:5] == -1) and np.isnan(got['achieved'][:, 1:5]).all() and np.isnan(got['joint'][:, 1:5]).all()
  assert np.isnan(got['obs_pit'][:, 1:]).all() and not np.isnan(got['obs_pit'][:, 0]).any()      # group 5: OD = S
  assert np.all(got['level'][:, [0, 5]] >= -1) and not np.isnan(got['achieved'][:, [0, 5]]).any()


def test_errors_write_nothing(eng):
  """Every BNF_ERR_INVALID case of the three entry points; the outputs keep their bytes."""
  S, C_, G, L = 20, 11, 3, 2
  dev = eng.device
  x = torch.zeros((S, C_), dtype=torch.float64, device=dev)
  cg = torch.zeros((C_,), dtype=torch.int32, device=dev)
  y = torch.zeros((C_,), dtype=torch.float64, device=dev)
  i32 = lambda *shape: torch.full(shape, 7, dtype=torch.int32, device=dev)
  f64 = lambda *shape: torch.full(shape, 7.0, dtype=torch.float64, device=dev)
  depth, od, level = i32(S, G), i32(G), i32(L, G)
  ach, joint, pit, lower, upper = f64(L, G), f64(L, G), f64(2, G), f64(L, C_), f64(L, C_)
  p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
  ints = lambda *v: (C.c_int32 * len(v))(*v)
  lib, h = eng.lib, eng.handle
  cap = _native.SUMMARY_MAX_SAMPLES

  def depths(x_=x, S_=S, C__=C_, cg_=cg, G_=G, y_=y, depth_=depth, od_=od):
    return lib.bnf_sample_depths(h, p(x_), S_, C__, p(cg_), G_, p(y_), p(depth_), p(od_))

  def levels(depth_=depth, S_=S, G_=G, need=ints(1, S), n_cov=2, kq=ints(0, 3), n_q=2, od_=od, level_=level, ach_=ach,
             joint_=joint, pit_=pit):
    return lib.bnf_depth_levels(h, p(depth_), S_, G_, need, n_cov, kq, n_q, p(od_), p(level_), p(ach_), p(joint_), p(pit_))

  def envelope(x_=x, S_=S, C__=C_, cg_=cg, level_=level, L_=L, G_=G, lower_=lower, upper_=upper):
    return lib.bnf_sample_envelope(h, p(x_), S_, C__, p(cg_), p(level_), L_, G_, p(lower_), p(upper_))

  bad = [depths(x_=None), depths(cg_=None), depths(depth_=None), depths(S_=0), depths(C__=0), depths(G_=0),
         depths(S_=cap + 1), depths(y_=None), depths(od_=None),
         levels(depth_=None), levels(S_=0), levels(G_=0), levels(S_=cap + 1), levels(need=ints(0, S)),
         levels(need=ints(1, S + 1)), levels(n_cov=_native.BAND_MAX_LEVELS + 1), levels(n_q=_native.BAND_MAX_LEVELS + 1),
         levels(n_cov=-1), levels(n_q=-1), levels(need=None), levels(level_=None, ach_=None), levels(kq=None),
         levels(joint_=None), levels(od_=None), levels(n_cov=0, n_q=0, pit_=None),
         envelope(x_=None), envelope(cg_=None), envelope(level_=None), envelope(lower_=None), envelope(upper_=None),
         envelope(L_=0), envelope(L_=_native.BAND_MAX_LEVELS + 1), envelope(S_=0), envelope(C__=0), envelope(G_=0),
         envelope(S_=cap + 1)]
  assert bad == [-1] * len(bad), bad
  torch.cuda.synchronize()
  for name, t in (('depth', depth), ('obs_depth', od), ('level', level), ('achieved', ach), ('joint', joint),
                  ('obs_pit', pit), ('lower', lower), ('upper', upper)):
    assert torch.all(t == 7), ('written by a refused call', name)
  # the smallest valid calls: depths without y; levels with one output; then everything on the same buffers
  depth.fill_(B.NONE)
  od.fill_(B.NONE)
  assert depths(y_=None, od_=None) == 0, _native.last_error()
  assert levels(ach_=None, n_q=0, joint_=None, od_=None, pit_=None) == 0, _native.last_error()
  torch.cuda.synchronize()
  assert torch.all(depth[:, 0] == S - 1) and torch.all(depth[:, 1:] == B.NONE) and torch.all(od == B.NONE)
  # 11 all-equal columns, all in group 0: the groups 1 and 2 stay empty
  assert level.cpu().tolist() == [[S - 1, -1, -1], [S - 1, -1, -1]]
  assert torch.all(ach == 7) and torch.all(joint == 7) and torch.all(pit == 7)
  assert depths() == 0 and levels() == 0 and envelope() == 0, _native.last_error()
  torch.cuda.synchronize()
  assert od.cpu().tolist() == [S - 1, B.NONE, B.NONE]
  assert torch.all(lower == 0) and torch.all(upper == 0) and ach.cpu()[:, 0].tolist() == [1.0, 1.0]
  assert pit.cpu()[:, 0].tolist() == [1.0, 0.0] and torch.isnan(pit[:, 1:]).all()
  # the wrappers refuse what the library would
  with pytest.raises(ValueError, match='at most 16384'):
    eng.sample_depths(torch.zeros((cap + 1, 1), dtype=torch.float64, device=dev), [0], 1)
  with pytest.raises(ValueError, match='one group per column'):
    eng.sample_depths(x, cg[:5], G)
  with pytest.raises(ValueError, match='need = 21'):
    eng.depth_levels(depth, [S + 1])
  with pytest.raises(ValueError, match='it needs y'):
    eng.sample_depths(x, cg, G, obs_depth=od)


def _layout(rng, R):
  """Groups that cross tile edges, one of 50 rows, singletons and an empty one; the rows of every group in a random time
  order -> (codes, G, seg_offsets, seg_rows)."""
  sizes = [1100, 50, 1, 0, 700, 3, 64]
  sizes.append(R - sum(sizes))
  codes = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
  G = len(sizes)
  off, rows = inference.csr_ordered(codes, G, rng.permutation(R))
  return codes, G, off, rows


def _coverage_relation(tag, obs, level, coverage, joint, k_pw, sizes):
  """The module docstring's relation between pointwise_joint_coverage and coverage, in every cell."""
  live = ~np.isnan(coverage)
  k_pw = np.asarray(k_pw)[:, None]
  below, above = live & (level <= k_pw), live & (level >= k_pw)
  assert np.all(joint[below] <= coverage[below]), (tag, 'level <= k_pw')
  assert np.all(joint[above] >= coverage[above]), (tag, 'level >= k_pw')
  big = np.asarray(sizes) >= 50
  assert np.all(joint[:, big] <= coverage[:, big]), (tag, 'groups of 50 rows or more')
  assert np.any(joint[:, big] < coverage[:, big]), (tag, 'the pointwise band holds as many whole paths as the simultaneous one')
  if obs == 'NORMAL':
    assert np.array_equal(below, live) and np.all(joint[live] <= coverage[live]), (tag, 'every cell')
  print(f'{tag}: cells with level > k_pw (ties): {int((live & ~below).sum())} of {int(live.sum())}; groups of >= 50 rows: '
        f'pointwise joint coverage {joint[:, big].min():.3f} .. {joint[:, big].max():.3f} against {coverage[:, big].min():.3f} .. '
        f'{coverage[:, big].max():.3f}')


@pytest.mark.parametrize('obs', ['NORMAL', 'NB', 'ZINB'])
def test_paths_through_the_real_draws(obs):
  """of='rows' on `predictive_samples` of the same seed and of='cumulative' on the GPU's own `running` matrix (the order
  of its f64 additions follows the tiling, so a host cumsum may break near-ties differently for NORMAL), against the
  reference; groups cross tile edges, rows sit in a random time order; one row of the group of 3 carries a NaN location,
  which poisons that group for NORMAL.  Weights wholly on one member give the bits of that member alone."""
  e, _ = _engine(obs)
  M, R, S = 4, 2 * TILE + 301, 200
  rng = np.random.default_rng(8)
  loc, aux = _mixed_inputs(obs, M, R, 17)
  codes, G, off, rows = _layout(rng, R)
  sizes = np.bincount(codes, minlength=G)
  loc[:, np.flatnonzero(codes == 5)[1]] = np.nan
  loc_d, aux_d = _dev(e, loc), _dev(e, aux)
  need = [B.need_of(c, S) for c in COV]
  k_pw = [(S - n) // 2 for n in need]
  pos_group = np.repeat(np.arange(G, dtype=np.int32), np.diff(off))

  def both(**kw):
    x32 = e.predictive_samples(loc_d, aux_d, S, seed=21, **kw)
    run = e.predictive_group_cumulative(loc_d, aux_d, off, rows, S, 21, running=True, **kw)['running']
    return {'rows': (x32.double(), codes.astype(np.int32)), 'cumulative': (run, pos_group)}

  curves = both()
  for of, (xd, cg) in curves.items():
    x = xd.cpu().numpy()
    y = x[rng.integers(0, S, size=R), np.arange(R)] + rng.choice([0.0, 0.0, 0.0, 1.0, -3.0], size=R)
    y[rng.random(R) < 0.1] = np.nan
    tag = f'{obs} {of}'
    e.debug_poison_lds()
    dep = e.sample_depths(xd, cg, G, y)
    lev = e.depth_levels(dep['depth'], need, k_pw, dep['obs_depth'])
    env = e.sample_envelope(xd, cg, lev['level'])
    got = {**_host(dep), **_host(lev), **_host(env)}
    ref = {'depth': B.group_depths(x, cg, G), 'obs_depth': B.observed_depths(x, cg, G, y)}
    ref.update(B.depth_levels(ref['depth'], need, k_pw, ref['obs_depth']))
    ref['lower'], ref['upper'] = B.envelope(x, cg, ref['level'])
    _equal(tag, got, ref)
    assert np.all(got['level'][:, 3] == -1) and np.isnan(got['achieved'][:, 3]).all()       # the empty group
    if obs == 'NORMAL':
      assert np.isnan(x).any() and np.all(got['depth'][:, 5] == -1) and np.all(got['achieved'][:, 5] == 1.0)
    _coverage_relation(tag, obs, got['level'], got['achieved'], got['joint'], k_pw, sizes)
  for m in (0, 3):
    one = both(cum_weights=np.cumsum(np.eye(M)[m]))
    alone_x = e.predictive_samples(loc_d[m:m + 1], aux_d[m:m + 1], S, seed=21).double()
    alone_run = e.predictive_group_cumulative(loc_d[m:m + 1], aux_d[m:m + 1], off, rows, S, 21, running=True)['running']
    for of, alone in (('rows', alone_x), ('cumulative', alone_run)):
      xd, cg = one[of]
      a, b = e.sample_depths(xd, cg, G)['depth'], e.sample_depths(alone, cg, G)['depth']
      assert torch.equal(a, b), ('one member', m, of)
      assert not torch.equal(a, e.sample_depths(curves[of][0], cg, G)['depth']), ('the weights change nothing', m, of)
  e.close()


def test_fresh_paths_inside_the_band_printed():
  """Printed, not asserted (a sampling property of the envelope, not a gate): the share of 4,096 fresh NB paths (another
  seed) that lie inside the 90 % band of a group of 50 rows built from 4,096 paths.  Asserted: the band holds its own
  paths as the reference counts them."""
  e, _ = _engine('NB')
  M, R, S = 4, 50, 4096
  loc, aux = _mixed_inputs('NB', M, R, 23)
  loc_d, aux_d = _dev(e, loc), _dev(e, aux)
  cg = np.zeros(R, dtype=np.int32)
  build = e.predictive_samples(loc_d, aux_d, S, seed=1).double()
  fresh = e.predictive_samples(loc_d, aux_d, S, seed=2).double().cpu().numpy()
  e.debug_poison_lds()
  dep = e.sample_depths(build, cg, 1)
  need = B.need_of(0.9, S)
  lev = e.depth_levels(dep['depth'], [need], [(S - need) // 2])
  env = _host(e.sample_envelope(build, cg, lev['level']))
  x = build.cpu().numpy()
  own = B.inside(x, env['lower'][0], env['upper'][0], np.arange(R)).mean()
  new = B.inside(fresh, env['lower'][0], env['upper'][0], np.arange(R)).mean()
  assert own == float(lev['achieved'].cpu()[0, 0]) >= need / S
  print(f'90 % band of 50 NB rows from {S} paths: level {int(lev["level"].cpu()[0, 0])}, holds {own:.4f} of its own paths, '
        f'{new:.4f} of {S} fresh ones; the pointwise band holds {float(lev["joint"].cpu()[0, 0]):.4f} of its own whole')
  e.close()


@pytest.mark.parametrize('kind', ['map', 'vi'])
def test_estimator_bands_end_to_end(golden_dir, kind):
  """chickenpox fixture (NB for MAP, NORMAL for VI) with its rows SHUFFLED: predict_bands / score_bands equal the
  reference on predict_samples(table, S, seed) for of='rows'; for of='cumulative' on the GPU's own running totals of the
  same seed in time order (`Engine.predictive_group_cumulative` on the estimator's forward pass: for NORMAL the order of
  the f64 additions follows the tiling, so a host cumsum may break near-ties differently), which for NB are the host
  cumsum of predict_samples bit for bit (integers)."""
  df, est = _fit(golden_dir, kind)
  df = df.assign(year=df['datetime'].dt.year).sample(frac=1.0, random_state=4).reset_index(drop=True)
  S, seed, cov = 300, 3, (0.5, 0.9)
  R = len(df)
  x = est.predict_samples(df, S, seed).astype(np.float64)
  y = df['chickenpox'].to_numpy(dtype=np.float64).copy()
  y[[5, 17]] = np.nan
  d = df.assign(chickenpox=y)
  keys_of = ('keys', 'level', 'coverage', 'pointwise_joint_coverage', 'lower', 'upper', 'pointwise_lower', 'pointwise_upper')
  for by in ('location', 'year', None):
    if by is None:
      codes, G = np.zeros(R, dtype=np.int64), 1
    else:
      keys = np.sort(df[by].unique())
      codes, G = np.searchsorted(keys, df[by].to_numpy()), len(keys)
    ref = B.band_summaries(x, codes.astype(np.int32), G, cov, y)
    res = est.score_bands(d, by, coverage=cov, num_samples=S, seed=seed)
    assert list(res['keys']) == (list(keys) if by is not None else [0])
    for k in ('level', 'coverage', 'pointwise_joint_coverage', 'lower', 'upper', 'pointwise_lower', 'pointwise_upper',
              'observed_depth', 'inside', 'depth_pit'):
      assert np.array_equal(res[k], ref[k], equal_nan=True), (kind, by, k)
    assert np.array_equal(res['observed'], y, equal_nan=True) and res['n'] == G
    assert np.array_equal(res['share_inside'], ref['inside'].mean(axis=1))
    pred = est.predict_bands(df, by, coverage=cov, num_samples=S, seed=seed)
    assert set(pred) == set(keys_of)
    for k in set(pred) - {'keys'}:
      assert _same(np.asarray(pred[k]), np.asarray(res[k])), (kind, by, k)
    print(f'{kind} by {by}: level {res["level"].tolist()}, coverage {res["coverage"].tolist()}, pointwise band holds '
          f'{res["pointwise_joint_coverage"].tolist()}, observed depth {res["observed_depth"].tolist()}, PIT {res["depth_pit"].tolist()}')
  # of='cumulative': the running totals in time order
  for by in ('location', 'year'):
    keys = np.sort(df[by].unique())
    codes, G = np.searchsorted(keys, df[by].to_numpy()), len(keys)
    rows = df.assign(_g=codes).sort_values(['_g', 'datetime'], kind='stable').index.to_numpy()
    off = np.concatenate([[0], np.cumsum(np.bincount(codes, minlength=G))])
    run = np.empty((S, R))                                   # column = table row
    for g in range(G):
      r = rows[off[g]:off[g + 1]]
      run[:, r] = np.cumsum(x[:, r], axis=1)
    obs = spatiotemporal.group_target_cumulative(y, off, rows)['running']
    res = est.score_bands(d, by, coverage=cov, of='cumulative', num_samples=S, seed=seed)
    assert np.array_equal(res['observed'], obs, equal_nan=True) and np.isnan(obs).sum() >= 2     # NaN from a group's first on
    assert res['n'] == G - int(np.sum([np.isnan(obs[rows[off[g]:off[g + 1]]]).all() for g in range(G)]))
    feats = est.data_handler.get_test(df)
    with inference._sample_paths(feats, est.observation_model, est.params_, est._model_args(feats.shape),
                                 est._ensemble_dims, est.compute_dtype, None, seed) as (e, loc, aux, seed64, _):
      own = e.predictive_group_cumulative(loc, aux, off.astype(np.int32), rows.astype(np.int32), S, seed64,
                                          running=True)['running'].cpu().numpy()      # column = position
    if kind == 'map':
      assert np.array_equal(own, run[:, rows]), 'NB: the running totals are integers'
    run[:, rows] = own
    ref = B.band_summaries(run, codes.astype(np.int32), G, cov, obs)
    for k in ('level', 'coverage', 'pointwise_joint_coverage', 'lower', 'upper', 'pointwise_lower', 'pointwise_upper',
              'observed_depth', 'inside', 'depth_pit'):
      assert np.array_equal(res[k], ref[k], equal_nan=True), (kind, by, 'cumulative', k)
    pred = est.predict_bands(df, by, coverage=cov, of='cumulative', num_samples=S, seed=seed)
    for k in set(pred) - {'keys'}:
      assert _same(np.asarray(pred[k]), np.asarray(res[k])), (kind, by, 'cumulative', k)
    other = est.predict_bands(df, by, coverage=cov, of='cumulative', order_by='chickenpox', num_samples=S, seed=seed)
    assert not np.array_equal(other['lower'], pred['lower'], equal_nan=True)
  # weights are passed through: all weight on one member gives the reference on that member's samples
  wts = np.zeros(np.shape(est.params_[0])[:est._ensemble_dims])
  wts.flat[0] = 1.0
  xw = est.predict_samples(df, S, seed, weights=wts).astype(np.float64)
  keys = np.sort(df['year'].unique())
  codes = np.searchsorted(keys, df['year'].to_numpy()).astype(np.int32)
  one = est.predict_bands(df, 'year', coverage=cov, num_samples=S, seed=seed, weights=wts)
  refw = B.band_summaries(xw, codes, len(keys), cov)
  for k in set(one) - {'keys'}:
    assert np.array_equal(one[k], refw[k], equal_nan=True), (kind, 'weights', k)
  assert not np.array_equal(one['lower'], est.predict_bands(df, 'year', coverage=cov, num_samples=S, seed=seed)['lower'])
