"""Spells above a threshold in the sample paths on the GPU (include/bnf.h bnf_predictive_group_episodes) against the
naive loop of tests/episodes_ref.py on `Engine.predictive_samples` for the same seed.  Every output is an integer, so
every comparison is EXACT.  The engine-level tests use synthetic loc / aux on a forward-only engine with M = 4, as
tests/test_gpu_extremes.py does."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from bayesnf_amd import _native, inference, spatiotemporal
from tests import episodes_ref as E
from tests import totals_ref as T
from tests.test_gpu_extremes import _grouping, _host, _same
from tests.test_gpu_sampling import _dev, _engine, _fit, _mixed_inputs, dkw_eps

pytestmark = pytest.mark.gpu

TILE = 1024
MATRICES = ('longest', 'longest_row', 'spells', 'onset_step', 'first_row', 'last_row')
HI, LO = np.float32(3e38), np.float32(-1.0)      # thresholds no count draw exceeds / every count draw exceeds


def _check(tag, got, ref, off):
  """Exact equality of everything `got` holds with the reference; groups without positions report 0 / -1 / 0 / 0 / -1 / -1."""
  for k in MATRICES:
    assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (tag, k, got[k].dtype, got[k].shape)
    assert np.array_equal(got[k], ref[k]), (tag, k, int((got[k] != ref[k]).sum()))
  empty = np.diff(np.asarray(off)) == 0
  for k, v in zip(MATRICES, (0, -1, 0, 0, -1, -1)):
    assert np.all(got[k][:, empty] == v), (tag, 'empty groups', k)
  if 'onset_count' in got:
    hit = got['first_row'][got['first_row'] >= 0]
    assert np.array_equal(got['onset_count'], np.bincount(hit, minlength=len(got['onset_count']))), (tag, 'onset_count')
    assert np.array_equal(got['onset_count'], ref['onset_count']), (tag, 'onset_count against the host')


def _median_threshold(x):
  nan = np.isnan(x).all(axis=0)                          # a row whose every draw is NaN: any threshold, nothing exceeds
  return np.where(nan, 0.0, np.nanmedian(np.where(nan[None, :], 0.0, x), axis=0)).astype(np.float32)


@pytest.mark.parametrize('kind', ['sizes', 'half'])
@pytest.mark.parametrize('obs', ['NORMAL', 'NB', 'ZINB'])
def test_mixed_and_crossing_tiles(obs, kind):
  """Tiles inside one group, mixed tiles and groups that cross tile edges; the rows of every group in a random order
  (time is position order, not row order).  The threshold is the per-row median of the draws: runs are short and
  frequent.  A few rows carry a NaN location: NORMAL draws NaN there, which must break a run and count as a step."""
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
  thr = _median_threshold(x)
  got = _host(eng.predictive_group_episodes(loc_d, aux_d, off, rows, n, 42, thr))
  again = _host(eng.predictive_group_episodes(loc_d, aux_d, off, rows, n, 42, thr))
  bare = _host(eng.predictive_group_episodes(loc_d, aux_d, off, rows, n, 42, thr, per_row=False))
  eng.close()
  assert set(got) == set(MATRICES) | {'onset_count'} and set(bare) == set(MATRICES)
  assert got['longest'].shape == (n, G) and got['longest'].dtype == np.float64 and got['first_row'].dtype == np.int32
  ref = E.group_episodes(x, off, rows, thr)
  print(f'{obs} {kind}: {G} groups, longest run {int(got["longest"].max())}, most spells {int(got["spells"].max())}, '
        f'{int(np.isnan(x).sum())} NaN draws')
  _check(f'{obs} {kind}', got, ref, off)
  assert got['spells'].max() > 100 and 2 <= got['longest'].max() < 64         # short and frequent
  if obs == 'NORMAL':
    # the NaN rows took part: the onset step of a path that never exceeds counts them, and no run contains one
    sizes = np.diff(off)
    never = got['longest'] == 0
    assert np.array_equal(got['onset_step'][never], np.broadcast_to(sizes, (n, G))[never])
    assert not np.isin(got['first_row'], nan_rows).any() and not np.isin(got['longest_row'], nan_rows).any()
  for k in got:
    assert _same(got[k], again[k]), ('two runs differ', k)
  for k in bare:
    assert _same(got[k], bare[k]), ('per_row changes the matrices', k)


def test_scripted_patterns():
  """NB with a threshold of -1 where a position shall exceed and 3e38 where not: the expected output follows from the
  pattern alone.  Five groups on one position axis (tile = 1024 positions):
    A  2 tiles: a run over the positions 1000 .. 1030 (it ends tile 0 at 1023 and continues at 1024) and a short one
    B  5 tiles: a run that covers its tiles 1 to 3 whole (pre == len chains through the combine pass) and a short one
    C  2 tiles: two runs of 7 in different tiles -- the earlier one wins
    D  300 positions: only the last one exceeds
    E  100 positions: entries of -1 in seg_rows inside a run (they must not break it) and before it (no step)."""
  eng, _ = _engine('NB')
  M, n = 4, 3
  sizes = [2 * TILE, 5 * TILE, 2 * TILE, 300, 100]
  off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
  R = int(off[-1])
  above = np.zeros(R, dtype=bool)
  a, b, c, d, e = (int(v) for v in off[:5])
  above[a + 1000:a + 1031] = True
  above[a + 5:a + 10] = True
  above[b + 1000:b + 4 * TILE + 5] = True
  above[b + 17:b + 20] = True
  above[c + 100:c + 107] = True
  above[c + 1500:c + 1507] = True
  above[d + 299] = True
  above[e + 10:e + 41] = True
  rng = np.random.default_rng(2)
  rows = rng.permutation(R).astype(np.int32)              # the table row of every position: not the position itself
  thr = np.empty(R, dtype=np.float32)
  thr[rows] = np.where(above, LO, HI)
  gone = np.asarray([e + 3, e + 20, e + 21, e + 30])
  table_rows = rows.copy()
  rows[gone] = -1
  loc, aux = _mixed_inputs('NB', M, R, 4)
  got = _host(eng.predictive_group_episodes(_dev(eng, loc), _dev(eng, aux), off, rows, n, 1, thr))
  eng.close()
  part = rows >= 0
  for g in range(5):
    seg = slice(int(off[g]), int(off[g + 1]))
    keep = part[seg]
    want = E.naive_episodes(above[seg][keep].tolist(), table_rows[seg][keep].tolist())
    have = tuple(got[k][:, g].tolist() for k in MATRICES)
    assert have == tuple([v] * n for v in want), ('group', g, want, [h[0] for h in have])
  r = lambda p: int(table_rows[p])
  assert got['longest'][0].tolist() == [31.0, 3 * TILE + 29.0, 7.0, 1.0, 28.0] and got['longest'][0, 1] > 2048
  assert got['longest_row'][0].tolist() == [r(a + 1000), r(b + 1000), r(c + 100), r(d + 299), r(e + 10)]
  assert got['spells'][0].tolist() == [2.0, 2.0, 2.0, 1.0, 1.0]
  assert got['onset_step'][0].tolist() == [5.0, 17.0, 100.0, 299.0, 9.0]
  assert got['first_row'][0].tolist() == [r(a + 5), r(b + 17), r(c + 100), r(d + 299), r(e + 10)]
  assert got['last_row'][0].tolist() == [r(a + 1030), r(b + 4 * TILE + 4), r(c + 1506), r(d + 299), r(e + 40)]
  assert got['onset_count'].sum() == 5 * n and np.all(got['onset_count'][got['first_row'][0]] == n)


@pytest.mark.parametrize('obs', ['NORMAL', 'NB'])
def test_more_than_64_tiles_in_one_group(obs):
  """One group over 66 tiles and a piece, and the same shifted by a leading singleton: the combine pass gives every
  lane a contiguous range of more than one tile and joins the lanes in order."""
  eng, _ = _engine(obs)
  M, R, n = 4, 66 * TILE + 5, 4
  loc, aux = _mixed_inputs(obs, M, R, 3)
  rng = np.random.default_rng(6)
  order = rng.permutation(R)
  codes = np.zeros(R, dtype=np.int64)
  codes[700] = 1                                       # the singleton's position comes last: the big group starts at 0
  off, rows = inference.csr_ordered(codes, 2, order)
  loc_d, aux_d = _dev(eng, loc), _dev(eng, aux)
  x = eng.predictive_samples(loc_d, aux_d, n, seed=9).cpu().numpy()
  thr = _median_threshold(x)
  thr[rows[:300]] = HI                                 # no path starts before position 300 ...
  thr[rows[40 * TILE:40 * TILE + 3000]] = -HI          # ... and every path has a run over three whole tiles
  got = _host(eng.predictive_group_episodes(loc_d, aux_d, off, rows, n, 9, thr))
  # the same with the singleton in front: the big group starts one position into tile 0 and ends in tile 66
  off2, rows2 = inference.csr_ordered(1 - codes, 2, order)
  got2 = _host(eng.predictive_group_episodes(loc_d, aux_d, off2, rows2, n, 9, thr))
  eng.close()
  _check(f'{obs} 66 tiles', got, E.group_episodes(x, off, rows, thr), off)
  _check(f'{obs} 66 tiles, shifted', got2, E.group_episodes(x, off2, rows2, thr), off2)
  assert got['longest'][:, 0].min() >= 3000 and got['onset_step'][:, 0].min() >= 300 and got['spells'][:, 0].min() > 64


def _raw_call(eng, loc_d, aux_d, off, rows, n, seed, thr, work_bytes, sample0=0):
  """The C entry point with a work buffer of `work_bytes`."""
  M, R = loc_d.shape
  G = len(off) - 1
  dev = eng.device
  off_d, rows_d = torch.from_numpy(off).to(dev), torch.from_numpy(rows).to(dev)
  thr_d = torch.from_numpy(thr).to(dev)
  work = torch.empty(max(1, work_bytes), dtype=torch.uint8, device=dev)
  f64 = lambda: torch.empty((n, G), dtype=torch.float64, device=dev)
  i32 = lambda: torch.empty((n, G), dtype=torch.int32, device=dev)
  out = {'longest': f64(), 'longest_row': i32(), 'spells': f64(), 'onset_step': f64(), 'first_row': i32(), 'last_row': i32(),
         'onset_count': torch.zeros(R, dtype=torch.int32, device=dev)}
  p = lambda t: C.c_void_p(t.data_ptr())
  call = lambda nbytes, thr_p, longest_p: eng.lib.bnf_predictive_group_episodes(
      eng.handle, p(loc_d), p(aux_d), M, R, p(off_d), p(rows_d), G, n, C.c_uint64(seed), 0, sample0, None, thr_p, p(work),
      C.c_size_t(nbytes), longest_p, p(out['longest_row']), p(out['spells']), p(out['onset_step']), p(out['first_row']),
      p(out['last_row']), p(out['onset_count']))
  assert call(work_bytes - 1, p(thr_d), p(out['longest'])) == -1 and 'work buffer' in _native.last_error()
  assert call(work_bytes, None, p(out['longest'])) == -1 and call(work_bytes, p(thr_d), None) == -1      # both required
  assert call(work_bytes, p(thr_d), p(out['longest'])) == 0, _native.last_error()
  torch.cuda.synchronize()
  return _host(out)


@pytest.mark.parametrize('obs', ['NORMAL', 'ZINB'])
def test_invariance_under_passes_chunking_and_weights(obs):
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
  thr = _median_threshold(x)
  full = _host(eng.predictive_group_episodes(loc_d, aux_d, off, rows, n, 5, thr))
  _check(f'{obs} one pass', full, E.group_episodes(x, off, rows, thr), off)
  # (a) a work buffer of exactly one path's worth: 16 passes, the bits of the roomy call
  per_path = _native.EPISODES_WORK_PER_TILE * (-(-R // TILE))
  cut = _raw_call(eng, loc_d, aux_d, off, rows, n, 5, thr, per_path)
  for k in full:
    assert _same(full[k], cut[k]), ('passes', k)
  # (b) two calls of 8 paths give the rows of the one call of 16; their per-row counters add up
  halves = [_host(eng.predictive_group_episodes(loc_d, aux_d, off, rows, 8, 5, thr, sample0=s0)) for s0 in (0, 8)]
  for k in MATRICES:
    assert _same(np.concatenate([halves[0][k], halves[1][k]]), full[k]), ('sample0', k)
  assert np.array_equal(halves[0]['onset_count'] + halves[1]['onset_count'], full['onset_count'])
  # (c) weights wholly on one member: that member's M = 1 result
  for m in (0, 2):
    cum = np.cumsum(np.eye(M)[m])
    one = _host(eng.predictive_group_episodes(loc_d, aux_d, off, rows, n, 5, thr, cum_weights=cum))
    alone = _host(eng.predictive_group_episodes(loc_d[m:m + 1], aux_d[m:m + 1], off, rows, n, 5, thr))
    for k in one:
      assert _same(one[k], alone[k]), ('one member', m, k)
  # (d) general weights: the reference on the weighted draws
  cum = np.cumsum([0.4, 0.1, 0.2, 0.3])
  cum[-1] = 1.0
  xw = eng.predictive_samples(loc_d, aux_d, n, seed=5, cum_weights=cum).cpu().numpy()
  wgt = _host(eng.predictive_group_episodes(loc_d, aux_d, off, rows, n, 5, thr, cum_weights=cum))
  eng.close()
  _check(f'{obs} weighted', wgt, E.group_episodes(xw, off, rows, thr), off)
  assert not np.array_equal(wgt['spells'], full['spells'])


def test_onset_and_spells_against_the_closed_form():
  """NORMAL, identical members, threshold = the mean: the exceedances of a path are i.i.d. with probability 1/2.
  One group of 40 rows, S = 4096 paths.
  onset_step: P(step = k) = 2^-(k + 1) for k < 40 and the censored value 40 has 2^-40; the empirical CDF of S i.i.d.
    paths lies within dkw_eps(S) of it except with probability 1e-9 (the bound of tests/test_gpu_sampling.py).
  spells = I_0 + sum_{i = 1}^{39} I_i, I_0 = b_0, I_i = (1 - b_{i-1}) b_i: mean 1/2 + 39/4; Var I_0 = 1/4, Var I_i = 3/16,
    Cov(I_0, I_1) = -1/8, Cov(I_i, I_{i+1}) = -1/16, every other pair independent, so
    Var = 1/4 + 39 * 3/16 - 2/8 - 2 * 38/16 = 2.5625 and the mean of S paths is within 6 sqrt(2.5625 / S) = 0.150 (six
    standard errors of a sum of bounded terms; 2e-9 under the normal law)."""
  eng, _ = _engine('NORMAL')
  M, R, S = 4, 40, 4096
  rng = np.random.default_rng(23)
  mean = (20.0 * rng.standard_normal(R)).astype(np.float32)
  loc = np.tile(mean, (M, 1))
  aux = np.tile(np.asarray([2.5, 1.0, 0.0], dtype=np.float32), (M, 1))
  off, rows = inference.csr_ordered(np.zeros(R, dtype=np.int64), 1, rng.permutation(R))
  got = _host(eng.predictive_group_episodes(_dev(eng, loc), _dev(eng, aux), off, rows, S, 2025, mean))
  eng.close()
  step = got['onset_step'][:, 0]
  k = np.arange(R + 1)
  cdf = np.where(k < R, 1.0 - 2.0 ** -(k + 1.0), 1.0)
  emp = np.asarray([(step <= v).mean() for v in k])
  d = float(np.abs(emp - cdf).max())
  var = 0.25 + 39 * 3 / 16 - 2 / 8 - 2 * 38 / 16
  bound = 6.0 * math.sqrt(var / S)
  m = float(got['spells'].mean())
  print(f'onset_step: sup |F_n - F| = {d:.4f} (eps {dkw_eps(S):.4f}); mean spells {m:.4f} against 10.25 +- {bound:.3f}')
  assert step.min() >= 0 and step.max() <= R and np.array_equal(step, np.round(step))
  assert d <= dkw_eps(S), d
  assert var == 2.5625 and abs(m - (0.5 + 39 / 4)) <= bound, m
  assert np.array_equal(got['onset_count'], np.bincount(got['first_row'][got['first_row'] >= 0], minlength=R))


@pytest.mark.parametrize('kind', ['map', 'vi'])
def test_estimator_episodes_end_to_end(golden_dir, kind):
  """chickenpox fixture (NB for MAP, NORMAL for VI) with its rows SHUFFLED: predict_episodes / score_episodes against
  the naive loop on predict_samples(table, S, seed) with the time ordering applied on the host.  Exact: the per-row
  shares, no_episode, the observed columns and the means (integers below 2^53 add without rounding).  Quantiles against
  numpy at the bars of tests/totals_ref.py; CRPS and PIT bit for bit against Engine.sample_summaries on the matrices."""
  df, est = _fit(golden_dir, kind)
  df = df.assign(year=df['datetime'].dt.year).sample(frac=1.0, random_state=4).reset_index(drop=True)
  assert not df['datetime'].is_monotonic_increasing
  S, seed, levels = 300, 3, (0.025, 0.5, 0.975)
  R = len(df)
  x = est.predict_samples(df, S, seed)
  y = df['chickenpox'].to_numpy(dtype=np.float64)
  thr = np.median(x, axis=0).astype(np.float32)            # per row: about half of the paths are above
  eng, _ = _engine('NORMAL')                               # any engine: sample_summaries does not read the model
  try:
    for by in ('location', 'year'):
      keys = np.sort(df[by].unique())
      codes = np.searchsorted(keys, df[by].to_numpy())
      G = len(keys)
      # the ordering on the host, by pandas: by group, then by time, ties in table order
      rows = df.assign(_g=codes).sort_values(['_g', 'datetime'], kind='stable').index.to_numpy()
      off = np.concatenate([[0], np.cumsum(np.bincount(codes, minlength=G))])
      ref = E.group_episodes(x, off, rows, thr)
      res = est.score_episodes(df, by, thr, quantiles=levels, num_samples=S, seed=seed)
      assert list(res['keys']) == list(keys) and res['n'] == G
      assert np.array_equal(res['onset_probability'], ref['onset_count'] / S)
      assert np.array_equal(res['no_episode'], (ref['longest'] == 0).sum(axis=0) / S)
      # no_episode = 1 - the group's sum of onset_probability, exactly, as counts
      onset_counts = np.rint(res['onset_probability'] * S).astype(np.int64)
      assert np.array_equal(np.rint(res['no_episode'] * S).astype(np.int64), S - np.bincount(codes, weights=onset_counts, minlength=G).astype(np.int64))
      # observed columns: group_target_episodes, and once more by the naive loop on the target itself
      obs = spatiotemporal.group_target_episodes(y, off, rows, thr.astype(np.float64))
      for g in range(G):
        r = rows[off[g]:off[g + 1]]
        want = E.naive_episodes((y[r] > thr[r]).tolist(), r.tolist())
        assert (obs['longest'][g], obs['longest_row'][g], obs['spells'][g], obs['onset_step'][g], obs['first_row'][g],
                obs['last_row'][g]) == want
      assert np.array_equal(res['observed_onset_row'], obs['first_row'])
      want_p = np.where(obs['first_row'] >= 0, res['onset_probability'][np.maximum(obs['first_row'], 0)], res['no_episode'])
      assert np.array_equal(res['onset_row_probability'], want_p)
      for name in ('longest', 'spells', 'onset_step'):
        m = ref[name]
        assert np.array_equal(res[f'observed_{name}'], obs[name])
        assert np.array_equal(res[f'{name}_mean'], m.sum(axis=0) / S), name
        want = dict(mean=m.mean(axis=0), quantiles=T.quantiles_ref(m, levels), crps=T.crps_ref(m, obs[name]), pit=T.pit_ref(m, obs[name]))
        have = dict(mean=res[f'{name}_mean'], quantiles=res[f'{name}_quantiles'], crps=res[f'{name}_crps'], pit=res[f'{name}_pit'])
        T.check_summaries(f'{kind} by {by}: {name} (G={G})', have, m, obs[name], levels, want)
        dev = {k: v.cpu().numpy() for k, v in eng.sample_summaries(torch.from_numpy(m), torch.from_numpy(obs[name]), levels).items()}
        for k in ('mean', 'quantiles', 'crps', 'pit'):
          assert _same(dev[k], have[k]), (name, k)
        assert res[f'mean_{name}_crps'] == float(np.mean(res[f'{name}_crps'], dtype=np.float64))
      print(f'{kind} by {by}: observed longest {obs["longest"]}, forecast mean {res["longest_mean"]}, spells {res["spells_mean"]}, '
            f'onset step {res["onset_step_mean"]}, no_episode {res["no_episode"]}, P(observed onset row) {res["onset_row_probability"]}')
      pred = est.predict_episodes(df, by, thr, quantiles=levels, num_samples=S, seed=seed)
      assert set(pred) == {'keys', 'onset_probability', 'no_episode'} | {
          n + s for n in ('longest', 'spells', 'onset_step') for s in ('_mean', '_quantiles')}
      for k in set(pred) - {'keys'}:
        assert _same(pred[k], res[k]), k
    # another ordering column, a scalar threshold: the reference with that ordering
    flat = est.predict_episodes(df, 'year', 60, order_by='chickenpox', num_samples=S, seed=seed)
    rows = df.assign(_g=codes).sort_values(['_g', 'chickenpox'], kind='stable').index.to_numpy()
    ref60 = E.group_episodes(x, off, rows, np.full(R, 60.0, dtype=np.float32))
    assert np.array_equal(flat['onset_probability'], ref60['onset_count'] / S) and flat['longest_quantiles'].shape == (1, G)
    assert np.array_equal(flat['spells_mean'], ref60['spells'].sum(axis=0) / S)
    # a group with a NaN target row is not scored; the forecast does not change
    d = df.copy()
    d.loc[d.index[[1]], 'chickenpox'] = np.nan
    res2 = est.score_episodes(d, 'year', thr, quantiles=levels, num_samples=S, seed=seed)
    gone = codes[1]
    assert res2['n'] == G - 1 and np.isnan(res2['observed_longest'][gone]) and res2['observed_onset_row'][gone] == -1
    for k in ('longest_crps', 'spells_crps', 'onset_step_crps', 'onset_row_probability'):
      assert np.array_equal(np.isnan(res2[k]), np.arange(G) == gone), k
    assert _same(res2['longest_mean'], res['longest_mean']) and _same(res2['onset_probability'], res['onset_probability'])
  finally:
    eng.close()
