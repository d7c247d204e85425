"""Linear combinations of the rows of the sample paths formed on the GPU (include/bnf.h bnf_predictive_combinations),
against the float64 host reference of tests/combinations_ref.py on the per-row draws of the same seed.

The bar of a cell is (n_k + 1) 2^-52 sum |coef x| (combinations_ref: one rounding per product, at most n_k - 1 in any
summation order, a factor of two of margin); counts with integer coefficients are exact integers below 2^53 and must be
equal.  The LDS is poisoned before every call: nothing may be read that the call has not written."""
import copy
import ctypes as C
import math

import numpy as np
import pandas as pd
import pytest
import torch

from bayesnf_amd import _native, inference, spatiotemporal
from tests import combinations_ref as Cr
from tests import totals_ref as T
from tests.test_gpu_sampling import _dev, _engine, _fit, _mixed_inputs, _random_grouping

pytestmark = pytest.mark.gpu

TILE = _native.GROUP_TILE
M, R, S = 4, 3000, 24
OBS = ('NORMAL', 'NB', 'ZINB')


def _combine(eng, loc_d, aux_d, off, rows, coef, n=S, seed=42, **kw):
  eng.debug_poison_lds()
  got = eng.predictive_combinations(loc_d, aux_d, off, rows, coef, n, seed, **kw)
  assert got.shape == (n, len(off) - 1) and got.dtype == torch.float64
  return got.cpu().numpy()


def _bits(a):
  return np.ascontiguousarray(a).view(np.int64)


def _layout():
  """Form sizes of the one spec of the reference test, with the position at which every form starts:
  empty | 1024 from a tile edge | 1 | 1024 off the edge | 1023 (ends on an edge) | empty | 1025 from an edge |
  1100 singletons (more than a tile of them) | 70,000 (68 tiles and a bit: the second pass strides its lanes) | 1 | empty."""
  sizes = [0, 1024, 1, 1024, 1023, 0, 1025] + [1] * 1100 + [70000, 1, 0]
  off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
  assert off[1] % TILE == 0 and off[3] % TILE == 1 and off[5] % TILE == 0 and off[6] % TILE == 0
  assert (off[-3] - off[-4]) // TILE > 64
  return sizes, off


def _check(tag, got, x, off, rows, coef, exact):
  want, absum = Cr.combine_ref(x, off, rows, coef)
  empty = np.diff(off) == 0
  assert np.all(got[:, empty] == 0.0), (tag, 'empty forms')
  err, bar = np.abs(got - want), Cr.bar(off, absum)
  ratio = float(np.max(err / np.where(bar > 0, bar, np.inf), initial=0.0))
  print(f'{tag}: {len(off) - 1} forms, {off[-1]} positions, worst error / bar {ratio:.3f}, max |error| {err.max():.3e}')
  assert np.all(err <= bar), (tag, float(err.max()), ratio)
  if exact:
    assert np.array_equal(got, want), (tag, 'counts with integer coefficients')


@pytest.mark.parametrize('obs', OBS)
def test_combinations_equal_the_host_reference(obs):
  eng, _ = _engine(obs)
  rng = np.random.default_rng(17)
  loc, aux = _mixed_inputs(obs, M, R, 21)
  loc_d, aux_d = _dev(eng, loc), _dev(eng, aux)
  eng.debug_poison_lds()
  x = eng.predictive_samples(loc_d, aux_d, S, seed=42).cpu().numpy().astype(np.float64)
  sizes, off = _layout()
  nnz = int(off[-1])
  rows = rng.integers(0, R, nnz).astype(np.int32)            # rows repeat, inside a form and across forms
  big = int(off[-4])
  rows[big + 5], rows[big + 1024], rows[big + 69999], rows[3] = -1, R, R + 5, -7      # outside the table: add nothing
  real = rng.standard_normal(nnz) * np.exp(rng.uniform(-3.0, 3.0, nnz))               # mixed sign, six decades
  whole = rng.choice([-2.0, -1.0, 1.0, 3.0], nnz)
  _check(f'{obs} real', _combine(eng, loc_d, aux_d, off, rows, real), x, off, rows, real, False)
  _check(f'{obs} integer', _combine(eng, loc_d, aux_d, off, rows, whole), x, off, rows, whole, obs != 'NORMAL')
  # one form of nnz positions, and the same positions as two forms split unevenly at position 1000
  for n in (1, 1023, 1024, 1025, 2049):
    for cut in ((), (1000,)) if n >= 1024 else ((),):
      o = np.asarray([0, *cut, n], dtype=np.int32)
      for name, coef in (('real', real), ('integer', whole)):
        got = _combine(eng, loc_d, aux_d, o, rows[:n], coef[:n])
        _check(f'{obs} {name} nnz={n} cut={cut}', got, x, o, rows[:n], coef[:n], obs != 'NORMAL' and name == 'integer')
  # no position at all: every form empty
  none = _combine(eng, loc_d, aux_d, np.zeros(4, dtype=np.int32), rows[:0], real[:0])
  eng.close()
  assert none.shape == (S, 3) and np.all(none == 0.0)


@pytest.mark.parametrize('obs', OBS)
def test_partition_with_unit_coefficients_has_the_bits_of_the_group_sums(obs):
  eng, _ = _engine(obs)
  n_rows, n = 40000 + 37, 8
  rng = np.random.default_rng(5)
  loc, aux = _mixed_inputs(obs, M, n_rows, 21)
  codes, G = _random_grouping(n_rows, rng)
  off, rows = inference.csr_from_codes(codes, G)
  loc_d, aux_d = _dev(eng, loc), _dev(eng, aux)
  ones = np.ones(n_rows)
  cum = np.asarray([0.1, 0.15, 0.85, 1.0])
  for kw in ({}, {'cum_weights': cum}):
    eng.debug_poison_lds()
    sums = eng.predictive_group_sums(loc_d, aux_d, off, rows, n, 42, **kw).cpu().numpy()
    got = _combine(eng, loc_d, aux_d, off, rows, ones, n=n, **kw)
    assert np.array_equal(_bits(got), _bits(sums)), (obs, sorted(kw))
  # the member weights entered: other paths than the equal-weight call's
  plain = eng.predictive_group_sums(loc_d, aux_d, off, rows, n, 42).cpu().numpy()
  assert not np.array_equal(_bits(got), _bits(plain)), 'the member weights did not enter'
  eng.close()


@pytest.mark.parametrize('obs', OBS)
def test_overlap_the_draw_is_the_same_at_every_occurrence(obs):
  """Forms (+1, r), (-1, r) are exactly 0.0 wherever the pair lies: inside a tile, across a tile edge (odd start), in
  forms of their own and inside one long form of many pairs."""
  eng, _ = _engine(obs)
  rng = np.random.default_rng(3)
  loc, aux = _mixed_inputs(obs, M, R, 21)
  loc_d, aux_d = _dev(eng, loc), _dev(eng, aux)
  K = 1500
  r = rng.integers(0, R, K)
  # one leading singleton shifts every pair to an odd position: the pairs at 1023|1024 and 2047|2048 straddle a tile edge
  off = np.concatenate([[0, 1], 1 + 2 * np.arange(1, K + 1)]).astype(np.int32)
  rows = np.concatenate([[0], np.repeat(r, 2)]).astype(np.int32)
  coef = np.concatenate([[1.0], np.tile([1.0, -1.0], K)])
  assert off[512] == 1023 and off[1024] == 2047
  got = _combine(eng, loc_d, aux_d, off, rows, coef)
  assert np.all(got[:, 1:] == 0.0), (obs, int(np.count_nonzero(got[:, 1:])))
  # the same pairs from an even start: every pair inside a tile
  got = _combine(eng, loc_d, aux_d, off[1:] - 1, rows[1:], coef[1:])
  assert np.all(got == 0.0), (obs, 'pairs inside a tile')
  # pairs far apart: (+1, r) in the first tile, (-1, r) two tiles on, with rows between them that cancel among themselves
  far = np.concatenate([r[:700], np.repeat(r[700:1400], 2), r[:700]]).astype(np.int32)
  fcoef = np.concatenate([np.ones(700), np.tile([1.0, -1.0], 700), -np.ones(700)])
  got = _combine(eng, loc_d, aux_d, np.asarray([0, len(far)], dtype=np.int32), far, fcoef)
  if obs == 'NORMAL':                                        # the order of the f64 additions follows the tiling: a bar, not bits
    x = eng.predictive_samples(loc_d, aux_d, S, seed=42).cpu().numpy().astype(np.float64)
    _check('NORMAL far pairs', got, x, np.asarray([0, len(far)]), far, fcoef, False)
  else:
    assert np.all(got == 0.0), (obs, 'pairs across tiles')
  eng.close()


def test_a_hierarchy_adds_up_exactly_on_counts():
  """Leaves partition the rows, regions the leaves, the nation is everything: three levels in the same paths.  On NB every
  total is an exact integer, so a parent equals the sum of its children exactly."""
  eng, _ = _engine('NB')
  rng = np.random.default_rng(8)
  loc, aux = _mixed_inputs('NB', M, R, 21)
  loc_d, aux_d = _dev(eng, loc), _dev(eng, aux)
  leaf = rng.integers(0, 37, R)
  region = leaf % 5
  parts = []
  for codes, n in ((leaf, 37), (region, 5), (np.zeros(R, dtype=np.int64), 1)):
    o, rws = inference.csr_from_codes(codes, n)
    parts.append((pd.RangeIndex(n), (np.repeat(np.arange(n), np.diff(o)), rws, np.ones(R))))
  keys, spec = spatiotemporal.stack_combinations(*parts)
  _, off, rows, coef = inference.combinations_csr(spec, R, names=keys)
  assert len(keys) == 43 and off[-1] == 3 * R
  got = _combine(eng, loc_d, aux_d, off, rows, coef)
  eng.close()
  leaves, regions, nation = got[:, :37], got[:, 37:42], got[:, 42]
  assert nation.min() > 0 and np.all(got == np.floor(got))
  for g in range(5):
    assert np.array_equal(regions[:, g], leaves[:, np.arange(37) % 5 == g].sum(axis=1)), g
  assert np.array_equal(nation, regions.sum(axis=1)) and np.array_equal(nation, leaves.sum(axis=1))


def _raw(eng, loc_d, aux_d, off, rows, coef, n, seed, work_bytes):
  """The C entry point with a work buffer of `work_bytes` -> (return code, out); out is filled with 7 before the call."""
  dev = eng.device
  off_d, rows_d = torch.from_numpy(off).to(dev), torch.from_numpy(rows).to(dev)
  coef_d = torch.from_numpy(coef).to(dev)
  work = torch.empty(max(1, work_bytes), dtype=torch.uint8, device=dev)
  out = torch.full((n, len(off) - 1), 7.0, dtype=torch.float64, device=dev)
  p = lambda t: C.c_void_p(t.data_ptr())
  eng.debug_poison_lds()
  rc = eng.lib.bnf_predictive_combinations(
      eng.handle, p(loc_d), p(aux_d), loc_d.shape[0], loc_d.shape[1], p(off_d), p(rows_d), p(coef_d), len(off) - 1, n,
      C.c_uint64(seed), 0, 0, None, p(work), C.c_size_t(work_bytes), p(out))
  torch.cuda.synchronize()
  return rc, out.cpu().numpy()


@pytest.mark.parametrize('obs', ['NORMAL', 'ZINB'])
def test_determinism_chunks_passes_and_nan(obs):
  eng, _ = _engine(obs)
  rng = np.random.default_rng(23)
  loc, aux = _mixed_inputs(obs, M, R, 21)
  loc_d, aux_d = _dev(eng, loc), _dev(eng, aux)
  sizes = [0, 700, 1, 2500, 1, 1, 5000, 3, 0, 1024]          # crossing forms, singletons, empties; 10 tiles
  off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
  nnz = int(off[-1])
  rows = rng.integers(0, R, nnz).astype(np.int32)
  coef = rng.standard_normal(nnz)
  one = _combine(eng, loc_d, aux_d, off, rows, coef)
  assert np.array_equal(_bits(one), _bits(_combine(eng, loc_d, aux_d, off, rows, coef))), 'two runs differ'
  assert np.all(np.isfinite(one))
  parts = [_combine(eng, loc_d, aux_d, off, rows, coef, n=8, sample0=s0) for s0 in (0, 8, 16)]
  assert np.array_equal(_bits(np.concatenate(parts)), _bits(one)), 'sample0 chunks'
  # a work buffer of exactly one path's worth (24 passes) gives the bits of a large one; one byte less is refused, unlaunched
  per_path = 16 * (-(-nnz // TILE))
  rc, big = _raw(eng, loc_d, aux_d, off, rows, coef, S, 42, per_path * S)
  assert rc == 0 and np.array_equal(_bits(big), _bits(one))
  rc, tight = _raw(eng, loc_d, aux_d, off, rows, coef, S, 42, per_path)
  assert rc == 0, _native.last_error()
  assert np.array_equal(_bits(tight), _bits(one)), 'passes'
  rc, odd = _raw(eng, loc_d, aux_d, off, rows, coef, S, 42, 5 * per_path + 9)       # 5 paths a pass: 5 passes, the last of 4
  assert rc == 0 and np.array_equal(_bits(odd), _bits(one))
  rc, untouched = _raw(eng, loc_d, aux_d, off, rows, coef, S, 42, per_path - 1)
  assert rc == -1 and 'work buffer' in _native.last_error()
  assert np.all(untouched == 7.0), 'a refused call wrote to out'
  # a NaN coefficient makes its own form NaN and no other: in a singleton, inside a crossing form, next to a tile edge
  for at in (int(off[2]), int(off[3]) + 400, int(off[6]) + 3000, nnz - 1):
    bad = coef.copy()
    bad[at] = np.nan
    got = _combine(eng, loc_d, aux_d, off, rows, bad)
    k = int(np.searchsorted(off, at, side='right')) - 1
    assert np.all(np.isnan(got[:, k])), (at, k)
    others = np.arange(len(sizes)) != k
    assert np.array_equal(_bits(got[:, others]), _bits(one[:, others])), (at, k)
  eng.close()


def _exact_moments(lik, coef_dense, n_rows):
  """Mean and variance of sum_r c_r x_r under the mixture: rows independent given the member, law of total variance."""
  mu = np.asarray(lik.mean(), dtype=np.float64).reshape(-1, n_rows)
  sd = np.asarray(lik.stddev(), dtype=np.float64).reshape(-1, n_rows)
  t_m = mu @ coef_dense.T                                    # (members, K)
  v_m = (sd ** 2) @ (coef_dense ** 2).T
  mean = t_m.mean(axis=0)
  return mean, v_m.mean(axis=0) + (t_m ** 2).mean(axis=0) - mean ** 2


@pytest.mark.parametrize('kind', ['map', 'vi'])
def test_estimator_combinations_end_to_end(golden_dir, kind):
  """chickenpox fixture (one place, 100 weeks), NB for MAP and NORMAL for VI; a `block` column cuts the weeks into four
  quarters so that the hierarchy has more than one level."""
  df, est = _fit(golden_dir, kind)
  df = df.reset_index(drop=True)
  n_rows, n, seed = len(df), 1024, 11
  df['block'] = np.arange(n_rows) // 25
  df['all'] = 'nation'
  dates = np.sort(df['datetime'].unique())
  per_date = spatiotemporal.group_combinations(df, 'datetime', mean=True)          # the per-date mean over places
  grand = spatiotemporal.group_combinations(df, 'all', mean=True)                  # the grand mean
  contrast = spatiotemporal.group_combinations(                                    # last date minus first date, per place
      df, 'location', weight=np.where(df['datetime'] == dates[-1], 1.0, np.where(df['datetime'] == dates[0], -1.0, 0.0)))
  levels = (spatiotemporal.group_combinations(df, 'location'), spatiotemporal.group_combinations(df, 'block'),
            spatiotemporal.group_combinations(df, 'all'))
  keys, spec = spatiotemporal.stack_combinations(per_date, grand, contrast, *levels)
  K = len(keys)
  assert K == 100 + 1 + 1 + 1 + 4 + 1
  q = (0.025, 0.5, 0.975)
  pred = est.predict_combinations(df, (keys, spec), quantiles=q, num_samples=n, seed=seed, samples=True)
  assert list(pred['keys']) == list(keys) and pred['samples'].shape == (n, K) and pred['samples'].dtype == np.float64
  assert pred['mean'].shape == (K,) and pred['quantiles'].shape == (3, K)
  again = est.predict_combinations(df, (keys, spec), quantiles=q, num_samples=n, seed=seed)
  assert 'samples' not in again and np.array_equal(_bits(again['mean']), _bits(pred['mean']))

  # samples == predict_samples @ coef^T within the bar
  _, off, rows, coef = inference.combinations_csr(spec, n_rows, names=keys)
  x = est.predict_samples(df, n, seed=seed).astype(np.float64)
  _check(f'{kind} estimator', pred['samples'], x, off, rows, coef, False)
  dense = np.zeros((K, n_rows))
  dense[np.repeat(np.arange(K), np.diff(off)), rows] = coef
  assert np.array_equal(dense[101], np.r_[-1.0, np.zeros(98), 1.0])
  # the summaries are those of the matrix, at the bars of tests/totals_ref.py
  xs = pred['samples']
  ref = dict(mean=np.asarray([math.fsum(xs[:, c].tolist()) for c in range(K)]) / n, quantiles=T.quantiles_ref(xs, q))
  T.check_summaries(f'{kind} predict_combinations', pred, xs, None, q, ref)

  # 'mean' against the exact mixture moments: 6 sd / sqrt(S)
  mean, var = _exact_moments(est.likelihood_model(df), dense, n_rows)
  z = np.abs(pred['mean'] - mean) / np.sqrt(var / n)
  print(f'{kind}: worst |sample mean - exact| / (sd / sqrt(S)) = {z.max():.3f} over {K} combinations')
  assert np.all(z <= 6.0), (int(np.argmax(z)), float(z.max()))

  # the stacked totals have the bits of predict_totals / predict_samples(group_by=...) for the same grouping
  at = 102
  for col in ('location', 'block', 'all'):
    t_mean, t_q, t_keys = est.predict_totals(df, col, quantiles=q, num_samples=n, seed=seed)
    totals, _ = est.predict_samples(df, n, seed=seed, group_by=col)
    sl = slice(at, at + len(t_keys))
    assert list(keys[sl]) == list(t_keys)
    assert np.array_equal(_bits(pred['samples'][:, sl]), _bits(totals)), col
    assert np.array_equal(_bits(pred['mean'][sl]), _bits(t_mean)), col
    assert np.array_equal(_bits(pred['quantiles'][:, sl]), _bits(np.stack(t_q))), col
    at += len(t_keys)
  assert at == K

  # score_combinations: 'observed' agrees with pandas, 'crps' and 'pit' with totals_ref on the same samples
  scored_df = df.copy()
  scored_df.loc[40, 'chickenpox'] = np.nan                    # week 40: its date, block 1, the place and the nation go unscored
  res = est.score_combinations(scored_df, (keys, spec), quantiles=q, num_samples=n, seed=seed)
  y = scored_df['chickenpox'].to_numpy(dtype=np.float64)
  want = np.concatenate([scored_df.groupby('datetime')['chickenpox'].mean().to_numpy(), [np.nan],
                         [y[-1] - y[0]], [np.nan], scored_df.groupby('block')['chickenpox'].sum(min_count=25).to_numpy(),
                         [np.nan]])
  assert np.array_equal(np.isnan(res['observed']), np.isnan(want))
  np.testing.assert_allclose(res['observed'][~np.isnan(want)], want[~np.isnan(want)], rtol=1e-13, atol=0)
  assert np.isnan(want).sum() == 5 and res['n'] == K - 5
  ref = dict(ref, crps=T.crps_ref(xs, res['observed']), pit=T.pit_ref(xs, res['observed']))
  T.check_summaries(f'{kind} score_combinations', res, xs, res['observed'], q, ref)
  scored = ~np.isnan(res['observed'])
  assert res['mean_crps'] == float(np.mean(res['crps'][scored], dtype=np.float64)) and np.isfinite(res['energy_score'])
  assert list(res['keys']) == list(keys) and 'samples' not in res

  # one-hot weights: the bits of that member alone
  lead = np.shape(np.asarray(est.params_[0]))[:est._ensemble_dims]
  onehot = np.zeros(lead)
  onehot.reshape(-1)[1] = 1.0
  idx = tuple(slice(i, i + 1) for i in np.unravel_index(1, lead))
  alone = copy.copy(est)
  alone.params_ = tuple(np.asarray(p)[idx] for p in est.params_)
  one = est.predict_combinations(df, (keys, spec), quantiles=q, num_samples=256, seed=seed, weights=onehot, samples=True)
  solo = alone.predict_combinations(df, (keys, spec), quantiles=q, num_samples=256, seed=seed, samples=True)
  for k in ('samples', 'mean', 'quantiles'):
    assert np.array_equal(_bits(one[k]), _bits(solo[k])), k
  assert not np.array_equal(_bits(one['samples']), _bits(pred['samples'][:256]))
