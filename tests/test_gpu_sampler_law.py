"""The path sampler (bayesnf_amd/csrc/bnf_sampling.h, predictive_draw) held to its law: the pooled marginal law at the
branch points of the code, its tails and first two moments, the exact law of a total of independent rows, independence
across paths, members and counter words, rates beyond 2^24, non-finite parameters, and the recorded stream.

Every bar is a formula of tests/sampler_law_ref.py at the N drawn here, alpha = 1e-9; tests/test_sampler_law_host.py
shows numpy's samplers inside each of them and five wrong samplers outside.  The big arrays are reduced on the device
(sort, searchsorted, sum, var); counts and summaries come to the host.

Measured on an MI355X (worst value / bar; every test prints its own):
  pooled law, 28 cases + 9 at counter offsets, N = 2^22   DKW 0.00056 / 0.00160; tail count off by 162 / 393 (level 1e-3);
                                                          mean 340 / 1399 (ZINB tc 1e3, mean 1e6); variance 0.055 / 0.173
  rates beyond 2^24 (mean 1e8, tc 1e3), N = 2^22           DKW 0.00048 / 0.00160
  totals of 2 .. 40,000 rows, S = 32,768                   DKW 0.0063 / 0.0181; chi-square 33,339 in [31,227, 34,355]
  totals at row0 = 2^32 - 512, 2^40, sample0 = 2^32 - S    DKW 0.0094 / 0.0181
  lags 1, 2, 356 of the totals, S = 32,768                 |r| 0.0103 / 0.0338
  rows 1 and 256 apart, adjacent paths, N = 2^22           |r| 0.00096 / 0.00344; row0 = 2^32 against 0: 0.00074 / 0.00298
  M = 7, totals of 1,024 rows, S = 32,768                  mean 40 / 240, variance 4.7e4 / 2.1e6, corr(member, residual)
                                                          0.0036 / 0.0338
Before NaN parameters were made to give NaN draws (commit 70111c5) the poisoned cells of the last-but-one test held: NB
and ZINB, NaN loc or NaN aux[1]: the count 0 in every cell; ZINB, NaN aux[2]: the finite draws of the NB without
inflation; NORMAL: NaN; loc = -100: +inf (ZINB: 0 in the cells the inflation replaces)."""
import hashlib
import math

import numpy as np
import pytest
import torch

from bayesnf_amd import inference
from tests import sampler_law_ref as L
from tests.test_gpu_sampling import MEAN_F, TC_F, _dev, _engine, _mixed_inputs, inv_softplus

pytestmark = pytest.mark.gpu

S_POOL, R_POOL = 4096, 1024            # N = 2^22 i.i.d. draws per case: eps = 0.0016
N_POOL = S_POOL * R_POOL
S_TOT = 32768                           # paths of the totals: eps = 0.0181
GROUP_SIZES = (2, 256, 257, 1024, 1025, 4096, 40000)
TOTAL_THRESHOLDS = 128                  # thresholds per total (the ZINB total's CDF is a sum over ~1,000 NB laws)
PI = 0.35


@pytest.fixture(scope='module')
def engines():
  made = {}

  def get(obs):
    if obs not in made:
      made[obs] = _engine(obs)[0]
    return made[obs]
  yield get
  for eng in made.values():
    eng.close()


def _count_inputs(tc, mean, pi=0.0):
  """(loc scalar f32, aux row f32) of a count row with total_count tc and NB mean `mean`."""
  loc = np.float32(inv_softplus(tc * tc / mean))
  return loc, np.asarray([1.0, 1.0 / tc, pi], dtype=np.float32)


def _case(obs, a, b, pi=0.0):
  """obs NORMAL: (mu, sigma) = (a, b); counts: (total_count, mean) = (a, b) -> (loc, aux row, law of the f32 inputs)."""
  if obs == 'NORMAL':
    loc, aux = np.float32(a), np.asarray([b, 1.0, 0.0], dtype=np.float32)
    return loc, aux, L.NormalLaw(float(loc), float(aux[0]))
  loc, aux = _count_inputs(a, b, pi)
  return loc, aux, L.CountLaw.from_inputs(loc, aux[1], aux[2] if obs == 'ZINB' else 0.0)


def _draw_pool(eng, loc, aux, seed, row0=0, sample0=0):
  loc_d = _dev(eng, np.full((1, R_POOL), loc))
  return eng.predictive_samples(loc_d, _dev(eng, aux[None, :]), S_POOL, seed=seed, row0=row0, sample0=sample0)


def summarise_device(x, law, thr=None, with_tails=True):
  """sampler_law_ref.summarise_numpy with the sort and the counting on the device."""
  xs = x.reshape(-1).double().sort().values
  n = xs.numel()
  thr = L.thresholds(law) if thr is None else thr
  tails = [] if not with_tails else L.tail_points(law) + ([] if law.discrete else L.tail_points(law, lower=True))
  n_up = len(L.TAIL_LEVELS)
  pts = torch.from_numpy(np.concatenate([thr, [t for _, t, _ in tails]])).to(xs.device)
  le = torch.searchsorted(xs, pts, right=True).cpu().numpy()
  lt = torch.searchsorted(xs, pts, right=False).cpu().numpy()
  k = len(thr)
  out = dict(n=n, D=L.dkw_distance(n, thr, le[:k], lt[:k], law), mean=float(xs.mean()), var=float(xs.var()), tails=[])
  for i, (lv, t, mass) in enumerate(tails):
    cnt = int(n - le[k + i]) if i < n_up else int(lt[k + i])
    out['tails'].append((lv if i < n_up else -lv, cnt, n * mass, L.tail_count_bound(n, mass)))
  if law.discrete and with_tails:        # the mass at 0, held as a count
    p0 = float(law.cdf(0.0))
    out['tails'].append((0.0, int((xs == 0).sum()), n * p0, L.tail_count_bound(n, p0)))
  return out


def _assert_pool(x, law, label):
  sm = summarise_device(x, law)
  print(L.describe(sm, law, label))
  assert sm['n'] == N_POOL
  failed = L.check_summary(sm, law)
  assert not failed, (label, failed, sm)


POOL_CASES = (
    [(obs, tc, mean, PI if obs == 'ZINB' else 0.0) for obs in ('NB', 'ZINB') for tc in (0.05, 1e3) for mean in (0.02, 1e6)] +
    [('NB', 1e6, mean, 0.0) for mean in (9.9, 9.99, 10.01, 10.1, 30.0)] +                 # the inversion / PTRS switch
    [('NB', tc, mean, 0.0) for tc in (0.999, 1.0, 1.001) for mean in (5.0, 400.0)] +      # the boost switch
    [('NB', tc, 30.0, 0.0) for tc in (1e-3, 0.01)] +                                      # almost all mass at 0
    [('NB', 1e6, 1e6, 0.0)] +
    [('ZINB', 3.0, 8.0, pi) for pi in (0.0, 1e-3, 0.35, 0.999)] +
    [('NORMAL', 0.5, 0.01, 0.0), ('NORMAL', -1e3, 100.0, 0.0)])


@pytest.mark.parametrize('obs,a,b,pi', POOL_CASES)
def test_pooled_marginal_law_tails_and_moments(engines, obs, a, b, pi):
  """M = 1 and 1,024 identical columns: the 2^22 draws of a case are i.i.d.  (1) DKW distance at the law's own k / 4096
  quantiles <= eps(2^22) = 0.0016; (2) the counts beyond the law's 1 - 1e-2, 1 - 1e-3, 1 - 1e-4 quantiles (NORMAL: and
  below the mirror levels; counts: and the zeros) within Bernstein's bound of N x the exact mass; (3) sample mean and
  variance within 6 standard errors of the closed forms."""
  loc, aux, law = _case(obs, a, b, pi)
  x = _draw_pool(engines(obs), loc, aux, seed=2024)
  assert x.shape == (S_POOL, R_POOL) and x.dtype == torch.float32
  assert bool(torch.isfinite(x).all())
  if law.discrete:
    assert bool((x >= 0).all()) and bool((x == x.floor()).all())
  _assert_pool(x, law, f'{obs} a={a:g} b={b:g} pi={pi:g}')


def test_rates_beyond_2_pow_24(engines):
  """Mean 1e8 at total_count 1e3: every draw a finite, non-negative, integer-valued float (rounded to the float grid,
  spacing 8 at 1e8, against a standard deviation of 3e6); DKW against the law (the distance does not depend on the
  scale: x / mean and x give the same one)."""
  loc, aux, law = _case('NB', 1e3, 1e8)
  x = _draw_pool(engines('NB'), loc, aux, seed=77)
  assert bool(torch.isfinite(x).all()) and bool((x >= 0).all()) and bool((x == x.floor()).all())
  assert float(x.max()) > 2.0 ** 24
  sm = summarise_device(x, law)
  print(L.describe(sm, law, 'NB tc=1e3 mean=1e8'))
  assert sm['D'] <= L.dkw_eps(N_POOL), sm


TOTAL_CASES = {'NORMAL': ('NORMAL', 0.5, 2.0, 0.0), 'NB': ('NB', 3.0, 8.0, 0.0), 'ZINB': ('ZINB', 3.0, 8.0, PI)}


def _grouping(sizes, seed):
  """Groups of the given sizes, rows in permuted order -> (offsets, rows)."""
  codes = np.random.default_rng(seed).permutation(np.repeat(np.arange(len(sizes)), sizes))
  return inference.csr_from_codes(codes, len(sizes))


def _totals(eng, obs, sizes, seed, row0=0, sample0=0):
  _, a, b, pi = TOTAL_CASES[obs]
  loc, aux, law = _case(obs, a, b, pi)
  off, rows = _grouping(sizes, 9)
  R = int(sum(sizes))
  t = eng.predictive_group_sums(_dev(eng, np.full((1, R), loc)), _dev(eng, aux[None, :]), off, rows, S_TOT, seed=seed,
                                row0=row0, sample0=sample0)
  assert t.shape == (S_TOT, len(sizes)) and t.dtype == torch.float64
  return t, law


_cache = {}


def _big_totals(engines, obs):
  if obs not in _cache:
    _cache[obs] = _totals(engines(obs), obs, GROUP_SIZES, seed=31)
  return _cache[obs]


def _assert_totals(t, law, sizes, label):
  """Every column of t (S, G) against the exact law of a total of sizes[g] rows: DKW, eps(S); NORMAL also the
  chi-square interval of (S - 1) s^2 / (n sigma^2)."""
  S = t.shape[0]
  eps, worst = L.dkw_eps(S), 0.0
  lo, hi = L.chi2_bounds(S - 1)
  for g, n in enumerate(sizes):
    tl = law.total(n)
    sm = summarise_device(t[:, g], tl, thr=L.thresholds(tl, TOTAL_THRESHOLDS), with_tails=False)
    worst = max(worst, sm['D'])
    line = f'{label} n={n}: S={S} D={sm["D"]:.4f}/EPS={eps:.4f}'
    if not law.discrete:
      q = (S - 1) * sm['var'] / (n * law.sigma ** 2)
      line += f' chi2 {q:.0f} in [{lo:.0f}, {hi:.0f}]'
      assert lo <= q <= hi, (label, n, q, lo, hi)
    print(line)
    assert sm['D'] <= eps, (label, n, sm['D'], eps)
  print(f'{label}: worst D / EPS = {worst / eps:.3f}')


@pytest.mark.parametrize('obs', ['NORMAL', 'NB', 'ZINB'])
def test_law_of_a_total_of_independent_rows(engines, obs):
  """Identical rows of one member in permuted order, groups of 2 (inside a thread's four rows), 256 / 257, 1,024 / 1,025
  (a tile and across its edge), 4,096 and 40,000 (across the combine pass): the totals of 32,768 paths follow
  N(n mu, n sigma^2), NB(n tc, logits), sum_k Binom(k; n, 1 - pi) NB(k tc, logits).  A correlation of 1e-3 between rows
  fails this from n = 1,024 on (host test)."""
  t, law = _big_totals(engines, obs)
  _assert_totals(t, law, GROUP_SIZES, obs)


def _corr(a, b):
  a, b = a.double().reshape(-1), b.double().reshape(-1)
  a, b = a - a.mean(), b - b.mean()
  return float((a * b).sum() / torch.sqrt((a * a).sum() * (b * b).sum()))


def group_sums_sample_stride(R, S):
  """gridDim.y of k_predictive_group_sums: the stride at which one workgroup walks the paths (pred_grid in
  bayesnf_amd/csrc/bnf_api.hip; S paths in one pass)."""
  return min(S, 65535, max(1, 16384 // -(-R // 1024)))


@pytest.mark.parametrize('obs', ['NORMAL', 'NB', 'ZINB'])
def test_totals_of_different_paths_are_uncorrelated(engines, obs):
  """Autocorrelation of the totals over the path index at lags 1, 2 and the stride at which a workgroup revisits the
  paths: inside norm.isf(alpha / 2) / sqrt(S - lag)."""
  t, _ = _big_totals(engines, obs)
  stride = group_sums_sample_stride(sum(GROUP_SIZES), S_TOT)
  assert 2 < stride < S_TOT
  worst = 0.0
  for g, n in enumerate(GROUP_SIZES):
    for lag in (1, 2, stride):
      r, bar = _corr(t[:-lag, g], t[lag:, g]), L.lag_corr_bound(S_TOT - lag)
      worst = max(worst, abs(r) / bar)
      assert abs(r) <= bar, (obs, n, lag, r, bar)
  print(f'{obs}: lags 1, 2, {stride}: worst |r| / bar = {worst:.3f} (bar {L.lag_corr_bound(S_TOT - 1):.4f})')


OFFSETS = [dict(row0=2 ** 32 - 512), dict(row0=2 ** 40), dict(sample0=2 ** 32 - S_POOL)]


@pytest.mark.parametrize('obs', ['NORMAL', 'NB', 'ZINB'])
def test_law_holds_across_the_counter_word_boundaries(engines, obs):
  """The pooled law and the law of totals (groups of 1,024 and 1,025) where the row index crosses into counter word 3
  (row0 = 2^32 - 512: the block straddles it; row0 = 2^40) and where the path index ends (sample0 = 2^32 - S).  Rows
  next to each other, rows 256 apart (one thread) and adjacent paths are uncorrelated.  The block at row0 = 2^32 is
  another block than the one at row0 = 0."""
  eng = engines(obs)
  _, a, b, pi = TOTAL_CASES[obs]
  loc, aux, law = _case(obs, a, b, pi)
  bar = L.lag_corr_bound(N_POOL - S_POOL * 256)
  for kw in OFFSETS:
    x = _draw_pool(eng, loc, aux, seed=8, **kw)
    _assert_pool(x, law, f'{obs} {kw}')
    rs = dict(row1=_corr(x[:, :-1], x[:, 1:]), row256=_corr(x[:, :-256], x[:, 256:]), path1=_corr(x[:-1], x[1:]))
    print(f'{obs} {kw}: correlations {rs}, bar {bar:.5f}')
    assert all(abs(r) <= bar for r in rs.values()), (obs, kw, rs, bar)
    tkw = dict(kw, sample0=2 ** 32 - S_TOT) if 'sample0' in kw else kw
    t, _ = _totals(eng, obs, (1024, 1025), seed=8, **tkw)
    _assert_totals(t, law, (1024, 1025), f'{obs} totals {tkw}')
  x0 = _draw_pool(eng, loc, aux, seed=8)
  x1 = _draw_pool(eng, loc, aux, seed=8, row0=2 ** 32)
  differ, r = float((x0 != x1).float().mean()), _corr(x0, x1)
  print(f'{obs}: row0 = 2^32 against row0 = 0: {differ:.3f} of the cells differ, correlation {r:.5f} (bar {L.lag_corr_bound(N_POOL):.5f})')
  assert differ > 0.3
  assert abs(r) <= L.lag_corr_bound(N_POOL)


@pytest.mark.parametrize('obs', ['NB', 'ZINB'])
def test_members_mix_with_the_law_of_total_variance(engines, obs):
  """M = 7 members (TC_F, MEAN_F around total_count 3, mean 8), totals of 1,024 identical rows: mean and variance of the
  totals equal those of the equal-weight mixture of the members' total laws within 6 standard errors (the variance's
  from the mixture's fourth central moment); the member of a path -- read from a NORMAL engine with the same seed, whose
  component draw is the same function of (seed, path) -- is uncorrelated with the standardised within-member residual."""
  M, n, seed = 7, 1024, 123
  cases = [_case(obs, 3.0 * TC_F[m], 8.0 * MEAN_F[m], PI if obs == 'ZINB' else 0.0) for m in range(M)]
  eng = engines(obs)
  loc = np.stack([np.full(n, c[0]) for c in cases])
  aux = np.stack([c[1] for c in cases])
  off, rows = _grouping((n,), 3)
  t = eng.predictive_group_sums(_dev(eng, loc), _dev(eng, aux), off, rows, S_TOT, seed=seed)[:, 0]
  laws = [c[2].total(n) for c in cases]
  mean, var, mu4 = L.mixture_moments(laws)
  mbar, vbar = 6.0 * math.sqrt(var / S_TOT), 6.0 * math.sqrt((mu4 - var * var) / S_TOT)
  got_m, got_v = float(t.mean()), float(t.var())
  print(f'{obs} M=7: S={S_TOT} |mean err|={abs(got_m - mean):.4g}/{mbar:.4g} |var err|={abs(got_v - var):.4g}/{vbar:.4g}')
  assert abs(got_m - mean) <= mbar and abs(got_v - var) <= vbar

  en = engines('NORMAL')
  mark = en.predictive_samples(_dev(en, 100.0 * np.arange(M)[:, None]), _dev(en, np.tile([0.01, 1.0, 0.0], (M, 1))),
                               S_TOT, seed=seed)[:, 0].double()
  member = torch.round(mark / 100.0).long()
  assert float((mark - 100.0 * member).abs().max()) < 0.1 and int(member.min()) >= 0 and int(member.max()) < M
  mom = np.asarray([lw.moments()[:2] for lw in laws])
  z = (t - torch.from_numpy(mom[:, 0]).to(t.device)[member]) / torch.from_numpy(np.sqrt(mom[:, 1])).to(t.device)[member]
  r, bar = _corr(member, z), L.lag_corr_bound(S_TOT)
  zm, zv = float(z.mean()), float(z.var())
  print(f'{obs} M=7: corr(member, residual) = {r:.5f} (bar {bar:.5f}); residual mean {zm:.4f} variance {zv:.4f}')
  assert abs(r) <= bar


# ----------------------------------------------------------------------------------------------------------------------
# non-finite and overflowing parameters
# ----------------------------------------------------------------------------------------------------------------------
def _poison_setup(eng, obs):
  M, R, S = 3, 5, 64
  loc, aux = _mixed_inputs(obs, M, R, 4)
  en = eng('NORMAL')
  mark = en.predictive_samples(_dev(en, 100.0 * np.arange(M)[:, None]), _dev(en, np.tile([0.01, 1.0, 0.0], (M, 1))),
                               S, seed=17)[:, 0].cpu().numpy()
  member = np.rint(mark / 100.0).astype(int)
  assert all((member == m).any() for m in range(M))
  return M, R, S, loc, aux, member


def _poisons(obs):
  """(label, (array, index), value, rows hit (None: all), expected draw)."""
  out = [('loc nan', ('loc', (1, 2)), np.nan, [2], np.nan)]
  if obs == 'NORMAL':
    out.append(('aux0 nan', ('aux', (1, 0)), np.nan, None, np.nan))
  else:
    out.append(('aux1 nan', ('aux', (1, 1)), np.nan, None, np.nan))
    out.append(('loc -100: rate beyond f32', ('loc', (1, 2)), -100.0, [2], np.inf))
  if obs == 'ZINB':
    out.append(('aux2 nan', ('aux', (1, 2)), np.nan, None, np.nan))
  return out


def _same(a, b):
  return np.array_equal(np.asarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64),
                        np.asarray(b).view(np.uint32 if b.dtype == np.float32 else np.uint64))


@pytest.mark.parametrize('obs', ['NORMAL', 'NB', 'ZINB'])
def test_non_finite_parameters_give_nan_draws_and_overflowing_rates_inf(engines, obs):
  """One poisoned cell of member 1 (M = 3, R = 5, S = 64).  A NaN in loc[m, r] gives NaN at (s, r) for the paths of
  member m; a NaN in the member's scale (NORMAL aux[0]), dispersion (aux[1]) or inflation (ZINB aux[2]) gives NaN in
  every row of those paths; loc = -100 for a count model (softplus(loc) = 4e-44, the rate 1 / (aux[1]^2 softplus(loc))
  is beyond the f32 range) gives +inf, never NaN and never a positive finite count -- in the ZINB the cells that the
  zero inflation replaces keep their 0 (the law of a ZINB of unbounded rate: 0 with probability pi), and they are the
  cells that are 0 when that row's mean is 1e7 (P(NB = 0) = 1e-7).  Every other cell keeps the bits of the clean
  call.  predictive_group_sums gives the f64 sums of exactly these draws (NaN and inf propagate into the totals that
  hold such a cell, every other total keeps its bits); predictive_group_extremes then applies its NaN-draw rule (a NaN
  draw counts as -inf and never exceeds) to a count model."""
  eng = engines(obs)
  M, R, S, loc, aux, member = _poison_setup(engines, obs)
  grp = np.asarray([0, 0, 1, 1, 1])
  off, rows = inference.csr_from_codes(grp, 2)
  draw = lambda l, a: eng.predictive_samples(_dev(eng, l), _dev(eng, a), S, seed=17).cpu().numpy()
  sums_of = lambda l, a: eng.predictive_group_sums(_dev(eng, l), _dev(eng, a), off, rows, S, seed=17).cpu().numpy()
  clean, clean_sums = draw(loc, aux), sums_of(loc, aux)
  assert np.all(np.isfinite(clean))
  hit_paths = member == 1
  for label, (which, idx), value, hit_rows, want in _poisons(obs):
    l2, a2 = loc.copy(), aux.copy()
    (l2 if which == 'loc' else a2)[idx] = value
    x = draw(l2, a2)
    hit = np.zeros((S, R), dtype=bool)
    hit[np.ix_(hit_paths, range(R) if hit_rows is None else hit_rows)] = True
    got = np.unique(x[hit])
    print(f'{obs} {label}: the {hit.sum()} poisoned cells hold {got[:6]}{" ..." if len(got) > 6 else ""}')
    assert _same(x[~hit], clean[~hit]), (obs, label, 'a clean cell moved')
    if np.isnan(want):
      assert np.all(np.isnan(x[hit])), (obs, label, got)
    elif obs == 'ZINB':
      l3 = loc.copy()
      l3[idx] = inv_softplus(1.0 / (float(aux[1, 1]) ** 2 * 1e7))
      replaced = draw(l3, aux)[hit] == 0
      assert replaced.any() and not replaced.all()
      assert np.array_equal(x[hit], np.where(replaced, np.float32(0), np.float32(want))), (obs, label, got)
    else:
      assert np.all(x[hit] == want), (obs, label, got)
    sums = sums_of(l2, a2)
    host = np.stack([np.bincount(grp, weights=x[s].astype(np.float64), minlength=2) for s in range(S)])
    touched = ~np.isfinite(host)
    assert touched.any() and not (touched & ~hit_paths[:, None]).any()
    assert _same(sums[~touched], clean_sums[~touched]), (obs, label, 'a clean total moved')
    assert np.array_equal(sums[touched], host[touched], equal_nan=True), (obs, label, np.unique(sums[touched]))
    if obs == 'NB' and label == 'loc nan':
      ex = eng.predictive_group_extremes(_dev(eng, l2), _dev(eng, a2), off, rows, S, seed=17,
                                         threshold=np.zeros(R, dtype=np.float32))
      xm = np.where(np.isnan(x), -np.inf, x).astype(np.float64)
      assert np.array_equal(ex['max'].cpu().numpy()[:, 1], xm[:, 2:].max(axis=1))
      assert np.array_equal(ex['count'].cpu().numpy()[:, 1], (x[:, 2:] > 0).sum(axis=1).astype(np.float64))
      assert np.array_equal(ex['exceed_count'].cpu().numpy(), (x > 0).sum(axis=0).astype(np.int32))


# ----------------------------------------------------------------------------------------------------------------------
# the stream is pinned: a user's seed keeps giving the user's paths
# ----------------------------------------------------------------------------------------------------------------------
# SHA-256 of the (50, 3001) float32 arrays of test_gpu_sampling.py::test_draws_are_a_pure_function_of_seed_path_and_
# global_row (M = 4, seed 5), recorded on an MI355X from a build of commit 70111c5, before NaN parameters were made to
# give NaN draws.
STREAM_SHA256 = {
    'NORMAL': '9d1f1f74f6d24959b449800a268bb4ed20e618de148f7f8c4cbaf4b4cb061549',
    'NB': '00378e6701fa9dac854390773500b264436fbf61cf6eebf22fa144fcec9d6f3e',
    'ZINB': '69b01a147b568f69f07e6ec1f8a7cb0a6c4b63d2de199ebb4108635520579013',
}


@pytest.mark.parametrize('obs', ['NORMAL', 'NB', 'ZINB'])
def test_the_stream_is_pinned(engines, obs):
  eng = engines(obs)
  loc, aux = _mixed_inputs(obs, 4, 3001, 11)
  full = eng.predictive_samples(_dev(eng, loc), _dev(eng, aux), 50, seed=5).cpu().numpy()
  assert full.shape == (50, 3001) and full.dtype == np.float32
  digest = hashlib.sha256(np.ascontiguousarray(full).tobytes()).hexdigest()
  print(f'{obs}: sha256 {digest}')
  assert digest == STREAM_SHA256[obs]
