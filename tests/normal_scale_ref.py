"""The NORMAL forecast kernels at the data's own scale (bnf_quantiles.h k_quantile_root, k_quantile_approx; bnf_scoring.h):
cases whose `loc` sits where the target does -- the reference does not standardise it, the project's stated range is
|y| up to 1e5 with sigma at its 0.01 floor -- and references that are themselves good there.

  `case`             loc = centre + spread sigma randn, sigma_m in [sigma, 2 sigma] with sigma_0 = sigma, y around a member
  `moment_quantile`  the moment-matched Normal quantile, float64, CENTRED: mean = sum w mu, var = sum w (sd^2 + (mu - mean)^2).
                     (weighted_ref.normal_moment_quantile and the oracle's approximate_normal_quantile form
                     E[x^2] - E[x]^2, which loses 4 % of the variance in float64 at centre 1e5, sigma 0.01.)
  `cdf`              the mixture CDF, float64, of the float32 inputs
  `root_f32`         k_quantile_root restated in numpy float32, operation by operation
  `accept`           the acceptance rule for an exact quantile (see there)
The scores need no reference of their own: scoring_ref.normal_ref / normal_f32 and weighted_ref.normal_ref / normal_f32 work
on the differences y - mu and mu_i - mu_j, as the kernels do (tests/test_normal_scale_host.py holds them to that).
"""
import functools
from fractions import Fraction

import numpy as np
from scipy import special as sp

from tests import scoring_ref as S
from tests import weighted_ref as W

F = np.float32
CENTRES = (0.0, 1e3, 1e5, -1e5)
SIGMAS = (0.01, 1.0, 30.0)
SPREADS = (0.0, 3.0, 100.0)
LEVELS = (0.001, 0.025, 0.5, 0.975, 0.999)
QBAR = 2e-5                       # the quantile bar of tests/test_gpu_weighted.py and tests/test_gpu_parity.py
Q_ROWS = (1, 255, 257)            # around the 256-thread block of the quantile kernels
S_ROWS = (1, 65, 1025)            # around the 64-lane block of k_score_rows and the 1024-row tile of the pair kernel
MEMBERS = (1, 2, 7, 65)
VI_MEMBERS = 1920                 # a VI fit's component count, at 5 rows
OUTLIER = 50.0                    # 'tiny_outlier': the last member this many sigma away from where it was


def case(M, R, centre, sigma, spread, seed=0):
  """-> (loc (M, R) float32, sigma (M,) float32, y (R,) float32); y is a draw from the equal-weight mixture itself."""
  rng = np.random.default_rng([seed, M, R, int(abs(centre)), int(centre < 0), int(round(100 * sigma)), int(spread)])
  sig = sigma * rng.uniform(1.0, 2.0, M)
  sig[0] = sigma
  loc = centre + spread * sigma * rng.standard_normal((M, R))
  pick = rng.integers(0, M, R)
  y = loc[pick, np.arange(R)] + sig[pick] * rng.standard_normal(R)
  return loc.astype(F), sig.astype(F), y.astype(F)


def weighted(loc, sigma, pattern):
  """-> (loc, w): the weights of weighted_ref.PATTERNS; 'tiny_outlier' moves the last member OUTLIER sigma away."""
  M = loc.shape[0]
  if pattern == 'tiny_outlier' and M > 1:
    loc = np.array(loc)
    loc[-1] += F(OUTLIER) * sigma[-1]
  return loc, W.weights(pattern, M)


def _grid(rows):
  """The pruned product: every (centre, sigma, spread) at M = 7 and the middle row count; at centre 1e5 every M with
  every row count (sigma and spread taking turns), and the VI component count at 5 rows."""
  out = [(7, rows[1], c, s, sp_) for c in CENTRES for s in SIGMAS for sp_ in SPREADS]
  turn = 0
  for M in MEMBERS:
    for R in rows:
      if (M, R) != (7, rows[1]):
        out.append((M, R, 1e5, SIGMAS[turn % 3], SPREADS[(turn // 3) % 3]))
        turn += 1
  out += [(VI_MEMBERS, 5, 1e5, 0.01, 3.0), (VI_MEMBERS, 5, 1e5, 1.0, 100.0)]
  return out


def quantile_grid():
  return _grid(Q_ROWS)


def score_grid():
  """The score grid; the pair kernel's 1033 members (65 slots over 64 blocks) at 5 rows too."""
  return _grid(S_ROWS) + [(1033, 5, 1e5, 0.01, 3.0)]


# ------------------------------------------------------------------------------------------------------ float64 references
def _w(w, M):
  return np.full(M, 1.0 / M) if w is None else np.asarray(w, dtype=np.float64)


def mixture_moments(loc, sigma, w=None):
  """-> (mean (R,), var (R,)) float64, centred."""
  loc, sigma = np.asarray(loc, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
  w = _w(w, loc.shape[0])
  mean = w @ loc
  var = w @ (sigma[:, None] ** 2 + (loc - mean[None, :]) ** 2)
  return mean, var


def moment_quantile(loc, sigma, q, w=None):
  mean, var = mixture_moments(loc, sigma, w)
  return mean + np.sqrt(var) * sp.ndtri(q)


def naive_variance(loc, sigma, w=None):
  """E[x^2] - E[x]^2 in float64: what the references before this one form."""
  loc, sigma = np.asarray(loc, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
  w = _w(w, loc.shape[0])
  return w @ (sigma[:, None] ** 2 + loc ** 2) - (w @ loc) ** 2


def exact_variance(loc, sigma, r, w=None):
  """The variance of row r's mixture in rational arithmetic on the float32 inputs (the weights normalised exactly)."""
  M = loc.shape[0]
  ws = [Fraction(1, M)] * M if w is None else [Fraction(float(v)) for v in w]
  tot = sum(ws)
  ws = [v / tot for v in ws]
  mu = [Fraction(float(v)) for v in loc[:, r]]
  sd = [Fraction(float(v)) for v in sigma]
  mean = sum(a * b for a, b in zip(ws, mu))
  return sum(a * (s * s + (m - mean) ** 2) for a, s, m in zip(ws, sd, mu))


def cdf(loc, sigma, x, w=None):
  """F_w(x) per row, float64: loc (M, R), sigma (M,), x (R,) -> (R,)."""
  loc, sigma, x = (np.asarray(a, dtype=np.float64) for a in (loc, sigma, x))
  return _w(w, loc.shape[0]) @ sp.ndtr((x[None, :] - loc) / sigma[:, None])


def ulp32(x):
  return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(F)).astype(np.float64)


def accept(loc, sigma, x, q, w=None):
  """An exact quantile x (R,) float32 at level q -> (residual |F(x) - q32| (R,), first clause (R,) bool, second clause
  (R,) bool).  First: the residual is within QBAR.  Second: F(pred32(x)) <= q32 <= F(succ32(x)) -- the root lies within
  one float32 step of x; where adjacent floats are a good part of a sigma apart no float32 answer meets the first."""
  assert x.dtype == F
  q32 = float(F(q))
  res = np.abs(cdf(loc, sigma, x, w) - q32)
  below = cdf(loc, sigma, np.nextafter(x, F(-np.inf)), w)
  above = cdf(loc, sigma, np.nextafter(x, F(np.inf)), w)
  return res, res <= QBAR, (below <= q32) & (q32 <= above)


def moment_bar(loc, sigma, q, w=None):
  """-> (want, bar): 2 ulp32(want), what a float32 result costs, + 1e-5 sd_mix |z_q|: the rtol = 1e-5 of
  tests/test_gpu_weighted.py's moment-match check applied to the part of the quantile that is not the mean."""
  _, var = mixture_moments(loc, sigma, w)
  want = moment_quantile(loc, sigma, q, w)
  return want, 2.0 * ulp32(want) + 1e-5 * np.sqrt(var) * abs(float(sp.ndtri(q)))


# ---------------------------------------------------------------------------------- k_quantile_root, float32 restatement
def bracket_f32(loc, sigma):
  """k_bracket: [min mu - 5 max sigma, max mu + 5 max sigma] over ALL rows."""
  smax = F(sigma.max())
  return F(loc.min()) - F(5) * smax, F(loc.max()) + F(5) * smax


def _mix_cdf_f32(loc, sigma, x, w):
  """mix_cdf: unweighted a sequential float32 sum over the members divided by M; weighted a sequential float64 sum of
  w_m times the float32 term."""
  z = (x[None, :] - loc) / sigma[:, None]
  nd = F(0.5) * sp.erfc(-z * F(0.70710678118654752440))
  assert nd.dtype == F
  if w is None:
    return np.add.accumulate(nd, axis=0, dtype=F)[-1] / F(loc.shape[0])
  return np.add.accumulate(np.asarray(w)[:, None] * nd.astype(np.float64), axis=0)[-1].astype(F)


def root_f32(loc, sigma, q, w=None, bracket=None):
  """k_quantile_root<WEIGHTED> for every row at once: bracket, vtol = 1e-5, ptol = 1e-8, 60 iterations, the returned end
  the one with the smaller |f|.  -> x (R,) float32."""
  loc, sigma = np.asarray(loc, dtype=F), np.asarray(sigma, dtype=F)
  if w is not None:
    w, loc, sigma = W.kept(w, loc, sigma)
  R = loc.shape[1]
  q = F(q)
  vtol, ptol = F(1e-5), F(1e-8)
  lo, hi = bracket_f32(loc, sigma) if bracket is None else bracket
  a, b = np.full(R, lo, dtype=F), np.full(R, hi, dtype=F)
  with np.errstate(all='ignore'):
    fa, fb = _mix_cdf_f32(loc, sigma, a, w) - q, _mix_cdf_f32(loc, sigma, b, w) - q
    c, fc, t = a.copy(), fa.copy(), np.full(R, 0.5, dtype=F)
    first = np.abs(fa) < np.abs(fb)
    best, fbest = np.where(first, a, b), np.where(first, fa, fb)
    live = np.ones(R, dtype=bool)
    for _ in range(60):
      live &= np.abs(fbest) > vtol
      if not live.any():
        break
      xn = a + t * (b - a)
      fn = _mix_cdf_f32(loc, sigma, xn, w) - q
      same = ((fn > 0) == (fa > 0)) & ((fn < 0) == (fa < 0))
      nc, nfc = np.where(same, a, b), np.where(same, fa, fb)
      nb, nfb = np.where(same, b, a), np.where(same, fb, fa)
      na, nfa = xn, fn
      first = np.abs(nfa) < np.abs(nfb)
      nbest, nfbest = np.where(first, na, nb), np.where(first, nfa, nfb)
      a, fa, b, fb, c, fc = (np.where(live, n, o) for n, o in ((na, a), (nfa, fa), (nb, b), (nfb, fb), (nc, c), (nfc, fc)))
      best, fbest = np.where(live, nbest, best), np.where(live, nfbest, fbest)
      tol = ptol / np.abs(b - c)
      live &= ~((tol > F(0.5)) | (fbest == 0))
      xi, phi = (a - b) / (c - b), (fa - fb) / (fc - fb)
      iqi = (phi * phi < xi) & ((F(1) - phi) * (F(1) - phi) < F(1) - xi)
      tq = (fa / (fb - fa)) * (fc / (fb - fc)) + ((c - a) / (b - a)) * (fa / (fc - fa)) * (fb / (fc - fb))
      nt = np.where(iqi, tq, F(0.5))
      nt = np.fmin(np.fmax(nt, tol), F(1) - tol)             # fminf / fmaxf: a NaN operand gives the other one
      nt = np.where(np.isnan(nt), F(0.5), nt)
      t = np.where(live, nt, t).astype(F)
    for v in (a, b, c, fa, fb, fc, t, best):
      assert v.dtype == F, v.dtype
  return best


# --------------------------------------------------------------------------------------------------------- shared cases
@functools.lru_cache(maxsize=None)
def score_case(M, R, centre, sigma, spread):
  """-> (loc, sigma, y, float64 reference, float32 restatement) of the unweighted scores.  Computed once, read-only."""
  loc, sig, y = case(M, R, centre, sigma, spread)
  ref, f32 = S.normal_ref(loc, sig, y), S.normal_f32(loc, sig, y)
  for a in (loc, sig, y):
    a.setflags(write=False)
  return loc, sig, y, ref, f32


def tail_case(M, centre, R=96):
  """scoring_ref.tail_case around `centre`: |y - mu_m| = 40 sigma_m for every member, either side."""
  rng = np.random.default_rng([7, M, int(abs(centre))])
  sigma = rng.uniform(0.05, 2.0, M).astype(F)
  y = (centre + 3.0 * rng.standard_normal(R)).astype(F)
  side = rng.choice([-1.0, 1.0], (M, R))
  loc = (y[None, :].astype(np.float64) - 40.0 * side * sigma[:, None].astype(np.float64)).astype(F)
  return loc, sigma, y


def shift_case(M, R, seed=0):
  """loc and y multiples of 2^-6 with |value| < 64, and the same shifted by 2^17: both exact in float32 (the step of
  [2^17, 2^18) is 2^-6), so every difference y - mu and mu_i - mu_j has the same bits in the two.
  -> (loc, y, loc + 2^17, y + 2^17, sigma)."""
  rng = np.random.default_rng([seed, M, R, 17])
  grid = lambda shape: rng.integers(-64 * 64 + 1, 64 * 64, shape).astype(np.float64) / 64.0
  loc, y = grid((M, R)), grid(R)
  sigma = rng.uniform(0.01, 3.0, M).astype(F)
  sigma[0] = F(0.01)
  big = 2.0 ** 17
  out = loc.astype(F), y.astype(F), (loc + big).astype(F), (y + big).astype(F), sigma
  assert np.array_equal(out[0].astype(np.float64), loc) and np.array_equal(out[2].astype(np.float64), loc + big)
  assert np.array_equal(out[1].astype(np.float64), y) and np.array_equal(out[3].astype(np.float64), y + big)
  return out
