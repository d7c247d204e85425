"""The marginal forecast of the WEIGHTED mixture of members (include/bnf.h bnf_normal_mixture_quantiles_weighted,
bnf_count_mixture_quantiles_weighted, bnf_predictive_scores_weighted, bnf_count_rps_weighted) restated on the host: the
weighted forms of what tests/scoring_ref.py and tests/rps_ref.py hold for equal weights.

From the same float32 inputs (loc (M, R), aux (M, 3) or sigma (M,), y (R,)) and float64 weights w (M,) on the simplex:
  `normal_ref` / `count_ref` / `count_rps_ref`   float64, built on oracle/bnf_oracle.py (_ndtr, normal_loglik, count_cdf,
                                nb_log_prob, zinb_log_prob): lpd = log sum_m w_m p_m, pit = sum_m w_m F_m, the Normal CRPS
                                sum_i w_i A_i - (1 / 2) sum_ij w_i w_j A_ij over ALL ordered pairs (no use of the symmetry or
                                of the closed-form diagonal the kernel uses), the RPS by brute force over every k;
  `normal_f32` / `count_f32` / `count_rps_f64`   what the kernels evaluate, operation by operation: every per-(member, row)
                                term float32, every sum over members float64 of w_m times the term converted to double, no
                                division by M.  They start as the engine wrappers do, by dropping the members of weight 0.
Bars: `scoring_ref.bar` (max(1e-5, 4 x the restatement's own error)) with the error measures of scoring_ref / rps_ref; no
tolerance of its own.
"""
import functools

import numpy as np
from scipy import special as sp
from scipy import stats

from oracle import bnf_oracle as O
from tests import epilogue_f32 as E
from tests import rps_ref as P
from tests import scoring_ref as S
from tests.test_gpu_sampling import inv_softplus

F = np.float32
PATTERNS = ('uniform', 'dirichlet', 'one_hot', 'every_second_zero', 'tiny_outlier')
TINY = 1e-12


def weights(pattern, M, seed=0):
  """(M,) float64 on the simplex (sum within 1e-15 of 1).  'dirichlet': Dirichlet(0.3), spiky; 'one_hot': all on member
  M // 2; 'every_second_zero': members 1, 3, ... at exactly 0, the others equal; 'tiny_outlier': 1e-12 on the last member
  (which `outlier_normal` / `outlier_count` move away from the others), the rest equal."""
  if pattern == 'uniform' or M == 1:
    return np.full(M, 1.0 / M)
  if pattern == 'dirichlet':
    w = np.random.default_rng([seed, M, 11]).dirichlet(np.full(M, 0.3))
    return w / w.sum()
  if pattern == 'one_hot':
    w = np.zeros(M)
    w[M // 2] = 1.0
    return w
  if pattern == 'every_second_zero':
    w = np.zeros(M)
    w[0::2] = 1.0 / len(w[0::2])
    return w
  assert pattern == 'tiny_outlier', pattern
  w = np.full(M, (1.0 - TINY) / (M - 1))
  w[-1] = TINY
  return w


def outlier_normal(loc):
  """The last member 25 away from the others (sigma <= 3): it widens the quantile bracket and carries next to no mass."""
  loc = np.array(loc, dtype=F)
  if loc.shape[0] > 1:
    loc[-1] += F(25.0)
  return loc


def outlier_count(loc):
  """The last member's mean x 8 (its softplus(loc) / 8: the NB mean is total_count^2 / softplus(loc))."""
  loc = np.array(loc, dtype=F)
  if loc.shape[0] > 1:
    loc[-1] = inv_softplus(np.logaddexp(loc[-1].astype(np.float64), 0.0) / 8.0).astype(F)
  return loc


def kept(w, *per_member):
  """The engine wrappers' first step: the members with w_m != 0."""
  w = np.asarray(w, dtype=np.float64)
  keep = w != 0
  return (w[keep],) + tuple(np.asarray(a)[keep] for a in per_member)


def keep_fc(fc, w):
  keep = np.asarray(w) != 0
  return dict(tc=fc['tc'][keep], logits=fc['logits'][keep], pi=None if fc['pi'] is None else fc['pi'][keep])


# ------------------------------------------------------------------------------------------------------ float64 reference
def normal_cdf(loc, sigma, x, w):
  """F_w(x) per row: loc (M, R), sigma (M,), x (R,) -> (R,)."""
  loc, sigma, x, w = (np.asarray(a, dtype=np.float64) for a in (loc, sigma, x, w))
  return w @ O._ndtr((x[None, :] - loc) / sigma[:, None])   # pylint: disable=protected-access


def count_cdf(fc, x, w):
  """F_w(x) per row at x (R,) >= 0 (continuous in x, as the root finder sees it)."""
  return np.asarray(w, dtype=np.float64) @ O.count_cdf(fc, np.asarray(x, dtype=np.float64)[None, :])


def normal_moment_quantile(loc, sigma, q, w):
  loc, sigma, w = (np.asarray(a, dtype=np.float64) for a in (loc, sigma, w))
  mean = w @ loc
  var = w @ (sigma[:, None] ** 2 + loc ** 2) - mean ** 2
  return mean + np.sqrt(np.maximum(var, 0.0)) * sp.ndtri(q)


def normal_crps(loc, sigma, y, w):
  """-> (crps (R,), first term (R,)): sum_i w_i A(y - mu_i, s_i) - (1 / 2) sum_i sum_j w_i w_j A(mu_i - mu_j, s_ij)."""
  M = loc.shape[0]
  first = w @ S.abs_moment(y[None, :] - loc, sigma[:, None])
  pairs = np.zeros(loc.shape[1])
  for i in range(M):
    pairs += w[i] * (w @ S.abs_moment(loc[i][None, :] - loc, np.sqrt(sigma[i] ** 2 + sigma ** 2)[:, None]))
  return first - 0.5 * pairs, first


def normal_ref(loc, sigma, y, w):
  loc, sigma, y, w = (np.asarray(a, dtype=np.float64) for a in (loc, sigma, y, w))
  fin = np.isfinite(y)
  y0 = np.where(fin, y, 0.0)
  lp = O.normal_loglik(loc, y0[None, :], sigma, per_row=True)
  crps, first = normal_crps(loc, sigma, y0, w)
  cdf = normal_cdf(loc, sigma, y0, w)
  with np.errstate(divide='ignore'):
    lpd = sp.logsumexp(lp + np.log(w)[:, None], axis=0)
  out = dict(lp=lp, lpd=lpd, pit=np.stack([cdf, cdf]), crps=crps, crps_first=first)
  return S._mask_rows(out, y)   # pylint: disable=protected-access


def count_ref(fc, y, w):
  y, w = np.asarray(y, dtype=np.float64), np.asarray(w, dtype=np.float64)
  fin = np.isfinite(y)
  y0 = np.where(fin, y, 0.0)
  if fc['pi'] is None:
    lp = O.nb_log_prob(y0[None, :], fc['tc'][:, 0], fc['logits'])
  else:
    lp = O.zinb_log_prob(y0[None, :], fc['tc'][:, 0], fc['logits'], fc['pi'])
  upper = count_cdf(fc, y0, w)
  lower = np.where(y0 >= 1.0, count_cdf(fc, np.maximum(y0 - 1.0, 0.0), w), 0.0)
  with np.errstate(divide='ignore'):
    lpd = sp.logsumexp(lp + np.log(w)[:, None], axis=0)
  return S._mask_rows(dict(lp=lp, lpd=lpd, pit=np.stack([upper, lower])), y)   # pylint: disable=protected-access


def count_rps_ref(fc, y, w):
  """Brute force as rps_ref.count_rps_ref with F_r = sum_m w_m F_{m,r}; the sum runs to the widest member of positive
  weight (a member of weight 0 adds nothing to F)."""
  y, w = np.asarray(y, dtype=np.float64), np.asarray(w, dtype=np.float64)
  pos = w > 0
  out = np.full(y.shape, np.nan)
  cdfs = {}
  for r in np.nonzero(P.valid_target(y))[0]:
    key = fc['logits'][:, r].tobytes()
    if key not in cdfs:
      kmax = float(np.max(stats.nbinom.isf(1e-13, fc['tc'][pos, 0], sp.expit(-fc['logits'][pos, r]))))
      k = np.arange(0.0, kmax + 2.0)
      cdfs[key] = w @ O.count_cdf(dict(tc=fc['tc'], logits=fc['logits'][:, r:r + 1], pi=fc['pi']), k[None, :])
    cdf = cdfs[key]
    n = min(int(y[r]), len(cdf))
    out[r] = np.sum(cdf[:n] ** 2) + np.sum((cdf[n:] - 1.0) ** 2) + max(0.0, y[r] - len(cdf))
  return out


# --------------------------------------------------------------------------------------------------- float32 restatement
def _running_lse(lp, w):
  """k_score_rows<WEIGHTED>: running max over the members' lp, s = s e^(mx - nm) + w_m e^(lp_m - nm) in float64."""
  M, R = lp.shape
  mx = np.full(R, -np.inf, dtype=F)
  s = np.zeros(R)
  with np.errstate(all='ignore'):
    for m in range(M):
      nm = np.maximum(mx, lp[m])
      live = nm > -np.inf
      s = np.where(live, s * np.exp(mx - nm).astype(np.float64) + w[m] * np.exp(lp[m] - nm).astype(np.float64), s)
      mx = np.where(live, nm, mx)
    return mx + np.log(s.astype(F))


def normal_f32(loc, sigma, y, w):
  w, loc, sigma = kept(w, np.asarray(loc, dtype=F), np.asarray(sigma, dtype=F))
  sigma, y = sigma[:, None], np.asarray(y, dtype=F)
  M = loc.shape[0]
  fin = np.isfinite(y)
  y0 = np.where(fin, y, F(0))[None, :]
  d = y0 - loc
  z = d / sigma
  z64 = d.astype(np.float64) / sigma.astype(np.float64)      # score_log_density: f64 from the f32 difference, rounded once
  lp = (-0.5 * z64 * z64 - np.log(sigma.astype(np.float64)) - 0.918938533204672742).astype(F)
  ndtr = F(0.5) * sp.erfc(-(z) * F(0.70710678118654752440))
  first = S._abs_moment_f32(d, F(0.70710678118654752440) / sigma, sigma * F(0.79788456080286535588))   # pylint: disable=protected-access
  var = (sigma * sigma)[:, 0]
  pairs = np.zeros(loc.shape[1])
  for i in range(1, M):                         # j < i, each term times w_i w_j
    s2 = (var[i] + var[:i])[:, None]
    rs = F(1) / np.sqrt(s2)
    c1, c2 = rs * F(0.70710678118654752440), (s2 * rs) * F(0.79788456080286535588)
    a = S._abs_moment_f32(loc[i][None, :] - loc[:i], c1, c2)   # pylint: disable=protected-access
    assert a.dtype == F
    pairs += (w[i] * w[:i]) @ a.astype(np.float64)
  diag = (w * w) @ sigma[:, 0].astype(np.float64)
  for v in (lp, ndtr, first):
    assert v.dtype == F, v.dtype
  cdf = (w @ ndtr.astype(np.float64)).astype(F)
  crps = (w @ first.astype(np.float64) - (pairs + diag * 0.56418958354775628695)).astype(F)
  return S._mask_rows(dict(lp=lp, lpd=_running_lse(lp, w), pit=np.stack([cdf, cdf]), crps=crps), y)   # pylint: disable=protected-access


def count_mix_cdf_f32(loc, aux, x, obs, w):
  """count_mix_cdf<WEIGHTED>: float64 betainc of a float32 softplus, w_m times it, -> float32.  x (R,) float64."""
  w, loc, aux = kept(w, np.asarray(loc, dtype=F), np.asarray(aux, dtype=F))
  shape = aux[:, 1:2].astype(np.float64)
  sm = shape * E.softplusf(loc).astype(np.float64)
  c = sp.betainc(np.broadcast_to(1.0 / shape, sm.shape), 1.0 + np.asarray(x, dtype=np.float64)[None, :], sm / (1.0 + sm))
  if obs == 'ZINB':
    pi64 = aux[:, 2:3].astype(np.float64)
    c = pi64 + (1.0 - pi64) * c
  return (w @ c).astype(F)


def count_f32(loc, aux, y, obs, w):
  wk, lock, auxk = kept(w, np.asarray(loc, dtype=F), np.asarray(aux, dtype=F))
  y = np.asarray(y, dtype=F)
  fin = np.isfinite(y)
  y0 = np.where(fin, y, F(0))[None, :]
  shape = auxk[:, 1:2]
  with np.errstate(all='ignore'):
    lp, _, _ = E._nb_engine(y0, F(1) / shape, shape, E.softplusf(lock))   # pylint: disable=protected-access
    if obs == 'ZINB':
      pi = auxk[:, 2:3]
      lp = np.where(y0 == 0, np.log((F(1) - pi) * np.exp(lp) + pi), lp + np.log1p(-pi))
  assert lp.dtype == F, lp.dtype
  y64 = y0[0].astype(np.float64)
  upper = count_mix_cdf_f32(loc, aux, y64, obs, w)
  lower = np.where(y64 >= 1.0, count_mix_cdf_f32(loc, aux, np.maximum(y64 - 1.0, 0.0), obs, w), F(0))
  return S._mask_rows(dict(lp=lp, lpd=_running_lse(lp, wk), pit=np.stack([upper, lower])), y)   # pylint: disable=protected-access


def _window(s, mean, pi, w):
  """rps_ref._window with the member weights: the same anchors, walks, tiles and stop; the tile column is
  sum_m w_m (pi_m + (1 - pi_m) cdf_m), members in order, and is not divided by M."""
  M = len(s)
  sm = s * mean
  tc, q = 1.0 / s, 1.0 / (1.0 + sm)
  ks = np.floor(tc / sm)
  pm0 = np.exp(sp.gammaln(ks + tc) - sp.gammaln(ks + 1.0) - sp.gammaln(tc) - tc * np.log1p(1.0 / sm) - ks * np.log1p(sm))
  cd0 = sp.betainc(tc, 1.0 + ks, sm / (1.0 + sm))
  a, pm_a, cd_a = np.zeros(M), np.zeros(M), np.zeros(M)
  for m in range(M):
    n = int(min(ks[m], P.MAX_TERMS))
    k = ks[m] - np.arange(n)
    pms = pm0[m] * np.concatenate([[1.0], np.cumprod(k * (1.0 / q[m]) / (k - 1.0 + tc[m]))])
    cds = cd0[m] - np.concatenate([[0.0], np.cumsum(pms[:-1])])
    stop = ~((ks[m] - np.arange(n + 1) > 0) & (cds - pms >= P.EPS))
    if not stop.any():
      return None
    i = int(np.argmax(stop))
    a[m], pm_a[m], cd_a[m] = ks[m] - i, pms[i], cds[i]
  a_r = float(a.min())
  tcm1 = tc - 1.0
  L = 16 * P.TILE
  while True:
    L = min(L, P.MAX_TERMS)
    G, Pm = np.zeros((M, L + 1)), np.zeros((M, L + 1))
    for m in range(M):
      i0 = int(a[m] - a_r)
      if i0 <= L:
        k = a[m] + np.arange(L - i0)
        pm = pm_a[m] * np.concatenate([[1.0], np.cumprod(q[m] * (1.0 + tcm1[m] * (1.0 / (k + 1.0))))])
        Pm[m, i0:] = pm
        G[m, i0:] = cd_a[m] + np.concatenate([[0.0], np.cumsum(pm[1:])])
    ends = np.arange(P.TILE, L + 1, P.TILE)
    kn = a_r + ends
    rr = np.maximum(q[:, None], q[:, None] * (1.0 + tcm1[:, None] / (kn + 1.0)))
    done = ((kn > ks[:, None]) & (kn > a[:, None]) & (Pm[:, ends] < P.EPS * (1.0 - rr))).all(axis=0)
    if done.any():
      n_terms = int(ends[np.argmax(done)])
      break
    if L >= P.MAX_TERMS:
      return None
    L *= 4
  acc = np.zeros(n_terms)
  for m in range(M):
    acc += w[m] * (pi[m] + (1.0 - pi[m]) * G[m, :n_terms])
  return a_r, acc


def count_rps_f64(loc, aux, y, obs, w):
  """-> (rps (R,) float32 with NaN where the kernel gives NaN, window lengths (R,), -1 where capped or not scored)."""
  w, loc, aux = kept(w, np.asarray(loc, dtype=F), np.asarray(aux, dtype=F))
  y = np.asarray(y, dtype=F)
  M, R = loc.shape
  s = aux[:, 1].astype(np.float64)
  pi = aux[:, 2].astype(np.float64) if obs == 'ZINB' else np.zeros(M)
  p0 = 0.0
  for m in range(M):
    p0 += w[m] * pi[m]
  mean = E.softplusf(loc)
  assert mean.dtype == F
  out, terms = np.full(R, np.nan, dtype=F), np.full(R, -1, dtype=np.int64)
  windows = {}
  for r in np.nonzero(P.valid_target(y))[0]:
    key = loc[:, r].tobytes()
    if key not in windows:
      windows[key] = _window(s, mean[:, r].astype(np.float64), pi, w)
    if windows[key] is None:
      continue
    a_r, cdf = windows[key]
    yd = float(y[r])
    k = a_r + np.arange(len(cdf))
    d = cdf - (k >= yd)
    n_lt = min(yd, a_r)
    out[r] = F(p0 * p0 * n_lt + (1.0 - p0) * (1.0 - p0) * (a_r - n_lt) + np.sum(d * d) + max(yd - (a_r + len(cdf)), 0.0))
    terms[r] = len(cdf)
  return out, terms


# ------------------------------------------------------------------------------------------------------------- the cases
SCORE_MEMBERS_NORMAL = (1, 2, 7, S.MEMBER_CHUNK + 1, 2 * S.MEMBER_CHUNK + 4)   # 20: three chunks, the last one short
SCORE_MEMBERS_COUNT = (1, 7, 9)
SCORE_ROWS = (1, 63, 64, 65, S.ROW_TILE + 1)
RPS_MEMBERS = (1, 7, 64, 65, 70)
RPS_ROWS = 65
RPS_GRID_TCS = (0.3, 3.0, 1e3)


def normal_case(M, R, pattern):
  """scoring_ref.normal_case with the weights of `pattern`; 'tiny_outlier' moves the last member away."""
  loc, sigma, y = S.normal_case(M, R)
  if pattern == 'tiny_outlier':
    loc = outlier_normal(loc)
  return loc, sigma, y, weights(pattern, M)


def count_members(obs, M, R, tc=3.0):
  """rps_ref.many_member_case: M members (the grid's member factors with a jitter) x R rows over the first five grid
  means (<= 400) and the four kinds of target."""
  return P.many_member_case(obs, M=M, R=R, tc=tc)


def count_case_w(obs, M, R, pattern, tc=3.0):
  loc, aux, y = count_members(obs, M, R, tc)
  if pattern == 'tiny_outlier':
    loc = outlier_count(loc)
  return loc, aux, y, weights(pattern, M)


@functools.lru_cache(maxsize=None)
def rps_case(obs, M, pattern):
  """One RPS case of the GPU test -> (loc, aux, y, w, float64 reference, restatement, its window lengths).  Computed once,
  shared, read-only."""
  loc, aux, y, w = count_case_w(obs, M, RPS_ROWS, pattern)
  ref = count_rps_ref(P.forecast(S.count_grid_model(obs), loc, aux), y, w)
  f64, terms = count_rps_f64(loc, aux, y, obs, w)
  for a in (loc, aux, y, w, ref, f64, terms):
    a.setflags(write=False)
  return loc, aux, y, w, ref, f64, terms


@functools.lru_cache(maxsize=None)
def rps_grid_case(obs, tc, pattern):
  """rps_ref.grid_case (M = 7, means <= 400, four targets per row: 20 rows) with weights."""
  loc, aux, y, _, _, _ = P.grid_case(obs, tc, 7)
  w = weights(pattern, 7)
  if pattern == 'tiny_outlier':
    loc = outlier_count(loc)
  fc = P.forecast(S.count_grid_model(obs), loc, aux)
  ref = count_rps_ref(fc, y, w)
  f64, terms = count_rps_f64(loc, aux, y, obs, w)
  for a in (w, ref, f64, terms):
    a.setflags(write=False)
  return loc, aux, y, w, ref, f64, terms


def rps_cases():
  """Every (kind, obs, key, pattern) the GPU RPS test runs; `rps_get` builds it."""
  out = [('members', obs, M, p) for obs in ('NB', 'ZINB') for M in RPS_MEMBERS for p in PATTERNS]
  out += [('grid', obs, tc, p) for obs in ('NB', 'ZINB') for tc in RPS_GRID_TCS for p in PATTERNS]
  return out


def rps_get(kind, obs, key, pattern):
  return rps_case(obs, key, pattern) if kind == 'members' else rps_grid_case(obs, key, pattern)
