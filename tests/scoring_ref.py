"""Held-out scoring (bayesnf_amd/csrc/bnf_scoring.h, include/bnf.h bnf_predictive_scores) restated on the host.

Two evaluations of the four outputs from the same float32 inputs (loc (M, R), aux (M, 3), y (R,)):
  `normal_ref` / `count_ref`     float64, built on oracle/bnf_oracle.py (normal_loglik, mixture_cdf, count_forecast,
                                 nb_log_prob, zinb_log_prob, count_cdf); the CRPS is the closed form for a Normal mixture
                                 (Grimit et al. 2006) summed over ALL ordered pairs -- no use of the symmetry the kernel uses;
  `normal_f32` / `count_f32`     numpy float32, operation by operation, of what the kernels evaluate: every per-(member, row)
                                 term float32, every sum over members, pairs and rows float64 -- the accumulation the kernels
                                 use.  (The NORMAL log density is float64 of the float32 difference, rounded once; the count CDF is float64 on the device too, from a float32 softplus: restated so.)
The GPU tests take their bars from `bar(restatement error)`: max(FP32 gate 1e-5, 4 x the restatement's own error); the
factor 4 covers the device's expf / logf / erff differing from numpy's by a few ulp.

Errors: lpd and member_ll |v - ref| / max(1, |ref|); pit absolute; crps |v - ref| / first term of the reference (the
scale of the operands: the score itself is a difference).
"""
import functools

import numpy as np
from scipy import special as sp

from oracle import bnf_oracle as O
from tests import epilogue_f32 as E
from tests import util
from tests.test_gpu_sampling import MEANS, MEAN_F, PI, TC_F, TCS, count_case   # the count grid, shared not copied

F = np.float32
GATE = util.FP32_GATE['loss']
PIT_BAR = 1e-5                   # the value tolerance the project's quantile root finders work to (vtol)
COUNT_CAP = 2.0 ** 24            # the largest count float32 steps through one by one
ROW_TILE, MEMBER_CHUNK = 1024, 8  # include/bnf.h BNF_SCORE_ROW_TILE, BNF_SCORE_MEMBER_CHUNK


def bar(err_f32):
  return max(GATE, 4.0 * err_f32)


def rel1(v, ref):
  """max |v - ref| / max(1, |ref|) over the entries where the reference is finite; NaN must sit where NaN sits."""
  v, ref = np.asarray(v, dtype=np.float64), np.asarray(ref, dtype=np.float64)
  assert np.array_equal(np.isnan(v), np.isnan(ref)), 'NaN pattern differs'
  ok = ~np.isnan(ref)
  if not ok.any():
    return 0.0
  return float(np.max(np.abs(v[ok] - ref[ok]) / np.maximum(1.0, np.abs(ref[ok]))))


def abs_err(v, ref):
  v, ref = np.asarray(v, dtype=np.float64), np.asarray(ref, dtype=np.float64)
  assert np.array_equal(np.isnan(v), np.isnan(ref)), 'NaN pattern differs'
  ok = ~np.isnan(ref)
  return float(np.max(np.abs(v[ok] - ref[ok]))) if ok.any() else 0.0


def crps_err(v, ref):
  """max |crps - ref crps| / ref first term."""
  v = np.asarray(v, dtype=np.float64)
  assert np.array_equal(np.isnan(v), np.isnan(ref['crps'])), 'NaN pattern differs'
  ok = ~np.isnan(ref['crps'])
  return float(np.max(np.abs(v[ok] - ref['crps'][ok]) / ref['crps_first'][ok])) if ok.any() else 0.0


def _mask_rows(out, y):
  """Rows whose y is not finite: NaN in every per-row output (member_ll has left them out already)."""
  bad = ~np.isfinite(y)
  for k in ('lpd', 'crps', 'crps_first'):
    if k in out:
      out[k] = np.where(bad, np.nan, out[k])
  out['pit'] = np.where(bad[None, :], np.nan, out['pit'])
  return out


# ------------------------------------------------------------------------------------------------------ float64 reference
def abs_moment(m, s):
  """A(m, s) = E|m + s Z| = m (2 Phi(m / s) - 1) + 2 s phi(m / s)."""
  z = m / s
  return m * sp.erf(z / np.sqrt(2.0)) + 2.0 * s * np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi)


def normal_crps(loc, sigma, y):
  """-> (crps (R,), first term (R,)): (1 / M) sum_i A(y - mu_i, s_i) - (1 / (2 M^2)) sum_i sum_j A(mu_i - mu_j, s_ij)."""
  M = loc.shape[0]
  first = abs_moment(y[None, :] - loc, sigma[:, None]).sum(axis=0) / M
  pairs = np.zeros(loc.shape[1])
  for i in range(M):
    pairs += abs_moment(loc[i][None, :] - loc, np.sqrt(sigma[i] ** 2 + sigma ** 2)[:, None]).sum(axis=0)
  return first - pairs / (2.0 * M * M), first


def normal_ref(loc, sigma, y):
  loc, sigma, y = (np.asarray(a, dtype=np.float64) for a in (loc, sigma, y))
  fin = np.isfinite(y)
  y0 = np.where(fin, y, 0.0)
  lp = O.normal_loglik(loc, y0[None, :], sigma, per_row=True)
  crps, first = normal_crps(loc, sigma, y0)
  cdf = O.mixture_cdf(loc, sigma, y0)
  out = dict(lp=lp, member_ll=lp[:, fin].sum(axis=1), lpd=sp.logsumexp(lp, axis=0) - np.log(loc.shape[0]),
             pit=np.stack([cdf, cdf]), crps=crps, crps_first=first)
  return _mask_rows(out, y)


def count_ref(fc, y):
  """fc: oracle count_forecast of the float32 inputs (tc (M, 1), logits (M, R), pi (M, 1) or None)."""
  y = np.asarray(y, dtype=np.float64)
  fin = np.isfinite(y)
  y0 = np.where(fin, y, 0.0)
  if fc['pi'] is None:
    lp = O.nb_log_prob(y0[None, :], fc['tc'][:, 0], fc['logits'])
  else:
    lp = O.zinb_log_prob(y0[None, :], fc['tc'][:, 0], fc['logits'], fc['pi'])
  M = lp.shape[0]
  upper = O.count_cdf(fc, y0[None, :]).mean(axis=0)
  lower = np.where(y0 >= 1.0, O.count_cdf(fc, np.maximum(y0 - 1.0, 0.0)[None, :]).mean(axis=0), 0.0)
  out = dict(lp=lp, member_ll=lp[:, fin].sum(axis=1), lpd=sp.logsumexp(lp, axis=0) - np.log(M),
             pit=np.stack([upper, lower]))
  return _mask_rows(out, y)


# --------------------------------------------------------------------------------------------------- float32 restatement
def _running_lse(lp):
  """k_score_rows: running max, the scaled sum carried in float64, members in order -> float32 (R,)."""
  M, R = lp.shape
  mx = np.full(R, -np.inf, dtype=F)
  s = np.zeros(R)
  with np.errstate(all='ignore'):
    for m in range(M):
      nm = np.maximum(mx, lp[m])
      live = nm > -np.inf
      s = np.where(live, s * np.exp(mx - nm).astype(np.float64) + np.exp(lp[m] - nm).astype(np.float64), s)
      mx = np.where(live, nm, mx)
    return mx + np.log((s / M).astype(F))


def _abs_moment_f32(d, c1, c2):
  t = d * c1
  return d * sp.erf(t) + c2 * np.exp(-t * t)


def normal_f32(loc, sigma, y):
  loc, sigma, y = np.asarray(loc, dtype=F), np.asarray(sigma, dtype=F)[:, None], np.asarray(y, dtype=F)
  M = loc.shape[0]
  fin = np.isfinite(y)
  y0 = np.where(fin, y, F(0))[None, :]
  d = y0 - loc
  z = d / sigma
  z64 = d.astype(np.float64) / sigma.astype(np.float64)      # score_log_density: f64 from the f32 difference, rounded once
  lp = (-0.5 * z64 * z64 - np.log(sigma.astype(np.float64)) - 0.918938533204672742).astype(F)
  ndtr = F(0.5) * sp.erfc(-(z) * F(0.70710678118654752440))
  first = _abs_moment_f32(d, F(0.70710678118654752440) / sigma, sigma * F(0.79788456080286535588))
  var = (sigma * sigma)[:, 0]
  pairs = np.zeros(loc.shape[1])
  for i in range(1, M):                         # j < i; the diagonal A(0, s) = 2 s phi(0) is added in closed form
    s2 = (var[i] + var[:i])[:, None]
    rs = F(1) / np.sqrt(s2)
    c1, c2 = rs * F(0.70710678118654752440), (s2 * rs) * F(0.79788456080286535588)
    a = _abs_moment_f32(loc[i][None, :] - loc[:i], c1, c2)
    assert a.dtype == F
    pairs += a.astype(np.float64).sum(axis=0)
  diag = sigma.astype(np.float64).sum()
  for v in (lp, ndtr, first):
    assert v.dtype == F, v.dtype
  cdf = (ndtr.astype(np.float64).sum(axis=0) / M).astype(F)
  crps = (first.astype(np.float64).sum(axis=0) / M - (pairs + diag * 0.56418958354775628695) / (float(M) * M)).astype(F)
  out = dict(lp=lp, member_ll=lp.astype(np.float64)[:, fin].sum(axis=1), lpd=_running_lse(lp), pit=np.stack([cdf, cdf]),
             crps=crps)
  return _mask_rows(out, y)


def count_f32(loc, aux, y, obs):
  """bnf_scoring.h score_log_density for NB / ZINB (tests/epilogue_f32.py `_nb_engine` holds row_loss_eval's forms, which
  it copies), and count_mix_cdf: float64 betainc of a float32 softplus."""
  loc, aux, y = np.asarray(loc, dtype=F), np.asarray(aux, dtype=F), np.asarray(y, dtype=F)
  fin = np.isfinite(y)
  y0 = np.where(fin, y, F(0))[None, :]
  shape = aux[:, 1:2]
  tc = F(1) / shape
  mean = E.softplusf(loc)
  with np.errstate(all='ignore'):
    lp, _, _ = E._nb_engine(y0, tc, shape, mean)   # pylint: disable=protected-access
    if obs == 'ZINB':
      pi = aux[:, 2:3]
      lp = np.where(y0 == 0, np.log((F(1) - pi) * np.exp(lp) + pi), lp + np.log1p(-pi))
  assert lp.dtype == F, lp.dtype
  M = lp.shape[0]
  sm = shape.astype(np.float64) * mean.astype(np.float64)

  def mix_cdf(x):
    c = sp.betainc(np.broadcast_to(1.0 / shape.astype(np.float64), sm.shape), 1.0 + x, sm / (1.0 + sm))
    if obs == 'ZINB':
      pi64 = aux[:, 2:3].astype(np.float64)
      c = pi64 + (1.0 - pi64) * c
    return (c.sum(axis=0) / M).astype(F)
  y64 = y0.astype(np.float64)
  upper = mix_cdf(y64)
  lower = np.where(y64[0] >= 1.0, mix_cdf(np.maximum(y64 - 1.0, 0.0)), F(0))
  out = dict(lp=lp, member_ll=lp.astype(np.float64)[:, fin].sum(axis=1), lpd=_running_lse(lp), pit=np.stack([upper, lower]))
  return _mask_rows(out, y)


# ------------------------------------------------------------------------------------------------------------- the cases
def normal_case(M, R, seed=0):
  """Random loc, per-member sigma in [0.01, 3] (both ends present when M >= 2), y around the members."""
  rng = np.random.default_rng([seed, M, R])
  sigma = rng.uniform(0.01, 3.0, M)
  sigma[0] = 0.01
  if M > 1:
    sigma[-1] = 3.0
  loc = 2.0 * rng.standard_normal((M, R))
  y = loc[rng.integers(0, M, R), np.arange(R)] + 1.5 * rng.standard_normal(R)
  return loc.astype(F), sigma.astype(F), y.astype(F)


def normal_aux(sigma):
  return np.stack([sigma, np.ones_like(sigma), np.zeros_like(sigma)], axis=1).astype(F)


def tail_case(M, R=96):
  """|y - mu_m| / sigma_m = 40 for every member (either side): every member's density is e^-800, below float32 and
  float64's exp alike -- log(mean(exp(lp))) is -inf, the mixture's log density about -800."""
  rng = np.random.default_rng([7, M])
  sigma = rng.uniform(0.05, 2.0, M).astype(F)
  y = (3.0 * rng.standard_normal(R)).astype(F)
  side = rng.choice([-1.0, 1.0], (M, R))
  loc = (y[None, :].astype(np.float64) - 40.0 * side * sigma[:, None].astype(np.float64)).astype(F)
  return loc, sigma, y


def count_grid_model(obs):
  return util.make_problem(n_rows=16, width=64, depth=1, observation_model=obs)[1]


@functools.lru_cache(maxsize=None)
def count_grid_case(obs, tc, M):
  """One grid point of tests/test_gpu_sampling.py's count_case (7 rows, one per grid mean), each row at the four targets
  0, 1, round(mean), round(mean + 3 sd) capped at 2^24 (mean, sd of the grid's own NB(total_count = tc, mean)): 28 rows.
  -> (loc (M, 28), aux (M, 3), y (28,), float64 reference, float32 restatement).  Computed once, shared, read-only."""
  model = count_grid_model(obs)
  loc7, aux, fc7 = count_case(model, tc, M)
  means = np.asarray(MEANS)
  sd = np.sqrt(means * (1.0 + means / tc))
  y = np.minimum(np.concatenate([np.zeros(7), np.ones(7), np.round(means), np.round(means + 3.0 * sd)]), COUNT_CAP)
  loc = np.tile(loc7, (1, 4))
  fc = dict(tc=fc7['tc'], logits=np.tile(fc7['logits'], (1, 4)), pi=fc7['pi'])
  ref, f32 = count_ref(fc, y), count_f32(loc, aux, y, obs)
  for a in (loc, aux, y):
    a.setflags(write=False)
  return loc, aux, y.astype(F), ref, f32


def restatement_errors(ref, f32):
  out = dict(lpd=rel1(f32['lpd'], ref['lpd']), member_ll=rel1(f32['member_ll'], ref['member_ll']),
             pit=abs_err(f32['pit'], ref['pit']))
  if 'crps' in ref:
    out['crps'] = crps_err(f32['crps'], ref)
  return out


def count_grid():
  return [(obs, tc, M) for obs in ('NB', 'ZINB') for M in (1, 7) for tc in TCS]
