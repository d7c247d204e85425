"""The ranked probability score of NB / ZINB forecasts (bayesnf_amd/csrc/bnf_rps.h, include/bnf.h bnf_count_rps) restated
on the host: rps_r = sum_{k >= 0} (F_r(k) - 1{k >= y_r})^2 with F_r the equal-weight mixture CDF.

Two evaluations from the same float32 inputs (loc (M, R), aux (M, 3), y (R,)):
  `count_rps_ref`   float64, brute force: every term from k = 0 up to scipy's nbinom.isf(1e-13) of the widest member (and
                    past y), the CDF from oracle/bnf_oracle.py count_cdf (scipy's betainc at every k).  No window logic.
                    Left out: terms (1 - F)^2 < 1e-26.
  `count_rps_f64`   the kernel's own algorithm in numpy: float32 softplus, then float64 -- anchor at floor(mean) (pmf from
                    lgamma, cdf from one betainc), the pmf recurrence down to a_m, tiles of 64 k from a_r = min a_m summed
                    until every member's geometric tail bound is under eps at the end of a tile, closed-form terms outside,
                    the cap.  The recurrences are numpy cumprod / cumsum: the kernel's operations in the kernel's order up to
                    the association of one product per step (1e-16 per step).
The GPU tests take their bars from `bar(restatement error)`: max(1e-5, 4 x the restatement's own error at that input), the
project's rule (tests/scoring_ref.py).  Error measure: |v - ref| / |ref|; the score is strictly positive on every case here.
"""
import functools

import numpy as np
from scipy import special as sp
from scipy import stats

from oracle import bnf_oracle as O
from tests import epilogue_f32 as E
from tests import scoring_ref as S
from tests.test_gpu_sampling import MEANS, TCS, count_case

F = np.float32
EPS = 1e-9                        # bnf_rps.h kRpsEps
TILE = 64                         # bnf_rps.h kRpsTile
MAX_TERMS = 1 << 20               # include/bnf.h BNF_RPS_MAX_TERMS
GRID_MEANS = MEANS[:5]            # 0.02 .. 400
bar = S.bar


def rel_err(v, ref):
  """max |v - ref| / |ref| over the rows where the reference is finite; NaN must sit where NaN sits."""
  v, ref = np.asarray(v, dtype=np.float64), np.asarray(ref, dtype=np.float64)
  assert np.array_equal(np.isnan(v), np.isnan(ref)), ('NaN pattern differs', np.isnan(v).nonzero(), np.isnan(ref).nonzero())
  ok = ~np.isnan(ref)
  return float(np.max(np.abs(v[ok] - ref[ok]) / np.abs(ref[ok]))) if ok.any() else 0.0


def valid_target(y):
  y = np.asarray(y, dtype=np.float64)
  with np.errstate(invalid='ignore'):
    return np.isfinite(y) & (y >= 0) & (y == np.floor(y))


# ------------------------------------------------------------------------------------------------------ float64 reference
def count_rps_ref(fc, y):
  """fc: oracle count_forecast of the float32 inputs (tc (M, 1), logits (M, R), pi (M, 1) or None) -> (R,) float64."""
  y = np.asarray(y, dtype=np.float64)
  ok = valid_target(y)
  out = np.full(y.shape, np.nan)
  cdfs = {}
  for r in np.nonzero(ok)[0]:
    key = fc['logits'][:, r].tobytes()
    if key not in cdfs:
      kmax = float(np.max(stats.nbinom.isf(1e-13, fc['tc'][:, 0], sp.expit(-fc['logits'][:, r]))))
      k = np.arange(0.0, kmax + 2.0)
      cdfs[key] = O.count_cdf(dict(tc=fc['tc'], logits=fc['logits'][:, r:r + 1], pi=fc['pi']), k[None, :]).mean(axis=0)
    cdf = cdfs[key]
    n = min(int(y[r]), len(cdf))
    out[r] = np.sum(cdf[:n] ** 2) + np.sum((cdf[n:] - 1.0) ** 2) + max(0.0, y[r] - len(cdf))
  return out


def rps_by_expectations(pmf, ys):
  """E|X - y| - 0.5 E|X - X'| for every y of `ys`, from an explicit pmf vector on 0 .. len(pmf) - 1: the other form of
  the CRPS."""
  k = np.arange(len(pmf), dtype=np.float64)
  pairs = float(pmf @ np.abs(k[:, None] - k[None, :]) @ pmf)
  return np.asarray([float(pmf @ np.abs(k - y)) - 0.5 * pairs for y in ys])


# ------------------------------------------------------------------------------------------- the kernel's algorithm, numpy
def _window(s, mean, pi):
  """One row: s = aux[:, 1], mean = float32 softplus(loc), pi = aux[:, 2] (zeros for NB), all float64 (M,).
  -> None (capped) or (a_r, mixture cdf on a_r .. a_r + n_terms - 1)."""
  M = len(s)
  sm = s * mean
  tc, q = 1.0 / s, 1.0 / (1.0 + sm)
  ks = np.floor(tc / sm)
  pm0 = np.exp(sp.gammaln(ks + tc) - sp.gammaln(ks + 1.0) - sp.gammaln(tc) - tc * np.log1p(1.0 / sm) - ks * np.log1p(sm))
  cd0 = sp.betainc(tc, 1.0 + ks, sm / (1.0 + sm))
  a, pm_a, cd_a = np.zeros(M), np.zeros(M), np.zeros(M)
  for m in range(M):                                   # down from the anchor: state i is k = k* - i
    n = int(min(ks[m], MAX_TERMS))
    k = ks[m] - np.arange(n)
    pms = pm0[m] * np.concatenate([[1.0], np.cumprod(k * (1.0 / q[m]) / (k - 1.0 + tc[m]))])
    cds = cd0[m] - np.concatenate([[0.0], np.cumsum(pms[:-1])])
    stop = ~((ks[m] - np.arange(n + 1) > 0) & (cds - pms >= EPS))
    if not stop.any():
      return None
    i = int(np.argmax(stop))
    a[m], pm_a[m], cd_a[m] = ks[m] - i, pms[i], cds[i]
  a_r = float(a.min())
  tcm1 = tc - 1.0
  L = 16 * TILE
  while True:
    L = min(L, MAX_TERMS)
    G, P = np.zeros((M, L + 1)), np.zeros((M, L + 1))
    for m in range(M):
      i0 = int(a[m] - a_r)
      if i0 <= L:
        k = a[m] + np.arange(L - i0)
        pm = pm_a[m] * np.concatenate([[1.0], np.cumprod(q[m] * (1.0 + tcm1[m] * (1.0 / (k + 1.0))))])
        P[m, i0:] = pm
        G[m, i0:] = cd_a[m] + np.concatenate([[0.0], np.cumsum(pm[1:])])
    ends = np.arange(TILE, L + 1, TILE)
    kn = a_r + ends
    rr = np.maximum(q[:, None], q[:, None] * (1.0 + tcm1[:, None] / (kn + 1.0)))
    done = ((kn > ks[:, None]) & (kn > a[:, None]) & (P[:, ends] < EPS * (1.0 - rr))).all(axis=0)
    if done.any():
      n_terms = int(ends[np.argmax(done)])
      break
    if L >= MAX_TERMS:
      return None
    L *= 4
  acc = np.zeros(n_terms)
  for m in range(M):                                   # members in order, as a tile column is added
    acc += pi[m] + (1.0 - pi[m]) * G[m, :n_terms]
  return a_r, acc / M


def count_rps_f64(loc, aux, y, obs):
  """-> (rps (R,) float32 with NaN where the kernel gives NaN, window lengths b_r - a_r (R,), window starts a_r (R,) --
  both -1 where the row is capped or not scored)."""
  loc, aux, y = np.asarray(loc, dtype=F), np.asarray(aux, dtype=F), np.asarray(y, dtype=F)
  M, R = loc.shape
  s = aux[:, 1].astype(np.float64)
  pi = aux[:, 2].astype(np.float64) if obs == 'ZINB' else np.zeros(M)
  p0 = 0.0
  for m in range(M):
    p0 += pi[m]
  p0 /= M
  mean = E.softplusf(loc)
  assert mean.dtype == F
  out, terms, starts = np.full(R, np.nan, dtype=F), np.full(R, -1, dtype=np.int64), np.full(R, -1, dtype=np.int64)
  windows = {}
  for r in np.nonzero(valid_target(y))[0]:
    key = loc[:, r].tobytes()
    if key not in windows:
      windows[key] = _window(s, mean[:, r].astype(np.float64), pi)
    if windows[key] is None:
      continue
    a_r, cdf = windows[key]
    yd = float(y[r])
    k = a_r + np.arange(len(cdf))
    d = cdf - (k >= yd)
    n_lt = min(yd, a_r)
    out[r] = F(p0 * p0 * n_lt + (1.0 - p0) * (1.0 - p0) * (a_r - n_lt) + np.sum(d * d) + max(yd - (a_r + len(cdf)), 0.0))
    terms[r], starts[r] = len(cdf), int(a_r)
  return out, terms, starts


# ------------------------------------------------------------------------------------------------------------- the cases
def grid_targets(means, tc):
  """Four targets per row: 0, 1, round(mean), round(mean + 3 sd) (mean, sd of the grid's own NB(tc, mean))."""
  means = np.asarray(means, dtype=np.float64)
  sd = np.sqrt(means * (1.0 + means / tc))
  return np.concatenate([np.zeros(len(means)), np.ones(len(means)), np.round(means), np.round(means + 3.0 * sd)])


@functools.lru_cache(maxsize=None)
def grid_case(obs, tc, M):
  """One grid point of tests/test_gpu_sampling.py's count_case restricted to its first five means, every row at the four
  targets: 20 rows.  -> (loc (M, 20), aux (M, 3), y (20,), float64 reference, restatement, restatement's window lengths).
  Computed once, shared, read-only."""
  model = S.count_grid_model(obs)
  loc7, aux, fc7 = count_case(model, tc, M)
  n = len(GRID_MEANS)
  y = grid_targets(GRID_MEANS, tc)
  loc = np.tile(loc7[:, :n], (1, 4))
  fc = dict(tc=fc7['tc'], logits=np.tile(fc7['logits'][:, :n], (1, 4)), pi=fc7['pi'])
  ref = count_rps_ref(fc, y)
  f64, terms, _ = count_rps_f64(loc, aux, y, obs)
  for a in (loc, aux, y, ref, f64, terms):
    a.setflags(write=False)
  return loc, aux, y.astype(F), ref, f64, terms


def grid():
  return [(obs, tc, M) for obs in ('NB', 'ZINB') for M in (1, 7) for tc in TCS]


def forecast(model, loc, aux):
  """The oracle's count_forecast of float32 device inputs (loc (M, R), aux (M, 3)): the reference's view of them."""
  from tests.test_gpu_sampling import inv_softplus
  aux = np.asarray(aux, dtype=np.float64)
  theta = np.zeros((aux.shape[0], model.P))
  theta[:, model.leaf['shape'].offset] = inv_softplus(aux[:, 1])
  theta[:, model.leaf['inflated_loc_probs'].offset] = np.log(aux[:, 2]) - np.log1p(-aux[:, 2])
  return O.count_forecast(model, theta, np.asarray(loc, dtype=np.float64))


def many_member_case(obs, M=70, R=65, tc=3.0):
  """M components and R rows that are no multiple of the 64-member chunk: the grid's member factors repeated with a
  deterministic jitter, the rows cycling through the first five grid means and the four kinds of target."""
  from tests.test_gpu_sampling import MEAN_F, PI, TC_F, inv_softplus
  j = np.arange(M)
  jit = 1.0 + 0.01 * ((j * 37) % 11 - 5)
  tcs = tc * np.asarray(TC_F)[j % 7] * jit
  row_means = np.asarray(GRID_MEANS)[np.arange(R) % 5]
  means = row_means[None, :] * (np.asarray(MEAN_F)[j % 7] * jit[::-1])[:, None]
  aux = np.stack([np.ones(M), 1.0 / tcs, np.clip(PI * jit, 0.01, 0.9)], axis=1).astype(F)
  loc = inv_softplus(tcs[:, None] ** 2 / means).astype(F)
  sd = np.sqrt(row_means * (1.0 + row_means / tc))
  kind = (np.arange(R) // 5) % 4
  y = np.choose(kind, [np.zeros(R), np.ones(R), np.round(row_means), np.round(row_means + 3.0 * sd)])
  return loc, aux, y.astype(F)
