"""Stacking of the ensemble members (bayesnf_amd/csrc/bnf_stacking.h, include/bnf.h bnf_member_log_density /
bnf_stacking_weights) restated on the host in float64.

  logdens_ref(obs, loc, aux, y)   the matrix L (M, R) of per-member log densities from the float32 inputs, built on
                                  oracle/bnf_oracle.py (normal_loglik, nb_log_prob, zinb_log_prob); NaN columns where y is
                                  not finite
  lse, objective, grad, gap       of a matrix L at weights w: lse_r = log sum_m w_m exp(L_mr); a row is SCORED when it holds
                                  no NaN and lse_r is finite, DROPPED when it holds no NaN and lse_r is not; f = mean of lse
                                  over the scored rows, g_m = mean of exp(L_mr - lse_r), gap = max g - 1
  em(L, w0, max_iter, tol)        the update w <- w g (renormalised) until gap <= tol or max_iter updates; everything it
                                  reports is evaluated at the weights it returns

The gap is a bound, not a tuned tolerance: f is concave with gradient g, so f(w*) - f(w) <= sum_m w*_m g_m - 1 <= gap.
"""
import numpy as np
from scipy import special as sp

from oracle import bnf_oracle as O
from tests import scoring_ref as S    # the count grid of tests/test_gpu_sampling.py comes through it, shared not copied

F = np.float32
ROW_TILE = 1024                        # include/bnf.h BNF_STACK_ROW_TILE
CONVERGENCE_SHAPES = ((2, 65), (7, 1025), (65, 2049), (257, 65))
BLOCK_SIZES = (3, 64, 1, 200, 757)


def logdens_ref(obs, loc, aux, y):
  loc, aux, y = (np.asarray(a, dtype=np.float64) for a in (loc, aux, y))
  fin = np.isfinite(y)
  y0 = np.where(fin, y, 0.0)[None, :]
  if obs == 'NORMAL':
    lp = O.normal_loglik(loc, y0, aux[:, 0], per_row=True)
  else:
    shape = aux[:, 1]
    tc = 1.0 / shape
    logits = -np.log(shape)[:, None] - np.log(O.softplus(loc))
    lp = O.nb_log_prob(y0, tc, logits) if obs == 'NB' else O.zinb_log_prob(y0, tc, logits, aux[:, 2:3])
  return np.where(fin[None, :], lp, np.nan)


def lse(L, w):
  """log sum_m w_m exp(L_mr) (R,): -inf where every weighted member is at -inf, NaN where the row holds a NaN."""
  L, w = np.asarray(L, dtype=np.float64), np.asarray(w, dtype=np.float64)
  pos = w > 0
  with np.errstate(all='ignore'):
    out = sp.logsumexp(L[pos], b=w[pos][:, None], axis=0)
  return np.where(np.isnan(L).any(axis=0), np.nan, out)


def rows(L, w):
  """-> (lse, scored mask, dropped mask)"""
  v = lse(L, w)
  nan = np.isnan(L).any(axis=0)
  scored = ~nan & np.isfinite(v)
  return v, scored, ~nan & ~scored


def objective(L, w):
  v, scored, _ = rows(L, w)
  return float(np.mean(v[scored])) if scored.any() else float('nan')


def grad(L, w):
  v, scored, _ = rows(L, w)
  if not scored.any():
    return np.full(np.shape(L)[0], np.nan)
  with np.errstate(all='ignore'):
    return np.exp(np.asarray(L, dtype=np.float64)[:, scored] - v[scored][None, :]).mean(axis=1)


def gap(L, w):
  return float(np.max(grad(L, w)) - 1.0)


def em(L, w0, max_iter, tol, trajectory=False):
  """-> dict(weights, objective, objective_start, gap, iterations, dropped[, trajectory: the weights of every iterate])."""
  w = np.array(w0, dtype=np.float64)
  f0 = objective(L, w)
  path = [w.copy()]
  it = 0
  while True:
    g = grad(L, w)
    gp = float(np.max(g) - 1.0)
    if not gp > tol or it >= max_iter:        # NaN (no scored row) stops too
      break
    w = w * g
    w = w / w.sum()
    it += 1
    path.append(w.copy())
  out = dict(weights=w, objective=objective(L, w), objective_start=f0, gap=gp, iterations=it,
             dropped=int(rows(L, w)[2].sum()))
  if trajectory:
    out['trajectory'] = path
  return out


# ------------------------------------------------------------------------------------------------------------- the cases
def normal_case(M, R, seed=None):
  """A NORMAL ensemble around a common truth: -> (loc (M, R), sigma (M,), y (R,)) float32, the inputs
  bnf_member_log_density takes.  One generator, the draws in the order truth, member offsets, noise, sigma, y."""
  rng = np.random.default_rng(100 * M + R if seed is None else seed)
  truth = rng.standard_normal(R)
  offset = rng.standard_normal(M)
  noise = rng.standard_normal((M, R))
  sigma = rng.uniform(0.3, 2.0, M)
  y = truth + 0.5 * rng.standard_normal(R)
  loc = truth[None, :] + 0.5 * offset[:, None] + 0.3 * noise
  return loc.astype(F), sigma.astype(F), y.astype(F)


def normal_L(loc, sigma, y):
  """The NORMAL log density of the float32 inputs, rounded to float32 and widened again: a matrix the device can be handed
  bit for bit."""
  return logdens_ref('NORMAL', loc, S.normal_aux(sigma), y).astype(F).astype(np.float64)


def block_case(sizes, dead=0):
  """L[m][r] = 0 on member m's own block of rows, -inf elsewhere (plus `dead` members at -inf everywhere): the optimum is
  w_m = n_m / n, reached by ONE update from uniform.  -> L (len(sizes) + dead, sum(sizes)) float32"""
  n = int(sum(sizes))
  L = np.full((len(sizes) + dead, n), -np.inf, dtype=F)
  r0 = 0
  for m, k in enumerate(sizes):
    L[m, r0:r0 + k] = 0.0
    r0 += k
  return L
