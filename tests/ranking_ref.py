"""Ranks of the columns within a sample path and rank probabilities (bayesnf_amd/csrc/bnf_ranking.h, include/bnf.h
bnf_sample_ranks / bnf_rank_probabilities) on the host.  x (S, G): S sample paths of G totals; scale (G,) or None: the
ranked values are v = x / scale, a float64 division.  Rank 1 is the largest value.

  brute force, straight from the definitions
    `ranks_brute`      O(G^2) per path, explicit comparisons in the total order (no sort):  h is above g when v_h > v_g, or
                       when v_g is NaN and v_h is not (a NaN ranks below everything, -inf included); h ties with g when
                       v_h == v_g (so -0.0 ties with +0.0 and +inf with +inf) or both are NaN.
                       above = #above, ties = #ties (>= 1: g itself), rank = above + (ties + 1) / 2
    `rank_prob_ref`    (1 / S) sum_s [above < k <= above + ties] / ties as a fractions.Fraction per cell, rounded once
    `rank_prob_both`[0]  the same for the shapes of the GPU grid, at which a Fraction per cell takes minutes: the terms
                       and their sum in np.longdouble (64-bit significand: at most S non-negative terms, each within 2^-64
                       of 1 / t, so the sum is within 2 S 2^-64 of the cell: 0.03 ulp of float64 at S = 257), rounded to
                       float64 once.  It may differ from the Fraction in the last bit where that lies within 2 S 2^-64 of
                       a rounding boundary; tests/test_ranking_host.py holds it to one ulp of `rank_prob_ref` and counts.
    `ranks_sorted`     above / ties through a sort and two binary searches on the host: the reference at G = 16,384, where
                       the brute force is too slow; cross-checked against it at G = 257.
  the kernel's form, restated in numpy
    `rank_prob_kernel_form`  one float64 sum per cell over the paths in path order of 1.0 / ties, then / S
    (`rank_prob_both`[1]: the two are formed in one pass; `rank_prob_kernel_form_dense` is the restatement as it reads)

Bars:
  rank, above, ties   exact: integers and half-integers are representable
  rank_prob cell      (S + 8) eps x the cell: S non-negative terms, each within eps / 2 of 1 / t, added in a fixed order,
                      one division.  The device is expected to equal `rank_prob_kernel_form` bit for bit (float64 add and
                      divide are correctly rounded and nothing can contract).
"""
import fractions
import functools

import numpy as np

from tests import totals_ref

EPS = 2.0 ** -52
MAX_COLS, CHUNK, MAX_CELLS = 16384, 32, 1 << 24          # BNF_RANK_MAX_COLS, BNF_RANK_PATH_CHUNK, BNF_RANK_MAX_CELLS
KINDS = ('normal', 'count', 'edge')
GRID_G = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1025)
GRID_S = (1, 2, 31, 32, 33, 257)
# the reference of the GPU grid sums in np.longdouble: it must be wider than float64, or it would be the restatement itself
assert np.finfo(np.longdouble).nmant >= 63, 'tests/ranking_ref.py needs a long double with a 64-bit significand'


def values(x, scale=None):
  x = np.asarray(x, dtype=np.float64)
  if scale is None:
    return x
  with np.errstate(divide='ignore', invalid='ignore'):
    return x / np.asarray(scale, dtype=np.float64)[None, :]


# ---- brute force ---------------------------------------------------------------------------------------------------
def ranks_brute(x, scale=None, block=8):
  """-> (rank (S, G) float64, above (S, G) int64, ties (S, G) int64)."""
  v = values(x, scale)
  S, G = v.shape
  above, ties = np.empty((S, G), dtype=np.int64), np.empty((S, G), dtype=np.int64)
  for s0 in range(0, S, block):
    a = v[s0:s0 + block]
    h, g = a[:, :, None], a[:, None, :]                 # [path, h, g]
    nan_h, nan_g = np.isnan(h), np.isnan(g)
    with np.errstate(invalid='ignore'):
      gt = (h > g) | (nan_g & ~nan_h)
      eq = (h == g) | (nan_g & nan_h)
    above[s0:s0 + block] = gt.sum(axis=1)
    ties[s0:s0 + block] = eq.sum(axis=1)
  return above + 0.5 * (ties + 1), above, ties


def ranks_sorted(x, scale=None):
  """The same integers through a sort: NaNs apart (below everything, tied with each other), the rest by np.sort and two
  np.searchsorted (equal values, -0.0 and +0.0 among them, compare equal there)."""
  v = values(x, scale)
  S, G = v.shape
  above, ties = np.empty((S, G), dtype=np.int64), np.empty((S, G), dtype=np.int64)
  for s in range(S):
    nan = np.isnan(v[s])
    w = v[s][~nan]
    ordered = np.sort(w)
    hi = np.searchsorted(ordered, w, side='right')
    ties[s][~nan] = hi - np.searchsorted(ordered, w, side='left')
    above[s][~nan] = w.size - hi
    ties[s][nan] = nan.sum()
    above[s][nan] = w.size
  return above + 0.5 * (ties + 1), above, ties


def rank_prob_ref(above, ties, K):
  """(K, G) float64: every cell an exact Fraction, rounded once."""
  S, G = above.shape
  out = np.empty((K, G))
  for g in range(G):
    a, t = above[:, g].tolist(), ties[:, g].tolist()
    for k in range(1, K + 1):
      total = sum((fractions.Fraction(1, tt) for aa, tt in zip(a, t) if aa < k <= aa + tt), fractions.Fraction(0))
      out[k - 1, g] = float(total / S)
  return out


# ---- the kernel's form ---------------------------------------------------------------------------------------------------
def rank_prob_kernel_form_dense(above, ties, K):
  """The restatement as it reads: every cell visited for every path."""
  S, G = above.shape
  k = np.arange(1, K + 1)[:, None]
  acc = np.zeros((K, G))
  for s in range(S):
    a, t = above[s][None, :], ties[s][None, :]
    acc = acc + np.where((a < k) & (k <= a + t), 1.0 / t.astype(np.float64), 0.0)
  return acc / float(S)


def rank_prob_both(above, ties, K):
  """-> (reference, restatement), both (K, G) float64, in one pass over the paths, a path taken by its tie blocks: the
  columns of a block share (above, ties), so a block of t columns is the rows above .. above + t - 1 of those columns.
  Untied columns (t = 1) are one fancy-indexed add; a tied block adds (1 / t) x its membership row to its slab of rows --
  the columns outside it get + 0.0, which changes no bit of a non-negative sum (a masked add is slower).  A path touches a
  cell at most once, so the additions of every cell are still in path order.  The restatement adds 1.0 / ties in float64 and divides by S; the
  reference adds np.longdouble(1) / ties in np.longdouble and is rounded to float64 once at the end."""
  S, G = above.shape
  acc, wide = np.zeros((K, G)), np.zeros((K, G), dtype=np.longdouble)
  cols = np.arange(G)
  for s in range(S):
    a, t = above[s], ties[s]
    single = (t == 1) & (a < K)
    acc[a[single], cols[single]] += 1.0
    wide[a[single], cols[single]] += np.longdouble(1)
    tied = t > 1
    for a0, t0 in np.unique(np.stack([a[tied], t[tied]], axis=1), axis=0).tolist() if tied.any() else ():
      if a0 < K:
        member = (a == a0) & (t == t0)
        rows = slice(a0, min(a0 + t0, K))
        acc[rows] += (1.0 / np.float64(t0)) * member.astype(np.float64)
        wide[rows] += (np.longdouble(1) / np.longdouble(t0)) * member.astype(np.longdouble)
  return (wide / np.longdouble(S)).astype(np.float64), acc / float(S)


def rank_prob_kernel_form(above, ties, K):
  return rank_prob_both(above, ties, K)[1]


# ---- bars ------------------------------------------------------------------------------------------------------------
def prob_bars(S, ref_prob):
  return (S + 8) * EPS * ref_prob


def same_bits(a, b):
  return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


def check_ranks(tag, got, ref):
  """got / ref: dicts with 'rank', 'above', 'ties' (S, G).  Exact; and the ranks of every path add up to G (G + 1) / 2."""
  G = ref['above'].shape[1]
  for key in ('above', 'ties'):
    assert np.array_equal(np.asarray(got[key], dtype=np.int64), ref[key]), (tag, key)
  assert np.array_equal(got['rank'], ref['rank']), (tag, 'rank')
  assert np.all(np.asarray(got['ties']) >= 1), (tag, 'ties >= 1')
  assert np.array_equal(np.asarray(got['rank']).sum(axis=1), np.full(ref['above'].shape[0], G * (G + 1) / 2.0)), (tag, 'sum')


def check_prob(tag, got, S, ref_prob, form=None):
  """got (K, G) against the brute force at the bar; -> (worst error / bar, cells whose bits differ from the restatement)."""
  err, bar = np.abs(got - ref_prob), prob_bars(S, ref_prob)
  assert not np.isnan(got).any(), (tag, 'NaN')
  over = err > bar
  assert not over.any(), (tag, 'rank_prob', float(err[over].max()), float(bar[over].min()))
  worst = float(np.max(err / np.where(bar > 0, bar, np.inf), initial=0.0))
  differ = 0 if form is None else int((np.asarray(got).view(np.int64) != form.view(np.int64)).sum())
  return worst, differ


# ---- the shared cases (computed once, read-only) ---------------------------------------------------------------------
def _frozen(*arrays):
  for a in arrays:
    if isinstance(a, np.ndarray):
      a.setflags(write=False)


def make_x(S, G, kind, rng):
  if kind == 'normal':                    # continuous: no ties
    return rng.standard_normal((S, G)) * rng.uniform(0.5, 30.0, G)[None, :] + rng.uniform(-20.0, 20.0, G)[None, :]
  if kind == 'count':                     # Poisson with mean 0.7: most cells tie
    return rng.poisson(0.7, (S, G)).astype(np.float64)
  if kind == 'edge':                      # small integers with NaN, +-inf and +-0.0 sprinkled in; paths 0 (mod 4) all equal,
    x = rng.integers(-3, 4, (S, G)).astype(np.float64)                       # paths 1 (mod 4) all distinct
    special = np.asarray([np.nan, np.inf, -np.inf, 0.0, -0.0, np.nan, -0.0])
    pick = rng.random((S, G)) < 0.3
    x[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
    x[0::4] = 2.5
    for s in range(1, S, 4):
      x[s] = rng.permutation(G).astype(np.float64) - G // 2
    return x
  raise ValueError(kind)


def make_scale(G, kind, rng):
  if kind == 'normal':
    return rng.uniform(0.5, 3.0, G)
  return rng.integers(1, 4, G).astype(np.float64)       # small integer divisors: the quotients still tie


@functools.lru_cache(maxsize=None)
def ranking_case(S, G, kind, scaled=False):
  """-> (x (S, G), scale (G,) or None, ref) with ref = dict(rank, above, ties) from the brute force."""
  rng = np.random.default_rng([S, G, KINDS.index(kind), 31])
  x = make_x(S, G, kind, rng)
  scale = make_scale(G, kind, rng) if scaled else None
  rank, above, ties = ranks_brute(x, scale)
  _frozen(x, scale, rank, above, ties)
  return x, scale, dict(rank=rank, above=above, ties=ties)


def prob_case(S, G, kind, scaled, K):
  """-> (reference (K, G), restatement (K, G)) of the case's rank probabilities.  Not kept: one test reads each, and the
  K = G matrices of the grid would add up to 100 MB per kind."""
  ref = ranking_case(S, G, kind, scaled)[2]
  return rank_prob_both(ref['above'], ref['ties'], K)


# ---- the scores of a ranking ---------------------------------------------------------------------------------------------
def graded_case(seed, S=1000, G=12):
  """x_sg = 10 g + N(0, 10^2): the groups are graded, neighbours overlap; y one more draw -> (x, y)."""
  rng = np.random.default_rng(seed)
  level = 10.0 * np.arange(G)
  return level[None, :] + 10.0 * rng.standard_normal((S, G)), level + 10.0 * rng.standard_normal(G)


def mean_rank_crps(x, y):
  """The mean over the groups of the CRPS of the forecast mid-ranks of x against the observed mid-ranks of y."""
  rank = ranks_brute(x)[0]
  observed = ranks_brute(y[None, :])[0][0]
  return float(np.mean(totals_ref.summaries_sorted(rank, observed, ())['crps']))
