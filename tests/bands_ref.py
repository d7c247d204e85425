"""Simultaneous bands of an ensemble of sample paths (bayesnf_amd/csrc/bnf_bands.h, include/bnf.h bnf_sample_depths /
bnf_depth_levels / bnf_sample_envelope) on the host: a numpy restatement of the definitions -- np.sort, searchsorted and a
sort of the depths -- not of the kernels.  x (S, C): S sample paths of C columns; col_group (C,) the group of every column,
an entry outside [0, G) takes no part.  Everything is an integer, a value picked from x, or one float64 division of a count
by S: the GPU is held to EXACT equality.

  d[s][c]  = min(#{t : x_tc <= x_sc}, #{t : x_tc >= x_sc}) - 1; -1 for every path in a column that holds a NaN
  D[s][g]  = min of d[s][c] over the columns of g; NONE for a group without columns
  band k   = [x_(k), x_(S-1-k)] of the sorted column
  od[c]    = min(#{x_tc <= y_c}, #{x_tc >= y_c}) - 1 for y_c not NaN (-1 in a NaN column); OD[g] = min over g's columns
numpy's comparisons are the kernel's total order on what they meet here: -0.0 == +0.0, infinities of one sign tie."""
import numpy as np

NONE = 0x7fffffff                     # BNF_DEPTH_NONE
MAX_LEVELS = 64                       # BNF_BAND_MAX_LEVELS
MAX_SAMPLES = 16384                   # BNF_SUMMARY_MAX_SAMPLES


def need_of(coverage, S):
  """ceil(coverage S - 1e-9) clamped to [1, S] (inference.band_need)."""
  return max(1, min(int(S), int(np.ceil(float(coverage) * int(S) - 1e-9))))


def _depth_in(srt, v):
  """min(#{srt <= v}, #{srt >= v}) - 1 for the sorted column srt and the values v."""
  le = np.searchsorted(srt, v, side='right')
  ge = srt.size - np.searchsorted(srt, v, side='left')
  return np.minimum(le, ge).astype(np.int64) - 1


def column_depths(x):
  """d (S, C) int64."""
  x = np.asarray(x, dtype=np.float64)
  d = np.empty(x.shape, dtype=np.int64)
  for c in range(x.shape[1]):
    col = x[:, c]
    d[:, c] = -1 if np.isnan(col).any() else _depth_in(np.sort(col), col)
  return d


def group_depths(x, col_group, G, depth=None):
  """D (S, G) int64, lowered from `depth` (None: all NONE) as the entry point lowers it."""
  x = np.asarray(x, dtype=np.float64)
  col_group = np.asarray(col_group)
  D = np.full((x.shape[0], G), NONE, dtype=np.int64) if depth is None else np.array(depth, dtype=np.int64)
  d = column_depths(x)
  for c in range(x.shape[1]):
    g = int(col_group[c])
    if 0 <= g < G:
      D[:, g] = np.minimum(D[:, g], d[:, c])
  return D


def observed_depths(x, col_group, G, y, obs_depth=None):
  """OD (G,) int64: NONE for a group none of whose columns has an observed value."""
  x = np.asarray(x, dtype=np.float64)
  OD = np.full(G, NONE, dtype=np.int64) if obs_depth is None else np.array(obs_depth, dtype=np.int64)
  for c in range(x.shape[1]):
    g = int(col_group[c])
    if not 0 <= g < G or np.isnan(y[c]):
      continue
    col = x[:, c]
    od = -1 if np.isnan(col).any() else int(_depth_in(np.sort(col), np.asarray([y[c]]))[0])
    OD[g] = min(OD[g], od)
  return OD


def depth_levels(D, need, k_query=(), OD=None):
  """-> dict: level (n_cov, G) int64, achieved (n_cov, G), joint (n_query, G), obs_pit (2, G) with OD.  A group with a
  depth outside [-1, S - 1] is empty: level -1, NaN ratios."""
  D = np.asarray(D, dtype=np.int64)
  S, G = D.shape
  empty = ((D < -1) | (D > S - 1)).any(axis=0)
  desc = -np.sort(-D, axis=0)                                # every group's depths, largest first
  level = np.full((len(need), G), -1, dtype=np.int64)
  achieved = np.full((len(need), G), np.nan)
  for i, n in enumerate(need):
    assert 1 <= n <= S
    k = desc[n - 1]                                          # the need-th largest
    level[i] = np.where(empty, -1, k)
    achieved[i] = np.where(empty, np.nan, (D >= k[None, :]).sum(axis=0) / S)
  out = {'level': level, 'achieved': achieved,
         'joint': np.asarray([np.where(empty, np.nan, (D >= k).sum(axis=0) / S) for k in k_query]).reshape(len(k_query), G)}
  if OD is not None:
    OD = np.asarray(OD, dtype=np.int64)
    ok = ~empty & (OD >= -1) & (OD <= S - 1)
    out['obs_pit'] = np.stack([np.where(ok, (D <= OD[None, :]).sum(axis=0) / S, np.nan),
                               np.where(ok, (D < OD[None, :]).sum(axis=0) / S, np.nan)])
  return out


def envelope(x, col_group, level):
  """lower, upper (n_levels, C): x_(k) and x_(S-1-k), k = level[j][group of c]; NaN for k outside [0, S - 1], a column
  that takes no part and one holding a NaN."""
  x = np.asarray(x, dtype=np.float64)
  level = np.asarray(level)
  S, C = x.shape
  L, G = level.shape
  lower, upper = np.full((L, C), np.nan), np.full((L, C), np.nan)
  for c in range(C):
    g = int(col_group[c])
    if not 0 <= g < G or np.isnan(x[:, c]).any():
      continue
    srt = np.sort(x[:, c])
    for j in range(L):
      k = int(level[j, g])
      if 0 <= k <= S - 1:
        lower[j, c], upper[j, c] = srt[k], srt[S - 1 - k]
  return lower, upper


def inside(x, lower, upper, cols):
  """Per path: does it lie inside [lower, upper] at every column of `cols` (by the definition, not by the depth)."""
  x = np.asarray(x, dtype=np.float64)
  return np.all((x[:, cols] >= lower[cols][None, :]) & (x[:, cols] <= upper[cols][None, :]), axis=1)


def band_summaries(x, col_group, G, coverage, y=None):
  """What inference.band_summaries returns, per COLUMN of x (the caller maps positions to table rows)."""
  x = np.asarray(x, dtype=np.float64)
  S = x.shape[0]
  need = [need_of(c, S) for c in coverage]
  k_pw = [(S - n) // 2 for n in need]
  D = group_depths(x, col_group, G)
  OD = None if y is None else observed_depths(x, col_group, G, y)
  lev = depth_levels(D, need, k_pw, OD)
  out = {'level': lev['level'], 'coverage': lev['achieved'], 'pointwise_joint_coverage': lev['joint']}
  out['lower'], out['upper'] = envelope(x, col_group, lev['level'])
  out['pointwise_lower'], out['pointwise_upper'] = envelope(x, col_group, np.repeat(np.asarray(k_pw)[:, None], G, axis=1))
  if y is not None:
    seen = OD != NONE
    out['observed_depth'] = np.where(seen, OD.astype(np.float64), np.nan)
    out['inside'] = np.where(seen[None, :], (OD[None, :] >= lev['level']).astype(np.float64), np.nan)
    out['depth_pit'] = lev['obs_pit']
  return out


KINDS = ('normal', 'count', 'edge')


def band_case(S, C, G, kind, seed=0):
  """A synthetic matrix -> (x (S, C) float64, col_group (C,) int32, y (C,)).  'normal': continuous, strongly dependent
  along the columns (a random walk per path); 'count': Poisson, mostly zeros -- ties everywhere; 'edge': the count
  matrix with an all-equal column, a column of +-0.0, one of +-inf and finite values, and a NaN column.  col_group is a
  random interleaving of the G groups plus entries of -1 and G (out of range); y has NaN entries and values outside the
  envelope of all paths."""
  rng = np.random.default_rng([S, C, G, KINDS.index(kind), seed])
  if kind == 'normal':
    x = np.cumsum(rng.standard_normal((S, C)), axis=1)
  else:
    x = rng.poisson(0.3, size=(S, C)).astype(np.float64)
  col_group = rng.integers(-1, G + 1, size=C).astype(np.int32)
  if kind == 'edge':
    own = np.flatnonzero((col_group >= 0) & (col_group < G))
    pick = own[np.linspace(0, own.size - 1, 4).astype(int)] if own.size >= 4 else own
    if pick.size >= 1:
      x[:, pick[0]] = 3.0
    if pick.size >= 2:
      x[:, pick[1]] = np.where(rng.random(S) < 0.5, -0.0, 0.0)
    if pick.size >= 3:
      x[:, pick[2]] = rng.choice([-np.inf, -1.0, 0.0, 2.5, np.inf], size=S)
    if pick.size >= 4 and G > 1:
      x[0 if S < 3 else 2, pick[3]] = np.nan
  y = x[rng.integers(0, S, size=C), np.arange(C)].copy()     # a value of some path at every column: inside the envelope
  y[rng.random(C) < 0.2] = np.nan
  far = rng.random(C) < 0.1
  y[far] = np.where(rng.random(int(far.sum())) < 0.5, -1e9, 1e9)
  return x, col_group, y
