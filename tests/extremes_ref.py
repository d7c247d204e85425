"""Host reference of the group peaks and threshold exceedances of sample paths (bayesnf_amd/csrc/bnf_extremes.h,
include/bnf.h bnf_predictive_group_extremes): plain numpy on the (S, R) matrix of draws `Engine.predictive_samples`
returns for the same seed.  Per path and group, over the group's rows in ascending table row,
  max     the largest draw, a NaN draw counted as -inf
  argmax  the first table row at which it is reached (np.argmax takes the first of equal values)
  count   the rows whose draw is > their threshold (a NaN draw never is)
An empty group gives (NaN, -1, 0).  Everything is exact: max, argmax and integer counts have no rounding."""
import numpy as np


def group_extremes(x, codes, n_groups, threshold=None):
  """x (S, R) draws, codes (R,) the group of every table row, threshold (R,) or None ->
  dict(max (S, G) f64, argmax (S, G) int32, peak_count (R,) int64[, count (S, G) f64, exceed_count (R,) int64])."""
  x = np.asarray(x)
  S, R = x.shape
  codes = np.asarray(codes)
  v = np.where(np.isnan(x), -np.inf, x).astype(np.float64)
  out = {'max': np.full((S, n_groups), np.nan), 'argmax': np.full((S, n_groups), -1, dtype=np.int32),
         'peak_count': np.zeros(R, dtype=np.int64)}
  above = None
  if threshold is not None:
    with np.errstate(invalid='ignore'):
      above = x > np.asarray(threshold)[None, :]              # False for a NaN draw
    out['count'] = np.zeros((S, n_groups))
    out['exceed_count'] = above.sum(axis=0).astype(np.int64)
  for g in range(n_groups):
    rows = np.flatnonzero(codes == g)                         # ascending table row
    if rows.size == 0:
      continue
    first = np.argmax(v[:, rows], axis=1)
    out['max'][:, g] = v[np.arange(S), rows[first]]
    out['argmax'][:, g] = rows[first]
    np.add.at(out['peak_count'], rows[first], 1)
    if above is not None:
      out['count'][:, g] = above[:, rows].sum(axis=1)
  return out


def tie_share(x, codes, n_groups):
  """Share of the (path, non-empty group) cells in which the maximum is reached at more than one row."""
  x = np.asarray(x)
  v = np.where(np.isnan(x), -np.inf, x)
  tied = cells = 0
  for g in range(n_groups):
    rows = np.flatnonzero(np.asarray(codes) == g)
    if rows.size:
      tied += int(((v[:, rows] == v[:, rows].max(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
      cells += x.shape[0]
  return tied / max(1, cells)
