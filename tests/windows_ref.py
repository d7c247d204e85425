"""Host reference of the moving-window totals of sample paths (bayesnf_amd/csrc/bnf_windows.h, include/bnf.h
bnf_predictive_group_windows).  Deliberately naive: a Python loop per path, group and position with `np.sum` in float64
over the draws of the clipped window (0 where a position takes no part) -- no sliding update, no difference of running
totals; peak, row, count and the per-row counters are read off that matrix.

Positions: a group's positions in `seg_rows` order are its time axis, and a window is counted in POSITIONS.  A position
whose entry of seg_rows lies outside [0, R) takes no part: it occupies a slot of the window, adds nothing, is never NaN
and is never a candidate.  A NaN draw makes exactly the windows that hold it NaN.  A CANDIDATE is a participating
position with at least min(w, the group's size) positions of its group up to and including it: the full-length windows,
and for a group shorter than w the one window that is the whole group."""
import numpy as np


def candidates(seg_offsets, seg_rows, n_table_rows, window):
  """(len(seg_rows),) bool: a full-length window ends at the position and the position takes part."""
  off = np.asarray(seg_offsets, dtype=np.int64)
  rows = np.asarray(seg_rows, dtype=np.int64)
  cand = np.zeros(len(rows), dtype=bool)
  for g in range(len(off) - 1):
    a, b = int(off[g]), int(off[g + 1])
    need = min(int(window), b - a)
    for p in range(a, b):
      cand[p] = 0 <= rows[p] < n_table_rows and p - a + 1 >= need
  return cand


def from_windows(win, seg_offsets, seg_rows, n_table_rows, window, threshold=None):
  """Peak, row, count and the per-row counters recomputed from a (S, positions) matrix of window totals alone, with the
  rules of the contract: the largest candidate window that is not NaN, the earliest position among equal ones (NaN and
  -1 without one); `win > threshold[g]` strict and false for NaN -> dict: 'peak' (S, G) float64, 'peak_row' (S, G)
  int32, 'peak_count' (R,) int64 and, with a threshold, 'count' (S, G) float64, 'exceed_count' (R,) int64."""
  win = np.asarray(win, dtype=np.float64)
  S = win.shape[0]
  off = np.asarray(seg_offsets, dtype=np.int64)
  rows = np.asarray(seg_rows, dtype=np.int64)
  G, R = len(off) - 1, int(n_table_rows)
  cand = candidates(off, rows, R, window)
  out = dict(peak=np.full((S, G), np.nan), peak_row=np.full((S, G), -1, dtype=np.int32),
             peak_count=np.zeros(R, dtype=np.int64))
  if threshold is not None:
    threshold = np.asarray(threshold, dtype=np.float64)
    out.update(count=np.zeros((S, G), dtype=np.float64), exceed_count=np.zeros(R, dtype=np.int64))
  for g in range(G):
    idx = np.arange(off[g], off[g + 1])[cand[off[g]:off[g + 1]]]
    if idx.size == 0:
      continue
    for s in range(S):
      v = win[s, idx]
      seen = np.flatnonzero(~np.isnan(v))
      if seen.size:
        at = seen[np.argmax(v[seen])]                       # np.argmax: the first of equal values
        out['peak'][s, g] = v[at]
        out['peak_row'][s, g] = rows[idx[at]]
        out['peak_count'][rows[idx[at]]] += 1
      if threshold is not None:
        above = v > threshold[g]
        out['count'][s, g] = float(above.sum())
        out['exceed_count'][rows[idx[above]]] += 1
  return out


def group_windows(x, seg_offsets, seg_rows, window, threshold=None):
  """x (S, R) draws, CSR (seg_offsets, seg_rows) with positions in time order, window w >= 1, threshold (G,) f64 or None
  -> dict: 'window' (S, len(seg_rows)) float64 by POSITION, the clipped sum at every position; 'candidate'
  (len(seg_rows),) bool; and what `from_windows` reads off that matrix."""
  x = np.asarray(x).astype(np.float64)                        # the float32 draws widened, exactly
  S, R = x.shape
  off = np.asarray(seg_offsets, dtype=np.int64)
  rows = np.asarray(seg_rows, dtype=np.int64)
  w = int(window)
  assert w >= 1
  win = np.zeros((S, len(rows)), dtype=np.float64)
  part = (rows >= 0) & (rows < R)
  # the draws by position, 0 where none takes part: a window of a path is one contiguous block
  by_pos = np.ascontiguousarray(np.where(part[None, :], x[:, np.where(part, rows, 0)], 0.0))
  for s in range(S):
    path, to = by_pos[s], win[s]
    for g in range(len(off) - 1):
      a, b = int(off[g]), int(off[g + 1])
      for p in range(a, b):
        to[p] = np.sum(path[max(a, p - w + 1):p + 1])
  out = from_windows(win, off, rows, R, w, threshold)
  out.update(window=win, candidate=candidates(off, rows, R, w))
  return out


def undecided(ref, bound, seg_offsets, threshold=None):
  """(S, G) bool: the (path, group) cells in which the reference does not decide by more than the bound -- another
  candidate window lies within the sum of the two bounds of the largest one (the peak row could differ), or a candidate
  lies within its bound of the threshold.  ref as `group_windows` returns it, bound (S, positions) >= the error of a
  window at the position (all zero for counts: every cell is decided, equal windows tie by position in both)."""
  win, cand = ref['window'], ref['candidate']
  off = np.asarray(seg_offsets, dtype=np.int64)
  S, G = ref['peak'].shape
  out = np.zeros((S, G), dtype=bool)
  if not np.any(np.nan_to_num(bound) > 0):
    return out
  for g in range(G):
    idx = np.arange(off[g], off[g + 1])[cand[off[g]:off[g + 1]]]
    for s in range(S):
      v, e = win[s, idx], bound[s, idx]
      seen = ~np.isnan(v)
      v, e = v[seen], e[seen]
      if v.size >= 2:
        top = int(np.argmax(v))
        margin = (v[top] - e[top]) - (v + e)                # > 0: the largest window stays the largest
        margin[top] = np.inf
        out[s, g] |= bool(np.any(margin <= 0))
      if threshold is not None and v.size:
        out[s, g] |= bool(np.any(np.abs(v - threshold[g]) <= e))
  return out
