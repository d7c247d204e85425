"""Host reference of the running totals of sample paths and of when they pass a level
(bayesnf_amd/csrc/bnf_cumulative.h, include/bnf.h bnf_predictive_group_cumulative).  Deliberately naive: a Python loop per
path and group with `np.cumsum` in float64 over the participating positions of the float32 draws, and the crossing
quantities read off that running sum.

Positions: a group's positions in `seg_rows` order are its time axis.  A position whose entry of seg_rows lies outside
[0, R) takes no part: its running total is the value carried so far (0 at a group's start) and it is not a step.  A NaN
draw takes part: every later running total of its group is NaN, it counts as a step, and `run > level` is false for it."""
import numpy as np


def crossing_of(run, level):
  """One path, one group: `run` the running totals at the participating positions in time order.
  -> (cross_step, index of the crossing position among them or -1, above): the first index with run > level (strict,
  false for NaN), censored at len(run) when there is none."""
  above = run > level
  hit = np.flatnonzero(above)
  return (float(hit[0]), int(hit[0]), above) if hit.size else (float(len(run)), -1, above)


def group_cumulative(x, seg_offsets, seg_rows, level=None):
  """x (S, R) draws, CSR (seg_offsets, seg_rows) with positions in time order, level (G,) f64 or None -> dict:
  'running' (S, len(seg_rows)) float64 by POSITION; 'steps' (len(seg_rows),) int64, the participating positions of the
  group up to and including each position; 'total' (S, G) float64; with a level 'cross_step' (S, G) float64, 'cross_row'
  (S, G) int32 (-1 if none), 'cross_count', 'above_count' (R,) int64."""
  x = np.asarray(x)
  S, R = x.shape
  off = np.asarray(seg_offsets, dtype=np.int64)
  rows = np.asarray(seg_rows, dtype=np.int64)
  G = len(off) - 1
  out = {'running': np.zeros((S, len(rows)), dtype=np.float64), 'steps': np.zeros(len(rows), dtype=np.int64),
         'total': np.zeros((S, G), dtype=np.float64)}
  if level is not None:
    level = np.asarray(level, dtype=np.float64)
    out.update(cross_step=np.zeros((S, G), dtype=np.float64), cross_row=np.full((S, G), -1, dtype=np.int32),
               cross_count=np.zeros(R, dtype=np.int64), above_count=np.zeros(R, dtype=np.int64))
  for g in range(G):
    a, b = int(off[g]), int(off[g + 1])
    seg = rows[a:b]
    part = (seg >= 0) & (seg < R)
    r = seg[part]
    if r.size == 0:
      continue                                             # run 0 everywhere, total 0, censored at 0 steps, row -1
    idx = np.cumsum(part) - 1                               # the last participating position at or before each position
    out['steps'][a:b] = idx + 1
    for s in range(S):
      run = np.cumsum(x[s, r].astype(np.float64))
      out['running'][s, a:b] = np.where(idx >= 0, run[np.maximum(idx, 0)], 0.0)
      out['total'][s, g] = run[-1]
      if level is not None:
        step, at, above = crossing_of(run, level[g])
        out['cross_step'][s, g] = step
        out['above_count'][r[above]] += 1
        if at >= 0:
          out['cross_row'][s, g] = r[at]
          out['cross_count'][r[at]] += 1
  return out


def crossings_from_running(running, seg_offsets, seg_rows, n_table_rows, level):
  """The crossing outputs recomputed from a (S, positions) matrix of running totals alone (the GPU's own), with the same
  rules -> dict as `group_cumulative` without 'running', 'steps' and 'total'."""
  S = running.shape[0]
  off = np.asarray(seg_offsets, dtype=np.int64)
  rows = np.asarray(seg_rows, dtype=np.int64)
  G, R = len(off) - 1, int(n_table_rows)
  out = dict(cross_step=np.zeros((S, G), dtype=np.float64), cross_row=np.full((S, G), -1, dtype=np.int32),
             cross_count=np.zeros(R, dtype=np.int64), above_count=np.zeros(R, dtype=np.int64))
  for g in range(G):
    a, b = int(off[g]), int(off[g + 1])
    seg = rows[a:b]
    part = (seg >= 0) & (seg < R)
    r = seg[part]
    if r.size == 0:
      continue
    for s in range(S):
      step, at, above = crossing_of(running[s, a:b][part], level[g])
      out['cross_step'][s, g] = step
      out['above_count'][r[above]] += 1
      if at >= 0:
        out['cross_row'][s, g] = r[at]
        out['cross_count'][r[at]] += 1
  return out


def normal_bound(x, seg_offsets, seg_rows):
  """n 2^-52 cumsum(|x|) per (path, position), n the participating positions of the group so far: twice the standard
  bound gamma_{n-1} sum |x| on the error of a float64 sum of n terms in ANY order, so it covers the difference of two
  orders.  NaN where the running total is NaN."""
  x = np.asarray(x)
  ref = group_cumulative(np.abs(x), seg_offsets, seg_rows)
  return ref['steps'][None, :] * 2.0 ** -52 * ref['running']
