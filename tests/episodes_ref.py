"""Host reference of the spells above a threshold in sample paths (bayesnf_amd/csrc/bnf_episodes.h, include/bnf.h
bnf_predictive_group_episodes).  Two independent statements:

`group_episodes`: deliberately naive -- a Python loop per path and group over the ordered draws, one position at a time.
`piece_of`, `join`, `IDENTITY`: a restatement of the kernel's piece and join operator, so that the operator's own
properties (associative, not commutative, identity) can be checked on the CPU against the naive loop.

Positions: a group's positions in `seg_rows` order are its time axis.  A position whose entry of seg_rows lies outside
[0, R) takes no part (it neither breaks a run nor counts as a step); a NaN draw takes part and does not exceed."""
import numpy as np

FIELDS = ('len', 'lead', 'pre', 'suf', 'suf_pos', 'best', 'best_pos', 'runs', 'first', 'last')
NONE = -1
IDENTITY = dict(len=0, lead=0, pre=0, suf=0, suf_pos=NONE, best=0, best_pos=NONE, runs=0, first=NONE, last=NONE)


def naive_episodes(above, positions):
  """One path, one group: `above` the booleans of the participating positions in time order, `positions` their labels.
  -> (longest, longest_pos, spells, onset_step, first_pos, last_pos), the scan a reader would write by hand."""
  longest, longest_pos, spells, onset, first, last = 0, NONE, 0, None, NONE, NONE
  run, run_pos = 0, NONE
  for step, (a, p) in enumerate(zip(above, positions)):
    if a:
      if run == 0:
        run_pos = p
        spells += 1
      run += 1
      if run > longest:                      # strict: the earliest of equally long runs keeps the title
        longest, longest_pos = run, run_pos
      if onset is None:
        onset, first = step, p
      last = p
    else:
      run = 0
  return longest, longest_pos, spells, (len(above) if onset is None else onset), first, last


def group_episodes(x, seg_offsets, seg_rows, threshold):
  """x (S, R) draws, CSR (seg_offsets, seg_rows) with positions in time order, threshold (R,) f32 -> dict:
  'longest', 'spells', 'onset_step' (S, G) float64; 'longest_row', 'first_row', 'last_row' (S, G) int32 table rows (-1 if
  none); 'onset_count' (R,) int64."""
  x = np.asarray(x)
  S, R = x.shape
  off = np.asarray(seg_offsets, dtype=np.int64)
  rows = np.asarray(seg_rows, dtype=np.int64)
  thr = np.asarray(threshold, dtype=np.float32)
  G = len(off) - 1
  out = {k: np.zeros((S, G), dtype=np.float64) for k in ('longest', 'spells', 'onset_step')}
  out.update({k: np.full((S, G), -1, dtype=np.int32) for k in ('longest_row', 'first_row', 'last_row')})
  out['onset_count'] = np.zeros(R, dtype=np.int64)
  for g in range(G):
    r = rows[off[g]:off[g + 1]]
    r = r[(r >= 0) & (r < R)]
    if r.size == 0:
      continue
    above = x[:, r] > thr[r][None, :]          # False for a NaN draw
    for s in range(S):
      longest, lrow, spells, onset, first, last = naive_episodes(above[s].tolist(), r.tolist())
      out['longest'][s, g], out['spells'][s, g], out['onset_step'][s, g] = longest, spells, onset
      out['longest_row'][s, g], out['first_row'][s, g], out['last_row'][s, g] = lrow, first, last
      if first >= 0:
        out['onset_count'][first] += 1
  return out


def piece_of(exceeds, pos):
  """The piece of ONE participating position."""
  if exceeds:
    return dict(len=1, lead=0, pre=1, suf=1, suf_pos=pos, best=1, best_pos=pos, runs=1, first=pos, last=pos)
  return dict(len=1, lead=1, pre=0, suf=0, suf_pos=NONE, best=0, best_pos=NONE, runs=0, first=NONE, last=NONE)


def join(a, b):
  """a BEFORE b."""
  r = {}
  r['len'] = a['len'] + b['len']
  r['lead'] = a['len'] + b['lead'] if a['best'] == 0 else a['lead']
  r['pre'] = a['len'] + b['pre'] if a['pre'] == a['len'] else a['pre']
  b_all = b['suf'] == b['len']
  r['suf'] = b['len'] + a['suf'] if b_all else b['suf']
  r['suf_pos'] = a['suf_pos'] if (b_all and a['suf'] > 0) else b['suf_pos']
  mid = a['suf'] + b['pre']
  mid_pos = a['suf_pos'] if a['suf'] > 0 else b['first']
  r['best'], r['best_pos'] = a['best'], a['best_pos']
  if mid > r['best']:
    r['best'], r['best_pos'] = mid, mid_pos
  if b['best'] > r['best']:
    r['best'], r['best_pos'] = b['best'], b['best_pos']
  r['runs'] = a['runs'] + b['runs'] - (1 if (a['suf'] > 0 and b['pre'] > 0) else 0)
  r['first'] = a['first'] if a['first'] >= 0 else b['first']
  r['last'] = b['last'] if b['last'] >= 0 else a['last']
  return r


def result_of(piece):
  """The six outputs in the order of `naive_episodes`."""
  return (piece['best'], piece['best_pos'], piece['runs'], piece['lead'], piece['first'], piece['last'])
