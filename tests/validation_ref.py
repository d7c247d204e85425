"""A numpy restatement of the decision rule of bnf_validation_check (include/bnf.h), shared by the CPU and the GPU
tests of the held-out validation during a fit.  Everything is float64 and sequential: one check after the other, as the
device sees them."""
import numpy as np


def keeps(check, score, best):
  """Does `score` at check number `check` become the member's best, given the best so far?"""
  if check == 0:
    return True
  return bool(score > best or (np.isnan(best) and not np.isnan(score)))


def run(member_ll, n_scored, epochs):
  """member_ll (K, M): the sums the K checks see, in order; epochs (K,).  -> dict:
    'curve' (M, K) = member_ll.T / n_scored   'keep' (K, M) int32   'best_score' (M,)   'best_epoch' (M,) int64
    'best_check' (M,) the index of the check whose snapshot is kept   'history' per check (best_score, best_epoch)"""
  member_ll = np.asarray(member_ll, dtype=np.float64)
  K, M = member_ll.shape
  curve = (member_ll / np.float64(n_scored)).T.copy()
  keep = np.zeros((K, M), dtype=np.int32)
  best_score = np.full(M, np.nan)
  best_epoch = np.full(M, -1, dtype=np.int64)
  best_check = np.full(M, -1, dtype=np.int64)
  history = []
  for c in range(K):
    for m in range(M):
      if keeps(c, curve[m, c], best_score[m]):
        keep[c, m], best_score[m], best_epoch[m], best_check[m] = 1, curve[m, c], epochs[c], c
    history.append((best_score.copy(), best_epoch.copy()))
  return dict(curve=curve, keep=keep, best_score=best_score, best_epoch=best_epoch, best_check=best_check, history=history)


def best_of_curve(curve, epochs):
  """curve (..., K) of scores -> (best (...,), best_epoch (...,)) by the rule: the first occurrence of the maximum, a NaN
  never beating a number."""
  curve = np.asarray(curve, dtype=np.float64)
  flat = curve.reshape(-1, curve.shape[-1])
  res = run(flat.T * 1.0, 1, epochs)
  lead = curve.shape[:-1]
  return res['best_score'].reshape(lead), res['best_epoch'].reshape(lead)


# The hand-made columns of the GPU test, one per member, six checks each; n_scored = 7 makes every division round.
N_SCORED = 7
EPOCHS = (5, 10, 15, 20, 25, 27)
NAN, NINF = float('nan'), float('-inf')
COLUMNS = {
    'interior maximum': (-5.0, -3.0, -1.0, -2.0, -4.0, -6.0),
    'tie': (-2.0, -1.0, -1.0, -3.0, -1.0, -4.0),
    'nan first': (NAN, -7.0, -8.0, -6.0, -6.0, -9.0),
    'number then nan': (-3.0, NAN, NAN, -4.0, NAN, -5.0),
    '-inf throughout': (NINF,) * 6,
}
# worked by hand: the check whose snapshot each column ends with, and the checks at which keep is 1
HAND_BEST_CHECK = {'interior maximum': 2, 'tie': 1, 'nan first': 3, 'number then nan': 0, '-inf throughout': 0}
HAND_KEEP = {'interior maximum': (1, 1, 1, 0, 0, 0), 'tie': (1, 1, 0, 0, 0, 0), 'nan first': (1, 1, 0, 1, 0, 0),
             'number then nan': (1, 0, 0, 0, 0, 0), '-inf throughout': (1, 0, 0, 0, 0, 0)}


def columns(names):
  """-> member_ll (6, len(names)) float64."""
  return np.asarray([COLUMNS[n] for n in names], dtype=np.float64).T.copy()
