"""HIP-event time of the weighted entry points next to their unweighted siblings: bnf_predictive_scores with the CRPS and the
exact quantile root at three levels (NORMAL, 10,232 rows, 64 and 1,920 mixture components), and bnf_count_rps (NB, 64
members, the shape of scripts/profile_count_rps.py).  The weighted and the unweighted call alternate in one process; each
figure is the median of 5 calls after 2 warm-up calls.  Prints the table rows of profiles/weighted_forecast.md.
usage: python scripts/profile_weighted_forecast.py"""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bayesnf_amd import _native             # noqa: E402
from bayesnf_amd.engine import Engine       # noqa: E402
from tests import scoring_ref as S          # noqa: E402
from tests import util                      # noqa: E402
from tests.test_gpu_sampling import inv_softplus   # noqa: E402

R = 10232
LEVELS = (0.025, 0.5, 0.975)
p = lambda a: C.c_void_p(a.data_ptr()) if a is not None else None


def alternate(dev, plain, weighted, reps=5, warmup=2):
  """-> (median ms of `plain`, median ms of `weighted`), the two calls taking turns."""
  times = ([], [])
  for i in range(reps + warmup):
    for which, call in enumerate((plain, weighted)):
      a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      a.record()
      _native.check(call(), 'call')
      b.record()
      torch.cuda.synchronize(dev)
      if i >= warmup:
        times[which].append(a.elapsed_time(b))
  return float(np.median(times[0])), float(np.median(times[1]))


def row(name, M, t):
  print(f'| {name} | {M} | {R} | {t[0]:.3f} | {t[1]:.3f} | {t[1] / t[0]:.3f} |', flush=True)


def main():
  rng = np.random.default_rng(0)
  print('| call | M | R | unweighted, ms | weighted, ms | weighted / unweighted |\n|---|---|---|---|---|---|')
  net = util.make_problem(n_rows=16, width=64, depth=1, observation_model='NORMAL')[0]
  eng = Engine(net, members=1, forward_only=True, row_capacity=128, compute_dtype='fp32')
  dev = eng.device
  t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
  for M in (64, 1920):
    sigma = rng.uniform(0.3, 1.5, M)
    loc = 2.0 * rng.standard_normal((M, R))
    y = loc[rng.integers(0, M, R), np.arange(R)] + rng.standard_normal(R)
    w = rng.dirichlet(np.full(M, 1.0))
    loc_d, aux_d, sig_d, y_d = t32(loc), t32(S.normal_aux(sigma)), t32(sigma), t32(y)
    w_d = torch.from_numpy(w).to(dev)
    lpd = torch.empty(R, dtype=torch.float32, device=dev)
    pit = torch.empty((2, R), dtype=torch.float32, device=dev)
    cr = torch.empty(R, dtype=torch.float32, device=dev)
    n_chunks = -(-M // _native.SCORE_MEMBER_CHUNK)
    n_work = R * min((n_chunks + 1) // 2, _native.SCORE_MAX_SLOTS)
    work = torch.empty(n_work, dtype=torch.float64, device=dev)
    row('`bnf_predictive_scores` lpd + pit + crps, NORMAL', M, alternate(
        dev,
        lambda: eng.lib.bnf_predictive_scores(eng.handle, p(loc_d), p(aux_d), M, R, p(y_d), p(work), C.c_size_t(n_work * 8),
                                              None, p(lpd), p(pit), p(cr)),
        lambda: eng.lib.bnf_predictive_scores_weighted(eng.handle, p(loc_d), p(aux_d), p(w_d), M, R, p(y_d), p(work),
                                                       C.c_size_t(n_work * 8), p(lpd), p(pit), p(cr))))
    qa = (C.c_float * len(LEVELS))(*LEVELS)
    out = torch.empty((len(LEVELS), R), dtype=torch.float32, device=dev)
    row('`bnf_normal_mixture_quantiles` exact, 3 levels', M, alternate(
        dev,
        lambda: eng.lib.bnf_normal_mixture_quantiles(eng.handle, p(loc_d), p(sig_d), M, R, qa, len(LEVELS), 0, p(out)),
        lambda: eng.lib.bnf_normal_mixture_quantiles_weighted(eng.handle, p(loc_d), p(sig_d), p(w_d), M, R, qa, len(LEVELS),
                                                              0, p(out))))
  eng.close()

  M = 64                                      # the shape of scripts/profile_count_rps.py
  tcs = rng.uniform(2.0, 20.0, M)
  means = 400.0 * np.exp(0.3 * rng.standard_normal(R))[None, :] * np.exp(0.1 * rng.standard_normal((M, R)))
  aux = np.stack([np.ones(M), 1.0 / tcs, np.zeros(M)], axis=1)
  loc = inv_softplus(tcs[:, None] ** 2 / means)
  y = np.round(means.mean(axis=0) * np.exp(0.4 * rng.standard_normal(R)))
  net = util.make_problem(n_rows=16, width=64, depth=1, observation_model='NB')[0]
  eng = Engine(net, members=1, forward_only=True, row_capacity=128, compute_dtype='fp32')
  dev = eng.device
  loc_d, aux_d, y_d = t32(loc), t32(aux), t32(y)
  w_d = torch.from_numpy(rng.dirichlet(np.full(M, 1.0))).to(dev)
  out = torch.empty(R, dtype=torch.float32, device=dev)
  row('`bnf_count_rps`, NB', M, alternate(
      dev,
      lambda: eng.lib.bnf_count_rps(eng.handle, p(loc_d), p(aux_d), M, R, p(y_d), p(out)),
      lambda: eng.lib.bnf_count_rps_weighted(eng.handle, p(loc_d), p(aux_d), p(w_d), M, R, p(y_d), p(out))))
  assert not bool(torch.isnan(out).any())
  eng.close()


if __name__ == '__main__':
  main()
