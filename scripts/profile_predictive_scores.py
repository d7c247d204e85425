"""HIP-event time of one bnf_predictive_scores call at three shapes, next to the wall time of the host path it replaces
(likelihood_model's log_prob in numpy / scipy plus the numpy closed-form CRPS of tests/scoring_ref.py).
Writes profiles/predictive_scores.md's table rows to stdout.  usage: python scripts/profile_predictive_scores.py"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bayesnf_amd import _native, inference   # noqa: E402
from bayesnf_amd.engine import Engine       # noqa: E402
from tests import scoring_ref as S          # noqa: E402
from tests import util                      # noqa: E402
from tests.test_gpu_sampling import inv_softplus   # noqa: E402

R = 10232
HOST_CRPS_ROWS = 256      # the numpy CRPS is timed on this many rows and scaled to R (it is linear in the rows)


def device_time(eng, loc, aux, y, crps, reps=5):
  M = loc.shape[0]
  dev = eng.device
  t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
  loc_d, aux_d, y_d = t(loc), t(aux), t(y)
  ll = torch.empty(M, dtype=torch.float64, device=dev)
  lpd = torch.empty(R, dtype=torch.float32, device=dev)
  pit = torch.empty((2, R), dtype=torch.float32, device=dev)
  cr = torch.empty(R, dtype=torch.float32, device=dev) if crps else None
  n_chunks = -(-M // _native.SCORE_MEMBER_CHUNK)
  n_work = M * (-(-R // _native.SCORE_ROW_TILE)) + (R * min((n_chunks + 1) // 2, _native.SCORE_MAX_SLOTS) if crps else 0)
  work = torch.empty(n_work, dtype=torch.float64, device=dev)
  p = lambda a: C.c_void_p(a.data_ptr()) if a is not None else None
  times = []
  for i in range(reps + 2):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    _native.check(eng.lib.bnf_predictive_scores(eng.handle, p(loc_d), p(aux_d), M, R, p(y_d), p(work), C.c_size_t(n_work * 8),
                                                p(ll), p(lpd), p(pit), p(cr)), 'bnf_predictive_scores')
    b.record()
    torch.cuda.synchronize(dev)
    if i >= 2:
      times.append(a.elapsed_time(b))
  return float(np.median(times)), min(times), max(times)


def main():
  rng = np.random.default_rng(0)
  for name, obs, M, crps in (('C2 NORMAL', 'NORMAL', 64, True), ('VI NORMAL + CRPS', 'NORMAL', 1920, True), ('C2 NB', 'NB', 64, False)):
    net = util.make_problem(n_rows=16, width=64, depth=1, observation_model=obs)[0]
    eng = Engine(net, members=1, forward_only=True, row_capacity=128, compute_dtype='fp32')
    if obs == 'NORMAL':
      sigma = rng.uniform(0.3, 1.5, M)
      loc = 2.0 * rng.standard_normal((M, R))
      y = loc[rng.integers(0, M, R), np.arange(R)] + rng.standard_normal(R)
      aux = S.normal_aux(sigma)
    else:
      tcs = rng.uniform(0.5, 20.0, M)
      means = np.exp(rng.uniform(np.log(0.5), np.log(3e3), R))[None, :] * rng.uniform(0.7, 1.4, (M, 1))
      loc = inv_softplus(tcs[:, None] ** 2 / means)
      aux = np.stack([np.ones(M), 1.0 / tcs, np.zeros(M)], axis=1)
      y = rng.poisson(rng.gamma(tcs[0], means[0] / tcs[0])).astype(np.float64)
    loc, aux, y = loc.astype(np.float32), aux.astype(np.float32), y.astype(np.float32)
    med, lo, hi = device_time(eng, loc, aux, y, crps)
    eng.close()
    loc64, aux64, y64 = loc.astype(np.float64), aux.astype(np.float64), y.astype(np.float64)
    t0 = time.perf_counter()
    if obs == 'NORMAL':
      lik = inference.EnsembleLikelihood(loc64, aux64[:, 0])
    else:
      lik = inference.CountEnsembleLikelihood(1.0 / aux64[:, 1], -np.log(aux64[:, 1])[:, None] - np.log(np.logaddexp(loc64, 0.0)))
    lik.log_prob(y64)
    lik.mixture_cdf(y64)
    t_lp = time.perf_counter() - t0
    t_crps = float('nan')
    if crps:
      t0 = time.perf_counter()
      S.normal_crps(loc64[:, :HOST_CRPS_ROWS], aux64[:, 0], y64[:HOST_CRPS_ROWS])
      t_crps = (time.perf_counter() - t0) * R / HOST_CRPS_ROWS
    print(f'| {name} | {M} | {R} | {med:.3f} ({lo:.3f} .. {hi:.3f}) | {1e3 * t_lp:.1f} | {1e3 * t_crps:.0f} |', flush=True)


if __name__ == '__main__':
  main()
