"""Wall time of the simultaneous-band kernels (bnf_sample_depths, bnf_depth_levels, bnf_sample_envelope) beside
bnf_sample_summaries on the same matrix, which runs the same slab sort: the figures of profiles/sample_bands.md.  Run
from the repository root on one MI355X: python scripts/profile_sample_bands.py [--samples 1000 --cols 10232 --groups 200].
Median of 5 calls after one warm-up; the device is synchronised before the clock is read, so every figure is the Engine
call: output allocation (and pre-fill), launch and synchronisation."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bayesnf_amd.engine import Engine  # noqa: E402
from tests import util  # noqa: E402


def median_of(fn, rep=5):
  fn()
  torch.cuda.synchronize()
  times = []
  for _ in range(rep):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    times.append(time.perf_counter() - t0)
  return float(np.median(times))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--samples', type=int, default=1000)
  ap.add_argument('--cols', type=int, default=10232)
  ap.add_argument('--groups', type=int, default=200)
  args = ap.parse_args()
  S, C, G = args.samples, args.cols, args.groups
  rng = np.random.default_rng(1)
  net, _, _, _ = util.make_problem(n_rows=16, width=64, depth=1, observation_model='NORMAL')
  eng = Engine(net, members=1, forward_only=True, row_capacity=128, compute_dtype='fp32')
  print(f'{torch.cuda.get_device_name(0)}: S = {S}, C = {C}, G = {G}')
  need = [int(np.ceil(0.9 * S - 1e-9))]
  for tag, x in (('counts (Poisson 3: ties)', rng.poisson(3.0, (S, C)).astype(np.float64)),
                 ('running totals (continuous)', np.cumsum(rng.standard_normal((S, C)), axis=1))):
    for layout, cg in (('contiguous groups', (np.arange(C) * G // C).astype(np.int32)),
                       ('interleaved groups', rng.integers(0, G, size=C).astype(np.int32))):
      xd = torch.from_numpy(x).to(eng.device)
      cgd = torch.from_numpy(cg).to(eng.device)
      y = torch.from_numpy(x[0].copy()).to(eng.device)
      dep = eng.sample_depths(xd, cgd, G, y)
      lev = eng.depth_levels(dep['depth'], need, [(S - need[0]) // 2], dep['obs_depth'])
      print(f'{tag}, {layout}:')
      for name, fn in (('bnf_sample_summaries (mean, 3 levels, crps, pit)', lambda: eng.sample_summaries(xd, y, (0.05, 0.5, 0.95))),
                       ('bnf_sample_depths (with y)', lambda: eng.sample_depths(xd, cgd, G, y)),
                       ('bnf_depth_levels', lambda: eng.depth_levels(dep['depth'], need, [(S - need[0]) // 2], dep['obs_depth'])),
                       ('bnf_sample_envelope (1 level)', lambda: eng.sample_envelope(xd, cgd, lev['level']))):
        print(f'  {name}: {median_of(fn) * 1e3:.3f} ms')
  eng.close()


if __name__ == '__main__':
  main()
