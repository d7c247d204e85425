"""Device time of Engine.predictive_group_episodes (all outputs) beside Engine.predictive_group_extremes with a threshold
(all outputs) and Engine.predictive_group_sums on the same inputs, in one process: the figures of
profiles/group_episodes.md.  Run from the repository root on one MI355X:
python scripts/profile_group_episodes.py [M R S rows_per_group].  HIP events around the whole call (upload of the CSR
arrays, work buffer, pre-fill, both kernels), warm-up 2 of every call, then 7 rounds that ALTERNATE the calls, so that a
drift of the box hits all of them alike; mean, min and max per call."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayesnf_amd import inference  # noqa: E402
from bayesnf_amd.engine import Engine  # noqa: E402
from tests import util  # noqa: E402


def alternate(calls, rounds=7, warm=2):
  """calls: dict name -> fn.  -> dict name -> list of ms, one per round; round r runs every call once, in order."""
  for fn in calls.values():
    for _ in range(warm):
      fn()
  torch.cuda.synchronize()
  ms = {k: [] for k in calls}
  for _ in range(rounds):
    for k, fn in calls.items():
      a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      a.record()
      fn()
      b.record()
      torch.cuda.synchronize()
      ms[k].append(a.elapsed_time(b))
  return ms


def main():
  M, R, S, per = (int(v) for v in (sys.argv[1:5] + ['64', '1000000', '1000', '50'][len(sys.argv) - 1:]))
  for obs in ('NB', 'NORMAL'):
    net, _, _, _ = util.make_problem(n_rows=16, width=64, depth=1, observation_model=obs)
    eng = Engine(net, members=1, forward_only=True, row_capacity=128, compute_dtype='fp32')
    gen = torch.Generator(device=eng.device).manual_seed(1)
    if obs == 'NB':        # total_count 0.3 .. 60 per member, means log-uniform on 0.05 .. 3e3: the mix of the GPU tests
      tcs = torch.exp(torch.linspace(np.log(0.3), np.log(60.0), M, device=eng.device))
      means = torch.exp(torch.empty((M, R), device=eng.device).uniform_(np.log(0.05), np.log(3e3), generator=gen))
      sp = tcs[:, None] ** 2 / means
      loc = torch.where(sp > 30.0, sp, torch.log(torch.expm1(sp.clamp(max=30.0))))
      aux = torch.stack([torch.ones_like(tcs), 1.0 / tcs, torch.full_like(tcs, 0.35)], dim=1)
      thr = means.mean(dim=0)
    else:
      loc = 50.0 * torch.randn((M, R), device=eng.device, generator=gen)
      aux = torch.stack([torch.linspace(0.5, 3.0, M, device=eng.device), torch.ones(M, device=eng.device),
                         torch.zeros(M, device=eng.device)], dim=1)
      thr = loc.mean(dim=0)
    G = -(-R // per)
    rng = np.random.default_rng(2)
    codes = rng.permutation(np.arange(R) // per)
    off, rows = inference.csr_ordered(codes, G, rng.permutation(R))        # the rows of a group in a random time order
    off_d, rows_d = torch.from_numpy(off).to(eng.device), torch.from_numpy(rows).to(eng.device)
    thr = thr.float().contiguous()
    tag = f'{obs} M={M} R={R} S={S} G={G}'
    ms = alternate({
        'predictive_group_sums': lambda: eng.predictive_group_sums(loc, aux, off_d, rows_d, S, seed=7),
        'predictive_group_extremes (threshold, all outputs)':
            lambda: eng.predictive_group_extremes(loc, aux, off_d, rows_d, S, seed=7, threshold=thr),
        'predictive_group_episodes (all outputs)':
            lambda: eng.predictive_group_episodes(loc, aux, off_d, rows_d, S, 7, thr),
        'predictive_group_episodes (per_row=False)':
            lambda: eng.predictive_group_episodes(loc, aux, off_d, rows_d, S, 7, thr, per_row=False)})
    base = min(ms['predictive_group_extremes (threshold, all outputs)'])
    for k, v in ms.items():
      print(f'{tag}: {k:52s} mean {np.mean(v):9.3f} ms  min {min(v):9.3f} ms  max {max(v):9.3f} ms  '
            f'({min(v) / base:.2f} x the extremes)', flush=True)
    ep = eng.predictive_group_episodes(loc, aux, off_d, rows_d, 8, 7, thr)
    print(f'{tag}: mean longest {float(ep["longest"].mean()):.2f}, mean spells {float(ep["spells"].mean()):.2f}, '
          f'mean onset step {float(ep["onset_step"].mean()):.2f}', flush=True)
    eng.close()


if __name__ == '__main__':
  main()
