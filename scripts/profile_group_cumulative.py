"""Device time of Engine.predictive_group_cumulative without the running matrix (with a level: every other output; and
the totals alone) beside Engine.predictive_group_sums and Engine.predictive_group_episodes (all outputs) on the same
inputs, in one process: the figures of profiles/group_cumulative.md.  Two layouts: groups of `rows_per_group` rows, and
ONE group of all rows -- the worst case of the kernel, which finishes a group that leaves its tile by one block per path.
Run from the repository root on one MI355X: python scripts/profile_group_cumulative.py [M R S rows_per_group].  HIP
events around the whole call (upload of the CSR arrays, work buffer, pre-fill, the kernels), warm-up 2 of every call,
then 7 rounds that ALTERNATE the calls, so that a drift of the box hits all of them alike; mean, min and max per call.
Prints the rows of the table as markdown."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayesnf_amd import _native, inference  # noqa: E402
from bayesnf_amd.engine import Engine  # noqa: E402
from scripts.profile_group_episodes import alternate  # noqa: E402
from tests import util  # noqa: E402


def grid_y(R, G, S):
  """grid.y of k_predictive_group_cumulative (bayesnf_amd/csrc/bnf_api.hip cum_grid)."""
  gx = -(-R // _native.GROUP_TILE)
  return min(S, 65535, max(1, 16384 // gx, -(-2048 // min(gx, G))))


def main():
  M, R, S, per = (int(v) for v in (sys.argv[1:5] + ['64', '1000000', '1000', '50'][len(sys.argv) - 1:]))
  print('| observation model | groups | grid.y | call | mean ms | min ms | max ms | min / sums |\n|---|---|---|---|---|---|---|---|')
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
    thr = thr.float().contiguous()
    rng = np.random.default_rng(2)
    for n_per in (per, R):
      G = -(-R // n_per)
      codes = rng.permutation(np.arange(R) // n_per)
      off, rows = inference.csr_ordered(codes, G, rng.permutation(R))      # the rows of a group in a random time order
      off_d, rows_d = torch.from_numpy(off).to(eng.device), torch.from_numpy(rows).to(eng.device)
      # the level of a group: half the mean of its totals over 8 paths -- most paths cross about half way
      level = 0.5 * eng.predictive_group_sums(loc, aux, off_d, rows_d, 8, seed=7).mean(dim=0)
      ms = alternate({
          '`predictive_group_sums`': lambda: eng.predictive_group_sums(loc, aux, off_d, rows_d, S, seed=7),
          '`predictive_group_episodes`, all outputs': lambda: eng.predictive_group_episodes(loc, aux, off_d, rows_d, S, 7, thr),
          '`predictive_group_cumulative`, level, all outputs but `running`':
              lambda: eng.predictive_group_cumulative(loc, aux, off_d, rows_d, S, 7, level=level),
          '`predictive_group_cumulative`, totals alone': lambda: eng.predictive_group_cumulative(loc, aux, off_d, rows_d, S, 7)})
      base = min(ms['`predictive_group_sums`'])
      for k, v in ms.items():
        print(f'| {obs} | {G:,} of {n_per:,} | {grid_y(R, G, S) if "cumulative" in k else ""} | {k} | {np.mean(v):.3f} | '
              f'{min(v):.3f} | {max(v):.3f} | {min(v) / base:.2f} |', flush=True)
      cu = eng.predictive_group_cumulative(loc, aux, off_d, rows_d, 8, 7, level=level)
      sums = eng.predictive_group_sums(loc, aux, off_d, rows_d, 8, seed=7)
      same = bool(torch.equal(cu['total'], sums)) if obs == 'NB' else bool(torch.allclose(cu['total'], sums, rtol=1e-12))
      print(f'<!-- {obs} M={M} R={R} S={S} G={G}: totals agree with the group sums: {same}; mean crossing step '
            f'{float(cu["cross_step"].mean()):.1f} of {n_per}, never {float((cu["cross_row"] < 0).double().mean()):.3f} -->',
            flush=True)
    eng.close()


if __name__ == '__main__':
  main()
