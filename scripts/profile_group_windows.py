"""Device time of Engine.predictive_group_windows (windows of 7 and of 5,000 positions, with a threshold and every
output) beside Engine.predictive_group_cumulative (with a level and every output) on the same inputs, in one process:
the figures of profiles/group_windows.md.  Every call is timed twice: with its (paths, rows) matrix (`window` /
`running`: 8 bytes per path and row are written) and without it.  Two layouts: groups of `rows_per_group` rows, and ONE
group of all rows -- the worst case of both kernels, which finish a group that leaves its tile by one block per path,
and the only one in which a window of 5,000 draws again.
Run from the repository root on one MI355X: python scripts/profile_group_windows.py [M R S rows_per_group].  HIP events
around the whole call (upload of the CSR arrays, allocation and pre-fill of the outputs, the kernel), warm-up 2 of every
call, then 11 rounds that ALTERNATE the calls, so that a drift of the box hits all of them alike; median, min and max
per call.  Prints the rows of the table as markdown."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayesnf_amd import inference  # noqa: E402
from bayesnf_amd.engine import Engine  # noqa: E402
from scripts.profile_group_cumulative import grid_y  # noqa: E402
from scripts.profile_group_episodes import alternate  # noqa: E402
from tests import util  # noqa: E402

WINDOWS = (7, 5000)


def main():
  M, R, S, per = (int(v) for v in (sys.argv[1:5] + ['64', '1000000', '1000', '50'][len(sys.argv) - 1:]))
  print('| observation model | groups | grid.y | call | matrix | median ms | min ms | max ms | median / cumulative |\n'
        '|---|---|---|---|---|---|---|---|---|')
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
    else:
      loc = 50.0 * torch.randn((M, R), device=eng.device, generator=gen)
      aux = torch.stack([torch.linspace(0.5, 3.0, M, device=eng.device), torch.ones(M, device=eng.device),
                         torch.zeros(M, device=eng.device)], dim=1)
    rng = np.random.default_rng(2)
    for n_per in (per, R):
      G = -(-R // n_per)
      codes = rng.permutation(np.arange(R) // n_per)
      off, rows = inference.csr_ordered(codes, G, rng.permutation(R))      # the rows of a group in a random time order
      off_d, rows_d = torch.from_numpy(off).to(eng.device), torch.from_numpy(rows).to(eng.device)
      # the level of a group: half the mean of its totals over 8 paths; the threshold: half the mean of its peaks
      level = 0.5 * eng.predictive_group_sums(loc, aux, off_d, rows_d, 8, seed=7).mean(dim=0)
      thr = {w: 0.5 * eng.predictive_group_windows(loc, aux, off_d, rows_d, 8, 7, w)['peak'].mean(dim=0) for w in WINDOWS}
      for matrix in (True, False):
        calls = {'`predictive_group_cumulative`, level': lambda: eng.predictive_group_cumulative(
            loc, aux, off_d, rows_d, S, 7, level=level, running=matrix)}
        for w in WINDOWS:
          calls[f'`predictive_group_windows`, w = {w:,}, threshold'] = lambda w=w: eng.predictive_group_windows(
              loc, aux, off_d, rows_d, S, 7, w, threshold=thr[w], windows=matrix)
        ms = alternate(calls, rounds=11)
        base = float(np.median(ms['`predictive_group_cumulative`, level']))
        for k, v in ms.items():
          print(f'| {obs} | {G:,} of {n_per:,} | {grid_y(R, G, S)} | {k} | {"on" if matrix else "off"} | {np.median(v):.3f} | '
                f'{min(v):.3f} | {max(v):.3f} | {np.median(v) / base:.2f} |', flush=True)
      for w in WINDOWS:
        wi = eng.predictive_group_windows(loc, aux, off_d, rows_d, 8, 7, w, threshold=thr[w])
        note = ''
        if w >= n_per:       # the only candidate window is the group's total
          sums = eng.predictive_group_sums(loc, aux, off_d, rows_d, 8, seed=7)
          same = bool(torch.equal(wi['peak'], sums)) if obs == 'NB' else bool(torch.allclose(wi['peak'], sums, rtol=1e-12))
          note = f'; peaks agree with the group sums: {same}'
        print(f'<!-- {obs} M={M} R={R} S={S} G={G} w={w}: mean windows above the threshold {float(wi["count"].mean()):.1f} of '
              f'{max(n_per - min(w, n_per) + 1, 1)}, paths with one above {float((wi["count"] > 0).double().mean()):.3f}{note} -->',
              flush=True)
    eng.close()


if __name__ == '__main__':
  main()
