"""Device time of Engine.predictive_combinations on the partition-anchor case (every row once, every coefficient 1.0)
beside Engine.predictive_group_sums on the same inputs, and on a three-level hierarchy of the same rows: the figures of
profiles/combinations.md.  Run from the repository root on one MI355X:
python scripts/profile_combinations.py [M R S rows_per_group].  HIP events around the whole call (upload of the CSR
arrays, work buffer, kernels); three rounds in which the calls alternate, each warm-up 2 and 5 timed calls: mean of the 15, min, the round means."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayesnf_amd import inference  # noqa: E402
from bayesnf_amd.engine import Engine  # noqa: E402
from scripts.profile_group_extremes import events  # noqa: E402
from tests import util  # noqa: E402


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
    else:
      loc = 50.0 * torch.randn((M, R), device=eng.device, generator=gen)
      aux = torch.stack([torch.linspace(0.5, 3.0, M, device=eng.device), torch.ones(M, device=eng.device),
                         torch.zeros(M, device=eng.device)], dim=1)
    G = -(-R // per)
    codes = np.random.default_rng(2).permutation(np.arange(R) // per)
    off, rows = inference.csr_from_codes(codes, G)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
    off_d, rows_d, ones_d = dev(off), dev(rows), torch.ones(R, dtype=torch.float64, device=eng.device)
    tag = f'{obs} M={M} R={R} S={S} G={G}'
    sums = eng.predictive_group_sums(loc, aux, off_d, rows_d, 8, seed=7)
    comb = eng.predictive_combinations(loc, aux, off_d, rows_d, ones_d, 8, seed=7)
    print(f'{tag}: partition anchor, bits equal: {bool(torch.equal(sums.view(torch.int64), comb.view(torch.int64)))}', flush=True)
    # three levels in one call: the groups, 100 regions of groups, everything; every row at three positions
    o2, r2 = inference.csr_from_codes(codes % 100, 100)
    h_off = dev(np.concatenate([off, off[-1] + o2[1:], [3 * R]]).astype(np.int32))
    h_rows = dev(np.concatenate([rows, r2, np.arange(R, dtype=np.int32)]))
    h_coef = torch.ones(3 * R, dtype=torch.float64, device=eng.device)
    calls = (('predictive_group_sums', lambda: eng.predictive_group_sums(loc, aux, off_d, rows_d, S, seed=7)),
             ('predictive_combinations, the same partition', lambda: eng.predictive_combinations(loc, aux, off_d, rows_d, ones_d, S, seed=7)),
             ('predictive_combinations, three levels (3 R)', lambda: eng.predictive_combinations(loc, aux, h_off, h_rows, h_coef, S, seed=7)))
    ms = {name: [] for name, _ in calls}
    for _ in range(3):                                       # the calls alternate: a drift of the box hits all of them
      for name, fn in calls:
        ms[name].append(events(fn))
    base = min(lo for _, lo in ms['predictive_group_sums'])
    for name, _ in calls:
      mean, lo = float(np.mean([m for m, _ in ms[name]])), min(lo for _, lo in ms[name])
      rounds = ' '.join(f'{m:.3f}' for m, _ in ms[name])
      print(f'{tag}: {name:44s} mean {mean:9.3f} ms  min {lo:9.3f} ms  ({lo / base:.3f} x the sums)  round means {rounds}',
            flush=True)
    eng.close()


if __name__ == '__main__':
  main()
