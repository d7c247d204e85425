"""Device time of Engine.predictive_group_extremes (all outputs) beside Engine.predictive_group_sums on the same inputs:
the figures of profiles/group_extremes.md.  Run from the repository root on one MI355X:
python scripts/profile_group_extremes.py [M R S rows_per_group].  HIP events around the whole call (upload of the CSR
arrays, work buffer, kernels), warm-up 2, mean and min of 5 calls."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayesnf_amd import inference  # noqa: E402
from bayesnf_amd.engine import Engine  # noqa: E402
from tests import util  # noqa: E402


def events(fn, rep=5, warm=2):
  for _ in range(warm):
    fn()
  torch.cuda.synchronize()
  ms = []
  for _ in range(rep):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    ms.append(a.elapsed_time(b))
  return float(np.mean(ms)), float(np.min(ms))


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
    codes = np.random.default_rng(2).permutation(np.arange(R) // per)
    off, rows = inference.csr_from_codes(codes, G)
    off_d, rows_d = torch.from_numpy(off).to(eng.device), torch.from_numpy(rows).to(eng.device)
    thr = thr.float().contiguous()
    tag = f'{obs} M={M} R={R} S={S} G={G}'
    m, lo = events(lambda: eng.predictive_group_sums(loc, aux, off_d, rows_d, S, seed=7))
    print(f'{tag}: predictive_group_sums                    mean {m:9.3f} ms  min {lo:9.3f} ms', flush=True)
    base = lo
    for what, kw in (('max, argmax', dict(per_row=False)), ('max, argmax, peak_count', dict()),
                     ('all outputs (threshold)', dict(threshold=thr))):
      m, lo = events(lambda: eng.predictive_group_extremes(loc, aux, off_d, rows_d, S, seed=7, **kw))
      print(f'{tag}: predictive_group_extremes {what:24s} mean {m:9.3f} ms  min {lo:9.3f} ms  ({lo / base:.2f} x the sums)',
            flush=True)
    eng.close()


if __name__ == '__main__':
  main()
