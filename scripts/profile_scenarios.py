"""Device times of bnf_sample_distances and bnf_scenario_select beside bnf_sample_energy_score (k_energy_pairs: the same
pair arithmetic without the S^2 stores) and the host path: the figures of profiles/sample_scenarios.md, which this script
writes (--out PATH for another place).  Run from the repository root on one MI355X:
python scripts/profile_scenarios.py  Device times: HIP events on the handle's stream around one call, one warm-up call
before, mean and min of `rep` calls, all in one process.  Host times: time.perf_counter around the device-to-host copy of
the totals and around the numpy distance step (row by row)."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bayesnf_amd import _native  # noqa: E402
from bayesnf_amd.engine import Engine, _ptr  # noqa: E402
from tests import util  # noqa: E402

LINES = []


def say(line=''):
  print(line, flush=True)
  LINES.append(line)


def events(fn, rep, warm=1):
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


def make_x(S, G, device):
  """Integer totals with a factor shared by the columns of a path, made on the device."""
  gen = torch.Generator(device=device).manual_seed(S + G)
  f = torch.randn((S, 1), generator=gen, device=device, dtype=torch.float64)
  e = torch.randn((S, G), generator=gen, device=device, dtype=torch.float64)
  return torch.round(200.0 + 30.0 * f + 10.0 * e).contiguous()


def case(eng, S, G, k, rep):
  x = make_x(S, G, eng.device)
  f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=eng.device)
  i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=eng.device)
  y = (x[S // 2] + 3.0).contiguous()
  scale = x.std(dim=0).clamp(min=1.0).contiguous()
  say(f'### S = {S:,} paths x G = {G:,} columns, k = {k}: {S * (S + 1) // 2 * G:.3g} differences, a matrix of '
      f'{S * S * 8 / 1e6:.1f} MB')
  say()
  say('| call | mean ms | min ms | calls |')
  say('|---|---|---|---|')
  tiles = -(-S // _native.ENERGY_SAMPLE_TILE)
  n_work = S + tiles * (tiles + 1) // 2
  work, out = f64(n_work), f64(1)

  def energy():
    _native.check(eng.lib.bnf_sample_energy_score(eng.handle, _ptr(x), S, G, _ptr(y), _ptr(work), C.c_size_t(n_work * 8),
                                                  _ptr(out)), 'bnf_sample_energy_score')
  m, lo = events(energy, rep)
  say(f'| bnf_sample_energy_score (k_energy_first, k_energy_pairs, k_energy_finish): the yardstick | {m:.3f} | {lo:.3f} | {rep} |')
  dist, ydist = f64(S, S), f64(S)
  for p, sc, yy, what in ((2, None, None, 'p = 2'), (1, None, None, 'p = 1'), (2, scale, None, 'p = 2, scale'),
                          (2, None, y, 'p = 2, y and ydist')):
    def distances():
      _native.check(eng.lib.bnf_sample_distances(eng.handle, _ptr(x), S, G, _ptr(sc), _ptr(yy), p, _ptr(dist),
                                                 _ptr(ydist if yy is not None else None)), 'bnf_sample_distances')
    m, lo = events(distances, rep)
    say(f'| bnf_sample_distances, {what} | {m:.3f} | {lo:.3f} | {rep} |')
  fill = f64(S, S)
  m, lo = events(lambda: fill.fill_(1.0), rep)
  say(f'| storing S^2 doubles (torch fill_) | {m:.3f} | {lo:.3f} | {rep} |')
  _native.check(eng.lib.bnf_sample_distances(eng.handle, _ptr(x), S, G, None, _ptr(y), 2, _ptr(dist), _ptr(ydist)),
                'bnf_sample_distances')
  nb = _native.scenario_work_bytes(S)
  swork = f64(-(-nb // 8))
  chosen, objective, prob, assign, nearest, on, obs = i32(k), f64(k), f64(k), i32(S), f64(S), i32(1), f64(3)

  def select():
    _native.check(eng.lib.bnf_scenario_select(
        eng.handle, _ptr(dist), S, k, _ptr(ydist), _ptr(swork), C.c_size_t(nb), _ptr(chosen), _ptr(objective), _ptr(prob),
        _ptr(assign), _ptr(nearest), _ptr(on), _ptr(obs)), 'bnf_scenario_select')
  m, lo = events(select, rep)
  say(f'| bnf_scenario_select, k = {k} ({2 * k + 3} launches) | {m:.3f} | {lo:.3f} | {rep} |')
  say()
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  xh = x.cpu().numpy()
  t_copy = time.perf_counter() - t0
  t0 = time.perf_counter()
  host = np.stack([np.sqrt(((xh[s] - xh) ** 2).sum(axis=1)) for s in range(S)])
  t_host = time.perf_counter() - t0
  eng.debug_poison_lds()
  got, _ = eng.sample_distances(x, 2)
  err = np.abs(got.cpu().numpy() - host)
  say(f'Host path on the same box: device-to-host copy of the {S * G * 8 / 1e6:.1f} MB totals {t_copy * 1e3:.1f} ms; the '
      f'distance matrix in numpy, row by row, {t_host:.2f} s.  Device matrix against it: max relative difference '
      f'{np.max(err / np.maximum(host, 1e-300)):.2e}.')
  say(f'Objective after 1 .. {k} scenarios: ' + ', '.join(f'{v:.4g}' for v in objective.cpu().tolist()) + '; probabilities '
      + ', '.join(f'{v:.3f}' for v in prob.cpu().tolist()) + '.')
  say()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sample_scenarios.md'))
  args = ap.parse_args()
  net, _, _, _ = util.make_problem(n_rows=16, width=64, depth=1, observation_model='NORMAL')
  eng = Engine(net, members=1, forward_only=True, row_capacity=128, compute_dtype='fp32')
  say('# bnf_sample_distances / bnf_scenario_select: representative scenarios of sample paths')
  say()
  say(f'Written by scripts/profile_scenarios.py on {torch.cuda.get_device_name(0)}, one process.  Device times are HIP '
      'events on the handle\'s stream around one call, one warm-up call before.  The yardstick is the energy score of the '
      'same matrix: k_energy_pairs forms the same differences in the same tiles and stores one partial sum per tile.')
  say()
  case(eng, 1000, 520, 10, 20)
  case(eng, 4096, 64, 10, 10)
  eng.close()
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f:
    f.write('\n'.join(LINES) + '\n')


if __name__ == '__main__':
  main()
