"""What the held-out checks of a validated fit cost (include/bnf.h bnf_validation_check; inference._HeldOut): an
Engine-level run of the benchmark's C2 shape in bf16 -- 64 members, 10,232 rows, width 512, depth 2 -- for 200 full-batch
epochs, without checks and with a check on 2,048 held-out rows every 20 epochs (10 checks), the two alternated three times
in one session; plus one check on its own, timed with device events over 20 back-to-back checks.  Writes the figures as
markdown (default profiles/validation_overhead.md) and prints them as one JSON line.
Run from the repository root: python scripts/profile_validation_overhead.py [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayesnf_amd import inference
from bayesnf_amd.engine import Engine
from bayesnf_amd.spec import NetSpec
from bench import MODEL_KW, synthetic_grid

E, EPOCHS, EVERY, N_VAL, REPS, DTYPE = 64, 200, 20, 2048, 3, 'bf16'


def engine(net, X, y, seed):
  eng = Engine(net, mode='map', X=X, y=y, members=E, seed=seed, learning_rate=0.005, prior_weight=1.0, compute_dtype=DTYPE)
  eng.init_params(float(np.log(np.nanstd(y) / 2)))
  return eng


def timed(fn, device):
  torch.cuda.synchronize(device)
  t0 = time.perf_counter()
  fn()
  torch.cuda.synchronize(device)
  return (time.perf_counter() - t0) * 1e3


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=os.path.join('profiles', 'validation_overhead.md'))
  args = ap.parse_args()
  X, y, scales = synthetic_grid()
  Xv, yv, _ = synthetic_grid(seed=4321)             # the same law, other sites and noise
  Xv, yv = Xv[:N_VAL], yv[:N_VAL]
  net = NetSpec(input_scales=scales, **MODEL_KW)
  checks = inference.validation_epochs(EPOCHS, EVERY)

  def plain(seed):
    eng = engine(net, X, y, seed)
    ms = timed(lambda: eng.train(0, EPOCHS), eng.device)
    eng.close()
    return ms

  def validated(seed):
    eng = engine(net, X, y, seed)
    setup = timed(lambda: held.append(inference._HeldOut(net, eng, Xv, yv, checks, DTYPE, eng.dev_index)), eng.device)
    h = held.pop()
    ms = timed(lambda: h.train(0, EPOCHS), eng.device)
    curve = h.curve.cpu().numpy()
    fwd_ws = int(h.fwd.workspace.numel())
    h.close()
    eng.close()
    return ms, setup, curve, fwd_ws

  held = []
  plain(9), validated(9)                             # warm-up: code objects, the device's clocks
  runs = {'plain': [], 'validated': [], 'setup': []}
  for rep in range(REPS):
    runs['plain'].append(plain(rep))
    ms, setup, curve, fwd_ws = validated(rep)
    runs['validated'].append(ms)
    runs['setup'].append(setup)

  # one check on its own: 20 back to back between two device events (the parameters do not move in between)
  eng = engine(net, X, y, 0)
  h = inference._HeldOut(net, eng, Xv, yv, list(range(1, 25)), DTYPE, eng.dev_index)
  for _ in range(4):
    h.check(0)
  ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  ev0.record(eng.stream)
  for _ in range(20):
    h.check(0)
  ev1.record(eng.stream)
  torch.cuda.synchronize(eng.device)
  check_ms = ev0.elapsed_time(ev1) / 20
  # the snapshot copy alone: check 0 keeps every member
  h.done = 0
  copy_bytes = 8 * E * net.P
  ev0.record(eng.stream)
  for _ in range(20):
    eng.validation_check(h.ll, h.n, 0, 0, len(h.epochs), h.curve, h.best_score, h.best_epoch, h.keep, h.best_params)
  ev1.record(eng.stream)
  torch.cuda.synchronize(eng.device)
  keep_ms = ev0.elapsed_time(ev1) / 20
  h.close()
  eng.close()

  med = {k: float(np.median(v)) for k, v in runs.items()}
  out = dict(members=E, rows=int(X.shape[0]), held_out_rows=N_VAL, epochs=EPOCHS, every=EVERY, checks=len(checks), dtype=DTYPE,
             P=int(net.P), plain_ms=runs['plain'], validated_ms=runs['validated'], setup_ms=runs['setup'],
             plain_median_ms=med['plain'], validated_median_ms=med['validated'], setup_median_ms=med['setup'],
             overhead_ms=med['validated'] - med['plain'], overhead_pct=100.0 * (med['validated'] / med['plain'] - 1.0),
             per_check_from_runs_ms=(med['validated'] - med['plain']) / len(checks), check_ms=check_ms,
             decide_and_copy_ms=keep_ms, copy_GBps=copy_bytes / (keep_ms * 1e-3) / 1e9,
             snapshot_bytes=4 * E * int(net.P), forward_workspace_bytes=fwd_ws, loc_bytes=4 * E * N_VAL,
             curve_first_member=[float(v) for v in curve[0]])
  fmt = lambda v: ', '.join(f'{x:.1f}' for x in v)
  lines = [
      '# Cost of the held-out checks of a validated fit', '',
      f'`scripts/profile_validation_overhead.py` on one MI355X: Engine level, the benchmark\'s C2 shape ({E} members, '
      f'{out["rows"]:,} rows, width 512, depth 2, P = {out["P"]:,}), `{DTYPE}`, {EPOCHS} full-batch epochs; the validated run '
      f'checks {N_VAL:,} held-out rows every {EVERY} epochs ({len(checks)} checks: forward on a forward-only handle, '
      f'`bnf_predictive_scores` member_ll, `bnf_validation_check`).  Host clock around work that ends in a device '
      f'synchronise; the two runs alternated {REPS} times in one process after one warm-up of each.  A record, not a gate.', '',
      '| | runs (ms) | median (ms) |', '|---|---|---|',
      f'| {EPOCHS} epochs, no checks | {fmt(runs["plain"])} | {med["plain"]:.1f} |',
      f'| {EPOCHS} epochs, {len(checks)} checks | {fmt(runs["validated"])} | {med["validated"]:.1f} |',
      f'| set-up of the checks (forward-only handle, uploads, buffers; not in the rows above) | {fmt(runs["setup"])} | {med["setup"]:.1f} |',
      '',
      f'- overhead of the {len(checks)} checks: {out["overhead_ms"]:.1f} ms = {out["overhead_pct"]:.2f} % of the run, '
      f'{out["per_check_from_runs_ms"]:.2f} ms per check',
      f'- one check on its own (device events over 20 back-to-back checks): {check_ms:.3f} ms',
      f'- `bnf_validation_check` alone with every member kept (decide + copy of {copy_bytes / 1e6:.1f} MB read + written): '
      f'{keep_ms:.3f} ms = {out["copy_GBps"]:.0f} GB/s -- 20 copies of the same rows back to back, which the 256 MB '
      f'Infinity Cache can hold: a rate with warm caches, not an HBM stream rate; inside a fit the rows come from HBM',
      f'- extra device memory: snapshots {out["snapshot_bytes"] / 1e6:.1f} MB, forward workspace '
      f'{fwd_ws / 1e6:.1f} MB, `loc` {out["loc_bytes"] / 1e6:.2f} MB',
      '']
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f:
    f.write('\n'.join(lines))
  print(json.dumps(out))


if __name__ == '__main__':
  main()
