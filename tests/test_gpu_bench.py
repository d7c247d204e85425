"""bench.py on one GPU: a plain run times exactly K steps of the C2 workload and writes the last step's outputs with
`--dump-outputs` (the same in two runs); `--full` adds the roofline of the dominant kernel (here without the CPU baseline)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args):
  env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1'] + args, capture_output=True,
                     text=True, timeout=600, env=env, cwd=ROOT)
  assert r.returncode == 0, r.stderr[-3000:]
  return json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][0])


def test_plain_run_times_k_steps_and_dumps_the_last_step(tmp_path):
  out = {}
  for run in ('a', 'b'):
    out[run] = tmp_path / run
    d = _bench(['--steps', '4', '--warmup', '2', '--dump-outputs', str(out[run])])
    assert d['steps'] == 4 and d['n_gpus'] == 1 and d['dtype'] == 'bf16' and d['unit'] == 'member-steps/s'
    assert d['ms_per_step'] > 0 and abs(d['value'] - 64 * 4 / (d['ms_per_step'] * 4e-3)) < 1e-6 * d['value']
    for side in ('roofline', 'other_dtypes', 'cpu_baseline'):
      assert side not in d
    loss = np.load(out[run] / 'loss.npy')
    assert loss.dtype == np.float32 and loss.shape == (64,) and np.all(np.isfinite(loss))
    np.testing.assert_allclose(loss.mean(dtype=np.float64), d['final_loss_mean'], rtol=1e-5)
  # the same arguments: the same inputs, the same outputs up to the order of the engine's float-atomic sums
  np.testing.assert_allclose(np.load(out['a'] / 'loss.npy'), np.load(out['b'] / 'loss.npy'), rtol=1e-5)


def test_full_run_reports_the_roofline():
  d = _bench(['--steps', '2', '--warmup', '1', '--full', '--no-cpu-baseline'])
  rf = d['roofline']
  assert rf['launches'] == 2 and rf['achieved'] > 0 and 0 < rf['frac'] < 1 and rf['kernel']
  assert 'cpu_baseline' not in d and 'other_dtypes' not in d
