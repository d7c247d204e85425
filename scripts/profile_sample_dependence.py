"""Device times of bnf_sample_pair_moments beside the host path: the figures of profiles/sample_dependence.md, which this
script writes (--out PATH for another place).  Run from the repository root on one MI355X:
python scripts/profile_sample_dependence.py  Device times: HIP events on the handle's stream, warm-up 1, mean and min of `rep`
calls.  Host times: time.perf_counter around the device-to-host copy of the matrix and around numpy (np.cov; the variogram
row by row, on a subset of the rows where all of them would take minutes, extrapolated by the number of pair terms)."""
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
from tests import dependence_ref as D  # noqa: E402
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


def device_times(eng, x, y, matrices, rep):
  S, G = x.shape
  f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=eng.device)
  mean, score = f64(G), f64(1)
  cov = f64(G, G) if matrices else None
  vario = f64(G, G) if matrices else None
  n_work = _native.pair_work_doubles(G)
  work = f64(n_work)
  terms = S * G * (G + 1) / 2
  out = {}
  for p in D.ORDERS:
    def call():
      _native.check(eng.lib.bnf_sample_pair_moments(
          eng.handle, _ptr(x), S, G, C.c_double(p), _ptr(y), None, _ptr(mean), _ptr(cov), _ptr(vario), _ptr(work),
          C.c_size_t(n_work * 8), _ptr(score)), 'bnf_sample_pair_moments')
    m, lo = events(call, rep)
    out[p] = float(score.cpu()[0])
    say(f'| p = {p} | {"mean, covariance, variogram, score" if matrices else "mean, score"} | {m:.3f} | {lo:.3f} | {rep} | '
        f'{terms / (lo * 1e-3) / 1e12:.2f} |')
  return out, (None if cov is None else cov.cpu().numpy()), (None if vario is None else vario.cpu().numpy())


def host_times(x, y, rows, matrices):
  """-> (seconds of the copy, of np.cov, of the variogram + score at one p extrapolated to all rows, the subset's rows of the
  variogram at p = 0.5)."""
  S, G = x.shape
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  xh = x.cpu().numpy()
  t_copy = time.perf_counter() - t0
  t_cov = float('nan')
  if matrices:
    t0 = time.perf_counter()
    np.cov(xh.T, bias=True)
    t_cov = time.perf_counter() - t0
  pick = np.linspace(0, G - 1, rows).astype(int) if rows < G else np.arange(G)
  t0 = time.perf_counter()
  sub = np.stack([np.sqrt(np.abs(xh[:, i:i + 1] - xh)).mean(axis=0) for i in pick])
  float(np.sum((np.sqrt(np.abs(y[pick][:, None] - y[None, :])) - sub) ** 2))
  t_var = (time.perf_counter() - t0) * G / len(pick) / 2          # whole rows were formed: the upper triangle is half
  return t_copy, t_cov, t_var, pick, sub


def case(eng, S, G, matrices, rep, rows):
  x = make_x(S, G, eng.device)
  y_h = (x[S // 2] + 3.0).cpu().numpy()
  y_h[3::5] = np.nan
  y = torch.from_numpy(y_h).to(eng.device)
  say(f'### S = {S:,} x G = {G:,}, {"matrices" if matrices else "score only"}: {S * G * (G + 1) / 2:.3g} pair terms')
  say()
  say('| form | outputs | mean ms | min ms | calls | T pair terms / s (min) |')
  say('|---|---|---|---|---|---|')
  scores, cov, vario = device_times(eng, x, y, matrices, rep)
  say()
  t_copy, t_cov, t_var, pick, sub = host_times(x, y_h, rows, matrices)
  say(f'Host path on the same box: device-to-host copy of the {S * G * 8 / 1e6:.0f} MB matrix {t_copy * 1e3:.1f} ms'
      + (f'; np.cov {t_cov * 1e3:.1f} ms' if matrices else '')
      + f'; variogram and score of one p in numpy, row by row, {t_var:.2f} s'
      + (f' (extrapolated from {len(pick)} of {G} rows)' if len(pick) < G else '') + '.')
  if vario is not None:
    eng.debug_poison_lds()
    got = eng.sample_pair_moments(x, 0.5, y)
    err = np.abs(got['variogram'].cpu().numpy()[pick] - sub)
    say(f'Device variogram (p = 0.5) against those numpy rows: max relative difference {np.max(err / np.maximum(sub, 1e-300)):.2e}.')
  say(f'Scores: ' + ', '.join(f'p = {p}: {v:.6g}' for p, v in scores.items()) + '.')
  say()


def accuracy(eng):
  """The worst device error over bar on the grid of tests/test_gpu_dependence.py."""
  worst = {}
  for kind in D.KINDS + ('big',):
    for S in D.GRID_S:
      for G in D.GRID_G:
        if G == D.GRID_G[-1] and S not in D.GRID_S_AT_LARGEST_G:
          continue
        x, y, ref = D.dependence_case(S, G, kind)
        for p in D.ORDERS:
          eng.debug_poison_lds()
          got = eng.sample_pair_moments(torch.from_numpy(np.array(x)).to(eng.device), p, np.array(y))
          got = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in got.items()}
          checks = [('mean', np.abs(got['mean'] - ref['mean']), D.mean_bars(x)),
                    ('covariance', np.abs(got['covariance'] - ref['cov']), D.cov_bars(x, ref['A'])),
                    (f'variogram p = {p}', np.abs(got['variogram'] - ref['vario'][p]), D.vario_bars(S, ref['vario'][p]))]
          score, e, wt = ref['score'][p]
          if not np.isnan(score):
            checks.append((f'score p = {p}', np.asarray([abs(got['variogram_score'] - score)]),
                           np.asarray([D.score_bar(S, ref['vario'][p], y, p, score, e, wt)])))
          for name, err, bar in checks:
            r = float(np.max(err / np.where(bar > 0, bar, np.inf), initial=0.0))
            worst[name] = max(worst.get(name, 0.0), r)
  say('| quantity | worst device error / bar |')
  say('|---|---|')
  for name, r in worst.items():
    say(f'| {name} | {r:.3f} |')
  say()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sample_dependence.md'))
  args = ap.parse_args()
  net, _, _, _ = util.make_problem(n_rows=16, width=64, depth=1, observation_model='NORMAL')
  eng = Engine(net, members=1, forward_only=True, row_capacity=128, compute_dtype='fp32')
  say('# bnf_sample_pair_moments: covariance, variogram and variogram score of sample paths')
  say()
  say(f'Written by scripts/profile_sample_dependence.py on {torch.cuda.get_device_name(0)}.  Device times are HIP events on '
      'the handle\'s stream around one call (k_column_means, k_pair_moments, k_vario_finish), one warm-up call before.  '
      'A pair term is one path of one pair of columns on or above the diagonal; with matrices it feeds the covariance and '
      'the variogram sum, without them the variogram sum alone.')
  say()
  say('## Error over bar (bars: tests/dependence_ref.py), kinds normal / count / 1e9 + small integers')
  say()
  accuracy(eng)
  say('## Times')
  say()
  case(eng, 1000, 522, True, 20, 1 << 30)
  case(eng, 4096, 4096, True, 3, 16)
  case(eng, 4096, 20000, False, 2, 4)
  eng.close()
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f:
    f.write('\n'.join(LINES) + '\n')


if __name__ == '__main__':
  main()
