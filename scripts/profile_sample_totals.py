"""Wall times of bnf_sample_summaries / bnf_sample_energy_score / score_totals beside the host path: the figures of
profiles/sample_totals.md.  Run from the repository root on one MI355X: python scripts/profile_sample_totals.py  Device times: HIP events on the handle's stream, warm-up 2, mean and min of `rep` calls.
Host times: time.perf_counter around work that ends in a device synchronise (or is pure numpy)."""
import os
import sys
import time

import numpy as np
import pandas as pd
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayesnf_amd import BayesianNeuralFieldMAP  # noqa: E402
from bayesnf_amd.engine import Engine  # noqa: E402
from tests import totals_ref as T  # noqa: E402
from tests import util  # noqa: E402
from tests.test_gpu_sampling import MODEL  # noqa: E402

LEVELS = (0.025, 0.5, 0.975)


def say(*a):
  print(*a, flush=True)


def events(fn, rep, warm=2):
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
  return float(np.mean(ms)), float(np.min(ms)), rep


def wall(fn, rep, warm=1):
  for _ in range(warm):
    fn()
  s = []
  for _ in range(rep):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    s.append(time.perf_counter() - t0)
  return float(np.mean(s)), float(np.min(s)), rep


def entry_points(eng, x, y, tag, rep_sum, rep_es):
  import ctypes as C
  from bayesnf_amd import _native
  from bayesnf_amd.engine import _ptr
  S, G = x.shape
  f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=eng.device)
  mean, quant, crps, pit, out = f64(G), f64(len(LEVELS), G), f64(G), f64(2, G), f64(1)
  qa = (C.c_double * len(LEVELS))(*LEVELS)
  tiles = -(-S // _native.ENERGY_SAMPLE_TILE)
  work = f64(S + tiles * (tiles + 1) // 2)

  def summ():
    _native.check(eng.lib.bnf_sample_summaries(eng.handle, _ptr(x), S, G, _ptr(y), qa, len(LEVELS), _ptr(mean), _ptr(quant),
                                               _ptr(crps), _ptr(pit)), 'summaries')

  def es():
    _native.check(eng.lib.bnf_sample_energy_score(eng.handle, _ptr(x), S, G, _ptr(y), _ptr(work),
                                                  C.c_size_t(work.numel() * 8), _ptr(out)), 'energy')
  m, lo, n = events(summ, rep_sum)
  say(f'{tag}: bnf_sample_summaries (3 levels, crps, pit)  mean {m:.3f} ms  min {lo:.3f} ms  ({n} calls, HIP events)')
  m, lo, n = events(es, rep_es)
  say(f'{tag}: bnf_sample_energy_score                      mean {m:.3f} ms  min {lo:.3f} ms  ({n} calls, HIP events); '
      f'{S * S * G / 2 / (lo * 1e-3) / 1e12:.2f} T differences / s')
  return crps.cpu().numpy(), float(out.cpu()[0])


def host_path(est, table, group_by, S, seed, crps_cols, es_cols, tag):
  t0 = time.perf_counter()
  totals, keys = est.predict_samples(table, S, seed, group_by=group_by)
  t_tot = time.perf_counter() - t0
  observed = table.groupby(group_by)[est.target_col].sum().reindex(keys).to_numpy(dtype=np.float64)
  t0 = time.perf_counter()
  np.quantile(totals, LEVELS, axis=0)
  totals.mean(axis=0)
  t_q = time.perf_counter() - t0
  G = totals.shape[1]
  cc = np.linspace(0, G - 1, crps_cols).astype(int) if crps_cols < G else np.arange(G)
  t0 = time.perf_counter()
  crps = T.crps_ref(np.ascontiguousarray(totals[:, cc]), observed[cc])
  t_c = time.perf_counter() - t0
  ce = np.linspace(0, G - 1, es_cols).astype(int) if es_cols < G else np.arange(G)
  t0 = time.perf_counter()
  es = T.energy_ref(np.ascontiguousarray(totals[:, ce]), observed[ce])[0]
  t_e = time.perf_counter() - t0
  say(f'{tag} host path: predict_samples totals -> numpy {t_tot:.3f} s; np.quantile (3 levels) + mean {t_q:.3f} s; '
      f'reference CRPS on {len(cc)} of {G} groups {t_c:.3f} s (all groups at that rate: {t_c * G / len(cc):.1f} s); '
      f'reference energy score on {len(ce)} of {G} groups {t_e:.3f} s (all groups at that rate: {t_e * G / len(ce):.1f} s)')
  return totals, observed, cc, crps, ce, es


def main():
  golden = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden')
  df = pd.read_csv(os.path.join(golden, 'chickenpox.8.train.csv'), index_col=0, parse_dates=['datetime'])
  est = BayesianNeuralFieldMAP(**MODEL, observation_model='NB', compute_dtype='fp32').fit(
      df, seed=3, ensemble_size=4, num_epochs=20, learning_rate=0.01)
  net, _, _, _ = util.make_problem(n_rows=16, width=64, depth=1, observation_model='NORMAL')
  eng = Engine(net, members=1, forward_only=True, row_capacity=128, compute_dtype='fp32')

  # ---- A: 522 weeks (the length of the whole chickenpox series) x the fixture's locations, synthetic counts -------------
  S = 1000
  places = df[['location', 'latitude', 'longitude']].drop_duplicates()
  weeks = pd.DataFrame({'datetime': pd.date_range('2005-01-03', periods=522, freq='W-MON')})
  df = weeks.merge(places, how='cross')
  df['chickenpox'] = np.random.default_rng(0).poisson(30.0, len(df)).astype(np.float64)
  say(f'A: {len(df)} rows = 522 weeks x {len(places)} places')
  totals, observed, cc, crps_h, ce, es_h = host_path(est, df, 'datetime', S, 3, 1 << 30, 1 << 30, 'A (S=1000, G=522)')
  x, y = torch.from_numpy(totals).to(eng.device), torch.from_numpy(observed).to(eng.device)
  crps_d, es_d = entry_points(eng, x, y, f'A (S={S}, G={totals.shape[1]})', 20, 20)
  say(f'A: device vs host reference: crps max abs diff {np.nanmax(np.abs(crps_d[cc] - crps_h)):.2e}, energy {abs(es_d - es_h):.2e}')
  m, lo, n = wall(lambda: est.score_totals(df, 'datetime', num_samples=S, seed=3), 5)
  say(f'A: score_totals end to end  mean {m:.3f} s  min {lo:.3f} s  ({n} calls, synchronised wall clock, 1 warm-up)')
  m, lo, n = wall(lambda: est.predict_samples(df, S, 3, group_by='datetime'), 5)
  say(f'A: predict_samples(group_by) end to end  mean {m:.3f} s  min {lo:.3f} s  ({n} calls): the part of score_totals '
      'that both paths share')

  # ---- B: 20,000 synthetic groups ------------------------------------------------------------------------------------
  S, G = 4096, 20000
  big = pd.concat([df] * (-(-4 * G // len(df))), ignore_index=True).iloc[:4 * G].copy()
  big['cell'] = np.arange(4 * G) // 4
  totals, observed, cc, crps_h, ce, es_h = host_path(est, big, 'cell', S, 3, 40, 200, f'B (S={S}, G={G})')
  x, y = torch.from_numpy(totals).to(eng.device), torch.from_numpy(observed).to(eng.device)
  crps_d, _ = entry_points(eng, x, y, f'B (S={S}, G={G})', 5, 3)
  say(f'B: device vs host reference on the subset: crps max abs diff {np.nanmax(np.abs(crps_d[cc] - crps_h)):.2e}')
  ysub = torch.full((G,), float('nan'), dtype=torch.float64)
  ysub[torch.from_numpy(ce)] = torch.from_numpy(observed[ce])
  say(f'B: energy score on the 200-group subset: device {eng.sample_energy_score(x, ysub.to(eng.device)):.9f} host {es_h:.9f}')
  del x
  m, lo, n = wall(lambda: est.score_totals(big, 'cell', num_samples=S, seed=3), 2)
  say(f'B: score_totals end to end  mean {m:.3f} s  min {lo:.3f} s  ({n} calls, synchronised wall clock, 1 warm-up)')
  m, lo, n = wall(lambda: est.predict_samples(big, S, 3, group_by='cell'), 2)
  say(f'B: predict_samples(group_by) end to end  mean {m:.3f} s  min {lo:.3f} s  ({n} calls)')
  eng.close()


if __name__ == '__main__':
  main()
