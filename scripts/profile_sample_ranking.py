"""Wall time of est.score_ranking (totals, ranks, summaries and rank probabilities on the GPU) beside the host route it
replaces: predict_samples(table, S, seed, group_by=...) copies the (S, G) totals to the host, tests/ranking_ref.py ranks
them with numpy (the sort route) and forms the same summaries.  Run from the repository root on one MI355X:
python scripts/profile_sample_ranking.py [--groups 3000 --samples 1000 --top_k 10].  Median of 5 calls after one warm-up;
the device is synchronised before the clock is read.  The two new Engine calls are timed alone the same way."""
import argparse
import os
import sys
import time

import numpy as np
import pandas as pd
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bayesnf_amd import BayesianNeuralFieldMAP  # noqa: E402
from bayesnf_amd.engine import Engine  # noqa: E402
from tests import ranking_ref as R  # noqa: E402
from tests import totals_ref as T  # noqa: E402
from tests import util  # noqa: E402
from tests.test_gpu_sampling import MODEL  # noqa: E402


def median_of(fn, rep=5):
  fn()
  torch.cuda.synchronize()
  times = []
  for _ in range(rep):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    times.append(time.perf_counter() - t0)
  return float(np.median(times))


def host_route(est, table, S, seed, K, levels):
  totals, keys = est.predict_samples(table, S, seed, group_by='location')
  observed = table.groupby('location')['chickenpox'].sum().reindex(keys).to_numpy(dtype=np.float64)
  rank, above, ties = R.ranks_sorted(totals)
  o_rank = R.ranks_sorted(observed[None, :])[0][0]
  summ = T.summaries_sorted(rank, o_rank, levels)
  return dict(rank_mean=summ['mean'], rank_quantiles=summ['quantiles'], rank_crps=summ['crps'], rank_pit=summ['pit'],
              rank_probability=R.rank_prob_kernel_form(above, ties, K))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--groups', type=int, default=3000)
  ap.add_argument('--samples', type=int, default=1000)
  ap.add_argument('--top_k', type=int, default=10)
  args = ap.parse_args()
  G, S, K, seed, levels = args.groups, args.samples, args.top_k, 3, (0.025, 0.5, 0.975)
  df = pd.read_csv(os.path.join(ROOT, 'tests', 'golden', 'chickenpox.8.train.csv'), index_col=0, parse_dates=['datetime'])
  est = BayesianNeuralFieldMAP(**MODEL, observation_model='NB', compute_dtype='fp32').fit(
      df, seed=3, ensemble_size=4, num_epochs=5, learning_rate=0.01)
  rng = np.random.default_rng(1)
  weeks = df['datetime'].iloc[:2].to_numpy()
  table = pd.DataFrame({'location': np.repeat(np.arange(G), 2), 'datetime': np.tile(weeks, G),
                        'latitude': np.repeat(df['latitude'].iloc[0] + rng.uniform(-1, 1, G), 2),
                        'longitude': np.repeat(df['longitude'].iloc[0] + rng.uniform(-1, 1, G), 2),
                        'chickenpox': rng.poisson(20.0, 2 * G).astype(np.float64)})
  print(f'{torch.cuda.get_device_name(0)}: S = {S}, G = {G}, top_k = {K}, {len(table)} rows')
  gpu = est.score_ranking(table, 'location', top_k=K, quantiles=levels, num_samples=S, seed=seed)
  host = host_route(est, table, S, seed, K, levels)
  assert np.allclose(gpu['rank_mean'], host['rank_mean'], rtol=1e-12) and np.allclose(gpu['rank_pit'], host['rank_pit'])
  assert np.allclose(gpu['rank_probability'], host['rank_probability'], rtol=1e-12, atol=0.0)
  t_gpu = median_of(lambda: est.score_ranking(table, 'location', top_k=K, quantiles=levels, num_samples=S, seed=seed))
  t_copy = median_of(lambda: est.predict_samples(table, S, seed, group_by='location'))
  t_host = median_of(lambda: host_route(est, table, S, seed, K, levels))
  print(f'score_ranking, everything on the device: {t_gpu * 1e3:.1f} ms')
  print(f'host route: predict_samples(group_by) {t_copy * 1e3:.1f} ms + numpy ranking and summaries '
        f'{(t_host - t_copy) * 1e3:.1f} ms = {t_host * 1e3:.1f} ms')
  # the two new kernels alone
  net, _, _, _ = util.make_problem(n_rows=16, width=64, depth=1, observation_model='NORMAL')
  eng = Engine(net, members=1, forward_only=True, row_capacity=128, compute_dtype='fp32')
  x = torch.from_numpy(rng.poisson(40.0, (S, G)).astype(np.float64)).to(eng.device)
  r = eng.sample_ranks(x)
  for name, fn in (('bnf_sample_ranks', lambda: eng.sample_ranks(x)),
                   ('bnf_rank_probabilities', lambda: eng.rank_probabilities(r['above'], r['ties'], K))):
    print(f'{name}: {median_of(fn) * 1e3:.3f} ms (the Engine call: output allocation, launch and synchronisation)')
  eng.close()


if __name__ == '__main__':
  main()
