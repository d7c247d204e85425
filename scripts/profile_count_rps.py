"""HIP-event time of bnf_count_rps at 10,232 rows x 64 members (NB, means around 400) next to the wall time of the same
sum in numpy float64 on the host (tests/rps_ref.py count_rps_ref on 32 of the rows, scaled to all of them).  Prints one JSON
line: the figures of profiles/count_rps.md.  Run from the repository root: python scripts/profile_count_rps.py"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayesnf_amd.engine import Engine
from tests import rps_ref as P
from tests import util
from tests.test_gpu_sampling import inv_softplus

R, M = 10232, 64
rng = np.random.default_rng(0)
tcs = rng.uniform(2.0, 20.0, M)
means = 400.0 * np.exp(0.3 * rng.standard_normal(R))[None, :] * np.exp(0.1 * rng.standard_normal((M, R)))
aux = np.stack([np.ones(M), 1.0 / tcs, np.zeros(M)], axis=1).astype(np.float32)
loc = inv_softplus(tcs[:, None] ** 2 / means).astype(np.float32)
y = np.round(means.mean(axis=0) * np.exp(0.4 * rng.standard_normal(R))).astype(np.float32)

net, model, _, _ = util.make_problem(n_rows=16, width=64, depth=1, observation_model='NB')
eng = Engine(net, members=1, forward_only=True, row_capacity=128, compute_dtype='fp32')
d = lambda a: torch.from_numpy(a).to(eng.device)
loc_d, aux_d, y_d = d(loc), d(aux), d(y)
out = torch.empty(R, dtype=torch.float32, device=eng.device)
p = lambda t: C.c_void_p(t.data_ptr())
call = lambda: eng.lib.bnf_count_rps(eng.handle, p(loc_d), p(aux_d), M, R, p(y_d), p(out))
for _ in range(2):
  assert call() == 0
torch.cuda.synchronize()
times = []
for _ in range(5):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  assert call() == 0
  e1.record()
  torch.cuda.synchronize()
  times.append(e0.elapsed_time(e1))
got = out.cpu().numpy()
eng.close()

n_host = 32
rows = np.arange(0, R, R // n_host)[:n_host]
fc = P.forecast(model, loc[:, rows], aux)
t0 = time.perf_counter()
ref = P.count_rps_ref(fc, y[rows])
host = time.perf_counter() - t0
f64, terms, _ = P.count_rps_f64(loc[:, rows], aux, y[rows], 'NB')
res = dict(rows=R, members=M, device_ms=times, device_ms_median=float(np.median(times)), nan_rows=int(np.isnan(got).sum()),
           host_rows=n_host, host_seconds=host, host_seconds_scaled=host * R / n_host,
           device_err=P.rel_err(got[rows], ref), restatement_err=P.rel_err(f64, ref),
           window_median=float(np.median(terms)), window_max=int(terms.max()), mean_rps=float(np.nanmean(got)))
print(json.dumps(res))
