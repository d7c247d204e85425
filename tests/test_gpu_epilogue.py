"""The likelihood epilogue at real-data scale, on its own, at every place that evaluates it; and the count forecast
moments / mixture quantiles on the same grid.

tests/epilogue_f32.py drives the epilogue alone: the output layer's Dense kernel is zero, so the step loss and the
gradients of the output bias, the output scale, `shape`, `inflated_loc_probs` and `log_noise_scale` depend on the row
epilogue only -- no contraction, no bf16 or fp8 operand.  The call sites:
  'fp32' 'layers'       k_row_loss
  'fp32' 'auto'         the fused last-layer kernel (bnf_gemm.h, width 64)
  'fp32_split' 'auto'   the same on the split-bf16 contractions
  'bf16' 'panel'        the row-panel kernel (bnf_panel.h), which also has a NORMAL branch of its own
  'fp8' 'panel'         the same with fp8 operand storage
Counts (NB, ZINB): total_count {0.05, 1, 40, 1e3} x mean {0.02, 5, 400, 2e4, 1e6}, three members at (total_count, mean) x
(0.5, 1, 2), 320 rows drawn from the centre member's law, one row 0 and one the largest draw; plus the suite's old toy
regime with half-integer targets (the branch for a y that is no integer).  NORMAL: log_noise_scale {-20, 0, 3} x outputs
and targets around {0, 1e3, 1e5}.

For the step loss and each of the five gradients:  err = |Q_dev - Q_f64| / sum over rows |q_r,f64|  must not exceed
max(util.FP32_GATE, 4 x err_f32), err_f32 being the same error of the float32 numpy restatement of row_loss_eval's forms
(the 4 covers a device logf / lgammaf / expf a few ulp off numpy's correctly rounded ones: a judgement, not a
measurement).  The same bar at all five call sites: the epilogue is f32 in every one of them.

Which side of that max applies is known before any GPU run (tests/test_epilogue_f32.py asserts it): the gate, at every
grid point and for every quantity -- 4 x err_f32 <= 1.3e-5 for the gradients (gate 1e-4) and <= 4.8e-6 for the loss (gate
1e-5); share of cases on the looser side: loss 0 / 40, shape gradient 0 / 40, output bias and output scale 0 / 40.
"""
import functools

import numpy as np
import pytest
import torch

from bayesnf_amd.engine import Engine
from oracle import bnf_oracle as O
from tests import epilogue_f32 as H
from tests import util
from tests.test_gpu_sampling import MEAN_F, PI, TC_F, inv_softplus

pytestmark = pytest.mark.gpu

SITES = [('fp32', 'layers', 64), ('fp32', 'auto', 64), ('fp32_split', 'auto', 64), ('bf16', 'panel', 256),
         ('fp8', 'panel', 256)]


@functools.lru_cache(maxsize=None)
def _cases(obs, width):
  """[(label, theta, y, float64 terms, bars)] of one observation model: computed once, shared by the call sites of equal
  width (the terms depend on the member scalars only, the parameter layout on the width)."""
  net, model, X = H.problem(obs, width)
  cases = []
  if obs == 'NORMAL':
    for lns in H.NORMAL_LNS:
      for mag in H.NORMAL_MAGS:
        cases.append((f'lns={lns:g} out~{mag:g}',) + H.normal_case(model, lns, mag))
  else:
    for tc in H.TCS:
      for mean in H.MEANS:
        cases.append((f'tc={tc:g} mean={mean:g}',) + H.count_case(model, tc, mean))
    cases.append(('toy, y + 0.5',) + H.toy_case(model, half_integer=True))
  out = []
  for label, theta, y in cases:
    ref = H.oracle_terms(model, theta, y)
    out.append((label, theta, y, ref, H.bars(H.errors(H.f32_terms(model, theta, y, 'engine'), ref))))
  return net, model, X, out


def _device_terms(model, loss, g):
  return {q: (loss if q == 'loss' else g[:, model.leaf[H.leaf_name(model, q)].offset]) for q in H.QUANTITIES}


@pytest.mark.parametrize('obs', ['NB', 'ZINB', 'NORMAL'])
@pytest.mark.parametrize('dtype,pipeline,width', SITES)
def test_epilogue_alone_against_float64(dtype, pipeline, width, obs):
  net, model, X, cases = _cases(obs, width)
  eng = Engine(net, X=X, y=cases[0][2], members=3, prior_weight=0.0, compute_dtype=dtype, pipeline=pipeline)
  used = [q for q in H.QUANTITIES if not (q == 'infl' and obs != 'ZINB')]
  unused = {'NB': ('log_noise_scale', 'inflated_loc_probs'), 'ZINB': ('log_noise_scale',),
            'NORMAL': ('shape', 'inflated_loc_probs')}[obs]
  bad = []
  for poisoned in (True, False):       # the whole grid once with every CU's LDS full of quiet NaNs, then plainly
    for label, theta, y, ref, bars in cases:
      eng.set_targets(y)
      eng.set_params(theta)
      if poisoned:
        eng.debug_poison_lds(0x7fc00000)
      loss, g = eng.debug_loss_and_grad()
      assert np.all(np.isfinite(loss)) and np.all(np.isfinite(g)), (label, poisoned)
      for name in unused:               # likelihood-only gradient of the unused observation leaves is exactly 0
        assert np.all(g[:, model.leaf[name].offset] == 0), (label, name)
      err = H.errors(_device_terms(model, loss, g), ref)
      print(f'{dtype} {pipeline} {obs} {label}{" (LDS poisoned)" if poisoned else ""}: ' +
            ' '.join(f'{q} {err[q]:.1e} ({bars[q][1]} {bars[q][0]:.1e})' for q in used))
      bad += [(label, poisoned, q, err[q], bars[q]) for q in used if not err[q] <= bars[q][0]]
  eng.close()
  assert not bad, bad


# --------------------------------------------------------------------------- count moments and quantiles
QS = (0.001, 0.025, 0.5, 0.975, 0.999)


def _quantile_case(model, tc, M):
  """tests/test_gpu_sampling.py count_case on the thinned means: one row per mean, all in ONE call, so the bracket the
  rows share spans [0, ~1e7] while the smallest mean is 0.02."""
  tcs = tc * np.asarray(TC_F[:M])
  means = np.asarray(H.MEANS)[None, :] * np.asarray(MEAN_F[:M])[:, None]
  aux = np.stack([np.ones(M), 1.0 / tcs, np.full(M, PI)], axis=1).astype(np.float32)
  loc = inv_softplus(tcs[:, None] ** 2 / means).astype(np.float32)
  theta = np.zeros((M, model.P))
  theta[:, model.leaf['shape'].offset] = inv_softplus(aux[:, 1].astype(np.float64))
  p = aux[:, 2].astype(np.float64)
  theta[:, model.leaf['inflated_loc_probs'].offset] = np.log(p) - np.log1p(-p)
  return loc, aux, O.count_forecast(model, theta, loc.astype(np.float64))


@pytest.mark.parametrize('M', [1, 7])
@pytest.mark.parametrize('obs', ['NB', 'ZINB'])
def test_count_moments_and_quantiles_on_the_grid(obs, M):
  """bnf_count_mixture_quantiles on float32 inputs built directly: means against the float64 forecast at the existing
  test's 3e-4; every returned k a non-negative integer with mixture cdf(k) >= q - 3e-5 and cdf(k - 1) <= q + 3e-5 (or
  k = 0) under the float64 CDF of the same float32 inputs -- 3e-5 is test_extreme_quantiles_normal_and_counts' allowance
  over the root finder's 1e-5 value tolerance."""
  net, model, _, _ = util.make_problem(n_rows=16, width=64, depth=1, observation_model=obs)
  eng = Engine(net, members=1, forward_only=True, row_capacity=128, compute_dtype='fp32')
  bad = []
  for tc in H.TCS:
    loc, aux, fc = _quantile_case(model, tc, M)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(eng.device)
    means, k = eng.count_mixture_quantiles(dev(loc), dev(aux), QS)
    torch.cuda.synchronize()
    means, k = means.cpu().numpy(), k.cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(means)) and np.all(np.isfinite(k))
    e_mean = max(util.rel_err(means, fc['mean']), float(np.max(np.abs(means - fc['mean']) / fc['mean'])))   # and row by row
    assert np.all(k == np.round(k)) and np.all(k >= 0), (tc, k)
    for i, q in enumerate(QS):
      F_k = O.count_cdf(fc, k[i][None, :]).mean(axis=0)
      F_lo = O.count_cdf(fc, np.maximum(k[i] - 1, 0)[None, :]).mean(axis=0)
      print(f'{obs} M={M} tc={tc:g} q={q:g}: k={k[i].tolist()} cdf(k)-q={np.round(F_k - q, 6).tolist()} '
            f'cdf(k-1)-q={np.round(F_lo - q, 6).tolist()} means rel err {e_mean:.1e}')
      for r in range(k.shape[1]):
        if not (F_k[r] >= q - 3e-5 and (F_lo[r] <= q + 3e-5 or k[i, r] == 0)):
          bad.append((tc, H.MEANS[r], q, k[i, r], F_k[r] - q, F_lo[r] - q))
    assert e_mean < 3e-4, (tc, e_mean)
  eng.close()
  assert not bad, bad
