"""The likelihood epilogue (bayesnf_amd/csrc/bnf_device.h row_loss_eval) driven on its own, and restated in float32.

`epilogue_theta` makes the output layer's Dense kernel zero, so that member e's network output is exactly
softplus(inv_sp_output_scale_e) * output_bias_e on every pipeline and in every compute dtype: no contraction and no bf16
operand enters the step loss or the gradients of the output bias, the output scale, `shape`, `inflated_loc_probs` and
`log_noise_scale`.  Those five depend on the row epilogue alone.

Three evaluations of the same per-row terms, from the same float32 parameters and targets:
  `oracle_terms`   float64, through oracle/bnf_oracle.py;
  `f32_terms(.., form='tfp')`     numpy float32, operation by operation, of TFP's formulas as written (what the engine
                                  evaluated before the well-conditioned forms went in; kept as the yardstick);
  `f32_terms(.., form='engine')`  numpy float32, operation by operation, of what row_loss_eval evaluates now.
The rows' float32 terms are summed in float64: the restatements measure the conditioning of the row formula, not the
order of a float32 sum (which costs a few 1e-7 of the sum of the terms' magnitudes, far inside the gate).

Every error is |Q - Q_f64| / sum over rows |q_r,f64|: the rows' terms of a gradient cancel by design near the optimum, so
the sum itself is no scale to measure against.
"""
import numpy as np
from scipy import special as sp

from oracle import bnf_oracle as O
from tests import util

F = np.float32
QUANTITIES = ('loss', 'bias', 'scale', 'par', 'infl')   # par: `shape` (NB / ZINB) or `log_noise_scale` (NORMAL)

# the count grid: tests/test_gpu_sampling.py's TCS / MEANS, thinned
TCS = (0.05, 1.0, 40.0, 1e3)
MEANS = (0.02, 5.0, 400.0, 2e4, 1e6)
MEMBER_F = (0.5, 1.0, 2.0)      # the three members sit at (total_count, mean) x these; the targets are drawn from the centre one
PI = 0.35
N_ROWS = 320                    # not a multiple of 256: a ragged last block
NORMAL_LNS = (-20.0, 0.0, 3.0)  # the first puts sigma at its 0.01 floor
NORMAL_MAGS = (0.0, 1e3, 1e5)


def inv_softplus(y):
  """log(expm1(y)) without overflow."""
  y = np.asarray(y, dtype=np.float64)
  return np.where(y > 30.0, y, np.log(np.expm1(np.minimum(y, 30.0))))


def leaf_name(model, q):
  L = model.depth
  return {'bias': f'Dense_{L}/bias', 'scale': 'inv_sp_output_scale', 'infl': 'inflated_loc_probs',
          'par': 'log_noise_scale' if model.observation_model == 'NORMAL' else 'shape'}[q]


def epilogue_theta(model, outs, seed=1, **leaves):
  """(E, P) float32-representable parameters: small random values (util.random_theta, scale 0.1), the output layer's
  kernel zero, and the output bias chosen so that the network output of member e is outs[e] (to float32 rounding)."""
  E = len(outs)
  theta = util.random_theta(model, E, seed=seed, scale=0.1)
  L = model.depth
  k = model.leaf[f'Dense_{L}/kernel']
  theta[:, k.offset:k.offset + k.size] = 0.0
  for name, val in leaves.items():
    theta[:, model.leaf[name].offset] = val
  theta = theta.astype(np.float32).astype(np.float64)
  gam = O.softplus(theta[:, model.leaf['inv_sp_output_scale'].offset])
  theta[:, model.leaf[f'Dense_{L}/bias'].offset] = np.asarray(outs, dtype=np.float64) / gam
  return theta.astype(np.float32).astype(np.float64)


def count_case(model, tc, mean, seed=0):
  """theta (3, P) and y (N_ROWS,) of one grid point: members at (tc, mean) x MEMBER_F, 318 targets drawn from the centre
  member's law with numpy's Gamma-Poisson sampler (capped at 2^24, the largest count float32 steps through one by one: the
  cap binds at total_count 0.05, mean 1e6 only), one row forced to 0 and one to the largest draw."""
  tcs = tc * np.asarray(MEMBER_F)
  means = mean * np.asarray(MEMBER_F)
  shape = 1.0 / tcs
  outs = inv_softplus(tcs ** 2 / means)            # NB mean = 1 / (shape^2 softplus(out))
  p = PI
  theta = epilogue_theta(model, outs, shape=inv_softplus(shape), inflated_loc_probs=np.log(p) - np.log1p(-p))
  rng = np.random.default_rng([seed, int(round(tc * 100)), int(round(mean * 100))])
  y = np.minimum(rng.poisson(rng.gamma(tc, mean / tc, N_ROWS - 2)).astype(np.float64), 2.0 ** 24)
  if model.observation_model == 'ZINB':
    y = y * (rng.random(N_ROWS - 2) >= PI)
  y = np.concatenate([[0.0, y.max()], y])
  assert y.max() <= 2.0 ** 24, y.max()             # every count is a float32 integer
  return theta, y


def normal_case(model, lns, mag, seed=0):
  """Members whose outputs sit one sigma apart around `mag`, targets `mag` + 2 sigma N(0, 1) rounded to float32.
  inv_sp_output_scale is 32 here: softplus(32) is 32 in float32 whatever log1p / exp are used (the correction, 1.3e-14,
  is far below half an ulp), so the output 32 * bias is the float32 number it was meant to be on the device, in the
  float32 restatement and in float64 alike.  Otherwise the rounding of that one product (up to 0.004 at 1e5, against
  sigma = 0.01) would be all that the comparison sees, and it belongs to the forward pass, not to the epilogue."""
  sigma = 0.01 + np.exp(lns)
  outs = (mag + sigma * np.asarray([-1.0, 0.0, 1.0])).astype(np.float32).astype(np.float64)
  theta = epilogue_theta(model, outs, log_noise_scale=lns, inv_sp_output_scale=32.0)
  L = model.depth
  assert np.all(32.0 * theta[:, model.leaf[f'Dense_{L}/bias'].offset] == outs)
  rng = np.random.default_rng([seed, int(lns) + 100, int(mag)])
  y = (mag + 2.0 * sigma * rng.standard_normal(N_ROWS)).astype(np.float32).astype(np.float64)
  return theta, y


def toy_case(model, half_integer=False):
  """The regime the suite had before the grid: the counts of util.make_problem (up to ~30), shape parameters of order
  0.4 (total_count 1 .. 2), network outputs of order 1.  half_integer: every target + 0.5 -- no count, but the engine
  takes any float, and below its thresholds such a y goes down TFP's own forms."""
  _, _, _, y = util.make_problem(n_rows=N_ROWS, width=model.width, depth=model.depth,
                                 observation_model=model.observation_model)
  theta = epilogue_theta(model, [0.3, 1.0, 1.7], shape=[-0.4, 0.0, 0.4])
  return theta, y + (0.5 if half_integer else 0.0)


def problem(obs, width=64, depth=2):
  """NetSpec, oracle Model and inputs X for N_ROWS rows (the targets come from count_case / normal_case)."""
  net, model, X, _ = util.make_problem(n_rows=N_ROWS, width=width, depth=depth, observation_model=obs)
  return net, model, X


def _member_scalars(model, theta):
  L = model.depth
  os_ = theta[:, model.leaf['inv_sp_output_scale'].offset]
  return os_, theta[:, model.leaf[f'Dense_{L}/bias'].offset]


def oracle_terms(model, theta, y):
  """{Q: (value (E,), sum over rows of |row term| (E,))} in float64 for the step loss (full batch, prior_weight 0) and
  the five scalar-leaf gradients, from the oracle's per-row likelihood terms."""
  os_, b = _member_scalars(model, theta)
  gam = O.softplus(os_)
  E = theta.shape[0]
  out = np.broadcast_to((gam * b)[:, None], (E, len(y)))
  yb = np.broadcast_to(y, out.shape)
  ll = O.loglik(model, theta, out, yb, per_row=True)
  dll_dout, _, rows = O._dloglik_dout_and_params(model, theta, out, yb, per_row=True)   # pylint: disable=protected-access
  dout = -dll_dout
  t = {'loss': -ll, 'bias': gam[:, None] * dout, 'scale': (O.sigmoid(os_) * b)[:, None] * dout,
       'par': -rows[leaf_name(model, 'par')],
       'infl': -rows['inflated_loc_probs'] if 'inflated_loc_probs' in rows else np.zeros_like(ll)}
  return {q: (v.sum(axis=1), np.abs(v).sum(axis=1)) for q, v in t.items()}


# ------------------------------------------------------------------------------------------------ float32 restatement
def softplusf(x):
  return np.maximum(x, F(0)) + np.log1p(np.exp(-np.abs(x)))


def sigmoidf(x):
  e = np.exp(-np.abs(x))
  return np.where(x >= 0, F(1) / (F(1) + e), e / (F(1) + e))


def lgammaf(x):
  return sp.gammaln(np.asarray(x, dtype=F)).astype(F)


def _psi_tail(x):
  """x >= 6: digamma(x) = log x - 1 / (2 x) - tail(x)."""
  r = F(1) / x
  r2 = r * r
  return r2 * (F(1 / 12) - r2 * (F(1 / 120) - r2 * (F(1 / 252) - r2 * F(1 / 240))))


def digammaf(x):
  """bnf_device.h digammaf: recurrence up to x >= 6, then the asymptotic series."""
  x = np.array(x, dtype=F)
  acc = np.zeros_like(x)
  for _ in range(6):
    lo = x < F(6)
    acc = np.where(lo, acc - F(1) / x, acc)
    x = np.where(lo, x + F(1), x)
  return acc + np.log(x) - F(0.5) / x - _psi_tail(x)


def _stirling_corr(x):
  """x >= 10: lgamma(x + 1) = x log x - x + log(2 pi x) / 2 + corr(x), corr = 1 / (12 x) - 1 / (360 x^3)."""
  ix = F(1) / x
  return ix * F(1 / 12) * (F(1) - ix * ix * F(1 / 30))


def _nb_tfp(y, tc, shape, mean):
  """TFP 0.24 NegativeBinomial.log_prob and its derivatives, term by term."""
  logits = -np.log(shape) - np.log(mean)
  sg = sigmoidf(logits)
  lsn = -softplusf(logits)
  lp = tc * lsn + y * (-softplusf(-logits)) + lgammaf(tc + y) - lgammaf(F(1) + y) - lgammaf(tc)
  dl_dlogits = y * (F(1) - sg) - tc * sg
  dl_dtc = lsn + digammaf(tc + y) - digammaf(tc)
  return lp, dl_dlogits, dl_dtc


def _nb_engine(y, tc, shape, mean):
  """row_loss_eval's forms (see its header comment)."""
  y, tc, shape, mean = np.broadcast_arrays(y, tc, shape, mean)
  sm = shape * mean                 # e^-logits = total_count / NB mean
  rsm = F(1) / sm                   # e^logits
  mu = tc * rsm                     # NB mean
  lsn = -np.log1p(rsm)              # log sigmoid(-logits)
  sgp = F(1) / (F(1) + sm)          # sigmoid(logits)
  dl_dlogits = (y - mu) * (F(1) / (F(1) + rsm))
  n = tc + y
  den = tc + mu
  delta = y - mu
  l1 = np.where(np.abs(delta) <= F(0.5) * den, np.log1p(delta / den), np.log(n / den))   # log((tc + y) / (tc + mu))
  integer = y == np.floor(y)
  # -- log pmf
  small = integer & (y < F(10))
  acc = np.zeros_like(sm)
  for j in range(9):
    fj = F(j)
    acc = np.where(fj < y, acc + np.log((tc + fj) / (F(1) + fj) * sgp), acc)
  lp_small = tc * lsn + acc
  ys = np.maximum(y, F(10))         # the large-y branch on safe arguments where it is not selected
  ns = tc + ys
  x2 = tc * (mu - ys) / (ys * den)
  l1s = np.where(np.abs(ys - mu) <= F(0.5) * den, np.log1p((ys - mu) / den), np.log(ns / den))
  l2 = np.where(np.abs(x2) <= F(0.5), np.log1p(x2), np.log((ns / den) * (mu / ys)))
  tcb = np.maximum(tc, F(10))
  a_big = F(0.5) * np.log(tcb) - F(0.918938533204672742) - _stirling_corr(tcb)
  tcs_ = np.minimum(tc, F(10))
  a_small = tcs_ * np.log(tcs_) - tcs_ - lgammaf(tcs_)
  a_tc = np.where(tc >= F(10), a_big, a_small)
  lp_big = tc * l1s + ys * l2 - F(0.5) * (np.log(ns) + np.log(ys)) + a_tc + _stirling_corr(ns) - _stirling_corr(ys)
  lp_tfp = tc * lsn + y * (-np.log1p(sm)) + lgammaf(n) - lgammaf(F(1) + y) - lgammaf(tc)
  lp = np.where(y >= F(10), lp_big, np.where(small, lp_small, lp_tfp))
  # -- d log pmf / d total_count
  n6 = np.maximum(n, F(6))
  tc6 = np.maximum(tc, F(6))
  g_tc = np.where(tc >= F(6), F(0.5) / tc6 + _psi_tail(tc6), np.log(tc) - digammaf(tc))
  d_big = g_tc + l1 - F(0.5) / n6 - _psi_tail(n6)
  hs = np.zeros_like(sm)
  for j in range(6):
    fj = F(j)
    hs = np.where(fj < y, hs + F(1) / (tc + fj), hs)
  d_small = lsn + hs
  d_tfp = lsn + digammaf(n) - digammaf(tc)
  dl_dtc = np.where(n >= F(6), d_big, np.where(integer, d_small, d_tfp))
  return lp, dl_dlogits, dl_dtc


def f32_terms(model, theta, y, form):
  """{Q: value (E,)} of the float32 restatement `form` ('tfp' or 'engine'); rows summed in float64."""
  assert form in ('tfp', 'engine')
  th = theta.astype(F)
  yv = np.asarray(y, dtype=F)[None, :]
  os_, b = (v.astype(F) for v in _member_scalars(model, theta))
  gam = softplusf(os_)
  out = (gam * b)[:, None]
  obs = model.observation_model
  d_infl = np.zeros((th.shape[0], yv.shape[1]), dtype=F)
  with np.errstate(all='ignore'):
    if obs == 'NORMAL':     # one form: both the shared epilogue and the row-panel kernel's own branch evaluate this
      lns = th[:, model.leaf['log_noise_scale'].offset][:, None]
      sigma = F(0.01) + np.exp(lns)
      res = yv - out
      z = res / sigma
      ll = -F(0.5) * z * z - np.log(sigma) - F(0.918938533204672742)
      dout = -res / (sigma * sigma)
      d_par = -(res * res / (sigma * sigma * sigma) - F(1) / sigma) * np.exp(lns)
    else:
      ths = th[:, model.leaf['shape'].offset][:, None]
      shape = softplusf(ths)
      tc = F(1) / shape
      mean = softplusf(out)
      lp, dl_dlogits, dl_dtc = (_nb_tfp if form == 'tfp' else _nb_engine)(yv, tc, shape, mean)
      if obs == 'ZINB':
        thp = th[:, model.leaf['inflated_loc_probs'].offset][:, None]
        pi = sigmoidf(thp)
        p0 = np.exp(lp)
        den = (F(1) - pi) * p0 + pi
        w = (F(1) - pi) * p0 / den
        zero = yv == 0
        dlp_dpi = np.where(zero, (F(1) - p0) / den, -F(1) / (F(1) - pi))
        lp = np.where(zero, np.log(den), lp + (-softplusf(thp)))
        dl_dlogits = np.where(zero, dl_dlogits * w, dl_dlogits)
        dl_dtc = np.where(zero, dl_dtc * w, dl_dtc)
        d_infl = -dlp_dpi * pi * (F(1) - pi)
      ll = lp
      dout = -(-dl_dlogits / mean) * sigmoidf(out)
      d_par = -(-dl_dlogits / shape - dl_dtc / (shape * shape)) * sigmoidf(ths)
    dout = np.broadcast_to(dout, ll.shape)
    rows = {'loss': -ll, 'bias': gam[:, None] * dout, 'scale': dout * b[:, None], 'par': d_par, 'infl': d_infl}
  for v in rows.values():
    assert v.dtype == F, v.dtype
  res = {q: v.astype(np.float64).sum(axis=1) for q, v in rows.items()}
  res['scale'] = res['scale'] * sigmoidf(os_).astype(np.float64)
  return res


def errors(vals, ref):
  """{Q: max over members of |Q - Q_f64| / sum |q_r,f64|} (0 where the quantity has no rows' terms at all)."""
  out = {}
  for q in QUANTITIES:
    v, (r, den) = np.asarray(vals[q], dtype=np.float64), ref[q]
    out[q] = float(np.max(np.where(den > 0, np.abs(v - r) / np.where(den > 0, den, 1.0), np.abs(v))))
  return out


def gate(q):
  return util.FP32_GATE['loss' if q == 'loss' else 'grad']


def bars(err_f32):
  """{Q: (bar, side)}: max(FP32 gate, 4 x the float32 restatement's own error); side says which one applied."""
  return {q: (max(gate(q), 4.0 * err_f32[q]), 'gate' if gate(q) >= 4.0 * err_f32[q] else '4xf32') for q in QUANTITIES}
