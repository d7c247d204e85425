"""Summaries and scores of an ensemble of sample paths (bayesnf_amd/csrc/bnf_totals.h, include/bnf.h bnf_sample_summaries /
bnf_sample_energy_score) on the host, in float64.  x (S, G): S sample paths of G totals; y (G,): the observed totals.

  brute force, straight from the definitions
    `quantiles_ref`  np.quantile (default 'linear' method)
    `pit_ref`        counting, no sort: #{x_s <= y} / S and #{x_s < y} / S
    `crps_ref`       (1 / S) sum_s |x_s - y| - (1 / (2 S^2)) sum_s sum_t |x_s - x_t|: the O(S^2) double sum per column
    `energy_ref`     (1 / S) sum_s |X_s - y| - (1 / (2 S^2)) sum_s sum_t |X_s - X_t|: the O(S^2 G) double sum, over the
                     columns with a finite y
    (math.fsum for the sums over S values; the S^2 pair terms are added per row block by numpy's pairwise sum, the block
    sums by fsum)
  the forms the kernels use, restated in numpy
    `summaries_sorted`  sort, then the mean, the lerp of the two neighbours, the counts, and the CRPS in its sorted form on
                        the centred values d_(i) = x_(i) - y
    `energy_upper`      the pairs s < t only, once: T1 / S - P / S^2

Bars (each from float64 rounding, eps = 2^-52; the issue that introduced the feature states them):
  pit        exact equality
  quantile   4 eps max(|x_(lo)|, |x_(lo+1)|) of np.quantile: one subtraction, one product, one sum, and numpy's own lerp
             variant; exact when the two neighbours are equal or (S - 1) q is an integer
  mean       S eps max |x|
  crps       S eps max_s |x_s - y|  (absolute): S terms of that size in each sum
  energy     (G + 2 S + 64) eps (T1 + T2) with T1, T2 the two positive terms of the reference: G / 2 roundings inside a
             distance, up to 2 S in the two levels of summation
"""
import functools
import math

import numpy as np

EPS = 2.0 ** -52
MAX_SAMPLES = 16384                   # BNF_SUMMARY_MAX_SAMPLES
LEVELS = (0.0, 0.025, 0.25, 0.5, 0.975, 1.0)
SUMMARY_S = (1, 2, 63, 64, 65, 1000)
SUMMARY_G = (1, 9, 65)
KINDS = ('normal', 'count')
ENERGY_SHAPES = ((1, 1), (2, 33), (65, 130), (200, 7))


# ---- brute force ---------------------------------------------------------------------------------------------------
def quantiles_ref(x, q):
  return np.quantile(np.asarray(x, dtype=np.float64), np.asarray(q, dtype=np.float64), axis=0).reshape(len(q), x.shape[1])


def pit_ref(x, y):
  S = x.shape[0]
  out = np.stack([(x <= y[None, :]).sum(axis=0), (x < y[None, :]).sum(axis=0)]).astype(np.float64) / float(S)
  out[:, ~np.isfinite(y)] = np.nan
  return out


def _pair_abs_sum(col, block=1024):
  """sum_s sum_t |col_s - col_t|"""
  parts = [float(np.abs(col[i:i + block, None] - col[None, :]).sum()) for i in range(0, len(col), block)]
  return math.fsum(parts)


def crps_ref(x, y):
  S, G = x.shape
  out = np.full(G, np.nan)
  for c in range(G):
    if np.isfinite(y[c]) and not np.isnan(x[:, c]).any():
      first = math.fsum(np.abs(x[:, c] - y[c]).tolist()) / S
      out[c] = first - _pair_abs_sum(x[:, c]) / (2.0 * S * S)
  return out


def energy_ref(x, y):
  """-> (score, T1, T2): score = T1 - T2, T1 = (1 / S) sum_s |X_s - y|, T2 = (1 / (2 S^2)) sum_st |X_s - X_t|."""
  keep = np.isfinite(y)
  if not keep.any():
    return float('nan'), float('nan'), float('nan')
  X, yk = x[:, keep], y[keep]
  S = X.shape[0]
  norm = lambda d: np.sqrt(np.sum(d * d, axis=1))
  t1 = math.fsum(norm(X - yk[None, :]).tolist()) / S
  t2 = math.fsum(float(norm(X - X[s][None, :]).sum()) for s in range(S)) / (2.0 * S * S)
  return t1 - t2, t1, t2


# ---- the kernels' forms ----------------------------------------------------------------------------------------------
def summaries_sorted(x, y, q):
  """-> dict(mean (G,), quantiles (n_q, G), crps (G,), pit (2, G)) the way k_sample_summaries forms them."""
  S, G = x.shape
  xs = np.sort(x, axis=0)
  bad = np.isnan(x).any(axis=0)
  out = {'mean': xs.sum(axis=0) / S}
  quant = np.empty((len(q), G))
  for k, level in enumerate(q):
    h = (S - 1) * float(level)
    lo = int(math.floor(h))
    f = h - lo
    if lo >= S - 1:
      lo, f = S - 1, 0.0
    quant[k] = xs[lo] if f == 0.0 else xs[lo] + f * (xs[lo + 1] - xs[lo])
  out['quantiles'] = quant
  if y is not None:
    have = np.isfinite(y)
    d = xs - np.where(have, y, 0.0)[None, :]
    coef = 2.0 * np.arange(1, S + 1) - S - 1.0
    crps = np.abs(d).sum(axis=0) / S - (coef[:, None] * d).sum(axis=0) / (float(S) * S)
    pit = np.stack([(xs <= y[None, :]).sum(axis=0), (xs < y[None, :]).sum(axis=0)]).astype(np.float64) / float(S)
    crps[~have | bad] = np.nan
    pit[:, ~have | bad] = np.nan
    out['crps'], out['pit'] = crps, pit
  out['mean'][bad] = np.nan
  out['quantiles'][:, bad] = np.nan
  return out


def energy_upper(x, y):
  keep = np.isfinite(y)
  if not keep.any():
    return float('nan')
  X, yk = x[:, keep], y[keep]
  S = X.shape[0]
  norm = lambda d: np.sqrt(np.sum(d * d, axis=1))
  t1 = norm(X - yk[None, :]).sum()
  pairs = sum(float(norm(X[s + 1:] - X[s][None, :]).sum()) for s in range(S - 1))
  return t1 / S - pairs / (float(S) * S)


# ---- bars and errors ---------------------------------------------------------------------------------------------------
def quantile_bars(x, q):
  """(n_q, G): 4 eps max(|x_(lo)|, |x_(lo+1)|); 0 where the neighbours are equal or (S - 1) q is an integer."""
  S, G = x.shape
  xs = np.sort(x, axis=0)
  bars = np.empty((len(q), G))
  for k, level in enumerate(q):
    h = (S - 1) * float(level)
    lo = min(int(math.floor(h)), S - 1)
    hi = min(lo + 1, S - 1)
    bars[k] = 4.0 * EPS * np.maximum(np.abs(xs[lo]), np.abs(xs[hi]))
    if h == lo:
      bars[k] = 0.0
    bars[k][xs[lo] == xs[hi]] = 0.0
  return bars


def mean_bars(x):
  return x.shape[0] * EPS * np.abs(x).max(axis=0)


def crps_bars(x, y):
  return x.shape[0] * EPS * np.abs(x - y[None, :]).max(axis=0)


def energy_bar(S, G, t1, t2):
  return (G + 2 * S + 64) * EPS * (t1 + t2)


def check_summaries(tag, got, x, y, q, ref):
  """Asserts `got` (dict of numpy arrays) against the brute-force `ref` of (x, y, q) at the bars above; prints and returns
  the worst error / bar ratio of each quantity (pit: the number of cells that differ)."""
  scored = np.isfinite(y) & ~np.isnan(x).any(axis=0) if y is not None else np.zeros(x.shape[1], dtype=bool)
  clean = ~np.isnan(x).any(axis=0)
  worst = {}

  def ratio(name, err, bar, ok):
    err, bar = err[..., ok], bar[..., ok]
    assert not np.isnan(err).any(), (tag, name, 'NaN where a value is due')
    over = err > bar
    assert not over.any(), (tag, name, float(err[over].max()), float(bar[over].min()))
    worst[name] = float(np.max(err / np.where(bar > 0, bar, np.inf), initial=0.0))

  assert np.isnan(got['mean'][~clean]).all() and np.isnan(got['quantiles'][:, ~clean]).all(), (tag, 'NaN columns')
  ratio('mean', np.abs(got['mean'] - ref['mean']), mean_bars(x), clean)
  ratio('quantiles', np.abs(got['quantiles'] - ref['quantiles']), quantile_bars(x, q), clean)
  if y is not None:
    assert np.isnan(got['crps'][~scored]).all() and np.isnan(got['pit'][:, ~scored]).all(), (tag, 'NaN pattern')
    ratio('crps', np.abs(got['crps'] - ref['crps']), crps_bars(x, np.where(np.isfinite(y), y, 0.0)), scored)
    differ = int((got['pit'][:, scored] != ref['pit'][:, scored]).sum())
    assert differ == 0, (tag, 'pit', differ)
    worst['pit'] = 0.0
  print(f'{tag}: error / bar ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
  return worst


# ---- the shared cases (computed once, read-only) ---------------------------------------------------------------------
def _frozen(*arrays):
  for a in arrays:
    if a is not None:
      a.setflags(write=False)
  return arrays


def make_y(x, rng):
  """One observed value per column, by column index mod 5: a tied sample value, below every sample, above every sample,
  NaN, between the samples."""
  S, G = x.shape
  y = np.empty(G)
  for c in range(G):
    kind = c % 5
    col = x[:, c]
    y[c] = (col[S // 2], col.min() - 1.5, col.max() + 2.5, np.nan, float(np.median(col)) + 0.3)[kind]
  return y


def make_x(S, G, kind, rng):
  if kind == 'normal':                    # mixed sign, a location and a spread per column
    return rng.standard_normal((S, G)) * rng.uniform(0.1, 30.0, G)[None, :] + rng.uniform(-20.0, 20.0, G)[None, :]
  if kind == 'count':                     # integer totals with heavy ties
    return rng.poisson(rng.uniform(0.3, 6.0, G)[None, :], (S, G)).astype(np.float64)
  if kind == 'big':                       # a total of 1e9 with a spread of 10
    return 1e9 + rng.integers(-10, 11, (S, G)).astype(np.float64)
  raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def summary_case(S, G, kind):
  """-> (x (S, G), y (G,), reference dict) for the levels LEVELS."""
  rng = np.random.default_rng([S, G, KINDS.index(kind) if kind in KINDS else 7])
  x = make_x(S, G, kind, rng)
  y = make_y(x, rng)
  ref = dict(mean=np.asarray([math.fsum(x[:, c].tolist()) for c in range(G)]) / S, quantiles=quantiles_ref(x, LEVELS),
             crps=crps_ref(x, y), pit=pit_ref(x, y))
  _frozen(x, y, *ref.values())
  return x, y, ref


@functools.lru_cache(maxsize=None)
def energy_case(S, G):
  """-> (x (S, G), y (G,) all finite, (score, T1, T2))."""
  rng = np.random.default_rng([S, G, 11])
  x = make_x(S, G, 'normal', rng)
  y = x[rng.integers(0, S)] + rng.standard_normal(G)
  _frozen(x, y)
  return x, y, energy_ref(x, y)
