"""Covariance, variogram and variogram score of an ensemble of sample paths (bayesnf_amd/csrc/bnf_dependence.h, include/bnf.h
bnf_sample_pair_moments) on the host.  x (S, G): S sample paths of G totals; y (G,): the observed totals; p in {0.5, 1, 2}.

  brute force, straight from the definitions
    `mean_ref`     (1 / S) fsum_s x_sc
    `cov_ref`      (1 / S) fsum_s (x_si - m_i) (x_sj - m_j), centred in np.longdouble (64-bit significand: the centring
                   and the products of the reference are exact to 2^-63); also A_ij = (1 / S) fsum_s |(x_si - m_i)(x_sj - m_j)|
    `vario_ref`    (1 / S) fsum_s |x_si - x_sj|^p, the differences in np.longdouble
    `score_ref`    fsum over the pairs i < j with y_i, y_j finite of w_ij (|y_i - y_j|^p - vario_ij)^2, taken from a given
                   variogram (the reference's own, to score the reference)
    (math.fsum over the S terms of every cell and over the pair sum: each term is rounded to float64 once, the sum is exact)
  the kernel's form, restated in numpy
    `means_kernel_form`         8 strided sequential partial sums per column, added in order
    `pair_moments_kernel_form`  means first, then per 64 x 64 tile on or above the diagonal a sequential float64 sum over the
                                paths in chunks of 32, cells i <= j mirrored, one partial score per tile

Bars (each from float64 rounding, eps = 2^-52; the issue that introduced the feature states and derives them):
  mean             S eps max|x_c|
  variogram cell   (S + 8) eps ref cell: S non-negative terms, each within 2 eps, summed in any fixed order
  covariance cell  (S + 8) eps A_ij + (S eps)^2 max|x_i| max|x_j|: the summation error, and delta_i delta_j, the only effect of
                   the rounding of the means (the cross terms vanish: the centred values sum to 0)
  variogram score  sum_pairs w_ij (2 |e_ij| b_ij + b_ij^2) + (n_pairs + 8) eps ref score, e_ij the reference difference,
                   b_ij = (S + 8) eps vario_ij + 2 eps |y_i - y_j|^p
  correlation      host arithmetic on the device covariance: compared with the same formula on the reference covariance,
                   at the bar propagated from the covariance bars, `correlation_bars`
"""
import functools
import math

import numpy as np

EPS = 2.0 ** -52
TILE, CHUNK = 64, 32                  # BNF_PAIR_COL_TILE, BNF_PAIR_PATH_CHUNK
ORDERS = (0.5, 1.0, 2.0)
KINDS = ('normal', 'count')
HOST_S = (1, 2, 33, 1000)
HOST_G = (2, 9)
GRID_S = (1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 1000)
GRID_G = (1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 2)
GRID_S_AT_LARGEST_G = (2, CHUNK + 1)      # the fsum reference of 130 x 130 cells at S = 1000 takes seconds


def _ld(a):
  return np.asarray(a, dtype=np.longdouble)


def _fsum_columns(terms):
  """terms (S, n) float64 -> (n,) the exact sums of the columns, rounded once."""
  return np.asarray([math.fsum(col) for col in np.ascontiguousarray(terms.T).tolist()], dtype=np.float64)


def term(d, p):
  """|d|^p in the three compiled forms; d in any float type, the result in the same."""
  a = np.abs(d)
  if p == 0.5:
    return np.sqrt(a)
  if p == 1.0:
    return a
  if p == 2.0:
    return a * a
  raise ValueError(p)


# ---- brute force ---------------------------------------------------------------------------------------------------
def mean_ref(x):
  return _fsum_columns(np.asarray(x, dtype=np.float64)) / x.shape[0]


def cov_ref(x):
  """-> (cov (G, G), A (G, G))."""
  S, G = x.shape
  xl = _ld(x)
  xc = xl - xl.sum(axis=0) / S
  cov, A = np.empty((G, G)), np.empty((G, G))
  for i in range(G):
    prod = xc[:, i:i + 1] * xc[:, i:]
    cov[i, i:] = _fsum_columns(prod.astype(np.float64)) / S
    A[i, i:] = _fsum_columns(np.abs(prod).astype(np.float64)) / S
    cov[i:, i], A[i:, i] = cov[i, i:], A[i, i:]
  return cov, A


def vario_ref(x, p):
  S, G = x.shape
  xl = _ld(x)
  out = np.empty((G, G))
  for i in range(G):
    out[i, i:] = _fsum_columns(term(xl[:, i:i + 1] - xl[:, i:], p).astype(np.float64)) / S
    out[i:, i] = out[i, i:]
  return out


def scored_pairs(y):
  """-> (I, J): the pairs i < j with y_i and y_j finite."""
  idx = np.flatnonzero(np.isfinite(y))
  i, j = np.triu_indices(len(idx), 1)
  return idx[i], idx[j]


def score_ref(vario, y, p, w=None):
  """-> (score, e (n_pairs,), weights (n_pairs,)) from the variogram `vario`; score NaN with fewer than two finite y."""
  I, J = scored_pairs(y)
  if np.isfinite(y).sum() < 2:
    return float('nan'), np.zeros(0), np.zeros(0)
  e = term(_ld(y[I]) - _ld(y[J]), p) - _ld(vario[I, J])
  wt = np.ones(len(I)) if w is None else np.asarray(w, dtype=np.float64)[I, J]
  return math.fsum((_ld(wt) * e * e).astype(np.float64).tolist()), e.astype(np.float64), wt


# ---- the kernel's form ---------------------------------------------------------------------------------------------------
def _seq_sum(acc, terms):
  """acc + terms[0] + terms[1] + ... one after the other in float64 (np.cumsum accumulates sequentially)."""
  return np.cumsum(np.concatenate([acc[None], terms], axis=0), axis=0)[-1]


def means_kernel_form(x):
  S, G = x.shape
  t = np.zeros(G)
  for r in range(8):
    t = t + _seq_sum(np.zeros(G), x[r::8])
  return t / S


def pair_moments_kernel_form(x, p, y=None, w=None):
  """-> dict(mean, covariance, variogram[, variogram_score])."""
  S, G = x.shape
  mean = means_kernel_form(x)
  cov, vario = np.empty((G, G)), np.empty((G, G))
  nT = -(-G // TILE)
  partials = []
  for ti in range(nT):
    for tj in range(ti, nT):
      a, b = slice(ti * TILE, min(G, (ti + 1) * TILE)), slice(tj * TILE, min(G, (tj + 1) * TILE))
      na, nb = a.stop - a.start, b.stop - b.start
      accc, accv = np.zeros((na, nb)), np.zeros((na, nb))
      for s0 in range(0, S, CHUNK):
        xa, xb = x[s0:s0 + CHUNK, a], x[s0:s0 + CHUNK, b]
        accc = _seq_sum(accc, (xa - mean[a])[:, :, None] * (xb - mean[b])[:, None, :])
        accv = _seq_sum(accv, term(xa[:, :, None] - xb[:, None, :], p))
      ci, cj = np.meshgrid(np.arange(a.start, a.stop), np.arange(b.start, b.stop), indexing='ij')
      keep = ci <= cj
      for out, acc in ((cov, accc), (vario, accv)):
        out[ci[keep], cj[keep]] = acc[keep] / S
        out[cj[keep], ci[keep]] = acc[keep] / S
      if y is not None:
        scored = (ci < cj) & np.isfinite(y)[ci] & np.isfinite(y)[cj]
        e = term(y[ci[scored]] - y[cj[scored]], p) - accv[scored] / S
        wt = 1.0 if w is None else w[ci[scored], cj[scored]]
        partials.append(float(np.sum(wt * (e * e))))
  out = dict(mean=mean, covariance=cov, variogram=vario)
  if y is not None:
    out['variogram_score'] = float(np.sum(partials)) if np.isfinite(y).sum() >= 2 else float('nan')
  return out


# ---- bars ------------------------------------------------------------------------------------------------------------
def mean_bars(x):
  return x.shape[0] * EPS * np.abs(x).max(axis=0)


def vario_bars(S, ref_vario):
  return (S + 8) * EPS * ref_vario


def cov_bars(x, A):
  S = x.shape[0]
  big = np.abs(x).max(axis=0)
  return (S + 8) * EPS * A + (S * EPS) ** 2 * big[:, None] * big[None, :]


def score_bar(S, ref_vario, y, p, ref_score, e, wt):
  I, J = scored_pairs(y)
  b = (S + 8) * EPS * ref_vario[I, J] + 2 * EPS * term(y[I] - y[J], p)
  return float(np.sum(wt * (2 * np.abs(e) * b + b * b)) + (len(I) + 8) * EPS * ref_score)


def correlation(cov):
  """cov_ij / (std_i std_j), NaN in the row and column of a column whose std is not > 0: the estimators' formula."""
  std = np.sqrt(np.diagonal(cov))
  flat = ~(std > 0)
  with np.errstate(divide='ignore', invalid='ignore'):
    corr = cov / (std[:, None] * std[None, :])
  corr[flat, :] = np.nan
  corr[:, flat] = np.nan
  return corr


def correlation_bars(ref_cov, bars):
  """First-order propagation of the covariance bars through r = c_ij / sqrt(c_ii c_jj):
  |dr| <= bar_ij / (s_i s_j) + |r| (bar_ii / (2 c_ii) + bar_jj / (2 c_jj)), doubled for the second-order terms, plus the
  4 eps of the formula's own roundings (a square root each, a product, a quotient)."""
  var = np.diagonal(ref_cov)
  with np.errstate(divide='ignore', invalid='ignore'):
    std = np.sqrt(var)
    r = np.abs(ref_cov) / (std[:, None] * std[None, :])
    rel = np.diagonal(bars) / (2 * var)
    return 2 * (bars / (std[:, None] * std[None, :]) + r * (rel[:, None] + rel[None, :])) + 4 * EPS * r


def check_moments(tag, got, x, y, p, ref, w=None, ref_score=None):
  """Asserts `got` (dict of numpy arrays / floats, keys as Engine.sample_pair_moments returns them) against the
  brute-force `ref` of `dependence_case` at the bars above; x must hold no NaN.  Prints and returns the worst error / bar
  of every quantity present.  ref_score: (score, e, wt) for weights other than the case's own (w)."""
  S = x.shape[0]
  worst = {}

  def ratio(name, err, bar):
    err, bar = np.atleast_1d(err), np.atleast_1d(bar)
    assert not np.isnan(err).any(), (tag, name, 'NaN where a value is due')
    over = err > bar
    assert not over.any(), (tag, name, float(err[over].max()), float(bar[over].min()))
    worst[name] = float(np.max(err / np.where(bar > 0, bar, np.inf), initial=0.0))

  ratio('mean', np.abs(got['mean'] - ref['mean']), mean_bars(x))
  if 'covariance' in got:
    ratio('covariance', np.abs(got['covariance'] - ref['cov']), cov_bars(x, ref['A']))
  if 'variogram' in got:
    ratio('variogram', np.abs(got['variogram'] - ref['vario'][p]), vario_bars(S, ref['vario'][p]))
  if 'variogram_score' in got:
    score, e, wt = ref_score if ref_score is not None else ref['score'][p]
    if np.isnan(score):
      assert np.isnan(got['variogram_score']), (tag, 'score', got['variogram_score'])
    else:
      ratio('score', abs(got['variogram_score'] - score), score_bar(S, ref['vario'][p], y, p, score, e, wt))
  print(f'{tag}: error / bar ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
  return worst


# ---- the shared cases (computed once, read-only) ---------------------------------------------------------------------
def _frozen(*arrays):
  for a in arrays:
    if isinstance(a, np.ndarray):
      a.setflags(write=False)


def make_x(S, G, kind, rng):
  if kind == 'normal':                    # mixed sign, a location and a spread per column, a factor shared by a path
    f = rng.standard_normal((S, 1)) * rng.uniform(0.0, 20.0, G)[None, :]
    return f + rng.standard_normal((S, G)) * rng.uniform(0.1, 30.0, G)[None, :] + rng.uniform(-20.0, 20.0, G)[None, :]
  if kind == 'count':                     # integer totals with heavy ties
    return rng.poisson(rng.uniform(0.3, 6.0, G)[None, :], (S, G)).astype(np.float64)
  if kind == 'big':                       # a total of 1e9 with a spread of 10
    return 1e9 + rng.integers(-10, 11, (S, G)).astype(np.float64)
  raise ValueError(kind)


def make_y(x, kind, rng):
  """One more path of the same kind; NaN in the columns c = 3 (mod 5)."""
  S, G = x.shape
  y = x[rng.integers(0, S)] + (rng.standard_normal(G) if kind == 'normal' else rng.integers(-2, 3, G).astype(np.float64))
  y[3::5] = np.nan
  return y


@functools.lru_cache(maxsize=None)
def dependence_case(S, G, kind):
  """-> (x (S, G), y (G,), ref) with ref = dict(mean, cov, A, vario {p: (G, G)}, score {p: (score, e, wt)})."""
  rng = np.random.default_rng([S, G, ('normal', 'count', 'big').index(kind), 23])
  x = make_x(S, G, kind, rng)
  y = make_y(x, kind, rng)
  return (x, y, reference(x, y))


def reference(x, y):
  cov, A = cov_ref(x)
  vario = {p: vario_ref(x, p) for p in ORDERS}
  ref = dict(mean=mean_ref(x), cov=cov, A=A, vario=vario,
             score={p: score_ref(vario[p], y, p) for p in ORDERS} if y is not None else {})
  _frozen(x, y, ref['mean'], cov, A, *vario.values())
  return ref


def shared_factor_case(seed=0, S=400, G=12):
  """x = 100 + f_s + e_sc with f ~ N(0, 10^2) shared by the columns of a path and e ~ N(0, 1); y one more draw of the same
  law; and x with every column independently permuted over the paths: the same marginals, no dependence.
  -> (x, shuffled, y)"""
  rng = np.random.default_rng(seed)
  x = 100.0 + 10.0 * rng.standard_normal((S, 1)) + rng.standard_normal((S, G))
  y = 100.0 + 10.0 * rng.standard_normal() + rng.standard_normal(G)
  shuffled = np.stack([rng.permutation(x[:, c]) for c in range(G)], axis=1)
  return x, shuffled, y
