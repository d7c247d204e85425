"""Bounds and exact laws the predictive sampler (bayesnf_amd/csrc/bnf_sampling.h) is held to.  Host, float64, scipy.

Every bar is one of the formulas below at the N actually drawn and alpha = 1e-9; none is tuned.

  dkw_eps           sup |F_n - F| of n i.i.d. draws of ANY law exceeds it with probability <= alpha (Dvoretzky-Kiefer-
                    Wolfowitz with Massart's constant); the supremum over a subset of thresholds is no larger
  tail_count_bound  Bernstein: a Binomial(n, p) count leaves n p +- t with probability <= alpha
  chi2_bounds       the two-sided alpha interval of a chi-square variable
  lag_corr_bound    the two-sided alpha interval of sqrt(n) r, r a sample correlation of two independent sequences
                    (asymptotically N(0, 1 / n); n >= 32,768 wherever it is used)

Laws: `NormalLaw`, `CountLaw` (NB, ZINB with pi > 0) in the sampler's parametrisation, total_count = 1 / aux[1],
logits = -log aux[1] - log softplus(loc), evaluated in float64 on the float32 inputs; `law.total(n)` is the exact law
of the sum of n independent rows of one member."""
import math

import numpy as np
from scipy import special, stats

ALPHA = 1e-9
TAIL_LEVELS = (1e-2, 1e-3, 1e-4)
MAX_THRESHOLDS = 4096


def dkw_eps(n, alpha=ALPHA):
  return math.sqrt(math.log(2.0 / alpha) / (2.0 * n))


def tail_count_bound(n, p, alpha=ALPHA):
  """The smallest t with 2 exp(-t^2 / (2 (n p (1 - p) + t / 3))) <= alpha: the positive root of
  t^2 - (2 L / 3) t - 2 L n p (1 - p) = 0, L = ln(2 / alpha)."""
  L = math.log(2.0 / alpha)
  v = n * p * (1.0 - p)
  return L / 3.0 + math.sqrt(L * L / 9.0 + 2.0 * L * v)


def chi2_bounds(dof, alpha=ALPHA):
  return float(stats.chi2.ppf(alpha / 2.0, dof)), float(stats.chi2.isf(alpha / 2.0, dof))


def lag_corr_bound(n, alpha=ALPHA):
  return float(stats.norm.isf(alpha / 2.0)) / math.sqrt(n)


def softplus(x):
  return np.logaddexp(np.asarray(x, dtype=np.float64), 0.0)


def central_from_raw(m1, m2, m3, m4):
  """(mean, variance, fourth central moment) from the raw moments E x .. E x^4."""
  return m1, m2 - m1 * m1, m4 - 4.0 * m1 * m3 + 6.0 * m1 * m1 * m2 - 3.0 * m1 ** 4


def raw_from_cumulants(k1, k2, k3, k4):
  return (k1, k2 + k1 * k1, k3 + 3.0 * k2 * k1 + k1 ** 3,
          k4 + 4.0 * k3 * k1 + 3.0 * k2 * k2 + 6.0 * k2 * k1 * k1 + k1 ** 4)


def cumulants_from_raw(m1, m2, m3, m4):
  k2 = m2 - m1 * m1
  k3 = m3 - 3.0 * m1 * m2 + 2.0 * m1 ** 3
  mu4 = m4 - 4.0 * m1 * m3 + 6.0 * m1 * m1 * m2 - 3.0 * m1 ** 4
  return m1, k2, k3, mu4 - 3.0 * k2 * k2


class Law:
  """What every law offers beside cdf / cdf_left / sf / ppf: its first four cumulants."""

  def raw_moments(self):
    return raw_from_cumulants(*self.cumulants())

  def moments(self):
    """(mean, variance, fourth central moment)."""
    k1, k2, _, k4 = self.cumulants()
    return k1, k2, k4 + 3.0 * k2 * k2


class NormalLaw(Law):
  discrete = False

  def __init__(self, mu, sigma):
    self.mu, self.sigma = float(mu), float(sigma)

  def cdf(self, x):
    return special.ndtr((np.asarray(x, dtype=np.float64) - self.mu) / self.sigma)

  cdf_left = cdf

  def sf(self, x):
    return special.ndtr(-(np.asarray(x, dtype=np.float64) - self.mu) / self.sigma)

  def ppf(self, q):
    return self.mu + self.sigma * special.ndtri(np.asarray(q, dtype=np.float64))

  def cumulants(self):
    return self.mu, self.sigma ** 2, 0.0, 0.0

  def total(self, n):
    return NormalLaw(n * self.mu, math.sqrt(n) * self.sigma)


class CountLaw(Law):
  """NB(total_count tc, logits), with probability pi replaced by 0 (pi = 0: the plain NB).  scipy's nbinom(n, p) with
  n = tc, p = sigmoid(-logits) = 1 / (1 + e^logits): mean tc e^logits."""
  discrete = True

  def __init__(self, tc, logits, pi=0.0):
    self.tc, self.logits, self.pi = float(tc), float(logits), float(pi)
    self.p = float(special.expit(-self.logits))
    self.nb = stats.nbinom(self.tc, self.p)

  @classmethod
  def from_inputs(cls, loc, aux1, pi=0.0):
    """The law of the kernel's float32 inputs: loc the network output, aux1 = 1 / total_count, pi = aux[2]."""
    a1 = float(np.float32(aux1))
    return cls(1.0 / a1, -math.log(a1) - math.log(float(softplus(np.float32(loc)))), float(np.float32(pi)))

  def cdf(self, k):
    k = np.asarray(k, dtype=np.float64)
    return np.where(k < 0, 0.0, self.pi + (1.0 - self.pi) * self.nb.cdf(np.maximum(k, 0.0)))

  def cdf_left(self, k):
    return self.cdf(np.asarray(k, dtype=np.float64) - 1.0)

  def sf(self, k):
    k = np.asarray(k, dtype=np.float64)
    return np.where(k < 0, 1.0, (1.0 - self.pi) * self.nb.sf(np.maximum(k, 0.0)))

  def ppf(self, q):
    q = np.asarray(q, dtype=np.float64)
    inner = np.clip((q - self.pi) / (1.0 - self.pi), 0.0, 1.0)
    return np.where(q <= self.pi, 0.0, self.nb.ppf(inner))

  def nb_cumulants(self):
    m = self.tc * math.exp(self.logits)
    P = m / self.tc
    v = m * (1.0 + P)
    return m, v, v * (1.0 + 2.0 * P), v * (1.0 + 6.0 * P * (1.0 + P))

  def cumulants(self):
    """NB: mean tc e^logits, variance mean (1 + mean / tc), ...; with pi the raw moments are (1 - pi) times the NB's
    (the two-point mixture with the mass at 0)."""
    if self.pi == 0.0:
      return self.nb_cumulants()
    return cumulants_from_raw(*((1.0 - self.pi) * r for r in raw_from_cumulants(*self.nb_cumulants())))

  def moments_from_pmf(self, mass=1e-18):
    """The same three numbers summed from the pmf (the check of the closed forms; small supports only)."""
    hi = int(self.nb.isf(mass)) + 1
    k = np.arange(hi + 1, dtype=np.float64)
    w = (1.0 - self.pi) * self.nb.pmf(k)
    w[0] += self.pi
    mean = float((w * k).sum())
    return mean, float((w * (k - mean) ** 2).sum()), float((w * (k - mean) ** 4).sum())

  def total(self, n):
    if self.pi == 0.0:
      return CountLaw(n * self.tc, self.logits)       # equal p: the sum of independent NB is NB
    return ZinbTotalLaw(self, n)


class ZinbTotalLaw(Law):
  """Sum of n independent ZINB rows: the number K of rows that are not replaced is Binomial(n, 1 - pi), and given K = k
  the total is NB(k tc, logits).  The sum over k runs over the K of binomial mass >= 1 - 2e-12 (an error of 2e-12 in
  every CDF value)."""
  discrete = True

  def __init__(self, row, n):
    self.row, self.n = row, int(n)
    b = stats.binom(self.n, 1.0 - row.pi)
    lo, hi = int(b.ppf(1e-12)), int(b.isf(1e-12))
    self.k = np.arange(lo, hi + 1, dtype=np.float64)
    self.w = b.pmf(self.k)

  def cdf(self, x):
    """sum_k w_k betainc(k tc, x + 1, p): the NB CDF as the oracle writes it; K = 0 is the mass at 0."""
    x = np.asarray(x, dtype=np.float64)
    xs = np.maximum(x.reshape(-1), 0.0)
    pos = self.k > 0
    f = self.w[pos] @ special.betainc(self.k[pos, None] * self.row.tc, xs[None, :] + 1.0, self.row.p)
    f = f + self.w[~pos].sum()
    return np.where(x < 0, 0.0, f.reshape(x.shape))

  def cdf_left(self, x):
    return self.cdf(np.asarray(x, dtype=np.float64) - 1.0)

  def ppf(self, q):
    """The smallest integer with cdf >= q: a grid of 257 points over mean +- sd / sqrt(min(q, 1 - q)) (Chebyshev: the
    quantile lies inside), then bisection on the integers between two grid points (cdf is nondecreasing)."""
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    m, v, _ = self.moments()
    w = math.sqrt(v / float(np.minimum(q, 1.0 - q).min())) + 1.0
    grid = np.unique(np.floor(np.linspace(max(-1.0, m - w - 1.0), m + w + 1.0, 257)))
    f = self.cdf(grid)
    at = np.searchsorted(f, q, side='left')               # the first grid point with cdf >= q
    assert at.min() >= 1 and at.max() < len(grid)
    lo, hi = grid[at - 1], grid[at]
    while np.any(hi - lo > 1):
      mid = np.floor((lo + hi) / 2)
      ok = self.cdf(mid) >= q
      hi, lo = np.where(ok, mid, hi), np.where(ok, lo, mid)
    return hi

  def cumulants(self):
    """Cumulants of independent rows add."""
    return tuple(self.n * k for k in self.row.cumulants())


def mixture_moments(laws):
  """(mean, variance, fourth central moment) of the equal-weight mixture of `laws`: raw moments average."""
  return central_from_raw(*np.mean(np.asarray([law.raw_moments() for law in laws], dtype=np.float64), axis=0))


def thresholds(law, n_max=MAX_THRESHOLDS):
  """At most n_max thresholds, chosen from the law and not from the sample: its k / n_max quantiles, distinct."""
  q = np.arange(1, n_max) / n_max
  return np.unique(np.asarray(law.ppf(q), dtype=np.float64))


def dkw_distance(n, thr, cnt_le, cnt_lt, law):
  """max over the thresholds of |F_n(t) - F(t)| and |F_n(t-) - F(t-)| from the counts #{x <= t} and #{x < t}."""
  d_le = np.abs(np.asarray(cnt_le, dtype=np.float64) / n - law.cdf(thr))
  d_lt = np.abs(np.asarray(cnt_lt, dtype=np.float64) / n - law.cdf_left(thr))
  return float(max(d_le.max(), d_lt.max()))


def tail_points(law, lower=False):
  """[(level, threshold t, exact mass beyond t)]: t the law's 1 - level quantile (an integer for counts) and the mass
  P(x > t); lower=True: t the level quantile and the mass P(x < t) (continuous laws)."""
  out = []
  for lv in TAIL_LEVELS:
    if lower:
      t = float(law.ppf(lv))
      out.append((lv, t, float(law.cdf(t))))
    else:
      t = float(law.ppf(1.0 - lv))
      out.append((lv, t, float(law.sf(t))))
  return out


def moment_bars(law, n, k_sd=6.0):
  """(mean, bar of the sample mean, variance, bar of the sample variance): k_sd standard errors, the variance's from
  the fourth central moment."""
  m, v, mu4 = law.moments()
  return m, k_sd * math.sqrt(v / n), v, k_sd * math.sqrt(max(mu4 - v * v, 0.0) / n)


def summarise_numpy(x, law, thr=None, with_tails=True):
  """The summaries the GPU tests bring to the host, computed with numpy from draws x: dict(n, D, tails [(level, count,
  expected, bound)], mean, var)."""
  x = np.sort(np.asarray(x, dtype=np.float64).ravel())
  n = x.size
  thr = thresholds(law) if thr is None else thr
  le, lt = np.searchsorted(x, thr, side='right'), np.searchsorted(x, thr, side='left')
  out = dict(n=n, D=dkw_distance(n, thr, le, lt, law), mean=float(x.mean()), var=float(x.var(ddof=1)), tails=[])
  if not with_tails:
    return out
  for lv, t, mass in tail_points(law):
    out['tails'].append((lv, int(n - np.searchsorted(x, t, side='right')), n * mass, tail_count_bound(n, mass)))
  if law.discrete:                       # the mass at 0, held as a count
    p0 = float(law.cdf(0.0))
    out['tails'].append((0.0, int(np.searchsorted(x, 0.0, side='right')), n * p0, tail_count_bound(n, p0)))
  else:
    for lv, t, mass in tail_points(law, lower=True):
      out['tails'].append((-lv, int(np.searchsorted(x, t, side='left')), n * mass, tail_count_bound(n, mass)))
  return out


def check_summary(sm, law, label=''):
  """The checks of the pooled law on such a summary -> list of the names of those that fail (empty: all pass)."""
  failed = []
  if sm['D'] > dkw_eps(sm['n']):
    failed.append('dkw')
  for lv, cnt, want, bound in sm['tails']:
    if abs(cnt - want) > bound:
      failed.append(f'tail{lv:g}')
  m, mbar, v, vbar = moment_bars(law, sm['n'])
  if abs(sm['mean'] - m) > mbar:
    failed.append('mean')
  if abs(sm['var'] - v) > vbar:
    failed.append('var')
  return failed


def describe(sm, law, label):
  """One line per case: every figure over its bar."""
  m, mbar, v, vbar = moment_bars(law, sm['n'])
  tails = ' '.join(f'{lv:g}:{abs(c - w):.0f}/{b:.0f}' for lv, c, w, b in sm['tails'])
  return (f'{label}: N={sm["n"]} D={sm["D"]:.5f}/EPS={dkw_eps(sm["n"]):.5f} tails |count - N p|/bound {tails} '
          f'|mean err|={abs(sm["mean"] - m):.4g}/{mbar:.4g} |var err|={abs(sm["var"] - v):.4g}/{vbar:.4g}')
