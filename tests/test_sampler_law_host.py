"""The bounds of tests/sampler_law_ref.py have teeth, and the truth stays inside them (CPU, numpy's own Generator).

At the N of tests/test_gpu_sampler_law.py: numpy's samplers (normal, poisson(gamma)) pass every kind of check made on
the GPU sampler, and each of five wrong samplers fails the check aimed at it.  The closed forms are held to the
project's oracle and to sums over the pmf."""
import math

import numpy as np
import pytest
from scipy import stats

from oracle import bnf_oracle as O
from tests import sampler_law_ref as L

N_POOL = 4096 * 1024
S_TOT = 32768
STRIDE = 356                  # what group_sums_sample_stride gives for the 46,660 rows of the GPU test


def _nb(rng, tc, mean, size, pi=0.0, tc_factor=1.0, rate_shift=None):
  """numpy's NB as the kernel builds it: Poisson(Gamma(shape tc, scale mean / tc)), then the zero inflation."""
  lam = rng.gamma(tc * tc_factor, mean / (tc * tc_factor), size)
  if rate_shift is not None:
    lam = np.where(lam >= 10.0, lam + rate_shift, lam)
  x = rng.poisson(lam).astype(np.float64)
  if pi > 0:
    x[rng.random(size) < pi] = 0.0
  return x


def _law(tc, mean, pi=0.0):
  return L.CountLaw(tc, math.log(mean / tc), pi)


def test_bounds_are_the_formulas():
  assert abs(L.dkw_eps(32768) - 0.0181) < 5e-5 and abs(L.dkw_eps(N_POOL) - 0.0016) < 5e-5
  for n, p in ((N_POOL, 1e-4), (N_POOL, 0.3), (1000, 0.5)):
    t = L.tail_count_bound(n, p)
    f = lambda t: 2.0 * math.exp(-t * t / (2.0 * (n * p * (1 - p) + t / 3.0)))
    assert f(t) <= L.ALPHA * (1 + 1e-9) and f(t * (1 - 1e-6)) > L.ALPHA
  lo, hi = L.chi2_bounds(S_TOT - 1)
  assert abs(stats.chi2.cdf(lo, S_TOT - 1) - L.ALPHA / 2) < 1e-12 and abs(stats.chi2.sf(hi, S_TOT - 1) - L.ALPHA / 2) < 1e-12
  assert abs(L.lag_corr_bound(S_TOT) * math.sqrt(S_TOT) - stats.norm.isf(L.ALPHA / 2)) < 1e-12


@pytest.mark.parametrize('tc,mean,pi', [(0.05, 5.0, 0.0), (3.0, 8.0, 0.35), (1.0, 30.0, 1e-3), (40.0, 2.0, 0.999)])
def test_closed_forms_against_the_oracle_and_the_pmf(tc, mean, pi):
  """CountLaw's CDF is the oracle's count_cdf; its mean, variance and fourth central moment are the sums over the pmf;
  the total of n rows has the law of the n-fold convolution."""
  law = _law(tc, mean, pi)
  k = np.arange(0.0, 200.0)
  fc = dict(tc=np.asarray([[tc]]), logits=np.full((1, len(k)), law.logits), pi=np.asarray([[pi]]) if pi > 0 else None)
  np.testing.assert_allclose(law.cdf(k), O.count_cdf(fc, k[None, :])[0], rtol=1e-12, atol=1e-15)
  np.testing.assert_allclose(law.sf(k) + law.cdf(k), 1.0, atol=1e-12)
  np.testing.assert_allclose(law.moments(), law.moments_from_pmf(), rtol=1e-7)
  kk = np.arange(0.0, 4000.0)
  pm = np.diff(np.concatenate([[0.0], law.cdf(kk)]))
  conv = np.convolve(np.convolve(pm, pm), pm)[:len(kk)]
  np.testing.assert_allclose(law.total(3).cdf(kk[:300]), np.cumsum(conv)[:300], atol=1e-9)
  q = np.asarray([0.01, 0.5, 0.99, 0.9999])
  t = law.total(3).ppf(q)
  assert np.all(law.total(3).cdf(t) >= q) and np.all(law.total(3).cdf(t - 1.0) < q)
  m, v, mu4 = law.total(3).moments()
  np.testing.assert_allclose([m, v], [(conv * kk).sum(), (conv * (kk - m) ** 2).sum()], rtol=1e-6)
  assert abs((conv * (kk - m) ** 4).sum() / mu4 - 1.0) < 1e-5


POOLED_TRUTH = [('NB', 0.05, 1e6, 0.0), ('NB', 1e6, 10.01, 0.0), ('NB', 1.0, 30.0, 0.0), ('ZINB', 3.0, 8.0, 0.35),
                ('NORMAL', 0.5, 0.01, 0.0)]


@pytest.mark.parametrize('obs,a,b,pi', POOLED_TRUTH)
def test_numpy_passes_the_pooled_checks(obs, a, b, pi):
  """DKW at the law's quantiles, the tail counts, the zeros, mean and variance at N = 2^22: numpy inside every bar,
  the heaviest case (total_count 0.05, mean 1e6) included."""
  rng = np.random.default_rng(1)
  if obs == 'NORMAL':
    law, x = L.NormalLaw(a, b), rng.normal(a, b, N_POOL)
  else:
    law, x = _law(a, b, pi), _nb(rng, a, b, N_POOL, pi)
  sm = L.summarise_numpy(x, law)
  print(L.describe(sm, law, f'numpy {obs} {a:g} {b:g} {pi:g}'))
  assert L.check_summary(sm, law) == []


def test_total_count_off_by_5_percent_fails():
  rng = np.random.default_rng(2)
  law = _law(1.0, 30.0)
  sm = L.summarise_numpy(_nb(rng, 1.0, 30.0, N_POOL, tc_factor=1.05), law)
  print(L.describe(sm, law, 'total_count x 1.05'))
  failed = L.check_summary(sm, law)
  assert 'dkw' in failed and 'var' in failed


@pytest.mark.parametrize('obs', ['NORMAL', 'NB'])
def test_upper_tail_cut_at_1e_4_fails_the_tail_count(obs):
  """The draws beyond the 1 - 1e-4 quantile pulled back onto it: DKW (a move of 1e-4 against eps 0.0016) and the mean
  cannot see it, the tail count at 1e-4 does."""
  rng = np.random.default_rng(3)
  if obs == 'NORMAL':
    law, x = L.NormalLaw(0.5, 0.01), rng.normal(0.5, 0.01, N_POOL)
  else:
    law, x = _law(1e6, 30.0), _nb(rng, 1e6, 30.0, N_POOL)
  x = np.minimum(x, float(law.ppf(1.0 - 1e-4)))
  sm = L.summarise_numpy(x, law)
  print(L.describe(sm, law, f'{obs} cut tail'))
  failed = L.check_summary(sm, law)
  assert 'tail0.0001' in failed and 'dkw' not in failed and 'mean' not in failed


def test_poisson_mean_shifted_above_the_switch_fails():
  """Rates >= 10 drawn 0.43 too high (PTRS's centring constant applied twice), next to the switch."""
  rng = np.random.default_rng(4)
  law = _law(1e6, 10.01)
  sm = L.summarise_numpy(_nb(rng, 1e6, 10.01, N_POOL, rate_shift=0.43), law)
  print(L.describe(sm, law, 'rate + 0.43'))
  failed = L.check_summary(sm, law)
  assert 'dkw' in failed and 'mean' in failed


def _normal_totals(rng, n, mu, sigma, rho=0.0):
  """Totals of n N(mu, sigma^2) rows with pairwise correlation rho: rows sqrt(1 - rho) z_i + sqrt(rho) z_0, drawn row
  by row in chunks of paths (rho = 0: numpy's i.i.d. rows)."""
  out = np.empty(S_TOT)
  for s0 in range(0, S_TOT, 2048):
    z = rng.standard_normal((2048, n))
    if rho > 0:
      z = math.sqrt(1.0 - rho) * z + math.sqrt(rho) * rng.standard_normal((2048, 1))
    out[s0:s0 + 2048] = (mu + sigma * z).sum(axis=1)
  return out


def _total_checks(t, law, n):
  tl = law.total(n)
  sm = L.summarise_numpy(t, tl, thr=L.thresholds(tl, 128), with_tails=False)
  lo, hi = L.chi2_bounds(len(t) - 1)
  q = (len(t) - 1) * sm['var'] / tl.moments()[1]
  return sm['D'], L.dkw_eps(len(t)), q, lo, hi


@pytest.mark.parametrize('n', [2, 257, 1025])
def test_numpy_passes_the_total_checks(n):
  """Sums of numpy's own i.i.d. rows against the exact law of the total: NORMAL at every n (DKW and chi-square), NB and
  ZINB at n <= 257 (DKW); the lag autocorrelations of independent totals inside their bar."""
  rng = np.random.default_rng(5)
  law = L.NormalLaw(0.5, 2.0)
  t = _normal_totals(rng, n, 0.5, 2.0)
  d, eps, q, lo, hi = _total_checks(t, law, n)
  print(f'numpy NORMAL n={n}: D={d:.4f}/EPS={eps:.4f} chi2 {q:.0f} in [{lo:.0f}, {hi:.0f}]')
  assert d <= eps and lo <= q <= hi
  for lag in (1, 2, STRIDE):
    assert abs(np.corrcoef(t[:-lag], t[lag:])[0, 1]) <= L.lag_corr_bound(S_TOT - lag)
  if n <= 257:
    for pi in (0.0, 0.35):
      t = _nb(rng, 3.0, 8.0, (S_TOT, n), pi).sum(axis=1)
      d, eps, _, _, _ = _total_checks(t, _law(3.0, 8.0, pi), n)
      print(f'numpy counts pi={pi} n={n}: D={d:.4f}/EPS={eps:.4f}')
      assert d <= eps


@pytest.mark.parametrize('n', [1024, 1025])
def test_rows_correlated_at_1e_3_fail_the_total_checks(n):
  """A pairwise correlation of 1e-3 between rows (what a counter collision would give) multiplies the variance of a
  total by 1 + (n - 1) 1e-3: outside the DKW bar and the chi-square interval from n = 1,024 on."""
  rng = np.random.default_rng(6)
  t = _normal_totals(rng, n, 0.5, 2.0, rho=1e-3)
  d, eps, q, lo, hi = _total_checks(t, L.NormalLaw(0.5, 2.0), n)
  print(f'rho=1e-3 n={n}: D={d:.4f}/EPS={eps:.4f} chi2 {q:.0f} outside [{lo:.0f}, {hi:.0f}]')
  assert d > eps and q > hi


def test_adjacent_paths_correlated_at_005_fail_the_lag_check():
  rng = np.random.default_rng(7)
  z = rng.standard_normal(S_TOT + 1)
  a = (1.0 - math.sqrt(1.0 - 4.0 * 0.05 ** 2)) / (2.0 * 0.05)      # a / (1 + a^2) = 0.05
  t = z[1:] + a * z[:-1]
  r = np.corrcoef(t[:-1], t[1:])[0, 1]
  print(f'lag-1 correlation {r:.4f}, bar {L.lag_corr_bound(S_TOT - 1):.4f}')
  assert abs(r) > L.lag_corr_bound(S_TOT - 1)
  assert abs(np.corrcoef(t[:-2], t[2:])[0, 1]) <= L.lag_corr_bound(S_TOT - 2)


def test_mixture_moments_against_a_direct_sum():
  """The law of total variance across members, as the M = 7 test uses it."""
  laws = [_law(3.0 * f, 8.0 * g).total(16) for f, g in ((1.0, 1.0), (0.6, 0.5), (2.0, 3.0))]
  m, v, mu4 = L.mixture_moments(laws)
  ms = np.asarray([lw.moments()[0] for lw in laws])
  vs = np.asarray([lw.moments()[1] for lw in laws])
  np.testing.assert_allclose([m, v], [ms.mean(), vs.mean() + (ms ** 2).mean() - ms.mean() ** 2], rtol=1e-12)
  k = np.arange(0.0, 20000.0)
  pm = np.mean([np.diff(np.concatenate([[0.0], lw.cdf(k)])) for lw in laws], axis=0)
  assert abs((pm * (k - m) ** 4).sum() / mu4 - 1.0) < 1e-6
