"""CPU-only: the references of tests/normal_scale_ref.py stay inside the bars tests/test_gpu_normal_scale.py holds the
NORMAL forecast kernels to, at the data's own scale (centres 0, 1e3, +-1e5; sigma 0.01, 1, 30).

  the centred float64 moment match against exact rational arithmetic; the naive float64 form shown to fail;
  the float32 restatement of the scores against the float64 reference: under 1e-6, so every score bar is the 1e-5 gate;
  k_quantile_root restated in float32 (sequential float32 CDF sum, bracket, tolerances, 60 iterations) against the
  acceptance rule for exact quantiles.
Every test prints its table (-s shows it)."""
import functools

import numpy as np
import pytest

from tests import normal_scale_ref as N
from tests import scoring_ref as S
from tests import weighted_ref as W

EMULATED_ROWS = 48      # rows of each case the root finder's restatement runs on (they are independent; the bracket is
                        # that of the whole case)


def _rows(R):
  return sorted({0, R // 2, R - 1})


def test_centred_moments_against_exact_rational_arithmetic():
  """Variance of `mixture_moments` against fractions.Fraction on the float32 inputs, unweighted and Dirichlet weights, on
  the whole quantile grid (first, middle and last row of each case): relative error <= 1e-12."""
  worst = {}
  for M, R, centre, sigma, spread in N.quantile_grid():
    loc, sig, _ = N.case(M, R, centre, sigma, spread)
    for w in (None, W.weights('dirichlet', M)):
      _, var = N.mixture_moments(loc, sig, w)
      for r in _rows(R):
        exact = N.exact_variance(loc, sig, r, w)
        err = abs(float((exact - N.Fraction(float(var[r]))) / exact))
        worst[centre] = max(worst.get(centre, 0.0), err)
        assert err <= 1e-12, (M, R, centre, sigma, spread, w is None, err)
  print('centred float64 variance, relative error against exact:', {f'{c:g}': f'{v:.1e}' for c, v in worst.items()})


def test_the_naive_float64_form_loses_the_variance_at_scale():
  """Why there is a new reference: sum w (sd^2 + mu^2) - (sum w mu)^2 in float64 -- the form of
  weighted_ref.normal_moment_quantile and of the weighted kernel before it was centred -- at centre 1e5, sigma 0.01,
  spread 0, Dirichlet weights is off by more than 1 % of the variance: one float64 step of 1e10 is 0.8 % of sd^2 = 2e-4.
  (Equal weights, the oracle's approximate_normal_quantile: the same size, printed.)"""
  loc, sig, _ = N.case(7, 255, 1e5, 0.01, 0.0)
  w = W.weights('dirichlet', 7)
  errs = []
  for ww in (w, None):
    naive = N.naive_variance(loc, sig, ww)
    errs.append(max(abs(float((N.Fraction(float(naive[r])) - N.exact_variance(loc, sig, r, ww)) / N.exact_variance(loc, sig, r, ww)))
                    for r in _rows(255)))
  print(f'naive float64 variance at (1e5, 0.01, spread 0), M = 7: relative error {errs[0]:.2e} weighted, {errs[1]:.2e} equal weights')
  assert errs[0] > 1e-2
  want = W.normal_moment_quantile(loc, sig, 0.975, w)             # the reference that cannot judge this path at scale
  mean, var = N.mixture_moments(loc, sig, w)
  assert np.max(np.abs((want - mean) / (np.sqrt(var) * 1.959963984540054) - 1.0)) > 4e-3
  loc0, sig0, _ = N.case(7, 255, 0.0, 0.01, 3.0)                  # at O(1) centres it is fine
  np.testing.assert_allclose(N.naive_variance(loc0, sig0), N.mixture_moments(loc0, sig0)[1], rtol=1e-12)


@functools.lru_cache(maxsize=None)
def _restatement_table():
  """{(centre, output): (worst restatement error, its grid point)} over the score grid, the weighted pair on Dirichlet
  weights ('w ...') and the tails at 1e5 included."""
  worst = {}

  def note(centre, point, e):
    for k, v in e.items():
      if v >= worst.get((centre, k), (0.0,))[0]:
        worst[centre, k] = (v, point)
  for M, R, centre, sigma, spread in N.score_grid():
    loc, sig, y, ref, f32 = N.score_case(M, R, centre, sigma, spread)
    e = S.restatement_errors(ref, f32)
    if M <= 65:
      w = W.weights('dirichlet', M)
      rw, fw = W.normal_ref(loc, sig, y, w), W.normal_f32(loc, sig, y, w)
      e['w lpd'], e['w pit'], e['w crps'] = S.rel1(fw['lpd'], rw['lpd']), S.abs_err(fw['pit'], rw['pit']), S.crps_err(fw['crps'], rw)
    note(centre, (M, R, sigma, spread), e)
  loc, sig, y = N.tail_case(7, 1e5)
  note(1e5, 'tails', S.restatement_errors(S.normal_ref(loc, sig, y), S.normal_f32(loc, sig, y)))
  for c in N.CENTRES:
    print(f'restatement, centre {c:g}:', ' '.join(f'{k} {v[0]:.1e}' for (cc, k), v in worst.items() if cc == c))
  return worst


def test_score_restatement_stays_under_1e6_on_the_grid():
  """restatement_errors(normal_ref, normal_f32) <= 1e-6 on the whole score grid (lpd, member_ll, pit, crps), and lpd, pit,
  crps of the weighted pair on Dirichlet weights: S.bar = max(1e-5, 4 x restatement) is then the 1e-5 gate everywhere.
  Measured: lpd <= 2.1e-7, pit <= 6.9e-8, crps <= 1.4e-7, member_ll <= 6.5e-7 (M = 1,920, 5 rows, sigma 0.01, spread 3: a
  row's log density is 3.69 - log(s_m / s) - z^2 / 2 there, its mean over the rows about 0, and the sum comes out at a few
  units).  member_ll is why the log density is formed in float64 and rounded once: a float32 chain, z then z^2 then the two
  subtractions, is off by 1e-5 of a row at |z| = 10 and measured 1.0e-6 .. 8.5e-6 here, at centre 0 as much as at 1e5."""
  for (centre, k), (v, point) in _restatement_table().items():
    assert v <= 1e-6, (centre, point, k, v)


@pytest.mark.parametrize('centre', N.CENTRES)
def test_root_finder_restated_in_f32_meets_the_acceptance_rule(centre):
  """`root_f32` (k_quantile_root operation by operation) on every grid point of this centre and every level: each (row,
  level) meets the first clause (residual <= 2e-5) or the second (the root within one float32 step); at centre 0 the
  first alone.  Unweighted (the float32 CDF sum) and Dirichlet weights (the float64 one)."""
  n = n_second = 0
  worst = 0.0
  for M, R, c, sigma, spread in N.quantile_grid():
    if c != centre:
      continue
    loc, sig, _ = N.case(M, R, c, sigma, spread)
    rows = slice(0, min(R, EMULATED_ROWS))
    for w in (None, W.weights('dirichlet', M)):
      if w is not None and M > 65:
        continue
      for q in N.LEVELS:
        x = N.root_f32(loc[:, rows], sig, q, w, bracket=N.bracket_f32(loc, sig))
        res, first, second = N.accept(loc[:, rows], sig, x, q, w)
        assert np.all(first | second), (M, R, c, sigma, spread, q, w is None, float(res[~(first | second)].max()))
        if centre == 0:
          assert np.all(first), (M, R, sigma, spread, q, float(res.max()))
        n += len(x)
        n_second += int(np.sum(~first))
        worst = max(worst, float(res[first].max()) if first.any() else 0.0)
  print(f'root finder in f32, centre {centre:g}: {n} (row, level) pairs, {n - n_second} on the first clause (worst residual '
        f'{worst:.2e}, bar {N.QBAR:.0e}), {n_second} on the second')
