"""The NORMAL forecast kernels at the data's own scale: bnf_normal_mixture_quantiles (exact and moment-matched),
bnf_predictive_scores and their *_weighted forms with `loc` around 0, 1e3 and +-1e5, sigma 0.01, 1 and 30 -- the reference
does not standardise the target, and the stated range is |y| up to 1e5 with sigma at its 0.01 floor.  Cases and references:
tests/normal_scale_ref.py (tests/test_normal_scale_host.py holds the references themselves to the bars below).

Bars (none tuned on the code under test):
  exact quantiles    per (row, level), q32 = float32(q): |F64(x) - q32| <= 2e-5, the bar of tests/test_gpu_weighted.py, OR
                     F64(pred32(x)) <= q32 <= F64(succ32(x)): the root lies within one float32 step of x.  At centre 1e5 and
                     sigma 0.01 adjacent floats are 0.78 sigma apart and no float32 answer meets the first clause; at
                     centre 0 the first clause alone must hold.
  moment match       |x - want| <= 2 ulp32(want) + 1e-5 sd_mix |z_q| against the centred float64 moment match: what a
                     float32 result costs, plus the rtol 1e-5 of tests/test_gpu_weighted.py on the part that is not the mean.
  scores             `_check` of tests/test_gpu_scoring.py and `_check_scores` of tests/test_gpu_weighted.py, unchanged.
  shift, two calls   bit equality.
Every test prints what it measured (-s shows it)."""
import numpy as np
import pytest

from tests import normal_scale_ref as N
from tests import scoring_ref as S
from tests import test_gpu_scoring as TS
from tests import test_gpu_weighted as TW
from tests import weighted_ref as W

pytestmark = pytest.mark.gpu

CALLS = (None,) + W.PATTERNS          # the unweighted call, then every weight pattern


def _engine():
  return TW._engine('NORMAL')[0]       # forward-only, LDS poisoned


def _scores(eng, loc, aux, y, **kw):
  """All four outputs (member_ll is per member: the unweighted one with weights too)."""
  out = eng.predictive_scores(TW._dev(eng, loc), TW._dev(eng, aux), TW._dev(eng, y), **kw)
  return {k: v.cpu().numpy() for k, v in out.items()}


def _case_w(loc, sig, p):
  """-> (loc, w, keywords): p None is the unweighted call."""
  if p is None:
    return loc, None, {}
  loc, w = N.weighted(loc, sig, p)
  return loc, w, {'weights': w}


def _score_calls(M, R):
  """Every pattern while the float64 pair sums stay small; Dirichlet weights alone beyond."""
  return CALLS if M * M * R <= 1_000_000 else (None, 'dirichlet')


# ------------------------------------------------------------------------------------------------------ exact quantiles
@pytest.mark.parametrize('centre', N.CENTRES)
def test_exact_quantiles(centre):
  """k_quantile_root, unweighted and every weight pattern, on every grid point of this centre: M 1, 2, 7, 65 and 1,920, rows
  1, 255, 257 at centre 1e5."""
  eng = _engine()
  n = n_second = 0
  worst = 0.0
  for M, R, c, sigma, spread in N.quantile_grid():
    if c != centre:
      continue
    loc0, sig, _ = N.case(M, R, c, sigma, spread)
    for p in CALLS:
      loc, w, kw = _case_w(loc0, sig, p)
      x = TW._nq(eng, loc, sig, levels=N.LEVELS, **kw)
      assert x.shape == (len(N.LEVELS), R) and x.dtype == np.float32
      for i, q in enumerate(N.LEVELS):
        res, first, second = N.accept(loc, sig, x[i], q, w)
        ok = first | second
        assert np.all(ok), (M, R, c, sigma, spread, p, q, float(res[~ok].max()))
        if centre == 0:
          assert np.all(first), (M, R, sigma, spread, p, q, float(res.max()))
        n += R
        n_second += int(np.sum(~first))
        worst = max(worst, float(res[first].max()) if first.any() else 0.0)
  eng.close()
  print(f'exact quantiles, centre {centre:g}: {n} (row, level) pairs, worst residual on the first clause {worst:.2e} (bar '
        f'{N.QBAR:.0e}), {n_second / n:.1%} on the second clause')


# ------------------------------------------------------------------------------------------------- moment-matched quantiles
@pytest.mark.parametrize('centre', N.CENTRES)
def test_moment_matched_quantiles(centre):
  """k_quantile_approx, unweighted, uniform weights and the other patterns, against the centred float64 moment match.  The
  unweighted and the uniform-weights call each meet the bar (no bit equality asked)."""
  eng = _engine()
  worst = worst_sd = 0.0
  for M, R, c, sigma, spread in N.quantile_grid():
    if c != centre:
      continue
    loc0, sig, _ = N.case(M, R, c, sigma, spread)
    for p in CALLS:
      loc, w, kw = _case_w(loc0, sig, p)
      x = TW._nq(eng, loc, sig, levels=N.LEVELS, approximate=True, **kw)
      assert x.shape == (len(N.LEVELS), R) and x.dtype == np.float32
      _, var = N.mixture_moments(loc, sig, w)
      for i, q in enumerate(N.LEVELS):
        want, bar = N.moment_bar(loc, sig, float(np.float32(q)), w)
        err = np.abs(x[i].astype(np.float64) - want)
        worst, worst_sd = max(worst, float(np.max(err / bar))), max(worst_sd, float(np.max(err / np.sqrt(var))))
        assert np.all(err <= bar), (M, R, c, sigma, spread, p, q, float(np.max(err / bar)), float(np.max(err / np.sqrt(var))))
  eng.close()
  print(f'moment-matched quantiles, centre {centre:g}: worst error {worst:.2f} of the bar, {worst_sd:.2e} mixture sd')


# ---------------------------------------------------------------------------------------------------------------- scores
def _score_both(eng, tag, loc0, sig, y, calls, ref=None, f32=None):
  """The unweighted call under tests/test_gpu_scoring.py's `_check`, the weighted ones under tests/test_gpu_weighted.py's
  `_check_scores`; crps > 0 and pit[0] == pit[1] in each."""
  R = len(y)
  aux = S.normal_aux(sig)
  for p in calls:
    loc, w, kw = _case_w(loc0, sig, p)
    got = _scores(eng, loc, aux, y, **kw)
    assert got['lpd'].shape == (R,) and got['pit'].shape == (2, R) and got['crps'].shape == (R,)
    assert np.array_equal(got['pit'][0], got['pit'][1]), (tag, p)
    assert np.all(got['crps'] > 0), (tag, p)
    if p is None:
      TS._check(f'{tag} unweighted:', got, ref if ref is not None else S.normal_ref(loc, sig, y),
                f32 if f32 is not None else S.normal_f32(loc, sig, y))
    else:
      TW._check_scores(f'{tag} {p}:', got, W.normal_ref(loc, sig, y, w), W.normal_f32(loc, sig, y, w), True)


@pytest.mark.parametrize('centre', N.CENTRES)
def test_scores_on_the_grid(centre):
  """lpd, pit, crps and member_ll, unweighted and weighted, on every grid point of this centre: M 1, 2, 7, 65, 1,033 and
  1,920, rows 1, 65, 1025 at centre 1e5."""
  eng = _engine()
  for M, R, c, sigma, spread in N.score_grid():
    if c != centre:
      continue
    loc, sig, y, ref, f32 = N.score_case(M, R, c, sigma, spread)
    _score_both(eng, f'NORMAL centre {c:g} sigma {sigma:g} spread {spread:g} M={M} R={R}', loc, sig, y, _score_calls(M, R), ref, f32)
  eng.close()


@pytest.mark.parametrize('M', [1, 7])
def test_scores_tails_at_scale(M):
  """scoring_ref.tail_case around 1e5: |y - mu_m| = 40 sigma_m for every member.  lpd finite, about -800, within its bar;
  every member's CDF exactly 0 or 1: pit is exactly the (weighted) share of the members below y, 0 or 1 for one member."""
  eng = _engine()
  loc, sig, y = N.tail_case(M, 1e5)
  aux = S.normal_aux(sig)
  for p in (None, 'dirichlet'):
    _, w, kw = _case_w(loc, sig, p)
    got = _scores(eng, loc, aux, y, **kw)
    assert np.all(np.isfinite(got['lpd'])) and got['lpd'].max() < -700, p
    below = (loc < y[None, :]).astype(np.float64)
    share = below.sum(axis=0) / M if w is None else np.add.accumulate(w[:, None] * below, axis=0)[-1]
    assert np.array_equal(got['pit'], np.stack([share, share]).astype(np.float32)), p
    if M == 1:
      assert np.all((got['pit'] == 0.0) | (got['pit'] == 1.0)), p
  _score_both(eng, f'tails at 1e5 M={M}', loc, sig, y, (None, 'dirichlet'))
  eng.close()


# ------------------------------------------------------------------------------------------------------ shift, determinism
@pytest.mark.parametrize('M,R', [(1, 65), (20, 1025)])
def test_scores_do_not_change_under_an_exact_shift(M, R):
  """loc and y multiples of 2^-6 below 64, and the same plus 2^17 (exact in float32): every term of every score is a
  function of y - mu or mu_i - mu_j, and those have the same bits in the two calls, so lpd, pit, crps and member_ll must
  too.  A kernel that forms anything from an uncentred value fails here."""
  eng = _engine()
  loc, y, loc_s, y_s, sig = N.shift_case(M, R)
  aux = S.normal_aux(sig)
  for p in (None, 'dirichlet', 'tiny_outlier'):
    kw = {} if p is None else {'weights': W.weights(p, M)}
    a, b = _scores(eng, loc, aux, y, **kw), _scores(eng, loc_s, aux, y_s, **kw)
    assert set(a) == set(b) == {'member_ll', 'lpd', 'pit', 'crps'}
    for k in a:
      assert np.all(np.isfinite(a[k])), (p, k)
      assert TW._same(a[k], b[k]), (p, k, float(np.max(np.abs(a[k].astype(np.float64) - b[k]))))
  eng.close()


def test_two_calls_give_the_same_bits_at_scale():
  """Centre 1e5: exact and moment-matched quantiles and all four scores, unweighted and weighted, twice."""
  eng = _engine()
  loc0, sig, y = N.case(65, 257, 1e5, 1.0, 3.0)
  aux = S.normal_aux(sig)
  for p in (None, 'dirichlet'):
    loc, _, kw = _case_w(loc0, sig, p)
    runs = []
    for _ in range(2):
      eng.debug_poison_lds()
      runs.append([TW._nq(eng, loc, sig, levels=N.LEVELS, **kw), TW._nq(eng, loc, sig, levels=N.LEVELS, approximate=True, **kw)]
                  + list(_scores(eng, loc, aux, y, **kw).values()))
    assert len(runs[0]) == 6 and all(TW._same(a, b) for a, b in zip(*runs)), p
  eng.close()
