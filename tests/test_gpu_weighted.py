"""The marginal forecast of the weighted mixture of members on the GPU (include/bnf.h bnf_normal_mixture_quantiles_weighted,
bnf_count_mixture_quantiles_weighted, bnf_predictive_scores_weighted, bnf_count_rps_weighted) against the float64
references of tests/weighted_ref.py evaluated on the same float32 inputs and float64 weights.

Bars (none tuned on the code under test):
  quantiles   |F_w(x) - q| <= 2e-5 under the float64 weighted CDF -- the kernel's 1e-5 value tolerance plus the float32
              CDF, the project's quantile bar (tests/test_gpu_parity.py); counts: an integer k with F_w(k) >= q - 2e-5 and
              (F_w(k - 1) <= q + 2e-5 or k = 0); the moment-matched form rtol 1e-5 against float64 at the float32 level
  scores      lpd max(1e-5, 4 x the float32 restatement's own error) of |dev - ref| / max(1, |ref|); pit 1e-5 absolute;
              crps the same rule relative to the first term of the reference (tests/scoring_ref.py)
  rps         the same rule on |dev - ref| / |ref| (tests/rps_ref.py)
tests/test_weighted_host.py prints the restatements' tables: they stay under 4e-7, so every bar here is the 1e-5 gate.
Every test prints what it measured (-s shows it)."""
import ctypes as C
import os

import numpy as np
import pandas as pd
import pytest
import torch
from scipy import special as sp

from bayesnf_amd import BayesianNeuralFieldMAP, BayesianNeuralFieldVI, _native
from bayesnf_amd.engine import Engine
from oracle import bnf_oracle as O
from tests import rps_ref as P
from tests import scoring_ref as S
from tests import util
from tests import weighted_ref as W
from tests.test_gpu_sampling import MODEL, TCS, inv_softplus

pytestmark = pytest.mark.gpu

LEVELS = (0.025, 0.5, 0.975)
QBAR = 2e-5


def _engine(obs):
  net, model, _, _ = util.make_problem(n_rows=16, width=64, depth=1, observation_model=obs)
  eng = Engine(net, members=1, forward_only=True, row_capacity=128, compute_dtype='fp32')
  eng.debug_poison_lds()
  return eng, model


def _dev(eng, a):
  return torch.from_numpy(np.array(a, dtype=np.float32)).to(eng.device)     # (a copy: the shared cases are read-only)


def _bits(a):
  a = np.ascontiguousarray(a)
  return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def _same(a, b):
  return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _nq(eng, loc, sigma, levels=LEVELS, **kw):
  return eng.normal_mixture_quantiles(_dev(eng, loc), _dev(eng, sigma), levels, **kw).cpu().numpy()


def _cq(eng, loc, aux, levels=LEVELS, **kw):
  means, q = eng.count_mixture_quantiles(_dev(eng, loc), _dev(eng, aux), levels, **kw)
  return means.cpu().numpy(), q.cpu().numpy()


def _scores(eng, loc, aux, y, **kw):
  kw.setdefault('member_ll', False)
  out = eng.predictive_scores(_dev(eng, loc), _dev(eng, aux), _dev(eng, y), **kw)
  return {k: v.cpu().numpy() for k, v in out.items()}


def _rps(eng, loc, aux, y, **kw):
  out = eng.count_rps(_dev(eng, loc), _dev(eng, aux), _dev(eng, y), **kw)
  assert out.shape == (len(y),) and out.dtype == torch.float32
  return out.cpu().numpy()


def _check_scores(tag, got, ref, f32, crps):
  errs = dict(lpd=S.rel1(got['lpd'], ref['lpd']), pit=S.abs_err(got['pit'], ref['pit']))
  rest = dict(lpd=S.rel1(f32['lpd'], ref['lpd']), pit=S.abs_err(f32['pit'], ref['pit']))
  bars = dict(lpd=S.bar(rest['lpd']), pit=S.PIT_BAR)
  if crps:
    errs['crps'], rest['crps'] = S.crps_err(got['crps'], ref), S.crps_err(f32['crps'], ref)
    bars['crps'] = S.bar(rest['crps'])
  print(tag, ' '.join(f'{k} {v:.2e} (f32 {rest[k]:.1e}, bar {bars[k]:.0e})' for k, v in errs.items()))
  for k, v in errs.items():
    assert v <= bars[k], (tag, k, v, bars[k])


def _check_count_quantiles(tag, k, fc, w, levels=LEVELS):
  """The assertions of tests/test_gpu_parity.py's count quantile test with the weighted CDF."""
  assert np.all(k == np.round(k)) and np.all(k >= 0), tag
  worst = 0.0
  for i, q in enumerate(levels):
    F_k = W.count_cdf(fc, k[i], w)
    F_lo = W.count_cdf(fc, np.maximum(k[i] - 1.0, 0.0), w)
    worst = max(worst, float(np.max(q - F_k)), float(np.max(np.where(k[i] == 0, -1.0, F_lo - q))))
    assert np.all(F_k >= q - QBAR), (tag, q, float(np.min(F_k - q)))
    assert np.all((F_lo <= q + QBAR) | (k[i] == 0)), (tag, q, float(np.max(F_lo - q)))
  return worst


# ----------------------------------------------------------------------------------------------------- Normal quantiles
@pytest.mark.parametrize('M', [1, 2, 7, 65])
def test_normal_quantiles(M):
  """Rows 1 and around the 256-thread block; members 1, 2, 7 and 65; every weight pattern.  Exact form: the residual of the
  float64 weighted CDF; one-hot: the residual of that member's own CDF; approximate form: the float64 moment match."""
  eng, _ = _engine('NORMAL')
  worst = worst_a = 0.0
  for R in (1, 255, 256, 257):
    for p in W.PATTERNS:
      loc, sigma, _, w = W.normal_case(M, R, p)
      x = _nq(eng, loc, sigma, weights=w)
      assert x.shape == (3, R) and x.dtype == np.float32
      for i, q in enumerate(LEVELS):
        res = np.abs(W.normal_cdf(loc, sigma, x[i], w) - q)
        worst = max(worst, float(res.max()))
        assert np.all(res <= QBAR), (M, R, p, q, float(res.max()))
        if p == 'one_hot':
          m = int(np.argmax(w))
          own = np.abs(sp.ndtr((x[i].astype(np.float64) - loc[m]) / float(sigma[m])) - q)
          assert np.all(own <= QBAR), (M, R, q, float(own.max()))
      xa = _nq(eng, loc, sigma, weights=w, approximate=True)
      for i, q in enumerate(LEVELS):
        want = W.normal_moment_quantile(loc, sigma, float(np.float32(q)), w)
        worst_a = max(worst_a, float(np.max(np.abs(xa[i] - want) / np.abs(want))))
        np.testing.assert_allclose(xa[i], want, rtol=1e-5, atol=0.0)
  eng.close()
  print(f'NORMAL M={M}: worst CDF residual {worst:.2e} (bar {QBAR:.0e}), moment match rel {worst_a:.2e} (bar 1e-05)')


# ------------------------------------------------------------------------------------------------------ count quantiles
@pytest.mark.parametrize('M', [1, 7, 65])
@pytest.mark.parametrize('obs', ['NB', 'ZINB'])
def test_count_quantiles(obs, M):
  """The total counts of tests/test_gpu_sampling.py at 65 rows, and rows 1, 63, 64 (around the 64-thread block) at
  total_count 3; row means <= 400; every weight pattern.  The per-member means are those of the unweighted call."""
  eng, model = _engine(obs)
  worst = -1.0
  for tc, R in [(tc, 65) for tc in TCS] + [(3.0, R) for R in (1, 63, 64)]:
    plain = None
    for p in W.PATTERNS:
      loc, aux, _, w = W.count_case_w(obs, M, R, p, tc=tc)
      means, k = _cq(eng, loc, aux, weights=w)
      assert means.shape == (M, R) and k.shape == (3, R)
      if p != 'tiny_outlier':
        plain = _cq(eng, loc, aux)[0] if plain is None else plain
        assert _same(means, plain), (obs, M, R, tc, p)
      worst = max(worst, _check_count_quantiles((obs, M, R, tc, p), k, P.forecast(model, loc, aux), w))
  eng.close()
  print(f'{obs} M={M}: worst violation of F_w(k) >= q, F_w(k - 1) <= q: {worst:.2e} (bar {QBAR:.0e})')


# --------------------------------------------------------------------------------------------------------------- scores
@pytest.mark.parametrize('M', list(W.SCORE_MEMBERS_NORMAL) + [1033])
def test_scores_normal(M):
  """Members 1, 2, 7, 9 (one more than the 8-member chunk), 20 (three chunks, the last one short) and 1033 (more slots than
  the 64 blocks they round-robin over; 5 rows); rows 1, 63, 64, 65, 1025; every weight pattern."""
  eng, _ = _engine('NORMAL')
  for R in ((5,) if M > 1000 else W.SCORE_ROWS):
    for p in W.PATTERNS:
      loc, sigma, y, w = W.normal_case(M, R, p)
      got = _scores(eng, loc, S.normal_aux(sigma), y, weights=w)
      assert set(got) == {'lpd', 'pit', 'crps'}
      assert got['lpd'].shape == (R,) and got['pit'].shape == (2, R) and got['crps'].shape == (R,)
      assert np.array_equal(got['pit'][0], got['pit'][1]) and np.all(got['crps'] > 0)
      _check_scores(f'NORMAL M={M} R={R} {p}:', got, W.normal_ref(loc, sigma, y, w), W.normal_f32(loc, sigma, y, w), True)
  eng.close()


@pytest.mark.parametrize('M', W.SCORE_MEMBERS_COUNT)
@pytest.mark.parametrize('obs', ['NB', 'ZINB'])
def test_scores_counts(obs, M):
  eng, model = _engine(obs)
  for R in W.SCORE_ROWS:
    for p in W.PATTERNS:
      loc, aux, y, w = W.count_case_w(obs, M, R, p)
      got = _scores(eng, loc, aux, y, weights=w)
      assert set(got) == {'lpd', 'pit'}
      assert np.all(got['pit'][1][y == 0] == 0.0) and np.all(got['pit'][0] >= got['pit'][1])
      _check_scores(f'{obs} M={M} R={R} {p}:', got, W.count_ref(P.forecast(model, loc, aux), y, w),
                    W.count_f32(loc, aux, y, obs, w), False)
  with pytest.raises(ValueError, match='crps'):
    _scores(eng, loc, aux, y, weights=w, crps=True)
  eng.close()


@pytest.mark.parametrize('M', [1, 7])
def test_scores_tails_and_nan_rows(M):
  """|y - mu_m| / sigma_m = 40 for every member: every density underflows; the weighted lpd stays finite, about -800, and
  within its bar.  Rows with a NaN y: NaN in every per-row output."""
  eng, _ = _engine('NORMAL')
  loc, sigma, y = S.tail_case(M)
  y = y.copy()
  y[[0, 17, 64, 95]] = np.nan
  w = W.weights('dirichlet', M)
  got = _scores(eng, loc, S.normal_aux(sigma), y, weights=w)
  keep = np.isfinite(y)
  assert np.all(np.isfinite(got['lpd'][keep])) and got['lpd'][keep].max() < -700
  for k in ('lpd', 'crps'):
    assert np.array_equal(np.isnan(got[k]), ~keep), k
  assert np.array_equal(np.isnan(got['pit']), np.stack([~keep, ~keep]))
  _check_scores(f'tails M={M}:', got, W.normal_ref(loc, sigma, y, w), W.normal_f32(loc, sigma, y, w), True)
  eng.close()
  eng, model = _engine('NB')
  loc, aux, yc, w = W.count_case_w('NB', 7, 65, 'dirichlet')
  yc = yc.copy()
  yc[3] = np.nan
  got = _scores(eng, loc, aux, yc, weights=w)
  eng.close()
  assert np.isnan(got['lpd'][3]) and np.all(np.isnan(got['pit'][:, 3])) and np.isnan(got['lpd']).sum() == 1


def test_scores_outputs_are_optional_and_bad_arguments_are_refused():
  """Each output alone gives the bits of the full call; a short work buffer, no members, no rows and no weights are
  BNF_ERR_INVALID, and so is crps on a count handle."""
  eng, _ = _engine('NORMAL')
  loc, sigma, y, w = W.normal_case(9, 65, 'dirichlet')
  aux = S.normal_aux(sigma)
  full = _scores(eng, loc, aux, y, weights=w)
  for only in ('lpd', 'pit', 'crps'):
    kw = dict(lpd=False, pit=False, crps=False)
    kw[only] = True
    part = _scores(eng, loc, aux, y, weights=w, **kw)
    assert list(part) == [only] and _same(part[only], full[only]), only
  with_ll = _scores(eng, loc, aux, y, weights=w, member_ll=True)
  plain = _scores(eng, loc, aux, y, member_ll=True)
  assert _same(with_ll['member_ll'], plain['member_ll']) and _same(with_ll['crps'], full['crps'])
  loc_d, aux_d, y_d = _dev(eng, loc), _dev(eng, aux), _dev(eng, y)
  w_d = torch.from_numpy(w).to(eng.device)
  crps = torch.empty(65, dtype=torch.float32, device=eng.device)
  work = torch.empty(65, dtype=torch.float64, device=eng.device)          # 65 rows x 1 slot
  p = lambda t: C.c_void_p(t.data_ptr())
  call = lambda wts, M, R, nbytes: eng.lib.bnf_predictive_scores_weighted(
      eng.handle, p(loc_d), p(aux_d), wts, M, R, p(y_d), p(work), C.c_size_t(nbytes), None, None, p(crps))
  assert call(p(w_d), 9, 65, 8 * 65) == 0
  torch.cuda.synchronize()
  assert _same(crps.cpu().numpy(), full['crps'])
  for wts, M, R, nbytes in ((p(w_d), 9, 65, 8 * 65 - 1), (p(w_d), 0, 65, 1 << 20), (p(w_d), 9, 0, 1 << 20),
                            (None, 9, 65, 8 * 65)):
    assert call(wts, M, R, nbytes) == -1, (M, R, nbytes)
  q = (C.c_float * 1)(0.5)
  out = torch.empty(65, dtype=torch.float32, device=eng.device)
  assert eng.lib.bnf_normal_mixture_quantiles_weighted(eng.handle, p(loc_d), p(aux_d), None, 9, 65, q, 1, 0, p(out)) == -1
  eng.close()
  eng, _ = _engine('NB')
  loc, aux, yc, w = W.count_case_w('NB', 7, 65, 'dirichlet')
  loc_d, aux_d, y_d, w_d = _dev(eng, loc), _dev(eng, aux), _dev(eng, yc), torch.from_numpy(np.array(w)).to(eng.device)
  assert eng.lib.bnf_predictive_scores_weighted(eng.handle, p(loc_d), p(aux_d), p(w_d), 7, 65, p(y_d), p(work),
                                                C.c_size_t(8 * 65), None, None, p(crps)) == -1
  assert 'crps' in _native.last_error()
  assert eng.lib.bnf_count_rps_weighted(eng.handle, p(loc_d), p(aux_d), None, 7, 65, p(y_d), p(out)) == -1
  means = torch.empty((7, 65), dtype=torch.float32, device=eng.device)
  assert eng.lib.bnf_count_mixture_quantiles_weighted(eng.handle, p(loc_d), p(aux_d), None, 7, 65, q, 1, p(means),
                                                      p(out)) == -1
  torch.cuda.synchronize()
  eng.close()


# ------------------------------------------------------------------------------------------------------------------ rps
def _rps_params():
  seen = []
  for kind, obs, key, _ in W.rps_cases():
    if (kind, obs, key) not in seen:
      seen.append((kind, obs, key))
  return seen


@pytest.mark.parametrize('kind,obs,key', _rps_params())
def test_rps(kind, obs, key):
  """`members`: 1, 7, 64, 65 and 70 mixture components (chunks of 64 with and without a remainder) x 65 rows of
  rps_ref.many_member_case; `grid`: the grid of tests/test_gpu_sampling.py at M = 7, means <= 400.  Every weight pattern,
  under the bar, NaN nowhere (tests/test_weighted_host.py: the restatement caps no row of these cases)."""
  eng, _ = _engine(obs)
  for p in W.PATTERNS:
    loc, aux, y, w, ref, f64, terms = W.rps_get(kind, obs, key, p)
    eng.debug_poison_lds()
    got = _rps(eng, loc, aux, y, weights=w)
    assert np.all(np.isfinite(got)) and np.all(got > 0), (kind, obs, key, p)
    rest, err = P.rel_err(f64, ref), P.rel_err(got, ref)
    print(f'{kind} {obs} {key:g} {p} (longest window {terms.max()}): device {err:.2e} (restatement {rest:.1e}, bar {P.bar(rest):.0e})')
    assert err <= P.bar(rest), (kind, obs, key, p, err)
  eng.close()


@pytest.mark.parametrize('obs', ['NB', 'ZINB'])
def test_rps_a_member_of_weight_zero_cannot_cap_a_row(obs):
  """A member with mean 1e6 at total_count 0.05 would need 3e8 terms: alone it caps every row (NaN).  At weight 0 it changes
  nothing: the bits of the call without it."""
  eng, _ = _engine(obs)
  loc, aux, y, w = W.count_case_w(obs, 7, 65, 'dirichlet')
  wide_loc = np.full((1, 65), inv_softplus(0.05 ** 2 / 1e6), dtype=np.float32)
  wide_aux = np.asarray([[1.0, 1.0 / 0.05, 0.35]], dtype=np.float32)
  loc8, aux8 = np.concatenate([loc, wide_loc]), np.concatenate([aux, wide_aux])
  without = _rps(eng, loc, aux, y, weights=w)
  got = _rps(eng, loc8, aux8, y, weights=np.append(w, 0.0))
  alone = _rps(eng, loc8, aux8, y, weights=np.append(np.zeros(7), 1.0))
  eng.close()
  assert np.all(np.isnan(alone))
  assert np.all(np.isfinite(got)) and _same(got, without)


# ------------------------------------------------------------------- zero weights, uniform weights, None, determinism
def _families(p, M=7, R=65):
  """The four families at one shape: (name, obs, w, the per-member arrays, call(eng, per-member arrays, keywords) -> list
  of result arrays)."""
  nloc, nsig, ny, nw = W.normal_case(M, R, p)
  fams = [('normal quantiles', 'NORMAL', nw, (nloc, nsig),
           lambda eng, a, kw: [_nq(eng, a[0], a[1], **kw), _nq(eng, a[0], a[1], approximate=True, **kw)]),
          ('normal scores', 'NORMAL', nw, (nloc, S.normal_aux(nsig)),
           lambda eng, a, kw: list(_scores(eng, a[0], a[1], ny, **kw).values()))]
  for obs in ('NB', 'ZINB'):
    loc, aux, y, cw = W.count_case_w(obs, M, R, p)
    fams += [(f'{obs} quantiles', obs, cw, (loc, aux), lambda eng, a, kw: [_cq(eng, a[0], a[1], **kw)[1]]),
             (f'{obs} scores', obs, cw, (loc, aux), lambda eng, a, kw, y=y: list(_scores(eng, a[0], a[1], y, **kw).values())),
             (f'{obs} rps', obs, cw, (loc, aux), lambda eng, a, kw, y=y: [_rps(eng, a[0], a[1], y, **kw)])]
  return fams


def test_zero_weights_give_the_bits_of_the_call_on_the_kept_members():
  """Every second weight 0, and NaN in the network output of exactly those members: the result is finite and has the bits
  of the call on the other members with the same positive weights -- a member of weight 0 plays no part at all."""
  engines = {}
  for name, obs, w, arrays, call in _families('every_second_zero'):
    eng = engines.setdefault(obs, _engine(obs)[0])
    keep = np.nonzero(w)[0]
    assert 0 < len(keep) < len(w)
    poisoned = np.array(arrays[0])
    poisoned[w == 0] = np.nan
    a = call(eng, (poisoned, arrays[1]), {'weights': w})
    b = call(eng, (arrays[0][keep], arrays[1][keep]), {'weights': w[keep]})
    assert len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b)), name
    assert all(np.all(np.isfinite(x)) for x in a), name
  for eng in engines.values():
    eng.close()


def test_uniform_weights_meet_the_bars_of_the_unweighted_call():
  """w = 1 / M against the equal-weight references of tests/scoring_ref.py / tests/rps_ref.py (no bit equality asked)."""
  M, R = 7, 65
  w = np.full(M, 1.0 / M)
  eng, _ = _engine('NORMAL')
  loc, sigma, y = S.normal_case(M, R)
  got = _scores(eng, loc, S.normal_aux(sigma), y, weights=w)
  _check_scores('NORMAL uniform:', got, S.normal_ref(loc, sigma, y), S.normal_f32(loc, sigma, y), True)
  x = _nq(eng, loc, sigma, weights=w)
  for i, q in enumerate(LEVELS):
    assert np.all(np.abs(O.mixture_cdf(loc, sigma, x[i].astype(np.float64)) - q) <= QBAR)
  eng.close()
  for obs in ('NB', 'ZINB'):
    eng, model = _engine(obs)
    loc, aux, y = P.many_member_case(obs, M=M, R=R)
    fc = P.forecast(model, loc, aux)
    got = _scores(eng, loc, aux, y, weights=w)
    _check_scores(f'{obs} uniform:', got, S.count_ref(fc, y), S.count_f32(loc, aux, y, obs), False)
    ref, (f64, _, _) = P.count_rps_ref(fc, y), P.count_rps_f64(loc, aux, y, obs)
    err = P.rel_err(_rps(eng, loc, aux, y, weights=w), ref)
    assert err <= P.bar(P.rel_err(f64, ref)), (obs, err)
    _check_count_quantiles((obs, 'uniform'), _cq(eng, loc, aux, weights=w)[1], fc, w)
    eng.close()


def test_weights_none_is_the_call_without_the_keyword_and_two_calls_give_the_same_bits():
  engines = {}
  for name, obs, w, arrays, call in _families('dirichlet'):
    eng = engines.setdefault(obs, _engine(obs)[0])
    plain = call(eng, arrays, {})
    assert all(_same(x, y) for x, y in zip(plain, call(eng, arrays, {'weights': None}))), name
    a = call(eng, arrays, {'weights': w})
    eng.debug_poison_lds()
    b = call(eng, arrays, {'weights': w})
    assert all(_same(x, y) for x, y in zip(a, b)), name
    assert not all(_same(x, y) for x, y in zip(a, plain)), name          # the weights do reach the kernels
  eng = engines['NORMAL']
  loc, sigma, y, w = W.normal_case(7, 65, 'dirichlet')
  a = _scores(eng, loc, S.normal_aux(sigma), y, weights=None, member_ll=True)
  b = _scores(eng, loc, S.normal_aux(sigma), y, member_ll=True)
  assert list(a) == list(b) == ['member_ll', 'lpd', 'pit', 'crps'] and all(_same(a[k], b[k]) for k in a)
  for eng in engines.values():
    eng.close()


# -------------------------------------------------------------------------------------------- cross-checks between kernels
@pytest.mark.parametrize('obs', ['NORMAL', 'NB', 'ZINB'])
def test_weighted_lpd_agrees_with_the_stacking_kernel(obs):
  eng, _ = _engine(obs)
  if obs == 'NORMAL':
    loc, sigma, y, w = W.normal_case(20, 1025, 'dirichlet')
    aux = S.normal_aux(sigma)
  else:
    loc, aux, y, w = W.count_case_w(obs, 9, 1025, 'dirichlet')
  L = eng.member_log_density(_dev(eng, loc), _dev(eng, aux), _dev(eng, y))
  want = eng.stacking_weights(L, w_init=w, max_iter=0)['lpd'].cpu().numpy()
  got = _scores(eng, loc, aux, y, weights=w, pit=False, crps=False)['lpd']
  eng.close()
  err = S.rel1(got, want)
  print(f'{obs}: weighted lpd vs stacking lpd {err:.2e} (bar {S.GATE:.0e})')
  assert err <= S.GATE


def test_pit_at_the_weighted_quantile_is_the_level():
  """NORMAL: pit[0] at y = the weighted quantile returned for level q is within 3e-5 of q (the 2e-5 quantile bar plus the
  1e-5 PIT bar)."""
  eng, _ = _engine('NORMAL')
  worst = 0.0
  for p in W.PATTERNS:
    loc, sigma, _, w = W.normal_case(7, 257, p)
    x = _nq(eng, loc, sigma, weights=w)
    for i, q in enumerate(LEVELS):
      pit = _scores(eng, loc, S.normal_aux(sigma), x[i], weights=w, lpd=False, crps=False)['pit'][0]
      worst = max(worst, float(np.max(np.abs(pit - q))))
      assert np.all(np.abs(pit - q) <= 3e-5), (p, q)
  eng.close()
  print(f'pit at the weighted quantile: worst |pit - q| {worst:.2e} (bar 3e-05)')


# ----------------------------------------------------------------------------------------------------------- estimators
def _frames(golden_dir):
  """-> (the chickenpox fixture `fit` sees, the rows the weights are learned and checked on: every fourth row of it).  The
  fixture holds one location, so no row can be kept from `fit` (its constant columns would standardise to NaN) and the
  fixture's test rows lie eight years past it; tests/test_gpu_stacking.py stacks on the fitted table too."""
  df = pd.read_csv(os.path.join(golden_dir, 'chickenpox.8.train.csv'), index_col=0, parse_dates=['datetime'])
  return df, df.iloc[::4]


def test_estimator_map_counts(golden_dir):
  df, held = _frames(golden_dir)
  est = BayesianNeuralFieldMAP(**MODEL, observation_model='NB', compute_dtype='fp32').fit(
      df, seed=3, ensemble_size=4, num_epochs=20, learning_rate=0.01)
  st = est.stacking_weights(held)
  w = st['weights']
  assert w.shape == (1, 4)
  plain, sc = est.score(held, rps=True), est.score(held, rps=True, weights=w)
  assert set(sc) == set(plain) and sc['n'] == plain['n'] == len(held)
  assert _same(sc['member_log_prob'], plain['member_log_prob'])
  wl = est.weighted_log_density(held, w)
  e = S.rel1(sc['log_density'], wl['log_density'])
  print(f'MAP NB: weights {w.ravel()}, score(weights) vs weighted_log_density {e:.2e}; mean log density '
        f'{plain["mean_log_density"]:.5f} -> {sc["mean_log_density"]:.5f} (gap {st["gap"]:.1e}); mean rps '
        f'{plain["mean_rps"]:.4f} -> {sc["mean_rps"]:.4f}')
  assert e <= S.GATE
  assert sc['mean_log_density'] >= plain['mean_log_density'] - st['gap']
  assert sc['rps_capped'] == 0 and np.all(np.isfinite(sc['rps']))
  # the scores against the float64 references of the forecast likelihood_model reports
  lik = est.likelihood_model(held)
  R = len(held)
  y = held['chickenpox'].to_numpy(dtype=np.float64)
  fc = dict(tc=lik.total_count.reshape(-1, 1), logits=lik.logits.reshape(-1, R), pi=None)
  ref = W.count_ref(fc, y, w.reshape(-1))
  assert S.rel1(sc['log_density'], ref['lpd']) <= S.GATE and S.abs_err(sc['pit'], ref['pit']) <= S.PIT_BAR
  assert P.rel_err(sc['rps'], W.count_rps_ref(fc, y, w.reshape(-1))) <= S.GATE
  # predict: the quantiles of the weighted mixture, the per-member means untouched
  means0, q0 = est.predict(held, quantiles=LEVELS)
  means, q = est.predict(held, quantiles=LEVELS, weights=w)
  assert _same(means, means0) and len(q) == 3
  k = np.stack(q).astype(np.float64)
  assert np.all(k == np.round(k)) and np.all(k >= 0)
  for i, lev in enumerate(LEVELS):
    assert np.all(lik.mixture_cdf(k[i], weights=w) >= lev - QBAR)
    assert np.all((lik.mixture_cdf(np.maximum(k[i] - 1.0, 0.0), weights=w) <= lev + QBAR) | (k[i] == 0))
  hot = np.zeros((1, 4))
  hot[0, 2] = 1.0
  _, qh = est.predict(held, quantiles=LEVELS, weights=hot)
  own = lambda x: lik.cdf(x)[0, 2]
  for i, lev in enumerate(LEVELS):
    kh = qh[i].astype(np.float64)
    assert np.all(own(kh) >= lev - QBAR) and np.all((own(np.maximum(kh - 1.0, 0.0)) <= lev + QBAR) | (kh == 0))
  assert np.array_equal(lik.quantile(LEVELS, weights=w), k)
  # weights=None is the call without the keyword
  again = est.score(held, rps=True, weights=None)
  assert all(np.array_equal(again[key], plain[key], equal_nan=True) for key in plain)
  m2, q2 = est.predict(held, quantiles=LEVELS, weights=None)
  assert _same(m2, means0) and all(_same(a, b) for a, b in zip(q2, q0))
  with pytest.raises(ValueError, match='shape'):
    est.predict(held, weights=np.full(4, 0.25))
  with pytest.raises(ValueError, match='sum to 1'):
    est.score(held, weights=np.full((1, 4), 0.3))


def test_estimator_vi_normal(golden_dir):
  """The posterior draws count as components: weights (1, 5, 2), flattened in the order of member_log_prob."""
  df, held = _frames(golden_dir)
  est = BayesianNeuralFieldVI(**MODEL, observation_model='NORMAL', compute_dtype='fp32').fit(
      df, seed=1, ensemble_size=2, num_epochs=10, learning_rate=0.01, sample_size_posterior=5)
  st = est.stacking_weights(held, max_iter=2000)
  w = st['weights']
  assert w.shape == (1, 5, 2)
  plain, sc = est.score(held), est.score(held, weights=w)
  assert set(sc) == set(plain) == {'n', 'log_density', 'pit', 'crps', 'member_log_prob', 'mean_log_density', 'mean_crps'}
  assert _same(sc['member_log_prob'], plain['member_log_prob'])
  e = S.rel1(sc['log_density'], est.weighted_log_density(held, w)['log_density'])
  print(f'VI NORMAL: weights {w.ravel()}, score(weights) vs weighted_log_density {e:.2e}; mean log density '
        f'{plain["mean_log_density"]:.5f} -> {sc["mean_log_density"]:.5f} (gap {st["gap"]:.1e}); mean crps '
        f'{plain["mean_crps"]:.4f} -> {sc["mean_crps"]:.4f}')
  assert e <= S.GATE
  assert sc['mean_log_density'] >= plain['mean_log_density'] - st['gap']
  lik = est.likelihood_model(held)
  R = len(held)
  y = held['chickenpox'].to_numpy(dtype=np.float64)
  ref = W.normal_ref(lik.loc.reshape(-1, R), lik.scale.reshape(-1), y, w.reshape(-1))
  assert S.rel1(sc['log_density'], ref['lpd']) <= S.GATE and S.abs_err(sc['pit'], ref['pit']) <= S.PIT_BAR
  assert S.crps_err(sc['crps'], ref) <= S.GATE
  means0, _ = est.predict(held, quantiles=LEVELS)
  means, q = est.predict(held, quantiles=LEVELS, weights=w)
  assert _same(means, means0)
  for i, lev in enumerate(LEVELS):
    assert np.all(np.abs(lik.mixture_cdf(q[i].astype(np.float64), weights=w) - lev) <= QBAR)
  hot = np.zeros_like(w)
  hot[0, 3, 1] = 1.0
  _, qh = est.predict(held, quantiles=LEVELS, weights=hot)
  for i, lev in enumerate(LEVELS):
    assert np.all(np.abs(lik.cdf(qh[i].astype(np.float64))[0, 3, 1] - lev) <= QBAR)
  _, qa = est.predict(held, quantiles=LEVELS, approximate_quantiles=True, weights=w)
  want = W.normal_moment_quantile(lik.loc.reshape(-1, R), lik.scale.reshape(-1), float(np.float32(0.975)), w.reshape(-1))
  np.testing.assert_allclose(qa[2], want, rtol=1e-5, atol=0.0)
  np.testing.assert_allclose(lik.quantile(0.5, weights=w), q[1], rtol=0, atol=0)
  with pytest.raises(ValueError, match='shape'):
    est.predict(held, weights=w.reshape(5, 2))
  with pytest.raises(ValueError, match='shape'):
    est.score(held, weights=w.reshape(5, 2))
