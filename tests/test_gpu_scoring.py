"""Held-out observations scored on the GPU (include/bnf.h bnf_predictive_scores) against the float64 references of
tests/scoring_ref.py evaluated on the same float32 inputs.

Bars (none tuned on the code under test; tests/scoring_ref.py): lpd and member_ll max(1e-5, 4 x the float32 restatement's
own error at that input) of |dev - ref| / max(1, |ref|); pit 1e-5 absolute; crps the same max(1e-5, 4 x) rule relative to
the first term of the reference.  tests/test_scoring_host.py prints the restatement's table: it stays under 6e-7, so
every bar here is the 1e-5 gate.

Every test prints the errors it measured next to the restatement's and the bar (-s shows them).
"""
import ctypes as C
import os

import numpy as np
import pandas as pd
import pytest
import torch

from bayesnf_amd import BayesianNeuralFieldMAP, BayesianNeuralFieldVI, _native
from bayesnf_amd.engine import Engine
from oracle import bnf_oracle as O
from tests import scoring_ref as S
from tests import util
from tests.test_gpu_sampling import MODEL, TCS

pytestmark = pytest.mark.gpu


def _engine(obs):
  net, model, _, _ = util.make_problem(n_rows=16, width=64, depth=1, observation_model=obs)
  eng = Engine(net, members=1, forward_only=True, row_capacity=128, compute_dtype='fp32')
  eng.debug_poison_lds()
  return eng, model


def _dev(eng, a):
  return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(eng.device)


def _scores(eng, loc, aux, y, **kw):
  out = eng.predictive_scores(_dev(eng, loc), _dev(eng, aux), _dev(eng, y), **kw)
  return {k: v.cpu().numpy() for k, v in out.items()}


def _check(tag, got, ref, f32, crps=True):
  """Every output against the reference, each under its bar; returns the measured errors."""
  rest = S.restatement_errors(ref, f32)
  errs = dict(lpd=S.rel1(got['lpd'], ref['lpd']), member_ll=S.rel1(got['member_ll'], ref['member_ll']),
              pit=S.abs_err(got['pit'], ref['pit']))
  bars = dict(lpd=S.bar(rest['lpd']), member_ll=S.bar(rest['member_ll']), pit=S.PIT_BAR)
  if crps:
    errs['crps'], bars['crps'] = S.crps_err(got['crps'], ref), S.bar(rest['crps'])
  print(tag, ' '.join(f'{k} {v:.2e} (f32 {rest[k]:.1e}, bar {bars[k]:.0e})' for k, v in errs.items()))
  for k, v in errs.items():
    assert v <= bars[k], (tag, k, v, bars[k])
  return errs


ROWS = (1, 63, 64, 65, S.ROW_TILE + 1)


@pytest.mark.parametrize('M', [1, 2, 7, S.MEMBER_CHUNK + 1, 2 * S.MEMBER_CHUNK + 4, 1033])
def test_edge_shapes_normal(M):
  """(a) NORMAL, random loc, per-member sigma in [0.01, 3], all four outputs.  Rows 1, 63, 64, 65 and one more than the
  1024-row tile; members 1, 2, 7, one more than the 8-member chunk, 20 (three chunks: the middle one is its own partner,
  the last is short) and 1033 (130 chunks = 65 slots, one more than the 64 blocks they round-robin over; last chunk of one
  member; 5 rows only)."""
  eng, _ = _engine('NORMAL')
  for R in ((5,) if M > 1000 else ROWS):
    loc, sigma, y = S.normal_case(M, R)
    got = _scores(eng, loc, S.normal_aux(sigma), y)
    assert got['member_ll'].shape == (M,) and got['member_ll'].dtype == np.float64
    assert got['lpd'].shape == (R,) and got['pit'].shape == (2, R) and got['crps'].shape == (R,)
    assert np.array_equal(got['pit'][0], got['pit'][1])
    assert np.all(got['crps'] > 0)
    _check(f'NORMAL M={M} R={R}:', got, S.normal_ref(loc, sigma, y), S.normal_f32(loc, sigma, y))
  eng.close()


def test_outputs_are_optional_and_the_work_buffer_is_checked():
  """Each output alone gives what the full call gives; a short work buffer, no rows and no members are BNF_ERR_INVALID."""
  eng, _ = _engine('NORMAL')
  loc, sigma, y = S.normal_case(9, 65)
  aux = S.normal_aux(sigma)
  full = _scores(eng, loc, aux, y)
  for only in ('member_ll', 'lpd', 'pit', 'crps'):
    kw = dict(member_ll=False, lpd=False, pit=False, crps=False)
    kw[only] = True
    part = _scores(eng, loc, aux, y, **kw)
    assert list(part) == [only] and np.array_equal(part[only], full[only]), only
  loc_d, aux_d, y_d = _dev(eng, loc), _dev(eng, aux), _dev(eng, y)
  ll = torch.empty(9, dtype=torch.float64, device=eng.device)
  crps = torch.empty(65, dtype=torch.float32, device=eng.device)
  work = torch.empty(9 + 65, dtype=torch.float64, device=eng.device)      # 9 members x 1 tile + 65 rows x 1 slot
  p = lambda t: C.c_void_p(t.data_ptr())
  call = lambda M, R, nbytes: eng.lib.bnf_predictive_scores(eng.handle, p(loc_d), p(aux_d), M, R, p(y_d), p(work),
                                                            C.c_size_t(nbytes), p(ll), None, None, p(crps))
  assert call(9, 65, 8 * (9 + 65)) == 0
  torch.cuda.synchronize()
  assert np.array_equal(ll.cpu().numpy(), full['member_ll']) and np.array_equal(crps.cpu().numpy(), full['crps'])
  for M, R, nbytes in ((9, 65, 8 * (9 + 65) - 1), (0, 65, 1 << 20), (9, 0, 1 << 20)):
    assert call(M, R, nbytes) == -1, (M, R, nbytes)
  assert 'work buffer' in _native.last_error() or 'argument' in _native.last_error()
  eng.close()


@pytest.mark.parametrize('M', [1, 7])
def test_tails_and_nan_rows(M):
  """(b) |y - mu_m| / sigma_m = 40 for every member: every density is e^-800, log(mean(exp)) is -inf in float32 and
  float64; lpd must be finite, about -800, and within bar.  Rows with a NaN y: NaN in every per-row output, left out of
  member_ll."""
  eng, _ = _engine('NORMAL')
  loc, sigma, y = S.tail_case(M)
  y = y.copy()
  y[[0, 17, 64, 95]] = np.nan
  got = _scores(eng, loc, S.normal_aux(sigma), y)
  ref = S.normal_ref(loc, sigma, y)
  keep = np.isfinite(y)
  assert np.all(np.isfinite(got['lpd'][keep])) and got['lpd'][keep].max() < -700
  for k in ('lpd', 'crps'):
    assert np.array_equal(np.isnan(got[k]), ~keep), k
  assert np.array_equal(np.isnan(got['pit']), np.stack([~keep, ~keep]))
  assert np.all(np.isfinite(got['member_ll']))
  _check(f'tails M={M}:', got, ref, S.normal_f32(loc, sigma, y))
  # member_ll without the NaN rows at all: the same sums
  alone = _scores(eng, loc[:, keep], S.normal_aux(sigma), y[keep])
  assert S.rel1(alone['member_ll'], got['member_ll']) <= 1e-12
  eng.close()


@pytest.mark.parametrize('M', [1, 7])
@pytest.mark.parametrize('obs', ['NB', 'ZINB'])
def test_counts_at_real_data_scale(obs, M):
  """(c) the grid of tests/test_gpu_sampling.py (total_count 0.05 .. 1e3 x mean 0.02 .. 1e6), every row at y = 0, 1,
  round(mean), round(mean + 3 sd) (capped at 2^24): lpd, pit and member_ll against the oracle; pit[1] == 0 exactly at
  y = 0; crps on a count handle is BNF_ERR_INVALID."""
  eng, _ = _engine(obs)
  for tc in TCS:
    loc, aux, y, ref, f32 = S.count_grid_case(obs, tc, M)
    got = _scores(eng, loc, aux, y)
    assert 'crps' not in got
    assert np.all(got['pit'][1][y == 0] == 0.0)
    assert np.all(got['pit'][0] >= got['pit'][1]) and np.all(got['pit'][0] <= 1.0)
    _check(f'{obs} M={M} tc={tc:g}:', got, ref, f32, crps=False)
  with pytest.raises(ValueError, match='crps'):
    _scores(eng, loc, aux, y, crps=True)
  # a NaN row among counts
  y2 = np.array(y)
  y2[3] = np.nan
  got = _scores(eng, loc, aux, y2)
  assert np.isnan(got['lpd'][3]) and np.all(np.isnan(got['pit'][:, 3])) and np.isnan(got['lpd']).sum() == 1
  eng.close()


@pytest.mark.parametrize('obs', ['NORMAL', 'NB', 'ZINB'])
def test_held_out_likelihood_agrees_with_the_training_loss(obs):
  """(d) MLE engine (prior_weight 0, full batch): the step loss of debug_loss_and_grad against -member_ll of the same
  parameters on the same rows (forward + predictive_scores on a forward-only handle), normalised as the oracle's map_loss
  does: -(loglik x n_total / batch) with no prior term.  Within FP32_GATE['loss'] relative."""
  n_rows, E = 300, 3
  net, model, X, y = util.make_problem(n_rows=n_rows, width=64, depth=2, observation_model=obs)
  theta = util.random_theta(model, E, scale=0.3)
  eng = Engine(net, X=X, y=y, members=E, prior_weight=0.0, compute_dtype='fp32')
  eng.set_params(theta)
  loss, _ = eng.debug_loss_and_grad()
  c = eng.n_rows / eng.batch                     # map_loss: c = n_total / y.shape[-1]
  assert c == 1.0
  eng.close()
  fwd = Engine(net, members=E, forward_only=True, row_capacity=n_rows, compute_dtype='fp32')
  fwd.debug_poison_lds()
  loc, aux = fwd.forward(_dev(fwd, theta), _dev(fwd, X))
  ll = fwd.predictive_scores(loc, aux, _dev(fwd, y), lpd=False, pit=False, crps=False)['member_ll'].cpu().numpy()
  fwd.close()
  want = O.map_loss(model, theta, X, y, n_total=n_rows, prior_weight=0.0)
  err = np.abs(-ll * c - loss) / np.abs(loss)
  print(f'{obs}: step loss {loss}, -member_ll {-ll}, oracle {want}, rel err {err.max():.2e}')
  assert np.all(err <= util.FP32_GATE['loss']), err
  assert np.all(np.abs(-ll * c - want) / np.abs(want) <= util.FP32_GATE['loss'])


def test_two_calls_give_the_same_bits():
  """(e) member_ll and crps (every sum in an order the shapes fix, no float atomics), lpd and pit too."""
  eng, _ = _engine('NORMAL')
  loc, sigma, y = S.normal_case(64, 2 * S.ROW_TILE + 1)
  a = _scores(eng, loc, S.normal_aux(sigma), y)
  eng.debug_poison_lds()
  b = _scores(eng, loc, S.normal_aux(sigma), y)
  eng.close()
  assert np.array_equal(a['member_ll'].view(np.int64), b['member_ll'].view(np.int64))
  for k in ('crps', 'lpd', 'pit'):
    assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k


def _frame(golden_dir):
  return pd.read_csv(os.path.join(golden_dir, 'chickenpox.8.train.csv'), index_col=0, parse_dates=['datetime'])


def test_estimator_score_map_counts(golden_dir):
  """(f) NB MAP fit on the chickenpox fixture: keys and shapes, member_log_prob against likelihood_model(df).log_prob(y),
  log_density / pit against the host mixture, NaN targets as NaN rows, ValueError before fit and for non-integer targets."""
  df = _frame(golden_dir)
  est = BayesianNeuralFieldMAP(**MODEL, observation_model='NB', compute_dtype='fp32')
  with pytest.raises(ValueError, match='before fit'):
    est.score(df)
  est.fit(df, seed=3, ensemble_size=4, num_epochs=20, learning_rate=0.01)
  R = len(df)
  res = est.score(df)
  assert set(res) == {'n', 'log_density', 'pit', 'member_log_prob', 'mean_log_density'}
  assert res['n'] == R and res['log_density'].shape == (R,) and res['pit'].shape == (2, R)
  lik = est.likelihood_model(df)
  y = df['chickenpox'].to_numpy(dtype=np.float64)
  want = lik.log_prob(y)
  assert res['member_log_prob'].shape == want.shape == (1, 4)
  fc = dict(tc=lik.total_count.reshape(-1, 1), logits=lik.logits.reshape(-1, R), pi=None)
  ref = S.count_ref(fc, y)
  e = (S.rel1(res['member_log_prob'], want), S.rel1(res['log_density'], ref['lpd']), S.abs_err(res['pit'], ref['pit']))
  print(f'MAP NB: member_log_prob {e[0]:.2e}, log_density {e[1]:.2e}, pit {e[2]:.2e}; mean log density {res["mean_log_density"]:.4f}')
  assert e[0] <= S.GATE and e[1] <= S.GATE and e[2] <= S.PIT_BAR
  assert abs(res['mean_log_density'] - ref['lpd'].mean()) <= S.GATE * max(1.0, abs(ref['lpd'].mean()))
  assert np.all(res['pit'][1] <= res['pit'][0]) and np.all(res['pit'][1][y == 0] == 0.0)
  # NaN targets: NaN rows, left out of the sums and the means
  d = df.copy()
  gone = [1, 5, R - 1]
  d.loc[d.index[gone], 'chickenpox'] = np.nan
  res2 = est.score(d)
  keep = np.ones(R, dtype=bool)
  keep[gone] = False
  assert res2['n'] == R - 3 and np.array_equal(np.isnan(res2['log_density']), ~keep)
  assert np.array_equal(np.isnan(res2['pit']), np.stack([~keep, ~keep]))
  assert np.array_equal(res2['log_density'][keep], res['log_density'][keep])
  assert S.rel1(res2['member_log_prob'], S.count_ref(fc, np.where(keep, y, np.nan))['member_ll'].reshape(1, 4)) <= S.GATE
  assert abs(res2['mean_log_density'] - ref['lpd'][keep].mean()) <= S.GATE * max(1.0, abs(ref['lpd'][keep].mean()))
  d.loc[d.index[2], 'chickenpox'] = 2.5
  with pytest.raises(ValueError, match='non-negative integer'):
    est.score(d)
  with pytest.raises(ValueError, match='target column'):
    est.score(df.drop(columns='chickenpox'))


def test_estimator_score_vi_normal(golden_dir):
  """(f) NORMAL VI fit: the posterior draws count as components (member_log_prob has the extra dim), crps and mean_crps are
  there."""
  df = _frame(golden_dir)
  est = BayesianNeuralFieldVI(**MODEL, observation_model='NORMAL', compute_dtype='fp32').fit(
      df, seed=1, ensemble_size=2, num_epochs=10, learning_rate=0.01, sample_size_posterior=5)
  R = len(df)
  res = est.score(df)
  assert set(res) == {'n', 'log_density', 'pit', 'crps', 'member_log_prob', 'mean_log_density', 'mean_crps'}
  lik = est.likelihood_model(df)
  y = df['chickenpox'].to_numpy(dtype=np.float64)
  want = lik.log_prob(y)
  assert res['member_log_prob'].shape == want.shape == (1, 5, 2)
  assert res['crps'].shape == (R,) and res['n'] == R
  ref = S.normal_ref(lik.loc.reshape(-1, R), lik.scale.reshape(-1), y)
  e = (S.rel1(res['member_log_prob'], want), S.rel1(res['log_density'], ref['lpd']), S.abs_err(res['pit'], ref['pit']),
       S.crps_err(res['crps'], ref))
  print(f'VI NORMAL: member_log_prob {e[0]:.2e}, log_density {e[1]:.2e}, pit {e[2]:.2e}, crps {e[3]:.2e}; '
        f'mean crps {res["mean_crps"]:.4f}')
  assert e[0] <= S.GATE and e[1] <= S.GATE and e[2] <= S.PIT_BAR and e[3] <= S.GATE
  assert abs(res['mean_crps'] - ref['crps'].mean()) <= S.GATE * ref['crps_first'].mean()
