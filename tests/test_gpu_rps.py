"""The ranked probability score of NB / ZINB forecasts on the GPU (include/bnf.h bnf_count_rps) against the brute-force
float64 reference of tests/rps_ref.py evaluated on the same float32 inputs.

Error |dev - ref| / |ref| (the score is strictly positive on every case); bar max(1e-5, 4 x the numpy restatement's own
error at that input) -- tests/test_rps_host.py prints the restatement's table: it stays under 3e-7 (the float32 rounding of
the result), so every bar here is the 1e-5 gate.  Every test prints what it measured (-s shows it)."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

from bayesnf_amd import BayesianNeuralFieldMAP
from bayesnf_amd.engine import Engine
from tests import rps_ref as P
from tests import scoring_ref as S
from tests import util
from tests.test_gpu_sampling import MODEL, TCS, count_case

pytestmark = pytest.mark.gpu


def _engine(obs, **kw):
  net, model, _, _ = util.make_problem(n_rows=16, width=64, depth=1, observation_model=obs)
  eng = Engine(net, members=1, forward_only=True, row_capacity=128, compute_dtype='fp32', **kw)
  eng.debug_poison_lds()
  return eng, model


def _rps(eng, loc, aux, y):
  dev = lambda a: torch.from_numpy(np.array(a, dtype=np.float32)).to(eng.device)       # (a copy: the shared cases are read-only)
  out = eng.count_rps(dev(loc), dev(aux), dev(y))
  assert out.shape == (len(y),) and out.dtype == torch.float32
  return out.cpu().numpy()


def _check(tag, got, ref, f64):
  rest, err = P.rel_err(f64, ref), P.rel_err(got, ref)
  print(f'{tag} device {err:.2e} (restatement {rest:.1e}, bar {P.bar(rest):.0e})')
  assert err <= P.bar(rest), (tag, err, P.bar(rest))
  return err


@pytest.mark.parametrize('M', [1, 7])
@pytest.mark.parametrize('obs', ['NB', 'ZINB'])
def test_grid_at_real_data_scale(obs, M):
  """total_count 0.05 .. 1e3 x mean 0.02 .. 400, every row at y = 0, 1, round(mean), round(mean + 3 sd): 20 rows per
  point.  The longest window of the grid (M = 7, total_count 0.05, mean 400) is 3e5 terms, under the cap: every row is
  finite.  LDS poisoned before every call."""
  eng, _ = _engine(obs)
  for tc in TCS:
    loc, aux, y, ref, f64, terms = P.grid_case(obs, tc, M)
    eng.debug_poison_lds()
    got = _rps(eng, loc, aux, y)
    assert np.all(np.isfinite(got)) and np.all(got > 0), (tc, got)
    _check(f'{obs} M={M} tc={tc:g} (longest window {terms.max()}):', got, ref, f64)
  eng.close()


@pytest.mark.parametrize('obs', ['NB', 'ZINB'])
def test_member_chunks_and_rows_with_a_remainder(obs):
  """70 components (one chunk of 64 and one of 6) x 65 rows."""
  eng, model = _engine(obs)
  loc, aux, y = P.many_member_case(obs)
  assert loc.shape == (70, 65)
  ref = P.count_rps_ref(P.forecast(model, loc, aux), y)
  f64, _, _ = P.count_rps_f64(loc, aux, y, obs)
  got = _rps(eng, loc, aux, y)
  eng.close()
  assert np.all(np.isfinite(got))
  _check(f'{obs} M=70 R=65:', got, ref, f64)


@pytest.mark.parametrize('obs', ['NB', 'ZINB'])
def test_closed_form_terms_and_rows_that_are_not_counts(obs):
  """Mean 400 at total_count 1e3, 7 members: y = 0 under a window that starts above 0, y more than 1,000 above the window's
  end, and y NaN / negative / not an integer -- NaN there, the neighbours bit for bit what they are without those rows."""
  eng, model = _engine(obs)
  loc7, aux, _ = count_case(model, 1e3, 7)
  y = np.asarray([0.0, 5000.0, 400.0, np.nan, 400.0, -1.0, 2.5, 400.0, np.inf, 431.0], dtype=np.float32)
  loc = np.tile(loc7[:, 4:5], (1, len(y)))
  f64, terms, starts = P.count_rps_f64(loc, aux, y, obs)
  assert starts[0] > 0 and starts[1] + terms[1] + 1000 <= y[1]
  ref = P.count_rps_ref(P.forecast(model, loc, aux), y)
  got = _rps(eng, loc, aux, y)
  keep = np.asarray([0, 1, 2, 4, 7, 9])
  assert np.array_equal(np.isnan(got), ~np.isin(np.arange(len(y)), keep))
  _check(f'{obs} edges:', got, ref, f64)
  alone = _rps(eng, loc[:, keep], aux, y[keep])
  eng.close()
  assert np.array_equal(alone.view(np.int32), got[keep].view(np.int32))


def test_the_cap_is_nan_and_leaves_the_other_rows_alone():
  """Mean 1e6 at total_count 0.05 needs 3e8 terms: NaN, in the restatement too; the other rows of the call keep their bits."""
  eng, model = _engine('NB')
  loc7, aux, _ = count_case(model, 0.05, 1)
  loc = loc7[:, [0, 1, 2, 3, 4, 6]]
  y = np.asarray([0.0, 1.0, 5.0, 30.0, 400.0, 1e6], dtype=np.float32)
  f64, terms, _ = P.count_rps_f64(loc, aux, y, 'NB')
  assert np.isnan(f64[5]) and terms[5] == -1 and np.all(np.isfinite(f64[:5]))
  got = _rps(eng, loc, aux, y)
  without = _rps(eng, loc[:, :5], aux, y[:5])
  eng.close()
  assert np.isnan(got[5]) and np.all(np.isfinite(got[:5]))
  assert np.array_equal(got[:5].view(np.int32), without.view(np.int32))
  ref = P.count_rps_ref(P.forecast(model, loc[:, :5], aux), y[:5])
  _check('NB beside the capped row:', got[:5], ref, f64[:5])


def test_two_calls_give_the_same_bits_and_a_training_handle_works():
  loc, aux, y = P.many_member_case('ZINB')
  eng, _ = _engine('ZINB')
  a = _rps(eng, loc, aux, y)
  eng.debug_poison_lds()
  b = _rps(eng, loc, aux, y)
  eng.close()
  assert np.array_equal(a.view(np.int32), b.view(np.int32))
  net, _, X, yt = util.make_problem(n_rows=64, width=64, depth=1, observation_model='ZINB')
  full = Engine(net, X=X, y=yt, members=2, compute_dtype='fp32')              # not forward-only
  c = _rps(full, loc, aux, y)
  full.close()
  assert np.array_equal(a.view(np.int32), c.view(np.int32))


def test_a_normal_handle_and_bad_shapes_are_refused():
  eng, _ = _engine('NORMAL')
  loc, aux, y = P.many_member_case('NB', M=3, R=5)
  with pytest.raises(ValueError, match='count observation models'):
    _rps(eng, loc, aux, y)
  eng.close()
  eng, _ = _engine('NB')
  with pytest.raises(ValueError, match='one observation per row'):
    eng.count_rps(torch.from_numpy(loc).to(eng.device), torch.from_numpy(aux).to(eng.device), y[:4])
  big = np.zeros((2049, 1), dtype=np.float32)
  with pytest.raises(ValueError, match='at most 2048'):
    _rps(eng, big, np.ones((2049, 3), dtype=np.float32), np.zeros(1, dtype=np.float32))
  eng.close()


def _frame(golden_dir):
  return pd.read_csv(os.path.join(golden_dir, 'chickenpox.8.train.csv'), index_col=0, parse_dates=['datetime'])


def test_estimator_score_with_rps(golden_dir):
  """A small NB fit on the chickenpox fixture: score(df, rps=True) adds 'rps', 'mean_rps', 'rps_capped' == 0 and matches the
  reference computed from likelihood_model(df); score(df) has today's keys; NaN targets are NaN rows outside the mean."""
  df = _frame(golden_dir)
  est = BayesianNeuralFieldMAP(**MODEL, observation_model='NB', compute_dtype='fp32').fit(
      df, seed=3, ensemble_size=4, num_epochs=5, learning_rate=0.01)
  R = len(df)
  plain = est.score(df)
  assert set(plain) == {'n', 'log_density', 'pit', 'member_log_prob', 'mean_log_density'}
  res = est.score(df, rps=True)
  assert set(res) == set(plain) | {'rps', 'mean_rps', 'rps_capped'}
  for k in ('log_density', 'pit', 'member_log_prob'):
    assert np.array_equal(res[k], plain[k]), k
  assert res['rps'].shape == (R,) and res['rps'].dtype == np.float32 and res['rps_capped'] == 0
  lik = est.likelihood_model(df)
  y = df['chickenpox'].to_numpy(dtype=np.float64)
  ref = P.count_rps_ref(dict(tc=lik.total_count.reshape(-1, 1), logits=lik.logits.reshape(-1, R), pi=None), y)
  err = P.rel_err(res['rps'], ref)
  print(f'MAP NB: rps {err:.2e}; mean rps {res["mean_rps"]:.4f}')
  assert err <= S.GATE
  assert abs(res['mean_rps'] - ref.mean()) <= S.GATE * ref.mean()
  d = df.copy()
  d.loc[d.index[[1, 5]], 'chickenpox'] = np.nan
  res2 = est.score(d, rps=True)
  keep = np.ones(R, dtype=bool)
  keep[[1, 5]] = False
  assert np.array_equal(np.isnan(res2['rps']), ~keep) and res2['rps_capped'] == 0 and res2['n'] == R - 2
  assert np.array_equal(res2['rps'][keep], res['rps'][keep])
  assert abs(res2['mean_rps'] - ref[keep].mean()) <= S.GATE * ref[keep].mean()


def test_estimator_rps_on_a_normal_model_raises(golden_dir):
  df = _frame(golden_dir)
  est = BayesianNeuralFieldMAP(**MODEL, observation_model='NORMAL', compute_dtype='fp32').fit(
      df, seed=1, ensemble_size=2, num_epochs=2, learning_rate=0.01)
  with pytest.raises(ValueError, match="'crps'"):
    est.score(df, rps=True)
  assert 'rps' not in est.score(df)
