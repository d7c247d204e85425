"""CPU-only checks of the held-out validation during a fit (include/bnf.h bnf_validation_check; inference.fit_map
validation=...; BayesianNeuralFieldMAP.fit validation=...): the entry point's declaration, export and refusal without a
device; the estimator's checks, which fire before any engine is created; the schedule of segments and checks a recording
stand-in engine sees on all three shuffle paths, and the untouched call sequence of validation=None; the numpy
restatement of the decision rule (tests/validation_ref.py) against hand-worked cases."""
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

from bayesnf_amd import BayesianNeuralFieldMAP, BayesianNeuralFieldMLE, BayesianNeuralFieldVI, _native, inference
from tests import validation_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_declared_listed_and_exported():
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'bnf.h')).read(), flags=re.S)
  lib = _native.load()
  assert re.search(r'\bint\s+bnf_validation_check\s*\(', src), 'bnf_validation_check is not declared in include/bnf.h'
  assert 'bnf_validation_check' in _native.EXPORTS
  fn = lib.bnf_validation_check
  assert fn.argtypes is not None and len(fn.argtypes) == 11
  assert _native.ABI_VERSION == 6 and lib.bnf_abi_version() == 6          # purely additive
  from bayesnf_amd.engine import Engine
  assert callable(getattr(Engine, 'validation_check', None))


@pytest.mark.skipif(torch.cuda.is_available(), reason='checks the no-GPU failure mode')
def test_the_entry_point_refuses_without_a_device():
  lib = _native.load()
  assert lib.bnf_validation_check(None, None, 1, 0, 0, 1, None, None, None, None, None) == -2
  assert 'no CPU fallback' in _native.last_error()


# ---- the decision rule ------------------------------------------------------------------------------------------------
def test_the_rule_on_hand_worked_cases():
  names = list(V.COLUMNS)
  res = V.run(V.columns(names), V.N_SCORED, V.EPOCHS)
  for m, name in enumerate(names):
    col = np.asarray(V.COLUMNS[name])
    assert tuple(res['keep'][:, m]) == V.HAND_KEEP[name], name
    c = V.HAND_BEST_CHECK[name]
    assert res['best_check'][m] == c and res['best_epoch'][m] == V.EPOCHS[c], name
    want = col[c] / 7.0
    assert res['best_score'][m] == want or (np.isnan(want) and np.isnan(res['best_score'][m])), name
  assert np.array_equal(res['curve'], V.columns(names).T / 7.0, equal_nan=True)
  # single comparisons: a tie keeps the earlier epoch, a NaN never replaces a number, -inf never replaces -inf, anything
  # replaces a NaN but a NaN, and check 0 keeps whatever comes
  inf = float('inf')
  for check, score, best, want in ((1, -1.0, -1.0, False), (1, V.NAN, -1.0, False), (1, -inf, -inf, False),
                                   (1, -1.0, V.NAN, True), (1, -inf, V.NAN, True), (1, V.NAN, V.NAN, False),
                                   (1, -1.0, -inf, True), (3, -0.5, -1.0, True), (3, -1.5, -1.0, False),
                                   (0, V.NAN, 5.0, True), (0, -inf, 5.0, True), (0, -9.0, 5.0, True)):
    assert V.keeps(check, score, best) is want, (check, score, best)
  best, ep = V.best_of_curve([[-3.0, -1.0, -1.0], [V.NAN, V.NAN, -2.0], [V.NAN, V.NAN, V.NAN]], (4, 8, 9))
  assert best[0] == -1.0 and best[1] == -2.0 and np.isnan(best[2]) and tuple(ep) == (8, 9, 4)


def test_the_check_epochs():
  assert inference.validation_epochs(12, 5) == [5, 10, 12]
  assert inference.validation_epochs(20, 7) == [7, 14, 20]
  assert inference.validation_epochs(10, 5) == [5, 10]
  assert inference.validation_epochs(3, 10) == [3]
  assert inference.validation_epochs(4, 1) == [1, 2, 3, 4]


# ---- the estimator's checks fire before any GPU work ----------------------------------------------------------------------
def _frame(n_t=4):
  t = pd.date_range('2020-01-06', periods=n_t, freq='W-MON')
  return pd.DataFrame({'t': np.repeat(t, 3), 'place': np.tile(['a', 'b', 'c'], n_t), 'y': np.arange(3.0 * n_t)})


@pytest.mark.parametrize('cls', [BayesianNeuralFieldMAP, BayesianNeuralFieldMLE])
def test_fit_checks_the_validation_table_before_any_gpu_work(cls, monkeypatch):
  def no_gpu(*a, **k):
    raise AssertionError('GPU work was reached')
  monkeypatch.setattr(inference, 'Engine', no_gpu)
  df, val = _frame(), _frame(3)
  est = cls(feature_cols=['t'], target_col='y', freq='W', width=64, observation_model='NB')
  fit = lambda v, **kw: est.fit(df, seed=1, ensemble_size=2, num_epochs=3, validation=v, **kw)
  with pytest.raises(ValueError, match='target column'):
    fit(val.drop(columns='y'))
  bad = val.copy()
  bad.loc[2, 'y'] = np.inf
  with pytest.raises(ValueError, match='infinite'):
    fit(bad)
  bad.loc[2, 'y'] = 2.5
  with pytest.raises(ValueError, match='non-negative integer'):
    fit(bad)
  bad['y'] = np.nan
  with pytest.raises(ValueError, match='no row with a finite target'):
    fit(bad)
  for every in (0, -3, 2.5, 2.0, '5', True):
    with pytest.raises(ValueError, match='validation_every'):
      fit(val, validation_every=every)
  ok = val.copy()
  ok.loc[2, 'y'] = np.nan                              # a NaN target is no error: it reaches the GPU seam
  for kw in ({}, {'validation_every': 2}, {'validation_every': np.int64(1), 'restore_best': False}):
    with pytest.raises(AssertionError, match='GPU work'):
      fit(ok, **kw)
  assert est.validation_ is None


def test_vi_fit_does_not_take_the_keyword():
  est = BayesianNeuralFieldVI(feature_cols=['t'], target_col='y', freq='W', width=64, observation_model='NORMAL')
  with pytest.raises(TypeError, match='validation'):
    est.fit(_frame(), seed=1, ensemble_size=2, num_epochs=3, validation=_frame(3))


# ---- the schedule a recording engine sees ------------------------------------------------------------------------------------
KW = dict(width=64, depth=1, input_scales=[9.0, 1.0], fourier_degrees=[2, 0], interactions=[[0, 1]],
          seasonality_periods=[], num_seasonal_harmonics=[])


class RecordingEngine:
  """Stands where `inference.Engine` stands and writes down what is asked of it.  A check scores -|epoch - 10|: the best
  check is the one after epoch 10."""
  log = []

  def __init__(self, net, *, mode='map', members=1, forward_only=False, row_capacity=None, device_index=None, **_):
    self.net, self.members, self.forward_only = net, int(members), bool(forward_only)
    self.device = torch.device('cpu')
    self.params = None if forward_only else torch.zeros(self.members * net.P)
    self.epoch = 0
    RecordingEngine.log.append(('forward_engine', self.members, row_capacity) if forward_only else ('engine', self.members))

  def init_params_keys(self, leaf_keys, log_noise_init):
    pass

  def init_params(self, log_noise_init):
    pass

  def set_row_keys(self, subkeys, epoch0=0):
    RecordingEngine.log.append(('row_keys', epoch0, int(np.asarray(subkeys).shape[0])))

  def set_row_tables(self, tables, epoch0=0):
    RecordingEngine.log.append(('row_tables', epoch0, int(np.asarray(tables).shape[0])))

  def train(self, epoch0, n):
    RecordingEngine.log.append(('train', epoch0, n))
    self.epoch = epoch0 + n
    self.params += float(n)                                     # in place: the forward engine reads this very tensor
    return torch.arange(epoch0, epoch0 + n, dtype=torch.float32).repeat(self.members, 1)

  def forward(self, theta, X):
    assert self.forward_only
    RecordingEngine.log.append(('forward', tuple(theta.shape), tuple(X.shape), float(theta[0, 0])))
    return torch.zeros((theta.shape[0], X.shape[0])), torch.zeros((theta.shape[0], 3))

  def predictive_scores(self, loc, aux, y, crps=None, member_ll=True, lpd=True, pit=True, weights=None, into=None):
    assert self.forward_only and member_ll and not (crps or lpd or pit) and weights is None and into is not None
    RecordingEngine.log.append(('scores', tuple(y.shape)))
    return {'member_ll': into['member_ll']}

  def validation_check(self, member_ll, n_scored, epoch, check, n_checks, curve, best_score, best_epoch, keep, best_params):
    assert not self.forward_only and epoch == self.epoch
    RecordingEngine.log.append(('check', epoch, check, n_checks, n_scored))
    score = -abs(epoch - 10.0)
    curve[:, check] = score
    if check == 0 or score > float(best_score[0]):
      best_score[:] = score
      best_epoch[:] = epoch
      best_params.copy_(self.params.view(self.members, -1))

  def close(self):
    RecordingEngine.log.append(('close', self.forward_only))


def _problem():
  rng = np.random.default_rng(0)
  X = np.stack([rng.integers(0, 10, 40).astype(float), rng.standard_normal(40)], axis=1)
  y = np.sin(X[:, 0]) + X[:, 1] + 0.1 * rng.standard_normal(40)
  return X, y


@pytest.fixture
def recorder(monkeypatch):
  monkeypatch.setattr(inference, 'Engine', RecordingEngine)
  monkeypatch.delenv('BNF_DEVICES', raising=False)
  monkeypatch.delenv('BNF_ROW_TABLES', raising=False)
  del RecordingEngine.log[:]
  return RecordingEngine


def _calls(log, *kinds):
  return [e for e in log if e[0] in kinds]


@pytest.mark.parametrize('path', ['full', 'keys', 'host'])
def test_segments_and_checks_in_order(recorder, monkeypatch, path):
  X, y = _problem()
  Xv, yv = X[:9] + 0.5, y[:9].copy()
  yv[4] = np.nan
  bs = None if path == 'full' else 16
  if path == 'host':
    monkeypatch.setenv('BNF_ROW_TABLES', 'host')
  params, losses, info = inference.fit_map(X, y, 7, 'NORMAL', dict(KW), num_particles=3, learning_rate=0.01, num_epochs=12,
                                           batch_size=bs, validation=(Xv, yv, 5, True))
  log, P = recorder.log, inference._net_from_args(dict(KW), 'NORMAL').P
  assert _calls(log, 'train', 'check') == [('train', 0, 5), ('check', 5, 0, 3, 8), ('train', 5, 5), ('check', 10, 1, 3, 8),
                                           ('train', 10, 2), ('check', 12, 2, 3, 8)]
  # every check is forward -> scores -> check, on the one forward-only engine, reading the training parameters in place
  assert _calls(log, 'engine', 'forward_engine') == [('engine', 3), ('forward_engine', 3, 9)]
  order = [e[0] for e in log if e[0] in ('train', 'forward', 'scores', 'check')]
  assert order == ['train', 'forward', 'scores', 'check'] * 3
  assert [e[3] for e in _calls(log, 'forward')] == [5.0, 10.0, 12.0] and _calls(log, 'forward')[0][1:3] == ((3, P), (9, 2))
  assert _calls(log, 'scores') == [('scores', (9,))] * 3
  assert _calls(log, 'row_keys') == ([('row_keys', 0, 12)] if path == 'keys' else [])
  assert _calls(log, 'row_tables') == ([('row_tables', 0, 12)] if path == 'host' else [])
  assert sorted(_calls(log, 'close')) == [('close', False), ('close', True)]
  # what comes back: the loss pieces joined, the curve, and each member at its best epoch
  assert losses.shape == (1, 3, 12) and np.array_equal(losses[0, 0], np.arange(12.0))
  assert set(info) == {'epochs', 'member_log_density', 'best', 'best_epoch', 'n', 'restored'}
  assert info['epochs'].tolist() == [5, 10, 12] and info['n'] == 8 and info['restored'] is True
  assert info['member_log_density'].shape == (1, 3, 3) and info['member_log_density'].dtype == np.float64
  assert np.array_equal(info['member_log_density'][0, 1], [-5.0, 0.0, -2.0])
  assert np.array_equal(info['best'], np.zeros((1, 3))) and np.array_equal(info['best_epoch'], np.full((1, 3), 10))
  theta = inference._flatten_struct(inference._net_from_args(dict(KW), 'NORMAL'), params)
  assert theta.shape == (1, 3, P) and np.all(theta == 10.0)
  del log[:]
  params, _, info = inference.fit_map(X, y, 7, 'NORMAL', dict(KW), num_particles=3, learning_rate=0.01, num_epochs=12,
                                      batch_size=bs, validation=(Xv, yv, 5, False))
  theta = inference._flatten_struct(inference._net_from_args(dict(KW), 'NORMAL'), params)
  assert np.all(theta == 12.0) and info['restored'] is False and np.array_equal(info['best_epoch'], np.full((1, 3), 10))


@pytest.mark.parametrize('path', ['full', 'keys', 'host'])
def test_no_validation_is_the_call_sequence_of_before(recorder, monkeypatch, path):
  X, y = _problem()
  bs = None if path == 'full' else 16
  if path == 'host':
    monkeypatch.setenv('BNF_ROW_TABLES', 'host')
  out = inference.fit_map(X, y, 7, 'NORMAL', dict(KW), num_particles=3, learning_rate=0.01, num_epochs=12, batch_size=bs)
  assert len(out) == 2 and out[1].shape == (1, 3, 12)
  log = recorder.log
  assert _calls(log, 'train') == [('train', 0, 12)]
  assert not _calls(log, 'forward_engine', 'forward', 'scores', 'check')
  assert _calls(log, 'engine') == [('engine', 3)] and _calls(log, 'close') == [('close', False)]
  assert _calls(log, 'row_keys') == ([('row_keys', 0, 12)] if path == 'keys' else [])
  assert _calls(log, 'row_tables') == ([('row_tables', 0, 12)] if path == 'host' else [])


def test_fit_map_refuses_a_validation_it_cannot_run(recorder):
  X, y = _problem()
  fit = lambda v, n=12: inference.fit_map(X, y, 7, 'NORMAL', dict(KW), num_particles=3, learning_rate=0.01, num_epochs=n,
                                          validation=v)
  with pytest.raises(ValueError, match='finite target'):
    fit((X[:4], np.full(4, np.nan), 5, True))
  with pytest.raises(ValueError, match='one target per row'):
    fit((X[:4], y[:5], 5, True))
  with pytest.raises(ValueError, match='>= 1'):
    fit((X[:4], y[:4], 0, True))
  with pytest.raises(ValueError, match='>= 1'):
    fit((X[:4], y[:4], 5, True), n=0)
  assert not recorder.log
