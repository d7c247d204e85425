"""Held-out validation during a fit, on the GPU (include/bnf.h bnf_validation_check; inference.fit_map validation=...;
BayesianNeuralFieldMAP.fit validation=...).

1. the decision rule and the snapshot copy against the numpy rule of tests/validation_ref.py, on hand-made scores;
2. training in segments with checks in between leaves the training where one bnf_train call leaves it;
3. the curve and the restored parameters mean what they say: the float64 oracle on the restored parameters gives 'best',
   and a plain fit of best_epoch epochs gives the restored parameters;
4. bf16 on the row-panel kernel, whose training handle refuses bnf_forward;
5. the estimator surface.

Bars: 1 is bit for bit.  2, 3c, 3d hold two executions of the same steps to rtol 1e-5 on the losses and rel_err < 1e-5 on
the parameters -- the bars of test_graph_replayed_training_equals_eager and test_forward_leaves_a_training_handle_alone on
this shape.  3b is util.FP32_GATE['loss'] relative, the gate of test_held_out_likelihood_agrees_with_the_training_loss
for the same quantity.  4 measures its own bar (see its docstring)."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

from bayesnf_amd import BayesianNeuralFieldMAP, BayesianNeuralFieldMLE, BayesianNeuralFieldVI, inference
from bayesnf_amd.engine import Engine
from oracle import bnf_oracle as O
from tests import util
from tests import validation_ref as V
from tests.test_gpu_sampling import MODEL

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


def _pattern(check, members, P):
  """Parameters that say where they come from: every element a function of (check, member, index), exact in float32 and
  distinct across checks (the member and index parts stay below 4096)."""
  m = np.arange(members, dtype=np.float64)[:, None]
  i = np.arange(P, dtype=np.float64)[None, :]
  return ((check + 1) * 4096.0 + m * 512.0 + i % 509.0).astype(np.float32)


class _Buffers:
  def __init__(self, eng, members, P, n_checks):
    dev = eng.device
    self.ll = torch.empty((members,), dtype=torch.float64, device=dev)
    self.curve = torch.full((members, n_checks), SENTINEL, dtype=torch.float64, device=dev)
    self.best_score = torch.full((members,), SENTINEL, dtype=torch.float64, device=dev)
    self.best_epoch = torch.full((members,), -777, dtype=torch.int64, device=dev)
    self.keep = torch.full((members,), -5, dtype=torch.int32, device=dev)
    self.best_params = torch.full((members, P), SENTINEL, dtype=torch.float32, device=dev)

  def args(self):
    return self.curve, self.best_score, self.best_epoch, self.keep, self.best_params

  def untouched(self):
    return (bool((self.curve == SENTINEL).all()) and bool((self.best_score == SENTINEL).all())
            and bool((self.best_epoch == -777).all()) and bool((self.keep == -5).all())
            and bool((self.best_params == SENTINEL).all()))


def _same(a, b):
  """Bit for bit in float64; a NaN equals a NaN whatever its payload."""
  a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
  nan = np.isnan(b)
  return np.array_equal(np.isnan(a), nan) and np.array_equal(a.view(np.int64)[~nan], b.view(np.int64)[~nan])


@pytest.mark.parametrize('names', [(n,) for n in V.COLUMNS] + [tuple(V.COLUMNS)], ids=lambda n: f'{len(n)}-{n[0][:8]}')
def test_the_rule_and_the_copy_on_hand_made_scores(names):
  M, K = len(names), len(V.EPOCHS)
  # width 64, depth 1, without the interaction features: P = 3151 (with them P = 3280, a multiple of 4)
  net, _, X, y = util.make_problem(n_rows=64, width=64, depth=1, interactions=())
  P = net.P
  assert P % 4 != 0 and P > 1024           # rows of the snapshot are not 16-byte aligned; more than one copy tile
  ll = V.columns(names)                     # (K, M)
  ref = V.run(ll, V.N_SCORED, V.EPOCHS)
  for name, m in zip(names, range(M)):
    assert tuple(ref['keep'][:, m]) == V.HAND_KEEP[name] and ref['best_check'][m] == V.HAND_BEST_CHECK[name]
  eng = Engine(net, X=X, y=y, members=M, compute_dtype='fp32')
  buf = _Buffers(eng, M, P, K)
  for c in range(K):
    eng.set_params(_pattern(c, M, P))
    buf.ll.copy_(torch.from_numpy(ll[c]))
    before = buf.best_params.cpu().numpy().copy()
    eng.validation_check(buf.ll, V.N_SCORED, V.EPOCHS[c], c, K, *buf.args())
    keep = buf.keep.cpu().numpy()
    assert np.array_equal(keep, ref['keep'][c]), (c, keep)
    assert _same(buf.best_score.cpu().numpy(), ref['history'][c][0]), c
    assert np.array_equal(buf.best_epoch.cpu().numpy(), ref['history'][c][1]), c
    after = buf.best_params.cpu().numpy()
    want = np.where(keep[:, None] == 1, _pattern(c, M, P), before)
    assert np.array_equal(after.view(np.int32), want.view(np.int32)), c
    assert np.array_equal(eng.get_params().view(np.int32), _pattern(c, M, P).view(np.int32))     # the parameters are only read
  assert _same(buf.curve.cpu().numpy(), ll.T / np.float64(V.N_SCORED))
  final = buf.best_params.cpu().numpy()
  for m in range(M):
    want = _pattern(int(ref['best_check'][m]), M, P)[m]
    assert np.array_equal(final[m].view(np.int32), want.view(np.int32)), names[m]
  # a second run: rows of members that a check does not keep are not written by it -- a sentinel laid before check 1
  # survives exactly there -- and two calls give the same bits
  buf2 = _Buffers(eng, M, P, K)
  for c in range(2):
    eng.set_params(_pattern(c, M, P))
    buf2.ll.copy_(torch.from_numpy(ll[c]))
    if c == 1:
      buf2.best_params.fill_(SENTINEL)
    eng.validation_check(buf2.ll, V.N_SCORED, V.EPOCHS[c], c, K, *buf2.args())
  got, keep1 = buf2.best_params.cpu().numpy(), ref['keep'][1]
  want = np.where(keep1[:, None] == 1, _pattern(1, M, P), np.float32(SENTINEL))
  assert np.array_equal(got.view(np.int32), want.view(np.int32))
  assert _same(buf2.curve.cpu().numpy()[:, :2], buf.curve.cpu().numpy()[:, :2])
  eng.close()


def test_refusals_launch_nothing():
  net, _, X, y = util.make_problem(n_rows=64, width=64, depth=1)
  M, P, K = 2, net.P, 3
  eng = Engine(net, X=X, y=y, members=M, compute_dtype='fp32')
  eng.set_params(_pattern(0, M, P))
  buf = _Buffers(eng, M, P, K)
  buf.ll.fill_(-1.0)
  for kw in (dict(n_scored=0), dict(check=K), dict(check=-1), dict(n_checks=0, check=0)):
    a = dict(n_scored=5, check=0, n_checks=K)
    a.update(kw)
    curve = buf.curve if a['n_checks'] == K else buf.curve[:, :0].contiguous()
    with pytest.raises(ValueError, match='bnf_validation_check'):
      eng.validation_check(buf.ll, a['n_scored'], 4, a['check'], a['n_checks'], curve, buf.best_score, buf.best_epoch,
                           buf.keep, buf.best_params)
  for hole in range(6):                              # a NULL pointer in every place
    args = [buf.ll, buf.curve, buf.best_score, buf.best_epoch, buf.keep, buf.best_params]
    args[hole] = None
    with pytest.raises(ValueError, match='bnf_validation_check'):
      eng.validation_check(args[0], 5, 4, 0, K, *args[1:])
  with pytest.raises(ValueError, match='overlaps'):  # the snapshot may not be the parameters themselves
    eng.validation_check(buf.ll, 5, 4, 0, K, buf.curve, buf.best_score, buf.best_epoch, buf.keep, eng.params.view(M, P))
  torch.cuda.synchronize()
  assert buf.untouched()
  eng.close()
  vi = Engine(net, mode='vi', X=X, y=y, members=M, vi_samples=1, compute_dtype='fp32')
  fwd = Engine(net, members=M, forward_only=True, row_capacity=64, compute_dtype='fp32')
  for other in (vi, fwd):
    with pytest.raises(RuntimeError, match=r'bnf_validation_check.*code -4'):
      other.validation_check(buf.ll, 5, 4, 0, K, *buf.args())
  torch.cuda.synchronize()
  assert buf.untouched()
  vi.close()
  fwd.close()


# ---- 2: segments with checks change nothing in training ------------------------------------------------------------------
SHAPE = dict(n_rows=200, width=64, depth=2)
ARGS = dict(width=64, depth=2, input_scales=[103.0, 1.0, 1.0], fourier_degrees=[5, 3, 2], interactions=[[0, 1], [1, 2]],
            seasonality_periods=[4.0, 52.1775], num_seasonal_harmonics=[2, 10])      # util.make_problem's network


def _held_out(obs='NORMAL'):
  """77 held-out rows of the same law, 3 of them without a target."""
  _, _, Xv, yv = util.make_problem(n_rows=77, width=64, depth=2, seed=1, observation_model=obs)
  yv = yv.copy()
  yv[[3, 40, 76]] = np.nan
  return Xv, yv


@pytest.mark.parametrize('pipeline', ['layers', 'auto'])
def test_segments_with_checks_change_nothing_in_training(pipeline):
  net, _, X, y = util.make_problem(**SHAPE)
  Xv, yv = _held_out()
  lni = float(np.log(np.nanstd(y) / 2))
  out = {}
  for run in 'AB':
    eng = Engine(net, X=X, y=y, members=3, seed=4, learning_rate=0.005, compute_dtype='fp32', pipeline=pipeline)
    eng.init_params(lni)
    if run == 'A':
      losses = eng.train(0, 12)
    else:
      held = inference._HeldOut(net, eng, Xv, yv, inference.validation_epochs(12, 5), 'fp32', eng.dev_index)
      parts = held.train(0, 12)
      assert [p.shape[1] for p in parts] == [5, 5, 2] and held.done == 3
      losses = torch.cat(parts, dim=1)
    out[run] = (losses.cpu().numpy(), eng.get_params().copy())
    if run == 'B':
      curve, best_epoch = held.curve.cpu().numpy(), held.best_epoch.cpu().numpy()
      held.close()
    eng.close()
  perr = util.rel_err(out['B'][1], out['A'][1])
  lerr = float(np.max(np.abs(out['B'][0] - out['A'][0]) / np.abs(out['A'][0])))
  print(f'{pipeline}: segments vs one call: loss rel err {lerr:.2e}, param rel err {perr:.2e}; curve {curve[0]}, best epochs {best_epoch}')
  np.testing.assert_allclose(out['B'][0], out['A'][0], rtol=1e-5)
  assert perr < 1e-5
  assert np.all(np.isfinite(curve)) and set(best_epoch.tolist()) <= {5, 10, 12}


# ---- 3: the curve and the restored parameters mean what they say ------------------------------------------------------------
def _fit(X, y, obs, num_epochs, validation=None):
  return inference.fit_map(X, y, 4, obs, dict(ARGS), num_particles=3, learning_rate=0.005, num_epochs=num_epochs,
                           compute_dtype='fp32', validation=validation)


def _oracle_mean_log_density(model, theta, Xv, yv):
  kept = np.isfinite(yv)
  n = int(kept.sum())
  return -O.map_loss(model, np.asarray(theta, dtype=np.float64), Xv[kept], yv[kept], n_total=n, prior_weight=0.0) / n


@pytest.mark.parametrize('obs', ['NORMAL', 'NB'])
def test_the_curve_and_the_restored_parameters_mean_what_they_say(obs):
  net, model, X, y = util.make_problem(**SHAPE, observation_model=obs)
  Xv, yv = _held_out(obs)
  gate = util.FP32_GATE['loss']
  params, losses, info = _fit(X, y, obs, 24, validation=(Xv, yv, 5, True))
  theta = inference._flatten_struct(net, params)[0]                       # (3, P)
  curve, best, best_epoch = info['member_log_density'][0], info['best'][0], info['best_epoch'][0]
  assert info['epochs'].tolist() == [5, 10, 15, 20, 24] and info['n'] == 74 and info['restored'] is True
  assert curve.shape == (3, 5) and curve.dtype == np.float64 and losses.shape == (1, 3, 24)
  # (a) best is the curve's maximum at its first occurrence, by the rule
  want_best, want_epoch = V.best_of_curve(curve, info['epochs'])
  assert np.array_equal(best, want_best, equal_nan=True) and np.array_equal(best_epoch, want_epoch)
  assert np.all(np.isfinite(curve))
  # (b) the float64 oracle on the restored parameters gives best
  want = _oracle_mean_log_density(model, theta, Xv, yv)
  err_b = np.abs(best - want) / np.abs(want)
  # (c) a plain fit of best_epoch epochs gives the restored parameters
  err_c = {}
  for ep in sorted(set(best_epoch.tolist())):
    plain, _ = _fit(X, y, obs, int(ep))
    plain = inference._flatten_struct(net, plain)[0]
    for m in np.nonzero(best_epoch == ep)[0]:
      err_c[int(m)] = util.rel_err(theta[m], plain[m])
  # (d) restore_best=False: the parameters and losses of a plain 24-epoch fit; the last curve column is theirs
  params_f, losses_f, info_f = _fit(X, y, obs, 24, validation=(Xv, yv, 5, False))
  plain24, losses24 = _fit(X, y, obs, 24)
  theta_f, theta24 = inference._flatten_struct(net, params_f)[0], inference._flatten_struct(net, plain24)[0]
  err_d = util.rel_err(theta_f, theta24)
  want_last = _oracle_mean_log_density(model, theta_f, Xv, yv)
  err_last = np.abs(info_f['member_log_density'][0][:, -1] - want_last) / np.abs(want_last)
  print(f'{obs}: curve[0] {curve[0]}, best epochs {best_epoch}; (b) {err_b.max():.2e} (gate {gate:.0e}); (c) {err_c}; '
        f'(d) params {err_d:.2e}, last column {err_last.max():.2e}')
  assert np.all(err_b <= gate), err_b
  assert all(e < 1e-5 for e in err_c.values()) and len(err_c) == 3, err_c
  assert err_d < 1e-5 and info_f['restored'] is False
  np.testing.assert_allclose(losses_f, losses24, rtol=1e-5)
  np.testing.assert_allclose(losses, losses24, rtol=1e-5)                 # the losses are the same either way
  assert np.all(err_last <= gate), err_last


# ---- 4 and 5: the estimator ---------------------------------------------------------------------------------------------------
def _frames(golden_dir):
  read = lambda name: pd.read_csv(os.path.join(golden_dir, name), index_col=0, parse_dates=['datetime'])
  return read('chickenpox.8.train.csv'), read('chickenpox.8.test.csv')


def test_bf16_on_the_row_panel_kernel(golden_dir):
  """width 256, depth 2, bf16: the training handle runs the row-panel kernel and refuses bnf_forward -- why the checks own
  a second handle.  validation_['best'] against score(val)['member_log_prob'] / n on the restored parameters: both are the
  bf16 forward of the same parameters on a forward-only handle, so the bar is 4 x the largest mutual relative difference
  of three repeated score calls (run-to-run freedom: the order of the f32 atomics in the output dot), and never below
  util.FP32_GATE['loss'] = 1e-5.  MEASURED on an MI355X: spread of the three score calls 0.0 (bitwise equal), so the bar is
  1e-5; 'best' against score 0.0 as well (best = -5.667, -5.660, -5.663, every member at epoch 12).  The test prints both."""
  table, _ = _frames(golden_dir)
  df, val = table.iloc[:70], table.iloc[70:]          # the first 70 weeks of the one place, validated on its last 30
  model = dict(MODEL, width=256)
  est = BayesianNeuralFieldMAP(**model, observation_model='NORMAL', compute_dtype='bf16')
  est.fit(df, seed=2, ensemble_size=3, num_epochs=12, learning_rate=0.005, validation=val, validation_every=5)
  assert np.all(np.isfinite(est.losses_)) and est.losses_.shape == (1, 3, 12)
  v = est.validation_
  assert v['epochs'].tolist() == [5, 10, 12] and v['member_log_density'].shape == (1, 3, 3) and v['restored'] is True
  n = v['n']
  assert n == int(np.isfinite(val['chickenpox'].to_numpy(dtype=np.float64)).sum())
  scores = [est.score(val)['member_log_prob'] / n for _ in range(3)]
  spread = max(float(np.max(np.abs(a - b) / np.abs(b))) for a in scores for b in scores)
  bar = max(4.0 * spread, util.FP32_GATE['loss'])
  err = float(np.max(np.abs(v['best'] - scores[0]) / np.abs(scores[0])))
  print(f'bf16 panel: best {v["best"]}, best epochs {v["best_epoch"]}; score spread {spread:.2e}, bar {bar:.2e}, err {err:.2e}')
  # the training handle of this fit is a row-panel handle: bnf_forward refuses it
  x = est.data_handler.get_train(df)
  net = inference._net_from_args(est._model_args(x.shape), 'NORMAL')
  eng = Engine(net, X=x, y=est.data_handler.get_target(df), members=1, compute_dtype='bf16')
  with pytest.raises(RuntimeError, match='forward_only'):
    eng.forward(eng.params.view(1, net.P), eng.X)
  eng.close()
  assert err <= bar, (err, bar)


def test_estimator_surface(golden_dir):
  df, val = _frames(golden_dir)
  val = val.copy()
  val.loc[val.index[[0, 9]], 'chickenpox'] = np.nan
  n = int(np.isfinite(val['chickenpox'].to_numpy(dtype=np.float64)).sum())
  assert n == len(val) - 2
  est = BayesianNeuralFieldMAP(**MODEL, observation_model='NB', compute_dtype='fp32')
  assert est.validation_ is None
  est.fit(df, seed=3, ensemble_size=4, num_epochs=20, learning_rate=0.01, validation=val, validation_every=7)
  v = est.validation_
  assert set(v) == {'epochs', 'member_log_density', 'best', 'best_epoch', 'n', 'restored'}
  assert v['epochs'].tolist() == [7, 14, 20] and v['n'] == n and v['restored'] is True
  lead = est.losses_.shape[:-1]
  assert lead == (1, 4) and est.losses_.shape[-1] == 20
  assert v['member_log_density'].shape == lead + (3,) and v['member_log_density'].dtype == np.float64
  assert v['best'].shape == lead and v['best_epoch'].shape == lead
  want_best, want_epoch = V.best_of_curve(v['member_log_density'], v['epochs'])
  assert np.array_equal(v['best'], want_best, equal_nan=True) and np.array_equal(v['best_epoch'], want_epoch)
  print(f'NB estimator, test table: curve {v["member_log_density"][0]}, best epochs {v["best_epoch"]}')
  # (the train fixture holds ONE place, so the standardised coordinates of the test fixture's other places are ~1e14 and
  # this curve may well be NaN: the rule above covers it.  What the numbers mean is checked on rows of the place itself:)
  # fit on the first 70 weeks, validate on the last 30: params_ holds every member at its best epoch, so score() of the
  # validation table gives 'best' back -- two forwards of the same parameters, within the gate of the held-out likelihood
  head, tail = df.iloc[:70], df.iloc[70:].copy()
  tail.loc[tail.index[[4]], 'chickenpox'] = np.nan
  est.fit(head, seed=3, ensemble_size=4, num_epochs=20, learning_rate=0.01, validation=tail, validation_every=7)
  v = est.validation_
  assert v['n'] == 29 and np.all(np.isfinite(v['member_log_density']))
  got = est.score(tail)['member_log_prob'] / 29
  err = float(np.max(np.abs(got - v['best']) / np.abs(v['best'])))
  print(f'NB estimator, last 30 weeks: curve {v["member_log_density"][0]}, best epochs {v["best_epoch"]}, score vs best {err:.2e}')
  assert err <= util.FP32_GATE['loss']
  # the default period: ceil(num_epochs / 50), at least 1
  est.fit(df, seed=3, ensemble_size=4, num_epochs=3, learning_rate=0.01, validation=val, restore_best=False)
  assert est.validation_['epochs'].tolist() == [1, 2, 3] and est.validation_['restored'] is False
  est.fit(df, seed=3, ensemble_size=4, num_epochs=3, learning_rate=0.01)
  assert est.validation_ is None
  mle = BayesianNeuralFieldMLE(**MODEL, observation_model='NB', compute_dtype='fp32')
  mle.fit(df, seed=3, ensemble_size=4, num_epochs=4, learning_rate=0.01, validation=val, validation_every=3)
  assert mle.validation_['epochs'].tolist() == [3, 4] and mle.validation_['member_log_density'].shape == (1, 4, 2)
  vi = BayesianNeuralFieldVI(**MODEL, observation_model='NORMAL', compute_dtype='fp32')
  with pytest.raises(TypeError, match='validation'):
    vi.fit(df, seed=1, ensemble_size=2, num_epochs=2, validation=val)
