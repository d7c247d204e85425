"""tests/optimizer_ref.py against the oracle's own Adam (oracle/bnf_oracle.py adam_update, train_map, train_vi) on a
width-8 problem, and the checker against the failure it is for: a gradient range that carries the previous step's value
into this one must be reported far above the GPU test's bar, in the leaf it sits in.  CPU only."""
import numpy as np
import pytest

from oracle import bnf_oracle as O
from tests import optimizer_ref as R
from tests import util

GPU_BAR = 1e-4      # tests/test_gpu_optimizer.py: the floor of the bar for the moments
E, LR = 3, 0.005


@pytest.fixture(scope='module')
def problem():
  net, model, X, y = util.make_problem(n_rows=40, width=8, depth=2)
  theta0 = util.random_theta(model, E, seed=2, scale=0.4)
  return model, X, y, theta0


@pytest.fixture(scope='module')
def map_run(problem):
  """Five full-batch steps by hand with O.adam_update: (thetas 0..5, gradients 1..5, (m, v) after every step)."""
  model, X, y, theta0 = problem
  thetas, grads, states = [theta0], [], []
  m, v = np.zeros_like(theta0), np.zeros_like(theta0)
  for t in range(1, 6):
    _, g = O.map_loss_and_grad(model, thetas[-1], X, y, n_total=len(y))
    th, m, v = O.adam_update(thetas[-1], m, v, g, t, LR)
    thetas.append(th); grads.append(g); states.append((m, v))
  return thetas, grads, states


def test_moments_and_theta_next_reproduce_adam_update_step_by_step(map_run):
  thetas, grads, states = map_run
  for t in range(1, 6):
    m_o, v_o = states[t - 1]
    m, v = R.moments(grads[:t])
    np.testing.assert_allclose(m, m_o, rtol=1e-12, atol=0)
    np.testing.assert_allclose(v, v_o, rtol=1e-12, atol=0)
    if t > 1:
      m2, v2 = R.moments_next(*states[t - 2], grads[t - 1])
      np.testing.assert_allclose(m2, m_o, rtol=1e-14, atol=0)
      np.testing.assert_allclose(v2, v_o, rtol=1e-14, atol=0)
    np.testing.assert_allclose(R.theta_next(thetas[t - 1], m_o, v_o, t, LR), thetas[t], rtol=1e-14, atol=1e-15)


def test_closed_forms_reproduce_train_map(problem, map_run):
  model, X, y, theta0 = problem
  thetas, grads, _ = map_run
  theta_o, _, m_o, v_o = O.train_map(model, theta0, X, y, lr=LR, num_epochs=5, return_state=True)
  th = theta0
  for t in range(1, 6):
    th = R.theta_next(th, *R.moments(grads[:t]), t, LR)
  np.testing.assert_allclose(th, theta_o, rtol=1e-12, atol=1e-12)
  m, v = R.moments(grads)
  np.testing.assert_allclose(m, m_o, rtol=1e-12, atol=0)
  np.testing.assert_allclose(v, v_o, rtol=1e-12, atol=0)


def test_vi_forms_reproduce_train_vi(problem):
  model, X, y, theta0 = problem
  S, kl, steps = 2, 0.2, 4
  rng = np.random.default_rng(5)
  eps = rng.standard_normal((steps, E, S, model.P))
  mu, rho = theta0, np.full_like(theta0, np.log(np.expm1(0.3)))
  mu_o, rho_o, _ = O.train_vi(model, mu, rho, X, y, lr=LR, num_steps=steps, sample_size=S, kl_weight=kl,
                              eps_fn=lambda s: eps[s])
  params, grads = np.stack([mu, rho]), []
  state4 = tuple(np.zeros_like(mu) for _ in range(4))
  for t in range(1, steps + 1):
    _, gmu, grho = O.vi_loss_and_grad(model, params[0], params[1], eps[t - 1], X, y, len(y), kl)
    grads.append(np.stack([gmu, grho]))
    nxt = R.vi_moments_next(state4, grads[-1])
    for a, b in zip(nxt, R.vi_moments(grads)):          # the recursion and the closed form agree
      np.testing.assert_allclose(a, b, rtol=1e-12, atol=0)
    state4 = nxt
    params = R.vi_params_next(params, state4, t, LR)
  np.testing.assert_allclose(params[0], mu_o, rtol=1e-12, atol=1e-12)
  np.testing.assert_allclose(params[1], rho_o, rtol=1e-12, atol=1e-12)
  # the flat layout of the handle's state: four blocks of E * P
  flat = np.concatenate([s.reshape(-1) for s in state4])
  for a, b in zip(R.vi_split_state(flat, E, model.P), state4):
    np.testing.assert_array_equal(a, b)


def test_leaf_report_is_per_leaf_rel_err_with_the_worst_index(problem, map_run):
  model = problem[0]
  _, grads, _ = map_run
  got = grads[1].copy()
  lf = model.leaf['Dense_1/kernel']
  got[2, lf.offset + 5] += 0.25
  rep = R.leaf_report(model, got, grads[1])
  errs = util.per_leaf_rel_err(model, got, grads[1])
  assert {k: v[0] for k, v in rep.items()} == errs
  assert rep['Dense_1/kernel'][1] == (2, 5) and rep['Dense_1/kernel'][0] > 0
  assert all(v[0] == 0 for k, v in rep.items() if k != 'Dense_1/kernel')
  got[1, model.leaf['Dense_0/bias'].offset + 3] = np.nan      # a NaN is the worst element of its leaf
  rep = R.leaf_report(model, got, grads[1])
  assert rep['Dense_0/bias'] == (np.inf, (1, 3))
  assert set(R.leaf_failures(model, got, grads[1], 1e-2)) == {'Dense_0/bias', 'Dense_1/kernel'}


@pytest.mark.parametrize('what', ['kept range', 'quad past it'])
def test_a_planted_stale_gradient_is_reported_far_above_the_gpu_bar(problem, map_run, what):
  """What an uncleared gradient range does: the second step's weight gradient is ADDED to the first step's instead of
  replacing it, so g_2 reads g_1 + g_2 there.  Once over the whole Dense_1 kernel (a range kept although the next step
  accumulates), once over the four entries right behind it (a bound rounded outwards by a quad: the Dense_2 bias and the
  first three entries of the Dense_2 kernel).  Both moments after the second step must miss the expected ones by >= 100
  times the GPU bar, in exactly the leaves the entries belong to, with the worst element inside the range."""
  model = problem[0]
  _, grads, _ = map_run
  lf = model.leaf['Dense_1/kernel']
  lo, hi = (lf.offset, lf.offset + lf.size) if what == 'kept range' else (lf.offset + lf.size, lf.offset + lf.size + 4)
  touched = {l.name for l in model.leaves if l.offset < hi and l.offset + l.size > lo}
  assert touched == ({'Dense_1/kernel'} if what == 'kept range' else {'Dense_2/bias', 'Dense_2/kernel'})
  g2 = grads[1].copy()
  g2[:, lo:hi] += grads[0][:, lo:hi]
  want = R.moments(grads[:2])
  got = R.moments([grads[0], g2])
  for k, bar in ((0, GPU_BAR), (1, 2 * GPU_BAR)):             # m at the bar, v at twice it
    assert R.leaf_failures(model, want[k], want[k], bar) == {}
    bad = R.leaf_failures(model, got[k], want[k], bar)
    assert set(bad) == touched, (what, k, bad)
    for name, (err, (e, off)) in bad.items():
      assert err >= 100 * bar, (what, k, name, err)
      assert lo <= model.leaf[name].offset + off < hi, (what, k, name, off)
