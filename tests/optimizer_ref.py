"""Float64 restatement of what one optimiser step leaves behind (k_adam_map / k_vi_adam, optax.adam defaults): the two
moments as closed forms in the gradients of the steps taken so far, the parameter update from the moments, and a per-leaf
comparison that names the worst element.  Nothing here touches the GPU; tests/test_gpu_optimizer.py holds the engine's
`state` and `params` to it after every call of `train`."""
import numpy as np

B1, B2, EPS = 0.9, 0.999, 1e-8


def moments(grads):
  """grads: the gradients g_1 .. g_K of the steps taken so far, each (E, P) -> (m_K, v_K), the moments after step K from
  zero state: m_K = sum_k (1 - b1) b1^(K - k) g_k, v_K = sum_k (1 - b2) b2^(K - k) g_k^2."""
  K = len(grads)
  m = np.zeros_like(np.asarray(grads[0], dtype=np.float64))
  v = np.zeros_like(m)
  for k, g in enumerate(grads, start=1):
    g = np.asarray(g, dtype=np.float64)
    m += (1 - B1) * B1 ** (K - k) * g
    v += (1 - B2) * B2 ** (K - k) * g * g
  return m, v


def moments_next(m, v, g):
  """One step of the same recursion from the moments (m, v) before it."""
  m, v, g = (np.asarray(a, dtype=np.float64) for a in (m, v, g))
  return B1 * m + (1 - B1) * g, B2 * v + (1 - B2) * g * g


def theta_next(theta, m, v, t, lr):
  """The parameters after step t (1-based) from those before it and the moments AFTER the step's update."""
  theta, m, v = (np.asarray(a, dtype=np.float64) for a in (theta, m, v))
  return theta - lr * (m / (1 - B1 ** t)) / (np.sqrt(v / (1 - B2 ** t)) + EPS)


def leaf_report(model, got, want):
  """`util.per_leaf_rel_err` with the place of the worst element: {leaf: (err, index)} where err is max |got - want| over
  the leaf divided by the leaf's max |want| (over every leading axis; the absolute error where want is all zero) and
  index = (*leading, offset in the leaf) of that element.  A quad at the edge of a kernel and a whole stale layer read
  differently here: the offset is 0 .. 3 from an end of the leaf, or anywhere."""
  got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
  assert got.shape == want.shape and got.shape[-1] == model.P, (got.shape, want.shape, model.P)
  out = {}
  for lf in model.leaves:
    sl = slice(lf.offset, lf.offset + lf.size)
    d = np.abs(got[..., sl] - want[..., sl])
    d = np.where(np.isnan(d), np.inf, d)        # a NaN on either side is the worst element, not an ignored one
    ref = float(np.max(np.abs(want[..., sl])))
    worst = np.unravel_index(int(np.argmax(d)), d.shape)
    out[lf.name] = (float(d[worst]) / ref if ref > 0 else float(d[worst]), tuple(int(i) for i in worst))
  return out


def leaf_failures(model, got, want, bar):
  """The leaves of `leaf_report` above `bar`: {} when got meets want."""
  return {k: v for k, v in leaf_report(model, got, want).items() if not v[0] <= bar}


# ---- VI: the same over (mu, rho); the state holds m_mu, v_mu, m_rho, v_rho, each E * P floats, in this order (step_vi)
def vi_split_state(state, E, P):
  """The flat state of a VI handle -> (m_mu, v_mu, m_rho, v_rho), each (E, P)."""
  s = np.asarray(state).reshape(4, E, P)
  return s[0], s[1], s[2], s[3]


def vi_moments(grads):
  """grads: per step (2, E, P) = (d mu, d rho) as `debug_loss_and_grad` returns them -> (m_mu, v_mu, m_rho, v_rho)."""
  m_mu, v_mu = moments([g[0] for g in grads])
  m_rho, v_rho = moments([g[1] for g in grads])
  return m_mu, v_mu, m_rho, v_rho


def vi_moments_next(state4, g):
  """One step from (m_mu, v_mu, m_rho, v_rho) with the gradients g (2, E, P)."""
  m_mu, v_mu = moments_next(state4[0], state4[1], g[0])
  m_rho, v_rho = moments_next(state4[2], state4[3], g[1])
  return m_mu, v_mu, m_rho, v_rho


def vi_params_next(params, state4, t, lr):
  """params (2, E, P) = (mu, rho) before step t, state4 the moments after it -> (2, E, P) after it."""
  return np.stack([theta_next(params[0], state4[0], state4[1], t, lr),
                   theta_next(params[1], state4[2], state4[3], t, lr)])
