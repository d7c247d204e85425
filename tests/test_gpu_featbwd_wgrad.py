"""The fused featurisation backward formed by the layer-0 weight-gradient kernel (gemm_tn_skinny_featbwd, bnf_gemm.h;
StepPlan::featbwd_in_wgrad) against the path it replaces: the last phase of the panel kernel (BNF_FEATBWD_WGRAD=0), which
forms the same triple products h dz k from the same bf16 values in another f32 summation order.

Bars.  The featurisation leaves (feature_inv_sp_scale*, log_scale_adjustment):
  * against the float64 oracle, either path: 2e-2 of the leaf's maximum (the bar of
    test_fused_featurisation_backward_matches_the_separate_kernel);
  * new path against in-panel path: SAME_PRODUCTS, ten times the spread the in-panel path shows against its own second
    evaluation on case a (the order of its float atomics; profiles/featbwd_in_wgrad.md has the measurement).
Every other leaf: 2e-3 between the paths (dK0 and d bias0 still come out of the same accumulators); loss 1e-5 relative."""
import numpy as np
import pytest

from oracle import bnf_oracle as O
from tests import util

pytestmark = pytest.mark.gpu

# in-panel path, case a, second evaluation against the first: at most IN_PANEL_SPREAD of a featurisation leaf's maximum
IN_PANEL_SPREAD = 1.3e-7   # measured on an MI355X (1.275e-7) before the new path was held to it (see the note)
SAME_PRODUCTS = 10 * IN_PANEL_SPREAD


def _engine(net, X, y, **kw):
  from bayesnf_amd.engine import Engine
  return Engine(net, X=X, y=y, **kw)


def _feat_leaves(model):
  names = [k for k in model.leaf if k.startswith('feature_inv_sp_scale') or k == 'log_scale_adjustment']
  assert len(names) >= 5
  return names


def _in_wgrad(eng, net, width, depth, nets, n_rows):
  """Which form ran, from the flops the engine books to the panel kernel: without its dH0 contraction it is
  2 E B F W short of forward + backward-data of every layer + the output layer."""
  full = 4.0 * nets * n_rows * (net.F * width + (depth - 1) * width * width) + 2.0 * nets * n_rows * width
  got = eng.lib.bnf_kernel_flops(eng.handle, b'panel_fwd_bwd')
  moved = 2.0 * nets * n_rows * net.F * width
  assert got in (full, full - moved), (got, full, moved)
  return got == full - moved


def _both_paths(monkeypatch, net, X, y, width, depth, n_rows, expect_new=True, setup=None, **kw):
  """-> {'1': (loss, grad), '0': (loss, grad)}, extra: each path evaluated twice (scratch that is not re-initialised
  shows up in the second evaluation)."""
  res, extra = {}, {}
  for flag in ('1', '0'):
    monkeypatch.setenv('BNF_FEATBWD_WGRAD', flag)
    eng = _engine(net, X, y, compute_dtype='bf16', pipeline='panel', **kw)
    nets = kw['members'] * kw.get('vi_samples', 1)
    assert _in_wgrad(eng, net, width, depth, nets, n_rows) == (expect_new and flag == '1')
    if setup is not None:
      extra[flag] = setup(eng)
    loss, g = eng.debug_loss_and_grad(0, 0)
    loss2, g2 = eng.debug_loss_and_grad(0, 0)
    eng.close()
    res[flag] = (loss, g, loss2, g2)
  return res, extra


def _compare(model, res, names, tag):
  (l1, g1, l1b, g1b), (l0, g0, l0b, g0b) = res['1'], res['0']
  spread0 = util.per_leaf_rel_err(model, g0b, g0)
  spread1 = util.per_leaf_rel_err(model, g1b, g1)
  errs = util.per_leaf_rel_err(model, g1, g0)
  errs_b = util.per_leaf_rel_err(model, g1b, g0)
  print(f'[{tag}] in-panel, 2nd vs 1st evaluation: max over the featurisation leaves {max(spread0[k] for k in names):.3e}')
  print(f'[{tag}] new path, 2nd vs 1st evaluation: max over the featurisation leaves {max(spread1[k] for k in names):.3e}')
  print(f'[{tag}] new vs in-panel: featurisation leaves {max(errs[k] for k in names):.3e} (2nd evaluation '
        f'{max(errs_b[k] for k in names):.3e}), other leaves {max(v for k, v in errs.items() if k not in names):.3e}, '
        f'loss {np.max(np.abs(l1 - l0) / np.abs(l0)):.3e}')
  np.testing.assert_allclose(l1, l0, rtol=1e-5)
  np.testing.assert_allclose(l1b, l0, rtol=1e-5)
  for e in (errs, errs_b):
    bad = {k: e[k] for k in names if e[k] > SAME_PRODUCTS}
    assert not bad, ('featurisation leaves, new vs in-panel', bad)
    rest = {k: v for k, v in e.items() if k not in names and v > 2e-3}
    assert not rest, ('other leaves, new vs in-panel', rest)


CASES = {
    # Bp = 1024, split-K 4, 24 padding rows: the atomic epilogue
    'a': dict(width=512, depth=2, n_rows=1000, members=3),
    # Bp = 256, split-K 1: the store epilogue; one partly empty panel
    'b': dict(width=512, depth=2, n_rows=130, members=3),
    # the DEEP form
    'c': dict(width=512, depth=3, n_rows=300, members=3),
    # two column tiles per member
    'd': dict(width=1024, depth=2, n_rows=300, members=2),
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_map_step_matches_the_in_panel_path_and_the_oracle(monkeypatch, case):
  c = CASES[case]
  net, model, X, y = util.make_problem(n_rows=c['n_rows'], width=c['width'], depth=c['depth'])
  assert net.F <= 62
  E = c['members']
  theta = util.random_theta(model, E, scale=0.3)
  _, g_o = O.map_loss_and_grad(model, theta, X, y, n_total=c['n_rows'])
  res, _ = _both_paths(monkeypatch, net, X, y, c['width'], c['depth'], c['n_rows'], members=E,
                       setup=lambda eng: eng.set_params(theta))
  names = _feat_leaves(model)
  for flag in res:
    for g in (res[flag][1], res[flag][3]):
      errs = util.per_leaf_rel_err(model, g, g_o)
      print(f'[{case}] path {flag} vs oracle: featurisation leaves {max(errs[k] for k in names):.3e}')
      bad = {k: errs[k] for k in names if errs[k] > 2e-2}
      assert not bad, (flag, 'vs oracle', bad)
  _compare(model, res, names, case)


def test_vi_step_takes_kb_from_the_sampled_network(monkeypatch):
  """Case a as VI, 2 members x 2 samples, on the noise the device drew (as test_panel_vi_step_vs_oracle): the Dense
  kernels' samples exist only as the bf16 fragments k_vi_sample_pack wrote, and those are what the epilogue reads."""
  n_rows, width, E, S = 1000, 512, 2, 2
  net, model, X, y = util.make_problem(n_rows=n_rows, width=width, depth=2)

  def setup(eng):
    eng.init_params(0.0)
    return eng.get_params().astype(np.float64), eng.debug_vi_eps(0)

  res, extra = _both_paths(monkeypatch, net, X, y, width, 2, n_rows, members=E, mode='vi', vi_samples=S, kl_weight=0.2,
                           seed=5, learning_rate=0.01, setup=setup)
  p0, eps0 = extra['1']
  np.testing.assert_array_equal(eps0, extra['0'][1])
  _, gmu_o, grho_o = O.vi_loss_and_grad(model, p0[0], p0[1], eps0, X, y, n_rows, 0.2)
  names = _feat_leaves(model)
  for flag in res:
    for g in (res[flag][1], res[flag][3]):
      for k, ref in ((0, gmu_o), (1, grho_o)):
        errs = util.per_leaf_rel_err(model, g[k], ref)
        print(f'[e] path {flag} vs oracle, {"gmu" if k == 0 else "grho"}: worst leaf {max(errs.values()):.3e}, '
              f'featurisation leaves {max(errs[n] for n in names):.3e}')
        bad = {n: v for n, v in errs.items() if v > 6e-2}
        assert not bad, (flag, k, bad)
        bad = {n: errs[n] for n in names if errs[n] > 2e-2}
        assert not bad, (flag, k, 'featurisation leaves vs oracle', bad)
  _compare(model, res, names, 'e')


def test_more_than_32_fourier_columns_keep_the_in_panel_form(monkeypatch):
  """36 Fourier columns at Fp = 64: more than the weight-gradient kernel has slots for -- the plan keeps the panel
  kernel's own phase (seen in the flops the engine books to it), with the switch on or off, and the oracle's bar holds."""
  n_rows, width, E = 300, 512, 2
  net, model, X, y = util.make_problem(n_rows=n_rows, width=width, depth=2, fourier_degrees=(6, 6, 6), harmonics=(2, 5))
  assert net.F <= 62
  theta = util.random_theta(model, E, scale=0.3)
  _, g_o = O.map_loss_and_grad(model, theta, X, y, n_total=n_rows)
  res, _ = _both_paths(monkeypatch, net, X, y, width, 2, n_rows, expect_new=False, members=E,
                       setup=lambda eng: eng.set_params(theta))
  names = _feat_leaves(model)
  for flag in res:
    errs = util.per_leaf_rel_err(model, res[flag][1], g_o)
    bad = {k: errs[k] for k in names if errs[k] > 2e-2}
    assert not bad, (flag, bad)
  _compare(model, res, names, 'f')
