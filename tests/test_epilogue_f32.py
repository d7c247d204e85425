"""The two float32 restatements of the likelihood epilogue (tests/epilogue_f32.py) against the float64 oracle, on the CPU.

'tfp' is TFP's log_prob term by term (what the reference evaluates, in float32 too); 'engine' is what
bayesnf_amd/csrc/bnf_device.h row_loss_eval evaluates.  The rule the engine's forms are held to: on every grid case each
of the five quantities is no less accurate than the reference's own arithmetic plus the fp32 gate.  tests/test_gpu_epilogue.py
then holds the device to max(gate, 4 x the 'engine' restatement's error)."""
import numpy as np
import pytest

from tests import epilogue_f32 as H

GRID = [(tc, mean) for tc in H.TCS for mean in H.MEANS]


def _errs(model, theta, y):
  ref = H.oracle_terms(model, theta, y)
  return {form: H.errors(H.f32_terms(model, theta, y, form), ref) for form in ('tfp', 'engine')}


@pytest.mark.parametrize('obs', ['NB', 'ZINB'])
def test_engine_forms_are_no_worse_than_tfp_verbatim_on_the_grid(obs):
  """... and where they are better (printed: tfp -> engine).  Measured, NB, worst member: at total_count 0.05, mean 1e6
  the output-bias gradient 7.4e-1 -> 1.1e-6, the loss 5.5e-2 -> 1.9e-8, the shape gradient 6.4e-2 -> 1.1e-7; at
  total_count 1e3, mean 0.02 the loss 4.7e-4 -> 8.0e-8 and the shape gradient 4.8e-4 -> 5.4e-7.  The engine's forms
  stay <= 3.0e-6 on the whole grid (loss <= 1.2e-6), so 4 x their error is inside the gate for every quantity at every
  grid point: the device test's bar is the gate itself everywhere (asserted below for the output bias and the output scale
  at mean <= 2e4, the cases the rewrite of d lp / d logits was made for)."""
  _, model, _ = H.problem(obs)
  worse, loose = [], []
  for tc, mean in GRID:
    theta, y = H.count_case(model, tc, mean)
    e = _errs(model, theta, y)
    print(f'{obs} tc={tc:g} mean={mean:g} max y={y.max():g}: ' +
          ' '.join(f'{q} {e["tfp"][q]:.1e} -> {e["engine"][q]:.1e}' for q in H.QUANTITIES))
    bars = H.bars(e['engine'])
    for q in H.QUANTITIES:
      if not e['engine'][q] <= e['tfp'][q] + H.gate(q):
        worse.append((tc, mean, q, e['tfp'][q], e['engine'][q]))
      if q in ('bias', 'scale') and mean <= 2e4 and bars[q][1] != 'gate':
        loose.append((tc, mean, q, e['engine'][q]))
  assert not worse, worse
  assert not loose, loose


@pytest.mark.parametrize('half_integer', [False, True])
@pytest.mark.parametrize('obs', ['NB', 'ZINB'])
def test_both_restatements_meet_the_gate_on_the_toy_regime(obs, half_integer):
  """Counts up to ~30, total_count 1 .. 2, outputs of order 1 -- what the suite checked before the grid; with
  half-integer targets the engine's forms are TFP's own below the thresholds."""
  _, model, _ = H.problem(obs)
  theta, y = H.toy_case(model, half_integer)
  assert y.max() < 60
  for form, e in _errs(model, theta, y).items():
    for q in H.QUANTITIES:
      assert e[q] <= H.gate(q), (form, q, e[q])


def test_normal_restatement_meets_the_gate():
  _, model, _ = H.problem('NORMAL')
  for lns in H.NORMAL_LNS:
    for mag in H.NORMAL_MAGS:
      theta, y = H.normal_case(model, lns, mag)
      e = _errs(model, theta, y)['engine']
      for q in H.QUANTITIES:
        assert e[q] <= H.gate(q), (lns, mag, q, e[q])


def test_oracle_per_row_terms_sum_to_the_oracle_gradient():
  """oracle_terms' rows add up to what O.map_loss_and_grad returns for the same parameters (prior_weight 0, full batch)."""
  from oracle import bnf_oracle as O
  for obs, case in (('ZINB', lambda m: H.count_case(m, 1.0, 400.0)), ('NORMAL', lambda m: H.normal_case(m, 0.0, 1e3))):
    _, model, X = H.problem(obs)
    theta, y = case(model)
    loss, g = O.map_loss_and_grad(model, theta, X, y, n_total=len(y), prior_weight=0.0)
    ref = H.oracle_terms(model, theta, y)
    np.testing.assert_allclose(ref['loss'][0], loss, rtol=1e-12)
    for q in H.QUANTITIES[1:]:
      if q == 'infl' and obs == 'NORMAL':
        continue
      got, den = ref[q]
      want = g[:, model.leaf[H.leaf_name(model, q)].offset]
      assert np.all(np.abs(got - want) <= 1e-12 * den), (obs, q, got, want)
