"""CPU-only checks of the helpers the path forecasts share (DESIGN.md "Adding a path forecast"): the size of the work
buffer of the three group reductions, the estimators' per-row threshold and the set-up of everything that draws sample
paths.  No GPU and no library load."""
import numpy as np
import pandas as pd
import pytest

from bayesnf_amd import _native, engine, inference
from bayesnf_amd.spatiotemporal import BayesianNeuralFieldEstimator


# ---- the work buffer of bnf_predictive_group_sums / _extremes / _episodes ---------------------------------------------
def _sums_bytes(R, n_samples):
  """The group sums as they sized their buffer of doubles: two per tile and path, 64 MB worth of paths, 8 bytes each."""
  per_path = 2 * (-(-R // _native.GROUP_TILE))
  return per_path * max(1, min(n_samples, (64 << 20) // (8 * per_path))) * 8


def _extremes_bytes(R, n_samples):
  per_path = _native.EXTREMES_WORK_PER_TILE * (-(-R // _native.GROUP_TILE))
  return per_path * max(1, min(n_samples, (64 << 20) // per_path))


def _episodes_bytes(R, n_samples):
  per_path = _native.EPISODES_WORK_PER_TILE * (-(-R // _native.GROUP_TILE))
  return per_path * max(1, min(n_samples, (64 << 20) // per_path))


@pytest.mark.parametrize('R', [1, 1023, 1024, 1025, 1_000_000])
@pytest.mark.parametrize('n_samples', [1, 7, 100_000])
def test_group_work_bytes_is_what_each_reduction_computed(R, n_samples):
  assert engine.group_work_bytes(16, R, n_samples) == _sums_bytes(R, n_samples)
  assert engine.group_work_bytes(_native.EXTREMES_WORK_PER_TILE, R, n_samples) == _extremes_bytes(R, n_samples)
  assert engine.group_work_bytes(_native.EPISODES_WORK_PER_TILE, R, n_samples) == _episodes_bytes(R, n_samples)


# ---- the threshold of predict_extremes / score_extremes / predict_episodes / score_episodes ------------------------------
def test_row_threshold_broadcasts_a_scalar_and_rounds_to_float32():
  table = pd.DataFrame({'x': np.arange(5.0)})
  thr = BayesianNeuralFieldEstimator._row_threshold
  got = thr('predict_episodes', table, 0.1, True)
  assert got.dtype == np.float64 and got.shape == (5,)
  assert np.array_equal(got, np.full(5, np.float64(np.float32(0.1))))
  per_row = [0.1, 2.0, -3.5, 1e-3, 7.0]
  got = thr('predict_extremes', table, per_row, False)
  assert got.dtype == np.float64 and got.shape == (5,)
  assert np.array_equal(got, np.asarray(per_row, dtype=np.float32).astype(np.float64))
  assert np.array_equal(thr('predict_extremes', table, got, False), got)        # float32 values pass through unchanged
  assert thr('predict_extremes', table, None, False) is None
  with pytest.raises(ValueError, match='predict_episodes: threshold is required: a number or one number per row of the '
                                       'table'):
    thr('predict_episodes', table, None, True)


@pytest.mark.parametrize('bad,text', [
    ('high', 'score_extremes: threshold must be a number or one number per row of the table'),
    ([1.0, 2.0], r'score_extremes: threshold must be a scalar or hold one limit per row \(5,\); got \(2,\)'),
    (np.zeros((5, 1)), r'score_extremes: threshold must be a scalar or hold one limit per row \(5,\); got \(5, 1\)'),
    ([1.0, 2.0, np.inf, 0.0, 0.0], 'score_extremes: threshold must be finite'),
])
def test_row_threshold_refuses_bad_input_with_the_methods_texts(bad, text):
  table = pd.DataFrame({'x': np.arange(5.0)})
  for required in (False, True):
    with pytest.raises(ValueError, match=text):
      BayesianNeuralFieldEstimator._row_threshold('score_extremes', table, bad, required)


# ---- the set-up of everything that draws sample paths -------------------------------------------------------------------
class _FakeEngine:
  def __init__(self):
    self.closed = 0

  def close(self):
    self.closed += 1


def _patch_forecast(monkeypatch, M=3, R=4):
  eng, calls = _FakeEngine(), []

  def forecast(features, observation_model, params, model_args, ensemble_dims, compute_dtype):
    calls.append((np.shape(features), observation_model, ensemble_dims, compute_dtype))
    return None, eng, (1, M), np.zeros((1, M, R), dtype=np.float32), np.zeros((1, M, 3), dtype=np.float32)

  monkeypatch.setattr(inference, '_ensemble_forecast', forecast)
  params = [np.zeros((1, M, 2))]
  return eng, calls, params, np.zeros((R, 2))


def test_sample_paths_closes_the_engine_and_passes_cum_weights_only_with_weights(monkeypatch):
  eng, calls, params, features = _patch_forecast(monkeypatch)
  with inference._sample_paths(features, 'NB', params, {}, 2, 'bf16', None, 5) as (e, loc, aux, seed64, kw):
    assert e is eng and eng.closed == 0
    assert loc.shape == (3, 4) and aux.shape == (3, 3)
    assert seed64 == 5 and kw == {}
  assert eng.closed == 1
  assert calls == [((4, 2), 'NB', 2, 'bf16')]

  w = np.array([[0.5, 0.25, 0.25]])
  with inference._sample_paths(features, 'NB', params, {}, 2, None, w, 5) as (_, _, _, _, kw):
    assert list(kw) == ['cum_weights']
    assert np.array_equal(kw['cum_weights'], [0.5, 0.75, 1.0])
  assert eng.closed == 2

  with pytest.raises(RuntimeError, match='in the body'):
    with inference._sample_paths(features, 'NB', params, {}, 2, None, None, 5):
      raise RuntimeError('in the body')
  assert eng.closed == 3


def test_sample_paths_checks_the_weights_before_the_forward_pass(monkeypatch):
  eng, calls, params, features = _patch_forecast(monkeypatch)
  with pytest.raises(ValueError, match='weights must sum to 1'):
    with inference._sample_paths(features, 'NB', params, {}, 2, None, np.array([[0.5, 0.25, 0.5]]), 5):
      pass
  assert calls == [] and eng.closed == 0
