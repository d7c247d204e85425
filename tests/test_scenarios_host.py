"""CPU-only checks of the scenario reduction of sample paths (include/bnf.h bnf_sample_distances / bnf_scenario_select): the
numpy restatement of the kernels' own order against the brute-force references of tests/scenarios_ref.py at the bars the
GPU tests use; known answers of fast forward selection; that the generated cases have the gaps the GPU tests rely on; the
entry points' declarations and exports; their refusal without a handle; the estimators' argument checks; the work-bytes
formula."""
import itertools
import os
import re

import numpy as np
import pandas as pd
import pytest

from bayesnf_amd import BayesianNeuralFieldMAP, BayesianNeuralFieldVI, _native, inference
from tests import scenarios_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('kind', R.KINDS)
def test_distances_restated_against_the_brute_force(kind):
  worst = 0.0
  for S, C in ((1, 1), (2, 33), (65, 33), (33, 65)):
    for p, scaled, with_y in itertools.product(R.NORMS, (False, True), (False, True)):
      x, y, scale, ref = R.distance_case(S, C, kind, p, scaled, with_y)
      dist, ydist = R.distances_kernel_form(x, p, scale, y)
      worst = max(worst, R.check_distances(f'{kind} S={S} C={C} p={p} scale={scaled} y={with_y} restatement', dist, ydist,
                                           x, p, scale, y, ref))
      assert np.array_equal(dist, dist.T) and not np.diagonal(dist).any() and not np.signbit(np.diagonal(dist)).any()
      if kind == 'counts' and p == 1 and not scaled:
        assert np.array_equal(dist, ref[0])            # integers: exact
  print(f'{kind}: worst error / bar of the restatement {worst:.3f}')


def test_a_column_without_y_and_a_path_with_nan():
  x, y, scale, _ = R.distance_case(65, 33, 'normal', 2, True, True)
  xn = np.array(x)
  xn[:, 3] = np.nan                                    # y[3] is NaN: the column takes no part
  assert np.isnan(y[3])
  a, ay = R.distances_kernel_form(x, 2, scale, y)
  b, by = R.distances_kernel_form(xn, 2, scale, y)
  assert np.array_equal(a, b) and np.array_equal(ay, by)
  xn = np.array(x)
  xn[7, 0] = np.nan
  b, by = R.distances_kernel_form(xn, 2, scale, y)
  others = np.arange(65) != 7
  assert np.isnan(b[7]).all() and np.isnan(b[:, 7]).all() and np.isnan(by[7])
  assert np.array_equal(b[np.ix_(others, others)], a[np.ix_(others, others)]) and np.array_equal(by[others], ay[others])
  none, ny = R.distances_kernel_form(x, 1, None, np.full(33, np.nan))
  assert not none.any() and not ny.any()               # no participating column: +0.0 everywhere
  assert np.isnan(R.select_kernel_form(b, 3, by)['objective']).all() and (R.select_kernel_form(b, 3, by)['chosen'] == -1).all()


@pytest.mark.parametrize('kind', ('normal', 'big', 'clusters'))
def test_generated_cases_have_the_gaps_and_the_restatement_selects_like_the_brute_force(kind):
  """No normal, big or clusters case may fall below MIN_GAP: the GPU tests demand the reference's exact selection there."""
  for S, C in R.SELECT_SHAPES:
    for p in R.NORMS:
      x, y, ref, sel = R.selection_case(S, C, kind, p)
      k = len(sel['chosen'])
      assert np.all(sel['gaps'] >= R.MIN_GAP), (kind, S, C, p, sel['gaps'].tolist())
      assert 3 * R.objective_rel(S, C) < 1e-12
      got = R.scenarios_kernel_form(x, p, k, None, y)
      R.check_distances(f'{kind} S={S} C={C} p={p} restatement', got['dist'], got['ydist'], x, p, None, y, ref)
      R.check_selection(f'{kind} S={S} C={C} p={p} restatement', got, ref[0], k, C, ref[1], ref=sel, need_gaps=True,
                        own=(got['dist'], got['ydist']))


def test_counts_are_exact_ties_included():
  for S, C in ((65, 2), (257, 2), (129, 3)):
    x, y, ref, sel = R.selection_case(S, C, 'counts', 1, k=12)
    assert len(np.unique(x, axis=0)) < S
    got = R.scenarios_kernel_form(x, 1, 12, None, y)
    assert np.array_equal(got['dist'], ref[0]) and np.array_equal(got['ydist'], ref[1])
    R.check_selection(f'counts S={S} C={C} restatement', got, ref[0], 12, C, ref[1], exact=True, ref=sel)
    assert sel['gaps'].min() == 0.0 or len(np.unique(x, axis=0)) > 12     # ties do occur once the distinct paths run out
  for kind, S in itertools.product(('random', 'duplicates', 'equal', 'zero'), (1, 2, 65, 257)):
    d = R.integer_matrix(S, kind)
    for k in sorted({1, min(2, S), S if S <= 65 else 9}):
      got, ref = R.select_kernel_form(d, k), R.select_ref(d, k)
      for key in ('chosen', 'objective', 'prob', 'assign', 'nearest'):
        assert np.array_equal(got[key], ref[key]), (kind, S, k, key)
      if kind in ('equal', 'zero'):
        assert got['chosen'].tolist() == list(range(k))   # every candidate ties: the lowest index


def test_known_answers():
  x, _, _ = R.scenario_case(10, 4, 'clusters')
  for p in R.NORMS:
    dist, _ = R.distances_ref(x, p)
    sel = R.select_ref(dist, 3)
    blob = np.asarray([0, 0, 0, 0, 0, 1, 1, 1, 2, 2])
    assert sorted(blob[sel['chosen']].tolist()) == [0, 1, 2]               # one scenario per blob
    assert sorted(sel['prob'].tolist()) == [0.2, 0.3, 0.5]
    assert np.array_equal(blob[sel['chosen']][sel['assign']], blob)
    assert blob[sel['chosen'][0]] == 0                                       # the largest blob holds the medoid
  x, _, _ = R.scenario_case(33, 5, 'normal')
  dist, _ = R.distances_ref(x, 2)
  full = R.select_ref(dist, 33)
  assert sorted(full['chosen'].tolist()) == list(range(33)) and full['objective'][-1] == 0.0
  assert np.all(np.diff(full['objective']) <= 0) and np.all(full['prob'] == 1.0 / 33)
  assert full['chosen'][0] == int(np.argmin([np.sum(dist[:, u]) for u in range(33)]))      # the medoid
  assert np.array_equal(full['assign'], np.argsort(full['chosen']))
  for i in range(8):                                   # each step is the exhaustive best single addition to its prefix
    chosen = full['chosen'][:i].tolist()               # (two paths that only improve each other tie exactly: by value)
    best = min(np.sum(dist[:, chosen + [u]].min(axis=1)) / 33 for u in range(33) if u not in chosen)
    assert abs(full['objective'][i] - best) <= 64 * R.EPS * best
    if full['gaps'][i] >= R.MIN_GAP:
      objs = [np.sum(dist[:, chosen + [u]].min(axis=1)) if u not in chosen else np.inf for u in range(33)]
      assert full['chosen'][i] == int(np.argmin(objs))
  x, y, ref, sel = R.selection_case(65, 33, 'normal', 2)
  on_path = R.finish_ref(ref[0], sel['chosen'], ref[0][:, sel['chosen'][2]])    # the observed vector IS the third scenario
  assert on_path['obs_nearest'] == 2 and on_path['obs'][0] == 0.0 and on_path['obs'][2] == 0.0
  assert on_path['obs'][1] == np.sum(sel['nearest'] == 0) / 65.0


def test_entry_points_declared_listed_and_exported():
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'bnf.h')).read(), flags=re.S)
  lib = _native.load()
  for name, n_want in (('bnf_sample_distances', 9), ('bnf_scenario_select', 14)):
    m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)', src)
    assert m, f'{name} is not declared in include/bnf.h'
    n_args = len(m.group(1).split(','))
    assert n_args == n_want and name in _native.EXPORTS
    fn = getattr(lib, name)
    assert fn.argtypes is not None and len(fn.argtypes) == n_args
  assert _native.ABI_VERSION == 6 and lib.bnf_abi_version() == 6          # purely additive
  assert int(re.search(r'#define\s+BNF_SCENARIO_MAX_SAMPLES\s+(\d+)', src).group(1)) == _native.SCENARIO_MAX_SAMPLES == 4096
  from bayesnf_amd.engine import Engine
  assert callable(getattr(Engine, 'sample_distances', None)) and callable(getattr(Engine, 'scenario_select', None))
  assert callable(getattr(inference, 'scenario_summaries', None))
  for cls in (BayesianNeuralFieldMAP, BayesianNeuralFieldVI):
    assert callable(getattr(cls, 'predict_scenarios', None)) and callable(getattr(cls, 'score_scenarios', None))
    assert '`predict_scenarios`, `score_scenarios`' in cls.stacking_weights.__doc__
    for word in ('backward reduction', 'k-medoids', 'combinations=', '4,096'):
      assert word in cls.predict_scenarios.__doc__, word


def test_the_work_bytes_formula():
  """dmin and z (S f64 each), the taken marks (S int32), the flag and the pick (2 int32): 20 S + 16 covers them with the
  int32 block 8-byte aligned at either parity of S; the header states the same formula."""
  doc = open(os.path.join(ROOT, 'include', 'bnf.h')).read()
  assert '20 * n_samples + 16 bytes' in doc
  for S in (1, 2, 65, 4096):
    assert _native.scenario_work_bytes(S) == 20 * S + 16 >= 16 * S + 4 * (S + S % 2) + 8
  assert _native.scenario_work_bytes(4096) == 81936


def test_a_null_handle_is_refused_like_the_energy_score_refuses_it():
  lib = _native.load()
  want = lib.bnf_sample_energy_score(None, None, 4, 2, None, None, 0, None)
  message = _native.last_error()
  assert want < 0
  assert lib.bnf_sample_distances(None, None, 4, 2, None, None, 2, None, None) == want
  assert _native.last_error() == message
  assert lib.bnf_scenario_select(None, None, 4, 2, None, None, 0, None, None, None, None, None, None, None) == want
  assert _native.last_error() == message


def _frame():
  t = pd.date_range('2020-01-06', periods=4, freq='W-MON')
  return pd.DataFrame({'t': np.repeat(t, 3), 'place': np.tile(['a', 'b', 'c'], 4), 'y': np.arange(12.0)})


@pytest.mark.parametrize('cls', [BayesianNeuralFieldMAP, BayesianNeuralFieldVI])
def test_scenarios_refuse_bad_calls_before_any_gpu_work(cls, monkeypatch):
  df = _frame()
  est = cls(feature_cols=['t'], target_col='y', freq='W', width=64, observation_model='NB')
  for call in (est.predict_scenarios, est.score_scenarios):
    with pytest.raises(ValueError, match=f'{call.__name__} before fit'):
      call(df, 't')

  def no_gpu(*a, **k):
    raise AssertionError('GPU work was reached')
  monkeypatch.setattr(inference, '_ensemble_forecast', no_gpu)
  est.params_ = object()                          # "fitted": everything below must fail on its arguments alone
  with pytest.raises(ValueError, match='score_scenarios: the target column'):
    est.score_scenarios(df.drop(columns='y'), 't')
  with pytest.raises(ValueError, match='not among the columns'):
    est.predict_scenarios(df, 'week')
  for call in (est.predict_scenarios, est.score_scenarios):
    name = call.__name__
    with pytest.raises(ValueError, match=f'{name}: num_samples=0: need at least one sample path'):
      call(df, 't', num_samples=0)
    with pytest.raises(ValueError, match=f'{name}: num_samples=4097: the scenarios are chosen among at most 4096'):
      call(df, 't', num_samples=4097)
    for bad in (0, 11, 2.0, '3', None, True):
      with pytest.raises(ValueError, match=f'{name}: k=.*an integer in 1..10'):
        call(df, 't', k=bad, num_samples=10)
    for bad in (0, 3, 0.5, 'l2', None, True):
      with pytest.raises(ValueError, match=f'{name}: norm=.*formed for norm in \\(1, 2\\)'):
        call(df, 't', norm=bad)
    for bad, why in ((np.ones(3), 'one divisor per group \\(4,\\)'), (np.ones((4, 1)), 'one divisor per group'),
                     (2.0, 'one divisor per group'), ([1, 2, 0, 1], 'finite and > 0'), ([1, -2, 1, 1], 'finite and > 0'),
                     ([1, np.inf, 1, 1], 'finite and > 0'), ([1, np.nan, 1, 1], 'finite and > 0'),
                     (['a', 'b', 'c', 'd'], 'one positive finite number per group')):
      with pytest.raises(ValueError, match=f'{name}: scale must .*{why}'):
        call(df, 't', scale=bad)
    with pytest.raises(AssertionError, match='GPU work'):                # a good call reaches the GPU seam
      call(df, 't', k=np.int64(3), norm=1, scale=[1.0, 2.0, 3.0, 4.0], num_samples=4096)
  d = df.copy()
  d.loc[[0, 3, 6, 9], 'y'] = np.nan                 # every week holds a NaN target
  with pytest.raises(ValueError, match='score_scenarios: no group has an observed total'):
    est.score_scenarios(d, 't')
  with pytest.raises(AssertionError, match='GPU work'):                  # the forecast does not read the target
    est.predict_scenarios(d, 't')
  d = df.copy()
  d.loc[3, 'y'] = np.nan                            # one NaN target is no error
  with pytest.raises(AssertionError, match='GPU work'):
    est.score_scenarios(d, 't')
  groups = inference.csr_from_codes(np.arange(12) // 3, 4)
  call = lambda **kw: inference.scenario_summaries(np.zeros((12, 1)), 'NB', None, None, kw.pop('S', 10), 0, 2, groups, **kw)
  with pytest.raises(ValueError, match='at most 4096'):
    call(S=4097, k=3)
  with pytest.raises(ValueError, match='k=11'):
    call(k=11)
  with pytest.raises(ValueError, match='norm=3'):
    call(k=2, norm=3)
  with pytest.raises(ValueError, match='one divisor per group'):
    call(k=2, scale=np.ones(3))
  with pytest.raises(ValueError, match='finite and > 0'):
    call(k=2, scale=np.zeros(4))
  with pytest.raises(ValueError, match='one total per group'):
    call(k=2, observed=np.zeros(3))
  with pytest.raises(ValueError, match='no group has an observed total'):
    call(k=2, observed=np.full(4, np.nan))
  with pytest.raises(AssertionError, match='GPU work'):
    call(k=10, observed=np.array([1.0, np.nan, 2.0, 3.0]))


def test_what_the_estimators_add_on_the_host(monkeypatch):
  df = _frame()
  df.loc[[4], 'y'] = np.nan                       # week 1
  seen = {}

  def fake(features, observation_model, params, model_args, num_samples, seed, ensemble_dims, groups, k, norm=2,
           scale=None, observed=None, compute_dtype=None):
    seen.update(k=k, norm=norm, scale=scale, observed=observed, num_samples=num_samples)
    out = dict(scenarios=np.arange(8.0).reshape(2, 4), path=np.array([5, 1]), probability=np.array([0.75, 0.25]),
               distance=np.array([3.0, 1.0]), assignment=np.array([0, 1, 0, 0, 0, 0, 0, 1]))
    if observed is not None:
      out.update(nearest=1, nearest_distance=0.5, pit=np.array([0.25, 0.125]))
    return out
  monkeypatch.setattr(inference, 'scenario_summaries', fake)
  est = BayesianNeuralFieldMAP(feature_cols=['t'], target_col='y', freq='W', width=64, observation_model='NORMAL')
  est.params_ = object()
  res = est.predict_scenarios(df, 't', k=2, num_samples=8)
  assert set(res) == {'keys', 'scenarios', 'probability', 'path', 'distance', 'assignment'} and seen['observed'] is None
  assert (seen['k'], seen['norm'], seen['scale'], seen['num_samples']) == (2, 2, None, 8)
  assert list(res['keys']) == list(df['t'].unique())
  res = est.score_scenarios(df, 't', k=2, norm=1, scale=[1, 2, 3, 4], num_samples=8)
  want = df.groupby('t')['y'].sum(min_count=3).to_numpy()
  assert np.array_equal(res['observed'], want, equal_nan=True) and np.array_equal(seen['observed'], want, equal_nan=True)
  assert res['n'] == 3 and res['nearest'] == 1 and res['nearest_distance'] == 0.5 and res['pit'].tolist() == [0.25, 0.125]
  assert seen['norm'] == 1 and seen['scale'].dtype == np.float64 and seen['scale'].tolist() == [1.0, 2.0, 3.0, 4.0]
  assert set(res) == {'keys', 'scenarios', 'probability', 'path', 'distance', 'assignment', 'observed', 'n', 'nearest',
                      'nearest_distance', 'pit'}
