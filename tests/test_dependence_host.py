"""CPU-only checks of the covariance / variogram / variogram score of group totals (include/bnf.h bnf_sample_pair_moments):
the numpy restatement of the kernel's form against the brute-force references of tests/dependence_ref.py, at the bars the
GPU tests use (the restatement's own error is printed: the bars have slack); the entry point's declaration and export; its
refusal without a handle; the estimators' argument checks; that the score sees dependence."""
import os
import re

import numpy as np
import pandas as pd
import pytest

from bayesnf_amd import BayesianNeuralFieldMAP, BayesianNeuralFieldVI, _native, inference
from tests import dependence_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('kind', D.KINDS + ('big',))
def test_kernel_form_against_the_brute_force(kind):
  worst = {}
  for S, G in [(S, G) for S in D.HOST_S for G in D.HOST_G] + [(D.CHUNK + 1, D.TILE + 2)]:     # (the last: three tiles)
    x, y, ref = D.dependence_case(S, G, kind)
    for p in D.ORDERS:
      got = D.pair_moments_kernel_form(x, p, y)
      w = D.check_moments(f'{kind} S={S} G={G} p={p} restatement', got, x, y, p, ref)
      for k, v in w.items():
        worst[k] = max(worst.get(k, 0.0), v)
      assert np.array_equal(got['covariance'], got['covariance'].T) and np.array_equal(got['variogram'], got['variogram'].T)
      assert not np.diagonal(got['variogram']).any()
      if kind != 'normal' and p != 0.5:             # integer-valued x: every term and every sum is exact
        assert np.array_equal(got['variogram'], ref['vario'][p])
  print(f'{kind}: worst error / bar of the restatement {worst}')


def test_references_against_numpy_and_each_other():
  x, y, ref = D.dependence_case(1000, 9, 'normal')
  assert np.allclose(ref['cov'], np.cov(x.T, bias=True), rtol=1e-12, atol=0.0)
  assert np.allclose(ref['mean'], x.mean(axis=0), rtol=1e-13)
  # E|X - X'|^2 = var_i + var_j - 2 cov_ij + (m_i - m_j)^2: the variogram of order 2 from the moments
  var, m = np.diagonal(ref['cov']), ref['mean']
  want = var[:, None] + var[None, :] - 2 * ref['cov'] + (m[:, None] - m[None, :]) ** 2
  assert np.allclose(ref['vario'][2.0], want, rtol=1e-11, atol=1e-11)
  corr = D.correlation(ref['cov'])
  assert np.allclose(corr, np.corrcoef(x.T), rtol=1e-12) and np.all(np.abs(np.diagonal(corr) - 1.0) <= 4 * D.EPS)
  flat = np.array(x)
  flat[:, 2] = 7.0                                   # a column without spread: NaN in its row and column, 1 elsewhere
  c = D.correlation(D.cov_ref(flat)[0])
  assert np.isnan(c[2]).all() and np.isnan(c[:, 2]).all() and np.isfinite(np.delete(np.delete(c, 2, 0), 2, 1)).all()
  # a NaN y leaves its pairs out: the score on the kept columns alone
  keep = np.isfinite(y)
  assert not keep.all()
  for p in D.ORDERS:
    alone = D.score_ref(D.vario_ref(x[:, keep], p), y[keep], p)[0]
    assert ref['score'][p][0] == alone
  assert np.isnan(D.score_ref(ref['vario'][1.0], np.where(np.arange(9) == 0, 1.0, np.nan), 1.0)[0])


def test_the_score_sees_dependence():
  """x = 100 + f_s + e_sc, a factor of spread 10 shared by the 12 columns of a path; permuting every column over the
  paths keeps each marginal and removes the dependence.  The reference score of the permuted ensemble at p = 0.5 is at
  least 5 times that of x (measured over the seeds 0..19: never below 18; 85 at p = 1)."""
  x, shuffled, y = D.shared_factor_case(0)
  for p in (0.5, 1.0):
    good = D.score_ref(D.vario_ref(x, p), y, p)[0]
    bad = D.score_ref(D.vario_ref(shuffled, p), y, p)[0]
    print(f'p={p}: score {good:.4f}, columns permuted {bad:.4f}, ratio {bad / good:.1f}')
    assert bad >= 5 * good
  assert np.array_equal(np.sort(x, axis=0), np.sort(shuffled, axis=0))


def test_entry_point_declared_listed_and_exported():
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'bnf.h')).read(), flags=re.S)
  lib = _native.load()
  m = re.search(r'\bint\s+bnf_sample_pair_moments\s*\(([^)]*)\)', src)
  assert m, 'bnf_sample_pair_moments is not declared in include/bnf.h'
  n_args = len(m.group(1).split(','))
  assert n_args == 13 and 'bnf_sample_pair_moments' in _native.EXPORTS
  fn = lib.bnf_sample_pair_moments
  assert fn.argtypes is not None and len(fn.argtypes) == n_args
  assert _native.ABI_VERSION == 6 and lib.bnf_abi_version() == 6          # purely additive
  for macro, val in (('BNF_PAIR_COL_TILE', _native.PAIR_COL_TILE), ('BNF_PAIR_PATH_CHUNK', _native.PAIR_PATH_CHUNK),
                     ('BNF_PAIR_MATRIX_MAX_COLS', _native.PAIR_MATRIX_MAX_COLS)):
    assert int(re.search(r'#define\s+' + macro + r'\s+(\d+)', src).group(1)) == val
  assert (_native.PAIR_COL_TILE, _native.PAIR_PATH_CHUNK) == (D.TILE, D.CHUNK) and _native.PAIR_MATRIX_MAX_COLS == 4096
  assert _native.pair_work_doubles(1) == 1 and _native.pair_work_doubles(64) == 1 and _native.pair_work_doubles(65) == 3
  assert _native.pair_work_doubles(20000) == 313 * 314 // 2
  from bayesnf_amd.engine import Engine
  assert callable(getattr(Engine, 'sample_pair_moments', None))
  assert callable(getattr(inference, 'dependence_summaries', None))


def test_a_null_handle_is_refused_like_the_energy_score_refuses_it():
  lib = _native.load()
  want = lib.bnf_sample_energy_score(None, None, 4, 2, None, None, 0, None)
  message = _native.last_error()
  assert want < 0
  assert lib.bnf_sample_pair_moments(None, None, 4, 2, 0.5, None, None, None, None, None, None, 0, None) == want
  assert _native.last_error() == message


def _frame():
  t = pd.date_range('2020-01-06', periods=4, freq='W-MON')
  return pd.DataFrame({'t': np.repeat(t, 3), 'place': np.tile(['a', 'b', 'c'], 4), 'y': np.arange(12.0)})


@pytest.mark.parametrize('cls', [BayesianNeuralFieldMAP, BayesianNeuralFieldVI])
def test_dependence_refuses_bad_calls_before_any_gpu_work(cls, monkeypatch):
  df = _frame()
  est = cls(feature_cols=['t'], target_col='y', freq='W', width=64, observation_model='NB')
  with pytest.raises(ValueError, match='before fit'):
    est.predict_dependence(df, 't')
  with pytest.raises(ValueError, match='before fit'):
    est.score_dependence(df, 't')

  def no_gpu(*a, **k):
    raise AssertionError('GPU work was reached')
  monkeypatch.setattr(inference, '_ensemble_forecast', no_gpu)
  est.params_ = object()                          # "fitted": everything below must fail on its arguments alone
  with pytest.raises(ValueError, match='target column'):
    est.score_dependence(df.drop(columns='y'), 't')
  for bad in (0.5, -1.0):
    d = df.copy()
    d.loc[3, 'y'] = bad
    with pytest.raises(ValueError, match='non-negative integer'):
      est.score_dependence(d, 't')
  with pytest.raises(ValueError, match='not among the columns'):
    est.predict_dependence(df, 'week')
  for call in (est.score_dependence, est.predict_dependence):
    with pytest.raises(ValueError, match='at least one sample path'):
      call(df, 't', num_samples=0)
  with pytest.raises(ValueError, match='p=0.75'):
    est.score_dependence(df, 't', p=0.75)
  sym = np.ones((4, 4))
  for bad, why in ((np.ones((4, 3)), 'one weight per pair'), (np.ones(4), 'one weight per pair'),
                   (np.where(np.eye(4, k=1) > 0, -1.0, 1.0) * sym, '>= 0'), (np.triu(sym), 'symmetric'),
                   (np.where(np.eye(4) > 0, np.nan, 1.0), 'finite')):
    with pytest.raises(ValueError, match=why):
      est.score_dependence(df, 't', pair_weights=bad)
  groups = inference.csr_from_codes(np.arange(12) // 3, 4)
  with pytest.raises(ValueError, match='p=0.75'):
    inference.dependence_summaries(np.zeros((12, 1)), 'NB', None, None, 10, 0, 2, groups, p=0.75)
  with pytest.raises(ValueError, match='need `observed`'):
    inference.dependence_summaries(np.zeros((12, 1)), 'NB', None, None, 10, 0, 2, groups, pair_weights=sym)
  with pytest.raises(ValueError, match='one total per group'):
    inference.dependence_summaries(np.zeros((12, 1)), 'NB', None, None, 10, 0, 2, groups, observed=np.zeros(3))
  wide = inference.csr_from_codes(np.arange(4097), 4097)
  for kw in (dict(matrices=True), dict(matrices=False, observed=np.zeros(4097), pair_weights=np.ones((2, 2)))):
    with pytest.raises(ValueError, match='at most 4096'):
      inference.dependence_summaries(np.zeros((4097, 1)), 'NB', None, None, 10, 0, 2, wide, **kw)
  with pytest.raises(AssertionError, match='GPU work'):                  # the score alone takes more groups
    inference.dependence_summaries(np.zeros((4097, 1)), 'NB', None, None, 10, 0, 2, wide, matrices=False,
                                   observed=np.zeros(4097))
  big = inference.csr_from_codes(np.arange(1 << 15), 1 << 15)
  with pytest.raises(ValueError, match='held whole'):                    # 2^29 cells; no cap on the paths alone
    inference.dependence_summaries(np.zeros((1 << 15, 1)), 'NB', None, None, 16384, 0, 2, big, matrices=False)
  with pytest.raises(AssertionError, match='GPU work'):
    inference.dependence_summaries(np.zeros((12, 1)), 'NB', None, None, 100000, 0, 2, groups)
  d = df.copy()
  d.loc[3, 'y'] = np.nan                          # a NaN target is no error: it reaches the GPU seam
  with pytest.raises(AssertionError, match='GPU work'):
    est.score_dependence(d, 't', pair_weights=sym)


def test_what_the_estimators_add_on_the_host(monkeypatch):
  """observed is NaN exactly for the groups with a NaN target row; n, n_pairs, the mean score over the weights of the scored
  pairs, the observed variogram and the correlation are formed on the host from what the GPU seam returns."""
  df = _frame()
  df.loc[[4], 'y'] = np.nan                       # week 1
  x, _, ref = D.dependence_case(33, 9, 'normal')
  cov = np.array(ref['cov'][:4, :4])
  cov[2, :] = cov[:, 2] = 0.0                     # a group without spread
  seen = {}

  def fake(features, observation_model, params, model_args, num_samples, seed, ensemble_dims, groups, observed=None,
           p=0.5, pair_weights=None, matrices=True, compute_dtype=None):
    seen.update(observed=observed, p=p, pair_weights=pair_weights, matrices=matrices, num_samples=num_samples)
    out = dict(mean=np.arange(4.0))
    if matrices:
      out.update(covariance=cov, variogram=np.full((4, 4), 2.0))
    if observed is not None:
      out['variogram_score'] = 6.0
    return out
  monkeypatch.setattr(inference, 'dependence_summaries', fake)
  est = BayesianNeuralFieldMAP(feature_cols=['t'], target_col='y', freq='W', width=64, observation_model='NORMAL')
  est.params_ = object()
  res = est.predict_dependence(df, 't', num_samples=7)
  assert set(res) == {'keys', 'mean', 'std', 'covariance', 'correlation'} and seen['observed'] is None
  assert np.array_equal(res['std'], np.sqrt(np.diagonal(cov))) and res['std'][2] == 0.0
  assert np.array_equal(res['correlation'], D.correlation(cov), equal_nan=True)
  assert np.isnan(res['correlation'][2]).all() and np.isnan(res['correlation'][:, 2]).all()
  others = [0, 1, 3]
  assert np.all(np.abs(np.diagonal(res['correlation'])[others] - 1.0) <= 4 * D.EPS)
  assert list(res['keys']) == list(df['t'].unique())

  res = est.score_dependence(df, 't', p=1, num_samples=7)
  want = df.groupby('t')['y'].sum(min_count=3).to_numpy()
  assert np.array_equal(res['observed'], want, equal_nan=True) and np.array_equal(seen['observed'], want, equal_nan=True)
  assert (res['n'], res['n_pairs']) == (3, 3) and res['variogram_score'] == 6.0 and res['mean_variogram_score'] == 2.0
  ov = np.abs(want[:, None] - want[None, :])
  assert np.array_equal(res['observed_variogram'], ov, equal_nan=True) and np.isnan(res['observed_variogram'][1]).all()
  assert set(res) == {'keys', 'mean', 'std', 'covariance', 'correlation', 'observed', 'variogram', 'observed_variogram',
                      'variogram_score', 'n', 'n_pairs', 'mean_variogram_score'}
  w = np.arange(16.0).reshape(4, 4)
  w = w + w.T
  res = est.score_dependence(df, 't', p=0.5, pair_weights=w, matrices=False)
  assert set(res) == {'keys', 'mean', 'observed', 'variogram_score', 'n', 'n_pairs', 'mean_variogram_score'}
  assert res['mean_variogram_score'] == 6.0 / (w[0, 2] + w[0, 3] + w[2, 3]) and seen['matrices'] is False
  d2 = df.copy()
  d2.loc[[0, 3, 6], 'y'] = np.nan                 # one group left: no pair
  res = est.score_dependence(d2, 't', matrices=False)
  assert (res['n'], res['n_pairs']) == (1, 0) and np.isnan(res['mean_variogram_score'])
  keys = est.predict_dependence(df, ['place', 't'])['keys']
  assert isinstance(keys, pd.MultiIndex) and len(keys) == 12
