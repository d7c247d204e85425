"""CPU-only checks of the linear combinations of the sample paths (include/bnf.h bnf_predictive_combinations): the CSR
builder on its three spec forms and every refusal; the per-group combinations and their stacking on a hand-made frame;
the observed combinations; the entry point's declaration and export; the estimators' argument checks, which fire before
any GPU work; the host reference of tests/combinations_ref.py on a hand-worked case."""
import os
import re

import numpy as np
import pandas as pd
import pytest

from bayesnf_amd import BayesianNeuralFieldMAP, BayesianNeuralFieldVI, _native, inference, spatiotemporal
from tests import combinations_ref as Cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'bnf_predictive_combinations'
nan = np.nan

DENSE = np.asarray([[0.0, 2.0, 0.0, -1.0, 0.5],
                    [0.0, 0.0, 0.0, 0.0, 0.0],
                    [1.0, 1.0, 1.0, 1.0, 1.0],
                    [0.0, 0.0, 0.0, -3.0, 0.0]])
OFF, ROWS, COEF = [0, 3, 3, 8, 9], [1, 3, 4, 0, 1, 2, 3, 4, 3], [2.0, -1.0, 0.5, 1.0, 1.0, 1.0, 1.0, 1.0, -3.0]


def _same(got, keys, off=OFF, rows=ROWS, coef=COEF):
  k, o, r, c = got
  assert list(k) == list(keys)
  assert o.dtype == np.int32 and r.dtype == np.int32 and c.dtype == np.float64
  assert o.tolist() == off and r.tolist() == rows and c.tolist() == coef


def test_the_three_spec_forms_give_the_same_csr():
  got = inference.combinations_csr(DENSE, 5)
  _same(got, range(4))
  assert isinstance(got[0], pd.RangeIndex)
  _same(inference.combinations_csr(DENSE.tolist(), 5, names=['a', 'b', 'c', 'd']), 'abcd')
  by_name = inference.combinations_csr({'a': DENSE[0], 'b': DENSE[1], 'z': DENSE[2], 'd': DENSE[3]}, 5)
  _same(by_name, 'abzd')                                    # the dict's order, not sorted
  assert isinstance(by_name[0], pd.Index)
  # COO in a scrambled order, with explicit zeros: sorted by form, then by row; the zeros dropped; the empty form kept
  form, row = np.nonzero(np.ones_like(DENSE))
  rng = np.random.default_rng(0)
  p = rng.permutation(form.size)
  _same(inference.combinations_csr((form[p], row[p], DENSE[form[p], row[p]]), 5), range(4))
  # without the zeros and without names K = max(form) + 1; with names the trailing empty forms stay
  form, row = np.nonzero(DENSE)
  _same(inference.combinations_csr((form, row, DENSE[form, row]), 5), range(4))
  _same(inference.combinations_csr((form, row, DENSE[form, row]), 5, names=list('abcdef')), 'abcdef', off=OFF + [9, 9])
  first = inference.combinations_csr((form + 2, row, DENSE[form, row]), 5)        # empty forms first
  assert first[1].tolist() == [0, 0] + OFF and len(first[0]) == 6
  # all zero: every form empty, no position
  k, o, r, c = inference.combinations_csr(np.zeros((2, 5)), 5)
  assert o.tolist() == [0, 0, 0] and r.size == 0 and c.size == 0 and len(k) == 2
  # a row in several forms and in none is fine (row 2 only in form 2); integer input is taken
  _same(inference.combinations_csr((np.asarray([0, 0]), np.asarray([4, 0]), [1, 2]), 5), [0], [0, 2], [0, 4], [2.0, 1.0])


def test_combinations_csr_refusals():
  csr = inference.combinations_csr
  f, r, c = np.asarray([0, 1, 1]), np.asarray([0, 1, 2]), np.asarray([1.0, 2.0, 3.0])
  for bad in (nan, np.inf, -np.inf):
    with pytest.raises(ValueError, match='finite'):
      csr((f, r, np.asarray([1.0, bad, 3.0])), 5)
    d = DENSE.copy()
    d[1, 1] = bad
    with pytest.raises(ValueError, match='finite'):
      csr(d, 5)
    with pytest.raises(ValueError, match='finite'):
      csr({'a': d[1]}, 5)
  for bad in (-1, 5):
    with pytest.raises(ValueError, match=r'rows must lie in \[0, 5\)'):
      csr((f, np.asarray([0, bad, 2]), c), 5)
  with pytest.raises(ValueError, match='negative form index'):
    csr((np.asarray([0, -1, 1]), r, c), 5)
  with pytest.raises(ValueError, match='form index 1 with 1 names'):
    csr((f, r, c), 5, names=['only'])
  with pytest.raises(ValueError, match='repeated'):
    csr((np.asarray([0, 1, 1]), np.asarray([0, 2, 2]), c), 5)
  with pytest.raises(ValueError, match='repeated'):                      # also when one of the pair has coefficient 0
    csr((np.asarray([0, 1, 1]), np.asarray([0, 2, 2]), np.asarray([1.0, 0.0, 3.0])), 5)
  with pytest.raises(ValueError, match='one length'):
    csr((f, r, c[:2]), 5)
  with pytest.raises(ValueError, match='one length'):
    csr((f, r, c.reshape(3, 1)), 5)
  with pytest.raises(ValueError, match='1-d integer array'):
    csr((f.astype(np.float64), r, c), 5)
  with pytest.raises(ValueError, match='1-d integer array'):
    csr((f, r.reshape(1, 3), c), 5)
  with pytest.raises(ValueError, match='COO triple'):
    csr((f, r), 5)
  with pytest.raises(ValueError, match=r'dense spec must be \(K, 5\)'):
    csr(DENSE[:, :4], 5)
  with pytest.raises(ValueError, match=r'dense spec must be \(K, 5\)'):
    csr(DENSE[0], 5)
  with pytest.raises(ValueError, match=r'dense spec must be \(K, 5\)'):
    csr(np.zeros((0, 5)), 5)
  with pytest.raises(ValueError, match='3 names for 4 combinations'):
    csr(DENSE, 5, names=['a', 'b', 'c'])
  with pytest.raises(ValueError, match="'b' must hold one coefficient per row"):
    csr({'a': DENSE[0], 'b': DENSE[0, :4]}, 5)
  with pytest.raises(ValueError, match='names must be None'):
    csr({'a': DENSE[0]}, 5, names=['a'])
  with pytest.raises(ValueError, match='at least one combination'):
    csr({}, 5)
  with pytest.raises(ValueError, match='at least one combination'):
    csr((f[:0], r[:0], c[:0]), 5)
  with pytest.raises(ValueError, match='array of numbers'):
    csr([['x'] * 5], 5)
  with pytest.raises(ValueError, match='n_rows=0'):
    csr(DENSE, 0)


def test_too_many_positions_are_refused(monkeypatch):
  """nnz >= 2^31 is refused; exercised at a lowered cap, since 2^31 positions take 32 GB."""
  assert inference._COMBINATION_MAX_POSITIONS == 2 ** 31 - 1
  monkeypatch.setattr(inference, '_COMBINATION_MAX_POSITIONS', 8)
  with pytest.raises(ValueError, match='9 positions; at most 8'):
    inference.combinations_csr(DENSE, 5)
  form, row = np.nonzero(DENSE)
  with pytest.raises(ValueError, match='9 positions; at most 8'):
    inference.combinations_csr((form, row, DENSE[form, row]), 5)
  d = DENSE.copy()
  d[3, 3] = 0.0
  assert inference.combinations_csr(d, 5)[1][-1] == 8


def _frame():
  t = pd.date_range('2020-01-06', periods=4, freq='W-MON')
  return pd.DataFrame({'t': np.repeat(t, 3), 'place': np.tile(['a', 'b', 'c'], 4), 'y': np.arange(12.0),
                       'pop': np.tile([10.0, 30.0, 60.0], 4), 'net': np.tile([1.0, -1.0, 0.0], 4)})


def _dense(spec, K, R):
  form, row, coef = spec
  d = np.zeros((K, R))
  d[form, row] = coef
  return d


def test_group_combinations_and_stack_combinations():
  df = _frame()
  keys, spec = spatiotemporal.group_combinations(df, 'place')
  assert list(keys) == ['a', 'b', 'c'] and keys.name == 'place'
  d = _dense(spec, 3, 12)
  assert np.array_equal(d, (df['place'].to_numpy()[None, :] == np.asarray(['a', 'b', 'c'])[:, None]).astype(float))
  # weights by column name and by array; mean=True rows sum to 1
  tkeys, tspec = spatiotemporal.group_combinations(df, 't', weight='pop')
  assert len(tkeys) == 4 and np.array_equal(_dense(tspec, 4, 12)[1], np.r_[np.zeros(3), 10.0, 30.0, 60.0, np.zeros(6)])
  _, again = spatiotemporal.group_combinations(df, 't', weight=df['pop'].to_numpy())
  assert all(np.array_equal(a, b) for a, b in zip(tspec, again))
  _, mspec = spatiotemporal.group_combinations(df, 't', weight='pop', mean=True)
  m = _dense(mspec, 4, 12)
  assert np.array_equal(m[2], np.r_[np.zeros(6), 0.1, 0.3, 0.6, np.zeros(3)])
  np.testing.assert_allclose(m.sum(axis=1), 1.0, rtol=0, atol=1e-15)
  _, plain = spatiotemporal.group_combinations(df, 'place', mean=True)
  assert np.array_equal(_dense(plain, 3, 12), d / 4.0)
  # a MultiIndex grouping; the CSR builder takes the triple with the keys as names
  k2, s2 = spatiotemporal.group_combinations(df, ['place', 't'])
  assert isinstance(k2, pd.MultiIndex) and len(k2) == 12
  kk, off, rows, coef = inference.combinations_csr(spec, 12, names=keys)
  assert list(kk) == ['a', 'b', 'c'] and off.tolist() == [0, 4, 8, 12] and rows.tolist() == [0, 3, 6, 9, 1, 4, 7, 10, 2, 5, 8, 11]
  # refusals
  with pytest.raises(ValueError, match="mean=True: the weights of group 'c' sum to 0"):
    spatiotemporal.group_combinations(df, 'place', weight='net', mean=True)
  with pytest.raises(ValueError, match='sum to 0'):
    spatiotemporal.group_combinations(df, 't', weight='net', mean=True)       # 1 - 1 + 0
  spatiotemporal.group_combinations(df, 'place', weight='net')                # without mean: a contrast, fine
  with pytest.raises(ValueError, match="'area' is not among the columns"):
    spatiotemporal.group_combinations(df, 'place', weight='area')
  with pytest.raises(ValueError, match='one value per row'):
    spatiotemporal.group_combinations(df, 'place', weight=np.ones(3))
  with pytest.raises(ValueError, match='finite'):
    spatiotemporal.group_combinations(df, 'place', weight=np.r_[np.ones(11), nan])
  with pytest.raises(ValueError, match='not among the columns'):
    spatiotemporal.group_combinations(df, 'region')
  # a hierarchy: places, then the nation
  df['all'] = 'nation'
  hk, hs = spatiotemporal.stack_combinations(spatiotemporal.group_combinations(df, 'place'),
                                             spatiotemporal.group_combinations(df, 'all'),
                                             spatiotemporal.group_combinations(df, 't', weight='pop', mean=True))
  assert list(hk[:4]) == ['a', 'b', 'c', 'nation'] and len(hk) == 8 and list(hk[4:]) == list(tkeys)
  h = _dense(hs, 8, 12)
  assert np.array_equal(h[:3], d) and np.array_equal(h[3], np.ones(12)) and np.array_equal(h[4:], m)
  assert np.array_equal(h[3], h[:3].sum(axis=0))
  from_coo, from_dense = inference.combinations_csr(hs, 12, names=hk), inference.combinations_csr(h, 12)
  assert list(from_coo[0]) == list(hk) and all(np.array_equal(a, b) for a, b in zip(from_coo[1:], from_dense[1:]))
  with pytest.raises(ValueError, match='nothing to stack'):
    spatiotemporal.stack_combinations()
  with pytest.raises(ValueError, match='every part is'):
    spatiotemporal.stack_combinations((keys, spec), keys)


def test_observed_combinations_and_the_nan_rule():
  target = np.asarray([1.0, nan, 3.0, 4.0, 5.0])
  _, off, rows, coef = inference.combinations_csr(DENSE, 5)
  got = spatiotemporal.combination_target_sums(target, off, rows, coef)
  # form 0 names row 1 (NaN target); form 1 is empty; form 2 names every row; form 3 row 3 only
  assert np.array_equal(got, [nan, 0.0, nan, -12.0], equal_nan=True)
  target[1] = 7.0
  assert spatiotemporal.combination_target_sums(target, off, rows, coef).tolist() == [12.5, 0.0, 20.0, -12.0]


def test_score_combinations_assembles_observed(monkeypatch):
  """'observed' = sum coef x target; NaN when a row with a nonzero coefficient has a NaN target, and only then: the
  combination whose NaN row has coefficient 0 is scored."""
  df = _frame()
  df.loc[4, 'y'] = nan                                      # week 1, place b
  seen = {}

  def fake(features, observation_model, params, model_args, num_samples, seed, ensemble_dims, combinations, observed=None,
           quantiles=(), energy=True, samples=False, compute_dtype=None, weights=None):
    seen.update(combinations=combinations, observed=observed, energy=energy, samples=samples, n=num_samples)
    K = len(combinations[0]) - 1
    out = {'mean': np.zeros(K), 'quantiles': np.zeros((len(quantiles), K))}
    if observed is not None:
      out.update(crps=np.where(np.isnan(observed), nan, 2.0), pit=np.zeros((2, K)))
      if energy:
        out['energy_score'] = 1.5
    if samples:
      out['samples'] = np.zeros((num_samples, K))
    return out
  monkeypatch.setattr(inference, 'combination_summaries', fake)
  est = BayesianNeuralFieldMAP(feature_cols=['t'], target_col='y', freq='W', width=64, observation_model='NORMAL')
  est.params_ = object()
  skip_b = np.ones(12)
  skip_b[[1, 4, 7, 10]] = 0.0                               # every row of place b has coefficient 0
  spec = {'all': np.ones(12), 'not b': skip_b, 'week 3 - week 0': np.r_[-np.ones(3), np.zeros(6), np.ones(3)],
          'nothing': np.zeros(12)}
  res = est.score_combinations(df, spec, num_samples=7, seed=1)
  y = df['y'].to_numpy()
  assert list(res['keys']) == list(spec)
  assert np.array_equal(res['observed'], [nan, y[skip_b > 0].sum(), 27.0, 0.0], equal_nan=True)
  assert np.array_equal(seen['observed'], res['observed'], equal_nan=True)
  off, rows, coef = seen['combinations']
  assert off.tolist() == [0, 12, 20, 26, 26] and rows[12:20].tolist() == [0, 2, 3, 5, 6, 8, 9, 11]
  assert res['n'] == 3 and res['mean_crps'] == 2.0 and res['energy_score'] == 1.5 and seen['samples'] is False
  assert set(res) == {'keys', 'mean', 'quantiles', 'observed', 'crps', 'pit', 'n', 'mean_crps', 'energy_score'}
  assert res['quantiles'].shape == (3, 4)
  assert 'energy_score' not in est.score_combinations(df, spec, num_samples=7, energy=False)
  # predict: no target needed, 'samples' on request; the (keys, triple) form of group_combinations is taken as it is
  part = spatiotemporal.group_combinations(df, 'place', weight='pop', mean=True)
  pred = est.predict_combinations(df.drop(columns='y'), part, num_samples=5, samples=True)
  assert set(pred) == {'keys', 'mean', 'quantiles', 'samples'} and pred['samples'].shape == (5, 3)
  assert list(pred['keys']) == ['a', 'b', 'c'] and seen['observed'] is None and seen['energy'] is False
  assert seen['combinations'][2].tolist() == [0.25] * 12
  assert set(est.predict_combinations(df, (np.asarray([1]), np.asarray([3]), [2.0]))) == {'keys', 'mean', 'quantiles'}
  assert seen['combinations'][0].tolist() == [0, 0, 1]


def test_entry_point_declared_listed_and_exported():
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'bnf.h')).read(), flags=re.S)
  lib = _native.load()
  assert re.search(r'\bint\s+' + NAME + r'\s*\(', src), f'{NAME} is not declared in include/bnf.h'
  assert NAME in _native.EXPORTS
  fn = getattr(lib, NAME)
  assert fn.argtypes is not None and len(fn.argtypes) == 17
  assert _native.ABI_VERSION == 6 and lib.bnf_abi_version() == 6          # purely additive
  from bayesnf_amd.engine import Engine
  assert callable(getattr(Engine, 'predictive_combinations', None))
  assert callable(getattr(inference, 'combination_summaries', None)) and callable(getattr(inference, 'combinations_csr', None))
  # an unbound handle is refused with the code bnf_predictive_group_sums gives
  args = (None, None, None, 2, 4, None, None)
  assert (fn(*args, None, 1, 1, 0, 0, 0, None, None, 0, None)
          == lib.bnf_predictive_group_sums(*args, 1, 1, 0, 0, 0, None, 0, None) != 0)
  # the contract is in the header, above the declaration
  text = open(os.path.join(ROOT, 'include', 'bnf.h')).read()
  doc = text[:text.index('int ' + NAME)].rsplit('/*', 1)[1]
  for word in ('COEFFICIENT', 'OVERLAP', 'EMPTY', 'NaN', 'DETERMINISM', 'BNF_ERR_INVALID'):
    assert word in doc, word
  assert 'bnf_combinations.h' in open(os.path.join(ROOT, 'bayesnf_amd', 'csrc', 'Makefile')).read()


def _params(lead):
  return (np.zeros(lead + (3,)), np.zeros(lead))


@pytest.mark.parametrize('cls,lead', [(BayesianNeuralFieldMAP, (1, 4)), (BayesianNeuralFieldVI, (1, 5, 2))])
def test_combinations_refuse_bad_calls_before_any_gpu_work(cls, lead, monkeypatch):
  df = _frame()
  est = cls(feature_cols=['t'], target_col='y', freq='W', width=64, observation_model='NB')
  spec = {'all': np.ones(12), 'a - b': df['net'].to_numpy()}
  for call in (est.predict_combinations, est.score_combinations):
    with pytest.raises(ValueError, match='before fit'):
      call(df, spec)

  def no_gpu(*a, **k):
    raise AssertionError('GPU work was reached')
  monkeypatch.setattr(inference, '_ensemble_forecast', no_gpu)
  est.params_ = _params(lead)                      # "fitted": everything below must fail on its arguments alone
  good = np.full(lead, 1.0 / np.prod(lead))
  for call in (est.predict_combinations, est.score_combinations):
    what = call.__name__
    with pytest.raises(ValueError, match='combinations are summarised from at most 16384'):
      call(df, spec, num_samples=16385)
    for n in (0, -2):
      with pytest.raises(ValueError, match='at least one sample path'):
        call(df, spec, num_samples=n)
    for bad, msg in (({'x': np.ones(11)}, 'one coefficient per row'), ({'x': np.r_[np.ones(11), nan]}, 'finite'),
                     (np.ones((2, 13)), 'dense spec'), ((np.asarray([0]), np.asarray([12]), [1.0]), 'rows must lie'),
                     ((np.asarray([-1]), np.asarray([0]), [1.0]), 'negative form'),
                     ((np.asarray([0, 0]), np.asarray([3, 3]), [1.0, 2.0]), 'repeated'), ({}, 'at least one'),
                     ((['a', 'b'], (np.asarray([2]), np.asarray([0]), [1.0])), 'form index 2 with 2 names')):
      with pytest.raises(ValueError, match=f'{what}: combinations: .*{msg}'):
        call(df, bad)
    for bad, msg in ((good.reshape(-1), 'shape'), (good * 1.001, 'sum to 1'), (-good, '>= 0')):
      with pytest.raises(ValueError, match=msg):
        call(df, spec, weights=bad)
    with pytest.raises(ValueError, match=r'\[0, 1\]'):
      call(df, spec, quantiles=(0.5, 1.5))
    for kw in (dict(weights=good, num_samples=5), dict(num_samples=16384), dict(quantiles=())):
      with pytest.raises(AssertionError, match='GPU work'):      # a good call passes the checks and reaches the GPU seam
        call(df, spec, **kw)
    with pytest.raises(AssertionError, match='GPU work'):
      call(df, spatiotemporal.group_combinations(df, 'place', weight='pop', mean=True))
  with pytest.raises(AssertionError, match='GPU work'):
    est.predict_combinations(df, spec, samples=True)
  with pytest.raises(ValueError, match='target column'):
    est.score_combinations(df.drop(columns='y'), spec)
  with pytest.raises(AssertionError, match='GPU work'):         # predict needs no target
    est.predict_combinations(df.drop(columns='y'), spec)
  d = df.copy()
  d.loc[3, 'y'] = 2.5
  with pytest.raises(ValueError, match='non-negative integer'):
    est.score_combinations(d, spec)
  d.loc[3, 'y'] = np.nan                            # a NaN target is no error: it reaches the GPU seam
  with pytest.raises(AssertionError, match='GPU work'):
    est.score_combinations(d, spec)
  # the cell cap: S x K <= 2^28
  wide = pd.DataFrame({'t': pd.Timestamp('2020-01-06'), 'place': np.arange(1 << 15), 'y': 0.0})
  singles = spatiotemporal.group_combinations(wide, 'place')
  with pytest.raises(ValueError, match='predict_combinations: 16384 sample paths x 32768 combinations'):
    est.predict_combinations(wide, singles, num_samples=16384)
  with pytest.raises(AssertionError, match='GPU work'):
    est.predict_combinations(wide, singles, num_samples=8192)
  # the seam's own checks
  _, off, rows, coef = inference.combinations_csr(spec, 12)
  seam = lambda *a, **k: inference.combination_summaries(np.zeros((12, 1)), 'NB', est.params_, None, *a, **k)
  with pytest.raises(ValueError, match='combinations are summarised from at most 16384'):
    seam(16385, 0, len(lead), (off, rows, coef))
  with pytest.raises(ValueError, match='at least one sample path'):
    seam(0, 0, len(lead), (off, rows, coef))
  _, woff, wrows, wcoef = inference.combinations_csr(singles[1], 1 << 15)
  with pytest.raises(ValueError, match='matrix of combinations is held whole'):
    inference.combination_summaries(np.zeros((1 << 15, 1)), 'NB', est.params_, None, 16384, 0, len(lead), (woff, wrows, wcoef))
  with pytest.raises(ValueError, match='one value per group'):
    seam(10, 0, len(lead), (off, rows, coef), observed=np.zeros(3))
  with pytest.raises(ValueError, match=r'\[0, 1\]'):
    seam(10, 0, len(lead), (off, rows, coef), quantiles=(-0.1,))
  with pytest.raises(ValueError, match='sum to 1'):
    seam(10, 0, len(lead), (off, rows, coef), weights=good * 2)
  with pytest.raises(AssertionError, match='GPU work'):
    seam(10, 0, len(lead), (off, rows, coef), observed=np.zeros(2), samples=True)


def test_reference_on_a_hand_worked_case():
  x = np.asarray([[1.0, 2.0, 3.0, 4.0, 5.0], [0.5, nan, 0.0, -1.0, 2.0]], dtype=np.float32)
  val, ab = Cr.combine_ref(x, OFF, ROWS, COEF)
  assert np.array_equal(val, [[2.5, 0.0, 15.0, -12.0], [nan, 0.0, nan, 3.0]], equal_nan=True)
  assert np.array_equal(ab[0], [10.5, 0.0, 15.0, 12.0])
  assert np.array_equal(Cr.bar(OFF, ab)[0], np.asarray([4, 1, 6, 2]) * 2.0 ** -52 * ab[0])
  # a row outside the table adds nothing; a row twice adds twice
  val, ab = Cr.combine_ref(x[:1], [0, 3], [7, 2, 2], [9.0, 1.0, -0.5])
  assert val.tolist() == [[1.5]] and ab.tolist() == [[4.5]]
  # cancellation: fsum is exact where a running sum is not
  big = np.asarray([[1e16, 1.0, -1e16]])
  assert Cr.combine_ref(big, [0, 3], [0, 1, 2], [1.0, 1.0, 1.0])[0].tolist() == [[1.0]]
