"""CPU-only checks of the posterior-predictive sampling feature: the two C-ABI entry points are declared, listed and
exported; the host builder of the rows-sorted-by-group layout is correct; `predict_samples` refuses bad calls before
any GPU work."""
import os
import re

import numpy as np
import pandas as pd
import pytest

from bayesnf_amd import BayesianNeuralFieldMAP, BayesianNeuralFieldVI, _native, inference, spatiotemporal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('bnf_predictive_samples', 'bnf_predictive_group_sums')


def test_entry_points_declared_listed_and_exported():
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'bnf.h')).read(), flags=re.S)
  lib = _native.load()
  for name in NAMES:
    assert re.search(r'\bint\s+' + name + r'\s*\(', src), f'{name} is not declared in include/bnf.h'
    assert name in _native.EXPORTS
    fn = getattr(lib, name)
    assert fn.argtypes is not None and len(fn.argtypes) == (10 if name == NAMES[0] else 15)
  assert _native.ABI_VERSION == 6 and lib.bnf_abi_version() == 6          # purely additive
  tile = int(re.search(r'#define\s+BNF_GROUP_TILE\s+(\d+)', src).group(1))
  assert tile == _native.GROUP_TILE


def _check_csr(codes, n_groups, seg_offsets, seg_rows):
  R = len(codes)
  assert seg_offsets.dtype == np.int32 and seg_rows.dtype == np.int32
  assert seg_offsets.shape == (n_groups + 1,) and seg_rows.shape == (R,)
  assert seg_offsets[0] == 0 and seg_offsets[-1] == R and np.all(np.diff(seg_offsets) >= 0)
  assert np.array_equal(np.sort(seg_rows), np.arange(R))                 # every row exactly once
  for g in range(n_groups):
    seg = seg_rows[seg_offsets[g]:seg_offsets[g + 1]]
    assert np.all(codes[seg] == g)                                        # ... inside its group's segment
    assert np.all(np.diff(seg) > 0)                                       # rows ascending inside a group
    assert len(seg) == np.sum(codes == g)


@pytest.mark.parametrize('seed', range(4))
def test_csr_from_codes_random_labels_with_empty_and_singleton_groups(seed):
  rng = np.random.default_rng(seed)
  R, G = 5000, 300
  codes = rng.integers(0, G, R)
  codes[codes % 7 == 3] = 5                      # the codes 3, 10, 17, ... are carried by nobody: empty groups
  codes[codes == 11] = 12
  codes[0] = 11                                  # a singleton
  assert np.sum(codes == 11) == 1 and np.sum(codes == 3) == 0
  off, rows = inference.csr_from_codes(codes, G)
  _check_csr(codes, G, off, rows)
  assert off[4] == off[3] and off[12] - off[11] == 1
  # one group holding everything; every row its own group
  _check_csr(np.zeros(17, dtype=int), 1, *inference.csr_from_codes(np.zeros(17, dtype=int), 1))
  _check_csr(np.arange(17)[::-1].copy(), 17, *inference.csr_from_codes(np.arange(17)[::-1].copy(), 17))
  for bad in (np.array([0, 3]), np.array([-1, 0]), np.array([0.5, 1.0]), np.zeros((2, 2), dtype=int)):
    with pytest.raises(ValueError):
      inference.csr_from_codes(bad, 3)


def test_group_rows_single_column_and_multiindex():
  rng = np.random.default_rng(7)
  R = 3000
  df = pd.DataFrame({'week': pd.to_datetime('2020-01-06') + pd.to_timedelta(7 * rng.integers(0, 40, R), unit='D'),
                     'county': rng.choice(['B', 'a', 'zz', 'M'], R), 'zone': rng.integers(0, 5, R),
                     'y': rng.standard_normal(R)})
  df.index = rng.permutation(R) + 100            # positions, not index labels, are what seg_rows holds
  keys, off, rows = spatiotemporal.group_rows(df, 'week')
  assert isinstance(keys, pd.Index) and keys.is_monotonic_increasing and keys.is_unique
  assert set(keys) == set(df['week'])
  _check_csr(keys.get_indexer(df['week']), len(keys), off, rows)
  keys2, off2, rows2 = spatiotemporal.group_rows(df, ['county', 'zone'])
  assert isinstance(keys2, pd.MultiIndex) and keys2.names == ['county', 'zone']
  assert keys2.is_monotonic_increasing and keys2.is_unique
  assert set(keys2) == set(zip(df['county'], df['zone']))
  _check_csr(keys2.get_indexer(pd.MultiIndex.from_frame(df[['county', 'zone']])), len(keys2), off2, rows2)
  # the totals a caller would form from the layout are the pandas group sums
  y = df['y'].to_numpy()
  tot = np.array([y[rows2[off2[g]:off2[g + 1]]].sum() for g in range(len(keys2))])
  want = df.groupby(['county', 'zone'])['y'].sum()
  np.testing.assert_allclose(tot, want.loc[keys2].to_numpy(), rtol=1e-12)
  for bad in ('nope', ['county', 'nope'], []):
    with pytest.raises(ValueError):
      spatiotemporal.group_rows(df, bad)


@pytest.mark.parametrize('cls', [BayesianNeuralFieldMAP, BayesianNeuralFieldVI])
def test_predict_samples_refuses_bad_calls_before_any_gpu_work(cls, monkeypatch):
  df = pd.DataFrame({'t': pd.date_range('2020-01-06', periods=8, freq='W-MON'), 'y': np.arange(8.0), 'g': list('aabbccdd')})
  est = cls(feature_cols=['t'], target_col='y', freq='W', width=64)
  with pytest.raises(ValueError, match='before fit'):
    est.predict_samples(df, 10)

  def no_gpu(*a, **k):
    raise AssertionError('GPU work was reached')
  seam = inference.sample_predictive
  monkeypatch.setattr(inference, 'sample_predictive', no_gpu)
  monkeypatch.setattr(inference, '_ensemble_forecast', no_gpu)
  est.params_ = object()                          # "fitted": everything below must fail on its arguments alone
  for n in (0, -3):
    with pytest.raises(ValueError, match='num_samples'):
      est.predict_samples(df, n)
  for bad in ('nope', ['g', 'nope']):
    with pytest.raises(ValueError, match='group_by'):
      est.predict_samples(df, 10, group_by=bad)
  with pytest.raises(ValueError, match='num_samples'):
    seam(np.zeros((8, 1)), 'NORMAL', None, {}, 0, 0, ensemble_dims=2)
