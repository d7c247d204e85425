"""CPU-only checks of the ranking of group totals (include/bnf.h bnf_sample_ranks / bnf_rank_probabilities): the numpy
restatement of the kernel's form against the brute-force references of tests/ranking_ref.py at the bars the GPU tests use;
the references against numpy and each other; the tie and NaN rules on a hand-written row; the entry points' declaration and
export; their refusal without a handle; the estimators' argument checks and what they add on the host; that the score sees
the ranking."""
import os
import re

import numpy as np
import pandas as pd
import pytest

from bayesnf_amd import BayesianNeuralFieldMAP, BayesianNeuralFieldVI, _native, inference
from bayesnf_amd.spatiotemporal import group_target_ranks
from tests import ranking_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('kind', R.KINDS)
def test_kernel_form_against_the_brute_force(kind):
  """rank_prob: the restatement within (S + 8) eps of a Fraction per cell; the longdouble route (the reference of the GPU
  grid) within one ulp of the Fraction route; rows and columns sum to 1."""
  worst, last_bit, cells = 0.0, 0, 0
  for S, G in ((1, 1), (2, 3), (33, 9), (257, 5), (31, 65)):
    for scaled in (False, True):
      x, scale, ref = R.ranking_case(S, G, kind, scaled)
      R.check_ranks(f'{kind} S={S} G={G} brute force', ref, ref)
      for K in sorted({1, min(2, G), G}):
        exact = R.rank_prob_ref(ref['above'], ref['ties'], K)
        wide, form = R.prob_case(S, G, kind, scaled, K)
        assert np.all(np.abs(wide - exact) <= R.EPS * exact), (kind, S, G, K, 'longdouble route')
        last_bit, cells = last_bit + int((wide != exact).sum()), cells + exact.size
        assert R.same_bits(form, R.rank_prob_kernel_form_dense(ref['above'], ref['ties'], K)), (kind, S, G, K, 'dense form')
        w, _ = R.check_prob(f'{kind} S={S} G={G} K={K} restatement', form, S, exact)
        worst = max(worst, w)
        assert np.all(np.abs(form.sum(axis=1) - 1.0) <= 3e-15)
        if K == G:
          assert np.all(np.abs(form.sum(axis=0) - 1.0) <= 3e-15)
          assert R.same_bits(form[:min(2, G)], R.prob_case(S, G, kind, scaled, min(2, G))[1])
  print(f'{kind}: worst error / bar of the restatement {worst:.3f}; the longdouble route differs from the Fraction in '
        f'{last_bit} of {cells} cells')


def test_rows_and_columns_of_count_totals_sum_to_one():
  """Poisson(0.7) totals at S = 257, G = 65: most cells tie, every rank slot is still handed out exactly once per path."""
  x, _, ref = R.ranking_case(257, 65, 'count')
  assert (ref['ties'] > 1).mean() > 0.9
  form = R.prob_case(257, 65, 'count', False, 65)[1]
  rows, cols = np.abs(form.sum(axis=1) - 1.0).max(), np.abs(form.sum(axis=0) - 1.0).max()
  print(f'rank_prob sums: rows within {rows:.2e}, columns within {cols:.2e} of 1')
  assert rows <= 3e-15 and cols <= 3e-15


def test_references_against_numpy_and_each_other():
  x, _, ref = R.ranking_case(33, 257, 'normal')
  assert np.all(ref['ties'] == 1)
  assert np.array_equal(ref['above'], 257 - 1 - np.argsort(np.argsort(x, axis=1), axis=1))
  for kind in R.KINDS:                                # the sort route of the G = 16,384 case against the brute force
    for scaled in (False, True):
      x, scale, ref = R.ranking_case(33, 257, kind, scaled)
      rank, above, ties = R.ranks_sorted(x, scale)
      assert np.array_equal(above, ref['above']) and np.array_equal(ties, ref['ties']) and np.array_equal(rank, ref['rank'])
  x, _, ref = R.ranking_case(33, 9, 'edge')
  assert np.all(ref['ties'][0] == 9) and np.all(ref['above'][0] == 0) and np.all(ref['rank'][0] == 5.0)      # all equal
  assert np.array_equal(np.sort(ref['rank'][1]), np.arange(1.0, 10.0))                                        # all distinct
  assert np.isnan(x).any() and np.isinf(x).any() and (np.signbit(x) & (x == 0)).any()


def test_the_tie_and_nan_rules_on_a_hand_written_row():
  row = np.asarray([[np.nan, -np.inf, 0.0, -0.0, 3.0, np.nan]])
  for route in (R.ranks_brute, R.ranks_sorted):
    rank, above, ties = route(row)
    assert above[0].tolist() == [4, 3, 1, 1, 0, 4] and ties[0].tolist() == [2, 1, 2, 2, 1, 2]
    assert rank[0].tolist() == [5.5, 4.0, 2.5, 2.5, 1.0, 5.5] and rank.sum() == 21.0
  rank, above, ties = R.ranks_brute(np.asarray([[np.inf, 1.0, np.inf]]))
  assert above[0].tolist() == [0, 2, 0] and ties[0].tolist() == [2, 1, 2]
  # the divisor: 6 / 3 ties with 4 / 2
  rank, above, ties = R.ranks_brute(np.asarray([[6.0, 4.0, 1.0]]), np.asarray([3.0, 2.0, 0.25]))
  assert above[0].tolist() == [1, 1, 0] and ties[0].tolist() == [2, 2, 1]
  # the host helper: the same rule, NaN groups left out
  rank, above, ties = group_target_ranks(np.asarray([3.0, np.nan, 6.0, 6.0, -0.0, 0.0]))
  assert above.tolist() == [2, -1, 0, 0, 3, 3] and ties.tolist() == [1, -1, 2, 2, 2, 2]
  assert np.array_equal(rank, [3.0, np.nan, 1.5, 1.5, 4.5, 4.5], equal_nan=True)
  rank, above, ties = group_target_ranks(np.asarray([6.0, 4.0, np.nan]), np.asarray([3.0, 2.0, 1.0]))
  assert above.tolist() == [0, 0, -1] and ties.tolist() == [2, 2, -1]
  x, _, ref = R.ranking_case(33, 9, 'count')
  for s in range(33):
    got = group_target_ranks(x[s])
    assert np.array_equal(got[0], ref['rank'][s]) and np.array_equal(got[1], ref['above'][s])
  with pytest.raises(ValueError, match='one divisor per group'):
    group_target_ranks(np.zeros(3), np.ones(2))


def test_entry_points_declared_listed_and_exported():
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'bnf.h')).read(), flags=re.S)
  lib = _native.load()
  for name, n_args in (('bnf_sample_ranks', 8), ('bnf_rank_probabilities', 7)):
    m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)', src)
    assert m, f'{name} is not declared in include/bnf.h'
    assert len(m.group(1).split(',')) == n_args and name in _native.EXPORTS
    fn = getattr(lib, name)
    assert fn.argtypes is not None and len(fn.argtypes) == n_args
  assert _native.ABI_VERSION == 6 and lib.bnf_abi_version() == 6          # purely additive
  macro = lambda name: re.search(r'#define\s+' + name + r'\s+(.+)', src).group(1).strip()
  assert int(macro('BNF_RANK_MAX_COLS')) == _native.RANK_MAX_COLS == R.MAX_COLS == 16384
  assert int(macro('BNF_RANK_PATH_CHUNK')) == _native.RANK_PATH_CHUNK == R.CHUNK == 32
  assert re.fullmatch(r'\(1 << 24\)', macro('BNF_RANK_MAX_CELLS')) and _native.RANK_MAX_CELLS == R.MAX_CELLS == 1 << 24
  from bayesnf_amd.engine import Engine
  assert callable(getattr(Engine, 'sample_ranks', None)) and callable(getattr(Engine, 'rank_probabilities', None))
  assert callable(getattr(inference, 'ranking_summaries', None))
  header = open(os.path.join(ROOT, 'bayesnf_amd', 'csrc', 'Makefile')).read()
  assert 'bnf_ranking.h' in re.search(r'^HDR\s*:=(.*)$', header, flags=re.M).group(1)


def test_a_null_handle_is_refused_like_the_energy_score_refuses_it():
  lib = _native.load()
  want = lib.bnf_sample_energy_score(None, None, 4, 2, None, None, 0, None)
  message = _native.last_error()
  assert want < 0
  assert lib.bnf_sample_ranks(None, None, 4, 2, None, None, None, None) == want
  assert _native.last_error() == message
  assert lib.bnf_rank_probabilities(None, None, None, 4, 2, 1, None) == want
  assert _native.last_error() == message


def _frame():
  t = pd.date_range('2020-01-06', periods=4, freq='W-MON')
  return pd.DataFrame({'t': np.repeat(t, 3), 'place': np.tile(['a', 'b', 'c'], 4), 'y': np.arange(12.0),
                       'pop': np.tile([10.0, 20.0, 5.0], 4)})


def _params(lead):
  return (np.zeros(lead + (3,)), np.zeros(lead))


@pytest.mark.parametrize('cls,lead', [(BayesianNeuralFieldMAP, (1, 4)), (BayesianNeuralFieldVI, (1, 5, 2))])
def test_ranking_refuses_bad_calls_before_any_gpu_work(cls, lead, monkeypatch):
  df = _frame()
  est = cls(feature_cols=['t'], target_col='y', freq='W', width=64, observation_model='NB')
  for call in (est.predict_ranking, est.score_ranking):
    with pytest.raises(ValueError, match='before fit'):
      call(df, 'place')

  def no_gpu(*a, **k):
    raise AssertionError('GPU work was reached')
  monkeypatch.setattr(inference, '_ensemble_forecast', no_gpu)
  est.params_ = _params(lead)                      # "fitted": everything below must fail on its arguments alone
  good = np.full(lead, 1.0 / np.prod(lead))
  for call in (est.predict_ranking, est.score_ranking):
    with pytest.raises(ValueError, match='at most 16384'):
      call(df, 'place', num_samples=16385)
    for n in (0, -2):
      with pytest.raises(ValueError, match='at least one sample path'):
        call(df, 'place', num_samples=n)
    for k in (0, -1, 4):                            # three places
      with pytest.raises(ValueError, match=r'top_k=.*1\.\.3'):
        call(df, 'place', top_k=k)
    with pytest.raises(ValueError, match='top_k'):
      call(df, 'place', top_k='many')
    with pytest.raises(ValueError, match=r'\[0, 1\]'):
      call(df, 'place', quantiles=(0.5, 1.5))
    with pytest.raises(ValueError, match='not among the columns'):
      call(df, 'week')
    with pytest.raises(ValueError, match='per: .* not among the columns'):
      call(df, 'place', per='people')
    with pytest.raises(ValueError, match='constant within every group'):
      call(df, 't', per='pop')                      # three populations inside every week
    with pytest.raises(ValueError, match='constant within every group'):
      call(df, 'place', per=np.arange(1.0, 13.0))
    for bad in (np.where(np.arange(12) == 4, 0.0, 1.0), np.where(np.arange(12) == 4, -2.0, 1.0),
                np.where(np.arange(12) == 4, np.nan, 1.0), np.where(np.arange(12) == 4, np.inf, 1.0)):
      with pytest.raises(ValueError, match='finite and > 0'):
        call(df, 'place', per=bad)
    for bad in (np.ones(11), np.ones((12, 1)), 3.0):
      with pytest.raises(ValueError, match='one value per row'):
        call(df, 'place', per=bad)
    with pytest.raises(ValueError, match='per must be'):
      call(df, 'place', per=['x'] * 12)
    for bad, msg in ((good.reshape(-1), 'shape'), (good * 1.001, 'sum to 1'), (-good, '>= 0')):
      with pytest.raises(ValueError, match=msg):
        call(df, 'place', weights=bad)
    with pytest.raises(AssertionError, match='GPU work'):        # a good call passes the checks and reaches the GPU seam
      call(df, 'place', per='pop', weights=good, num_samples=5)
    with pytest.raises(AssertionError, match='GPU work'):
      call(df, ['place', 't'], top_k=12, per=df['pop'].to_numpy())
  with pytest.raises(ValueError, match='target column'):
    est.score_ranking(df.drop(columns='y'), 'place')
  d = df.copy()
  d.loc[3, 'y'] = 2.5
  with pytest.raises(ValueError, match='non-negative integer'):
    est.score_ranking(d, 'place')
  d.loc[3, 'y'] = np.nan                            # a NaN target is no error: it reaches the GPU seam
  with pytest.raises(AssertionError, match='GPU work'):
    est.score_ranking(d, 'place')
  # more groups than a path's values fit in LDS, on a table of singleton groups
  wide = pd.DataFrame({'t': pd.Timestamp('2020-01-06'), 'place': np.arange(16385), 'y': 0.0})
  with pytest.raises(ValueError, match='16385 groups.*at most 16384'):
    est.predict_ranking(wide, 'place', num_samples=10)
  with pytest.raises(ValueError, match='at most 16777216'):      # top_k * G
    est.predict_ranking(wide.iloc[:16384], 'place', top_k=1025, num_samples=10)
  with pytest.raises(AssertionError, match='GPU work'):
    est.predict_ranking(wide.iloc[:16384], 'place', top_k=1024, num_samples=16384)      # 2^28 cells: the cap itself
  # the seam's own checks
  groups = inference.csr_from_codes(np.arange(12) // 3, 4)
  seam = lambda *a, **k: inference.ranking_summaries(np.zeros((12, 1)), 'NB', est.params_, None, *a, **k)
  with pytest.raises(ValueError, match='at most 16384'):
    seam(16385, 0, len(lead), groups)
  with pytest.raises(ValueError, match='at least one sample path'):
    seam(0, 0, len(lead), groups)
  with pytest.raises(ValueError, match=r'\[0, 1\]'):
    seam(10, 0, len(lead), groups, quantiles=(-0.1,))
  for k in (0, 5):
    with pytest.raises(ValueError, match=r'top_k=.*1\.\.4'):
      seam(10, 0, len(lead), groups, top_k=k)
  with pytest.raises(ValueError, match='one total per group'):
    seam(10, 0, len(lead), groups, observed=np.zeros(3))
  with pytest.raises(ValueError, match='one divisor per group'):
    seam(10, 0, len(lead), groups, scale=np.ones(3))
  for bad in ([1.0, 0.0, 1.0, 1.0], [1.0, np.nan, 1.0, 1.0], [1.0, -1.0, 1.0, 1.0]):
    with pytest.raises(ValueError, match='finite and > 0'):
      seam(10, 0, len(lead), groups, scale=bad)
  big = inference.csr_from_codes(np.arange(16385), 16385)
  with pytest.raises(ValueError, match='at most 16384'):
    inference.ranking_summaries(np.zeros((16385, 1)), 'NB', est.params_, None, 10, 0, len(lead), big)
  with pytest.raises(AssertionError, match='GPU work'):
    seam(10, 0, len(lead), groups, observed=np.asarray([1.0, np.nan, 2.0, 2.0]), scale=np.ones(4), top_k=4)


def _fake_seam(prob_scored, seen):
  """A stand-in for inference.ranking_summaries: the observed ranks by the host helper, the given probabilities in the
  scored columns."""
  def fake(features, observation_model, params, model_args, num_samples, seed, ensemble_dims, groups, observed=None,
           scale=None, top_k=1, quantiles=(), compute_dtype=None):
    G = len(groups[0]) - 1
    seen.update(observed=observed, scale=scale, top_k=top_k, quantiles=quantiles, num_samples=num_samples)
    plain = np.full((top_k, G), 1.0 / G)
    out = dict(rank_mean=np.full(G, (G + 1) / 2.0), rank_quantiles=np.zeros((len(quantiles), G)), rank_probability=plain)
    if observed is not None:
      scored = ~np.isnan(observed)
      rank, above, ties = group_target_ranks(observed, scale)
      prob = np.full((top_k, G), np.nan)
      prob[:, scored] = prob_scored[:top_k, :int(scored.sum())]
      out.update(observed_rank=rank, observed_above=above, observed_ties=ties,
                 rank_crps=np.where(scored, 0.25, np.nan), rank_pit=np.where(scored, 0.5, np.nan)[None, :].repeat(2, 0),
                 scored_rank_mean=np.where(scored, 2.0, np.nan),
                 scored_rank_quantiles=np.where(scored, 2.0, np.nan)[None, :].repeat(len(quantiles), 0),
                 scored_rank_probability=prob)
    return out
  return fake


def test_what_the_estimators_add_on_the_host(monkeypatch):
  """Weeks with the totals 3, 6, 6 and one week with a NaN row: the observed ranks are 3, 1.5, 1.5 among the three scored
  weeks.  top_probability is the running sum over k; observed_top the share of the group in the observed top k; top_brier
  their squared difference averaged over the scored groups; observed_rank_probability the forecast mass on the observed
  block of ranks, NaN when the block lies beyond top_k."""
  df = _frame()
  df['y'] = [1.0, 1.0, 1.0, 2.0, 2.0, 2.0, 3.0, 3.0, 0.0, 5.0, np.nan, 5.0]
  prob = np.asarray([[0.2, 0.5, 0.3], [0.3, 0.3, 0.4], [0.5, 0.2, 0.3]])
  seen = {}
  monkeypatch.setattr(inference, 'ranking_summaries', _fake_seam(prob, seen))
  est = BayesianNeuralFieldMAP(feature_cols=['t'], target_col='y', freq='W', width=64, observation_model='NORMAL')
  est.params_ = object()
  res = est.score_ranking(df, 't', top_k=3, num_samples=7)
  keys = list(df['t'].unique())
  assert set(res) == {'keys', 'rank_mean', 'rank_quantiles', 'rank_probability', 'top_probability', 'most_likely_top',
                      'observed', 'observed_rank', 'rank_crps', 'rank_pit', 'observed_top', 'top_brier',
                      'observed_rank_probability', 'n', 'mean_rank_crps'}
  assert list(res['keys']) == keys and seen['top_k'] == 3 and seen['scale'] is None and seen['num_samples'] == 7
  assert np.array_equal(res['observed'], [3.0, 6.0, 6.0, np.nan], equal_nan=True)
  assert np.array_equal(seen['observed'], res['observed'], equal_nan=True)
  assert np.array_equal(res['observed_rank'], [3.0, 1.5, 1.5, np.nan], equal_nan=True)
  assert res['n'] == 3 and res['mean_rank_crps'] == 0.25 and res['most_likely_top'] == keys[1]
  assert np.array_equal(res['rank_probability'][:, :3], prob) and np.isnan(res['rank_probability'][:, 3]).all()
  top = np.cumsum(prob, axis=0)
  assert np.array_equal(res['top_probability'][:, :3], top) and np.isnan(res['top_probability'][:, 3]).all()
  want_top = np.asarray([[0.0, 0.5, 0.5], [0.0, 1.0, 1.0], [1.0, 1.0, 1.0]])
  assert np.array_equal(res['observed_top'][:, :3], want_top) and np.isnan(res['observed_top'][:, 3]).all()
  assert np.allclose(res['top_brier'], np.mean((top - want_top) ** 2, axis=1), rtol=1e-15, atol=0.0)
  assert np.allclose(res['observed_rank_probability'][:3], [0.5, 0.5 + 0.3, 0.3 + 0.4], rtol=1e-15)
  assert np.isnan(res['observed_rank_probability'][3])
  # top_k = 1: the block of week 0 (rank 3) lies beyond it; the tied block 1..2 keeps its first slot
  res = est.score_ranking(df, 't', top_k=1)
  assert np.array_equal(res['observed_rank_probability'], [np.nan, 0.5, 0.3, np.nan], equal_nan=True)
  assert res['observed_top'].shape == (1, 4) and np.allclose(res['top_brier'], [(0.04 + 0.0 + 0.04) / 3])
  # no group scored
  d = df.copy()
  d['y'] = np.nan
  res = est.score_ranking(d, 't', top_k=2)
  assert res['n'] == 0 and np.isnan(res['mean_rank_crps']) and np.isnan(res['top_brier']).all()
  assert res['most_likely_top'] is None and np.isnan(res['observed_rank_probability']).all()
  # per: a column, or one value per row; the divisor reaches the seam per group, and the observed ranks use it
  d = df.copy()
  d['y'] = np.tile([30.0, 40.0, 10.0], 4)             # totals 120, 160, 40 by place: per head 12, 8, 8
  for per in ('pop', d['pop'].to_numpy(), d['pop'].tolist()):
    res = est.score_ranking(d, 'place', top_k=3, per=per)
    assert np.array_equal(seen['scale'], [10.0, 20.0, 5.0])
    assert np.array_equal(res['observed'], [120.0, 160.0, 40.0]) and np.array_equal(res['observed_rank'], [1.0, 2.5, 2.5])
  assert np.array_equal(est.score_ranking(d, 'place', top_k=3)['observed_rank'], [2.0, 1.0, 3.0])
  # the forecast alone; several group columns give MultiIndex keys
  pred = est.predict_ranking(df, ['place', 't'], top_k=2, quantiles=(0.1, 0.9))
  assert set(pred) == {'keys', 'rank_mean', 'rank_quantiles', 'rank_probability', 'top_probability', 'most_likely_top'}
  assert isinstance(pred['keys'], pd.MultiIndex) and len(pred['keys']) == 12 and seen['observed'] is None
  assert pred['rank_probability'].shape == (2, 12) and pred['rank_quantiles'].shape == (2, 12)
  assert np.array_equal(pred['top_probability'][1], np.full(12, 1.0 / 12) + np.full(12, 1.0 / 12))
  assert pred['most_likely_top'] == pred['keys'][0] and seen['quantiles'] == (0.1, 0.9)


def test_the_score_sees_the_ranking():
  """x_sg = 10 g + N(0, 10^2), 12 groups, y one more draw.  Reversing the columns of x keeps the multiset of every path and
  turns the forecast ranking upside down: its mean rank CRPS is at least 4 times as large for the seeds 0..19 (measured:
  never below 8.8)."""
  lowest = np.inf
  for seed in range(20):
    x, y = R.graded_case(seed)
    good, bad = R.mean_rank_crps(x, y), R.mean_rank_crps(x[:, ::-1], y)
    lowest = min(lowest, bad / good)
    assert bad >= 4 * good, (seed, good, bad)
  print(f'mean rank CRPS, columns reversed / as forecast: lowest ratio over 20 seeds {lowest:.1f}')
