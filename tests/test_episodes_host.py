"""CPU-only checks of the spells above a threshold (include/bnf.h bnf_predictive_group_episodes): the naive reference on
hand-worked patterns; the piece / join operator of bayesnf_amd/csrc/bnf_episodes.h restated in numpy (associative under
any bracketing, NOT commutative, skipped positions are the identity); the ordered CSR builder; the observed spells; the
entry point's declaration and export; the estimators' argument checks, which fire before any GPU work."""
import os
import re

import numpy as np
import pandas as pd
import pytest

from bayesnf_amd import BayesianNeuralFieldMAP, BayesianNeuralFieldVI, _native, inference, spatiotemporal
from tests import episodes_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'bnf_predictive_group_episodes'


def _bools(pattern):
  return [c == '#' for c in pattern]


@pytest.mark.parametrize('pattern,want', [
    # pattern ('#' above, '.' not)   longest, its start, spells, onset step, first, last
    ('.##..##.#', (2, 1, 3, 1, 1, 8)),        # a tie of two longest runs: the earlier one (position 1, not 5) wins
    ('.....', (0, -1, 0, 5, -1, -1)),         # no exceedance: onset censored at the group's size
    ('####', (4, 0, 1, 0, 0, 3)),             # all exceed
    ('#..##.###', (3, 6, 3, 0, 0, 8)),        # the longest run ends on the last position
    ('....#', (1, 4, 1, 4, 4, 4)),            # the only exceeding position is the last
    ('', (0, -1, 0, 0, -1, -1)),              # an empty group
])
def test_hand_worked_patterns(pattern, want):
  above = _bools(pattern)
  assert E.naive_episodes(above, list(range(len(above)))) == want
  piece = dict(E.IDENTITY)
  for p, a in enumerate(above):
    piece = E.join(piece, E.piece_of(a, p))
  assert E.result_of(piece) == want
  # through group_episodes: one path whose draws are 1 where the pattern is above a threshold of 0.5; positions = rows
  if above:
    x = np.asarray([above], dtype=np.float32)
    res = E.group_episodes(x, [0, len(above)], np.arange(len(above)), np.full(len(above), 0.5, dtype=np.float32))
    got = tuple(int(res[k][0, 0]) for k in ('longest', 'longest_row', 'spells', 'onset_step', 'first_row', 'last_row'))
    assert got == want
    assert res['onset_count'].sum() == (1 if want[4] >= 0 else 0)


def _fold(pieces, rng):
  """Joins a list of pieces in position order under a random bracketing."""
  pieces = list(pieces)
  while len(pieces) > 1:
    k = int(rng.integers(0, len(pieces) - 1))
    pieces[k:k + 2] = [E.join(pieces[k], pieces[k + 1])]
  return pieces[0] if pieces else dict(E.IDENTITY)


def test_operator_matches_the_naive_loop_under_any_bracketing_and_is_not_commutative():
  rng = np.random.default_rng(0)
  order_bugs_seen = 0
  for trial in range(300):
    n = int(rng.integers(0, 40))
    above = rng.random(n) < rng.choice([0.2, 0.5, 0.8])
    skipped = rng.random(n) < 0.2                        # positions that take no part: the identity
    labels = rng.permutation(1000)[:n]                   # positions are labels, not 0 .. n - 1
    part = ~skipped
    want = E.naive_episodes(above[part].tolist(), labels[part].tolist())
    singles = [dict(E.IDENTITY) if skipped[i] else E.piece_of(bool(above[i]), int(labels[i])) for i in range(n)]
    # (a) random bracketing of the single positions
    assert E.result_of(_fold(singles, rng)) == want, (trial, 'bracketing')
    # (b) random cut points: pieces of contiguous stretches, each folded left to right, then joined in random brackets
    cuts = np.sort(rng.integers(0, n + 1, size=int(rng.integers(0, 6))))
    edges = [0, *cuts.tolist(), n]
    chunks = []
    for a, b in zip(edges[:-1], edges[1:]):
      p = dict(E.IDENTITY)
      for q in singles[a:b]:
        p = E.join(p, q)
      chunks.append(p)
    whole = _fold(chunks, rng)
    assert E.result_of(whole) == want, (trial, 'cut points')
    assert whole['len'] == int(part.sum())
    # (c) the identity on either side changes nothing
    assert E.join(E.IDENTITY, whole) == whole and E.join(whole, E.IDENTITY) == whole
    # (d) the halves in the WRONG order: a different answer whenever order matters -- the test can see an order bug
    if n >= 2:
      h = n // 2
      left, right = _fold(singles[:h], rng), _fold(singles[h:], rng)
      assert E.result_of(E.join(left, right)) == want
      if E.result_of(E.join(right, left)) != want:
        order_bugs_seen += 1
  assert order_bugs_seen > 100, order_bugs_seen


def test_ordered_csr_builder_sorts_by_key_and_keeps_table_order_on_ties():
  rng = np.random.default_rng(3)
  R, G = 200, 5
  codes = rng.integers(0, G, R)
  codes[codes == 3] = 2                                  # group 3 is empty
  key = rng.integers(0, 12, R)                           # many ties
  off, rows = inference.csr_ordered(codes, G, key)
  off0, rows0 = inference.csr_from_codes(codes, G)
  assert off.dtype == rows.dtype == np.int32 and np.array_equal(off, off0)
  assert sorted(rows.tolist()) == list(range(R))
  for g in range(G):
    r = rows[off[g]:off[g + 1]]
    assert np.all(codes[r] == g)
    want = sorted(np.flatnonzero(codes == g).tolist(), key=lambda i: (key[i], i))   # by key, ties in table order
    assert r.tolist() == want
  # float and datetime keys; csr_from_codes itself is untouched (rows ascend inside a group)
  t = np.datetime64('2020-01-01') + key.astype('timedelta64[D]')
  for k in (key.astype(np.float64), t):
    assert np.array_equal(inference.csr_ordered(codes, G, k)[1], rows)
  assert all(np.all(np.diff(rows0[off0[g]:off0[g + 1]]) > 0) for g in range(G))
  for bad, msg in ((key[:-1], 'one value per row'), (np.where(key == 3, np.nan, key.astype(float)), 'missing'),
                   (key.astype(str), 'numeric or datetime')):
    with pytest.raises(ValueError, match=msg):
      inference.csr_ordered(codes, G, bad)
  # a shuffled table through group_rows_ordered: time order inside every group, ties in table order
  df = pd.DataFrame({'t': pd.Timestamp('2021-03-01') + pd.to_timedelta(key, unit='D'), 'place': codes, 'n': np.arange(R)})
  df = df.sample(frac=1.0, random_state=1).reset_index(drop=True)
  keys, o, r = spatiotemporal.group_rows_ordered(df, 'place', 't')
  keys0, o0, r0 = spatiotemporal.group_rows(df, 'place')
  assert list(keys) == list(keys0) == [0, 1, 2, 4] and np.array_equal(o, o0)
  for g in range(len(keys)):
    seg = r[o[g]:o[g + 1]]
    tt = df['t'].to_numpy()[seg]
    assert np.all(np.diff(tt) >= np.timedelta64(0)) and set(seg.tolist()) == set(r0[o0[g]:o0[g + 1]].tolist())
    same = np.diff(tt) == np.timedelta64(0)
    assert np.all(np.diff(seg)[same] > 0)
  with pytest.raises(ValueError, match='order_by'):
    spatiotemporal.group_rows_ordered(df, 'place', 'week')


def test_group_target_episodes():
  nan = np.nan
  #         row  0    1    2    3    4    5    6    7    8    9   10   11
  target = [5.0, 0.0, 9.0, 9.0, 1.0, 9.0, nan, 2.0, 0.0, 0.0, 7.0, 3.0]
  thr = np.full(12, 2.0)
  thr[11] = 3.0                                          # strict >: 3 does not exceed 3
  # group 0: rows 3, 0, 2, 1, 5, 4 in that time order -> # # # . # .   group 1: empty   group 2: rows 6, 7 (a NaN target)
  # group 3: rows 8, 9 -> . .      group 4: rows 11, 10 -> . #
  off = [0, 6, 6, 8, 10, 12]
  rows = [3, 0, 2, 1, 5, 4, 6, 7, 8, 9, 11, 10]
  got = spatiotemporal.group_target_episodes(target, off, rows, thr)
  assert np.array_equal(got['longest'], [3.0, nan, nan, 0.0, 1.0], equal_nan=True)
  assert np.array_equal(got['spells'], [2.0, nan, nan, 0.0, 1.0], equal_nan=True)
  assert np.array_equal(got['onset_step'], [0.0, nan, nan, 2.0, 1.0], equal_nan=True)    # censored at the group's size
  assert got['longest_row'].tolist() == [3, -1, -1, -1, 10]
  assert got['first_row'].tolist() == [3, -1, -1, -1, 10] and got['last_row'].tolist() == [5, -1, -1, -1, 10]
  # the same through the naive reference on the target as a single "path"
  t = np.asarray(target, dtype=np.float32)[None, :]
  ref = E.group_episodes(np.nan_to_num(t, nan=0.0), off, rows, thr.astype(np.float32))
  for g in (0, 3, 4):
    for k in ('longest', 'spells', 'onset_step', 'longest_row', 'first_row', 'last_row'):
      assert got[k][g] == ref[k][0, g], (g, k)


def test_entry_point_declared_listed_and_exported():
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'bnf.h')).read(), flags=re.S)
  lib = _native.load()
  assert re.search(r'\bint\s+' + NAME + r'\s*\(', src), f'{NAME} is not declared in include/bnf.h'
  assert NAME in _native.EXPORTS
  fn = getattr(lib, NAME)
  assert fn.argtypes is not None and len(fn.argtypes) == 23
  assert _native.ABI_VERSION == 6 and lib.bnf_abi_version() == 6          # purely additive
  assert int(re.search(r'#define\s+BNF_EPISODES_WORK_PER_TILE\s+(\d+)', src).group(1)) == _native.EPISODES_WORK_PER_TILE
  assert _native.EPISODES_WORK_PER_TILE == 2 * 4 * len(E.FIELDS)          # two pieces of ten int32 fields
  from bayesnf_amd.engine import Engine
  assert callable(getattr(Engine, 'predictive_group_episodes', None))
  assert callable(getattr(inference, 'episode_summaries', None))
  # an unbound handle is refused with the code bnf_predictive_group_sums gives
  args = (None, None, None, 2, 4, None, None, 1, 1, 0, 0, 0)
  assert lib.bnf_predictive_group_episodes(*args, None, None, None, 0, None, None, None, None, None, None, None) == \
      lib.bnf_predictive_group_sums(*args, None, 0, None) != 0


def _frame():
  t = pd.date_range('2020-01-06', periods=4, freq='W-MON')
  return pd.DataFrame({'t': np.repeat(t, 3), 'place': np.tile(['a', 'b', 'c'], 4), 'y': np.arange(12.0)})


def _params(lead):
  return (np.zeros(lead + (3,)), np.zeros(lead))


@pytest.mark.parametrize('cls,lead', [(BayesianNeuralFieldMAP, (1, 4)), (BayesianNeuralFieldVI, (1, 5, 2))])
def test_episodes_refuse_bad_calls_before_any_gpu_work(cls, lead, monkeypatch):
  df = _frame()
  est = cls(feature_cols=['t'], target_col='y', freq='W', width=64, observation_model='NB')
  for call in (est.predict_episodes, est.score_episodes):
    with pytest.raises(ValueError, match='before fit'):
      call(df, 'place', 3.0)

  def no_gpu(*a, **k):
    raise AssertionError('GPU work was reached')
  monkeypatch.setattr(inference, '_ensemble_forecast', no_gpu)
  est.params_ = _params(lead)                      # "fitted": everything below must fail on its arguments alone
  good = np.full(lead, 1.0 / np.prod(lead))
  for call in (est.predict_episodes, est.score_episodes):
    with pytest.raises(ValueError, match='at most 16384'):
      call(df, 'place', 3.0, num_samples=16385)
    for n in (0, -2):
      with pytest.raises(ValueError, match='at least one sample path'):
        call(df, 'place', 3.0, num_samples=n)
    with pytest.raises(ValueError, match='threshold is required'):
      call(df, 'place', None)
    for bad in (np.nan, np.inf, np.where(np.arange(12) == 5, -np.inf, 3.0)):
      with pytest.raises(ValueError, match='finite'):
        call(df, 'place', bad)
    for bad in (np.zeros(11), np.zeros((12, 1)), np.zeros(4)):
      with pytest.raises(ValueError, match='one limit per row'):
        call(df, 'place', bad)
    with pytest.raises(ValueError, match='threshold'):
      call(df, 'place', 'high')
    for bad, msg in ((good.reshape(-1), 'shape'), (good * 1.001, 'sum to 1'), (-good, '>= 0')):
      with pytest.raises(ValueError, match=msg):
        call(df, 'place', 3.0, weights=bad)
    with pytest.raises(ValueError, match='not among the columns'):
      call(df, 'week', 3.0)
    with pytest.raises(ValueError, match='order_by'):
      call(df, 'place', 3.0, order_by='week')
    with pytest.raises(ValueError, match=r'\[0, 1\]'):
      call(df, 'place', 3.0, quantiles=(0.5, 1.5))
    with pytest.raises(AssertionError, match='GPU work'):        # a good call passes the checks and reaches the GPU seam
      call(df, 'place', 3.0, weights=good, num_samples=5)
    with pytest.raises(AssertionError, match='GPU work'):
      call(df, ['place'], np.arange(12.0), order_by='y')
  with pytest.raises(ValueError, match='target column'):
    est.score_episodes(df.drop(columns='y'), 'place', 3.0)
  d = df.copy()
  d.loc[3, 'y'] = 2.5
  with pytest.raises(ValueError, match='non-negative integer'):
    est.score_episodes(d, 'place', 3.0)
  d.loc[3, 'y'] = np.nan                            # a NaN target is no error: it reaches the GPU seam
  with pytest.raises(AssertionError, match='GPU work'):
    est.score_episodes(d, 'place', 3.0)
  # the cell cap, on a table of 2^15 singleton groups
  wide = pd.DataFrame({'t': pd.Timestamp('2020-01-06'), 'place': np.arange(1 << 15), 'y': 0.0})
  with pytest.raises(ValueError, match='held whole'):
    est.predict_episodes(wide, 'place', 3.0, num_samples=16384)
  # the seam's own checks
  groups = inference.csr_from_codes(np.arange(12) // 3, 4)
  seam = lambda *a, **k: inference.episode_summaries(np.zeros((12, 1)), 'NB', est.params_, None, *a, **k)
  thr = np.full(12, 3.0)
  with pytest.raises(ValueError, match='at most 16384'):
    seam(16385, 0, len(lead), groups, thr)
  with pytest.raises(ValueError, match='at least one sample path'):
    seam(0, 0, len(lead), groups, thr)
  big = inference.csr_from_codes(np.arange(1 << 15), 1 << 15)
  with pytest.raises(ValueError, match='held whole'):
    inference.episode_summaries(np.zeros((1 << 15, 1)), 'NB', est.params_, None, 16384, 0, len(lead), big, np.zeros(1 << 15))
  with pytest.raises(ValueError, match=r'\[0, 1\]'):
    seam(10, 0, len(lead), groups, thr, quantiles=(0.5, 1.5))
  with pytest.raises(ValueError, match='threshold is required'):
    seam(10, 0, len(lead), groups, None)
  with pytest.raises(ValueError, match='finite'):
    seam(10, 0, len(lead), groups, np.full(12, np.nan))
  with pytest.raises(ValueError, match='one limit per row'):
    seam(10, 0, len(lead), groups, np.zeros(3))
  with pytest.raises(ValueError, match='one value per group'):
    seam(10, 0, len(lead), groups, thr, observed_spells=np.zeros(3))
  with pytest.raises(AssertionError, match='GPU work'):
    seam(10, 0, len(lead), groups, thr, observed_longest=np.zeros(4))


def test_score_episodes_assembles_observed_values_and_onset_row_probability(monkeypatch):
  df = _frame()                                     # 4 weeks x 3 places, rows in week order
  df['y'] = [3.0, 0.0, 9.0, 7.0, 0.0, np.nan, 7.0, 0.0, 1.0, 0.0, 0.0, 8.0]
  df = df.iloc[::-1].reset_index(drop=True)         # the table in REVERSE time order: the ordering must undo it
  seen = {}

  def fake(features, observation_model, params, model_args, num_samples, seed, ensemble_dims, groups, threshold,
           observed_longest=None, observed_spells=None, observed_onset_step=None, quantiles=(), compute_dtype=None):
    seen.update(groups=groups, threshold=threshold, longest=observed_longest, spells=observed_spells, onset=observed_onset_step)
    G, R = len(groups[0]) - 1, len(features)
    out = dict(onset_probability=np.arange(R) / 100.0, no_episode=np.full(G, 0.5))
    for name, obs in (('longest', observed_longest), ('spells', observed_spells), ('onset_step', observed_onset_step)):
      out[f'{name}_mean'], out[f'{name}_quantiles'] = np.zeros(G), np.zeros((len(quantiles), G))
      if obs is not None:
        out[f'{name}_pit'], out[f'{name}_crps'] = np.zeros((2, G)), np.where(np.isnan(obs), np.nan, 2.0)
    return out
  monkeypatch.setattr(inference, 'episode_summaries', fake)
  est = BayesianNeuralFieldMAP(feature_cols=['t'], target_col='y', freq='W', width=64, observation_model='NORMAL')
  est.params_ = object()
  res = est.score_episodes(df, 'place', 2.0, num_samples=7, seed=1)
  off, rows = seen['groups']
  t = df['t'].to_numpy()
  for g in range(3):
    assert np.all(np.diff(t[rows[off[g]:off[g + 1]]]) > np.timedelta64(0))      # time order inside every group
  # place a: 3 7 7 0 -> ###. ; place b: 0 0 0 0 ; place c: 9 nan 1 8 -> not scored
  assert np.array_equal(res['observed_longest'], [3.0, 0.0, np.nan], equal_nan=True)
  assert np.array_equal(res['observed_spells'], [1.0, 0.0, np.nan], equal_nan=True)
  assert np.array_equal(res['observed_onset_step'], [0.0, 4.0, np.nan], equal_nan=True)
  first_a = int(np.flatnonzero((df['place'] == 'a') & (df['t'] == df['t'].min()))[0])
  assert res['observed_onset_row'].tolist() == [first_a, -1, -1]
  assert np.array_equal(res['onset_row_probability'], [first_a / 100.0, 0.5, np.nan], equal_nan=True)
  assert res['n'] == 2 and res['mean_longest_crps'] == 2.0 and res['mean_onset_row_probability'] == (first_a / 100.0 + 0.5) / 2
  assert np.array_equal(seen['threshold'], np.full(12, 2.0)) and np.array_equal(seen['longest'], res['observed_longest'], equal_nan=True)
  assert set(res) == {'keys', 'onset_probability', 'no_episode', 'observed_onset_row', 'onset_row_probability', 'n',
                      'mean_onset_row_probability'} | {
                          f(n) for n in ('longest', 'spells', 'onset_step') for f in (
                              lambda n: n + '_mean', lambda n: n + '_quantiles', lambda n: 'observed_' + n,
                              lambda n: n + '_crps', lambda n: n + '_pit', lambda n: 'mean_' + n + '_crps')}
  yy = np.nan_to_num(df['y'].to_numpy(), nan=99.0)
  pred = est.predict_episodes(df.assign(y=yy), 'place', 2.0, order_by='y')      # another ordering column
  assert seen['longest'] is None and pred['longest_quantiles'].shape == (1, 3)
  assert set(pred) == {'keys', 'onset_probability', 'no_episode'} | {
      n + s for n in ('longest', 'spells', 'onset_step') for s in ('_mean', '_quantiles')}
  off, rows = seen['groups']
  for g in range(3):
    assert np.all(np.diff(yy[rows[off[g]:off[g + 1]]]) >= 0)
  with pytest.raises(ValueError, match='missing values'):
    est.predict_episodes(df, 'place', 2.0, order_by='y')
