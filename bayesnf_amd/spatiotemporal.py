"""Estimator API of the MI355X-native BayesNF path.

Drop-in for the public surface of /root/reference/src/bayesnf/spatiotemporal.py:
`BayesianNeuralFieldMAP`, `BayesianNeuralFieldMLE`, `BayesianNeuralFieldVI`
(ctor kwargs :217-232, `MAP.fit` :480-489, `VI.fit` :565-576, `predict`
:372-408, attributes `params_`, `losses_`, `data_handler`) and of the pandas
glue (`SpatiotemporalDataHandler` :114-192, `seasonality_to_float` :31-59,
`seasonalities_to_array` :62-95).  The three engine calls underneath
(`inference.fit_map / fit_vi / predict_bnf`, reference seam :400,:529,:634) go
to the HIP library instead of jax.

Differences a caller can see:
  * `seed` is an int or a length-2 uint32 array (a `jax.random.PRNGKey` also
    works, it is such an array).  With `init_rng='jax'` (the default) every
    estimator draws from the reference's own streams for that seed (threefry + the
    TFP seed chain, `jaxseed`): the initial particles of MAP / MLE and their
    per-member per-epoch minibatch shuffles (`jax.random.permutation`); the initial
    surrogate means, the optimisation noise and the posterior draws of a full-batch
    VI fit -- full-batch fits reproduce the reference's golden predictions.  Only a
    VI fit WITH `batch_size` keeps this package's counter-based generator for its
    noise and row batches (which split of the step seed the reference uses there is
    pinned by no golden).  `init_rng='philox'` selects the device generator everywhere.
  * limits of the HIP engine, checked when the estimator is constructed / fitted
    (the reference accepts any size): `depth` <= 8 (any `width` up to 8192 -- widths that are
    not a multiple of 64 run zero-padded inside the engine, same model and parameters);
    at most 8 feature columns, 96 distinct seasonal frequencies, 16 interactions;
    at most 512 (fp32: 256) features in total; `batch_size` <= number of rows.
  * the leading `(num_devices, ensemble_size // num_devices)` dimensions use
    `num_devices = distributed.device_count()`: the devices this ONE process drives
    (every visible GPU, or `BNF_DEVICES`; the reference's `jax.local_devices()` shape),
    or the torch.distributed world size under a one-process-per-GPU launcher.
  * `likelihood_model()` returns `bayesnf_amd.inference.EnsembleLikelihood`,
    not a TFP distribution.
"""

from __future__ import annotations

import numbers
import types
from collections.abc import Sequence

import numpy as np
import pandas as pd

from . import distributed
from . import inference


# ---------------------------------------------------------------------------
# pandas helpers
# ---------------------------------------------------------------------------
def seasonality_to_float(seasonality: str, freq: str) -> float:
  """How many `freq` steps make one `seasonality` period, on average.

  Averaged over the four years 2020-2023 so that a leap day is included, e.g.
  ('Y','D') -> 365.25, ('M','D') -> 30.4375, ('M','h') -> 730.5.
  """
  anchors = pd.date_range('2020-01-01', periods=5, freq='YS')
  coarse = anchors.to_period(seasonality)
  n_coarse = (coarse[-1] - coarse[0]).n
  fine = pd.date_range(coarse[0].start_time,
                       coarse[-1].start_time).to_period(freq)
  n_fine = (fine[-1] - fine[0]).n
  return n_fine / n_coarse


def seasonalities_to_array(seasonalities: Sequence[float | str],
                           freq: str) -> np.ndarray:
  """Periods (numbers, or pandas offset aliases) as floats in units of `freq`.

  Raises TypeError for a period shorter than one `freq` step.
  """
  out = []
  for s in seasonalities:
    if isinstance(s, str):
      value = seasonality_to_float(s, freq)
      if value < 1:
        raise TypeError(
            f'seasonality={s!r} should represent a time span greater than '
            f'freq={freq!r}, but {s} is {value:.2f} of a {freq}')
    else:
      value = s
      if value < 1:
        raise TypeError(f'seasonality_float={value!r} should be larger than 1.')
    out.append(value)
  return np.array(out)


_EPOCH = '2020-01-01'


def _convert_datetime_col(table, time_column, timetype, freq, time_min=None):
  """Replace `time_column` by a number, shifted so the training minimum is 0.

  'index': number of `freq` periods since 2020-01-01; 'float': the value as is.
  Mutates `table` (callers pass a copy) and returns (table, time_min).
  """
  col = table[time_column]
  if timetype == 'index':
    origin = pd.to_datetime(_EPOCH).to_period(freq)
    col = (col.dt.to_period(freq) - origin).apply(lambda delta: delta.n)
  elif timetype == 'float':
    col = col.apply(float)
  else:
    raise ValueError(f'Unknown timetype: {timetype}')
  if time_min is None:
    time_min = col.min()
  table[time_column] = col - time_min
  return table, time_min


class SpatiotemporalDataHandler:
  """DataFrame -> (N, D) float features / (N,) target.

  Column 0 of `feature_cols` is time.  `get_train` learns the time origin, the
  time scale (max training index, used as `input_scales[0]`) and the
  mean / std of the columns listed in `standardize`; `get_test` re-applies them.
  """

  def __init__(self, feature_cols, target_col, timetype, freq,
               standardize=None):
    self.feature_cols = feature_cols
    self.target_col = target_col
    self.timetype = timetype
    self.freq = freq
    self.standardize = standardize
    self.mu_ = None
    self.std_ = None
    self.time_min_ = None
    self.time_scale_ = None

  @property
  def _time_idx(self) -> int:
    return 0

  @property
  def _time_column(self) -> str:
    return self.feature_cols[self._time_idx]

  def _maybe_filter_target_nans(self, table):
    if self.target_col in table.columns:
      return table[table[self.target_col].notna()]
    return table

  def copy_and_filter_table(self, table):
    return self._maybe_filter_target_nans(table.copy())

  def get_target(self, table) -> np.ndarray:
    return self._maybe_filter_target_nans(table)[self.target_col].values

  def get_train(self, table) -> np.ndarray:
    work = self.copy_and_filter_table(table)
    ncol = len(self.feature_cols)
    self.mu_, self.std_ = np.zeros(ncol), np.ones(ncol)
    work, self.time_min_ = _convert_datetime_col(
        work, self._time_column, self.timetype, self.freq, None)
    feats = work[self.feature_cols].values
    self.time_scale_ = feats[:, self._time_idx].max()
    if self.standardize:
      if self._time_column in self.standardize:
        raise TypeError('Do not standardize the time column!')
      cols = [self.feature_cols.index(c) for c in self.standardize]
      block = feats[:, cols].astype(float)
      self.mu_[cols] = block.mean(axis=0)
      self.std_[cols] = block.std(axis=0)
      feats = (feats - self.mu_) / self.std_
    return feats

  def get_test(self, table) -> np.ndarray:
    work, _ = _convert_datetime_col(
        table.copy(), self._time_column, self.timetype, self.freq,
        self.time_min_)
    feats = work[self.feature_cols].values
    if self.standardize:
      feats = (feats - self.mu_) / self.std_
    return feats

  def get_input_scales(self) -> np.ndarray:
    scales = np.ones(len(self.feature_cols))
    scales[self._time_idx] = self.time_scale_
    return scales


def group_rows(table, group_by):
  """Rows of `table` grouped by one column or a list of columns -> (keys, seg_offsets, seg_rows): `keys` the sorted
  pandas Index (a MultiIndex for several columns) of the groups that occur, and the rows sorted by group as CSR
  (`inference.csr_from_codes`): group keys[g] owns seg_rows[seg_offsets[g]:seg_offsets[g + 1]]."""
  keys, codes = _group_codes(table, group_by)
  seg_offsets, seg_rows = inference.csr_from_codes(codes, len(keys))
  return keys, seg_offsets, seg_rows


def _group_codes(table, group_by):
  """-> (keys, codes): the sorted Index of the groups that occur and every row's group as a position in it."""
  cols = [group_by] if isinstance(group_by, str) or not isinstance(group_by, (list, tuple)) else list(group_by)
  missing = [c for c in cols if c not in table.columns]
  if not cols or missing:
    raise ValueError(f'group_by: {missing or "no column"} not among the columns of the table')
  if len(table) == 0:
    raise ValueError('group_by on an empty table')
  index = pd.Index(table[cols[0]]) if len(cols) == 1 else pd.MultiIndex.from_frame(table[cols])
  codes, keys = index.factorize(sort=True)
  keys = keys.set_names(cols)
  if (codes < 0).any():
    raise ValueError('group_by columns hold missing values')
  return keys, codes.astype(np.int64)


def group_rows_ordered(table, group_by, order_by):
  """`group_rows` with the rows of every group in the order of the column `order_by`: ascending, rows with equal
  values in table order (`inference.csr_ordered`).  The layout in which position order inside a group is time."""
  keys, codes = _group_codes(table, group_by)
  if not isinstance(order_by, str) or order_by not in table.columns:
    raise ValueError(f'order_by: {order_by!r} is not among the columns of the table')
  rank, _ = pd.factorize(table[order_by], sort=True)          # any sortable column -> its rank
  if (rank < 0).any():
    raise ValueError(f'order_by: the column {order_by!r} holds missing values')
  seg_offsets, seg_rows = inference.csr_ordered(codes, len(keys), rank.astype(np.int64))
  return keys, seg_offsets, seg_rows


def group_combinations(table, group_by, weight=None, mean=False):
  """One linear combination of the rows per group of `group_by` (the grouping of `group_rows`) -> (keys, (form, row,
  coef)): `keys` the sorted Index of the groups, and a COO triple `inference.combinations_csr` and
  `predict_combinations` take.  The coefficient of a row is 1, or its `weight`: a column name or one finite value per row
  (an area, a population).  mean=True divides by the group's sum of coefficients: the (weighted) mean of the group
  instead of its (weighted) total; a group whose weights sum to 0 is a ValueError."""
  keys, seg_offsets, seg_rows = group_rows(table, group_by)
  row = seg_rows.astype(np.int64)
  form = np.repeat(np.arange(len(keys), dtype=np.int64), np.diff(seg_offsets.astype(np.int64)))
  if weight is None:
    coef = np.ones(len(row), dtype=np.float64)
  else:
    if isinstance(weight, str):
      if weight not in table.columns:
        raise ValueError(f'weight: {weight!r} is not among the columns of the table')
      weight = table[weight].values
    try:
      w = np.asarray(weight, dtype=np.float64)
    except (TypeError, ValueError) as e:
      raise ValueError('weight must be a column name or one number per row of the table') from e
    if w.shape != (len(table),):
      raise ValueError(f'weight must hold one value per row ({len(table)},); got {w.shape}')
    if not np.all(np.isfinite(w)):
      raise ValueError('weight must be finite')
    coef = w[row]
  if mean:
    total = np.add.reduceat(coef, seg_offsets[:-1].astype(np.int64))      # group_rows makes no empty group
    if np.any(total == 0):
      raise ValueError(f'mean=True: the weights of group {keys[int(np.flatnonzero(total == 0)[0])]!r} sum to 0')
    coef = coef / total[form]
  return keys, (form, row, coef)


def stack_combinations(*parts):
  """Several (keys, (form, row, coef)) results of `group_combinations` joined into one: the keys concatenated in the
  order given, the form indices shifted to match.  How a hierarchy is written -- places, regions and the whole table as
  combinations of the same sample paths: stack_combinations(group_combinations(t, 'place'), group_combinations(t,
  'region'), ...)."""
  if not parts:
    raise ValueError('stack_combinations: nothing to stack')
  labels, forms, rows, coefs, base = [], [], [], [], 0
  for part in parts:
    try:
      keys, (form, row, coef) = part
    except (TypeError, ValueError) as e:
      raise ValueError('stack_combinations: every part is (keys, (form, row, coef))') from e
    labels.extend(list(keys))
    forms.append(np.asarray(form, dtype=np.int64) + base)
    rows.append(np.asarray(row, dtype=np.int64))
    coefs.append(np.asarray(coef, dtype=np.float64))
    base += len(keys)
  keys = pd.Index(labels, tupleize_cols=False)
  return keys, (np.concatenate(forms), np.concatenate(rows), np.concatenate(coefs))


def combination_target_sums(target, form_offsets, form_rows, form_coef):
  """Observed combinations: the float64 sum of coef * target over the positions of every form of the CSR layout
  `inference.combinations_csr` returns -> (K,); NaN for a form with a NaN target among its positions, 0 for an empty
  form.  Rows whose coefficient is 0 hold no position and do not count."""
  target = np.asarray(target, dtype=np.float64)
  form_offsets = np.asarray(form_offsets, dtype=np.int64)
  term = np.asarray(form_coef, dtype=np.float64) * target[np.asarray(form_rows, dtype=np.int64)]
  out = np.zeros(len(form_offsets) - 1)
  full = np.diff(form_offsets) > 0
  if term.size:
    out[full] = np.add.reduceat(term, form_offsets[:-1][full])
  return out


def group_target_sums(target, seg_offsets, seg_rows):
  """Observed totals: the float64 sum of `target` (R,) over the rows of every group of the CSR layout `group_rows`
  returns -> (G,); NaN for a group with a NaN target among its rows (and for an empty one, which `group_rows` never makes)."""
  target = np.asarray(target, dtype=np.float64)
  sorted_target = target[np.asarray(seg_rows, dtype=np.int64)]
  starts = np.asarray(seg_offsets[:-1], dtype=np.int64)
  sizes = np.diff(np.asarray(seg_offsets, dtype=np.int64))
  out = np.full(len(starts), np.nan)
  if sorted_target.size:
    full = sizes > 0
    out[full] = np.add.reduceat(sorted_target, starts[full])
  return out


def group_target_ranks(observed, scale=None):
  """Observed ranks: the groups ranked by their observed totals `observed` (G,), divided by `scale` (G,) when given,
  with the tie rule of the forecast (include/bnf.h bnf_sample_ranks) -> (rank (G,) float64, above (G,) int64, ties (G,)
  int64): above the groups with a larger value, ties those with an equal one (the group itself included), rank the
  mid-rank above + (ties + 1) / 2, so rank 1 is the largest and tied groups share their block of ranks.  A group with a
  NaN total gives NaN / -1 / -1 and takes no part in the ranks of the others."""
  v = np.asarray(observed, dtype=np.float64)
  if v.ndim != 1:
    raise ValueError(f'observed must be (G,); got {v.shape}')
  if scale is not None:
    scale = np.asarray(scale, dtype=np.float64)
    if scale.shape != v.shape:
      raise ValueError(f'scale must hold one divisor per group {v.shape}; got {scale.shape}')
    v = v / scale
  seen = ~np.isnan(v)
  rank, above, ties = np.full(v.shape, np.nan), np.full(v.shape, -1), np.full(v.shape, -1)
  w = v[seen]
  ordered = np.sort(w)
  hi = np.searchsorted(ordered, w, side='right')
  ties[seen] = hi - np.searchsorted(ordered, w, side='left')
  above[seen] = w.size - hi
  rank[seen] = above[seen] + 0.5 * (ties[seen] + 1)
  return rank, above, ties


def group_target_extremes(target, seg_offsets, seg_rows, threshold=None):
  """Observed peaks: per group of the CSR layout `group_rows` returns, the largest `target` (R,) over the group's rows,
  the lowest table row at which it is reached and, with `threshold` (R,), the number of rows whose target is > their
  threshold -> (max (G,) float64, peak_row (G,) int64, count (G,) float64 or None).  A group with a NaN target among its
  rows (and an empty one, which `group_rows` never makes) gives NaN, -1, NaN."""
  target = np.asarray(target, dtype=np.float64)
  order = np.asarray(seg_rows, dtype=np.int64)
  sorted_target = target[order]
  starts = np.asarray(seg_offsets[:-1], dtype=np.int64)
  sizes = np.diff(np.asarray(seg_offsets, dtype=np.int64))
  n_groups = len(starts)
  peak = np.full(n_groups, np.nan)
  peak_row = np.full(n_groups, -1, dtype=np.int64)
  count = None if threshold is None else np.full(n_groups, np.nan)
  full = sizes > 0
  if sorted_target.size and full.any():
    peak[full] = np.maximum.reduceat(sorted_target, starts[full])              # NaN if any row is NaN
    group_of = np.repeat(np.arange(n_groups), sizes)
    pos = np.arange(sorted_target.size, dtype=np.int64)
    first = np.minimum.reduceat(np.where(sorted_target == peak[group_of], pos, sorted_target.size), starts[full])
    seen = ~np.isnan(peak[full])
    peak_row[np.flatnonzero(full)[seen]] = order[first[seen]]
    if threshold is not None:
      above = (sorted_target > np.asarray(threshold, dtype=np.float64)[order]).astype(np.float64)
      count[full] = np.where(seen, np.add.reduceat(above, starts[full]), np.nan)
  return peak, peak_row, count


def group_target_episodes(target, seg_offsets, seg_rows, threshold):
  """Observed spells: per group of a CSR layout whose positions are in time order (`group_rows_ordered`), with
  above = target > threshold (both (R,)) read along the group's positions -> dict of (G,) arrays:
    'longest' float64      length of the longest run of consecutive rows above, 0 if none
    'longest_row' int64    the table row at which it starts (the earliest of equally long runs), -1 if none
    'spells' float64       the number of maximal runs
    'onset_step' float64   the rows before the first one above; the group's size if none (censored, as the forecast is)
    'first_row', 'last_row' int64   the first / last table row above, -1 if none
  A group with a NaN target among its rows (and an empty one, which `group_rows` never makes) gives NaN in the float
  columns and -1 in the row columns: it is not scored."""
  target = np.asarray(target, dtype=np.float64)
  order = np.asarray(seg_rows, dtype=np.int64)
  offsets = np.asarray(seg_offsets, dtype=np.int64)
  above = target[order] > np.asarray(threshold, dtype=np.float64)[order]
  missing = np.isnan(target[order])
  n_groups = len(offsets) - 1
  out = {k: np.full(n_groups, np.nan) for k in ('longest', 'spells', 'onset_step')}
  out.update({k: np.full(n_groups, -1, dtype=np.int64) for k in ('longest_row', 'first_row', 'last_row')})
  for g in range(n_groups):
    a, b = offsets[g], offsets[g + 1]
    if a == b or missing[a:b].any():
      continue
    hit = np.flatnonzero(above[a:b])
    out['longest'][g], out['spells'][g], out['onset_step'][g] = 0.0, 0.0, float(b - a)
    if hit.size:
      cut = np.flatnonzero(np.diff(hit) > 1)
      starts, ends = hit[np.r_[0, cut + 1]], hit[np.r_[cut, hit.size - 1]]
      lengths = ends - starts + 1
      best = int(np.argmax(lengths))                           # the first of equally long runs
      out['longest'][g], out['spells'][g], out['onset_step'][g] = float(lengths[best]), float(len(starts)), float(hit[0])
      out['longest_row'][g], out['first_row'][g], out['last_row'][g] = order[a + starts[best]], order[a + hit[0]], order[a + hit[-1]]
  return out


def group_target_cumulative(target, seg_offsets, seg_rows, level=None):
  """Observed running totals: per group of a CSR layout whose positions are in time order (`group_rows_ordered`), the
  float64 cumulative sum of `target` (R,) along the group's positions -> dict:
    'running' (R,) float64     per TABLE ROW: the running total at the row; NaN from the group's first NaN target on
    'total' (G,) float64       the running total at the group's last row
  and with `level` (G,), one per group, compared with strict >:
    'cross_step' (G,) float64  the rows before the first one whose running total is above the level; the group's size if
                               none (censored, as the forecast is)
    'cross_row' (G,) int64     that table row, -1 if none
  A group with a NaN target among its rows (and an empty one, which `group_rows` never makes) gives NaN in 'total' and
  'cross_step' and -1 in 'cross_row': it is not scored."""
  target = np.asarray(target, dtype=np.float64)
  order = np.asarray(seg_rows, dtype=np.int64)
  offsets = np.asarray(seg_offsets, dtype=np.int64)
  n_groups = len(offsets) - 1
  out = {'running': np.full(target.shape, np.nan), 'total': np.full(n_groups, np.nan)}
  if level is not None:
    level = np.asarray(level, dtype=np.float64)
    out['cross_step'] = np.full(n_groups, np.nan)
    out['cross_row'] = np.full(n_groups, -1, dtype=np.int64)
  for g in range(n_groups):
    a, b = offsets[g], offsets[g + 1]
    if a == b:
      continue
    run = np.cumsum(target[order[a:b]])
    out['running'][order[a:b]] = run
    if np.isnan(run[-1]):
      continue
    out['total'][g] = run[-1]
    if level is not None:
      hit = np.flatnonzero(run > level[g])
      out['cross_step'][g] = float(hit[0]) if hit.size else float(b - a)
      if hit.size:
        out['cross_row'][g] = order[a + hit[0]]
  return out


def group_target_windows(target, seg_offsets, seg_rows, window, threshold=None):
  """Observed moving-window totals: per group of a CSR layout whose positions are in time order (`group_rows_ordered`),
  the float64 sum of `target` (R,) over the last `window` rows at every row at which a FULL-LENGTH window ends (a group
  shorter than `window` has one: the whole group, at its last row) -> dict:
    'window' (R,) float64      per TABLE ROW: the window total ending at the row; NaN where no full-length window ends
                               and where the window holds a NaN target
    'peak' (G,) float64        the largest window total of the group
    'peak_row' (G,) int64      the table row at which it is first reached
  and with `threshold` (G,), one per group, compared with strict >:
    'count' (G,) float64       the windows of the group above it
  A group with a NaN target among its rows (and an empty one, which `group_rows` never makes) gives NaN in 'peak' and
  'count' and -1 in 'peak_row': it is not scored; its windows without a NaN target keep their totals."""
  target = np.asarray(target, dtype=np.float64)
  order = np.asarray(seg_rows, dtype=np.int64)
  offsets = np.asarray(seg_offsets, dtype=np.int64)
  window = inference._window_length(window)
  n_groups = len(offsets) - 1
  out = {'window': np.full(target.shape, np.nan), 'peak': np.full(n_groups, np.nan),
         'peak_row': np.full(n_groups, -1, dtype=np.int64)}
  if threshold is not None:
    threshold = np.asarray(threshold, dtype=np.float64)
    out['count'] = np.full(n_groups, np.nan)
  for g in range(n_groups):
    a, b = offsets[g], offsets[g + 1]
    if a == b:
      continue
    w = min(window, int(b - a))
    win = np.lib.stride_tricks.sliding_window_view(target[order[a:b]], w).sum(axis=1)   # ends at a + w - 1 .. b - 1
    out['window'][order[a + w - 1:b]] = win
    if np.isnan(win).any():                                      # every row lies in some full-length window
      continue
    best = int(np.argmax(win))                                   # the first of equal totals
    out['peak'][g], out['peak_row'][g] = win[best], order[a + w - 1 + best]
    if threshold is not None:
      out['count'][g] = float((win > threshold[g]).sum())
  return out


# ---------------------------------------------------------------------------
# estimators
# ---------------------------------------------------------------------------
class BayesianNeuralFieldEstimator:
  """Common constructor / predict for the MAP, MLE and VI estimators.

  Keyword arguments (all keyword-only, as in the reference):
    feature_cols, target_col: column names; feature_cols[0] is the time column.
    seasonality_periods / num_seasonal_harmonics: seasonal Fourier features of
      the raw time index; periods may be pandas aliases when timetype='index'.
    fourier_degrees: octaves of Fourier features per input (default 5 each).
    interactions: list of (i, j) input-column pairs whose product is a feature.
    freq, timetype: 'index' needs a datetime column and `freq`; 'float' a
      float column and no `freq`.
    depth, width: hidden layers and units.
    observation_model: 'NORMAL', 'NB' or 'ZINB'.
    standardize: columns to z-score (never the time column).
  Extra (not in the reference): compute_dtype 'fp32' | 'fp32_split' | 'bf16' | 'fp8' selects the
    arithmetic of the dense contractions on the GPU (fp32 accumulate either
    way; engine.default_dtype); default from env BNF_DTYPE, else 'fp32_split' (f32 storage, split-bf16 contractions:
    within the fp32 parity gates; 'fp32' = the exact f32 MFMA chain).  init_rng 'jax' | 'philox': 'jax'
    (default, env BNF_INIT_RNG) draws the initial Dense kernels from the reference's own streams
    for `seed` (jax threefry + TFP seed chain restated in `jaxseed`), so a full-batch fit follows
    the reference's trajectory; 'philox' uses the device generator.
  """

  _ensemble_dims: int
  _prior_weight: float = 1.0
  _scale_epochs_by_batch_size: bool = False

  def __init__(self, *, feature_cols, target_col, seasonality_periods=None,
               num_seasonal_harmonics=None, fourier_degrees=None,
               interactions=None, freq=None, timetype='index', depth=2,
               width=512, observation_model='NORMAL', standardize=None,
               compute_dtype=None, init_rng=None):
    self.feature_cols = feature_cols
    self.target_col = target_col
    self.seasonality_periods = seasonality_periods
    self.num_seasonal_harmonics = num_seasonal_harmonics
    self.fourier_degrees = fourier_degrees
    self.interactions = interactions
    self.freq = freq
    self.timetype = timetype
    self.depth = depth
    self.width = width
    self.observation_model = observation_model
    self.standardize = standardize
    self.compute_dtype = compute_dtype
    self.init_rng = init_rng
    self._check_engine_limits(len(feature_cols))
    self.losses_ = None
    self.params_ = None
    self.data_handler = SpatiotemporalDataHandler(
        feature_cols, target_col, timetype, freq, standardize=standardize)

  # ---- argument normalisation (reference :296-358) ------------------------
  def _get_fourier_degrees(self, batch_shape):
    ncol = batch_shape[-1]
    if self.fourier_degrees is None:
      return np.full(ncol, 5, dtype=int)
    degrees = np.atleast_1d(self.fourier_degrees).astype(int)
    if degrees.shape[-1] != ncol:
      raise ValueError(
          f'The length of fourier_degrees ({degrees.shape[-1]}) must match the '
          f'input dimension dimension ({ncol}).')
    return degrees

  def _get_interactions(self):
    if self.interactions is None:
      return np.zeros((0, 2), dtype=int)
    pairs = np.array(self.interactions).astype(int)
    if pairs.ndim != 2 or pairs.shape[-1] != 2:
      raise ValueError(
          'The argument for `interactions` should be a 2-d array of integers '
          'of shape (N, 2), indicating the column indices to interact (the '
          f' passed shape was {pairs.shape})')
    return pairs

  def _get_seasonality_periods(self):
    index_time = self.timetype == 'index'
    if (index_time and self.freq is None) or (
        self.timetype == 'float' and self.freq is not None):
      raise ValueError(f'Invalid {self.freq=} with {self.timetype=}.')
    if self.seasonality_periods is None:
      return np.zeros(0)
    if index_time:
      return seasonalities_to_array(self.seasonality_periods, self.freq)
    if self.timetype == 'float':
      return np.asarray(self.seasonality_periods, dtype=float)
    raise AssertionError(f'Impossible {self.timetype=}.')

  def _get_num_seasonal_harmonics(self):
    if self.timetype == 'index':
      if self.num_seasonal_harmonics is None:
        return np.zeros(0)
      return np.array(self.num_seasonal_harmonics)
    if self.timetype == 'float':
      if self.num_seasonal_harmonics is not None:
        raise ValueError(
            f'Cannot use num_seasonal_harmonics with {self.timetype=}.')
      # continuous time: exactly one harmonic per period; any 0 < h <= p/2
      # below 1 makes arange(1, 1 + h) == [1] in the frequency table.
      return np.fmin(.5, self._get_seasonality_periods() / 2)
    raise AssertionError(f'Impossible {self.timetype=}.')

  def _check_engine_limits(self, n_inputs=None):
    """The HIP engine's hard limits, reported here with the estimator's own argument names
    instead of as an error code from deep inside `fit` (include/bnf.h BNF_MAX_*)."""
    if not isinstance(self.width, (int, np.integer)) or not 1 <= self.width <= 8192:
      raise ValueError(f'width={self.width}: the MI355X engine supports widths 1..8192')
    if not 1 <= int(self.depth) <= 8:
      raise ValueError(f'depth={self.depth}: the MI355X engine supports 1..8 hidden layers')
    if n_inputs is not None and n_inputs > 8:
      raise ValueError(f'{n_inputs} feature columns: the MI355X engine supports at most 8')
    if self.interactions is not None and len(self.interactions) > 16:
      raise ValueError(f'{len(self.interactions)} interactions: the MI355X engine supports at most 16')

  def _model_args(self, batch_shape):
    self._check_engine_limits(batch_shape[-1])
    return dict(
        depth=self.depth,
        input_scales=self.data_handler.get_input_scales(),
        num_seasonal_harmonics=self._get_num_seasonal_harmonics(),
        seasonality_periods=self._get_seasonality_periods(),
        width=self.width,
        init_x=batch_shape,
        fourier_degrees=self._get_fourier_degrees(batch_shape),
        interactions=self._get_interactions(),
    )

  # ---- public API -----------------------------------------------------------
  def fit(self, table, seed):
    raise NotImplementedError('Should be implemented by subclass')

  def predict(self, table, quantiles=(0.5,), approximate_quantiles=False, weights=None):
    """-> (means, quantiles): means has shape
    (num_devices, ensemble_size // num_devices, len(table)) (VI: an extra
    posterior-sample axis after num_devices); quantiles is a list with one
    (len(table),) array per requested level, for the equal-weight mixture of
    all members.  Exact quantiles use Chandrupatla root finding; approximate
    ones the moment-matched Normal.
    weights (the shape of `score(...)['member_log_prob']`, e.g. `stacking_weights(...)['weights']`): the quantiles are
    those of the weighted mixture of members; `means` is per member and does not change.  None: equal weights."""
    kw = self._weights_kw(weights)
    rows = self.data_handler.get_test(table)
    return inference.predict_bnf(
        rows,
        self.observation_model,
        params=self.params_,
        model_args=self._model_args(rows.shape),
        quantiles=quantiles,
        ensemble_dims=self._ensemble_dims,
        approximate_quantiles=approximate_quantiles,
        compute_dtype=self.compute_dtype,
        **kw,
    )

  def predict_samples(self, table, num_samples=1000, seed=0, group_by=None, weights=None):
    """Joint posterior-predictive sample paths at the rows of `table`, drawn on the GPU.  Each path uses one member
    (VI: one member and one posterior draw) for all rows and adds that member's observation noise per row, so sums
    over rows carry the right spread -- what no marginal quantile of `predict` gives.
      group_by=None                    -> (num_samples, len(table)) float32
      group_by=column or [columns]     -> (totals, keys): totals (num_samples, G) float64, the paths summed over
        the rows of every group; keys the sorted pandas Index (MultiIndex for several columns) of the groups.  The
        group columns are any columns of `table`, feature or not.
    The same (seed, table) gives the same numbers whatever num_samples is asked for (path s does not change).
    weights (the shape of `score(...)['member_log_prob']`, e.g. `stacking_weights(...)['weights']`): a path draws its
    member with these probabilities instead of equal ones.  None: equal weights, nothing changes."""
    f = self._paths('predict_samples', table, group_by, num_samples, seed, weights, tag='')
    out = f.run(inference.sample_predictive)
    return out if group_by is None else (out, f.keys)

  def _paths(self, what, table, group_by, num_samples, seed, weights, noun=None, tag=None, target=False,
             threshold=None, needs_threshold=None, ordered=False, order_by=None):
    """The front of every method that works on sample paths, its stages in the one order all of them check in: fitted;
    the target column (target=True: a score_* method); the sample count, capped where `noun` names what
    bnf_sample_summaries summarises; the per-row threshold (needs_threshold True: required, False: optional, None: the
    method has none); the member weights; the grouping (group_by=None: none; ordered=True: the rows of a group in the
    order of `order_by`, None = the time column).  All of it ValueError before any GPU work.
    -> namespace: y, thr, keys, seg_offsets, seg_rows, and run(fn, **particular): the call of the inference function
    `fn` at the rows of `table` with the arguments all of them share plus its particular ones."""
    if self.params_ is None:
      raise ValueError(f'{what} before fit')
    tag = f'{what}: ' if tag is None else tag
    y = self._targets(what, table) if target else None
    if int(num_samples) < 1:
      raise ValueError(f'{tag}num_samples={num_samples}: need at least one sample path')
    if noun is not None and int(num_samples) > inference._native.SUMMARY_MAX_SAMPLES:
      raise ValueError(f'{tag}num_samples={num_samples}: the {noun} are summarised from at most '
                       f'{inference._native.SUMMARY_MAX_SAMPLES} sample paths')
    thr = None if needs_threshold is None else self._row_threshold(what, table, threshold, needs_threshold)
    kw = self._weights_kw(weights)
    keys = seg_offsets = seg_rows = None
    if ordered:
      keys, seg_offsets, seg_rows = group_rows_ordered(
          table, group_by, self.data_handler._time_column if order_by is None else order_by)
    elif group_by is not None:
      keys, seg_offsets, seg_rows = group_rows(table, group_by)

    def run(fn, **particular):
      rows = self.data_handler.get_test(table)
      return fn(rows, self.observation_model, self.params_, self._model_args(rows.shape), int(num_samples), seed,
                ensemble_dims=self._ensemble_dims, compute_dtype=self.compute_dtype,
                **({} if keys is None else {'groups': (seg_offsets, seg_rows)}), **particular, **kw)

    return types.SimpleNamespace(y=y, thr=thr, keys=keys, seg_offsets=seg_offsets, seg_rows=seg_rows, run=run)

  @staticmethod
  def _row_threshold(what, table, threshold, required):
    """`threshold`, a scalar or one limit per row of `table` -> (len(table),) float64 holding float32 values (the draws
    are float32: compared at that precision); None stays None unless `required`."""
    if threshold is None:
      if required:
        raise ValueError(f'{what}: threshold is required: a number or one number per row of the table')
      return None
    try:
      thr = np.asarray(threshold, dtype=np.float64)
    except (TypeError, ValueError) as e:
      raise ValueError(f'{what}: threshold must be a number or one number per row of the table') from e
    if thr.ndim == 0:
      thr = np.full(len(table), float(thr))
    if thr.shape != (len(table),):
      raise ValueError(f'{what}: threshold must be a scalar or hold one limit per row ({len(table)},); got {thr.shape}')
    if not np.all(np.isfinite(thr)):
      raise ValueError(f'{what}: threshold must be finite')
    return thr.astype(np.float32).astype(np.float64)

  def _weights_kw(self, weights):
    """{} for weights=None (the callee is called as before), else the checked weights as a keyword argument."""
    if weights is None:
      return {}
    inference.mixture_weights(weights, self.params_, self._ensemble_dims)      # ValueError before any GPU work
    return {'weights': np.asarray(weights, dtype=np.float64)}

  def _targets(self, what, table):
    """The target column as float64, with the checks of `score`: NaN allowed, infinite or (count models) non-integer
    targets refused."""
    if self.target_col not in table.columns:
      raise ValueError(f'{what}: the target column {self.target_col!r} is not among the columns of the table')
    y = np.asarray(table[self.target_col].values, dtype=np.float64)
    if np.isinf(y).any():
      raise ValueError(f'{what}: infinite targets')
    seen = y[np.isfinite(y)]
    if self.observation_model != 'NORMAL' and (np.any(seen < 0) or np.any(seen != np.floor(seen))):
      raise ValueError(f'{what}: the {self.observation_model} observation model takes non-negative integer targets')
    return y

  def _stack(self, what, table, weights, max_iter, tol):
    y = self._targets(what, table)
    rows = self.data_handler.get_test(table)
    return inference.stack_members(
        rows, y, self.observation_model, self.params_, self._model_args(rows.shape), ensemble_dims=self._ensemble_dims,
        weights=weights, max_iter=max_iter, tol=tol, compute_dtype=self.compute_dtype)

  def stacking_weights(self, table, max_iter=10000, tol=1e-5):
    """Stacking of the members' predictive distributions (Yao et al. 2018) on the rows of `table`, which should be
    held out from `fit`: the simplex weights that maximise the mean log density of `table[target_col]` under the
    weighted mixture of members, found on the GPU by EM from equal weights.  The loop stops when gap <= tol: gap bounds
    how far 'mean_log_density' is from the best any weights reach on these rows.  NaN targets are allowed (left out);
    the target checks are those of `score`.  -> dict:
      'weights'                       shape of `score(table)['member_log_prob']` (VI: posterior draws are components)
      'log_density'                   (len(table),) log density of the weighted mixture; NaN where the target is NaN,
                                      -inf on a dropped row
      'mean_log_density'              mean over the scored rows at 'weights'
      'equal_weight_mean_log_density' the same at equal weights: what `score(table)['mean_log_density']` reports
      'gap', 'iterations', 'converged'   converged: gap <= tol within max_iter updates
      'n', 'dropped'                  rows scored; rows to which every member with a positive weight gives density 0
    The weights are taken by `predict_samples`, `predict_totals`, `score_totals`, `predict_extremes`, `score_extremes`,
    `predict_episodes`, `score_episodes`, `predict_cumulative`, `score_cumulative`, `predict_windows`, `score_windows`,
    `predict_dependence`, `score_dependence`, `predict_ranking`, `score_ranking`, `predict_scenarios`, `score_scenarios`,
    `predict_combinations` and `score_combinations`
    (weights=...) and scored on another table by `weighted_log_density`; they are taken by the marginal forecast as well:
    `predict` and `score` (weights=...) give the quantiles, log density, pit, crps and rps of the weighted mixture.
    `fit` is unchanged."""
    if self.params_ is None:
      raise ValueError('stacking_weights before fit')
    res = self._stack('stacking_weights', table, None, max_iter, tol)
    lpd = res['log_density']
    return {'weights': res['weights'], 'log_density': lpd, 'mean_log_density': res['objective'],
            'equal_weight_mean_log_density': res['objective_start'], 'gap': res['gap'], 'iterations': res['iterations'],
            'converged': res['converged'], 'n': int(np.isfinite(lpd).sum()), 'dropped': res['dropped']}

  def weighted_log_density(self, table, weights):
    """The log density of `table[target_col]` under the mixture of members with the given `weights` (the shape of
    `score(table)['member_log_prob']`), e.g. weights learned by `stacking_weights` on another table.  -> dict:
      'log_density' (len(table),)   NaN where the target is NaN, -inf where every weighted member gives density 0
      'mean_log_density'            mean over the n scored rows        'n'
    With equal weights this is `score(table)['log_density']`."""
    if self.params_ is None:
      raise ValueError('weighted_log_density before fit')
    if weights is None:
      raise ValueError('weighted_log_density: weights are required')
    inference.mixture_weights(weights, self.params_, self._ensemble_dims)
    res = self._stack('weighted_log_density', table, weights, 0, 0.0)
    lpd = res['log_density']
    return {'log_density': lpd, 'mean_log_density': res['objective'], 'n': int(np.isfinite(lpd).sum())}

  def score(self, table, rps=False, weights=None):
    """The forecast at the rows of `table` scored against the observations `table[target_col]`, on the GPU.  NaN
    targets are allowed: their rows are reported as NaN and left out of every sum and mean.  rps=True (NB / ZINB;
    ValueError on NORMAL, whose score of this kind is 'crps') adds the ranked probability score, the CRPS of a count
    forecast: sum_k (F(k) - 1{k >= target})^2 with F the mixture CDF.  -> dict:
      'n'                 number of rows scored (finite targets)
      'log_density'       (len(table),) log density of the equal-weight mixture over members at the target
      'pit'               (2, len(table)) mixture CDF at the target and just below it (equal for NORMAL; for counts a
                          randomised PIT is uniform between the two)
      'crps'              (len(table),) continuous ranked probability score; NORMAL only, absent otherwise
      'member_log_prob'   leading ensemble dims of `params_`: every member's log density summed over the scored rows
                          (`likelihood_model(table).log_prob(target)` without the trip through the host)
      'mean_log_density', 'mean_crps' (NORMAL)   means over the scored rows
      'rps'               rps=True: (len(table),) ranked probability score; NaN also on a row whose forecast is so wide
                          that the sum would take more than 2^20 terms (a mean of 1e6 at total_count 0.05 is)
      'mean_rps'          rps=True: mean over the scored rows whose 'rps' is not NaN
      'rps_capped'        rps=True: the rows with a finite target whose 'rps' is NaN -- capped, or a member whose
                          parameters are not finite (0 at any realistic count forecast)
    weights (the shape of 'member_log_prob', e.g. `stacking_weights(...)['weights']`): 'log_density', 'pit', 'crps',
    'rps' and their 'mean_*' / 'rps_capped' are those of the weighted mixture of members -- the forecast whose
    quantiles `predict(weights=...)` reports; 'member_log_prob' and 'n' do not change.  None: equal weights."""
    if self.params_ is None:
      raise ValueError('score before fit')
    if rps and self.observation_model == 'NORMAL':
      raise ValueError("score: rps=True is for the count observation models (NB, ZINB); NORMAL is scored by 'crps'")
    y = self._targets('score', table)
    seen = y[np.isfinite(y)]
    kw = self._weights_kw(weights)
    rows = self.data_handler.get_test(table)
    out = inference.score_predictive(
        rows, y, self.observation_model, self.params_, self._model_args(rows.shape),
        ensemble_dims=self._ensemble_dims, compute_dtype=self.compute_dtype, rps=bool(rps), **kw)
    out['n'] = int(seen.size)
    for key in ('log_density', 'crps'):
      if key in out:
        out['mean_' + key] = float(np.mean(out[key][np.isfinite(y)], dtype=np.float64)) if seen.size else float('nan')
    if rps:
      kept = np.isfinite(y) & ~np.isnan(out['rps'])
      out['rps_capped'] = int(seen.size - kept.sum())
      out['mean_rps'] = float(np.mean(out['rps'][kept], dtype=np.float64)) if kept.any() else float('nan')
    return out

  def predict_totals(self, table, group_by, quantiles=(0.5,), num_samples=1000, seed=0, weights=None):
    """Mean and quantile bands of the group totals of `predict_samples(table, num_samples, seed, group_by=group_by)`,
    summarised on the GPU: the (num_samples, G) matrix of totals never leaves the device.  -> (mean (G,), [one (G,) array
    per level, numpy's default 'linear' quantile of the sampled totals], keys) with keys as in `predict_samples`.
    num_samples <= 16,384.  weights: member weights of the sample paths as in `predict_samples`; None: equal weights."""
    f = self._paths('predict_totals', table, group_by, num_samples, seed, weights, noun='totals')
    out = f.run(inference.total_summaries, quantiles=tuple(quantiles), energy=False)
    return out['mean'], [out['quantiles'][i] for i in range(out['quantiles'].shape[0])], f.keys

  def score_totals(self, table, group_by, quantiles=(0.025, 0.5, 0.975), num_samples=1000, seed=0, energy=True,
                   weights=None):
    """The forecast of the group totals -- the sample paths of `predict_samples(table, num_samples, seed,
    group_by=group_by)` -- scored against the observed totals of `table[target_col]`, on the GPU.  -> dict:
      'keys'          the groups, as in `predict_samples`
      'observed'      (G,) sum of the target over the group's rows; NaN when any row of the group has a NaN target: such
                      a group is not scored
      'mean'          (G,) mean of the sampled totals       'quantiles'  (len(quantiles), G) their 'linear' quantiles
      'crps'          (G,) ensemble CRPS of every total, E|X - y| - E|X - X'| / 2 over the sample paths; NaN where not scored
      'pit'           (2, G) share of the sampled totals <= and < the observed one (totals of counts tie)
      'n'             number of groups scored       'mean_crps'  mean of 'crps' over them
      'energy_score'  energy=True: the energy score of the joint paths over the scored groups, one number for the
                      whole vector of totals (num_samples^2 G / 2 differences)
    num_samples <= 16,384.  weights: member weights of the sample paths as in `predict_samples`; None: equal weights."""
    f = self._paths('score_totals', table, group_by, num_samples, seed, weights, noun='totals', target=True)
    observed = group_target_sums(f.y, f.seg_offsets, f.seg_rows)
    out = f.run(inference.total_summaries, observed=observed, quantiles=tuple(quantiles), energy=bool(energy))
    scored = ~np.isnan(observed)
    out.update(keys=f.keys, observed=observed, n=int(scored.sum()))
    out['mean_crps'] = float(np.mean(out['crps'][scored], dtype=np.float64)) if scored.any() else float('nan')
    return out

  def _combination_summaries(self, what, table, combinations, quantiles, num_samples, seed, weights, samples=False,
                             target=False, energy=False):
    """The shared front (`_paths` without a grouping), then the spec -> CSR, the observed combinations for a score, and the
    call.  -> (keys, observed or None, dict of `inference.combination_summaries`)."""
    f = self._paths(what, table, None, num_samples, seed, weights, noun='combinations', target=target)
    names = None
    if (isinstance(combinations, tuple) and len(combinations) == 2 and isinstance(combinations[1], tuple)
        and len(combinations[1]) == 3):                       # what group_combinations / stack_combinations return
      names, combinations = combinations
    try:
      keys, off, rows, coef = inference.combinations_csr(combinations, len(table), names=names)
    except ValueError as e:
      raise ValueError(f'{what}: {e}') from e
    if int(num_samples) * len(keys) > inference._TOTALS_MAX_CELLS:
      raise ValueError(f'{what}: {num_samples} sample paths x {len(keys)} combinations: at most '
                       f'{inference._TOTALS_MAX_CELLS} cells')
    observed = combination_target_sums(f.y, off, rows, coef) if target else None
    out = f.run(inference.combination_summaries, combinations=(off, rows, coef), observed=observed, quantiles=tuple(quantiles), energy=bool(energy),
                samples=bool(samples))
    return keys, observed, out

  def predict_combinations(self, table, combinations, quantiles=(0.5,), num_samples=1000, seed=0, weights=None,
                           samples=False):
    """Mean and quantile bands of LINEAR COMBINATIONS of the rows of the sample paths of `predict_samples(table,
    num_samples, seed)`: weighted means (the population-weighted mean of a region, incidence per 100k), contrasts (this
    week minus last week, place A minus place B) and overlapping groups (a row in its county, its state and the nation),
    all in the same paths, formed and summarised on the GPU.  `combinations` is
      a dict name -> one coefficient per row of `table`, a dense (K, len(table)) array, or a COO tuple (form, row, coef)
      (`inference.combinations_csr`), or
      what `group_combinations` / `stack_combinations` return: (keys, (form, row, coef)).
    A row may occur in many combinations or in none; coefficients of 0 are dropped.  -> dict:
      'keys'       the combinations: the dict's names, the keys given, or a RangeIndex
      'mean' (K,)  'quantiles' (len(quantiles), K)   numpy's default 'linear' quantile of the sampled values
      'samples'    samples=True: (num_samples, K) float64, the sampled values themselves; equal to
                   predict_samples(table, num_samples, seed) @ coefficients.T up to float64 rounding
    num_samples <= 16,384 and num_samples * K <= 2^28.  A row named by m combinations is drawn m times.
    weights: member weights of the sample paths as in `predict_samples`; None: equal weights."""
    keys, _, out = self._combination_summaries('predict_combinations', table, combinations, quantiles, num_samples, seed,
                                               weights, samples=samples)
    out['keys'] = keys
    return out

  def score_combinations(self, table, combinations, quantiles=(0.025, 0.5, 0.975), num_samples=1000, seed=0, energy=True,
                         weights=None):
    """The forecast of `predict_combinations(table, combinations, ...)` scored against the same combinations of the
    observations `table[target_col]`, on the GPU.  -> the dict of `predict_combinations` (with 'samples' left out) plus
      'observed'      (K,) sum of coefficient x target over the combination's rows; NaN when any of them has a NaN
                      target (rows with coefficient 0 do not count): such a combination is not scored
      'crps'          (K,) ensemble CRPS of every combination; NaN where not scored       'pit'  (2, K) as in `score_totals`
      'n'             number of combinations scored       'mean_crps'  mean of 'crps' over them
      'energy_score'  energy=True: the energy score of the joint paths over the scored combinations
    The target checks are those of `score_totals`."""
    keys, observed, out = self._combination_summaries('score_combinations', table, combinations, quantiles, num_samples,
                                                      seed, weights, target=True, energy=energy)
    scored = ~np.isnan(observed)
    out.update(keys=keys, observed=observed, n=int(scored.sum()))
    out['mean_crps'] = float(np.mean(out['crps'][scored], dtype=np.float64)) if scored.any() else float('nan')
    return out

  def _extreme_summaries(self, what, table, group_by, threshold, quantiles, num_samples, seed, weights, target=False):
    f = self._paths(what, table, group_by, num_samples, seed, weights, noun='extremes', target=target,
                    threshold=threshold, needs_threshold=False)
    thr = f.thr
    observed = None if f.y is None else group_target_extremes(f.y, f.seg_offsets, f.seg_rows, thr)
    out = f.run(inference.extreme_summaries, threshold=thr, observed_max=None if observed is None else observed[0],
                observed_count=None if observed is None else observed[2], quantiles=tuple(quantiles))
    res = {'keys': f.keys, 'max_mean': out['max_mean'], 'max_quantiles': out['max_quantiles'],
           'peak_probability': out['peak_probability']}
    if thr is not None:
      res.update(exceed_any=out['exceed_any'], exceed_count_mean=out['count_mean'],
                 exceed_count_quantiles=out['count_quantiles'], exceed_probability=out['exceed_probability'])
    return res, out, observed

  def predict_extremes(self, table, group_by, threshold=None, quantiles=(0.5,), num_samples=1000, seed=0, weights=None):
    """Group peaks and threshold exceedances of the sample paths of `predict_samples(table, num_samples, seed)`, formed
    and summarised on the GPU: neither the draws nor the (num_samples, G) matrices leave the device.  What no marginal
    quantile of `predict` gives: the maximum and the count of a path depend on one member driving all rows.  -> dict:
      'keys'                    the groups, as in `predict_samples`
      'max_mean' (G,)  'max_quantiles' (len(quantiles), G)   the distribution of the group's peak value ('linear' quantiles)
      'peak_probability' (len(table),)   the share of the paths in which the row is where its group first reaches its
                                maximum (ties, frequent for counts, go to the group's first row in table order): sums to 1
                                over the rows of every group
    and with `threshold`, a scalar or one finite limit per row, in the units of the target column, compared with strict >
    at float32 precision (the precision of the draws):
      'exceed_any' (G,)         the share of the paths with at least one row of the group above its threshold
      'exceed_count_mean' (G,)  'exceed_count_quantiles' (len(quantiles), G)   the number of rows of the group above
      'exceed_probability' (len(table),)   the share of the paths whose draw at the row is above its threshold
    num_samples <= 16,384.  weights: member weights of the sample paths as in `predict_samples`; None: equal weights."""
    return self._extreme_summaries('predict_extremes', table, group_by, threshold, quantiles, num_samples, seed, weights)[0]

  def score_extremes(self, table, group_by, threshold=None, quantiles=(0.025, 0.5, 0.975), num_samples=1000, seed=0,
                     weights=None):
    """The forecast of `predict_extremes` scored against the peaks and exceedances observed in `table[target_col]`, on
    the GPU.  -> the dict of `predict_extremes` plus
      'observed_max' (G,)  'observed_peak_row' (G,)   the largest target of the group and the first table row (position)
                                at which it is reached; NaN / -1 when any row of the group has a NaN target: such a
                                group is not scored
      'max_crps' (G,)  'max_pit' (2, G)   ensemble CRPS of the peak value and the share of the sampled peaks <= and < the
                                observed one; NaN where not scored
      'peak_row_probability' (G,)   the forecast probability ('peak_probability') of the observed peak row
      'n'                       number of groups scored       'mean_max_crps', 'mean_peak_row_probability'  means over them
    and with `threshold`:
      'observed_count' (G,)     the rows of the group whose target is > their threshold
      'count_crps' (G,)  'count_pit' (2, G)   the same scores of the number of rows above
      'brier' (G,)              (exceed_any - 1{observed_count > 0})^2
      'mean_count_crps', 'mean_brier'
    The target checks are those of `score_totals`."""
    res, out, (obs_max, obs_row, obs_count) = self._extreme_summaries(
        'score_extremes', table, group_by, threshold, quantiles, num_samples, seed, weights, target=True)
    scored = ~np.isnan(obs_max)
    mean = lambda a: float(np.mean(a[scored], dtype=np.float64)) if scored.any() else float('nan')
    prob = np.where(scored, res['peak_probability'][np.maximum(obs_row, 0)], np.nan)
    res.update(observed_max=obs_max, observed_peak_row=obs_row, max_crps=out['max_crps'], max_pit=out['max_pit'],
               peak_row_probability=prob, n=int(scored.sum()), mean_max_crps=mean(out['max_crps']),
               mean_peak_row_probability=mean(prob))
    if obs_count is not None:
      hit = np.where(scored, (obs_count > 0).astype(np.float64), np.nan)
      brier = (res['exceed_any'] - hit) ** 2
      res.update(observed_count=obs_count, count_crps=out['count_crps'], count_pit=out['count_pit'], brier=brier,
                 mean_count_crps=mean(out['count_crps']), mean_brier=mean(brier))
    return res

  def _episode_summaries(self, what, table, group_by, threshold, order_by, quantiles, num_samples, seed, weights,
                         target=False):
    f = self._paths(what, table, group_by, num_samples, seed, weights, noun='episodes', target=target,
                    threshold=threshold, needs_threshold=True, ordered=True, order_by=order_by)
    n_groups = len(f.keys)
    if int(num_samples) * n_groups > inference._TOTALS_MAX_CELLS:      # before the host pass over the observed spells
      raise ValueError(f'{what}: {num_samples} sample paths x {n_groups} groups: the matrices are held whole on the '
                       f'device, at most {inference._TOTALS_MAX_CELLS} cells')
    observed = None if f.y is None else group_target_episodes(f.y, f.seg_offsets, f.seg_rows, f.thr)
    obs_kw = {} if observed is None else {f'observed_{k}': observed[k] for k in inference.EPISODE_SERIES}
    out = f.run(inference.episode_summaries, threshold=f.thr, quantiles=tuple(quantiles), **obs_kw)
    res = {'keys': f.keys, 'onset_probability': out['onset_probability'], 'no_episode': out['no_episode']}
    for name in inference.EPISODE_SERIES:
      res[f'{name}_mean'], res[f'{name}_quantiles'] = out[f'{name}_mean'], out[f'{name}_quantiles']
    return res, out, observed

  def predict_episodes(self, table, group_by, threshold, order_by=None, quantiles=(0.5,), num_samples=1000, seed=0,
                       weights=None):
    """Spells above a threshold in the sample paths of `predict_samples(table, num_samples, seed)`: when a group's
    series first goes above its limit, how long it stays there and whether it is one wave or several, formed and
    summarised on the GPU (neither the draws nor the (num_samples, G) matrices leave the device).  These depend on the
    ORDER of a group's rows: `order_by=None` orders them by the time column (feature_cols[0]), a column name by that
    column; ties keep table order.  threshold: a scalar or one finite limit per row, in the units of the target column,
    compared with strict > at float32 precision (the precision of the draws).  -> dict:
      'keys'                     the groups, as in `predict_samples`
      'longest_mean' (G,)  'longest_quantiles' (len(quantiles), G)   the longest run of consecutive rows above
      'spells_mean', 'spells_quantiles'                              the number of separate runs
      'onset_step_mean', 'onset_step_quantiles'                      the rows before the first one above; a path that
                                 never goes above counts the group's size (censored at the horizon)
      'onset_probability' (len(table),)   the share of the paths in which the row is its group's first row above
      'no_episode' (G,)          the share of the paths that never go above: 1 - the group's sum of 'onset_probability'
    num_samples <= 16,384.  weights: member weights of the sample paths as in `predict_samples`; None: equal weights."""
    return self._episode_summaries('predict_episodes', table, group_by, threshold, order_by, quantiles, num_samples, seed,
                                   weights)[0]

  def score_episodes(self, table, group_by, threshold, order_by=None, quantiles=(0.025, 0.5, 0.975), num_samples=1000,
                     seed=0, weights=None):
    """The forecast of `predict_episodes` scored against the spells observed in `table[target_col]`, on the GPU.  -> the
    dict of `predict_episodes` plus, for name in 'longest', 'spells', 'onset_step':
      'observed_<name>' (G,)     `group_target_episodes` on the target (onset_step censored as the forecast is); NaN when
                                 any row of the group has a NaN target: such a group is not scored
      '<name>_crps' (G,)  '<name>_pit' (2, G)   ensemble CRPS and the share of the sampled values <= and < the observed
                                 one; NaN where not scored
      'mean_<name>_crps'         mean over the scored groups
    and
      'observed_onset_row' (G,)  the first table row above its threshold, -1 if none (or not scored)
      'onset_row_probability' (G,)   the forecast probability ('onset_probability') of the observed onset row, or
                                 'no_episode' when nothing was observed above; NaN where not scored
      'n'                        number of groups scored       'mean_onset_row_probability'
    The target checks are those of `score_totals`."""
    res, out, observed = self._episode_summaries(
        'score_episodes', table, group_by, threshold, order_by, quantiles, num_samples, seed, weights, target=True)
    scored = ~np.isnan(observed['longest'])
    mean = lambda a: float(np.mean(a[scored], dtype=np.float64)) if scored.any() else float('nan')
    first = observed['first_row']
    prob = np.where(first >= 0, res['onset_probability'][np.maximum(first, 0)], res['no_episode'])
    prob = np.where(scored, prob, np.nan)
    res.update(observed_onset_row=first, onset_row_probability=prob, n=int(scored.sum()),
               mean_onset_row_probability=mean(prob))
    for name in inference.EPISODE_SERIES:
      res[f'observed_{name}'] = observed[name]
      res[f'{name}_crps'], res[f'{name}_pit'] = out[f'{name}_crps'], out[f'{name}_pit']
      res[f'mean_{name}_crps'] = mean(out[f'{name}_crps'])
    return res

  @staticmethod
  def _group_level(what, table, level, seg_offsets, seg_rows, name='level'):
    """The level (or, under another `name`, threshold) of every group from `level`: None, a scalar, a column of `table`
    or one value per table row; constant within every group and finite, any sign -> (G,) float64 or None."""
    if level is None:
      return None
    if isinstance(level, str):
      if level not in table.columns:
        raise ValueError(f'{what}: {name}: {level!r} is not among the columns of the table')
      level = table[level].values
    try:
      v = np.asarray(level, dtype=np.float64)
    except (TypeError, ValueError) as e:
      raise ValueError(f'{what}: {name} must be a number, a column of the table or one number per row') from e
    if v.ndim == 0:
      v = np.full(len(table), float(v))
    if v.shape != (len(table),):
      raise ValueError(f'{what}: {name} must be a scalar or hold one value per row ({len(table)},); got {v.shape}')
    if not np.all(np.isfinite(v)):
      raise ValueError(f'{what}: {name} must be finite')
    ordered = v[np.asarray(seg_rows, dtype=np.int64)]
    starts = np.asarray(seg_offsets[:-1], dtype=np.int64)
    lo, hi = np.minimum.reduceat(ordered, starts), np.maximum.reduceat(ordered, starts)
    if np.any(lo != hi):
      raise ValueError(f'{what}: {name} must be constant within every group')
    return lo

  def _cumulative_summaries(self, what, table, group_by, level, order_by, quantiles, curve, num_samples, seed, weights,
                            target=False):
    f = self._paths(what, table, group_by, num_samples, seed, weights, noun='running totals', target=target,
                    ordered=True, order_by=order_by)
    lvl = self._group_level(what, table, level, f.seg_offsets, f.seg_rows)
    for n, held in ((len(f.keys), 'groups: the totals matrix is'), (len(table) if curve else 0, 'rows: the running totals are')):
      if int(num_samples) * n > inference._TOTALS_MAX_CELLS:             # before the host pass over the observed curve
        raise ValueError(f'{what}: {num_samples} sample paths x {n} {held} held whole on the device, at most '
                         f'{inference._TOTALS_MAX_CELLS} cells')
    observed = None if f.y is None else group_target_cumulative(f.y, f.seg_offsets, f.seg_rows, lvl)
    obs_kw = {}
    if observed is not None:
      obs_kw['observed_total'] = observed['total']
      if curve:
        obs_kw['observed_running'] = observed['running']
      if lvl is not None:
        obs_kw['observed_cross_step'] = observed['cross_step']
    out = f.run(inference.cumulative_summaries, level=lvl, curve=bool(curve), quantiles=tuple(quantiles), **obs_kw)
    res = {'keys': f.keys, 'total_mean': out['total_mean'], 'total_quantiles': out['total_quantiles']}
    if curve:
      res.update(running_mean=out['running_mean'], running_quantiles=out['running_quantiles'])
    if lvl is not None:
      res.update(crossing_step_mean=out['cross_step_mean'], crossing_step_quantiles=out['cross_step_quantiles'],
                 crossing_probability=out['crossing_probability'], above_probability=out['above_probability'],
                 never=out['never'])
    return res, out, observed

  def predict_cumulative(self, table, group_by, level=None, order_by=None, quantiles=(0.5,), curve=True, num_samples=1000,
                         seed=0, weights=None):
    """Running totals of the sample paths of `predict_samples(table, num_samples, seed)`: the cumulative curve of every
    group with its band, and when it passes a level, formed and summarised on the GPU (neither the draws nor the
    matrices leave the device).  The band of a running total at a row cannot be taken from any marginal of `predict`: it
    needs the joint paths.  These depend on the ORDER of a group's rows: `order_by=None` orders them by the time column
    (feature_cols[0]), a column name by that column; ties keep table order.  level: a scalar, a column name or one value
    per row, constant within every group and finite (any sign), in the units of the target column; a running total
    crosses at the first row at which it is strictly above.  -> dict:
      'keys'                     the groups, as in `predict_samples`
      'total_mean' (G,)  'total_quantiles' (len(quantiles), G)   the group's total: the curve's last value
    with curve=True (holds num_samples x len(table) values on the device, at most 2^28):
      'running_mean' (len(table),)  'running_quantiles' (len(quantiles), len(table))   the running total at every row
    and with `level`:
      'crossing_step_mean' (G,)  'crossing_step_quantiles' (len(quantiles), G)   the rows before the crossing row; a path
                                 that never crosses counts the group's size (censored at the horizon)
      'crossing_probability' (len(table),)   the share of the paths in which the row is its group's crossing row
      'above_probability' (len(table),)      the share of the paths whose running total at the row is above the level
                                 (for NORMAL a curve can come back under it: this is not the running sum of the former)
      'never' (G,)               the share of the paths that never cross: 1 - the group's sum of 'crossing_probability'
    num_samples <= 16,384.  A group of more than 1,024 rows is worked on by one workgroup per path: with 1,000 paths a
    table that is a single group of 10^6 rows takes 1.3 times the device time of its totals alone, with far fewer paths it
    fills the device only in part (profiles/group_cumulative.md).
    weights: member weights of the sample paths as in `predict_samples`; None: equal weights."""
    return self._cumulative_summaries('predict_cumulative', table, group_by, level, order_by, quantiles, curve,
                                      num_samples, seed, weights)[0]

  def score_cumulative(self, table, group_by, level=None, order_by=None, quantiles=(0.025, 0.5, 0.975), curve=True,
                       num_samples=1000, seed=0, weights=None):
    """The forecast of `predict_cumulative` scored against the running totals observed in `table[target_col]`, on the
    GPU.  -> the dict of `predict_cumulative` plus
      'observed_total' (G,)      `group_target_cumulative` on the target; NaN when any row of the group has a NaN target:
                                 such a group is not scored
      'total_crps' (G,)  'total_pit' (2, G)   ensemble CRPS and the share of the sampled totals <= and < the observed one;
                                 NaN where not scored
      'n'                        number of groups scored       'mean_total_crps'  mean over them
    with curve=True:
      'observed_running' (len(table),)   the observed running total at the row; NaN from a group's first NaN target on
      'running_crps' (len(table),)  'running_pit' (2, len(table))   the same scores row by row; NaN where not scored
      'mean_running_crps'        mean over the scored rows
    and with `level`:
      'observed_crossing_step' (G,)  'observed_crossing_row' (G,)   censored as the forecast is; -1 if none (or not scored)
      'crossing_step_crps' (G,)  'crossing_step_pit' (2, G)  'mean_crossing_step_crps'
      'crossing_row_probability' (G,)   the forecast probability ('crossing_probability') of the observed crossing row, or
                                 'never' when none was observed; NaN where not scored
      'mean_crossing_row_probability'
    The target checks are those of `score_totals`."""
    res, out, observed = self._cumulative_summaries('score_cumulative', table, group_by, level, order_by, quantiles, curve,
                                                    num_samples, seed, weights, target=True)
    scored = ~np.isnan(observed['total'])
    mean = lambda a: float(np.mean(a[scored], dtype=np.float64)) if scored.any() else float('nan')
    res.update(observed_total=observed['total'], total_crps=out['total_crps'], total_pit=out['total_pit'],
               n=int(scored.sum()), mean_total_crps=mean(out['total_crps']))
    if curve:
      rows = ~np.isnan(observed['running'])
      res.update(observed_running=observed['running'], running_crps=out['running_crps'], running_pit=out['running_pit'],
                 mean_running_crps=float(np.mean(out['running_crps'][rows], dtype=np.float64)) if rows.any() else float('nan'))
    if 'cross_step' in observed:
      row = observed['cross_row']
      prob = np.where(row >= 0, res['crossing_probability'][np.maximum(row, 0)], res['never'])
      prob = np.where(scored, prob, np.nan)
      res.update(observed_crossing_step=observed['cross_step'], observed_crossing_row=row,
                 crossing_step_crps=out['cross_step_crps'], crossing_step_pit=out['cross_step_pit'],
                 mean_crossing_step_crps=mean(out['cross_step_crps']), crossing_row_probability=prob,
                 mean_crossing_row_probability=mean(prob))
    return res

  def _window_summaries(self, what, table, group_by, window, threshold, order_by, quantiles, curve, num_samples, seed,
                        weights, target=False):
    f = self._paths(what, table, group_by, num_samples, seed, weights, noun='window totals', target=target,
                    ordered=True, order_by=order_by)
    try:
      window = inference._window_length(window)
    except ValueError as e:
      raise ValueError(f'{what}: {e}') from None
    thr = self._group_level(what, table, threshold, f.seg_offsets, f.seg_rows, name='threshold')
    for n, held in ((len(f.keys), 'groups: the peak matrix is'), (len(table) if curve else 0, 'rows: the window totals are')):
      if int(num_samples) * n > inference._TOTALS_MAX_CELLS:             # before the host pass over the observed windows
        raise ValueError(f'{what}: {num_samples} sample paths x {n} {held} held whole on the device, at most '
                         f'{inference._TOTALS_MAX_CELLS} cells')
    observed = None if f.y is None else group_target_windows(f.y, f.seg_offsets, f.seg_rows, window, thr)
    obs_kw = {}
    if observed is not None:
      obs_kw['observed_peak'] = observed['peak']
      if curve:
        obs_kw['observed_window'] = observed['window']
      if thr is not None:
        obs_kw['observed_count'] = observed['count']
    out = f.run(inference.window_summaries, window=window, threshold=thr, curve=bool(curve), quantiles=tuple(quantiles),
                **obs_kw)
    res = {'keys': f.keys, 'peak_mean': out['peak_mean'], 'peak_quantiles': out['peak_quantiles'],
           'peak_probability': out['peak_probability']}
    if curve:
      res.update(window_mean=out['window_mean'], window_quantiles=out['window_quantiles'])
    if thr is not None:
      res.update(count_mean=out['count_mean'], count_quantiles=out['count_quantiles'],
                 exceed_probability=out['exceed_probability'], any=out['any'])
    return res, out, observed

  def predict_windows(self, table, group_by, window, threshold=None, order_by=None, quantiles=(0.5,), curve=True,
                      num_samples=1000, seed=0, weights=None):
    """Moving-window totals of the sample paths of `predict_samples(table, num_samples, seed)`: the total over the last
    `window` rows of a group at every row (7-day incidence from daily rows), the worst `window` rows of the group and
    how often a window total passes a limit, formed and summarised on the GPU (neither the draws nor the matrices leave
    the device).  A window total is not a difference of two marginal bands: its band, its peak and the probability that
    it passes a limit need the joint paths.  These depend on the ORDER of a group's rows: `order_by=None` orders them by
    the time column (feature_cols[0]), a column name by that column; ties keep table order.  window: an integer number
    of rows >= 1.  Only FULL-LENGTH windows count; a group with fewer rows than `window` has one, its total.
    threshold: a scalar, a column name or one value per row, constant within every group and finite (any sign), in the
    units of the target column, compared with strict >.  -> dict:
      'keys'                     the groups, as in `predict_samples`
      'peak_mean' (G,)  'peak_quantiles' (len(quantiles), G)   the largest window total of the group
      'peak_probability' (len(table),)   the share of the paths whose largest window ends at the row (ties, frequent for
                                 counts, go to the earliest row): sums to 1 over the rows of every group
    with curve=True (holds num_samples x len(table) values on the device, at most 2^28):
      'window_mean' (len(table),)  'window_quantiles' (len(quantiles), len(table))   the window total ending at the row;
                                 NaN at the first window - 1 rows of a group, at which no full-length window ends
    and with `threshold`:
      'count_mean' (G,)  'count_quantiles' (len(quantiles), G)   the number of windows of the group above the threshold
      'exceed_probability' (len(table),)   the share of the paths whose window ending at the row is above it
      'any' (G,)                 the share of the paths with at least one window above it
    num_samples <= 16,384.  A group of more than 1,024 rows is worked on by one workgroup per path
    (profiles/group_windows.md).  weights: member weights of the sample paths as in `predict_samples`; None: equal
    weights."""
    return self._window_summaries('predict_windows', table, group_by, window, threshold, order_by, quantiles, curve,
                                  num_samples, seed, weights)[0]

  def score_windows(self, table, group_by, window, threshold=None, order_by=None, quantiles=(0.025, 0.5, 0.975),
                    curve=True, num_samples=1000, seed=0, weights=None):
    """The forecast of `predict_windows` scored against the window totals observed in `table[target_col]`, on the GPU.
    -> the dict of `predict_windows` plus
      'observed_peak' (G,)  'observed_peak_row' (G,)   `group_target_windows` on the target; NaN / -1 when any row of the
                                 group has a NaN target: such a group is not scored
      'peak_crps' (G,)  'peak_pit' (2, G)   ensemble CRPS and the share of the sampled peaks <= and < the observed one;
                                 NaN where not scored
      'peak_row_probability' (G,)   the forecast probability ('peak_probability') of the observed peak row
      'n'                        number of groups scored       'mean_peak_crps', 'mean_peak_row_probability'  means over them
    with curve=True:
      'observed_window' (len(table),)   the observed window total ending at the row; NaN where no full-length window
                                 ends or the window holds a NaN target
      'window_crps' (len(table),)  'window_pit' (2, len(table))   the same scores row by row; NaN where not scored
      'mean_window_crps'         mean over the scored rows
    and with `threshold`:
      'observed_count' (G,)      the observed windows of the group above the threshold
      'count_crps' (G,)  'count_pit' (2, G)  'mean_count_crps'
    The target checks are those of `score_totals`."""
    res, out, observed = self._window_summaries('score_windows', table, group_by, window, threshold, order_by, quantiles,
                                                curve, num_samples, seed, weights, target=True)
    scored = ~np.isnan(observed['peak'])
    mean = lambda a: float(np.mean(a[scored], dtype=np.float64)) if scored.any() else float('nan')
    row = observed['peak_row']
    prob = np.where(scored, res['peak_probability'][np.maximum(row, 0)], np.nan)
    res.update(observed_peak=observed['peak'], observed_peak_row=row, peak_crps=out['peak_crps'],
               peak_pit=out['peak_pit'], peak_row_probability=prob, n=int(scored.sum()),
               mean_peak_crps=mean(out['peak_crps']), mean_peak_row_probability=mean(prob))
    if curve:
      rows = ~np.isnan(observed['window'])
      res.update(observed_window=observed['window'], window_crps=out['window_crps'], window_pit=out['window_pit'],
                 mean_window_crps=float(np.mean(out['window_crps'][rows], dtype=np.float64)) if rows.any() else float('nan'))
    if 'count' in observed:
      res.update(observed_count=observed['count'], count_crps=out['count_crps'], count_pit=out['count_pit'],
                 mean_count_crps=mean(out['count_crps']))
    return res

  def _band_summaries(self, what, table, group_by, coverage, of, order_by, num_samples, seed, weights, target=False):
    if self.params_ is None:
      raise ValueError(f'{what} before fit')
    if of not in inference.BAND_OF:
      raise ValueError(f"{what}: of={of!r}: 'rows' (the draws at the rows) or 'cumulative' (their running totals)")
    if of == 'rows' and order_by is not None:
      raise ValueError(f"{what}: order_by orders a running total: it needs of='cumulative'")
    if of == 'cumulative' and group_by is None:
      raise ValueError(f"{what}: of='cumulative' needs group_by: a running total runs along the rows of a group")
    f = self._paths(what, table, group_by, num_samples, seed, weights, noun='bands', target=target,
                    ordered=of == 'cumulative', order_by=order_by)
    try:
      levels = inference._coverage_levels(coverage)
    except ValueError as e:
      raise ValueError(f'{what}: {e}') from e
    if len(table) == 0:
      raise ValueError(f'{what}: the table has no rows')
    if int(num_samples) * len(table) > inference._TOTALS_MAX_CELLS:
      raise ValueError(f'{what}: {num_samples} sample paths x {len(table)} rows: the sample paths are held whole on the '
                       f'device, at most {inference._TOTALS_MAX_CELLS} cells')
    keys, particular = f.keys, {}
    seg_offsets, seg_rows = f.seg_offsets, f.seg_rows
    if keys is None:                            # of='rows' without group_by: one group of all rows
      keys = pd.RangeIndex(1)
      seg_offsets = np.asarray([0, len(table)], dtype=np.int32)
      seg_rows = np.arange(len(table), dtype=np.int32)
      particular['groups'] = (seg_offsets, seg_rows)
    observed = None
    if f.y is not None:
      observed = f.y if of == 'rows' else group_target_cumulative(f.y, seg_offsets, seg_rows)['running']
      particular['observed'] = observed
    out = f.run(inference.band_summaries, coverage=tuple(levels), of=of, **particular)
    res = {'keys': keys}
    res.update({k: out[k] for k in ('level', 'coverage', 'pointwise_joint_coverage', 'lower', 'upper', 'pointwise_lower',
                                    'pointwise_upper')})
    return res, out, observed

  def predict_bands(self, table, group_by, coverage=(0.9,), of='rows', order_by=None, num_samples=1000, seed=0,
                    weights=None):
    """SIMULTANEOUS bands of the sample paths of `predict_samples(table, num_samples, seed)`: for every group a band that
    holds a WHOLE path over the group's rows with probability `coverage`, formed on the GPU.  The quantiles of `predict`,
    `predict_cumulative` and `predict_windows` are pointwise: each holds, say, 90 % of the paths at one row, and far fewer
    paths stay inside at every row (`pointwise_joint_coverage` says how many); read a band of this method as "the curve
    stays in here".  The construction is the rank envelope: band k at a row runs from the k-th smallest to the k-th largest
    of the row's samples, and a group takes the largest k whose band still holds ceil(coverage * num_samples) paths whole.
      of='rows'         the curve is the value at every row of the group; group_by=None: one group of all rows
      of='cumulative'   the curve is the running total along the group's rows, ordered as in `predict_cumulative`
                        (`order_by=None`: by the time column); needs group_by
    -> dict, n_cov = len(coverage):
      'keys'                                     the groups, as in `predict_samples` (RangeIndex(1) for group_by=None)
      'level' (n_cov, G) int                     the band level k of the group, -1 where a draw of the group is NaN
      'coverage' (n_cov, G)                      the share of the paths the band holds whole, >= the coverage asked for
      'pointwise_joint_coverage' (n_cov, G)      the share of the paths that the pointwise band of the same coverage
                                                 (the one holding ceil(coverage * num_samples) samples at each row) holds whole
      'lower', 'upper' (n_cov, len(table))       the simultaneous band at every row (of='cumulative': of the running total)
      'pointwise_lower', 'pointwise_upper' (n_cov, len(table))   the pointwise band, for comparison
    1 <= len(coverage) <= 64, every level in (0, 1]; num_samples <= 16,384 and num_samples * len(table) <= 2^28.
    weights: member weights of the sample paths as in `predict_samples`; None: equal weights."""
    return self._band_summaries('predict_bands', table, group_by, coverage, of, order_by, num_samples, seed, weights)[0]

  def score_bands(self, table, group_by, coverage=(0.9,), of='rows', order_by=None, num_samples=1000, seed=0, weights=None):
    """The bands of `predict_bands` held against the curve observed in `table[target_col]` (of='cumulative': its running
    total per group, `group_target_cumulative`), on the GPU: a JOINT calibration check, which neither the energy nor the
    variogram score gives.  A NaN target takes no part (of='cumulative': nor does any later row of its group).  -> the
    dict of `predict_bands` plus
      'observed' (len(table),)      the observed curve, NaN where it takes no part
      'observed_depth' (G,)         the largest band level that holds the observed curve at every scored row of the group;
                                    -1: it leaves the envelope of all paths; NaN: no row of the group is scored
      'inside' (n_cov, G)           1.0 / 0.0: the band of that coverage holds the observed curve or not; NaN as above
      'depth_pit' (2, G)            the share of the paths whose depth is <= and < the observed curve's: a value drawn
                                    uniformly between the two is uniform for a calibrated forecast; near 0 = the observed
                                    curve is more extreme than nearly every path
      'n'                           number of groups scored       'share_inside' (n_cov,)   mean of 'inside' over them
    The target checks are those of `score_totals`."""
    res, out, observed = self._band_summaries('score_bands', table, group_by, coverage, of, order_by, num_samples, seed,
                                              weights, target=True)
    scored = ~np.isnan(out['observed_depth'])
    share = (np.mean(out['inside'][:, scored], axis=1, dtype=np.float64) if scored.any()
             else np.full(out['inside'].shape[0], np.nan))
    res.update(observed=observed, observed_depth=out['observed_depth'], inside=out['inside'], depth_pit=out['depth_pit'],
               n=int(scored.sum()), share_inside=share)
    return res

  def _dependence_summaries(self, what, table, group_by, num_samples, seed, weights, target=False, p=0.5,
                            pair_weights=None, matrices=True):
    f = self._paths(what, table, group_by, num_samples, seed, weights, target=target)
    observed = None if f.y is None else group_target_sums(f.y, f.seg_offsets, f.seg_rows)
    out = f.run(inference.dependence_summaries, observed=observed, p=p, pair_weights=pair_weights,
                matrices=bool(matrices))
    res = {'keys': f.keys, 'mean': out['mean']}
    if 'covariance' in out:
      cov = out['covariance']
      std = np.sqrt(np.diagonal(cov))
      flat = ~(std > 0)                             # a group without spread (or NaN) has no correlation
      with np.errstate(divide='ignore', invalid='ignore'):
        corr = cov / (std[:, None] * std[None, :])
      corr[flat, :] = np.nan
      corr[:, flat] = np.nan
      res.update(std=std, covariance=cov, correlation=corr)
    return res, out, observed

  def predict_dependence(self, table, group_by, num_samples=1000, seed=0, weights=None):
    """How the group totals of `predict_samples(table, num_samples, seed, group_by=group_by)` move together -- "if group A
    has a bad week, how likely is it that group B does too" -- formed on the GPU: the (num_samples, G) matrix of totals
    never leaves the device.  The sample paths are joint (one member drives all rows of a path), so the totals of
    different groups are dependent; no marginal forecast shows it.  -> dict:
      'keys'               the groups, as in `predict_samples`
      'mean' (G,)          'std' (G,)   mean and standard deviation of the sampled totals (std: sqrt of the diagonal below)
      'covariance' (G, G)  (1 / S) sum_s (x_sg - mean_g) (x_sh - mean_h) over the S = num_samples paths: the ensemble's own
                           moment, np.cov(totals.T, bias=True), bitwise symmetric
      'correlation' (G, G) covariance_gh / (std_g std_h), formed on the host; NaN in the row and column of a group whose
                           std is 0, 1 on the rest of the diagonal
    At most 4,096 groups, and num_samples * G <= 2^28.  weights: member weights of the sample paths as in
    `predict_samples`; None: equal weights."""
    return self._dependence_summaries('predict_dependence', table, group_by, num_samples, seed, weights)[0]

  def score_dependence(self, table, group_by, p=0.5, pair_weights=None, matrices=True, num_samples=1000, seed=0,
                       weights=None):
    """The co-movement of the group totals scored against the totals observed in `table[target_col]`, on the GPU: the
    variogram score of order p (Scheuerer & Hamill 2015), the companion of `score_totals(...)['energy_score']`, which is
    nearly blind to a wrong correlation structure.  p is 0.5, 1 or 2.  -> the dict of `predict_dependence` ('std',
    'covariance', 'correlation' with matrices=True only) plus
      'observed' (G,)             sum of the target over the group's rows; NaN when any row of the group has a NaN target:
                                  such a group is in no scored pair
      'variogram' (G, G)          matrices=True: (1 / S) sum_s |x_sg - x_sh|^p over the sample paths
      'observed_variogram' (G, G) matrices=True: |observed_g - observed_h|^p; NaN where not scored
      'variogram_score'           sum over the pairs g < h of scored groups of w_gh (observed_variogram_gh - variogram_gh)^2;
                                  w_gh = 1, or pair_weights (G, G), finite, >= 0 and symmetric (e.g. decaying with the
                                  distance between two places); lower is better
      'n', 'n_pairs'              groups scored and n (n - 1) / 2
      'mean_variogram_score'      'variogram_score' / the sum of the weights of the scored pairs; NaN for n_pairs = 0
    matrices=False returns the score alone and lifts the cap of 4,096 groups (pair_weights keep it);
    num_samples * G <= 2^28 either way.  The target checks are those of `score_totals`.  weights: member weights of the
    sample paths as in `predict_samples`; None: equal weights."""
    res, out, observed = self._dependence_summaries(
        'score_dependence', table, group_by, num_samples, seed, weights, target=True, p=p, pair_weights=pair_weights,
        matrices=matrices)
    scored = ~np.isnan(observed)
    n = int(scored.sum())
    res.update(observed=observed, variogram_score=out['variogram_score'], n=n, n_pairs=n * (n - 1) // 2)
    if 'variogram' in out:
      d = np.abs(observed[:, None] - observed[None, :])
      res.update(variogram=out['variogram'],
                 observed_variogram=np.sqrt(d) if float(p) == 0.5 else d if float(p) == 1.0 else d * d)
    if pair_weights is None:
      total = float(res['n_pairs'])
    else:
      w = np.asarray(pair_weights, dtype=np.float64)[np.ix_(scored, scored)]
      total = float(np.sum(np.triu(w, 1), dtype=np.float64))
    res['mean_variogram_score'] = res['variogram_score'] / total if res['n_pairs'] > 0 and total > 0 else float('nan')
    return res

  def _scenario_summaries(self, what, table, group_by, k, norm, scale, num_samples, seed, weights, target=False):
    f = self._paths(what, table, group_by, num_samples, seed, weights, target=target)
    cap = inference._native.SCENARIO_MAX_SAMPLES
    if int(num_samples) > cap:
      raise ValueError(f'{what}: num_samples={num_samples}: the scenarios are chosen among at most {cap} sample paths')
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= int(num_samples):
      raise ValueError(f'{what}: k={k!r}: an integer in 1..{int(num_samples)}, the number of sample paths')
    if isinstance(norm, bool) or norm not in inference.SCENARIO_NORMS:
      raise ValueError(f'{what}: norm={norm!r}: the distance between two paths is formed for norm in '
                       f'{inference.SCENARIO_NORMS}')
    n_groups = len(f.keys)
    if scale is not None:
      try:
        scale = np.ascontiguousarray(scale, dtype=np.float64)
      except (TypeError, ValueError) as e:
        raise ValueError(f'{what}: scale must be one positive finite number per group ({n_groups},)') from e
      if scale.shape != (n_groups,):
        raise ValueError(f'{what}: scale must hold one divisor per group ({n_groups},); got {scale.shape}')
      if not (np.all(np.isfinite(scale)) and np.all(scale > 0)):
        raise ValueError(f'{what}: scale must be finite and > 0')
    observed = None if f.y is None else group_target_sums(f.y, f.seg_offsets, f.seg_rows)
    if observed is not None and not np.isfinite(observed).any():
      raise ValueError(f'{what}: no group has an observed total: every group holds a NaN target')
    out = f.run(inference.scenario_summaries, k=int(k), norm=int(norm), scale=scale, observed=observed)
    res = {'keys': f.keys, 'scenarios': out['scenarios'], 'probability': out['probability'], 'path': out['path'],
           'distance': out['distance'], 'assignment': out['assignment']}
    return res, out, observed

  def predict_scenarios(self, table, group_by, k=10, norm=2, scale=None, num_samples=1000, seed=0, weights=None):
    """The joint sample paths of `predict_samples(table, num_samples, seed, group_by=group_by)` reduced to k representative
    scenarios, each with a probability -- "three futures" for a staffing plan, a stochastic programme or a stress test --
    on the GPU: the (num_samples, G) matrix of totals never leaves the device.  Every scenario is an actual path of the
    forecast, so every group of it stays coherent with the others.  The method is fast forward selection (Heitsch &
    Roemisch 2003): greedily the paths that minimise the Kantorovich (Wasserstein-1) distance between the ensemble and the
    scenario set, every other path handing its probability to its nearest scenario (the earliest chosen among equally
    near).  The distance between two paths is the `norm`-norm (1 or 2) of the difference of their totals.  -> dict:
      'keys'                       the groups, as in `predict_samples`
      'scenarios' (k, G)           the totals of the chosen paths, in the order chosen (the first is the ensemble's medoid)
      'probability' (k,)           the share of the sample paths each scenario stands for; sums to 1
      'path' (k,) int              the index of each scenario among the sample paths: `predict_samples(table, num_samples,
                                   seed, group_by=group_by, weights=weights)[0][path]` is 'scenarios', and without group_by
                                   it gives the scenarios row by row
      'distance' (k,)              the Kantorovich distance between the ensemble and the first 1 .. k scenarios,
                                   nonincreasing: how much the ensemble loses, and so where to stop
      'assignment' (num_samples,)  the scenario of every sample path
    scale: None, or one positive finite number per group that divides the group's total before the distance is formed,
    e.g. `predict_dependence(...)['std']` or a population, so that no large group decides alone.  Paths that repeat
    (totals of counts do) have distance 0: once every distinct path is chosen the rest are taken in index order with
    probability 0.  1 <= k <= num_samples <= 4,096.  Out of scope: scenarios of single rows over more than 4,096 paths,
    scenarios of `combinations=`, backward reduction, and a k-medoids refinement of the greedy set.
    weights: member weights of the sample paths as in `predict_samples`; None: equal weights."""
    return self._scenario_summaries('predict_scenarios', table, group_by, k, norm, scale, num_samples, seed, weights)[0]

  def score_scenarios(self, table, group_by, k=10, norm=2, scale=None, num_samples=1000, seed=0, weights=None):
    """`predict_scenarios` held against the totals observed in `table[target_col]`: how near the scenario set comes to what
    happened, on the GPU.  A group with a NaN target among its rows has no observed total and is left out of EVERY
    distance, between paths as well, so that the observed vector and the paths are measured alike; at least one group must
    have one.  -> the dict of `predict_scenarios` ('scenarios' holds all groups) plus
      'observed' (G,)          sum of the target over the group's rows; NaN when any row of the group has a NaN target
      'n'                      groups with an observed total
      'nearest'                the scenario (0 .. k - 1) nearest to the observed vector
      'nearest_distance'       its distance to the observed vector
      'pit' (2,)               the shares of the sample paths whose distance to their own scenario is <= and <
                               'nearest_distance': near 1, the observed lies farther from every scenario than nearly every
                               path of the forecast does
    The target checks are those of `score_totals`; the limits, `scale`, what is out of scope and `weights` those of
    `predict_scenarios`."""
    res, out, observed = self._scenario_summaries('score_scenarios', table, group_by, k, norm, scale, num_samples, seed,
                                                  weights, target=True)
    res.update(observed=observed, n=int(np.isfinite(observed).sum()), nearest=out['nearest'],
               nearest_distance=out['nearest_distance'], pit=out['pit'])
    return res

  @staticmethod
  def _per_group(what, table, per, seg_offsets, seg_rows):
    """The divisor of every group from `per`: None, a column of `table` or one value per table row; constant within every
    group, finite and > 0 -> (G,) float64 or None."""
    if per is None:
      return None
    if isinstance(per, str):
      if per not in table.columns:
        raise ValueError(f'{what}: per: {per!r} is not among the columns of the table')
      per = table[per].values
    try:
      v = np.asarray(per, dtype=np.float64)
    except (TypeError, ValueError) as e:
      raise ValueError(f'{what}: per must be a column of the table or one number per row') from e
    if v.shape != (len(table),):
      raise ValueError(f'{what}: per must hold one value per row ({len(table)},); got {v.shape}')
    if not (np.all(np.isfinite(v)) and np.all(v > 0)):
      raise ValueError(f'{what}: per must be finite and > 0')
    ordered = v[np.asarray(seg_rows, dtype=np.int64)]
    starts = np.asarray(seg_offsets[:-1], dtype=np.int64)
    lo, hi = np.minimum.reduceat(ordered, starts), np.maximum.reduceat(ordered, starts)
    if np.any(lo != hi):
      raise ValueError(f'{what}: per must be constant within every group')
    return lo

  def _ranking_summaries(self, what, table, group_by, top_k, per, quantiles, num_samples, seed, weights, target=False):
    f = self._paths(what, table, group_by, num_samples, seed, weights, noun='ranks', target=target)
    scale = self._per_group(what, table, per, f.seg_offsets, f.seg_rows)
    observed = None if f.y is None else group_target_sums(f.y, f.seg_offsets, f.seg_rows)
    out = f.run(inference.ranking_summaries, observed=observed, scale=scale, top_k=top_k, quantiles=tuple(quantiles))
    return out, f.keys, observed

  @staticmethod
  def _ranking_result(keys, mean, quant, prob):
    lead = prob[0]
    best = None if np.all(np.isnan(lead)) else keys[int(np.nanargmax(lead))]
    return {'keys': keys, 'rank_mean': mean, 'rank_quantiles': quant, 'rank_probability': prob,
            'top_probability': np.cumsum(prob, axis=0), 'most_likely_top': best}

  def predict_ranking(self, table, group_by, top_k=3, per=None, quantiles=(0.5,), num_samples=1000, seed=0, weights=None):
    """How the groups rank against each other by their totals in `predict_samples(table, num_samples, seed,
    group_by=group_by)` -- "which places are among the three worst hit" -- formed on the GPU: every path is ranked on the
    device and the (num_samples, G) matrix of totals never leaves it.  One member drives all rows of a path, so the totals
    rise and fall together: the rank of a group is a property of the whole vector and of no marginal.  Rank 1 is the
    largest total; groups whose totals tie in a path share their block of ranks equally (totals of counts tie often; they
    are never told apart by their position).  -> dict:
      'keys'                       the groups, as in `predict_samples`
      'rank_mean' (G,)             'rank_quantiles' (len(quantiles), G)   of the mid-rank over the paths
      'rank_probability' (top_k, G)   P(the group takes rank k), k = 1 .. top_k; every row sums to 1
      'top_probability' (top_k, G) its running sum over k: P(the group is among the k largest), ties sharing
      'most_likely_top'            the key of the group with the largest rank_probability[0]
    per: None, or a column of `table` (or one value per row) that is constant within every group, finite and > 0, such as
    a population: the groups are then ranked by total / per.  At most 16,384 groups, num_samples <= 16,384,
    num_samples * G <= 2^28, 1 <= top_k <= G and top_k * G <= 2^24.  weights: member weights of the sample paths as in
    `predict_samples`; None: equal weights."""
    out, keys, _ = self._ranking_summaries('predict_ranking', table, group_by, top_k, per, quantiles, num_samples, seed,
                                           weights)
    return self._ranking_result(keys, out['rank_mean'], out['rank_quantiles'], out['rank_probability'])

  def score_ranking(self, table, group_by, top_k=3, per=None, quantiles=(0.025, 0.5, 0.975), num_samples=1000, seed=0,
                    weights=None):
    """The forecast ranking of the groups scored against the ranking of the totals observed in `table[target_col]`, on
    the GPU.  A group with a NaN target among its rows is not scored, and the scored forecast is the ranking AMONG THE
    SCORED GROUPS (they are ranked again without the others, so that forecast and observed ranks mean the same thing).
    -> the dict of `predict_ranking` among the scored groups, NaN in the columns of the others (rows k > n of
    'rank_probability' are 0: no such rank is taken), plus
      'observed' (G,)          sum of the target over the group's rows; NaN when any row of the group has a NaN target
      'observed_rank' (G,)     the mid-rank of the observed total (divided by `per`) among the scored groups
      'rank_crps' (G,)  'rank_pit' (2, G)   ensemble CRPS and PIT of the mid-rank over the paths against the observed one
      'observed_top' (top_k, G)   the share of the group in the observed top k: clip((k - above) / ties, 0, 1) of the
                               observed ranks -- 1 or 0 without ties
      'top_brier' (top_k,)     mean over the scored groups of (top_probability - observed_top)^2
      'observed_rank_probability' (G,)   the forecast probability of the observed rank block: the sum of 'rank_probability'
                               over the ranks above + 1 .. above + ties that are <= top_k; NaN when the block lies wholly
                               beyond top_k
      'n'                      groups scored          'mean_rank_crps'  mean of 'rank_crps' over them
    The target checks are those of `score_totals`; the limits and `per`, `weights` those of `predict_ranking`."""
    out, keys, observed = self._ranking_summaries('score_ranking', table, group_by, top_k, per, quantiles, num_samples,
                                                  seed, weights, target=True)
    prob = out['scored_rank_probability']
    res = self._ranking_result(keys, out['scored_rank_mean'], out['scored_rank_quantiles'], prob)
    scored = ~np.isnan(observed)
    n = int(scored.sum())
    above, ties = out['observed_above'].astype(np.float64), out['observed_ties'].astype(np.float64)
    k = np.arange(1, prob.shape[0] + 1, dtype=np.float64)[:, None]
    observed_top = np.where(scored[None, :], np.clip((k - above[None, :]) / np.where(scored, ties, 1.0)[None, :], 0.0, 1.0),
                            np.nan)
    in_block = (k > above[None, :]) & (k <= (above + ties)[None, :])
    block = np.sum(np.where(in_block, prob, 0.0), axis=0)
    block[~scored | (above + 1 > prob.shape[0])] = np.nan
    err = (res['top_probability'] - observed_top) ** 2
    res.update(observed=observed, observed_rank=out['observed_rank'], rank_crps=out['rank_crps'], rank_pit=out['rank_pit'],
               observed_top=observed_top,
               top_brier=np.mean(err[:, scored], axis=1, dtype=np.float64) if n else np.full(prob.shape[0], np.nan),
               observed_rank_probability=block, n=n,
               mean_rank_crps=float(np.mean(out['rank_crps'][scored], dtype=np.float64)) if n else float('nan'))
    return res

  def likelihood_model(self, table):
    """Predictive distribution of every member at the rows of `table`
    (reference :433-468 returns a TFP Independent(Normal/NB/ZINB))."""
    rows = self.data_handler.get_test(table)
    return inference.likelihood_model(
        rows, self.observation_model, self.params_,
        self._model_args(rows.shape), ensemble_dims=self._ensemble_dims,
        compute_dtype=self.compute_dtype)


class BayesianNeuralFieldMAP(BayesianNeuralFieldEstimator):
  """Ensemble of maximum-a-posteriori fits (Adam on -log posterior)."""

  _ensemble_dims = 2

  validation_ = None

  def fit(self, table, seed, ensemble_size=16, learning_rate=0.005,
          num_epochs=5_000, batch_size=None, num_splits=1, validation=None, validation_every=None, restore_best=True):
    """Train `ensemble_size` independent members; members are sharded over the
    GPUs (ranks) of the job.  `batch_size=None` is full batch; otherwise each
    epoch does len(table)//batch_size Adam steps on a per-member shuffle.
    `num_splits` trains the ensemble in that many sequential chunks.

    validation: a table of held-out rows that holds the target column, scored on the GPU while the fit runs (the target
    checks are those of `score`: NaN targets are left out, infinite or -- count models -- non-integer targets, a missing
    target column and a table without a finite target are a ValueError before any GPU work).  Every member's mean
    held-out log density is recorded after the epochs validation_every, 2 validation_every, ... and after the last one;
    validation_every counts the epochs `fit` actually runs (the columns of `losses_`) and defaults to
    ceil(num_epochs / 50).  The decision and the snapshots stay on the device: the fit waits for nothing.  Afterwards
    `validation_` is a dict (None after a fit without validation):
      'epochs' (K,) int                 the epochs of the checks
      'member_log_density'              lead dims of losses_[..., 0] + (K,) float64: mean held-out log density per
                                        member and check
      'best', 'best_epoch'              lead dims: each member's largest value (the first of equal ones; a NaN never
                                        beats a number) and the epoch of that check
      'n' rows scored                   'restored' what restore_best was
    restore_best=True leaves every member in `params_` at its OWN best epoch, False at the last epoch; `losses_` is the
    same either way.  Out of scope: `BayesianNeuralFieldVI.fit` (its held-out score is a mixture over posterior draws and
    would need draws at every check); early stopping (a host sync per check and one decision across the shards); the
    curve of the ensemble mixture (all shards' rows on one device at every check)."""
    held = None
    if validation is not None:
      y_val = self._targets('fit: validation', validation)
      if not np.isfinite(y_val).any():
        raise ValueError('fit: validation: no row with a finite target')
    if validation_every is not None:
      if (isinstance(validation_every, bool) or not isinstance(validation_every, numbers.Integral)
          or validation_every < 1):
        raise ValueError(f'fit: validation_every must be an integer >= 1; got {validation_every!r}')
    if ensemble_size < distributed.device_count():
      raise ValueError('ensemble_size cannot be smaller than device_count. '
                       'https://github.com/google/bayesnf/issues/28.')
    x = self.data_handler.get_train(table)
    y = self.data_handler.get_target(table)
    if batch_size is None:
      batch_size = x.shape[0]
    if self._scale_epochs_by_batch_size:
      num_epochs = num_epochs * (x.shape[0] // batch_size)
    if validation is not None:
      every = max(1, -(-num_epochs // 50)) if validation_every is None else int(validation_every)
      held = (self.data_handler.get_test(validation), y_val, every, bool(restore_best))
    # (without validation fit_map is called exactly as before, and returns its two values)
    fitted = inference.fit_map(
        x, y,
        seed=seed,
        observation_model=self.observation_model,
        model_args=self._model_args((batch_size, x.shape[-1])),
        num_particles=ensemble_size,
        learning_rate=learning_rate,
        num_epochs=num_epochs,
        prior_weight=self._prior_weight,
        batch_size=batch_size,
        num_splits=num_splits,
        compute_dtype=self.compute_dtype,
        init_rng=self.init_rng,
        **({} if held is None else {'validation': held}))
    self.params_, self.losses_ = fitted[0], fitted[1]
    self.validation_ = None if held is None else fitted[2]
    return self


class BayesianNeuralFieldMLE(BayesianNeuralFieldMAP):
  """Ensemble of maximum-likelihood fits: MAP without the prior term."""

  _prior_weight = 0.0


class BayesianNeuralFieldVI(BayesianNeuralFieldEstimator):
  """Ensemble of mean-field Gaussian surrogate posteriors (reparameterised
  ELBO with the KL term weighted by `kl_weight`)."""

  _ensemble_dims = 3
  _scale_epochs_by_batch_size = True

  def fit(self, table, seed, ensemble_size=16, learning_rate=0.01,
          num_epochs=1_000, sample_size_posterior=30, sample_size_divergence=5,
          kl_weight=0.1, batch_size=None):
    """`num_epochs` is multiplied by len(table)//batch_size to get the number
    of optimisation steps; each step uses one random batch.  After fitting,
    `sample_size_posterior` parameter draws per member are kept as `params_`."""
    x = self.data_handler.get_train(table)
    y = self.data_handler.get_target(table)
    if batch_size is None:
      batch_size = x.shape[0]
    if self._scale_epochs_by_batch_size:
      num_epochs = num_epochs * (x.shape[0] // batch_size)
    _, self.losses_, self.params_ = inference.fit_vi(
        x, y,
        seed=seed,
        observation_model=self.observation_model,
        model_args=self._model_args((batch_size, x.shape[-1])),
        ensemble_size=ensemble_size,
        learning_rate=learning_rate,
        num_epochs=num_epochs,
        sample_size_posterior=sample_size_posterior,
        sample_size_divergence=sample_size_divergence,
        kl_weight=kl_weight,
        batch_size=batch_size,
        compute_dtype=self.compute_dtype,
        init_rng=self.init_rng)
    return self
