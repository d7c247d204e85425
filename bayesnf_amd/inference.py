"""Engine seam: same three entry points as the reference's inference module.

  fit_map      /root/reference/src/bayesnf/inference.py:376-458
  fit_vi       /root/reference/src/bayesnf/inference.py:336-373
  predict_bnf  /root/reference/src/bayesnf/inference.py:461-507

with identical argument names / meaning / return structure, so the estimator
layer (spatiotemporal.py) reads like the reference's.  Underneath, every member
lives on one GPU (`engine.Engine` -> libbnf_hip.so); ranks hold disjoint member
shards and the fitted parameters / predictive means are gathered once at the end (the
reference's implicit pmap output gather, inference.py:452,486-492).  Which devices a
process drives -- every visible GPU from one process like the reference's pmap, or one
per torchrun rank -- is `distributed.local_shards()`.
"""

from __future__ import annotations

import contextlib
import math
import numbers
import os
import warnings
from typing import Any

import numpy as np
import pandas as pd
import torch

from . import _native
from . import distributed
from . import jaxseed
from .engine import Engine
from .spec import NetSpec


def _net_from_args(model_args: dict[str, Any], observation_model: str) -> NetSpec:
  args = dict(model_args)
  args.pop('likelihood_distribution', None)
  return NetSpec(observation_model=observation_model, **args)


def _struct_tuple(net: NetSpec, theta: np.ndarray):
  """(..., P) -> StructTuple(var0, var1, ...) of (..., *leaf_shape) arrays."""
  return net.struct_tuple_type()(*net.unpack(theta))


def _flatten_struct(net: NetSpec, params) -> np.ndarray:
  """StructTuple with arbitrary leading dims -> (..., P) float32."""
  return net.pack(list(params), dtype=np.float32)


# ---------------------------------------------------------------------------
# MAP / MLE
# ---------------------------------------------------------------------------
def validation_epochs(num_epochs, every):
  """The epochs after which a validated fit checks the held-out rows: every, 2 every, ... and always the last one."""
  return sorted(set(range(every, num_epochs + 1, every)) | {num_epochs})


class _HeldOut:
  """One shard's held-out checks during `fit_map` (include/bnf.h bnf_validation_check).  Owns a forward-only engine on
  the training engine's device and stream -- the training handle itself cannot serve: `bnf_forward` refuses row-panel
  handles, and on a layer pipeline its weight packing would overwrite the packed weights of the training step -- the
  device copies of the held-out rows, and the buffers of the checks: the curve, every member's best score and epoch and
  the snapshot of its parameters at that epoch.  The forward reads theta straight from the training engine's `params`
  tensor (no copy); everything is enqueued, nothing is waited for."""

  def __init__(self, net, eng, features_val, target_val, epochs, compute_dtype, device_index):
    self.eng, self.epochs, self.done = eng, list(epochs), 0
    E, n_val = eng.members, features_val.shape[0]
    # capacity: the rule of _forward_local
    cells = max(1, (1 << 28) // max(1, net.width))
    row_cap = int(min(n_val, _ROW_CHUNK))
    mem_cap = int(max(1, min(E, cells // row_cap)))
    self.fwd = Engine(net, mode='map', members=mem_cap, forward_only=True, row_capacity=row_cap,
                      compute_dtype=compute_dtype, device_index=device_index)
    dev = eng.device
    self.X = torch.from_numpy(np.ascontiguousarray(features_val, dtype=np.float32)).to(dev)
    self.y = torch.from_numpy(np.ascontiguousarray(target_val, dtype=np.float32)).to(dev)
    self.n = int(np.isfinite(target_val).sum())
    self.theta = eng.params.view(E, net.P)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    self.curve, self.best_score, self.ll = f64(E, len(self.epochs)), f64(E), f64(E)
    self.work = f64(max(1, E * (-(-n_val // _native.SCORE_ROW_TILE))))
    self.best_epoch = torch.empty((E,), dtype=torch.int64, device=dev)
    self.keep = torch.empty((E,), dtype=torch.int32, device=dev)
    self.best_params = torch.empty((E, net.P), dtype=torch.float32, device=dev)

  def check(self, epoch):
    loc, aux = self.fwd.forward(self.theta, self.X)
    self.fwd.predictive_scores(loc, aux, self.y, crps=False, member_ll=True, lpd=False, pit=False,
                               into={'member_ll': self.ll, 'work': self.work})
    self.eng.validation_check(self.ll, self.n, epoch, self.done, len(self.epochs), self.curve, self.best_score,
                              self.best_epoch, self.keep, self.best_params)
    self.done += 1

  def train(self, e0, n):
    """The epochs [e0, e0 + n) in segments cut at the check epochs, each check right after its epoch -> loss pieces."""
    parts, stop = [], e0 + n
    while e0 < stop:
      nxt = self.epochs[self.done] if self.done < len(self.epochs) else stop
      e1 = min(stop, nxt)
      parts.append(self.eng.train(e0, e1 - e0))
      if e1 == nxt:
        self.check(e1)
      e0 = e1
    return parts

  def close(self):
    self.fwd.close()


def fit_map(features, target, seed, observation_model, model_args, num_particles,
            learning_rate, num_epochs, prior_weight=1.0, batch_size=None,
            num_splits=1, compute_dtype=None, init_rng=None, validation=None):
  """Fit `num_particles` MAP (or MLE, prior_weight=0) members.

  init_rng: 'jax' (default; env BNF_INIT_RNG) starts every member from the initial parameters the
  reference itself would draw for `seed` (threefry + TFP seed chain restated on the host,
  `jaxseed`) and, for minibatch fits, shuffles every epoch with the reference's own per-member
  `jax.random.permutation` stream (`jaxseed.map_shuffle_subkeys` -> `bnf_row_keys`: drawn on the device): same seed => the same
  initial particles and shuffles as the reference (pinned by its goldens for full-batch fits; the shuffle chain rests on
  the reference's source + the pinned split / bits restatements -- no golden exercises a minibatch fit, and no end-to-end
  known-answer vector of `jax.random.permutation` is held: DESIGN.md section 5).  'philox' draws the initial parameters from the device generator
  (`bnf_init_params`) and shuffles with the device's keyed Feistel permutation (no index arrays).

  Returns (params, losses): params is a StructTuple whose leaves have shape
  (num_devices, num_particles // num_devices, *leaf_shape); losses has shape
  (num_devices, num_particles // num_devices, num_epochs).

  validation = (features_val, target_val, every, restore_best): held-out rows (NaN targets allowed: left out) scored
  after the epochs `validation_epochs(num_epochs, every)` -- training runs in segments between the checks, every shard
  validates its own members on its own device with a forward-only engine, nothing is waited for (`_HeldOut`, include/bnf.h
  bnf_validation_check) -- and a third value is returned, a dict:
    'epochs' (K,) int                    'member_log_density' lead dims of losses[..., 0] + (K,) float64: every member's
    'best', 'best_epoch' lead dims       mean held-out log density at each check; its maximum (first occurrence; a NaN
    'n' rows scored  'restored' bool     never beats a number) and the epoch of that check
  With restore_best the returned params are every member's own at its 'best_epoch', else the final ones; losses are the
  same either way.  None: the Engine calls, and the two return values, of a fit without validation.
  """
  net = _net_from_args(model_args, observation_model)
  features = np.asarray(features, dtype=np.float64)
  target = np.asarray(target, dtype=np.float64)
  n_rows = target.shape[0]
  checks = None
  if validation is not None:
    features_val, target_val, every, restore_best = validation
    features_val = np.asarray(features_val, dtype=np.float64)
    target_val = np.asarray(target_val, dtype=np.float64)
    every = int(every)
    if features_val.ndim != 2 or features_val.shape[1] != features.shape[1] or target_val.shape != (features_val.shape[0],):
      raise ValueError(f'validation: features ({features_val.shape}) need the columns of the training features and one '
                       f'target per row; got targets {target_val.shape}')
    if not np.isfinite(target_val).any():
      raise ValueError('validation: no row with a finite target')
    if every < 1 or num_epochs < 1:
      raise ValueError(f'validation: every={every} and num_epochs={num_epochs} must be >= 1')
    checks = validation_epochs(num_epochs, every)
  if batch_size is None:
    batch_size = n_rows
  world = distributed.device_count()
  seed64 = _native.seed_to_u64(seed)
  per_device = (num_particles // num_splits) // world
  if per_device < 1:
    raise ValueError('fewer than one particle per device and split')
  log_noise_init = float(np.log(np.nanstd(target) / 2.0))
  init_rng = init_rng or os.environ.get('BNF_INIT_RNG', 'jax')
  if init_rng not in ('jax', 'philox'):
    raise ValueError("init_rng must be 'jax' or 'philox'")
  thetas, losses, curves, bests, best_epochs = [], [], [], [], []
  for i in range(num_splits):
    seed_i = _native.fold_in(seed64, i) if num_splits > 1 else seed64
    keys = (jaxseed.member_keys(seed, world, per_device, i if num_splits > 1 else None)
            if init_rng == 'jax' else None)

    # minibatch epochs under init_rng='jax': every member's per-epoch `jax.random.permutation` of the
    # reference (inference.py:593-597), keys on the host once per fit
    want_ref_shuffles = init_rng == 'jax' and batch_size < n_rows and num_epochs > 0
    if (want_ref_shuffles and per_device * n_rows >= 2**31
        and os.environ.get('BNF_ROW_TABLES', 'device') != 'host'):
      # the device-side sort addresses (member, row) pairs with 32-bit offsets (include/bnf.h bnf_row_keys)
      warnings.warn(f'{per_device} members x {n_rows} rows per device exceed 2^31 - 1: the epoch shuffles of this fit come '
                    "from the engine's index-free generator (same law as jax.random.permutation, other numbers); "
                    'BNF_ROW_TABLES=host keeps the reference stream at the price of host-drawn tables.')
      want_ref_shuffles = False
    pkeys = (jaxseed.map_permute_keys(seed, world, per_device, num_epochs, i if num_splits > 1 else None)
             if want_ref_shuffles else None)

    def train_shard(sh):
      # device sh.index of the job owns the members [index * per_device, (index + 1) * per_device): the
      # whole optimisation is enqueued on that device's stream; nothing is waited for here
      eng = Engine(net, mode='map', X=features, y=target, batch=batch_size,
                   members=per_device, member_offset=sh.index * per_device, seed=seed_i,
                   learning_rate=learning_rate, prior_weight=prior_weight,
                   compute_dtype=compute_dtype, device_index=sh.device)
      if keys is not None:
        # the reference's own initial particles for this seed: key chain on the host, values drawn on the device
        eng.init_params_keys(jaxseed.map_leaf_keys(net, keys[sh.index]), log_noise_init)
      else:
        eng.init_params(log_noise_init)
      # held-out checks: the epochs run in segments cut at the check epochs, each check enqueued right after its epoch
      held = (None if checks is None else
              _HeldOut(net, eng, features_val, target_val, checks, compute_dtype, sh.device))
      train = (lambda e0, n: [eng.train(e0, n)]) if held is None else held.train
      joined = lambda parts: parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)
      if pkeys is None:
        return eng, joined(train(0, num_epochs)), held
      # the shuffles are drawn on the device, epoch by epoch, from the sub keys of their sort rounds
      # (BNF_ROW_TABLES=host: drawn here instead -- threefry bits + stable sort per member and epoch -- and uploaded
      # in chunks of <= ~64 MB of row ids, chunk c + 1 while the device runs the epochs of chunk c)
      if os.environ.get('BNF_ROW_TABLES', 'device') != 'host':
        eng.set_row_keys(jaxseed.map_shuffle_subkeys(pkeys[sh.index], n_rows), epoch0=0)
        return eng, joined(train(0, num_epochs)), held
      keep = (n_rows // batch_size) * batch_size
      per_chunk = int(max(1, min(num_epochs, (64 << 20) // max(1, 4 * per_device * keep))))
      parts = []
      for e0 in range(0, num_epochs, per_chunk):
        n = min(per_chunk, num_epochs - e0)
        eng.set_row_tables(jaxseed.map_row_tables(pkeys[sh.index][:, e0:e0 + n], n_rows, batch_size), epoch0=e0)
        parts.extend(train(e0, n))
      return eng, torch.cat(parts, dim=1), held

    runs = distributed.run_shards(train_shard)
    gathered = lambda parts: distributed.gather_shards(parts).cpu().numpy()
    if checks is not None and restore_best:
      thetas.append(gathered([h.best_params for _, _, h in runs]))
    else:
      thetas.append(gathered([e.params.view(per_device, net.P) for e, _, _ in runs]))
    losses.append(gathered([l for _, l, _ in runs]))
    if checks is not None:
      curves.append(gathered([h.curve for _, _, h in runs]))
      bests.append(gathered([h.best_score for _, _, h in runs]))
      best_epochs.append(gathered([h.best_epoch for _, _, h in runs]))
    for e, _, h in runs:
      if h is not None:
        h.close()
      e.close()
  theta = np.concatenate(thetas, axis=1)          # (world, E/world, P)
  if checks is None:
    return _struct_tuple(net, theta), np.concatenate(losses, axis=1)
  info = {'epochs': np.asarray(checks, dtype=np.int64), 'member_log_density': np.concatenate(curves, axis=1),
          'best': np.concatenate(bests, axis=1), 'best_epoch': np.concatenate(best_epochs, axis=1),
          'n': int(np.isfinite(target_val).sum()), 'restored': bool(restore_best)}
  return _struct_tuple(net, theta), np.concatenate(losses, axis=1), info


# ---------------------------------------------------------------------------
# VI
# ---------------------------------------------------------------------------
class MeanFieldSurrogate:
  """What `ensemble_vi` returns first (a JointDistribution of Normals in the
  reference, inference.py:760-764): per-coordinate mean and scale."""

  def __init__(self, net: NetSpec, mu: np.ndarray, rho: np.ndarray):
    self.net = net
    self.loc = _struct_tuple(net, mu)
    self.scale = _struct_tuple(net, 1e-4 + np.logaddexp(rho, 0.0))
    self._mu, self._rho = mu, rho

  def mean(self):
    return self.loc

  def stddev(self):
    return self.scale


def fit_vi(features, target, seed, observation_model, model_args, ensemble_size,
           learning_rate, num_epochs, sample_size_divergence,
           sample_size_posterior, kl_weight, batch_size=None, compute_dtype=None, init_rng=None):
  """Fit mean-field surrogates.  Returns (surrogate, losses, predictions):
  losses (num_devices, E/num_devices, num_epochs) already multiplied by
  kl_weight; predictions = StructTuple of posterior draws with leaves
  (num_devices, sample_size_posterior, E/num_devices, *leaf_shape).

  init_rng='jax' (default): initial surrogate means, optimisation noise and posterior draws are the reference's own for
  `seed` (pinned by its VI golden: 2 full-batch steps; longer fits extrapolate the same key recurrence).  With `batch_size`
  the one row permutation every step shares between the device's members is the reference's too as far as its source shows
  it (inference.py:704-709) -- UNPINNED by any golden and resting on one stated assumption about tfp
  (jaxseed.vi_batch_subkeys); 'philox': the device generator throughout (same law, other numbers)."""
  net = _net_from_args(model_args, observation_model)
  init_rng = init_rng or os.environ.get('BNF_INIT_RNG', 'jax')
  if init_rng not in ('jax', 'philox'):
    raise ValueError("init_rng must be 'jax' or 'philox'")
  features = np.asarray(features, dtype=np.float64)
  target = np.asarray(target, dtype=np.float64)
  n_rows = target.shape[0]
  if batch_size is not None and n_rows < batch_size:
    raise AssertionError(f'batch_size={batch_size} exceeds target.shape[0]={n_rows}')
  world = distributed.device_count()
  per_device = ensemble_size // world
  if per_device < 1:
    raise ValueError('fewer than one surrogate per device')
  full_batch = batch_size is None or batch_size >= n_rows
  mu_keys = jaxseed.vi_mean_leaf_keys(net, seed, world, per_device) if init_rng == 'jax' else None

  def train_shard(sh):
    eng = Engine(net, mode='vi', X=features, y=target,
                 batch=n_rows if batch_size is None else batch_size,
                 members=per_device, member_offset=sh.index * per_device,
                 seed=_native.seed_to_u64(seed), learning_rate=learning_rate,
                 kl_weight=kl_weight, vi_samples=sample_size_divergence,
                 compute_dtype=compute_dtype, device_index=sh.device)
    if mu_keys is None:
      eng.init_params(0.0)
    else:
      # the reference's own initial surrogate means for this seed (key chain on the host, values on the device)
      eng.init_params_keys(mu_keys[sh.index], 0.0)
      # the optimisation noise and the posterior draws come from the reference's stream too (keys on the host once per
      # fit, normals on the device), so the fit runs on the reference's numbers (pinned by the reference's VI golden:
      # 2 full-batch optimisation steps; longer fits extrapolate the same key recurrence) ...
      eng.set_vi_noise_keys(jaxseed.vi_noise_keys(net, seed, world, sh.index, num_epochs, sample_size_divergence),
                            jaxseed.vi_draw_keys(net, seed, world, sh.index, sample_size_posterior),
                            jaxseed.leaf_offsets(net))
      if not full_batch:
        # ... and so does the ONE minibatch every step shares between the device's members: permutation(seed_step, N)[:B]
        # (inference.py:704-709), sort-round keys from the host, bits and sorts on the device.  Unpinned by any golden
        # (jaxseed.vi_batch_subkeys states the one assumption it rests on).
        eng.set_row_keys(jaxseed.vi_batch_subkeys(seed, world, sh.index, num_epochs, n_rows))
    loss_dev = eng.train(0, num_epochs)
    return eng, loss_dev, eng.vi_posterior_draws(sample_size_posterior)   # draws (n, E_local, P)

  runs = distributed.run_shards(train_shard)
  mu = distributed.gather_shards([e.params.view(2, per_device, net.P)[0] for e, _, _ in runs]).cpu().numpy()
  rho = distributed.gather_shards([e.params.view(2, per_device, net.P)[1] for e, _, _ in runs]).cpu().numpy()
  losses = distributed.gather_shards([l for _, l, _ in runs]).cpu().numpy()
  preds = distributed.gather_shards([d for _, _, d in runs]).cpu().numpy()   # (world, n, E/world, P)
  for e, _, _ in runs:
    e.close()
  return MeanFieldSurrogate(net, mu, rho), losses, _struct_tuple(net, preds)


# ---------------------------------------------------------------------------
# predict
# ---------------------------------------------------------------------------
_ROW_CHUNK = 8192


def _forward_local(net, theta_local, features, compute_dtype, device_index=None):
  """theta_local (M, P) numpy: members handled by one device -> loc (M, R), aux (M, 3)
  as device tensors, plus the engine (kept alive for the quantile kernels)."""
  n_rows = features.shape[0]
  M = theta_local.shape[0]
  # capacity: bound activation memory to ~2 GiB of (members x rows x width) cells
  cells = max(1, (1 << 28) // max(1, net.width))
  row_cap = int(min(n_rows, _ROW_CHUNK))
  mem_cap = int(max(1, min(M, cells // row_cap)))
  eng = Engine(net, mode='map', members=mem_cap, forward_only=True,
               row_capacity=row_cap, compute_dtype=compute_dtype, device_index=device_index)
  theta = torch.from_numpy(np.ascontiguousarray(theta_local, dtype=np.float32)).to(eng.device)
  X = torch.from_numpy(np.ascontiguousarray(
      np.asarray(features, dtype=np.float64), dtype=np.float32)).to(eng.device)
  loc, aux = eng.forward(theta, X)
  return eng, loc, aux


def _ensemble_forecast(features, observation_model, params, model_args,
                       ensemble_dims, compute_dtype):
  """Forward pass of every member on the new rows -> (net, engine, lead dims, loc (M, R), aux (M, 3))
  with all M members on the first local device.  The members are dealt out over the devices of the
  job in equal contiguous blocks whatever device count the parameters were fitted on (the leading
  dims of `params` only shape the result)."""
  net = _net_from_args(model_args, observation_model)
  theta_all = _flatten_struct(net, params)            # ([devices,] [S,] E/devices, P)
  lead = theta_all.shape[:-1]
  if len(lead) != ensemble_dims:
    raise ValueError(f'params have {len(lead)} ensemble dims, expected {ensemble_dims}')
  theta_flat = theta_all.reshape(-1, net.P)
  M = theta_flat.shape[0]
  world = distributed.device_count()
  per = -(-M // world)                                # ceil: the last block may be short

  def block(index):                                   # rows of theta_flat device `index` handles, padded to `per`
    lo = min(index * per, M - 1)
    idx = np.minimum(np.arange(lo, lo + per), M - 1)
    return theta_flat[idx]

  runs = distributed.run_shards(
      lambda sh: _forward_local(net, block(sh.index), features, compute_dtype, device_index=sh.device))
  loc_all = distributed.gather_shards([r[1] for r in runs])      # (world, per, R)
  aux_all = distributed.gather_shards([r[2] for r in runs])
  for r in runs[1:]:
    r[0].close()
  n_rows = features.shape[0]
  loc_all = loc_all.reshape(-1, n_rows)[:M]
  aux_all = aux_all.reshape(-1, 3)[:M]
  return net, runs[0][0], lead, loc_all, aux_all


def predict_bnf(features, observation_model, params, model_args, quantiles,
                ensemble_dims=2, approximate_quantiles=False, compute_dtype=None, weights=None):
  """-> (means, [quantile arrays]).  means: leading ensemble dims of `params`
  + (n_rows,); each quantile array has shape (n_rows,).
  weights (shape of the ensemble dims, `mixture_weights`): the quantiles are those of the weighted mixture over the
  members -- the weights `stack_members` returns; the per-member means do not change.  None: equal weights."""
  assert ensemble_dims >= 1
  w, _ = mixture_weights(weights, params, ensemble_dims)
  kw = {} if w is None else {'weights': w}
  features = np.asarray(features, dtype=np.float64)
  net, eng, lead, loc_all, aux_all = _ensemble_forecast(
      features, observation_model, params, model_args, ensemble_dims, compute_dtype)
  n_rows = features.shape[0]
  loc = loc_all.reshape(-1, n_rows)
  if observation_model == 'NORMAL':
    means = loc
    q = eng.normal_mixture_quantiles(means, aux_all.reshape(-1, 3)[:, 0], quantiles,
                                     approximate=approximate_quantiles, **kw)
  else:
    # NB / ZINB (inference.py:493-502): distribution means + root-found integer quantiles
    means, q = eng.count_mixture_quantiles(loc, aux_all.reshape(-1, 3), quantiles, **kw)
  torch.cuda.synchronize(eng.device)
  means_np = means.cpu().numpy().reshape(tuple(lead) + (n_rows,))
  q_np = q.cpu().numpy()
  eng.close()
  return means_np, [q_np[i] for i in range(q_np.shape[0])]


# ---------------------------------------------------------------------------
# posterior-predictive sample paths
# ---------------------------------------------------------------------------
_SAMPLE_CHUNK_CELLS = 1 << 26     # cells (sample x row, f32) of the device buffer one row chunk of sample_predictive fills


def csr_from_codes(codes, n_groups):
  """Rows sorted by group as CSR: integer group codes (R,) in [0, n_groups) -> (seg_offsets (n_groups + 1,) int32,
  seg_rows (R,) int32); group g owns seg_rows[seg_offsets[g]:seg_offsets[g + 1]], rows ascending inside a group,
  a code nobody carries is an empty segment.  The layout `bnf_predictive_group_sums` takes (include/bnf.h)."""
  codes = np.asarray(codes)
  if codes.ndim != 1 or (codes.size and not np.issubdtype(codes.dtype, np.integer)):
    raise ValueError('group codes must be a 1-d integer array')
  n_groups = int(n_groups)
  if n_groups < 1 or codes.size == 0 or codes.size >= 2**31:
    raise ValueError('need at least one group and between 1 and 2^31 - 1 rows')
  if codes.min() < 0 or codes.max() >= n_groups:
    raise ValueError(f'group codes must lie in [0, {n_groups})')
  seg_offsets = np.zeros(n_groups + 1, dtype=np.int64)
  np.cumsum(np.bincount(codes, minlength=n_groups), out=seg_offsets[1:])
  seg_rows = np.argsort(codes, kind='stable')
  return seg_offsets.astype(np.int32), seg_rows.astype(np.int32)


def csr_ordered(codes, n_groups, key):
  """`csr_from_codes` with the rows of every group in the order of `key` (R,), a sortable numeric or datetime array:
  ascending, rows with equal keys in table order (the sort is stable).  The layout `bnf_predictive_group_episodes` reads
  as time: position order inside a group.  -> (seg_offsets (n_groups + 1,) int32, seg_rows (R,) int32)."""
  seg_offsets, _ = csr_from_codes(codes, n_groups)
  codes = np.asarray(codes)
  key = np.asarray(key)
  if key.shape != codes.shape:
    raise ValueError(f'the order key must hold one value per row {codes.shape}; got {key.shape}')
  if key.dtype.kind in 'mM':
    if np.isnat(key).any():
      raise ValueError('the order key holds missing values')
    key = key.view(np.int64)
  elif key.dtype.kind not in 'biuf':
    raise ValueError(f'the order key must be numeric or datetime; got dtype {key.dtype}')
  elif key.dtype.kind == 'f' and np.isnan(key).any():
    raise ValueError('the order key holds missing values')
  seg_rows = np.lexsort((key, codes))          # by group, then by key; lexsort is stable
  return seg_offsets, seg_rows.astype(np.int32)


def mixture_weights(weights, params, ensemble_dims):
  """Member weights checked and flattened: `weights` must have the shape of the leading ensemble dims of `params` (what
  `member_log_prob` of score_predictive has; for VI the posterior draws count as components), every entry finite and >= 0,
  the sum within 1e-9 of 1; anything else is a ValueError.  -> (w (M,), cum (M,)) float64, flattened in the order the
  members are flattened everywhere else; cum = cumsum(w) with the last entry set to exactly 1, the form the sampling
  kernels take (include/bnf.h bnf_predictive_samples_weighted).  weights=None -> (None, None): equal weights.
  A weight below 2^-32 is never drawn by the sampling kernels."""
  if weights is None:
    return None, None
  lead = tuple(np.shape(params[0])[:ensemble_dims])
  try:
    w = np.asarray(weights, dtype=np.float64)
  except (TypeError, ValueError) as e:
    raise ValueError(f'weights must be an array of numbers of shape {lead}') from e
  if w.shape != lead:
    raise ValueError(f'weights must have the shape of the ensemble dims of the fitted parameters {lead}; got {w.shape}')
  if not np.all(np.isfinite(w)):
    raise ValueError('weights must be finite')
  if np.any(w < 0):
    raise ValueError('weights must be >= 0')
  total = float(np.sum(w, dtype=np.float64))
  if abs(total - 1.0) > 1e-9:
    raise ValueError(f'weights must sum to 1 (within 1e-9); got {total!r}')
  w = np.ascontiguousarray(w.reshape(-1))
  cum = np.cumsum(w, dtype=np.float64)
  cum[-1] = 1.0
  return w, cum


def _num_samples(num_samples, noun=None):
  """The sample count as an int >= 1 and, for a forecast that goes through bnf_sample_summaries (`noun` says what is
  summarised), at most its cap."""
  num_samples = int(num_samples)
  if num_samples < 1:
    raise ValueError(f'num_samples={num_samples}: need at least one sample path')
  if noun is not None and num_samples > _native.SUMMARY_MAX_SAMPLES:
    raise ValueError(f'num_samples={num_samples}: the {noun} are summarised from at most {_native.SUMMARY_MAX_SAMPLES} '
                     'sample paths')
  return num_samples


def _quantile_levels(quantiles):
  levels = [float(v) for v in quantiles]
  if any(not 0.0 <= v <= 1.0 for v in levels):
    raise ValueError(f'quantiles must lie in [0, 1]; got {levels}')
  return levels


def _check_cells(num_samples, n_groups, held='totals matrix is'):
  if num_samples * n_groups > _TOTALS_MAX_CELLS:
    raise ValueError(f'{num_samples} sample paths x {n_groups} groups: the {held} held whole on the device, at '
                     f'most {_TOTALS_MAX_CELLS} cells')


def _per_group(name, noun, values, n_groups):
  """An observed (G,) array as contiguous float64; None stays None."""
  if values is None:
    return None
  values = np.ascontiguousarray(values, dtype=np.float64)
  if values.shape != (n_groups,):
    raise ValueError(f'{name} must hold one {noun} per group ({n_groups},); got {values.shape}')
  return values


def _row_threshold(threshold, n_rows):
  """A (n_rows,) finite threshold as contiguous float64."""
  threshold = np.ascontiguousarray(threshold, dtype=np.float64)
  if threshold.shape != (n_rows,):
    raise ValueError(f'threshold must hold one limit per row ({n_rows},); got {threshold.shape}')
  if not np.all(np.isfinite(threshold)):
    raise ValueError('threshold must be finite')
  return threshold


@contextlib.contextmanager
def _sample_paths(features, observation_model, params, model_args, ensemble_dims, compute_dtype, weights, seed):
  """What everything that draws sample paths starts from: the member weights checked, the seed, the forward pass of every
  member -> (engine, loc (M, R), aux (M, 3), seed64, kw) with kw = {'cum_weights': ...} when weights are given, else {}.
  The engine is closed on exit.  Every check of the caller comes before this: nothing above `_ensemble_forecast` touches
  the GPU."""
  _, cum = mixture_weights(weights, params, ensemble_dims)
  kw = {} if cum is None else {'cum_weights': cum}
  seed64 = _native.seed_to_u64(seed)
  features = np.asarray(features, dtype=np.float64)
  _, eng, _, loc_all, aux_all = _ensemble_forecast(
      features, observation_model, params, model_args, ensemble_dims, compute_dtype)
  try:
    yield eng, loc_all.reshape(-1, features.shape[0]), aux_all.reshape(-1, 3), seed64, kw
  finally:
    eng.close()


def sample_predictive(features, observation_model, params, model_args, num_samples, seed, ensemble_dims,
                      groups=None, compute_dtype=None, weights=None):
  """Joint posterior-predictive draws on the GPU (include/bnf.h bnf_predictive_samples / bnf_predictive_group_sums;
  the reference draws with `.sample()` on its `likelihood_model()`).  Every leading ensemble dim of `params` --
  devices, members, and for VI the posterior draws -- flattens to the M equally weighted mixture components, exactly
  as in predict_bnf.  Sample path s uses ONE component for all rows, with observation noise per row on top.
    groups=None                      -> (num_samples, n_rows) float32
    groups=(seg_offsets, seg_rows)   -> (num_samples, G) float64 totals per group (`csr_from_codes`), summed on the
                                        device without materialising the draws
  The rows are drawn in chunks of _SAMPLE_CHUNK_CELLS // num_samples so that the device buffer stays bounded; the
  values do not depend on the chunking (counter-based generator keyed by seed, path and global row).
  weights (shape of the ensemble dims, `mixture_weights`): path s draws its component with these probabilities instead
  of equal ones -- the weights `stack_members` returns.  None: nothing changes."""
  num_samples = _num_samples(num_samples)
  with _sample_paths(features, observation_model, params, model_args, ensemble_dims, compute_dtype, weights,
                     seed) as (eng, loc, aux, seed64, kw):
    if groups is not None:
      seg_offsets, seg_rows = groups
      return eng.predictive_group_sums(loc, aux, seg_offsets, seg_rows, num_samples, seed64, **kw).cpu().numpy()
    n_rows = loc.shape[1]
    out = np.empty((num_samples, n_rows), dtype=np.float32)
    chunk = max(1, _SAMPLE_CHUNK_CELLS // num_samples)
    for r0 in range(0, n_rows, chunk):
      r1 = min(n_rows, r0 + chunk)
      out[:, r0:r1] = eng.predictive_samples(loc[:, r0:r1], aux, num_samples, seed64, row0=r0, **kw).cpu().numpy()
    return out


_TOTALS_MAX_CELLS = 1 << 28      # cells (sample x group, f64) of the totals matrix total_summaries holds on the device


def total_summaries(features, observation_model, params, model_args, num_samples, seed, ensemble_dims, groups,
                    observed=None, quantiles=(), energy=True, compute_dtype=None, weights=None):
  """Group totals of the joint sample paths summarised and scored on the GPU: the (num_samples, G) matrix
  `sample_predictive(..., groups=groups)` would return stays on the device (include/bnf.h bnf_predictive_group_sums) and
  only the summaries come back (bnf_sample_summaries, bnf_sample_energy_score).  groups = (seg_offsets, seg_rows) as
  `csr_from_codes` builds them; observed (G,) the observed totals, NaN where a group is not to be scored.
  -> dict of float64 numpy arrays:
    'mean' (G,)   'quantiles' (len(quantiles), G)   numpy's default 'linear' rule
    'crps' (G,)   'pit' (2, G)                      with `observed`: the ensemble CRPS of every total and #{x <= y} / S,
                                                    #{x < y} / S; NaN where observed is NaN
    'energy_score' float                            with `observed` and energy=True: the energy score of the joint paths
                                                    over the groups with an observed total (num_samples^2 G / 2 differences)
  The matrix is held whole (the energy score needs every column): num_samples <= 16,384 (BNF_SUMMARY_MAX_SAMPLES: a
  column is sorted in LDS) and num_samples * G <= 2^28 cells, ValueError beyond.
  weights: member weights of the sample paths as in `sample_predictive`; None: equal weights, nothing changes."""
  num_samples = _num_samples(num_samples, 'totals')
  levels = _quantile_levels(quantiles)
  seg_offsets, seg_rows = groups
  n_groups = len(seg_offsets) - 1
  _check_cells(num_samples, n_groups)
  observed = _per_group('observed', 'total', observed, n_groups)
  with _sample_paths(features, observation_model, params, model_args, ensemble_dims, compute_dtype, weights,
                     seed) as (eng, loc, aux, seed64, kw):
    totals = eng.predictive_group_sums(loc, aux, seg_offsets, seg_rows, num_samples, seed64, **kw)
    y = None if observed is None else torch.from_numpy(observed).to(eng.device)
    res = eng.sample_summaries(totals, y, levels)
    out = {k: v.cpu().numpy() for k, v in res.items()}
    if y is not None and energy:
      out['energy_score'] = eng.sample_energy_score(totals, y)
    return out


_COMBINATION_MAX_POSITIONS = (1 << 31) - 1     # nnz of bnf_predictive_combinations: the CSR offsets are int32


def combinations_csr(spec, n_rows, names=None):
  """Linear combinations of the rows of a sample path as CSR over positions -> (keys, form_offsets (K + 1,) int32,
  form_rows (nnz,) int32, form_coef (nnz,) float64), the layout `bnf_predictive_combinations` takes (include/bnf.h):
  combination k is sum_p form_coef[p] * x[form_rows[p]] over its positions form_offsets[k] <= p < form_offsets[k + 1].
  `spec` is one of
    a dict name -> (n_rows,) coefficients           keys = pd.Index of the names, in the dict's order
    a dense (K, n_rows) array (not a tuple)         keys = RangeIndex(K), or `names`
    a tuple (form, row, coef) of equal-length 1-d arrays (COO)
                                                    K = len(names) if given, else max(form) + 1; keys as for dense
  Coefficients equal to 0 are dropped; the positions are sorted by form, then by row; a combination left without a
  position stays, as an empty form (its value is 0).  A row may occur in many combinations or in none.
  ValueError for non-finite coefficients, rows outside [0, n_rows), negative form indices (or ones >= len(names)), a
  repeated (form, row) pair in a COO triple, 2^31 positions or more, and shapes that do not fit."""
  n_rows = int(n_rows)
  if n_rows < 1:
    raise ValueError(f'n_rows={n_rows}: need at least one row')

  def numbers_of(a, what, dtype=np.float64):
    try:
      return np.asarray(a, dtype=dtype)
    except (TypeError, ValueError) as e:
      raise ValueError(f'combinations: {what} must be an array of numbers') from e

  def integers_of(a, what):
    a = np.asarray(a)
    if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
      raise ValueError(f'combinations: {what} must be a 1-d integer array')
    return a.astype(np.int64)

  if isinstance(spec, dict):
    if names is not None:
      raise ValueError('combinations: a dict names its combinations itself; names must be None')
    if not spec:
      raise ValueError('combinations: need at least one combination')
    names = list(spec.keys())
    rows_of = [numbers_of(v, f'the coefficients of {k!r}') for k, v in spec.items()]
    bad = [k for k, v in zip(names, rows_of) if v.shape != (n_rows,)]
    if bad:
      raise ValueError(f'combinations: {bad[0]!r} must hold one coefficient per row ({n_rows},)')
    spec = np.stack(rows_of)
  if isinstance(spec, tuple):
    if len(spec) != 3:
      raise ValueError('combinations: a tuple must be the COO triple (form, row, coef)')
    form, row = integers_of(spec[0], 'form'), integers_of(spec[1], 'row')
    coef = numbers_of(spec[2], 'coef')
    if coef.ndim != 1 or not form.shape == row.shape == coef.shape:
      raise ValueError(f'combinations: form, row and coef must be 1-d arrays of one length; got {form.shape}, '
                       f'{row.shape}, {coef.shape}')
    if form.size and form.min() < 0:
      raise ValueError('combinations: negative form index')
    K = len(names) if names is not None else (int(form.max()) + 1 if form.size else 0)
    if K < 1:
      raise ValueError('combinations: need at least one combination')
    if form.size and form.max() >= K:
      raise ValueError(f'combinations: form index {int(form.max())} with {K} names')
    if row.size and (row.min() < 0 or row.max() >= n_rows):
      raise ValueError(f'combinations: rows must lie in [0, {n_rows})')
    if not np.all(np.isfinite(coef)):
      raise ValueError('combinations: coefficients must be finite')
    cell = form * n_rows + row
    order = np.argsort(cell, kind='stable')                 # by form, then by row
    cell = cell[order]
    if cell.size > 1 and np.any(cell[1:] == cell[:-1]):
      raise ValueError('combinations: a (form, row) pair is repeated in the COO triple')
    keep = order[coef[order] != 0]
    form, row, coef = form[keep], row[keep], coef[keep]
  else:
    dense = numbers_of(spec, 'a dense spec')
    if dense.ndim != 2 or dense.shape[0] < 1 or dense.shape[1] != n_rows:
      raise ValueError(f'combinations: a dense spec must be (K, {n_rows}) with K >= 1; got {dense.shape}')
    if not np.all(np.isfinite(dense)):
      raise ValueError('combinations: coefficients must be finite')
    K = dense.shape[0]
    if names is not None and len(names) != K:
      raise ValueError(f'combinations: {len(names)} names for {K} combinations')
    form, row = np.nonzero(dense)                            # row-major: by form, then by row
    coef = dense[form, row]
  if form.size > _COMBINATION_MAX_POSITIONS:
    raise ValueError(f'combinations: {form.size} positions; at most {_COMBINATION_MAX_POSITIONS}')
  keys = pd.RangeIndex(K) if names is None else pd.Index(names)
  form_offsets = np.zeros(K + 1, dtype=np.int64)
  np.cumsum(np.bincount(form, minlength=K), out=form_offsets[1:])
  return (keys, form_offsets.astype(np.int32), np.ascontiguousarray(row, dtype=np.int32),
          np.ascontiguousarray(coef, dtype=np.float64))


def combination_summaries(features, observation_model, params, model_args, num_samples, seed, ensemble_dims, combinations,
                          observed=None, quantiles=(), energy=True, samples=False, compute_dtype=None, weights=None):
  """Linear combinations of the rows of the joint sample paths -- weighted means, contrasts, overlapping groups --
  summarised and scored on the GPU: the (num_samples, K) matrix out[s][k] = sum_p coef[p] * draw(s, rows[p]) is formed
  without materialising the draws (include/bnf.h bnf_predictive_combinations), stays on the device and only the summaries
  come back (bnf_sample_summaries, bnf_sample_energy_score).  combinations = (form_offsets, form_rows, form_coef) as
  `combinations_csr` builds them; observed (K,) the observed values, NaN where a combination is not to be scored.
  -> the dict of `total_summaries` ('mean', 'quantiles', with `observed` 'crps', 'pit' and 'energy_score'), and with
  samples=True also 'samples' (num_samples, K) float64, the matrix itself.
  The caps of `total_summaries` apply: num_samples <= 16,384 and num_samples * K <= 2^28 cells, ValueError beyond.  A row
  that occurs at m positions is drawn m times.
  weights: member weights of the sample paths as in `sample_predictive`; None: equal weights."""
  num_samples = _num_samples(num_samples, 'combinations')
  levels = _quantile_levels(quantiles)
  form_offsets, form_rows, form_coef = combinations
  n_forms = len(form_offsets) - 1
  _check_cells(num_samples, n_forms, 'matrix of combinations is')
  observed = _per_group('observed', 'value', observed, n_forms)
  with _sample_paths(features, observation_model, params, model_args, ensemble_dims, compute_dtype, weights,
                     seed) as (eng, loc, aux, seed64, kw):
    x = eng.predictive_combinations(loc, aux, form_offsets, form_rows, form_coef, num_samples, seed64, **kw)
    y = None if observed is None else torch.from_numpy(observed).to(eng.device)
    res = eng.sample_summaries(x, y, levels)
    out = {k: v.cpu().numpy() for k, v in res.items()}
    if y is not None and energy:
      out['energy_score'] = eng.sample_energy_score(x, y)
    if samples:
      out['samples'] = x.cpu().numpy()
    return out


VARIOGRAM_ORDERS = (0.5, 1.0, 2.0)      # the p the variogram is compiled for (include/bnf.h bnf_sample_pair_moments)


def dependence_summaries(features, observation_model, params, model_args, num_samples, seed, ensemble_dims, groups,
                         observed=None, p=0.5, pair_weights=None, matrices=True, compute_dtype=None, weights=None):
  """How the group totals of the joint sample paths move together, formed and scored on the GPU: the (num_samples, G)
  matrix `sample_predictive(..., groups=groups)` would return stays on the device (include/bnf.h
  bnf_predictive_group_sums) and only the results come back (bnf_sample_pair_moments).  groups = (seg_offsets, seg_rows) as
  `csr_from_codes` builds them; observed (G,) the observed totals, NaN where a group is not to be scored.
  -> dict of float64 numpy arrays:
    'mean' (G,)
    'covariance' (G, G)  'variogram' (G, G)   matrices=True: (1 / S) sum_s (x_si - m_i) (x_sj - m_j) -- np.cov(bias=True)
                                              -- and (1 / S) sum_s |x_si - x_sj|^p, both bitwise symmetric
    'variogram_score' float                   with `observed`: sum over the pairs i < j of scored groups of
                                              w_ij (|y_i - y_j|^p - variogram_ij)^2, w_ij = 1 or pair_weights[i][j]
  p is 0.5, 1 or 2; pair_weights (G, G) finite, >= 0 and symmetric.  num_samples * G <= 2^28 cells (there is no cap on the
  sample paths alone: nothing is sorted), and G <= 4,096 with `matrices` or `pair_weights`; ValueError beyond, before any
  GPU work.  num_samples G^2 / 2 pair terms.
  weights: member weights of the sample paths as in `sample_predictive`; None: equal weights."""
  num_samples = _num_samples(num_samples)
  try:
    p = float(p)
  except (TypeError, ValueError) as e:
    raise ValueError(f'p must be one of {VARIOGRAM_ORDERS}') from e
  if p not in VARIOGRAM_ORDERS:
    raise ValueError(f'p={p!r}: the variogram is formed for p in {VARIOGRAM_ORDERS}')
  seg_offsets, seg_rows = groups
  n_groups = len(seg_offsets) - 1
  _check_cells(num_samples, n_groups)
  if (matrices or pair_weights is not None) and n_groups > _native.PAIR_MATRIX_MAX_COLS:
    raise ValueError(f'{n_groups} groups: a pair matrix (matrices=True, pair_weights) has at most '
                     f'{_native.PAIR_MATRIX_MAX_COLS} groups a side; matrices=False gives the variogram score alone')
  observed = _per_group('observed', 'total', observed, n_groups)
  if pair_weights is not None:
    if observed is None:
      raise ValueError('pair_weights weight the variogram score: they need `observed`')
    try:
      pair_weights = np.ascontiguousarray(pair_weights, dtype=np.float64)
    except (TypeError, ValueError) as e:
      raise ValueError(f'pair_weights must be an array of numbers of shape ({n_groups}, {n_groups})') from e
    if pair_weights.shape != (n_groups, n_groups):
      raise ValueError(f'pair_weights must hold one weight per pair of groups ({n_groups}, {n_groups}); got '
                       f'{pair_weights.shape}')
    if not np.all(np.isfinite(pair_weights)):
      raise ValueError('pair_weights must be finite')
    if np.any(pair_weights < 0):
      raise ValueError('pair_weights must be >= 0')
    if not np.array_equal(pair_weights, pair_weights.T):
      raise ValueError('pair_weights must be symmetric')
  with _sample_paths(features, observation_model, params, model_args, ensemble_dims, compute_dtype, weights,
                     seed) as (eng, loc, aux, seed64, kw):
    totals = eng.predictive_group_sums(loc, aux, seg_offsets, seg_rows, num_samples, seed64, **kw)
    y = None if observed is None else torch.from_numpy(observed).to(eng.device)
    w = None if pair_weights is None else torch.from_numpy(pair_weights).to(eng.device)
    res = eng.sample_pair_moments(totals, p, y, w, matrices=bool(matrices))
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in res.items()}


SCENARIO_NORMS = (1, 2)      # the norms the path distances are compiled for (include/bnf.h bnf_sample_distances)


def scenario_summaries(features, observation_model, params, model_args, num_samples, seed, ensemble_dims, groups, k,
                       norm=2, scale=None, observed=None, compute_dtype=None, weights=None):
  """The joint sample paths reduced to k representative scenarios on the GPU -- fast forward selection (Heitsch & Roemisch
  2003): the (num_samples, G) matrix of group totals `sample_predictive(..., groups=groups)` would return stays on the
  device (include/bnf.h bnf_predictive_group_sums), the paths' pairwise distances are formed there (bnf_sample_distances:
  the `norm`-norm, 1 or 2, of the difference of two vectors of totals, every total divided by scale (G,) finite and > 0 when
  given), the scenarios are picked there (bnf_scenario_select) and their k rows of totals gathered there.  groups =
  (seg_offsets, seg_rows) as `csr_from_codes` builds them; observed (G,) the observed totals, NaN where a group is to be
  left out of every distance.  -> dict of numpy arrays:
    'scenarios' (k, G) f64      the totals of the chosen paths, in the order chosen
    'path' (k,) int64           their indices among the sample paths
    'probability' (k,) f64      the share of the paths nearest to each (the earliest chosen among equally near)
    'distance' (k,) f64         the Kantorovich distance between the ensemble and the first 1 .. k scenarios, nonincreasing
    'assignment' (num_samples,) int64   the scenario of every path
  and with `observed`:
    'nearest' int               the scenario nearest to the observed vector      'nearest_distance' float
    'pit' (2,) f64              the shares of the paths whose distance to their scenario is <= and < 'nearest_distance'
  1 <= k <= num_samples <= 4,096 (BNF_SCENARIO_MAX_SAMPLES: the distance matrix is held whole), ValueError beyond, before
  any GPU work.  num_samples^2 G / 2 differences, k num_samples^2 reads of the matrix.
  weights: member weights of the sample paths as in `sample_predictive`; None: equal weights."""
  num_samples = _num_samples(num_samples)
  if num_samples > _native.SCENARIO_MAX_SAMPLES:
    raise ValueError(f'num_samples={num_samples}: the scenarios are chosen among at most {_native.SCENARIO_MAX_SAMPLES} '
                     'sample paths')
  if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= num_samples:
    raise ValueError(f'k={k!r}: an integer in 1..{num_samples}, the number of sample paths')
  k = int(k)
  if isinstance(norm, bool) or norm not in SCENARIO_NORMS:
    raise ValueError(f'norm={norm!r}: the distance between two paths is formed for norm in {SCENARIO_NORMS}')
  norm = int(norm)
  seg_offsets, seg_rows = groups
  n_groups = len(seg_offsets) - 1
  _check_cells(num_samples, n_groups)
  if scale is not None:
    try:
      scale = np.ascontiguousarray(scale, dtype=np.float64)
    except (TypeError, ValueError) as e:
      raise ValueError(f'scale must be an array of numbers of shape ({n_groups},)') from e
    if scale.shape != (n_groups,):
      raise ValueError(f'scale must hold one divisor per group ({n_groups},); got {scale.shape}')
    if not (np.all(np.isfinite(scale)) and np.all(scale > 0)):
      raise ValueError('scale must be finite and > 0')
  observed = _per_group('observed', 'total', observed, n_groups)
  if observed is not None and not np.isfinite(observed).any():
    raise ValueError('observed: no group has an observed total')
  with _sample_paths(features, observation_model, params, model_args, ensemble_dims, compute_dtype, weights,
                     seed) as (eng, loc, aux, seed64, kw):
    totals = eng.predictive_group_sums(loc, aux, seg_offsets, seg_rows, num_samples, seed64, **kw)
    sc = None if scale is None else torch.from_numpy(scale).to(eng.device)
    y = None if observed is None else torch.from_numpy(observed).to(eng.device)
    dist, ydist = eng.sample_distances(totals, norm, sc, y)
    res = eng.scenario_select(dist, k, ydist)
    scenarios = totals.index_select(0, res['chosen'].clamp(min=0).to(torch.int64))       # (-1: a NaN total; NaN below)
    host = lambda t: t.cpu().numpy()
    path = host(res['chosen']).astype(np.int64)
    out = {'scenarios': host(scenarios), 'path': path, 'probability': host(res['prob']),
           'distance': host(res['objective']), 'assignment': host(res['assign']).astype(np.int64)}
    if np.any(path < 0):
      out['scenarios'][:] = np.nan
    if y is not None:
      obs = host(res['obs'])
      out.update(nearest=int(host(res['obs_nearest'])[0]), nearest_distance=float(obs[0]), pit=obs[1:3].copy())
    return out


def ranking_summaries(features, observation_model, params, model_args, num_samples, seed, ensemble_dims, groups,
                      observed=None, scale=None, top_k=1, quantiles=(), compute_dtype=None, weights=None):
  """How the group totals of the joint sample paths rank against each other within a path, formed and scored on the GPU:
  the (num_samples, G) matrix `sample_predictive(..., groups=groups)` would return stays on the device (include/bnf.h
  bnf_predictive_group_sums), every path is ranked there (bnf_sample_ranks: rank 1 is the largest total, tied groups
  share their block of ranks), and only the results come back.  groups = (seg_offsets, seg_rows) as `csr_from_codes`
  builds them; scale (G,) finite and > 0 divides the totals before they are ranked (a population: rank per capita);
  observed (G,) the observed totals, NaN where a group is not to be scored.
  -> dict of numpy arrays, float64 unless noted:
    'rank_mean' (G,)   'rank_quantiles' (len(quantiles), G)   of the mid-rank over the paths (bnf_sample_summaries)
    'rank_probability' (top_k, G)                             P(the group takes rank slot k), ties sharing
                                                              (bnf_rank_probabilities); every row sums to 1
  and with `observed`:
    'observed_rank' (G,)  'observed_above' (G,) int64  'observed_ties' (G,) int64
                                      bnf_sample_ranks on the observed totals as one path; NaN / -1 / -1 where not scored
    'rank_crps' (G,)  'rank_pit' (2, G)   the ensemble CRPS and PIT of the mid-rank against the observed one
    'scored_rank_mean', 'scored_rank_quantiles', 'scored_rank_probability'   the three forecast outputs of the ranking
                                      AMONG THE SCORED GROUPS (NaN in the other columns; rows k > their number are 0)
  When `observed` holds NaN the scored forecast is not the plain one: the scored columns are selected on the device and
  ranked again among themselves, so that forecast and observed ranks mean the same thing; the plain outputs rank all groups.
  num_samples <= 16,384 (the summaries' cap), num_samples * G <= 2^28 cells, G <= 16,384, 1 <= top_k <= G and
  top_k * G <= 2^24; ValueError beyond, before any GPU work.
  weights: member weights of the sample paths as in `sample_predictive`; None: equal weights."""
  num_samples = _num_samples(num_samples, 'ranks')
  levels = _quantile_levels(quantiles)
  seg_offsets, seg_rows = groups
  n_groups = len(seg_offsets) - 1
  if n_groups > _native.RANK_MAX_COLS:
    raise ValueError(f'{n_groups} groups: the totals of a path are ranked in LDS, at most {_native.RANK_MAX_COLS}')
  _check_cells(num_samples, n_groups)
  try:
    top_k = int(top_k)
  except (TypeError, ValueError) as e:
    raise ValueError(f'top_k must be an integer in 1..{n_groups}') from e
  if not 1 <= top_k <= n_groups:
    raise ValueError(f'top_k={top_k}: 1..{n_groups}, the number of groups')
  if top_k * n_groups > _native.RANK_MAX_CELLS:
    raise ValueError(f'top_k={top_k} x {n_groups} groups: at most {_native.RANK_MAX_CELLS} rank probabilities')
  observed = _per_group('observed', 'total', observed, n_groups)
  if scale is not None:
    try:
      scale = np.ascontiguousarray(scale, dtype=np.float64)
    except (TypeError, ValueError) as e:
      raise ValueError(f'scale must be an array of numbers of shape ({n_groups},)') from e
    if scale.shape != (n_groups,):
      raise ValueError(f'scale must hold one divisor per group ({n_groups},); got {scale.shape}')
    if not (np.all(np.isfinite(scale)) and np.all(scale > 0)):
      raise ValueError('scale must be finite and > 0')
  with _sample_paths(features, observation_model, params, model_args, ensemble_dims, compute_dtype, weights,
                     seed) as (eng, loc, aux, seed64, kw):
    totals = eng.predictive_group_sums(loc, aux, seg_offsets, seg_rows, num_samples, seed64, **kw)
    sc = None if scale is None else torch.from_numpy(scale).to(eng.device)

    def forecast(x, s, y_rank, k):
      r = eng.sample_ranks(x, s)
      summ = eng.sample_summaries(r['rank'], y_rank, levels)
      return summ, eng.rank_probabilities(r['above'], r['ties'], k)

    host = lambda t: t.cpu().numpy()
    scored = None if observed is None else ~np.isnan(observed)
    out = {}
    if scored is None or not scored.all():              # the plain forecast: all groups
      summ, prob = forecast(totals, sc, None, top_k)
      out.update(rank_mean=host(summ['mean']), rank_quantiles=host(summ['quantiles']), rank_probability=host(prob))
    if scored is not None:
      n = int(scored.sum())
      sub = {'rank_mean': np.full(n_groups, np.nan), 'rank_quantiles': np.full((len(levels), n_groups), np.nan),
             'rank_probability': np.full((top_k, n_groups), np.nan), 'rank_crps': np.full(n_groups, np.nan),
             'rank_pit': np.full((2, n_groups), np.nan)}
      obs_rank, obs_above, obs_ties = np.full(n_groups, np.nan), np.full(n_groups, -1), np.full(n_groups, -1)
      if n:
        whole = n == n_groups
        idx = None if whole else torch.from_numpy(np.flatnonzero(scored)).to(eng.device)
        x = totals if whole else totals.index_select(1, idx)
        s = sc if whole or sc is None else sc.index_select(0, idx)
        y = torch.from_numpy(observed).to(eng.device)
        y = y if whole else y.index_select(0, idx)
        o = eng.sample_ranks(y.reshape(1, n), s)        # the observed ranks: the same call on one path
        k = min(top_k, n)
        summ, prob = forecast(x, s, o['rank'].reshape(n), k)
        sub['rank_mean'][scored], sub['rank_quantiles'][:, scored] = host(summ['mean']), host(summ['quantiles'])
        sub['rank_crps'][scored], sub['rank_pit'][:, scored] = host(summ['crps']), host(summ['pit'])
        sub['rank_probability'][:k, scored] = host(prob)
        sub['rank_probability'][k:, scored] = 0.0       # among n groups no rank slot beyond n is ever taken
        obs_rank[scored] = host(o['rank'])[0]
        obs_above[scored], obs_ties[scored] = host(o['above'])[0], host(o['ties'])[0]
      if scored.all():
        out.update({key: sub[key] for key in ('rank_mean', 'rank_quantiles', 'rank_probability')})
      out.update(observed_rank=obs_rank, observed_above=obs_above, observed_ties=obs_ties, rank_crps=sub['rank_crps'],
                 rank_pit=sub['rank_pit'], scored_rank_mean=sub['rank_mean'], scored_rank_quantiles=sub['rank_quantiles'],
                 scored_rank_probability=sub['rank_probability'])
    return out


def extreme_summaries(features, observation_model, params, model_args, num_samples, seed, ensemble_dims, groups,
                      threshold=None, observed_max=None, observed_count=None, quantiles=(), compute_dtype=None,
                      weights=None):
  """Group peaks and threshold exceedances of the joint sample paths, summarised and scored on the GPU: per path and
  group the largest draw, the row where it is first reached and the number of rows above their threshold are formed
  without materialising the draws (include/bnf.h bnf_predictive_group_extremes); the (num_samples, G) matrices stay on the
  device and go through bnf_sample_summaries.  groups = (seg_offsets, seg_rows) as `csr_from_codes` builds them;
  threshold (n_rows,) finite, in the units of the draws, compared with strict >; observed_max / observed_count (G,) the
  observed peak value / number of exceedances, NaN where a group is not to be scored.  -> dict of numpy arrays:
    'max_mean' (G,)  'max_quantiles' (len(quantiles), G)   of the group's peak value, numpy's default 'linear' rule
    'max_crps' (G,)  'max_pit' (2, G)                      with observed_max, as `total_summaries` forms them
    'peak_probability' (n_rows,)                           share of the paths in which the row is where its group first
                                                           reaches its maximum (ties: the lowest table row)
  and with `threshold`:
    'count_mean', 'count_quantiles', ('count_crps', 'count_pit' with observed_count)   of the number of rows above
    'exceed_any' (G,)                                      share of the paths with at least one row above its threshold
                                                           (the paths counted on the device, divided on the host)
    'exceed_probability' (n_rows,)                         share of the paths whose draw at the row is above its threshold
  The caps of `total_summaries` apply: num_samples <= 16,384 and num_samples * G <= 2^28 cells, ValueError beyond.
  weights: member weights of the sample paths as in `sample_predictive`; None: equal weights."""
  num_samples = _num_samples(num_samples, 'extremes')
  levels = _quantile_levels(quantiles)
  seg_offsets, seg_rows = groups
  n_groups = len(seg_offsets) - 1
  _check_cells(num_samples, n_groups, 'matrices are')
  features = np.asarray(features, dtype=np.float64)
  if threshold is not None:
    threshold = _row_threshold(threshold, features.shape[0])
  elif observed_count is not None:
    raise ValueError('observed_count needs a threshold')
  observed = {name: _per_group(f'observed_{name}', 'value', obs, n_groups)
              for name, obs in (('max', observed_max), ('count', observed_count))}
  with _sample_paths(features, observation_model, params, model_args, ensemble_dims, compute_dtype, weights,
                     seed) as (eng, loc, aux, seed64, kw):
    thr = None if threshold is None else threshold.astype(np.float32)
    ext = eng.predictive_group_extremes(loc, aux, seg_offsets, seg_rows, num_samples, seed64, threshold=thr, **kw)
    out = {'peak_probability': ext['peak_count'].cpu().numpy().astype(np.float64) / num_samples}
    for name in ('max', 'count') if thr is not None else ('max',):
      y = None if observed[name] is None else torch.from_numpy(observed[name]).to(eng.device)
      for k, v in eng.sample_summaries(ext[name], y, levels).items():
        out[f'{name}_{k}'] = v.cpu().numpy()
    if thr is not None:
      out['exceed_any'] = (ext['count'] > 0).sum(dim=0).cpu().numpy().astype(np.float64) / num_samples
      out['exceed_probability'] = ext['exceed_count'].cpu().numpy().astype(np.float64) / num_samples
    return out


EPISODE_SERIES = ('longest', 'spells', 'onset_step')


def episode_summaries(features, observation_model, params, model_args, num_samples, seed, ensemble_dims, groups,
                      threshold, observed_longest=None, observed_spells=None, observed_onset_step=None, quantiles=(),
                      compute_dtype=None, weights=None):
  """Spells above a threshold in the joint sample paths, summarised and scored on the GPU: per path and group the
  longest run of consecutive rows above their threshold, the number of runs and the number of steps before the first row
  above are formed without materialising the draws (include/bnf.h bnf_predictive_group_episodes); the (num_samples, G)
  matrices stay on the device and go through bnf_sample_summaries.  groups = (seg_offsets, seg_rows) with the rows of a
  group in TIME order (`csr_ordered`); threshold (n_rows,) finite, in the units of the draws, compared with strict >;
  observed_longest / observed_spells / observed_onset_step (G,) the observed values, NaN where a group is not to be
  scored.  -> dict of numpy arrays, for name in 'longest', 'spells', 'onset_step' (censored at the group's size when a
  path never goes above):
    '<name>_mean' (G,)  '<name>_quantiles' (len(quantiles), G)   numpy's default 'linear' rule
    '<name>_crps' (G,)  '<name>_pit' (2, G)                      with observed_<name>, as `total_summaries` forms them
  and
    'onset_count' (n_rows,) int64     the paths in which the row is its group's first row above its threshold
    'onset_probability' (n_rows,)     onset_count / num_samples
    'no_episode_count' (G,) int64     the paths that never go above (longest == 0, counted on the device)
    'no_episode' (G,)                 no_episode_count / num_samples = 1 - the group's sum of onset_probability
  The caps of `total_summaries` apply: num_samples <= 16,384 and num_samples * G <= 2^28 cells, ValueError beyond.
  weights: member weights of the sample paths as in `sample_predictive`; None: equal weights."""
  num_samples = _num_samples(num_samples, 'episodes')
  levels = _quantile_levels(quantiles)
  seg_offsets, seg_rows = groups
  n_groups = len(seg_offsets) - 1
  _check_cells(num_samples, n_groups, 'matrices are')
  features = np.asarray(features, dtype=np.float64)
  if threshold is None:
    raise ValueError('threshold is required: one limit per row')
  threshold = _row_threshold(threshold, features.shape[0])
  observed = {name: _per_group(f'observed_{name}', 'value', obs, n_groups)
              for name, obs in zip(EPISODE_SERIES, (observed_longest, observed_spells, observed_onset_step))}
  with _sample_paths(features, observation_model, params, model_args, ensemble_dims, compute_dtype, weights,
                     seed) as (eng, loc, aux, seed64, kw):
    ep = eng.predictive_group_episodes(loc, aux, seg_offsets, seg_rows, num_samples, seed64,
                                       threshold.astype(np.float32), **kw)
    out = {'onset_count': ep['onset_count'].cpu().numpy().astype(np.int64),
           'no_episode_count': (ep['longest'] == 0).sum(dim=0).cpu().numpy().astype(np.int64)}
    out['onset_probability'] = out['onset_count'].astype(np.float64) / num_samples
    out['no_episode'] = out['no_episode_count'].astype(np.float64) / num_samples
    for name in EPISODE_SERIES:
      y = None if observed[name] is None else torch.from_numpy(observed[name]).to(eng.device)
      for k, v in eng.sample_summaries(ep[name], y, levels).items():
        out[f'{name}_{k}'] = v.cpu().numpy()
    return out


def _group_level(level, n_groups, name='level'):
  """A (G,) finite level (or, under another `name`, threshold) as contiguous float64; None stays None."""
  if level is None:
    return None
  try:
    level = np.ascontiguousarray(level, dtype=np.float64)
  except (TypeError, ValueError) as e:
    raise ValueError(f'{name} must be an array of numbers of shape ({n_groups},)') from e
  if level.shape != (n_groups,):
    raise ValueError(f'{name} must hold one {name} per group ({n_groups},); got {level.shape}')
  if not np.all(np.isfinite(level)):
    raise ValueError(f'{name} must be finite')
  return level


def cumulative_summaries(features, observation_model, params, model_args, num_samples, seed, ensemble_dims, groups,
                         level=None, curve=True, observed_total=None, observed_running=None, observed_cross_step=None,
                         quantiles=(), compute_dtype=None, weights=None):
  """Running totals of the joint sample paths and when they pass a level, summarised and scored on the GPU: per path and
  group the cumulative curve over the group's rows in time order, its last value and the step at which it first lies
  above the group's level are formed without materialising the draws (include/bnf.h bnf_predictive_group_cumulative);
  the matrices stay on the device and go through bnf_sample_summaries.  groups = (seg_offsets, seg_rows) with the rows
  of a group in TIME order (`csr_ordered`); level (G,) finite, any sign, compared with strict >; observed_total /
  observed_cross_step (G,) and observed_running (n_rows,), per TABLE ROW, the observed values, NaN where not to be scored.
  -> dict of float64 numpy arrays:
    'total_mean' (G,)  'total_quantiles' (len(quantiles), G)     numpy's default 'linear' rule
    'total_crps' (G,)  'total_pit' (2, G)                        with observed_total, as `total_summaries` forms them
  with curve=True, per table row (NaN at a row no position of seg_rows names):
    'running_mean' (n_rows,)  'running_quantiles' (len(quantiles), n_rows)   of the running total at the row: the band
                                                                 of the joint paths, which no marginal forecast gives
    'running_crps' (n_rows,)  'running_pit' (2, n_rows)          with observed_running
  and with `level`:
    'cross_step_mean', 'cross_step_quantiles', ('cross_step_crps', 'cross_step_pit' with observed_cross_step)   of the
                                      number of steps before the crossing row, censored at the group's size
    'crossing_probability' (n_rows,)  share of the paths in which the row is where its group first lies above its level
    'above_probability' (n_rows,)     share of the paths whose running total at the row lies above the level
    'never' (G,)                      share of the paths that never cross (cross_row < 0, counted on the device) = 1 - the
                                      group's sum of crossing_probability
  The caps of `total_summaries` apply: num_samples <= 16,384 and num_samples * G <= 2^28 cells; curve=True holds the
  (num_samples, n_rows) curves whole as well: num_samples * n_rows <= 2^28.  ValueError beyond, before any GPU work.
  A group longer than a tile of 1,024 rows is parallel over the paths only (profiles/group_cumulative.md:
  one group of 10^6 rows and 1,000 paths takes 1.3 times the group sums).
  weights: member weights of the sample paths as in `sample_predictive`; None: equal weights."""
  num_samples = _num_samples(num_samples, 'running totals')
  levels = _quantile_levels(quantiles)
  seg_offsets, seg_rows = groups
  n_groups = len(seg_offsets) - 1
  _check_cells(num_samples, n_groups)
  features = np.asarray(features, dtype=np.float64)
  n_rows = features.shape[0]
  if curve:
    _check_cells(num_samples, n_rows, 'running totals are')
  level = _group_level(level, n_groups)
  if level is None and observed_cross_step is not None:
    raise ValueError('observed_cross_step needs a level')
  if not curve and observed_running is not None:
    raise ValueError('observed_running needs curve=True')
  observed = {'total': _per_group('observed_total', 'value', observed_total, n_groups),
              'cross_step': _per_group('observed_cross_step', 'value', observed_cross_step, n_groups)}
  if observed_running is not None:
    observed_running = np.ascontiguousarray(observed_running, dtype=np.float64)
    if observed_running.shape != (n_rows,):
      raise ValueError(f'observed_running must hold one value per row ({n_rows},); got {observed_running.shape}')
  with _sample_paths(features, observation_model, params, model_args, ensemble_dims, compute_dtype, weights,
                     seed) as (eng, loc, aux, seed64, kw):
    cu = eng.predictive_group_cumulative(loc, aux, seg_offsets, seg_rows, num_samples, seed64, level=level,
                                         running=bool(curve), **kw)
    out = {}
    for name in ('total', 'cross_step') if level is not None else ('total',):
      y = None if observed[name] is None else torch.from_numpy(observed[name]).to(eng.device)
      for k, v in eng.sample_summaries(cu[name], y, levels).items():
        out[f'{name}_{k}'] = v.cpu().numpy()
    if curve:                                   # column = position: back to table rows through seg_rows
      pos_rows = np.asarray(seg_rows, dtype=np.int64)
      named = (pos_rows >= 0) & (pos_rows < n_rows)
      y = None
      if observed_running is not None:
        y_pos = np.full(pos_rows.shape, np.nan)
        y_pos[named] = observed_running[pos_rows[named]]
        y = torch.from_numpy(y_pos).to(eng.device)
      for k, v in eng.sample_summaries(cu['running'], y, levels).items():
        v = v.cpu().numpy()
        by_row = np.full(v.shape, np.nan)
        by_row[..., pos_rows[named]] = v[..., named]
        out[f'running_{k}'] = by_row
    if level is not None:
      out['crossing_probability'] = cu['cross_count'].cpu().numpy().astype(np.float64) / num_samples
      out['above_probability'] = cu['above_count'].cpu().numpy().astype(np.float64) / num_samples
      out['never'] = (cu['cross_row'] < 0).sum(dim=0).cpu().numpy().astype(np.float64) / num_samples
    return out


def _window_length(window):
  """The length of a moving window in positions: an integer (not a bool) in [1, 2^31 - 1] -> int."""
  if isinstance(window, (bool, np.bool_)) or not isinstance(window, numbers.Integral):
    raise ValueError(f'window must be an integer number of rows; got {window!r}')
  if not 1 <= int(window) <= 0x7fffffff:
    raise ValueError(f'window={int(window)}: 1..{0x7fffffff} rows')
  return int(window)


def window_candidates(seg_offsets, seg_rows, n_rows, window):
  """Per POSITION of seg_rows: does a full-length window end here?  The position takes part (its entry of seg_rows is a
  table row) and has at least min(window, the group's size) positions of its group up to and including it (include/bnf.h
  bnf_predictive_group_windows: CANDIDATE) -> (len(seg_rows),) bool."""
  off = np.asarray(seg_offsets, dtype=np.int64)
  rows = np.asarray(seg_rows, dtype=np.int64)
  sizes = np.diff(off)
  at = np.arange(len(rows), dtype=np.int64) - np.repeat(off[:-1], sizes) + 1      # positions of the group so far
  return (rows >= 0) & (rows < n_rows) & (at >= np.minimum(int(window), np.repeat(sizes, sizes)))


def window_summaries(features, observation_model, params, model_args, num_samples, seed, ensemble_dims, groups, window,
                     threshold=None, curve=True, observed_peak=None, observed_window=None, observed_count=None,
                     quantiles=(), compute_dtype=None, weights=None):
  """Moving-window totals of the joint sample paths, summarised and scored on the GPU: per path and group the total over
  the last `window` rows at every row in time order, its largest value over the group and the number of windows above
  the group's threshold are formed without materialising the draws (include/bnf.h bnf_predictive_group_windows); the
  matrices stay on the device and go through bnf_sample_summaries.  groups = (seg_offsets, seg_rows) with the rows of a
  group in TIME order (`csr_ordered`); window an integer >= 1; threshold (G,) finite, any sign, compared with strict >;
  observed_peak / observed_count (G,) and observed_window (n_rows,), per TABLE ROW, the observed values, NaN where not
  to be scored.  Only FULL-LENGTH windows count (`window_candidates`): a group shorter than `window` has one, the whole
  group.  -> dict of float64 numpy arrays:
    'peak_mean' (G,)  'peak_quantiles' (len(quantiles), G)     of the largest window of the group, 'linear' quantiles
    'peak_crps' (G,)  'peak_pit' (2, G)                        with observed_peak, as `total_summaries` forms them
    'peak_probability' (n_rows,)      share of the paths whose largest window ends at the row (ties: the earliest)
  with curve=True, per table row (NaN at a row at which no full-length window ends, so that nobody reads a clipped
  window as a full one):
    'window_mean' (n_rows,)  'window_quantiles' (len(quantiles), n_rows)   of the window total ending at the row: the
                                                               band of the joint paths, which no marginal forecast gives
    'window_crps' (n_rows,)  'window_pit' (2, n_rows)          with observed_window
  and with `threshold`:
    'count_mean', 'count_quantiles', ('count_crps', 'count_pit' with observed_count)   of the number of windows above
    'exceed_probability' (n_rows,)    share of the paths whose window ending at the row is above the threshold
    'any' (G,)                        share of the paths with at least one window above (count > 0, formed on the device)
  The caps of `cumulative_summaries` apply: num_samples <= 16,384 and num_samples * G <= 2^28 cells; curve=True holds the
  (num_samples, n_rows) windows whole as well: num_samples * n_rows <= 2^28.  ValueError beyond, before any GPU work.
  A group longer than a tile of 1,024 rows is parallel over the paths only (profiles/group_windows.md).
  weights: member weights of the sample paths as in `sample_predictive`; None: equal weights."""
  num_samples = _num_samples(num_samples, 'window totals')
  levels = _quantile_levels(quantiles)
  window = _window_length(window)
  seg_offsets, seg_rows = groups
  n_groups = len(seg_offsets) - 1
  _check_cells(num_samples, n_groups, 'peak matrix is')
  features = np.asarray(features, dtype=np.float64)
  n_rows = features.shape[0]
  if curve:
    _check_cells(num_samples, n_rows, 'window totals are')
  threshold = _group_level(threshold, n_groups, name='threshold')
  if threshold is None and observed_count is not None:
    raise ValueError('observed_count needs a threshold')
  if not curve and observed_window is not None:
    raise ValueError('observed_window needs curve=True')
  observed = {'peak': _per_group('observed_peak', 'value', observed_peak, n_groups),
              'count': _per_group('observed_count', 'value', observed_count, n_groups)}
  if observed_window is not None:
    observed_window = np.ascontiguousarray(observed_window, dtype=np.float64)
    if observed_window.shape != (n_rows,):
      raise ValueError(f'observed_window must hold one value per row ({n_rows},); got {observed_window.shape}')
  with _sample_paths(features, observation_model, params, model_args, ensemble_dims, compute_dtype, weights,
                     seed) as (eng, loc, aux, seed64, kw):
    wi = eng.predictive_group_windows(loc, aux, seg_offsets, seg_rows, num_samples, seed64, window,
                                      threshold=threshold, windows=bool(curve), **kw)
    out = {'peak_probability': wi['peak_count'].cpu().numpy().astype(np.float64) / num_samples}
    for name in ('peak', 'count') if threshold is not None else ('peak',):
      y = None if observed[name] is None else torch.from_numpy(observed[name]).to(eng.device)
      for k, v in eng.sample_summaries(wi[name], y, levels).items():
        out[f'{name}_{k}'] = v.cpu().numpy()
    if curve:                                   # column = position: back to table rows through seg_rows
      pos_rows = np.asarray(seg_rows, dtype=np.int64)
      full = window_candidates(seg_offsets, seg_rows, n_rows, window)
      y = None
      if observed_window is not None:
        y_pos = np.full(pos_rows.shape, np.nan)
        y_pos[full] = observed_window[pos_rows[full]]
        y = torch.from_numpy(y_pos).to(eng.device)
      for k, v in eng.sample_summaries(wi['window'], y, levels).items():
        v = v.cpu().numpy()
        by_row = np.full(v.shape, np.nan)
        by_row[..., pos_rows[full]] = v[..., full]
        out[f'window_{k}'] = by_row
    if threshold is not None:
      out['exceed_probability'] = wi['exceed_count'].cpu().numpy().astype(np.float64) / num_samples
      out['any'] = (wi['count'] > 0).sum(dim=0).cpu().numpy().astype(np.float64) / num_samples
    return out


def band_need(coverage, num_samples):
  """The number of whole sample paths a simultaneous band of the given coverage must hold: ceil(coverage * num_samples),
  formed as ceil(coverage * num_samples - 1e-9) because a product such as 0.07 * 100 is 7.000000000000001 in float64, clamped to
  [1, num_samples].  coverage in (0, 1], ValueError otherwise."""
  try:
    c = float(coverage)
  except (TypeError, ValueError) as e:
    raise ValueError(f'coverage must be a number in (0, 1]; got {coverage!r}') from e
  if not 0.0 < c <= 1.0:
    raise ValueError(f'coverage must lie in (0, 1]; got {coverage!r}')
  num_samples = int(num_samples)
  if num_samples < 1:
    raise ValueError(f'num_samples={num_samples}: need at least one sample path')
  return max(1, min(num_samples, int(math.ceil(c * num_samples - 1e-9))))


def _coverage_levels(coverage):
  try:
    levels = [float(v) for v in coverage]
  except (TypeError, ValueError) as e:
    raise ValueError(f'coverage must be a sequence of numbers in (0, 1]; got {coverage!r}') from e
  if not levels or len(levels) > _native.BAND_MAX_LEVELS:
    raise ValueError(f'coverage: 1..{_native.BAND_MAX_LEVELS} levels; got {len(levels)}')
  if any(not 0.0 < v <= 1.0 for v in levels):
    raise ValueError(f'coverage must lie in (0, 1]; got {levels}')
  return levels


BAND_OF = ('rows', 'cumulative')


def band_summaries(features, observation_model, params, model_args, num_samples, seed, ensemble_dims, groups,
                   coverage=(0.9,), of='rows', observed=None, compute_dtype=None, weights=None):
  """SIMULTANEOUS bands of the joint sample paths, per group of rows, on the GPU (include/bnf.h bnf_sample_depths,
  bnf_depth_levels, bnf_sample_envelope): bands that hold a whole path over the rows of a group with probability
  `coverage`, where a quantile band holds each row alone -- the rank envelope: band k at a row is [x_(k), x_(S-1-k)] of the
  row's S sorted samples, and the level of a group is the largest k whose band still holds ceil(coverage S) of the paths
  (`band_need`) at EVERY row of the group.  groups = (seg_offsets, seg_rows);
    of='rows'         the curve of a group is the draws at its rows (`csr_from_codes`; a row in no group takes no part)
    of='cumulative'   the curve is the running total along the group's rows in TIME order (`csr_ordered`), as
                      `cumulative_summaries` forms it
  observed (n_rows,), per TABLE ROW: the observed value (of='cumulative': the observed running total) at the row, NaN
  where it takes no part.  -> dict of numpy arrays, n_cov = len(coverage):
    'level' (n_cov, G) int32                 the band level k* of the group; -1 for a group without rows and one with a NaN draw
    'coverage' (n_cov, G) float64            the share of the paths band k* holds whole: >= ceil(coverage S) / S
    'pointwise_joint_coverage' (n_cov, G)    the share of the paths that the POINTWISE band holds whole: band
                                             floor((S - need) / 2), which holds need samples at each row
    'lower', 'upper' (n_cov, n_rows) float64             the simultaneous band, values picked from the samples
    'pointwise_lower', 'pointwise_upper' (n_cov, n_rows) the pointwise band, for comparison
  per-row results are NaN at a row that takes no part and at one with a NaN draw, the simultaneous band also at every other
  row of that draw's group (its level is -1); with `observed`:
    'observed_depth' (G,) float64   the largest band level that still holds the observed curve at every scored row, -1 = it
                                    leaves the envelope of all paths; NaN for a group without an observed value
    'inside' (n_cov, G) float64     1.0 where the simultaneous band holds the observed curve, 0.0 where not, NaN as above
    'depth_pit' (2, G) float64      #{paths of depth <= the observed} / S and #{... <} / S: uniform between the two when the
                                    observed curve is exchangeable with the paths; small = more extreme than nearly all
  The matrix of curves is held whole: num_samples <= 16,384 and num_samples * n_rows <= 2^28 cells, ValueError beyond,
  like every check before any GPU work.  weights: member weights of the sample paths as in `sample_predictive`."""
  num_samples = _num_samples(num_samples, 'bands')
  levels = _coverage_levels(coverage)
  if of not in BAND_OF:
    raise ValueError(f"of={of!r}: 'rows' (the draws at the rows) or 'cumulative' (their running totals)")
  seg_offsets, seg_rows = groups
  n_groups = len(seg_offsets) - 1
  features = np.asarray(features, dtype=np.float64)
  n_rows = features.shape[0]
  if n_groups < 1:
    raise ValueError('groups: need at least one group')
  if of == 'cumulative' and len(seg_rows) != n_rows:
    raise ValueError(f"of='cumulative': seg_rows must hold one entry per row ({n_rows}); got {len(seg_rows)}")
  _check_cells(num_samples, n_rows, 'sample paths are')
  if observed is not None:
    observed = np.ascontiguousarray(observed, dtype=np.float64)
    if observed.shape != (n_rows,):
      raise ValueError(f'observed must hold one value per row ({n_rows},); got {observed.shape}')
  need = [band_need(v, num_samples) for v in levels]
  k_pw = [(num_samples - n) // 2 for n in need]
  pos_rows = np.asarray(seg_rows, dtype=np.int64)
  named = (pos_rows >= 0) & (pos_rows < n_rows)
  pos_group = np.repeat(np.arange(n_groups, dtype=np.int32), np.diff(np.asarray(seg_offsets, dtype=np.int64)))
  if pos_group.shape != pos_rows.shape:
    raise ValueError(f'groups: seg_offsets covers {pos_group.size} positions, seg_rows holds {pos_rows.size}')
  if of == 'rows':                              # column = table row
    col_group = np.full(n_rows, -1, dtype=np.int32)
    col_group[pos_rows[named]] = pos_group[named]
    y_col = observed
  else:                                         # column = position
    col_group = np.where(named, pos_group, np.int32(-1)).astype(np.int32)
    y_col = None
    if observed is not None:
      y_col = np.full(pos_rows.shape, np.nan)
      y_col[named] = observed[pos_rows[named]]
  with _sample_paths(features, observation_model, params, model_args, ensemble_dims, compute_dtype, weights,
                     seed) as (eng, loc, aux, seed64, kw):
    if of == 'rows':
      x = torch.empty((num_samples, n_rows), dtype=torch.float64, device=eng.device)
      chunk = max(1, _SAMPLE_CHUNK_CELLS // num_samples)
      for r0 in range(0, n_rows, chunk):
        r1 = min(n_rows, r0 + chunk)
        x[:, r0:r1] = eng.predictive_samples(loc[:, r0:r1], aux, num_samples, seed64, row0=r0, **kw)
    else:
      x = eng.predictive_group_cumulative(loc, aux, seg_offsets, seg_rows, num_samples, seed64, running=True, **kw)['running']
    cg = torch.from_numpy(col_group).to(eng.device)
    y = None if y_col is None else torch.from_numpy(y_col).to(eng.device)
    dep = eng.sample_depths(x, cg, n_groups, y)
    lev = eng.depth_levels(dep['depth'], need, k_pw, dep.get('obs_depth'))
    out = {'level': lev['level'].cpu().numpy(), 'coverage': lev['achieved'].cpu().numpy()}
    out['pointwise_joint_coverage'] = lev['joint'].cpu().numpy()          # row i: band k_pw[i], the one of coverage[i]
    pw_level = torch.from_numpy(np.repeat(np.asarray(k_pw, dtype=np.int32)[:, None], n_groups, axis=1)).to(eng.device)
    for prefix, lv in (('', lev['level']), ('pointwise_', pw_level)):
      env = eng.sample_envelope(x, cg, lv)
      for k in ('lower', 'upper'):
        v = env[k].cpu().numpy()
        if of == 'cumulative':                  # column = position: back to table rows through seg_rows
          by_row = np.full((v.shape[0], n_rows), np.nan)
          by_row[:, pos_rows[named]] = v[:, named]
          v = by_row
        out[prefix + k] = v
    if y is not None:
      od = dep['obs_depth'].cpu().numpy()
      seen = od != _native.DEPTH_NONE
      out['observed_depth'] = np.where(seen, od.astype(np.float64), np.nan)
      out['inside'] = np.where(seen[None, :], (od[None, :] >= out['level']).astype(np.float64), np.nan)
      out['depth_pit'] = lev['obs_pit'].cpu().numpy()
    return out


# ---------------------------------------------------------------------------
# scores of held-out observations
# ---------------------------------------------------------------------------
def score_predictive(features, target, observation_model, params, model_args, ensemble_dims, compute_dtype=None,
                     rps=False, weights=None):
  """Held-out observations `target` (n_rows,) scored against the ensemble on the GPU (include/bnf.h
  bnf_predictive_scores).  Every leading ensemble dim of `params` flattens to the M mixture components, exactly as in
  predict_bnf: equally weighted, or with `weights` (shape of the ensemble dims, `mixture_weights`; the weights
  `stack_members` returns) -- then 'log_density', 'pit', 'crps' and 'rps' are those of the weighted mixture
  (bnf_predictive_scores_weighted, bnf_count_rps_weighted) and 'member_log_prob' does not change.  NaN targets are allowed: their rows come back NaN and do not enter the
  per-member sums.  -> dict of numpy arrays:
    'log_density' (n_rows,) float32      log density of the mixture at the target
    'pit' (2, n_rows) float32            mixture CDF at the target and just below it (equal for NORMAL)
    'crps' (n_rows,) float32             NORMAL only
    'member_log_prob' lead dims, float64 every member's log density summed over the scored rows -- what
                                         `likelihood_model(...).log_prob(target)` gives on the host
    'rps' (n_rows,) float32              with rps=True, NB / ZINB only: the ranked probability score (the CRPS of a count
                                         forecast; include/bnf.h bnf_count_rps), NaN where the row's window is longer
                                         than BNF_RPS_MAX_TERMS"""
  if rps and observation_model == 'NORMAL':
    raise ValueError("rps=True is for the count observation models (NB, ZINB); the NORMAL model's score is 'crps'")
  features = np.asarray(features, dtype=np.float64)
  target = np.asarray(target, dtype=np.float64)
  n_rows = features.shape[0]
  if target.shape != (n_rows,):
    raise ValueError(f'target must hold one observation per row ({n_rows},); got {target.shape}')
  w, _ = mixture_weights(weights, params, ensemble_dims)
  kw = {} if w is None else {'weights': w}
  net, eng, lead, loc_all, aux_all = _ensemble_forecast(
      features, observation_model, params, model_args, ensemble_dims, compute_dtype)
  try:
    loc, aux, y32 = loc_all.reshape(-1, n_rows), aux_all.reshape(-1, 3), np.ascontiguousarray(target, dtype=np.float32)
    res = eng.predictive_scores(loc, aux, y32, **kw)
    out = {'log_density': res['lpd'].cpu().numpy(), 'pit': res['pit'].cpu().numpy(),
           'member_log_prob': res['member_ll'].cpu().numpy().reshape(tuple(lead))}
    if 'crps' in res:
      out['crps'] = res['crps'].cpu().numpy()
    if rps:
      out['rps'] = eng.count_rps(loc, aux, y32, **kw).cpu().numpy()
    return out
  finally:
    eng.close()


def stack_members(features, target, observation_model, params, model_args, ensemble_dims, weights=None, max_iter=10000,
                  tol=1e-5, compute_dtype=None):
  """Stacking of the members on held-out rows, on the GPU (include/bnf.h bnf_member_log_density, bnf_stacking_weights):
  the simplex weights over the M flattened members (VI: posterior draws count as components) that maximise the mean log
  density of `target` under the weighted mixture, found by EM from `weights` (None: equal weights) and stopped when
  gap = max_m g_m - 1 <= tol -- a bound on how far the objective is from its optimum -- or after max_iter updates.
  max_iter=0 evaluates `weights` as they are.  NaN targets are allowed: their rows are left out.  -> dict:
    'weights'          leading ensemble dims of `params`, float64
    'log_density'      (n_rows,) float32 log density of the weighted mixture; NaN rows NaN, dropped rows -inf
    'objective', 'objective_start'   mean log density over the scored rows at the returned / the starting weights
    'gap', 'iterations', 'converged', 'dropped'   dropped: rows to which every member with a positive weight gives the
                                                  density 0 (left out of the means)
  The weights are taken by the sample-path family (`sample_predictive`, `total_summaries`) and by the marginal forecast:
  the quantiles of predict_bnf and the log density / pit / crps / rps of score_predictive; fit is untouched."""
  w0, _ = mixture_weights(weights, params, ensemble_dims)
  max_iter = int(max_iter)
  tol = float(tol)
  if max_iter < 0 or not tol >= 0.0:
    raise ValueError(f'max_iter={max_iter}, tol={tol}: both must be >= 0')
  features = np.asarray(features, dtype=np.float64)
  target = np.asarray(target, dtype=np.float64)
  n_rows = features.shape[0]
  if target.shape != (n_rows,):
    raise ValueError(f'target must hold one observation per row ({n_rows},); got {target.shape}')
  net, eng, lead, loc_all, aux_all = _ensemble_forecast(
      features, observation_model, params, model_args, ensemble_dims, compute_dtype)
  try:
    loc, aux, y32 = loc_all.reshape(-1, n_rows), aux_all.reshape(-1, 3), np.ascontiguousarray(target, dtype=np.float32)
    res = eng.stacking_weights(eng.member_log_density(loc, aux, y32), w_init=w0, max_iter=max_iter, tol=tol)
    out = {k: res[k] for k in ('objective', 'objective_start', 'gap', 'iterations', 'converged', 'dropped')}
    out['weights'] = res['weights'].cpu().numpy().reshape(tuple(lead))
    out['log_density'] = res['lpd'].cpu().numpy()
    return out
  finally:
    eng.close()


def _quantile_engine(net, obs, compute_dtype):
  """Forward-only handle that owns the quantile kernels (bnf_*_mixture_quantiles)."""
  return Engine(net, mode='map', members=1, forward_only=True, row_capacity=128, compute_dtype=compute_dtype)


def _lead_weights(weights, lead):
  """Member weights of a likelihood object, shape of its ensemble dims `lead` -> (M,) float64 in member order."""
  w = np.asarray(weights, dtype=np.float64)
  if w.shape != tuple(lead):
    raise ValueError(f'weights must have the shape of the ensemble dims {tuple(lead)}; got {w.shape}')
  return np.ascontiguousarray(w.reshape(-1))


def _mixture_cdf(c, weights):
  """Per-member cdf c (*ens, R) -> the mixture's (R,): the mean over members, or the sum weighted by `weights` (*ens)."""
  if weights is None:
    return c.reshape(-1, c.shape[-1]).mean(axis=0)
  return _lead_weights(weights, c.shape[:-1]) @ c.reshape(-1, c.shape[-1])


class EnsembleLikelihood:
  """Stand-in for the TFP distribution returned by the reference's `likelihood_model`
  (spatiotemporal.py:433-468): Independent Normal per member with event shape (n_rows,) and
  batch shape = ensemble dims.  mean / stddev / log_prob / sample are per member (as TFP's);
  cdf is the per-member, per-row Normal cdf; mixture_cdf / quantile treat the ensemble as the
  equally weighted mixture `predict` reports quantiles of (inference.py:42-52), the root found
  on the GPU by the same kernel (`bnf_normal_mixture_quantiles`); with weights= (shape of the ensemble
  dims, on the simplex) as the weighted mixture (`bnf_normal_mixture_quantiles_weighted`)."""

  def __init__(self, loc: np.ndarray, scale: np.ndarray, net=None, compute_dtype=None):
    self.loc = loc                       # (*ens, R)
    self.scale = scale[..., None]        # (*ens, 1)
    self._net, self._dtype = net, compute_dtype

  def mean(self):
    return self.loc

  def stddev(self):
    return np.broadcast_to(self.scale, self.loc.shape)

  def log_prob(self, y):
    y = np.asarray(y, dtype=np.float64)
    z = (y - self.loc) / self.scale
    return np.sum(-0.5 * z * z - np.log(self.scale) - 0.5 * np.log(2 * np.pi), axis=-1)

  def cdf(self, x):
    from scipy import special as sp
    return sp.ndtr((np.asarray(x, dtype=np.float64) - self.loc) / self.scale)

  def mixture_cdf(self, x, weights=None):
    return _mixture_cdf(self.cdf(x), weights)

  def quantile(self, q, approximate=False, weights=None):
    """Mixture quantile(s) per row: q scalar -> (R,), sequence -> (len(q), R)."""
    kw = {} if weights is None else {'weights': _lead_weights(weights, self.loc.shape[:-1])}
    qs = np.atleast_1d(np.asarray(q, dtype=np.float64))
    eng = _quantile_engine(self._net, 'NORMAL', self._dtype)
    means = torch.from_numpy(np.ascontiguousarray(self.loc.reshape(-1, self.loc.shape[-1]), dtype=np.float32)).to(eng.device)
    scales = torch.from_numpy(np.ascontiguousarray(self.scale.reshape(-1), dtype=np.float32)).to(eng.device)
    out = eng.normal_mixture_quantiles(means, scales, qs.tolist(), approximate=approximate, **kw)
    torch.cuda.synchronize(eng.device)
    res = out.cpu().numpy().astype(np.float64)
    eng.close()
    return res[0] if np.ndim(q) == 0 else res

  def sample(self, seed=0):
    """One draw per member, on the host (numpy).  Joint draws of the mixture -- any number of sample paths, or their
    totals over groups of rows -- come from the GPU: `BayesianNeuralFieldEstimator.predict_samples`."""
    rng = np.random.default_rng(_native.seed_to_u64(seed))
    return self.loc + self.scale * rng.standard_normal(self.loc.shape)


class CountEnsembleLikelihood:
  """NB / ZINB counterpart (models.py:166-191): Independent (ZI)NegativeBinomial per member.
  total_count (*ens, 1), logits (*ens, R), inflated_loc_probs (*ens, 1) or None.  cdf /
  mixture_cdf / quantile as in EnsembleLikelihood; the integer quantile follows
  inference.py:298-333 (`bnf_count_mixture_quantiles`)."""

  def __init__(self, total_count, logits, inflated_loc_probs=None, net=None, compute_dtype=None, loc=None,
               aux=None):
    self.total_count = total_count[..., None]
    self.logits = logits
    self.inflated_loc_probs = None if inflated_loc_probs is None else inflated_loc_probs[..., None]
    self._net, self._dtype, self._loc, self._aux = net, compute_dtype, loc, aux

  def _nb_mean_var(self):
    mean = self.total_count * np.exp(self.logits)
    return mean, mean * (1.0 + np.exp(self.logits))       # mean / sigmoid(-logits)

  def mean(self):
    mean, _ = self._nb_mean_var()
    return mean if self.inflated_loc_probs is None else (1.0 - self.inflated_loc_probs) * mean

  def stddev(self):
    mean, var = self._nb_mean_var()
    if self.inflated_loc_probs is not None:
      pi = self.inflated_loc_probs
      var = (1.0 - pi) * (var + mean * mean) - ((1.0 - pi) * mean) ** 2
    return np.sqrt(var)

  def log_prob(self, y):
    from scipy import special as sp
    y = np.asarray(y, dtype=np.float64)
    tc, lg = self.total_count, self.logits
    lp = (tc * -np.logaddexp(lg, 0.0) + y * -np.logaddexp(-lg, 0.0) + sp.gammaln(tc + y) -
          sp.gammaln(1.0 + y) - sp.gammaln(tc))
    if self.inflated_loc_probs is not None:
      pi = self.inflated_loc_probs
      lp = np.where(y == 0, np.logaddexp(np.log1p(-pi) + lp, np.log(pi)), np.log1p(-pi) + lp)
    return np.sum(lp, axis=-1)

  def cdf(self, x):
    """P(Y <= x) per member and row (TFP: betainc(total_count, 1 + floor(x), sigmoid(-logits)))."""
    from scipy import special as sp
    x = np.floor(np.asarray(x, dtype=np.float64))
    tc = np.broadcast_to(self.total_count, self.logits.shape)
    c = np.where(x < 0, 0.0, sp.betainc(tc, 1.0 + np.maximum(x, 0.0), sp.expit(-self.logits)))
    if self.inflated_loc_probs is not None:
      c = np.where(x < 0, 0.0, self.inflated_loc_probs + (1.0 - self.inflated_loc_probs) * c)
    return c

  def mixture_cdf(self, x, weights=None):
    return _mixture_cdf(self.cdf(x), weights)

  def quantile(self, q, weights=None):
    kw = {} if weights is None else {'weights': _lead_weights(weights, self._loc.shape[:-1])}
    qs = np.atleast_1d(np.asarray(q, dtype=np.float64))
    eng = Engine(self._net, mode='map', members=1, forward_only=True, row_capacity=128, compute_dtype=self._dtype)
    loc = torch.from_numpy(np.ascontiguousarray(self._loc.reshape(-1, self._loc.shape[-1]), dtype=np.float32)).to(eng.device)
    aux = torch.from_numpy(np.ascontiguousarray(self._aux.reshape(-1, 3), dtype=np.float32)).to(eng.device)
    _, out = eng.count_mixture_quantiles(loc, aux, qs.tolist(), **kw)
    torch.cuda.synchronize(eng.device)
    res = out.cpu().numpy().astype(np.float64)
    eng.close()
    return res[0] if np.ndim(q) == 0 else res

  def sample(self, seed=0):
    """One draw per member, on the host (numpy).  Joint draws of the mixture -- any number of sample paths, or their
    totals over groups of rows -- come from the GPU: `BayesianNeuralFieldEstimator.predict_samples`."""
    rng = np.random.default_rng(_native.seed_to_u64(seed))
    shape = np.broadcast_shapes(self.total_count.shape, self.logits.shape)
    # NB(tc, p) as a Gamma-Poisson mixture: rate ~ Gamma(tc, scale = e^logits)
    rate = rng.gamma(np.broadcast_to(self.total_count, shape), np.exp(self.logits))
    draw = rng.poisson(rate).astype(np.float64)
    if self.inflated_loc_probs is not None:
      draw = np.where(rng.random(shape) < self.inflated_loc_probs, 0.0, draw)
    return draw


def likelihood_model(features, observation_model, params, model_args,
                     ensemble_dims=2, compute_dtype=None):
  features = np.asarray(features, dtype=np.float64)
  net, eng, lead, loc_all, aux_all = _ensemble_forecast(
      features, observation_model, params, model_args, ensemble_dims, compute_dtype)
  torch.cuda.synchronize(eng.device)
  n_rows = features.shape[0]
  loc = loc_all.cpu().numpy().reshape(tuple(lead) + (n_rows,)).astype(np.float64)
  aux = aux_all.cpu().numpy().reshape(tuple(lead) + (3,)).astype(np.float64)
  eng.close()
  if observation_model == 'NORMAL':
    return EnsembleLikelihood(loc, aux[..., 0], net=net, compute_dtype=compute_dtype)
  shape = aux[..., 1]
  logits = -np.log(shape)[..., None] - np.log(np.logaddexp(loc, 0.0))
  return CountEnsembleLikelihood(1.0 / shape, logits,
                                 aux[..., 2] if observation_model == 'ZINB' else None, net=net,
                                 compute_dtype=compute_dtype, loc=loc, aux=aux)
