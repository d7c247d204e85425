"""Thin Python owner of one `bnf_handle` and of the device buffers it uses.

torch-ROCm supplies device memory and the HIP stream; every computation is a
call into libbnf_hip.so through ctypes (`_native`).  No computation here.
"""

from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import _native
from . import distributed
from .spec import NetSpec


_warned_default_dtype = False


def default_dtype(compute_dtype=None) -> str:
  """Canonical name of the engine arithmetic.
  'fp32' (= 'f32', 'float32', 'fp32_exact'; include/bnf.h BNF_DTYPE_F32): f32 storage, accumulation and epilogues,
  contractions on the exact `v_mfma_f32_32x32x2_f32` -- an explicit 'fp32' always means this.
  'fp32_split' (= 'bf16x3'; BNF_DTYPE_F32S): the same storage and epilogues, every contraction as three bf16 MFMAs on
  operands split in registers (16 operand bits, ~5e-6 per contraction where the exact chain measures 1e-7), 1.8x the exact
  chain.  WHAT THE ESTIMATORS RUN WHEN NOTHING IS SAID (compute_dtype=None and no BNF_DTYPE): both f32-class engines hold
  SURVEY 8d's fp32 gates verbatim -- forward / loss 1e-5, gradients 1e-4, parameters after 100 full-batch Adam steps 1e-3 on
  the C2 and C4 layouts (tests/util.py FP32_GATE; measured profiles/r06_fp32_contract_diag.txt: split 3.1e-6 / 2.4e-7 /
  7.7e-5 / 2.7e-5) -- and both reproduce the reference's golden predictions to < 1e-4, so the default is the faster one
  (the condition VERDICT r05 item 2 set for keeping it); the once-per-process warning below says so.
  'bf16': the throughput path (bf16 contraction operands, f32 accumulation -- the numerics class of the reference's TPU
  runs; ~6x the exact chain at the benchmark size).  'fp8' = 'bf16' with FP8 OPERAND STORAGE for the weight-gradient
  contractions and, on the folded two-layer row-panel forms, the W x W forward / backward-data contractions on the fp8 MFMA
  (include/bnf.h BNF_DTYPE_FP8; training handles on the row-panel pipeline only -- a forward-only handle of an 'fp8'
  estimator runs the bf16 forward)."""
  global _warned_default_dtype
  if compute_dtype is None and 'BNF_DTYPE' not in os.environ and not _warned_default_dtype:
    _warned_default_dtype = True
    import warnings
    warnings.warn("bayesnf_amd: compute_dtype defaults to 'fp32_split' (f32 storage and epilogues, contractions as three "
                  "split-bf16 MFMAs: within SURVEY 8d's fp32 gates, 1.8x the exact chain). Pass compute_dtype='fp32' for the exact "
                  "f32 MFMA chain, 'bf16' (~3.5x faster again) or 'fp8' -- or set BNF_DTYPE.", stacklevel=3)
  dt = compute_dtype or os.environ.get('BNF_DTYPE', 'fp32_split')
  if dt not in _native.DTYPE:
    raise ValueError(f'compute_dtype must be one of {sorted(_native.DTYPE)}')
  return _native.DTYPE_NAME[_native.DTYPE[dt]]


def _ptr(t):
  return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def group_work_bytes(bytes_per_tile, R, n_samples):
  """Size in bytes of the work buffer of a group reduction over R rows (include/bnf.h bnf_predictive_group_*): the
  per-tile pieces of `bytes_per_tile` bytes per tile and path, for every path up to ~64 MB and for one path at least
  (the library makes several passes beyond that)."""
  per_path = bytes_per_tile * (-(-R // _native.GROUP_TILE))
  return per_path * max(1, min(n_samples, (64 << 20) // per_path))


class Engine:
  """One GPU's share of an ensemble: `members` networks trained side by side.

  mode 'map' (MAP / MLE via prior_weight) or 'vi'.  X (N, D) and y (N,) are
  copied to the device once, as float32 (what `jnp.array` does with x64 off,
  reference inference.py:553-554).
  """

  def __init__(self, net: NetSpec, *, mode='map', X=None, y=None, batch=None,
               members=1, member_offset=0, seed=0, learning_rate=0.005,
               prior_weight=1.0, kl_weight=1.0, vi_samples=1,
               compute_dtype=None, forward_only=False, row_capacity=None,
               device_index=None, pipeline='auto'):
    self.lib = _native.load()
    if not torch.cuda.is_available():
      raise RuntimeError(
          'bayesnf_amd: no GPU visible (torch.cuda.is_available() is False). '
          'The engine is HIP-only; there is no CPU fallback.')
    self.net = net
    self.mode = mode
    self.dtype = default_dtype(compute_dtype)
    # default device: the first one this process drives (LOCAL_RANK's under torch.distributed, else the first of
    # BNF_DEVICES / of the visible devices) -- the same list fit() / predict() deal members over
    self.dev_index = (distributed.local_devices()[0]
                      if device_index is None else int(device_index))
    self.device = torch.device(f'cuda:{self.dev_index}')
    torch.cuda.set_device(self.device)
    self.members = int(members)
    self.member_offset = int(member_offset)
    self.forward_only = bool(forward_only)
    if forward_only:
      n_rows = batch = int(row_capacity)
      self.X = self.y = None
    else:
      X = np.ascontiguousarray(np.asarray(X, dtype=np.float64), dtype=np.float32)
      y = np.ascontiguousarray(np.asarray(y, dtype=np.float64), dtype=np.float32)
      n_rows = X.shape[0]
      batch = n_rows if batch is None else int(batch)
      self.X = torch.from_numpy(X).to(self.device)
      self.y = torch.from_numpy(y).to(self.device)
    self.n_rows, self.batch = n_rows, batch
    self.S = int(vi_samples) if mode == 'vi' else 1
    cfg = _native.make_config(
        net, device=self.dev_index, dtype=self.dtype,
        mode=_native.MODE_VI if mode == 'vi' else _native.MODE_MAP,
        n_rows=n_rows, batch=batch, members=members,
        member_offset=member_offset, seed=_native.seed_to_u64(seed),
        learning_rate=learning_rate, prior_weight=prior_weight,
        kl_weight=kl_weight, vi_samples=self.S, forward_only=forward_only,
        pipeline=pipeline)
    self.cfg = cfg
    handle = C.c_void_p()
    _native.check(self.lib.bnf_create(C.byref(cfg), C.byref(handle)), 'bnf_create')
    self.handle = handle
    ws_bytes = self.lib.bnf_workspace_bytes(handle)
    self.workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
    if forward_only:
      self.params = self.state = None
    else:
      self.params = torch.empty(self.lib.bnf_param_bytes(handle) // 4,
                                dtype=torch.float32, device=self.device)
      self.state = torch.empty(self.lib.bnf_state_bytes(handle) // 4,
                               dtype=torch.float32, device=self.device)
    self.stream = torch.cuda.current_stream(self.device)
    _native.check(
        self.lib.bnf_bind(handle, _ptr(self.params), _ptr(self.state),
                          _ptr(self.workspace), _ptr(self.X), _ptr(self.y),
                          C.c_void_p(self.stream.cuda_stream)), 'bnf_bind')

  def owned_bytes(self) -> int:
    """Device memory the engine allocated itself (include/bnf.h bnf_owned_bytes): the row-key work buffers."""
    return int(self.lib.bnf_owned_bytes(self.handle))

  # -- lifecycle ---------------------------------------------------------------
  def close(self):
    if getattr(self, 'handle', None) is not None:
      torch.cuda.synchronize(self.device)
      self.lib.bnf_destroy(self.handle)
      self.handle = None
      self.workspace = None

  def __del__(self):
    try:
      self.close()
    except Exception:  # pylint: disable=broad-except
      pass

  # -- training ----------------------------------------------------------------
  def init_params(self, log_noise_init: float):
    _native.check(self.lib.bnf_init_params(self.handle, C.c_float(log_noise_init)),
                  'bnf_init_params')

  def init_params_keys(self, leaf_keys, log_noise_init: float = 0.0):
    """The reference's own initial parameters (VI: surrogate means) drawn on the device from the members' per-leaf
    keys (include/bnf.h bnf_init_params_keys): uint32 (members, n_leaves, 2) from jaxseed.map_leaf_keys /
    vi_mean_leaf_keys."""
    from . import jaxseed
    k = np.ascontiguousarray(leaf_keys, dtype=np.uint32)
    n_leaves = len(self.net.leaves)
    if k.shape != (self.members, n_leaves, 2):
      raise ValueError(f'leaf keys must be uint32 ({self.members}, {n_leaves}, 2); got {k.shape}')
    t = torch.from_numpy(k.view(np.int32)).to(self.device)
    off = jaxseed.leaf_offsets(self.net)
    arr = (C.c_int32 * len(off))(*[int(v) for v in off])
    _native.check(self.lib.bnf_init_params_keys(self.handle, _ptr(t), arr, n_leaves, float(log_noise_init)),
                  'bnf_init_params_keys')
    torch.cuda.synchronize(self.device)     # `t` is released on return

  def set_params(self, theta):
    """theta: array (members, P) [MAP] or (2, members, P) = (mu, rho) [VI]."""
    t = torch.as_tensor(np.ascontiguousarray(theta, dtype=np.float32))
    self.params.copy_(t.reshape(-1).to(self.device))

  def set_targets(self, y):
    """New targets y (N,) for the rows bound at construction: overwrites the device copy in place (every step gathers
    its batch's targets from it)."""
    t = torch.as_tensor(np.ascontiguousarray(np.asarray(y, dtype=np.float64), dtype=np.float32))
    if self.y is None or t.shape != self.y.shape:
      raise ValueError(f'targets must have shape {None if self.y is None else tuple(self.y.shape)}; got {tuple(t.shape)}')
    self.y.copy_(t.to(self.device))

  def get_params(self) -> np.ndarray:
    p = self.params.detach().cpu().numpy()
    if self.mode == 'vi':
      return p.reshape(2, self.members, self.net.P)
    return p.reshape(self.members, self.net.P)

  def train(self, epoch0: int, num_epochs: int) -> torch.Tensor:
    """Enqueue the whole optimisation; returns the (members, num_epochs) loss
    tensor on the device (valid after a stream sync)."""
    losses = torch.zeros((self.members, num_epochs), dtype=torch.float32,
                         device=self.device)
    if num_epochs > 0:
      _native.check(self.lib.bnf_train(self.handle, int(epoch0), int(num_epochs),
                                       _ptr(losses)), 'bnf_train')
    return losses

  def validation_check(self, member_ll, n_scored, epoch, check, n_checks, curve, best_score, best_epoch, keep,
                       best_params):
    """One held-out check of a MAP / MLE fit (include/bnf.h bnf_validation_check), enqueued on the handle's stream
    without waiting: member_ll (members,) f64 as `predictive_scores` writes it for the held-out rows, n_scored of which
    have a finite target; column `check` of curve (members, n_checks) f64 receives member_ll / n_scored, and where that
    is the member's best so far (check 0: always) keep (members,) int32 is 1, best_score (members,) f64 and best_epoch
    (members,) int64 are updated and the member's row of the training parameters is copied to best_params (members, P)
    f32.  All device tensors, owned by the caller."""
    E = self.members
    for name, t, dtype, shape in (('member_ll', member_ll, torch.float64, (E,)), ('curve', curve, torch.float64, (E, int(n_checks))),
                                  ('best_score', best_score, torch.float64, (E,)), ('best_epoch', best_epoch, torch.int64, (E,)),
                                  ('keep', keep, torch.int32, (E,)), ('best_params', best_params, torch.float32, (E, self.net.P))):
      if t is not None and (t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != self.device):
        raise ValueError(f'{name} must be a contiguous {dtype} tensor of shape {shape} on {self.device}; got '
                         f'{t.dtype} {tuple(t.shape)} on {t.device}')
    _native.check(self.lib.bnf_validation_check(
        self.handle, _ptr(member_ll), int(n_scored), int(epoch), int(check), int(n_checks), _ptr(curve), _ptr(best_score),
        _ptr(best_epoch), _ptr(keep), _ptr(best_params)), 'bnf_validation_check')

  def set_row_tables(self, tables, epoch0=0):
    """Epoch shuffles supplied by the caller (include/bnf.h bnf_row_tables): int32 (n_epochs, members,
    (N // batch) * batch) row ids for the epochs [epoch0, epoch0 + n_epochs); uploaded and kept alive
    here (together with the previous chunk, which may still be executing).  None restores the engine's
    own shuffle."""
    if tables is None:
      self._row_tables = []
      _native.check(self.lib.bnf_row_tables(self.handle, None, 0, 0), 'bnf_row_tables')
      return
    t = tables if isinstance(tables, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(tables, dtype=np.int32))
    t = t.to(self.device, non_blocking=True).contiguous()
    keep = (self.n_rows // self.batch) * self.batch
    if t.dtype != torch.int32 or t.dim() != 3 or t.shape[1] != self.members or t.shape[2] != keep:
      raise ValueError(f'row tables must be int32 (n_epochs, {self.members}, {keep}); got {tuple(t.shape)} {t.dtype}')
    self._row_tables = (getattr(self, '_row_tables', []) + [t])[-2:]
    _native.check(self.lib.bnf_row_tables(self.handle, _ptr(t), int(epoch0), int(t.shape[0])), 'bnf_row_tables')

  def set_row_keys(self, subkeys, epoch0=0):
    """The reference's epoch shuffles drawn on the device (include/bnf.h bnf_row_keys): uint32 (n_epochs, members,
    rounds, 2) sub keys of `jax.random.permutation`'s sort rounds (jaxseed.map_shuffle_subkeys) for the epochs
    [epoch0, epoch0 + n_epochs); uploaded and kept alive here.  None switches it off."""
    if subkeys is None:
      self._row_keys = None
      _native.check(self.lib.bnf_row_keys(self.handle, None, 0, 0, 0), 'bnf_row_keys')
      return
    k = np.ascontiguousarray(subkeys, dtype=np.uint32)
    per = 1 if self.mode == 'vi' else self.members     # VI: one batch per step, shared by every member (jaxseed.vi_batch_subkeys)
    if k.ndim != 4 or k.shape[1] != per or k.shape[3] != 2:
      raise ValueError(f'row keys must be uint32 (n_epochs, {per}, rounds, 2); got {k.shape}')
    t = torch.from_numpy(k.view(np.int32)).to(self.device)
    self._row_keys = t
    _native.check(self.lib.bnf_row_keys(self.handle, _ptr(t), int(epoch0), int(k.shape[0]), int(k.shape[2])), 'bnf_row_keys')

  def vi_posterior_draws(self, n_draws: int) -> torch.Tensor:
    out = torch.empty((n_draws, self.members, self.net.P), dtype=torch.float32,
                      device=self.device)
    _native.check(self.lib.bnf_vi_posterior_draws(self.handle, int(n_draws), _ptr(out)),
                  'bnf_vi_posterior_draws')
    return out

  # -- prediction --------------------------------------------------------------
  def forward(self, theta: torch.Tensor, Xnew: torch.Tensor):
    """theta (M, P) f32 device, Xnew (R, D) f32 device -> loc (M, R), aux (M, 3)."""
    theta = theta.contiguous()
    Xnew = Xnew.contiguous()
    M, R = theta.shape[0], Xnew.shape[0]
    loc = torch.empty((M, R), dtype=torch.float32, device=self.device)
    aux = torch.empty((M, 3), dtype=torch.float32, device=self.device)
    _native.check(self.lib.bnf_forward(self.handle, _ptr(theta), M, _ptr(Xnew), R,
                                       _ptr(loc), _ptr(aux)), 'bnf_forward')
    return loc, aux

  def _kept(self, weights, per_member, per_row):
    """Member weights (M,) for the *_weighted entry points -> (w, per_member, per_row) on the device without the members
    of weight exactly 0 (a device index_select along dim 0): such a member plays no part at all -- it neither widens a
    quantile bracket or an RPS window nor hands on a NaN.  The weights are taken as they come (`inference.mixture_weights`
    validates them); weights that are all zero are a ValueError."""
    M = per_row.shape[0]
    w = self._as_f64(weights, (M,), 'weights')
    keep = torch.nonzero(w != 0).flatten()
    if keep.numel() == 0:
      raise ValueError('weights: every member has weight 0')
    if keep.numel() == M:
      return w, per_member, per_row
    return (w.index_select(0, keep).contiguous(), per_member.index_select(0, keep).contiguous(),
            per_row.index_select(0, keep).contiguous())

  def normal_mixture_quantiles(self, means: torch.Tensor, scales: torch.Tensor,
                               quantiles, approximate=False, weights=None) -> torch.Tensor:
    """means (M, R), scales (M,) -> (n_q, R).  weights (M,) array or device tensor: the quantiles of the mixture
    sum_m w_m N(mu_m, s_m) (bnf_normal_mixture_quantiles_weighted) after the members of weight 0 are dropped; None: the
    equal-weight call, bit for bit."""
    means = means.contiguous().float()
    scales = scales.contiguous().float()
    q = np.asarray(list(quantiles), dtype=np.float32)
    out = torch.empty((len(q), means.shape[1]), dtype=torch.float32, device=self.device)
    qa = (C.c_float * len(q))(*q.tolist())
    if weights is None:
      _native.check(self.lib.bnf_normal_mixture_quantiles(
          self.handle, _ptr(means), _ptr(scales), means.shape[0], means.shape[1], qa,
          len(q), 1 if approximate else 0, _ptr(out)), 'bnf_normal_mixture_quantiles')
      return out
    w, scales, means = self._kept(weights, scales, means)
    _native.check(self.lib.bnf_normal_mixture_quantiles_weighted(
        self.handle, _ptr(means), _ptr(scales), _ptr(w), means.shape[0], means.shape[1], qa,
        len(q), 1 if approximate else 0, _ptr(out)), 'bnf_normal_mixture_quantiles_weighted')
    torch.cuda.synchronize(self.device)     # `w` and the kept members' copies are released on return
    return out

  def count_mixture_quantiles(self, loc: torch.Tensor, aux: torch.Tensor, quantiles, weights=None):
    """NB / ZINB: loc (M, R) network output, aux (M, 3) -> (means (M, R), quantiles (n_q, R)).  weights (M,) array or
    device tensor: the quantiles of the weighted mixture (bnf_count_mixture_quantiles_weighted) after the members of
    weight 0 are dropped; the per-member means are those of every member either way.  None: the equal-weight call."""
    loc = loc.contiguous().float()
    aux = aux.contiguous().float()
    q = np.asarray(list(quantiles), dtype=np.float32)
    means = torch.empty_like(loc)
    out = torch.empty((len(q), loc.shape[1]), dtype=torch.float32, device=self.device)
    qa = (C.c_float * max(1, len(q)))(*q.tolist())
    if weights is None:
      _native.check(self.lib.bnf_count_mixture_quantiles(
          self.handle, _ptr(loc), _ptr(aux), loc.shape[0], loc.shape[1], qa, len(q),
          _ptr(means), _ptr(out)), 'bnf_count_mixture_quantiles')
      return means, out
    w, kaux, kloc = self._kept(weights, aux, loc)
    kmeans = means
    if kloc.shape[0] != loc.shape[0]:       # the means of all members: the unweighted call without levels
      _native.check(self.lib.bnf_count_mixture_quantiles(
          self.handle, _ptr(loc), _ptr(aux), loc.shape[0], loc.shape[1], qa, 0, _ptr(means), None),
          'bnf_count_mixture_quantiles')
      kmeans = torch.empty_like(kloc)
    _native.check(self.lib.bnf_count_mixture_quantiles_weighted(
        self.handle, _ptr(kloc), _ptr(kaux), _ptr(w), kloc.shape[0], kloc.shape[1], qa, len(q),
        _ptr(kmeans), _ptr(out)), 'bnf_count_mixture_quantiles_weighted')
    torch.cuda.synchronize(self.device)     # `w` and the kept members' copies are released on return
    return means, out

  def _cum(self, cum_weights, M):
    """cum_weights (M,) -> f64 device tensor (None stays None: the equal-weight call)."""
    if cum_weights is None:
      return None
    return self._as_f64(cum_weights, (M,), 'cum_weights')

  def predictive_samples(self, loc: torch.Tensor, aux: torch.Tensor, n_samples: int, seed, row0=0,
                         sample0=0, cum_weights=None) -> torch.Tensor:
    """Posterior-predictive sample paths (include/bnf.h bnf_predictive_samples): loc (M, R), aux (M, 3) as `forward`
    returns them -> (n_samples, R) f32 on the device.  Path s draws one member for all rows, then every row from that
    member's observation model.  row0 / sample0: global index of loc's first column / of the first path -- the values
    are a pure function of (seed, path, global row), so chunks of any size reproduce the one big call.
    cum_weights (M,) f64: the running sum of member weights (nondecreasing, last entry 1; bnf_predictive_samples_weighted):
    path s draws member #{m : cum[m] <= u} instead of floor(u M).  None: the equal-weight call, bit for bit."""
    loc = loc.contiguous().float()
    aux = aux.contiguous().float()
    M, R = loc.shape
    out = torch.empty((int(n_samples), R), dtype=torch.float32, device=self.device)
    if cum_weights is None:
      _native.check(self.lib.bnf_predictive_samples(
          self.handle, _ptr(loc), _ptr(aux), M, R, int(n_samples), C.c_uint64(_native.seed_to_u64(seed)), int(row0),
          int(sample0), _ptr(out)), 'bnf_predictive_samples')
      return out
    cum = self._cum(cum_weights, M)
    _native.check(self.lib.bnf_predictive_samples_weighted(
        self.handle, _ptr(loc), _ptr(aux), M, R, int(n_samples), C.c_uint64(_native.seed_to_u64(seed)), int(row0),
        int(sample0), _ptr(cum), _ptr(out)), 'bnf_predictive_samples_weighted')
    torch.cuda.synchronize(self.device)     # the device copy of `cum_weights` is released on return
    return out

  def predictive_group_sums(self, loc: torch.Tensor, aux: torch.Tensor, seg_offsets, seg_rows, n_samples: int, seed,
                            row0=0, sample0=0, cum_weights=None) -> torch.Tensor:
    """Totals of the same sample paths over groups of rows (include/bnf.h bnf_predictive_group_sums) -> (n_samples, G)
    f64 on the device, without materialising the draws.  The rows come sorted by group as CSR: seg_offsets (G + 1),
    seg_rows (R) int32 (`inference.csr_from_codes`).  Deterministic: the same call gives the same bits.
    cum_weights as for `predictive_samples` (bnf_predictive_group_sums_weighted); None: the equal-weight call."""
    loc, aux, off, rows, M, R, G = self._group_inputs(loc, aux, seg_offsets, seg_rows)
    n_samples = int(n_samples)
    out = torch.empty((n_samples, G), dtype=torch.float64, device=self.device)
    work = self._group_work(16, R, n_samples)       # per-tile partial sums: two doubles per tile and path
    if cum_weights is None:
      _native.check(self.lib.bnf_predictive_group_sums(
          self.handle, _ptr(loc), _ptr(aux), M, R, _ptr(off), _ptr(rows), G, n_samples,
          C.c_uint64(_native.seed_to_u64(seed)), int(row0), int(sample0), _ptr(work), C.c_size_t(work.numel()),
          _ptr(out)), 'bnf_predictive_group_sums')
    else:
      cum = self._cum(cum_weights, M)
      _native.check(self.lib.bnf_predictive_group_sums_weighted(
          self.handle, _ptr(loc), _ptr(aux), M, R, _ptr(off), _ptr(rows), G, n_samples,
          C.c_uint64(_native.seed_to_u64(seed)), int(row0), int(sample0), _ptr(cum), _ptr(work),
          C.c_size_t(work.numel()), _ptr(out)), 'bnf_predictive_group_sums_weighted')
    torch.cuda.synchronize(self.device)     # `work`, `off` and `rows` are released on return
    return out

  def predictive_combinations(self, loc: torch.Tensor, aux: torch.Tensor, form_offsets, form_rows, form_coef,
                              n_samples: int, seed, row0=0, sample0=0, cum_weights=None) -> torch.Tensor:
    """Linear combinations of the rows of the same sample paths (include/bnf.h bnf_predictive_combinations) ->
    (n_samples, K) f64 on the device, without materialising the draws: out[s][k] = sum_p form_coef[p] * draw(s,
    form_rows[p]) over the positions of form k.  form_offsets (K + 1) int32, form_rows (nnz) int32, form_coef (nnz) f64:
    a CSR over positions (`inference.combinations_csr`); a row may occur at many positions or at none, an empty form is
    0.  Deterministic: the same call gives the same bits; forms that partition the rows with coefficients 1 give the bits
    of `predictive_group_sums`.  cum_weights as for `predictive_samples`; None: equal weights."""
    loc = loc.contiguous().float()
    aux = aux.contiguous().float()
    M, R = loc.shape
    as_i32 = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))
                        ).to(self.device, dtype=torch.int32).contiguous()
    off, rows = as_i32(form_offsets), as_i32(form_rows)
    coef = self._as_f64(form_coef, None, 'form_coef')
    K, nnz = off.numel() - 1, rows.numel()
    if K < 1 or off.dim() != 1 or rows.dim() != 1 or tuple(coef.shape) != (nnz,):
      raise ValueError(f'form_offsets needs >= 2 entries and form_rows, form_coef one entry per position; got '
                       f'{tuple(off.shape)}, {tuple(rows.shape)}, {tuple(coef.shape)}')
    # the library takes the position count from form_offsets: it must be the arrays' length (read on the host when the
    # offsets arrive there, else 4 bytes back from the device)
    end = int(off[-1].item()) if isinstance(form_offsets, torch.Tensor) else int(np.asarray(form_offsets).reshape(-1)[-1])
    if end != nnz:
      raise ValueError(f'form_offsets ends at {end}; form_rows and form_coef hold {nnz} positions')
    n_samples = int(n_samples)
    out = torch.empty((n_samples, K), dtype=torch.float64, device=self.device)
    # per-tile partial sums: two doubles per tile of positions and path.  Arrays without a position have no device
    # address: one spare entry keeps every pointer the library checks non-NULL.
    work = self._group_work(16, max(nnz, 1), n_samples)
    if nnz == 0:
      rows, coef = rows.new_zeros(1), coef.new_zeros(1)
    cum = self._cum(cum_weights, M)
    _native.check(self.lib.bnf_predictive_combinations(
        self.handle, _ptr(loc), _ptr(aux), M, R, _ptr(off), _ptr(rows), _ptr(coef), K, n_samples,
        C.c_uint64(_native.seed_to_u64(seed)), int(row0), int(sample0), _ptr(cum), _ptr(work),
        C.c_size_t(work.numel()), _ptr(out)), 'bnf_predictive_combinations')
    torch.cuda.synchronize(self.device)     # `work`, `off`, `rows`, `coef` and `cum` are released on return
    return out

  def _group_inputs(self, loc, aux, seg_offsets, seg_rows):
    """The inputs the group reductions share, normalised -> (loc (M, R) f32, aux f32, seg_offsets (G + 1,) int32,
    seg_rows (R,) int32, M, R, G), all contiguous on the device."""
    loc = loc.contiguous().float()
    aux = aux.contiguous().float()
    M, R = loc.shape
    as_i32 = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))
                        ).to(self.device, dtype=torch.int32).contiguous()
    off, rows = as_i32(seg_offsets), as_i32(seg_rows)
    G = off.numel() - 1
    if G < 1 or rows.numel() != R:
      raise ValueError(f'seg_offsets needs >= 2 entries and seg_rows one entry per row ({R}); got {off.numel()}, {rows.numel()}')
    return loc, aux, off, rows, M, R, G

  def _row_threshold(self, threshold, R):
    """threshold (R,) -> f32 device tensor, one limit per table row."""
    thr = (threshold if isinstance(threshold, torch.Tensor)
           else torch.from_numpy(np.ascontiguousarray(threshold, dtype=np.float32))).to(self.device, dtype=torch.float32).contiguous()
    if tuple(thr.shape) != (R,):
      raise ValueError(f'threshold must hold one limit per row ({R},); got {tuple(thr.shape)}')
    return thr

  def _group_work(self, bytes_per_tile, R, n_samples):
    """The work buffer of a group reduction (`group_work_bytes`); its numel() is the byte count the library takes."""
    return torch.empty(group_work_bytes(bytes_per_tile, R, n_samples), dtype=torch.uint8, device=self.device)

  def predictive_group_extremes(self, loc: torch.Tensor, aux: torch.Tensor, seg_offsets, seg_rows, n_samples: int, seed,
                                threshold=None, row0=0, sample0=0, cum_weights=None, per_row=True) -> dict:
    """Peaks and threshold exceedances of the same sample paths over groups of rows (include/bnf.h
    bnf_predictive_group_extremes), without materialising the draws; loc, aux, seg_offsets, seg_rows, row0, sample0 and
    cum_weights as for `predictive_group_sums`.  -> dict of device tensors:
      'max' (n_samples, G) f64       the largest draw over the group's rows (a NaN draw counts as -inf)
      'argmax' (n_samples, G) int32  the table row at which it is first reached: ties go to the lowest position of seg_rows
      'count' (n_samples, G) f64     with `threshold` (R,) f32, one limit per table row: the rows whose draw is > their limit
      'peak_count' (R,) int32        per_row=True: the paths in which the row is its group's argmax
      'exceed_count' (R,) int32      per_row=True with `threshold`: the paths whose draw at the row is > its limit
    A group without rows gives max NaN, argmax -1, count 0.  Deterministic: the same call gives the same bits."""
    loc, aux, off, rows, M, R, G = self._group_inputs(loc, aux, seg_offsets, seg_rows)
    thr = None if threshold is None else self._row_threshold(threshold, R)
    n_samples = int(n_samples)
    out = {'max': torch.empty((n_samples, G), dtype=torch.float64, device=self.device),
           'argmax': torch.empty((n_samples, G), dtype=torch.int32, device=self.device)}
    if thr is not None:
      out['count'] = torch.empty((n_samples, G), dtype=torch.float64, device=self.device)
    if per_row:                             # the library adds to these: zeroed here
      out['peak_count'] = torch.zeros((R,), dtype=torch.int32, device=self.device)
      if thr is not None:
        out['exceed_count'] = torch.zeros((R,), dtype=torch.int32, device=self.device)
    work = self._group_work(_native.EXTREMES_WORK_PER_TILE, R, n_samples)
    cum = self._cum(cum_weights, M)
    _native.check(self.lib.bnf_predictive_group_extremes(
        self.handle, _ptr(loc), _ptr(aux), M, R, _ptr(off), _ptr(rows), G, n_samples,
        C.c_uint64(_native.seed_to_u64(seed)), int(row0), int(sample0), _ptr(cum), _ptr(thr), _ptr(work),
        C.c_size_t(work.numel()), _ptr(out['max']), _ptr(out['argmax']), _ptr(out.get('count')),
        _ptr(out.get('peak_count')), _ptr(out.get('exceed_count'))), 'bnf_predictive_group_extremes')
    torch.cuda.synchronize(self.device)     # `work`, `off`, `rows`, `thr` and `cum` are released on return
    return out

  def predictive_group_episodes(self, loc: torch.Tensor, aux: torch.Tensor, seg_offsets, seg_rows, n_samples: int, seed,
                                threshold, cum_weights=None, per_row=True, row0=0, sample0=0) -> dict:
    """Spells above a threshold in the same sample paths, per group of rows (include/bnf.h
    bnf_predictive_group_episodes), without materialising the draws; loc, aux, seg_offsets, seg_rows, row0, sample0 and
    cum_weights as for `predictive_group_sums`.  TIME is the order of the positions of seg_rows inside a group
    (`inference.csr_ordered`).  threshold (R,) f32, one limit per table row: a position exceeds when its draw is > its
    limit; a NaN draw does not exceed but breaks a spell and counts as a step; an entry of seg_rows outside [0, R) takes
    no part.  -> dict of device tensors:
      'longest' (n_samples, G) f64        length of the longest run of consecutive exceeding positions, 0 if none
      'longest_row' (n_samples, G) int32  the table row at which it starts (the earliest of equally long runs), -1 if none
      'spells' (n_samples, G) f64         the number of maximal runs
      'onset_step' (n_samples, G) f64     participating positions before the first exceeding one; all of them if none
      'first_row', 'last_row' (n_samples, G) int32   table row of the first / last exceeding position, -1 if none
      'onset_count' (R,) int32            per_row=True: the paths in which the row is its group's first exceeding row
    Deterministic: the same call gives the same bits."""
    loc, aux, off, rows, M, R, G = self._group_inputs(loc, aux, seg_offsets, seg_rows)
    if threshold is None:
      raise ValueError('threshold is required: one limit per row')
    thr = self._row_threshold(threshold, R)
    n_samples = int(n_samples)
    f64 = lambda: torch.empty((n_samples, G), dtype=torch.float64, device=self.device)
    i32 = lambda: torch.empty((n_samples, G), dtype=torch.int32, device=self.device)
    out = {'longest': f64(), 'longest_row': i32(), 'spells': f64(), 'onset_step': f64(), 'first_row': i32(),
           'last_row': i32()}
    if per_row:                             # the library adds to it: zeroed here
      out['onset_count'] = torch.zeros((R,), dtype=torch.int32, device=self.device)
    work = self._group_work(_native.EPISODES_WORK_PER_TILE, R, n_samples)
    cum = self._cum(cum_weights, M)
    _native.check(self.lib.bnf_predictive_group_episodes(
        self.handle, _ptr(loc), _ptr(aux), M, R, _ptr(off), _ptr(rows), G, n_samples,
        C.c_uint64(_native.seed_to_u64(seed)), int(row0), int(sample0), _ptr(cum), _ptr(thr), _ptr(work),
        C.c_size_t(work.numel()), _ptr(out['longest']), _ptr(out['longest_row']), _ptr(out['spells']),
        _ptr(out['onset_step']), _ptr(out['first_row']), _ptr(out['last_row']), _ptr(out.get('onset_count'))),
        'bnf_predictive_group_episodes')
    torch.cuda.synchronize(self.device)     # `work`, `off`, `rows`, `thr` and `cum` are released on return
    return out

  def predictive_group_cumulative(self, loc: torch.Tensor, aux: torch.Tensor, seg_offsets, seg_rows, n_samples: int, seed,
                                  level=None, running=False, per_row=True, cum_weights=None, row0=0, sample0=0) -> dict:
    """Running totals of the same sample paths, per group of rows, and when they pass a level (include/bnf.h
    bnf_predictive_group_cumulative), without materialising the draws; loc, aux, seg_offsets, seg_rows, row0, sample0 and
    cum_weights as for `predictive_group_sums`.  TIME is the order of the positions of seg_rows inside a group
    (`inference.csr_ordered`).  The run at a position is the f64 sum of the group's draws up to and including it; an
    entry of seg_rows outside [0, R) takes no part (the run is carried, it is not a step); a NaN draw makes every later
    run of its group NaN and counts as a step.  level (G,) f64, one per group: the crossing position is the first
    participating one with run > level (strict, false for NaN).  -> dict of device tensors:
      'total' (n_samples, G) f64        the run at the group's last position, 0 for a group without rows
      'running' (n_samples, R) f64      running=True: the run, column = POSITION of seg_rows (not table row)
      'cross_step' (n_samples, G) f64   with `level`: participating positions before the crossing one; all of them if none
      'cross_row' (n_samples, G) int32  with `level`: the table row of the crossing position, -1 if none
      'cross_count' (R,) int32          with `level`, per_row=True: the paths in which the row is its group's crossing row
      'above_count' (R,) int32          with `level`, per_row=True: the paths whose run at the row's position is > the level
    One kernel without a work buffer: a group longer than a tile is finished by one block per path, so a table that is
    one long group is parallel over the paths only (profiles/group_cumulative.md).  Deterministic: the same call gives
    the same bits, whatever n_samples, the cut into calls (sample0) and the outputs asked for."""
    loc, aux, off, rows, M, R, G = self._group_inputs(loc, aux, seg_offsets, seg_rows)
    lvl = None if level is None else self._as_f64(level, (G,), 'level')
    n_samples = int(n_samples)
    out = {'total': torch.empty((n_samples, G), dtype=torch.float64, device=self.device)}
    if running:
      out['running'] = torch.empty((n_samples, R), dtype=torch.float64, device=self.device)
    if lvl is not None:
      out['cross_step'] = torch.empty((n_samples, G), dtype=torch.float64, device=self.device)
      out['cross_row'] = torch.empty((n_samples, G), dtype=torch.int32, device=self.device)
      if per_row:                           # the library adds to these: zeroed here
        out['cross_count'] = torch.zeros((R,), dtype=torch.int32, device=self.device)
        out['above_count'] = torch.zeros((R,), dtype=torch.int32, device=self.device)
    cum = self._cum(cum_weights, M)
    _native.check(self.lib.bnf_predictive_group_cumulative(
        self.handle, _ptr(loc), _ptr(aux), M, R, _ptr(off), _ptr(rows), G, n_samples,
        C.c_uint64(_native.seed_to_u64(seed)), int(row0), int(sample0), _ptr(cum), _ptr(lvl), _ptr(out['total']),
        _ptr(out.get('running')), _ptr(out.get('cross_step')), _ptr(out.get('cross_row')), _ptr(out.get('cross_count')),
        _ptr(out.get('above_count'))), 'bnf_predictive_group_cumulative')
    torch.cuda.synchronize(self.device)     # `off`, `rows`, `lvl` and `cum` are released on return
    return out

  def predictive_group_windows(self, loc: torch.Tensor, aux: torch.Tensor, seg_offsets, seg_rows, n_samples: int, seed,
                               window, threshold=None, windows=False, per_row=True, cum_weights=None, row0=0,
                               sample0=0) -> dict:
    """Moving-window totals of the same sample paths, per group of rows (include/bnf.h bnf_predictive_group_windows),
    without materialising the draws; loc, aux, seg_offsets, seg_rows, row0, sample0 and cum_weights as for
    `predictive_group_sums`.  TIME is the order of the positions of seg_rows inside a group (`inference.csr_ordered`).
    The window at a position is the f64 sum of the draws at the last `window` positions up to and including it, clipped
    at the group's start; an entry of seg_rows outside [0, R) occupies a slot and adds nothing; a NaN draw makes exactly
    the windows that hold it NaN.  The CANDIDATES are the full-length windows that end at a participating position (for
    a group shorter than `window`: the whole group, at its last position).  threshold (G,) f64, one per group, compared
    with strict > (false for NaN).  -> dict of device tensors:
      'peak' (n_samples, G) f64         the largest candidate window that is not NaN; NaN if there is none
      'peak_row' (n_samples, G) int32   the table row at which it is first reached, -1 if none
      'window' (n_samples, R) f64       windows=True: the window, column = POSITION of seg_rows (not table row), at every
                                        position, candidate or not
      'count' (n_samples, G) f64        with `threshold`: the candidate windows above it
      'peak_count' (R,) int32           per_row=True: the paths whose peak window ends at the row
      'exceed_count' (R,) int32         with `threshold`, per_row=True: the paths whose candidate window ending at the
                                        row is above it
    One kernel without a work buffer; a group longer than a tile is finished by one block per path, as in
    `predictive_group_cumulative` (profiles/group_windows.md).  Deterministic: the same call gives the same bits,
    whatever n_samples, the cut into calls (sample0) and the outputs asked for."""
    loc, aux, off, rows, M, R, G = self._group_inputs(loc, aux, seg_offsets, seg_rows)
    thr = None if threshold is None else self._as_f64(threshold, (G,), 'threshold')
    n_samples = int(n_samples)
    out = {'peak': torch.empty((n_samples, G), dtype=torch.float64, device=self.device),
           'peak_row': torch.empty((n_samples, G), dtype=torch.int32, device=self.device)}
    if windows:
      out['window'] = torch.empty((n_samples, R), dtype=torch.float64, device=self.device)
    if thr is not None:
      out['count'] = torch.empty((n_samples, G), dtype=torch.float64, device=self.device)
    if per_row:                             # the library adds to these: zeroed here
      out['peak_count'] = torch.zeros((R,), dtype=torch.int32, device=self.device)
      if thr is not None:
        out['exceed_count'] = torch.zeros((R,), dtype=torch.int32, device=self.device)
    cum = self._cum(cum_weights, M)
    _native.check(self.lib.bnf_predictive_group_windows(
        self.handle, _ptr(loc), _ptr(aux), M, R, _ptr(off), _ptr(rows), G, n_samples,
        C.c_uint64(_native.seed_to_u64(seed)), int(row0), int(sample0), _ptr(cum), int(window), _ptr(thr),
        _ptr(out['peak']), _ptr(out['peak_row']), _ptr(out.get('window')), _ptr(out.get('count')),
        _ptr(out.get('peak_count')), _ptr(out.get('exceed_count'))), 'bnf_predictive_group_windows')
    torch.cuda.synchronize(self.device)     # `off`, `rows`, `thr` and `cum` are released on return
    return out

  def predictive_scores(self, loc: torch.Tensor, aux: torch.Tensor, y: torch.Tensor, crps=None, member_ll=True,
                        lpd=True, pit=True, weights=None, into=None) -> dict:
    """Held-out observations y (R,) scored against the ensemble (include/bnf.h bnf_predictive_scores): loc (M, R),
    aux (M, 3) as `forward` returns them -> dict of device tensors, one per output asked for:
      'member_ll' (M,) f64   sum over the rows with a finite y of each member's log density
      'lpd' (R,) f32         log density of the equal-weight mixture
      'pit' (2, R) f32       mixture CDF at y and just below y
      'crps' (R,) f32        NORMAL only (crps=None: exactly then; crps=True on a count handle is the library's error)
    Rows whose y is NaN come back NaN and do not enter member_ll.  Deterministic: the same call gives the same bits.
    weights (M,) array or device tensor: 'lpd', 'pit' and 'crps' are those of the mixture sum_m w_m p_m
    (bnf_predictive_scores_weighted) after the members of weight 0 are dropped; 'member_ll' is per member and comes from
    the unweighted call on all members.  None: the equal-weight call, bit for bit.
    into {'member_ll': (M,) f64, 'work': f64 of at least M * ceil(R / BNF_SCORE_ROW_TILE)}, device tensors the CALLER
    keeps alive, with y a float32 device tensor: 'member_ll' alone is written there, nothing is allocated here and the
    call returns without waiting for the device (the validation checks of `inference.fit_map`)."""
    loc = loc.contiguous().float()
    aux = aux.contiguous().float()
    M, R = loc.shape
    y = (y if isinstance(y, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32))
         ).to(self.device, dtype=torch.float32).contiguous()
    if y.shape != (R,):
      raise ValueError(f'y must hold one observation per row ({R},); got {tuple(y.shape)}')
    if into is not None:
      ll, work = into['member_ll'], into['work']
      n_work = M * (-(-R // _native.SCORE_ROW_TILE))
      if (weights is not None or ll.dtype != torch.float64 or tuple(ll.shape) != (M,) or work.dtype != torch.float64
          or work.numel() < n_work or not ll.is_contiguous() or not work.is_contiguous()):
        raise ValueError(f'into: member_ll (M,) f64 and work f64 of >= {n_work} are needed, and no weights')
      _native.check(self.lib.bnf_predictive_scores(
          self.handle, _ptr(loc), _ptr(aux), M, R, _ptr(y), _ptr(work), C.c_size_t(work.numel() * 8), _ptr(ll),
          None, None, None), 'bnf_predictive_scores')
      return {'member_ll': ll}
    if crps is None:
      crps = self.net.observation_model == 'NORMAL'
    if weights is not None:
      out = self.predictive_scores(loc, aux, y, crps=False, member_ll=True, lpd=False, pit=False) if member_ll else {}
      w, aux, loc = self._kept(weights, aux, loc)
      M = loc.shape[0]
      if lpd:
        out['lpd'] = torch.empty((R,), dtype=torch.float32, device=self.device)
      if pit:
        out['pit'] = torch.empty((2, R), dtype=torch.float32, device=self.device)
      if crps:
        out['crps'] = torch.empty((R,), dtype=torch.float32, device=self.device)
      n_chunks = -(-M // _native.SCORE_MEMBER_CHUNK)
      n_work = R * min((n_chunks + 1) // 2, _native.SCORE_MAX_SLOTS) if crps else 0
      work = torch.empty(max(1, n_work), dtype=torch.float64, device=self.device)
      _native.check(self.lib.bnf_predictive_scores_weighted(
          self.handle, _ptr(loc), _ptr(aux), _ptr(w), M, R, _ptr(y), _ptr(work), C.c_size_t(n_work * 8),
          _ptr(out.get('lpd')), _ptr(out.get('pit')), _ptr(out.get('crps'))), 'bnf_predictive_scores_weighted')
      torch.cuda.synchronize(self.device)   # `work`, `w` and the kept members' copies are released on return
      return out
    out = {}
    if member_ll:
      out['member_ll'] = torch.empty((M,), dtype=torch.float64, device=self.device)
    if lpd:
      out['lpd'] = torch.empty((R,), dtype=torch.float32, device=self.device)
    if pit:
      out['pit'] = torch.empty((2, R), dtype=torch.float32, device=self.device)
    if crps:
      out['crps'] = torch.empty((R,), dtype=torch.float32, device=self.device)
    # partial sums (the formula of include/bnf.h): per member and row tile for member_ll, per row and slot for crps
    n_chunks = -(-M // _native.SCORE_MEMBER_CHUNK)
    n_work = ((M * (-(-R // _native.SCORE_ROW_TILE)) if member_ll else 0) +
              (R * min((n_chunks + 1) // 2, _native.SCORE_MAX_SLOTS) if crps else 0))
    work = torch.empty(max(1, n_work), dtype=torch.float64, device=self.device)
    _native.check(self.lib.bnf_predictive_scores(
        self.handle, _ptr(loc), _ptr(aux), M, R, _ptr(y), _ptr(work), C.c_size_t(n_work * 8), _ptr(out.get('member_ll')),
        _ptr(out.get('lpd')), _ptr(out.get('pit')), _ptr(out.get('crps'))), 'bnf_predictive_scores')
    torch.cuda.synchronize(self.device)     # `work` and the device copy of `y` are released on return
    return out

  def count_rps(self, loc: torch.Tensor, aux: torch.Tensor, y, weights=None) -> torch.Tensor:
    """NB / ZINB: the ranked probability score -- the CRPS of a count forecast -- of the observations y (R,) against
    the equal-weight mixture over members (include/bnf.h bnf_count_rps): loc (M, R), aux (M, 3) as `forward` returns
    them -> (R,) f32 on the device.  NaN where y is NaN, negative or not an integer, and where the row's window is longer
    than BNF_RPS_MAX_TERMS.  A NORMAL handle is the library's error (ValueError).  Deterministic.
    weights (M,) array or device tensor: the score of the weighted mixture (bnf_count_rps_weighted) after the members
    of weight 0 are dropped -- such a member cannot cap a row; None: the equal-weight call, bit for bit."""
    loc = loc.contiguous().float()
    aux = aux.contiguous().float()
    M, R = loc.shape
    y = (y if isinstance(y, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32))
         ).to(self.device, dtype=torch.float32).contiguous()
    if y.shape != (R,):
      raise ValueError(f'y must hold one observation per row ({R},); got {tuple(y.shape)}')
    out = torch.empty((R,), dtype=torch.float32, device=self.device)
    if weights is not None:
      w, aux, loc = self._kept(weights, aux, loc)
      _native.check(self.lib.bnf_count_rps_weighted(self.handle, _ptr(loc), _ptr(aux), _ptr(w), loc.shape[0], R, _ptr(y),
                                                    _ptr(out)), 'bnf_count_rps_weighted')
      torch.cuda.synchronize(self.device)   # `w`, the kept members' copies and the device copy of `y` are released
      return out
    _native.check(self.lib.bnf_count_rps(self.handle, _ptr(loc), _ptr(aux), M, R, _ptr(y), _ptr(out)), 'bnf_count_rps')
    torch.cuda.synchronize(self.device)     # the device copy of `y` is released on return
    return out

  def member_log_density(self, loc: torch.Tensor, aux: torch.Tensor, y) -> torch.Tensor:
    """log p_m(y_r) of every member at every row (include/bnf.h bnf_member_log_density): loc (M, R), aux (M, 3) as
    `forward` returns them, y (R,) -> (M, R) f32 on the device -- the terms `predictive_scores` sums into 'member_ll'.
    NaN in every member of a row whose y is not finite; -inf where a member gives the observation density 0."""
    loc = loc.contiguous().float()
    aux = aux.contiguous().float()
    M, R = loc.shape
    y = (y if isinstance(y, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32))
         ).to(self.device, dtype=torch.float32).contiguous()
    if y.shape != (R,):
      raise ValueError(f'y must hold one observation per row ({R},); got {tuple(y.shape)}')
    out = torch.empty((M, R), dtype=torch.float32, device=self.device)
    _native.check(self.lib.bnf_member_log_density(self.handle, _ptr(loc), _ptr(aux), M, R, _ptr(y), _ptr(out)),
                  'bnf_member_log_density')
    torch.cuda.synchronize(self.device)     # the device copy of `y` is released on return
    return out

  def stacking_weights(self, logdens: torch.Tensor, w_init=None, max_iter=10000, tol=1e-5, lpd=True) -> dict:
    """Stacking weights of the members (include/bnf.h bnf_stacking_weights): logdens (M, R) f32 as `member_log_density`
    returns it -> the simplex weights that maximise the mean over the scored rows of log sum_m w_m p_m(y_r), by EM from
    w_init (None: uniform), stopped at gap = max_m g_m - 1 <= tol (a bound on the distance of the objective from its
    optimum) or after max_iter updates.  max_iter=0 evaluates w_init.  -> dict:
      'weights' (M,) f64 device tensor   'lpd' (R,) f32 device tensor with lpd=True: the log density of the weighted
                                         mixture; NaN rows NaN, dropped rows -inf
      'objective', 'objective_start', 'gap' floats   'iterations', 'dropped' ints   'converged' gap <= tol
    A row is dropped when every member with a positive weight gives it the density 0.  Deterministic."""
    logdens = logdens.contiguous().float()
    if logdens.dim() != 2:
      raise ValueError(f'logdens must be (n_members, n_rows); got {tuple(logdens.shape)}')
    M, R = logdens.shape
    w0 = None if w_init is None else self._as_f64(w_init, (M,), 'w_init')
    weights = torch.empty((M,), dtype=torch.float64, device=self.device)
    info = torch.empty((5,), dtype=torch.float64, device=self.device)
    out_lpd = torch.empty((R,), dtype=torch.float32, device=self.device) if lpd else None
    n_work = _native.stacking_work_doubles(M, R)
    work = torch.empty(n_work, dtype=torch.float64, device=self.device)
    _native.check(self.lib.bnf_stacking_weights(
        self.handle, _ptr(logdens), M, R, _ptr(w0), int(max_iter), C.c_double(float(tol)), _ptr(work),
        C.c_size_t(n_work * 8), _ptr(weights), _ptr(out_lpd), _ptr(info)), 'bnf_stacking_weights')
    torch.cuda.synchronize(self.device)     # `work` and the device copy of `w_init` are released on return
    f, f0, gap, iters, dropped = info.cpu().tolist()
    out = {'weights': weights, 'objective': f, 'objective_start': f0, 'gap': gap, 'iterations': int(iters),
           'dropped': int(dropped), 'converged': bool(gap <= float(tol))}
    if lpd:
      out['lpd'] = out_lpd
    return out

  def _as_f64(self, a, shape, what):
    t = (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
         ).to(self.device, dtype=torch.float64).contiguous()
    if shape is not None and tuple(t.shape) != shape:
      raise ValueError(f'{what} must have shape {shape}; got {tuple(t.shape)}')
    return t

  def sample_summaries(self, x, y=None, q=()) -> dict:
    """Column summaries of an ensemble of sample paths (include/bnf.h bnf_sample_summaries): x (S, G) f64 as
    `predictive_group_sums` returns it, optionally the observed totals y (G,) -> dict of f64 device tensors:
      'mean' (G,)            'quantiles' (len(q), G)   numpy's default 'linear' rule at the levels q
      'crps' (G,)  'pit' (2, G)   with y only: the ensemble CRPS (V-statistic) and #{x <= y} / S, #{x < y} / S; NaN where
                                  y is NaN
    A column holding a NaN sample is NaN everywhere.  More than BNF_SUMMARY_MAX_SAMPLES paths, or a level outside [0, 1],
    is the library's error (ValueError).  Deterministic: the same call gives the same bits."""
    x = self._as_f64(x, None, 'x')
    if x.dim() != 2:
      raise ValueError(f'x must be (n_samples, n_cols); got {tuple(x.shape)}')
    S, G = x.shape
    y = None if y is None else self._as_f64(y, (G,), 'y')
    levels = [float(v) for v in q]
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=self.device)
    out = {'mean': f64(G), 'quantiles': f64(len(levels), G)}
    if y is not None:
      out['crps'], out['pit'] = f64(G), f64(2, G)
    step = _native.SUMMARY_MAX_QUANTILES          # the levels of one call; more: further calls (each sorts again)
    for j0 in range(0, max(1, len(levels)), step):
      part = levels[j0:j0 + step]
      first = j0 == 0
      qa = (C.c_double * max(1, len(part)))(*part)
      _native.check(self.lib.bnf_sample_summaries(
          self.handle, _ptr(x), S, G, _ptr(y), qa, len(part), _ptr(out['mean'] if first else None),
          _ptr(out['quantiles'][j0:j0 + step] if part else None), _ptr(out.get('crps') if first else None),
          _ptr(out.get('pit') if first else None)), 'bnf_sample_summaries')
    torch.cuda.synchronize(self.device)     # device copies of `x` and `y` made here are released on return
    return out

  def sample_energy_score(self, x, y) -> float:
    """The energy score (1 / S) sum_s |X_s - y| - (1 / (2 S^2)) sum_st |X_s - X_t| of the joint paths x (S, G) f64
    against the observed vector y (G,) (include/bnf.h bnf_sample_energy_score).  Columns whose y is NaN are left out of
    both terms; NaN when none is left.  S^2 G / 2 differences.  Deterministic."""
    x = self._as_f64(x, None, 'x')
    if x.dim() != 2:
      raise ValueError(f'x must be (n_samples, n_cols); got {tuple(x.shape)}')
    S, G = x.shape
    y = self._as_f64(y, (G,), 'y')
    tiles = -(-S // _native.ENERGY_SAMPLE_TILE)
    n_work = S + tiles * (tiles + 1) // 2                  # the formula of include/bnf.h
    work = torch.empty(max(1, n_work), dtype=torch.float64, device=self.device)
    out = torch.empty((1,), dtype=torch.float64, device=self.device)
    _native.check(self.lib.bnf_sample_energy_score(
        self.handle, _ptr(x), S, G, _ptr(y), _ptr(work), C.c_size_t(n_work * 8), _ptr(out)), 'bnf_sample_energy_score')
    torch.cuda.synchronize(self.device)     # `work` is released on return
    return float(out.cpu()[0])

  def sample_pair_moments(self, x, p=0.5, y=None, pair_weights=None, matrices=True) -> dict:
    """How the columns of the joint paths x (S, G) f64 move together (include/bnf.h bnf_sample_pair_moments) -> dict of
    f64 device tensors:
      'mean' (G,)
      'covariance' (G, G)   matrices=True: (1 / S) sum_s (x_si - m_i) (x_sj - m_j), np.cov(x.T, bias=True)
      'variogram' (G, G)    matrices=True: (1 / S) sum_s |x_si - x_sj|^p
    and with the observed vector y (G,)
      'variogram_score' float   sum over the pairs i < j with y_i, y_j not NaN of w_ij (|y_i - y_j|^p - variogram_ij)^2,
                                w_ij = 1 or pair_weights (G, G) (read above the diagonal)
    p is 0.5, 1 or 2.  Both matrices are whole and bitwise symmetric; matrices=False writes nothing of size G^2 and gives
    the same score bits.  matrices / pair_weights with G > BNF_PAIR_MATRIX_MAX_COLS is a ValueError, as is another p (the
    library's error).  S G^2 / 2 pair terms.  Deterministic."""
    x = self._as_f64(x, None, 'x')
    if x.dim() != 2:
      raise ValueError(f'x must be (n_samples, n_cols); got {tuple(x.shape)}')
    S, G = x.shape
    y = None if y is None else self._as_f64(y, (G,), 'y')
    if pair_weights is not None and y is None:
      raise ValueError('pair_weights weight the variogram score: they need y')
    if (matrices or pair_weights is not None) and G > _native.PAIR_MATRIX_MAX_COLS:
      raise ValueError(f'{G} columns: a pair matrix (matrices, pair_weights) has at most {_native.PAIR_MATRIX_MAX_COLS} '
                       'a side')
    w = None if pair_weights is None else self._as_f64(pair_weights, (G, G), 'pair_weights')
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=self.device)
    out = {'mean': f64(G)}
    if matrices:
      out['covariance'], out['variogram'] = f64(G, G), f64(G, G)
    n_work = _native.pair_work_doubles(G) if y is not None else 0
    work = f64(n_work) if y is not None else None
    score = f64(1) if y is not None else None
    _native.check(self.lib.bnf_sample_pair_moments(
        self.handle, _ptr(x), S, G, C.c_double(float(p)), _ptr(y), _ptr(w), _ptr(out['mean']),
        _ptr(out.get('covariance')), _ptr(out.get('variogram')), _ptr(work), C.c_size_t(n_work * 8), _ptr(score)),
        'bnf_sample_pair_moments')
    torch.cuda.synchronize(self.device)     # `work` and the device copies made here are released on return
    if y is not None:
      out['variogram_score'] = float(score.cpu()[0])
    return out

  def sample_distances(self, x, p, scale=None, y=None):
    """The pairwise distances of the joint paths x (S, C) f64 (include/bnf.h bnf_sample_distances) -> (dist, ydist):
    dist (S, S) f64 device tensor, dist[s][t] = sum_c |x_sc - x_tc| (p = 1) or sqrt(sum_c (x_sc - x_tc)^2) (p = 2), with
    scale (C,) every difference divided by scale_c; ydist (S,) the same distance between every path and y (C,), None
    without y.  With y only the columns whose y_c is finite take part.  The matrix is whole and bitwise symmetric, the
    diagonal +0.0; a path with a NaN is NaN in its row and column.  A cell's bits depend on its two paths and the
    participating columns only.  S > BNF_SCENARIO_MAX_SAMPLES or another p is a ValueError.  S^2 C / 2 differences.
    Deterministic."""
    x = self._as_f64(x, None, 'x')
    if x.dim() != 2:
      raise ValueError(f'x must be (n_samples, n_cols); got {tuple(x.shape)}')
    S, G = x.shape
    if S < 1 or G < 1:
      raise ValueError(f'x must hold at least one path and one column; got {tuple(x.shape)}')
    if S > _native.SCENARIO_MAX_SAMPLES:
      raise ValueError(f'{S} sample paths: the distance matrix has at most {_native.SCENARIO_MAX_SAMPLES} a side')
    scale = None if scale is None else self._as_f64(scale, (G,), 'scale')
    y = None if y is None else self._as_f64(y, (G,), 'y')
    dist = torch.empty((S, S), dtype=torch.float64, device=self.device)
    ydist = None if y is None else torch.empty((S,), dtype=torch.float64, device=self.device)
    _native.check(self.lib.bnf_sample_distances(self.handle, _ptr(x), S, G, _ptr(scale), _ptr(y), int(p), _ptr(dist),
                                                _ptr(ydist)), 'bnf_sample_distances')
    torch.cuda.synchronize(self.device)     # device copies of `x`, `scale` and `y` made here are released on return
    return dist, ydist

  def scenario_select(self, dist, k, ydist=None) -> dict:
    """Fast forward selection of k scenarios on the symmetric distance matrix dist (S, S) f64 `sample_distances` returns
    (include/bnf.h bnf_scenario_select) -> dict of device tensors:
      'chosen' (k,) int32       the paths picked, in the order picked: each minimises sum_s min(nearest so far, dist[s][u]),
                                the lowest index among equal ones
      'objective' (k,) f64      that sum / S after 1 .. k scenarios: the Kantorovich distance to the ensemble, nonincreasing
      'prob' (k,) f64           the share of the paths nearest to each scenario (the earliest chosen among equally near)
      'assign' (S,) int32       the scenario 0 .. k - 1 of every path        'nearest' (S,) f64   its distance to it
    and with ydist (S,), the distances of an observed vector:
      'obs_nearest' (1,) int32  the scenario nearest to the observed vector
      'obs' (3,) f64            that distance, and the shares of the paths whose 'nearest' is <= and < it
    A NaN cell in dist gives -1 / NaN everywhere.  1 <= k <= S <= BNF_SCENARIO_MAX_SAMPLES, ValueError otherwise.  k S^2
    reads of dist, all steps enqueued at once.  Deterministic."""
    if not (isinstance(dist, torch.Tensor) and dist.dim() == 2 and dist.shape[0] == dist.shape[1]
            and dist.dtype == torch.float64):
      raise ValueError('dist must be the (n_samples, n_samples) f64 device tensor sample_distances returns')
    dist = dist.to(self.device).contiguous()
    S = dist.shape[0]
    k = int(k)
    if S < 1 or S > _native.SCENARIO_MAX_SAMPLES:
      raise ValueError(f'{S} sample paths: 1..{_native.SCENARIO_MAX_SAMPLES}')
    if not 1 <= k <= S:
      raise ValueError(f'k={k}: 1..{S}, the number of sample paths')
    ydist = None if ydist is None else self._as_f64(ydist, (S,), 'ydist')
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=self.device)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=self.device)
    out = {'chosen': i32(k), 'objective': f64(k), 'prob': f64(k), 'assign': i32(S), 'nearest': f64(S)}
    if ydist is not None:
      out['obs_nearest'], out['obs'] = i32(1), f64(3)
    n_work = _native.scenario_work_bytes(S)
    work = torch.empty(-(-n_work // 8), dtype=torch.float64, device=self.device)
    _native.check(self.lib.bnf_scenario_select(
        self.handle, _ptr(dist), S, k, _ptr(ydist), _ptr(work), C.c_size_t(n_work), _ptr(out['chosen']),
        _ptr(out['objective']), _ptr(out['prob']), _ptr(out['assign']), _ptr(out['nearest']), _ptr(out.get('obs_nearest')),
        _ptr(out.get('obs'))), 'bnf_scenario_select')
    torch.cuda.synchronize(self.device)     # `work` and the device copies made here are released on return
    return out

  def sample_ranks(self, x, scale=None) -> dict:
    """How the columns of every joint path of x (S, G) f64 rank against each other (include/bnf.h bnf_sample_ranks), on
    the values x / scale with scale (G,) an optional per-column divisor -> dict of (S, G) device tensors:
      'above' int32   columns of the path with a larger value
      'ties' int32    columns of the path with an equal value, the column itself included
      'rank' f64      the mid-rank above + (ties + 1) / 2: rank 1 is the largest value, tied columns share their block
    -0.0 ties with +0.0; NaNs tie with each other and rank below everything.  G > BNF_RANK_MAX_COLS is a ValueError.
    G log^2 G per path.  Deterministic."""
    x = self._as_f64(x, None, 'x')
    if x.dim() != 2:
      raise ValueError(f'x must be (n_samples, n_cols); got {tuple(x.shape)}')
    S, G = x.shape
    if S < 1 or G < 1:
      raise ValueError(f'x must hold at least one path and one column; got {tuple(x.shape)}')
    if G > _native.RANK_MAX_COLS:
      raise ValueError(f'{G} columns: the values of a path are ranked in LDS, at most {_native.RANK_MAX_COLS}')
    scale = None if scale is None else self._as_f64(scale, (G,), 'scale')
    out = {'rank': torch.empty((S, G), dtype=torch.float64, device=self.device),
           'above': torch.empty((S, G), dtype=torch.int32, device=self.device),
           'ties': torch.empty((S, G), dtype=torch.int32, device=self.device)}
    _native.check(self.lib.bnf_sample_ranks(self.handle, _ptr(x), S, G, _ptr(scale), _ptr(out['rank']),
                                            _ptr(out['above']), _ptr(out['ties'])), 'bnf_sample_ranks')
    torch.cuda.synchronize(self.device)     # device copies of `x` and `scale` made here are released on return
    return out

  def rank_probabilities(self, above, ties, top_k) -> torch.Tensor:
    """P(column g takes rank slot k), k = 1 .. top_k, from the (S, G) int32 matrices `sample_ranks` returns (include/bnf.h
    bnf_rank_probabilities) -> (top_k, G) f64 device tensor: (1 / S) sum_s [above < k <= above + ties] / ties, a tied block
    handing each of its slots out in equal shares.  Every row sums to 1 over the columns.  1 <= top_k <= G and
    top_k * G <= BNF_RANK_MAX_CELLS, ValueError otherwise.  Deterministic."""
    if not (isinstance(above, torch.Tensor) and isinstance(ties, torch.Tensor)):
      raise ValueError('above and ties must be the device tensors sample_ranks returns')
    if above.dim() != 2 or above.shape != ties.shape or above.dtype != torch.int32 or ties.dtype != torch.int32:
      raise ValueError(f'above and ties must be int32 of one shape (n_samples, n_cols); got {tuple(above.shape)} '
                       f'{above.dtype} and {tuple(ties.shape)} {ties.dtype}')
    above, ties = above.to(self.device).contiguous(), ties.to(self.device).contiguous()
    S, G = above.shape
    if S < 1 or G < 1:
      raise ValueError(f'above must hold at least one path and one column; got {tuple(above.shape)}')
    top_k = int(top_k)
    if not 1 <= top_k <= G:
      raise ValueError(f'top_k={top_k}: 1..{G}, the number of columns')
    if top_k * G > _native.RANK_MAX_CELLS:
      raise ValueError(f'top_k={top_k} x {G} columns: at most {_native.RANK_MAX_CELLS} cells')
    out = torch.empty((top_k, G), dtype=torch.float64, device=self.device)
    _native.check(self.lib.bnf_rank_probabilities(self.handle, _ptr(above), _ptr(ties), S, G, top_k, _ptr(out)),
                  'bnf_rank_probabilities')
    torch.cuda.synchronize(self.device)     # device copies made here are released on return
    return out

  def _band_inputs(self, x, col_group, n_groups):
    """x (S, C) f64, col_group (C,) int32 on the device, and the sizes checked -> (x, col_group, S, C, G)."""
    x = self._as_f64(x, None, 'x')
    if x.dim() != 2:
      raise ValueError(f'x must be (n_samples, n_cols); got {tuple(x.shape)}')
    S, C_ = x.shape
    if S < 1 or C_ < 1:
      raise ValueError(f'x must hold at least one path and one column; got {tuple(x.shape)}')
    if S > _native.SUMMARY_MAX_SAMPLES:
      raise ValueError(f'{S} sample paths: a column is sorted in LDS, at most {_native.SUMMARY_MAX_SAMPLES}')
    G = int(n_groups)
    if G < 1:
      raise ValueError(f'n_groups={G}: need at least one group')
    cg = (col_group if isinstance(col_group, torch.Tensor)
          else torch.from_numpy(np.ascontiguousarray(col_group, dtype=np.int32))).to(self.device, dtype=torch.int32).contiguous()
    if tuple(cg.shape) != (C_,):
      raise ValueError(f'col_group must hold one group per column ({C_},); got {tuple(cg.shape)}')
    return x, cg, S, C_, G

  def sample_depths(self, x, col_group, n_groups, y=None, depth=None, obs_depth=None) -> dict:
    """The depth of every joint path of x (S, C) f64 in every group of columns (include/bnf.h bnf_sample_depths):
    col_group (C,) int32 the group of every column, an entry outside [0, n_groups) = the column takes no part -> dict of
    int32 device tensors:
      'depth' (S, G)      min over the group's columns of min(#{x_t <= x_s}, #{x_t >= x_s}) - 1; path s lies inside the band
                          [x_(k), x_(S-1-k)] at every column of g exactly when depth[s][g] >= k.  -1 in a group with a NaN
                          column, BNF_DEPTH_NONE (0x7fffffff) in a group without columns
      'obs_depth' (G,)    with y (C,), the observed values (NaN: takes no part): the same for the observed curve, -1 =
                          outside the envelope of all paths; BNF_DEPTH_NONE where no column has an observed value
    depth / obs_depth: tensors an earlier call returned -- the call lowers them further, so chunks of columns, or several
    curves of the same paths, accumulate into one joint depth; None: allocated here and filled with BNF_DEPTH_NONE.
    More than BNF_SUMMARY_MAX_SAMPLES paths is a ValueError.  Integer atomicMin only: deterministic."""
    x, cg, S, C_, G = self._band_inputs(x, col_group, n_groups)
    y = None if y is None else self._as_f64(y, (C_,), 'y')

    def held(t, shape, what):
      if t is None:
        return torch.full(shape, _native.DEPTH_NONE, dtype=torch.int32, device=self.device)
      if not (isinstance(t, torch.Tensor) and t.dtype == torch.int32 and tuple(t.shape) == shape and t.is_contiguous()
              and t.device == x.device):
        raise ValueError(f'{what} must be the contiguous int32 device tensor {shape} an earlier call returned')
      return t

    out = {'depth': held(depth, (S, G), 'depth')}
    if y is not None:
      out['obs_depth'] = held(obs_depth, (G,), 'obs_depth')
    elif obs_depth is not None:
      raise ValueError('obs_depth accumulates the depth of the observed values: it needs y')
    _native.check(self.lib.bnf_sample_depths(self.handle, _ptr(x), S, C_, _ptr(cg), G, _ptr(y), _ptr(out['depth']),
                                             _ptr(out.get('obs_depth'))), 'bnf_sample_depths')
    torch.cuda.synchronize(self.device)     # device copies of `x`, `col_group` and `y` made here are released on return
    return out

  def depth_levels(self, depth, need, k_query=(), obs_depth=None) -> dict:
    """The band levels that hold `need` whole paths, from the (S, G) int32 depths `sample_depths` returns (include/bnf.h
    bnf_depth_levels).  need: ints in [1, S] (`inference.band_need`); k_query: band levels to evaluate -> dict of device
    tensors:
      'level' (len(need), G) int32      the largest k with #{s : depth >= k} >= need: the need-th largest depth of the group
      'achieved' (len(need), G) f64     #{s : depth >= level} / S >= need / S
      'joint' (len(k_query), G) f64     with k_query: #{s : depth >= k_query} / S, the share of the paths band k holds whole
      'obs_pit' (2, G) f64              with obs_depth (G,) int32: #{depth <= obs_depth} / S and #{depth < obs_depth} / S;
                                        NaN where obs_depth is BNF_DEPTH_NONE
    A group without columns (a depth outside [-1, S - 1]) has level -1 and NaN ratios; a group with a NaN column level -1
    and achieved 1.  At most BNF_BAND_MAX_LEVELS entries in need and in k_query, a need outside [1, S] is the library's
    error (ValueError).  Deterministic."""
    if not (isinstance(depth, torch.Tensor) and depth.dim() == 2 and depth.dtype == torch.int32):
      raise ValueError('depth must be the (n_samples, n_groups) int32 device tensor sample_depths returns')
    depth = depth.to(self.device).contiguous()
    S, G = depth.shape
    if S < 1 or G < 1:
      raise ValueError(f'depth must hold at least one path and one group; got {tuple(depth.shape)}')
    need = [int(v) for v in need]
    k_query = [int(v) for v in k_query]
    if not need:
      raise ValueError('need: at least one count of paths to hold')
    if max(len(need), len(k_query)) > _native.BAND_MAX_LEVELS:
      raise ValueError(f'{len(need)} coverage levels, {len(k_query)} queried bands: at most {_native.BAND_MAX_LEVELS} each')
    if obs_depth is not None:
      if not (isinstance(obs_depth, torch.Tensor) and obs_depth.dtype == torch.int32 and tuple(obs_depth.shape) == (G,)):
        raise ValueError(f'obs_depth must be the ({G},) int32 device tensor sample_depths returns')
      obs_depth = obs_depth.to(self.device).contiguous()
    out = {'level': torch.empty((len(need), G), dtype=torch.int32, device=self.device),
           'achieved': torch.empty((len(need), G), dtype=torch.float64, device=self.device)}
    if k_query:
      out['joint'] = torch.empty((len(k_query), G), dtype=torch.float64, device=self.device)
    if obs_depth is not None:
      out['obs_pit'] = torch.empty((2, G), dtype=torch.float64, device=self.device)
    clamp = lambda v: max(-0x80000000, min(0x7fffffff, v))
    na = (C.c_int32 * len(need))(*[clamp(v) for v in need])
    ka = (C.c_int32 * max(1, len(k_query)))(*[clamp(v) for v in k_query])
    _native.check(self.lib.bnf_depth_levels(
        self.handle, _ptr(depth), S, G, na, len(need), ka, len(k_query), _ptr(obs_depth), _ptr(out['level']),
        _ptr(out['achieved']), _ptr(out.get('joint')), _ptr(out.get('obs_pit'))), 'bnf_depth_levels')
    torch.cuda.synchronize(self.device)     # device copies made here are released on return
    return out

  def sample_envelope(self, x, col_group, level) -> dict:
    """The bands [x_(k), x_(S-1-k)] of the columns of x (S, C) f64 at the levels k = level[j][group of the column]
    (include/bnf.h bnf_sample_envelope): col_group (C,) int32 as for `sample_depths`, level (n_levels, G) int32 as
    `depth_levels` returns it -> {'lower', 'upper'}: (n_levels, C) f64 device tensors, values picked from x; NaN where the
    level is outside [0, S - 1], the column takes no part or holds a NaN sample.  Deterministic."""
    if not (isinstance(level, torch.Tensor) and level.dim() == 2 and level.dtype == torch.int32):
      raise ValueError('level must be the (n_levels, n_groups) int32 device tensor depth_levels returns')
    level = level.to(self.device).contiguous()
    L, G = level.shape
    x, cg, S, C_, G = self._band_inputs(x, col_group, G)
    if not 1 <= L <= _native.BAND_MAX_LEVELS:
      raise ValueError(f'{L} levels: 1..{_native.BAND_MAX_LEVELS}')
    out = {'lower': torch.empty((L, C_), dtype=torch.float64, device=self.device),
           'upper': torch.empty((L, C_), dtype=torch.float64, device=self.device)}
    _native.check(self.lib.bnf_sample_envelope(self.handle, _ptr(x), S, C_, _ptr(cg), _ptr(level), L, G, _ptr(out['lower']),
                                               _ptr(out['upper'])), 'bnf_sample_envelope')
    torch.cuda.synchronize(self.device)     # device copies of `x` and `col_group` made here are released on return
    return out

  # -- introspection (tests, bench) -------------------------------------------
  def debug_loss_and_grad(self, epoch=0, step=0):
    k = 2 if self.mode == 'vi' else 1
    grads = torch.empty((k * self.members, self.net.P), dtype=torch.float32, device=self.device)
    loss = torch.empty((self.members,), dtype=torch.float32, device=self.device)
    _native.check(self.lib.bnf_debug_loss_and_grad(self.handle, epoch, step, _ptr(grads),
                                                   _ptr(loss)), 'bnf_debug_loss_and_grad')
    torch.cuda.synchronize(self.device)
    g = grads.cpu().numpy()
    if self.mode == 'vi':
      g = g.reshape(2, self.members, self.net.P)
    return loss.cpu().numpy(), g

  def debug_row_index(self, epoch=0, step=0) -> np.ndarray:
    out = torch.empty((self.members, self.batch), dtype=torch.int32, device=self.device)
    _native.check(self.lib.bnf_debug_row_index(self.handle, epoch, step, _ptr(out)),
                  'bnf_debug_row_index')
    torch.cuda.synchronize(self.device)
    return out.cpu().numpy()

  def debug_vi_eps(self, step=0) -> np.ndarray:
    out = torch.empty((self.members, self.S, self.net.P), dtype=torch.float32, device=self.device)
    _native.check(self.lib.bnf_debug_vi_eps(self.handle, step, _ptr(out)), 'bnf_debug_vi_eps')
    torch.cuda.synchronize(self.device)
    return out.cpu().numpy()

  def set_vi_noise_keys(self, step_keys, draw_keys, leaf_offsets):
    """The reference's VI noise stream (include/bnf.h bnf_vi_noise_keys): key tables from
    jaxseed.vi_noise_keys / vi_draw_keys (uint32 numpy), uploaded and kept alive here."""
    if step_keys is None and draw_keys is None:
      self._vi_keys = None
      _native.check(self.lib.bnf_vi_noise_keys(self.handle, None, 0, None, 0, None, 0), 'bnf_vi_noise_keys')
      return
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(self.device)
    sk, dk = up(step_keys), up(draw_keys)
    lo = np.ascontiguousarray(leaf_offsets, dtype=np.int32)
    self._vi_keys = (sk, dk)
    _native.check(self.lib.bnf_vi_noise_keys(
        self.handle, None if sk is None else _ptr(sk), 0 if sk is None else int(step_keys.shape[0]),
        None if dk is None else _ptr(dk), 0 if dk is None else int(draw_keys.shape[0]),
        lo.ctypes.data_as(C.c_void_p), int(len(lo) - 1)), 'bnf_vi_noise_keys')

  def debug_vi_noise(self, eps):
    """Verification hook (include/bnf.h bnf_debug_vi_noise): every following VI step reads its
    (members, S, P) standard normals from `eps` (device tensor, kept alive here); None restores
    the engine's generator."""
    self._ext_eps = None if eps is None else eps.contiguous().float().to(self.device)
    _native.check(self.lib.bnf_debug_vi_noise(self.handle, None if eps is None else _ptr(self._ext_eps)),
                  'bnf_debug_vi_noise')

  def debug_poison_lds(self, pattern=0x7fc00000):
    """Test hook (include/bnf.h bnf_debug_poison_lds): garbage in every CU's LDS before the next kernels."""
    _native.check(self.lib.bnf_debug_poison_lds(self.handle, int(pattern) & 0xffffffff), 'bnf_debug_poison_lds')

  def debug_activation(self, what: int) -> np.ndarray:
    ev = self.members * self.S
    if what == 0 or what == 400:
      shape = (ev, self.batch, self.net.F)
    elif what == 200:
      shape = (ev, self.batch)
    else:
      shape = (ev, self.batch, self.net.width)
    out = torch.empty(shape, dtype=torch.float32, device=self.device)
    _native.check(self.lib.bnf_debug_activation(self.handle, what, _ptr(out)),
                  'bnf_debug_activation')
    torch.cuda.synchronize(self.device)
    return out.cpu().numpy()

  def debug_gemm_nt(self, A: np.ndarray, Bt: np.ndarray) -> np.ndarray:
    A = torch.as_tensor(np.ascontiguousarray(A, dtype=np.float32)).to(self.device)
    Bt = torch.as_tensor(np.ascontiguousarray(Bt, dtype=np.float32)).to(self.device)
    Cout = torch.empty((A.shape[0], Bt.shape[0]), dtype=torch.float32, device=self.device)
    _native.check(self.lib.bnf_debug_gemm_nt(self.handle, _ptr(A), _ptr(Bt), A.shape[0],
                                             Bt.shape[0], A.shape[1], _ptr(Cout)),
                  'bnf_debug_gemm_nt')
    torch.cuda.synchronize(self.device)
    return Cout.cpu().numpy()

  def debug_gemm_tn(self, A: np.ndarray, B: np.ndarray) -> np.ndarray:
    """A (R, M), B (R, N) row-major -> A^T B (M, N) through the weight-gradient core."""
    A = torch.as_tensor(np.ascontiguousarray(A, dtype=np.float32)).to(self.device)
    B = torch.as_tensor(np.ascontiguousarray(B, dtype=np.float32)).to(self.device)
    Cout = torch.empty((A.shape[1], B.shape[1]), dtype=torch.float32, device=self.device)
    _native.check(self.lib.bnf_debug_gemm_tn(self.handle, _ptr(A), _ptr(B), A.shape[0], A.shape[1],
                                             B.shape[1], _ptr(Cout)), 'bnf_debug_gemm_tn')
    torch.cuda.synchronize(self.device)
    return Cout.cpu().numpy()

  def profile(self, kernel):
    """kernel: '*' (all), a kernel name, or None (off)."""
    arg = None if kernel is None else str(kernel).encode()
    _native.check(self.lib.bnf_profile_enable(self.handle, arg), 'bnf_profile_enable')

  def profile_read(self) -> dict:
    cap = 32
    n = C.c_int32(cap)
    names = (C.c_char_p * cap)()
    avg = (C.c_double * cap)()
    calls = (C.c_int64 * cap)()
    _native.check(self.lib.bnf_profile_read(self.handle, C.byref(n), names, avg, calls),
                  'bnf_profile_read')
    out = {}
    for i in range(n.value):
      name = names[i].decode()
      out[name] = dict(avg_ms=avg[i], calls=calls[i],
                       flops=self.lib.bnf_kernel_flops(self.handle, names[i]))
    return out
