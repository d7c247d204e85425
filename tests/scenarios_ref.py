"""Representative scenarios of an ensemble of sample paths (bayesnf_amd/csrc/bnf_scenarios.h, include/bnf.h
bnf_sample_distances / bnf_scenario_select) on the host.  x (S, C): S sample paths of C totals; y (C,): the observed totals,
a column with a NaN y takes no part; scale (C,): divides every difference; p in {1, 2}.

  brute force, straight from the definitions
    `distances_ref`   per cell math.fsum over the participating columns of |d| or d * d, d = (x_sc - x_tc) / scale_c formed in
                      np.longdouble and rounded to float64 once per term; sqrt for p = 2.  -> (dist (S, S), ydist (S,) or None)
    `select_ref`      fast forward selection with math.fsum sums and np.argmin's first-of-equal rule; reports per step the
                      relative gap between its best and its second-best candidate
    `step_sums_ref`   z(u) of one step from a given prefix of chosen paths (to hold a device's step greedy-valid)
    (integer-valued inputs -- counts, p = 1, no scale -- are summed with numpy instead: every partial sum is an integer
    below 2^53, exact in any order)
  the kernels' own order, restated in numpy
    `distances_kernel_form`   one sequential float64 sum per cell over the participating columns in ascending order
    `select_kernel_form`      z(u): "thread" t adds s = t, t + 256, ... in that order, the wave butterfly (off = 32 .. 1), the four
                              waves in order; (z, u) compared lexicographically
    `scenarios_kernel_form`   both, -> the dict of `select_ref`

Bars, each from float64 rounding with EPS = 2^-53:
  a distance cell   (C + 8) EPS of itself: every term has a relative error of a few EPS, the terms are nonnegative (a sum of
                    C of them adds at most C EPS), sqrt halves the error and adds one
  objective         (C + S + 16) EPS =: r of itself (the cells' bar, S nonnegative terms, one division)
  prob, assign, path, pit   integers or one division of a count: exact, given the selection
Selection equality is conditional on the reference: the exact `chosen` is demanded where every gap of the reference is at
least MIN_GAP = 1e-9 (more than three orders above 3 r < 1e-12 for the shapes used); whatever the gaps, every step must be
greedy-valid, z_ref(chosen_i) <= min_u z_ref(u) (1 + 3 r), the reference sums formed from the device's own prefix.
"""
import functools
import math

import numpy as np

EPS = 2.0 ** -53
TILE, CHUNK, THREADS = 64, 32, 256    # paths per side of a pair tile, columns per LDS chunk, threads of a candidate's sum
NORMS = (1, 2)
KINDS = ('normal', 'counts', 'big', 'clusters')
MIN_GAP = 1e-9
GRID_S = (1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
GRID_C = (1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)
SELECT_SHAPES = ((65, 33), (129, 12), (257, 5))       # (S, C) of the generated selection cases
SELECT_K = 6


def _ld(a):
  return np.asarray(a, dtype=np.longdouble)


def _fsum_rows(terms):
  """terms (n, m) float64 -> (n,) the exact sums of the rows, rounded once."""
  return np.asarray([math.fsum(row) for row in np.ascontiguousarray(terms).tolist()], dtype=np.float64).reshape(len(terms))


def participating(C, y):
  return np.ones(C, dtype=bool) if y is None else np.isfinite(y)


def _integers(*arrays):
  return all(a is None or (np.all(np.isfinite(a)) and np.all(a == np.floor(a)) and np.abs(a).max(initial=0.0) < 2.0 ** 40)
             for a in arrays)


# ---- brute force ---------------------------------------------------------------------------------------------------
def distances_ref(x, p, scale=None, y=None):
  S, C = x.shape
  keep = participating(C, y)
  xs = np.asarray(x, dtype=np.float64)[:, keep]
  sc = None if scale is None else _ld(np.asarray(scale)[keep])
  rows = xs if y is None else np.concatenate([xs, np.asarray(y)[keep][None, :]], axis=0)
  n = rows.shape[0]
  if p == 1 and scale is None and _integers(rows):        # exact in any order
    full = np.abs(rows[:, None, :] - rows[None, :, :]).sum(axis=2) if n <= 512 else np.stack(
        [np.abs(rows[i] - rows).sum(axis=1) for i in range(n)])
  else:
    rl = _ld(rows)
    full = np.zeros((n, n))
    for i in range(n):
      d = rl[i] - rl[i:]
      if sc is not None:
        d = d / sc
      t = (np.abs(d) if p == 1 else d * d).astype(np.float64)
      v = _fsum_rows(t) if t.shape[1] else np.zeros(n - i)
      full[i, i:] = full[i:, i] = v if p == 1 else np.sqrt(v)
  if y is None:
    return full, None
  return np.ascontiguousarray(full[:S, :S]), np.ascontiguousarray(full[:S, S])


def step_sums_ref(dist, prefix):
  """z(u) = fsum_s min(dmin_s, dist[s][u]) with dmin from the chosen `prefix`; +inf at the paths of the prefix."""
  S = dist.shape[0]
  dmin = np.full(S, np.inf) if len(prefix) == 0 else dist[:, list(prefix)].min(axis=1)
  m = np.minimum(dmin[None, :], dist.T)                    # (u, s)
  z = m.sum(axis=1) if _integers(dist) else _fsum_rows(m)
  z[list(prefix)] = np.inf
  return z


def finish_ref(dist, chosen, ydist=None):
  """assign, nearest, prob and the observed outputs that follow from a selection."""
  S = dist.shape[0]
  near = dist[:, chosen]                                   # (S, k)
  nearest = near.min(axis=1)
  assign = np.argmax(near == nearest[:, None], axis=1)     # the earliest chosen among equally near
  out = dict(assign=assign, nearest=nearest, prob=np.bincount(assign, minlength=len(chosen)) / float(S))
  if ydist is not None:
    j = int(np.argmin(ydist[chosen]))
    d0 = float(ydist[chosen][j])
    out.update(obs_nearest=j, obs=np.array([d0, np.sum(nearest <= d0) / float(S), np.sum(nearest < d0) / float(S)]))
  return out


def select_ref(dist, k, ydist=None):
  """-> dict(chosen (k,), objective (k,), gaps (k,), prob, assign, nearest[, obs_nearest, obs]); gaps[i] = (second-best z -
  best z) / best z of step i among the candidates (inf with one candidate left or a best of 0 below a positive second)."""
  S = dist.shape[0]
  chosen, objective, gaps = [], [], []
  for _ in range(k):
    z = step_sums_ref(dist, chosen)
    u = int(np.argmin(z))
    rest = np.delete(z, u)
    rest = rest[np.isfinite(rest)]
    if rest.size == 0 or (z[u] == 0 and rest.min() > 0):
      gaps.append(np.inf)
    elif z[u] == 0:
      gaps.append(0.0)
    else:
      gaps.append(float((rest.min() - z[u]) / z[u]))
    chosen.append(u)
    objective.append(z[u] / float(S))
  out = dict(chosen=np.asarray(chosen), objective=np.asarray(objective), gaps=np.asarray(gaps))
  out.update(finish_ref(dist, out['chosen'], ydist))
  return out


# ---- the kernels' own order ----------------------------------------------------------------------------------------------
def distances_kernel_form(x, p, scale=None, y=None):
  S, C = x.shape
  keep = participating(C, y)
  rows = np.asarray(x, dtype=np.float64) if y is None else np.concatenate([x, np.where(keep, y, 0.0)[None, :]], axis=0)
  n = rows.shape[0]
  acc = np.zeros((n, n))
  with np.errstate(invalid='ignore'):
    for c in np.flatnonzero(keep):
      d = rows[:, None, c] - rows[None, :, c]
      if scale is not None:
        d = d / scale[c]
      acc = acc + (np.abs(d) if p == 1 else d * d)
    full = acc if p == 1 else np.sqrt(acc)
  if y is None:
    return full, None
  return np.ascontiguousarray(full[:S, :S]), np.ascontiguousarray(full[:S, S])


def kernel_sums(dmin, dist_rows):
  """The sums of k_scn_sums for the candidates whose rows of dist are given (U, S) -> (U,)."""
  U, S = dist_rows.shape
  n = -(-S // THREADS)
  m = np.zeros((U, n * THREADS))
  m[:, :S] = np.minimum(dmin[None, :], dist_rows)
  per_thread = np.cumsum(m.reshape(U, n, THREADS), axis=1)[:, -1, :]       # thread t: s = t, t + 256, ... in that order
  v = per_thread.reshape(U, THREADS // 64, 64)
  lane = np.arange(64)
  for off in (32, 16, 8, 4, 2, 1):
    v = v + v[:, :, lane ^ off]
  w = v[:, :, 0]
  return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def select_kernel_form(dist, k, ydist=None):
  S = dist.shape[0]
  if np.isnan(dist).any():
    out = dict(chosen=np.full(k, -1), objective=np.full(k, np.nan), prob=np.full(k, np.nan), assign=np.full(S, -1),
               nearest=np.full(S, np.nan))
    if ydist is not None:
      out.update(obs_nearest=-1, obs=np.full(3, np.nan))
    return out
  dmin = np.full(S, np.inf)
  taken = np.zeros(S, dtype=bool)
  chosen, objective = [], []
  for _ in range(k):
    z = np.where(taken, np.inf, kernel_sums(dmin, dist))
    order = np.lexsort((np.arange(S), z))                  # by z, the lower index among equal ones
    u = int(next(i for i in order if not taken[i]))
    chosen.append(u)
    objective.append(z[u] / float(S))
    taken[u] = True
    dmin = np.minimum(dmin, dist[u])
  out = dict(chosen=np.asarray(chosen), objective=np.asarray(objective))
  out.update(finish_ref(dist, out['chosen'], ydist))
  return out


def scenarios_kernel_form(x, p, k, scale=None, y=None):
  dist, ydist = distances_kernel_form(x, p, scale, y)
  out = select_kernel_form(dist, k, ydist)
  out.update(dist=dist, ydist=ydist)
  return out


# ---- bars and checks -------------------------------------------------------------------------------------------------
def cell_bar(C, ref):
  return (C + 8) * EPS * np.abs(ref)


def objective_rel(S, C):
  return (C + S + 16) * EPS


def check_distances(tag, got, got_y, x, p, scale, y, ref=None):
  """Asserts a device (or restated) distance matrix against the brute force at the cell bar; x without NaN.  Prints and
  returns the worst error / bar."""
  S, C = x.shape
  want, want_y = ref if ref is not None else distances_ref(x, p, scale, y)
  worst = 0.0
  for name, g, w in (('dist', got, want), ('ydist', got_y, want_y)):
    if w is None:
      assert g is None, (tag, name)
      continue
    err, bar = np.abs(g - w), cell_bar(C, w)
    assert not np.isnan(g).any(), (tag, name, 'NaN where a value is due')
    assert np.all(err <= bar), (tag, name, float(np.max(err - bar)))
    worst = max(worst, float(np.max(err / np.where(bar > 0, bar, np.inf), initial=0.0)))
  print(f'{tag}: distance error / bar {worst:.3f}')
  return worst


def check_selection(tag, got, dist, k, C, ydist=None, exact=False, ref=None, need_gaps=False, own=None):
  """Asserts a selection `got` (numpy arrays, keys as Engine.scenario_select returns them) against the reference matrix
  `dist` (and `ydist`).  exact=True (integer arithmetic): everything bit for bit against `select_ref`, ties included.
  Otherwise: the exact `chosen` where every reference gap is >= MIN_GAP (need_gaps=True: they must be); the objective
  within r of the reference sum of the step; every step greedy-valid, the reference sums formed from the selection's own
  prefix; and, given the selection, assign, nearest, prob and the observed outputs EXACTLY what follows from own =
  (dist, ydist), the matrix the selection itself ran on (held to the cell bars by `check_distances`)."""
  S = dist.shape[0]
  ref = ref if ref is not None else select_ref(dist, k, ydist)
  r = objective_rel(S, C)
  chosen = np.asarray(got['chosen']).astype(np.int64)
  assert chosen.shape == (k,) and len(set(chosen.tolist())) == k and chosen.min() >= 0 and chosen.max() < S, (tag, chosen)
  objective = np.asarray(got['objective'])
  if exact:
    for key in ('chosen', 'objective', 'prob', 'assign', 'nearest'):
      if key in got:                                       # (the estimators do not return 'nearest')
        assert np.array_equal(np.asarray(got[key], dtype=np.float64), np.asarray(ref[key], dtype=np.float64)), (tag, key)
    if ydist is not None:
      assert int(got['obs_nearest']) == ref['obs_nearest'] and np.array_equal(got['obs'], ref['obs']), (tag, 'obs')
    print(f'{tag}: exact; chosen {chosen[:8].tolist()} objective {objective[:4].tolist()}')
    return ref
  gaps_ok = bool(np.all(ref['gaps'] >= MIN_GAP))
  assert gaps_ok or not need_gaps, (tag, 'a reference gap below MIN_GAP: change the seed of the case', ref['gaps'].tolist())
  worst_valid = 0.0
  for i in range(k):                                       # greedy-valid, whatever the gaps
    z = step_sums_ref(dist, chosen[:i].tolist())
    assert z[chosen[i]] <= z.min() * (1 + 3 * r), (tag, 'step', i, float(z[chosen[i]]), float(z.min()))
    err = abs(objective[i] - z[chosen[i]] / S)
    assert err <= r * z[chosen[i]] / S, (tag, 'objective', i, err)
    worst_valid = max(worst_valid, err / (r * z[chosen[i]] / S) if z[chosen[i]] > 0 else 0.0)
  assert np.all(np.diff(objective) <= 0), (tag, 'objective increases')
  if gaps_ok:
    assert np.array_equal(chosen, ref['chosen']), (tag, chosen.tolist(), ref['chosen'].tolist())
  own_dist, own_ydist = own
  fin = finish_ref(own_dist, chosen, own_ydist)            # what follows from the selection, on its own matrix
  for key in ('assign', 'nearest', 'prob'):
    assert key not in got or np.array_equal(np.asarray(got[key], dtype=np.float64), np.asarray(fin[key], dtype=np.float64)), (tag, key)
  if ydist is not None:
    assert int(got['obs_nearest']) == fin['obs_nearest'] and np.array_equal(got['obs'], fin['obs']), (tag, 'obs')
    if gaps_ok:
      d0 = ydist[chosen].min()
      assert abs(got['obs'][0] - d0) <= cell_bar(C, d0), (tag, 'obs[0] against the reference')
  print(f'{tag}: min gap {ref["gaps"].min():.3g} ({"exact chosen demanded" if gaps_ok else "greedy-valid only"}); '
        f'objective error / bar {worst_valid:.3f}')
  return ref


# ---- the shared cases (computed once, read-only) ---------------------------------------------------------------------
def _frozen(*arrays):
  for a in arrays:
    if isinstance(a, np.ndarray):
      a.setflags(write=False)


def make_x(S, C, kind, rng):
  if kind == 'normal':                    # 100 + a factor shared by the columns of a path + noise
    return 100.0 + 10.0 * rng.standard_normal((S, 1)) * rng.uniform(0.5, 1.5, C)[None, :] + rng.standard_normal((S, C)) * 3.0
  if kind == 'counts':                    # Poisson(1): with few columns the paths repeat
    x = rng.poisson(1.0, (S, C)).astype(np.float64)
    if C <= 3 and S >= 32:
      assert len(np.unique(x, axis=0)) < S, 'the counts case is there for repeated paths'
    return x
  if kind == 'big':                       # a total of 1e9 with a spread of 10
    return 1e9 + 10.0 * rng.standard_normal((S, C))
  if kind == 'clusters':                  # three well-separated blobs, of sizes 5 : 3 : 2 in every ten paths
    blob = np.asarray([0, 0, 0, 0, 0, 1, 1, 1, 2, 2])[np.arange(S) % 10]
    centre = np.asarray([0.0, 1000.0, -2000.0])[blob]
    return centre[:, None] * np.linspace(1.0, 2.0, C)[None, :] + rng.standard_normal((S, C))
  raise ValueError(kind)


def make_y(x, kind, rng):
  """One more path of the same kind; NaN in the columns c = 3 (mod 5)."""
  S, C = x.shape
  y = x[rng.integers(0, S)] + (rng.integers(-2, 3, C).astype(np.float64) if kind == 'counts' else rng.standard_normal(C))
  y[3::5] = np.nan
  return y


def make_scale(C, rng):
  return rng.uniform(0.5, 40.0, C)


@functools.lru_cache(maxsize=None)
def scenario_case(S, C, kind, seed=0):
  """-> (x (S, C), y (C,), scale (C,)), read-only."""
  rng = np.random.default_rng([S, C, KINDS.index(kind), seed, 41])
  x = make_x(S, C, kind, rng)
  y = make_y(x, kind, rng)
  scale = make_scale(C, rng)
  _frozen(x, y, scale)
  return x, y, scale


@functools.lru_cache(maxsize=None)
def distance_case(S, C, kind, p, scaled, with_y):
  """-> (x, y or None, scale or None, (dist_ref, ydist_ref)), the brute force computed once."""
  x, y, scale = scenario_case(S, C, kind)
  y, scale = (y if with_y else None), (scale if scaled else None)
  ref = distances_ref(x, p, scale, y)
  _frozen(*ref)
  return x, y, scale, ref


@functools.lru_cache(maxsize=None)
def selection_case(S, C, kind, p, k=SELECT_K):
  """-> (x, y, (dist_ref, ydist_ref), select_ref on them): scale off, y on."""
  x, y, _, ref = distance_case(S, C, kind, p, False, True)
  sel = select_ref(ref[0], min(k, S), ref[1])
  _frozen(*sel.values())
  return x, y, ref, sel


def integer_matrix(S, kind, seed=0):
  """Hand-made symmetric integer distance matrices with a zero diagonal: 'random' (entries 1 .. 9), 'duplicates' (the
  1-norm distances of S paths of two small counts: repeated paths), 'equal' (every off-diagonal entry 7: every candidate
  ties at every step), 'zero' (all paths identical)."""
  rng = np.random.default_rng([S, seed, 43])
  if kind == 'random':
    a = rng.integers(1, 10, (S, S)).astype(np.float64)
    d = np.triu(a, 1)
    return d + d.T
  if kind == 'duplicates':
    x = rng.integers(0, 3, (S, 2)).astype(np.float64)
    return np.abs(x[:, None, :] - x[None, :, :]).sum(axis=2)
  if kind == 'equal':
    return 7.0 * (1.0 - np.eye(S))
  if kind == 'zero':
    return np.zeros((S, S))
  raise ValueError(kind)
