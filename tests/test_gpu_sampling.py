"""Posterior-predictive sample paths and group totals drawn on the GPU (include/bnf.h bnf_predictive_samples /
bnf_predictive_group_sums), against the float64 oracle evaluated on the same float32 inputs.

The law is checked with the Dvoretzky-Kiefer-Wolfowitz bound: for S i.i.d. draws the sup-distance D between the
empirical CDF and the true one exceeds eps = sqrt(ln(2 / alpha) / (2 S)) with probability <= alpha, for ANY law
(discrete ones included).  alpha = 1e-9 and S = 32768 give eps = 0.0181: derived, not tuned."""
import math
import os

import numpy as np
import pandas as pd
import pytest
import torch

from bayesnf_amd import BayesianNeuralFieldMAP, BayesianNeuralFieldVI, inference
from bayesnf_amd.engine import Engine
from oracle import bnf_oracle as O
from tests import util

pytestmark = pytest.mark.gpu

S = 32768
ALPHA = 1e-9


def dkw_eps(n):
  return math.sqrt(math.log(2.0 / ALPHA) / (2.0 * n))


EPS = dkw_eps(S)
TCS = (0.05, 0.3, 1.0, 3.0, 40.0, 1e3)
MEANS = (0.02, 0.7, 5.0, 30.0, 400.0, 2e4, 1e6)
PI = 0.35
# the M = 7 members: total_count and mean of member m are the grid values times these
TC_F = (1.0, 0.6, 0.8, 1.25, 1.5, 2.0, 0.5)
MEAN_F = (1.0, 0.5, 2.0, 0.7, 1.4, 3.0, 0.3)


def inv_softplus(y):
  """log(expm1(y)), evaluated without overflow (y > 30: y + log1p(-e^-y) = y to 1e-13)."""
  y = np.asarray(y, dtype=np.float64)
  return np.where(y > 30.0, y, np.log(np.expm1(np.minimum(y, 30.0))))


def _engine(obs):
  net, model, _, _ = util.make_problem(n_rows=16, width=64, depth=1, observation_model=obs)
  return Engine(net, members=1, forward_only=True, row_capacity=128, compute_dtype='fp32'), model


def _dev(eng, a):
  return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(eng.device)


def count_case(model, tc, M):
  """One row per grid mean at total_count `tc`: aux[1] = 1 / tc, loc = log(expm1(tc^2 / mean)) as float32 device
  inputs, and the oracle's forecast (count_forecast) of exactly those float32 values."""
  tcs = tc * np.asarray(TC_F[:M])
  means = np.asarray(MEANS)[None, :] * np.asarray(MEAN_F[:M])[:, None]
  aux = np.stack([np.ones(M), 1.0 / tcs, np.full(M, PI)], axis=1).astype(np.float32)
  loc = inv_softplus(tcs[:, None] ** 2 / means).astype(np.float32)
  theta = np.zeros((M, model.P))
  theta[:, model.leaf['shape'].offset] = inv_softplus(aux[:, 1].astype(np.float64))
  p = aux[:, 2].astype(np.float64)
  theta[:, model.leaf['inflated_loc_probs'].offset] = np.log(p) - np.log1p(-p)
  fc = O.count_forecast(model, theta, loc.astype(np.float64))
  np.testing.assert_allclose(fc['tc'][:, 0], tcs, rtol=1e-6)
  want = means * ((1 - PI) if model.observation_model == 'ZINB' else 1.0)
  np.testing.assert_allclose(fc['mean'], want, rtol=2e-5)     # float32 loc: 19.8 x 6e-8 at the far corner
  return loc, aux, fc


def fc_row(fc, r, tc_scale=1.0):
  """The forecast of row r alone; tc_scale != 1: total_count scaled at equal mean (the sharpness alternative)."""
  return dict(tc=fc['tc'] * tc_scale, logits=fc['logits'][:, r:r + 1] - math.log(tc_scale), pi=fc['pi'])


def dkw_counts(x, mix_cdf):
  """sup |F_n - F| of integer-valued samples x: at every distinct sampled value, on both sides of the jump.
  mix_cdf(k) = mixture CDF at the integers k (k = -1 gives 0)."""
  ks, cnt = np.unique(np.asarray(x, dtype=np.float64), return_counts=True)
  assert ks[0] >= 0 and np.all(ks == np.floor(ks)), 'count samples must be non-negative integers'
  fn = np.cumsum(cnt) / len(x)
  fn_left = fn - cnt / len(x)
  return max(np.abs(fn - mix_cdf(ks)).max(), np.abs(fn_left - mix_cdf(ks - 1.0)).max())


def oracle_count_cdf(fcr):
  def cdf(k):
    k = np.asarray(k, dtype=np.float64)
    return np.where(k < 0, 0.0, O.count_cdf(fcr, np.maximum(k, 0.0)[None, :]).mean(axis=0))
  return cdf


def dkw_continuous(x, cdf):
  xs = np.sort(np.asarray(x, dtype=np.float64))
  f = cdf(xs)
  n = len(xs)
  return max((np.arange(1, n + 1) / n - f).max(), (f - np.arange(n) / n).max())


@pytest.mark.parametrize('M', [1, 7])
@pytest.mark.parametrize('obs', ['NB', 'ZINB'])
def test_marginal_law_of_counts_and_its_sharpness(obs, M):
  """(1) every row of the grid total_count x mean: D <= eps against the oracle's mixture CDF.
  (2) sharpness, on the rows with total_count <= 1 and mean >= 30: against the oracle CDF with total_count scaled by
  1.2 at equal mean D must EXCEED eps, or a sampler that ignores the dispersion would pass (1).  Asserted for the plain
  NB with one component, where the two laws are >= 0.033 apart (numpy's Gamma-Poisson sampler on this grid); zero
  inflation multiplies every CDF difference by 1 - pi = 0.65 and seven members of different dispersion average
  differences that peak at different counts, so there the alternative lies within ~eps of the truth (0.018 .. 0.029) and
  the distance is printed only."""
  eng, model = _engine(obs)
  worst, rows = 0.0, []
  for tc in TCS:
    loc, aux, fc = count_case(model, tc, M)
    x = eng.predictive_samples(_dev(eng, loc), _dev(eng, aux), S, seed=1234).cpu().numpy()
    assert x.shape == (S, len(MEANS)) and x.dtype == np.float32
    for r, mean in enumerate(MEANS):
      d = dkw_counts(x[:, r], oracle_count_cdf(fc_row(fc, r)))
      d_alt = dkw_counts(x[:, r], oracle_count_cdf(fc_row(fc, r, 1.2)))
      print(f'{obs} M={M} tc={tc:g} mean={mean:g}: D={d:.4f} D(1.2 tc)={d_alt:.4f} sample mean={x[:, r].mean():.5g}')
      rows.append((tc, mean, d, d_alt))
      worst = max(worst, d)
  eng.close()
  for tc, mean, d, d_alt in rows:
    assert d <= EPS, (obs, M, tc, mean, d)
    if obs == 'NB' and M == 1 and tc <= 1 and mean >= 30:
      assert d_alt > EPS, (obs, M, tc, mean, d_alt)


@pytest.mark.parametrize('M', [1, 7])
def test_marginal_law_normal(M):
  """NORMAL: scales over four decades (one call per scale: the scale is per member), locations from -1e3 to 1e3."""
  eng, _ = _engine('NORMAL')
  rng = np.random.default_rng(3)
  for scale in (0.01, 0.1, 1.0, 10.0, 100.0):
    scales = (scale * np.asarray(TC_F[:M])).astype(np.float32)
    loc = np.stack([np.asarray([-1e3, -1.0, 0.0, 0.5, 7.0, 1e3]) + scale * k * rng.standard_normal(6)
                    for k in range(M)]).astype(np.float32)
    aux = np.stack([scales, np.ones(M), np.zeros(M)], axis=1).astype(np.float32)
    x = eng.predictive_samples(_dev(eng, loc), _dev(eng, aux), S, seed=99).cpu().numpy()
    assert x.shape == (S, 6) and x.dtype == np.float32
    for r in range(6):
      d = dkw_continuous(x[:, r], lambda v: O.mixture_cdf(loc[:, r:r + 1].astype(np.float64), scales.astype(np.float64), v))
      print(f'NORMAL M={M} scale={scale:g} row {r}: D={d:.4f}')
      assert d <= EPS, (M, scale, r, d)
  eng.close()


def test_path_coherence_and_component_law():
  """A sample path uses ONE member for all its rows, and the members are drawn with equal weights."""
  eng, _ = _engine('NORMAL')
  M, R = 8, 64
  loc = np.repeat(100.0 * np.arange(M)[:, None], R, axis=1)
  aux = np.stack([np.full(M, 0.01), np.ones(M), np.zeros(M)], axis=1)
  x = eng.predictive_samples(_dev(eng, loc), _dev(eng, aux), S, seed=7).cpu().numpy().astype(np.float64)
  eng.close()
  member = np.rint(x / 100.0).astype(int)
  assert np.abs(x - 100.0 * member).max() < 0.1                      # 10 sigma
  assert np.all(member == member[:, :1]), 'a path mixed members across its rows'
  freq = np.bincount(member[:, 0], minlength=M) / S
  print('member frequencies', freq)
  assert member.min() >= 0 and member.max() < M and np.abs(freq - 1.0 / M).max() <= EPS
  assert np.std(x - 100.0 * member, axis=0).min() > 0.009             # and the rows carry their own noise


def _mixed_inputs(obs, M, R, seed):
  rng = np.random.default_rng(seed)
  if obs == 'NORMAL':
    loc = 50.0 * rng.standard_normal((M, R))
    aux = np.stack([rng.uniform(0.5, 3.0, M), np.ones(M), np.zeros(M)], axis=1)
  else:
    tcs = np.asarray([0.3, 1.0, 5.0, 60.0])[:M]
    means = np.exp(rng.uniform(np.log(0.05), np.log(3e3), (M, R)))
    loc = inv_softplus(tcs[:, None] ** 2 / means)
    aux = np.stack([np.ones(M), 1.0 / tcs, np.full(M, PI)], axis=1)
  return loc.astype(np.float32), aux.astype(np.float32)


@pytest.mark.parametrize('obs', ['NORMAL', 'NB', 'ZINB'])
def test_draws_are_a_pure_function_of_seed_path_and_global_row(obs):
  """Counter-based: a row chunk drawn with row0, a sample chunk drawn with sample0, reproduce the slice of the one
  big call bit for bit; the same seed twice gives the same array, another seed another one."""
  eng, _ = _engine(obs)
  M, R, n = 4, 3001, 50
  loc, aux = _mixed_inputs(obs, M, R, 11)
  loc_d, aux_d = _dev(eng, loc), _dev(eng, aux)
  full = eng.predictive_samples(loc_d, aux_d, n, seed=5).cpu().numpy()
  assert np.all(np.isfinite(full))
  for a, b in ((0, 1), (1, 1025), (1023, 2049), (2990, 3001), (700, 707)):
    part = eng.predictive_samples(loc_d[:, a:b], aux_d, n, seed=5, row0=a).cpu().numpy()
    assert np.array_equal(part, full[:, a:b]), (a, b)
  for s0, k in ((0, 1), (17, 20), (49, 1)):
    part = eng.predictive_samples(loc_d, aux_d, k, seed=5, sample0=s0).cpu().numpy()
    assert np.array_equal(part, full[s0:s0 + k]), (s0, k)
  assert np.array_equal(eng.predictive_samples(loc_d, aux_d, n, seed=5).cpu().numpy(), full)
  other = eng.predictive_samples(loc_d, aux_d, n, seed=6).cpu().numpy()
  assert np.mean(other != full) > 0.3
  eng.close()


def _random_grouping(R, rng):
  """Group sizes 1 .. 5000 plus one group holding half the rows; segment edges on and off the 1024-row tile edges;
  a few empty groups; rows in random order."""
  sizes = [1024, 2048, 1, 1023, 3, 0, 5000, R // 2, 0, 1, 1, 1]
  menu = [1, 1, 1, 2, 3, 7, 40, 300, 1024, 2500, 5000]
  while sum(sizes) < R:
    sizes.append(min(int(rng.choice(menu)), R - sum(sizes)))
  sizes.append(0)
  codes = np.repeat(np.arange(len(sizes)), sizes)
  assert len(codes) == R
  return rng.permutation(codes), len(sizes)


@pytest.mark.parametrize('obs', ['NORMAL', 'NB', 'ZINB'])
def test_group_sums_equal_the_host_sums_of_the_per_row_draws(obs):
  """predictive_group_sums == float64 host sum by group of predictive_samples for the same seed: counts exactly,
  NORMAL within 1e-12 sum |x| per cell (n 2^-53 for n <= 1e4 terms bounds ANY summation order); two runs bitwise equal."""
  eng, _ = _engine(obs)
  M, R, n = 4, 40000 + 37, 24
  rng = np.random.default_rng(5)
  loc, aux = _mixed_inputs(obs, M, R, 21)
  codes, G = _random_grouping(R, rng)
  off, rows = inference.csr_from_codes(codes, G)
  loc_d, aux_d = _dev(eng, loc), _dev(eng, aux)
  x = eng.predictive_samples(loc_d, aux_d, n, seed=42).cpu().numpy().astype(np.float64)
  want = np.stack([np.bincount(codes, weights=x[s], minlength=G) for s in range(n)])
  absum = np.stack([np.bincount(codes, weights=np.abs(x[s]), minlength=G) for s in range(n)])
  got = eng.predictive_group_sums(loc_d, aux_d, off, rows, n, seed=42)
  assert got.shape == (n, G) and got.dtype == torch.float64
  got = got.cpu().numpy()
  again = eng.predictive_group_sums(loc_d, aux_d, off, rows, n, seed=42).cpu().numpy()
  eng.close()
  err = np.abs(got - want)
  print(f'{obs}: {G} groups, max |device - host| = {err.max():.3e}, max sum|x| = {absum.max():.3e}')
  assert np.array_equal(got.view(np.int64), again.view(np.int64)), 'two runs differ'
  assert np.all(got[:, np.bincount(codes, minlength=G) == 0] == 0.0)     # empty groups
  if obs == 'NORMAL':
    assert np.all(err <= 1e-12 * absum), float((err - 1e-12 * absum).max())
  else:
    assert np.array_equal(got, want)


MODEL = dict(width=64, depth=2, seasonality_periods=np.asarray([4.0, 52.1775]),
             num_seasonal_harmonics=np.asarray([2.0, 10]), feature_cols=['datetime', 'latitude', 'longitude'],
             target_col='chickenpox', timetype='index', freq='W', standardize=['latitude', 'longitude'])


def _frame(golden_dir):
  return pd.read_csv(os.path.join(golden_dir, 'chickenpox.8.train.csv'), index_col=0, parse_dates=['datetime'])


def _fit(golden_dir, kind):
  df = _frame(golden_dir)
  if kind == 'map':
    est = BayesianNeuralFieldMAP(**MODEL, observation_model='NB', compute_dtype='fp32').fit(
        df, seed=3, ensemble_size=4, num_epochs=40, learning_rate=0.01)
  else:
    est = BayesianNeuralFieldVI(**MODEL, observation_model='NORMAL', compute_dtype='fp32').fit(
        df, seed=1, ensemble_size=2, num_epochs=30, learning_rate=0.01, sample_size_posterior=5)
  return df, est


def _rowwise_mixture_cdf(lik, pts):
  """lik.mixture_cdf at pts (K, R): one call per evaluation level (mixture_cdf takes one point per row)."""
  return np.stack([lik.mixture_cdf(pts[i]) for i in range(pts.shape[0])])


@pytest.mark.parametrize('kind', ['map', 'vi'])
def test_estimator_sample_paths_end_to_end(golden_dir, kind, monkeypatch):
  """chickenpox fixture, NB for MAP and NORMAL for VI (posterior draws count as components): totals by time step have
  the exact mixture mean within a 6-sigma CLT bound; the per-row draws pass the DKW check against
  likelihood_model(test).mixture_cdf; shapes and dtypes; a forced small row chunk gives the same array."""
  df, est = _fit(golden_dir, kind)
  n = 4096
  totals, keys = est.predict_samples(df, n, seed=11, group_by='datetime')
  assert isinstance(keys, pd.Index) and keys.is_monotonic_increasing and set(keys) == set(df['datetime'])
  G = len(keys)
  assert totals.shape == (n, G) and totals.dtype == np.float64
  lik = est.likelihood_model(df)
  R = len(df)
  mu = np.asarray(lik.mean(), dtype=np.float64).reshape(-1, R)
  sd = np.asarray(lik.stddev(), dtype=np.float64).reshape(-1, R)
  assert mu.shape[0] == (4 if kind == 'map' else 10)
  code = keys.get_indexer(df['datetime'])
  for g in range(G):
    sel = code == g
    t_m, v_m = mu[:, sel].sum(axis=1), (sd[:, sel] ** 2).sum(axis=1)     # rows are independent given the member
    mean = t_m.mean()
    var = v_m.mean() + (t_m ** 2).mean() - mean ** 2                      # law of total variance across members
    got = totals[:, g].mean()
    print(f'{kind} group {g}: sample mean {got:.4f}, exact {mean:.4f}, 6 sd / sqrt(S) = {6 * math.sqrt(var / n):.4f}')
    assert abs(got - mean) <= 6.0 * math.sqrt(var / n), (g, got, mean, var)
  # two key columns: a MultiIndex, and the totals over everything add up
  t2, k2 = est.predict_samples(df, 64, seed=11, group_by=['latitude', 'longitude'])
  assert isinstance(k2, pd.MultiIndex) and t2.shape == (64, len(k2)) and t2.dtype == np.float64
  np.testing.assert_allclose(t2.sum(axis=1), totals[:64].sum(axis=1), rtol=1e-12)

  x = est.predict_samples(df, S, seed=11)
  assert x.shape == (S, R) and x.dtype == np.float32
  np.testing.assert_allclose(np.stack([np.bincount(code, weights=x[s].astype(np.float64), minlength=G) for s in range(64)]),
                             totals[:64], rtol=1e-12, atol=1e-9)         # the same paths, grouped or not
  if kind == 'vi':
    xs = np.sort(x.astype(np.float64), axis=0)
    f = _rowwise_mixture_cdf(lik, xs)
    up = (np.arange(1, S + 1)[:, None] / S - f).max(axis=0)
    dn = (f - np.arange(S)[:, None] / S).max(axis=0)
    d = np.maximum(up, dn)
  else:
    assert x.min() >= 0 and np.all(x == np.floor(x))
    d = np.zeros(R)
    uniq = [np.unique(x[:, r].astype(np.float64), return_counts=True) for r in range(R)]
    kmax = max(len(u[0]) for u in uniq)
    pts = np.stack([np.pad(u[0], (0, kmax - len(u[0])), mode='edge') for u in uniq], axis=1)      # (kmax, R)
    f, f_left = _rowwise_mixture_cdf(lik, pts), _rowwise_mixture_cdf(lik, pts - 1.0)
    for r, (ks, cnt) in enumerate(uniq):
      fn = np.cumsum(cnt) / S
      d[r] = max(np.abs(fn - f[:len(ks), r]).max(), np.abs(fn - cnt / S - f_left[:len(ks), r]).max())
  print(f'{kind}: per-row DKW distances max {d.max():.4f} (eps {EPS:.4f})')
  assert np.all(d <= EPS), d.max()

  # the row chunking of the seam does not enter the values
  small = est.predict_samples(df, 200, seed=11)
  monkeypatch.setattr(inference, '_SAMPLE_CHUNK_CELLS', 200 * 7)
  assert np.array_equal(est.predict_samples(df, 200, seed=11), small)
  assert np.array_equal(small, x[:200])
