// bnf_forecast.hip -- the forecast entry points of libbnf_hip.so (include/bnf.h): mixture quantiles, posterior-predictive
// sample paths and their group reductions, held-out scores, the ranked probability score, stacking, and the summaries,
// dependence, scenarios, ranks and bands of sample paths.
//
// None of them touches training state.  bnf_handle is an opaque type in this unit: an entry point asks the engine unit
// for the Forecast view of its handle (bnf_host.h) -- bound, device, observation model, stream, quantile scratch -- and
// the compiler refuses anything else.  No training kernel is compiled here: the headers below stop at bnf_device.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "../../include/bnf.h"
#include "bnf_host.h"
#include "bnf_quantiles.h"
#include "bnf_sampling.h"
#include "bnf_combinations.h"
#include "bnf_extremes.h"
#include "bnf_episodes.h"
#include "bnf_cumulative.h"
#include "bnf_windows.h"
#include "bnf_scoring.h"
#include "bnf_rps.h"
#include "bnf_totals.h"
#include "bnf_dependence.h"
#include "bnf_ranking.h"
#include "bnf_bands.h"
#include "bnf_scenarios.h"
#include "bnf_stacking.h"

using namespace bnf;

// the observation model of the handle as a compile-time constant: f(tag) with decltype(tag)::value the BNF_OBS_* code
template <typename F>
static void with_obs(const Forecast& fc, F&& f) {
  switch (fc.obs_model) {
    case BNF_OBS_NORMAL: f(std::integral_constant<int, BNF_OBS_NORMAL>{}); break;
    case BNF_OBS_NB: f(std::integral_constant<int, BNF_OBS_NB>{}); break;
    default: f(std::integral_constant<int, BNF_OBS_ZINB>{}); break;
  }
}

// the passes of a group reduction through its work buffer, `chunk` sample paths each (group_chunk): launch(obs, s0, n)
// enqueues the n paths from s0 on, obs as in with_obs
template <typename F>
static void group_passes(const Forecast& fc, int64_t n_samples, int64_t chunk, F&& launch) {
  with_obs(fc, [&](auto obs) {
    for (int64_t s0 = 0; s0 < n_samples; s0 += chunk) launch(obs, s0, std::min(chunk, n_samples - s0));
  });
}

// the launch shape of the sample-path kernels: x = blocks of `per_block` rows (positions), y = the samples, strided; the
// combine kernel of a group reduction (one wave per tile and sample) takes (grid.x, cdiv(S, 4)).
// tests/test_gpu_sampler_law.py restates gy (group_sums_sample_stride) to test the totals for correlation at that lag:
// change both together.
static dim3 pred_grid(int64_t R, int64_t per_block, int64_t S) {
  const int64_t gx = cdiv(R, per_block);
  const int64_t gy = std::min<int64_t>(std::min<int64_t>(S, 65535), std::max<int64_t>(1, 16384 / gx));
  return dim3((unsigned)gx, (unsigned)gy);
}

// posterior-predictive sampling launches (bnf_sampling.h), one instantiation per observation model
template <int OBS>
static void launch_predictive_samples(const Forecast& fc, const float* loc, const float* aux, int64_t M, int64_t R, int64_t S,
                                      uint64_t seed, int64_t row0, int64_t sample0, const double* cum, float* out) {
  hipLaunchKernelGGL((k_predictive_samples<OBS>), pred_grid(R, 256 * kPredRowsPerThread, S), dim3(256), 0, fc.stream, loc,
                     aux, (int32_t)M, R, S, seed, row0, sample0, cum, out);
}

// held-out scoring launches (bnf_scoring.h), one instantiation per observation model and for the member weights wts
// (WEIGHTED: wts non-null, no member_ll)
template <int OBS, bool WEIGHTED>
static void launch_predictive_scores(const Forecast& fc, const float* loc, const float* aux, const double* wts, int64_t M,
                                     int64_t R, const float* y, double* ll_partial, double* pair_partial, int64_t n_slots, double* member_ll,
                                     float* lpd, float* pit, float* crps) {
  const int64_t nt = cdiv(R, kScoreTile);
  if (member_ll) {
    hipLaunchKernelGGL((k_score_member_ll<OBS>), dim3((unsigned)nt, (unsigned)std::min<int64_t>(M, 65535)), dim3(256), 0,
                       fc.stream, loc, aux, (int32_t)M, R, y, ll_partial);
    hipLaunchKernelGGL(k_score_member_ll_combine, dim3(cdiv(M, 4)), dim3(256), 0, fc.stream, ll_partial, (int32_t)M, nt,
                       member_ll);
  }
  if (crps)
    hipLaunchKernelGGL((k_score_crps_pairs<WEIGHTED>), dim3((unsigned)nt, (unsigned)n_slots), dim3(256), 0, fc.stream, loc,
                       aux, wts, (int32_t)M, R, pair_partial);
  if (lpd || crps || (pit && OBS == BNF_OBS_NORMAL))
    hipLaunchKernelGGL((k_score_rows<OBS, WEIGHTED>), dim3(cdiv(R, 64)), dim3(64), 0, fc.stream, loc, aux, wts, (int32_t)M, R, y,
                       pair_partial, (int32_t)n_slots, lpd, pit, crps);
  if (pit && OBS != BNF_OBS_NORMAL)
    hipLaunchKernelGGL((k_score_count_pit<WEIGHTED>), dim3(cdiv(R, 64), 2), dim3(64), 0, fc.stream, loc, aux, wts, (int32_t)M, R,
                       (int32_t)OBS, y, pit);
}

// ranked probability score (bnf_rps.h): one wave per row, the rows beyond 2^20 blocks by grid stride
template <int OBS, bool WEIGHTED>
static void launch_count_rps(const Forecast& fc, const float* loc, const float* aux, const double* wts, int64_t M, int64_t R,
                             const float* y, float* rps) {
  static std::atomic<uint64_t> attr_done{0};
  allow_lds(fc.device, &k_count_rps<OBS, WEIGHTED>, (int)rps_lds_bytes(BNF_RPS_MAX_MEMBERS), &attr_done);
  hipLaunchKernelGGL((k_count_rps<OBS, WEIGHTED>), dim3((unsigned)std::min<int64_t>(R, 1 << 20)), dim3(64), rps_lds_bytes(M),
                     fc.stream, loc, aux, wts, (int32_t)M, R, y, rps);
}

// summaries of sample paths (bnf_totals.h): one workgroup per slab of C adjacent columns, C * P <= 16,384 doubles of LDS
static void launch_sample_summaries(const Forecast& fc, const double* x, int64_t S, int64_t G, const double* y,
                                    const SummaryQ& q, double* mean, double* quant, double* crps, double* pit) {
  int P = 1;
  while (P < S) P <<= 1;
  const int C = std::min(kSumMaxCols, kSumMaxSamples / P);
  const int threads = std::min(1024, std::max(64, C * P / 2));          // a multiple of 64: C * P is a power of two
  static std::atomic<uint64_t> attr_done{0};
  allow_lds(fc.device, &k_sample_summaries, (int)(sizeof(double) * kSumMaxSamples), &attr_done);
  hipLaunchKernelGGL(k_sample_summaries, dim3(cdiv(G, C)), dim3(threads), sizeof(double) * (size_t)C * (size_t)P, fc.stream,
                     x, (int32_t)S, G, (int32_t)P, (int32_t)C, y, q, mean, quant, crps, pit);
}

extern "C" {

// wts: the member weights of the *_weighted entry points, DEVICE (n_members,) f64; NULL = the equal-weight kernels
static int normal_mixture_quantiles_impl(const Forecast& fc, const float* means, const float* scales, const double* wts,
                                         int64_t n_members, int64_t n_rows, const float* q, int32_t n_q,
                                         int32_t approximate, float* out) {
  if (!fc.bound) return fail(BNF_ERR_STATE, "not bound");
  if (!means || !scales || !q || !out || n_members < 1 || n_rows < 1 || n_q < 0)
    return fail(BNF_ERR_INVALID, "argument");
  HIPCHK(hipSetDevice(fc.device));
  float* mpart = fc.qscratch;
  float* spart = fc.qscratch + 2048;
  float* bracket = fc.qscratch + 4096;
  if (!approximate) {
    const int nb_m = (int)std::min<int64_t>(1024, cdiv(n_members * n_rows, 256));
    const int nb_s = (int)std::min<int64_t>(1024, cdiv(n_members, 256));
    hipLaunchKernelGGL(k_minmax_partial, dim3(nb_m), dim3(256), 0, fc.stream, means,
                       n_members * n_rows, mpart);
    hipLaunchKernelGGL(k_minmax_partial, dim3(nb_s), dim3(256), 0, fc.stream, scales, n_members, spart);
    hipLaunchKernelGGL(k_bracket, dim3(1), dim3(64), 0, fc.stream, mpart, nb_m, spart, nb_s, bracket);
  }
  for (int i = 0; i < n_q; ++i) {
    float* o = out + (int64_t)i * n_rows;
    const dim3 grid(cdiv(n_rows, 256));
    if (approximate && wts)
      hipLaunchKernelGGL(k_quantile_approx<true>, grid, dim3(256), 0, fc.stream, means, scales, wts, n_members, n_rows, q[i], o);
    else if (approximate)
      hipLaunchKernelGGL(k_quantile_approx<false>, grid, dim3(256), 0, fc.stream, means, scales, wts, n_members, n_rows, q[i], o);
    else if (wts)
      hipLaunchKernelGGL(k_quantile_root<true>, grid, dim3(256), 0, fc.stream, means, scales, wts, n_members, n_rows, bracket, q[i], o);
    else
      hipLaunchKernelGGL(k_quantile_root<false>, grid, dim3(256), 0, fc.stream, means, scales, wts, n_members, n_rows, bracket, q[i], o);
  }
  HIPCHK(hipGetLastError());
  return BNF_OK;
}

int bnf_normal_mixture_quantiles(bnf_handle* h, const float* means, const float* scales,
                                 int64_t n_members, int64_t n_rows, const float* q, int32_t n_q,
                                 int32_t approximate, float* out) {
  const Forecast fc = forecast_view(h);
  return normal_mixture_quantiles_impl(fc, means, scales, nullptr, n_members, n_rows, q, n_q, approximate, out);
}

static int count_mixture_quantiles_impl(const Forecast& fc, const float* loc, const float* aux, const double* wts,
                                        int64_t n_members, int64_t n_rows, const float* q, int32_t n_q,
                                        float* means, float* out) {
  if (!fc.bound) return fail(BNF_ERR_STATE, "not bound");
  if (fc.obs_model != BNF_OBS_NB && fc.obs_model != BNF_OBS_ZINB)
    return fail(BNF_ERR_STATE, "handle's observation model is not NB / ZINB");
  if (!loc || !aux || !means || n_members < 1 || n_rows < 1 || n_q < 0 || (n_q > 0 && (!q || !out)))
    return fail(BNF_ERR_INVALID, "argument");
  for (int i = 0; i < n_q; ++i)
    if (!(q[i] > 0.f && q[i] < 1.f)) return fail(BNF_ERR_INVALID, "quantile %g outside (0, 1)", q[i]);
  HIPCHK(hipSetDevice(fc.device));
  float* part = fc.qscratch;
  float* bracket = fc.qscratch + 4096;
  const int nb = (int)std::min<int64_t>(1024, cdiv(n_members * n_rows, 256));
  hipLaunchKernelGGL(k_count_moments, dim3(nb), dim3(256), 0, fc.stream, loc, aux, n_members, n_rows,
                     fc.obs_model, means, part);
  hipLaunchKernelGGL(k_count_bracket, dim3(1), dim3(64), 0, fc.stream, part, nb, bracket);
  for (int i = 0; i < n_q; ++i) {
    if (wts)
      hipLaunchKernelGGL(k_count_quantile_root<true>, dim3(cdiv(n_rows, 64)), dim3(64), 0, fc.stream, loc, aux, wts,
                         n_members, n_rows, fc.obs_model, bracket, q[i], out + (int64_t)i * n_rows);
    else
      hipLaunchKernelGGL(k_count_quantile_root<false>, dim3(cdiv(n_rows, 64)), dim3(64), 0, fc.stream, loc, aux, wts,
                         n_members, n_rows, fc.obs_model, bracket, q[i], out + (int64_t)i * n_rows);
  }
  HIPCHK(hipGetLastError());
  return BNF_OK;
}

int bnf_count_mixture_quantiles(bnf_handle* h, const float* loc, const float* aux,
                                int64_t n_members, int64_t n_rows, const float* q, int32_t n_q,
                                float* means, float* out) {
  const Forecast fc = forecast_view(h);
  return count_mixture_quantiles_impl(fc, loc, aux, nullptr, n_members, n_rows, q, n_q, means, out);
}


// ---- posterior-predictive sampling (bnf_sampling.h) -----------------------------
static int predictive_args(const Forecast& fc, const float* loc, const float* aux, int64_t n_members, int64_t n_rows,
                           int64_t n_samples, int64_t row0, int64_t sample0) {
  if (!fc.bound) return fail(BNF_ERR_STATE, "not bound");
  if (!loc || !aux || n_members < 1 || n_members > 0x7fffffffLL || n_rows < 1 || n_rows > 0x7fffffffLL || n_samples < 1)
    return fail(BNF_ERR_INVALID, "argument");
  if (row0 < 0 || row0 + n_rows > (1LL << 56)) return fail(BNF_ERR_INVALID, "row0 + n_rows exceeds 2^56");
  if (sample0 < 0 || sample0 + n_samples > (1LL << 32)) return fail(BNF_ERR_INVALID, "sample0 + n_samples exceeds 2^32");
  return BNF_OK;
}

static int predictive_samples_impl(const Forecast& fc, const float* loc, const float* aux, int64_t n_members, int64_t n_rows,
                                   int64_t n_samples, uint64_t seed, int64_t row0, int64_t sample0, const double* cum,
                                   float* out) {
  if (const int rc = predictive_args(fc, loc, aux, n_members, n_rows, n_samples, row0, sample0)) return rc;
  if (!out) return fail(BNF_ERR_INVALID, "argument");
  HIPCHK(hipSetDevice(fc.device));
  with_obs(fc, [&](auto obs) {
    launch_predictive_samples<decltype(obs)::value>(fc, loc, aux, n_members, n_rows, n_samples, seed, row0, sample0, cum, out);
  });
  HIPCHK(hipGetLastError());
  return BNF_OK;
}

int bnf_predictive_samples(bnf_handle* h, const float* loc, const float* aux, int64_t n_members, int64_t n_rows,
                           int64_t n_samples, uint64_t seed, int64_t row0, int64_t sample0, float* out) {
  const Forecast fc = forecast_view(h);
  return predictive_samples_impl(fc, loc, aux, n_members, n_rows, n_samples, seed, row0, sample0, nullptr, out);
}

// what the three group reductions check alike: predictive_args, the CSR arrays, the work pointer and n_groups
static int group_args(const Forecast& fc, const float* loc, const float* aux, int64_t n_members, int64_t n_rows,
                      const int32_t* seg_offsets, const int32_t* seg_rows, int64_t n_groups, int64_t n_samples,
                      int64_t row0, int64_t sample0, const void* work) {
  if (const int rc = predictive_args(fc, loc, aux, n_members, n_rows, n_samples, row0, sample0)) return rc;
  if (!seg_offsets || !seg_rows || !work || n_groups < 1 || n_groups > 0x7fffffffLL)
    return fail(BNF_ERR_INVALID, "argument");
  return BNF_OK;
}

// *chunk = the sample paths one pass through the work buffer takes, at per_tile bytes per tile and path
static int group_chunk(int64_t n_rows, int64_t n_samples, size_t per_tile, size_t work_bytes, int64_t* chunk) {
  const size_t per_sample = (size_t)cdiv(n_rows, kPredTile) * per_tile;
  *chunk = (int64_t)std::min<size_t>(std::min<size_t>((size_t)n_samples, work_bytes / per_sample), 65535 * 4);
  if (*chunk < 1)
    return fail(BNF_ERR_INVALID, "work buffer of %zu bytes: one sample path of %lld rows needs %zu", work_bytes,
                (long long)n_rows, per_sample);
  return BNF_OK;
}

static int predictive_group_sums_impl(const Forecast& fc, const float* loc, const float* aux, int64_t n_members, int64_t n_rows,
                                      const int32_t* seg_offsets, const int32_t* seg_rows, int64_t n_groups,
                                      int64_t n_samples, uint64_t seed, int64_t row0, int64_t sample0, const double* cum,
                                      void* work, size_t work_bytes, double* out) {
  if (const int rc = group_args(fc, loc, aux, n_members, n_rows, seg_offsets, seg_rows, n_groups, n_samples, row0, sample0,
                                work)) return rc;
  if (!out) return fail(BNF_ERR_INVALID, "argument");
  int64_t chunk;
  if (const int rc = group_chunk(n_rows, n_samples, 2 * sizeof(double), work_bytes, &chunk)) return rc;
  HIPCHK(hipSetDevice(fc.device));
  HIPCHK(hipMemsetAsync(out, 0, (size_t)n_samples * (size_t)n_groups * sizeof(double), fc.stream));   // empty groups
  group_passes(fc, n_samples, chunk, [&](auto obs, int64_t s0, int64_t n) {
    const dim3 grid = pred_grid(n_rows, kPredTile, n);
    double* partial = (double*)work, *o = out + s0 * n_groups;
    hipLaunchKernelGGL((k_predictive_group_sums<decltype(obs)::value>), grid, dim3(256), 0, fc.stream, loc, aux,
                       (int32_t)n_members, n_rows, seg_offsets, seg_rows, (int32_t)n_groups, n, seed, row0, sample0 + s0,
                       cum, partial, o);
    hipLaunchKernelGGL(k_predictive_group_combine, dim3(grid.x, cdiv(n, 4)), dim3(256), 0, fc.stream, seg_offsets,
                       (int32_t)n_groups, n_rows, n, partial, o);
  });
  HIPCHK(hipGetLastError());
  return BNF_OK;
}

int bnf_predictive_group_sums(bnf_handle* h, const float* loc, const float* aux, int64_t n_members, int64_t n_rows,
                              const int32_t* seg_offsets, const int32_t* seg_rows, int64_t n_groups, int64_t n_samples,
                              uint64_t seed, int64_t row0, int64_t sample0, void* work, size_t work_bytes, double* out) {
  const Forecast fc = forecast_view(h);
  return predictive_group_sums_impl(fc, loc, aux, n_members, n_rows, seg_offsets, seg_rows, n_groups, n_samples, seed, row0,
                                    sample0, nullptr, work, work_bytes, out);
}

// the same paths with member weights: cum_weights DEVICE (n_members,) f64 running sum, NULL = the calls above

int bnf_predictive_samples_weighted(bnf_handle* h, const float* loc, const float* aux, int64_t n_members, int64_t n_rows,
                                    int64_t n_samples, uint64_t seed, int64_t row0, int64_t sample0,
                                    const double* cum_weights, float* out) {
  const Forecast fc = forecast_view(h);
  if (const int rc = no_device()) return rc;
  return predictive_samples_impl(fc, loc, aux, n_members, n_rows, n_samples, seed, row0, sample0, cum_weights, out);
}

int bnf_predictive_group_sums_weighted(bnf_handle* h, const float* loc, const float* aux, int64_t n_members, int64_t n_rows,
                                       const int32_t* seg_offsets, const int32_t* seg_rows, int64_t n_groups,
                                       int64_t n_samples, uint64_t seed, int64_t row0, int64_t sample0,
                                       const double* cum_weights, void* work, size_t work_bytes, double* out) {
  const Forecast fc = forecast_view(h);
  if (const int rc = no_device()) return rc;
  return predictive_group_sums_impl(fc, loc, aux, n_members, n_rows, seg_offsets, seg_rows, n_groups, n_samples, seed, row0,
                                    sample0, cum_weights, work, work_bytes, out);
}

// ---- linear combinations of the rows of the sample paths (bnf_combinations.h) ----
// The position count nnz = form_offsets[n_forms] sizes the grid and the work buffer and lives on the device: it is read
// back (4 bytes) after everything that can be refused without it has been.
int bnf_predictive_combinations(bnf_handle* h, const float* loc, const float* aux, int64_t n_members, int64_t n_rows,
                                const int32_t* form_offsets, const int32_t* form_rows, const double* form_coef,
                                int64_t n_forms, int64_t n_samples, uint64_t seed, int64_t row0, int64_t sample0,
                                const double* cum_weights, void* work, size_t work_bytes, double* out) {
  const Forecast fc = forecast_view(h);
  if (const int rc = predictive_args(fc, loc, aux, n_members, n_rows, n_samples, row0, sample0)) return rc;
  if (!form_offsets || !form_rows || !form_coef || !work || !out || n_forms < 1 || n_forms > 0x7ffffffeLL)
    return fail(BNF_ERR_INVALID, "argument");
  HIPCHK(hipSetDevice(fc.device));
  int32_t nnz32 = -1;
  HIPCHK(hipMemcpyAsync(&nnz32, form_offsets + n_forms, sizeof(nnz32), hipMemcpyDeviceToHost, fc.stream));
  HIPCHK(hipStreamSynchronize(fc.stream));
  const int64_t nnz = nnz32;
  if (nnz < 0) return fail(BNF_ERR_INVALID, "form_offsets[n_forms] = %lld: the position count must be in [0, 2^31)", (long long)nnz);
  int64_t chunk = n_samples;
  if (nnz > 0)
    if (const int rc = group_chunk(nnz, n_samples, 2 * sizeof(double), work_bytes, &chunk)) return rc;
  HIPCHK(hipMemsetAsync(out, 0, (size_t)n_samples * (size_t)n_forms * sizeof(double), fc.stream));   // EMPTY forms
  if (nnz > 0)
    group_passes(fc, n_samples, chunk, [&](auto obs, int64_t s0, int64_t n) {
      const dim3 grid = pred_grid(nnz, kPredTile, n);
      double* partial = (double*)work, *o = out + s0 * n_forms;
      hipLaunchKernelGGL((k_predictive_combinations<decltype(obs)::value>), grid, dim3(256), 0, fc.stream, loc, aux,
                         (int32_t)n_members, n_rows, nnz, form_offsets, form_rows, form_coef, (int32_t)n_forms, n, seed,
                         row0, sample0 + s0, cum_weights, partial, o);
      hipLaunchKernelGGL(k_predictive_group_combine, dim3(grid.x, cdiv(n, 4)), dim3(256), 0, fc.stream, form_offsets,
                         (int32_t)n_forms, nnz, n, partial, o);
    });
  HIPCHK(hipGetLastError());
  return BNF_OK;
}

// ---- group peaks and threshold exceedances of the sample paths (bnf_extremes.h) ----
int bnf_predictive_group_extremes(bnf_handle* h, const float* loc, const float* aux, int64_t n_members, int64_t n_rows,
                                  const int32_t* seg_offsets, const int32_t* seg_rows, int64_t n_groups, int64_t n_samples,
                                  uint64_t seed, int64_t row0, int64_t sample0, const double* cum_weights,
                                  const float* threshold, void* work, size_t work_bytes, double* out_max,
                                  int32_t* out_argmax, double* out_count, uint32_t* peak_count, uint32_t* exceed_count) {
  const Forecast fc = forecast_view(h);
  if (const int rc = group_args(fc, loc, aux, n_members, n_rows, seg_offsets, seg_rows, n_groups, n_samples, row0, sample0,
                                work)) return rc;
  if (!out_max) return fail(BNF_ERR_INVALID, "argument");
  if ((threshold == nullptr) != (out_count == nullptr) || (exceed_count && !threshold))
    return fail(BNF_ERR_INVALID, "out_count goes with threshold, and exceed_count needs one");
  int64_t chunk;
  if (const int rc = group_chunk(n_rows, n_samples, BNF_EXTREMES_WORK_PER_TILE, work_bytes, &chunk)) return rc;
  HIPCHK(hipSetDevice(fc.device));
  // groups without a row: max NaN (all bits set), argmax -1, count 0
  const size_t cells = (size_t)n_samples * (size_t)n_groups;
  HIPCHK(hipMemsetAsync(out_max, 0xff, cells * sizeof(double), fc.stream));
  if (out_argmax) HIPCHK(hipMemsetAsync(out_argmax, 0xff, cells * sizeof(int32_t), fc.stream));
  if (out_count) HIPCHK(hipMemsetAsync(out_count, 0, cells * sizeof(double), fc.stream));
  group_passes(fc, n_samples, chunk, [&](auto obs, int64_t s0, int64_t n) {
    const ExtOut o{seg_rows, out_max + s0 * n_groups, out_argmax ? out_argmax + s0 * n_groups : nullptr,
                   out_count ? out_count + s0 * n_groups : nullptr, peak_count};
    const dim3 grid = pred_grid(n_rows, kPredTile, n);
    hipLaunchKernelGGL((k_predictive_group_extremes<decltype(obs)::value>), grid, dim3(256), 0, fc.stream, loc, aux,
                       (int32_t)n_members, n_rows, seg_offsets, seg_rows, (int32_t)n_groups, n, seed, row0, sample0 + s0,
                       cum_weights, threshold, (ExtPiece*)work, o, exceed_count);
    hipLaunchKernelGGL(k_predictive_group_extremes_combine, dim3(grid.x, cdiv(n, 4)), dim3(256), 0, fc.stream, seg_offsets,
                       (int32_t)n_groups, n_rows, n, (ExtPiece*)work, o);
  });
  HIPCHK(hipGetLastError());
  return BNF_OK;
}

// ---- spells above a threshold in the sample paths (bnf_episodes.h) ----
int bnf_predictive_group_episodes(bnf_handle* h, const float* loc, const float* aux, int64_t n_members, int64_t n_rows,
                                  const int32_t* seg_offsets, const int32_t* seg_rows, int64_t n_groups, int64_t n_samples,
                                  uint64_t seed, int64_t row0, int64_t sample0, const double* cum_weights,
                                  const float* threshold, void* work, size_t work_bytes, double* out_longest,
                                  int32_t* out_longest_row, double* out_spells, double* out_onset_step,
                                  int32_t* out_first_row, int32_t* out_last_row, uint32_t* onset_count) {
  const Forecast fc = forecast_view(h);
  if (const int rc = group_args(fc, loc, aux, n_members, n_rows, seg_offsets, seg_rows, n_groups, n_samples, row0, sample0,
                                work)) return rc;
  if (!threshold || !out_longest) return fail(BNF_ERR_INVALID, "threshold and out_longest are required");
  int64_t chunk;
  if (const int rc = group_chunk(n_rows, n_samples, BNF_EPISODES_WORK_PER_TILE, work_bytes, &chunk)) return rc;
  HIPCHK(hipSetDevice(fc.device));
  // groups without a row: 0 / -1 / 0 / 0 / -1 / -1
  const size_t cells = (size_t)n_samples * (size_t)n_groups;
  HIPCHK(hipMemsetAsync(out_longest, 0, cells * sizeof(double), fc.stream));
  if (out_longest_row) HIPCHK(hipMemsetAsync(out_longest_row, 0xff, cells * sizeof(int32_t), fc.stream));
  if (out_spells) HIPCHK(hipMemsetAsync(out_spells, 0, cells * sizeof(double), fc.stream));
  if (out_onset_step) HIPCHK(hipMemsetAsync(out_onset_step, 0, cells * sizeof(double), fc.stream));
  if (out_first_row) HIPCHK(hipMemsetAsync(out_first_row, 0xff, cells * sizeof(int32_t), fc.stream));
  if (out_last_row) HIPCHK(hipMemsetAsync(out_last_row, 0xff, cells * sizeof(int32_t), fc.stream));
  group_passes(fc, n_samples, chunk, [&](auto obs, int64_t s0, int64_t n) {
    const int64_t at = s0 * n_groups;
    const EpOut o{seg_rows, out_longest + at, out_longest_row ? out_longest_row + at : nullptr,
                  out_spells ? out_spells + at : nullptr, out_onset_step ? out_onset_step + at : nullptr,
                  out_first_row ? out_first_row + at : nullptr, out_last_row ? out_last_row + at : nullptr, onset_count};
    const dim3 grid = pred_grid(n_rows, kPredTile, n);
    hipLaunchKernelGGL((k_predictive_group_episodes<decltype(obs)::value>), grid, dim3(256), 0, fc.stream, loc, aux,
                       (int32_t)n_members, n_rows, seg_offsets, seg_rows, (int32_t)n_groups, n, seed, row0, sample0 + s0,
                       cum_weights, threshold, (EpPiece*)work, o);
    hipLaunchKernelGGL(k_predictive_group_episodes_combine, dim3(grid.x, cdiv(n, 4)), dim3(256), 0, fc.stream, seg_offsets,
                       (int32_t)n_groups, n_rows, n, (EpPiece*)work, o);
  });
  HIPCHK(hipGetLastError());
  return BNF_OK;
}

// ---- running totals of the sample paths and when they pass a level (bnf_cumulative.h) ----
// The launch shape of k_predictive_group_cumulative.  Only the block of a tile in which a group STARTS has work, and at
// most min(tiles, groups) tiles have one; a table that is one long group has a single working tile and is parallel over
// the samples alone.  So grid.y is pred_grid's 16384 / gx, raised until min(tiles, groups) x grid.y reaches
// kCumMinBlocks = 2048 blocks (256 CUs x 8), never above the samples.  A block that owns nothing costs one bisection.
constexpr int64_t kCumMinBlocks = 2048;
static dim3 cum_grid(int64_t R, int64_t G, int64_t S) {
  const int64_t gx = cdiv(R, kPredTile);
  const int64_t want = std::max<int64_t>(std::max<int64_t>(1, 16384 / gx), cdiv(kCumMinBlocks, std::min(gx, G)));
  return dim3((unsigned)gx, (unsigned)std::min<int64_t>(std::min<int64_t>(S, 65535), want));
}

int bnf_predictive_group_cumulative(bnf_handle* h, const float* loc, const float* aux, int64_t n_members, int64_t n_rows,
                                    const int32_t* seg_offsets, const int32_t* seg_rows, int64_t n_groups,
                                    int64_t n_samples, uint64_t seed, int64_t row0, int64_t sample0,
                                    const double* cum_weights, const double* level, double* out_total,
                                    double* out_running, double* out_cross_step, int32_t* out_cross_row,
                                    uint32_t* cross_count, uint32_t* above_count) {
  const Forecast fc = forecast_view(h);
  if (const int rc = predictive_args(fc, loc, aux, n_members, n_rows, n_samples, row0, sample0)) return rc;
  if (!seg_offsets || !seg_rows || n_groups < 1 || n_groups > 0x7fffffffLL) return fail(BNF_ERR_INVALID, "argument");
  if (!out_total) return fail(BNF_ERR_INVALID, "out_total is required");
  if (!level && (out_cross_step || out_cross_row || cross_count || above_count))
    return fail(BNF_ERR_INVALID, "out_cross_step, out_cross_row, cross_count and above_count need a level");
  HIPCHK(hipSetDevice(fc.device));
  // groups without a row: total 0, cross_step 0 (censored at 0 steps), cross_row -1
  const size_t cells = (size_t)n_samples * (size_t)n_groups;
  HIPCHK(hipMemsetAsync(out_total, 0, cells * sizeof(double), fc.stream));
  if (out_cross_step) HIPCHK(hipMemsetAsync(out_cross_step, 0, cells * sizeof(double), fc.stream));
  if (out_cross_row) HIPCHK(hipMemsetAsync(out_cross_row, 0xff, cells * sizeof(int32_t), fc.stream));
  const CumOut o{level, out_total, out_running, out_cross_step, out_cross_row, cross_count, above_count};
  with_obs(fc, [&](auto obs) {
    hipLaunchKernelGGL((k_predictive_group_cumulative<decltype(obs)::value>), cum_grid(n_rows, n_groups, n_samples),
                       dim3(256), 0, fc.stream, loc, aux, (int32_t)n_members, n_rows, seg_offsets, seg_rows,
                       (int32_t)n_groups, n_samples, seed, row0, sample0, cum_weights, o);
  });
  HIPCHK(hipGetLastError());
  return BNF_OK;
}

// ---- moving-window totals of the sample paths (bnf_windows.h) ----
// The launch shape is cum_grid's: only the block of a tile in which a group starts has work.
int bnf_predictive_group_windows(bnf_handle* h, const float* loc, const float* aux, int64_t n_members, int64_t n_rows,
                                 const int32_t* seg_offsets, const int32_t* seg_rows, int64_t n_groups, int64_t n_samples,
                                 uint64_t seed, int64_t row0, int64_t sample0, const double* cum_weights, int32_t window,
                                 const double* threshold, double* out_peak, int32_t* out_peak_row, double* out_window,
                                 double* out_count, uint32_t* peak_count, uint32_t* exceed_count) {
  const Forecast fc = forecast_view(h);
  if (const int rc = predictive_args(fc, loc, aux, n_members, n_rows, n_samples, row0, sample0)) return rc;
  if (!seg_offsets || !seg_rows || n_groups < 1 || n_groups > 0x7fffffffLL) return fail(BNF_ERR_INVALID, "argument");
  if (!out_peak) return fail(BNF_ERR_INVALID, "out_peak is required");
  if (window < 1) return fail(BNF_ERR_INVALID, "window must be >= 1 position; got %d", (int)window);
  if (!threshold && (out_count || exceed_count))
    return fail(BNF_ERR_INVALID, "out_count and exceed_count need a threshold");
  HIPCHK(hipSetDevice(fc.device));
  // groups without a candidate window: peak NaN (all bits set), peak_row -1, count 0
  const size_t cells = (size_t)n_samples * (size_t)n_groups;
  HIPCHK(hipMemsetAsync(out_peak, 0xff, cells * sizeof(double), fc.stream));
  if (out_peak_row) HIPCHK(hipMemsetAsync(out_peak_row, 0xff, cells * sizeof(int32_t), fc.stream));
  if (out_count) HIPCHK(hipMemsetAsync(out_count, 0, cells * sizeof(double), fc.stream));
  const WinOut o{threshold, out_peak, out_peak_row, out_window, out_count, peak_count, exceed_count};
  with_obs(fc, [&](auto obs) {
    hipLaunchKernelGGL((k_predictive_group_windows<decltype(obs)::value>), cum_grid(n_rows, n_groups, n_samples),
                       dim3(256), 0, fc.stream, loc, aux, (int32_t)n_members, n_rows, seg_offsets, seg_rows,
                       (int32_t)n_groups, n_samples, seed, row0, sample0, cum_weights, window, o);
  });
  HIPCHK(hipGetLastError());
  return BNF_OK;
}

// ---- held-out scoring (bnf_scoring.h) ---------------------------------------------
static int predictive_scores_impl(const Forecast& fc, const float* loc, const float* aux, const double* wts, int64_t n_members,
                                  int64_t n_rows, const float* y, void* work, size_t work_bytes, double* member_ll,
                                  float* lpd, float* pit, float* crps) {
  if (!fc.bound) return fail(BNF_ERR_STATE, "not bound");
  if (!loc || !aux || !y || n_members < 1 || n_members > 0x7fffffffLL || n_rows < 1 || n_rows > 0x7fffffffLL)
    return fail(BNF_ERR_INVALID, "argument");
  if (crps && fc.obs_model != BNF_OBS_NORMAL)
    return fail(BNF_ERR_INVALID, "crps: closed form for the NORMAL observation model only");
  const int64_t nt = cdiv(n_rows, kScoreTile);
  const int64_t n_chunks = cdiv(n_members, kScoreChunk);
  const int64_t n_slots = std::min<int64_t>((n_chunks + 1) / 2, kScoreMaxSlots);
  const size_t ll_bytes = member_ll ? (size_t)n_members * (size_t)nt * sizeof(double) : 0;
  const size_t pair_bytes = crps ? (size_t)n_rows * (size_t)n_slots * sizeof(double) : 0;
  if (ll_bytes + pair_bytes > 0 && (!work || work_bytes < ll_bytes + pair_bytes))
    return fail(BNF_ERR_INVALID, "work buffer of %zu bytes: %lld members x %lld rows need %zu", work ? work_bytes : (size_t)0,
                (long long)n_members, (long long)n_rows, ll_bytes + pair_bytes);
  if (!member_ll && !lpd && !pit && !crps) return BNF_OK;
  HIPCHK(hipSetDevice(fc.device));
  double* ll_partial = (double*)work;
  double* pair_partial = (double*)((char*)work + ll_bytes);
  with_obs(fc, [&](auto obs) {
    constexpr int OBS = decltype(obs)::value;
    if (wts)
      launch_predictive_scores<OBS, true>(fc, loc, aux, wts, n_members, n_rows, y, ll_partial, pair_partial, n_slots,
                                          member_ll, lpd, pit, crps);
    else
      launch_predictive_scores<OBS, false>(fc, loc, aux, wts, n_members, n_rows, y, ll_partial, pair_partial, n_slots,
                                           member_ll, lpd, pit, crps);
  });
  HIPCHK(hipGetLastError());
  return BNF_OK;
}

int bnf_predictive_scores(bnf_handle* h, const float* loc, const float* aux, int64_t n_members, int64_t n_rows,
                          const float* y, void* work, size_t work_bytes, double* member_ll, float* lpd, float* pit,
                          float* crps) {
  const Forecast fc = forecast_view(h);
  return predictive_scores_impl(fc, loc, aux, nullptr, n_members, n_rows, y, work, work_bytes, member_ll, lpd, pit, crps);
}

// ---- stacking of the members on held-out rows (bnf_stacking.h) ----------------------
int bnf_member_log_density(bnf_handle* h, const float* loc, const float* aux, int64_t n_members, int64_t n_rows,
                           const float* y, float* out) {
  const Forecast fc = forecast_view(h);
  if (const int rc = no_device()) return rc;
  if (!fc.bound) return fail(BNF_ERR_STATE, "not bound");
  if (!loc || !aux || !y || !out || n_members < 1 || n_members > 0x7fffffffLL || n_rows < 1 || n_rows > 0x7fffffffLL)
    return fail(BNF_ERR_INVALID, "argument");
  HIPCHK(hipSetDevice(fc.device));
  const dim3 grid(cdiv(n_rows, kStackTile), (unsigned)std::min<int64_t>(n_members, 65535));
  with_obs(fc, [&](auto obs) {
    hipLaunchKernelGGL((k_member_log_density<decltype(obs)::value>), grid, dim3(256), 0, fc.stream, loc, aux,
                       (int32_t)n_members, n_rows, y, out);
  });
  HIPCHK(hipGetLastError());
  return BNF_OK;
}

int bnf_stacking_weights(bnf_handle* h, const float* logdens, int64_t n_members, int64_t n_rows, const double* w_init,
                         int64_t max_iter, double tol, void* work, size_t work_bytes, double* weights, float* lpd,
                         double* info) {
  const Forecast fc = forecast_view(h);
  if (const int rc = no_device()) return rc;
  if (!fc.bound) return fail(BNF_ERR_STATE, "not bound");
  if (!logdens || !weights || !info || n_members < 1 || n_members > 0x7fffffffLL || n_rows < 1 || n_rows > 0x7fffffffLL)
    return fail(BNF_ERR_INVALID, "argument");
  if (max_iter < 0 || !(tol >= 0.0)) return fail(BNF_ERR_INVALID, "max_iter = %lld, tol = %g: both must be >= 0",
                                                  (long long)max_iter, tol);
  const int64_t nt = cdiv(n_rows, kStackTile);
  const size_t need = sizeof(double) * ((size_t)kStackState + (size_t)(n_members + 3) * (size_t)nt);
  if (!work || work_bytes < need)
    return fail(BNF_ERR_INVALID, "work buffer of %zu bytes: %lld members x %lld rows need %zu", work ? work_bytes : (size_t)0,
                (long long)n_members, (long long)n_rows, need);
  HIPCHK(hipSetDevice(fc.device));
  double* state = (double*)work;
  double* tile_stat = state + kStackState;
  double* partial = tile_stat + 3 * nt;
  const int32_t M = (int32_t)n_members;
  hipLaunchKernelGGL(k_stack_init, dim3(1), dim3(256), 0, fc.stream, w_init, M, weights, state);
  // max_iter updates need max_iter + 1 evaluations: the last one is of the weights that are returned
  bool done = false;
  for (int64_t left = max_iter + 1; left > 0 && !done;) {
    const int64_t batch = std::min<int64_t>(left, BNF_STACK_BATCH);
    for (int64_t i = 0; i < batch; ++i) {
      hipLaunchKernelGGL((k_stack_rows<false>), dim3((unsigned)nt), dim3(256), 0, fc.stream, logdens, M, n_rows,
                         (const double*)weights, (const double*)state, partial, tile_stat, (float*)nullptr);
      hipLaunchKernelGGL(k_stack_combine, dim3(1), dim3(256), 0, fc.stream, (const double*)partial,
                         (const double*)tile_stat, M, nt, max_iter, tol, weights, state, info);
    }
    left -= batch;
    HIPCHK(hipGetLastError());
    double flag = 0.0;
    HIPCHK(hipMemcpyAsync(&flag, state + STACK_DONE, sizeof(double), hipMemcpyDeviceToHost, fc.stream));
    HIPCHK(hipStreamSynchronize(fc.stream));
    done = flag != 0.0;
  }
  if (!done) return fail(BNF_ERR_STATE, "stacking: the iteration budget ran out without the stop being recorded");
  if (lpd)
    hipLaunchKernelGGL((k_stack_rows<true>), dim3((unsigned)nt), dim3(256), 0, fc.stream, logdens, M, n_rows,
                       (const double*)weights, (const double*)state, (double*)nullptr, (double*)nullptr, lpd);
  HIPCHK(hipGetLastError());
  return BNF_OK;
}

// ---- ranked probability score of count forecasts (bnf_rps.h) -----------------------
static int count_rps_impl(const Forecast& fc, const float* loc, const float* aux, const double* wts, int64_t n_members,
                          int64_t n_rows, const float* y, float* rps) {
  if (!fc.bound) return fail(BNF_ERR_STATE, "not bound");
  if (!loc || !aux || !y || !rps || n_members < 1 || n_rows < 1 || n_rows > 0x7fffffffLL)
    return fail(BNF_ERR_INVALID, "argument");
  if (n_members > BNF_RPS_MAX_MEMBERS)
    return fail(BNF_ERR_INVALID, "%lld members: the ranked probability score takes at most %d", (long long)n_members,
                BNF_RPS_MAX_MEMBERS);
  if (fc.obs_model == BNF_OBS_NORMAL)
    return fail(BNF_ERR_INVALID, "rps: count observation models only (NORMAL: the crps of bnf_predictive_scores)");
  HIPCHK(hipSetDevice(fc.device));
  const bool nb = fc.obs_model == BNF_OBS_NB;
  if (wts && nb) launch_count_rps<BNF_OBS_NB, true>(fc, loc, aux, wts, n_members, n_rows, y, rps);
  else if (wts) launch_count_rps<BNF_OBS_ZINB, true>(fc, loc, aux, wts, n_members, n_rows, y, rps);
  else if (nb) launch_count_rps<BNF_OBS_NB, false>(fc, loc, aux, wts, n_members, n_rows, y, rps);
  else launch_count_rps<BNF_OBS_ZINB, false>(fc, loc, aux, wts, n_members, n_rows, y, rps);
  HIPCHK(hipGetLastError());
  return BNF_OK;
}

int bnf_count_rps(bnf_handle* h, const float* loc, const float* aux, int64_t n_members, int64_t n_rows, const float* y,
                  float* rps) {
  const Forecast fc = forecast_view(h);
  return count_rps_impl(fc, loc, aux, nullptr, n_members, n_rows, y, rps);
}

// ---- the marginal forecast of the WEIGHTED mixture: quantiles, scores and the RPS with member weights ------------------
// weights DEVICE (n_members,) f64 as bnf_stacking_weights writes them; NULL is BNF_ERR_INVALID (the unweighted calls have
// their own names).  Not validated: reading them would cost a sync.
int bnf_normal_mixture_quantiles_weighted(bnf_handle* h, const float* means, const float* scales, const double* weights,
                                          int64_t n_members, int64_t n_rows, const float* q, int32_t n_q,
                                          int32_t approximate, float* out) {
  const Forecast fc = forecast_view(h);
  if (const int rc = no_device()) return rc;
  if (!weights) return fail(BNF_ERR_INVALID, "weights");
  return normal_mixture_quantiles_impl(fc, means, scales, weights, n_members, n_rows, q, n_q, approximate, out);
}

int bnf_count_mixture_quantiles_weighted(bnf_handle* h, const float* loc, const float* aux, const double* weights,
                                         int64_t n_members, int64_t n_rows, const float* q, int32_t n_q, float* means,
                                         float* out) {
  const Forecast fc = forecast_view(h);
  if (const int rc = no_device()) return rc;
  if (!weights) return fail(BNF_ERR_INVALID, "weights");
  return count_mixture_quantiles_impl(fc, loc, aux, weights, n_members, n_rows, q, n_q, means, out);
}

int bnf_predictive_scores_weighted(bnf_handle* h, const float* loc, const float* aux, const double* weights,
                                   int64_t n_members, int64_t n_rows, const float* y, void* work, size_t work_bytes,
                                   float* lpd, float* pit, float* crps) {
  const Forecast fc = forecast_view(h);
  if (const int rc = no_device()) return rc;
  if (!weights) return fail(BNF_ERR_INVALID, "weights");
  return predictive_scores_impl(fc, loc, aux, weights, n_members, n_rows, y, work, work_bytes, nullptr, lpd, pit, crps);
}

int bnf_count_rps_weighted(bnf_handle* h, const float* loc, const float* aux, const double* weights, int64_t n_members,
                           int64_t n_rows, const float* y, float* rps) {
  const Forecast fc = forecast_view(h);
  if (const int rc = no_device()) return rc;
  if (!weights) return fail(BNF_ERR_INVALID, "weights");
  return count_rps_impl(fc, loc, aux, weights, n_members, n_rows, y, rps);
}

// ---- summaries and scores of sample paths (bnf_totals.h) -----------------------------
static int totals_args(const Forecast& fc, const double* x, int64_t n_samples, int64_t n_cols) {
  if (const int rc = no_device()) return rc;
  if (!fc.bound) return fail(BNF_ERR_STATE, "not bound");
  if (!x || n_samples < 1 || n_cols < 1 || n_cols > 0x7fffffffLL) return fail(BNF_ERR_INVALID, "argument");
  if (n_samples > BNF_SUMMARY_MAX_SAMPLES)
    return fail(BNF_ERR_INVALID, "%lld sample paths: a column is sorted in LDS, at most %d", (long long)n_samples,
                BNF_SUMMARY_MAX_SAMPLES);
  return BNF_OK;
}

int bnf_sample_summaries(bnf_handle* h, const double* x, int64_t n_samples, int64_t n_cols, const double* y,
                         const double* q, int32_t n_q, double* mean, double* quant, double* crps, double* pit) {
  const Forecast fc = forecast_view(h);
  if (const int rc = totals_args(fc, x, n_samples, n_cols)) return rc;
  if (n_q < 0 || n_q > BNF_SUMMARY_MAX_QUANTILES || (n_q > 0 && (!q || !quant)))
    return fail(BNF_ERR_INVALID, "n_q = %d: 0..%d quantile levels, with q and quant", n_q, BNF_SUMMARY_MAX_QUANTILES);
  if (!y && (crps || pit)) return fail(BNF_ERR_INVALID, "crps and pit need the observations y");
  SummaryQ sq;
  sq.n = n_q;
  for (int32_t j = 0; j < kSumMaxQ; ++j) { sq.lo[j] = 0; sq.frac[j] = 0.0; }
  for (int32_t j = 0; j < n_q; ++j) {
    if (!(q[j] >= 0.0 && q[j] <= 1.0)) return fail(BNF_ERR_INVALID, "quantile level %g outside [0, 1]", q[j]);
    const double hq = (double)(n_samples - 1) * q[j];
    double lo = std::floor(hq);
    double frac = hq - lo;
    if (lo >= (double)(n_samples - 1)) { lo = (double)(n_samples - 1); frac = 0.0; }
    sq.lo[j] = (int32_t)lo;
    sq.frac[j] = frac;
  }
  if (!mean && !crps && !pit && n_q == 0) return BNF_OK;
  HIPCHK(hipSetDevice(fc.device));
  launch_sample_summaries(fc, x, n_samples, n_cols, y, sq, mean, quant, crps, pit);
  HIPCHK(hipGetLastError());
  return BNF_OK;
}

int bnf_sample_energy_score(bnf_handle* h, const double* x, int64_t n_samples, int64_t n_cols, const double* y,
                            void* work, size_t work_bytes, double* out) {
  const Forecast fc = forecast_view(h);
  if (const int rc = totals_args(fc, x, n_samples, n_cols)) return rc;
  if (!y || !out) return fail(BNF_ERR_INVALID, "argument");
  const size_t need = sizeof(double) * (size_t)energy_work_doubles(n_samples);
  if (!work || work_bytes < need)
    return fail(BNF_ERR_INVALID, "work buffer of %zu bytes: %lld sample paths need %zu", work ? work_bytes : (size_t)0,
                (long long)n_samples, need);
  HIPCHK(hipSetDevice(fc.device));
  const int64_t nT = energy_tiles(n_samples);
  hipLaunchKernelGGL(k_energy_first, dim3((unsigned)n_samples), dim3(256), 0, fc.stream, x, n_cols, y, (double*)work);
  hipLaunchKernelGGL(k_energy_pairs, dim3((unsigned)nT, (unsigned)nT), dim3(256), 0, fc.stream, x, n_samples, n_cols, y,
                     (double*)work);
  hipLaunchKernelGGL(k_energy_finish, dim3(1), dim3(256), 0, fc.stream, (const double*)work, n_samples,
                     nT * (nT + 1) / 2, y, n_cols, out);
  HIPCHK(hipGetLastError());
  return BNF_OK;
}

// ---- covariance, variogram and variogram score of sample paths (bnf_dependence.h) ------
int bnf_sample_pair_moments(bnf_handle* h, const double* x, int64_t n_samples, int64_t n_cols, double p, const double* y,
                            const double* pair_w, double* mean, double* cov, double* vario, void* work, size_t work_bytes,
                            double* score) {
  const Forecast fc = forecast_view(h);
  if (const int rc = no_device()) return rc;
  if (!fc.bound) return fail(BNF_ERR_STATE, "not bound");
  if (!x || n_samples < 1 || n_cols < 1 || n_cols > 0x7fffffffLL) return fail(BNF_ERR_INVALID, "argument");
  const int form = p == 0.5 ? 0 : p == 1.0 ? 1 : p == 2.0 ? 2 : -1;
  if (form < 0) return fail(BNF_ERR_INVALID, "p = %g: the variogram is compiled for p = 0.5, 1 and 2", p);
  if ((cov || vario || pair_w) && n_cols > BNF_PAIR_MATRIX_MAX_COLS)
    return fail(BNF_ERR_INVALID, "%lld columns: a pair matrix has at most %d a side", (long long)n_cols,
                BNF_PAIR_MATRIX_MAX_COLS);
  const int64_t nT = pair_tiles(n_cols);
  if (nT > 65535) return fail(BNF_ERR_INVALID, "%lld columns: at most %d pair tiles a side", (long long)n_cols, 65535);
  if (cov && !mean) return fail(BNF_ERR_INVALID, "cov needs mean: the centred products read it");
  if (score) {
    if (!y) return fail(BNF_ERR_INVALID, "score needs the observations y");
    const size_t need = sizeof(double) * (size_t)pair_work_doubles(n_cols);
    if (!work || work_bytes < need)
      return fail(BNF_ERR_INVALID, "work buffer of %zu bytes: %lld columns need %zu", work ? work_bytes : (size_t)0,
                  (long long)n_cols, need);
  }
  if (!mean && !cov && !vario && !score) return BNF_OK;
  HIPCHK(hipSetDevice(fc.device));
  if (mean)
    hipLaunchKernelGGL(k_column_means, dim3((unsigned)((n_cols + kDpMeanCols - 1) / kDpMeanCols)),
                       dim3(kDpMeanCols * kDpMeanLanes), 0, fc.stream, x, n_samples, n_cols, mean);
  if (cov || vario || score) {
    double* partials = score ? (double*)work : nullptr;
    const double* yy = score ? y : nullptr;
    const double* ww = score ? pair_w : nullptr;
    if (!vario && !score)                              // the covariance alone: p plays no part
      launch_pair_moments<2>(fc.stream, x, n_samples, n_cols, mean, yy, ww, cov, vario, partials);
    else if (form == 0)
      launch_pair_moments<0>(fc.stream, x, n_samples, n_cols, mean, yy, ww, cov, vario, partials);
    else if (form == 1)
      launch_pair_moments<1>(fc.stream, x, n_samples, n_cols, mean, yy, ww, cov, vario, partials);
    else
      launch_pair_moments<2>(fc.stream, x, n_samples, n_cols, mean, yy, ww, cov, vario, partials);
    if (score)
      hipLaunchKernelGGL(k_vario_finish, dim3(1), dim3(256), 0, fc.stream, (const double*)work, nT * (nT + 1) / 2, y,
                         n_cols, score);
  }
  HIPCHK(hipGetLastError());
  return BNF_OK;
}

// ---- representative scenarios: pairwise distances of the paths, forward selection (bnf_scenarios.h) ------
static int scenario_sizes(const Forecast& fc, int64_t n_samples) {
  if (!fc.bound) return fail(BNF_ERR_STATE, "not bound");
  if (n_samples < 1) return fail(BNF_ERR_INVALID, "argument");
  if (n_samples > BNF_SCENARIO_MAX_SAMPLES)
    return fail(BNF_ERR_INVALID, "%lld sample paths: the distance matrix has at most %d a side", (long long)n_samples,
                BNF_SCENARIO_MAX_SAMPLES);
  return BNF_OK;
}

int bnf_sample_distances(bnf_handle* h, const double* x, int64_t n_samples, int64_t n_cols, const double* scale,
                         const double* y, int32_t p, double* dist, double* ydist) {
  const Forecast fc = forecast_view(h);
  if (const int rc = no_device()) return rc;
  if (const int rc = scenario_sizes(fc, n_samples)) return rc;
  if (!x || !dist || n_cols < 1 || n_cols > 0x7fffffffLL) return fail(BNF_ERR_INVALID, "argument");
  if (p != 1 && p != 2) return fail(BNF_ERR_INVALID, "p = %d: the distance is the 1-norm (p = 1) or the 2-norm (p = 2)", p);
  if ((y == nullptr) != (ydist == nullptr))
    return fail(BNF_ERR_INVALID, "y and ydist go together: both, or both NULL");
  HIPCHK(hipSetDevice(fc.device));
  if (p == 1 && scale) launch_scn_distances<1, true>(fc.stream, x, n_samples, n_cols, scale, y, dist, ydist);
  else if (p == 1) launch_scn_distances<1, false>(fc.stream, x, n_samples, n_cols, scale, y, dist, ydist);
  else if (scale) launch_scn_distances<2, true>(fc.stream, x, n_samples, n_cols, scale, y, dist, ydist);
  else launch_scn_distances<2, false>(fc.stream, x, n_samples, n_cols, scale, y, dist, ydist);
  HIPCHK(hipGetLastError());
  return BNF_OK;
}

int bnf_scenario_select(bnf_handle* h, const double* dist, int64_t n_samples, int32_t k, const double* ydist, void* work,
                        size_t work_bytes, int32_t* chosen, double* objective, double* prob, int32_t* assign,
                        double* nearest, int32_t* obs_nearest, double* obs) {
  const Forecast fc = forecast_view(h);
  if (const int rc = no_device()) return rc;
  if (const int rc = scenario_sizes(fc, n_samples)) return rc;
  if (k < 1 || k > n_samples)
    return fail(BNF_ERR_INVALID, "k = %d: 1..%lld, the number of sample paths", k, (long long)n_samples);
  if (!dist || !chosen || !objective || !prob) return fail(BNF_ERR_INVALID, "argument");
  if (ydist && (!obs_nearest || !obs)) return fail(BNF_ERR_INVALID, "ydist needs obs_nearest and obs");
  const size_t need = scenario_work_bytes(n_samples);
  if (!work || work_bytes < need || ((uintptr_t)work & 7u))
    return fail(BNF_ERR_INVALID, "work buffer of %zu bytes: %lld sample paths need %zu, 8-byte aligned",
                work ? work_bytes : (size_t)0, (long long)n_samples, need);
  HIPCHK(hipSetDevice(fc.device));
  const ScnWork w = scenario_work(work, n_samples);
  const int64_t S = n_samples;
  HIPCHK(hipMemsetAsync(w.flag, 0, 2 * sizeof(int32_t), fc.stream));
  hipLaunchKernelGGL(k_scn_init, dim3(std::min<unsigned>(1024u, cdiv(S * S, 256 * 4))), dim3(256), 0, fc.stream, dist, S, w);
  for (int32_t i = 0; i < k; ++i) {
    hipLaunchKernelGGL(k_scn_sums, dim3((unsigned)S), dim3(kScnThreads), 0, fc.stream, dist, S, w);
    hipLaunchKernelGGL(k_scn_pick, dim3(1), dim3(kScnThreads), 0, fc.stream, dist, S, i, w, chosen, objective);
  }
  hipLaunchKernelGGL(k_scn_assign, dim3(cdiv(S, 256)), dim3(256), 0, fc.stream, dist, S, k, w, (const int32_t*)chosen,
                     assign, nearest);
  hipLaunchKernelGGL(k_scn_finish, dim3((unsigned)k + 1u), dim3(kScnThreads), 0, fc.stream, S, k, w,
                     (const int32_t*)chosen, ydist, prob, obs_nearest, obs);
  HIPCHK(hipGetLastError());
  return BNF_OK;
}

// ---- ranks of the columns within a sample path, rank probabilities (bnf_ranking.h) ------
int bnf_sample_ranks(bnf_handle* h, const double* x, int64_t n_samples, int64_t n_cols, const double* scale,
                     double* out_rank, int32_t* out_above, int32_t* out_ties) {
  const Forecast fc = forecast_view(h);
  if (const int rc = no_device()) return rc;
  if (!fc.bound) return fail(BNF_ERR_STATE, "not bound");
  if (!x || n_samples < 1 || n_cols < 1) return fail(BNF_ERR_INVALID, "argument");
  if (n_cols > BNF_RANK_MAX_COLS)
    return fail(BNF_ERR_INVALID, "%lld columns: a path's values are sorted in LDS, at most %d", (long long)n_cols,
                BNF_RANK_MAX_COLS);
  if (!out_rank && !out_above && !out_ties) return fail(BNF_ERR_INVALID, "no output: rank, above and ties are all NULL");
  HIPCHK(hipSetDevice(fc.device));
  int P = 1;
  while (P < n_cols) P <<= 1;
  const int threads = std::min(1024, std::max(64, P / 2));          // a multiple of 64: P is a power of two
  static std::atomic<uint64_t> attr_done{0};
  allow_lds(fc.device, &k_sample_ranks, (int)(sizeof(uint64_t) * kRankMaxCols), &attr_done);
  hipLaunchKernelGGL(k_sample_ranks, dim3((unsigned)std::min<int64_t>(n_samples, 1 << 16)), dim3(threads),
                     sizeof(uint64_t) * (size_t)P, fc.stream, x, n_samples, (int32_t)n_cols, (int32_t)P, scale, out_rank,
                     out_above, out_ties);
  HIPCHK(hipGetLastError());
  return BNF_OK;
}

int bnf_rank_probabilities(bnf_handle* h, const int32_t* above, const int32_t* ties, int64_t n_samples, int64_t n_cols,
                           int32_t top_k, double* out) {
  const Forecast fc = forecast_view(h);
  if (const int rc = no_device()) return rc;
  if (!fc.bound) return fail(BNF_ERR_STATE, "not bound");
  if (!above || !ties || !out || n_samples < 1 || n_cols < 1 || n_cols > 0x7fffffffLL)
    return fail(BNF_ERR_INVALID, "argument");
  if (top_k < 1 || top_k > n_cols)
    return fail(BNF_ERR_INVALID, "top_k = %d: 1..%lld, the number of columns", top_k, (long long)n_cols);
  if ((int64_t)top_k * n_cols > BNF_RANK_MAX_CELLS)
    return fail(BNF_ERR_INVALID, "top_k = %d x %lld columns: at most %d cells", top_k, (long long)n_cols,
                BNF_RANK_MAX_CELLS);
  HIPCHK(hipSetDevice(fc.device));
  hipLaunchKernelGGL(k_rank_probabilities, dim3(cdiv(n_cols, kRankSlab), cdiv(top_k, kRankKPerBlock)), dim3(256), 0,
                     fc.stream, above, ties, n_samples, n_cols, top_k, out);
  HIPCHK(hipGetLastError());
  return BNF_OK;
}

// ---- simultaneous bands of sample paths: depths, levels, envelopes (bnf_bands.h) --------
struct BandSlab { int P, W, threads; };
static BandSlab band_slab(int64_t S) {
  BandSlab b;
  b.P = 1;
  while (b.P < S) b.P <<= 1;
  b.W = std::min(kSumMaxCols, kSumMaxSamples / b.P);
  b.threads = std::min(1024, std::max(64, b.W * b.P / 2));          // a multiple of 64: W * P is a power of two
  return b;
}

static int bands_args(const Forecast& fc, const double* x, int64_t n_samples, int64_t n_cols, const int32_t* col_group,
                      int64_t n_groups) {
  if (const int rc = totals_args(fc, x, n_samples, n_cols)) return rc;
  if (!col_group || n_groups < 1 || n_groups > 0x7fffffffLL) return fail(BNF_ERR_INVALID, "argument");
  return BNF_OK;
}

int bnf_sample_depths(bnf_handle* h, const double* x, int64_t n_samples, int64_t n_cols, const int32_t* col_group,
                      int64_t n_groups, const double* y, int32_t* depth, int32_t* obs_depth) {
  const Forecast fc = forecast_view(h);
  if (const int rc = bands_args(fc, x, n_samples, n_cols, col_group, n_groups)) return rc;
  if (!depth) return fail(BNF_ERR_INVALID, "depth is NULL");
  if ((y == nullptr) != (obs_depth == nullptr)) return fail(BNF_ERR_INVALID, "y and obs_depth are given together or not at all");
  HIPCHK(hipSetDevice(fc.device));
  const BandSlab b = band_slab(n_samples);
  static std::atomic<uint64_t> attr_done{0};
  allow_lds(fc.device, &k_sample_depths, (int)(sizeof(uint64_t) * kSumMaxSamples), &attr_done);
  hipLaunchKernelGGL(k_sample_depths, dim3(cdiv(n_cols, b.W)), dim3(b.threads), sizeof(uint64_t) * (size_t)b.W * (size_t)b.P,
                     fc.stream, x, (int32_t)n_samples, n_cols, (int32_t)b.P, (int32_t)b.W, col_group, (int32_t)n_groups, y,
                     depth, obs_depth);
  HIPCHK(hipGetLastError());
  return BNF_OK;
}

int bnf_depth_levels(bnf_handle* h, const int32_t* depth, int64_t n_samples, int64_t n_groups, const int32_t* need,
                     int32_t n_cov, const int32_t* k_query, int32_t n_query, const int32_t* obs_depth, int32_t* level,
                     double* achieved, double* joint, double* obs_pit) {
  const Forecast fc = forecast_view(h);
  if (const int rc = no_device()) return rc;
  if (!fc.bound) return fail(BNF_ERR_STATE, "not bound");
  if (!depth || n_samples < 1 || n_groups < 1 || n_groups > 0x7fffffffLL) return fail(BNF_ERR_INVALID, "argument");
  if (n_samples > BNF_SUMMARY_MAX_SAMPLES)
    return fail(BNF_ERR_INVALID, "%lld sample paths: the depths are counted in LDS, at most %d", (long long)n_samples,
                BNF_SUMMARY_MAX_SAMPLES);
  if (n_cov < 0 || n_cov > BNF_BAND_MAX_LEVELS || (n_cov > 0 && (!need || (!level && !achieved))))
    return fail(BNF_ERR_INVALID, "n_cov = %d: 0..%d coverage levels, with need and level or achieved", n_cov,
                BNF_BAND_MAX_LEVELS);
  if (n_query < 0 || n_query > BNF_BAND_MAX_LEVELS || (n_query > 0 && (!k_query || !joint)))
    return fail(BNF_ERR_INVALID, "n_query = %d: 0..%d band levels, with k_query and joint", n_query, BNF_BAND_MAX_LEVELS);
  if (obs_pit && !obs_depth) return fail(BNF_ERR_INVALID, "obs_pit needs obs_depth");
  if (n_cov < 1 && n_query < 1 && !obs_pit) return fail(BNF_ERR_INVALID, "no output asked for");
  BandLevels q;
  q.n_cov = n_cov;
  q.n_query = n_query;
  for (int32_t i = 0; i < kBandMaxLevels; ++i) { q.need[i] = 1; q.k_query[i] = 0; }
  for (int32_t i = 0; i < n_cov; ++i) {
    if (need[i] < 1 || need[i] > n_samples)
      return fail(BNF_ERR_INVALID, "need = %d: 1..%lld, the number of sample paths", need[i], (long long)n_samples);
    q.need[i] = need[i];
  }
  for (int32_t i = 0; i < n_query; ++i) q.k_query[i] = k_query[i];
  HIPCHK(hipSetDevice(fc.device));
  static std::atomic<uint64_t> attr_done{0};
  allow_lds(fc.device, &k_depth_levels, (int)(sizeof(int32_t) * (kSumMaxSamples + 1)), &attr_done);
  hipLaunchKernelGGL(k_depth_levels, dim3((unsigned)n_groups), dim3(kBandThreads), sizeof(int32_t) * (size_t)(n_samples + 1),
                     fc.stream, depth, (int32_t)n_samples, (int32_t)n_groups, q, obs_depth, level, achieved, joint, obs_pit);
  HIPCHK(hipGetLastError());
  return BNF_OK;
}

int bnf_sample_envelope(bnf_handle* h, const double* x, int64_t n_samples, int64_t n_cols, const int32_t* col_group,
                        const int32_t* level, int32_t n_levels, int64_t n_groups, double* lower, double* upper) {
  const Forecast fc = forecast_view(h);
  if (const int rc = bands_args(fc, x, n_samples, n_cols, col_group, n_groups)) return rc;
  if (!level || !lower || !upper) return fail(BNF_ERR_INVALID, "level, lower or upper is NULL");
  if (n_levels < 1 || n_levels > BNF_BAND_MAX_LEVELS)
    return fail(BNF_ERR_INVALID, "n_levels = %d: 1..%d", n_levels, BNF_BAND_MAX_LEVELS);
  HIPCHK(hipSetDevice(fc.device));
  const BandSlab b = band_slab(n_samples);
  static std::atomic<uint64_t> attr_done{0};
  allow_lds(fc.device, &k_sample_envelope, (int)(sizeof(uint64_t) * kSumMaxSamples), &attr_done);
  hipLaunchKernelGGL(k_sample_envelope, dim3(cdiv(n_cols, b.W)), dim3(b.threads),
                     sizeof(uint64_t) * (size_t)b.W * (size_t)b.P, fc.stream, x, (int32_t)n_samples, n_cols, (int32_t)b.P,
                     (int32_t)b.W, col_group, (int32_t)n_groups, level, n_levels, lower, upper);
  HIPCHK(hipGetLastError());
  return BNF_OK;
}

}  // extern "C"
