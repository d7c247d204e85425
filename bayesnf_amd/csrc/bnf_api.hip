// bnf_api.hip -- the training engine of libbnf_hip.so and its share of the C ABI (include/bnf.h): the handle, the
// train step, bnf_forward, the validation check, the debug and profile calls.  The forecast entry points are
// bnf_forecast.hip and the RCCL loader is bnf_comm.cpp; the three units share bnf_host.h.
//
// The reference runs a whole fit() as ONE XLA program (inference.py:621 is the
// single host->device dispatch).  Here the C side enqueues every kernel of every
// step on the caller's HIP stream without ever synchronising, so Python is not
// in the loop either.  One train step of all local members (MAP, depth L):
//
//   memset grad | pack weights | featurise | L x forward contraction |
//   output+likelihood+last-layer backward | (L-1) x dgrad | dgrad0 | featurise bwd |
//   L x wgrad | prior + Adam
//
// VI runs the same pipeline on members x S "virtual members" whose parameters
// are the reparameterised samples, bracketed by k_vi_sample / k_vi_adam.
#include <hip/hip_runtime.h>
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>            // the stable key-value sort of jax.random.permutation
#include <rocprim/device/device_segmented_radix_sort.hpp>  // (bnf_row_keys): the one library primitive in here

#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/bnf.h"
#include "bnf_host.h"
#include "bnf_gemm.h"
#include "bnf_kernels.h"
#include "bnf_panel.h"
#include "bnf_gemm8.h"
#include "bnf_validation.h"
#include "bnf_plan.h"

using namespace bnf;

// ---------------------------------------------------------------------------
// errors (bnf_host.h: the one definition of fail(), for every unit)
// ---------------------------------------------------------------------------
static thread_local char g_err[512] = "";
int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

// ---------------------------------------------------------------------------
// kernel ids for the event timer
// ---------------------------------------------------------------------------
enum KernelId {
  KID_PACK = 0, KID_FEAT, KID_FWD0, KID_FWD, KID_ROWLOSS, KID_LASTBWD, KID_DGRAD, KID_DGRAD0,
  KID_FEATBWD, KID_WGRAD0, KID_WGRAD, KID_ADAM, KID_VISAMPLE, KID_VIADAM, KID_FWDLAST, KID_PANEL, KID_COUNT
};
static const char* kKernelNames[KID_COUNT] = {
    "pack_weights", "featurize", "gemm_fwd_l0", "gemm_fwd", "row_loss", "last_bwd", "gemm_dgrad",
    "gemm_dgrad0", "feat_bwd", "gemm_wgrad_l0", "gemm_wgrad", "adam_map", "vi_sample", "vi_adam",
    "gemm_fwd_last", "panel_fwd_bwd"};

struct TimedLaunch {
  int kid;
  hipEvent_t t0, t1;
};

// Row pitch of the transposed pre-activations A_l^T is Bp + kAtPad elements: with pitch Bp
// (a multiple of 4 KiB in bytes at the benchmark sizes) the 32 columns one store / load
// instruction touches would all fall on the same L2 channel.
static constexpr int64_t kAtPad = 128;

struct bnf_handle {
  bnf_config cfg;
  Switches sw;     // the BNF_* environment, read once at bnf_create (bnf_plan.h)
  StepPlan plan;   // weight-gradient kernels, their launch order and the optimiser's kept ranges
  NetDev nd;
  FreqTab ft;
  bool bf16 = false;
  int f32_split = 0;      // BNF_DTYPE_F32S: the f32 contractions on split-bf16 MFMAs (GemmArgs.f32_split)
  uint8_t* Wf8[BNF_MAX_LAYERS] = {}; uint8_t* Wb8[BNF_MAX_LAYERS] = {};   // e4m3 x 2^5 K = 64 weight fragments (layers >= 1)
  uint8_t* H0q = nullptr; // (Ev, Bp, Fp) e4m3 copy of the features (layer-0 weight gradient)
  float* qscale = nullptr;   // (Ev) s_H s_dZ of the step: written by the panel kernel, read by the weight-gradient kernels
  int es = 4;          // element size of T
  int Ev = 0;          // virtual members = members * S
  int S = 1;
  int L = 0, W = 0, F = 0, Fp = 0, P = 0;
  // W: width the kernels run at (multiple of 64); Wt: the model's width.  Wt < W (pad): the
  // forward / backward kernels read theta_pad (stride Pf = Pp) and accumulate into gradf (k_pad_params)
  int Wt = 0;
  bool pad = false;
  int64_t Pf = 0, Pp = 0;
  float* gradf = nullptr;
  float* theta_pad = nullptr;
  int32_t* pad_src = nullptr;
  int32_t* fold_src = nullptr;
  std::vector<int32_t> pad_src_h, fold_src_h;
  int32_t* fbmeta = nullptr;
  int64_t N = 0, B = 0, Bp = 0;
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;            // weight-gradient contractions overlap the dgrad chain
  hipEvent_t ev_dz[BNF_MAX_LAYERS] = {};    // dZ_l is complete (main stream)
  hipEvent_t ev_wg = nullptr;               // all weight gradients are complete (stream2)
  bool bound = false;
  int64_t adam_t = 0;  // optimiser step count
  // caller buffers
  float* params = nullptr;   // MAP theta (E,P) | VI mu (E,P) then rho (E,P)
  float* state = nullptr;
  char* ws = nullptr;
  const float* X = nullptr;
  const float* y = nullptr;
  // carved from the workspace
  float* theta_c = nullptr;  // VI: z samples (Ev,P); MAP: == params
  float* grad = nullptr;
  float* stab = nullptr;
  float* stab_pred = nullptr;
  void* H0 = nullptr; void* H0t = nullptr;
  const float* ext_eps = nullptr;   // bnf_debug_vi_noise
  // the reference's VI noise stream (bnf_vi_noise_keys / bnf_vi_draw_keys): caller-owned key tables,
  // leaf tables in the workspace
  const uint32_t* vi_keys = nullptr; int64_t vi_key_rows = 0, vi_key_t0 = 0;
  const uint32_t* vi_draw_keys = nullptr; int64_t vi_draw_rows = 0;
  // caller's epoch shuffles (bnf_row_tables): (n_epochs, members, steps * B) int32 row ids from epoch row_tab_e0 on
  const int32_t* row_tab = nullptr; int64_t row_tab_epochs = 0, row_tab_e0 = 0;
  // ... or their keys (bnf_row_keys): the epoch's permutations are drawn on the device when the epoch starts
  const uint32_t* row_keys = nullptr; int64_t row_keys_epochs = 0, row_keys_e0 = 0; int32_t row_key_rounds = 0;
  uint32_t* perm_bits[2] = {nullptr, nullptr}; int32_t* perm_val[2] = {nullptr, nullptr};   // (members, N) each, hipMalloc'ed
  unsigned* perm_seg = nullptr; void* perm_tmp = nullptr; size_t perm_tmp_bytes = 0;
  bool perm_ready = false;       // every buffer above exists (set last: a failed allocation leaves none behind)
  size_t owned_bytes = 0;        // device memory the engine allocated itself (bnf_owned_bytes)
  int32_t* perm = nullptr; int64_t perm_epoch = -1;      // the current epoch's (members, N) row ids
  int32_t* leaf_off = nullptr; uint8_t* leaf_id = nullptr; int32_t n_leaves = 0;
  void* A[BNF_MAX_LAYERS]; void* H[BNF_MAX_LAYERS];
  void* dZ[BNF_MAX_LAYERS];
  void* Kn[BNF_MAX_LAYERS]; void* Kt[BNF_MAX_LAYERS];
  int64_t pack_batch[BNF_MAX_LAYERS];
  float* dH0 = nullptr; float* out = nullptr; float* ybat = nullptr; float* loss_raw = nullptr;
  float* vacc = nullptr; float* dv = nullptr;   // output-layer dot accumulator, d loss / d v
  void* Wf[BNF_MAX_LAYERS]; void* Wb[BNF_MAX_LAYERS];   // fragment-major packed weights
  void* park[BNF_MAX_LAYERS];                            // row-panel pipeline, depth > 2: parked pre-activations of the middle layers
    unsigned long long* prof_buf = nullptr;   // phase clocks (ABLATE builds)
  double prof_gap[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  double prof_blocks = 0;
  int prof_threads = 0;
  int num_cus = 256;          // multiProcessorCount of the device
  float* scal = nullptr;      // (Ev, kScalStride) transformed scalar leaves (k_member_scalars)
  StepState* step_state = nullptr;   // device: per-step state of the graph-replayed loop
  hipGraphExec_t graph_exec = nullptr;   // one captured full-batch MAP step (launch-bound sizes)
  int64_t graph_cols = 0;     // loss row stride the captured step was recorded with
  float* graph_losses = nullptr;
  float* qscratch = nullptr;  // quantile partials: 2*1024*2 + 2 floats
  float* dbg_a = nullptr; float* dbg_b = nullptr;  // small debug staging (gmu/grho)
  uint8_t* is_matrix = nullptr;
  size_t ws_bytes = 0;
  // profiling
  uint32_t prof = 0;   // bit k: bracket launches of kernel id k with HIP events
  std::vector<TimedLaunch> timed;
  std::vector<hipEvent_t> event_pool;
  size_t pool_used = 0;
  double acc_ms[KID_COUNT];
  int64_t acc_calls[KID_COUNT];
  // what bnf_create decided beside `plan` (bnf_plan.h)
  PipelinePlan pp;       // the forward / backward pipeline and its flags
  FeatBwdTable fb;       // row-panel kernel, H0L forms: per-column table of the fused featurisation backward (device copy: fbmeta)
  PanelForm form;        // the row-panel kernel's instantiation ...
  int form_index = -1;   // ... its row in kPanelForms / kPanelLaunch ...
  int32_t panels = 0;    // ... and its workgroups per member: Bp / form.panel_rows
};

static inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

// carve or just measure (base == nullptr) the workspace layout
static size_t carve(bnf_handle* h, char* base) {
  size_t off = 0;
  auto take = [&](size_t bytes) -> char* {
    char* p = base ? base + off : nullptr;
    off += (size_t)align_up((int64_t)bytes, 256);
    return p;
  };
  const int64_t Ev = h->Ev, Bp = h->Bp, W = h->W, Fp = h->Fp, P = h->P, es = h->es;
  const int nf2 = 2 * h->ft.n;
  const bool fo = h->cfg.forward_only != 0;
  h->grad = fo ? nullptr : (float*)take((size_t)Ev * P * 4);
  h->gradf = h->grad;
  if (h->pad) {
    h->theta_pad = (float*)take((size_t)Ev * h->Pp * 4);
    if (!fo) h->gradf = (float*)take((size_t)Ev * h->Pp * 4);
    h->pad_src = (int32_t*)take((size_t)(h->Pp - P) * 4);
    h->fold_src = (int32_t*)take((size_t)P * 4);
  }
  if (h->cfg.mode == BNF_MODE_VI) h->theta_c = (float*)take((size_t)Ev * P * 4);
  h->stab = (float*)take((size_t)std::max<int64_t>(1, h->N * nf2) * 4);
  h->stab_pred = (float*)take((size_t)std::max<int64_t>(1, Bp * nf2) * 4);
  h->H0 = take((size_t)Ev * Bp * Fp * es);
  h->H0q = (h->pp.q8 && !fo) ? (uint8_t*)take((size_t)Ev * Bp * Fp) : nullptr;
  h->qscale = (h->pp.q8 && !fo) ? (float*)take((size_t)Ev * 4) : nullptr;
  // no transposed copies (the weight-gradient contraction reads row-major, gemm_tn); the row-panel
  // kernel reads the features as MFMA A fragments from a second, fragment-major copy (H0t slot)
  // (the H0L forms stage the row-major copy in LDS instead and skip it)
  h->H0t = (h->pp.panel && !h->pp.h0l) ? take((size_t)Ev * Bp * Fp * es) : nullptr;
  for (int l = 0; l < h->L; ++l) {
    h->A[l] = (h->pp.panel || (h->pp.fuse_last && l == h->L - 1) || (h->pp.recompute_a0 && l == 0)) ? nullptr : take((size_t)Ev * W * (Bp + kAtPad) * es);  // A_l^T (W, Bp + pad)
    h->H[l] = (l < h->L - 1) ? take((size_t)Ev * Bp * W * es) : nullptr;       // H_{l+1} (Bp, W)
    h->dZ[l] = fo ? nullptr : take((size_t)Ev * Bp * W * es);
    const int64_t npad = (l == 0) ? Fp : W;
    h->pack_batch[l] = npad * W;
    h->Kn[l] = h->pp.panel ? nullptr : take((size_t)Ev * npad * W * es);
    h->Kt[l] = h->pp.panel ? nullptr : take((size_t)Ev * npad * W * es);
  }
  for (int l = 0; l < h->L; ++l) {
    const int64_t npad = (l == 0) ? Fp : W;
    h->Wf[l] = h->pp.panel ? take((size_t)Ev * npad * W * es) : nullptr;
    h->Wb[l] = h->pp.panel ? take((size_t)Ev * npad * W * es) : nullptr;
    h->park[l] = (h->pp.panel && !fo && l >= 1 && l < h->L - 1) ? take((size_t)Ev * Bp * W * es) : nullptr;
    h->Wf8[l] = (h->pp.c8 && l >= 1) ? (uint8_t*)take((size_t)Ev * W * W) : nullptr;
    h->Wb8[l] = (h->pp.c8 && l >= 1) ? (uint8_t*)take((size_t)Ev * W * W) : nullptr;
  }
  h->dH0 = fo ? nullptr : (float*)take((size_t)Ev * Fp * Bp * 4);            // dH0^T (Fp, Bp)
  h->out = (float*)take((size_t)Ev * Bp * 4);
  h->vacc = (float*)take((size_t)Ev * Bp * 4);
  h->dv = fo ? nullptr : (float*)take((size_t)Ev * Bp * 4);
  h->ybat = fo ? nullptr : (float*)take((size_t)Ev * Bp * 4);
  h->loss_raw = (float*)take((size_t)Ev * 4);
  h->qscratch = (float*)take((size_t)(4 * 1024 + 16) * 4);
  h->scal = (float*)take((size_t)Ev * kScalStride * 4);
  h->step_state = (StepState*)take(sizeof(StepState));
  h->dbg_a = (float*)take(256);
  h->is_matrix = (uint8_t*)take((size_t)P);
  h->fbmeta = h->fb.meta.empty() ? nullptr : (int32_t*)take(h->fb.meta.size() * 4);
  if (h->cfg.mode == BNF_MODE_VI) {
    h->leaf_off = (int32_t*)take(260 * 4);
    h->leaf_id = (uint8_t*)take((size_t)P);
  }
  return off;
}

// ---------------------------------------------------------------------------
// timed launch helper
// ---------------------------------------------------------------------------
struct LaunchScope {
  bnf_handle* h;
  int kid;
  hipEvent_t t0 = nullptr, t1 = nullptr;
  bool on;
  hipStream_t st;
  LaunchScope(bnf_handle* h_, int kid_, hipStream_t st_ = nullptr, bool use_st = false)
      : h(h_), kid(kid_), on(((h_->prof >> kid_) & 1u) != 0), st(use_st ? st_ : h_->stream) {
    if (!on) return;
    auto get = [&]() {
      if (h->pool_used == h->event_pool.size()) {
        hipEvent_t ev;
        hipEventCreate(&ev);
        h->event_pool.push_back(ev);
      }
      return h->event_pool[h->pool_used++];
    };
    t0 = get();
    t1 = get();
    hipEventRecord(t0, st);
  }
  ~LaunchScope() {
    if (!on) return;
    hipEventRecord(t1, st);
    h->timed.push_back({kid, t0, t1});
  }
};

static void drain_timers(bnf_handle* h) {
  for (auto& t : h->timed) {
    hipEventSynchronize(t.t1);
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, t.t0, t.t1) == hipSuccess) {
      h->acc_ms[t.kid] += ms;
      h->acc_calls[t.kid] += 1;
    }
  }
  h->timed.clear();
  h->pool_used = 0;
}

// ---------------------------------------------------------------------------
// contraction launcher
// ---------------------------------------------------------------------------
// Phase clocks (perf experiments; ABLATE builds only): BNF_PHASE_PROF=<kernel name> makes every
// launch of that contraction record clock64() at up to 8 marks per workgroup; the mean gaps
// are printed when the handle is destroyed.
static void phase_prof_begin(bnf_handle* h, int kid, unsigned blocks, EpiArgs* ep) {
  ep->prof = nullptr;
#ifdef BNF_ENABLE_ABLATE
  if (h->sw.phase_prof != kKernelNames[kid]) return;
  if (!h->prof_buf) (void)hipMalloc(&h->prof_buf, (size_t)(1 << 20) * 16 * sizeof(unsigned long long));
  if (blocks > (1u << 20)) return;
  (void)hipMemsetAsync(h->prof_buf, 0, (size_t)blocks * 128, h->stream);
  ep->prof = h->prof_buf;
#endif
}
static void phase_prof_end(bnf_handle* h, int kid, unsigned blocks, int threads) {
#ifdef BNF_ENABLE_ABLATE
  if (h->sw.phase_prof != kKernelNames[kid] || !h->prof_buf || blocks > (1u << 20)) return;
  std::vector<unsigned long long> host((size_t)blocks * 16);
  (void)hipStreamSynchronize(h->stream);
  (void)hipMemcpy(host.data(), h->prof_buf, host.size() * 8, hipMemcpyDeviceToHost);
  for (unsigned b = 0; b < blocks; ++b) {
    unsigned long long prev = host[(size_t)b * 16];
    for (int k = 1; k < 16; ++k) {
      const unsigned long long t = host[(size_t)b * 16 + k];
      if (!t) continue;
      h->prof_gap[k] += (double)(t - prev);
      prev = t;
    }
    h->prof_gap[0] += (double)(prev - host[(size_t)b * 16]);
  }
  h->prof_blocks += blocks;
  h->prof_threads = threads;
#endif
}

template <typename T, int EPI, int TAG, int WGM, int WGN>
static void launch_gemm_wg(bnf_handle* h, int kid, GemmArgs g, const EpiArgs& ep) {
  constexpr int kLds = Mma<T>::lds_bytes(WGM, WGN, epi_extra_lds(EPI, WGM, WGN, (int)sizeof(T)));
  static_assert(kLds <= 160 * 1024, "LDS per workgroup");
  g.tiles_m = (g.M + 64 * WGM - 1) / (64 * WGM);
  g.tiles_n = (g.N + 64 * WGN - 1) / (64 * WGN);
  if (g.splitk < 1) g.splitk = 1;
  if constexpr (std::is_same<T, float>::value) {
    if (h->f32_split) {      // BNF_DTYPE_F32S: the split-bf16 instantiation of the same kernel
      // B is a packed Dense kernel (split when packed: k_pack_weights) everywhere but in the test entry's plain product
      constexpr int kS = EPI == EPI_PLAIN ? 1 : 2;
      static std::atomic<uint64_t> attr_done_s{0};
      allow_lds(h->cfg.device, &gemm_nt<T, EPI, TAG, WGM, WGN, kS>, kLds, &attr_done_s);
      const unsigned blocks = (unsigned)(g.members * g.tiles_m * g.tiles_n * g.splitk);
      EpiArgs ep2 = ep;
      ep2.ablate = h->sw.ablate;
      phase_prof_begin(h, kid, blocks, &ep2);
      {
        LaunchScope ls(h, kid);
        hipLaunchKernelGGL((gemm_nt<T, EPI, TAG, WGM, WGN, kS>), dim3(blocks), dim3(64 * WGM * WGN), kLds, h->stream, g, ep2);
      }
      phase_prof_end(h, kid, blocks, 64 * WGM * WGN);
      return;
    }
  }
  static std::atomic<uint64_t> attr_done{0};
  allow_lds(h->cfg.device, &gemm_nt<T, EPI, TAG, WGM, WGN>, kLds, &attr_done);
  const unsigned blocks = (unsigned)(g.members * g.tiles_m * g.tiles_n * g.splitk);
  EpiArgs ep2 = ep;
  ep2.ablate = h->sw.ablate;
  phase_prof_begin(h, kid, blocks, &ep2);
  LaunchScope ls(h, kid);
  hipLaunchKernelGGL((gemm_nt<T, EPI, TAG, WGM, WGN>), dim3(blocks), dim3(64 * WGM * WGN), kLds, h->stream, g, ep2);
  phase_prof_end(h, kid, blocks, 64 * WGM * WGN);
}

// 256 x 256 tiles (16 waves) for the bf16 forward contractions whose output width is a
// multiple of 256; 128 x 128 tiles otherwise (and always for f32, whose epilogue tile would
// not fit in LDS).
template <typename T, int EPI, int TAG>
static void launch_gemm(bnf_handle* h, int kid, GemmArgs g, const EpiArgs& ep) {
  // (measured on C2: forward 916 -> 811 us, forward layer 0 497 -> 445 us; the backward-data
  // epilogue needs more registers than 16 waves leave it and got slower, 864 -> 1172 us)
  if constexpr (sizeof(T) == 2 && EPI == EPI_FWD) {
    // (layer 0 has a short K loop and, since A_0 is recomputed, writes only H_1: 316 us with
    // 128 x 128 tiles vs 362 us with 256 x 256 at C2)
    if (g.N % 256 == 0 && g.M >= 256 && h->sw.big_tiles && (g.K >= 256 || h->sw.big_tiles == 2)) {
      launch_gemm_wg<T, EPI, TAG, 4, 4>(h, kid, g, ep);
      return;
    }
  }
  launch_gemm_wg<T, EPI, TAG, 2, 2>(h, kid, g, ep);
}

// The one-kernel last layer (EPI_LAST: 128-row panels spanning the layer): one case per width fused_last_width() of
// bnf_plan.h admits -- PipelinePlan::fuse_last is on for no other
static_assert(fused_last_width(64, false) && fused_last_width(128, false) && fused_last_width(256, false) && fused_last_width(512, true) &&
              !fused_last_width(512, false) && !fused_last_width(1024, true) && !fused_last_width(192, true),
              "launch_fwd_last_obs has a case for every width the plan fuses");
template <typename T, int TAG>
static void launch_fwd_last_obs(bnf_handle* h, GemmArgs g, const EpiArgs& ep) {
  switch (g.N) {
    case 64: launch_gemm_wg<T, EPI_LAST, TAG, 2, 1>(h, KID_FWDLAST, g, ep); break;
    case 128: launch_gemm_wg<T, EPI_LAST, TAG, 2, 2>(h, KID_FWDLAST, g, ep); break;
    case 256: launch_gemm_wg<T, EPI_LAST, TAG, 2, 4>(h, KID_FWDLAST, g, ep); break;
    case 512:
      // 64-row panels: two 8-wave workgroups per CU (3.24 vs 3.28 ms/step for one 16-wave
      // workgroup on 128-row panels, profiles/r01g)
      if constexpr (sizeof(T) == 2) launch_gemm_wg<T, EPI_LAST, TAG, 1, 8>(h, KID_FWDLAST, g, ep);
      break;
  }
}
// TAG 3: NORMAL likelihood only; TAG 4: NB / ZINB as well (lgamma / digamma in the row phase)
template <typename T>
static void launch_fwd_last(bnf_handle* h, GemmArgs g, const EpiArgs& ep) {
  if (ep.obs == BNF_OBS_NORMAL) launch_fwd_last_obs<T, 3>(h, g, ep);
  else launch_fwd_last_obs<T, 4>(h, g, ep);
}

template <typename T, int TAG, int WG>
static void launch_gemm_tn_wg(bnf_handle* h, int kid, GemmArgs g, const EpiArgs& ep, hipStream_t st) {
  constexpr int kLds = gemm_tn_lds<T>(WG);
  g.tiles_m = (g.M + 64 * WG - 1) / (64 * WG);
  g.tiles_n = (g.N + 64 * WG - 1) / (64 * WG);
  if (g.splitk < 1) g.splitk = 1;
  if constexpr (std::is_same<T, float>::value) {
    if (h->f32_split) {      // BNF_DTYPE_F32S
      static std::atomic<uint64_t> attr_done_s{0};
      allow_lds(h->cfg.device, &gemm_tn<T, TAG, WG, true>, kLds, &attr_done_s);
      const unsigned blocks = (unsigned)(g.members * g.tiles_m * g.tiles_n * g.splitk);
      LaunchScope ls(h, kid, st, true);
      hipLaunchKernelGGL((gemm_tn<T, TAG, WG, true>), dim3(blocks), dim3(64 * WG * WG), kLds, st, g, ep);
      return;
    }
  }
  static std::atomic<uint64_t> attr_done{0};
  allow_lds(h->cfg.device, &gemm_tn<T, TAG, WG>, kLds, &attr_done);
  const unsigned blocks = (unsigned)(g.members * g.tiles_m * g.tiles_n * g.splitk);
  LaunchScope ls(h, kid, st, true);
  hipLaunchKernelGGL((gemm_tn<T, TAG, WG>), dim3(blocks), dim3(64 * WG * WG), kLds, st, g, ep);
}
// layer-0 weight gradient as a 64 x 512 row stream (gemm_tn_skinny): Fp = 64, W a multiple of 512
static void launch_gemm_tn_skinny(bnf_handle* h, int kid, GemmArgs g, const EpiArgs& ep, hipStream_t st) {
  g.tiles_m = 1;
  g.tiles_n = g.N / 512;
  if (g.splitk < 1) g.splitk = 1;
  static std::atomic<uint64_t> attr_done{0};
  allow_lds(h->cfg.device, &gemm_tn_skinny, kSkLds, &attr_done);
  const unsigned blocks = (unsigned)((int64_t)g.members * g.tiles_n * g.splitk);
  LaunchScope ls(h, kid, st, true);
  hipLaunchKernelGGL(gemm_tn_skinny, dim3(blocks), dim3(512), kSkLds, st, g, ep);
}
// the same stream with the fused featurisation backward in it (StepPlan::featbwd_in_wgrad: bf16, Fp = 64, the column
// table exists, at most kSkFbCols Fourier columns); the panel kernel of this step ended behind its dZ0 epilogue
static void launch_gemm_tn_skinny_featbwd(bnf_handle* h, int kid, GemmArgs g, const EpiArgs& ep, hipStream_t st) {
  g.tiles_m = 1;
  g.tiles_n = g.N / 512;
  if (g.splitk < 1) g.splitk = 1;
  FeatBwdArgs fw{};
  fw.Wb0 = (const bf16_t*)h->Wb[0]; fw.wb_batch = h->pack_batch[0];
  fw.scal = h->scal; fw.fbmeta = h->fbmeta;
  fw.F = h->F; fw.off_lsa = h->nd.off_lsa; fw.n_groups = h->nd.n_groups; fw.n_inputs = h->nd.D;
  fw.scal_stride = kScalStride; fw.scal_gfac = kScalGfac; fw.scal_sp_in = kScalGroup + h->fb.in_group;
  static std::atomic<uint64_t> attr_done{0};
  allow_lds(h->cfg.device, &gemm_tn_skinny_featbwd, kSkLdsFb, &attr_done);
  const unsigned blocks = (unsigned)((int64_t)g.members * g.tiles_n * g.splitk);
  LaunchScope ls(h, kid, st, true);
  hipLaunchKernelGGL(gemm_tn_skinny_featbwd, dim3(blocks), dim3(512), kSkLdsFb, st, g, ep, fw);
}
// `kind`: what wgrad_plan chose (WG_*); g.splitk is the plan's too
template <typename T, int TAG>
static void launch_gemm_tn(bnf_handle* h, int kid, GemmArgs g, const EpiArgs& ep, hipStream_t st, int kind) {
  if constexpr (sizeof(T) == 2 && TAG == 0) {
    if (kind == WG_SKINNY) {
      launch_gemm_tn_skinny(h, kid, g, ep, st);
      return;
    }
  }
  if constexpr (sizeof(T) == 2) {
    if (kind == WG_RING) {   // the 256 x 256 tile with the K loop as a four-stage ring
      g.tiles_m = g.M / 256; g.tiles_n = g.N / 256;
      if (g.splitk < 1) g.splitk = 1;
      static std::atomic<uint64_t> attr_done{0}, attr_done_s{0};
      const unsigned blocks = (unsigned)(g.members * g.tiles_m * g.tiles_n * g.splitk * (g.n_multi > 1 ? g.n_multi : 1));
      EpiArgs ep2 = ep;
      ep2.ablate = h->sw.ablate;
      LaunchScope ls(h, kid, st, true);
      if (g.splitk == 1) {   // plain stores: accumulators transposed, 16-byte stores
        allow_lds(h->cfg.device, &gemm_tn_ring<TAG, true>, kRgLds, &attr_done_s);
        hipLaunchKernelGGL((gemm_tn_ring<TAG, true>), dim3(blocks), dim3(512), kRgLds, st, g, ep2);
      } else {
        allow_lds(h->cfg.device, &gemm_tn_ring<TAG, false>, kRgLds, &attr_done);
        hipLaunchKernelGGL((gemm_tn_ring<TAG, false>), dim3(blocks), dim3(512), kRgLds, st, g, ep2);
      }
      return;
    }
  }
  if (kind == WG_TN256) {
    launch_gemm_tn_wg<T, TAG, 4>(h, kid, g, ep, st);
    return;
  }
  launch_gemm_tn_wg<T, TAG, 2>(h, kid, g, ep, st);
}

// the weight gradient on fp8 operand copies (bnf_gemm8.h): the same plan (wgrad_plan's kind and split-K), the fp8 kernel of
// that kind; both 128 x 128 and 256 x 256 two-stage kinds go to the generic 128 x 128 kernel
template <int TAG>
static void launch_gemm_tn8(bnf_handle* h, int kid, GemmArgs g, const EpiArgs& ep, hipStream_t st, int kind) {
  if (g.splitk < 1) g.splitk = 1;
  EpiArgs ep2 = ep;
  ep2.ablate = h->sw.ablate;
  LaunchScope ls(h, kid, st, true);
  if (kind == WG_SKINNY && TAG == 0) {
    g.tiles_m = 1; g.tiles_n = g.N / 512;
    static std::atomic<uint64_t> attr_done{0};
    allow_lds(h->cfg.device, &gemm_tn_skinny8, kSk8Lds, &attr_done);
    hipLaunchKernelGGL(gemm_tn_skinny8, dim3((unsigned)((int64_t)g.members * g.tiles_n * g.splitk)), dim3(512), kSk8Lds, st, g, ep2);
  } else if (kind == WG_RING) {
    g.tiles_m = g.M / 256; g.tiles_n = g.N / 256;
    static std::atomic<uint64_t> attr_done{0}, attr_done_s{0};
    const unsigned blocks = (unsigned)(g.members * g.tiles_m * g.tiles_n * g.splitk * (g.n_multi > 1 ? g.n_multi : 1));
    if (g.splitk == 1) {
      allow_lds(h->cfg.device, &gemm_tn_ring8<TAG, true>, kRgLds, &attr_done_s);
      hipLaunchKernelGGL((gemm_tn_ring8<TAG, true>), dim3(blocks), dim3(512), kRgLds, st, g, ep2);
    } else {
      allow_lds(h->cfg.device, &gemm_tn_ring8<TAG, false>, kRgLds, &attr_done);
      hipLaunchKernelGGL((gemm_tn_ring8<TAG, false>), dim3(blocks), dim3(512), kRgLds, st, g, ep2);
    }
  } else {
    g.tiles_m = (g.M + 127) / 128; g.tiles_n = (g.N + 127) / 128;
    static std::atomic<uint64_t> attr_done{0};
    allow_lds(h->cfg.device, &gemm_tn8<TAG>, kTn8Lds, &attr_done);
    hipLaunchKernelGGL((gemm_tn8<TAG>), dim3((unsigned)(g.members * g.tiles_m * g.tiles_n * g.splitk)), dim3(256), kTn8Lds, st, g, ep2);
  }
}

// ---------------------------------------------------------------------------
// pipeline pieces, templated on the storage type
// ---------------------------------------------------------------------------
template <typename T>
static void run_pack(bnf_handle* h, const float* theta, int nmem) {
  LaunchScope ls(h, KID_PACK);
  PackWJobs jb{};
  jb.n_layers = h->L;
  int tiles = 0;
  for (int l = 0; l < h->L; ++l) {
    jb.off_kernel[l] = h->nd.off_kernel[l];
    jb.n_in[l] = (l == 0) ? h->F : h->W;
    jb.n_pad[l] = (l == 0) ? h->Fp : h->W;
    jb.tile0[l] = tiles;
    tiles += (jb.n_pad[l] / 32) * (h->W / 32);
    jb.Kn[l] = h->Kn[l]; jb.Kt[l] = h->Kt[l]; jb.pack_batch[l] = h->pack_batch[l];
  }
  jb.tile0[h->L] = tiles;
  hipLaunchKernelGGL((k_pack_weights<T>), dim3((unsigned)tiles, (unsigned)nmem), dim3(256), 0, h->stream, theta,
                     (int64_t)h->Pf, jb, (int32_t)h->W, (int32_t)(sizeof(T) == 4 && h->f32_split ? 1 : 0), h->nd, h->scal);
}

// Hidden layer l's forward contraction H_l . K_l^T / sqrt(fan_in_l) and the parameter side of its epilogue; the caller
// adds where the results go (run_forward: activations; run_backward's one-kernel last layer: the likelihood's outputs)
static void fwd_layer_args(const bnf_handle* h, const float* theta, int nmem, int64_t rows, int l, GemmArgs* g, EpiArgs* ep) {
  const int64_t Bp = h->Bp;
  g->A = (l == 0) ? h->H0 : h->H[l - 1];
  g->a_ld = (l == 0) ? h->Fp : h->W;
  g->a_batch = Bp * g->a_ld;
  g->B = h->Kt[l];
  g->b_ld = g->a_ld;
  g->b_batch = h->pack_batch[l];
  g->M = (int)rows; g->N = h->W; g->K = g->a_ld; g->splitk = 1; g->members = nmem;
  ep->theta = theta; ep->theta_stride = h->Pf;
  ep->scale = 1.0f / sqrtf((float)((l == 0) ? h->F : h->Wt));
  ep->off_bias = h->nd.off_bias[l];
  ep->off_layer_scale = h->nd.off_ls[l];
  ep->off_act_weight = h->nd.off_law;
  ep->scal = h->scal; ep->scal_stride = kScalStride; ep->layer = l;
  ep->off_ko = h->nd.off_kernel[h->L];
  ep->act_batch = Bp * h->W; ep->ld = h->W;
}

// featurise + forward contractions for `rows` batch rows of `nmem` (virtual)
// members; leaves vacc[row] = H_L[row] . k_o for the row-loss kernel.
template <typename T>
static void run_forward(bnf_handle* h, const float* theta, int nmem, const RowSrc& rs,
                        const float* X, const float* stab, const float* y, int64_t rows,
                        bool train) {
  const int64_t Bp = h->Bp;
  {
    LaunchScope ls(h, KID_FEAT);
    dim3 grid(cdiv(rows, kFeatRows) * (unsigned)nmem);
    const size_t lds = (size_t)kFeatRows * (h->Fp + 16 / h->es) * h->es;
    static std::atomic<uint64_t> attr_done{0};
    allow_lds(h->cfg.device, &k_featurize<T>, 160 * 1024, &attr_done);
    hipLaunchKernelGGL((k_featurize<T>), grid, dim3(kFeatRows), lds, h->stream, h->nd, rs, X, stab,
                       y, h->scal, rows, (T*)h->H0, Bp * h->Fp,
                       (T*)nullptr, (int64_t)h->Fp * Bp, (int32_t)Bp,
                       train ? h->ybat : (float*)nullptr, Bp, (int32_t)nmem, (int32_t)0);
  }
  const int n_layers = (train && h->pp.fuse_last) ? h->L - 1 : h->L;   // EPI_LAST runs in run_backward
  for (int l = 0; l < n_layers; ++l) {
    const bool last = l == h->L - 1;
    GemmArgs g{};
    EpiArgs ep{};
    fwd_layer_args(h, theta, nmem, rows, l, &g, &ep);
    ep.out_a = h->A[l];   // null: not materialised in this pipeline
    ep.out_h = last ? nullptr : h->H[l];
    ep.vdot = last ? h->vacc : nullptr;
    ep.vdot_batch = Bp;
    ep.actt_batch = (int64_t)h->W * (Bp + kAtPad);
    ep.ldt = (int32_t)(Bp + kAtPad);
    if (l == 0) launch_gemm<T, EPI_FWD, 0>(h, KID_FWD0, g, ep);
    else launch_gemm<T, EPI_FWD, 1>(h, KID_FWD, g, ep);
  }
}

struct LossSink {
  float* loss; int64_t stride; float scale;   // loss[(e/S)*stride] += scale * step_loss
  float* raw;                                  // optional per-virtual-member raw loss
  const StepState* st = nullptr;               // graph replay: per-step state in device memory
};

static_assert(kPlanBM == kBM && kPlanBN == kBN && kPlanSkRows == kSkRows && kPlanFbCols == kSkFbCols,
              "bnf_plan.h counts tiles of the kernels' sizes");

static PlanShape plan_shape(const bnf_handle* h) {
  PlanShape ps{};
  ps.bf16 = h->bf16; ps.L = h->L; ps.W = h->W; ps.F = h->F; ps.Fp = h->Fp; ps.Bp = h->Bp;
  ps.num_cus = h->num_cus; ps.panel = h->pp.panel; ps.pad = h->pad;
  for (int l = 0; l < h->L; ++l) ps.off_kernel[l] = h->nd.off_kernel[l];
  ps.fp8 = h->pp.q8; ps.featbwd_fused = !h->fb.meta.empty(); ps.n_fourier = h->fb.n_fourier;
  return ps;
}

// weight gradient of layer l from the row-major H_l / dZ_l left in HBM, on stream `st`
template <typename T>
static void run_wgrad_layer(bnf_handle* h, int nmem, int l, hipStream_t st) {
  const int64_t Bp = h->Bp;
  // dK_l = H_l^T . dZ_l / sqrt(fan_in_l): contraction over the batch rows of the
  // row-major activations (transpose reads in LDS, no transposed copies in HBM)
  GemmArgs g{};
  g.A = (l == 0) ? h->H0 : h->H[l - 1];
  g.a_ld = (l == 0) ? h->Fp : h->W; g.a_batch = Bp * g.a_ld;
  g.B = h->dZ[l]; g.b_ld = h->W; g.b_batch = Bp * h->W;
  g.M = (l == 0) ? h->F : h->W; g.N = h->W; g.K = (int)Bp; g.members = nmem;
  const WgradPlan plan = h->plan.layer[l];
  g.splitk = plan.splitk;
  EpiArgs ep{};
  ep.scale = 1.0f / sqrtf((float)((l == 0) ? h->F : h->Wt));
  ep.grad = h->gradf; ep.grad_stride = h->Pf; ep.off_out = h->nd.off_kernel[l]; ep.ld_f32 = h->W;
  if (l == 0 && h->pp.fold0) {   // the ones column behind the features: its row of the product is d bias0
    ep.bias_row = 1; ep.off_bias_row = h->nd.off_bias[0];
  }
  if constexpr (sizeof(T) == 2) {
    if (h->pp.q8) {   // the fp8 copies: same shapes, one byte per element
      if (l == 0) g.A = h->H0q;
      ep.qscale = h->qscale;
      if (l == 0) launch_gemm_tn8<0>(h, KID_WGRAD0, g, ep, st, plan.kind);
      else launch_gemm_tn8<1>(h, KID_WGRAD, g, ep, st, plan.kind);
      return;
    }
  }
  if constexpr (sizeof(T) == 2) {
    if (l == 0 && h->plan.featbwd_in_wgrad) {
      launch_gemm_tn_skinny_featbwd(h, KID_WGRAD0, g, ep, st);
      return;
    }
  }
  if (l == 0) launch_gemm_tn<T, 0>(h, KID_WGRAD0, g, ep, st, plan.kind);
  else launch_gemm_tn<T, 1>(h, KID_WGRAD, g, ep, st, plan.kind);
}

// dZ_l has just been enqueued on the main stream: start its weight gradient on the side
// stream (or in line when overlap is off / unavailable)
template <typename T>
static void wgrad_after_dz(bnf_handle* h, int nmem, int l) {
  if (h->sw.overlap && h->stream2) {
    (void)hipEventRecord(h->ev_dz[l], h->stream);
    (void)hipStreamWaitEvent(h->stream2, h->ev_dz[l], 0);
    run_wgrad_layer<T>(h, nmem, l, h->stream2);
  } else {
    run_wgrad_layer<T>(h, nmem, l, h->stream);
  }
}
// before the optimiser: every weight gradient must have landed
static void wgrad_join(bnf_handle* h) {
  if (h->sw.overlap && h->stream2) {
    (void)hipEventRecord(h->ev_wg, h->stream2);
    (void)hipStreamWaitEvent(h->stream, h->ev_wg, 0);
  }
}

// the W x W weight gradients of layers 1 .. L-1 as ONE launch of the ring kernel (same shape, same split-K = 1):
// 3 x 320 tiles at C3/8 are 4 rounds of the chip instead of 3 x 2 (StepPlan::merged)
static void run_wgrad_merged(bnf_handle* h, int nmem) {
  const int64_t Bp = h->Bp;
  GemmArgs g{};
  g.a_ld = h->W; g.a_batch = Bp * h->W; g.b_ld = h->W; g.b_batch = Bp * h->W;
  g.M = h->W; g.N = h->W; g.K = (int)Bp; g.members = nmem; g.splitk = 1;
  g.n_multi = h->L - 1;
  for (int l = 1; l < h->L; ++l) {
    g.A_multi[l - 1] = h->H[l - 1]; g.B_multi[l - 1] = h->dZ[l]; g.off_out_multi[l - 1] = h->nd.off_kernel[l];
  }
  g.A = g.A_multi[0]; g.B = g.B_multi[0];
  EpiArgs ep{};
  ep.scale = 1.0f / sqrtf((float)h->Wt);
  ep.grad = h->gradf; ep.grad_stride = h->Pf; ep.off_out = h->nd.off_kernel[1]; ep.ld_f32 = h->W;
  if (h->pp.q8) {
    ep.qscale = h->qscale;
    launch_gemm_tn8<1>(h, KID_WGRAD, g, ep, h->stream, WG_RING);
  } else {
    launch_gemm_tn<bf16_t, 1>(h, KID_WGRAD, g, ep, h->stream, WG_RING);
  }
}
// the row-panel pipeline's weight gradients, in the plan's order (every dZ_l exists when this runs)
static void run_wgrad(bnf_handle* h, int nmem) {
  for (int i = 0; i < h->plan.n_launch; ++i) {
    if (h->plan.launch[i] == kWgradMerged) run_wgrad_merged(h, nmem);
    else wgrad_after_dz<bf16_t>(h, nmem, h->plan.launch[i]);
  }
  wgrad_join(h);
}

// backward of one step: fills h->gradf (likelihood part)
template <typename T>
static void run_backward(bnf_handle* h, const float* theta, int nmem, const RowSrc& rs,
                         int64_t rows, float c, const LossSink& sink) {
  const int64_t Bp = h->Bp;
  const int L = h->L;
  if (h->pp.fuse_last) {
    // last hidden layer forward + output layer + likelihood + backward through its
    // activation in one kernel (EPI_LAST): writes out, dZ_{L-1} and every gradient the
    // row-loss and last-backward kernels produce
    const int l = L - 1;
    GemmArgs g{};
    EpiArgs ep{};
    fwd_layer_args(h, theta, nmem, rows, l, &g, &ep);
    ep.inv_sw = 1.0f / sqrtf((float)h->Wt);
    ep.out_h = h->dZ[l];
    ep.grad = h->gradf; ep.grad_stride = h->Pf;
    ep.ybat = h->ybat; ep.row_batch = Bp;
    ep.out = h->out; ep.out_batch = Bp;
    ep.loss = sink.loss; ep.loss_raw = sink.raw; ep.loss_stride = sink.stride; ep.S = h->S;
    ep.loss_scale = sink.scale; ep.lik_c = c; ep.st = sink.st;
    ep.off_os = h->nd.off_os; ep.off_bias_out = h->nd.off_bias[L];
    ep.off_lns = h->nd.off_lns; ep.off_shape = h->nd.off_shape; ep.off_infl = h->nd.off_infl;
    ep.obs = h->nd.obs;
    launch_fwd_last<T>(h, g, ep);
    wgrad_after_dz<T>(h, nmem, L - 1);
  } else {
    {
      RowLossArgs a{};
      a.theta = theta; a.theta_stride = h->Pf; a.B = rows;
      a.vacc = h->vacc; a.vacc_batch = Bp; a.ybat = h->ybat;
      a.out = h->out; a.out_batch = Bp; a.dv = h->dv;
      a.grad = h->gradf; a.grad_stride = h->Pf;
      a.loss = sink.loss; a.loss_stride = sink.stride; a.S = h->S; a.loss_scale = sink.scale;
      a.c = c; a.loss_raw = sink.raw; a.st = sink.st;
      LaunchScope ls(h, KID_ROWLOSS);
      hipLaunchKernelGGL((k_row_loss<true>), dim3(cdiv(rows, 256), (unsigned)nmem), dim3(256), 0,
                         h->stream, h->nd, a);
    }
    {
      LastBwdArgs a{};
      a.theta = theta; a.theta_stride = h->Pf;
      a.At = h->A[L - 1]; a.dZ = h->dZ[L - 1];
      a.act_batch = Bp * h->W; a.actt_batch = (int64_t)h->W * (Bp + kAtPad); a.ldt = (int32_t)(Bp + kAtPad);
      a.dv = h->dv; a.dv_batch = Bp; a.grad = h->gradf; a.grad_stride = h->Pf;
      a.n_row_tiles = (int32_t)((rows + 63) / 64);
      a.tiles_per_task = 4;
      const int tasks = (h->W / 64) * ((a.n_row_tiles + a.tiles_per_task - 1) / a.tiles_per_task);
      {
        LaunchScope ls(h, KID_LASTBWD);
        hipLaunchKernelGGL((k_last_bwd<T>), dim3(cdiv(tasks, 4), (unsigned)nmem), dim3(256), 0, h->stream,
                           h->nd, a);
      }
      wgrad_after_dz<T>(h, nmem, L - 1);
    }
}
  for (int l = L - 1; l >= 0; --l) {
    // dH_l = dZ_l . K_l^T / sqrt(fan_in_l)
    GemmArgs g{};
    g.A = h->dZ[l]; g.a_ld = h->W; g.a_batch = Bp * h->W;
    g.B = h->Kn[l]; g.b_ld = h->W; g.b_batch = h->pack_batch[l];
    g.M = (int)rows; g.K = h->W; g.splitk = 1; g.members = nmem;
    EpiArgs ep{};
    ep.theta = theta; ep.theta_stride = h->Pf;
    ep.grad = h->gradf; ep.grad_stride = h->Pf;
    if (l > 0) {
      g.N = h->W;
      ep.scale = 1.0f / sqrtf((float)h->Wt);
      ep.off_bias = h->nd.off_bias[l - 1];
      ep.off_layer_scale = h->nd.off_ls[l - 1];
      ep.off_act_weight = h->nd.off_law;
      ep.scal = h->scal; ep.scal_stride = kScalStride; ep.layer = l - 1;
      ep.in_a = h->A[l - 1];
      ep.out_h = h->dZ[l - 1];
      ep.act_batch = Bp * h->W; ep.actt_batch = (int64_t)h->W * (Bp + kAtPad);
      ep.ld = h->W; ep.ldt = (int32_t)(Bp + kAtPad);
      if (l == 1 && h->pp.recompute_a0) {
        ep.aux_a = h->H0; ep.aux_a_batch = Bp * h->Fp;
        ep.aux_b = h->Kt[0]; ep.aux_b_batch = h->pack_batch[0];
        ep.aux_ld = h->Fp; ep.aux_scale = 1.0f / sqrtf((float)h->F);
        launch_gemm<T, EPI_DGRAD, 2>(h, KID_DGRAD, g, ep);
      } else {
        launch_gemm<T, EPI_DGRAD, 1>(h, KID_DGRAD, g, ep);
      }
      wgrad_after_dz<T>(h, nmem, l - 1);
    } else {
      g.N = h->Fp;
      ep.scale = 1.0f / sqrtf((float)h->F);
      ep.out_f32 = h->dH0; ep.f32_batch = (int64_t)h->Fp * Bp; ep.ld_f32 = (int32_t)Bp;
      launch_gemm<T, EPI_DGRAD0, 0>(h, KID_DGRAD0, g, ep);
    }
  }
  {
    LaunchScope ls(h, KID_FEATBWD);
    dim3 grid(cdiv(rows, 256), (unsigned)nmem);
    const float* X = h->X;
    hipLaunchKernelGGL(k_feat_bwd, grid, dim3(256), 0, h->stream, h->nd, rs, X, h->stab, theta,
                       (int64_t)h->Pf, h->scal, rows, h->dH0, (int64_t)h->Fp * Bp, (int32_t)Bp, h->gradf,
                       (int64_t)h->Pf);
  }
  wgrad_join(h);
}

// ---------------------------------------------------------------------------
// fragment-major weights for the row-panel kernel
// ---------------------------------------------------------------------------
static PackJobs pack_jobs(const bnf_handle* h, int* n_tiles) {
  PackJobs jb{};
  jb.n_layers = h->L; jb.W = h->W;
  int tiles = 0;
  for (int l = 0; l < h->L; ++l) {
    jb.off_kernel[l] = h->nd.off_kernel[l];
    jb.n_in[l] = (l == 0) ? h->F : h->W;
    jb.n_pad[l] = (l == 0) ? h->Fp : h->W;   // multiples of 64
    jb.tile0[l] = tiles;
    tiles += (jb.n_pad[l] / 64) * (h->W / 64);
    jb.wf[l] = h->Wf[l]; jb.wb[l] = h->Wb[l]; jb.batch[l] = h->pack_batch[l];
  }
  jb.tile0[h->L] = tiles;
  jb.fold0 = h->pp.fold0 ? 1 : 0; jb.F0n = h->F; jb.off_bias0 = h->nd.off_bias[0]; jb.off_ls0 = h->nd.off_ls[0];
  for (int l = 0; l < h->L; ++l) { jb.wf8[l] = h->Wf8[l]; jb.wb8[l] = h->Wb8[l]; }
  jb.batch8 = (int64_t)h->W * h->W;
  *n_tiles = tiles;
  return jb;
}
template <typename T>
static void run_pack_fragments(bnf_handle* h, const float* theta, int nmem) {
  LaunchScope ls(h, KID_PACK);
  int tiles = 0;
  const PackJobs jb = pack_jobs(h, &tiles);
  hipLaunchKernelGGL((k_pack_layers<T>), dim3((unsigned)tiles * (unsigned)nmem), dim3(256), 0, h->stream,
                     theta, (int64_t)h->Pf, jb, h->nd, h->scal);
}

// ---------------------------------------------------------------------------
// row-panel pipeline (bf16 / fp8, depth >= 2): pack fragments -> featurise -> k_panel_fwd_bwd ->
// featurise backward (where it is not fused) -> gemm_tn weight gradients
// ---------------------------------------------------------------------------
template <int WN, int RT, bool H0L, bool DEEP, int CH, int FP, bool F0, bool C8, bool FBW>
static void launch_panel_form(bnf_handle* h, const PanelArgs& pa) {
  constexpr int kLds = panel_lds_bytes(WN, RT, H0L, CH, FP);
  static_assert(kLds <= 160 * 1024, "LDS per workgroup");
  static std::atomic<uint64_t> attr_done{0};
  allow_lds(h->cfg.device, &k_panel_fwd_bwd<WN, RT, H0L, DEEP, CH, FP, F0, C8, FBW>, kLds, &attr_done);
  PanelArgs pa2 = pa;
  pa2.ablate = h->sw.ablate;
  const unsigned blocks = (unsigned)(pa.members * pa.panels);
  {
    EpiArgs tmp{};
    phase_prof_begin(h, KID_PANEL, blocks, &tmp);
    pa2.prof = tmp.prof;
  }
  {
    LaunchScope ls(h, KID_PANEL);
    hipLaunchKernelGGL((k_panel_fwd_bwd<WN, RT, H0L, DEEP, CH, FP, F0, C8, FBW>), dim3(blocks), dim3(512), kLds, h->stream, pa2);
  }
  phase_prof_end(h, KID_PANEL, blocks, 512);
}
// one launcher per row of kPanelForms (bnf_plan.h), in its order: h->form_index selects
using PanelLaunch = void (*)(bnf_handle*, const PanelArgs&);
#define BNF_PANEL_LAUNCH_ROW(WN, RT, H0L, DEEP, CH, FP, F0, C8, FBW) &launch_panel_form<WN, RT, H0L, DEEP, CH, FP, F0, C8, FBW>,
static const PanelLaunch kPanelLaunch[kNumPanelForms] = {BNF_PANEL_FORMS(BNF_PANEL_LAUNCH_ROW)};
#undef BNF_PANEL_LAUNCH_ROW
#define BNF_PANEL_ROWS_OK(WN, RT, H0L, DEEP, CH, FP, F0, C8, FBW) && panel_rows(WN, RT) == 32 * RT * (8 / WN)
static_assert(true BNF_PANEL_FORMS(BNF_PANEL_ROWS_OK), "PanelForm::panel_rows counts the kernel's rows per workgroup");
#undef BNF_PANEL_ROWS_OK

// fragments_packed: the caller has ALREADY written this step's weight fragments and scalar table (the VI sampler packs
// while it samples: k_vi_sample_pack) -- an argument of this call, not handle state, so that no early return or partial
// replay between the sampler and this call can leave a stale "already packed" behind
static void run_panel(bnf_handle* h, const float* theta, int nmem, const RowSrc& rs, float c,
                      const LossSink& sink, bool fragments_packed = false) {
  const int64_t Bp = h->Bp;
  if (!fragments_packed) run_pack_fragments<bf16_t>(h, theta, nmem);   // also fills the member scalar table the next kernels read
  {
    LaunchScope ls(h, KID_FEAT);
    dim3 grid(cdiv(h->B, kFeatRows) * (unsigned)nmem);
    const size_t lds = (size_t)kFeatRows * (h->Fp + 8) * 2;
    static std::atomic<uint64_t> attr_done{0};
    allow_lds(h->cfg.device, &k_featurize<bf16_t>, 160 * 1024, &attr_done);
    hipLaunchKernelGGL((k_featurize<bf16_t>), grid, dim3(kFeatRows), lds, h->stream, h->nd, rs, h->X, h->stab,
                       h->y, h->scal, h->B, (bf16_t*)h->H0, Bp * h->Fp, (bf16_t*)h->H0t,
                       (int64_t)h->Fp * Bp, (int32_t)Bp, h->ybat, Bp, (int32_t)nmem, (int32_t)(h->pp.fold0 ? 2 : 0), h->H0q);
  }
  PanelArgs pa{};
  pa.F = h->F; pa.Fp = h->Fp; pa.B = (int32_t)h->B; pa.members = nmem; pa.Wt = h->Wt;
  pa.theta = theta; pa.theta_stride = h->Pf; pa.scal = h->scal;
  const int L = h->L;
  pa.n_layers = L;
  for (int l = 0; l < L; ++l) {
    pa.off_bias[l] = h->nd.off_bias[l]; pa.off_ls[l] = h->nd.off_ls[l];
    pa.Wf[l] = (const bf16_t*)h->Wf[l]; pa.Wb[l] = (const bf16_t*)h->Wb[l];
    pa.Hout[l] = (bf16_t*)h->H[l]; pa.dZ[l] = (bf16_t*)h->dZ[l]; pa.park[l] = (bf16_t*)h->park[l];
  }
  pa.off_bias_out = h->nd.off_bias[L]; pa.off_ko = h->nd.off_kernel[L];
  pa.off_os = h->nd.off_os; pa.off_law = h->nd.off_law; pa.off_lns = h->nd.off_lns;
  pa.off_shape = h->nd.off_shape; pa.off_infl = h->nd.off_infl; pa.obs = h->nd.obs;
  pa.H0 = (const bf16_t*)h->H0t; pa.H0rm = (const bf16_t*)h->H0; pa.h0_batch = Bp * h->Fp;   // fragment-major / row-major
  pa.w0_batch = h->pack_batch[0]; pa.w1_batch = h->pack_batch[1];
  pa.act_batch = Bp * h->W;
  pa.dH0t = h->dH0; pa.dh0_batch = (int64_t)h->Fp * Bp; pa.ldt = (int32_t)Bp;
  pa.ybat = h->ybat; pa.row_batch = Bp; pa.out = h->out; pa.out_batch = Bp;
  pa.grad = h->gradf; pa.grad_stride = h->Pf;
  pa.loss = sink.loss; pa.loss_raw = sink.raw; pa.loss_stride = sink.stride; pa.S = h->S;
  pa.loss_scale = sink.scale; pa.lik_c = c; pa.st = sink.st;
  pa.q8 = h->pp.q8 ? 1 : 0; pa.qscale = h->qscale;
  pa.c8 = h->pp.c8 ? 1 : 0; pa.w8_batch = (int64_t)h->W * h->W;
  for (int l = 0; l < L; ++l) { pa.Wf8[l] = h->Wf8[l]; pa.Wb8[l] = h->Wb8[l]; }
  if (h->pp.h0l) {   // the fused featurisation backward (fbmeta null: no column table, k_feat_bwd below)
    pa.fbmeta = h->fbmeta; pa.off_lsa = h->nd.off_lsa; pa.n_groups = h->nd.n_groups; pa.n_inputs = h->nd.D;
    pa.fb_in_group = h->fb.in_group;
  }
  pa.panels = h->panels;
  kPanelLaunch[h->form_index](h, pa);
  if (h->form.separate_feat_bwd)
  {
    LaunchScope ls(h, KID_FEATBWD);
    dim3 grid(cdiv(h->B, 256), (unsigned)nmem);
    hipLaunchKernelGGL(k_feat_bwd, grid, dim3(256), 0, h->stream, h->nd, rs, h->X, h->stab, theta,
                       (int64_t)h->Pf, h->scal, h->B, h->dH0, (int64_t)h->Fp * Bp, (int32_t)Bp, h->gradf,
                       (int64_t)h->Pf);
  }
  run_wgrad(h, nmem);
}

// parameters as the forward / backward kernels read them (padded copy when the width is padded)
static const float* fw_theta(bnf_handle* h, const float* theta, int nmem) {
  if (!h->pad) return theta;
  hipLaunchKernelGGL(k_pad_params, dim3(cdiv(h->Pp, 256), (unsigned)nmem), dim3(256), 0, h->stream, theta,
                     (int64_t)h->P, h->theta_pad, h->Pp, h->pad_src);
  return h->theta_pad;
}
// gradient of the padded copy -> gradient in the parameter layout (before the optimiser kernel)
static void fold_grad(bnf_handle* h, int nmem) {
  if (!h->pad) return;
  hipLaunchKernelGGL(k_fold_grad, dim3(cdiv(h->P, 256), (unsigned)nmem), dim3(256), 0, h->stream, h->gradf,
                     h->Pp, h->fold_src, h->grad, (int64_t)h->P);
  (void)hipMemsetAsync(h->gradf, 0, (size_t)nmem * h->Pp * 4, h->stream);
}

static RowSrc make_rowsrc(const bnf_handle* h, int64_t epoch, int64_t step) {
  RowSrc rs{};
  rs.S = h->S;
  rs.seed = h->cfg.seed;
  rs.n_rows = h->N;
  rs.member_offset = h->cfg.member_offset;
  if (h->B >= h->N) {
    rs.mode = 0;
  } else if (h->cfg.mode == BNF_MODE_VI) {
    rs.mode = 2;
    rs.epoch = (uint64_t)step;  // VI: one shared random batch per optimisation step
    if (h->row_keys && h->perm && h->perm_epoch == step) {   // the reference's own batch of this step (ensure_row_perm drew it):
      rs.mode = 3;                                           // permutation(seed_step, N)[:B], the same rows for every member
      rs.table_ld = 0;
      rs.table = h->perm;
    }
  } else {
    rs.mode = 1;
    rs.epoch = (uint64_t)epoch;
    rs.pos0 = step * h->B;
    if (h->row_tab && epoch >= h->row_tab_e0 && epoch < h->row_tab_e0 + h->row_tab_epochs) {
      rs.mode = 3;
      rs.table_ld = (h->N / h->B) * h->B;
      rs.table = h->row_tab + (epoch - h->row_tab_e0) * (int64_t)h->cfg.members * rs.table_ld;
    } else if (h->row_keys && h->perm && h->perm_epoch == epoch) {   // (ensure_row_perm drew it)
      rs.mode = 3;
      rs.table_ld = h->N;
      rs.table = h->perm;
    }
  }
  return rs;
}

// jax.random.permutation(key, N) for every member, on the device (jax/_src/random.py `_shuffle`): `rounds` times
// { bits = random_bits(sub_key_r, (N,)); stable sort of the current order by bits }.  The sub keys are the
// caller's (bnf_row_keys); the bits are threefry2x32 over iota(N) split in halves (k_jax_perm_bits), the sort is
// rocPRIM's radix sort of (bits, row id) pairs -- LSD radix, stable -- one segment per member.
static size_t row_perm_bytes(int64_t members, int64_t n_rows) {   // without the sort's own scratch (a few MB)
  return 4 * (size_t)members * (size_t)n_rows * 4 + (size_t)(members + 1) * sizeof(unsigned);
}
// (VI handles: `epoch` is the optimisation STEP and there is ONE permutation per step, shared by every member --
// ensemble_vi's `jax.random.permutation(seed, arange(N))[:batch_size]`, inference.py:704-709)
static int perm_members(const bnf_handle* h) { return h->cfg.mode == BNF_MODE_VI ? 1 : h->cfg.members; }
static int ensure_row_perm(bnf_handle* h, int64_t epoch) {
  if (!h->row_keys || h->B >= h->N || epoch < h->row_keys_e0 || epoch >= h->row_keys_e0 + h->row_keys_epochs) return BNF_OK;
  if (h->row_tab && epoch >= h->row_tab_e0 && epoch < h->row_tab_e0 + h->row_tab_epochs) return BNF_OK;   // tables win
  if (h->perm_epoch == epoch) return BNF_OK;
  const int E = perm_members(h), R = h->row_key_rounds;
  const int64_t N = h->N, total = (int64_t)E * N;
  // (members x rows < 2^31 was checked by bnf_row_keys)
  const bool segmented = N <= (1 << 17);     // long segments: one device-wide sort per member instead
  if (!h->perm_ready) {
    // all or nothing: the handle's fields are set only when every buffer exists, so a failed allocation
    // leaves the handle as it was (the next epoch retries) instead of half-initialised
    uint32_t* bits[2] = {nullptr, nullptr}; int32_t* val[2] = {nullptr, nullptr};
    unsigned* seg = nullptr; void* tmp = nullptr; size_t tmp_bytes = 0;
    auto release = [&]() {
      for (int k = 0; k < 2; ++k) { if (bits[k]) (void)hipFree(bits[k]); if (val[k]) (void)hipFree(val[k]); }
      if (seg) (void)hipFree(seg);
      if (tmp) (void)hipFree(tmp);
    };
    hipError_t ae = hipSuccess;
    for (int k = 0; k < 2 && ae == hipSuccess; ++k) {
      ae = hipMalloc((void**)&bits[k], (size_t)total * 4);
      if (ae == hipSuccess) ae = hipMalloc((void**)&val[k], (size_t)total * 4);
    }
    if (ae == hipSuccess) ae = hipMalloc((void**)&seg, (size_t)(E + 1) * sizeof(unsigned));
    if (ae == hipSuccess) {
      std::vector<unsigned> off((size_t)E + 1);
      for (int e = 0; e <= E; ++e) off[(size_t)e] = (unsigned)((int64_t)e * N);
      ae = hipMemcpy(seg, off.data(), off.size() * sizeof(unsigned), hipMemcpyHostToDevice);
    }
    if (ae == hipSuccess) {
      size_t bytes = 0;
      if (segmented)
        ae = rocprim::segmented_radix_sort_pairs(nullptr, bytes, bits[0], bits[1], val[0], val[1], (unsigned)total,
                                                 (unsigned)E, seg, seg + 1, 0, 32, h->stream);
      else
        ae = rocprim::radix_sort_pairs(nullptr, bytes, bits[0], bits[1], val[0], val[1], (size_t)N, 0, 32, h->stream);
      tmp_bytes = std::max<size_t>(bytes, 16);
    }
    if (ae == hipSuccess) ae = hipMalloc(&tmp, tmp_bytes);
    if (ae != hipSuccess) {
      release();
      (void)hipGetLastError();
      return fail(BNF_ERR_HIP, "bnf_row_keys: work buffers for %d members x %lld rows (%.1f MB): %s", E, (long long)N,
                  (double)row_perm_bytes(E, N) / 1e6, hipGetErrorString(ae));
    }
    for (int k = 0; k < 2; ++k) { h->perm_bits[k] = bits[k]; h->perm_val[k] = val[k]; }
    h->perm_seg = seg; h->perm_tmp = tmp; h->perm_tmp_bytes = tmp_bytes;
    h->owned_bytes += 4 * (size_t)total * 4 + (size_t)(E + 1) * sizeof(unsigned) + tmp_bytes;
    h->perm_ready = true;
  }
  const uint32_t* keys = h->row_keys + ((epoch - h->row_keys_e0) * E) * (int64_t)R * 2;   // (members, rounds, 2)
  int cur = 0;
  for (int r = 0; r < R; ++r) {
    const unsigned half = (unsigned)((N + 1) / 2);
    hipLaunchKernelGGL(k_jax_perm_bits, dim3(cdiv(half, 256), (unsigned)E), dim3(256), 0, h->stream, keys, R, r,
                       (uint32_t)N, h->perm_bits[0], r == 0 ? h->perm_val[cur] : (int32_t*)nullptr);
    hipError_t se = hipSuccess;
    if (segmented) {
      size_t bytes = h->perm_tmp_bytes;
      se = rocprim::segmented_radix_sort_pairs(h->perm_tmp, bytes, h->perm_bits[0], h->perm_bits[1], h->perm_val[cur],
                                               h->perm_val[cur ^ 1], (unsigned)total, (unsigned)E, h->perm_seg,
                                               h->perm_seg + 1, 0, 32, h->stream);
    } else {
      for (int e = 0; e < E && se == hipSuccess; ++e) {
        size_t bytes = h->perm_tmp_bytes;
        se = rocprim::radix_sort_pairs(h->perm_tmp, bytes, h->perm_bits[0] + (int64_t)e * N, h->perm_bits[1] + (int64_t)e * N,
                                       h->perm_val[cur] + (int64_t)e * N, h->perm_val[cur ^ 1] + (int64_t)e * N, (size_t)N,
                                       0, 32, h->stream);
      }
    }
    if (se != hipSuccess) return fail(BNF_ERR_HIP, "radix sort: %s", hipGetErrorString(se));
    cur ^= 1;
  }
  h->perm = h->perm_val[cur];
  h->perm_epoch = epoch;
  HIPCHK(hipGetLastError());
  return BNF_OK;
}

// Adam's bias corrections at step t (the graph-replayed loop advances them on the device: k_step_advance)
static void adam_bias(int64_t t, float* bc1, float* bc2) {
  *bc1 = (float)(1.0 - std::pow(0.9, (double)t));
  *bc2 = (float)(1.0 - std::pow(0.999, (double)t));
}

// One MAP/MLE step.  apply=false: leave params untouched, grad holds the full
// gradient (likelihood + prior), loss_raw the step loss.
template <typename T>
static int step_map(bnf_handle* h, int64_t epoch, int64_t step, const LossSink& sink, bool apply) {
  if (const int prc = ensure_row_perm(h, epoch)) return prc;
  const RowSrc rs = make_rowsrc(h, epoch, step);
  const int E = h->cfg.members;
  const float c = (float)((double)h->N / (double)h->B);
  const float* thf = fw_theta(h, h->params, E);
  if (h->pp.panel) {
    run_panel(h, thf, E, rs, c, sink);
  } else {
    run_pack<T>(h, thf, E);
    run_forward<T>(h, thf, E, rs, h->X, h->stab, h->y, h->B, true);
    run_backward<T>(h, thf, E, rs, h->B, c, sink);
  }
  fold_grad(h, E);
  AdamArgs a{};
  a.theta = h->params; a.m = h->state; a.v = h->state + (int64_t)E * h->P; a.grad = h->grad;
  a.stride = h->P; a.P = h->P; a.off_shape = h->nd.off_shape;
  const int64_t t = h->adam_t + 1;
  a.lr = h->cfg.learning_rate;
  adam_bias(t, &a.bc1, &a.bc2);
  a.prior_weight = h->cfg.prior_weight;
  a.loss = sink.loss; a.loss_stride = sink.stride; a.loss_scale = sink.scale;
  a.apply = apply ? 1 : 0; a.loss_raw = sink.raw; a.st = sink.st;
  // the hidden-layer kernel whose gradient the next step stores (no split-K) is not cleared
  a.keep_lo = h->plan.n_keep ? h->plan.keep_lo[0] : 0;
  a.keep_hi = h->plan.n_keep ? h->plan.keep_hi[0] : 0;
  {
    LaunchScope ls(h, KID_ADAM);
    hipLaunchKernelGGL(k_adam_map, dim3(cdiv(cdiv(h->P, 4), 256 * BNF_ADAM_QUADS), (unsigned)E), dim3(256), 0, h->stream, a);
  }
  if (apply) h->adam_t = t;
  return BNF_OK;
}

// ---- VI sampler launch shapes -------------------------------------------------------------------------------
static ViSegs vi_segments_all(const bnf_handle* h) {
  ViSegs sg{};
  sg.n = 1; sg.lo[0] = 0; sg.hi[0] = h->P;
  return sg;
}
// what lies before, between and after the hidden Dense kernels (biases, scalars, the output layer)
static ViSegs vi_segments_between_kernels(const bnf_handle* h) {
  ViSegs sg{};
  int32_t at = 0;
  for (int l = 0; l < h->L; ++l) {
    sg.lo[sg.n] = at; sg.hi[sg.n] = h->nd.off_kernel[l]; ++sg.n;
    at = h->nd.off_kernel[l] + ((l == 0) ? h->F : h->W) * h->W;
  }
  sg.lo[sg.n] = at; sg.hi[sg.n] = h->P; ++sg.n;
  return sg;
}
static dim3 vi_sample_grid(const ViSegs& sg, int members) {
  int32_t longest = 1;
  for (int i = 0; i < sg.n; ++i) longest = std::max(longest, sg.hi[i] - sg.lo[i]);
  return dim3(cdiv(cdiv(longest, 4) + 1, 256), (unsigned)members, (unsigned)sg.n);   // + 1: a range may start mid-quad
}
// k_vi_sample_pack: row-panel pipeline on the parameter layout itself (no padded copy), every hidden kernel starting on
// a quad boundary of the noise stream (always, with spec.py's layout), BNF_VI_SAMPLE_PACK=0 restores the two kernels
static bool vi_sample_pack_ok(const bnf_handle* h) {
  if (!h->sw.vi_sample_pack || !h->pp.panel || h->pad || h->W % 64 != 0) return false;
  for (int l = 0; l < h->L; ++l)
    if ((h->nd.off_kernel[l] + kEpsQuadPhase) % 4 != 0) return false;
  return true;
}

static JaxNoise jax_noise_for_step(const bnf_handle* h) {
  JaxNoise jn{};
  if (!h->vi_keys) return jn;
  jn.keys = h->vi_keys; jn.leaf_off = h->leaf_off; jn.leaf_id = h->leaf_id;
  jn.n_leaves = h->n_leaves; jn.S = h->S; jn.members = h->cfg.members;
  jn.row = h->adam_t - h->vi_key_t0;
  return jn;
}

template <typename T>
static int step_vi(bnf_handle* h, int64_t step, float* loss, int64_t loss_stride, bool apply,
                   float* gmu_out, float* grho_out) {
  if (const int prc = ensure_row_perm(h, step)) return prc;
  const RowSrc rs = make_rowsrc(h, 0, step);
  const int E = h->cfg.members, S = h->S;
  float* mu = h->params;
  float* rho = h->params + (int64_t)E * h->P;
  const JaxNoise jn = jax_noise_for_step(h);
  if (jn.keys && (jn.row < 0 || jn.row >= h->vi_key_rows))
    return fail(BNF_ERR_STATE, "VI step %lld is outside the noise-key table (%lld rows from step %lld)",
                (long long)h->adam_t, (long long)h->vi_key_rows, (long long)h->vi_key_t0);
  // The hidden Dense kernels are sampled by the kernel that also packs them (k_vi_sample_pack) when the step draws the
  // device generator's noise and runs the row-panel pipeline on the parameter layout itself; k_vi_sample takes the rest
  // (or, otherwise, everything: k_pack_layers then packs from theta_c as in MAP).
  const bool fused = vi_sample_pack_ok(h) && !h->ext_eps && !jn.keys;
  {
    LaunchScope ls(h, KID_VISAMPLE);
    const ViSegs segs = fused ? vi_segments_between_kernels(h) : vi_segments_all(h);
    hipLaunchKernelGGL(k_vi_sample, vi_sample_grid(segs, E), dim3(256), 0, h->stream, mu, rho, h->P, S, h->cfg.seed,
                       h->cfg.member_offset, (uint64_t)step, (uint32_t)STREAM_VI_EPS, h->theta_c,
                       (int64_t)S * h->P, (int64_t)h->P, segs, h->ext_eps, jn);
    if (fused) {
      int tiles = 0;
      const PackJobs jb = pack_jobs(h, &tiles);
      ViSampleArgs sa{};
      sa.mu = mu; sa.rho = rho; sa.P = h->P; sa.S = S; sa.seed = h->cfg.seed; sa.member_offset = h->cfg.member_offset;
      sa.step = (uint64_t)step; sa.z = h->theta_c; sa.write_z = h->sw.vi_keep_z ? 1 : 0;
      hipLaunchKernelGGL((k_vi_sample_pack<bf16_t, BNF_VI_SP_THREADS>), dim3((unsigned)tiles * (unsigned)E),
                         dim3(BNF_VI_SP_THREADS), 0, h->stream, sa, jb,
                         h->nd, h->scal);
    }
  }
  const float kl = h->cfg.kl_weight;
  const float c = (float)((double)h->N / (double)h->B / (double)kl);
  LossSink sink{loss, loss_stride, kl / (float)S, nullptr};
  const float* thf = fw_theta(h, h->theta_c, h->Ev);
  if (h->pp.panel) {
    run_panel(h, thf, h->Ev, rs, c, sink, /*fragments_packed=*/fused);
  } else {
    run_pack<T>(h, thf, h->Ev);
    run_forward<T>(h, thf, h->Ev, rs, h->X, h->stab, h->y, h->B, true);
    run_backward<T>(h, thf, h->Ev, rs, h->B, c, sink);
  }
  fold_grad(h, h->Ev);
  ViAdamArgs a{};
  const int64_t EP = (int64_t)E * h->P;
  a.mu = mu; a.rho = rho;
  a.m_mu = h->state; a.v_mu = h->state + EP; a.m_rho = h->state + 2 * EP; a.v_rho = h->state + 3 * EP;
  a.grad = h->grad; a.P = h->P; a.S = S; a.off_shape = h->nd.off_shape;
  a.seed = h->cfg.seed; a.member_offset = h->cfg.member_offset; a.step = (uint64_t)step;
  const int64_t t = h->adam_t + 1;
  a.lr = h->cfg.learning_rate;
  adam_bias(t, &a.bc1, &a.bc2);
  a.kl_weight = kl; a.loss = loss; a.loss_stride = loss_stride; a.apply = apply ? 1 : 0;
  a.gmu_out = gmu_out; a.grho_out = grho_out; a.ext_eps = h->ext_eps; a.jn = jn;
  // the device generator's noise is made again in k_vi_adam (one Philox call per sample and quad); the caller's or the
  // reference's stream is recovered from the samples in theta_c
  a.z = (!h->ext_eps && !jn.keys && !h->sw.vi_keep_z) ? nullptr : h->theta_c;
  // the Dense kernels whose gradient the next step's weight-gradient kernel stores (split-K = 1) need no clearing
  a.n_keep = h->plan.n_keep;
  for (int r = 0; r < a.n_keep; ++r) { a.keep_lo[r] = h->plan.keep_lo[r]; a.keep_hi[r] = h->plan.keep_hi[r]; }
  {
    LaunchScope ls(h, KID_VIADAM);
    dim3 grid(cdiv(cdiv(h->P + kEpsQuadPhase, 4), 256), (unsigned)E);
    if (a.z) hipLaunchKernelGGL(k_vi_adam<false>, grid, dim3(256), 0, h->stream, a);
    else hipLaunchKernelGGL(k_vi_adam<true>, grid, dim3(256), 0, h->stream, a);
  }
  if (apply) h->adam_t = t;
  return BNF_OK;
}

// All the forecast unit (bnf_forecast.hip) sees of a handle, read from it at call time (bnf_host.h)
Forecast forecast_view(const bnf_handle* h) {
  if (!h) return Forecast{false, 0, 0, nullptr, nullptr};
  return Forecast{h->bound, h->cfg.device, h->cfg.obs_model, h->stream, h->qscratch};
}

// ---------------------------------------------------------------------------
// C ABI: the engine's share (the forecasts: bnf_forecast.hip; the posterior gather: bnf_comm.cpp)
// ---------------------------------------------------------------------------
extern "C" {

int bnf_abi_version(void) { return BNF_ABI_VERSION; }
const char* bnf_last_error(void) { return g_err; }

int bnf_create(const bnf_config* cfg, bnf_handle** out) {
  if (!cfg || !out) return fail(BNF_ERR_INVALID, "null argument");
  *out = nullptr;
  if (cfg->abi_version != BNF_ABI_VERSION)
    return fail(BNF_ERR_INVALID, "abi_version %d != %d", cfg->abi_version, BNF_ABI_VERSION);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(BNF_ERR_NO_DEVICE,
                "no HIP device visible: the BayesNF engine has no CPU fallback (needs gfx950)");
  if (cfg->device < 0 || cfg->device >= ndev)
    return fail(BNF_ERR_INVALID, "device %d out of range (0..%d)", cfg->device, ndev - 1);
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, cfg->device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(BNF_ERR_NO_DEVICE, "device %d is %s; this library is built for gfx950 only",
                cfg->device, prop.gcnArchName);
  if (cfg->dtype != BNF_DTYPE_F32 && cfg->dtype != BNF_DTYPE_BF16 && cfg->dtype != BNF_DTYPE_FP8 && cfg->dtype != BNF_DTYPE_F32S)
    return fail(BNF_ERR_INVALID, "dtype %d", cfg->dtype);
  if (cfg->obs_model != BNF_OBS_NORMAL && cfg->obs_model != BNF_OBS_NB && cfg->obs_model != BNF_OBS_ZINB)
    return fail(BNF_ERR_INVALID, "observation model %d", cfg->obs_model);
  if (cfg->mode != BNF_MODE_MAP && cfg->mode != BNF_MODE_VI) return fail(BNF_ERR_INVALID, "mode");
  if (cfg->n_inputs < 1 || cfg->n_inputs > BNF_MAX_INPUTS) return fail(BNF_ERR_INVALID, "n_inputs");
  if (cfg->depth < 1 || cfg->depth > BNF_MAX_LAYERS) return fail(BNF_ERR_INVALID, "depth");
  if (cfg->width < 1 || cfg->width > 8192) return fail(BNF_ERR_INVALID, "width %d (1..8192)", cfg->width);
  if (cfg->n_groups < 1 || cfg->n_groups > BNF_MAX_GROUPS) return fail(BNF_ERR_INVALID, "n_groups");
  if (cfg->n_freqs < 0 || cfg->n_freqs > BNF_MAX_FREQS) return fail(BNF_ERR_INVALID, "n_freqs");
  if (cfg->n_interact < 0 || cfg->n_interact > BNF_MAX_INTERACT)
    return fail(BNF_ERR_INVALID, "n_interact");
  if (cfg->n_features < 1 || cfg->n_params < 1) return fail(BNF_ERR_INVALID, "n_features/n_params");
  if (cfg->members < 1) return fail(BNF_ERR_INVALID, "members");
  if (cfg->n_rows < 1 || cfg->batch < 1 || cfg->batch > cfg->n_rows)
    return fail(BNF_ERR_INVALID, "batch %lld / n_rows %lld", (long long)cfg->batch,
                (long long)cfg->n_rows);
  if (cfg->n_rows > 0x7fffffffLL) return fail(BNF_ERR_INVALID, "n_rows too large");
  const int S = (cfg->mode == BNF_MODE_VI) ? cfg->vi_samples : 1;
  if (S < 1 || S > 64) return fail(BNF_ERR_INVALID, "vi_samples");
  if (cfg->mode == BNF_MODE_VI && !(cfg->kl_weight > 0.f)) return fail(BNF_ERR_INVALID, "kl_weight");
  if ((int64_t)cfg->members * S > 65535) return fail(BNF_ERR_INVALID, "members * vi_samples > 65535");

  bnf_handle* h = new bnf_handle();
  h->cfg = *cfg;
  h->bf16 = cfg->dtype == BNF_DTYPE_BF16 || cfg->dtype == BNF_DTYPE_FP8;   // (fp8: bf16 contractions, fp8 operand copies for the weight gradients)
  h->f32_split = cfg->dtype == BNF_DTYPE_F32S ? 2 : 0;
  h->es = h->bf16 ? 2 : 4;
  h->S = S;
  h->Ev = cfg->members * S;
  h->L = cfg->depth; h->Wt = cfg->width; h->W = (int)align_up(cfg->width, 64);
  h->pad = h->W != h->Wt;
  h->F = cfg->n_features; h->P = cfg->n_params;
  h->Fp = (int)align_up(h->F, 64);
  h->N = cfg->n_rows; h->B = cfg->batch;
  {
    // k_featurize stages kFeatRows rows of Fp (+ one 16-byte chunk) features in LDS
    const size_t feat_lds = (size_t)kFeatRows * (h->Fp + 16 / h->es) * h->es;
    if (feat_lds > 160 * 1024) {
      const int F = h->F, es = h->es;
      delete h;
      return fail(BNF_ERR_INVALID, "%d features need %zu bytes of LDS per featurisation workgroup (limit 163840): "
                  "at most %d features with this dtype", F, feat_lds, (160 * 1024 / (kFeatRows * es) - 16 / es) / 64 * 64);
    }
  }
  NetDev& nd = h->nd;
  memset(&nd, 0, sizeof(nd));
  nd.D = cfg->n_inputs; nd.F = h->F; nd.Fp = h->Fp; nd.W = h->W; nd.Wt = h->Wt; nd.depth = h->L; nd.P = h->P;
  nd.n_groups = cfg->n_groups; nd.n_freqs = cfg->n_freqs; nd.n_interact = cfg->n_interact;
  nd.obs = cfg->obs_model;
  for (int g = 0; g < cfg->n_groups; ++g) {
    nd.group_kind[g] = cfg->group_kind[g]; nd.group_arg[g] = cfg->group_arg[g];
    nd.group_ncols[g] = cfg->group_ncols[g]; nd.group_col0[g] = cfg->group_col0[g];
    nd.group_scale_off[g] = cfg->group_scale_off[g];
    if (cfg->group_col0[g] < 0 || cfg->group_col0[g] + cfg->group_ncols[g] > h->F ||
        cfg->group_scale_off[g] < 0 || cfg->group_scale_off[g] >= h->P) {
      delete h;
      return fail(BNF_ERR_INVALID, "feature group %d out of range", g);
    }
  }
  for (int d = 0; d < cfg->n_inputs; ++d) {
    nd.fdeg[d] = cfg->fourier_degree[d];
    nd.in_scale[d] = cfg->input_scale[d];
    if (cfg->fourier_degree[d] < 0 || cfg->fourier_degree[d] > 24) {
      delete h;
      return fail(BNF_ERR_INVALID, "fourier_degree[%d]", d);
    }
  }
  for (int k = 0; k < cfg->n_interact; ++k) {
    nd.interact[k][0] = cfg->interact[k][0];
    nd.interact[k][1] = cfg->interact[k][1];
  }
  nd.off_lns = cfg->off_log_noise_scale; nd.off_shape = cfg->off_shape; nd.off_infl = cfg->off_inflated;
  for (int l = 0; l <= h->L; ++l) {
    nd.off_bias[l] = cfg->off_bias[l];
    nd.off_kernel[l] = cfg->off_kernel[l];
  }
  h->Pf = h->P;
  if (h->pad) {
    // padded copies of the width-dependent leaves behind the P verbatim floats (k_pad_params)
    const int W = h->W, Wt = h->Wt;
    int64_t pos = h->P;
    h->fold_src_h.resize((size_t)h->P);
    for (int64_t i = 0; i < h->P; ++i) h->fold_src_h[(size_t)i] = (int32_t)i;
    auto leaf = [&](int32_t off_true, int rows_t, int cols_t, int rows_p, int cols_p) {
      const int32_t off_pad = (int32_t)pos;
      for (int r = 0; r < rows_p; ++r)
        for (int c = 0; c < cols_p; ++c) {
          const bool in = r < rows_t && c < cols_t;
          const int32_t src = in ? off_true + r * cols_t + c : -1;
          h->pad_src_h.push_back(src);
          if (in) h->fold_src_h[(size_t)src] = (int32_t)pos;
          ++pos;
        }
      return off_pad;
    };
    for (int l = 0; l < h->L; ++l) {
      nd.off_bias[l] = leaf(cfg->off_bias[l], 1, Wt, 1, W);
      const int rt = (l == 0) ? h->F : Wt, rp = (l == 0) ? h->F : W;
      nd.off_kernel[l] = leaf(cfg->off_kernel[l], rt, Wt, rp, W);
    }
    nd.off_kernel[h->L] = leaf(cfg->off_kernel[h->L], Wt, 1, W, 1);   // output kernel (W, 1)
    while (pos % 4) { h->pad_src_h.push_back(-1); ++pos; }
    h->Pp = pos; h->Pf = pos;
  }
  for (int l = 0; l < h->L; ++l) nd.off_ls[l] = cfg->off_layer_scale[l];
  nd.off_os = cfg->off_output_scale; nd.off_lsa = cfg->off_lsa; nd.off_law = cfg->off_act_weight;
  h->ft.n = cfg->n_freqs;
  for (int j = 0; j < cfg->n_freqs; ++j) {
    h->ft.f[j] = cfg->freq[j];
    h->ft.h[j] = cfg->harmonic[j];
  }
  for (int k = 0; k < KID_COUNT; ++k) { h->acc_ms[k] = 0; h->acc_calls[k] = 0; }
  h->sw = read_switches(getenv);   // the one read of the environment: every switch belongs to the handle from here on
  h->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  {
    bool input_group = false;
    for (int g = 0; g < cfg->n_groups; ++g) input_group = input_group || cfg->group_kind[g] == BNF_GROUP_INPUT;
    h->pp = make_pipeline_plan({cfg->dtype, cfg->forward_only != 0, h->L, h->W, h->F, h->Fp, cfg->pipeline, input_group}, h->sw);
    const PipelineRefusal refusal = h->pp.refusal;
    const int want = h->sw.pipeline_set ? h->sw.pipeline : cfg->pipeline;   // (the value the message names)
    if (refusal != PIPE_OK) delete h;
    switch (refusal) {
      case PIPE_OK: break;
      case PIPE_BAD_VALUE: return fail(BNF_ERR_INVALID, "pipeline %d (0 auto, 1 layers, 3 panel)", want);
      case PIPE_NO_PANEL:
        return fail(BNF_ERR_INVALID, "panel pipeline needs a bf16 training handle with depth >= 2, width 256/512/1024 and <= 128 features");
      case PIPE_FP8_NEEDS_PANEL:
        return fail(BNF_ERR_INVALID, "dtype fp8 (fp8 operand storage for the weight gradients) needs the row-panel pipeline: "
                    "depth >= 2, width 256 / 512 / 1024 after padding to 64, <= 128 padded features");
    }
  }
  // the plans, each from the ones before it (bnf_plan.h): pipeline -> Bp -> column table -> weight gradients -> panel form
  h->Bp = align_up(h->B, h->pp.bp_align);
  if (h->pp.fb_table)
    h->fb = make_featbwd_table(cfg->n_groups, cfg->group_kind, cfg->group_arg, cfg->group_ncols, cfg->group_col0,
                               cfg->group_scale_off, cfg->interact, h->Fp);
  h->plan = make_step_plan(plan_shape(h), h->sw, h->Ev, cfg->mode == BNF_MODE_VI);
  if (h->pp.panel) {
    h->form = make_panel_form(h->pp, h->plan, h->L, h->W, h->Fp);
    h->form_index = panel_form_index(h->form);
    h->panels = (int32_t)(h->Bp / h->form.panel_rows);
  }
  h->ws_bytes = carve(h, nullptr);
  *out = h;
  return BNF_OK;
}

void bnf_destroy(bnf_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->cfg.device);
  for (auto ev : h->event_pool) hipEventDestroy(ev);
  if (h->stream2) {
    (void)hipStreamSynchronize(h->stream2);
    (void)hipStreamDestroy(h->stream2);
  }
  for (int l = 0; l < BNF_MAX_LAYERS; ++l)
    if (h->ev_dz[l]) (void)hipEventDestroy(h->ev_dz[l]);
  if (h->ev_wg) (void)hipEventDestroy(h->ev_wg);
  if (h->graph_exec) (void)hipGraphExecDestroy(h->graph_exec);
  if (h->prof_buf) {
    if (h->prof_blocks > 0) {
      fprintf(stderr, "[phase clocks] %s: %d threads/workgroup, mean cycles per workgroup: total %.0f |",
              h->sw.phase_prof.c_str(), h->prof_threads, h->prof_gap[0] / h->prof_blocks);
      for (int k = 1; k < 16; ++k) fprintf(stderr, " m%d %.0f", k, h->prof_gap[k] / h->prof_blocks);
      fprintf(stderr, "\n");
    }
    (void)hipFree(h->prof_buf);
  }
  for (int k = 0; k < 2; ++k) {
    if (h->perm_bits[k]) (void)hipFree(h->perm_bits[k]);
    if (h->perm_val[k]) (void)hipFree(h->perm_val[k]);
  }
  if (h->perm_seg) (void)hipFree(h->perm_seg);
  if (h->perm_tmp) (void)hipFree(h->perm_tmp);
  delete h;
}

size_t bnf_workspace_bytes(const bnf_handle* h) { return h ? h->ws_bytes : 0; }
size_t bnf_owned_bytes(const bnf_handle* h) { return h ? h->owned_bytes : 0; }
size_t bnf_param_bytes(const bnf_handle* h) {
  if (!h) return 0;
  return (size_t)h->cfg.members * h->P * 4 * (h->cfg.mode == BNF_MODE_VI ? 2 : 1);
}
size_t bnf_state_bytes(const bnf_handle* h) {
  if (!h) return 0;
  return (size_t)h->cfg.members * h->P * 4 * (h->cfg.mode == BNF_MODE_VI ? 4 : 2);
}

int bnf_bind(bnf_handle* h, void* params, void* opt_state, void* workspace, const float* X,
             const float* y, void* stream) {
  if (!h || !workspace) return fail(BNF_ERR_INVALID, "null argument");
  if (!h->cfg.forward_only && (!params || !opt_state || !X))
    return fail(BNF_ERR_INVALID, "params / opt_state / X are required for a training handle");
  HIPCHK(hipSetDevice(h->cfg.device));
  h->stream = (hipStream_t)stream;
  h->params = (float*)params;
  h->state = (float*)opt_state;
  h->ws = (char*)workspace;
  h->X = X;
  h->y = y;
  carve(h, h->ws);
  if (h->cfg.mode != BNF_MODE_VI) h->theta_c = h->params;
  HIPCHK(hipMemsetAsync(h->ws, 0, h->ws_bytes, h->stream));
  if (h->state) HIPCHK(hipMemsetAsync(h->state, 0, bnf_state_bytes(h), h->stream));
  // which entries are Dense kernels (rank-2 leaves)
  std::vector<uint8_t> mm((size_t)h->P, 0);
  for (int l = 0; l <= h->L; ++l) {
    const int64_t n_in = (l == 0) ? h->F : h->Wt, n_out = (l == h->L) ? 1 : h->Wt;
    for (int64_t i = 0; i < n_in * n_out; ++i) mm[(size_t)h->cfg.off_kernel[l] + i] = 1;   // (parameter layout, not the padded copy's)
  }
  HIPCHK(hipMemcpyAsync(h->is_matrix, mm.data(), (size_t)h->P, hipMemcpyHostToDevice, h->stream));
  if (h->fbmeta)
    HIPCHK(hipMemcpyAsync(h->fbmeta, h->fb.meta.data(), h->fb.meta.size() * 4, hipMemcpyHostToDevice, h->stream));
  if (h->pad) {
    HIPCHK(hipMemcpyAsync(h->pad_src, h->pad_src_h.data(), h->pad_src_h.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->fold_src, h->fold_src_h.data(), h->fold_src_h.size() * 4, hipMemcpyHostToDevice, h->stream));
    if (h->gradf != h->grad) HIPCHK(hipMemsetAsync(h->gradf, 0, (size_t)h->Ev * h->Pp * 4, h->stream));
  }
  HIPCHK(hipStreamSynchronize(h->stream));  // mm is a stack-owned host buffer
  if (h->ft.n > 0 && X) {
    hipLaunchKernelGGL(k_seasonal_table, dim3(cdiv(h->N, 256)), dim3(256), 0, h->stream, X, h->N,
                       h->nd.D, h->ft, h->stab);
  }
  HIPCHK(hipGetLastError());
  if (!h->stream2 && !h->cfg.forward_only) {
    HIPCHK(hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking));
    for (int l = 0; l < h->L; ++l) HIPCHK(hipEventCreateWithFlags(&h->ev_dz[l], hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&h->ev_wg, hipEventDisableTiming));
  }
  h->bound = true;
  h->adam_t = 0;
  // key tables address rows by (adam_t - vi_key_t0): a re-bound handle starts again without them
  h->vi_keys = h->vi_draw_keys = nullptr; h->vi_key_rows = h->vi_draw_rows = 0; h->vi_key_t0 = 0;
  h->row_tab = nullptr; h->row_tab_epochs = 0;
  h->row_keys = nullptr; h->row_keys_epochs = 0; h->perm_epoch = -1;
  return BNF_OK;
}

int bnf_init_params(bnf_handle* h, float log_noise_init) {
  if (!h || !h->bound) return fail(BNF_ERR_STATE, "bnf_init_params before bnf_bind");
  if (h->cfg.forward_only || !h->params) return fail(BNF_ERR_STATE, "forward_only handle");
  HIPCHK(hipSetDevice(h->cfg.device));
  const int E = h->cfg.members;
  dim3 grid(cdiv(h->P, 256), (unsigned)E);
  hipLaunchKernelGGL(k_init_params, grid, dim3(256), 0, h->stream, h->params, h->P, h->is_matrix,
                     h->nd.off_lns, log_noise_init, h->cfg.seed, h->cfg.member_offset);
  if (h->cfg.mode == BNF_MODE_VI) {
    const int64_t n = (int64_t)E * h->P;
    // softplus^-1(0.3) = log(expm1(0.3)) = -1.0502256128148466
    hipLaunchKernelGGL(k_fill, dim3(cdiv(n, 256)), dim3(256), 0, h->stream, h->params + n, n,
                       -1.0502256128148466f);
  }
  HIPCHK(hipMemsetAsync(h->state, 0, bnf_state_bytes(h), h->stream));
  HIPCHK(hipGetLastError());
  h->adam_t = 0;
  // the VI noise-key tables are indexed from the step they were installed at: drop them (install after init)
  h->vi_keys = h->vi_draw_keys = nullptr; h->vi_key_rows = h->vi_draw_rows = 0; h->vi_key_t0 = 0;
  return BNF_OK;
}

int bnf_init_params_keys(bnf_handle* h, const uint32_t* leaf_keys, const int32_t* leaf_offsets, int32_t n_leaves,
                         float log_noise_init) {
  if (!h || !h->bound) return fail(BNF_ERR_STATE, "bnf_init_params_keys before bnf_bind");
  if (h->cfg.forward_only || !h->params) return fail(BNF_ERR_STATE, "forward_only handle");
  if (!leaf_keys || !leaf_offsets || n_leaves < 1 || n_leaves > 64) return fail(BNF_ERR_INVALID, "leaf_keys / leaf_offsets / n_leaves (1..64)");
  if (leaf_offsets[0] != 0 || leaf_offsets[n_leaves] != h->P) return fail(BNF_ERR_INVALID, "leaf_offsets must cover [0, P)");
  HIPCHK(hipSetDevice(h->cfg.device));
  LeafTable lt{};
  lt.n = n_leaves;
  for (int k = 0; k <= n_leaves; ++k) lt.off[k] = leaf_offsets[k];
  const int E = h->cfg.members;
  // bounds of the uniform: erf(-+2 / sqrt2) in f32, as jax.random.truncated_normal forms them
  const float ua = (float)std::erf((double)(-2.0f / 1.41421356237309504880f));
  const float ub = (float)std::erf((double)(2.0f / 1.41421356237309504880f));
  dim3 grid(cdiv(h->P, 256), (unsigned)E);
  hipLaunchKernelGGL(k_init_params_keys, grid, dim3(256), 0, h->stream, h->params, h->P, h->is_matrix, lt, leaf_keys,
                     h->nd.off_lns, log_noise_init, ua, ub);
  if (h->cfg.mode == BNF_MODE_VI) {
    const int64_t n = (int64_t)E * h->P;
    hipLaunchKernelGGL(k_fill, dim3(cdiv(n, 256)), dim3(256), 0, h->stream, h->params + n, n, -1.0502256128148466f);
  }
  HIPCHK(hipMemsetAsync(h->state, 0, bnf_state_bytes(h), h->stream));
  HIPCHK(hipGetLastError());
  h->adam_t = 0;
  h->vi_keys = h->vi_draw_keys = nullptr; h->vi_key_rows = h->vi_draw_rows = 0; h->vi_key_t0 = 0;
  return BNF_OK;
}

int bnf_train(bnf_handle* h, int64_t epoch0, int64_t num_epochs, float* losses) {
  if (!h || !h->bound) return fail(BNF_ERR_STATE, "bnf_train before bnf_bind");
  if (!losses || num_epochs < 0) return fail(BNF_ERR_INVALID, "losses / num_epochs");
  if (!h->y) return fail(BNF_ERR_STATE, "bnf_train needs a target bound");
  if (h->cfg.forward_only) return fail(BNF_ERR_STATE, "handle was created forward_only");
  HIPCHK(hipSetDevice(h->cfg.device));
  const int E = h->cfg.members;
  HIPCHK(hipMemsetAsync(losses, 0, (size_t)E * num_epochs * 4, h->stream));
  int rc = BNF_OK;
  if (h->cfg.mode == BNF_MODE_MAP) {
    const int64_t steps = h->N / h->B;  // ragged tail dropped (inference.py:583-589)
    // Launch-bound sizes (C1: W = 256, 8 members, 100 rows = 130 us per step of ~11
    // launches): a full-batch step is the same launch sequence every epoch, so ONE step can be
    // captured into a hipGraph and replayed; what changes per step (Adam bias corrections, loss
    // column) is read from StepState in device memory.  MEASURED (profiles/r02_c1_step_time.md):
    // replay 135 us vs 131 us eager -- the C loop already runs ahead of the GPU (11 launches x
    // ~3.5 us of host time), the step is bound by its ~11 DEPENDENT kernel boundaries on the device,
    // which a graph does not remove.  Hence opt-in; the lever for this regime is fewer kernels.
    const bool graph_ok = h->B >= h->N && !h->prof && !h->sw.overlap && h->stream2 && num_epochs >= 8 &&
                          h->sw.graph_mode == 1;   // opt-in (BNF_GRAPH=1): measured neutral, see below
    if (graph_ok) {
      StepState st0{};
      st0.t = h->adam_t + 1; st0.col = 0;
      adam_bias(st0.t, &st0.bc1, &st0.bc2);
      HIPCHK(hipMemcpyAsync(h->step_state, &st0, sizeof(st0), hipMemcpyHostToDevice, h->stream));
      HIPCHK(hipStreamSynchronize(h->stream));   // st0 lives on this stack frame
      if (!h->graph_exec || h->graph_cols != num_epochs || h->graph_losses != losses) {
        if (h->graph_exec) { (void)hipGraphExecDestroy(h->graph_exec); h->graph_exec = nullptr; }
        hipGraph_t graph = nullptr;
        // (the caller's stream may be the legacy default stream, which cannot capture: record the
        // step on the handle's own side stream; the graph is then launched on the caller's)
        hipStream_t user_stream = h->stream;
        h->stream = h->stream2;
        const hipError_t be = hipStreamBeginCapture(h->stream, hipStreamCaptureModeRelaxed);
        if (be != hipSuccess) {
          h->stream = user_stream;
            return fail(BNF_ERR_HIP, "hipStreamBeginCapture: %s", hipGetErrorString(be));
        }
        LossSink sink{losses, num_epochs, 1.0f, nullptr, h->step_state};
        rc = h->bf16 ? step_map<bf16_t>(h, epoch0, 0, sink, true) : step_map<float>(h, epoch0, 0, sink, true);
        h->adam_t -= 1;   // step_map counted the captured (not executed) step
        hipLaunchKernelGGL(k_step_advance, dim3(1), dim3(1), 0, h->stream, h->step_state);
        const hipError_t ce = hipStreamEndCapture(h->stream, &graph);
        h->stream = user_stream;
        if (rc != BNF_OK) return rc;
        if (ce != hipSuccess) return fail(BNF_ERR_HIP, "hipStreamEndCapture: %s", hipGetErrorString(ce));
        const hipError_t ie = hipGraphInstantiate(&h->graph_exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (ie != hipSuccess) return fail(BNF_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(ie));
        h->graph_cols = num_epochs; h->graph_losses = losses;
      }
      for (int64_t ep = 0; ep < num_epochs; ++ep) HIPCHK(hipGraphLaunch(h->graph_exec, h->stream));
      h->adam_t += num_epochs;
      HIPCHK(hipGetLastError());
      return BNF_OK;
    }
    for (int64_t ep = 0; ep < num_epochs && rc == BNF_OK; ++ep) {
      for (int64_t s = 0; s < steps && rc == BNF_OK; ++s) {
        LossSink sink{losses + ep, num_epochs, 1.0f / (float)steps, nullptr};
        rc = h->bf16 ? step_map<bf16_t>(h, epoch0 + ep, s, sink, true)
                     : step_map<float>(h, epoch0 + ep, s, sink, true);
      }
    }
  } else {
    for (int64_t st = 0; st < num_epochs && rc == BNF_OK; ++st) {
      rc = h->bf16 ? step_vi<bf16_t>(h, epoch0 + st, losses + st, num_epochs, true, nullptr, nullptr)
                   : step_vi<float>(h, epoch0 + st, losses + st, num_epochs, true, nullptr, nullptr);
    }
  }
  if (rc != BNF_OK) return rc;
  HIPCHK(hipGetLastError());
  return BNF_OK;
}

int bnf_vi_posterior_draws(bnf_handle* h, int32_t n_draws, float* out) {
  if (!h || !h->bound) return fail(BNF_ERR_STATE, "not bound");
  if (h->cfg.mode != BNF_MODE_VI) return fail(BNF_ERR_STATE, "not a VI handle");
  if (n_draws < 1 || n_draws > 65535 || !out) return fail(BNF_ERR_INVALID, "n_draws/out");
  HIPCHK(hipSetDevice(h->cfg.device));
  const int E = h->cfg.members;
  JaxNoise jn{};
  if (h->vi_draw_keys) {
    if (n_draws > h->vi_draw_rows) return fail(BNF_ERR_INVALID, "n_draws exceeds the draw-key table");
    jn.keys = h->vi_draw_keys; jn.leaf_off = h->leaf_off; jn.leaf_id = h->leaf_id;
    jn.n_leaves = h->n_leaves; jn.S = n_draws; jn.members = E; jn.row = 0;
  }
  // out[d][e][p]: member stride P, sample stride E*P
  const ViSegs segs = vi_segments_all(h);
  hipLaunchKernelGGL(k_vi_sample, vi_sample_grid(segs, E), dim3(256), 0, h->stream, h->params,
                     h->params + (int64_t)E * h->P, h->P, n_draws, h->cfg.seed,
                     h->cfg.member_offset, (uint64_t)0, (uint32_t)STREAM_VI_DRAW, out, (int64_t)h->P,
                     (int64_t)E * h->P, segs, (const float*)nullptr, jn);
  HIPCHK(hipGetLastError());
  return BNF_OK;
}

int bnf_forward(bnf_handle* h, const float* theta, int64_t n_members, const float* Xnew,
                int64_t n_rows, float* loc, float* aux) {
  if (!h || !h->bound) return fail(BNF_ERR_STATE, "bnf_forward before bnf_bind");
  if (!theta || !Xnew || !loc || n_members < 1 || n_rows < 1) return fail(BNF_ERR_INVALID, "argument");
  if (h->pp.panel) return fail(BNF_ERR_STATE, "bnf_forward needs a forward_only (or pipeline=1) handle");
  HIPCHK(hipSetDevice(h->cfg.device));
  const int64_t row_chunk = h->Bp, mem_chunk = h->Ev;
  RowSrc rs{};
  rs.mode = 0; rs.S = 1;
  for (int64_t m0 = 0; m0 < n_members; m0 += mem_chunk) {
    const int nm = (int)std::min<int64_t>(mem_chunk, n_members - m0);
    const float* th = fw_theta(h, theta + m0 * h->P, nm);
    if (h->bf16) run_pack<bf16_t>(h, th, nm); else run_pack<float>(h, th, nm);
    for (int64_t r0 = 0; r0 < n_rows; r0 += row_chunk) {
      const int64_t rows = std::min<int64_t>(row_chunk, n_rows - r0);
      const float* Xc = Xnew + r0 * h->nd.D;
      if (h->ft.n > 0)
        hipLaunchKernelGGL(k_seasonal_table, dim3(cdiv(rows, 256)), dim3(256), 0, h->stream, Xc, rows,
                           h->nd.D, h->ft, h->stab_pred);
      RowLossArgs a{};
      a.theta = th; a.theta_stride = h->Pf; a.B = rows;
      a.vacc = h->vacc; a.vacc_batch = h->Bp;
      a.out = loc + m0 * n_rows + r0; a.out_batch = n_rows;
      a.S = 1;
      if (h->bf16) run_forward<bf16_t>(h, th, nm, rs, Xc, h->stab_pred, nullptr, rows, false);
      else run_forward<float>(h, th, nm, rs, Xc, h->stab_pred, nullptr, rows, false);
      hipLaunchKernelGGL((k_row_loss<false>), dim3(cdiv(rows, 256), (unsigned)nm), dim3(256), 0,
                         h->stream, h->nd, a);
    }
  }
  if (aux)
    hipLaunchKernelGGL(k_forecast_aux, dim3(cdiv(n_members, 256)), dim3(256), 0, h->stream, theta,
                       (int64_t)h->P, (int32_t)n_members, h->nd.off_lns, h->nd.off_shape,
                       h->nd.off_infl, aux);
  HIPCHK(hipGetLastError());
  return BNF_OK;
}

// ---- held-out validation during a fit (bnf_validation.h) ----------------------------
int bnf_validation_check(bnf_handle* h, const double* member_ll, int64_t n_scored, int64_t epoch, int32_t check,
                         int32_t n_checks, double* curve, double* best_score, int64_t* best_epoch, int32_t* keep,
                         float* best_params) {
  if (const int rc = no_device()) return rc;
  if (!h || !h->bound) return fail(BNF_ERR_STATE, "not bound");
  if (h->cfg.forward_only || !h->params) return fail(BNF_ERR_STATE, "bnf_validation_check needs a training handle: this one is forward_only");
  if (h->cfg.mode != BNF_MODE_MAP) return fail(BNF_ERR_STATE, "bnf_validation_check needs a MAP / MLE handle");
  if (!member_ll || !curve || !best_score || !best_epoch || !keep || !best_params) return fail(BNF_ERR_INVALID, "argument");
  if (n_scored < 1 || n_checks < 1 || check < 0 || check >= n_checks)
    return fail(BNF_ERR_INVALID, "n_scored = %lld, check = %d of %d: n_scored and n_checks must be >= 1, check in [0, n_checks)",
                (long long)n_scored, (int)check, (int)n_checks);
  const int32_t M = h->cfg.members;
  const size_t row_bytes = (size_t)M * (size_t)h->P * sizeof(float);
  const char* a = (const char*)h->params;
  const char* b = (const char*)best_params;
  if (a < b + row_bytes && b < a + row_bytes) return fail(BNF_ERR_INVALID, "best_params overlaps the handle's parameters");
  HIPCHK(hipSetDevice(h->cfg.device));
  hipLaunchKernelGGL(k_validation_decide, dim3(cdiv(M, 256)), dim3(256), 0, h->stream, member_ll, n_scored, epoch, check,
                     n_checks, M, curve, best_score, best_epoch, keep);
  hipLaunchKernelGGL(k_validation_copy, dim3(cdiv(h->P, kValCopyTile), (unsigned)std::min<int32_t>(M, 65535)), dim3(256), 0,
                     h->stream, (const uint32_t*)h->params, (int64_t)h->P, M, (const int32_t*)keep, (uint32_t*)best_params);
  HIPCHK(hipGetLastError());
  return BNF_OK;
}

// ---- debug / introspection ---------------------------------------------------
int bnf_debug_loss_and_grad(bnf_handle* h, int64_t epoch, int64_t step, float* grads, float* loss) {
  if (!h || !h->bound) return fail(BNF_ERR_STATE, "not bound");
  if (h->cfg.forward_only) return fail(BNF_ERR_STATE, "forward_only handle");
  if (!grads || !loss) return fail(BNF_ERR_INVALID, "null");
  HIPCHK(hipSetDevice(h->cfg.device));
  const int E = h->cfg.members;
  int rc;
  if (h->cfg.mode == BNF_MODE_MAP) {
    HIPCHK(hipMemsetAsync(h->loss_raw, 0, (size_t)h->Ev * 4, h->stream));
    HIPCHK(hipMemsetAsync(loss, 0, (size_t)E * 4, h->stream));
    LossSink sink{loss, 1, 1.0f, nullptr};
    rc = h->bf16 ? step_map<bf16_t>(h, epoch, step, sink, false) : step_map<float>(h, epoch, step, sink, false);
    if (rc != BNF_OK) return rc;
    HIPCHK(hipMemcpyAsync(grads, h->grad, (size_t)E * h->P * 4, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemsetAsync(h->grad, 0, (size_t)h->Ev * h->P * 4, h->stream));
  } else {
    HIPCHK(hipMemsetAsync(loss, 0, (size_t)E * 4, h->stream));
    float* gmu = grads;
    float* grho = grads + (int64_t)E * h->P;
    rc = h->bf16 ? step_vi<bf16_t>(h, step, loss, 1, false, gmu, grho)
                 : step_vi<float>(h, step, loss, 1, false, gmu, grho);
    if (rc != BNF_OK) return rc;
    HIPCHK(hipMemsetAsync(h->grad, 0, (size_t)h->Ev * h->P * 4, h->stream));
  }
  HIPCHK(hipGetLastError());
  return BNF_OK;
}

int bnf_debug_row_index(bnf_handle* h, int64_t epoch, int64_t step, int32_t* out) {
  if (!h || !h->bound || !out) return fail(BNF_ERR_STATE, "not bound / null");
  HIPCHK(hipSetDevice(h->cfg.device));
  if (const int prc = ensure_row_perm(h, h->cfg.mode == BNF_MODE_VI ? step : epoch)) return prc;
  RowSrc rs = make_rowsrc(h, epoch, step);
  rs.S = 1;  // indexed by real member
  dim3 grid(cdiv(h->B, 256), (unsigned)h->cfg.members);
  hipLaunchKernelGGL(k_row_index, grid, dim3(256), 0, h->stream, rs, h->B, out);
  HIPCHK(hipGetLastError());
  return BNF_OK;
}

int bnf_vi_noise_keys(bnf_handle* h, const uint32_t* step_keys, int64_t n_steps, const uint32_t* draw_keys,
                      int64_t n_draws, const int32_t* leaf_offsets, int32_t n_leaves) {
  if (!h || !h->bound) return fail(BNF_ERR_STATE, "not bound");
  if (h->cfg.mode != BNF_MODE_VI) return fail(BNF_ERR_STATE, "not a VI handle");
  if (!step_keys && !draw_keys) {   // back to the engine's own generator
    h->vi_keys = h->vi_draw_keys = nullptr; h->vi_key_rows = h->vi_draw_rows = 0;
    return BNF_OK;
  }
  if (!leaf_offsets || n_leaves < 1 || n_leaves > 255 || leaf_offsets[0] != 0 || leaf_offsets[n_leaves] != h->P)
    return fail(BNF_ERR_INVALID, "leaf_offsets must be n_leaves + 1 increasing offsets from 0 to P (n_leaves <= 255)");
  if ((step_keys && n_steps < 1) || (draw_keys && n_draws < 1)) return fail(BNF_ERR_INVALID, "key-table rows");
  HIPCHK(hipSetDevice(h->cfg.device));
  std::vector<uint8_t> ids((size_t)h->P);
  for (int l = 0; l < n_leaves; ++l) {
    if (leaf_offsets[l + 1] <= leaf_offsets[l]) return fail(BNF_ERR_INVALID, "leaf_offsets not increasing");
    for (int32_t p = leaf_offsets[l]; p < leaf_offsets[l + 1]; ++p) ids[(size_t)p] = (uint8_t)l;
  }
  HIPCHK(hipMemcpyAsync(h->leaf_off, leaf_offsets, (size_t)(n_leaves + 1) * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->leaf_id, ids.data(), (size_t)h->P, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));   // ids is a stack-owned host buffer
  h->n_leaves = n_leaves;
  h->vi_keys = step_keys; h->vi_key_rows = step_keys ? n_steps : 0; h->vi_key_t0 = h->adam_t;
  h->vi_draw_keys = draw_keys; h->vi_draw_rows = draw_keys ? n_draws : 0;
  return BNF_OK;
}

int bnf_row_tables(bnf_handle* h, const int32_t* tables, int64_t epoch0, int64_t n_epochs) {
  if (!h || !h->bound) return fail(BNF_ERR_STATE, "not bound");
  if (h->cfg.mode != BNF_MODE_MAP) return fail(BNF_ERR_STATE, "row tables serve MAP / MLE epochs");
  if (!tables) { h->row_tab = nullptr; h->row_tab_epochs = 0; return BNF_OK; }
  if (n_epochs < 1 || epoch0 < 0) return fail(BNF_ERR_INVALID, "epoch0 / n_epochs");
  h->row_tab = tables; h->row_tab_e0 = epoch0; h->row_tab_epochs = n_epochs;
  return BNF_OK;
}

int bnf_row_keys(bnf_handle* h, const uint32_t* keys, int64_t epoch0, int64_t n_epochs, int32_t rounds) {
  if (!h || !h->bound) return fail(BNF_ERR_STATE, "not bound");
  h->perm_epoch = -1;
  if (!keys) { h->row_keys = nullptr; h->row_keys_epochs = 0; return BNF_OK; }
  if (n_epochs < 1 || epoch0 < 0 || rounds < 1 || rounds > 8) return fail(BNF_ERR_INVALID, "epoch0 / n_epochs / rounds");
  // jax: ceil(3 ln N / ln(2^32 - 1)) rounds -- anything else would be another permutation
  const int want = (int)std::ceil(3.0 * std::log((double)std::max<int64_t>(1, h->N)) / std::log(4294967295.0));
  if (rounds != want) return fail(BNF_ERR_INVALID, "rounds = %d, jax.random.permutation of %lld rows takes %d", rounds, (long long)h->N, want);
  // the sort addresses (member, row) pairs with 32-bit offsets; refuse here, where the caller can still choose the
  // index-free shuffle instead (bayesnf_amd/inference.py does, with a warning), not in the middle of bnf_train
  if ((int64_t)perm_members(h) * h->N > 0x7fffffffLL)
    return fail(BNF_ERR_INVALID, "bnf_row_keys: members x rows = %lld exceeds 2^31 - 1", (long long)((int64_t)perm_members(h) * h->N));
  h->row_keys = keys; h->row_keys_e0 = epoch0; h->row_keys_epochs = n_epochs; h->row_key_rounds = rounds;
  return BNF_OK;
}

int bnf_debug_vi_noise(bnf_handle* h, const float* eps) {
  if (!h || !h->bound) return fail(BNF_ERR_STATE, "not bound");
  if (h->cfg.mode != BNF_MODE_VI) return fail(BNF_ERR_STATE, "not a VI handle");
  h->ext_eps = eps;
  return BNF_OK;
}

int bnf_debug_vi_eps(bnf_handle* h, int64_t step, float* out) {
  if (!h || !h->bound || !out) return fail(BNF_ERR_STATE, "not bound / null");
  HIPCHK(hipSetDevice(h->cfg.device));
  dim3 grid(cdiv(h->P, 256), (unsigned)h->cfg.members, (unsigned)h->S);
  JaxNoise jn = jax_noise_for_step(h);
  if (jn.keys) {
    jn.row = step - h->vi_key_t0;
    if (jn.row < 0 || jn.row >= h->vi_key_rows) return fail(BNF_ERR_INVALID, "step outside the noise-key table");
  }
  hipLaunchKernelGGL(k_vi_eps_dump, grid, dim3(256), 0, h->stream, h->P, h->cfg.seed,
                     h->cfg.member_offset, (uint64_t)step, out, jn);
  HIPCHK(hipGetLastError());
  return BNF_OK;
}

int bnf_debug_activation(bnf_handle* h, int32_t what, float* out) {
  if (!h || !h->bound || !out) return fail(BNF_ERR_STATE, "not bound / null");
  HIPCHK(hipSetDevice(h->cfg.device));
  const int64_t B = h->B, Bp = h->Bp;
  const void* src = nullptr;
  int64_t batch = 0; int ld = 0, cols = 0, transposed = 0;
  if (what == 0) { src = h->H0; batch = Bp * h->Fp; ld = h->Fp; cols = h->F; }
  else if (what >= 1 && what < h->L) { src = h->H[what - 1]; batch = Bp * h->W; ld = h->W; cols = h->Wt; }
  else if (what >= 100 && what < 100 + h->L) {
    src = h->A[what - 100]; batch = (int64_t)h->W * (Bp + kAtPad); ld = (int)(Bp + kAtPad); cols = h->Wt; transposed = 1;
  } else if (what >= 300 && what < 300 + h->L) { src = h->dZ[what - 300]; batch = Bp * h->W; ld = h->W; cols = h->Wt; }
  else if (what == 200) {
    for (int e = 0; e < h->Ev; ++e)
      HIPCHK(hipMemcpyAsync(out + (int64_t)e * B, h->out + (int64_t)e * Bp, (size_t)B * 4,
                            hipMemcpyDeviceToDevice, h->stream));
    return BNF_OK;
  } else if (what == 400) {  // dH0 (Ev, B, F) f32, stored transposed
    dim3 grid(cdiv(B * h->F, 256), (unsigned)h->Ev);
    hipLaunchKernelGGL((k_to_f32<float>), grid, dim3(256), 0, h->stream, (const float*)h->dH0,
                       (int64_t)h->Fp * Bp, (int)Bp, B, h->F, out, 1);
    HIPCHK(hipGetLastError());
    return BNF_OK;
  } else {
    return fail(BNF_ERR_INVALID, "what=%d (the last hidden output is never stored)", what);
  }
  if (!src) return fail(BNF_ERR_STATE, "buffer not allocated on this handle");
  dim3 grid(cdiv(B * cols, 256), (unsigned)h->Ev);
  if (h->pp.q8 && h->pp.panel && what != 0) {   // the fp8 copies: H_l e4m3 un-scaled, dZ_l e5m2 x qscale[member]
    const bool dz = what >= 300;
    hipLaunchKernelGGL(k_q8_to_f32, grid, dim3(256), 0, h->stream, (const uint8_t*)src, batch, ld, B, cols, out,
                       dz ? 1 : 0, dz ? h->qscale : (const float*)nullptr);
    HIPCHK(hipGetLastError());
    return BNF_OK;
  }
  if (h->bf16)
    hipLaunchKernelGGL((k_to_f32<bf16_t>), grid, dim3(256), 0, h->stream, (const bf16_t*)src, batch, ld, B, cols, out, transposed);
  else
    hipLaunchKernelGGL((k_to_f32<float>), grid, dim3(256), 0, h->stream, (const float*)src, batch, ld, B, cols, out, transposed);
  HIPCHK(hipGetLastError());
  return BNF_OK;
}

int bnf_debug_gemm_nt(bnf_handle* h, const float* A, const float* Bt, int32_t M, int32_t N, int32_t K,
                      float* C) {
  if (!h || !A || !Bt || !C) return fail(BNF_ERR_INVALID, "null");
  if (M < 1 || N < 1 || K < 64 || K % 64 != 0) return fail(BNF_ERR_INVALID, "K must be a multiple of 64");
  HIPCHK(hipSetDevice(h->cfg.device));
  hipStream_t st = h->stream;
  void *dA = nullptr, *dB = nullptr;
  HIPCHK(hipMalloc(&dA, (size_t)M * K * h->es));
  HIPCHK(hipMalloc(&dB, (size_t)N * K * h->es));
  GemmArgs g{};
  g.A = dA; g.B = dB; g.a_ld = K; g.b_ld = K; g.a_batch = 0; g.b_batch = 0;
  g.M = M; g.N = N; g.K = K; g.splitk = 1; g.members = 1;
  EpiArgs ep{};
  ep.scale = 1.f; ep.out_f32 = C; ep.f32_batch = 0; ep.ld_f32 = N;
  if (h->bf16) {
    hipLaunchKernelGGL((k_from_f32<bf16_t>), dim3(cdiv((int64_t)M * K, 256)), dim3(256), 0, st, A, (int64_t)M, K, (bf16_t*)dA, K);
    hipLaunchKernelGGL((k_from_f32<bf16_t>), dim3(cdiv((int64_t)N * K, 256)), dim3(256), 0, st, Bt, (int64_t)N, K, (bf16_t*)dB, K);
    launch_gemm<bf16_t, EPI_PLAIN, 2>(h, KID_FWD, g, ep);
  } else {
    hipLaunchKernelGGL((k_from_f32<float>), dim3(cdiv((int64_t)M * K, 256)), dim3(256), 0, st, A, (int64_t)M, K, (float*)dA, K);
    hipLaunchKernelGGL((k_from_f32<float>), dim3(cdiv((int64_t)N * K, 256)), dim3(256), 0, st, Bt, (int64_t)N, K, (float*)dB, K);
    launch_gemm<float, EPI_PLAIN, 2>(h, KID_FWD, g, ep);
  }
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipFree(dA));
  HIPCHK(hipFree(dB));
  HIPCHK(hipGetLastError());
  return BNF_OK;
}

// the raw weight-gradient core on a caller's shape: the tile the production dispatch would pick for it
static int debug_tn_kind(const bnf_handle* h, const GemmArgs& g) {
  if (h->sw.big_tiles && g.M % 256 == 0 && g.N % 256 == 0 &&
      ((int64_t)g.members * (g.M / 256) * (g.N / 256) >= 128 || h->sw.big_tiles == 2))
    return (h->bf16 && h->sw.tn_ring && g.K % 64 == 0) ? WG_RING : WG_TN256;
  return WG_TN128;
}

int bnf_debug_gemm_tn(bnf_handle* h, const float* A, const float* B, int32_t R, int32_t M, int32_t N,
                      float* C) {
  if (!h || !A || !B || !C) return fail(BNF_ERR_INVALID, "null");
  if (R < 64 || R % 64 != 0 || M < 1 || N < 1 || M % 8 != 0 || N % 8 != 0)
    return fail(BNF_ERR_INVALID, "R must be a multiple of 64, M and N multiples of 8");
  HIPCHK(hipSetDevice(h->cfg.device));
  hipStream_t st = h->stream;
  void *dA = nullptr, *dB = nullptr;
  HIPCHK(hipMalloc(&dA, (size_t)R * M * h->es));
  HIPCHK(hipMalloc(&dB, (size_t)R * N * h->es));
  GemmArgs g{};
  g.A = dA; g.B = dB; g.a_ld = M; g.b_ld = N; g.M = M; g.N = N; g.K = R; g.splitk = 1; g.members = 1;
  EpiArgs ep{};
  ep.scale = 1.f; ep.out_f32 = C; ep.f32_batch = 0; ep.ld_f32 = N;
  if (h->pp.q8) {
    // A -> e4m3, B -> e5m2 (saturating, round to nearest even), then the fp8 kernel of the kind BNF_DEBUG_TN_KIND names
    // (0: the generic 128 x 128 tile, 2: ring -- M, N multiples of 256 --, 3: skinny -- M = 64, N a multiple of 512),
    // split-K BNF_DEBUG_TN_SPLITK: tests/test_gpu_fp8.py checks every kernel against the host product of the same
    // quantised operands.  (The two variables are arguments of THIS debug call, read when it is made -- not handle
    // state, so not in Switches.)
    const int kind = getenv("BNF_DEBUG_TN_KIND") ? atoi(getenv("BNF_DEBUG_TN_KIND")) : WG_TN128;
    g.splitk = getenv("BNF_DEBUG_TN_SPLITK") ? std::max(1, atoi(getenv("BNF_DEBUG_TN_SPLITK"))) : 1;
    if ((kind == WG_RING && (M % 256 || N % 256)) || (kind == WG_SKINNY && (M != 64 || N % 512)) ||
        (kind != WG_RING && kind != WG_SKINNY && kind != WG_TN128) || M % 16 || N % 16) {
      (void)hipFree(dA); (void)hipFree(dB);
      return fail(BNF_ERR_INVALID, "fp8 weight-gradient kernel kind %d does not take (M, N) = (%d, %d)", kind, M, N);
    }
    hipLaunchKernelGGL((k_from_f32_q8<false>), dim3(cdiv((int64_t)R * M, 256)), dim3(256), 0, st, A, (int64_t)R, M, (uint8_t*)dA, M);
    hipLaunchKernelGGL((k_from_f32_q8<true>), dim3(cdiv((int64_t)R * N, 256)), dim3(256), 0, st, B, (int64_t)R, N, (uint8_t*)dB, N);
    if (g.splitk > 1) HIPCHK(hipMemsetAsync(C, 0, (size_t)M * N * 4, st));
    if (kind == WG_SKINNY) launch_gemm_tn8<0>(h, KID_WGRAD0, g, ep, st, kind);
    else launch_gemm_tn8<1>(h, KID_WGRAD, g, ep, st, kind);
  } else if (h->bf16) {
    hipLaunchKernelGGL((k_from_f32<bf16_t>), dim3(cdiv((int64_t)R * M, 256)), dim3(256), 0, st, A, (int64_t)R, M, (bf16_t*)dA, M);
    hipLaunchKernelGGL((k_from_f32<bf16_t>), dim3(cdiv((int64_t)R * N, 256)), dim3(256), 0, st, B, (int64_t)R, N, (bf16_t*)dB, N);
    launch_gemm_tn<bf16_t, 2>(h, KID_WGRAD, g, ep, st, debug_tn_kind(h, g));
  } else {
    hipLaunchKernelGGL((k_from_f32<float>), dim3(cdiv((int64_t)R * M, 256)), dim3(256), 0, st, A, (int64_t)R, M, (float*)dA, M);
    hipLaunchKernelGGL((k_from_f32<float>), dim3(cdiv((int64_t)R * N, 256)), dim3(256), 0, st, B, (int64_t)R, N, (float*)dB, N);
    launch_gemm_tn<float, 2>(h, KID_WGRAD, g, ep, st, debug_tn_kind(h, g));
  }
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipFree(dA));
  HIPCHK(hipFree(dB));
  HIPCHK(hipGetLastError());
  return BNF_OK;
}

__global__ __launch_bounds__(1024) void k_poison_lds(uint32_t pattern, uint32_t* sink) {
  extern __shared__ uint32_t poison_sm[];
  for (int i = threadIdx.x; i < 160 * 1024 / 4; i += 1024) poison_sm[i] = pattern ^ ((uint32_t)i & 0xffu);   // (0x7fc00000: quiet NaNs with varying payloads)
  __syncthreads();
  if (sink && poison_sm[(threadIdx.x * 37) % (160 * 1024 / 4)] == 0x0badf00du) *sink = 1;   // keeps the stores alive
}

int bnf_debug_poison_lds(bnf_handle* h, uint32_t pattern) {
  if (!h || !h->bound) return fail(BNF_ERR_STATE, "not bound");
  HIPCHK(hipSetDevice(h->cfg.device));
  static std::atomic<uint64_t> attr_done{0};
  allow_lds(h->cfg.device, &k_poison_lds, 160 * 1024, &attr_done);
  // one workgroup per CU at a time (all of its LDS): several rounds so that every CU is visited
  hipLaunchKernelGGL(k_poison_lds, dim3((unsigned)h->num_cus * 4), dim3(1024), 160 * 1024, h->stream, pattern,
                     (uint32_t*)h->dbg_a);
  HIPCHK(hipGetLastError());
  return BNF_OK;
}

int bnf_profile_enable(bnf_handle* h, const char* kernel) {
  if (!h) return fail(BNF_ERR_INVALID, "null");
  if (h->prof) drain_timers(h);
  if (!kernel) {
    h->prof = 0;
    return BNF_OK;
  }
  uint32_t mask = 0;
  if (!strcmp(kernel, "*")) {
    mask = (1u << KID_COUNT) - 1u;
  } else {
    for (int k = 0; k < KID_COUNT; ++k)
      if (!strcmp(kernel, kKernelNames[k])) mask = 1u << k;
    if (!mask) return fail(BNF_ERR_INVALID, "unknown kernel '%s'", kernel);
  }
  for (int k = 0; k < KID_COUNT; ++k) { h->acc_ms[k] = 0; h->acc_calls[k] = 0; }
  h->prof = mask;
  return BNF_OK;
}

int bnf_profile_read(bnf_handle* h, int32_t* n, const char** names, double* avg_ms, int64_t* calls) {
  if (!h || !n) return fail(BNF_ERR_INVALID, "null");
  drain_timers(h);
  int used = 0;
  for (int k = 0; k < KID_COUNT && used < *n; ++k) {
    if (h->acc_calls[k] == 0) continue;
    names[used] = kKernelNames[k];
    avg_ms[used] = h->acc_ms[k] / (double)h->acc_calls[k];
    calls[used] = h->acc_calls[k];
    ++used;
  }
  *n = used;
  return BNF_OK;
}

double bnf_kernel_flops(const bnf_handle* h, const char* name) {
  if (!h || !name) return 0.0;
  const double Ev = h->Ev, B = (double)h->B, W = h->Wt, F = h->F;
  // featbwd_in_wgrad: the panel kernel no longer contracts dH0 (below); the layer-0 weight gradient contracts the
  // 2 x n_fourier rows of G (bf16 hi + lo) beside the F feature rows
  if (!strcmp(name, "gemm_wgrad_l0") && h->plan.featbwd_in_wgrad) return 2.0 * Ev * B * (F + 2.0 * h->fb.n_fourier) * W;
  if (!strcmp(name, "gemm_fwd_l0") || !strcmp(name, "gemm_dgrad0") || !strcmp(name, "gemm_wgrad_l0"))
    return 2.0 * Ev * B * F * W;
  if (!strcmp(name, "gemm_wgrad") && h->plan.merged)   // one launch for the layers 1 .. L-1
    return 2.0 * Ev * B * W * W * (h->L - 1);
  if (!strcmp(name, "gemm_fwd") || !strcmp(name, "gemm_dgrad") || !strcmp(name, "gemm_wgrad"))
    return 2.0 * Ev * B * W * W;
  if (!strcmp(name, "gemm_fwd_last"))   // last hidden layer + output-layer dot
    return 2.0 * Ev * B * (h->L > 1 ? W : F) * W + 2.0 * Ev * B * W;
  if (!strcmp(name, "panel_fwd_bwd"))  // forward + backward-data contractions of every layer + output layer
    return 4.0 * Ev * B * (F * W + (h->L - 1) * W * W) + 2.0 * Ev * B * W - (h->plan.featbwd_in_wgrad ? 2.0 * Ev * B * F * W : 0.0);
  return 0.0;
}

}  // extern "C"
