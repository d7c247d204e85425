// bnf_plan.h -- what a handle decides ONCE, at bnf_create: the environment switches (Switches), the forward / backward
// pipeline (PipelinePlan), the column table of the fused featurisation backward (FeatBwdTable), the weight-gradient side
// of the training step (StepPlan) and the instantiation of the row-panel kernel (PanelForm), in that order: each reads
// the ones before it.  Host only, plain C++17, no HIP headers: tests/test_step_plan_host.py and
// tests/test_pipeline_plan_host.py compile this file with g++ and assert the plans without a GPU.
//
// The step functions of bnf_api.hip execute h->plan; nothing on the step path reads the environment or derives a
// kernel choice again.  The launcher and the optimiser therefore cannot disagree about which gradient ranges the next
// step's kernels STORE (split-K 1) and which they accumulate into, whatever happens to the environment in between.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/bnf.h"

namespace bnf {

// ---- switches ------------------------------------------------------------------------------------------------
// Every BNF_* variable the library reads for a handle (INTEGRATION.md lists their meaning).  The only other reads are
// BNF_DEBUG_TN_KIND / BNF_DEBUG_TN_SPLITK, arguments of the one debug call bnf_debug_gemm_tn.
struct Switches {
  int ablate = 0;                // BNF_ABLATE (perf experiments, ABLATE builds)
  int big_tiles = 1;             // BNF_BIG_TILES: 0 = 128 x 128 tiles everywhere, 1 = auto, 2 = 256 x 256 wherever the shape divides
  int skinny = 1;                // BNF_WGRAD_SKINNY=0: layer-0 weight gradient through the 128 x 128 tiles
  int tn_ring = 1;               // BNF_TN_RING=0: the two-stage K loop for the 256 x 256 weight-gradient tile
  int graph_mode = 0;            // BNF_GRAPH=1: replay full-batch MAP steps from a hipGraph
  bool adam_clear_all = false;   // BNF_ADAM_CLEAR_ALL (presence): no kept gradient range
  bool vi_sample_pack = true;    // BNF_VI_SAMPLE_PACK=0: k_vi_sample + k_pack_layers instead of the fused sampler
  bool vi_keep_z = false;        // BNF_VI_KEEP_Z=1: every sample is written to theta_c
  bool pipeline_set = false;     // BNF_PIPELINE overrides bnf_config.pipeline when set (0 is a value: auto)
  int pipeline = 0;
  bool fp8_contract = true;      // BNF_FP8_CONTRACT=0: bf16 W x W contractions in the fp8 handle
  bool panel_fold0 = true;       // BNF_PANEL_FOLD0=0
  bool panel_featbwd = true;     // BNF_PANEL_FEATBWD=0
  bool featbwd_wgrad = true;     // BNF_FEATBWD_WGRAD=0: the fused featurisation backward stays in the panel kernel
  bool panel_no_h0l = false;     // BNF_PANEL_NO_H0L (presence)
  bool overlap = false;          // BNF_OVERLAP=1: weight gradients on a side stream
  bool wgrad_no_multi = false;   // BNF_WGRAD_NO_MULTI (presence): one launch per W x W layer
  bool wgrad_order_fwd = false;  // BNF_WGRAD_ORDER=fwd: layer 0 first
  int ring_splitk = 0;           // BNF_RING_SPLITK: split-K of the un-split ring plan (0 = unset)
  std::string phase_prof;        // BNF_PHASE_PROF: kernel name ("" = unset)
};

// lookup: const char*(const char*), getenv in production
template <typename Lookup>
inline Switches read_switches(Lookup&& lookup) {
  Switches s;
  const char* v;
  if ((v = lookup("BNF_ABLATE"))) s.ablate = atoi(v);
  if ((v = lookup("BNF_BIG_TILES"))) s.big_tiles = atoi(v);
  if ((v = lookup("BNF_WGRAD_SKINNY"))) s.skinny = atoi(v);
  if ((v = lookup("BNF_TN_RING"))) s.tn_ring = atoi(v);
  if ((v = lookup("BNF_GRAPH"))) s.graph_mode = atoi(v);
  s.adam_clear_all = lookup("BNF_ADAM_CLEAR_ALL") != nullptr;
  if ((v = lookup("BNF_VI_SAMPLE_PACK"))) s.vi_sample_pack = atoi(v) != 0;
  if ((v = lookup("BNF_VI_KEEP_Z"))) s.vi_keep_z = atoi(v) != 0;
  if ((v = lookup("BNF_PIPELINE"))) { s.pipeline_set = true; s.pipeline = atoi(v); }
  if ((v = lookup("BNF_FP8_CONTRACT"))) s.fp8_contract = atoi(v) != 0;
  if ((v = lookup("BNF_PANEL_FOLD0"))) s.panel_fold0 = atoi(v) != 0;
  if ((v = lookup("BNF_PANEL_FEATBWD"))) s.panel_featbwd = atoi(v) != 0;
  if ((v = lookup("BNF_FEATBWD_WGRAD"))) s.featbwd_wgrad = atoi(v) != 0;
  s.panel_no_h0l = lookup("BNF_PANEL_NO_H0L") != nullptr;
  if ((v = lookup("BNF_OVERLAP"))) s.overlap = atoi(v) != 0;
  s.wgrad_no_multi = lookup("BNF_WGRAD_NO_MULTI") != nullptr;
  if ((v = lookup("BNF_WGRAD_ORDER"))) s.wgrad_order_fwd = !strcmp(v, "fwd");
  if ((v = lookup("BNF_RING_SPLITK"))) s.ring_splitk = std::max(1, atoi(v));
  if ((v = lookup("BNF_PHASE_PROF"))) s.phase_prof = v;
  return s;
}

// tile sizes the plan counts with (bnf_api.hip asserts them equal to kBM, kBN and kSkRows of bnf_gemm.h)
constexpr int kPlanBM = 128, kPlanBN = 128, kPlanSkRows = 32;
// Fourier feature columns the layer-0 weight-gradient kernel can take the featurisation backward for: each becomes two
// extra operand rows (bf16 hi + lo of a product of two features) beside the 64 feature rows (kSkFbCols of bnf_gemm.h)
constexpr int kPlanFbCols = 32;

// ---- the pipeline plan ---------------------------------------------------------------------------------------
// Row-panel kernel (bnf_panel.h: rows stay in LDS / registers through ALL layers) or the layer kernels.
struct PipelineShape {
  int dtype;             // BNF_DTYPE_*
  bool forward_only;
  int L, W, F, Fp;       // hidden layers, width the kernels run at (the model's, padded to 64), features, padded features
  int pipeline;          // bnf_config.pipeline: 0 auto, 1 layer kernels with every activation materialised, 3 row-panel kernel
  bool input_group;      // the model has a raw-input feature group (the fused featurisation backward scales by its leaf)
};
enum PipelineRefusal { PIPE_OK = 0, PIPE_BAD_VALUE, PIPE_NO_PANEL, PIPE_FP8_NEEDS_PANEL };   // bnf_create: BNF_ERR_INVALID
struct PipelinePlan {
  PipelineRefusal refusal;
  bool panel;           // row-panel forward + backward kernel: a bf16 / fp8 training handle, depth >= 2, W = 256 / 512 / 1024, Fp <= 128
  bool fuse_last;       // layer kernels: last layer + likelihood + its backward in one kernel (EPI_LAST)
  bool recompute_a0;    // layer kernels: layer-0 pre-activation recomputed in the backward pass (DGRAD TAG 2)
  bool h0l;             // panel kernel: the feature panel staged in LDS (no fragment-major copy H0t)
  bool fold0;           // panel kernel's F0 forms: layer-0 scale / bias folded into its contraction
  bool q8;              // BNF_DTYPE_FP8: bf16 contractions + fp8 operand copies for the weight-gradient kernels (bnf_gemm8.h)
  bool c8;              // ... and the W x W contractions of the folded row-panel forms on the fp8 MFMA (PanelArgs.c8)
  bool fb_table;        // the column table of the fused featurisation backward is built (make_featbwd_table)
  int bp_align;         // the batch is padded to a multiple of this many rows
};
// widths the one-kernel last layer has an instantiation for (launch_fwd_last_obs of bnf_api.hip)
constexpr bool fused_last_width(int W, bool bf16) { return W == 64 || W == 128 || W == 256 || (W == 512 && bf16); }
inline PipelinePlan make_pipeline_plan(const PipelineShape& s, const Switches& sw) {
  PipelinePlan p{};
  const bool bf16 = s.dtype == BNF_DTYPE_BF16 || s.dtype == BNF_DTYPE_FP8;
  p.q8 = s.dtype == BNF_DTYPE_FP8;
  p.bp_align = 128;
  const int want = sw.pipeline_set ? sw.pipeline : s.pipeline;   // BNF_PIPELINE overrides the config
  if (want != 0 && want != 1 && want != 3) { p.refusal = PIPE_BAD_VALUE; return p; }
  const bool can_panel = !s.forward_only && bf16 && s.L >= 2 && (s.W == 256 || s.W == 512 || s.W == 1024) && s.Fp <= 128;
  if (want == 3 && !can_panel) { p.refusal = PIPE_NO_PANEL; return p; }
  p.panel = can_panel && want != 1;   // the default where it applies (C2: 2.71 -> 2.27 ms/step)
  if (p.q8 && !p.panel && !s.forward_only) { p.refusal = PIPE_FP8_NEEDS_PANEL; return p; }
  if (p.panel) p.bp_align = 256;
  // pipeline 0 (auto): the one-kernel last layer where the width allows; 1: every activation materialised (validation)
  const bool layers_auto = !s.forward_only && !p.panel && want == 0;
  p.fuse_last = layers_auto && fused_last_width(s.W, bf16);
  // its contraction depth is Fp <= 128: cheaper to redo than to write + gather A_0^T
  p.recompute_a0 = layers_auto && s.L >= 2 && s.Fp <= 128;
  // the H0L panel forms exist for these shapes; F0 needs two spare feature columns (the ones column and its partner)
  const bool h0l_shape = ((s.W == 512 || s.W == 1024) && s.Fp == 64) || (s.W == 256 && (s.Fp == 64 || s.Fp == 128));
  p.h0l = p.panel && h0l_shape && !sw.panel_no_h0l;
  p.fold0 = p.h0l && s.F + 2 <= s.Fp && sw.panel_fold0;
  // (the fp8-contraction kernels are instantiated for the folded forms; BNF_FP8_CONTRACT=0: the fp8 copies only)
  p.c8 = p.q8 && p.fold0 && sw.fp8_contract;
  p.fb_table = p.h0l && sw.panel_featbwd && s.input_group;
  return p;
}

// ---- the column table of the fused featurisation backward ----------------------------------------------------
// What each feature column contributes to the gradients of the feature scales and the raw-input scale: read by the H0L
// panel kernel (PanelArgs::fbmeta, bnf_panel.h) and by gemm_tn_skinny_featbwd (FeatBwdArgs::fbmeta, bnf_gemm.h).
//   words 4 c .. 4 c + 2 of column c: kind | group << 8 | d1 << 16 | d2 << 24;  partner column | input column << 8;  coefficient
//   words 4 Fp + g: the scale leaf of group g;  words 4 Fp + BNF_MAX_GROUPS + q (Fp = 64): slot q = f | p << 8 | u << 16 |
//   1 << 24 of the q-th Fourier column, the layer-0 weight gradient's extra operand rows (0: no such column)
constexpr int kFbNone = 0, kFbInput = 1, kFbFourier = 2, kFbInter = 3;   // column kinds
struct FeatBwdTable {
  std::vector<int32_t> meta;   // empty: no table (PipelinePlan::fb_table is off)
  int in_group = -1;           // the raw-input group
  int n_fourier = 0;           // Fourier feature columns of the model (StepPlan::featbwd_in_wgrad takes at most kPlanFbCols)
};
inline FeatBwdTable make_featbwd_table(int n_groups, const int32_t* kind, const int32_t* arg, const int32_t* ncols,
                                       const int32_t* col0, const int32_t* scale_off, const int32_t (*interact)[2], int Fp) {
  FeatBwdTable t;
  for (int g = 0; g < n_groups; ++g)
    if (kind[g] == BNF_GROUP_INPUT) t.in_group = g;
  if (t.in_group < 0) return t;
  std::vector<int32_t>& m = t.meta;
  m.assign(Fp * 4 + BNF_MAX_GROUPS + kPlanFbCols, 0);
  auto put = [&](int col, int knd, int g, int d1, int d2, int partner, int ucol, float coef) {
    m[4 * col] = knd | (g << 8) | (d1 << 16) | (d2 << 24);
    m[4 * col + 1] = partner | (ucol << 8);
    memcpy(&m[4 * col + 2], &coef, 4);
  };
  for (int c = 0; c < Fp; ++c) put(c, kFbNone, 0xff, 0xff, 0xff, 0, 0, 0.f);
  const int cin = col0[t.in_group];
  for (int g = 0; g < n_groups; ++g) {
    const int c0 = col0[g], nc = ncols[g];
    m[4 * Fp + g] = scale_off[g];
    switch (kind[g]) {
      case BNF_GROUP_INPUT:
        for (int d = 0; d < nc; ++d) put(c0 + d, kFbInput, g, d, 0xff, 0, 0, 0.f);
        break;
      case BNF_GROUP_FOURIER: {
        const int deg = nc / 2, d = arg[g];
        for (int k = 0; k < deg; ++k) {
          const float w = 6.28318530717958647692f * (float)(1u << k);
          put(c0 + k, kFbFourier, g, d, 0xff, c0 + deg + k, cin + d, -w);
          put(c0 + deg + k, kFbFourier, g, d, 0xff, c0 + k, cin + d, w);
        }
        break;
      }
      case BNF_GROUP_SEASONAL:
        for (int j = 0; j < nc; ++j) put(c0 + j, kFbNone, g, 0xff, 0xff, 0, 0, 0.f);
        break;
      default:
        for (int k = 0; k < nc; ++k) put(c0 + k, kFbInter, g, interact[k][0], interact[k][1], 0, 0, 0.f);
    }
  }
  for (int c = 0; c < Fp; ++c) {
    if ((m[4 * c] & 0xff) != kFbFourier) continue;
    if (t.n_fourier < kPlanFbCols && Fp == 64)
      m[4 * Fp + BNF_MAX_GROUPS + t.n_fourier] = c | ((m[4 * c + 1] & 0xffff) << 8) | (1 << 24);
    ++t.n_fourier;
  }
  return t;
}

// ---- the weight-gradient plan --------------------------------------------------------------------------------
enum { WG_TN128 = 0, WG_TN256 = 1, WG_RING = 2, WG_SKINNY = 3 };   // weight-gradient kernels

// what the plan depends on, and nothing else
struct PlanShape {
  bool bf16;          // bf16 (or fp8) storage
  int L, W, F, Fp;    // hidden layers, width the kernels run at, features, padded features
  int64_t Bp;         // padded batch rows: the contraction depth of the weight gradients
  int num_cus;
  bool panel;         // row-panel pipeline
  bool pad;           // model width < W: gradients pass through a padded copy, nothing is kept
  int32_t off_kernel[BNF_MAX_LAYERS];   // offsets of the hidden Dense kernels in the parameter vector
  bool fp8;           // the fp8 handle (dZ_0 leaves the panel kernel as e5m2)
  bool featbwd_fused; // the panel kernel's fused featurisation backward is on (its column table exists)
  int n_fourier;      // Fourier feature columns of the model
};

// Which kernel computes layer l's weight gradient and with what split-K (1: the kernel STORES dK_l, > 1: f32 atomics).
struct WgradPlan { int kind, splitk; };
inline WgradPlan wgrad_plan(const PlanShape& ps, const Switches& sw, int nmem, int l) {
  const int M = (l == 0) ? ps.F : ps.W, N = ps.W, a_ld = (l == 0) ? ps.Fp : ps.W;
  const int64_t K = ps.Bp;
  const int tiles = ((M + kPlanBM - 1) / kPlanBM) * ((N + kPlanBN - 1) / kPlanBN);
  const int nk = (int)(K / (ps.bf16 ? 64 : 32));
  const int sk = (1024 + nmem * tiles - 1) / (nmem * tiles);
  const int base_sk = std::max(1, std::min(sk, std::max(1, nk / 4)));
  if (ps.bf16 && l == 0 && sw.skinny && a_ld == 64 && N % 512 == 0 && K % 64 == 0) {
    // layer 0 as a 64 x 512 row stream, one workgroup per CU (144 KiB of LDS): the K split with the shortest
    // schedule -- rounds of the chip x rows per workgroup (C3/8, 80 members: 3 splits = 240 workgroups in one round
    // instead of 4 = 320 in two, the second a quarter full); ties go to the fewest splits (fewest atomics)
    const int64_t base = (int64_t)nmem * (N / 512);
    const int nks = (int)(K / kPlanSkRows);
    const int max_s = (int)std::max<int64_t>(1, std::min<int64_t>((ps.num_cus + base - 1) / base, std::max(1, nks / 8)));
    int best = 1;
    double best_cost = 1e30;
    for (int sp = 1; sp <= max_s; ++sp) {
      const int64_t rounds = (base * sp + ps.num_cus - 1) / ps.num_cus;
      const double cost = (double)rounds * (double)((nks + sp - 1) / sp);
      if (cost < best_cost * 0.98) { best_cost = cost; best = sp; }
    }
    return {WG_SKINNY, best};
  }
  // 256 x 256 tiles when they still fill the chip (members x tiles >= half the CUs)
  if (sw.big_tiles && M % 256 == 0 && N % 256 == 0) {
    const int64_t units = (int64_t)nmem * (M / 256) * (N / 256);
    if (units < 128 && sw.big_tiles != 2 && ps.bf16 && sw.tn_ring && K % 64 == 0 && K >= 16384) {
      // few large units with a long batch (C5/8: 64 members x one 256 x 256 tile x 71k rows): the ring kernel with K split
      // until the chip is full -- every operand byte is read ONCE (four 128 x 128 tiles read each half twice), and
      // the atomics of the splits (256 x 256 floats each) are nothing next to 2 x K x 256 operand elements
      const int sp = (int)std::min<int64_t>((ps.num_cus + units - 1) / units, K / 4096);
      if (sp >= 1) return {WG_RING, std::max(1, sp)};
    }
    if (units >= 128 || sw.big_tiles == 2) {
      if (ps.bf16 && sw.tn_ring && K % 64 == 0) {
        // the four-stage ring, one workgroup per CU, NO split-K: splitting to shorten the last, partly filled
        // round of workgroups was measured at C3/8 (320 tiles on 256 CUs) -- 2 splits 230 -> 300 us per launch,
        // 4 splits 438 us, 5,680 -> 5,290 -> 4,730 member-steps/s: the f32 atomics of 80 x 512 x 512 outputs
        // per split cost far more than the idle quarter round (round-3 measurement).  BNF_RING_SPLITK forces one.
        return {WG_RING, sw.ring_splitk ? sw.ring_splitk : 1};
      }
      return {WG_TN256, base_sk};
    }
  }
  return {WG_TN128, base_sk};
}

// ---- the step plan -------------------------------------------------------------------------------------------
constexpr int kWgradMerged = -1;   // StepPlan::launch entry: the W x W layers 1 .. L-1 as ONE launch of the ring kernel

struct StepPlan {
  WgradPlan layer[BNF_MAX_LAYERS];   // per layer: kernel and split-K
  bool merged;                       // row-panel pipeline: layers 1 .. L-1 in one launch
  // the weight-gradient launches of the row-panel pipeline, in order: a layer, or kWgradMerged (the layer kernels'
  // pipelines start each weight gradient behind its dZ, in the order of their backward chain: n_launch = 0)
  int n_launch;
  int launch[BNF_MAX_LAYERS];
  // gradient ranges [lo, hi) the NEXT step's weight-gradient kernels store, so the optimiser does not clear them.
  // MAP (k_adam_map takes one range): the first layer l >= 1 with split-K 1, rounded inwards to quads.
  // VI (k_vi_adam): every layer with split-K 1.
  int n_keep;
  int32_t keep_lo[BNF_MAX_LAYERS], keep_hi[BNF_MAX_LAYERS];
  // the fused featurisation backward is formed by the layer-0 weight-gradient kernel (gemm_tn_skinny_featbwd) from its
  // own accumulators instead of by the last phase of the panel kernel, which then ends behind its dZ_0 epilogue
  bool featbwd_in_wgrad;
};

// nmem: the members the step's kernels run over (members for MAP, members x samples for VI)
inline StepPlan make_step_plan(const PlanShape& ps, const Switches& sw, int nmem, bool vi) {
  StepPlan p{};
  for (int l = 0; l < ps.L; ++l) p.layer[l] = wgrad_plan(ps, sw, nmem, l);

  // one launch for the W x W layers: all on the un-split ring, and only where it saves rounds of the chip (C3/8: 3 x 320
  // tiles = 4 rounds instead of 6, +6.6 % on the step; C4/8: 3 x 512 tiles = 6 rounds either way and the merged launch
  // measured 1 % slower)
  p.merged = ps.panel && ps.bf16 && ps.L >= 3 && !sw.overlap && !sw.wgrad_no_multi;
  for (int l = 1; l < ps.L && p.merged; ++l) p.merged = p.layer[l].kind == WG_RING && p.layer[l].splitk == 1;
  if (p.merged) {
    const int64_t units = (int64_t)nmem * (ps.W / 256) * (ps.W / 256), cus = ps.num_cus, n = ps.L - 1;
    p.merged = (n * units + cus - 1) / cus < n * ((units + cus - 1) / cus);
  }

  // Order: the LAST layer's weight gradient first.  In the panel pipeline every dZ_l exists when these run, and the
  // panel kernel wrote dZ_0 last: read right away it comes back at two thirds of the HBM rate (dirty lines in the
  // memory-side cache, profiles/r02w_wgrad_streams.md); after the W x W kernels have streamed their operands it does not.
  // (BNF_WGRAD_ORDER=fwd: layer 0 first, the order of rounds 1 - 3.)
  if (ps.panel) {
    if (p.merged) {
      p.launch[p.n_launch++] = sw.wgrad_order_fwd ? 0 : kWgradMerged;
      p.launch[p.n_launch++] = sw.wgrad_order_fwd ? kWgradMerged : 0;
    } else {
      for (int i = 0; i < ps.L; ++i) p.launch[p.n_launch++] = sw.wgrad_order_fwd ? i : ps.L - 1 - i;
    }
  }

  p.featbwd_in_wgrad = ps.panel && ps.bf16 && !ps.fp8 && ps.featbwd_fused && sw.panel_featbwd && sw.featbwd_wgrad &&
                       ps.n_fourier <= kPlanFbCols && p.layer[0].kind == WG_SKINNY;

  if (!ps.pad && !sw.adam_clear_all && sw.ablate == 0) {
    for (int l = vi ? 0 : 1; l < ps.L; ++l) {
      if (p.layer[l].splitk != 1) continue;
      const int32_t lo = ps.off_kernel[l], hi = lo + ((l == 0) ? ps.F : ps.W) * ps.W;
      p.keep_lo[p.n_keep] = vi ? lo : (lo + 3) / 4 * 4;
      p.keep_hi[p.n_keep] = vi ? hi : hi / 4 * 4;
      ++p.n_keep;
      if (!vi) break;
    }
  }
  return p;
}

// ---- the form of the row-panel kernel ------------------------------------------------------------------------
// The template arguments of k_panel_fwd_bwd<WN, RT, H0L, DEEP, CH, FP, F0, C8, FBW> (bnf_panel.h) a handle launches: 128-row
// panels at W = 512, 64-row panels of two column slabs at W = 1024, 128-row (H0L) or 256-row panels at W = 256.
struct PanelForm {
  int WN, RT; bool H0L, DEEP; int CH, FP; bool F0, C8, FBW;
  int panel_rows;           // rows per workgroup: Bp / panel_rows workgroups per member
  bool separate_feat_bwd;   // k_feat_bwd runs behind the panel kernel (no column table: nothing fused)
};
constexpr PanelForm make_panel_form(const PipelinePlan& pp, const StepPlan& sp, int L, int W, int Fp) {
  PanelForm f{};
  f.H0L = pp.h0l; f.DEEP = L != 2; f.CH = 1; f.FP = 64;
  if (W == 1024) { f.WN = 8; f.RT = 2; f.CH = 2; }
  else if (W == 512) { f.WN = 8; f.RT = 4; }
  else if (pp.h0l) { f.WN = 4; f.RT = 2; f.FP = Fp == 128 ? 128 : 64; }
  else { f.WN = 4; f.RT = 4; }
  // FBW: the featurisation backward moved into the layer-0 weight gradient, the panel kernel ends behind its dZ0 epilogue
  f.FBW = f.H0L && f.WN == 8 && sp.featbwd_in_wgrad;
  f.F0 = pp.fold0;
  f.C8 = pp.c8;
  f.panel_rows = 32 * f.RT * (8 / f.WN);
  f.separate_feat_bwd = !pp.fb_table;
  return f;
}

// The instantiated forms, X(WN, RT, H0L, DEEP, CH, FP, F0, C8, FBW): bnf_api.hip expands the same list into its
// launchers, so an index into kPanelForms is an index into them.  A new form is a new row here.
#define BNF_PANEL_FORMS_H0L8(X, RT, CH, DEEP)                                                                 \
  X(8, RT, true, DEEP, CH, 64, true, false, true) X(8, RT, true, DEEP, CH, 64, false, false, true)             \
  X(8, RT, true, DEEP, CH, 64, true, true, false) X(8, RT, true, DEEP, CH, 64, true, false, false)             \
  X(8, RT, true, DEEP, CH, 64, false, false, false)
#define BNF_PANEL_FORMS_H0L4(X, FP, DEEP)                                                                     \
  X(4, 2, true, DEEP, 1, FP, true, true, false) X(4, 2, true, DEEP, 1, FP, true, false, false)                 \
  X(4, 2, true, DEEP, 1, FP, false, false, false)
#define BNF_PANEL_FORMS_PLAIN(X, WN, RT, CH)                                                                  \
  X(WN, RT, false, false, CH, 64, false, false, false) X(WN, RT, false, true, CH, 64, false, false, false)
#define BNF_PANEL_FORMS(X)                                                                                    \
  BNF_PANEL_FORMS_H0L8(X, 2, 2, false) BNF_PANEL_FORMS_H0L8(X, 2, 2, true)                                     \
  BNF_PANEL_FORMS_H0L8(X, 4, 1, false) BNF_PANEL_FORMS_H0L8(X, 4, 1, true)                                     \
  BNF_PANEL_FORMS_H0L4(X, 64, false) BNF_PANEL_FORMS_H0L4(X, 64, true)                                         \
  BNF_PANEL_FORMS_H0L4(X, 128, false) BNF_PANEL_FORMS_H0L4(X, 128, true)                                       \
  BNF_PANEL_FORMS_PLAIN(X, 8, 2, 2) BNF_PANEL_FORMS_PLAIN(X, 8, 4, 1) BNF_PANEL_FORMS_PLAIN(X, 4, 4, 1)
#define BNF_PANEL_FORM_ROW(WN, RT, H0L, DEEP, CH, FP, F0, C8, FBW) {WN, RT, H0L, DEEP, CH, FP, F0, C8, FBW, 0, false},
constexpr PanelForm kPanelForms[] = {BNF_PANEL_FORMS(BNF_PANEL_FORM_ROW)};
constexpr int kNumPanelForms = (int)(sizeof(kPanelForms) / sizeof(kPanelForms[0]));
#undef BNF_PANEL_FORM_ROW
// the row of kPanelForms with f's nine template arguments; -1: not instantiated
constexpr int panel_form_index(const PanelForm& f) {
  for (int i = 0; i < kNumPanelForms; ++i) {
    const PanelForm& r = kPanelForms[i];
    if (r.WN == f.WN && r.RT == f.RT && r.H0L == f.H0L && r.DEEP == f.DEEP && r.CH == f.CH && r.FP == f.FP &&
        r.F0 == f.F0 && r.C8 == f.C8 && r.FBW == f.FBW)
      return i;
  }
  return -1;
}

// Every form the plans can ask for has a row, over ALL combinations of what they guarantee: h0l at W >= 512 only with
// Fp = 64; fold0 only with h0l; c8 only with fold0; featbwd_in_wgrad only with h0l, W >= 512 and without fp8
constexpr bool every_panel_form_has_a_row() {
  for (int W = 256; W <= 1024; W *= 2)
    for (int Fp = 64; Fp <= 128; Fp += 64)
      for (int bits = 0; bits < 32; ++bits) {
        PipelinePlan pp{};
        StepPlan sp{};
        pp.panel = true; pp.h0l = bits & 1; pp.fold0 = bits & 2; pp.c8 = bits & 4; sp.featbwd_in_wgrad = bits & 8;
        if ((pp.h0l && W >= 512 && Fp != 64) || (pp.fold0 && !pp.h0l) || (pp.c8 && !pp.fold0)) continue;
        if (sp.featbwd_in_wgrad && (!pp.h0l || W < 512 || pp.c8)) continue;
        if (panel_form_index(make_panel_form(pp, sp, bits & 16 ? 3 : 2, W, Fp)) < 0) return false;
      }
  return true;
}
static_assert(every_panel_form_has_a_row(), "a plan can produce a panel form that BNF_PANEL_FORMS does not list");

}  // namespace bnf
