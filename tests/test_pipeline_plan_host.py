"""The pipeline plan, the panel kernel's form and the column table of the fused featurisation backward
(bayesnf_amd/csrc/bnf_plan.h), asserted on the host: g++ compiles a small program around the header, the way
tests/test_step_plan_host.py does, and the tests read what it prints.

Every expected row below was printed by the code this header replaced -- the decision block of `bnf_create`, `panel_h0l`,
the if-ladder of `run_panel` and the three launch levels behind it (`launch_panel`, `launch_panel_d`, `launch_panel_f`) and
the table loop, as they stood in bnf_api.hip, copied onto a mock handle and compiled as plain C++ -- never by the header
under test.  profiles/pipeline_plan_refactor.md records the sweep that compared the two over the whole grid.

A row: the PipelinePlan fields, the padded batch (300 rows: 384 = padded to 128, 512 = padded to 256), whether the column
table is built, the model's Fourier columns as the table counts them, StepPlan::featbwd_in_wgrad, and for a panel handle
the nine template arguments WN, RT, H0L, DEEP, CH, FP, F0, C8, FBW of k_panel_fwd_bwd, the rows per workgroup and whether
k_feat_bwd runs behind the kernel.  `refused=1 / 2 / 3`: the three BNF_ERR_INVALID returns of bnf_create, in their order
(bad pipeline value; panel pipeline asked for where it does not exist; fp8 without the panel pipeline).

Common settings: bf16, depth 2, width 512, 49 features of which 20 are Fourier columns, a raw-input group, 300 rows, 3
members, MAP, defaults unless said.  The probe lays the features out as raw inputs (3), Fourier groups of at most 16
columns, seasonal columns, 2 interactions.  Fourier columns come in pairs: "33 columns" is 34 here, the first count the
32 slots of the layer-0 weight-gradient kernel do not take.
"""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16, FP8, F32S = 0, 1, 2, 3

PROBE = r'''
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include "bnf_plan.h"
struct Case {
  int dtype, fo, L, Wt, F, pipeline, ingroup, nfourier;
  long long B; int nmem, vi;
};
struct Layout {
  int n_groups = 0, n_interact = 0;
  int32_t kind[12] = {}, arg[12] = {}, ncols[12] = {}, col0[12] = {}, scale_off[12] = {};
  int32_t interact[16][2] = {};
};
// raw inputs (3), Fourier groups of at most 16 columns, 2 interactions, seasonal columns for the rest
inline Layout gen_layout(int F, int ingroup, int nfourier) {
  Layout y;
  int col = 0;
  auto add = [&](int kind, int arg, int n) {
    if (n <= 0) return;
    const int g = y.n_groups++;
    y.kind[g] = kind; y.arg[g] = arg; y.ncols[g] = n; y.col0[g] = col; y.scale_off[g] = 7 + 3 * g;
    col += n;
  };
  if (ingroup) add(0, -1, F < 3 ? F : 3);
  int nf = nfourier & ~1;
  if (nf > ((F - col) & ~1)) nf = (F - col) & ~1;
  for (int d = 0; nf > 0; ++d) { const int n = nf < 16 ? nf : 16; add(1, d % 3, n); nf -= n; }
  const int ni = ingroup ? ((F - col) < 2 ? (F - col) : 2) : 0;
  const int ns = F - col - ni;
  add(2, -1, ns);
  add(3, -1, ni);
  y.n_interact = ni;
  for (int k = 0; k < ni; ++k) { y.interact[k][0] = k; y.interact[k][1] = k + 1; }
  return y;
}
struct Row {   // what both sides compute for a case
  int refusal = 0, panel = 0, fuse_last = 0, recompute_a0 = 0, h0l = 0, fold0 = 0, q8 = 0, c8 = 0, table = 0;
  long long Bp = 0;
  int n_fourier = 0, in_group = -1, fbw = 0;
  int form[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, rows = 0, sep = 0, index = -1;
  std::vector<int32_t> meta;
};
inline std::string show(const Row& r) {
  char buf[512];
  if (r.refusal) { snprintf(buf, sizeof(buf), "refused=%d", r.refusal); return buf; }
  int n = snprintf(buf, sizeof(buf), "panel=%d fuse_last=%d recompute_a0=%d h0l=%d fold0=%d q8=%d c8=%d Bp=%lld table=%d n_fourier=%d fbw=%d",
                   r.panel, r.fuse_last, r.recompute_a0, r.h0l, r.fold0, r.q8, r.c8, r.Bp, r.table, r.n_fourier, r.fbw);
  if (r.panel)
    snprintf(buf + n, sizeof(buf) - n, " form=%d,%d,%d,%d,%d,%d,%d,%d,%d rows=%d sep_feat_bwd=%d", r.form[0], r.form[1], r.form[2],
             r.form[3], r.form[4], r.form[5], r.form[6], r.form[7], r.form[8], r.rows, r.sep);
  return buf;
}
static Row new_row(const Case& c, const Layout& y, const bnf::Switches& sw) {
  using namespace bnf;
  Row r;
  const int W = (c.Wt + 63) / 64 * 64, Fp = (c.F + 63) / 64 * 64;
  const PipelinePlan pp = make_pipeline_plan({c.dtype, c.fo != 0, c.L, W, c.F, Fp, c.pipeline, c.ingroup != 0}, sw);
  r.refusal = (int)pp.refusal;
  if (r.refusal) return r;
  r.panel = pp.panel; r.fuse_last = pp.fuse_last; r.recompute_a0 = pp.recompute_a0; r.h0l = pp.h0l; r.fold0 = pp.fold0;
  r.q8 = pp.q8; r.c8 = pp.c8; r.table = pp.fb_table;
  r.Bp = (c.B + pp.bp_align - 1) / pp.bp_align * pp.bp_align;
  FeatBwdTable fb;
  if (pp.fb_table) fb = make_featbwd_table(y.n_groups, y.kind, y.arg, y.ncols, y.col0, y.scale_off, y.interact, Fp);
  if (pp.fb_table != !fb.meta.empty()) r.table = -1;   // the plan's flag and the builder must agree on "there is a table"
  r.n_fourier = fb.n_fourier; r.in_group = fb.in_group; r.meta = fb.meta;
  PlanShape ps{};
  ps.bf16 = c.dtype == BNF_DTYPE_BF16 || c.dtype == BNF_DTYPE_FP8; ps.L = c.L; ps.W = W; ps.F = c.F; ps.Fp = Fp; ps.Bp = r.Bp;
  ps.num_cus = 256; ps.panel = pp.panel; ps.pad = W != c.Wt;
  int32_t at = 0;
  for (int l = 0; l < c.L; ++l) { ps.off_kernel[l] = at + 5; at += 5 + ((l == 0) ? c.F : W) * W + W; }
  ps.fp8 = pp.q8; ps.featbwd_fused = !fb.meta.empty(); ps.n_fourier = fb.n_fourier;
  const StepPlan sp = make_step_plan(ps, sw, c.nmem, c.vi != 0);
  r.fbw = sp.featbwd_in_wgrad;
  if (pp.panel) {
    const PanelForm f = make_panel_form(pp, sp, c.L, W, Fp);
    const int v[9] = {f.WN, f.RT, f.H0L, f.DEEP, f.CH, f.FP, f.F0, f.C8, f.FBW};
    memcpy(r.form, v, sizeof(v));
    r.rows = f.panel_rows; r.sep = f.separate_feat_bwd; r.index = panel_form_index(f);
  }
  return r;
}
static std::map<std::string, std::string> g_env;
static const char* lookup(const char* name) {
  auto it = g_env.find(name);
  return it == g_env.end() ? nullptr : it->second.c_str();
}
// probe row dtype forward_only L Wt F pipeline input_group n_fourier B nmem vi [NAME=VALUE ...]
// probe table Fp n_groups (kind arg ncols col0 scale_off)* n_interact (i j)*
// probe forms
// probe grid
int main(int argc, char** argv) {
  const std::string mode = argv[1];
  if (mode == "row") {
    const Case c{atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), atoi(argv[7]), atoi(argv[8]), atoi(argv[9]),
                 atoll(argv[10]), atoi(argv[11]), atoi(argv[12])};
    for (int i = 13; i < argc; ++i) {
      const std::string a = argv[i];
      g_env[a.substr(0, a.find('='))] = a.substr(a.find('=') + 1);
    }
    const Row r = new_row(c, gen_layout(c.F, c.ingroup, c.nfourier), bnf::read_switches(lookup));
    if (!r.refusal && (r.table < 0 || (r.panel && r.index < 0))) return 3;   // table flag and builder disagree / form not instantiated
    printf("%s\n", show(r).c_str());
  } else if (mode == "table") {
    Layout y;
    int a = 3;
    y.n_groups = atoi(argv[a++]);
    for (int g = 0; g < y.n_groups; ++g) {
      y.kind[g] = atoi(argv[a++]); y.arg[g] = atoi(argv[a++]); y.ncols[g] = atoi(argv[a++]); y.col0[g] = atoi(argv[a++]);
      y.scale_off[g] = atoi(argv[a++]);
    }
    y.n_interact = atoi(argv[a++]);
    for (int k = 0; k < y.n_interact; ++k) { y.interact[k][0] = atoi(argv[a++]); y.interact[k][1] = atoi(argv[a++]); }
    const bnf::FeatBwdTable t = bnf::make_featbwd_table(y.n_groups, y.kind, y.arg, y.ncols, y.col0, y.scale_off, y.interact, atoi(argv[2]));
    printf("in_group=%d n_fourier=%d words=", t.in_group, t.n_fourier);
    for (size_t i = 0; i < t.meta.size(); ++i) printf("%s%d", i ? "," : "", t.meta[i]);
    printf("\n");
  } else if (mode == "grid") {   // every switch combination at each panel shape class: the forms, one line each
    const char* names[5] = {"BNF_PANEL_NO_H0L", "BNF_PANEL_FOLD0", "BNF_PANEL_FEATBWD", "BNF_FEATBWD_WGRAD", "BNF_FP8_CONTRACT"};
    const int shapes[3][4] = {{2, 49, 1, 20}, {3, 63, 1, 34}, {2, 100, 0, 20}};   // L, F, input group, Fourier columns
    for (int dtype = 1; dtype <= 2; ++dtype)
      for (int Wt = 256; Wt <= 1024; Wt *= 2)
        for (const auto& sh : shapes)
          for (int sw = 0; sw < 32; ++sw) {
            g_env.clear();
            for (int b = 0; b < 5; ++b)
              if (sw >> b & 1) g_env[names[b]] = b == 0 ? "1" : "0";
            const Case c{dtype, 0, sh[0], Wt, sh[1], 0, sh[2], sh[3], 300, 3, 0};
            const Row r = new_row(c, gen_layout(c.F, c.ingroup, c.nfourier), bnf::read_switches(lookup));
            if (r.refusal || !r.panel || r.table < 0 || r.index < 0) return 3;
            printf("%d,%d,%d,%d,%d,%d,%d,%d,%d\n", r.form[0], r.form[1], r.form[2], r.form[3], r.form[4], r.form[5], r.form[6],
                   r.form[7], r.form[8]);
          }
  } else {
    for (int i = 0; i < bnf::kNumPanelForms; ++i) {
      const bnf::PanelForm& f = bnf::kPanelForms[i];
      printf("%d,%d,%d,%d,%d,%d,%d,%d,%d\n", f.WN, f.RT, f.H0L, f.DEEP, f.CH, f.FP, f.F0, f.C8, f.FBW);
    }
  }
  return 0;
}
'''

# printed by the replaced code (see the module's docstring)
EXPECTED = {
    'C1-bf16':
        'panel=1 fuse_last=0 recompute_a0=0 h0l=1 fold0=1 q8=0 c8=0 Bp=512 table=1 n_fourier=20 fbw=0 form=4,2,1,0,1,64,1,0,0 rows=128 sep_feat_bwd=0',
    'C1-f32':
        'panel=0 fuse_last=1 recompute_a0=1 h0l=0 fold0=0 q8=0 c8=0 Bp=384 table=0 n_fourier=0 fbw=0',
    'C2':
        'panel=1 fuse_last=0 recompute_a0=0 h0l=1 fold0=1 q8=0 c8=0 Bp=512 table=1 n_fourier=20 fbw=1 form=8,4,1,0,1,64,1,0,1 rows=128 sep_feat_bwd=0',
    'C3-VI':
        'panel=1 fuse_last=0 recompute_a0=0 h0l=1 fold0=1 q8=0 c8=0 Bp=512 table=1 n_fourier=30 fbw=1 form=8,4,1,1,1,64,1,0,1 rows=128 sep_feat_bwd=0',
    'C4':
        'panel=1 fuse_last=0 recompute_a0=0 h0l=1 fold0=1 q8=0 c8=0 Bp=512 table=1 n_fourier=20 fbw=1 form=8,2,1,1,2,64,1,0,1 rows=64 sep_feat_bwd=0',
    'C5-fp8':
        'panel=1 fuse_last=0 recompute_a0=0 h0l=1 fold0=1 q8=1 c8=1 Bp=512 table=1 n_fourier=20 fbw=0 form=4,2,1,0,1,128,1,1,0 rows=128 sep_feat_bwd=0',
    'F62':
        'panel=1 fuse_last=0 recompute_a0=0 h0l=1 fold0=1 q8=0 c8=0 Bp=512 table=1 n_fourier=20 fbw=1 form=8,4,1,0,1,64,1,0,1 rows=128 sep_feat_bwd=0',
    'F63':
        'panel=1 fuse_last=0 recompute_a0=0 h0l=1 fold0=0 q8=0 c8=0 Bp=512 table=1 n_fourier=20 fbw=1 form=8,4,1,0,1,64,0,0,1 rows=128 sep_feat_bwd=0',
    'F64':
        'panel=1 fuse_last=0 recompute_a0=0 h0l=1 fold0=0 q8=0 c8=0 Bp=512 table=1 n_fourier=20 fbw=1 form=8,4,1,0,1,64,0,0,1 rows=128 sep_feat_bwd=0',
    'Fp128-W512':
        'panel=1 fuse_last=0 recompute_a0=0 h0l=0 fold0=0 q8=0 c8=0 Bp=512 table=0 n_fourier=0 fbw=0 form=8,4,0,0,1,64,0,0,0 rows=128 sep_feat_bwd=1',
    'Fp128-W1024':
        'panel=1 fuse_last=0 recompute_a0=0 h0l=0 fold0=0 q8=0 c8=0 Bp=512 table=0 n_fourier=0 fbw=0 form=8,2,0,0,2,64,0,0,0 rows=64 sep_feat_bwd=1',
    'W200-padded':
        'panel=1 fuse_last=0 recompute_a0=0 h0l=1 fold0=1 q8=0 c8=0 Bp=512 table=1 n_fourier=20 fbw=0 form=4,2,1,0,1,64,1,0,0 rows=128 sep_feat_bwd=0',
    'W320':
        'panel=0 fuse_last=0 recompute_a0=1 h0l=0 fold0=0 q8=0 c8=0 Bp=384 table=0 n_fourier=0 fbw=0',
    'W320-fp8':
        'refused=3',
    'Fp192':
        'panel=0 fuse_last=1 recompute_a0=0 h0l=0 fold0=0 q8=0 c8=0 Bp=384 table=0 n_fourier=0 fbw=0',
    'depth1':
        'panel=0 fuse_last=1 recompute_a0=0 h0l=0 fold0=0 q8=0 c8=0 Bp=384 table=0 n_fourier=0 fbw=0',
    'depth1-fp8':
        'refused=3',
    'forward_only':
        'panel=0 fuse_last=0 recompute_a0=0 h0l=0 fold0=0 q8=0 c8=0 Bp=384 table=0 n_fourier=0 fbw=0',
    'forward_only-fp8':
        'panel=0 fuse_last=0 recompute_a0=0 h0l=0 fold0=0 q8=1 c8=0 Bp=384 table=0 n_fourier=0 fbw=0',
    'forward_only-f32-W64':
        'panel=0 fuse_last=0 recompute_a0=0 h0l=0 fold0=0 q8=0 c8=0 Bp=384 table=0 n_fourier=0 fbw=0',
    'cfg-pipeline1':
        'panel=0 fuse_last=0 recompute_a0=0 h0l=0 fold0=0 q8=0 c8=0 Bp=384 table=0 n_fourier=0 fbw=0',
    'cfg-pipeline3':
        'panel=1 fuse_last=0 recompute_a0=0 h0l=1 fold0=1 q8=0 c8=0 Bp=512 table=1 n_fourier=20 fbw=1 form=8,4,1,0,1,64,1,0,1 rows=128 sep_feat_bwd=0',
    'cfg-pipeline3-W320':
        'refused=2',
    'cfg-pipeline1-fp8':
        'refused=3',
    'env-pipeline1':
        'panel=0 fuse_last=0 recompute_a0=0 h0l=0 fold0=0 q8=0 c8=0 Bp=384 table=0 n_fourier=0 fbw=0',
    'env-pipeline3':
        'panel=1 fuse_last=0 recompute_a0=0 h0l=1 fold0=1 q8=0 c8=0 Bp=512 table=1 n_fourier=20 fbw=1 form=8,4,1,0,1,64,1,0,1 rows=128 sep_feat_bwd=0',
    'env-pipeline0-over-cfg1':
        'panel=1 fuse_last=0 recompute_a0=0 h0l=1 fold0=1 q8=0 c8=0 Bp=512 table=1 n_fourier=20 fbw=1 form=8,4,1,0,1,64,1,0,1 rows=128 sep_feat_bwd=0',
    'env-pipeline3-f32':
        'refused=2',
    'env-pipeline2':
        'refused=1',
    'f32-W512':
        'panel=0 fuse_last=0 recompute_a0=1 h0l=0 fold0=0 q8=0 c8=0 Bp=384 table=0 n_fourier=0 fbw=0',
    'f32-W64-depth3':
        'panel=0 fuse_last=1 recompute_a0=1 h0l=0 fold0=0 q8=0 c8=0 Bp=384 table=0 n_fourier=0 fbw=0',
    'f32s-W256':
        'panel=0 fuse_last=1 recompute_a0=1 h0l=0 fold0=0 q8=0 c8=0 Bp=384 table=0 n_fourier=0 fbw=0',
    'bf16-W128':
        'panel=0 fuse_last=1 recompute_a0=1 h0l=0 fold0=0 q8=0 c8=0 Bp=384 table=0 n_fourier=0 fbw=0',
    'no_h0l-W512':
        'panel=1 fuse_last=0 recompute_a0=0 h0l=0 fold0=0 q8=0 c8=0 Bp=512 table=0 n_fourier=0 fbw=0 form=8,4,0,0,1,64,0,0,0 rows=128 sep_feat_bwd=1',
    'no_h0l-W256':
        'panel=1 fuse_last=0 recompute_a0=0 h0l=0 fold0=0 q8=0 c8=0 Bp=512 table=0 n_fourier=0 fbw=0 form=4,4,0,0,1,64,0,0,0 rows=256 sep_feat_bwd=1',
    'no_h0l-W1024-depth3':
        'panel=1 fuse_last=0 recompute_a0=0 h0l=0 fold0=0 q8=0 c8=0 Bp=512 table=0 n_fourier=0 fbw=0 form=8,2,0,1,2,64,0,0,0 rows=64 sep_feat_bwd=1',
    'fold0-off':
        'panel=1 fuse_last=0 recompute_a0=0 h0l=1 fold0=0 q8=0 c8=0 Bp=512 table=1 n_fourier=20 fbw=1 form=8,4,1,0,1,64,0,0,1 rows=128 sep_feat_bwd=0',
    'fold0-off-W256-Fp128':
        'panel=1 fuse_last=0 recompute_a0=0 h0l=1 fold0=0 q8=0 c8=0 Bp=512 table=1 n_fourier=20 fbw=0 form=4,2,1,0,1,128,0,0,0 rows=128 sep_feat_bwd=0',
    'featbwd-off':
        'panel=1 fuse_last=0 recompute_a0=0 h0l=1 fold0=1 q8=0 c8=0 Bp=512 table=0 n_fourier=0 fbw=0 form=8,4,1,0,1,64,1,0,0 rows=128 sep_feat_bwd=1',
    'featbwd_wgrad-off':
        'panel=1 fuse_last=0 recompute_a0=0 h0l=1 fold0=1 q8=0 c8=0 Bp=512 table=1 n_fourier=20 fbw=0 form=8,4,1,0,1,64,1,0,0 rows=128 sep_feat_bwd=0',
    'featbwd_wgrad-off-F63-depth3':
        'panel=1 fuse_last=0 recompute_a0=0 h0l=1 fold0=0 q8=0 c8=0 Bp=512 table=1 n_fourier=20 fbw=0 form=8,4,1,1,1,64,0,0,0 rows=128 sep_feat_bwd=0',
    'fp8-W512':
        'panel=1 fuse_last=0 recompute_a0=0 h0l=1 fold0=1 q8=1 c8=1 Bp=512 table=1 n_fourier=20 fbw=0 form=8,4,1,0,1,64,1,1,0 rows=128 sep_feat_bwd=0',
    'fp8_contract-off':
        'panel=1 fuse_last=0 recompute_a0=0 h0l=1 fold0=1 q8=1 c8=0 Bp=512 table=1 n_fourier=20 fbw=0 form=8,4,1,0,1,64,1,0,0 rows=128 sep_feat_bwd=0',
    'fp8-F63':
        'panel=1 fuse_last=0 recompute_a0=0 h0l=1 fold0=0 q8=1 c8=0 Bp=512 table=1 n_fourier=20 fbw=0 form=8,4,1,0,1,64,0,0,0 rows=128 sep_feat_bwd=0',
    'fp8-W1024-depth3':
        'panel=1 fuse_last=0 recompute_a0=0 h0l=1 fold0=1 q8=1 c8=1 Bp=512 table=1 n_fourier=20 fbw=0 form=8,2,1,1,2,64,1,1,0 rows=64 sep_feat_bwd=0',
    'no-input-group':
        'panel=1 fuse_last=0 recompute_a0=0 h0l=1 fold0=1 q8=0 c8=0 Bp=512 table=0 n_fourier=0 fbw=0 form=8,4,1,0,1,64,1,0,0 rows=128 sep_feat_bwd=1',
    'no-input-group-W256':
        'panel=1 fuse_last=0 recompute_a0=0 h0l=1 fold0=1 q8=0 c8=0 Bp=512 table=0 n_fourier=0 fbw=0 form=4,2,1,0,1,64,1,0,0 rows=128 sep_feat_bwd=1',
    'fourier32':
        'panel=1 fuse_last=0 recompute_a0=0 h0l=1 fold0=1 q8=0 c8=0 Bp=512 table=1 n_fourier=32 fbw=1 form=8,4,1,0,1,64,1,0,1 rows=128 sep_feat_bwd=0',
    'fourier34':
        'panel=1 fuse_last=0 recompute_a0=0 h0l=1 fold0=1 q8=0 c8=0 Bp=512 table=1 n_fourier=34 fbw=0 form=8,4,1,0,1,64,1,0,0 rows=128 sep_feat_bwd=0',
    'W256-Fp128-depth3':
        'panel=1 fuse_last=0 recompute_a0=0 h0l=1 fold0=1 q8=0 c8=0 Bp=512 table=1 n_fourier=20 fbw=0 form=4,2,1,1,1,128,1,0,0 rows=128 sep_feat_bwd=0',
    'W1024':
        'panel=1 fuse_last=0 recompute_a0=0 h0l=1 fold0=1 q8=0 c8=0 Bp=512 table=1 n_fourier=20 fbw=1 form=8,2,1,0,2,64,1,0,1 rows=64 sep_feat_bwd=0',
    'W256-depth4':
        'panel=1 fuse_last=0 recompute_a0=0 h0l=1 fold0=1 q8=0 c8=0 Bp=512 table=1 n_fourier=20 fbw=0 form=4,2,1,1,1,64,1,0,0 rows=128 sep_feat_bwd=0',
}


@pytest.fixture(scope='module')
def probe(tmp_path_factory):
  d = tmp_path_factory.mktemp('pipeline_plan')
  src, exe = d / 'probe.cc', d / 'probe'
  src.write_text(PROBE)
  subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'bayesnf_amd', 'csrc'),
                         str(src), '-o', str(exe)])
  return lambda *args: subprocess.check_output([str(exe)] + [str(a) for a in args]).decode().strip()


DEFAULT = dict(dtype=BF16, fo=0, L=2, Wt=512, F=49, pipeline=0, ingroup=1, nfourier=20, B=300, nmem=3, vi=0, env=())


def row_args(kw):
  c = {**DEFAULT, **kw}
  return [c[k] for k in ('dtype', 'fo', 'L', 'Wt', 'F', 'pipeline', 'ingroup', 'nfourier', 'B', 'nmem', 'vi')] + list(c['env'])


# id -> what leaves the common settings.  tests/test_gpu_workspace_layout.py creates a handle for each row that is not
# refused and holds its workspace size to the one recorded before the plan moved here.
CASES = {
    # the BASELINE layouts
    'C1-bf16': dict(Wt=256, F=57), 'C1-f32': dict(dtype=F32, Wt=256, F=57), 'C2': dict(F=57),
    'C3-VI': dict(L=4, nfourier=30, vi=1, nmem=6), 'C4': dict(Wt=1024, L=4, F=59), 'C5-fp8': dict(dtype=FP8, Wt=256, F=79),
    # layer-0 fold: F + 2 <= Fp
    'F62': dict(F=62), 'F63': dict(F=63), 'F64': dict(F=64),
    'Fp128-W512': dict(F=100), 'Fp128-W1024': dict(Wt=1024, F=100),                 # no H0L: the fragment-major copy H0t
    'W200-padded': dict(Wt=200), 'W320': dict(Wt=320), 'W320-fp8': dict(dtype=FP8, Wt=320),
    'Fp192': dict(F=150),
    'depth1': dict(L=1), 'depth1-fp8': dict(dtype=FP8, L=1),
    'forward_only': dict(fo=1), 'forward_only-fp8': dict(dtype=FP8, fo=1), 'forward_only-f32-W64': dict(dtype=F32, fo=1, Wt=64),
    'cfg-pipeline1': dict(pipeline=1), 'cfg-pipeline3': dict(pipeline=3), 'cfg-pipeline3-W320': dict(pipeline=3, Wt=320),
    'cfg-pipeline1-fp8': dict(dtype=FP8, pipeline=1),
    'env-pipeline1': dict(env=('BNF_PIPELINE=1',)), 'env-pipeline3': dict(pipeline=1, env=('BNF_PIPELINE=3',)),
    'env-pipeline0-over-cfg1': dict(pipeline=1, env=('BNF_PIPELINE=0',)),
    'env-pipeline3-f32': dict(dtype=F32, env=('BNF_PIPELINE=3',)), 'env-pipeline2': dict(env=('BNF_PIPELINE=2',)),
    'f32-W512': dict(dtype=F32), 'f32-W64-depth3': dict(dtype=F32, Wt=64, L=3), 'f32s-W256': dict(dtype=F32S, Wt=256),
    'bf16-W128': dict(Wt=128),
    'no_h0l-W512': dict(env=('BNF_PANEL_NO_H0L=1',)), 'no_h0l-W256': dict(Wt=256, env=('BNF_PANEL_NO_H0L=1',)),
    'no_h0l-W1024-depth3': dict(Wt=1024, L=3, env=('BNF_PANEL_NO_H0L=1',)),
    'fold0-off': dict(env=('BNF_PANEL_FOLD0=0',)), 'fold0-off-W256-Fp128': dict(Wt=256, F=100, env=('BNF_PANEL_FOLD0=0',)),
    'featbwd-off': dict(env=('BNF_PANEL_FEATBWD=0',)), 'featbwd_wgrad-off': dict(env=('BNF_FEATBWD_WGRAD=0',)),
    'featbwd_wgrad-off-F63-depth3': dict(F=63, L=3, env=('BNF_FEATBWD_WGRAD=0',)),
    'fp8-W512': dict(dtype=FP8), 'fp8_contract-off': dict(dtype=FP8, env=('BNF_FP8_CONTRACT=0',)),
    'fp8-F63': dict(dtype=FP8, F=63), 'fp8-W1024-depth3': dict(dtype=FP8, Wt=1024, L=3),
    'no-input-group': dict(ingroup=0), 'no-input-group-W256': dict(ingroup=0, Wt=256),
    'fourier32': dict(F=57, nfourier=32), 'fourier34': dict(F=57, nfourier=34),
    'W256-Fp128-depth3': dict(Wt=256, F=100, L=3), 'W1024': dict(Wt=1024), 'W256-depth4': dict(Wt=256, L=4),
}


@pytest.mark.parametrize('name', list(CASES))
def test_plan_and_form_are_the_ones_the_replaced_code_gave(probe, name):
  assert probe('row', *row_args(CASES[name])) == EXPECTED[name]


def test_every_instantiated_form_is_listed_once(probe):
  """The table bnf_api.hip expands into its launchers: the 38 forms the replaced ladder instantiated, each once."""
  forms = probe('forms').split('\n')
  assert len(forms) == 38 and len(set(forms)) == 38
  want = set()
  for deep in (0, 1):
    for rt, ch in ((2, 2), (4, 1)):
      for f0, c8, fbw in ((1, 0, 1), (0, 0, 1), (1, 1, 0), (1, 0, 0), (0, 0, 0)):
        want.add(f'8,{rt},1,{deep},{ch},64,{f0},{c8},{fbw}')
    for fp in (64, 128):
      for f0, c8, fbw in ((1, 1, 0), (1, 0, 0), (0, 0, 0)):
        want.add(f'4,2,1,{deep},1,{fp},{f0},{c8},{fbw}')
    for wn, rt, ch in ((8, 2, 2), (8, 4, 1), (4, 4, 1)):
      want.add(f'{wn},{rt},0,{deep},{ch},64,0,0,0')
  assert set(forms) == want


def test_no_plan_produces_a_form_outside_the_table(probe):
  """bnf_plan.h itself asserts (static_assert on every_panel_form_has_a_row) that every combination of flags the plans can
  hand to make_panel_form has a row, so the probe does not compile otherwise.  Here the plans themselves, end to end: the
  probe exits with status 3 where a panel handle's form is not in the table, or the plan's `fb_table` and the table builder
  disagree -- over every switch combination at each panel shape class, both depths and the fold boundary."""
  seen = set(probe('grid').split('\n'))      # 2 dtypes x 3 widths x 3 shapes x 32 switch combinations
  assert seen <= set(probe('forms').split('\n')) and len(seen) > 1


# ---- the column table ----------------------------------------------------------------------------------------
# three models through NetSpec (the layout bnf_create receives); tests/golden/featbwd_tables.json holds what the replaced
# loop of bnf_create printed for the same group arrays: every word of the table -- four per column, the group offsets,
# the Fourier slots -- the raw-input group and the Fourier column count
MODELS = {
    'C3-49-features': dict(width=512, depth=4, fourier_degrees=[5, 5, 5], interactions=[], seasonality_periods=[24, 168],
                           num_seasonal_harmonics=[4, 4]),
    'interactions': dict(width=512, depth=2, fourier_degrees=[3, 2, 0], interactions=[[0, 1], [1, 2], [0, 2]],
                         seasonality_periods=[7], num_seasonal_harmonics=[2]),
    'C5-Fp128': dict(width=256, depth=2, fourier_degrees=[5, 5, 5], interactions=[], seasonality_periods=[7, 30.4375, 365.25],
                     num_seasonal_harmonics=[3, 10, 10]),
}


def table_args(name):
  from bayesnf_amd.spec import NetSpec
  net = NetSpec(input_scales=[100.0, 1.0, 1.0], **MODELS[name])
  args = [(net.F + 63) // 64 * 64, len(net.groups)]
  for g in net.groups:
    args += [g.kind, g.arg, g.ncols, g.col0, g.scale_offset]
  args.append(net.interactions.shape[0])
  for i, j in net.interactions:
    args += [int(i), int(j)]
  return net, args


@pytest.mark.parametrize('name', list(MODELS))
def test_column_table_is_the_one_the_replaced_loop_built(probe, name):
  golden = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'featbwd_tables.json')))[name]
  net, args = table_args(name)
  assert net.F == golden['F'] and args == golden['args']
  head, words = probe('table', *args).split(' words=')
  assert head == golden['head']
  words = [int(w) for w in words.split(',')]
  Fp = args[0]
  assert len(words) == 4 * Fp + 12 + 32
  assert words == golden['words']
