"""The step plan and the environment switches (bayesnf_amd/csrc/bnf_plan.h), asserted on the host: g++ compiles a small
program around the header (the way tests/test_abi.py compiles its C probe) and the tests read what it prints.

Every expected plan below was produced by the function this header replaced -- `wgrad_plan` / `wgrad_multi_ok` and the
keep-range loops of `step_map` / `step_vi` as they stood in bnf_api.hip, compiled as plain C++ -- never by the header
under test; profiles/step_plan_refactor.md records the sweep that compared the two over the whole grid.  They are the
plans of the comment THE PLANS in tests/test_gpu_optimizer.py.

Common settings: 3 members (VI: 3 x S virtual members), F = 49 features, Fp = 64, 256 CUs, defaults unless said.  The
probe lays the parameters out with kernel_0 at 5 and each kernel followed by its W biases and 5 scalars, so that no
kernel starts on a multiple of 4: the MAP range is rounded inwards to quads at both ends, the VI ranges are exact.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROBE = r'''
#include <cstdio>
#include <map>
#include <string>
#include "bnf_plan.h"
using namespace bnf;
static std::map<std::string, std::string> g_env;
static const char* lookup(const char* name) {
  auto it = g_env.find(name);
  return it == g_env.end() ? nullptr : it->second.c_str();
}
// probe switches [NAME=VALUE ...]
// probe plan bf16 panel W L Bp F Fp cus nmem vi pad [NAME=VALUE ...]
int main(int argc, char** argv) {
  const bool plan = std::string(argv[1]) == "plan";
  for (int i = plan ? 13 : 2; i < argc; ++i) {
    const std::string a = argv[i];
    g_env[a.substr(0, a.find('='))] = a.substr(a.find('=') + 1);
  }
  const Switches sw = read_switches(lookup);
  if (!plan) {
    printf("ablate=%d big_tiles=%d skinny=%d tn_ring=%d graph_mode=%d adam_clear_all=%d vi_sample_pack=%d vi_keep_z=%d "
           "pipeline_set=%d pipeline=%d fp8_contract=%d panel_fold0=%d panel_featbwd=%d panel_no_h0l=%d overlap=%d "
           "wgrad_no_multi=%d wgrad_order_fwd=%d ring_splitk=%d phase_prof=%s\n",
           sw.ablate, sw.big_tiles, sw.skinny, sw.tn_ring, sw.graph_mode, sw.adam_clear_all, sw.vi_sample_pack, sw.vi_keep_z,
           sw.pipeline_set, sw.pipeline, sw.fp8_contract, sw.panel_fold0, sw.panel_featbwd, sw.panel_no_h0l, sw.overlap,
           sw.wgrad_no_multi, sw.wgrad_order_fwd, sw.ring_splitk, sw.phase_prof.c_str());
    return 0;
  }
  PlanShape ps{};
  ps.bf16 = atoi(argv[2]); ps.panel = atoi(argv[3]); ps.W = atoi(argv[4]); ps.L = atoi(argv[5]); ps.Bp = atoll(argv[6]);
  ps.F = atoi(argv[7]); ps.Fp = atoi(argv[8]); ps.num_cus = atoi(argv[9]);
  const int nmem = atoi(argv[10]);
  const bool vi = atoi(argv[11]);
  ps.pad = atoi(argv[12]);
  int32_t at = 0;
  for (int l = 0; l < ps.L; ++l) { ps.off_kernel[l] = at + 5; at += 5 + ((l == 0) ? ps.F : ps.W) * ps.W + ps.W; }
  const StepPlan p = make_step_plan(ps, sw, nmem, vi);
  const char* kind[] = {"TN128", "TN256", "RING", "SKINNY"};
  for (int l = 0; l < ps.L; ++l) {
    const WgradPlan one = wgrad_plan(ps, sw, nmem, l);   // the per-layer function and the plan's copy of it
    if (one.kind != p.layer[l].kind || one.splitk != p.layer[l].splitk) return 3;
    printf("%s%s*%d", l ? " " : "", kind[p.layer[l].kind], p.layer[l].splitk);
  }
  printf(" merged=%d order=", (int)p.merged);
  for (int i = 0; i < p.n_launch; ++i) printf("%d,", p.launch[i]);
  printf(" keep=");
  for (int r = 0; r < p.n_keep; ++r) printf("[%d,%d)", p.keep_lo[r], p.keep_hi[r]);
  printf("\n");
  return 0;
}
'''


@pytest.fixture(scope='module')
def probe(tmp_path_factory):
  d = tmp_path_factory.mktemp('step_plan')
  src, exe = d / 'probe.cc', d / 'probe'
  src.write_text(PROBE)
  subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'bayesnf_amd', 'csrc'),
                         str(src), '-o', str(exe)])
  return lambda *args: subprocess.check_output([str(exe)] + [str(a) for a in args]).decode().strip()


def _plan(probe, bf16=0, panel=0, W=64, L=2, Bp=128, F=49, Fp=64, cus=256, nmem=3, vi=0, pad=0, env=()):
  return probe('plan', bf16, panel, W, L, Bp, F, Fp, cus, nmem, vi, pad, *env)


# order: the panel pipeline's launches, first to last; -1 is the merged launch of the layers 1 .. L-1
PLANS = [
    # THE PLANS 1, 2: fp32 layer kernels
    (dict(W=64, L=2, Bp=128), 'TN128*1 TN128*1 merged=0 order= keep=[3212,7304)'),                   # MAP keeps L1
    (dict(W=64, L=2, Bp=256), 'TN128*2 TN128*2 merged=0 order= keep='),
    (dict(W=256, L=3, Bp=128), 'TN128*1 TN128*1 TN128*1 merged=0 order= keep=[12812,78344)'),      # L1 only
    # 4: bf16 layer kernels
    (dict(bf16=1, W=128, L=2, Bp=384), 'TN128*1 TN128*1 merged=0 order= keep=[6412,22792)'),
    (dict(bf16=1, W=128, L=2, Bp=640), 'TN128*2 TN128*2 merged=0 order= keep='),
    # 5: bf16 row-panel pipeline, the last layer's weight gradient first
    (dict(bf16=1, panel=1, W=256, L=2, Bp=256), 'TN128*1 TN128*1 merged=0 order=1,0, keep=[12812,78344)'),
    (dict(bf16=1, panel=1, W=256, L=2, Bp=768), 'TN128*3 TN128*3 merged=0 order=1,0, keep='),
    (dict(bf16=1, panel=1, W=512, L=2, Bp=256), 'SKINNY*1 TN128*1 merged=0 order=1,0, keep=[25612,287752)'),
    (dict(bf16=1, panel=1, W=512, L=2, Bp=768), 'SKINNY*3 TN128*3 merged=0 order=1,0, keep='),
    # 6: BNF_BIG_TILES=2, the ring kernel and the merged launch at their smallest geometry; the ring launch, then layer 0
    (dict(bf16=1, panel=1, W=256, L=3, Bp=512, env=('BNF_BIG_TILES=2',)),
     'TN128*2 RING*1 RING*1 merged=1 order=-1,0, keep=[12812,78344)'),
    (dict(bf16=1, panel=1, W=256, L=3, Bp=512, env=('BNF_BIG_TILES=2', 'BNF_WGRAD_NO_MULTI=1')),
     'TN128*2 RING*1 RING*1 merged=0 order=2,1,0, keep=[12812,78344)'),
    (dict(bf16=1, panel=1, W=256, L=3, Bp=512, env=('BNF_BIG_TILES=2', 'BNF_WGRAD_ORDER=fwd')),
     'TN128*2 RING*1 RING*1 merged=1 order=0,-1, keep=[12812,78344)'),
    (dict(bf16=1, panel=1, W=256, L=3, Bp=512, env=('BNF_BIG_TILES=2', 'BNF_RING_SPLITK=2')),
     'TN128*2 RING*2 RING*2 merged=0 order=2,1,0, keep='),
    (dict(bf16=1, panel=1, W=256, L=3, Bp=512, env=('BNF_BIG_TILES=2', 'BNF_ADAM_CLEAR_ALL=1')),
     'TN128*2 RING*1 RING*1 merged=1 order=-1,0, keep='),
    # 12, 14: VI, members x S virtual members; every stored layer is kept, layer 0 with F * W entries
    (dict(bf16=1, panel=1, W=256, L=2, Bp=512, nmem=9, vi=1), 'TN128*2 TN128*2 merged=0 order=1,0, keep='),
    (dict(bf16=1, panel=1, W=256, L=2, Bp=256, nmem=9, vi=1),
     'TN128*1 TN128*1 merged=0 order=1,0, keep=[5,12549)[12810,78346)'),
    (dict(W=64, L=1, Bp=128, nmem=6, vi=1), 'TN128*1 merged=0 order= keep=[5,3141)'),
    (dict(bf16=1, panel=1, W=256, L=2, Bp=256, nmem=9, vi=1, env=('BNF_ADAM_CLEAR_ALL=1',)),
     'TN128*1 TN128*1 merged=0 order=1,0, keep='),
    # the benchmark classes: 80 members W 512 depth 4 (3 x 320 tiles: 4 rounds of the chip merged instead of 6) and
    # 64 members W 256 with 100 features over 71,168 rows (the split ring; nothing merged at depth 2)
    (dict(bf16=1, panel=1, W=512, L=4, Bp=8192, nmem=80),
     'SKINNY*3 RING*1 RING*1 RING*1 merged=1 order=-1,0, keep=[25612,287752)'),
    (dict(bf16=1, panel=1, W=256, L=2, Bp=71168, F=100, Fp=128, nmem=64), 'TN128*8 RING*4 merged=0 order=1,0, keep='),
    # 3: a padded width (model width 100, run at 128) keeps nothing
    (dict(W=128, L=2, Bp=128, pad=1), 'TN128*1 TN128*1 merged=0 order= keep='),
]


@pytest.mark.parametrize('args,want', PLANS, ids=[' '.join(f'{k}={v}' for k, v in a.items()) for a, _ in PLANS])
def test_step_plan_is_the_one_the_replaced_functions_gave(probe, args, want):
  assert _plan(probe, **args) == want


DEFAULTS = dict(ablate='0', big_tiles='1', skinny='1', tn_ring='1', graph_mode='0', adam_clear_all='0', vi_sample_pack='1',
                vi_keep_z='0', pipeline_set='0', pipeline='0', fp8_contract='1', panel_fold0='1', panel_featbwd='1',
                panel_no_h0l='0', overlap='0', wgrad_no_multi='0', wgrad_order_fwd='0', ring_splitk='0', phase_prof='')

# each variable set alone -> the fields that leave their defaults (the parsing of the reads this header replaced: atoi;
# presence only for BNF_ADAM_CLEAR_ALL, BNF_WGRAD_NO_MULTI and BNF_PANEL_NO_H0L; "fwd" for the order)
ALONE = [
    ('BNF_ABLATE=3', dict(ablate='3')),
    ('BNF_BIG_TILES=0', dict(big_tiles='0')), ('BNF_BIG_TILES=2', dict(big_tiles='2')),
    ('BNF_WGRAD_SKINNY=0', dict(skinny='0')),
    ('BNF_TN_RING=0', dict(tn_ring='0')),
    ('BNF_GRAPH=1', dict(graph_mode='1')),
    ('BNF_ADAM_CLEAR_ALL=1', dict(adam_clear_all='1')), ('BNF_ADAM_CLEAR_ALL=0', dict(adam_clear_all='1')),
    ('BNF_VI_SAMPLE_PACK=0', dict(vi_sample_pack='0')), ('BNF_VI_SAMPLE_PACK=1', {}),
    ('BNF_VI_KEEP_Z=1', dict(vi_keep_z='1')), ('BNF_VI_KEEP_Z=0', {}),
    ('BNF_PIPELINE=0', dict(pipeline_set='1')),                              # set to 0 (auto) is not "unset"
    ('BNF_PIPELINE=3', dict(pipeline_set='1', pipeline='3')),
    ('BNF_FP8_CONTRACT=0', dict(fp8_contract='0')), ('BNF_FP8_CONTRACT=1', {}),
    ('BNF_PANEL_FOLD0=0', dict(panel_fold0='0')), ('BNF_PANEL_FOLD0=1', {}),
    ('BNF_PANEL_FEATBWD=0', dict(panel_featbwd='0')),
    ('BNF_PANEL_NO_H0L=1', dict(panel_no_h0l='1')), ('BNF_PANEL_NO_H0L=0', dict(panel_no_h0l='1')),
    ('BNF_OVERLAP=1', dict(overlap='1')), ('BNF_OVERLAP=0', {}),
    ('BNF_WGRAD_NO_MULTI=1', dict(wgrad_no_multi='1')), ('BNF_WGRAD_NO_MULTI=0', dict(wgrad_no_multi='1')),
    ('BNF_WGRAD_ORDER=fwd', dict(wgrad_order_fwd='1')), ('BNF_WGRAD_ORDER=bwd', {}),
    ('BNF_RING_SPLITK=2', dict(ring_splitk='2')), ('BNF_RING_SPLITK=0', dict(ring_splitk='1')),   # max(1, atoi)
    ('BNF_PHASE_PROF=gemm_wgrad', dict(phase_prof='gemm_wgrad')),
]


def _switches(probe, *env):
  return dict(kv.split('=', 1) for kv in probe('switches', *env).split(' '))


def test_switch_defaults_for_an_empty_environment(probe):
  assert _switches(probe) == DEFAULTS


@pytest.mark.parametrize('env,changed', ALONE, ids=[e for e, _ in ALONE])
def test_each_switch_set_alone(probe, env, changed):
  assert _switches(probe, env) == {**DEFAULTS, **changed}


def test_the_engine_reads_the_environment_in_bnf_create_and_one_debug_call_only():
  """After bnf_create the library calls getenv in exactly one place: BNF_DEBUG_TN_KIND / BNF_DEBUG_TN_SPLITK, arguments
  of the debug call bnf_debug_gemm_tn.  Every unit of the library is read: the three reads are the engine unit's
  (bnf_api.hip), and the forecast and comm units have none."""
  csrc = os.path.join(ROOT, 'bayesnf_amd', 'csrc')
  units = sorted(n for n in os.listdir(csrc) if n.endswith(('.hip', '.cpp')))
  assert 'bnf_api.hip' in units and len(units) >= 3, units
  reads = [(name, l.strip()) for name in units for l in open(os.path.join(csrc, name)).read().split('\n')
           if 'getenv' in l and not l.strip().startswith('//')]
  assert len(reads) == 3, reads
  assert [name for name, _ in reads] == ['bnf_api.hip'] * 3, reads
  assert 'read_switches(getenv)' in reads[0][1]
  assert 'BNF_DEBUG_TN_KIND' in reads[1][1] and 'BNF_DEBUG_TN_SPLITK' in reads[2][1]
  for name in os.listdir(csrc):
    if name.endswith('.h') and name != 'bnf_plan.h':
      assert 'getenv' not in open(os.path.join(csrc, name)).read(), name
