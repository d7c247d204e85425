"""StepPlan::featbwd_in_wgrad (bayesnf_amd/csrc/bnf_plan.h), asserted on the host the way tests/test_step_plan_host.py
asserts the weight-gradient plans: g++ compiles a small program around the header and the tests read what it prints.

The flag moves the fused featurisation backward from the last phase of the panel kernel into the layer-0 weight-gradient
kernel.  It is on only where that kernel is the 64 x 512 row stream on bf16 operands, the panel kernel's fused
featurisation backward is on, and the model's Fourier columns fit the kernel's 32 slots; BNF_FEATBWD_WGRAD=0 turns it off."""
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
// probe bf16 fp8 panel W Fp n_fourier fused [NAME=VALUE ...]
int main(int argc, char** argv) {
  for (int i = 8; i < argc; ++i) {
    const std::string a = argv[i];
    g_env[a.substr(0, a.find('='))] = a.substr(a.find('=') + 1);
  }
  const Switches sw = read_switches(lookup);
  PlanShape ps{};
  ps.bf16 = atoi(argv[1]); ps.fp8 = atoi(argv[2]); ps.panel = atoi(argv[3]); ps.W = atoi(argv[4]); ps.Fp = atoi(argv[5]);
  ps.n_fourier = atoi(argv[6]); ps.featbwd_fused = atoi(argv[7]);
  ps.L = 2; ps.Bp = 1024; ps.F = ps.Fp == 64 ? 49 : 105; ps.num_cus = 256;
  int32_t at = 0;
  for (int l = 0; l < ps.L; ++l) { ps.off_kernel[l] = at + 5; at += 5 + ((l == 0) ? ps.F : ps.W) * ps.W + ps.W; }
  const StepPlan p = make_step_plan(ps, sw, 3, false);
  const char* kind[] = {"TN128", "TN256", "RING", "SKINNY"};
  printf("featbwd_wgrad=%d l0=%s featbwd_in_wgrad=%d\n", (int)sw.featbwd_wgrad, kind[p.layer[0].kind], (int)p.featbwd_in_wgrad);
  return 0;
}
'''


@pytest.fixture(scope='module')
def probe(tmp_path_factory):
  d = tmp_path_factory.mktemp('featbwd_plan')
  src, exe = d / 'probe.cc', d / 'probe'
  src.write_text(PROBE)
  subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'bayesnf_amd', 'csrc'),
                         str(src), '-o', str(exe)])
  return lambda *args: subprocess.check_output([str(exe)] + [str(a) for a in args]).decode().strip()


def _flag(probe, bf16=1, fp8=0, panel=1, W=512, Fp=64, n_fourier=30, fused=1, env=()):
  out = probe(bf16, fp8, panel, W, Fp, n_fourier, fused, *env)
  return int(out.rsplit('=', 1)[1]), out


def test_on_for_the_benchmark_shape(probe):
  for kw in (dict(), dict(n_fourier=32), dict(n_fourier=0), dict(W=1024), dict(env=('BNF_FEATBWD_WGRAD=1',))):
    on, out = _flag(probe, **kw)
    assert on == 1 and 'l0=SKINNY' in out, (kw, out)


@pytest.mark.parametrize('kw', [
    dict(n_fourier=33),                        # more Fourier columns than slots
    dict(Fp=128),                              # the layer-0 weight gradient is not the 64-row stream
    dict(W=256),
    dict(env=('BNF_WGRAD_SKINNY=0',)),
    dict(env=('BNF_PANEL_FEATBWD=0',)),        # the separate k_feat_bwd reads dH0^T: the panel kernel must write it
    dict(fused=0),                             # no column table (no raw-input group)
    dict(env=('BNF_FEATBWD_WGRAD=0',)),
    dict(bf16=0),                              # f32
    dict(fp8=1),                               # dZ_0 leaves the panel kernel as e5m2
    dict(panel=0),
], ids=lambda kw: ','.join(f'{k}={v}' for k, v in kw.items()))
def test_off(probe, kw):
  on, out = _flag(probe, **kw)
  assert on == 0, out


def test_the_switch_is_read_once_with_the_others(probe):
  assert _flag(probe)[1].startswith('featbwd_wgrad=1')
  assert _flag(probe, env=('BNF_FEATBWD_WGRAD=0',))[1].startswith('featbwd_wgrad=0')
