"""`bnf_workspace_bytes` for every configuration of tests/test_pipeline_plan_host.py that creates a handle, held to the
sizes recorded (tests/golden/workspace_bytes.json) from the build before the pipeline plan moved into bnf_plan.h.  The
workspace layout (`carve` in bnf_api.hip) reads nearly every field of the plan -- panel, h0l, fuse_last, recompute_a0, q8,
c8, the padded batch, whether the column table exists -- so a plan that changes changes these numbers.

Scaled to 3 members, 300 rows, full batch; MAP, and VI with 2 samples.  Handles are created and destroyed only: no
kernel runs.  The features are 3 raw inputs, the case's Fourier columns, seasonal columns up to the count (their number
sizes the seasonal table, a part of the workspace) and one interaction where it is odd; "no input group" relabels the raw-input group in the config the way no NetSpec can."""
import ctypes as C
import json
import os

import pytest

from tests.test_pipeline_plan_host import CASES, DEFAULT, EXPECTED

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'workspace_bytes.json')
DTYPES = {0: 'fp32', 1: 'bf16', 2: 'fp8', 3: 'fp32_split'}
CREATED = [name for name in CASES if not EXPECTED[name].startswith('refused')]


def net_for(F, width, depth, nfourier):
  """3 raw inputs, `nfourier` Fourier columns dealt over them, seasonal columns up to F, one interaction where F is odd"""
  from bayesnf_amd.spec import NetSpec
  deg = nfourier // 2
  degrees = [(deg + 2 - d) // 3 for d in range(3)]      # 20 columns: 4 + 3 + 3; 30: 5 + 5 + 5; 34: 6 + 6 + 5
  rest = F - 3 - 2 * sum(degrees)
  assert rest >= 2 and 2 * sum(degrees) == nfourier
  return NetSpec(width=width, depth=depth, input_scales=[100.0, 1.0, 1.0], fourier_degrees=degrees,
                 interactions=[[0, 1]] * (rest % 2), seasonality_periods=[365.25], num_seasonal_harmonics=[rest // 2])


def create(name, mode, monkeypatch):
  """bnf_create for a case -> (return code, handle)"""
  from bayesnf_amd import _native
  c = {**DEFAULT, **CASES[name]}
  for kv in c['env']:
    monkeypatch.setenv(*kv.split('=', 1))
  net = net_for(c['F'], c['Wt'], c['L'], c['nfourier'])
  assert net.F == c['F'] and 2 * int(sum(net.fourier_degrees)) == c['nfourier']
  cfg = _native.make_config(net, device=0, dtype=DTYPES[c['dtype']], mode=_native.MODE_VI if mode == 'vi' else _native.MODE_MAP,
                            n_rows=300, batch=300, members=3, member_offset=0, seed=0, kl_weight=0.2,
                            vi_samples=2 if mode == 'vi' else 1, forward_only=bool(c['fo']), pipeline=c['pipeline'])
  if not c['ingroup']:
    assert cfg.group_kind[0] == 0
    cfg.group_kind[0] = 2   # BNF_GROUP_SEASONAL: nothing is a raw-input group any more
  handle = C.c_void_p()
  return _native.load().bnf_create(C.byref(cfg), C.byref(handle)), handle


def workspace_bytes(name, mode, monkeypatch):
  from bayesnf_amd import _native
  rc, handle = create(name, mode, monkeypatch)
  _native.check(rc, 'bnf_create')
  n = int(_native.load().bnf_workspace_bytes(handle))
  _native.load().bnf_destroy(handle)
  return n


@pytest.mark.parametrize('mode', ['map', 'vi'])
@pytest.mark.parametrize('name', CREATED)
def test_workspace_bytes_are_the_recorded_ones(name, mode, monkeypatch):
  want = json.load(open(GOLDEN))[name][mode]
  assert workspace_bytes(name, mode, monkeypatch) == want


# the three BNF_ERR_INVALID returns the pipeline plan reports as an enum: bnf_create's messages, word for word
REFUSALS = {
    'refused=1': 'pipeline 2 (0 auto, 1 layers, 3 panel)',
    'refused=2': 'panel pipeline needs a bf16 training handle with depth >= 2, width 256/512/1024 and <= 128 features',
    'refused=3': 'dtype fp8 (fp8 operand storage for the weight gradients) needs the row-panel pipeline: '
                 'depth >= 2, width 256 / 512 / 1024 after padding to 64, <= 128 padded features',
}


@pytest.mark.parametrize('name', [name for name in CASES if EXPECTED[name].startswith('refused')])
def test_refused_configurations_keep_their_messages(name, monkeypatch):
  from bayesnf_amd import _native
  rc, handle = create(name, 'map', monkeypatch)
  assert rc == -1 and not handle.value        # BNF_ERR_INVALID
  assert _native.last_error() == REFUSALS[EXPECTED[name]]
