"""CPU-only checks of how libbnf_hip.so is cut into units (bayesnf_amd/csrc: bnf_api.hip the training engine,
bnf_forecast.hip the forecast entry points, bnf_comm.* the RCCL loader).  Source text only: no GPU, no compiler.  The
forecast unit compiles no training kernel and cannot name a field of the handle; every entry point of include/bnf.h is
defined once; the Makefile knows every header and every unit."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'bayesnf_amd', 'csrc')
TRAINING_HEADERS = ('bnf_kernels.h', 'bnf_gemm.h', 'bnf_gemm8.h', 'bnf_panel.h', 'bnf_plan.h')


def _read(name):
  return open(os.path.join(CSRC, name)).read()


def _units():
  return sorted(n for n in os.listdir(CSRC) if n.endswith(('.hip', '.cpp')))


def _include_closure(name):
  """Base names of every file `name` reaches through #include "...", itself left out."""
  seen, todo = set(), [name]
  while todo:
    for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', _read(todo.pop()), flags=re.M):
      inc = os.path.basename(inc)
      if inc not in seen and os.path.exists(os.path.join(CSRC, inc)):
        todo.append(inc)
      seen.add(inc)
  return seen


def _makefile_words(var):
  return re.search(r'^%s\s*:=(.*)$' % var, _read('Makefile'), flags=re.M).group(1).split()


def test_the_units_are_the_engine_the_forecasts_and_the_comm_loader():
  units = _units()
  assert 'bnf_api.hip' in units and 'bnf_forecast.hip' in units, units
  assert [n for n in units if n.startswith('bnf_comm.')] and len(units) == 3, units


def test_the_forecast_unit_includes_no_training_header():
  closure = _include_closure('bnf_forecast.hip')
  assert 'bnf_quantiles.h' in closure and 'bnf_host.h' in closure and 'bnf_device.h' in closure, sorted(closure)
  assert not closure & set(TRAINING_HEADERS), sorted(closure & set(TRAINING_HEADERS))
  # and the engine unit does not compile the forecasts' quantile kernels a second time
  assert 'bnf_quantiles.h' not in _include_closure('bnf_api.hip')


def test_every_entry_point_of_the_header_is_defined_in_exactly_one_unit():
  header = open(os.path.join(ROOT, 'include', 'bnf.h')).read()
  header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
  header = re.sub(r'//[^\n]*', '', header)
  declared = set(re.findall(r'\b(bnf_[a-z0-9_]+)\s*\(', header))
  assert len(declared) > 60 and {'bnf_create', 'bnf_sample_envelope', 'bnf_allgather'} <= declared, len(declared)
  where = {}
  for unit in _units():
    for name in re.findall(r'^(?!static\b)[A-Za-z_][\w \*]*?\b(bnf_[a-z0-9_]+)\(', _read(unit), flags=re.M):
      where.setdefault(name, []).append(unit)
  for name in sorted(declared):
    assert len(where.get(name, [])) == 1, (name, where.get(name, []))
  assert not set(where) - declared, sorted(set(where) - declared)


def test_the_makefile_lists_every_header_and_every_unit():
  hdr = _makefile_words('HDR')
  for name in sorted(os.listdir(CSRC)):
    if name.endswith('.h'):
      assert name in hdr, name
  assert '../../include/bnf.h' in hdr
  for word in hdr:
    assert os.path.exists(os.path.join(CSRC, word)), word
  assert sorted(_makefile_words('SRC')) == _units()


def test_the_forecast_and_comm_units_cannot_reach_into_the_handle():
  """bnf_handle is an opaque type outside the engine unit: no `h->` to compile, and no definition of the struct."""
  for unit in _units():
    if unit == 'bnf_api.hip':
      assert re.search(r'^struct bnf_handle \{', _read(unit), flags=re.M)
      continue
    text = _read(unit)
    assert 'h->' not in text, unit
    assert not re.search(r'struct\s+bnf_handle\s*\{', text), unit
    assert not _include_closure(unit) & {'bnf_api.hip'}, unit
