#!/usr/bin/env python
"""Kernel-by-kernel comparison of two -save-temps device assemblies of the engine (scripts/build_variant.sh keeps them):
which kernels exist on one side only, and which of the common ones differ.  A kernel's text runs from its label to the
next kernel's and includes hipcc's resource comments (VGPRs, scratch, code length); function numbers in local labels
(BB<n>_, .Lfunc_end<n>) and the IR block names hipcc prints behind labels are masked: they are numbered per module and
shift when another kernel leaves the file.

  python scripts/isa_compare.py <parent.s> <child.s> [--mask-kernarg]

--mask-kernarg: also mask the literal offset of scalar loads (s_load_* ..., 0x<offset>) -- what moves when a field
leaves a kernel-argument struct -- and print the other differing lines of every kernel that still differs.
"""
import difflib
import re
import sys

from isa_report import demangle


def kernels(path, mask_kernarg):
  lines = open(path).read().split('\n')
  starts = [(i, m.group(1)) for i, l in enumerate(lines) for m in [re.match(r'^(_ZN3bnf\w+):', l)] if m]
  names = demangle([n for _, n in starts])
  out = {}
  for k, (i, _) in enumerate(starts):
    end = starts[k + 1][0] if k + 1 < len(starts) else len(lines)
    body, seen_info = [], False
    for l in lines[i:end]:
      if '__hip_cuid_' in l or (seen_info and re.match(r'^\s+(\.section\s+\.text\.|\.text$)', l)):
        break                                   # (the next function's directives; behind the last kernel the source hash)
      seen_info = seen_info or '.AMDGPU.csdata' in l
      l = re.sub(r'BB\d+_', 'BB_', l)
      l = re.sub(r'^(\.LBB_\d+:)\s+;', r'\1 ;', l)   # (the comment behind a label is padded to a column: by the masked digits)
      l = re.sub(r'\.L(func_begin|func_end|tmp)\d+', r'.L\1', l)
      l = re.sub(r'\s*; %[\w.]+$', '', l)      # (name of the IR block behind a label: numbered per module)
      if mask_kernarg and re.match(r'^\s+s_load_dword', l):
        l = re.sub(r'0x[0-9a-f]+', '0xNN', l)
      body.append(l)
    out[names[k]] = body
  return out


def code_len(body):
  for l in body:
    m = re.match(r'^; codeLenInByte = (\d+)', l.strip())
    if m:
      return int(m.group(1))
  return -1


def main(parent, child, mask_kernarg):
  a, b = kernels(parent, mask_kernarg), kernels(child, mask_kernarg)
  gone, new = sorted(set(a) - set(b)), sorted(set(b) - set(a))
  common = [n for n in a if n in b]
  differ = [n for n in common if a[n] != b[n]]
  print(f'kernels: parent {len(a)}, child {len(b)}, compared {len(common)}, removed {len(gone)}, added {len(new)}, '
        f'{len(differ)} differ')
  for n in gone:
    print('  removed:', n.split('(')[0])
  for n in new:
    print('  added:', n.split('(')[0])
  for n in differ:
    d = [l for l in difflib.unified_diff(a[n], b[n], lineterm='', n=0) if l[:1] in '+-' and l[:3] not in ('+++', '---')]
    print(f'  differs: {n.split("(")[0]}: code bytes {code_len(a[n])} -> {code_len(b[n])}, {len(d)} changed lines')
    if mask_kernarg:
      for l in d[:80]:
        print('    ' + l)
  return 1 if differ or new else 0


if __name__ == '__main__':
  args = [x for x in sys.argv[1:] if not x.startswith('--')]
  sys.exit(main(args[0], args[1], '--mask-kernarg' in sys.argv))
