#!/usr/bin/env python
"""Are the kernels two builds share the same, instruction for instruction?

  python tools/compare_kernel_asm.py BEFORE AFTER [--expect-new PREFIX]

BEFORE / AFTER: two builds of the product's device code - the assembly `make -C gym_solo_amd/csrc asm` writes
(solo_engine.gfx950.s), or a library (libsolo_hip.so), whose gfx950 code objects are disassembled with the ROCm LLVM tools.
Per kernel the instruction streams are compared after dropping comments, directives and blank lines and renumbering local
labels by first appearance (a function's label numbers move when functions are added in front of it); for a library, branch
targets are compared as offsets from the kernel's start.  Prints one line per kernel and a summary; exit status 1 when a
shared kernel differs or one is missing from AFTER.  --expect-new: kernels only in AFTER must start with this demangled name."""
import argparse
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get('ROCM_LLVM_BIN', '/opt/rocm/llvm/bin')


def demangle(names):
  tool = shutil.which('llvm-cxxfilt', path=LLVM) or shutil.which('llvm-cxxfilt') or shutil.which('c++filt')
  if tool is None or not names:
    return {n: n for n in names}
  out = subprocess.run([tool] + list(names), stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.split('\n')
  return dict(zip(names, out))


def kernels_of_asm(text):
  """{symbol: [normalised instruction lines]} of an assembly listing"""
  out = {}
  for m in re.finditer(r'^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:', text, re.S | re.M):
    name, body = m.group(1), m.group(2)
    if name.startswith('.') or name.startswith('__hip_cuid'):
      continue
    labels, lines = {}, []
    for line in body.split('\n'):
      line = line.split(';')[0].rstrip()
      lab = re.match(r'^(\.L\w+):$', line)
      if lab:
        lines.append('<label %s>' % lab.group(1))
        continue
      if not re.match(r'^\s+[a-z]\w+', line) or line.strip().startswith('.'):
        continue
      lines.append(' '.join(line.split()))
    def local(mm):
      return 'L%d' % labels.setdefault(mm.group(0), len(labels))
    # (labels numbered by first appearance, in the order of the normalised stream)
    out[name] = [re.sub(r'\.L\w+', local, l) for l in lines]
  return out


def kernels_of_library(path):
  """the same of a library's gfx950 code objects (disassembled; addresses relative to each function's start)"""
  out = {}
  with tempfile.TemporaryDirectory() as tmp:
    lib = os.path.join(tmp, 'lib.so')
    with open(path, 'rb') as f, open(lib, 'wb') as g:
      g.write(f.read())
    subprocess.run([os.path.join(LLVM, 'clang-offload-bundler'), '--list', '--type=o', '--input=' + lib], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '--offloading', lib], cwd=tmp, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True)
    for co in sorted(glob.glob(os.path.join(tmp, '*gfx950*'))):
      text = subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '-d', '--no-show-raw-insn', co], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
      cur, base, since_getpc = None, 0, 99
      for line in text.split('\n'):
        m = re.match(r'^([0-9a-f]+) <(\S+)>:$', line)
        if m:
          cur, base = m.group(2), int(m.group(1), 16)
          out[cur] = []
          continue
        m = re.match(r'^\s+(\S.*?)\s*//\s*([0-9A-Fa-f]+):', line)
        if m and cur is not None:
          ins = ' '.join(m.group(1).split())
          ins = re.sub(r'<[^>]*\+0x([0-9a-f]+)>', lambda mm: '<+%d>' % int(mm.group(1), 16), ins)   # (branch targets: symbol + offset)
          ins = re.sub(r'\b\d+ <', '<', ins)
          # (a pc-relative address - s_getpc_b64, then the distance to the data added to the pair: the distance moves with the
          # code in front of the data, the instructions do not)
          if ins.startswith('s_getpc_b64'):
            since_getpc = 0
          elif since_getpc < 4:
            since_getpc += 1
            if re.match(r's_addc?_u32 ', ins):
              ins = re.sub(r'0x[0-9a-f]{5,8}$', '<pcrel>', ins)
          out[cur].append(ins)
  return {k: v for k, v in out.items() if v}


def load(path):
  if path.endswith('.s'):
    return kernels_of_asm(open(path).read())
  return kernels_of_library(path)


def main():
  ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument('before')
  ap.add_argument('after')
  ap.add_argument('--expect-new', default=None)
  a = ap.parse_args()
  before, after = load(a.before), load(a.after)
  names = demangle(sorted(set(before) | set(after)))
  same = differ = missing = new = bad_new = 0
  for sym in sorted(names, key=lambda s: names[s]):
    nice = names[sym]
    if sym not in after:
      missing += 1
      print('MISSING    %6d -> ------  %s' % (len(before[sym]), nice))
    elif sym not in before:
      new += 1
      ok = a.expect_new is None or nice.replace('void ', '').startswith(a.expect_new)
      bad_new += not ok
      print('%s ------ -> %6d  %s' % ('NEW       ' if ok else 'UNEXPECTED', len(after[sym]), nice))
    elif before[sym] == after[sym]:
      same += 1
      print('identical  %6d == %6d  %s' % (len(before[sym]), len(after[sym]), nice))
    else:
      differ += 1
      first = next((i for i, (x, y) in enumerate(zip(before[sym], after[sym])) if x != y), min(len(before[sym]), len(after[sym])))
      print('DIFFERENT  %6d != %6d  %s  (first difference at instruction %d)' % (len(before[sym]), len(after[sym]), nice, first))
  print('summary: %d shared kernels identical, %d different, %d missing, %d new (%d unexpected)' % (same, differ, missing, new, bad_new))
  return 1 if differ or missing or bad_new else 0


if __name__ == '__main__':
  sys.exit(main())
