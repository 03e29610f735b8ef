"""The joint-control part of the C-ABI (ABI 7): SoloControl's layout in the header equals the ctypes mirror, the entry
points are exported, and the version is 7 on both sides."""
import ctypes as C
import os
import subprocess
import tempfile

from gym_solo_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'gym_solo_amd', 'csrc', 'libsolo_hip.so')


def _compile_and_run(lines):
  with tempfile.TemporaryDirectory() as d:
    open(os.path.join(d, 't.c'), 'w').write('\n'.join(lines) + '\n')
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), '-o', os.path.join(d, 't'), os.path.join(d, 't.c')])
    return [int(x) for x in subprocess.check_output([os.path.join(d, 't')]).split()]


def test_solo_control_layout_matches_header():
  lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "solo_engine.h"', 'int main(){',
           'printf("%zu\\n", sizeof(SoloControl));']
  want = [C.sizeof(abi.SoloControl)]
  for name, *_ in abi.SoloControl._fields_:
    lines.append('printf("%%zu\\n", offsetof(SoloControl, %s));' % name)
    want.append(getattr(abi.SoloControl, name).offset)
  lines += ['printf("%d %d %d %d\\n", SOLO_CTRL_POSITION, SOLO_CTRL_TORQUE, SOLO_CTRL_PD, SOLO_ABI_VERSION);', 'return 0;}']
  got = _compile_and_run(lines)
  assert got[:len(want)] == want
  assert got[len(want):] == [abi.CTRL_POSITION, abi.CTRL_TORQUE, abi.CTRL_PD, abi.ABI_VERSION]
  assert C.sizeof(abi.SoloControl) == 8 + 16 * 8 + 8


def test_version_and_exports():
  assert abi.ABI_VERSION == 7
  lib = C.CDLL(LIB)
  for name in ('solo_engine_set_control', 'solo_engine_get_control'):
    assert hasattr(lib, name), name
    assert name in abi.ENTRY_POINTS
  lib.solo_abi_version.restype = C.c_int
  assert lib.solo_abi_version() == 7


def test_set_control_rejects_null_arguments_without_a_device():
  lib = abi.bind(C.CDLL(LIB))
  c = abi.SoloControl()
  assert lib.solo_engine_set_control(None, C.byref(c), None) == abi.ERR_INVALID_ARG
  assert lib.solo_engine_get_control(None, C.byref(c)) == abi.ERR_INVALID_ARG
