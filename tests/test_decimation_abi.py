"""Control decimation at the C boundary (no GPU): the two entry points are declared in include/solo_engine.h, mirrored in
gym_solo_amd/abi.py and exported by the library; the ABI version stays 7 and no struct of the boundary changed."""
import ctypes as C
import os
import re

from gym_solo_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'solo_engine.h')
LIB = os.path.join(ROOT, 'gym_solo_amd', 'csrc', 'libsolo_hip.so')


def _header():
  return re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)


def test_entry_points_are_declared_and_mirrored():
  text = _header()
  assert re.search(r'int\s+solo_engine_set_decimation\s*\(\s*SoloEngine\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*\)\s*;', text)
  assert re.search(r'int\s+solo_engine_get_decimation\s*\(\s*SoloEngine\s*\*\s*\w+\s*,\s*int32_t\s*\*\s*\w+\s*\)\s*;', text)
  assert abi.ENTRY_POINTS['solo_engine_set_decimation'] == (C.c_int, [C.c_void_p, C.c_int32])
  assert abi.ENTRY_POINTS['solo_engine_get_decimation'] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)])
  assert re.search(r'#define\s+SOLO_MAX_DECIMATION\s+64\b', text)
  assert re.search(r'#define\s+SOLO_ABI_VERSION\s+7\b', text) and abi.ABI_VERSION == 7


def test_library_exports_them_and_rejects_a_null_engine():
  if not os.path.exists(LIB):
    import subprocess
    subprocess.check_call(['make', '-s', '-C', os.path.dirname(LIB)])
  lib = abi.bind(C.CDLL(LIB))
  assert lib.solo_abi_version() == 7
  d = C.c_int32(-5)
  assert lib.solo_engine_set_decimation(None, 2) == abi.ERR_INVALID_ARG
  assert lib.solo_engine_get_decimation(None, C.byref(d)) == abi.ERR_INVALID_ARG and d.value == -5


def test_engine_wrapper_has_the_setter_and_the_property():
  from gym_solo_amd.engine import Engine
  assert callable(Engine.set_decimation) and isinstance(Engine.decimation, property)
  assert 'decimation' not in Engine._CHECKPOINT   # (configuration, not state: checkpoints are unchanged)
  assert Engine.CHECKPOINT_VERSION == 2
