"""The base wrench block at the C boundary, without a GPU: the constants of include/solo_engine.h against gym_solo_amd.abi, the two
entry points in the header, the ctypes table and the library, the ABI version untouched, KParams' members where they were (through
the emulator harness), and the checks of solo_engine_set_base_wrench (solo_launch.h: validate_base_wrench, base_wrench_conflict)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gym_solo_amd import abi
from helpers import make_abi
import emu_push

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'solo_engine.h')).read()


def _define(name):
  return int(re.search(r'^#define %s (\d+)' % name, HEADER, re.M).group(1))


def test_constants_match_the_header():
  assert _define('SOLO_WRENCH_WIDTH') == abi.WRENCH_WIDTH == 8
  assert _define('SOLO_WRENCH_FORCE') == abi.WRENCH_FORCE == 0
  assert _define('SOLO_WRENCH_TORQUE') == abi.WRENCH_TORQUE == 3
  assert _define('SOLO_ABI_VERSION') == abi.ABI_VERSION == 7   # (no struct changed: the version stays)


def test_entry_points():
  assert abi.ENTRY_POINTS['solo_engine_set_base_wrench'] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p])
  assert abi.ENTRY_POINTS['solo_engine_get_base_wrench'] == (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)])
  assert re.search(r'int solo_engine_set_base_wrench\(SoloEngine\* eng, const void\* per_env_dev, void\* stream\);', HEADER)
  assert re.search(r'int solo_engine_get_base_wrench\(SoloEngine\* eng, void\*\* dev\);', HEADER)
  from gym_solo_amd.engine import load_library
  lib = load_library()
  # (the library exports them; a NULL handle is an invalid argument, not a crash)
  assert lib.solo_engine_set_base_wrench(None, None, None) == abi.ERR_INVALID_ARG
  p = C.c_void_p()
  assert lib.solo_engine_get_base_wrench(None, C.byref(p)) == abi.ERR_INVALID_ARG


@pytest.fixture(scope='module')
def lib():
  return emu_push.load()


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_kparams_members_in_front_of_wrench_are_where_they_were(lib, dtype):
  """KParams<T> from CtlConst on, restated as a ctypes struct of the members as they were BEFORE `wrench` was appended (the C
  layout rules are ctypes'): every offset the harness measures equals the mirror's, `wrench` sits behind `actuators`, and the
  struct ends with it"""
  real = C.c_float if dtype == 'float32' else C.c_double

  class CtlConst(C.Structure):
    _fields_ = [('mode', C.c_int32), ('pad', C.c_int32), ('kp', real * abi.NUM_DOF), ('kd', real * abi.NUM_DOF), ('action_scale', real),
                ('torque_limit', real), ('reset_cmd', real * abi.NUM_JOINTS)]

  class Tail(C.Structure):
    _fields_ = [('mu_base', real), ('ctl', CtlConst), ('contact', C.c_void_p), ('contact_traj', C.c_void_p), ('contact_traj_steps', C.c_int32),
                ('decimation', C.c_int32), ('term_value', real * abi.MAX_TERMS), ('term_fired', C.c_void_p), ('actuators', C.c_void_p)]

  got = emu_push.kparams_offsets(lib, dtype)
  base = got['mu_base']
  assert base % 8 == 0     # (the mirror starts on the struct's alignment)
  for name, _ in Tail._fields_:
    assert got[name] - base == getattr(Tail, name).offset, name
  assert got['wrench'] == got['actuators'] + 8 and got['sizeof'] == got['wrench'] + 8
  assert got['sizeof'] - base == C.sizeof(Tail) + 8


def _validate(lib, table, dtype):
  msg = C.create_string_buffer(200)
  t = np.ascontiguousarray(table, dtype=np.float64)
  rc = lib.solo_emu_push_validate(t.ctypes.data, t.shape[0], abi.F32 if dtype == 'float32' else abi.F64, msg, 200)
  return rc, msg.value.decode()


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_table_validation(lib, dtype):
  good = np.random.default_rng(0).uniform(-300.0, 300.0, (16, abi.WRENCH_WIDTH))
  good[5] = 0.0
  good[6] = -1e30     # (negative values and zero are legal)
  assert _validate(lib, good, dtype) == (abi.OK, '')
  for bad in (np.nan, np.inf, -np.inf):
    for col in range(abi.WRENCH_WIDTH):   # (the reserved columns are held to the same rule)
      t = good.copy()
      t[11, col] = bad
      rc, msg = _validate(lib, t, dtype)
      assert rc == abi.ERR_INVALID_ARG and 'finite' in msg and 'robot 11, column %d' % col in msg, (bad, col, msg)
  for big in (1e39, -1e39):   # (what overflows the engine's precision is not finite there)
    t = good.copy()
    t[0, 0] = big
    assert _validate(lib, t, 'float32')[0] == abi.ERR_INVALID_ARG
    assert _validate(lib, t, 'float64')[0] == abi.OK


def test_conflicts_name_the_option(lib):
  def conflict(sensing=0, **kw):
    warm = kw.pop('solver_warm_start', 0.0)   # (the host configuration refuses it without the threshold: set on the struct)
    ca, _ = make_abi('float64', **kw)
    ca.solver_warm_start = warm
    msg = C.create_string_buffer(200)
    return lib.solo_emu_push_conflict(C.byref(ca), sensing, msg, 200), msg.value.decode()
  assert conflict() == (abi.OK, '')
  assert conflict(migrate_steps=0) == (abi.OK, '') and conflict(migrate_steps=abi.AUTO) == (abi.OK, '')
  for kw, word in ((dict(migrate_steps=5), 'migrate_steps'), (dict(solver_residual_threshold=1e-7), 'solver_residual_threshold'),
                   (dict(solver_warm_start=0.5), 'solver_warm_start'), (dict(sensing=1), 'contact sensing')):
    rc, msg = conflict(**kw)
    assert rc == abi.ERR_INVALID_ARG and word in msg and msg.startswith('base wrenches do not support'), (kw, msg)
