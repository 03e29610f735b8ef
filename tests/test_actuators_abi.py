"""The actuator block at the C boundary, without a GPU: the constants of include/solo_engine.h against gym_solo_amd.abi, the two
entry points in the header, the ctypes table and the library, the ABI version and the structs untouched, and the checks of
solo_engine_set_actuators (solo_launch.h: validate_actuators, actuators_conflict) through the emulator harness."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gym_solo_amd import abi
from helpers import make_abi
import emu_actuator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'solo_engine.h')).read()


def _define(name):
  return int(re.search(r'^#define %s (\d+)' % name, HEADER, re.M).group(1))


def test_constants_match_the_header():
  assert _define('SOLO_ACTUATOR_WIDTH') == abi.ACTUATOR_WIDTH == 4
  assert _define('SOLO_ACT_TORQUE_LIMIT') == abi.ACT_TORQUE_LIMIT == 0
  assert _define('SOLO_ACT_KP') == abi.ACT_KP == 1
  assert _define('SOLO_ACT_KD') == abi.ACT_KD == 2
  assert _define('SOLO_ABI_VERSION') == abi.ABI_VERSION == 7   # (no struct changed: the version stays)


def test_entry_points():
  assert abi.ENTRY_POINTS['solo_engine_set_actuators'] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p])
  assert abi.ENTRY_POINTS['solo_engine_get_actuators'] == (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)])
  assert re.search(r'int solo_engine_set_actuators\(SoloEngine\* eng, const void\* per_env_dev, void\* stream\);', HEADER)
  assert re.search(r'int solo_engine_get_actuators\(SoloEngine\* eng, void\*\* dev\);', HEADER)
  from gym_solo_amd.engine import load_library
  lib = load_library()
  # (a NULL handle is an invalid argument, not a crash)
  assert lib.solo_engine_set_actuators(None, None, None) == abi.ERR_INVALID_ARG
  p = C.c_void_p()
  assert lib.solo_engine_get_actuators(None, C.byref(p)) == abi.ERR_INVALID_ARG


@pytest.fixture(scope='module')
def lib():
  return emu_actuator.load()


def _validate(lib, table, dtype):
  msg = C.create_string_buffer(200)
  t = np.ascontiguousarray(table, dtype=np.float64)
  rc = lib.solo_emu_act_validate(t.ctypes.data, t.shape[0], abi.F32 if dtype == 'float32' else abi.F64, msg, 200)
  return rc, msg.value.decode()


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_table_validation(lib, dtype):
  good = np.random.default_rng(0).uniform(0.0, 3.0, (16, abi.ACTUATOR_WIDTH))
  good[5] = 0.0   # (dead motors, zero gains: legal)
  assert _validate(lib, good, dtype) == (abi.OK, '')
  for bad in (np.nan, -1.0, np.inf, -np.inf, -1e-30):
    for col in range(abi.ACTUATOR_WIDTH):   # (the reserved column is held to the same rule)
      t = good.copy()
      t[11, col] = bad
      rc, msg = _validate(lib, t, dtype)
      assert rc == abi.ERR_INVALID_ARG and 'finite and >= 0' in msg and 'robot 11, column %d' % col in msg, (bad, col, msg)
  if dtype == 'float32':   # (what overflows the engine's precision is not finite there)
    t = good.copy()
    t[0, 0] = 1e39
    assert _validate(lib, t, dtype)[0] == abi.ERR_INVALID_ARG
    assert _validate(lib, t, 'float64')[0] == abi.OK


def test_conflicts_name_the_option(lib):
  def conflict(sensing=0, **kw):
    warm = kw.pop('solver_warm_start', 0.0)   # (the host configuration refuses it without the threshold: set on the struct)
    ca, _ = make_abi('float64', **kw)
    ca.solver_warm_start = warm
    msg = C.create_string_buffer(200)
    return lib.solo_emu_act_conflict(C.byref(ca), sensing, msg, 200), msg.value.decode()
  assert conflict() == (abi.OK, '')
  assert conflict(migrate_steps=0) == (abi.OK, '') and conflict(migrate_steps=abi.AUTO) == (abi.OK, '')
  for kw, word in ((dict(migrate_steps=5), 'migrate_steps'), (dict(solver_residual_threshold=1e-7), 'solver_residual_threshold'),
                   (dict(solver_warm_start=0.5), 'solver_warm_start'), (dict(sensing=1), 'contact sensing')):
    rc, msg = conflict(**kw)
    assert rc == abi.ERR_INVALID_ARG and word in msg and msg.startswith('actuator randomisation does not support'), (kw, msg)
