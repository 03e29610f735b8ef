"""State terminations at the C boundary (no GPU): the two kinds and the two entry points are declared in include/solo_engine.h,
mirrored in gym_solo_amd/abi.py and exported by the library; the ABI version stays 7 and every struct of the boundary keeps its
layout (the changes are append-only); pack_program accepts the new kinds and rejects a negative grace count; the thresholds
default to 0."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gym_solo_amd import abi
import emu_terms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'solo_engine.h')
LIB = os.path.join(ROOT, 'gym_solo_amd', 'csrc', 'libsolo_hip.so')


def _header():
  return re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)


def test_kinds_and_entry_points_are_declared_and_mirrored():
  text = _header()
  enum = re.search(r'typedef enum SoloTermKind \{(.*?)\} SoloTermKind;', text, re.S).group(1)
  kinds = dict((m.group(1), int(m.group(2))) for m in re.finditer(r'(SOLO_T_\w+)\s*=\s*(\d+)', enum))
  assert kinds == {'SOLO_T_PERPETUAL': 0, 'SOLO_T_TIME': 1, 'SOLO_T_CONST': 2, 'SOLO_T_HEIGHT_BELOW': 3, 'SOLO_T_TILT_ABOVE': 4}
  assert (abi.T_PERPETUAL, abi.T_TIME, abi.T_CONST, abi.T_HEIGHT_BELOW, abi.T_TILT_ABOVE) == (0, 1, 2, 3, 4)
  assert re.search(r'int\s+solo_engine_set_term_values\s*\(\s*SoloEngine\s*\*\s*\w+\s*,\s*const\s+double\s+\w+\s*\[\s*SOLO_MAX_TERMS\s*\]\s*\)\s*;', text)
  assert re.search(r'int\s+solo_engine_get_term_fired\s*\(\s*SoloEngine\s*\*\s*\w+\s*,\s*void\s*\*\*\s*\w+\s*\)\s*;', text)
  assert abi.ENTRY_POINTS['solo_engine_set_term_values'] == (C.c_int, [C.c_void_p, C.POINTER(C.c_double)])
  assert abi.ENTRY_POINTS['solo_engine_get_term_fired'] == (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)])
  assert re.search(r'#define\s+SOLO_ABI_VERSION\s+7\b', text) and abi.ABI_VERSION == 7
  assert re.search(r'#define\s+SOLO_MAX_TERMS\s+4\b', text) and abi.MAX_TERMS == 4


def test_layouts_are_append_only():
  """the structs of the boundary are what they were: sizes and the offsets of their last members (ctypes mirrors, which
  tests/test_abi.py ties to the header)"""
  assert C.sizeof(abi.SoloProgram) == 16 + abi.MAX_OBS * 48 + abi.MAX_REWARD_OPS * 32 + 2 * 4 * abi.MAX_TERMS
  assert abi.SoloProgram.term_kind.offset == C.sizeof(abi.SoloProgram) - 32 and abi.SoloProgram.term_param.offset == C.sizeof(abi.SoloProgram) - 16
  assert [n for n, _ in abi.SoloStateView._fields_] == ['num_envs', 'dtype', 'state_stride', 'obs_dim', 'state', 'snapshot', 'targets', 'obs',
                                                         'reward', 'done', 'term_count', 'params', 'stats', 'cost', 'warm']
  assert C.sizeof(abi.SoloStateView) == 16 + 11 * 8
  assert [n for n, _ in abi.SoloConfig._fields_][-3:] == ['reserved0', 'solver_warm_start', 'base_lateral_friction']
  text = _header()
  view = re.search(r'typedef struct SoloStateView \{(.*?)\} SoloStateView;', text, re.S).group(1)
  assert re.findall(r'(\w+)\s*;', view) == [n for n, _ in abi.SoloStateView._fields_]
  prog = re.search(r'typedef struct SoloProgram \{(.*?)\} SoloProgram;', text, re.S).group(1)
  assert re.findall(r'(\w+)(?:\[\w+\])?\s*;', prog) == [n for n, _ in abi.SoloProgram._fields_]


def test_library_exports_them_and_rejects_a_null_engine():
  if not os.path.exists(LIB):
    import subprocess
    subprocess.check_call(['make', '-s', '-C', os.path.dirname(LIB)])
  lib = abi.bind(C.CDLL(LIB))
  assert lib.solo_abi_version() == 7
  values = (C.c_double * abi.MAX_TERMS)(0.1, 0.2, 0.3, 0.4)
  p = C.c_void_p(5)
  assert lib.solo_engine_set_term_values(None, values) == abi.ERR_INVALID_ARG
  assert lib.solo_engine_get_term_fired(None, C.byref(p)) == abi.ERR_INVALID_ARG and p.value == 5


def _validate(prog):
  msg = C.create_string_buffer(160)
  return emu_terms.load().solo_emu_terms_validate(C.byref(prog), msg, 160), msg.value.decode()


def test_validate_accepts_the_new_kinds_and_rejects_a_negative_grace_count():
  p = abi.SoloProgram()
  p.num_terms = 4
  for t, (kind, param) in enumerate([(abi.T_HEIGHT_BELOW, 0), (abi.T_TILT_ABOVE, 120), (abi.T_TIME, 7), (abi.T_PERPETUAL, 0)]):
    p.term_kind[t], p.term_param[t] = kind, param
  assert _validate(p) == (abi.OK, '')
  for kind in abi.STATE_TERM_KINDS:
    p.term_kind[0], p.term_param[0] = kind, -1
    rc, msg = _validate(p)
    assert rc == abi.ERR_INVALID_ARG and 'grace' in msg
    p.term_param[0] = 0
  # (the other kinds keep their rules: a TimeBased limit may be negative - it then fires on the first tick -, kind 5 does not exist)
  p.term_kind[0], p.term_param[0] = abi.T_TIME, -1
  assert _validate(p)[0] == abi.OK
  p.term_kind[0] = 5
  assert _validate(p) == (abi.ERR_INVALID_ARG, 'bad termination kind')
  p.term_kind[0] = -1
  assert _validate(p)[0] == abi.ERR_INVALID_ARG
  # a slot beyond num_terms is not looked at
  p.term_kind[0], p.term_param[0], p.num_terms = abi.T_HEIGHT_BELOW, 0, 1
  p.term_kind[1], p.term_param[1] = abi.T_TILT_ABOVE, -3
  assert _validate(p)[0] == abi.OK


def test_default_thresholds_are_zero():
  """an engine that never called set_term_values compares with 0: on the emulator, a height termination with no values given
  fires for a robot below z = 0 only, a tilt termination for one tilted by more than 90 degrees only"""
  from helpers import make_abi
  from test_emu_terms import program, snapshot
  ca, ma = make_abi('float64', settle_steps=40)
  snap = snapshot('float64', 1)
  snap[1, abi.S_POS + 2] = -0.25                                   # robot 1 under the plane z = 0 ...
  snap[2, abi.S_QUAT:abi.S_QUAT + 4] = [np.sin(1.0), 0, 0, np.cos(1.0)]   # ... robot 2 rolled by 2 rad: c = cos 2 < 0
  s = emu_terms.TermsSim(emu_terms.load(), ca, ma, 3, program([(abi.T_HEIGHT_BELOW, 0), (abi.T_TILT_ABOVE, 0)]), snap, None)
  assert not s.values.any()
  s.step(None, abi.STEP_DONE)
  np.testing.assert_array_equal(s.term_fired, [0, 1, 2])
  np.testing.assert_array_equal(s.done, [0, 1, 1])
  with pytest.raises(ValueError):
    emu_terms.make_emu_terms_engine_class()(ca, ma, 1).set_term_values([0.0] * 5)
