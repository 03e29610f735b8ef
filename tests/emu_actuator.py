"""ctypes driver of tests/emu/emu_actuator_harness.cpp: actuator randomisation (solo_act_kernel) on the CPU wave emulator - the
product kernel source, the product's launch planning, kernel choice and the checks of solo_engine_set_actuators.  The harness is
compiled here, once per process, with the flags of tests/emu/Makefile's libsolo_emu.so, into a temporary directory that is removed
when the process ends.

ActSim: emu_terms.TermsSim with the engine's actuator block - set_actuators(table or dict or None) validates as the engine does
(a rejected table leaves the previous block, or "off", in force) and the calls go through solo_emu_act_call."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

from gym_solo_amd import abi
from emu_terms import EMU, FLAGS, TermsSim, _p

_LIBS = {}
COLUMNS = {'torque_limit': abi.ACT_TORQUE_LIMIT, 'kp': abi.ACT_KP, 'kd': abi.ACT_KD}


def load():
  if 'lib' not in _LIBS:
    tmp = tempfile.mkdtemp(prefix='solo_emu_act_')
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    out = os.path.join(tmp, 'libsolo_emu_act.so')
    subprocess.check_call(['g++'] + FLAGS + ['-o', out, os.path.join(EMU, 'emu_actuator_harness.cpp')])
    lib = C.CDLL(out)
    lib.solo_emu_act_call.restype = C.c_int
    lib.solo_emu_act_call.argtypes = ([C.POINTER(abi.SoloConfig), C.POINTER(abi.SoloModel), C.POINTER(abi.SoloProgram), C.c_void_p] +
                                      [C.c_int] * 5 + [C.c_uint32] + [C.c_void_p] * 16 + [C.c_char_p, C.c_int])
    lib.solo_emu_act_validate.restype = C.c_int
    lib.solo_emu_act_validate.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_int]
    lib.solo_emu_act_conflict.restype = C.c_int
    lib.solo_emu_act_conflict.argtypes = [C.POINTER(abi.SoloConfig), C.c_int, C.c_char_p, C.c_int]
    lib.solo_emu_act_plan.restype = None
    lib.solo_emu_act_plan.argtypes = [C.POINTER(abi.SoloConfig)] + [C.c_int] * 6 + [C.c_uint32] + [C.c_int] * 3 + [C.POINTER(C.c_int32)]
    lib.solo_emu_act_choose_kernel.restype = C.c_int
    lib.solo_emu_act_choose_kernel.argtypes = [C.c_int] * 5 + [C.c_uint32] + [C.c_int] * 4 + [C.POINTER(C.c_int32), C.c_char_p, C.c_int]
    _LIBS['lib'] = lib
  return _LIBS['lib']


def choose_kernel(lib, flags, dtype='float64', sensing=0, ctl=0, settling=0, resid=0, queue=0, decimation=1, state_terms=0, actuators=-1):
  """-> ((family, full, resid, migrate, ctl), name); actuators = -1: the call without the new argument"""
  out, name = (C.c_int32 * 5)(), C.create_string_buffer(96)
  lib.solo_emu_act_choose_kernel(sensing, ctl, settling, resid, queue, flags, decimation, state_terms, actuators,
                                 abi.F32 if dtype == 'float32' else abi.F64, out, name, 96)
  return tuple(out), name.value.decode()


def plan(lib, ca, n, k, resident=4096, ctl=0, sensing=0, flags=abi.STEP_ALL, decimation=1, state_terms=0, actuators=-1):
  """-> (S, launches, slices, migrate)"""
  out = (C.c_int32 * 4)()
  lib.solo_emu_act_plan(C.byref(ca), ca.dtype, n, resident, ctl, sensing, k, flags, decimation, state_terms, actuators, out)
  return tuple(out)


class ActSim(TermsSim):
  """One emulated engine with an actuator block (None = off)"""

  def __init__(self, lib, cfg, model, n, program, snapshot, values=None, control=None, decimation=1):
    super().__init__(lib, cfg, model, n, program, snapshot, values, control, decimation)
    self.actuators = None
    self.sensing = False

  def set_actuators(self, table):
    """solo_engine_set_actuators / Engine.set_actuators: [n, 4], a dict of [n] columns (missing ones are 1), or None"""
    if table is None:
      self.actuators = None
      return
    if isinstance(table, dict):
      full = np.ones((self.n, abi.ACTUATOR_WIDTH))
      for key, col in table.items():
        full[:, COLUMNS[key]] = col
      table = full
    table = np.ascontiguousarray(table, dtype=np.float64)
    assert table.shape == (self.n, abi.ACTUATOR_WIDTH)
    msg = C.create_string_buffer(200)
    if self.lib.solo_emu_act_conflict(C.byref(self.ca), int(self.sensing), msg, 200) or \
       self.lib.solo_emu_act_validate(table.ctypes.data, self.n, self.ca.dtype, msg, 200):
      raise ValueError(msg.value.decode())
    real = np.float32 if self.ca.dtype == abi.F32 else np.float64   # (the engine's block holds the engine's precision)
    self.actuators = table.astype(real).astype(np.float64)

  def set_contact_sensing(self, on):
    if on and self.actuators is not None:
      raise ValueError('contact sensing does not support actuator randomisation: turn it off first')
    self.sensing = bool(on)

  def _call(self, actions, flags, single, outs=(None, None, None)):
    a = None if actions is None else np.ascontiguousarray(actions, dtype=np.float64)
    name = C.create_string_buffer(96)
    rc = self.lib.solo_emu_act_call(C.byref(self.ca), C.byref(self.ma), C.byref(self.prog), C.addressof(self.ctl) if self.ctl is not None else None,
                                    self.ca.dtype, self.n, 1 if single else a.shape[0], int(single), self.decimation, flags, _p(self.state),
                                    _p(self.snapshot), _p(a), _p(self.targets), _p(self.params), _p(outs[0]), _p(outs[1]), _p(outs[2]),
                                    _p(self.obs), _p(self.reward), _p(self.done), _p(self.term_count), _p(self.stats), _p(self.values),
                                    _p(self.term_fired), _p(self.actuators), name, 96)
    if rc:
      raise RuntimeError('emulated call failed: %d' % rc)
    self.kernel = name.value.decode()

  def everything(self):
    out = super().everything()
    out.update(obs=self.obs.copy(), reward=self.reward.copy(), done=self.done.copy(), term_fired=self.term_fired.copy(), stats=self.stats.copy())
    return out
