"""ctypes driver of tests/emu/emu_push_harness.cpp: external base wrenches (solo_push_kernel) on the CPU wave emulator - the
product kernel source, the product's launch planning, kernel choice and the checks of solo_engine_set_base_wrench.  The harness is
compiled here, once per process, with the flags of tests/emu/Makefile's libsolo_emu.so (emu_terms.FLAGS), into a temporary
directory that is removed when the process ends.

PushSim: emu_actuator.ActSim with the engine's base wrench block - set_base_wrench(table or dict or None) validates as the engine
does (a rejected table leaves the previous block, or "off", in force), ``base_wrench`` is the block itself (in-place writes are
what the next call reads, as through Engine.base_wrench) and the calls go through solo_emu_push_call."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

from gym_solo_amd import abi
from emu_terms import EMU, FLAGS, _p
from emu_actuator import ActSim

_LIBS = {}
KPARAMS_TAIL = ('mu_base', 'ctl', 'contact', 'contact_traj', 'contact_traj_steps', 'decimation', 'term_value', 'term_fired', 'actuators',
                'wrench', 'sizeof')


def load():
  if 'lib' not in _LIBS:
    tmp = tempfile.mkdtemp(prefix='solo_emu_push_')
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    out = os.path.join(tmp, 'libsolo_emu_push.so')
    subprocess.check_call(['g++'] + FLAGS + ['-o', out, os.path.join(EMU, 'emu_push_harness.cpp')])
    lib = C.CDLL(out)
    call = ([C.POINTER(abi.SoloConfig), C.POINTER(abi.SoloModel), C.POINTER(abi.SoloProgram), C.c_void_p] + [C.c_int] * 5 + [C.c_uint32])
    lib.solo_emu_push_call.restype = C.c_int
    lib.solo_emu_push_call.argtypes = call + [C.c_void_p] * 17 + [C.c_char_p, C.c_int]
    lib.solo_emu_act_call.restype = C.c_int
    lib.solo_emu_act_call.argtypes = call + [C.c_void_p] * 16 + [C.c_char_p, C.c_int]
    lib.solo_emu_act_validate.restype = C.c_int
    lib.solo_emu_act_validate.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_int]
    lib.solo_emu_act_conflict.restype = C.c_int
    lib.solo_emu_act_conflict.argtypes = [C.POINTER(abi.SoloConfig), C.c_int, C.c_char_p, C.c_int]
    lib.solo_emu_push_validate.restype = C.c_int
    lib.solo_emu_push_validate.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_int]
    lib.solo_emu_push_conflict.restype = C.c_int
    lib.solo_emu_push_conflict.argtypes = [C.POINTER(abi.SoloConfig), C.c_int, C.c_char_p, C.c_int]
    lib.solo_emu_push_plan.restype = None
    lib.solo_emu_push_plan.argtypes = [C.POINTER(abi.SoloConfig)] + [C.c_int] * 6 + [C.c_uint32] + [C.c_int] * 4 + [C.POINTER(C.c_int32)]
    lib.solo_emu_push_choose_kernel.restype = C.c_int
    lib.solo_emu_push_choose_kernel.argtypes = [C.c_int] * 5 + [C.c_uint32] + [C.c_int] * 5 + [C.POINTER(C.c_int32), C.c_char_p, C.c_int]
    lib.solo_emu_push_kparams_offsets.restype = None
    lib.solo_emu_push_kparams_offsets.argtypes = [C.c_int, C.POINTER(C.c_int64)]
    _LIBS['lib'] = lib
  return _LIBS['lib']


def choose_kernel(lib, flags, dtype='float64', sensing=0, ctl=0, settling=0, resid=0, queue=0, decimation=1, state_terms=0, actuators=0, wrench=-1):
  """-> ((family, full, resid, migrate, ctl), name); wrench = -1: the call without the new argument"""
  out, name = (C.c_int32 * 5)(), C.create_string_buffer(96)
  lib.solo_emu_push_choose_kernel(sensing, ctl, settling, resid, queue, flags, decimation, state_terms, actuators, wrench,
                                  abi.F32 if dtype == 'float32' else abi.F64, out, name, 96)
  return tuple(out), name.value.decode()


def plan(lib, ca, n, k, resident=4096, ctl=0, sensing=0, flags=abi.STEP_ALL, decimation=1, state_terms=0, actuators=0, wrench=-1):
  """-> (S, launches, slices, migrate)"""
  out = (C.c_int32 * 4)()
  lib.solo_emu_push_plan(C.byref(ca), ca.dtype, n, resident, ctl, sensing, k, flags, decimation, state_terms, actuators, wrench, out)
  return tuple(out)


def kparams_offsets(lib, dtype):
  """{member: offsetof(KParams<T>, member)} for KPARAMS_TAIL ('sizeof': the struct's size)"""
  out = (C.c_int64 * len(KPARAMS_TAIL))()
  lib.solo_emu_push_kparams_offsets(abi.F32 if dtype == 'float32' else abi.F64, out)
  return dict(zip(KPARAMS_TAIL, [int(v) for v in out]))


def full_table(table, n):
  """[n, 6] / [n, 8] / {'force': [n, 3], 'torque': [n, 3]} -> [n, 8] (Engine.set_base_wrench's forms)"""
  if isinstance(table, dict):
    full = np.zeros((n, abi.WRENCH_WIDTH))
    for key, at in (('force', abi.WRENCH_FORCE), ('torque', abi.WRENCH_TORQUE)):
      if key in table:
        full[:, at:at + 3] = table[key]
    return full
  table = np.asarray(table, dtype=np.float64)
  if table.shape == (n, 6):
    full = np.zeros((n, abi.WRENCH_WIDTH))
    full[:, :6] = table
    return full
  assert table.shape == (n, abi.WRENCH_WIDTH)
  return np.ascontiguousarray(table)


class PushSim(ActSim):
  """One emulated engine with a base wrench block (None = off) next to the actuator block (None = off)"""

  def __init__(self, lib, cfg, model, n, program, snapshot, values=None, control=None, decimation=1):
    super().__init__(lib, cfg, model, n, program, snapshot, values, control, decimation)
    self.base_wrench = None

  def set_base_wrench(self, table):
    if table is None:
      self.base_wrench = None
      return
    table = full_table(table, self.n)
    msg = C.create_string_buffer(200)
    if self.lib.solo_emu_push_conflict(C.byref(self.ca), int(self.sensing), msg, 200) or \
       self.lib.solo_emu_push_validate(table.ctypes.data, self.n, self.ca.dtype, msg, 200):
      raise ValueError(msg.value.decode())
    real = np.float32 if self.ca.dtype == abi.F32 else np.float64   # (the engine's block holds the engine's precision)
    table = table.astype(real).astype(np.float64)
    if self.base_wrench is None:
      self.base_wrench = table
    else:
      self.base_wrench[:] = table   # (the engine's pointer is stable while the block stays on)

  def set_contact_sensing(self, on):
    if on and self.base_wrench is not None:
      raise ValueError('contact sensing does not support base wrenches: turn them off first')
    super().set_contact_sensing(on)

  def _call(self, actions, flags, single, outs=(None, None, None)):
    a = None if actions is None else np.ascontiguousarray(actions, dtype=np.float64)
    name = C.create_string_buffer(96)
    rc = self.lib.solo_emu_push_call(C.byref(self.ca), C.byref(self.ma), C.byref(self.prog), C.addressof(self.ctl) if self.ctl is not None else None,
                                     self.ca.dtype, self.n, 1 if single else a.shape[0], int(single), self.decimation, flags, _p(self.state),
                                     _p(self.snapshot), _p(a), _p(self.targets), _p(self.params), _p(outs[0]), _p(outs[1]), _p(outs[2]),
                                     _p(self.obs), _p(self.reward), _p(self.done), _p(self.term_count), _p(self.stats), _p(self.values),
                                     _p(self.term_fired), _p(self.actuators), _p(self.base_wrench), name, 96)
    if rc:
      raise RuntimeError('emulated call failed: %d' % rc)
    self.kernel = name.value.decode()
