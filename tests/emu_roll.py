"""ctypes driver of tests/emu/emu_roll_harness.cpp: fused segments (solo_roll_kernel) on the CPU wave emulator - the product kernel
source, the product's launch planning with PlanInput::fuse set as the engine sets it, its wiring and kernel choice.  The harness is
compiled here, once per process, with the flags of tests/emu/Makefile's libsolo_emu.so (emu_terms.FLAGS), into a temporary directory
that is removed when the process ends.

RollEngine: emu_kernel.EmuEngine whose rollout() goes through solo_emu_roll_rollout; ``info`` and ``kernels`` describe the last
rollout (the plan, the launches issued, the kernels they ran).  The same rollout without fused segments is EmuEngine.rollout itself,
on tests/emu/libsolo_emu.so."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

from gym_solo_amd import abi
from emu_kernel import EmuEngine, _dp
from emu_terms import EMU, FLAGS

_LIBS = {}
INFO = ('S', 'launches', 'slices', 'migrate', 'fuse', 'kernel_launches', 'segmented_launches', 'view_copied')


def load():
  if 'lib' not in _LIBS:
    tmp = tempfile.mkdtemp(prefix='solo_emu_roll_')
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    out = os.path.join(tmp, 'libsolo_emu_roll.so')
    subprocess.check_call(['g++'] + FLAGS + ['-o', out, os.path.join(EMU, 'emu_roll_harness.cpp')])
    lib = C.CDLL(out)
    dp = C.POINTER(C.c_double)
    lib.solo_emu_roll_rollout.restype = C.c_int
    lib.solo_emu_roll_rollout.argtypes = [C.POINTER(abi.SoloConfig), C.POINTER(abi.SoloModel), C.c_void_p, C.c_int, C.c_int, C.c_int, dp, dp, dp,
                                          dp, dp, dp, dp, C.c_void_p, dp, dp, C.c_void_p, C.c_void_p, dp, C.c_uint32, C.c_int, C.c_void_p,
                                          C.c_char_p, C.c_int]
    lib.solo_emu_roll_plan.restype = None
    lib.solo_emu_roll_plan.argtypes = [C.POINTER(abi.SoloConfig)] + [C.c_int] * 6 + [C.c_uint32] + [C.c_int] * 5 + [C.c_void_p]
    lib.solo_emu_roll_geometries.restype = C.c_int
    lib.solo_emu_roll_geometries.argtypes = [C.POINTER(abi.SoloConfig)] + [C.c_int] * 4 + [C.c_uint32, C.c_int, C.c_void_p, C.c_int]
    lib.solo_emu_choose_kernel.restype = C.c_int
    lib.solo_emu_choose_kernel.argtypes = [C.c_int] * 5 + [C.c_uint32, C.c_int, C.c_void_p, C.c_char_p, C.c_int]
    _LIBS['lib'] = lib
  return _LIBS['lib']


def plan(lib, ca, n, k, fuse=1, resident=4096, ctl=0, sensing=0, flags=abi.STEP_ALL, decimation=1, state_terms=0, actuators=0, wrench=0):
  """make_plan -> {S, launches, slices, migrate, fuse}"""
  out = np.zeros(5, dtype=np.int32)
  lib.solo_emu_roll_plan(C.byref(ca), ca.dtype, n, resident, ctl, sensing, k, flags, decimation, state_terms, actuators, wrench, fuse, out.ctypes.data)
  return dict(zip(INFO[:5], (int(x) for x in out)))


def geometries(lib, ca, n, k, fuse=1, resident=4096, flags=abi.STEP_ALL):
  """the plans for_each_geometry visits for rollouts of up to k steps: [(S, launches, slices, migrate, fuse)]"""
  out = np.zeros((1024, 5), dtype=np.int32)
  cnt = lib.solo_emu_roll_geometries(C.byref(ca), ca.dtype, n, resident, k, flags, fuse, out.ctypes.data, 1024)
  assert cnt <= 1024
  return [tuple(int(x) for x in row) for row in out[:cnt]]


class RollEngine(EmuEngine):
  """EmuEngine whose rollouts run under the launch policy with fused segments switched on (fuse=False: switched off - the same
  harness, the launches of before)"""

  def __init__(self, cfg, model, n, program=None, fuse=True):
    super().__init__(cfg, model, n, program=program)
    self.roll = load()
    self.fuse = fuse
    self.info, self.kernels = None, None

  def rollout(self, actions, flags=abi.STEP_ALL, record=True):
    a = np.ascontiguousarray(actions, dtype=np.float64)
    k = a.shape[0]
    d = self.program.num_obs
    obs = np.zeros((k, self.n, max(d, 1))) if record else None
    rew = np.zeros((k, self.n)) if record else None
    done = np.zeros((k, self.n), dtype=np.uint8) if record else None
    info, names = np.zeros(8, dtype=np.int32), C.create_string_buffer(256)
    rc = self.roll.solo_emu_roll_rollout(
      C.byref(self.cfg), C.byref(self.model), C.cast(C.pointer(self.program), C.c_void_p), self.cfg.dtype, self.n, k, _dp(self.state),
      _dp(self.snapshot), _dp(a), _dp(self.targets), _dp(self.params), _dp(obs) if record else None, _dp(rew) if record else None,
      done.ctypes.data if record else None, _dp(self.obs), _dp(self.reward), self.done.ctypes.data, self.term_count.ctypes.data,
      _dp(self.stats), flags, int(self.fuse), info.ctypes.data, names, 256)
    if rc:
      raise RuntimeError('emu rollout failed: %d' % rc)
    self.info = dict(zip(INFO, (int(x) for x in info)))
    self.kernels = names.value.decode().split(';')
    return (obs, rew, done) if record else None

  @property
  def cost(self):
    out = np.zeros(self.n, dtype=np.int32)
    self.roll.solo_emu_last_cost.restype = C.c_int
    self.roll.solo_emu_last_cost.argtypes = [C.c_void_p, C.c_int]
    self.roll.solo_emu_last_cost(out.ctypes.data, self.n)
    return out
