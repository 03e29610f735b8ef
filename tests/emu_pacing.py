"""ctypes driver of tests/emu/emu_pacing_harness.cpp: progress pacing of the segmented launch (solo_roll_kernel) on the CPU wave
emulator - the product kernel source, launch planning and wiring, with the progress block wired or null.  The harness is compiled
here, once per process, with the flags of tests/emu/Makefile's libsolo_emu.so (emu_terms.FLAGS), into a temporary directory that is
removed when the process ends.

PacedEngine: emu_kernel.EmuEngine whose rollout() goes through solo_emu_pacing_rollout; ``info`` and ``progress`` describe the last
rollout (the plan, the launches issued and wired, the block's counters afterwards)."""
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
INFO = ('S', 'launches', 'slices', 'migrate', 'fuse', 'kernel_launches', 'wired_launches', 'view_copied')
COUNTERS = 16   # kMaxFusedSegments


def load():
  if 'lib' not in _LIBS:
    tmp = tempfile.mkdtemp(prefix='solo_emu_pacing_')
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    out = os.path.join(tmp, 'libsolo_emu_pacing.so')
    subprocess.check_call(['g++'] + FLAGS + ['-o', out, os.path.join(EMU, 'emu_pacing_harness.cpp')])
    lib = C.CDLL(out)
    dp = C.POINTER(C.c_double)
    lib.solo_emu_pacing_rollout.restype = C.c_int
    lib.solo_emu_pacing_rollout.argtypes = [C.POINTER(abi.SoloConfig), C.POINTER(abi.SoloModel), C.c_void_p, C.c_int, C.c_int, C.c_int, dp, dp, dp,
                                            dp, dp, dp, dp, C.c_void_p, dp, dp, C.c_void_p, C.c_void_p, dp, C.c_uint32, C.c_int, C.c_void_p,
                                            C.c_void_p]
    lib.solo_emu_pacing_wiring.restype = C.c_int
    lib.solo_emu_pacing_wiring.argtypes = [C.POINTER(abi.SoloConfig), C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_void_p, C.c_int,
                                           C.c_void_p, C.c_void_p]
    _LIBS['lib'] = lib
  return _LIBS['lib']


def wiring(lib, ca, n, k, fuse=1, flags=abi.STEP_ALL):
  """(plan, launches, geometry_ints): plan = {S, launches, slices, fuse, progress_ints, paced}; launches = [(slice, segmented, block)]
  in issue order, block 0 = none, 1 = the engine's, 2 = another pointer; geometry_ints = the most counters a geometry of up to k
  steps needs (what reserve(k) has to allocate)"""
  out, plan, most = np.zeros((256, 3), dtype=np.int32), np.zeros(6, dtype=np.int32), np.zeros(1, dtype=np.int32)
  cnt = lib.solo_emu_pacing_wiring(C.byref(ca), ca.dtype, n, k, flags, fuse, out.ctypes.data, 256, plan.ctypes.data, most.ctypes.data)
  assert cnt <= 256
  return (dict(zip(('S', 'launches', 'slices', 'fuse', 'progress_ints', 'paced'), (int(x) for x in plan))),
          [tuple(int(x) for x in row) for row in out[:cnt]], int(most[0]))


class PacedEngine(EmuEngine):
  """EmuEngine whose rollouts run as fused segments with the progress block wired (paced=False: null - the kernel of before)"""

  def __init__(self, cfg, model, n, program=None, paced=True):
    super().__init__(cfg, model, n, program=program)
    self.pacing = load()
    self.paced = paced
    self.info, self.progress = None, None

  def rollout(self, actions, flags=abi.STEP_ALL, record=True):
    a = np.ascontiguousarray(actions, dtype=np.float64)
    k = a.shape[0]
    d = self.program.num_obs
    obs = np.zeros((k, self.n, max(d, 1))) if record else None
    rew = np.zeros((k, self.n)) if record else None
    done = np.zeros((k, self.n), dtype=np.uint8) if record else None
    info, progress = np.zeros(8, dtype=np.int32), np.zeros(COUNTERS, dtype=np.int32)
    rc = self.pacing.solo_emu_pacing_rollout(
      C.byref(self.cfg), C.byref(self.model), C.cast(C.pointer(self.program), C.c_void_p), self.cfg.dtype, self.n, k, _dp(self.state),
      _dp(self.snapshot), _dp(a), _dp(self.targets), _dp(self.params), _dp(obs) if record else None, _dp(rew) if record else None,
      done.ctypes.data if record else None, _dp(self.obs), _dp(self.reward), self.done.ctypes.data, self.term_count.ctypes.data,
      _dp(self.stats), flags, int(self.paced), info.ctypes.data, progress.ctypes.data)
    if rc:
      raise RuntimeError('emu rollout failed: %d' % rc)
    self.info = dict(zip(INFO, (int(x) for x in info)))
    self.progress = progress
    return (obs, rew, done) if record else None

  @property
  def cost(self):
    out = np.zeros(self.n, dtype=np.int32)
    self.pacing.solo_emu_last_cost.restype = C.c_int
    self.pacing.solo_emu_last_cost.argtypes = [C.c_void_p, C.c_int]
    self.pacing.solo_emu_last_cost(out.ctypes.data, self.n)
    return out
