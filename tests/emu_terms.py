"""ctypes driver of tests/emu/emu_terms_harness.cpp: state terminations (solo_term_kernel) on the CPU wave emulator - the
product kernel source, the product's launch planning and kernel choice.  The harness is compiled here, once per process, with the
flags of tests/emu/Makefile's libsolo_emu.so, into a temporary directory that is removed when the process ends.

TermsSim: the numpy buffers of one emulated engine and its calls (what tests/test_emu_terms.py drives).
EmuTermsTorchEngine / make_emu_terms_env_class: emu_kernel.EmuTorchEngine with set_term_values / term_fired / set_decimation,
so that the host API (envs, factories, the vector adapter) runs state terminations without a GPU."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

from gym_solo_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, 'tests', 'emu')
# (the flags of tests/emu/Makefile's libsolo_emu.so)
FLAGS = ['-O2', '-g', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-Wall', '-Wno-unknown-pragmas', '-Wno-unused-variable',
         '-Wno-unused-but-set-variable', '-Wno-unused-function', '-DSOLO_QUEUE_SPINS=64']
_LIBS = {}


def load():
  if 'lib' not in _LIBS:
    tmp = tempfile.mkdtemp(prefix='solo_emu_terms_')
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    out = os.path.join(tmp, 'libsolo_emu_terms.so')
    subprocess.check_call(['g++'] + FLAGS + ['-o', out, os.path.join(EMU, 'emu_terms_harness.cpp')])
    lib = C.CDLL(out)
    lib.solo_emu_terms_call.restype = C.c_int
    lib.solo_emu_terms_call.argtypes = ([C.POINTER(abi.SoloConfig), C.POINTER(abi.SoloModel), C.POINTER(abi.SoloProgram), C.c_void_p] +
                                        [C.c_int] * 5 + [C.c_uint32] + [C.c_void_p] * 15 + [C.c_char_p, C.c_int])
    lib.solo_emu_terms_validate.restype = C.c_int
    lib.solo_emu_terms_validate.argtypes = [C.POINTER(abi.SoloProgram), C.c_char_p, C.c_int]
    _LIBS['lib'] = lib
  return _LIBS['lib']


def _p(x):
  return None if x is None else x.ctypes.data


class TermsSim:
  """One emulated engine: buffers as doubles (the kernel's arithmetic is cfg.dtype's), calls through solo_emu_terms_call"""

  def __init__(self, lib, cfg, model, n, program, snapshot, values=None, control=None, decimation=1):
    self.lib, self.ca, self.ma, self.n = lib, cfg, model, n
    self.prog, self.ctl, self.decimation = program, control, decimation
    self.values = np.zeros(abi.MAX_TERMS)
    if values is not None:
      self.values[:len(values)] = values
    self.snapshot = np.array(snapshot, dtype=np.float64)
    self.state = self.snapshot.copy()
    self.targets = np.tile(self.reset_command(), (n, 1))
    self.params = np.zeros((n, 4))
    self.params[:, 0], self.params[:, 1] = cfg.lateral_friction, 1.0
    self.obs = np.zeros((n, max(program.num_obs, 1)))
    self.reward = np.zeros(n)
    self.done = np.zeros(n, dtype=np.uint8)
    self.term_count = np.zeros((n, abi.MAX_TERMS), dtype=np.int32)
    self.term_fired = np.zeros(n, dtype=np.uint8)
    self.stats = np.zeros((abi.STATS_SHARDS, abi.STATS_WIDTH))
    self.kernel = None

  def reset_command(self):
    """what a reset leaves the motors commanded to (torque mode: 0; position / PD: the settle pose)"""
    if self.ctl is not None and self.ctl.mode == abi.CTRL_TORQUE:
      return np.zeros(abi.NUM_JOINTS)
    real = np.float32 if self.ca.dtype == abi.F32 else np.float64   # (the parameter block holds them in the engine's precision)
    return np.array(list(self.ca.settle_targets)).astype(real).astype(np.float64)

  def _call(self, actions, flags, single, outs=(None, None, None)):
    a = None if actions is None else np.ascontiguousarray(actions, dtype=np.float64)
    name = C.create_string_buffer(96)
    rc = self.lib.solo_emu_terms_call(C.byref(self.ca), C.byref(self.ma), C.byref(self.prog), C.addressof(self.ctl) if self.ctl is not None else None,
                                      self.ca.dtype, self.n, 1 if single else a.shape[0], int(single), self.decimation, flags, _p(self.state),
                                      _p(self.snapshot), _p(a), _p(self.targets), _p(self.params), _p(outs[0]), _p(outs[1]), _p(outs[2]),
                                      _p(self.obs), _p(self.reward), _p(self.done), _p(self.term_count), _p(self.stats), _p(self.values),
                                      _p(self.term_fired), name, 96)
    if rc:
      raise RuntimeError('emulated call failed: %d' % rc)
    self.kernel = name.value.decode()

  def step(self, action=None, flags=abi.STEP_ALL):
    self._call(action, flags, True)

  def rollout(self, actions, flags=abi.STEP_ALL):
    k = actions.shape[0]
    outs = (np.zeros((k, self.n, max(self.prog.num_obs, 1))), np.zeros((k, self.n)), np.zeros((k, self.n), dtype=np.uint8))
    self._call(actions, flags, False, outs)
    return outs

  def reset(self, mask=None):
    """solo_reset_kernel"""
    m = slice(None) if mask is None else np.asarray(mask).astype(bool)
    self.state[m] = self.snapshot[m]
    self.term_count[m] = 0
    self.targets[m] = self.reset_command()

  def everything(self):
    return dict(state=self.state.copy(), targets=self.targets.copy(), term_count=self.term_count.copy())


def make_emu_terms_engine_class():
  from emu_kernel import EmuTorchEngine

  class EmuTermsTorchEngine(EmuTorchEngine):
    """The emulator engine with state terminations: its launches go through emu_terms_harness.cpp (the engine's kernel choice:
    solo_term_kernel while the program holds a state kind, else the kernels of before)"""

    def __init__(self, *a, **kw):
      super().__init__(*a, **kw)
      self._term_values = np.zeros(abi.MAX_TERMS)
      self._term_fired = np.zeros(self.num_envs, dtype=np.uint8)
      self.term_fired = self._torch.from_numpy(self._term_fired)
      self.decimation = 1
      self.launched = []

    def set_term_values(self, values):
      vals = [float(v) for v in values]
      if len(vals) > abi.MAX_TERMS:
        raise ValueError('at most {} termination thresholds'.format(abi.MAX_TERMS))
      self._term_values[:] = vals + [0.0] * (abi.MAX_TERMS - len(vals))

    def set_decimation(self, d):
      self.decimation = int(d)

    def set_program(self, program):
      msg = C.create_string_buffer(160)
      if load().solo_emu_terms_validate(C.byref(program), msg, 160):   # (pack_program's checks, as Engine<T>::set_program runs them)
        raise ValueError(msg.value.decode())
      super().set_program(program)

    def _terms_call(self, a, flags, single, outs=(None, None, None)):
      e = self._e
      name = C.create_string_buffer(96)
      rc = load().solo_emu_terms_call(C.byref(e.cfg), C.byref(e.model), C.byref(self.program), None, e.cfg.dtype, e.n,
                                      1 if single else a.shape[0], int(single), self.decimation, flags, _p(e.state), _p(e.snapshot), _p(a),
                                      _p(e.targets), _p(e.params), _p(outs[0]), _p(outs[1]), _p(outs[2]), _p(e.obs), _p(e.reward), _p(e.done),
                                      _p(e.term_count), _p(e.stats), _p(self._term_values), _p(self._term_fired), name, 96)
      if rc:
        raise RuntimeError('emulated call failed: %d' % rc)
      self.launched.append(name.value.decode())

    def step(self, actions=None, flags=abi.STEP_ALL):
      if self.program is None or flags == abi.STEP_PHYSICS and self.decimation == 1:
        return super().step(actions, flags)
      if (flags & abi.STEP_DONE) and self.program.num_terms == 0:
        raise ValueError('Need to register at least one termination instance')
      a = None if actions is None else np.ascontiguousarray(actions.detach().cpu().numpy(), dtype=np.float64)
      self._terms_call(a, flags, True)

    def rollout(self, actions, flags=abi.STEP_ALL, record=False, out=None):
      a = np.ascontiguousarray(actions.detach().cpu().numpy(), dtype=np.float64)
      k = a.shape[0]
      got = (np.zeros((k, self.num_envs, max(self.obs_dim, 1))), np.zeros((k, self.num_envs)), np.zeros((k, self.num_envs), dtype=np.uint8))
      self._terms_call(a, flags, False, got)
      if not record and out is None:
        return None
      obs, rew, done = out if out is not None else self.rollout_buffers(k)
      for dst, src in zip((obs, rew, done), got):
        dst.copy_(self._torch.from_numpy(src))
      return obs, rew, done

  return EmuTermsTorchEngine


def make_emu_terms_env_class():
  """Solo8VanillaEnv on that engine"""
  from gym_solo_amd.core.configs import config_to_abi
  from gym_solo_amd.envs.solo8v2vanilla import Solo8VanillaEnv
  from gym_solo_amd.model import JOINT_NAMES
  Engine = make_emu_terms_engine_class()

  class EmuTermsSolo8VanillaEnv(Solo8VanillaEnv):
    def create_engine(self):
      cfg = config_to_abi(self.config, self.config.starting_joint_pos, JOINT_NAMES, normalize_actions=self._normalize)
      return Engine(cfg, self.solo_model.to_abi(), self.config.num_envs)

  return EmuTermsSolo8VanillaEnv
