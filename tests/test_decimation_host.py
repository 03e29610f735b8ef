"""Host side of control decimation (no GPU): the launch policy and the kernel choice with D > 1 (solo_launch.h, through
tests/emu/emu_decimation_harness.cpp) - and unchanged results with D = 1, against the entry points of the emulator library
that pass no decimation at all -, the configuration field and the env plumbing on a stubbed engine."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from gym_solo_amd import abi
from helpers import make_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, 'tests', 'emu')


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
  out = str(tmp_path_factory.mktemp('emu_decim_host') / 'libsolo_emu_decimation.so')
  subprocess.check_call(['g++', '-O2', '-g', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-Wall', '-Wno-unknown-pragmas',
                         '-Wno-unused-variable', '-Wno-unused-but-set-variable', '-Wno-unused-function', '-DSOLO_QUEUE_SPINS=64',
                         '-o', out, os.path.join(EMU, 'emu_decimation_harness.cpp')])
  return C.CDLL(out)


def _plan(lib, ca, n, k, D=None, resident=None, ctl=0, sensing=0, flags=abi.STEP_ALL):
  out = np.zeros(4, dtype=np.int32)
  args = [C.byref(ca), ca.dtype, n, n if resident is None else resident, ctl, sensing, k, C.c_uint32(flags)]
  if D is None:
    lib.solo_emu_plan(*args, C.c_void_p(out.ctypes.data))            # (emu_harness.cpp's: a PlanInput without the new member)
  else:
    lib.solo_emu_decim_plan(*args, D, C.c_void_p(out.ctypes.data))
  return tuple(int(x) for x in out)   # S, launches, slices, migrate


def _kernel(lib, sensing, ctl, settling, resid, queue, flags, D=None, dtype=abi.F64):
  ident, name = np.zeros(5, dtype=np.int32), C.create_string_buffer(96)
  if D is None:
    lib.solo_emu_choose_kernel(sensing, ctl, settling, resid, queue, C.c_uint32(flags), dtype, C.c_void_p(ident.ctypes.data), name, 96)
  else:
    lib.solo_emu_decim_choose_kernel(sensing, ctl, settling, resid, queue, C.c_uint32(flags), D, dtype, C.c_void_p(ident.ctypes.data), name, 96)
  return tuple(int(x) for x in ident), name.value.decode()


def test_default_policy_keeps_the_physics_length_of_a_launch(lib):
  ca, _ = make_abi('float64')
  for D, S in ((2, 125), (4, 62), (10, 25), (64, 3)):
    assert _plan(lib, ca, 4096, 1000, D)[0] == S == max(1, 250 // D)
    assert _plan(lib, ca, 4096, 7, D)[:2] == (min(7, S), -(-7 // min(7, S)))
  # a configured value is taken as it is, in control steps
  ca10, _ = make_abi('float64', steps_per_launch=10)
  assert _plan(lib, ca10, 256, 27, 5) == (10, 3, 2, 0)
  # several launches: two slices, as with D = 1
  assert _plan(lib, ca, 4096, 1000, 4) == (62, 17, 2, 0)
  assert _plan(lib, ca, 4096, 20, 4) == (20, 1, 1, 0)


def test_decimated_launches_never_migrate(lib):
  ca, _ = make_abi('float64')
  assert _plan(lib, ca, 8192, 20, None, resident=4096)[3] == 10          # (D = 1, 8192 robots in f64: two chunks)
  assert _plan(lib, ca, 8192, 20, 1, resident=4096)[3] == 10
  assert _plan(lib, ca, 8192, 20, 2, resident=4096) == (20, 1, 1, 0)     # (-1 resolves to 0)
  assert _plan(lib, ca, 8192, 1000, 2, resident=4096) == (125, 8, 2, 0)


def test_decimation_one_plans_and_chooses_what_it_did(lib):
  rng = np.random.default_rng(0)
  for _ in range(300):
    dtype = ('float64', 'float32')[rng.integers(2)]
    ca, _ = make_abi(dtype, steps_per_launch=int(rng.choice([-1, 1, 7, 250, 400])), rollout_streams=int(rng.choice([-1, 1, 2, 4])),
                     migrate_steps=int(rng.choice([-1, 0, 5, 25])))
    n, k = int(rng.choice([1, 3, 256, 4096, 8192])), int(rng.integers(1, 1200))
    resident = int(rng.choice([n, 4096]))
    ctl, sensing = int(rng.integers(2)), int(rng.integers(2))
    flags = int(rng.choice([abi.STEP_ALL, abi.STEP_PHYSICS, abi.STEP_PHYSICS | abi.STEP_DONE]))
    assert _plan(lib, ca, n, k, 1, resident, ctl, sensing, flags) == _plan(lib, ca, n, k, None, resident, ctl, sensing, flags)
  for sensing in (0, 1):
    for ctl in (0, 1):
      for settling in (0, 1):
        for resid in (0, 1):
          for queue in (0, 1):
            for flags in (abi.STEP_ALL, abi.STEP_PHYSICS, abi.STEP_OBS):
              for dtype in (abi.F64, abi.F32):
                assert _kernel(lib, sensing, ctl, settling, resid, queue, flags, 1, dtype) == _kernel(lib, sensing, ctl, settling, resid, queue, flags, None, dtype)


def test_kernel_choice_with_decimation(lib):
  KERNEL_DECIM = 3
  for dtype, real in ((abi.F64, 'double'), (abi.F32, 'float')):
    assert _kernel(lib, 0, 0, 0, 0, 0, abi.STEP_ALL, 4, dtype) == ((KERNEL_DECIM, 1, 0, 0, 0), 'solo_decim_kernel<%s, true, false>' % real)
    assert _kernel(lib, 0, 1, 0, 0, 0, abi.STEP_ALL, 4, dtype) == ((KERNEL_DECIM, 1, 0, 0, 1), 'solo_decim_kernel<%s, true, true>' % real)
    assert _kernel(lib, 0, 0, 0, 0, 0, abi.STEP_PHYSICS, 4, dtype) == ((KERNEL_DECIM, 0, 0, 0, 0), 'solo_decim_kernel<%s, false, false>' % real)
    assert _kernel(lib, 0, 1, 0, 0, 0, abi.STEP_PHYSICS, 4, dtype) == ((KERNEL_DECIM, 0, 0, 0, 1), 'solo_decim_kernel<%s, false, true>' % real)
    # the settle loop stays in physics steps on the position kernels; a launch without physics has nothing to decimate
    assert _kernel(lib, 0, 1, 1, 0, 0, abi.STEP_PHYSICS, 4, dtype) == _kernel(lib, 0, 1, 1, 0, 0, abi.STEP_PHYSICS, None, dtype)
    assert _kernel(lib, 0, 0, 0, 0, 0, abi.STEP_OBS | abi.STEP_DONE, 4, dtype) == _kernel(lib, 0, 0, 0, 0, 0, abi.STEP_OBS | abi.STEP_DONE, None, dtype)
    assert _kernel(lib, 0, 1, 0, 0, 0, abi.STEP_OBS, 4, dtype)[1] == 'solo_ctl_step_kernel<%s, true>' % real


# ---- configuration and env plumbing on a stubbed engine ------------------------------------------------------------------
def _stub_env_class():
  from emu_kernel import EmuTorchEngine, make_emu_env_class
  from gym_solo_amd.core.configs import config_to_abi
  from gym_solo_amd.model import JOINT_NAMES

  class StubEngine(EmuTorchEngine):
    """the emulator engine plus a recording set_decimation (the emulator library itself steps one physics step per launch)"""

    def __init__(self, *a, **kw):
      super().__init__(*a, **kw)
      self.decimation_calls, self._decimation, self.step_calls = [], 1, 0

    def set_decimation(self, d):
      self.decimation_calls.append(d)
      self._decimation = d

    @property
    def decimation(self):
      return self._decimation

    def step(self, actions=None, flags=abi.STEP_ALL):
      self.step_calls += 1
      super().step(actions, flags)

  class StubEnv(make_emu_env_class()):
    def create_engine(self):
      cfg = config_to_abi(self.config, self.config.starting_joint_pos, JOINT_NAMES, normalize_actions=self._normalize)
      return StubEngine(cfg, self.solo_model.to_abi(), self.config.num_envs)

  return StubEnv


def _config(**kw):
  from gym_solo_amd.envs.solo8v2vanilla import Solo8VanillaConfig
  c = Solo8VanillaConfig()
  c.settle_steps = 20
  for k, v in kw.items():
    setattr(c, k, v)
  return c


def test_config_default_and_env_plumbing():
  from gym_solo_amd.core.configs import Solo8BaseConfig
  from gym_solo_amd.workloads import register_benchmark_workload
  assert Solo8BaseConfig().decimation == 1
  Env = _stub_env_class()
  plain = Env(config=_config())
  assert plain.engine.decimation_calls == [] and plain.decimation == 1 and plain.control_dt == pytest.approx(plain.config.dt)
  env = Env(config=_config(decimation=4))
  assert env.engine.decimation_calls == [4] and env.decimation == 4 and env.control_dt == pytest.approx(4 * env.config.dt)
  assert Env(config=_config(decimation=4), decimation=10).engine.decimation_calls == [10]   # (the argument wins)
  # step() is ONE engine call whatever the decimation
  register_benchmark_workload(env, max_steps=5)
  before = env.engine.step_calls
  env.step(np.zeros(12))
  assert env.engine.step_calls == before + 1
  for bad in (0, 65, -1, 2.5, True):
    with pytest.raises(ValueError):
      Env(config=_config(decimation=bad))
  # pybullet's numSubSteps divides dt - a different thing: still rejected
  with pytest.raises(ValueError):
    env.client.setPhysicsEngineParameter(numSubSteps=4)
  env.client.setPhysicsEngineParameter(fixedTimeStep=env.config.dt, numSubSteps=1)


def test_an_engine_without_decimation_rejects_the_configuration():
  from emu_kernel import make_emu_env_class
  Env = make_emu_env_class()
  with pytest.raises(ValueError, match='decimation'):
    Env(config=_config(decimation=2))
  assert Env(config=_config()).control_dt == pytest.approx(1e-3)
