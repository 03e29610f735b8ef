"""Host side of the state terminations (no GPU): HeightTermination / TiltTermination stand-alone and on the emulator env class
(tests/emu_terms.py: the product kernel source through tests/emu/emu_terms_harness.cpp), the argument checks, the Python fallback
against the fused path, TerminationFactory.fired(), the terminated / truncated split of Solo8VectorEnv with and without a state
termination, and the launch policy / kernel choice with a state termination in the program (solo_launch.h)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from gym_solo_amd import abi
from gym_solo_amd.core import termination as terms
from gym_solo_amd.testing import DummyTermination
from helpers import make_abi
import emu_terms

N = 3


class FakeClient:
  """getBasePositionAndOrientation over a settable state"""

  def __init__(self, n=N):
    self.pos, self.quat = torch.zeros(n, 3, dtype=torch.float64), torch.zeros(n, 4, dtype=torch.float64)
    self.quat[:, 3] = 1

  def getBasePositionAndOrientation(self, body):
    return self.pos, self.quat


# ---- the classes, stand-alone ---------------------------------------------------------------------------------------------
def test_argument_checks():
  for bad in (-1, 1.5, True, '2'):
    with pytest.raises((ValueError, TypeError)):
      terms.HeightTermination(0, 0.1, after_steps=bad)
  for bad in (0.0, math.pi, -0.3, 4.0, float('nan')):
    with pytest.raises(ValueError):
      terms.TiltTermination(0, bad)
  for bad in (float('nan'), float('inf')):
    with pytest.raises(ValueError):
      terms.HeightTermination(0, bad)
  assert terms.HeightTermination(0, -0.5, after_steps=2.0).after_steps == 2   # (a negative height is a height)


def test_program_and_values():
  h, t = terms.HeightTermination(7, 0.08, after_steps=120), terms.TiltTermination(7, 1.0)
  assert h.program() == (abi.T_HEIGHT_BELOW, 120) and t.program() == (abi.T_TILT_ABOVE, 0)
  assert h.value == 0.08 and t.value == math.cos(1.0)          # (cos(max_tilt), in double)
  f = terms.TerminationFactory()
  f.register_termination(terms.TimeBasedTermination(5), h, t)
  assert f.fusable() and f.has_state_termination()
  assert f.program() == [(abi.T_TIME, 5), (abi.T_HEIGHT_BELOW, 120), (abi.T_TILT_ABOVE, 0)]
  assert f.values() == [0.0, 0.08, math.cos(1.0)]
  g = terms.TerminationFactory()
  g.register_termination(terms.TimeBasedTermination(5))
  assert not g.has_state_termination() and g.values() == [0.0]
  with pytest.raises(ValueError):
    f.fired()    # (no env)


def test_stand_alone_evaluation_ticks_like_a_time_based_counter():
  h = terms.HeightTermination(0, 0.1, after_steps=2)
  with pytest.raises(ValueError, match='client'):
    h.is_terminated()
  c = FakeClient()
  h.client = c
  c.pos[:, 2] = torch.tensor([0.05, 0.2, 0.05])
  # grace 2: the first two evaluations never fire, the third does where the condition holds
  assert h.is_terminated().tolist() == [False, False, False]
  assert h.is_terminated().tolist() == [False, False, False]
  assert h.is_terminated().tolist() == [True, False, True]
  c.pos[0, 2] = 0.1     # (z < value is strict)
  assert h.is_terminated().tolist() == [False, False, True]
  # a masked evaluation ticks only the robots it asks about; a partial reset clears their counters
  h.reset()
  assert h.is_terminated_where(torch.tensor([True, True, False])).tolist() == [False] * 3
  assert h._count.tolist() == [1, 1, 0]
  h.reset_where(torch.tensor([1, 0, 0], dtype=torch.uint8))
  assert h._count.tolist() == [0, 1, 0]
  t = terms.TiltTermination(0, 0.5)
  t.client = c
  for i, angle in enumerate((0.4, 0.6, 3.0)):   # rolled about x
    c.quat[i] = torch.tensor([math.sin(angle / 2), 0, 0, math.cos(angle / 2)])
  assert t.is_terminated().tolist() == [False, True, True]
  c.quat[1] = torch.tensor([0, math.sin(0.3), 0, math.cos(0.3)])   # pitched by 0.6
  assert t.is_terminated().tolist() == [False, True, True]
  c.quat[1] = torch.tensor([0, 0, math.sin(1.0), math.cos(1.0)])   # yaw is no tilt
  assert t.is_terminated().tolist() == [False, False, True]


# ---- on the emulator env class ---------------------------------------------------------------------------------------------
Env = emu_terms.make_emu_terms_env_class()


def _config(**kw):
  from gym_solo_amd.envs.solo8v2vanilla import Solo8VanillaConfig
  c = Solo8VanillaConfig()
  c.settle_steps, c.num_envs, c.dtype = 20, N, 'float64'
  for k, v in kw.items():
    setattr(c, k, v)
  return c


def _env(terminations, **kw):
  from gym_solo_amd.core import obs as solo_obs
  from gym_solo_amd.testing import SimpleReward
  env = Env(config=_config(**kw))
  env.obs_factory.register_observation(solo_obs.TorsoIMU(env.robot))
  env.reward_factory.register_reward(1, SimpleReward())
  env.termination_factory.register_termination(*terminations(env))
  return env


def _actions(k):
  return torch.as_tensor(np.random.default_rng(3).uniform(-6, 6, (k, N, abi.NUM_JOINTS)))


class NeverPython(terms.Termination):
  """a Python-only termination (no program()): the factory is not fusable"""

  def reset(self):
    pass

  def is_terminated(self):
    return False


def _z0(env):
  return float(env.engine.snapshot[0, abi.S_POS + 2])


def test_fused_path_sets_the_thresholds_before_the_program():
  calls = []
  env = _env(lambda e: [terms.HeightTermination(e.robot, 0.3, after_steps=1), terms.TimeBasedTermination(4)])
  eng = env.engine
  real_values, real_program = eng.set_term_values, eng.set_program
  eng.set_term_values = lambda v: (calls.append(('values', list(v))), real_values(v))[1]
  eng.set_program = lambda p: (calls.append(('program', [p.term_kind[i] for i in range(p.num_terms)])), real_program(p))[1]
  env.step(_actions(1)[0])
  assert calls == [('values', [0.3, 0.0]), ('program', [abi.T_HEIGHT_BELOW, abi.T_TIME])]
  assert eng.launched[-1] == 'solo_term_kernel<double, true, false>'
  # a time-only program goes back to the kernels of before, and sets no thresholds
  plain = _env(lambda e: [terms.TimeBasedTermination(4)])
  plain.engine.set_term_values = lambda v: calls.append('unexpected')
  plain.step(_actions(1)[0])
  assert plain.engine.launched[-1] == 'solo_step_kernel<double, true, false, false>' and 'unexpected' not in calls
  with pytest.raises(ValueError):
    plain.termination_factory.fired()


def _height_first(e):
  """the robots fall (20 settle steps) ~0.2 mm per step: the height limit 0.7 mm under the snapshot is crossed on the fourth step"""
  return [terms.HeightTermination(e.robot, _z0(e) - 7e-4, after_steps=1), terms.TiltTermination(e.robot, 1.0), terms.TimeBasedTermination(6)]


def _time_first(e):
  """a tilt limit of 1e-6 rad behind a TimeBased(2): random targets tilt the falling base by far more within two steps"""
  return [terms.TimeBasedTermination(2), terms.TiltTermination(e.robot, 1e-6, after_steps=1)]


@pytest.mark.parametrize('auto_reset', [False, True])
@pytest.mark.parametrize('members', [_height_first, _time_first])
def test_python_fallback_equals_the_fused_path(members, auto_reset):
  """a termination list fused, and the same list plus a Python-only termination (not fusable: evaluated with torch from
  engine.state, the same formula and tick rule): the same flags, fired() and - with auto-reset - the same states, step by step"""
  fused = _env(members, auto_reset=auto_reset)
  python = _env(lambda e: members(e) + [NeverPython()], auto_reset=auto_reset)
  assert fused.termination_factory.fusable() and not python.termination_factory.fusable()
  seen = set()
  for k, a in enumerate(_actions(8)):
    _, _, df, _ = fused.step(a)
    _, _, dp, _ = python.step(a)
    assert hasattr(dp, 'dtype') and dp.dtype == torch.bool
    ff, fp = fused.termination_factory.fired(), python.termination_factory.fired()
    assert ff.dtype == torch.uint8 and ff.tolist() == fp.tolist(), (k, ff, fp)
    assert df.tolist() == dp.tolist() == [bool(x) for x in ff.tolist()]
    seen |= set(ff.tolist())
    if auto_reset:
      np.testing.assert_array_equal(fused.engine.state.numpy()[:, :abi.S_RETURN], python.engine.state.numpy()[:, :abi.S_RETURN])
  # the state termination fired; without the auto-reset the TimeBased in front of the tilt limit gets to fire too
  assert seen == ({0, 1} if members is _height_first else ({0, 2} if auto_reset else {0, 1, 2})), seen


def test_vector_env_splits_terminated_and_truncated():
  from gym_solo_amd.vector import Solo8VectorEnv
  # [Height, TimeBased(2)]: robots end by height (terminated) ...
  env = _env(lambda e: [terms.HeightTermination(e.robot, _z0(e) - 7e-4), terms.TimeBasedTermination(5)], auto_reset=True)
  v = Solo8VectorEnv(env)
  ended = []
  for a in _actions(7):
    obs, reward, terminated, truncated, info = v.step(a)
    assert terminated.dtype == torch.bool and truncated.dtype == torch.bool and not (terminated & truncated).any()
    fired = env.termination_factory.fired()
    assert terminated.tolist() == (fired == 1).tolist() and truncated.tolist() == (fired == 2).tolist()
    ended.append((bool(terminated.any()), bool(truncated.any())))
  assert (True, False) in ended
  # ... and by the clock (truncated) when the height limit is out of reach
  env = _env(lambda e: [terms.HeightTermination(e.robot, -1.0), terms.TimeBasedTermination(2)], auto_reset=True)
  v = Solo8VectorEnv(env)
  got = [v.step(a)[2:4] for a in _actions(3)]
  assert [(bool(t.any()), bool(u.all())) for t, u in got] == [(False, False), (False, False), (False, True)]


def test_vector_env_without_a_state_termination_behaves_as_before():
  from gym_solo_amd.vector import Solo8VectorEnv
  timed = Solo8VectorEnv(_env(lambda e: [terms.TimeBasedTermination(1)], auto_reset=True))
  assert timed._time_limited() and not timed._state_terminations()
  outs = [timed.step(a) for a in _actions(2)]
  assert [(bool(o[2].any()), bool(o[3].all())) for o in outs] == [(False, False), (False, True)]
  other = Solo8VectorEnv(_env(lambda e: [DummyTermination(e.robot, True)], auto_reset=True))
  assert not other._time_limited()
  o = other.step(_actions(1)[0])
  assert bool(o[2].all()) and not bool(o[3].any())


# ---- launch policy and kernel choice (solo_launch.h) --------------------------------------------------------------------------
def _plan(ca, n, k, D, state_terms, resident=None, ctl=0, flags=abi.STEP_ALL):
  out = np.zeros(4, dtype=np.int32)
  emu_terms.load().solo_emu_terms_plan(C.byref(ca), ca.dtype, n, n if resident is None else resident, ctl, k, C.c_uint32(flags), D, state_terms,
                                       C.c_void_p(out.ctypes.data))
  return tuple(int(x) for x in out)


def _kernel(sensing, ctl, settling, resid, queue, flags, D, state_terms, dtype=abi.F64):
  ident, name = np.zeros(5, dtype=np.int32), C.create_string_buffer(96)
  emu_terms.load().solo_emu_terms_choose_kernel(sensing, ctl, settling, resid, queue, C.c_uint32(flags), D, state_terms, dtype,
                                                C.c_void_p(ident.ctypes.data), name, 96)
  return tuple(int(x) for x in ident), name.value.decode()


def test_robots_never_migrate_under_a_state_termination():
  ca, _ = make_abi('float64')
  assert _plan(ca, 8192, 20, 1, 0, resident=4096) == (20, 1, 1, 10)   # (8192 robots in f64: two chunks)
  assert _plan(ca, 8192, 20, 1, 1, resident=4096) == (20, 1, 1, 0)    # (-1 resolves to 0)
  assert _plan(ca, 8192, 1000, 1, 1, resident=4096)[3] == 0
  assert _plan(ca, 4096, 1000, 4, 1) == _plan(ca, 4096, 1000, 4, 0) == (62, 17, 2, 0)


def test_kernel_choice_with_a_state_termination():
  KERNEL_TERM = 4
  for dtype, real in ((abi.F64, 'double'), (abi.F32, 'float')):
    for D in (1, 4):
      assert _kernel(0, 0, 0, 0, 0, abi.STEP_ALL, D, 1, dtype) == ((KERNEL_TERM, 1, 0, 0, 0), 'solo_term_kernel<%s, true, false>' % real)
      assert _kernel(0, 1, 0, 0, 0, abi.STEP_ALL, D, 1, dtype) == ((KERNEL_TERM, 1, 0, 0, 1), 'solo_term_kernel<%s, true, true>' % real)
      assert _kernel(0, 0, 0, 0, 0, abi.STEP_PHYSICS, D, 1, dtype) == ((KERNEL_TERM, 0, 0, 0, 0), 'solo_term_kernel<%s, false, false>' % real)
      assert _kernel(0, 1, 0, 0, 0, abi.STEP_PHYSICS, D, 1, dtype) == ((KERNEL_TERM, 0, 0, 0, 1), 'solo_term_kernel<%s, false, true>' % real)
      # a query evaluates the state terminations: the same family; an observation-only launch and the settle loop: the kernels of before
      assert _kernel(0, 0, 0, 0, 0, abi.STEP_DONE, D, 1, dtype)[1] == 'solo_term_kernel<%s, true, false>' % real
      assert _kernel(0, 0, 0, 0, 0, abi.STEP_OBS, D, 1, dtype) == _kernel(0, 0, 0, 0, 0, abi.STEP_OBS, D, 0, dtype)
      assert _kernel(0, 1, 1, 0, 0, abi.STEP_PHYSICS, D, 1, dtype) == _kernel(0, 1, 1, 0, 0, abi.STEP_PHYSICS, D, 0, dtype)
  # without one, every choice is what it was
  for sensing in (0, 1):
    for ctl in (0, 1):
      for settling in (0, 1):
        for resid in (0, 1):
          for queue in (0, 1):
            for flags in (abi.STEP_ALL, abi.STEP_PHYSICS, abi.STEP_OBS, abi.STEP_DONE):
              for D in (1, 4):
                ident, name = _kernel(sensing, ctl, settling, resid, queue, flags, D, 0)
                assert ident[0] != KERNEL_TERM and 'term' not in name
