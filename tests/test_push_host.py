"""The host side of the base wrenches without a GPU: the kernel choice and the launch policy with a block on (solo_launch.h, through
tests/emu/emu_push_harness.cpp), that every call WITHOUT the new argument chooses what it chose before, the setter's contract on
the emulated engine (a rejected table leaves the previous block, or "off", in force; the unsupported combinations in both orders),
that the block is configuration, not state, the RandomPushes schedule against a stand-in engine, and Solo8VanillaEnv.step's calls."""
import itertools

import numpy as np
import pytest

from gym_solo_amd import abi
from helpers import make_abi
import actuator_cases as ac
import emu_push
from emu_push import choose_kernel, plan

KERNEL_STEP, KERNEL_CTL, KERNEL_CONTACT, KERNEL_DECIM, KERNEL_TERM, KERNEL_ACT, KERNEL_PUSH = range(7)
FLAGS = [abi.STEP_PHYSICS, abi.STEP_ALL, abi.STEP_DONE, abi.STEP_OBS | abi.STEP_REWARD, abi.STEP_PHYSICS | abi.STEP_DONE]


@pytest.fixture(scope='module')
def lib():
  return emu_push.load()


def test_the_new_family_is_chosen_exactly_under_its_rule(lib):
  for sensing, ctl, settling, resid, queue, flags, D, st, act, dtype in itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (0, 1), FLAGS, (1, 3), (0, 1), (0, 1),
                                                                                          ('float64', 'float32')):
    got = choose_kernel(lib, flags, dtype, sensing, ctl, settling, resid, queue, D, st, act, wrench=1)
    if not settling and flags & abi.STEP_PHYSICS:
      full = int(flags != abi.STEP_PHYSICS)
      assert got[0] == (KERNEL_PUSH, full, 0, 0, ctl)
      assert got[1] == 'solo_push_kernel<%s, %s, %s>' % ('double' if dtype == 'float64' else 'float', 'true' if full else 'false', 'true' if ctl else 'false')
    else:     # (the settle loop, and a launch that only evaluates outputs: the kernel it has without a block)
      assert got == choose_kernel(lib, flags, dtype, sensing, ctl, settling, resid, queue, D, st, act, wrench=0)
      assert got[0][0] != KERNEL_PUSH


def test_every_call_without_the_new_argument_chooses_what_it_chose_before(lib):
  """the whole argument space: the defaulted argument and an explicit `false` give the choice of the rules as they were - restated
  here from the families' own conditions"""
  seen = set()
  for sensing, ctl, settling, resid, queue, flags, D, st, act, dtype in itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (0, 1), FLAGS, (1, 3), (0, 1), (0, 1),
                                                                                          ('float64', 'float32')):
    without = choose_kernel(lib, flags, dtype, sensing, ctl, settling, resid, queue, D, st, act, wrench=-1)
    assert without == choose_kernel(lib, flags, dtype, sensing, ctl, settling, resid, queue, D, st, act, wrench=0)
    full = int(flags != abi.STEP_PHYSICS)
    if act and not settling and (flags & abi.STEP_PHYSICS or (st and flags & abi.STEP_DONE)):
      want = (KERNEL_ACT, full, 0, 0, ctl)
    elif st and not settling and flags & (abi.STEP_PHYSICS | abi.STEP_DONE):
      want = (KERNEL_TERM, full, 0, 0, ctl)
    elif D > 1 and not settling and flags & abi.STEP_PHYSICS:
      want = (KERNEL_DECIM, full, 0, 0, ctl)
    elif sensing and not settling:
      want = (KERNEL_CONTACT, full, 0, 0, ctl)
    elif ctl and not settling:
      want = (KERNEL_CTL, full, 0, 0, 1)
    elif queue:
      want = (KERNEL_STEP, 1, resid, 1, 0)
    else:
      want = (KERNEL_STEP, full, resid, 0, 0)
    assert without[0] == want, (sensing, ctl, settling, resid, queue, flags, D, st, act)
    assert not without[1].startswith('solo_push_kernel')
    seen.add(without[0][0])
  assert seen == {KERNEL_STEP, KERNEL_CTL, KERNEL_CONTACT, KERNEL_DECIM, KERNEL_TERM, KERNEL_ACT}


def test_make_plan_without_the_new_argument_plans_what_it_planned_before(lib):
  for dtype, migrate, spl, streams in itertools.product(('float64', 'float32'), (abi.AUTO, 0, 5), (abi.AUTO, 1, 50), (abi.AUTO, 1, 4)):
    ca, _ = make_abi(dtype, migrate_steps=migrate, steps_per_launch=spl, rollout_streams=streams)
    for n, k, ctl, sensing, flags, D, st, act in itertools.product((64, 4096, 8192), (1, 20, 1000), (0, 1), (0, 1), (abi.STEP_PHYSICS, abi.STEP_ALL), (1, 4),
                                                                   (0, 1), (0, 1)):
      assert plan(lib, ca, n, k, 4096, ctl, sensing, flags, D, st, act, wrench=-1) == plan(lib, ca, n, k, 4096, ctl, sensing, flags, D, st, act, wrench=0)


def test_plan_reports_no_migration_while_a_block_is_on(lib):
  ca, _ = make_abi('float64')   # (migrate_steps = -1: the engine chooses)
  n, resident = 8192, 4096
  for k in (20, 1000):
    off = plan(lib, ca, n, k, resident)
    assert off[3] > 0   # (f64 beyond the resident robots: migration, as before)
    on = plan(lib, ca, n, k, resident, wrench=1)
    assert on[3] == 0 and on[0] == off[0]   # (the steps per launch are the policy's)
  assert plan(lib, ca, 4096, 20, resident, wrench=1) == plan(lib, ca, 4096, 20, resident)
  ca32, _ = make_abi('float32')
  assert plan(lib, ca32, n, 20, resident, wrench=1) == plan(lib, ca32, n, 20, resident)


def _sim(lib, n=4, **kw):
  from test_emu_terms import program
  warm = kw.pop('solver_warm_start', 0.0)   # (the host configuration refuses it without the threshold: set on the struct)
  ca, ma = make_abi('float64', **kw)
  ca.solver_warm_start = warm
  snap = np.tile(ac.settled_row(), (n, 1))
  return emu_push.PushSim(lib, ca, ma, n, program([(abi.T_TIME, 3)]), snap)


def test_a_rejected_table_leaves_the_previous_block_and_the_forms_of_the_table(lib):
  s = _sim(lib)
  good = np.full((4, abi.WRENCH_WIDTH), -0.5)
  for bad_value in (np.nan, np.inf, -np.inf):
    bad = good.copy()
    bad[2, abi.WRENCH_TORQUE] = bad_value
    with pytest.raises(ValueError, match='finite'):
      s.set_base_wrench(bad)
    assert s.base_wrench is None                      # ("off" stays in force)
  s.set_base_wrench(good)
  view = s.base_wrench
  bad = np.zeros_like(good)
  bad[0, 0] = np.nan
  with pytest.raises(ValueError, match='finite'):
    s.set_base_wrench(bad)
  np.testing.assert_array_equal(s.base_wrench, good)
  s.step(np.zeros((4, abi.NUM_JOINTS)), abi.STEP_ALL)
  assert s.kernel == 'solo_push_kernel<double, true, false>'
  s.set_base_wrench({'torque': np.full((4, 3), 2.0)})
  np.testing.assert_array_equal(s.base_wrench, np.array([[0.0, 0.0, 0.0, 2.0, 2.0, 2.0, 0.0, 0.0]] * 4))
  assert s.base_wrench is view                        # (the block's address is stable while it stays on)
  s.set_base_wrench(np.arange(24.0).reshape(4, 6))
  np.testing.assert_array_equal(s.base_wrench[:, :6], np.arange(24.0).reshape(4, 6))
  np.testing.assert_array_equal(s.base_wrench[:, 6:], 0.0)
  s.set_base_wrench(None)
  s.step(np.zeros((4, abi.NUM_JOINTS)), abi.STEP_ALL)
  assert s.kernel == 'solo_step_kernel<double, true, false, false>'


def test_unsupported_combinations_in_both_orders(lib):
  zeros = np.zeros((4, abi.WRENCH_WIDTH))
  for kw, word in ((dict(migrate_steps=5), 'migrate_steps'), (dict(solver_residual_threshold=1e-7), 'solver_residual_threshold'),
                   (dict(solver_residual_threshold=1e-7, solver_warm_start=0.5), 'solver_residual_threshold'), (dict(solver_warm_start=0.5), 'solver_warm_start')):
    s = _sim(lib, **kw)
    with pytest.raises(ValueError, match=word):
      s.set_base_wrench(zeros)
    assert s.base_wrench is None
    s.set_base_wrench(None)
  s = _sim(lib)
  s.set_contact_sensing(True)
  with pytest.raises(ValueError, match='contact sensing'):
    s.set_base_wrench(zeros)
  s.set_contact_sensing(False)
  s.set_base_wrench(zeros)
  with pytest.raises(ValueError, match='base wrenches'):
    s.set_contact_sensing(True)
  assert not s.sensing and s.base_wrench is not None
  # it runs with the actuator block and with decimation, in either order
  s.set_actuators(np.ones((4, abi.ACTUATOR_WIDTH)))
  s.decimation = 3
  s.step(np.zeros((4, abi.NUM_JOINTS)), abi.STEP_ALL)
  assert s.kernel == 'solo_push_kernel<double, true, false>'


def test_the_block_is_configuration_not_state():
  from gym_solo_amd.engine import Engine
  assert 'base_wrench' not in Engine._CHECKPOINT and 'wrench' not in Engine._CHECKPOINT
  assert Engine._CHECKPOINT == ('state', 'snapshot', 'targets', 'term_count', 'params', 'stats_shards', 'cost', 'warm')
  assert Engine.CHECKPOINT_VERSION == 2
  assert callable(Engine.set_base_wrench) and isinstance(Engine.base_wrench, property)


# ---- RandomPushes against a stand-in engine that holds a CPU tensor block -----------------------------------------------------------
class StandIn:
  def __init__(self, n, dtype):
    import torch
    self.base_wrench = torch.zeros(n, abi.WRENCH_WIDTH, dtype=dtype)
    self.base_wrench[:, 6:] = 7.0     # (reserved: the schedule leaves them alone)


def _history(seed, n=16, ticks=400, lo=5, hi=9, duration=3, max_force=20.0, max_torque=1.5, dtype=None):
  import torch
  from gym_solo_amd.core.disturbance import RandomPushes
  eng = StandIn(n, dtype or torch.float64)
  view = eng.base_wrench
  g = torch.Generator()
  g.manual_seed(seed)
  rp = RandomPushes(eng, interval=(lo, hi), duration=duration, max_force=max_force, max_torque=max_torque, generator=g)
  out = [eng.base_wrench.clone()]
  for _ in range(ticks):
    rp.tick()
    out.append(eng.base_wrench.clone())
  assert eng.base_wrench is view     # (written in place)
  return torch.stack(out).numpy()


def test_random_pushes_schedule():
  import torch
  lo, hi, duration, max_force, max_torque = 5, 9, 3, 20.0, 1.5
  for dtype in (torch.float64, torch.float32):
    h = _history(11, lo=lo, hi=hi, duration=duration, max_force=max_force, max_torque=max_torque, dtype=dtype)
    assert np.all(h[0, :, :6] == 0) and np.all(h[:, :, 6:] == 7.0)
    pushes = 0
    for r in range(h.shape[1]):
      w = h[:, r, :6]
      on = np.abs(w).max(axis=1) > 0
      # run lengths of the on / off phases, the unfinished last one dropped
      edges = np.flatnonzero(np.diff(on.astype(int))) + 1
      runs = np.split(np.arange(len(on)), edges)
      assert not on[0]
      for i, run in enumerate(runs[:-1]):
        if on[run[0]]:
          assert len(run) == duration, (r, i, len(run))
          assert np.all(w[run] == w[run[0]])                       # (held unchanged for the whole push)
          f, t = w[run[0], :3], w[run[0], 3:]
          assert f[2] == 0 and np.linalg.norm(f) <= max_force * (1 + 1e-6) and np.linalg.norm(t) <= max_torque * (1 + 1e-6)
          pushes += 1
        else:
          assert lo <= len(run) <= hi, (r, i, len(run))
    assert pushes > 16 * 400 // (hi + duration) - 16
  # two runs with the same seed agree; another seed differs
  assert np.array_equal(_history(3), _history(3)) and not np.array_equal(_history(3), _history(4))
  # max_torque = 0: pure forces, of every direction
  h = _history(5, max_torque=0.0)
  assert np.all(h[:, :, 3:6] == 0)
  f = h[:, :, :2].reshape(-1, 2)
  f = f[np.abs(f).max(axis=1) > 0]
  assert (f[:, 0] > 0).any() and (f[:, 0] < 0).any() and (f[:, 1] > 0).any() and (f[:, 1] < 0).any()


def test_random_pushes_arguments():
  import torch
  from gym_solo_amd.core.disturbance import RandomPushes
  eng = StandIn(4, torch.float64)
  for kw in (dict(interval=(0, 3), duration=1, max_force=1.0), dict(interval=(4, 3), duration=1, max_force=1.0),
             dict(interval=(1, 3), duration=0, max_force=1.0), dict(interval=(1, 3), duration=1, max_force=-1.0),
             dict(interval=(1, 3), duration=1, max_force=1.0, max_torque=float('nan'))):
    with pytest.raises(ValueError):
      RandomPushes(eng, **kw)


# ---- Solo8VanillaEnv.step --------------------------------------------------------------------------------------------------------
def _recording_env():
  from test_env_host import make_env
  from gym_solo_amd.core import obs as solo_obs, termination as terms
  from gym_solo_amd.testing import SimpleReward
  env = make_env()
  env.obs_factory.register_observation(solo_obs.TorsoIMU(env.robot))
  env.reward_factory.register_reward(1, SimpleReward())
  env.termination_factory.register_termination(terms.TimeBasedTermination(5))
  calls = []
  step = env.engine.step

  def recorded(actions=None, flags=abi.STEP_ALL):
    calls.append(('step', actions is not None, int(flags)))
    return step(actions, flags)
  env.engine.step = recorded
  return env, calls


def test_env_step_without_a_disturbance_issues_the_calls_of_before():
  from gym_solo_amd.envs.solo8v2vanilla import Solo8VanillaEnv
  assert Solo8VanillaEnv.disturbance is None
  env, calls = _recording_env()
  assert env.disturbance is None
  env.step(env.action_space.sample())
  env.step(env.action_space.sample())
  assert calls == [('step', True, abi.STEP_ALL)] * 2     # (one fused launch per step, nothing else)

  class Tick:
    def tick(self):
      calls.append(('tick',))
  env.disturbance = Tick()
  del calls[:]
  env.step(env.action_space.sample())
  assert calls == [('step', True, abi.STEP_ALL), ('tick',)]
