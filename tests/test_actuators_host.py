"""The host side of the actuator randomisation without a GPU: the kernel choice and the launch policy with a block on
(solo_launch.h, through tests/emu/emu_actuator_harness.cpp), that every call WITHOUT the new argument chooses what it chose before,
the setter's contract on the emulated engine (a rejected table leaves the previous block, or "off", in force; the unsupported
combinations in both orders), and that the block is configuration, not state."""
import itertools

import numpy as np
import pytest

from gym_solo_amd import abi
from helpers import make_abi
import actuator_cases as ac
import emu_actuator
from emu_actuator import choose_kernel, plan

KERNEL_STEP, KERNEL_CTL, KERNEL_CONTACT, KERNEL_DECIM, KERNEL_TERM, KERNEL_ACT = range(6)
FLAGS = [abi.STEP_PHYSICS, abi.STEP_ALL, abi.STEP_DONE, abi.STEP_OBS | abi.STEP_REWARD, abi.STEP_PHYSICS | abi.STEP_DONE]


@pytest.fixture(scope='module')
def lib():
  return emu_actuator.load()


def test_the_new_family(lib):
  for dtype, ctl, flags in itertools.product(('float64', 'float32'), (0, 1), (abi.STEP_PHYSICS, abi.STEP_ALL)):
    for D, state_terms in ((1, 0), (3, 0), (1, 1), (4, 1)):
      (family, full, resid, migrate, c), name = choose_kernel(lib, flags, dtype, ctl=ctl, decimation=D, state_terms=state_terms, actuators=1)
      assert (family, full, resid, migrate, c) == (KERNEL_ACT, int(flags != abi.STEP_PHYSICS), 0, 0, ctl)
      assert name == 'solo_act_kernel<%s, %s, %s>' % ('double' if dtype == 'float64' else 'float', 'true' if full else 'false', 'true' if ctl else 'false')
  # the settle loop stays on the plain position kernels, whatever is on
  for ctl, D, st in itertools.product((0, 1), (1, 3), (0, 1)):
    ids, name = choose_kernel(lib, abi.STEP_PHYSICS, settling=1, ctl=ctl, decimation=D, state_terms=st, actuators=1)
    assert ids == (KERNEL_STEP, 0, 0, 0, 0) and name == 'solo_step_kernel<double, false, false, false>'
  # a launch that neither steps the physics nor evaluates a state termination keeps its kernel; one that evaluates them is taken
  for flags in (abi.STEP_DONE, abi.STEP_OBS | abi.STEP_REWARD, abi.STEP_OBS | abi.STEP_DONE):
    assert choose_kernel(lib, flags, actuators=1) == choose_kernel(lib, flags, actuators=0)
    assert choose_kernel(lib, flags, ctl=1, decimation=3, actuators=1) == choose_kernel(lib, flags, ctl=1, decimation=3, actuators=0)
  assert choose_kernel(lib, abi.STEP_DONE, state_terms=1, actuators=1)[0][0] == KERNEL_ACT
  assert choose_kernel(lib, abi.STEP_OBS, state_terms=1, actuators=1)[0][0] != KERNEL_ACT


def test_every_call_without_the_new_argument_chooses_what_it_chose_before(lib):
  """the whole argument space: the defaulted argument and an explicit `false` give the choice of the rules as they were - restated
  here from the families' own conditions"""
  seen = set()
  for sensing, ctl, settling, resid, queue, flags, D, st, dtype in itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (0, 1), FLAGS, (1, 3), (0, 1),
                                                                                     ('float64', 'float32')):
    without = choose_kernel(lib, flags, dtype, sensing, ctl, settling, resid, queue, D, st, actuators=-1)
    assert without == choose_kernel(lib, flags, dtype, sensing, ctl, settling, resid, queue, D, st, actuators=0)
    full = int(flags != abi.STEP_PHYSICS)
    if st and not settling and flags & (abi.STEP_PHYSICS | abi.STEP_DONE):
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
    assert without[0] == want, (sensing, ctl, settling, resid, queue, flags, D, st)
    assert not without[1].startswith('solo_act_kernel')
    seen.add(without[0][0])
  assert seen == {KERNEL_STEP, KERNEL_CTL, KERNEL_CONTACT, KERNEL_DECIM, KERNEL_TERM}


def test_plan_reports_no_migration_while_a_block_is_on(lib):
  ca, _ = make_abi('float64')   # (migrate_steps = -1: the engine chooses)
  n, resident = 8192, 4096
  for k in (20, 1000):
    off = plan(lib, ca, n, k, resident)
    assert off == plan(lib, ca, n, k, resident, actuators=0) and off[3] > 0   # (f64 beyond the resident robots: migration, as before)
    on = plan(lib, ca, n, k, resident, actuators=1)
    assert on[3] == 0
    assert on[0] == off[0]   # (the steps per launch are the policy's)
  # within the resident robots nothing changes at all
  assert plan(lib, ca, 4096, 20, resident, actuators=1) == plan(lib, ca, 4096, 20, resident)
  ca32, _ = make_abi('float32')
  assert plan(lib, ca32, n, 20, resident, actuators=1) == plan(lib, ca32, n, 20, resident)


def _sim(lib, n=4, **kw):
  from test_emu_terms import program
  warm = kw.pop('solver_warm_start', 0.0)   # (the host configuration refuses it without the threshold: set on the struct)
  ca, ma = make_abi('float64', **kw)
  ca.solver_warm_start = warm
  snap = np.tile(ac.settled_row(), (n, 1))
  return emu_actuator.ActSim(lib, ca, ma, n, program([(abi.T_TIME, 3)]), snap)


def test_a_rejected_table_leaves_the_previous_block(lib):
  s = _sim(lib)
  good = np.full((4, abi.ACTUATOR_WIDTH), 0.5)
  for bad_value in (np.nan, -1.0, np.inf):
    bad = good.copy()
    bad[2, abi.ACT_KD] = bad_value
    with pytest.raises(ValueError, match='finite and >= 0'):
      s.set_actuators(bad)
    assert s.actuators is None                      # ("off" stays in force)
  s.set_actuators(good)
  for bad_value in (np.nan, -1.0, np.inf):
    bad = np.ones_like(good)
    bad[0, abi.ACT_TORQUE_LIMIT] = bad_value
    with pytest.raises(ValueError, match='finite and >= 0'):
      s.set_actuators(bad)
    np.testing.assert_array_equal(s.actuators, good)
  s.step(np.zeros((4, abi.NUM_JOINTS)), abi.STEP_ALL)
  assert s.kernel == 'solo_act_kernel<double, true, false>'
  s.set_actuators({'kp': np.full(4, 2.0)})
  np.testing.assert_array_equal(s.actuators, np.array([[1.0, 2.0, 1.0, 1.0]] * 4))
  s.set_actuators(None)
  s.step(np.zeros((4, abi.NUM_JOINTS)), abi.STEP_ALL)
  assert s.kernel == 'solo_step_kernel<double, true, false, false>'


def test_unsupported_combinations_in_both_orders(lib):
  ones = np.ones((4, abi.ACTUATOR_WIDTH))
  for kw, word in ((dict(migrate_steps=5), 'migrate_steps'), (dict(solver_residual_threshold=1e-7), 'solver_residual_threshold'),
                   (dict(solver_residual_threshold=1e-7, solver_warm_start=0.5), 'solver_residual_threshold'), (dict(solver_warm_start=0.5), 'solver_warm_start')):
    s = _sim(lib, **kw)
    with pytest.raises(ValueError, match=word):
      s.set_actuators(ones)
    assert s.actuators is None
    s.set_actuators(None)
  s = _sim(lib)
  s.set_contact_sensing(True)
  with pytest.raises(ValueError, match='contact sensing'):
    s.set_actuators(ones)
  s.set_contact_sensing(False)
  s.set_actuators(ones)
  with pytest.raises(ValueError, match='actuator randomisation'):
    s.set_contact_sensing(True)
  assert not s.sensing and s.actuators is not None


def test_the_block_is_configuration_not_state():
  from gym_solo_amd.engine import Engine
  assert 'actuators' not in Engine._CHECKPOINT
  assert Engine._CHECKPOINT == ('state', 'snapshot', 'targets', 'term_count', 'params', 'stats_shards', 'cost', 'warm')
  assert Engine.CHECKPOINT_VERSION == 2
  assert Engine.ACTUATOR_COLUMNS == {'torque_limit': abi.ACT_TORQUE_LIMIT, 'kp': abi.ACT_KP, 'kd': abi.ACT_KD}
