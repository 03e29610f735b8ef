"""The output epilogue of the HIP step kernels (solo_step_kernel, solo_ctl_step_kernel, solo_contact_kernel) against the
reference-pinned host references (tests/epilogue_cases.py), through the C ABI; tests/test_emu_epilogue.py runs the same
bodies on the CPU wave emulator."""
import pytest

import epilogue_cases as ec
from gym_solo_amd import abi
from test_gpu_env import make_env

pytestmark = pytest.mark.gpu

PAIRS = ec.golden_pairs()
IDS = ['%s-%s-%s' % (o, 'norm' if nrm else 'raw', r) for o, nrm, r in PAIRS]
N = 256


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('obs_name,normalize,rew_name', PAIRS, ids=IDS)
def test_golden_states_through_the_epilogue(obs_name, normalize, rew_name, dtype):
  ec.case_golden_through_epilogue(make_env, obs_name, normalize, rew_name, dtype)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('obs_name,normalize,rew_name', [('imu_deg', True, 'composite'), ('bench', False, 'hard_step'),
                                                         ('imu_rad', False, 'flat_torso'), ('enc_deg_clip', True, 'upright')])
def test_divergent_lanes_after_an_in_launch_restore(obs_name, normalize, rew_name, dtype):
  for m in ec.restart_steps(dtype):
    ec.case_divergent_lanes(make_env, obs_name, normalize, rew_name, dtype, m)


def test_random_reward_trees_through_the_epilogue():
  ec.case_random_trees_through_epilogue(make_env)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('normalize', [False, True])
def test_widest_observation_program(normalize, dtype):
  ec.case_widest_observation_program(make_env, dtype, normalize)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('normalize', [False, True])
def test_full_observation_program_with_foot_forces(normalize, dtype):
  ec.case_full_observation_program_with_foot_forces(make_env, dtype, normalize)


# ---- physics rollouts (B) and the episodic bookkeeping (C) ----------------------------------------------------------------
@pytest.mark.parametrize('spl', sorted({28, 29, ec.pass_steps('float64'), ec.pass_steps('float64') + 1}))
def test_rollout_degree_clip_normalised_weighted3(spl):
  ec.case_physics_rollout(make_env, 'float64', N, spl, 70, ('imu_deg', 'enc_deg_clip'), True, 'weighted3', seed=1)


@pytest.mark.parametrize('dtype,spl', [('float64', 57), ('float32', 65), ('float64', 2 * ec.pass_steps('float64') + 1)])
def test_rollout_bench_composite_two_launches_and_a_step(dtype, spl):
  ec.case_physics_rollout(make_env, dtype, N, spl, 2 * spl + 1, ('imu_rad', 'enc_rad'), False, 'composite', seed=2)


def test_rollout_degree_clip_normalised_weighted3_4096_robots():
  ec.case_physics_rollout(make_env, 'float64', 4096, ec.pass_steps('float64') + 1, 70, ('imu_deg', 'enc_deg_clip'), True, 'weighted3', seed=5)


@pytest.mark.parametrize('dtype,spl', [('float64', 57), ('float32', 65)])
def test_rollout_bench_composite_4096_robots(dtype, spl):
  ec.case_physics_rollout(make_env, dtype, 4096, spl, 2 * spl + 1, ('imu_rad', 'enc_rad'), False, 'composite', seed=6)


@pytest.mark.parametrize('dtype,migrate', [('float64', 5), ('float64', 0), ('float32', 0)])
def test_rollout_full_length_reward_program(dtype, migrate):
  tree = ec.full_length_tree()
  assert ec._program_length(tree) == abi.MAX_REWARD_OPS
  ec.case_physics_rollout(make_env, dtype, N, 33, 45, ('enc_clip',), False, tree, seed=3, streams=2, migrate=migrate)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('flags', [abi.STEP_PHYSICS | abi.STEP_REWARD, abi.STEP_PHYSICS | abi.STEP_OBS | abi.STEP_DONE])
def test_rollout_partial_flags_leave_the_bookkeeping_alone(flags, dtype):
  ec.case_physics_rollout(make_env, dtype, N, ec.pass_steps(dtype) + 1, 40, ('imu_rad', 'enc_rad'), False, 'hard_step+speed', flags=flags, seed=4)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('kernel', ['torque', 'contact'])
def test_rollout_control_and_contact_kernels(kernel, dtype):
  """solo_ctl_step_kernel (torque control) and solo_contact_kernel (contact sensing on): separately compiled copies of the
  same epilogue text, 250 steps per launch, 300 steps."""
  extra = dict(control_mode='torque') if kernel == 'torque' else dict(contact_sensing=True)
  scale = 2.0 if kernel == 'torque' else 6.28   # (torques up to motor_torque_limit; position targets)
  ec.case_physics_rollout(make_env, dtype, N, 250, 300, ('imu_rad', 'enc_rad'), False, 'composite', seed=7, extra=extra, action_scale=scale)
