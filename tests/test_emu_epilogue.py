"""The output epilogue of the step kernel against the reference-pinned host references (tests/epilogue_cases.py), on the
PRODUCT kernel source compiled for the CPU wave emulator; tests/test_gpu_epilogue.py runs the same bodies on the HIP
engine.  (The torque-control and contact-sensing kernels' copies of the epilogue have no emulator harness with outputs:
GPU suite only.)"""
import pytest

import epilogue_cases as ec
from gym_solo_amd import abi
from test_env_host import make_env

PAIRS = ec.golden_pairs()
IDS = ['%s-%s-%s' % (o, 'norm' if nrm else 'raw', r) for o, nrm, r in PAIRS]
N = 8   # robots of the physics rollouts (the emulator runs one wave after the other)


def test_pass_length_is_derived_from_the_kernel_source():
  """The launch lengths below sit around kPass.  It is 32 in f32; in f64 it follows the row-vector block, which the
  product build (four waves per SIMD) sizes for 25 steps and the three-wave A/B build for 28: both are in the lists, and
  a source that says something else moves the lists with it."""
  assert ec.pass_steps('float32') == 32
  assert ec.pass_steps('float64') in (25, 28)
  for dtype in ('float32', 'float64'):
    p = ec.pass_steps(dtype)
    assert {2, p - 1, p, p + 1, 2 * p + 1} <= set(ec.launch_lengths(dtype))
  assert {2, 27, 28, 29, 57} <= set(ec.launch_lengths('float64'))
  assert {2, 31, 32, 33, 65} <= set(ec.launch_lengths('float32'))


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


# ---- physics rollouts (B) and the episodic bookkeeping (C) ----------------------------------------------------------------
@pytest.mark.parametrize('spl', sorted({28, 29, ec.pass_steps('float64'), ec.pass_steps('float64') + 1}))
def test_rollout_degree_clip_normalised_weighted3(spl):
  ec.case_physics_rollout(make_env, 'float64', N, spl, 70, ('imu_deg', 'enc_deg_clip'), True, 'weighted3', seed=1)


@pytest.mark.parametrize('dtype,spl', [('float64', 57), ('float32', 65), ('float64', 2 * ec.pass_steps('float64') + 1)])
def test_rollout_bench_composite_two_launches_and_a_step(dtype, spl):
  ec.case_physics_rollout(make_env, dtype, N, spl, 2 * spl + 1, ('imu_rad', 'enc_rad'), False, 'composite', seed=2)


@pytest.mark.parametrize('dtype,migrate', [('float64', 5), ('float64', 0), ('float32', 0)])
def test_rollout_full_length_reward_program(dtype, migrate):
  tree = ec.full_length_tree()
  assert ec._program_length(tree) == abi.MAX_REWARD_OPS
  ec.case_physics_rollout(make_env, dtype, N, 33, 45, ('enc_clip',), False, tree, seed=3, streams=2, migrate=migrate)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('flags', [abi.STEP_PHYSICS | abi.STEP_REWARD, abi.STEP_PHYSICS | abi.STEP_OBS | abi.STEP_DONE])
def test_rollout_partial_flags_leave_the_bookkeeping_alone(flags, dtype):
  ec.case_physics_rollout(make_env, dtype, N, ec.pass_steps(dtype) + 1, 40, ('imu_rad', 'enc_rad'), False, 'hard_step+speed', flags=flags, seed=4)
