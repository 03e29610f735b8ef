"""GPU parity of the step kernels through the C-ABI on NON-DEFAULT robot models (tests/model_space.py): random points of the
family validate_model admits - all six inertia components of all nine bodies, link CoMs, hip and knee origins, spheres (one on
an upper link), per-joint limits, legs that are no mirror images - and edge models that move one term each.  Every other parity
test builds Solo8Model().to_abi(), where Ixy = Ixz = 0, the knee origin's x is 0 and both leg spheres sit on the lower link:
pack_params' xy / xz copies, the 6 x 6 composite inertia, the BODY_UPPER sphere transform and the per-leg table indices only
ever saw zeros or one branch.

256 robots per engine, the oracle on 8 threads.  The conditions that keep these tests from passing vacuously (contact rows
live, an upper-link sphere touching, limit rows live together with contact rows, an edge model's trajectory leaving the
default model's) are asserted on the ORACLE's trajectory (model_space.Liveness)."""
import ctypes as C

import numpy as np
import pytest

import model_space as ms
from gym_solo_amd import abi
from helpers import make_abi, random_actions

pytestmark = pytest.mark.gpu

N = 256
THREADS = 8
OBS_SPEC = [('torso_imu', {}), ('motor_encoder', {})]


@pytest.fixture(scope='module')
def torch():
  import torch
  if not torch.cuda.is_available():
    pytest.fail('GPU tests need a visible MI355X')
  return torch


def _engine(ca, ma, n=N):
  from gym_solo_amd.engine import Engine
  return Engine(ca, ma, n)


def _config(config_seed, **extra):
  """the default configuration, or a random point of the configuration space whose settle loop is long enough for the robot
  to land from the random start height (config_space draws 40 or 80 steps: the robot would still be falling, and the steps
  under test would have no contact rows)"""
  kw = dict(extra)
  if config_seed is not None:
    from config_space import random_config
    kw.update(random_config(config_seed))
    kw['settle_steps'] = 1000
  return kw


# Which points of the configuration space: the liveness conditions need a robot that is on the ground, and on the oracle the
# points 0 ... 4 land and keep >= 3 spheres touching in >= 90 % of the robot-steps on both models (5 and 7: 65 ... 72 %; 6,
# with its weak gravity and stiff motors, kicks itself off the ground and is still in the air after 1000 steps).  Of those,
# 1 (dt = 1e-3, 30 sweeps) and 3 (dt = 2e-3, 10 sweeps) differ in the two knobs the solver is most sensitive to.
CONFIG_SEEDS = (1, 3)


def reference_run(case, config_seed=None, steps=40, n=N, terrain=None, params=None, action_seed=0):
  """The ORACLE's side of a position-control case (no GPU): its settle snapshot [1 or n, 32], the per-robot random actions,
  its state after every step and what its steps had live."""
  from oracle import solo_oracle as so
  ca, _ = make_abi('float64', **_config(config_seed))
  ma = ms.get_model(case).to_abi()
  ph = so.OraclePhysics(ca, ma, terrain=terrain)
  snap = ph.settle(1) if params is None else ph.settle(n, params=params, threads=THREADS)
  st = np.tile(snap, (n, 1)) if params is None else snap.copy()
  rng = np.random.default_rng(300 + action_seed)
  live = ms.Liveness(ph, ma, ca)
  acts, states = [], []
  for k in range(steps):
    a = random_actions(rng, n)
    live.see(st, a, params, every=4)
    ph.step(st, a, params, threads=THREADS)
    acts.append(a)
    states.append(st.copy())
  return dict(ca=ca, ma=ma, ph=ph, snap=snap, acts=acts, states=states, live=live)


_DEFAULT_FINAL = {}


def leaves_the_default_trajectory(case, ref):
  """an edge model's oracle trajectory differs from the default model's under the same actions by more than 1e-6 after the
  steps: the term the model changes matters at the bar the parity is held to"""
  if 'flat' not in _DEFAULT_FINAL:
    _DEFAULT_FINAL['flat'] = reference_run('default')['states'][-1]
  return np.abs(ref['states'][-1][:, :29] - _DEFAULT_FINAL['flat'][:, :29]).max() > 1e-6


F64_CASES = [(c, None) for c in ms.ALL_CASES] + [('seed0', CONFIG_SEEDS[0]), ('seed1', CONFIG_SEEDS[1])]


@pytest.mark.parametrize('case,config_seed', F64_CASES, ids=['{}{}'.format(c, '' if s is None else '-config%d' % s) for c, s in F64_CASES])
def test_position_control_matches_oracle_f64(torch, case, config_seed):
  """The engine's settle snapshot against OraclePhysics.settle(1) tiled (1e-9), then 40 steps of per-robot random actions in
  single-step launches against the oracle (1e-9 on [:, :29]) - the bars of test_random_configurations_match_oracle_f64 - on
  every random model and edge model, and on two random models at random points of the configuration space (tests/config_space.py;
  the settle loop lengthened to 1000 steps so that the robot has landed).
  Measured on the MI355X over the eleven cases: settle 6e-16 ... 1.2e-12, 40 steps 8.5e-12 ... 1.4e-10 (seed1, whose knee
  limits are live throughout)."""
  ref = reference_run(case, config_seed)
  ca, ma, ph, live = ref['ca'], ref['ma'], ref['ph'], ref['live']
  live.check(case)
  if case == 'upper_spheres':
    assert ms.upper_sphere_touches(ph, ma, ca, ref['snap'][0])
  if case in ms.EDGE_MODELS:
    assert leaves_the_default_trajectory(case, ref)
  eng = _engine(ca, ma)
  snap = eng.snapshot.cpu().numpy()
  err_settle = np.abs(snap[:, :29] - np.tile(ref['snap'][:, :29], (N, 1))).max()
  for a in ref['acts']:
    eng.step(torch.as_tensor(a, device='cuda'), abi.STEP_PHYSICS)
  err = np.abs(eng.state.cpu().numpy()[:, :29] - ref['states'][-1][:, :29]).max()
  diverged = eng.stats.cpu().numpy()[5]
  eng.close()
  print('model space f64 ({}, config {}): settle {:.2e}, 40 steps {:.2e}; {}'.format(case, config_seed, err_settle, err, live))
  assert diverged == 0
  assert err_settle <= 1e-9, (case, config_seed, err_settle)
  assert err <= 1e-9, (case, config_seed, err)


def _bench_program(torch):
  """the benchmark workload's SoloProgram (it does not depend on the model), compiled by the host factories of a small env"""
  from gym_solo_amd.envs.solo8v2vanilla import Solo8VanillaConfig, Solo8VanillaEnv
  from gym_solo_amd.workloads import register_benchmark_workload
  cfg = Solo8VanillaConfig()
  cfg.dtype, cfg.num_envs, cfg.settle_steps = 'float64', 8, 5
  env = Solo8VanillaEnv(config=cfg, copy_outputs=False)
  register_benchmark_workload(env, max_steps=1000)
  env._ensure_program()
  prog = env.engine.program
  env._close()
  return prog


@pytest.mark.parametrize('case', ['seed0', 'seed1'])
def test_fused_launch_with_outputs_matches_oracle_f64(torch, case):
  """One rollout(record=True) of 20 steps of the benchmark workload at steps_per_launch = 20 - the step-loop kernel with its
  LDS-staged constants and the output epilogue, another code path than the single-step launches: the final state against the
  oracle (1e-9), and every recorded observation and reward against so.observations / so.factory_reward evaluated on the
  oracle's state of that step (1e-9).  Measured on the MI355X: state 6.1e-12 / 9.0e-11, observations 5.6e-13 / 1.4e-11,
  rewards 2.6e-14 / 8.3e-13 (seed0 / seed1)."""
  from env_cases import BENCH_REWARD
  from oracle import solo_oracle as so
  ref = reference_run(case, steps=20, action_seed=1)
  ref['live'].check(case)
  ca, _ = make_abi('float64', steps_per_launch=20)
  eng = _engine(ca, ref['ma'])
  eng.set_program(_bench_program(torch))
  plan = eng.plan(20)
  assert plan['steps_per_launch'] == 20 and plan['launches'] == 1, plan
  np.testing.assert_allclose(eng.snapshot.cpu().numpy()[:, :29], np.tile(ref['snap'][:, :29], (N, 1)), rtol=0, atol=1e-9)
  obs, rew, done = eng.rollout(torch.as_tensor(np.stack(ref['acts']), device='cuda'), abi.STEP_ALL, record=True)
  eng.synchronize()
  obs, rew, done = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()
  err = np.abs(eng.state.cpu().numpy()[:, :29] - ref['states'][-1][:, :29]).max()
  err_obs = max(np.abs(obs[k] - so.observations(ref['states'][k], OBS_SPEC)).max() for k in range(20))
  err_rew = max(np.abs(rew[k] - so.factory_reward(ref['states'][k], [(1, BENCH_REWARD)])).max() for k in range(20))
  diverged = eng.stats.cpu().numpy()[5]
  eng.close()
  print('model space fused ({}): state {:.2e}, observations {:.2e}, rewards {:.2e}'.format(case, err, err_obs, err_rew))
  assert diverged == 0 and not done.any()
  assert obs.shape == (20, N, 21)
  assert err <= 1e-9 and err_obs <= 1e-9 and err_rew <= 1e-9, (case, err, err_obs, err_rew)


_TERRAIN_REF = {}


def terrain_reference(case, n=N):
  """The ORACLE's side of the bumpy-terrain case (no GPU), with per-robot friction U(0.3, 1.0) and base-mass scale
  U(0.8, 1.2): its snapshot after a 300-step settle loop (the randomised robots fold their legs while they drop; the first
  sphere reaches the bumps within the next 20 steps), the landed states it reaches 200 steps later, then 25 steps of per-robot
  random actions - the state before and after every step, and for every robot-step whether it is REGULAR: the oracle's own
  twin, lifted by 1e-15 m before the step, stays within 1e-10 of it (a penetration d enters the normal rows as d / dt and
  turns a body through d / (dt r), r >= the smallest sphere radius, 0.016 m: a gain of up to 1e3 / 0.016 = 6e4; beyond that
  the step sits on a discontinuity of the solve, and no arithmetic can be held to a bar on it)."""
  if case in _TERRAIN_REF:
    return _TERRAIN_REF[case]
  import helpers
  from oracle import solo_oracle as so
  terrain = helpers.bumpy_terrain(seed=4)
  rng = np.random.default_rng(77)
  params = np.zeros((n, 4))
  params[:, 0] = rng.uniform(0.3, 1.0, n)
  params[:, 1] = rng.uniform(0.8, 1.2, n)
  ca, _ = make_abi('float64', settle_steps=300)
  ma = ms.get_model(case).to_abi()
  ph = so.OraclePhysics(ca, ma, terrain=terrain)
  snap = ph.settle(n, params=params, threads=THREADS)
  twin = ph.initial_state(n)
  twin[:, abi.S_POS + 2] += 1e-15
  hold = np.tile(np.array(list(ca.settle_targets)), (n, 1)) / ca.action_scale
  for _ in range(300):
    ph.step(twin, hold, params, threads=THREADS)
  settle_twin = np.abs(twin[:, :29] - snap[:, :29]).max()
  st = snap.copy()
  for _ in range(200):
    ph.step(st, hold, params, threads=THREADS)
  at_rest = ms.Liveness(ph, ma, ca)
  at_rest.see(st, hold, params, every=4)
  rng = np.random.default_rng(302)
  live = ms.Liveness(ph, ma, ca)
  acts, before, after, regular = [], [], [], []
  for k in range(25):
    a = random_actions(rng, n)
    live.see(st, a, params, every=4)
    twin = st.copy()
    twin[:, abi.S_POS + 2] += 1e-15
    before.append(st.copy())
    ph.step(st, a, params, threads=THREADS)
    ph.step(twin, a, params, threads=THREADS)
    acts.append(a)
    after.append(st.copy())
    regular.append(np.abs(twin[:, :29] - st[:, :29]).max(axis=1) <= 1e-10)
  _TERRAIN_REF[case] = dict(ca=ca, ma=ma, terrain=terrain, params=params, snap=snap, settle_twin=settle_twin, at_rest=at_rest,
                            live=live, acts=acts, before=before, after=after, regular=np.array(regular))
  return _TERRAIN_REF[case]


@pytest.mark.parametrize('case', ['seed2', 'offdiag_base', 'upper_spheres'])
def test_per_robot_parameters_and_terrain_f64(torch, case):
  """Per-robot friction U(0.3, 1.0) and base-mass scale U(0.8, 1.2) - mass_scale multiplies all six base_I entries, three of
  which are zero on the default model - on the bumpy heightfield, at the bars of
  test_random_configuration_terrain_and_parameters_together_f64 (settle 1e-8, steps 3e-8).  upper_spheres takes the BODY_UPPER
  sphere transform through the bilinear heightfield branch.

  The form is the well-conditioned one.  A 500-step settle onto the 2 cm bumps, or 25 chained flailing steps on them, are
  ill-conditioned in the ORACLE ITSELF (lifting the start by 1e-15 m moves its own 500-step snapshot by 1e-9 ... 1e-3, and its
  state after 25 chained steps by up to 5e-10 - measured on the oracle alone), so: the engine's settle loop runs 300 steps -
  the robots, each with its own base mass, fold their legs while they drop, and touch down within 20 steps after it; the
  oracle's twin stays within 1e-14 - and is compared on every robot at 1e-8; then the engine is given the oracle's landed
  per-robot state before EACH of 25 random-action steps and compared with the oracle after it at 3e-8, on the regular
  robot-steps (terrain_reference: decided by the oracle alone, the way tests/test_gpu_parity_scale.py chooses its robots),
  which must be at least 99 % of them (oracle: 99.94 ... 100 %).  On the oracle's steps: >= 3 touching spheres in >= 75 % of the robot-steps; on
  upper_spheres an upper-link sphere touches the terrain at rest and in >= 10 % of them; the edge models leave the default
  model's trajectory.
  Measured on the MI355X (seed2 / offdiag_base / upper_spheres): settle 5.4e-14 / 5.0e-14 / 5.4e-14; the 25 steps 6.0e-12 / 4.1e-12 / 1.2e-11 on
  the regular robot-steps (99.9 / 100 / 100 %), and 1.1e-9 / 4.1e-12 / 3.4e-11 on all of them."""
  ref = terrain_reference(case)
  ca, ma, params, live = ref['ca'], ref['ma'], ref['params'], ref['live']
  assert ref['settle_twin'] <= 1e-14, ref['settle_twin']
  live.check(case)
  if case == 'upper_spheres':
    assert ref['at_rest'].upper >= 0.5 * ref['at_rest'].pairs, str(ref['at_rest'])
  if case in ms.EDGE_MODELS:
    assert np.abs(ref['after'][-1][:, :29] - terrain_reference('default')['after'][-1][:, :29]).max() > 1e-6
  regular = ref['regular']
  assert regular.mean() >= 0.99, regular.mean()
  eng = _engine(ca, ma)
  eng.set_params(abi.PARAM_FRICTION, torch.as_tensor(params[:, 0], device='cuda').contiguous())
  eng.set_params(abi.PARAM_BASE_MASS_SCALE, torch.as_tensor(params[:, 1], device='cuda').contiguous())
  eng.set_terrain(ref['terrain'])   # (re-runs the settle loop: on the new ground, with the per-robot parameters)
  err_settle = np.abs(eng.snapshot.cpu().numpy()[:, :29] - ref['snap'][:, :29]).max()
  err = err_all = 0.0
  for k in range(25):
    eng.state.copy_(torch.as_tensor(ref['before'][k], device='cuda'))
    eng.step(torch.as_tensor(ref['acts'][k], device='cuda'), abi.STEP_PHYSICS)
    d = np.abs(eng.state.cpu().numpy()[:, :29] - ref['after'][k][:, :29]).max(axis=1)
    err, err_all = max(err, d[regular[k]].max()), max(err_all, d.max())
  diverged = eng.stats.cpu().numpy()[5]
  eng.close()
  print('model space terrain + parameters ({}): settle {:.2e} (oracle twin {:.1e}), 25 steps {:.2e} on the {:.1f} % regular robot-steps '
        '({:.2e} on all); {}'.format(case, err_settle, ref['settle_twin'], err, 100 * regular.mean(), err_all, live))
  assert diverged == 0
  assert err_settle <= 1e-8 and err <= 3e-8, (case, err_settle, err)


@pytest.mark.parametrize('case', ['seed%d' % s for s in ms.RANDOM_SEEDS] + ['offdiag_legs'])
def test_single_step_f32(torch, case):
  """The f32 kernel on non-default models: one step of the f32 engine against the f64 oracle from the engine's own state after
  40 decorrelating steps, at the bars of test_single_step_f32_over_random_configurations (3e-6 on pose and joint angles, 2e-3 on
  the velocities).  Measured on the MI355X over the four models: positions 1.2e-7 ... 1.4e-7, velocities 2.1e-5 ... 3.9e-5 -
  what the default model gives over random configurations (1.2e-7 ... 2.8e-7, 2e-5 ... 1.5e-4)."""
  from oracle import solo_oracle as so
  ca, _ = make_abi('float32')
  ca64, _ = make_abi('float64')
  ma = ms.get_model(case).to_abi()
  eng = _engine(ca, ma)
  ph = so.OraclePhysics(ca64, ma)
  rng = np.random.default_rng(17)
  for k in range(40):
    eng.step(torch.as_tensor(random_actions(rng, N), device='cuda', dtype=torch.float32), abi.STEP_PHYSICS)
  st = eng.state.cpu().numpy().astype(np.float64)
  a = random_actions(rng, N).astype(np.float32)
  live = ms.Liveness(ph, ma, ca64)
  live.see(st, a.astype(np.float64), every=4)
  ph.step(st, a.astype(np.float64), threads=THREADS)
  eng.step(torch.as_tensor(a, device='cuda'), abi.STEP_PHYSICS)
  got = eng.state.cpu().numpy().astype(np.float64)
  diverged = eng.stats.cpu().numpy()[5]
  eng.close()
  err = np.abs(got[:, :29] - st[:, :29])
  print('model space f32 ({}): positions {:.2e}, velocities {:.2e}; {}'.format(case, err[:, :15].max(), err[:, 15:29].max(), live))
  assert diverged == 0 and np.isfinite(got[:, :29]).all()
  live.check(case)
  assert err[:, :15].max() < 3e-6, (case, err[:, :15].max())
  assert err[:, 15:29].max() < 2e-3, (case, err[:, 15:29].max())


@pytest.mark.parametrize('mode', ['torque', 'pd'])
@pytest.mark.parametrize('case', ['seed0', 'offdiag_legs'])
def test_torque_in_the_air_equals_forward_dynamics(torch, case, mode):
  """The air identity of tests/test_gpu_control.py on non-default models: engine(S, tau) - oracle_motors_off(S) ==
  dt (fd(S, tau) - fd(S, 0)) with the oracle's CRBA / RNEA forward dynamics, 1e-12 - nothing but the inertia terms acts.
  Measured on the MI355X: joint rates <= 4.1e-14, base twist <= 1.5e-15."""
  from control_cases import air_identity_errors, air_states
  from gym_solo_amd.model import DOF_TO_JOINT
  from oracle import solo_oracle as so
  ca, _ = make_abi('float64')
  ca0, _ = make_abi('float64', motor_torque_limit=0.0)
  ma = ms.get_model(case).to_abi()
  rng = np.random.default_rng(31 if mode == 'torque' else 32)
  S = air_states(rng, N, ma, ca.joint_limit_margin)
  L = ca.motor_torque_limit
  eng = _engine(ca, ma)
  if mode == 'torque':
    tau = rng.uniform(-0.99 * L, 0.99 * L, (N, abi.NUM_DOF))
    a = np.zeros((N, abi.NUM_JOINTS))
    a[:, DOF_TO_JOINT] = tau
    eng.set_control('torque')
  else:
    kp, kd = rng.uniform(1.0, 4.0, abi.NUM_JOINTS), rng.uniform(0.01, 0.05, abi.NUM_JOINTS)
    a = rng.uniform(-3, 3, (N, abi.NUM_JOINTS))
    q, qd = S[:, abi.S_Q:abi.S_Q + 8], S[:, abi.S_QD:abi.S_QD + 8]
    tau = np.clip(kp[DOF_TO_JOINT] * (a[:, DOF_TO_JOINT] - q) - kd[DOF_TO_JOINT] * qd, -L, L)
    eng.set_control('pd', kp=kp, kd=kd)
  eng.state.copy_(torch.as_tensor(S, device='cuda'))
  eng.snapshot.copy_(eng.state)
  eng.step(torch.as_tensor(a, device='cuda'), abi.STEP_PHYSICS)
  got = eng.state.cpu().numpy()
  diverged = eng.stats.cpu().numpy()[5]
  eng.close()
  ref = S.copy()
  so.OraclePhysics(ca0, ma).step(ref, np.zeros((N, abi.NUM_JOINTS)), threads=THREADS)
  worst_qd, worst_twist = air_identity_errors(S, got, ref, tau, so.OraclePhysics(ca, ma), ca.dt)
  print('model space air identity ({}, {}): joint rates {:.2e}, base twist {:.2e}'.format(case, mode, worst_qd, worst_twist))
  assert diverged == 0
  assert worst_qd <= 1e-12 and worst_twist <= 1e-12, (worst_qd, worst_twist)
  assert np.abs(got[:, abi.S_QD:abi.S_QD + 8] - ref[:, abi.S_QD:abi.S_QD + 8]).max() > 1e-3   # (tau did something)


@pytest.mark.parametrize('case', ['seed0', 'offdiag_legs'])
def test_zero_torque_equals_oracle_with_motors_off(torch, case):
  """from the model's settled snapshot, 60 steps of tau = 0 against the oracle with motor_torque_limit = 0 (the robot
  collapses onto the ground: contact rows live), 1e-9.  Measured on the MI355X: 5.4e-13 / 5.9e-13."""
  from oracle import solo_oracle as so
  ca, _ = make_abi('float64')
  ca0, _ = make_abi('float64', motor_torque_limit=0.0)
  ma = ms.get_model(case).to_abi()
  eng = _engine(ca, ma)
  eng.set_control('torque')
  st = eng.state.cpu().numpy().copy()
  ph = so.OraclePhysics(ca0, ma)
  zero = torch.zeros(N, abi.NUM_JOINTS, device='cuda', dtype=torch.float64)
  tg = np.tile(np.array(list(ca.settle_targets)), (N, 1))
  for _ in range(60):
    eng.step(zero, abi.STEP_PHYSICS)
    ph.step(st, tg, threads=THREADS)
  got = eng.state.cpu().numpy()
  diverged = eng.stats.cpu().numpy()[5]
  eng.close()
  err = np.abs(got[:, :abi.S_RETURN] - st[:, :abi.S_RETURN]).max()
  print('model space zero torque ({}): {:.2e}'.format(case, err))
  assert st[:, abi.S_POS + 2].max() < 0.2   # (it lies on the ground)
  assert diverged == 0 and err <= 1e-9, (case, err)


@pytest.mark.parametrize('ground,dtype', [('flat', 'float64'), ('incline', 'float64'), ('flat', 'float32')])
@pytest.mark.parametrize('case', ['upper_spheres', 'seed0'])
def test_contact_record_parity_against_step_debug(torch, case, ground, dtype):
  """The one-step record parity of tests/test_gpu_contact.py (tests/contact_cases.py; same bars) on models whose sphere -> link
  layout is not the default's: the record's sphere -> link mapping and its forces follow the model, and an upper-link sphere is
  among the touching ones (10 flailing steps from the folded settle pose: after the 30 of tests/test_gpu_contact.py the legs
  have unfolded and the knees are off the ground - counted on the oracle).  Measured on the MI355X, worst |df| over 256 robots (upper_spheres / seed0): f64 flat 2.9e-12 / 2.8e-12 N,
  f64 incline 4.3e-11 / 3.1e-11 N (bar 1e-6 N); f32 flat 1.4e-3 / 9.8e-4 N (bar 0.5 N)."""
  import contact_cases as cc
  ma = ms.get_model(case).to_abi()
  touched, diverged = cc.one_step_parity_against_step_debug(torch, ground, dtype, ma, N, every=1, flail_steps=10)
  assert diverged == 0
  assert touched & {s for s in range(abi.MAX_SPHERES) if ma.sphere_body[s] != 0 and ma.sphere_body[s] % 2 == 1}


@pytest.mark.parametrize('mutate,fragment', ms.invalid_models(), ids=[m.__name__.strip('_') for m, _ in ms.invalid_models()])
def test_models_outside_the_family_are_rejected_by_create(torch, mutate, fragment):
  """one mutation per clause of validate_model: solo_engine_create returns SOLO_ERR_UNSUPPORTED_MODEL, leaves no handle, and
  solo_last_create_error() names the clause"""
  from gym_solo_amd.engine import load_library
  lib = load_library()
  ca, ma = make_abi('float64')
  mutate(ma)
  h = C.c_void_p()
  assert lib.solo_engine_create(C.byref(ca), C.byref(ma), 4, 0, C.byref(h)) == abi.ERR_UNSUPPORTED_MODEL
  assert not h.value
  assert fragment.encode() in lib.solo_last_create_error()
