"""GPU suite of the joint control modes (solo_engine_set_control: TORQUE, PD) through the C-ABI on the MI355X.

The oracle has no torque mode; parity comes from identities that hold with the oracle as it is:
  (a) zero torque == the oracle with motor_torque_limit = 0 (a motor row clamped to 0 contributes nothing);
  (b) saturated torque +-L == the oracle's position motors driven to saturation (targets +-1e3 rad: every motor row sits
      at +-L dt from the first sweep on - motor rows are solved first - which is exactly the pinned torque impulse);
  (c) arbitrary torque in the air (and the PD law at random gains) against the oracle's own forward dynamics;
  (d) PD == torque fed the PD law's torque computed on the host from the same state.
"""
import numpy as np
import pytest

from gym_solo_amd import abi
from helpers import make_abi

pytestmark = pytest.mark.gpu

N = 4096


@pytest.fixture(scope='module')
def torch():
  import torch
  if not torch.cuda.is_available():
    pytest.fail('GPU tests need a visible MI355X')
  return torch


def _engine(ca, ma, n=N):
  from gym_solo_amd.engine import Engine
  return Engine(ca, ma, n)


def _signs(rng, n):
  return rng.choice([-1.0, 1.0], (n, abi.NUM_JOINTS))


def _limit_distance(ma, st):
  q = st[:, abi.S_Q:abi.S_Q + abi.NUM_DOF]
  lo, hi = np.array(list(ma.joint_lower)), np.array(list(ma.joint_upper))
  return np.min(np.minimum(q - lo, hi - q))


def _joint_to_dof(a):
  from gym_solo_amd.model import DOF_TO_JOINT
  return a[:, DOF_TO_JOINT]


def _dof_to_joint(t):
  from gym_solo_amd.model import DOF_TO_JOINT
  out = np.zeros((t.shape[0], abi.NUM_JOINTS))
  out[:, DOF_TO_JOINT] = t
  return out


def test_zero_torque_equals_oracle_with_motors_off(torch):
  """(a): from the settled snapshot, 60 steps of tau = 0 against the oracle with motor_torque_limit = 0 (the robot
  collapses onto the ground: contact rows live)."""
  from oracle import solo_oracle as so
  ca, ma = make_abi('float64')
  eng = _engine(ca, ma)
  eng.set_control('torque')
  st = eng.state.cpu().numpy().copy()
  ca0, _ = make_abi('float64', motor_torque_limit=0.0)
  ph = so.OraclePhysics(ca0, ma)
  zero = torch.zeros(N, abi.NUM_JOINTS, device='cuda', dtype=torch.float64)
  tg = np.tile(np.array(list(ca.settle_targets)), (N, 1))
  for _ in range(60):
    eng.step(zero, abi.STEP_PHYSICS)
    ph.step(st, tg, threads=16)
  got = eng.state.cpu().numpy()
  assert st[:, abi.S_POS + 2].max() < 0.2   # (it fell)
  np.testing.assert_allclose(got[:, :abi.S_RETURN], st[:, :abi.S_RETURN], rtol=0, atol=1e-9)
  assert eng.stats.cpu().numpy()[5] == 0


def _randomised_params(torch, eng, ca, rng):
  params = np.zeros((eng.num_envs, 4))
  params[:, 0], params[:, 1] = ca.lateral_friction, 1.0
  half = np.arange(eng.num_envs) % 2 == 1
  params[half, 0] = rng.uniform(0.2, 1.2, half.sum())
  params[half, 1] = rng.uniform(0.7, 1.3, half.sum())
  eng.set_params(abi.PARAM_FRICTION, torch.as_tensor(params[:, 0], device='cuda', dtype=eng.tdtype))
  eng.set_params(abi.PARAM_BASE_MASS_SCALE, torch.as_tensor(params[:, 1], device='cuda', dtype=eng.tdtype))
  return params


def test_saturated_torque_equals_oracle_with_saturated_motors(torch):
  """(b): tau_j = s_j L (s = +-1 per robot, per step and per joint) against the oracle in POSITION_CONTROL with targets
  s_j 1e3 rad, 60 steps on the ground; half the robots with their own friction and base mass."""
  from oracle import solo_oracle as so
  ca, ma = make_abi('float64')
  eng = _engine(ca, ma)
  rng = np.random.default_rng(3)
  params = _randomised_params(torch, eng, ca, rng)
  eng.set_control('torque')
  st = eng.state.cpu().numpy().copy()
  ph = so.OraclePhysics(ca, ma)
  L = ca.motor_torque_limit
  for _ in range(60):
    s = _signs(rng, N)
    eng.step(torch.as_tensor(s * L, device='cuda'), abi.STEP_PHYSICS)
    ph.step(st, s * 1e3 / ca.action_scale, params, threads=16)
    assert _limit_distance(ma, st) > ca.joint_limit_margin   # no joint-limit row is live: limit rows interleave with motor rows
  got = eng.state.cpu().numpy()
  np.testing.assert_allclose(got[:, :abi.S_RETURN], st[:, :abi.S_RETURN], rtol=0, atol=1e-9)


def test_saturated_torque_f32_one_step_error(torch):
  """(b) in f32, at the one-step bars of tests/test_gpu_parity_f32.py (f32 and f64 trajectories decorrelate, so the
  comparison is local): every 10 steps of a 60-step saturated-torque run the oracle (f64, saturated position motors)
  steps once from the f32 engine's state."""
  from oracle import solo_oracle as so
  ca, ma = make_abi('float32')
  ca64, _ = make_abi('float64')
  eng = _engine(ca, ma)
  rng = np.random.default_rng(3)
  params = _randomised_params(torch, eng, ca, rng)
  eng.set_control('torque')
  ph = so.OraclePhysics(ca64, ma)
  L = ca.motor_torque_limit
  bounds = dict(pos=((abi.S_POS, 3), 6e-8), quat=((abi.S_QUAT, 4), 5e-7), q=((abi.S_Q, 8), 2e-6),
                angvel=((abi.S_ANGVEL, 3), 2e-4), linvel=((abi.S_LINVEL, 3), 3e-5), qd=((abi.S_QD, 8), 2e-3))
  for k in range(60):
    s = _signs(rng, N)
    if k % 10 == 0:
      st = eng.state.cpu().numpy().astype(np.float64)
      ph.step(st, s * 1e3 / ca64.action_scale, params, threads=16)
      assert _limit_distance(ma, st) > ca.joint_limit_margin
    eng.step(torch.as_tensor(s * L, device='cuda', dtype=torch.float32), abi.STEP_PHYSICS)
    if k % 10 == 0:
      got = eng.state.cpu().numpy().astype(np.float64)
      for name, ((o, w), mx) in bounds.items():
        err = np.abs(got[:, o:o + w] - st[:, o:o + w]).max()
        assert err <= mx, (k, name, err, mx)


def _pd_gains(rng):
  kp = rng.uniform(1.0, 4.0, abi.NUM_JOINTS)
  kd = rng.uniform(0.01, 0.05, abi.NUM_JOINTS)
  return kp, kd


def _pd_torque(st, cmd, kp, kd, L):
  """The PD law on the host, dof order: clamp(kp (cmd - q) - kd qd, +-L)."""
  q = st[:, abi.S_Q:abi.S_Q + abi.NUM_DOF]
  qd = st[:, abi.S_QD:abi.S_QD + abi.NUM_DOF]
  kpd, kdd = _joint_to_dof(kp[None, :])[0], _joint_to_dof(kd[None, :])[0]
  return np.clip(kpd * (_joint_to_dof(cmd) - q) - kdd * qd, -L, L)


def test_pd_equals_torque_fed_the_same_torque(torch):
  """(d): from the same state S, one PD step == one torque step fed tau_host(S), at 10 states along a 100-step PD run on
  the ground."""
  ca, ma = make_abi('float64')
  rng = np.random.default_rng(5)
  kp, kd = _pd_gains(rng)
  pd, tq = _engine(ca, ma), _engine(ca, ma)
  pd.set_control('pd', kp=kp, kd=kd)
  tq.set_control('torque')
  settle = np.array(list(ca.settle_targets))
  worst = 0.0
  for k in range(100):
    a = settle[None, :] + rng.uniform(-0.5, 0.5, (N, abi.NUM_JOINTS))
    if k % 10 == 0:
      S = pd.state.clone()
      tau = _pd_torque(S.cpu().numpy(), a, kp, kd, ca.motor_torque_limit)
      tq.state.copy_(S)
      tq.step(torch.as_tensor(_dof_to_joint(tau), device='cuda'), abi.STEP_PHYSICS)
    pd.step(torch.as_tensor(a, device='cuda'), abi.STEP_PHYSICS)
    if k % 10 == 0:
      d = (pd.state[:, :abi.S_RETURN] - tq.state[:, :abi.S_RETURN]).abs().max().item()
      worst = max(worst, d)
  assert worst <= 1e-13, worst
  assert pd.stats.cpu().numpy()[5] == 0


def _bench_env(torch, dtype='float64', n=N, **kw):
  from gym_solo_amd.envs.solo8v2vanilla import Solo8VanillaConfig, Solo8VanillaEnv
  from gym_solo_amd.workloads import register_benchmark_workload
  cfg = Solo8VanillaConfig()
  cfg.dtype, cfg.num_envs = dtype, n
  max_steps = kw.pop('max_steps', 1000)
  normalize = kw.pop('normalize_actions', False)
  for k, v in kw.items():
    setattr(cfg, k, v)
  env = Solo8VanillaEnv(config=cfg, normalize_actions=normalize)
  register_benchmark_workload(env, max_steps=max_steps)
  env._ensure_program()
  return env


def test_default_position_mode_is_unchanged(torch):
  """An engine that never calls set_control and one that went position -> torque -> position and was reset: state, obs,
  reward and done bit-identical over 100 steps of the benchmark workload, and the same kernel name."""
  a = _bench_env(torch, max_steps=40, auto_reset=True)
  b = _bench_env(torch, max_steps=40, auto_reset=True)
  name = a.engine.kernel_name
  b.engine.set_control('torque')
  assert b.engine.kernel_name == 'solo_ctl_step_kernel<double, true>'
  b.engine.set_control('position')
  b.engine.reset()
  assert b.engine.kernel_name == name and name.startswith('solo_step_kernel<double')
  g = torch.Generator(device='cuda').manual_seed(11)
  for _ in range(100):
    act = (torch.rand(N, 12, device='cuda', dtype=torch.float64, generator=g) * 2 - 1) * 6.28
    for e in (a, b):
      e.engine.step(act, abi.STEP_ALL)
    for t in ('state', 'obs', 'reward', 'done'):
      assert torch.equal(getattr(a.engine, t), getattr(b.engine, t)), t
  assert torch.equal(a.engine.targets, b.engine.targets)
  a._close(); b._close()


def _control_kwargs(mode, rng):
  if mode == 'pd':
    kp, kd = _pd_gains(rng)
    return dict(control_mode='pd', pd_kp=kp, pd_kd=kd)
  return dict(control_mode='torque')


def _actions(torch, mode, k, n, dtype, g, settle):
  tdt = torch.float32 if dtype == 'float32' else torch.float64
  r = torch.rand(k, n, 12, device='cuda', dtype=tdt, generator=g) * 2 - 1
  if mode == 'torque':
    return r * 2.5   # (some beyond the limit: clamped)
  return torch.as_tensor(settle, device='cuda', dtype=tdt) + 0.6 * r


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('mode', ['torque', 'pd'])
def test_fused_rollouts_equal_single_steps(torch, mode, dtype):
  """rollout(record=True) of 30 steps with steps_per_launch = 7, and of 300 steps with the engine's own geometry (two
  slices), equal single steps exactly, auto-resets included (TimeBased(11))."""
  rng = np.random.default_rng(2)
  kw = _control_kwargs(mode, rng)
  settle = None
  for k, spl in ((30, 7), (300, -1)):
    out = {}
    for fused in (False, True):
      env = _bench_env(torch, dtype, max_steps=11, auto_reset=True, steps_per_launch=spl if fused else 1, **kw)
      eng = env.engine
      settle = np.array(list(eng.cfg.settle_targets))
      if fused and spl == -1:
        p = eng.plan(k)
        assert p['slices'] == 2 and p['migrate_steps'] == 0, p
      g = torch.Generator(device='cuda').manual_seed(7)
      acts = _actions(torch, mode, k, eng.num_envs, dtype, g, settle)
      if not fused:
        obs, rew, done = [], [], []
        for i in range(k):
          eng.step(acts[i].contiguous(), abi.STEP_ALL)
          obs.append(eng.obs.clone()); rew.append(eng.reward.clone()); done.append(eng.done.clone())
        rec = (torch.stack(obs), torch.stack(rew), torch.stack(done))
      else:
        rec = eng.rollout(acts, abi.STEP_ALL, record=True)
      eng.synchronize()
      out[fused] = [t.cpu().numpy() for t in rec] + [eng.state.cpu().numpy(), eng.targets.cpu().numpy(),
                                                     eng.term_count.cpu().numpy(), eng.stats.cpu().numpy()]
      env._close()
    for x, y in zip(out[False][:-1], out[True][:-1]):
      np.testing.assert_array_equal(x, y)
    # (the episodic statistics are sums over all robots accumulated with atomics: their order, and with it the last bit,
    # depends on the launch geometry - in position mode too)
    np.testing.assert_allclose(out[False][-1], out[True][-1], rtol=1e-13, atol=0)
    assert out[False][2].sum() == (k // 12) * N


@pytest.mark.parametrize('mode', ['torque', 'pd'])
def test_auto_reset_restores_snapshot_and_reset_command(torch, mode):
  """TimeBased(11) + auto_reset: the restored robots equal the snapshot bit for bit, and their command is the mode's reset
  command (torque: 0; PD: the settle pose).  A get_state / set_state round trip resumes bit for bit."""
  rng = np.random.default_rng(4)
  env = _bench_env(torch, max_steps=11, auto_reset=True, **_control_kwargs(mode, rng))
  eng = env.engine
  settle = np.array(list(eng.cfg.settle_targets))
  reset_cmd = np.zeros(12) if mode == 'torque' else settle
  np.testing.assert_array_equal(eng.targets.cpu().numpy(), np.tile(reset_cmd, (N, 1)))   # (set_control's command)
  g = torch.Generator(device='cuda').manual_seed(3)
  acts = _actions(torch, mode, 24, N, 'float64', g, settle)
  for i in range(12):
    eng.step(acts[i].contiguous(), abi.STEP_ALL)
  assert eng.done.cpu().numpy().all()
  np.testing.assert_array_equal(eng.state[:, :abi.S_RETURN].cpu().numpy(), eng.snapshot[:, :abi.S_RETURN].cpu().numpy())
  np.testing.assert_array_equal(eng.targets.cpu().numpy(), np.tile(reset_cmd, (N, 1)))
  ck = eng.get_state()
  for i in range(12, 18):
    eng.step(acts[i].contiguous(), abi.STEP_ALL)
  first = eng.state.clone()
  eng.set_state(ck)
  for i in range(12, 18):
    eng.step(acts[i].contiguous(), abi.STEP_ALL)
  assert torch.equal(first, eng.state)
  eng.step(acts[18].contiguous(), abi.STEP_ALL)
  eng.reset()
  np.testing.assert_array_equal(eng.targets.cpu().numpy(), np.tile(reset_cmd, (N, 1)))
  assert eng.control['mode'] == mode
  env._close()


def test_env_and_facade_torque_and_pd(torch):
  """Solo8VanillaEnv(control_mode='torque', normalize_actions=True) stepping a = 0.5 == the engine stepping tau = 0.5 L;
  its obs / reward / done == the oracle's numpy reductions on the engine's own state; the facade's TORQUE_CONTROL and
  PD_CONTROL calls + stepSimulation == the engine calls."""
  from gym_solo_amd import client as p
  from oracle import solo_oracle as so
  from env_cases import BENCH_REWARD
  n = 256
  env = _bench_env(torch, n=n, control_mode='torque', normalize_actions=True, max_steps=1000)
  # (the reference engine: the same configuration - the settle loop's arithmetic depends on the position-mode action
  # scale, which normalize_actions sets -, commanding torques directly)
  ref = _bench_env(torch, n=n, control_mode='torque', normalize_actions=True, max_steps=1000)
  ref.engine.set_control('torque', action_scale=1.0)
  L = env.config.motor_torque_limit
  assert tuple(env.action_space.high) == (1.0,) * 12
  plain = _bench_env(torch, n=8, control_mode='torque', max_steps=1000)
  assert tuple(plain.action_space.high) == (np.float32(L),) * 12
  plain._close()
  for _ in range(5):
    o, r, d, _ = env.step(torch.full((n, 12), 0.5, device='cuda', dtype=torch.float64))
    ref.engine.step(torch.full((n, 12), 0.5 * L, device='cuda', dtype=torch.float64), abi.STEP_ALL)
  assert torch.equal(env.engine.state, ref.engine.state)
  st = env.engine.state.cpu().numpy()
  oo = so.observations(st, [('torso_imu', {}), ('motor_encoder', {})])
  np.testing.assert_allclose(o.cpu().numpy(), oo, rtol=0, atol=1e-12)
  np.testing.assert_allclose(r.cpu().numpy(), so.factory_reward(st, [(1, BENCH_REWARD)]), rtol=0, atol=1e-12)
  assert not d.cpu().numpy().any()
  # the facade, against the engine calls
  rng = np.random.default_rng(9)
  kp, kd = _pd_gains(rng)
  tau = torch.as_tensor(rng.uniform(-1, 1, (n, 12)), device='cuda')
  tgt = torch.as_tensor(np.array(list(ref.engine.cfg.settle_targets)) + rng.uniform(-0.3, 0.3, (n, 12)), device='cuda')
  c = env.client
  c.setJointMotorControlArray(1, list(range(12)), p.TORQUE_CONTROL, forces=tau)
  c.stepSimulation()
  c.setJointMotorControlArray(1, list(range(12)), p.PD_CONTROL, targetPositions=tgt, positionGains=kp, velocityGains=kd)
  c.stepSimulation()
  assert env.engine.control['mode'] == 'pd'
  e = ref.engine
  e.state.copy_(torch.as_tensor(st, device='cuda'))
  e.set_control('torque', action_scale=1.0)
  e.set_targets(tau)
  e.step(None, abi.STEP_PHYSICS)
  e.set_control('pd', kp=kp, kd=kd)
  e.set_targets(tgt)
  e.step(None, abi.STEP_PHYSICS)
  assert torch.equal(env.engine.state[:, :abi.S_RETURN], e.state[:, :abi.S_RETURN])
  env._close(); ref._close()


def test_beyond_resident_robots_torque(torch):
  """8192 robots (more than the 4096 resident waves) in torque mode: no migration, and the second half, given the first
  half's states and actions, ends identical to the first half."""
  ca, ma = make_abi('float64')
  n = 2 * N
  eng = _engine(ca, ma, n)
  eng.set_control('torque')
  assert eng.plan(20)['migrate_steps'] == 0
  g = torch.Generator(device='cuda').manual_seed(1)
  a = (torch.rand(20, N, 12, device='cuda', dtype=torch.float64, generator=g) * 2 - 1) * 2.5
  eng.state[N:].copy_(eng.state[:N])
  eng.rollout(torch.cat([a, a], dim=1).contiguous(), abi.STEP_PHYSICS)
  eng.synchronize()
  assert torch.equal(eng.state[:N], eng.state[N:])


def test_rejections(torch):
  """set_control rejects an invalid mode, negative gains, and a control mode together with the residual threshold,
  warm start or explicit migration: SOLO_ERR_INVALID_ARG -> ValueError, the previous mode stays in force."""
  import ctypes as C
  ca, ma = make_abi('float64', settle_steps=10)
  eng = _engine(ca, ma, 64)
  c = abi.SoloControl()
  c.mode, c.action_scale = 7, 1.0
  assert eng.lib.solo_engine_set_control(eng._handle(), C.byref(c), None) == abi.ERR_INVALID_ARG
  with pytest.raises(ValueError):
    eng.set_control('pd', kp=-1.0, kd=0.1)
  with pytest.raises(ValueError):
    eng.set_control('velocity')
  assert eng.control['mode'] == 'position'
  for kw in (dict(solver_residual_threshold=1e-7), dict(solver_residual_threshold=1e-7, solver_warm_start=1.0), dict(migrate_steps=5)):
    ca2, _ = make_abi('float64', settle_steps=10, **kw)
    e2 = _engine(ca2, ma, 64)
    c.mode = abi.CTRL_TORQUE
    assert e2.lib.solo_engine_set_control(e2._handle(), C.byref(c), None) == abi.ERR_INVALID_ARG
    with pytest.raises(ValueError):
      e2.set_control('torque')
    e2.set_control('position')   # (position mode is always legal)
    e2.close()
  eng.close()


@pytest.mark.parametrize('mode', ['torque', 'pd'])
def test_arbitrary_torque_in_the_air_equals_forward_dynamics(torch, mode):
  """(c): robots 2 m up from random q, qd, base twist and orientation (no contact, no live joint limit), gravity and
  damping on; one step with random torques |tau| < L - or the PD law at random gains, tau computed on the host from S -
  against the oracle with its motors off: engine(S, tau) - oracle_off(S) == dt (fd(S, tau) - fd(S, 0)), fd the oracle's
  CRBA / RNEA forward dynamics, on the joint rates and on the base twist in the body frame of S (1e-12)."""
  from control_cases import air_identity_errors, air_states
  from gym_solo_amd.model import DOF_TO_JOINT
  from oracle import solo_oracle as so
  ca, ma = make_abi('float64')
  ca0, _ = make_abi('float64', motor_torque_limit=0.0)
  rng = np.random.default_rng(21 if mode == 'torque' else 22)
  S = air_states(rng, N)
  L = ca.motor_torque_limit
  eng = _engine(ca, ma)
  if mode == 'torque':
    tau = rng.uniform(-0.99 * L, 0.99 * L, (N, abi.NUM_DOF))
    a = np.zeros((N, abi.NUM_JOINTS))
    a[:, DOF_TO_JOINT] = tau
    eng.set_control('torque')
  else:
    kp, kd = _pd_gains(rng)
    a = rng.uniform(-3, 3, (N, abi.NUM_JOINTS))
    tau = _pd_torque(S, a, kp, kd, L)
    eng.set_control('pd', kp=kp, kd=kd)
  eng.state.copy_(torch.as_tensor(S, device='cuda'))
  eng.snapshot.copy_(eng.state)
  eng.step(torch.as_tensor(a, device='cuda'), abi.STEP_PHYSICS)
  got = eng.state.cpu().numpy()
  ref = S.copy()
  so.OraclePhysics(ca0, ma).step(ref, np.zeros((N, abi.NUM_JOINTS)), threads=16)
  worst_qd, worst_twist = air_identity_errors(S, got, ref, tau, so.OraclePhysics(ca, ma), ca.dt)
  assert worst_qd <= 1e-12 and worst_twist <= 1e-12, (worst_qd, worst_twist)
  assert np.abs(got[:, abi.S_QD:abi.S_QD + 8] - ref[:, abi.S_QD:abi.S_QD + 8]).max() > 1e-3   # (tau did something)
  assert eng.stats.cpu().numpy()[5] == 0
