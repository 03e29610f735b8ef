"""GPU suite of the actuator randomisation (solo_engine_set_actuators: per-robot scales of the torque limit and the PD gains, read by
solo_act_kernel) through the C-ABI on the MI355X.  The cases of tests/test_emu_actuators.py at 64 robots:

  1. NEUTRAL BLOCK: all ones == actuators off, bit for bit (state, targets, obs, reward, done, term_count, term_fired, stats) -
     position / torque / PD, D in {1, 3}, with and without a tilt + time program, single steps and a fused recording rollout with
     auto-reset on; switching off again restores the previous kernel name and the same bits.
  2. POWER-OF-TWO TWIN: s, a_p, a_d in {1/4, 1/2, 1, 2} == a uniform engine with actuators off created with motor_torque_limit x s
     and gains kp x a_p, kd x a_d, bit for bit, under motions that make the limit bind; the groups end more than 1e-6 apart.
  3. ORACLE PARITY at eight limit scales in [0.3, 1.5], position mode, saturating targets, 60 steps on the ground, half the robots
     with their own friction and base mass: 1e-9 in f64, the one-step bars of tests/test_gpu_control.py in f32 (identity (b)'s).
  4. PD AT ARBITRARY SCALES: identity (d) in the air at its bar of 1e-13 (f64).
  5. WHAT THE BLOCK DOES NOT TOUCH: settle(), reset(mask), the auto-reset; a checkpoint round trip continues bit for bit.
  6. The setter's validation and the unsupported combinations, in both orders, on the engine itself."""
import ctypes as C

import numpy as np
import pytest

from gym_solo_amd import abi
from helpers import make_abi
import actuator_cases as ac

pytestmark = pytest.mark.gpu

N, K = 64, 6
TILT, TIME = abi.T_TILT_ABOVE, abi.T_TIME
PLAIN = [(TIME, ac.TIME_LIMIT, 0.0)]
FALLS = [(TILT, 0, ac.TILT_THRESHOLD), (TIME, ac.TIME_LIMIT, 0.0)]
_CACHE = {}


@pytest.fixture(scope='module')
def torch():
  import torch
  if not torch.cuda.is_available():
    pytest.fail('GPU tests need a visible MI355X')
  return torch


def program(terms):
  """the benchmark's observation / reward program with the termination list `terms`"""
  if 'prog' not in _CACHE:
    from gym_solo_amd.envs.solo8v2vanilla import Solo8VanillaConfig, Solo8VanillaEnv
    from gym_solo_amd.workloads import register_benchmark_workload
    cfg = Solo8VanillaConfig()
    cfg.dtype, cfg.num_envs = 'float64', 4
    env = Solo8VanillaEnv(config=cfg)
    register_benchmark_workload(env, max_steps=2)
    env._ensure_program()
    _CACHE['prog'] = abi.SoloProgram.from_buffer_copy(env.engine.program)
    env._close()
  p = abi.SoloProgram.from_buffer_copy(_CACHE['prog'])
  p.num_terms = len(terms)
  for t in range(abi.MAX_TERMS):
    p.term_kind[t], p.term_param[t] = (terms[t][0], terms[t][1]) if t < len(terms) else (0, 0)
  return p


def engine(torch, dtype, mode, D, terms, n=N, gains=None, auto_reset=True, start=None, **cfg):
  """an engine in `mode` with decimation D and the termination list `terms`; start: state records [n, 32] written into the state and
  the snapshot (in the engine's precision)"""
  from gym_solo_amd.engine import Engine
  ca, ma = make_abi(dtype, auto_reset=auto_reset, **cfg)
  eng = Engine(ca, ma, n)
  if mode != 'position':
    kp, kd = gains if gains is not None else ac.pd_gains()
    eng.set_control(mode, kp=ac.joint_gains(kp), kd=ac.joint_gains(kd), action_scale=1.0)
  if D > 1:
    eng.set_decimation(D)
  eng.set_term_values([v for _, _, v in terms])
  eng.set_program(program(terms))
  if start is not None:
    t = torch.as_tensor(np.asarray(start), device='cuda').to(eng.tdtype)
    eng.snapshot.copy_(t)
    eng.state.copy_(t)
  eng.synchronize()
  return eng


def dev(torch, eng, a):
  return torch.as_tensor(np.ascontiguousarray(a), device='cuda').to(eng.tdtype)


def everything(eng):
  eng.synchronize()
  return {name: getattr(eng, name).cpu().numpy().copy() for name in ('state', 'targets', 'obs', 'reward', 'done', 'term_count', 'term_fired', 'stats_shards')}


def _same(a, b, what):
  for name in a:
    np.testing.assert_array_equal(a[name], b[name], err_msg='%s: %s' % (what, name))


def _real(dtype):
  return 'double' if dtype == 'float64' else 'float'


def _name(family, dtype, mode, full=True):
  return 'solo_%s_kernel<%s, %s, %s>' % (family, _real(dtype), 'true' if full else 'false', 'false' if mode == 'position' else 'true')


# ---- 1. the neutral block ----------------------------------------------------------------------------------------------------
NEUTRAL = [(('float64', 'float32')[(m + d + p) % 2], mode, D, terms)
           for m, mode in enumerate(('position', 'torque', 'pd')) for d, D in enumerate((1, 3)) for p, terms in enumerate((PLAIN, FALLS))]
NEUTRAL_IDS = ['%s-%s-D%d-%s' % (dt, m, D, 'tilt+time' if t is FALLS else 'time') for dt, m, D, t in NEUTRAL]


def _neutral_actions(dtype, mode):
  rng = np.random.default_rng(17)
  ca, _ = make_abi(dtype)
  if mode == 'torque':
    return rng.uniform(-4.0, 4.0, (K, N, abi.NUM_JOINTS))
  if mode == 'pd':
    return np.array(list(ca.settle_targets))[None, None, :] + rng.uniform(-1.5, 1.5, (K, N, abi.NUM_JOINTS))
  return rng.uniform(-6, 6, (K, N, abi.NUM_JOINTS))


@pytest.mark.parametrize('dtype,mode,D,terms', NEUTRAL, ids=NEUTRAL_IDS)
def test_neutral_block_equals_actuators_off(torch, dtype, mode, D, terms):
  snap = ac.tilted_snapshot(N, dtype)
  state_terms = terms is FALLS
  runs = {}
  for on in (False, True):
    s = engine(torch, dtype, mode, D, terms, start=snap)
    r = engine(torch, dtype, mode, D, terms, start=snap)
    before = s.kernel_name
    if on:
      s.set_actuators(torch.ones(N, abi.ACTUATOR_WIDTH, device='cuda', dtype=s.tdtype))
      r.set_actuators({'torque_limit': torch.ones(N, device='cuda')})
      assert torch.equal(r.actuators, torch.ones(N, abi.ACTUATOR_WIDTH, device='cuda', dtype=r.tdtype))
    acts = dev(torch, s, _neutral_actions(dtype, mode))
    per_step = []
    for a in acts:
      s.step(a, abi.STEP_ALL)
      per_step.append(everything(s))
    rec = [t.cpu().numpy() for t in r.rollout(acts, abi.STEP_ALL, record=True)]
    runs[on] = (per_step, s.kernel_name, rec, everything(r), before, r, acts)
    s.close()
  off, new = runs[False], runs[True]
  assert new[1] == _name('act', dtype, mode) and new[4] == off[4] == off[1]
  assert off[1] == (_name('term', dtype, mode) if state_terms else _name('decim', dtype, mode) if D > 1 else
                    'solo_ctl_step_kernel<%s, true>' % _real(dtype) if mode != 'position' else 'solo_step_kernel<%s, true, false, false>' % _real(dtype))
  for k in range(K):
    _same(new[0][k], off[0][k], 'control step %d' % k)
  for g, w, name in zip(new[2], off[2], ('obs', 'reward', 'done')):
    np.testing.assert_array_equal(g, w, err_msg='recorded ' + name)
  _same(new[3], off[3], 'after the rollout')
  assert off[2][2].any() and not off[2][2].all()
  if state_terms:
    assert (off[3]['term_fired'] == 1).any() and (np.array([p['term_fired'] for p in off[0]]) == 2).any()
  else:
    assert not off[3]['term_fired'].any()
  # switching off again: the previous kernel name, and from the same start the same bits
  r = new[5]
  r.set_actuators(None)
  assert r.kernel_name == off[1]
  with pytest.raises(ValueError, match='off'):
    r.actuators
  r.reset()
  r.stats_shards.zero_()
  r.done.zero_()
  r.term_fired.zero_()
  r.obs.zero_()
  r.reward.zero_()
  again = [t.cpu().numpy() for t in r.rollout(new[6], abi.STEP_ALL, record=True)]
  for g, w, name in zip(again, off[2], ('obs', 'reward', 'done')):
    np.testing.assert_array_equal(g, w, err_msg='off again: recorded ' + name)
  _same(everything(r), off[3], 'off again')
  runs[False][5].close()
  r.close()


# ---- 2. the power-of-two twin ---------------------------------------------------------------------------------------------------
TWIN = [('float64', 'position', 1), ('float32', 'position', 3), ('float32', 'torque', 1), ('float64', 'torque', 3),
        ('float64', 'pd', 1), ('float32', 'pd', 3)]


@pytest.mark.parametrize('dtype,mode,D', TWIN, ids=['%s-%s-D%d' % c for c in TWIN])
def test_power_of_two_scales_equal_a_uniform_engine_with_the_scaled_values(torch, dtype, mode, D):
  k = 30 if D == 1 else 10
  ca, _ = make_abi(dtype)
  acts_np = ac.binding_actions(np.random.default_rng(23), mode, k, N, ca)
  table = ac.pow2_table(N)
  kp, kd = ac.pd_gains()
  s = engine(torch, dtype, mode, D, PLAIN, auto_reset=False)
  start = (s.state.clone(), s.snapshot.clone(), s.targets.clone())
  s.set_actuators(dev(torch, s, table))
  acts = dev(torch, s, acts_np)
  obs, rew, done = s.rollout(acts, abi.STEP_ALL, record=True)
  assert s.kernel_name == _name('act', dtype, mode)
  assert s.stats.cpu().numpy()[5] == 0
  for g in range(4):
    rows = torch.as_tensor(np.arange(N) % 4 == g, device='cuda')
    sc, ap, ad = table[g, :3]
    t = engine(torch, dtype, mode, D, PLAIN, gains=(kp * ap, kd * ad), auto_reset=False, motor_torque_limit=ca.motor_torque_limit * sc)
    for dst, src in zip((t.state, t.snapshot, t.targets), start):   # (the same start: the twin settled under its own limit)
      dst.copy_(src)
    t_obs, t_rew, t_done = t.rollout(acts, abi.STEP_ALL, record=True)
    assert not t.kernel_name.startswith('solo_act_kernel')
    assert torch.equal(s.state[rows], t.state[rows]), 'group %d: state' % g
    assert torch.equal(s.targets[rows], t.targets[rows]), 'group %d: targets' % g
    assert torch.equal(obs[:, rows], t_obs[:, rows]), 'group %d: obs' % g
    assert torch.equal(rew[:, rows], t_rew[:, rows]), 'group %d: reward' % g
    t.close()
  # the scales did something: from the same start and under the same actions (robot 0's), robots of different groups end more
  # than 1e-6 apart
  s.state.copy_(start[0]); s.targets.copy_(start[2])
  s.rollout(dev(torch, s, np.repeat(acts_np[:, :1], N, axis=1)), abi.STEP_ALL)
  st = s.state.cpu().numpy().astype(np.float64)
  for g in range(1, 4):
    assert np.abs(st[g, :abi.S_RETURN] - st[0, :abi.S_RETURN]).max() > 1e-6, g
  s.close()


# ---- 3. oracle parity at arbitrary scales, position mode ---------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_position_mode_equals_the_oracle_with_the_scaled_limit(torch, dtype):
  from oracle import solo_oracle as so
  ca, ma = make_abi(dtype)
  ca64, _ = make_abi('float64')
  rng = np.random.default_rng(3)
  table = ac.random_table(rng, N)
  params = ac.own_params(rng, N, ca64)
  acts = ac.binding_actions(rng, 'position', 60, N, ca64)
  s = engine(torch, dtype, 'position', 1, PLAIN, auto_reset=False)
  s.set_params(abi.PARAM_FRICTION, dev(torch, s, params[:, 0]))
  s.set_params(abi.PARAM_BASE_MASS_SCALE, dev(torch, s, params[:, 1]))
  s.set_actuators({'torque_limit': dev(torch, s, table[:, abi.ACT_TORQUE_LIMIT])})
  block = s.actuators.cpu().numpy().astype(np.float64)
  par = s.params.cpu().numpy().astype(np.float64)
  scales = sorted(set(block[:, 0]))
  assert len(scales) == 8 and scales[0] >= 0.3 - 1e-6 and scales[-1] <= 1.5 + 1e-6
  groups = [(np.flatnonzero(block[:, 0] == v), so.OraclePhysics(make_abi('float64', motor_torque_limit=ca64.motor_torque_limit * float(v))[0], ma))
            for v in scales]

  def oracle_step(st, a):
    for rows, ph in groups:
      sub = np.ascontiguousarray(st[rows])
      ph.step(sub, np.ascontiguousarray(a[rows]), np.ascontiguousarray(par[rows]))
      st[rows] = sub

  if dtype == 'float64':
    ref = s.state.cpu().numpy().copy()
    for k in range(60):
      s.step(dev(torch, s, acts[k]), abi.STEP_PHYSICS)
      oracle_step(ref, acts[k])
    assert s.kernel_name == _name('act', dtype, 'position')
    got = s.state.cpu().numpy()
    print('f64, 60 steps: max |engine - oracle| = %.3g (bar 1e-9)' % np.abs(got[:, :abi.S_RETURN] - ref[:, :abi.S_RETURN]).max())
    np.testing.assert_allclose(got[:, :abi.S_RETURN], ref[:, :abi.S_RETURN], rtol=0, atol=1e-9)
  else:
    worst = {name: 0.0 for name in ac.F32_ONE_STEP}
    for k in range(60):
      if k % 10 == 0:
        st = s.state.cpu().numpy().astype(np.float64)
        oracle_step(st, acts[k])
      s.step(dev(torch, s, acts[k]), abi.STEP_PHYSICS)
      if k % 10 == 0:
        got = s.state.cpu().numpy().astype(np.float64)
        for name, ((o, w), mx) in ac.F32_ONE_STEP.items():
          err = np.abs(got[:, o:o + w] - st[:, o:o + w]).max()
          worst[name] = max(worst[name], err)
          assert err <= mx, (k, name, err, mx)
    print('f32, one-step errors:', {n: '%.3g' % v for n, v in worst.items()})
  assert s.stats.cpu().numpy()[5] == 0
  s.close()


# ---- 4. PD at arbitrary scales: identity (d) ---------------------------------------------------------------------------------------
def test_pd_step_equals_torque_step_fed_the_scaled_law(torch):
  from control_cases import air_states
  ca, ma = make_abi('float64')
  rng = np.random.default_rng(12)
  S = air_states(rng, N)
  table = ac.random_table(rng, N)
  kp, kd = ac.pd_gains()
  cmd = rng.uniform(-3, 3, (N, abi.NUM_JOINTS))
  pd = engine(torch, 'float64', 'pd', 1, PLAIN, auto_reset=False, start=S)
  pd.set_actuators(dev(torch, pd, table))
  tq = engine(torch, 'float64', 'torque', 1, PLAIN, auto_reset=False, start=S)
  tq.set_actuators({'torque_limit': dev(torch, tq, table[:, abi.ACT_TORQUE_LIMIT])})
  tau = ac.pd_torque(S, cmd, kp, kd, table, ca.motor_torque_limit)
  lim = ca.motor_torque_limit * table[:, abi.ACT_TORQUE_LIMIT, None]
  assert (np.abs(tau) == lim).any() and (np.abs(tau) < lim).any()
  pd.step(dev(torch, pd, cmd), abi.STEP_PHYSICS)
  tq.step(dev(torch, tq, ac.dof_to_joint(tau)), abi.STEP_PHYSICS)
  worst = (pd.state[:, :abi.S_RETURN] - tq.state[:, :abi.S_RETURN]).abs().max().item()
  print('identity (d) under the block: %.3g (bar 1e-13)' % worst)
  assert worst <= 1e-13, worst
  assert (pd.state[:, abi.S_QD:abi.S_QD + 8].cpu().numpy() - S[:, abi.S_QD:abi.S_QD + 8]).__abs__().max() > 1e-3
  # D = 3: the law is re-evaluated under the scaled gains every physics step - one control step equals three single PD steps
  fused = engine(torch, 'float64', 'pd', 3, PLAIN, auto_reset=False, start=S)
  fused.set_actuators(dev(torch, fused, table))
  fused.step(dev(torch, fused, cmd), abi.STEP_PHYSICS)
  for _ in range(2):
    pd.step(dev(torch, pd, cmd), abi.STEP_PHYSICS)
  assert torch.equal(fused.state, pd.state)
  for e in (pd, tq, fused):
    e.close()


# ---- 5. what the block does not touch ---------------------------------------------------------------------------------------------
def test_settle_reset_and_checkpoints_leave_the_block_alone(torch):
  dtype, mode, D = 'float32', 'pd', 3
  table = ac.random_table(np.random.default_rng(9), N)
  a = engine(torch, dtype, mode, D, FALLS)
  snapshot = a.snapshot.clone()
  a.set_actuators(dev(torch, a, table))
  block = a.actuators.clone()
  a.settle()
  assert torch.equal(a.snapshot, snapshot) and torch.equal(a.state, snapshot)   # (the settle loop does not read the block)
  assert torch.equal(a.actuators, block)
  tilted = dev(torch, a, ac.tilted_snapshot(N, dtype))
  a.snapshot.copy_(tilted); a.state.copy_(tilted)
  acts = dev(torch, a, _neutral_actions(dtype, mode))
  a.rollout(acts[:3], abi.STEP_ALL)
  assert a.stats.cpu().numpy()[2] > 0            # (auto-resets happened: the tilted robots fire every control step)
  assert torch.equal(a.actuators, block)
  ck = a.get_state()
  assert 'actuators' not in ck
  a.rollout(acts[3:], abi.STEP_ALL)
  want = everything(a)
  mask = torch.zeros(N, device='cuda', dtype=torch.uint8)
  mask[::2] = 1
  a.reset(mask)
  assert torch.equal(a.actuators, block)
  # the checkpoint into ANOTHER engine with the same block: continues bit for bit
  b = engine(torch, dtype, mode, D, FALLS)
  b.set_actuators(dev(torch, b, table))
  b.set_state(ck)
  b.rollout(acts[3:], abi.STEP_ALL)
  got = everything(b)
  for name in ('state', 'targets', 'obs', 'reward', 'done', 'term_count', 'stats_shards'):
    np.testing.assert_array_equal(got[name], want[name], err_msg=name)
  a.close(); b.close()


# ---- 6. validation and the unsupported combinations, on the engine ---------------------------------------------------------------------
def test_validation_keeps_the_previous_block(torch):
  eng = engine(torch, 'float64', 'position', 1, PLAIN, n=8)
  good = torch.full((8, abi.ACTUATOR_WIDTH), 0.5, device='cuda', dtype=torch.float64)
  for bad_value in (float('nan'), -1.0, float('inf')):
    bad = good.clone()
    bad[3, abi.ACT_KP] = bad_value
    with pytest.raises(ValueError, match='finite and >= 0'):
      eng.set_actuators(bad)
    assert not eng.kernel_name.startswith('solo_act_kernel')   # ("off" stays in force)
    with pytest.raises(ValueError):
      eng.actuators
  eng.set_actuators(good)
  for bad_value in (float('nan'), -1.0, float('inf')):
    bad = torch.ones_like(good)
    bad[7, abi.ACT_TORQUE_LIMIT] = bad_value
    with pytest.raises(ValueError, match='finite and >= 0'):
      eng.set_actuators(bad)
    assert torch.equal(eng.actuators, good) and eng.kernel_name == 'solo_act_kernel<double, true, false>'
  zero = torch.zeros_like(good)     # (0 is legal: dead motors)
  eng.set_actuators(zero)
  eng.set_actuators(eng.actuators)   # (the view itself: validated in place)
  assert torch.equal(eng.actuators, zero)
  with pytest.raises(ValueError):
    eng.set_actuators(torch.ones(8, 3, device='cuda', dtype=torch.float64))
  with pytest.raises(ValueError, match='unknown actuator column'):
    eng.set_actuators({'ki': torch.ones(8, device='cuda')})
  assert eng.plan(20)['migrate_steps'] == 0
  eng.close()


def test_unsupported_combinations_in_both_orders(torch):
  ones = lambda e: torch.ones(e.num_envs, abi.ACTUATOR_WIDTH, device='cuda', dtype=e.tdtype)
  from gym_solo_amd.engine import Engine
  for kw, word in ((dict(migrate_steps=5), 'migrate_steps'), (dict(solver_residual_threshold=1e-7), 'solver_residual_threshold'),
                   (dict(solver_residual_threshold=1e-7, solver_warm_start=0.5), 'solver_')):
    ca, ma = make_abi('float64', **kw)
    eng = Engine(ca, ma, 8)
    with pytest.raises(ValueError, match=word):
      eng.set_actuators(ones(eng))
    eng.set_actuators(None)   # (off is always legal)
    eng.close()
  eng = engine(torch, 'float64', 'position', 1, PLAIN, n=8)
  eng.set_contact_sensing(True)
  with pytest.raises(ValueError, match='contact sensing'):
    eng.set_actuators(ones(eng))
  eng.set_contact_sensing(False)
  eng.set_actuators(ones(eng))
  with pytest.raises(ValueError, match='actuator randomisation'):
    eng.set_contact_sensing(True)
  assert not eng.contact_sensing and eng.kernel_name == 'solo_act_kernel<double, true, false>'
  # a block goes with every control mode, decimation and a state program, whichever is set first
  eng.set_control('pd', kp=1.0, kd=0.1)
  eng.set_decimation(4)
  assert eng.kernel_name == 'solo_act_kernel<double, true, true>'
  eng.set_term_values([ac.TILT_THRESHOLD, 0.0])
  eng.set_program(program(FALLS))
  assert eng.kernel_name == 'solo_act_kernel<double, true, true>'
  eng.set_actuators(None)
  assert eng.kernel_name == 'solo_term_kernel<double, true, true>'
  eng.close()
