"""GPU suite of control decimation (solo_engine_set_decimation: D physics steps per control step in ONE launch of
solo_decim_kernel) through the C-ABI on the MI355X.

THE TWIN every identity is taken against: an engine of the same library with D = 1 - for each control step D - 1 single-step
launches with flags = STEP_PHYSICS, then one single-step launch with STEP_ALL, all with the same action.  That is the code as
it was before decimation existed and nothing else.  The decimated engine must equal it BIT FOR BIT in state, targets,
term_count, stats and every control step's obs / reward / done.

(stats: slots 2 .. 7 - episodes, lengths, diverged - are sums of integers and compared exactly.  Slots 0 and 1, the sums of the
f64 returns and their squares, are accumulated with atomics from four robots per shard in whatever order their waves arrive -
two runs of the TWIN differ in the last bit there - so they are compared to 1e-13 relative, the bar tests/test_gpu_control.py
sets for the same sums; every robot's own return is compared exactly, in the state record.)"""
import numpy as np
import pytest

from gym_solo_amd import abi
from helpers import make_abi

pytestmark = pytest.mark.gpu

N = 256
K, SPL, LIMIT = 27, 10, 7   # launches of 10, 10 and 7 control steps (across the epilogue's pass of 25); TimeBased(7)


@pytest.fixture(scope='module')
def torch():
  import torch
  if not torch.cuda.is_available():
    pytest.fail('GPU tests need a visible MI355X')
  return torch


def _pd_gains(rng):
  return rng.uniform(1.0, 4.0, abi.NUM_JOINTS), rng.uniform(0.01, 0.05, abi.NUM_JOINTS)


def _env(torch, dtype='float64', n=N, mode='position', decimation=1, max_steps=LIMIT, **kw):
  """Solo8VanillaEnv with the benchmark's observation / reward program, TimeBased(max_steps) and auto-reset"""
  from gym_solo_amd.envs.solo8v2vanilla import Solo8VanillaConfig, Solo8VanillaEnv
  from gym_solo_amd.workloads import register_benchmark_workload
  cfg = Solo8VanillaConfig()
  cfg.dtype, cfg.num_envs, cfg.auto_reset = dtype, n, True
  if mode == 'pd':
    cfg.control_mode = 'pd'
    cfg.pd_kp, cfg.pd_kd = _pd_gains(np.random.default_rng(2))
  elif mode == 'torque':
    cfg.control_mode = 'torque'
  for k, v in kw.items():
    setattr(cfg, k, v)
  env = Solo8VanillaEnv(config=cfg, decimation=decimation)
  register_benchmark_workload(env, max_steps=max_steps)
  env._ensure_program()
  return env


def _actions(torch, mode, k, n, dtype, seed=7):
  tdt = torch.float32 if dtype == 'float32' else torch.float64
  g = torch.Generator(device='cuda').manual_seed(seed)
  r = torch.rand(k, n, 12, device='cuda', dtype=tdt, generator=g) * 2 - 1
  if mode == 'torque':
    return r * 2.5   # (some beyond the limit: clamped)
  if mode == 'pd':
    settle = np.array(list(make_abi(dtype)[0].settle_targets))
    return torch.as_tensor(settle, device='cuda', dtype=tdt) + 0.6 * r
  return r * 6.28


def _final(eng):
  eng.synchronize()
  return dict(state=eng.state.cpu().numpy(), targets=eng.targets.cpu().numpy(), term_count=eng.term_count.cpu().numpy(),
              stats=eng.stats.cpu().numpy())


def _run_twin(torch, acts, dtype, n, mode, D):
  env = _env(torch, dtype, n, mode)
  eng = env.engine
  assert eng.decimation == 1 and not eng.kernel_name.startswith('solo_decim_kernel')
  obs, rew, done = [], [], []
  for a in acts:
    a = a.contiguous()
    for _ in range(D - 1):
      eng.step(a, abi.STEP_PHYSICS)
    eng.step(a, abi.STEP_ALL)
    obs.append(eng.obs.clone()); rew.append(eng.reward.clone()); done.append(eng.done.clone())
  out = ([torch.stack(t).cpu().numpy() for t in (obs, rew, done)], _final(eng))
  env._close()
  return out


def _assert_equals_twin(got_rec, got_final, twin):
  want_rec, want_final = twin
  for name in ('state', 'targets', 'term_count'):
    np.testing.assert_array_equal(got_final[name], want_final[name], err_msg=name)
  np.testing.assert_array_equal(got_final['stats'][2:], want_final['stats'][2:], err_msg='stats[2:]')
  np.testing.assert_allclose(got_final['stats'][:2], want_final['stats'][:2], rtol=1e-13, atol=0, err_msg='stats[:2]')   # (module docstring)
  for got, want, name in zip(got_rec, want_rec, ('obs', 'reward', 'done')):
    np.testing.assert_array_equal(got, want, err_msg=name)


def _closed_loop(torch, env, acts):
  eng = env.engine
  obs, rew, done = [], [], []
  for a in acts:
    eng.step(a.contiguous(), abi.STEP_ALL)
    obs.append(eng.obs.clone()); rew.append(eng.reward.clone()); done.append(eng.done.clone())
  return [torch.stack(t).cpu().numpy() for t in (obs, rew, done)]


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('D', [2, 5])
@pytest.mark.parametrize('mode', ['position', 'torque', 'pd'])
def test_decimated_rollout_and_closed_loop_equal_the_twin(torch, mode, D, dtype):
  """27 control steps recorded with steps_per_launch = 10 (launches of 10, 10 and 7 on two slices), and the same 27 as
  closed-loop step() calls - each ONE launch -, against the twin's 27 x D single-step launches; TimeBased(7) with auto-reset"""
  acts = _actions(torch, mode, K, N, dtype)
  twin = _run_twin(torch, acts, dtype, N, mode, D)
  real = 'double' if dtype == 'float64' else 'float'
  fused = _env(torch, dtype, N, mode, decimation=D, steps_per_launch=SPL)
  assert fused.engine.decimation == D
  assert fused.engine.kernel_name == 'solo_decim_kernel<%s, true, %s>' % (real, 'false' if mode == 'position' else 'true')
  p = fused.engine.plan(K)
  assert (p['steps_per_launch'], p['launches'], p['migrate_steps']) == (SPL, 3, 0), p
  rec = [t.cpu().numpy() for t in fused.engine.rollout(acts, abi.STEP_ALL, record=True)]
  _assert_equals_twin(rec, _final(fused.engine), twin)
  fused._close()
  loop = _env(torch, dtype, N, mode, decimation=D)
  rec = _closed_loop(torch, loop, acts)
  _assert_equals_twin(rec, _final(loop.engine), twin)
  loop._close()
  done = twin[0][2]
  assert done.sum() == (K // (LIMIT + 1)) * N and done[LIMIT].all()   # (control steps, not physics steps, are counted)
  assert twin[1]['stats'][5] == 0


def test_twin_identity_at_4096_robots(torch):
  """every wave slot of the device taken: D = 4, 5 control steps, f64, one fused launch and the closed loop"""
  n, D, k = 4096, 4, 5
  acts = _actions(torch, 'position', k, n, 'float64', seed=9)
  twin = _run_twin(torch, acts, 'float64', n, 'position', D)
  fused = _env(torch, 'float64', n, decimation=D)
  assert fused.engine.plan(k)['launches'] == 1
  rec = [t.cpu().numpy() for t in fused.engine.rollout(acts, abi.STEP_ALL, record=True)]
  _assert_equals_twin(rec, _final(fused.engine), twin)
  fused._close()
  loop = _env(torch, 'float64', n, decimation=D)
  rec = _closed_loop(torch, loop, acts)
  _assert_equals_twin(rec, _final(loop.engine), twin)
  loop._close()


def test_oracle_parity_of_a_fused_decimated_launch(torch):
  """D = 4 over 15 control steps of U(-2 pi, 2 pi) targets as ONE fused launch; the oracle steps 4 times per action.  Every robot
  within 1e-9: the project's bar for 60 chaotic physics steps"""
  from gym_solo_amd.engine import Engine
  from oracle import solo_oracle as so
  ca, ma = make_abi('float64')
  eng = Engine(ca, ma, N)
  eng.set_decimation(4)
  assert eng.plan(15)['launches'] == 1
  st = eng.state.cpu().numpy().copy()
  rng = np.random.default_rng(21)
  acts = rng.uniform(-2 * np.pi, 2 * np.pi, (15, N, abi.NUM_JOINTS))
  eng.rollout(torch.as_tensor(acts, device='cuda'), abi.STEP_PHYSICS)
  ph = so.OraclePhysics(ca, ma)
  for a in acts:
    for _ in range(4):
      ph.step(st, a, threads=16)
  got = _final(eng)
  worst = np.abs(got['state'][:, :abi.S_RETURN] - st[:, :abi.S_RETURN]).max(axis=1)
  print('decimated launch vs oracle, worst robot: %.3e' % worst.max())
  assert worst.max() <= 1e-9, worst.max()
  assert got['stats'][5] == 0
  assert np.abs(got['state'][:, :abi.S_RETURN] - eng.snapshot.cpu().numpy()[:, :abi.S_RETURN]).max() > 1e-2   # (it moved)
  eng.close()


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_counting_is_in_control_steps(torch, dtype):
  """TimeBased(7), D = 4: after 7 control steps (28 physics steps) the episode length reads 7 and the episodic return equals the
  host's sum of the 7 recorded rewards bit for bit; the termination fires when its counter exceeds 7, as in the reference
  (termination.py:72-83) - every robot's first done is at control step 7, counted from 0, and closes an episode of 8 control
  steps"""
  env = _env(torch, dtype, N, decimation=4)
  eng = env.engine
  acts = _actions(torch, 'position', 9, N, dtype, seed=5)
  obs, rew, done = eng.rollout(acts[:7], abi.STEP_ALL, record=True)
  eng.synchronize()
  assert not bool(done.any())
  st = eng.state.cpu().numpy()
  np.testing.assert_array_equal(st[:, abi.S_EPLEN], 7)
  np.testing.assert_array_equal(eng.term_count.cpu().numpy()[:, 0], 7)
  r = rew.cpu().numpy()
  host = np.zeros(N, dtype=r.dtype)
  for k in range(7):
    host = host + r[k]
  np.testing.assert_array_equal(st[:, abi.S_RETURN], host)
  _, rew2, done2 = eng.rollout(acts[7:], abi.STEP_ALL, record=True)
  eng.synchronize()
  d = done2.cpu().numpy()
  assert d[0].all() and not d[1].any()
  stats = eng.stats.cpu().numpy()
  assert stats[2] == N and stats[3] == 8 * N
  np.testing.assert_allclose(stats[0], (host + rew2.cpu().numpy()[0]).astype(np.float64).sum(), rtol=1e-13)
  np.testing.assert_array_equal(eng.state.cpu().numpy()[:, abi.S_EPLEN], 1)
  env._close()


@pytest.mark.parametrize('mode', ['position', 'pd'])
def test_nan_action_restores_once_and_leaves_the_others_alone(torch, mode):
  """a NaN action of robot 5 in control step 3 (D = 3): its first substep diverges and ends the control step - restored from
  the snapshot once, counted once, restarted under auto-reset - and every other robot is bit for bit what it is without it"""
  acts = _actions(torch, mode, 6, N, 'float64', seed=4)
  bad = acts.clone()
  bad[3, 5, 0] = float('nan')
  others = np.arange(N) != 5
  runs = []
  for a in (acts, bad):
    env = _env(torch, 'float64', N, mode, decimation=3)
    rec = [t.cpu().numpy() for t in env.engine.rollout(a, abi.STEP_ALL, record=True)]
    runs.append((rec, _final(env.engine)))
    env._close()
  (clean_rec, clean), (rec, got) = runs
  assert clean['stats'][5] == 0 and got['stats'][5] == 1
  for g, w in zip(rec, clean_rec):
    np.testing.assert_array_equal(g[:, others], w[:, others])
  for name in ('state', 'term_count', 'targets'):
    np.testing.assert_array_equal(got[name][others], clean[name][others], err_msg=name)
  assert np.isfinite(got['state']).all() and not rec[2][3, 5]
  # the closed loop: after the control step the robot IS its snapshot
  env = _env(torch, 'float64', N, mode, decimation=3)
  for k in range(4):
    env.engine.step(bad[k].contiguous(), abi.STEP_ALL)
  f = _final(env.engine)
  assert f['stats'][5] == 1
  np.testing.assert_array_equal(f['state'][5, :abi.S_RETURN], env.engine.snapshot.cpu().numpy()[5, :abi.S_RETURN])
  assert f['term_count'][5, 0] == 0 and (f['term_count'][others, 0] == 4).all()
  env._close()


def test_rejections_raise_value_error_in_both_orders(torch):
  from gym_solo_amd.engine import Engine
  for kw in (dict(migrate_steps=5), dict(solver_residual_threshold=1e-7), dict(solver_residual_threshold=1e-7, solver_warm_start=0.85)):
    ca, ma = make_abi('float64', **kw)
    eng = Engine(ca, ma, 64)
    with pytest.raises(ValueError, match='decimation'):
      eng.set_decimation(2)
    eng.set_decimation(1)   # (D = 1 is always accepted)
    assert eng.decimation == 1
    eng.close()
  ca, ma = make_abi('float64')
  eng = Engine(ca, ma, 64)
  for d in (0, -1, 65):
    with pytest.raises(ValueError):
      eng.set_decimation(d)
  eng.set_contact_sensing(True)
  with pytest.raises(ValueError, match='contact sensing'):
    eng.set_decimation(2)
  assert eng.decimation == 1
  eng.set_contact_sensing(False)
  eng.set_decimation(2)
  with pytest.raises(ValueError, match='decimation'):
    eng.set_contact_sensing(True)
  assert eng.decimation == 2 and not eng.contact_sensing
  # robot migration left to the engine resolves to none; 8192 robots in f64 migrate with D = 1
  eng.close()
  big = Engine(ca, ma, 8192)
  assert big.plan(20)['migrate_steps'] > 0
  big.set_decimation(2)
  p = big.plan(20)
  assert p['migrate_steps'] == 0 and p['steps_per_launch'] == 20
  assert big.plan(1000)['steps_per_launch'] == 125
  big.close()


def test_checkpoint_resumes_bit_for_bit_mid_rollout(torch):
  env = _env(torch, 'float64', N, 'pd', decimation=4, steps_per_launch=5)
  eng = env.engine
  acts = _actions(torch, 'pd', 24, N, 'float64', seed=6)
  eng.rollout(acts[:11], abi.STEP_ALL)
  ck = eng.get_state()
  assert 'decimation' not in ck   # (configuration, not state)
  first = [t.clone() for t in eng.rollout(acts[11:], abi.STEP_ALL, record=True)] + [eng.state.clone(), eng.term_count.clone()]
  eng.set_state(ck)
  again = list(eng.rollout(acts[11:], abi.STEP_ALL, record=True)) + [eng.state, eng.term_count]
  eng.synchronize()
  for x, y in zip(first, again):
    assert torch.equal(x, y)
  assert bool(first[2].any())
  env._close()


def test_env_step_is_the_engine_path(torch):
  """Solo8VanillaEnv(decimation=4).step() == Engine.set_decimation(4) + Engine.step, and control_dt = 4 dt"""
  a = _env(torch, 'float32', N, decimation=4)
  b = _env(torch, 'float32', N)
  assert a.decimation == 4 and a.control_dt == pytest.approx(4 * a.config.dt) and b.control_dt == pytest.approx(b.config.dt)
  b.engine.set_decimation(4)
  assert a.engine.kernel_name == b.engine.kernel_name == 'solo_decim_kernel<float, true, false>'
  acts = _actions(torch, 'position', 10, N, 'float32', seed=8)
  ended = []
  for k in range(10):
    obs, rew, done, _ = a.step(acts[k])
    b.engine.step(acts[k].contiguous(), abi.STEP_ALL)
    assert torch.equal(obs, b.engine.obs) and torch.equal(rew, b.engine.reward) and torch.equal(done, b.engine.done.bool())
    ended.append(bool(done.all()))
  assert torch.equal(a.engine.state, b.engine.state) and ended == [k == LIMIT for k in range(10)]
  with pytest.raises(ValueError):
    a.client.setPhysicsEngineParameter(numSubSteps=4)
  a._close(); b._close()


def test_a_graph_recaptured_after_set_decimation_replays_the_new_kernel(torch):
  eager = _env(torch, 'float64', N, decimation=4)
  cap = _env(torch, 'float64', N)
  eng = cap.engine
  static = torch.zeros(N, 12, device='cuda', dtype=torch.float64)
  eng.step(static, abi.STEP_ALL)   # (warm-up, then back to the snapshot)
  eng.reset()
  torch.cuda.synchronize()
  old = torch.cuda.CUDAGraph()
  with torch.cuda.graph(old):
    eng.step(static, abi.STEP_ALL)
  eng.set_decimation(4)
  new = torch.cuda.CUDAGraph()
  with torch.cuda.graph(new):
    eng.step(static, abi.STEP_ALL)
  acts = _actions(torch, 'position', 4, N, 'float64', seed=3)
  for k in range(3):
    eager.engine.step(acts[k].contiguous(), abi.STEP_ALL)
    static.copy_(acts[k])
    new.replay()
    torch.cuda.synchronize()
    assert torch.equal(eager.engine.state, eng.state) and torch.equal(eager.engine.obs, eng.obs), k
  # the graph captured BEFORE the call still launches the one-step kernel: one replay advances one physics step
  one = _env(torch, 'float64', N)
  one.engine.set_state(eng.get_state())
  static.copy_(acts[3])
  old.replay()
  one.engine.step(acts[3].contiguous(), abi.STEP_ALL)
  torch.cuda.synchronize()
  assert torch.equal(one.engine.state, eng.state)
  for e in (eager, cap, one):
    e._close()
