"""GPU suite of the state terminations (HeightTermination / TiltTermination: SOLO_T_HEIGHT_BELOW / SOLO_T_TILT_ABOVE evaluated
inside solo_term_kernel) through the C-ABI on the MI355X.

Every identity is taken against THE TWIN of tests/terms_cases.py: an engine of the same library whose program holds no state
termination (one PerpetualTermination) with auto-reset off - the step / control kernels with D = 1, the decimation kernels with
D > 1, as they are without this feature -, one control step per launch, the criterion applied to the twin's own state in numpy in
the engine's precision, the grace / TimeBased counters kept on the host and reset(mask) for the robots that fired.  The engine
under test runs the same actions with auto-reset on - closed loop, as fused recorded rollouts of 16 + 16 + 8 control steps and as
one launch of 40 (two passes of the output epilogue: 25 + 15 in f64, 32 + 8 in f32) - and must equal the twin BIT FOR BIT in
state, targets, term_count, term_fired, every control step's obs / reward / done and the episode / length statistics (the return
sums: 1e-12 relative, the twin's are host-side additions in another order).

Thresholds come from a free run of the twin (terms_cases.gap_thresholds_among), never from a constant: tilt - near the median
over the robots of their largest tilt over the horizon; height, with after_steps = 20 - near the median z at control step 20; in
the widest gap that ALL the evaluated values leave there.  The tests assert on the twin alone that no evaluated value - the grace
period's included - lies within 1e-9 (f64) / 1e-5 (f32) of the threshold, that at least a quarter of the robots fire and at
least a quarter never do.

THE ROBOTS START SPREAD OUT (_spread): the default snapshot has all of them on their bellies, where cos(tilt) moves by a few 1e-6
per control step inside a range of ~2e-4 and the heights lie within micrometres of each other - no threshold near a median keeps
8000 such values 1e-5 away in f32, and a robot cannot step over a band of 2e-5.  So three robots of four start lifted by 0.15 to
0.75 m, rolled by 0.2 to 1.2 rad, rolling at up to 3 rad/s and sinking at 0.3 m/s - in the snapshot too, so a restart puts them
back there: cos(tilt) then moves by ~1e-3 and the height by ~3e-4 m per physics step, and the values spread over 0.5 / 0.6 m.  With
D = 4 the lower ones land within the horizon; every fourth robot stays on its belly and flails in contact from the first step."""
import numpy as np
import pytest

from gym_solo_amd import abi
from gym_solo_amd.core import termination as terms
from helpers import incline_terrain, make_abi
import terms_cases as tc

pytestmark = pytest.mark.gpu

N, K, SPL, GRACE, LIMIT = 200, 40, 16, 20, 39
MARGIN = tc.MARGIN   # 1e-9 (f64) / 1e-5 (f32): what every evaluated value keeps from the threshold
HEIGHT, TILT = abi.T_HEIGHT_BELOW, abi.T_TILT_ABOVE


@pytest.fixture(scope='module')
def torch():
  import torch
  if not torch.cuda.is_available():
    pytest.fail('GPU tests need a visible MI355X')
  return torch


def _env(torch, dtype, n, mode, D, members, auto_reset, **kw):
  """Solo8VanillaEnv with the benchmark's observation / reward program and the termination list members(env)"""
  from gym_solo_amd.envs.solo8v2vanilla import Solo8VanillaConfig, Solo8VanillaEnv
  from gym_solo_amd.workloads import register_benchmark_workload
  cfg = Solo8VanillaConfig()
  cfg.dtype, cfg.num_envs, cfg.auto_reset = dtype, n, auto_reset
  if mode == 'pd':
    cfg.control_mode = 'pd'
    rng = np.random.default_rng(2)
    cfg.pd_kp, cfg.pd_kd = rng.uniform(1.0, 4.0, abi.NUM_JOINTS), rng.uniform(0.01, 0.05, abi.NUM_JOINTS)
  elif mode == 'torque':
    cfg.control_mode = 'torque'
  for k, v in kw.items():
    setattr(cfg, k, v)
  env = Solo8VanillaEnv(config=cfg, decimation=D)
  _spread(torch, env)
  register_benchmark_workload(env, max_steps=LIMIT)
  env.termination_factory._terminations = list(members(env))
  for t in env.termination_factory._terminations:
    if isinstance(t, terms.StateTermination):
      t.client = env.client
  env._mark_dirty()
  env._ensure_program()
  return env


def _spread(torch, env):
  """three robots of four lifted, rolled, rolling and sinking (module docstring), the same for every engine of a size: written into
  the snapshot and the state in the engine's precision"""
  eng = env.engine
  n = eng.num_envs
  rng = np.random.default_rng(11)
  lift, roll, rate = rng.uniform(0.15, 0.75, n), rng.uniform(0.2, 1.2, n) * rng.choice([-1.0, 1.0], n), rng.uniform(-3.0, 3.0, n)
  snap = eng.snapshot.cpu().numpy().astype(np.float64)
  up = np.arange(n) % 4 != 0
  snap[up, abi.S_POS + 2] += lift[up]
  snap[up, abi.S_QUAT:abi.S_QUAT + 4] = np.stack([np.sin(roll / 2), 0 * roll, 0 * roll, np.cos(roll / 2)], axis=1)[up]
  snap[up, abi.S_ANGVEL] = rate[up]
  snap[up, abi.S_LINVEL + 2] = -0.3
  t = torch.as_tensor(snap, device=eng.snapshot.device).to(eng.tdtype)
  eng.snapshot.copy_(t)
  eng.state.copy_(t)
  eng.synchronize()


def _actions(torch, mode, k, n, dtype, seed=7):
  """random +-6 rad targets (position and PD), or the mode's own distribution (torque)"""
  tdt = torch.float32 if dtype == 'float32' else torch.float64
  g = torch.Generator(device='cuda').manual_seed(seed)
  r = torch.rand(k, n, 12, device='cuda', dtype=tdt, generator=g) * 2 - 1
  if mode == 'torque':
    return r * 2.5   # (some beyond the limit: clamped)
  return r * 6.0


class Twin:
  """terms_cases.run_twin's view of an engine whose program never fires"""

  def __init__(self, torch, dtype, n, mode, D, **kw):
    self.torch = torch
    self.env = _env(torch, dtype, n, mode, D, lambda e: [terms.PerpetualTermination()], False, **kw)
    self.eng = self.env.engine
    assert not self.eng.kernel_name.startswith('solo_term_kernel')

  def step(self, a):
    self.eng.step(a.contiguous(), abi.STEP_ALL)

  def reset(self, mask):
    self.eng.reset(self.torch.as_tensor(mask, device='cuda'))

  def state(self):
    return self.eng.state.cpu().numpy()

  def targets(self):
    return self.eng.targets.cpu().numpy()

  def obs(self):
    return self.eng.obs.cpu().numpy()

  def reward(self):
    return self.eng.reward.cpu().numpy()

  def close(self):
    self.env._close()


def _layout(kind, grace):
  """the termination list of a case, None where the state termination sits: tilt in front of a TimeBased(39), height behind it"""
  return [None, (abi.T_TIME, LIMIT, 0.0)] if kind == TILT else [(abi.T_TIME, LIMIT, 0.0), None]


def _threshold_values(kind, free):
  """(one value per robot - what the median is taken of -, every evaluated value [K, N]) of the free run"""
  values = np.array([tc.criterion(kind, s['before_reset'], 'float64') for s in free])   # (exact: the records hold the engine's reals)
  return (values.min(axis=0) if kind == TILT else values[min(GRACE, len(values) - 1)]), values


_FREE = {}


def _twin_case(torch, dtype, n, mode, D, kind, k=K, grace=None, layout=None, values_of=None, **kw):
  """the threshold from the free run, then the twin's control steps: (terms, steps, host)"""
  grace = (GRACE if kind == HEIGHT else 0) if grace is None else grace
  layout = _layout(kind, grace) if layout is None else layout
  acts = _actions(torch, mode, k, n, dtype)
  key = (dtype, n, mode, D, k, tuple(sorted(kw)))
  if key not in _FREE:
    twin = Twin(torch, dtype, n, mode, D, **kw)
    _FREE[key] = tc.run_twin(twin, [], acts, dtype, reset_where=False)[0]
    twin.close()
  per_robot, evaluated = (values_of or _threshold_values)(kind, _FREE[key])
  # the gaps that all the evaluated values leave near the median, widest first: the first one that meets the conditions on the inputs
  # (_assert_inputs) - the robots that are restarted add values the free run does not have
  first = None
  for thr in tc.gap_thresholds_among(per_robot, evaluated, 0.5)[:16]:
    case = [(kind, grace, thr) if t is None else t for t in layout]
    twin = Twin(torch, dtype, n, mode, D, **kw)
    steps, host = tc.run_twin(twin, case, acts, dtype)
    twin.close()
    first = first or (case, steps, host, acts)
    if _inputs_ok(case, steps, host, dtype, n):
      return case, steps, host, acts
  return first


def _fired_by_state(case, steps):
  fired = np.array([s['term_fired'] for s in steps])
  return fired, (fired == 1 + [c[0] in abi.STATE_TERM_KINDS for c in case].index(True)).any(0)


def _inputs_ok(case, steps, host, dtype, n):
  by_state = _fired_by_state(case, steps)[1]
  return host.margin >= MARGIN[dtype] and by_state.sum() * 4 >= n and (~by_state).sum() * 4 >= n


def _members(case):
  def members(env):
    out = []
    for kind, param, value in case:
      if kind == HEIGHT:
        out.append(terms.HeightTermination(env.robot, value, after_steps=param))
      elif kind == TILT:
        t = terms.TiltTermination(env.robot, 1.0, after_steps=param)
        t.value = value       # (the threshold itself - cos(max_tilt) - is what the twin gives)
        out.append(t)
      else:
        out.append(terms.TimeBasedTermination(param))
    return out
  return members


def _assert_inputs(case, steps, host, dtype, n):
  fired, by_state = _fired_by_state(case, steps)
  print('smallest |value - threshold| over all evaluations (%s): %.3e; robots that fire by state: %d of %d' % (dtype, host.margin, by_state.sum(), n))
  assert host.margin >= MARGIN[dtype]
  assert by_state.sum() * 4 >= n and (~by_state).sum() * 4 >= n
  return fired


def _final(eng):
  eng.synchronize()
  return dict(state=eng.state.cpu().numpy(), targets=eng.targets.cpu().numpy(), term_count=eng.term_count.cpu().numpy())


def _assert_final(eng, want):
  got = _final(eng)
  for name in ('state', 'targets', 'term_count'):
    np.testing.assert_array_equal(got[name], want[name], err_msg=name)
  np.testing.assert_array_equal(eng.term_fired.cpu().numpy(), want['term_fired'], err_msg='term_fired')
  tc.assert_stats(eng.stats.cpu().numpy(), want['stats'])


def _assert_rollout(torch, env, acts, steps):
  obs, rew, done = [t.cpu().numpy() for t in env.engine.rollout(acts, abi.STEP_ALL, record=True)]
  for k, want in enumerate(steps):
    for got, name in ((obs[k], 'obs'), (rew[k], 'reward'), (done[k], 'done')):
      np.testing.assert_array_equal(got, want[name], err_msg='%s of control step %d' % (name, k))
  _assert_final(env.engine, steps[-1])
  for name in ('obs', 'reward', 'done'):    # (the view: the last control step)
    np.testing.assert_array_equal(getattr(env.engine, name).cpu().numpy(), steps[-1][name], err_msg=name)


def _assert_closed_loop(torch, env, acts, steps):
  eng = env.engine
  obs, rew, done, fired, count = [], [], [], [], []
  for a in acts:
    eng.step(a.contiguous(), abi.STEP_ALL)
    obs.append(eng.obs.clone()); rew.append(eng.reward.clone()); done.append(eng.done.clone())
    fired.append(eng.term_fired.clone()); count.append(eng.term_count.clone())
  got = [torch.stack(t).cpu().numpy() for t in (obs, rew, done, fired, count)]
  for k, want in enumerate(steps):
    for g, name in zip(got, ('obs', 'reward', 'done', 'term_fired', 'term_count')):
      np.testing.assert_array_equal(g[k], want[name], err_msg='%s of control step %d' % (name, k))
  _assert_final(eng, steps[-1])


def _name(dtype, mode):
  return 'solo_term_kernel<%s, true, %s>' % ('double' if dtype == 'float64' else 'float', 'false' if mode == 'position' else 'true')


@pytest.mark.parametrize('kind', [TILT, HEIGHT], ids=['tilt', 'height'])
@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('D', [1, 4])
@pytest.mark.parametrize('mode', ['position', 'torque', 'pd'])
def test_rollouts_and_closed_loop_equal_the_twin(torch, mode, D, dtype, kind):
  """200 robots (not a multiple of the XCD count), 40 control steps from the default snapshot: launches of 16 + 16 + 8 (episodes end
  inside a launch and - TimeBased(39) for the robots that never fell - on the last launch's last step), one launch of 40 (both sides
  of the epilogue's pass boundary) and 40 closed-loop steps"""
  case, steps, host, acts = _twin_case(torch, dtype, N, mode, D, kind)
  fired = _assert_inputs(case, steps, host, dtype, N)
  assert (fired[LIMIT] == 1 + [c[0] for c in case].index(abi.T_TIME)).any()            # (a launch's last step)
  assert fired[1:SPL - 1].any() or fired[SPL + 1:2 * SPL - 1].any()                    # (inside a launch)
  for spl in (SPL, -1):
    env = _env(torch, dtype, N, mode, D, _members(case), True, steps_per_launch=spl)
    assert env.engine.kernel_name == _name(dtype, mode)
    p = env.engine.plan(K)
    assert (p['steps_per_launch'], p['launches'], p['migrate_steps']) == ((SPL, 3, 0) if spl == SPL else (K, 1, 0)), p
    _assert_rollout(torch, env, acts, steps)
    env._close()
  env = _env(torch, dtype, N, mode, D, _members(case), True)
  _assert_closed_loop(torch, env, acts, steps)
  env._close()


def test_height_is_world_z_over_a_heightfield(torch):
  """on a 10 degree incline the criterion is still the base's world z"""
  kw = dict(terrain=incline_terrain())
  case, steps, host, acts = _twin_case(torch, 'float64', N, 'position', 1, HEIGHT, **kw)
  _assert_inputs(case, steps, host, 'float64', N)
  env = _env(torch, 'float64', N, 'position', 1, _members(case), True, steps_per_launch=SPL, **kw)
  _assert_rollout(torch, env, acts, steps)
  env._close()


def test_8192_robots_never_migrate(torch):
  """more robots than wave slots, f64: without a state termination plan(20) cuts the launch into two chunks of migrating robots;
  with one it reports none, and 8 control steps as one fused launch equal the twin (height without a grace period: the median of
  the robots' lowest z)"""
  n, k = 8192, 8
  def lowest(kind, free):
    values = np.array([tc.criterion(kind, s['before_reset'], 'float64') for s in free])
    return values.min(axis=0), values
  case, steps, host, acts = _twin_case(torch, 'float64', n, 'position', 1, HEIGHT, k=k, grace=0, layout=[None], values_of=lowest)
  _assert_inputs(case, steps, host, 'float64', n)
  plain = Twin(torch, 'float64', n, 'position', 1)
  assert plain.eng.plan(20)['migrate_steps'] > 0
  plain.close()
  env = _env(torch, 'float64', n, 'position', 1, _members(case), True)
  assert env.engine.plan(20)['migrate_steps'] == 0 and env.engine.plan(k)['launches'] == 1
  _assert_rollout(torch, env, acts, steps)
  env._close()


def _program(torch, members):
  env = _env(torch, 'float64', 8, 'position', 1, members, True)
  prog = abi.SoloProgram.from_buffer_copy(env.engine.program)
  env._close()
  return prog


def test_rejections_raise_value_error_in_both_orders(torch):
  from gym_solo_amd.engine import Engine
  state_prog = _program(torch, lambda e: [terms.TiltTermination(e.robot, 1.0), terms.TimeBasedTermination(5)])
  time_prog = _program(torch, lambda e: [terms.TimeBasedTermination(5)])
  # (solver_warm_start > 0 cannot be configured without solver_residual_threshold > 0 - engine creation rejects it -, and set_program
  # tests the threshold first: the warm-start rejection of its own is unreachable through the ABI and stays as a guard)
  for kw, word in ((dict(migrate_steps=5), 'migration'), (dict(solver_residual_threshold=1e-7), 'residual'),
                   (dict(solver_residual_threshold=1e-7, solver_warm_start=0.85), 'residual|warm')):
    ca, ma = make_abi('float64', **kw)
    eng = Engine(ca, ma, 64)
    eng.set_term_values([0.5, 0.0])        # (the thresholds alone are always accepted)
    with pytest.raises(ValueError, match=word):
      eng.set_program(state_prog)
    eng.set_program(time_prog)             # (a program without a state kind runs as before)
    assert not eng.kernel_name.startswith('solo_term_kernel')
    eng.step(None, abi.STEP_ALL)
    eng.close()
  ca, ma = make_abi('float64')
  eng = Engine(ca, ma, 64)
  with pytest.raises(ValueError):
    eng.set_term_values([float('nan')])
  with pytest.raises(ValueError):
    eng.set_term_values([0.0] * 5)
  bad = abi.SoloProgram.from_buffer_copy(state_prog)
  bad.term_param[0] = -1
  with pytest.raises(ValueError, match='grace'):
    eng.set_program(bad)
  # contact sensing first, then the program ...
  eng.set_contact_sensing(True)
  with pytest.raises(ValueError, match='contact sensing'):
    eng.set_program(state_prog)
  eng.set_program(time_prog)
  eng.set_contact_sensing(False)
  # ... and the program first, then contact sensing
  eng.set_program(state_prog)
  assert eng.kernel_name == 'solo_term_kernel<double, true, false>'
  with pytest.raises(ValueError, match='state terminations'):
    eng.set_contact_sensing(True)
  assert not eng.contact_sensing
  # control modes and decimation go with it
  eng.set_decimation(4)
  eng.set_control('torque')
  assert eng.kernel_name == 'solo_term_kernel<double, true, true>'
  eng.step(None, abi.STEP_ALL)
  eng.synchronize()
  # back to a time-only program: the kernels of before, and contact sensing with D > 1 still raises
  eng.set_program(time_prog)
  assert eng.kernel_name == 'solo_decim_kernel<double, true, true>'
  with pytest.raises(ValueError, match='decimation'):
    eng.set_contact_sensing(True)
  eng.set_decimation(1)
  eng.set_control('position')
  assert eng.kernel_name == 'solo_step_kernel<double, true, false, false>'
  eng.close()


def test_checkpoint_resumes_bit_for_bit_mid_rollout(torch):
  case, steps, host, acts = _twin_case(torch, 'float64', N, 'pd', 4, TILT)
  env = _env(torch, 'float64', N, 'pd', 4, _members(case), True, steps_per_launch=5)
  eng = env.engine
  eng.rollout(acts[:11], abi.STEP_ALL)
  ck = eng.get_state()
  assert 'term_values' not in ck and 'term_fired' not in ck   # (thresholds are configuration; the counters are in it)
  first = [t.clone() for t in eng.rollout(acts[11:], abi.STEP_ALL, record=True)] + [eng.state.clone(), eng.term_count.clone(), eng.term_fired.clone()]
  eng.set_state(ck)
  again = list(eng.rollout(acts[11:], abi.STEP_ALL, record=True)) + [eng.state, eng.term_count, eng.term_fired]
  eng.synchronize()
  for x, y in zip(first, again):
    assert torch.equal(x, y)
  assert bool(first[2].any())
  _assert_final(eng, steps[-1])
  env._close()


def test_set_program_back_to_time_only_launches_the_old_kernels(torch):
  """... with the old results: after the switch the engine equals one that never saw a state termination"""
  case, steps, host, acts = _twin_case(torch, 'float32', N, 'position', 1, TILT)
  env = _env(torch, 'float32', N, 'position', 1, _members(case), True)
  plain = _env(torch, 'float32', N, 'position', 1, lambda e: [terms.TimeBasedTermination(3)], True)
  assert env.engine.kernel_name == 'solo_term_kernel<float, true, false>'
  env.termination_factory._terminations = [terms.TimeBasedTermination(3)]
  env._mark_dirty()
  env._ensure_program()
  assert env.engine.kernel_name == plain.engine.kernel_name == 'solo_step_kernel<float, true, false, false>'
  for a in acts[:6]:
    o, r, d, _ = env.step(a)
    po, pr, pd, _ = plain.step(a)
    assert torch.equal(o, po) and torch.equal(r, pr) and torch.equal(d, pd)
  assert torch.equal(env.engine.state, plain.engine.state) and torch.equal(env.engine.term_count, plain.engine.term_count)
  env._close(); plain._close()


def test_a_captured_closed_loop_step_replays_as_eager(torch):
  case, steps, host, acts = _twin_case(torch, 'float64', N, 'position', 4, TILT)
  cap = _env(torch, 'float64', N, 'position', 4, _members(case), True)
  eng = cap.engine
  static = torch.zeros(N, 12, device='cuda', dtype=torch.float64)
  eng.step(static, abi.STEP_ALL)   # (warm-up, then back to the snapshot)
  eng.reset()
  eng.stats_shards.zero_()
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    eng.step(static, abi.STEP_ALL)
  eng.reset()
  eng.stats_shards.zero_()
  for k, want in enumerate(steps):
    static.copy_(acts[k])
    graph.replay()
    torch.cuda.synchronize()
    for name in ('obs', 'reward', 'done', 'term_fired', 'term_count'):
      np.testing.assert_array_equal(getattr(eng, name).cpu().numpy(), want[name], err_msg='%s of control step %d' % (name, k))
  _assert_final(eng, steps[-1])
  cap._close()


def test_env_and_vector_adapter(torch):
  """Solo8VanillaEnv.step with a TiltTermination and a TimeBasedTermination: fired() is the engine's term_fired, and the vector
  adapter reports a fall as terminated and the time limit as truncated"""
  from gym_solo_amd.vector import Solo8VectorEnv
  case, steps, host, acts = _twin_case(torch, 'float32', N, 'position', 4, TILT)
  env = _env(torch, 'float32', N, 'position', 4, _members(case), True)
  v = Solo8VectorEnv(env)
  for k, want in enumerate(steps):
    obs, rew, terminated, truncated, _ = v.step(acts[k])
    fired = env.termination_factory.fired().cpu().numpy()
    np.testing.assert_array_equal(fired, want['term_fired'])
    np.testing.assert_array_equal(terminated.cpu().numpy(), want['term_fired'] == 1)
    np.testing.assert_array_equal(truncated.cpu().numpy(), want['term_fired'] == 2)
  assert any((s['term_fired'] == 2).any() for s in steps) and any((s['term_fired'] == 1).any() for s in steps)
  env._close()
