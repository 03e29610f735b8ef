"""GPU suite of the external base wrenches (solo_engine_set_base_wrench: a per-robot world-frame force and torque on the base link,
read by solo_push_kernel) through the C-ABI on the MI355X.  The cases of tests/test_emu_push.py at 64 robots:

  1. THE FREE DYNAMICS under a random block against the kinematics-only reference (tests/push_cases.py: air): every model, position /
     torque / PD, damping on and off, within the counted rounding budget; the reference with the wrench omitted, doubled or read in
     the base frame misses by >= 100 budgets on >= 90 % of the pushed robots.
  2. ON THE GROUND: Newton's law with the contact multipliers eliminated (tests/push_cases.py: ground); friction holds a standing
     robot against 0.2 m g, 3 m g moves it.
  3. TWINS, bit for bit: an all-zero block == off; a fused launch == single steps; D = 3 == three single steps; an in-place write ==
     set_base_wrench; settle, reset, the auto-reset, the restore of a diverged robot and checkpoints leave the block alone; different
     wrenches move robots apart.
  4. The setter's validation and the unsupported combinations, in both orders, on the engine itself."""
import numpy as np
import pytest

from gym_solo_amd import abi
from helpers import make_abi
import actuator_cases as ac
import dynamics_cases as dc
import push_cases as pc
from test_gpu_actuators import engine, program, dev, everything, _name, _real, PLAIN, FALLS

pytestmark = pytest.mark.gpu

N, K = 64, 6
DTYPES = ['float64', 'float32']


@pytest.fixture(scope='module')
def torch():
  import torch
  if not torch.cuda.is_available():
    pytest.fail('GPU tests need a visible MI355X')
  return torch


def _same(a, b, what):
  for name in a:
    assert np.array_equal(a[name], b[name]), '%s: %s' % (what, name)


class Hip:
  """push_cases' engine interface on the HIP engine"""

  def __init__(self, torch):
    self.torch = torch

  def _t(self, e, a):
    return self.torch.as_tensor(np.ascontiguousarray(a), device='cuda', dtype=e.tdtype)

  def open(self, ca, ma, n, mode, scales, gains=None, wrench=None, params=None):
    from gym_solo_amd.engine import Engine
    ca.settle_steps = 1     # (the case puts its own states)
    e = Engine(ca, ma, n)
    e.set_params(abi.PARAM_BASE_MASS_SCALE, self._t(e, scales))
    if params is not None:
      e.set_params(abi.PARAM_FRICTION, self._t(e, params[:, 0]))
    if mode != 'position':
      kp, kd = (dc.joint_actions(np.asarray(g)) for g in gains) if gains is not None else (None, None)
      e.set_control(mode, kp=kp, kd=kd, action_scale=1.0)
    if wrench is not None:
      e.set_base_wrench(self._t(e, wrench))
      assert e.kernel_name.startswith('solo_push_kernel')
    return e

  def run(self, e, state, acts):
    e.state.copy_(self._t(e, state))
    if len(acts) == 1:
      e.step(self._t(e, acts[0]), abi.STEP_PHYSICS)
    else:
      e.rollout(self._t(e, np.asarray(acts)), abi.STEP_PHYSICS)
    assert float(e.stats.cpu().numpy()[5]) == 0     # (no robot was restored)
    return e.state.cpu().numpy().astype(np.float64)

  def close(self, e):
    e.close()


# ---- 1. the free dynamics --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('damping', [True, False], ids=['damped', 'undamped'])
@pytest.mark.parametrize('mode', ['position', 'torque', 'pd'])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('model', dc.MODELS)
def test_a_step_in_the_air_under_a_wrench_against_the_kinematics_only_reference(torch, model, dtype, mode, damping):
  report, power = pc.air(Hip(torch), dtype, model, N, mode, damping)
  dc.show('MI355X ' + dtype, '%s, %s, %s' % (mode, model, 'damped' if damping else 'undamped'), report)
  print('self-check, fraction of the pushed robots that miss by >= 100 budgets:', power)
  dc.assert_within_budget(report)
  assert min(power.values()) >= 0.9, power


# ---- 3. twins ---------------------------------------------------------------------------------------------------------------------
ZERO = [(('float64', 'float32')[(m + d + p + a) % 2], mode, D, terms, act)
        for m, mode in enumerate(('position', 'torque', 'pd')) for d, D in enumerate((1, 3)) for p, terms in enumerate((PLAIN, FALLS))
        for a, act in enumerate((False, True))]
ZERO_IDS = ['%s-%s-D%d-%s-%s' % (dt, m, D, 'tilt+time' if t is FALLS else 'time', 'act' if a else 'noact') for dt, m, D, t, a in ZERO]


@pytest.mark.parametrize('dtype,mode,D,terms,act', ZERO, ids=ZERO_IDS)
def test_an_all_zero_block_equals_off(torch, dtype, mode, D, terms, act):
  snap = ac.tilted_snapshot(N, dtype)
  acts_np = pc.twin_actions(np.random.default_rng(17), dtype, mode, K, N)
  table = ac.random_table(np.random.default_rng(4), N) if act else None
  runs = {}
  for on in (False, True):
    s = engine(torch, dtype, mode, D, terms, start=snap)
    r = engine(torch, dtype, mode, D, terms, start=snap)
    if act:
      s.set_actuators(dev(torch, s, table))
      r.set_actuators(dev(torch, r, table))
    before = s.kernel_name
    assert s.base_wrench is None
    if on:
      s.set_base_wrench(torch.zeros(N, abi.WRENCH_WIDTH, device='cuda', dtype=s.tdtype))
      r.set_base_wrench({})
      assert torch.equal(r.base_wrench, torch.zeros(N, abi.WRENCH_WIDTH, device='cuda', dtype=r.tdtype))
    acts = dev(torch, s, acts_np)
    per_step = []
    for a in acts:
      s.step(a, abi.STEP_ALL)
      per_step.append(everything(s))
    rec = [t.cpu().numpy() for t in r.rollout(acts, abi.STEP_ALL, record=True)]
    runs[on] = (per_step, s.kernel_name, rec, everything(r), before, r, acts)
    s.close()
  off, new = runs[False], runs[True]
  assert new[1] == _name('push', dtype, mode) and new[4] == off[4] == off[1]
  if act:
    assert off[1] == _name('act', dtype, mode)
  for k in range(K):
    _same(new[0][k], off[0][k], 'control step %d' % k)
  for g, w, name in zip(new[2], off[2], ('obs', 'reward', 'done')):
    assert np.array_equal(g, w), 'recorded ' + name
  _same(new[3], off[3], 'after the rollout')
  assert off[2][2].any() and not off[2][2].all()
  # switching off again: the previous kernel name, and from the same start the same bits
  r = new[5]
  r.set_base_wrench(None)
  assert r.kernel_name == off[1] and r.base_wrench is None
  r.reset()
  for t in (r.stats_shards, r.done, r.term_fired, r.obs, r.reward):
    t.zero_()
  again = [t.cpu().numpy() for t in r.rollout(new[6], abi.STEP_ALL, record=True)]
  for g, w, name in zip(again, off[2], ('obs', 'reward', 'done')):
    assert np.array_equal(g, w), 'off again: recorded ' + name
  _same(everything(r), off[3], 'off again')
  runs[False][5].close()
  r.close()


FUSED = [('float64', 'position'), ('float32', 'torque'), ('float64', 'pd'), ('float32', 'position')]


@pytest.mark.parametrize('dtype,mode', FUSED, ids=['%s-%s' % c for c in FUSED])
def test_a_fused_launch_equals_single_steps_and_decimation_equals_substeps_under_a_random_block(torch, dtype, mode):
  _, ma = make_abi(dtype)
  snap = ac.tilted_snapshot(N, dtype)
  rng = np.random.default_rng(29)
  acts_np = pc.twin_actions(rng, dtype, mode, K, N)
  table = pc.twin_table(rng, N, ma, dtype)
  fused = engine(torch, dtype, mode, 1, FALLS, start=snap)
  fused.set_base_wrench(dev(torch, fused, table[:, :6]))     # (the [N, 6] form)
  acts = dev(torch, fused, acts_np)
  rec = fused.rollout(acts, abi.STEP_ALL, record=True)
  single = engine(torch, dtype, mode, 1, FALLS, start=snap)
  single.set_base_wrench({'force': dev(torch, single, table[:, 0:3]), 'torque': dev(torch, single, table[:, 3:6])})
  assert torch.equal(single.base_wrench, fused.base_wrench)
  for k in range(K):
    single.step(acts[k], abi.STEP_ALL)
    assert torch.equal(single.obs, rec[0][k]) and torch.equal(single.reward, rec[1][k]) and torch.equal(single.done, rec[2][k]), k
  _same(everything(fused), everything(single), 'fused against single steps')
  assert bool(rec[2].any())
  d3 = engine(torch, dtype, mode, 3, PLAIN, auto_reset=False, start=snap)
  d1 = engine(torch, dtype, mode, 1, PLAIN, auto_reset=False, start=snap)
  off = engine(torch, dtype, mode, 1, PLAIN, auto_reset=False, start=snap)
  for e in (d3, d1):
    e.set_base_wrench(dev(torch, e, table))
  d3.step(acts[0], abi.STEP_PHYSICS)
  for _ in range(3):
    d1.step(acts[0], abi.STEP_PHYSICS)
    off.step(acts[0], abi.STEP_PHYSICS)
  assert d3.kernel_name == d1.kernel_name == _name('push', dtype, mode)
  assert torch.equal(d3.state, d1.state)
  pushed = np.abs(table[:, :6]).max(axis=1) > 0
  a, b = off.state.cpu().numpy(), d1.state.cpu().numpy()
  assert (np.abs(a - b).max(axis=1)[pushed] > 1e-6).all() and np.array_equal(a[~pushed], b[~pushed])
  for e in (fused, single, d3, d1, off):
    e.close()


@pytest.mark.parametrize('dtype', DTYPES)
def test_an_in_place_write_equals_set_base_wrench(torch, dtype):
  _, ma = make_abi(dtype)
  snap = ac.tilted_snapshot(N, dtype)
  rng = np.random.default_rng(31)
  acts_np = pc.twin_actions(rng, dtype, 'position', 2, N)
  t1, t2 = pc.twin_table(rng, N, ma, dtype), pc.twin_table(rng, N, ma, dtype)
  a = engine(torch, dtype, 'position', 1, PLAIN, start=snap)
  b = engine(torch, dtype, 'position', 1, PLAIN, start=snap)
  acts = dev(torch, a, acts_np)
  a.set_base_wrench(dev(torch, a, t1))
  view = a.base_wrench
  a.step(acts[0])
  view.copy_(dev(torch, a, t2))
  a.step(acts[1])
  b.set_base_wrench(dev(torch, b, t1))
  ptr = b.base_wrench.data_ptr()
  b.step(acts[0])
  b.set_base_wrench(dev(torch, b, t2))
  assert b.base_wrench.data_ptr() == ptr     # (the pointer is stable while the block stays on)
  b.step(acts[1])
  _same(everything(a), everything(b), 'in place against the setter')
  a.close(); b.close()


def test_settle_resets_restores_and_checkpoints_leave_the_block_alone(torch):
  dtype, mode, D = 'float32', 'pd', 3
  _, ma = make_abi(dtype)
  rng = np.random.default_rng(9)
  table = pc.twin_table(rng, N, ma, dtype)
  table[:, 6:] = 5.0     # (the reserved columns stay as uploaded)
  a = engine(torch, dtype, mode, D, FALLS)
  snapshot = a.snapshot.clone()
  a.set_base_wrench(dev(torch, a, table))
  block = a.base_wrench.clone()
  a.settle()
  assert torch.equal(a.snapshot, snapshot) and torch.equal(a.state, snapshot)   # (the settle loop does not read the block)
  assert torch.equal(a.base_wrench, block)
  tilted = dev(torch, a, ac.tilted_snapshot(N, dtype))
  a.snapshot.copy_(tilted); a.state.copy_(tilted)
  acts = dev(torch, a, pc.twin_actions(rng, dtype, mode, K, N))
  a.rollout(acts[:3], abi.STEP_ALL)
  assert a.stats.cpu().numpy()[2] > 0            # (auto-resets happened: the tilted robots fire every control step)
  assert torch.equal(a.base_wrench, block)
  ck = a.get_state()
  assert 'base_wrench' not in ck and 'wrench' not in ck
  a.rollout(acts[3:], abi.STEP_ALL)
  want = everything(a)
  mask = torch.zeros(N, device='cuda', dtype=torch.uint8)
  mask[::2] = 1
  a.reset(mask)
  assert torch.equal(a.base_wrench, block)
  b = engine(torch, dtype, mode, D, FALLS)
  b.set_base_wrench(dev(torch, b, table))
  b.set_state(ck)
  b.rollout(acts[3:], abi.STEP_ALL)
  got = everything(b)
  for name in ('state', 'targets', 'obs', 'reward', 'done', 'term_count', 'stats_shards'):
    assert np.array_equal(got[name], want[name]), name
  # a non-finite in-place write: the robot diverges, is restored and counted; the block stays as written
  before = float(b.stats.cpu().numpy()[5])
  b.base_wrench[2, abi.WRENCH_FORCE] = float('nan')
  kept = b.base_wrench.clone()
  b.step(acts[0], abi.STEP_ALL)
  assert float(b.stats.cpu().numpy()[5]) == before + 1 and bool(torch.isfinite(b.state).all())
  assert torch.equal(torch.nan_to_num(b.base_wrench, nan=-1.0), torch.nan_to_num(kept, nan=-1.0))
  a.close(); b.close()


@pytest.mark.parametrize('dtype', DTYPES)
def test_different_wrenches_move_robots_apart_under_equal_actions(torch, dtype):
  _, ma = make_abi(dtype)
  eng = engine(torch, dtype, 'position', 1, [(abi.T_TIME, 1000, 0.0)], auto_reset=False)
  acts = dev(torch, eng, np.repeat(pc.twin_actions(np.random.default_rng(2), dtype, 'position', 20, 1), N, axis=1))
  mg = pc.total_mass(ma) * pc.G_ACC
  force = torch.zeros(N, 3, device='cuda', dtype=eng.tdtype)
  force[:, 0] = (1.0 + 0.05 * torch.arange(N, device='cuda')) * mg     # (all beyond what friction holds: every robot slides, each its own way)
  eng.set_base_wrench({'force': force})
  eng.rollout(acts, abi.STEP_ALL)
  x = np.sort(eng.state[:, abi.S_POS].cpu().numpy().astype(np.float64))
  assert np.diff(x).min() > 1e-6
  eng.close()


# ---- 4. validation and the unsupported combinations, on the engine ---------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_validation_keeps_the_previous_block(torch, dtype):
  eng = engine(torch, dtype, 'position', 1, PLAIN, n=8)
  good = torch.full((8, abi.WRENCH_WIDTH), -0.5, device='cuda', dtype=eng.tdtype)
  for bad_value in (float('nan'), float('inf'), float('-inf')):
    bad = good.clone()
    bad[3, abi.WRENCH_TORQUE] = bad_value
    with pytest.raises(ValueError, match='finite'):
      eng.set_base_wrench(bad)
    assert not eng.kernel_name.startswith('solo_push_kernel') and eng.base_wrench is None   # ("off" stays in force)
  eng.set_base_wrench(good)
  for bad_value in (float('nan'), float('inf')):
    bad = torch.zeros_like(good)
    bad[7, 0] = bad_value
    with pytest.raises(ValueError, match='finite'):
      eng.set_base_wrench(bad)
    assert torch.equal(eng.base_wrench, good) and eng.kernel_name == 'solo_push_kernel<%s, true, false>' % _real(dtype)
  if dtype == 'float32':     # (what overflows the engine's precision is not finite there)
    with pytest.raises(ValueError, match='finite'):
      eng.set_base_wrench(torch.full((8, 6), 1e39, device='cuda', dtype=torch.float64))
  eng.set_base_wrench(eng.base_wrench)   # (the view itself: validated in place)
  assert torch.equal(eng.base_wrench, good)
  with pytest.raises(ValueError):
    eng.set_base_wrench(torch.ones(8, 5, device='cuda', dtype=eng.tdtype))
  with pytest.raises(ValueError, match='unknown wrench'):
    eng.set_base_wrench({'moment': torch.ones(8, 3, device='cuda')})
  assert eng.plan(20)['migrate_steps'] == 0
  eng.close()


def test_unsupported_combinations_in_both_orders(torch):
  from gym_solo_amd.engine import Engine
  for kw, word in ((dict(migrate_steps=5), 'migrate_steps'), (dict(solver_residual_threshold=1e-7), 'solver_residual_threshold'),
                   (dict(solver_residual_threshold=1e-7, solver_warm_start=0.5), 'solver_')):
    ca, ma = make_abi('float64', **kw)
    eng = Engine(ca, ma, 8)
    with pytest.raises(ValueError, match=word):
      eng.set_base_wrench({})
    eng.set_base_wrench(None)   # (off is always legal)
    eng.close()
  eng = engine(torch, 'float64', 'position', 1, PLAIN, n=8)
  eng.set_contact_sensing(True)
  with pytest.raises(ValueError, match='contact sensing'):
    eng.set_base_wrench({})
  eng.set_contact_sensing(False)
  eng.set_base_wrench({})
  with pytest.raises(ValueError, match='base wrenches'):
    eng.set_contact_sensing(True)
  assert not eng.contact_sensing and eng.kernel_name == 'solo_push_kernel<double, true, false>'
  # a block goes with every control mode, decimation, a state program and the actuator block, whichever is set first
  eng.set_control('pd', kp=1.0, kd=0.1)
  eng.set_decimation(4)
  assert eng.kernel_name == 'solo_push_kernel<double, true, true>'
  eng.set_term_values([ac.TILT_THRESHOLD, 0.0])
  eng.set_program(program(FALLS))
  eng.set_actuators(torch.full((8, abi.ACTUATOR_WIDTH), 0.5, device='cuda', dtype=torch.float64))
  assert eng.kernel_name == 'solo_push_kernel<double, true, true>'
  eng.set_base_wrench(None)
  assert eng.kernel_name == 'solo_act_kernel<double, true, true>'
  eng.set_actuators(None)
  assert eng.kernel_name == 'solo_term_kernel<double, true, true>'
  eng.close()


# ---- 2. on the ground -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_newtons_law_on_the_ground_with_the_multipliers_eliminated(torch, dtype):
  ca, _ = make_abi(dtype)
  report, skipped, power, pressing = pc.ground(Hip(torch), dtype, N, ca.solver_ulp_tolerance)
  dc.show('MI355X ' + dtype, 'ground, torque', report)
  print('skipped %.2f of the robot-steps; without Q\' the fit misses by >= 100 budgets on %.2f of the pushed ones; %d pressing rows' % (skipped, power, pressing))
  dc.assert_within_budget(report)
  assert skipped <= pc.MAX_SKIPPED and power >= 0.9 and pressing > 0


@pytest.mark.parametrize('dtype', DTYPES)
def test_friction_holds_a_standing_robot_against_a_small_push_and_a_large_one_moves_it(torch, dtype):
  from f32_cases import REST
  speed, _ = pc.standing_push(Hip(torch), dtype, 0.2)
  _, moved = pc.standing_push(Hip(torch), dtype, 3.0, steps=50)
  print('0.2 m g for 200 steps: base speed %.3g m/s (rest: %.3g); 3 m g for 50 steps: moved %.3g m' % (speed, REST, moved))
  assert speed < REST
  assert moved > 1e-2
