"""External base wrenches (solo_push_kernel: the per-robot world-frame force and torque on the base link in the fused step) on the
CPU wave emulator - the product kernel source, launch planning, kernel choice and the checks of solo_engine_set_base_wrench, run
without a GPU (tests/emu/emu_push_harness.cpp, built by tests/emu_push.py with the flags of tests/emu/Makefile), 8 robots a case.

  1. THE FREE DYNAMICS under a random block against the kinematics-only reference of tests/dynamics_cases.py (tests/push_cases.py:
     air): every model, position / torque / PD, damping on and off, within the counted rounding budget - and the reference with the
     wrench omitted, doubled or read in the base frame misses the same results by >= 100 budgets on >= 90 % of the pushed robots.
  2. ON THE GROUND: Newton's law with the contact multipliers eliminated (tests/push_cases.py: ground), and a standing robot that
     friction holds against 0.2 m g and that 3 m g moves.
  3. TWINS, bit for bit: an all-zero block == off; a fused launch == single steps; D = 3 == three single steps; an in-place write
     == set_base_wrench; resets and restores leave the block alone; a continued run continues; different wrenches move robots apart."""
import os
import subprocess

import numpy as np
import pytest

from gym_solo_amd import abi
from helpers import make_abi
import actuator_cases as ac
import dynamics_cases as dc
import emu_push
import push_cases as pc
from test_emu_terms import program

N, K = 8, 6
TILT, TIME = abi.T_TILT_ABOVE, abi.T_TIME
PLAIN = [(TIME, ac.TIME_LIMIT, 0.0)]
FALLS = [(TILT, 0, ac.TILT_THRESHOLD), (TIME, ac.TIME_LIMIT, 0.0)]
DTYPES = ['float64', 'float32']


@pytest.fixture(scope='module')
def lib():
  return emu_push.load()


def _name(family, dtype, mode, full=True):
  return 'solo_%s_kernel<%s, %s, %s>' % (family, 'double' if dtype == 'float64' else 'float', 'true' if full else 'false',
                                         'false' if mode == 'position' else 'true')


def sim(lib, dtype, mode, D, terms, snapshot, n=N, gains=None, auto_reset=True, ma=None, **cfg):
  ca, ma0 = make_abi(dtype, auto_reset=auto_reset, **cfg)
  kp, kd = gains if gains is not None else ac.pd_gains()
  ctl = None if mode == 'position' else ac.control(mode, kp, kd)
  return emu_push.PushSim(lib, ca, ma if ma is not None else ma0, n, program([(k, p) for k, p, _ in terms]), snapshot, [v for _, _, v in terms], ctl, D)


def _same(a, b, what):
  for name in a:
    assert np.array_equal(a[name], b[name]), '%s: %s' % (what, name)


class Emu:
  """push_cases' engine interface on the emulator"""

  def __init__(self, lib):
    self.lib = lib

  def open(self, ca, ma, n, mode, scales, gains=None, wrench=None, params=None):
    p = np.zeros((n, 4))
    p[:, 0], p[:, 1] = ca.lateral_friction, scales
    if params is not None:
      p[:] = params
    ctl = None
    if mode != 'position':
      kp, kd = gains if gains is not None else (None, None)
      ctl = ac.control(mode, kp, kd)
    return dict(ca=ca, ma=ma, n=n, ctl=ctl, params=p, wrench=wrench)

  def run(self, h, state, acts):
    st = np.ascontiguousarray(state, dtype=np.float64).copy()
    s = emu_push.PushSim(self.lib, h['ca'], h['ma'], h['n'], program([(TIME, 100000)]), st, None, h['ctl'], 1)
    s.params[:] = h['params']
    s.set_base_wrench(h['wrench'])
    if len(acts) == 1:
      s.step(acts[0], abi.STEP_PHYSICS)
    else:
      s.rollout(np.asarray(acts), abi.STEP_PHYSICS)
    assert (s.kernel.startswith('solo_push_kernel') or h['wrench'] is None) and s.stats[:, 5].sum() == 0
    return s.state.copy()

  def close(self, h):
    pass


# ---- 1. the free dynamics --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('damping', [True, False], ids=['damped', 'undamped'])
@pytest.mark.parametrize('mode', ['position', 'torque', 'pd'])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('model', dc.MODELS)
def test_a_step_in_the_air_under_a_wrench_against_the_kinematics_only_reference(lib, model, dtype, mode, damping):
  report, power = pc.air(Emu(lib), dtype, model, N, mode, damping)
  dc.show('emu ' + dtype, '%s, %s, %s' % (mode, model, 'damped' if damping else 'undamped'), report)
  print('self-check, fraction of the pushed robots that miss by >= 100 budgets:', power)
  dc.assert_within_budget(report)
  assert min(power.values()) >= 0.9, power


# ---- 3. twins ---------------------------------------------------------------------------------------------------------------------
ZERO = [(('float64', 'float32')[(m + d + p + a) % 2], mode, D, terms, act)
        for m, mode in enumerate(('position', 'torque', 'pd')) for d, D in enumerate((1, 3)) for p, terms in enumerate((PLAIN, FALLS))
        for a, act in enumerate((False, True))]
ZERO_IDS = ['%s-%s-D%d-%s-%s' % (dt, m, D, 'tilt+time' if t is FALLS else 'time', 'act' if a else 'noact') for dt, m, D, t, a in ZERO]


@pytest.mark.parametrize('dtype,mode,D,terms,act', ZERO, ids=ZERO_IDS)
def test_an_all_zero_block_equals_off(lib, dtype, mode, D, terms, act):
  snap = ac.tilted_snapshot(N, dtype)
  acts = pc.twin_actions(np.random.default_rng(17), dtype, mode, K, N)
  table = ac.random_table(np.random.default_rng(4), N) if act else None
  runs = {}
  for on in (False, True):
    s = sim(lib, dtype, mode, D, terms, snap)     # closed loop ...
    s.set_actuators(table)
    if on:
      s.set_base_wrench(np.zeros((N, abi.WRENCH_WIDTH)))
    per_step = []
    for a in acts:
      s.step(a, abi.STEP_ALL)
      per_step.append(s.everything())
    step_kernel = s.kernel
    r = sim(lib, dtype, mode, D, terms, snap)     # ... and one fused recording rollout, auto-reset on: episodes end inside it
    r.set_actuators(table)
    if on:
      r.set_base_wrench({})
    rec = r.rollout(acts)
    runs[on] = (per_step, step_kernel, rec, r.everything(), r.kernel, r)
  off, new = runs[False], runs[True]
  assert new[1] == new[4] == _name('push', dtype, mode)
  assert not off[1].startswith('solo_push_kernel') and off[1] == off[4]
  if act:
    assert off[1] == _name('act', dtype, mode)
  for k in range(K):
    _same(new[0][k], off[0][k], 'control step %d' % k)
  for g, w, name in zip(new[2], off[2], ('obs', 'reward', 'done')):
    assert np.array_equal(g, w), 'recorded ' + name
  _same(new[3], off[3], 'after the rollout')
  assert off[2][2].any() and not off[2][2].all()     # (episodes ended inside the rollout)
  # switching off again: the previous kernel, and from the same start the same bits
  r = new[5]
  r.set_base_wrench(None)
  r.reset()
  for name in ('stats', 'done', 'term_fired', 'obs', 'reward'):
    getattr(r, name)[:] = 0
  again = r.rollout(acts)
  assert r.kernel == off[4]
  for g, w, name in zip(again, off[2], ('obs', 'reward', 'done')):
    assert np.array_equal(g, w), 'off again: recorded ' + name
  _same(r.everything(), off[3], 'off again')


def test_a_launch_without_physics_keeps_its_kernel(lib):
  snap = ac.tilted_snapshot(N, 'float64')
  s = sim(lib, 'float64', 'position', 1, FALLS, snap)
  s.set_base_wrench(np.zeros((N, 6)))
  s.step(None, abi.STEP_DONE)
  assert s.kernel == _name('term', 'float64', 'position')
  s.set_actuators(np.ones((N, abi.ACTUATOR_WIDTH)))
  s.step(None, abi.STEP_DONE)
  assert s.kernel == _name('act', 'float64', 'position')
  s.step(None, abi.STEP_PHYSICS)
  assert s.kernel == _name('push', 'float64', 'position', full=False)


FUSED = [('float64', 'position'), ('float32', 'torque'), ('float64', 'pd'), ('float32', 'position')]


@pytest.mark.parametrize('dtype,mode', FUSED, ids=['%s-%s' % c for c in FUSED])
def test_a_fused_launch_equals_single_steps_and_decimation_equals_substeps_under_a_random_block(lib, dtype, mode):
  _, ma = make_abi(dtype)
  snap = ac.tilted_snapshot(N, dtype)
  rng = np.random.default_rng(29)
  acts = pc.twin_actions(rng, dtype, mode, K, N)
  table = pc.twin_table(rng, N, ma, dtype)
  fused = sim(lib, dtype, mode, 1, FALLS, snap)
  fused.set_base_wrench(table)
  rec = fused.rollout(acts)
  single = sim(lib, dtype, mode, 1, FALLS, snap)
  single.set_base_wrench(table)
  for k in range(K):
    single.step(acts[k], abi.STEP_ALL)
    assert np.array_equal(single.obs, rec[0][k]) and np.array_equal(single.reward, rec[1][k]) and np.array_equal(single.done, rec[2][k]), k
  _same(fused.everything(), single.everything(), 'fused against single steps')
  assert rec[2].any()
  # D = 3: one control step == three single physics steps under the same block and action
  d3 = sim(lib, dtype, mode, 3, PLAIN, snap, auto_reset=False)
  d3.set_base_wrench(table)
  d3.step(acts[0], abi.STEP_PHYSICS)
  d1 = sim(lib, dtype, mode, 1, PLAIN, snap, auto_reset=False)
  d1.set_base_wrench(table)
  for _ in range(3):
    d1.step(acts[0], abi.STEP_PHYSICS)
  assert np.array_equal(d3.state, d1.state)
  # ... and the block did something: against the run without it
  off = sim(lib, dtype, mode, 1, PLAIN, snap, auto_reset=False)
  for _ in range(3):
    off.step(acts[0], abi.STEP_PHYSICS)
  pushed = np.abs(table[:, :6]).max(axis=1) > 0
  assert (np.abs(off.state - d1.state).max(axis=1)[pushed] > 1e-6).all() and np.array_equal(off.state[~pushed], d1.state[~pushed])


@pytest.mark.parametrize('dtype', DTYPES)
def test_an_in_place_write_equals_set_base_wrench(lib, dtype):
  _, ma = make_abi(dtype)
  snap = ac.tilted_snapshot(N, dtype)
  rng = np.random.default_rng(31)
  acts = pc.twin_actions(rng, dtype, 'position', 2, N)
  t1, t2 = pc.twin_table(rng, N, ma, dtype), pc.twin_table(rng, N, ma, dtype)
  a = sim(lib, dtype, 'position', 1, PLAIN, snap)
  a.set_base_wrench(t1)
  view = a.base_wrench
  a.step(acts[0])
  view[:] = t2
  a.step(acts[1])
  b = sim(lib, dtype, 'position', 1, PLAIN, snap)
  b.set_base_wrench(t1)
  b.step(acts[0])
  b.set_base_wrench(t2)
  assert b.base_wrench is not None and np.array_equal(b.base_wrench, t2)
  b.step(acts[1])
  _same(a.everything(), b.everything(), 'in place against the setter')


def test_resets_leave_the_block_alone_and_a_continued_run_continues(lib):
  dtype, mode, D = 'float32', 'pd', 3
  _, ma = make_abi(dtype)
  snap = ac.tilted_snapshot(N, dtype)
  rng = np.random.default_rng(9)
  acts = pc.twin_actions(rng, dtype, mode, K, N)
  table = pc.twin_table(rng, N, ma, dtype)
  a = sim(lib, dtype, mode, D, FALLS, snap)
  a.set_actuators(ac.random_table(rng, N))
  a.set_base_wrench(table)
  a.rollout(acts[:3])
  saved = {name: getattr(a, name).copy() for name in ('state', 'snapshot', 'targets', 'term_count', 'params', 'stats')}
  a.rollout(acts[3:])
  b = sim(lib, dtype, mode, D, FALLS, snap)
  b.set_actuators(a.actuators)
  b.set_base_wrench(table)
  for name, v in saved.items():
    getattr(b, name)[:] = v
  b.rollout(acts[3:])
  _same(b.everything(), a.everything(), 'continued')
  assert np.array_equal(a.base_wrench, table)     # (the auto-resets inside the rollouts - the tilted robots, TimeBased(3) - left it alone)
  assert a.stats[:, 2].sum() > 0
  a.reset(np.arange(N) % 2 == 0)
  assert np.array_equal(a.base_wrench, table) and np.array_equal(a.snapshot, snap)


@pytest.mark.parametrize('dtype', DTYPES)
def test_a_non_finite_in_place_write_restores_the_robot_and_leaves_the_block(lib, dtype):
  snap = np.tile(ac.settled_row(), (N, 1)).astype(ac.real(dtype)).astype(np.float64)
  s = sim(lib, dtype, 'position', 1, PLAIN, snap)
  s.set_base_wrench(np.zeros((N, 6)))
  s.base_wrench[2, abi.WRENCH_FORCE] = np.nan
  before = s.base_wrench.copy()
  s.step(np.zeros((N, abi.NUM_JOINTS)))
  assert s.stats[:, 5].sum() == 1 and np.isfinite(s.state).all()
  assert np.array_equal(s.state[2, :abi.S_RETURN], snap[2, :abi.S_RETURN])
  np.testing.assert_array_equal(s.base_wrench, before)


@pytest.mark.parametrize('dtype', DTYPES)
def test_different_wrenches_move_robots_apart_under_equal_actions(lib, dtype):
  _, ma = make_abi(dtype)
  snap = np.tile(ac.settled_row(), (N, 1)).astype(ac.real(dtype)).astype(np.float64)
  acts = np.repeat(pc.twin_actions(np.random.default_rng(2), dtype, 'position', 20, 1), N, axis=1)
  mg = pc.total_mass(ma) * pc.G_ACC
  force = np.zeros((N, 3))
  force[:, 0] = np.arange(N) * 0.5 * mg
  s = sim(lib, dtype, 'position', 1, [(TIME, 1000, 0.0)], snap, auto_reset=False)
  s.set_base_wrench({'force': force})
  s.rollout(acts)
  pos = s.state[:, abi.S_POS:abi.S_POS + 3]
  for i in range(N):
    for j in range(i):
      assert np.abs(pos[i] - pos[j]).max() > 1e-6, (i, j)


def test_the_table_is_validated_and_conflicts_are_named(lib):
  snap = ac.tilted_snapshot(N, 'float32')
  s = sim(lib, 'float32', 'position', 1, PLAIN, snap)
  good = np.zeros((N, abi.WRENCH_WIDTH))
  good[:, 0] = -3.0
  s.set_base_wrench(good)
  for bad in (np.nan, np.inf, -np.inf, 1e39):     # (1e39 overflows f32)
    t = good.copy()
    t[3, 4] = bad
    with pytest.raises(ValueError, match='finite'):
      s.set_base_wrench(t)
    assert np.array_equal(s.base_wrench, good)
  with pytest.raises(ValueError, match='base wrenches'):
    s.set_contact_sensing(True)
  s.set_base_wrench(None)
  s.set_contact_sensing(True)
  with pytest.raises(ValueError, match='contact sensing'):
    s.set_base_wrench(good)
  assert s.base_wrench is None


def test_ubsan_build_runs_clean(lib, tmp_path):
  """the same harness under UBSan, as a stand-alone program (tests/emu/emu_push_ubsan_main.cpp): a recording rollout and a
  physics-only launch (f32, PD, D = 3, tilt + time, random scales and a random block) - no finding, and the results of the plain build"""
  dtype, mode, D = 'float32', 'pd', 3
  exe = str(tmp_path / 'emu_push_ubsan')
  flags = ['-O1' if f == '-O2' else f for f in emu_push.FLAGS if f not in ('-shared', '-fPIC')]
  subprocess.check_call(['g++'] + flags + ['-fsanitize=undefined', '-fno-sanitize-recover=undefined', '-o', exe,
                                           os.path.join(emu_push.EMU, 'emu_push_ubsan_main.cpp')])
  n, k = 4, 4
  _, ma = make_abi(dtype)
  rng = np.random.default_rng(9)
  s = sim(lib, dtype, mode, D, FALLS, ac.tilted_snapshot(8, dtype)[4:], n=n)
  s.set_actuators(ac.random_table(rng, n))
  s.set_base_wrench(pc.twin_table(rng, n, ma, dtype))
  acts = np.ascontiguousarray(pc.twin_actions(rng, dtype, mode, k, n))
  blob = b''.join([bytes(s.ca), bytes(s.ma), bytes(s.prog), np.int32(1).tobytes(), bytes(s.ctl),
                   np.array([s.ca.dtype, n, k, D], dtype=np.int32).tobytes(), s.values.tobytes(), s.state.tobytes(), s.snapshot.tobytes(),
                   acts.tobytes(), s.targets.tobytes(), s.params.tobytes(), s.actuators.tobytes(), s.base_wrench.tobytes()])
  (tmp_path / 'call.bin').write_bytes(blob)
  run = subprocess.run([exe, str(tmp_path / 'call.bin'), str(tmp_path / 'out.bin')], capture_output=True, text=True,
                       env=dict(os.environ, UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1'))
  assert run.returncode == 0 and 'runtime error' not in run.stderr, run.stderr[-2000:]
  assert run.stdout.split('\n')[:2] == [_name('push', dtype, mode), _name('push', dtype, mode, full=False)]
  obs, rew, done = s.rollout(acts)
  s.step(acts[0], abi.STEP_PHYSICS)
  out = (tmp_path / 'out.bin').read_bytes()
  want = b''.join([s.state.tobytes(), s.targets.tobytes(), obs.tobytes(), rew.tobytes(), s.term_count.tobytes(), done.tobytes(), s.term_fired.tobytes()])
  assert out == want


# ---- 2. on the ground -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_newtons_law_on_the_ground_with_the_multipliers_eliminated(lib, dtype):
  ca, _ = make_abi(dtype)
  report, skipped, power, pressing = pc.ground(Emu(lib), dtype, N, ca.solver_ulp_tolerance)
  dc.show('emu ' + dtype, 'ground, torque', report)
  print('skipped %.2f of the robot-steps; without Q\' the fit misses by >= 100 budgets on %.2f of the pushed ones; %d pressing rows' % (skipped, power, pressing))
  dc.assert_within_budget(report)
  assert skipped <= pc.MAX_SKIPPED and power >= 0.9 and pressing > 0


@pytest.mark.parametrize('dtype', DTYPES)
def test_friction_holds_a_standing_robot_against_a_small_push_and_a_large_one_moves_it(lib, dtype):
  from f32_cases import REST
  speed, _ = pc.standing_push(Emu(lib), dtype, 0.2)
  _, moved = pc.standing_push(Emu(lib), dtype, 3.0, steps=50)
  print('0.2 m g for 200 steps: base speed %.3g m/s (rest: %.3g); 3 m g for 50 steps: moved %.3g m' % (speed, REST, moved))
  assert speed < REST
  assert moved > 1e-2
