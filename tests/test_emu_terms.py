"""State terminations (solo_term_kernel: SOLO_T_HEIGHT_BELOW / SOLO_T_TILT_ABOVE in the fused step) on the CPU wave emulator - the
product kernel source, launch planning and kernel choice, run without a GPU (tests/emu/emu_terms_harness.cpp, built by
tests/emu_terms.py with the flags of tests/emu/Makefile).

Every identity is taken against THE TWIN of tests/terms_cases.py: the kernels that exist without state terminations, one control
step per launch with auto-reset off, the criterion applied to the twin's own state in numpy and reset(mask) for the robots that
fired.  The engine under test runs the same actions with auto-reset on, closed loop and as fused recorded rollouts, and must
equal the twin BIT FOR BIT in state, targets, term_count, term_fired, every control step's obs / reward / done and the episode /
length statistics (the return sums: 1e-12 relative).

3 robots, 40 settle steps (they are still falling from 0.5 m, ~0.4 mm per physics step), K = 5 control steps, D in {1, 3}, f64 and
f32, position and PD.  The snapshot puts the robots at different heights and roll angles, rolling at 3 rad/s, so that within the
five control steps robot 0 crosses a threshold twice (it fires inside a launch, is restored and fires again), robot 1 on the last
step and robot 2 never.  Thresholds come from a free run of the twin (terms_cases.gap_thresholds)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from gym_solo_amd import abi
from helpers import make_abi
import emu_terms
import terms_cases as tc

N, K = 3, 5
HEIGHT, TILT, TIME = abi.T_HEIGHT_BELOW, abi.T_TILT_ABOVE, abi.T_TIME


@pytest.fixture(scope='module')
def lib():
  return emu_terms.load()


_CACHE = {}


def _base_program():
  """The benchmark's observation / reward program (its termination list is replaced per case)"""
  if 'prog' not in _CACHE:
    from test_env_host import make_env
    from gym_solo_amd.workloads import register_benchmark_workload
    env = make_env()
    register_benchmark_workload(env, max_steps=2)
    env._ensure_program()
    _CACHE['prog'] = env.engine.program
  return _CACHE['prog']


def program(terms):
  p = abi.SoloProgram.from_buffer_copy(_base_program())
  p.num_terms = len(terms)
  for t in range(abi.MAX_TERMS):
    p.term_kind[t], p.term_param[t] = (terms[t][0], terms[t][1]) if t < len(terms) else (0, 0)
  return p


def snapshot(dtype, D):
  """the settled snapshot (40 steps: mid-fall, ~0.65 mm per physics step and accelerating), robot i 2.1 mm x D x i higher and
  9.5 mrad x D x i less rolled than robot 0, which is rolled by 0.25 rad; all rolling at 3 rad/s - values of the engine's precision"""
  if dtype not in _CACHE:
    from emu_kernel import EmuEngine
    ca, ma = make_abi(dtype, settle_steps=40)
    e = EmuEngine(ca, ma, N)
    e.settle()
    _CACHE[dtype] = e.snapshot.copy()
  s = _CACHE[dtype].copy()
  for i in range(N):
    a = 0.25 - 9.5e-3 * D * i
    s[i, abi.S_POS + 2] += 2.1e-3 * D * i
    s[i, abi.S_QUAT:abi.S_QUAT + 4] = [np.sin(a / 2), 0.0, 0.0, np.cos(a / 2)]
    s[i, abi.S_ANGVEL] = 3.0
  return s.astype(tc.real(dtype)).astype(np.float64)


def pd_control():
  c = abi.SoloControl()
  c.mode, c.action_scale = abi.CTRL_PD, 1.0
  rng = np.random.default_rng(5)
  for d in range(abi.NUM_DOF):
    c.kp[d], c.kd[d] = rng.uniform(1.0, 4.0), rng.uniform(0.01, 0.05)
  return c


def actions(dtype, mode):
  rng = np.random.default_rng(17)
  ca, _ = make_abi(dtype)
  if mode == 'pd':
    return np.array(list(ca.settle_targets))[None, None, :] + rng.uniform(-0.5, 0.5, (K, N, abi.NUM_JOINTS))
  return rng.uniform(-6, 6, (K, N, abi.NUM_JOINTS))


def sim(lib, dtype, mode, D, terms, auto_reset, **geometry):
  ca, ma = make_abi(dtype, auto_reset=auto_reset, settle_steps=40, **geometry)
  return emu_terms.TermsSim(lib, ca, ma, N, program([(k, p) for k, p, _ in terms]), snapshot(dtype, D), [v for _, _, v in terms],
                            pd_control() if mode == 'pd' else None, D)


class Twin:
  """terms_cases.run_twin's view of a TermsSim whose program never fires"""

  def __init__(self, lib, dtype, mode, D):
    self.sim = sim(lib, dtype, mode, D, [(abi.T_PERPETUAL, 0, 0.0)], False)

  def step(self, a):
    self.sim.step(a, abi.STEP_ALL)

  def reset(self, mask):
    self.sim.reset(mask)

  state = lambda self: self.sim.state
  targets = lambda self: self.sim.targets
  obs = lambda self: self.sim.obs
  reward = lambda self: self.sim.reward


# (dtype, mode, D, kind of the state termination, its grace count, the termination list with None where it sits)
CASES = [
  ('float64', 'position', 3, HEIGHT, 0, [None]),
  ('float32', 'pd', 3, HEIGHT, 1, [None, (TIME, 2, 0.0)]),        # in front of a TimeBased(2)
  ('float64', 'pd', 1, TILT, 0, [(TIME, 2, 0.0), None]),          # behind it
  ('float32', 'position', 1, TILT, 1, [None]),
  ('float32', 'position', 3, TILT, 0, [None, (TIME, 2, 0.0)]),
  ('float64', 'position', 1, HEIGHT, 0, [(TIME, 2, 0.0), None]),
]
IDS = ['%s-%s-D%d-%s-grace%d-%s' % (d, m, D, 'height' if k == HEIGHT else 'tilt', g, 'x'.join('state' if t is None else 'time' for t in l))
       for d, m, D, k, g, l in CASES]


def _twin(lib, case):
  """once per case: the threshold from the free run, then the twin's control steps"""
  if case not in _CACHE:
    dtype, mode, D, kind, grace, layout = CASES[case]
    acts = actions(dtype, mode)
    free, _ = tc.run_twin(Twin(lib, dtype, mode, D), [], acts, dtype, reset_where=False)
    values = np.array([tc.criterion(kind, s['before_reset'], dtype) for s in free])   # [K, N]
    # a third of the evaluated values lie below the threshold: robot 0's from its second control step, robot 1's last
    chosen = None
    for thr in tc.gap_thresholds(values, 1.0 / 3.0):
      terms = [(kind, grace, thr) if t is None else t for t in layout]
      steps, host = tc.run_twin(Twin(lib, dtype, mode, D), terms, acts, dtype)
      if host.margin >= tc.MARGIN[dtype]:
        chosen = (terms, steps, host)
        break
    assert chosen is not None, 'no threshold keeps every evaluated value %g away' % tc.MARGIN[dtype]
    _CACHE[case] = chosen
  return _CACHE[case]


def test_the_twin_runs_the_kernels_of_before(lib):
  for (dtype, mode, D), want in ((('float64', 'position', 1), 'solo_step_kernel<double, true, false, false>'),
                                 (('float32', 'pd', 1), 'solo_ctl_step_kernel<float, true>'),
                                 (('float64', 'pd', 3), 'solo_decim_kernel<double, true, true>')):
    t = Twin(lib, dtype, mode, D)
    t.step(actions(dtype, mode)[0])
    assert t.sim.kernel == want


@pytest.mark.parametrize('case', range(len(CASES)), ids=IDS)
def test_the_inputs_separate_the_robots(lib, case):
  """a condition on the inputs, checked on the twin alone: no evaluated value within 1e-9 (f64) / 1e-5 (f32) of the threshold; at
  least a quarter of the robots fire and at least a quarter never do; an episode ends inside a launch, and in the cases with
  TimeBased(2) that one fires too - on the third control step, the last step of the first launch of 3 + 2"""
  dtype, mode, D, kind, grace, layout = CASES[case]
  terms, steps, host = _twin(lib, case)
  assert host.margin >= tc.MARGIN[dtype]
  fired = np.array([s['term_fired'] for s in steps])   # [K, N]
  by_state = fired == 1 + layout.index(None)
  assert by_state.any(0).sum() * 4 >= N and (~by_state.any(0)).sum() * 4 >= N, fired
  assert fired[1:K - 1].any(), fired
  if len(layout) > 1:
    assert (fired[2] == 1 + (1 - layout.index(None))).any(), fired


def test_the_cases_cover_the_edges(lib):
  """for each kind: a robot that fires inside a launch, is restored and fires again, and an episode that ends on the rollout's last
  control step"""
  for kind in (HEIGHT, TILT):
    twice = last = False
    for case, (dtype, mode, D, k, grace, layout) in enumerate(CASES):
      if k == kind:
        fired = np.array([s['term_fired'] for s in _twin(lib, case)[1]]) == 1 + layout.index(None)
        twice |= bool((fired.sum(0) >= 2).any())
        last |= bool(fired[K - 1].any())
    assert twice and last, kind


def _name(dtype, mode):
  return 'solo_term_kernel<%s, true, %s>' % ('double' if dtype == 'float64' else 'float', 'true' if mode == 'pd' else 'false')


def _assert_step(got, want, k):
  for name in ('state', 'targets', 'term_count'):
    np.testing.assert_array_equal(got[name], want[name], err_msg='%s after control step %d' % (name, k))


@pytest.mark.parametrize('case', range(len(CASES)), ids=IDS)
def test_closed_loop_equals_the_twin(lib, case):
  """K step() calls, each ONE launch of D physics steps with in-place outputs and the in-kernel auto-reset"""
  dtype, mode, D, kind, grace, layout = CASES[case]
  terms, twin, _ = _twin(lib, case)
  s = sim(lib, dtype, mode, D, terms, True)
  for k, a in enumerate(actions(dtype, mode)):
    s.step(a, abi.STEP_ALL)
    assert s.kernel == _name(dtype, mode)
    _assert_step(s.everything(), twin[k], k)
    for name in ('obs', 'reward', 'done', 'term_fired'):
      np.testing.assert_array_equal(getattr(s, name), twin[k][name], err_msg='%s of control step %d' % (name, k))
    tc.assert_stats(s.stats.sum(0), twin[k]['stats'])


@pytest.mark.parametrize('case', range(len(CASES)), ids=IDS)
@pytest.mark.parametrize('spl', [-1, 3])
def test_fused_rollout_equals_the_twin(lib, case, spl):
  """one launch of 5 control steps (episodes end inside it and on its last step) and launches of 3 + 2"""
  dtype, mode, D, kind, grace, layout = CASES[case]
  terms, twin, _ = _twin(lib, case)
  s = sim(lib, dtype, mode, D, terms, True, steps_per_launch=spl)
  obs, rew, done = s.rollout(actions(dtype, mode))
  assert s.kernel == _name(dtype, mode)
  _assert_step(s.everything(), twin[-1], K - 1)
  for k in range(K):
    for got, name in ((obs[k], 'obs'), (rew[k], 'reward'), (done[k], 'done')):
      np.testing.assert_array_equal(got, twin[k][name], err_msg='%s of control step %d' % (name, k))
  for name in ('obs', 'reward', 'done', 'term_fired'):   # (the view: the last control step)
    np.testing.assert_array_equal(getattr(s, name), twin[-1][name], err_msg=name)
  tc.assert_stats(s.stats.sum(0), twin[-1]['stats'])


def test_the_later_counter_is_not_ticked_in_a_firing_step(lib):
  """[Height, TimeBased(2)]: in the control step in which the height termination fires, the TimeBased counter behind it keeps
  its value (and the auto-reset then clears both) - seen with auto-reset OFF, where nothing clears them"""
  case = 1
  dtype, mode, D, kind, grace, layout = CASES[case]
  terms, twin, _ = _twin(lib, case)
  s = sim(lib, dtype, mode, D, terms, False)
  host = tc.HostTerminations(terms, N, dtype)
  seen, history = False, []
  for k, a in enumerate(actions(dtype, mode)):
    s.step(a, abi.STEP_ALL)
    before = host.count.copy()
    fired = host.evaluate(s.state)
    np.testing.assert_array_equal(s.term_fired, fired)
    np.testing.assert_array_equal(s.term_count, host.count)
    by_height = fired == 1
    history.append(by_height)
    if by_height.any():
      seen = True
      np.testing.assert_array_equal(s.term_count[by_height, 1], before[by_height, 1])
      np.testing.assert_array_equal(s.term_count[by_height, 0], before[by_height, 0] + 1)
  assert seen
  # (auto-reset off: it keeps firing while the condition holds)
  history = np.array(history)
  assert (history[1:] & history[:-1]).any()


@pytest.mark.parametrize('case', [0, 2], ids=[IDS[0], IDS[2]])
def test_query_only_launch_evaluates_and_ticks(lib, case):
  """SOLO_STEP_DONE without physics (TerminationFactory.is_terminated() outside step()): the state is not touched, nothing is
  restored, the counters tick and the flags / term_fired are those of the current state"""
  dtype, mode, D, kind, grace, layout = CASES[case]
  terms, twin, _ = _twin(lib, case)
  s = sim(lib, dtype, mode, D, terms, True)
  acts = actions(dtype, mode)
  s.step(acts[0], abi.STEP_ALL)
  host = tc.HostTerminations(terms, N, dtype)
  host.count[:] = s.term_count
  state, targets = s.state.copy(), s.targets.copy()
  for _ in range(2):
    s.step(None, abi.STEP_DONE)
    assert s.kernel == _name(dtype, mode)
    fired = host.evaluate(s.state)
    np.testing.assert_array_equal(s.term_fired, fired)
    np.testing.assert_array_equal(s.done, (fired != 0).astype(np.uint8))
    np.testing.assert_array_equal(s.term_count, host.count)
    np.testing.assert_array_equal(s.state, state)
    np.testing.assert_array_equal(s.targets, targets)


NEVER = [('float64', 'position', 3), ('float32', 'pd', 3), ('float64', 'pd', 1), ('float32', 'position', 1)]


@pytest.mark.parametrize('dtype,mode,D', NEVER)
def test_thresholds_that_never_fire_equal_the_kernels_of_before(lib, dtype, mode, D):
  """height -1e9 and tilt cos = -2 next to a TimeBased(2), against the same program with two PerpetualTerminations in their place on
  the existing kernels: state, obs, reward, done bit for bit; without the TimeBased, the state terminations' counters equal the
  number of control steps"""
  acts = actions(dtype, mode)
  new = sim(lib, dtype, mode, D, [(HEIGHT, 0, -1e9), (TILT, 0, -2.0), (TIME, 2, 0.0)], True)
  old = sim(lib, dtype, mode, D, [(abi.T_PERPETUAL, 0, 0.0), (abi.T_PERPETUAL, 0, 0.0), (TIME, 2, 0.0)], True)
  got, want = new.rollout(acts), old.rollout(acts)
  assert new.kernel == _name(dtype, mode) and not old.kernel.startswith('solo_term_kernel')
  for g, w, name in zip(got, want, ('obs', 'reward', 'done')):
    np.testing.assert_array_equal(g, w, err_msg=name)
  assert want[2].any() and not want[2].all()
  for name in ('state', 'targets', 'obs', 'reward', 'done', 'stats'):
    np.testing.assert_array_equal(getattr(new, name), getattr(old, name), err_msg=name)
  np.testing.assert_array_equal(new.term_count[:, 2], old.term_count[:, 2])
  np.testing.assert_array_equal(new.term_fired, 3 * old.done)   # (the TimeBased in slot 2, where it fired on the last step)
  alone = sim(lib, dtype, mode, D, [(HEIGHT, 0, -1e9), (TILT, 0, -2.0)], True)
  for a in acts[:2]:
    alone.step(a, abi.STEP_ALL)
  alone.rollout(acts[2:])
  np.testing.assert_array_equal(alone.term_count[:, :2], K)
  assert not alone.done.any() and not alone.term_fired.any()


def test_ubsan_build_runs_clean(lib, tmp_path):
  """the same harness under UBSan, as a stand-alone program (tests/emu/emu_terms_ubsan_main.cpp): a recording rollout and a
  query-only launch of case 1 (f32, PD, D = 3, [Height, TimeBased(2)]) - no finding, and the results of the plain build"""
  case = 1
  dtype, mode, D, kind, grace, layout = CASES[case]
  terms, twin, _ = _twin(lib, case)
  exe = str(tmp_path / 'emu_terms_ubsan')
  flags = [f for f in emu_terms.FLAGS if f not in ('-shared', '-fPIC')]
  subprocess.check_call(['g++'] + flags + ['-fsanitize=undefined', '-fno-sanitize-recover=undefined', '-o', exe,
                                           os.path.join(emu_terms.EMU, 'emu_terms_ubsan_main.cpp')])
  s = sim(lib, dtype, mode, D, terms, True)
  acts = np.ascontiguousarray(actions(dtype, mode))
  blob = b''.join([bytes(s.ca), bytes(s.ma), bytes(s.prog), np.int32(1).tobytes(), bytes(s.ctl),
                   np.array([s.ca.dtype, N, K, D], dtype=np.int32).tobytes(), s.values.tobytes(), s.state.tobytes(), s.snapshot.tobytes(),
                   acts.tobytes(), s.targets.tobytes(), s.params.tobytes()])
  (tmp_path / 'call.bin').write_bytes(blob)
  run = subprocess.run([exe, str(tmp_path / 'call.bin'), str(tmp_path / 'out.bin')], capture_output=True, text=True,
                       env=dict(os.environ, UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1'))
  assert run.returncode == 0 and 'runtime error' not in run.stderr, run.stderr[-2000:]
  assert run.stdout.split('\n')[:2] == [_name(dtype, mode)] * 2
  obs, rew, done = s.rollout(acts)
  s.step(None, abi.STEP_DONE)
  out = (tmp_path / 'out.bin').read_bytes()
  want = b''.join([s.state.tobytes(), s.targets.tobytes(), obs.tobytes(), rew.tobytes(), s.term_count.tobytes(), done.tobytes(), s.term_fired.tobytes()])
  assert out == want
