"""Fused segments (solo_roll_kernel: one launch runs what were consecutive S-step launches of a rollout slice, with the output epilogue
after every S steps) on the CPU wave emulator - the product kernel source, launch planning, wiring and kernel choice, without a GPU
(tests/emu/emu_roll_harness.cpp, built by tests/emu_roll.py with the flags of tests/emu/Makefile), 8 robots a case.

Every rollout is compared BIT FOR BIT with the existing emulator library (tests/emu/libsolo_emu.so) running the same rollout as the
launches of before: obs, reward and done of every step, the view, state (return and length slots included), counters, targets, the
statistics shards and the per-robot cost.  The harness sizes the record scratch at exactly record_reals(n, S), as the engine does.

The cases: S = 3, K = 10 (a one-step ragged last segment) and S = kPass + 1, K = 2 S + 1 (two epilogue passes per segment, the second
of one step; a one-step ragged segment again), each on one and on two slices, in f64 and f32, with TimeBased(7) and auto-reset on
robots whose counters are staggered so that episodes end on a segment's last step, on the next segment's first step and on the
rollout's last step.

MUTATIONS of the segment code, each applied alone to a copy of the tree, and the tests of this file that then fail (checked by hand
when the kernel was written; `tail_needs_copy` needs a rollout whose last SEGMENT is one step, the others any segmented rollout):
  1. absolute record index - the store `(step - step_begin)` -> `step`, or the epilogue's `k - step_begin` -> `k`:
     test_fused_rollout_equals_the_launches_of_before (every case), and the AddressSanitizer run reports the heap overflow;
  2. missing re-zero - `s_hext` zeroed only `if (first_seg)`: test_a_full_length_reward_program_f32 (the benchmark's reward
     program is too short to reach that block: the other f32 cases pass);
  3. reload of state in segment 2 - the state / counter loads and LDS stores without `first_seg`: every case of
     test_fused_rollout_equals_the_launches_of_before (the second segment restarts from the state before the launch);
  4. ragged count - `step_end = step_begin + seg_len` without the min against B.steps: every case (steps past the rollout's
     end: the action rows, the done rows and the state are wrong; under AddressSanitizer a heap overflow);
  5. tail_needs_copy - `span = plan.S` instead of the launch's span: the one-step last segment is taken for a one-step launch and
     the view is copied once more from the caller's rows (the same bits: three needless copies on the engine's stream) - the
     `view_copied` count of test_fused_rollout_equals_the_launches_of_before and test_view_copy_predicate."""
import os
import subprocess

import numpy as np
import pytest

from gym_solo_amd import abi
from helpers import make_abi
import emu_roll
from emu_kernel import EmuEngine
from epilogue_cases import pass_steps

N = 8
DTYPES = ['float64', 'float32']
_CACHE = {}


@pytest.fixture(scope='module')
def lib():
  return emu_roll.load()


def program():
  """the benchmark's program with TimeBased(7): episodes of 8 steps"""
  if 'program' not in _CACHE:
    from test_env_host import make_env
    from gym_solo_amd.workloads import register_benchmark_workload
    env = make_env()
    register_benchmark_workload(env, max_steps=7)
    env._ensure_program()
    _CACHE['program'] = env.engine.program
  prog = _CACHE['program']
  assert prog.num_terms == 1 and prog.term_kind[0] == abi.T_TIME and prog.term_param[0] == 7
  return prog


def cases(dtype):
  p = pass_steps(dtype)
  return [(3, 10), (p + 1, 2 * (p + 1) + 1)]


def start(dtype):
  """(state, snapshot, counters, actions [max K][N][12]): the settled robots, their TimeBased counters 0 .. 7"""
  if dtype not in _CACHE:
    ca, ma = make_abi(dtype, auto_reset=True, settle_steps=40)
    e = EmuEngine(ca, ma, N, program=program())
    e.settle()
    kmax = max(k for _, k in cases(dtype))
    acts = np.random.default_rng(23).uniform(-6, 6, (kmax, N, abi.NUM_JOINTS))
    tc = np.zeros((N, abi.MAX_TERMS), dtype=np.int32)
    tc[:, 0] = np.arange(N) % 8
    _CACHE[dtype] = (e.state.copy(), e.snapshot.copy(), tc, acts)
  return _CACHE[dtype]


def engine(dtype, fused, S, streams):
  ca, ma = make_abi(dtype, auto_reset=True, settle_steps=40, steps_per_launch=S, rollout_streams=streams)
  e = emu_roll.RollEngine(ca, ma, N, program=program()) if fused else EmuEngine(ca, ma, N, program=program())
  state, snapshot, tc, _ = start(dtype)
  e.state[:], e.snapshot[:], e.term_count[:] = state, snapshot, tc
  e.targets[:] = np.array(list(ca.settle_targets))
  return e


def everything(e, outs):
  obs, rew, done = outs
  return dict(obs_rec=obs, reward_rec=rew, done_rec=done, obs=e.obs.copy(), reward=e.reward.copy(), done=e.done.copy(), state=e.state.copy(),
              term_count=e.term_count.copy(), targets=e.targets.copy(), stats=e.stats.copy(), cost=e.cost.copy())


def unfused(dtype, S, K, streams):
  """the existing emulator library's rollout: computed once per case, shared, never modified"""
  key = (dtype, S, K, streams)
  if key not in _CACHE:
    e = engine(dtype, False, S, streams)
    assert e.plan(K) == dict(steps_per_launch=S, launches=-(-K // S), slices=streams, migrate_steps=0)
    _CACHE[key] = everything(e, e.rollout(start(dtype)[3][:K]))
    for v in _CACHE[key].values():
      v.setflags(write=False)
  return _CACHE[key]


@pytest.mark.parametrize('streams', [1, 2])
@pytest.mark.parametrize('which', [0, 1], ids=['S3-K10', 'Spass+1-K2S+1'])
@pytest.mark.parametrize('dtype', DTYPES)
def test_fused_rollout_equals_the_launches_of_before(lib, dtype, which, streams):
  S, K = cases(dtype)[which]
  want = unfused(dtype, S, K, streams)
  e = engine(dtype, True, S, streams)
  got = everything(e, e.rollout(start(dtype)[3][:K]))
  real = 'double' if dtype == 'float64' else 'float'
  # one segmented launch per slice: the plan's report is the one of before, its segments run inside one kernel
  assert e.info == dict(S=S, launches=-(-K // S), slices=streams, migrate=0, fuse=-(-K // S), kernel_launches=streams,
                        segmented_launches=streams, view_copied=0)
  assert e.kernels == ['solo_roll_kernel<%s>' % real]
  for name in want:
    np.testing.assert_array_equal(got[name], want[name], err_msg=name)
  # the schedule the case is about: episodes end on a segment's last step, on a segment's first step and on the rollout's last
  # step; and the last segment is ragged, of one step
  done = want['done_rec'].astype(bool)
  ends = np.flatnonzero(done.any(axis=1))
  assert any(s % S == S - 1 and s != K - 1 for s in ends) and any(s % S == 0 and s > 0 for s in ends) and done[K - 1].any()
  assert not done.all(axis=0).any() and K % S == 1
  assert e.lib.solo_emu_take_fault() == 0


def test_a_full_length_reward_program_f32(lib):
  """f32, lane = row: the epilogue's reward values [instructions][steps of a pass] reach the rows' joint-space block (s_hext) from
  instruction 16 on - the benchmark's program has fewer - and every segment has to zero that block again before its steps, as
  every task of the migrating kernel does.  A reward program of exactly SOLO_MAX_REWARD_OPS instructions, S = kPass + 1 = 33 (a full
  pass: every column of the block is written), K = 2 S + 1."""
  S, K = cases('float32')[1]
  from test_env_host import make_env
  from gym_solo_amd.core import obs as solo_obs
  from gym_solo_amd.core import termination as terms
  import epilogue_cases as ec
  env = make_env()
  env.obs_factory.register_observation(solo_obs.TorsoIMU(env.robot))
  for w, node in ec.full_length_tree():
    env.reward_factory.register_reward(w, ec.build_reward(env, node))
  env.termination_factory.register_termination(terms.TimeBasedTermination(7))
  env._ensure_program()
  prog = env.engine.program
  assert prog.num_reward_ops == abi.MAX_REWARD_OPS > 16
  state, snapshot, tc, acts = start('float32')
  runs = []
  for fused in (False, True):
    ca, ma = make_abi('float32', auto_reset=True, settle_steps=40, steps_per_launch=S, rollout_streams=1)
    e = emu_roll.RollEngine(ca, ma, N, program=prog) if fused else EmuEngine(ca, ma, N, program=prog)
    e.state[:], e.snapshot[:], e.term_count[:] = state, snapshot, tc
    e.targets[:] = np.array(list(ca.settle_targets))
    runs.append(everything(e, e.rollout(acts[:K])))
  assert e.kernels == ['solo_roll_kernel<float>'] and e.info['segmented_launches'] == 1
  for name in runs[0]:
    np.testing.assert_array_equal(runs[1][name], runs[0][name], err_msg=name)
  assert runs[0]['reward_rec'].std() > 0


@pytest.mark.parametrize('dtype', DTYPES)
def test_switched_off_it_is_the_launches_of_before(lib, dtype):
  """PlanInput::fuse = false through the same harness: the kernels of before, launch by launch (the one-step remainder in place, the
  view copied), and the same bits"""
  S, K = cases(dtype)[0]
  want = unfused(dtype, S, K, 2)
  e = engine(dtype, True, S, 2)
  e.fuse = False
  got = everything(e, e.rollout(start(dtype)[3][:K]))
  assert e.info == dict(S=S, launches=4, slices=2, migrate=0, fuse=0, kernel_launches=8, segmented_launches=0, view_copied=1)
  assert e.kernels == ['solo_step_kernel<%s, true, false, false>' % ('double' if dtype == 'float64' else 'float')]
  for name in want:
    np.testing.assert_array_equal(got[name], want[name], err_msg=name)


def test_groups_of_sixteen_segments(lib):
  """K = 17 S + 1 at S = 2: a launch of 16 segments, then one of two (the last one ragged, of one step) - and K = 33: the
  remainder is a single-step LAUNCH, which evaluates in place and has its view copied"""
  dtype = 'float32'
  acts = np.random.default_rng(5).uniform(-6, 6, (35, N, abi.NUM_JOINTS))
  for K, launches, segmented, copied, kernels in ((35, 2, 2, 0, ['solo_roll_kernel<float>']),
                                                  (33, 2, 1, 1, ['solo_roll_kernel<float>', 'solo_step_kernel<float, true, false, false>'])):
    a, b = engine(dtype, False, 2, 1), engine(dtype, True, 2, 1)
    want, got = everything(a, a.rollout(acts[:K])), everything(b, b.rollout(acts[:K]))
    assert b.info == dict(S=2, launches=-(-K // 2), slices=1, migrate=0, fuse=16, kernel_launches=launches, segmented_launches=segmented,
                          view_copied=copied)
    assert b.kernels == kernels
    for name in want:
      np.testing.assert_array_equal(got[name], want[name], err_msg='K = %d: %s' % (K, name))


def test_policy(lib):
  """make_plan: S, launches, slices and migrate are what they were, with the switch on or off; fuse only where the issue allows it"""
  f64, _ = make_abi('float64')
  P = lambda k, **kw: emu_roll.plan(lib, f64, 4096, k, **kw)
  assert P(1000) == dict(S=250, launches=4, slices=2, migrate=0, fuse=4)
  assert P(3000) == dict(S=250, launches=12, slices=2, migrate=0, fuse=12)
  assert P(300) == dict(S=250, launches=2, slices=2, migrate=0, fuse=2)
  assert P(4250)['fuse'] == 16 == P(100000)['fuse']          # (kMaxFusedSegments)
  assert P(20) == dict(S=20, launches=1, slices=1, migrate=0, fuse=0) == P(20, fuse=0)
  assert P(1000, fuse=0) == dict(S=250, launches=4, slices=2, migrate=0, fuse=0)
  for off in (dict(ctl=1), dict(sensing=1), dict(decimation=4), dict(state_terms=1), dict(actuators=1), dict(wrench=1),
              dict(flags=abi.STEP_PHYSICS), dict(flags=abi.STEP_PHYSICS | abi.STEP_DONE), dict(flags=abi.STEP_ALL & ~abi.STEP_PHYSICS)):
    on, was = P(1000, **off), P(1000, fuse=0, **off)
    assert on == was and on['fuse'] == 0 and on['launches'] > 1, off
  one, _ = make_abi('float64', steps_per_launch=1)
  assert emu_roll.plan(lib, one, 64, 33) == dict(S=1, launches=33, slices=2, migrate=0, fuse=0)   # (single steps keep their launches)
  mig, _ = make_abi('float64', migrate_steps=5, steps_per_launch=20)
  assert emu_roll.plan(lib, mig, 64, 100)['migrate'] == 5 and emu_roll.plan(lib, mig, 64, 100)['fuse'] == 0
  # 8192 robots in f64 migrate on one chain: never fused; in f32 they do not, and are
  f32, _ = make_abi('float32')
  assert emu_roll.plan(lib, f64, 8192, 1000) == dict(S=250, launches=4, slices=1, migrate=25, fuse=0)
  assert emu_roll.plan(lib, f32, 8192, 1000) == dict(S=250, launches=4, slices=2, migrate=0, fuse=4)


def test_kernel_choice_and_name(lib):
  """choose_kernel(..., segmented): the roll kernel exactly where solo_step_kernel<T, true, false, false> would have run; today's
  callers (no trailing argument) get today's answers (tests/test_launch_plan.py pins the whole table)"""
  ident, name = np.zeros(5, dtype=np.int32), emu_roll.C.create_string_buffer(96)
  lib.solo_emu_choose_kernel(0, 0, 0, 0, 0, abi.STEP_ALL, abi.F64, ident.ctypes.data, name, 96)
  assert name.value.decode() == 'solo_step_kernel<double, true, false, false>' and int(ident[0]) == 0


def test_every_geometry_is_visited(lib):
  """for_each_geometry (what solo_engine_reserve prepares for): the two-slice geometry of a rollout of several launches is a
  geometry of its own - with the same S and migrate as the 250-step single launch in front of it, it used to be skipped, and the
  slices' streams were never created ahead of a capture"""
  f64, _ = make_abi('float64')
  got = emu_roll.geometries(lib, f64, 256, 600)
  assert (250, 1, 1, 0, 0) in got and (250, 2, 2, 0, 2) in got and (250, 3, 2, 0, 3) in got
  assert any(g[2] == 2 for g in emu_roll.geometries(lib, f64, 256, 600, fuse=0))


def test_view_copy_predicate(lib):
  """tail_needs_copy, seen through the harness: a one-step last SEGMENT inside a fused launch leaves the view itself (K = 10, S = 3);
  a one-step last LAUNCH does not (K = 33, S = 2: test_groups_of_sixteen_segments); without fused segments both are copied"""
  e = engine('float64', True, 3, 1)
  e.rollout(start('float64')[3][:10])
  assert e.info['view_copied'] == 0 and e.info['segmented_launches'] == 1
  e = engine('float64', True, 3, 1)
  e.fuse = False
  e.rollout(start('float64')[3][:10])
  assert e.info['view_copied'] == 1 and e.info['segmented_launches'] == 0


@pytest.mark.parametrize('dtype', DTYPES)
def test_sanitizer_build_runs_clean(dtype, tmp_path):
  """the cases above in a stand-alone program (tests/emu/emu_roll_check.cpp, its own main) under AddressSanitizer and UBSan: fused
  against unfused inside the program, bit for bit, no report"""
  exe = str(tmp_path / 'emu_roll_check')
  flags = ['-O1' if f == '-O2' else f for f in emu_roll.FLAGS if f not in ('-shared', '-fPIC')]
  subprocess.check_call(['g++'] + flags + ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-o', exe,
                                           os.path.join(emu_roll.EMU, 'emu_roll_check.cpp')])
  ca, ma = make_abi(dtype, auto_reset=True, settle_steps=40)
  state, _, tc, acts = start(dtype)
  spec = np.array([(S, K, streams) for S, K in cases(dtype) for streams in (1, 2)], dtype=np.int32)
  params = np.zeros((N, 4))
  params[:, 0], params[:, 1] = ca.lateral_friction, 1.0
  targets = np.tile(np.array(list(ca.settle_targets)), (N, 1))
  blob = b''.join([bytes(ca), bytes(ma), bytes(program()), np.array([N, len(spec), acts.shape[0]], dtype=np.int32).tobytes(), spec.tobytes(),
                   state.tobytes(), params.tobytes(), targets.tobytes(), np.ascontiguousarray(acts).tobytes(), tc.tobytes()])
  (tmp_path / 'call.bin').write_bytes(blob)
  run = subprocess.run([exe, str(tmp_path / 'call.bin')], capture_output=True, text=True,
                       env=dict(os.environ, UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1', ASAN_OPTIONS='detect_leaks=0'))
  assert run.returncode == 0 and 'runtime error' not in run.stderr and 'AddressSanitizer' not in run.stderr, (run.stdout + run.stderr)[-3000:]
  lines = [l for l in run.stdout.split('\n') if l]
  assert len(lines) == len(spec) and all('solo_roll_kernel' in l and l.endswith('equals the unfused rollout') for l in lines), run.stdout
