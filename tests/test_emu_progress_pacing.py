"""Progress pacing of the segmented launch (solo_roll_kernel's segment boundary: a wave counts itself in the progress block and takes
its issue priority for the next segment from its rank) on the CPU wave emulator - the product kernel source with the block wired
(tests/emu/emu_pacing_harness.cpp, built by tests/emu_pacing.py with the flags of tests/emu/Makefile).  4 robots, S = 3, K = 8:
segments of 3, 3 and 2 steps, on one slice and on two, f64 and f32, TimeBased(7) with auto-reset on staggered counters.

Pacing is scheduling: the emulator's waves run one after the other, so the ranks are the issue order (0, 1, 2, 3: with quarters, robot 0
is "early" and robot 3 "late" at both boundaries - both biases are exercised, and the bias of the first boundary is taken back out at
the second), and every value a caller can see has to equal the run with a null block BIT FOR BIT: obs, reward and done of every
step, the view, state, counters, targets, the statistics and the per-robot cost (a difference inside one segment, which the bias
must cancel out of).  The block itself: n in the counters of the segments that have a successor, 0 elsewhere.

What the emulator cannot see is the priority itself (its wave_set_priority_level does nothing): that the bias holds the pin's test one
way or the other, and comes back out of the history, is pinned by the static_asserts next to pace_sweeps / pace_bias
(solo_step_kernel.h) and measured on the GPU (tools/gpu_tail.py)."""
import os
import subprocess

import numpy as np
import pytest

from gym_solo_amd import abi
from helpers import make_abi
import emu_pacing
from emu_kernel import EmuEngine

N, S, K = 4, 3, 8
DTYPES = ['float64', 'float32']
_CACHE = {}


def program():
  """the benchmark's program with TimeBased(7): episodes of 8 steps"""
  if 'program' not in _CACHE:
    from test_env_host import make_env
    from gym_solo_amd.workloads import register_benchmark_workload
    env = make_env()
    register_benchmark_workload(env, max_steps=7)
    env._ensure_program()
    _CACHE['program'] = env.engine.program
  return _CACHE['program']


def start(dtype):
  """(state, snapshot, counters, actions [12][N][12]): the settled robots, their TimeBased counters 0, 2, 4, 6"""
  if dtype not in _CACHE:
    ca, ma = make_abi(dtype, auto_reset=True, settle_steps=40)
    e = EmuEngine(ca, ma, N, program=program())
    e.settle()
    acts = np.random.default_rng(41).uniform(-6, 6, (12, N, abi.NUM_JOINTS))
    tc = np.zeros((N, abi.MAX_TERMS), dtype=np.int32)
    tc[:, 0] = 2 * np.arange(N)
    _CACHE[dtype] = (e.state.copy(), e.snapshot.copy(), tc, acts)
  return _CACHE[dtype]


def engine(dtype, kind, streams, spl=S):
  """kind: 'paced' / 'null' (the pacing harness, block wired / null) or 'unfused' (the existing emulator library)"""
  ca, ma = make_abi(dtype, auto_reset=True, settle_steps=40, steps_per_launch=spl, rollout_streams=streams)
  e = EmuEngine(ca, ma, N, program=program()) if kind == 'unfused' else emu_pacing.PacedEngine(ca, ma, N, program=program(), paced=kind == 'paced')
  state, snapshot, tc, _ = start(dtype)
  e.state[:], e.snapshot[:], e.term_count[:] = state, snapshot, tc
  e.targets[:] = np.array(list(ca.settle_targets))
  return e


def everything(e, outs):
  obs, rew, done = outs
  return dict(obs_rec=obs, reward_rec=rew, done_rec=done, obs=e.obs.copy(), reward=e.reward.copy(), done=e.done.copy(), state=e.state.copy(),
              term_count=e.term_count.copy(), targets=e.targets.copy(), stats=e.stats.copy(), cost=e.cost.copy())


def reference(dtype, kind, streams):
  """the runs without the block: computed once per case, shared, never modified"""
  key = (dtype, kind, streams)
  if key not in _CACHE:
    e = engine(dtype, kind, streams)
    _CACHE[key] = everything(e, e.rollout(start(dtype)[3][:K]))
    if kind == 'null':
      assert e.info['wired_launches'] == 0 and not e.progress.any()
    for v in _CACHE[key].values():
      v.setflags(write=False)
  return _CACHE[key]


@pytest.mark.parametrize('streams', [1, 2])
@pytest.mark.parametrize('dtype', DTYPES)
def test_paced_rollout_equals_the_null_block(dtype, streams):
  e = engine(dtype, 'paced', streams)
  got = everything(e, e.rollout(start(dtype)[3][:K]))
  assert e.info == dict(S=S, launches=3, slices=streams, migrate=0, fuse=3, kernel_launches=streams, wired_launches=streams, view_copied=0)
  assert e.progress.tolist() == [N, N] + [0] * (emu_pacing.COUNTERS - 2)   # (all slices count into ONE block)
  for kind in ('null', 'unfused'):
    want = reference(dtype, kind, streams)
    for name in want:
      np.testing.assert_array_equal(got[name], want[name], err_msg='%s: %s' % (kind, name))
  done = got['done_rec'].astype(bool)
  assert done.any() and not done.all(axis=0).any() and got['cost'].min() > 0   # (episodes end inside the rollout; the cost is the last segment's sweeps)


def test_a_rollout_of_several_launches_per_slice_is_not_paced():
  """K = 17 S + 1 at S = 2 crosses kMaxFusedSegments: the slice's second launch would count into the counters of the first - such a
  rollout gets no block, and runs as before"""
  e = engine('float32', 'paced', 1, spl=2)
  acts = np.random.default_rng(5).uniform(-6, 6, (35, N, abi.NUM_JOINTS))
  e.rollout(acts)
  assert e.info['fuse'] == 16 and e.info['kernel_launches'] == 2 and e.info['wired_launches'] == 0 and not e.progress.any()


@pytest.fixture(scope='module')
def sanitizer_exe(tmp_path_factory):
  """tests/emu/emu_pacing_check.cpp under AddressSanitizer and UBSan: built ONCE for both precisions (the compile is the test's cost)"""
  exe = str(tmp_path_factory.mktemp('pacing_check') / 'emu_pacing_check')
  # (-O0: the instrumented build of every kernel instantiation takes half a minute instead of several at -O1, and nothing the
  # sanitizers look at is optimised away; the emulated rollouts are tiny)
  flags = ['-O0' if f == '-O2' else f for f in emu_pacing.FLAGS if f not in ('-shared', '-fPIC')]
  subprocess.check_call(['g++'] + flags + ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-o', exe,
                                           os.path.join(emu_pacing.EMU, 'emu_pacing_check.cpp')])
  return exe


@pytest.mark.parametrize('dtype', DTYPES)
def test_sanitizer_build_runs_clean(dtype, tmp_path, sanitizer_exe):
  """the cases above, and S = 2, K = 8 (three boundaries: a wave that is late every time) in a stand-alone program
  (tests/emu/emu_pacing_check.cpp, its own main) under AddressSanitizer and UBSan: paced against the null block inside the program,
  bit for bit, the counters, no report"""
  exe = sanitizer_exe
  ca, ma = make_abi(dtype, auto_reset=True, settle_steps=40)
  state, _, tc, acts = start(dtype)
  spec = np.array([(S, K, 1), (S, K, 2), (2, K, 1)], dtype=np.int32)
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
  assert len(lines) == len(spec) and all(l.endswith('equals the run with a null block') for l in lines), run.stdout
