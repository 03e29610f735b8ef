"""The launch planning the engine and the CPU emulator share (gym_solo_amd/csrc/solo_launch.h), without a GPU: the launch
policy, the choice of the step-kernel instantiation, the sizing of the migration queues, and WHOLE rollouts on the emulator -
cut into launches and slices by the product's own enumerator, wired by the product's own wire_launch, on record scratch and
queues of exactly the sizes the engine allocates - against single step() launches, bit for bit.

The view after a recording rollout whose last launch cannot write it (a one-step remainder with in-place outputs; a rollout
without observations and rewards, which has no epilogue): the COPY stays with the caller - Engine::rollout enqueues three
device-to-device copies, the emulator harness copies the same rows - and both ask the shared predicate tail_needs_copy.

`python tests/test_launch_plan.py DIR` writes the configuration, model and program of the rollout cases as raw structs for
tests/emu/emu_launch_check.cpp, the stand-alone AddressSanitizer / UBSan run of the same cases (make -C tests/emu asan-check)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import emu_kernel
from emu_kernel import EmuEngine
from gym_solo_amd import abi
from helpers import make_abi

N = 8


@pytest.fixture(scope='module')
def lib():
  lib = emu_kernel.load()
  lib.solo_emu_choose_kernel.restype = C.c_int
  lib.solo_emu_choose_kernel.argtypes = [C.c_int] * 5 + [C.c_uint32, C.c_int, C.c_void_p, C.c_char_p, C.c_int]
  lib.solo_emu_queue_ints.restype = C.c_longlong
  lib.solo_emu_queue_ints.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_longlong)]
  lib.solo_emu_queue_sweep.restype = C.c_longlong
  lib.solo_emu_queue_sweep.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_longlong)]
  return lib


def _plan(lib, n, dtype, k, flags=abi.STEP_ALL, resident=4096, ctl=False, sensing=False, **geometry):
  ca, _ = make_abi(dtype, **geometry)
  out = np.zeros(4, dtype=np.int32)
  lib.solo_emu_plan(C.byref(ca), ca.dtype, n, resident, int(ctl), int(sensing), k, flags, out.ctypes.data)
  return dict(zip(('S', 'launches', 'slices', 'migrate'), (int(x) for x in out)))


def test_policy_table(lib):
  """make_plan, every value read off the launch policy as it stood inside Engine<T> (4096 resident robots)."""
  def check(expected, *a, **kw):
    got = _plan(lib, *a, **kw)
    assert {key: got[key] for key in expected} == expected, (a, kw, got)
  check(dict(S=20, launches=1, slices=1, migrate=0), 4096, 'float64', 20)
  check(dict(migrate=10, slices=1), 8192, 'float64', 20)
  check(dict(S=250, launches=4, migrate=25, slices=1), 8192, 'float64', 1000)
  check(dict(migrate=0, slices=2), 8192, 'float32', 1000)
  check(dict(migrate=0, slices=2), 8192, 'float64', 1000, flags=abi.STEP_PHYSICS)
  check(dict(migrate=0, slices=2), 8192, 'float64', 1000, ctl=True)
  check(dict(migrate=0, slices=2), 8192, 'float64', 1000, sensing=True)
  check(dict(S=40, launches=1, migrate=20), 8192, 'float64', 40)    # (S < 50: only the single-launch branch migrates)
  check(dict(S=7), 1 << 24, 'float64', 20)                           # (the 2^32-element cap of one launch's records)
  check(dict(S=1, launches=33), 4096, 'float64', 33, steps_per_launch=1)
  check(dict(slices=8), 4096, 'float64', 20, rollout_streams=64)
  check(dict(slices=1), 3, 'float64', 20, rollout_streams=2)         # (a slice needs n >= 2 x streams)
  check(dict(migrate=7), 4096, 'float64', 20, migrate_steps=7)


# sensing, control active, settling, residual threshold, queue, flags -> the instantiation (f64), transcribed from the ladder
# of Engine<T>::launch_chain as it stood before solo_launch.h
KERNELS = """
0 0 0 0 0 PHYSICS solo_step_kernel<double, false, false, false>
0 0 0 0 0 ALL     solo_step_kernel<double, true, false, false>
0 0 0 0 1 PHYSICS solo_step_kernel<double, true, false, true>
0 0 0 0 1 ALL     solo_step_kernel<double, true, false, true>
0 0 0 1 0 PHYSICS solo_step_kernel<double, false, true, false>
0 0 0 1 0 ALL     solo_step_kernel<double, true, true, false>
0 0 0 1 1 PHYSICS solo_step_kernel<double, true, true, true>
0 0 0 1 1 ALL     solo_step_kernel<double, true, true, true>
0 0 1 0 0 PHYSICS solo_step_kernel<double, false, false, false>
0 0 1 0 0 ALL     solo_step_kernel<double, true, false, false>
0 0 1 0 1 PHYSICS solo_step_kernel<double, true, false, true>
0 0 1 0 1 ALL     solo_step_kernel<double, true, false, true>
0 0 1 1 0 PHYSICS solo_step_kernel<double, false, true, false>
0 0 1 1 0 ALL     solo_step_kernel<double, true, true, false>
0 0 1 1 1 PHYSICS solo_step_kernel<double, true, true, true>
0 0 1 1 1 ALL     solo_step_kernel<double, true, true, true>
0 1 0 0 0 PHYSICS solo_ctl_step_kernel<double, false>
0 1 0 0 0 ALL     solo_ctl_step_kernel<double, true>
0 1 0 0 1 PHYSICS solo_ctl_step_kernel<double, false>
0 1 0 0 1 ALL     solo_ctl_step_kernel<double, true>
0 1 0 1 0 PHYSICS solo_ctl_step_kernel<double, false>
0 1 0 1 0 ALL     solo_ctl_step_kernel<double, true>
0 1 0 1 1 PHYSICS solo_ctl_step_kernel<double, false>
0 1 0 1 1 ALL     solo_ctl_step_kernel<double, true>
0 1 1 0 0 PHYSICS solo_step_kernel<double, false, false, false>
0 1 1 0 0 ALL     solo_step_kernel<double, true, false, false>
0 1 1 0 1 PHYSICS solo_step_kernel<double, true, false, true>
0 1 1 0 1 ALL     solo_step_kernel<double, true, false, true>
0 1 1 1 0 PHYSICS solo_step_kernel<double, false, true, false>
0 1 1 1 0 ALL     solo_step_kernel<double, true, true, false>
0 1 1 1 1 PHYSICS solo_step_kernel<double, true, true, true>
0 1 1 1 1 ALL     solo_step_kernel<double, true, true, true>
1 0 0 0 0 PHYSICS solo_contact_kernel<double, false, false>
1 0 0 0 0 ALL     solo_contact_kernel<double, true, false>
1 0 0 0 1 PHYSICS solo_contact_kernel<double, false, false>
1 0 0 0 1 ALL     solo_contact_kernel<double, true, false>
1 0 0 1 0 PHYSICS solo_contact_kernel<double, false, false>
1 0 0 1 0 ALL     solo_contact_kernel<double, true, false>
1 0 0 1 1 PHYSICS solo_contact_kernel<double, false, false>
1 0 0 1 1 ALL     solo_contact_kernel<double, true, false>
1 0 1 0 0 PHYSICS solo_step_kernel<double, false, false, false>
1 0 1 0 0 ALL     solo_step_kernel<double, true, false, false>
1 0 1 0 1 PHYSICS solo_step_kernel<double, true, false, true>
1 0 1 0 1 ALL     solo_step_kernel<double, true, false, true>
1 0 1 1 0 PHYSICS solo_step_kernel<double, false, true, false>
1 0 1 1 0 ALL     solo_step_kernel<double, true, true, false>
1 0 1 1 1 PHYSICS solo_step_kernel<double, true, true, true>
1 0 1 1 1 ALL     solo_step_kernel<double, true, true, true>
1 1 0 0 0 PHYSICS solo_contact_kernel<double, false, true>
1 1 0 0 0 ALL     solo_contact_kernel<double, true, true>
1 1 0 0 1 PHYSICS solo_contact_kernel<double, false, true>
1 1 0 0 1 ALL     solo_contact_kernel<double, true, true>
1 1 0 1 0 PHYSICS solo_contact_kernel<double, false, true>
1 1 0 1 0 ALL     solo_contact_kernel<double, true, true>
1 1 0 1 1 PHYSICS solo_contact_kernel<double, false, true>
1 1 0 1 1 ALL     solo_contact_kernel<double, true, true>
1 1 1 0 0 PHYSICS solo_step_kernel<double, false, false, false>
1 1 1 0 0 ALL     solo_step_kernel<double, true, false, false>
1 1 1 0 1 PHYSICS solo_step_kernel<double, true, false, true>
1 1 1 0 1 ALL     solo_step_kernel<double, true, false, true>
1 1 1 1 0 PHYSICS solo_step_kernel<double, false, true, false>
1 1 1 1 0 ALL     solo_step_kernel<double, true, true, false>
1 1 1 1 1 PHYSICS solo_step_kernel<double, true, true, true>
1 1 1 1 1 ALL     solo_step_kernel<double, true, true, true>
"""


def test_kernel_choice_table(lib):
  rows = [line.split(None, 6) for line in KERNELS.strip().splitlines()]
  want = {(int(s), int(c), int(t), int(r), int(q), f): name for s, c, t, r, q, f, name in rows}
  flags = {'PHYSICS': abi.STEP_PHYSICS, 'ALL': abi.STEP_ALL}
  assert len(want) == 64
  for key in itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (0, 1), ('PHYSICS', 'ALL')):
    for dtype, real in ((abi.F64, 'double'), (abi.F32, 'float')):
      ident, name = np.zeros(5, dtype=np.int32), C.create_string_buffer(96)
      lib.solo_emu_choose_kernel(*key[:5], flags[key[5]], dtype, ident.ctypes.data, name, 96)
      assert name.value.decode() == want[key].replace('double', real), key
      family, full, resid, migrate, ctl = (int(x) for x in ident)
      args = want[key].split('<')[1].rstrip('>').split(', ')[1:]
      assert ['solo_step_kernel', 'solo_ctl_step_kernel', 'solo_contact_kernel'][family] == want[key].split('<')[0]
      assert {0: [full, resid, migrate], 1: [full], 2: [full, ctl]}[family] == [a == 'true' for a in args], key


def test_reported_kernel_names(lib):
  """what solo_engine_kernel_name reports (the full, non-migrating instantiation): the literal strings of Engine<T>::kernel_name
  as it stood - tests, bench.py and tools compare them"""
  literal = {
    (1, 1, 0): 'solo_contact_kernel<%s, true, true>', (1, 0, 0): 'solo_contact_kernel<%s, true, false>',
    (1, 1, 1): 'solo_contact_kernel<%s, true, true>', (1, 0, 1): 'solo_contact_kernel<%s, true, false>',
    (0, 1, 0): 'solo_ctl_step_kernel<%s, true>', (0, 1, 1): 'solo_ctl_step_kernel<%s, true>',
    (0, 0, 1): 'solo_step_kernel<%s, true, true, false>', (0, 0, 0): 'solo_step_kernel<%s, true, false, false>'}
  for (sensing, ctl, resid), fmt in literal.items():
    for dtype, real in ((abi.F64, 'double'), (abi.F32, 'float')):
      ident, name = np.zeros(5, dtype=np.int32), C.create_string_buffer(96)
      lib.solo_emu_choose_kernel(sensing, ctl, 0, resid, 0, abi.STEP_ALL, dtype, ident.ctypes.data, name, 96)
      assert name.value.decode() == fmt % real


def test_every_launch_of_a_chain_fits_its_queue_region(lib):
  """The queue of a launch of `steps` <= S steps against the region queue_slots_per_robot gives it, for every S <= 260, every
  migrate <= S and every steps <= S at 16 robots: chunks <= min(127, ceil(S / migrate)) whatever migration_chunk_steps does
  to the chunk length.  Includes the tail of ADVICE r5: S 128, migrate 1, 65 steps - 65 chunks where the full launch has 64."""
  region = C.c_longlong()
  ints = lib.solo_emu_queue_ints(128, 1, 65, 16, C.byref(region))
  assert ints == 256 + 16 + 16 * 65 and ints <= region.value == 256 + 16 * 128
  assert lib.solo_emu_queue_ints(128, 1, 128, 16, C.byref(region)) == 256 + 16 + 16 * 64   # (the full launch: 64 chunks of 2)
  cases = C.c_longlong()
  assert lib.solo_emu_queue_sweep(260, 16, C.byref(cases)) == 0
  assert cases.value == sum(s * s for s in range(1, 261))


# ---- whole rollouts -----------------------------------------------------------------------------------------------------
CASES = {
  # a ragged last launch of 2 steps on two slices
  'a': dict(k=23, geometry=dict(steps_per_launch=7, rollout_streams=2), plan=dict(steps_per_launch=7, launches=4, slices=2, migrate_steps=0)),
  # the remainder is a one-step launch: in-place outputs, the view is copied (module docstring)
  'b': dict(k=22, geometry=dict(steps_per_launch=7, rollout_streams=2), plan=dict(steps_per_launch=7, launches=4, slices=2, migrate_steps=0)),
  # the ragged tail (65 steps: 65 chunks of 1) needs more chunks than the full launch (128 steps: 64 chunks of 2)
  'c1': dict(k=193, geometry=dict(steps_per_launch=128, migrate_steps=1, rollout_streams=1), plan=dict(steps_per_launch=128, launches=2, slices=1, migrate_steps=1)),
  'c2': dict(k=193, geometry=dict(steps_per_launch=128, migrate_steps=1, rollout_streams=2), plan=dict(steps_per_launch=128, launches=2, slices=2, migrate_steps=1)),
  # no observations, no rewards: no epilogue, the done flags go straight to [K][N]
  'd': dict(k=23, geometry=dict(steps_per_launch=7, rollout_streams=2), flags=abi.STEP_PHYSICS | abi.STEP_DONE, plan=dict(steps_per_launch=7, launches=4, slices=2, migrate_steps=0)),
}
_REFERENCE = {}


def _program():
  from test_emu_kernel import bench_program
  if 'program' not in _REFERENCE:
    _REFERENCE['program'] = bench_program()
  return _REFERENCE['program']


def _engine(dtype, **geometry):
  ca, ma = make_abi(dtype, auto_reset=True, settle_steps=40, **geometry)
  return EmuEngine(ca, ma, N, program=_program())


def _reference(dtype, flags):
  """193 single step() launches from the settled state, computed once per precision and flag set: the state, counters and view
  after every step"""
  key = (dtype, flags)
  if key not in _REFERENCE:
    e = _engine(dtype)
    e.settle()
    start = (e.state.copy(), e.snapshot.copy())
    acts = np.random.default_rng(11).uniform(-6, 6, (193 if flags == abi.STEP_ALL else 23, N, 12))
    steps = []
    for a in acts:
      e.step(a, flags)
      steps.append((e.state.copy(), e.term_count.copy(), e.obs.copy(), e.reward.copy(), e.done.copy()))
    _REFERENCE[key] = (start, acts, steps)
  return _REFERENCE[key]


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('case', sorted(CASES))
def test_whole_rollout_equals_single_steps(case, dtype):
  spec = CASES[case]
  k, flags = spec['k'], spec.get('flags', abi.STEP_ALL)
  start, acts, steps = _reference(dtype, flags)
  e = _engine(dtype, **spec['geometry'])
  assert e.plan(k, flags) == spec['plan']
  e.state[:], e.snapshot[:] = start
  obs, rew, done = e.rollout(acts[:k], flags)
  state, term_count, view_obs, view_reward, view_done = steps[k - 1]
  np.testing.assert_array_equal(e.state, state)
  np.testing.assert_array_equal(e.term_count, term_count)
  np.testing.assert_array_equal(done, np.stack([s[4] for s in steps[:k]]))
  np.testing.assert_array_equal(e.done, view_done)
  assert done.any() and not done.all()   # (TimeBased(4) with auto-reset: episodes end inside the launches)
  if flags & abi.STEP_OBS:
    np.testing.assert_array_equal(obs, np.stack([s[2] for s in steps[:k]]))
    np.testing.assert_array_equal(rew, np.stack([s[3] for s in steps[:k]]))
    np.testing.assert_array_equal(e.obs, view_obs)
    np.testing.assert_array_equal(e.reward, view_reward)
  assert e.lib.solo_emu_take_fault() == 0


if __name__ == '__main__':
  import os
  import sys
  ca, ma = make_abi('float64', auto_reset=True, settle_steps=40)
  for name, struct in (('config', ca), ('model', ma), ('program', _program())):
    with open(os.path.join(sys.argv[1], name + '.bin'), 'wb') as f:
      f.write(C.string_at(C.addressof(struct), C.sizeof(struct)))
