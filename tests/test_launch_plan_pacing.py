"""The wiring of the progress block (gym_solo_amd/csrc/solo_launch.h: progress_ints, rollout_is_paced, wire_launch's
KBuffers::progress), without a GPU and without running a kernel: tests/emu/emu_pacing_harness.cpp's solo_emu_pacing_wiring plans a
rollout with the product's make_plan, enumerates its launches with for_each_launch, wires each with wire_launch against an engine
whose EngineBuffers::progress is set, and reports which block every launch got."""
import pytest

from gym_solo_amd import abi
from helpers import make_abi
import emu_pacing


@pytest.fixture(scope='module')
def lib():
  return emu_pacing.load()


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_every_slice_of_a_fused_plan_gets_the_same_block(lib, dtype):
  ca, _ = make_abi(dtype)
  plan, launches, _ = emu_pacing.wiring(lib, ca, 4096, 3000)
  assert plan == dict(S=250, launches=12, slices=2, fuse=12, progress_ints=16, paced=1)
  assert launches == [(0, 1, 1), (1, 1, 1)]          # (slice, segmented, the engine's block)
  one, _ = make_abi(dtype, rollout_streams=1)
  plan, launches, _ = emu_pacing.wiring(lib, one, 4096, 3000)
  assert plan['slices'] == 1 and launches == [(0, 1, 1)]
  small, _ = make_abi(dtype, steps_per_launch=3, rollout_streams=2)
  plan, launches, _ = emu_pacing.wiring(lib, small, 128, 8)
  assert plan == dict(S=3, launches=3, slices=2, fuse=3, progress_ints=16, paced=1) and launches == [(0, 1, 1), (1, 1, 1)]


def test_an_unfused_plan_gets_none(lib):
  ca, _ = make_abi('float64')
  # the policy switched off (the emulator harnesses of the other kernels, the settle loop): the launches of before, no block
  plan, launches, most = emu_pacing.wiring(lib, ca, 4096, 1000, fuse=0)
  assert plan['fuse'] == 0 and plan['progress_ints'] == 0 and plan['paced'] == 0 and most == 0
  assert len(launches) == 8 and all(l[1:] == (0, 0) for l in launches)
  # a single launch, single steps, physics only: nothing fuses
  for k, geometry, flags in ((20, {}, abi.STEP_ALL), (33, dict(steps_per_launch=1), abi.STEP_ALL), (1000, {}, abi.STEP_PHYSICS)):
    cfg, _ = make_abi('float64', **geometry)
    plan, launches, _ = emu_pacing.wiring(lib, cfg, 4096, k, flags=flags)
    assert plan['fuse'] == 0 and plan['paced'] == 0 and all(l[2] == 0 for l in launches), (k, geometry)


def test_a_rollout_of_several_fused_launches_per_slice_gets_none(lib):
  """17 segments: a launch of 16 and one of 1 (a plain launch) per slice - the second group would count into the first one's counters"""
  ca, _ = make_abi('float64')
  plan, launches, _ = emu_pacing.wiring(lib, ca, 4096, 4250)
  assert plan['fuse'] == 16 and plan['progress_ints'] == 16 and plan['paced'] == 0
  assert [l[1] for l in launches] == [1, 1, 0, 0] and all(l[2] == 0 for l in launches)
  plan, launches, _ = emu_pacing.wiring(lib, ca, 4096, 4000)     # exactly sixteen: one launch per slice
  assert plan['paced'] == 1 and launches == [(0, 1, 1), (1, 1, 1)]


def test_reserve_sees_the_block(lib):
  """for_each_geometry - what solo_engine_reserve walks - visits a plan that needs the block as soon as k reaches two launches, and
  none below"""
  ca, _ = make_abi('float64')
  assert emu_pacing.wiring(lib, ca, 256, 250)[2] == 0
  assert emu_pacing.wiring(lib, ca, 256, 251)[2] == 16
  assert emu_pacing.wiring(lib, ca, 256, 600)[2] == 16
  small, _ = make_abi('float32', steps_per_launch=3)
  assert emu_pacing.wiring(lib, small, 128, 8)[2] == 16 and emu_pacing.wiring(lib, small, 128, 3)[2] == 0
