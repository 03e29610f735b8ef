"""The wave-ops probes (tests/waveops/probe_body.h) on the CPU emulator: tests/emu/wave_emu.h's cross-lane primitives and its
Real<T> under a direct test - moves against numpy indexing, sums of integer-valued data exactly, sums of reals against
math.fsum, the math (libm here) against mpmath at the bars that tests/test_gpu_waveops.py holds the GPU's solo_wave_ops.h to.
The same probe body, inputs, references and checkers run on the GPU there (tests/waveops_cases.py); here they are proven
without one."""
import numpy as np
import pytest

import waveops_cases as wc


@pytest.fixture(scope='module')
def run():
  return wc.host_run(wc.load_emu())


@pytest.mark.parametrize('case', sorted(wc.MATH_CASES))
def test_math_within_its_bar(run, case):
  wc.check(wc.MATH_CASES[case](run))


@pytest.mark.parametrize('dtype', [wc.F32, wc.F64], ids=['f32', 'f64'])
@pytest.mark.parametrize('case', sorted(wc.EXACT_CASES))
def test_exact_semantics(run, case, dtype):
  wc.EXACT_CASES[case](run, dtype)


@pytest.mark.parametrize('dtype', [wc.F32, wc.F64, wc.I32], ids=['f32', 'f64', 'int'])
def test_moves(run, dtype):
  wc.move_readlane(run, dtype)
  wc.move_push(run, dtype)
  if dtype == wc.I32:
    wc.move_ballot(run)
  else:
    wc.move_halves16(run, dtype)
    wc.move_below(run, dtype)
    wc.move_pull(run, dtype)


def test_the_emulator_build_leaves_out_what_it_does_not_have(run):
  lib = wc.load_emu()
  pid = wc.PROBES['lower_half32'][0]
  x = np.zeros(64)
  assert lib.solo_waveops_probe(pid, 1, x.ctypes.data, x.ctypes.data, 1, None) == -1


@pytest.mark.parametrize('dtype', [wc.F32, wc.F64], ids=['f32', 'f64'])
@pytest.mark.parametrize('integer', [True, False], ids=['integers', 'reals'])
def test_sums(run, dtype, integer):
  wc.sum_check(wc.sum_run(run, dtype, integer), dtype, integer)


@pytest.mark.parametrize('dtype', [wc.F32, wc.F64], ids=['f32', 'f64'])
def test_rowdot(run, dtype):
  wc.rowdot_check(run, dtype)
