"""gym_solo_amd/csrc/solo_wave_ops.h - the one layer that only the GPU build contains - under a direct test ON THE GPU: the
straight-line probes of tests/waveops/probe_body.h, built over that header as gym_solo_amd/csrc/libsolo_waveops_probe.so
(SOLO_WAVEOPS_LIB overrides the path), one wave per workgroup.

  * Real<float> / Real<double>: the Cody-Waite sincos, the Goldschmidt sqrt / rsqrt / rcp on the hardware seeds, the even-Taylor
    sinc_cos and its switch, the minimax atan2, the exp2-based exp, the pinned constants - against mpmath, in ulps, at the bars
    of tests/waveops_cases.py (the header's own claims, or derived there); exact semantics against numpy.
  * the DPP / permlane / LDS-crossbar moves against numpy indexing;
  * the cross-lane sums: integer-valued data exactly (a wrong lane, mask or row shows whatever the emulator says), reals within
    64 eps sum|x| of math.fsum AND bit for bit equal to the CPU emulator's restatement (tests/emu/wave_emu.h), on which every
    emulator test rests;
  * RowDot<T>::dot in both forms.
tests/test_emu_waveops.py runs the same probes on the emulator."""
import ctypes as C
import os

import numpy as np
import pytest

import waveops_cases as wc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.environ.get('SOLO_WAVEOPS_LIB') or os.path.join(ROOT, 'gym_solo_amd', 'csrc', 'libsolo_waveops_probe.so')


@pytest.fixture(scope='module')
def torch():
  import torch
  if not torch.cuda.is_available():
    pytest.fail('GPU tests need a visible MI355X')
  return torch


@pytest.fixture(scope='module')
def run(torch):
  assert os.path.isfile(LIB), 'build it: make -C gym_solo_amd/csrc test-libs (or __graft_entry__.build())'
  lib = wc.declare(C.CDLL(LIB))

  def run(name, dtype, ins):
    pid, code, buf, blocks, nout, n0 = wc.pack(name, dtype, ins)
    d_in = torch.from_numpy(buf).cuda()
    d_out = torch.zeros((nout, blocks * 64), dtype=d_in.dtype, device='cuda')
    assert d_in.is_contiguous() and d_in.numel() == buf.size and d_out.is_contiguous()
    rc = lib.solo_waveops_probe(pid, code, d_in.data_ptr(), d_out.data_ptr(), blocks, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, 'solo_waveops_probe(%s) returned HIP status %d' % (name, rc)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()[:, :n0]
  return run


@pytest.fixture(scope='module')
def emu_run():
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
  if dtype != wc.F32:
    wc.move_lower_half32(run, dtype)   # (GPU only: the emulator has no such primitive)


@pytest.mark.parametrize('dtype', [wc.F32, wc.F64], ids=['f32', 'f64'])
def test_sums_of_integers_are_exact(run, dtype):
  wc.sum_check(wc.sum_run(run, dtype, True), dtype, True)


@pytest.mark.parametrize('dtype', [wc.F32, wc.F64], ids=['f32', 'f64'])
def test_sums_of_reals_equal_the_emulator_bit_for_bit(run, emu_run, dtype):
  gpu = wc.sum_run(run, dtype, False)
  wc.sum_check(gpu, dtype, False)
  wc.sum_same_bits(gpu, wc.sum_run(emu_run, dtype, False), dtype)


@pytest.mark.parametrize('dtype', [wc.F32, wc.F64], ids=['f32', 'f64'])
def test_rowdot(run, dtype):
  wc.rowdot_check(run, dtype)
