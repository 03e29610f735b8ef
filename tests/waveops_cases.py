"""Inputs, references, bars and checkers of the wave-ops probes (tests/waveops/probe_body.h), shared by
tests/test_emu_waveops.py (the CPU emulator's wave_emu.h) and tests/test_gpu_waveops.py (the GPU's solo_wave_ops.h).

A `run` is a callable run(name, dtype, [input planes]) -> [nout, n] array: it packs the planes with pack(), calls the
library's solo_waveops_probe and returns the first len(input) elements of every output plane.

MATH.  The reference is mpmath at 160 bits, evaluated at the exact value of the rounded input and kept as a double-double
(hi, lo), so that the error of a float64 result is measured to ~2^-100 relative.  "ulp" is the unit in the last place of
the EXACT reference value in the result's format.  Every bar is the header's claim for the function or is derived from
the formats (issue "Pin the GPU-only wave-ops header"); none is fitted to what the code gives.  MEASURED, next to each bar,
is the worst error seen on the MI355X / on the emulator (libm) at these inputs.

CROSS-LANE.  Moves against numpy indexing; sums on integer-valued data exactly, on reals within 64 eps sum|x| of
math.fsum - and, in the GPU test, bit for bit against the emulator's result for the same input."""
import ctypes as C
import functools
import math
import os
import re
import subprocess
from collections import namedtuple
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, 'tests', 'emu')
BODY = os.path.join(ROOT, 'tests', 'waveops', 'probe_body.h')
F32, F64, I32 = np.float32, np.float64, np.int32
CODE = {F32: 0, F64: 1, I32: 2}
EPS = {F32: 2.0 ** -23, F64: 2.0 ** -52}
FMT = {F32: (24, -126), F64: (53, -1022)}   # (bits of the significand, exponent of the smallest normal)
NPTS = 1 << 13
BLOCKS = 16                                  # of the cross-lane probes


def _parse_probes():
  """SOLO_WAVEOPS_PROBES of probe_body.h: name -> (id, nin, nout, types)"""
  text = open(BODY).read()
  out = {}
  for m in re.finditer(r'X\((\d+),\s*(\w+),\s*(\d+),\s*(\d+),\s*(\d+)\)', text):
    out[m.group(2)] = tuple(int(m.group(i)) for i in (1, 3, 4, 5))
  assert len(out) == 23 and len({v[0] for v in out.values()}) == 23
  return out


PROBES = _parse_probes()


def declare(lib):
  lib.solo_waveops_probe.restype = C.c_int
  lib.solo_waveops_probe.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
  return lib


def load_emu():
  """tests/emu/libsolo_emu_waveops.so (SOLO_EMU_WAVEOPS_LIB overrides the path), built when it is missing or stale"""
  path = os.environ.get('SOLO_EMU_WAVEOPS_LIB')
  if not path:
    path = os.path.join(EMU_DIR, 'libsolo_emu_waveops.so')
    deps = [os.path.join(EMU_DIR, 'emu_waveops_harness.cpp'), os.path.join(EMU_DIR, 'wave_emu.h'), BODY]
    if not os.path.exists(path) or any(os.path.getmtime(d) > os.path.getmtime(path) for d in deps):
      subprocess.check_call(['make', '-s', '-C', EMU_DIR, 'libsolo_emu_waveops.so'])
  return declare(C.CDLL(path))


def pack(name, dtype, ins):
  """-> (probe id, type code, [nin, 64 blocks] input buffer, blocks, nout, n0); a last block is filled with each plane's
  last element (so a sinc_cos block stays on its side of the switch)"""
  pid, nin, nout, types = PROBES[name]
  assert len(ins) == nin and types & (1 << CODE[dtype])
  n0 = len(ins[0])
  blocks = -(-n0 // 64)
  buf = np.empty((nin, blocks * 64), dtype)
  for p, a in enumerate(ins):
    a = np.asarray(a)
    assert a.dtype == dtype and a.shape == (n0,)
    buf[p, :n0] = a
    buf[p, n0:] = a[-1]
  return pid, CODE[dtype], buf, blocks, nout, n0


def host_run(lib):
  def run(name, dtype, ins):
    pid, code, buf, blocks, nout, n0 = pack(name, dtype, ins)
    out = np.zeros((nout, blocks * 64), dtype)
    rc = lib.solo_waveops_probe(pid, code, buf.ctypes.data, out.ctypes.data, blocks, None)
    assert rc == 0, 'solo_waveops_probe(%s) returned %d' % (name, rc)
    return out[:, :n0]
  return run


# ---- references and error measures --------------------------------------------------------------------------------
Measure = namedtuple('Measure', 'label worst bar unit where')


def report(measures):
  for m in measures:
    print('waveops %-34s worst %.4g %s (bar %.4g) at %s' % (m.label, m.worst, m.unit, m.bar, m.where))


def check(measures):
  report(measures)
  bad = [m for m in measures if not m.worst <= m.bar]
  assert not bad, 'over the bar: ' + '; '.join('%s %.4g > %.4g %s at %s' % (m.label, m.worst, m.bar, m.unit, m.where) for m in bad)


def _mp():
  import mpmath
  mpmath.mp.prec = 160
  return mpmath


def dd(values):
  """mpmath numbers -> the double-double (hi, lo)"""
  mp = _mp()
  hi = np.array([float(v) for v in values], F64)
  lo = np.array([float(v - mp.mpf(h)) for v, h in zip(values, hi)], F64)
  return hi, lo


def ref1(fn, x):
  """fn over the exact values of x -> (hi, lo)"""
  mp = _mp()
  return dd([fn(mp.mpf(float(v))) for v in x])


def abs_err(got, ref):
  hi, lo = ref
  return np.abs((got.astype(F64) - hi) - lo)


def ulp_of(ref, dtype):
  """the unit in the last place of the exact value hi + lo in dtype's format"""
  hi, lo = ref
  p, emin = FMT[dtype]
  m, e = np.frexp(np.abs(hi))                                   # |hi| = m 2^e, m in [0.5, 1)
  e = e - ((m == 0.5) & (np.sign(lo) * np.sign(hi) < 0))        # (just below a power of two: the finer binade)
  return np.ldexp(1.0, np.maximum(e, emin + 1) - p)


def m_ulp(label, got, ref, dtype, bar, x, mask=None):
  err = abs_err(got, ref) / ulp_of(ref, dtype)
  if mask is not None:
    err = np.where(mask, err, 0.0)
  assert not np.isnan(err).any(), label
  i = int(np.argmax(err))
  return Measure(label, float(err[i]), bar, 'ulp', repr(x[i]))


def m_abs(label, got, ref, bar, x):
  err = abs_err(got, ref)
  assert not np.isnan(err).any(), label
  i = int(np.argmax(err))
  return Measure(label, float(err[i]), bar, 'abs', repr(x[i]))


def m_ratio(label, err, bars, x):
  """per-point bars: the worst err / bar against 1"""
  r = err / bars
  assert not np.isnan(r).any(), label
  i = int(np.argmax(r))
  return Measure(label, float(r[i]), 1.0, 'of its bar (err %.3g, bar %.3g)' % (err[i], bars[i]), repr(x[i]))


def _rng(seed):
  return np.random.default_rng(seed)


def _signs(r, n):
  return r.choice([-1.0, 1.0], n)


def _name(dtype):
  return 'f32' if dtype == F32 else 'f64'


# ---- sqrt / rsqrt / rcp --------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _roots_in(dtype):
  r = _rng(1)
  x = 10.0 ** r.uniform(-30, 30, NPTS - 512)
  if dtype == F64:
    k = np.concatenate([np.arange(1, 65), r.integers(1, 1 << 26, 190)]).astype(F64)
    x = np.concatenate([x, k * k, [1 + 2.0 ** -52, 1 - 2.0 ** -52]])      # (exact squares; the neighbours of 1)
  x = x.astype(dtype)
  mp = _mp()
  return x, ref1(mp.sqrt, x), ref1(lambda v: 1 / mp.sqrt(v), x), ref1(lambda v: 1 / v, x)


def case_roots(run, dtype):
  """f64 sqrt, rsqrt: 2 ulp (simulated 1.38 / 1.48); f64 rcp: 1 ulp (0.50); f32: 1 ulp each, the header's claim for v_sqrt_f32 /
  v_rsq_f32 / v_rcp_f32.  sqrt(0) == 0.
  MEASURED (MI355X | emulator): f64 sqrt 1.20 | 0.50, rsqrt 1.27 | 1.36, rcp 0.50 | 0.50 ulp; f32 sqrt 0.86 | 0.50, rsqrt 0.78 | 0.50, rcp 0.81 | 0.50 ulp."""
  x, rs, rr, rc = _roots_in(dtype)
  bar = 2.0 if dtype == F64 else 1.0
  s = run('sqrt_rsqrt', dtype, [np.concatenate([x, [0]]).astype(dtype)])
  assert s[0, -1] == 0.0                                                     # (rsq(0) = inf: the product 0 x inf is selected away)
  c = run('rcp', dtype, [np.concatenate([x, -x])])
  n = len(x)
  t = _name(dtype)
  return [m_ulp(t + ' sqrt', s[0, :n], rs, dtype, bar, x), m_ulp(t + ' rsqrt', s[1, :n], rr, dtype, bar, x),
          m_ulp(t + ' rcp', c[0, :n], rc, dtype, 1.0, x), m_ulp(t + ' rcp(-x)', -c[0, n:], rc, dtype, 1.0, x)]


# ---- sincos --------------------------------------------------------------------------------------------------------
def _nearest_multiples(ks):
  mp = _mp()
  return np.array([float(mp.mpf(int(k)) * mp.pi / 2) for k in ks], F64)


def _sincos_ref(x):
  mp = _mp()
  return ref1(mp.sin, x), ref1(mp.cos, x)


@functools.lru_cache(None)
def _sincos_small_in():
  r = _rng(2)
  tiny = [0.0, 5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308, 1e-300, -1e-300, 1e-20, -1e-20]
  x = np.concatenate([r.uniform(-20, 20, NPTS - 64), tiny, _nearest_multiples(range(-13, 14))])
  return (x,) + _sincos_ref(x)


@functools.lru_cache(None)
def _sincos_large_in():
  r = _rng(3)
  x = np.concatenate([r.uniform(-1e5, 1e5, NPTS - 2000), _nearest_multiples(r.integers(-63661, 63662, 2000))])
  assert np.abs(x).max() <= 1e5
  return (x,) + _sincos_ref(x)


@functools.lru_cache(None)
def _sincos_f32_in():
  r = _rng(4)
  x = np.concatenate([r.uniform(-20, 20, NPTS // 2), r.uniform(-1e4, 1e4, NPTS // 2 - 64), [0.0, 1e-30, -1e-30, 1e4, -1e4],
                      _nearest_multiples(range(-13, 14))]).astype(F32)
  assert np.abs(x).max() <= 1e4
  return (x,) + _sincos_ref(x)


def case_sincos_f64_small(run):
  """|x| <= 20, 0, +-tiny and the doubles nearest to k pi/2, |k| <= 13: 2 ulp of the result, the header's claim (simulated 1.36)
  MEASURED (MI355X | emulator): sin 1.28 | 0.51, cos 1.42 | 0.51 ulp."""
  x, rs, rc = _sincos_small_in()
  o = run('sincos', F64, [x])
  return [m_ulp('f64 sin |x|<=20', o[0], rs, F64, 2.0, x), m_ulp('f64 cos |x|<=20', o[1], rc, F64, 2.0, x)]


def case_sincos_f64_large(run):
  """|x| <= 1e5 with the doubles nearest to 2000 random multiples of pi/2: absolute 2^-52 (simulated 1.07e-16; the RELATIVE error
  next to a zero of sin / cos grows with k: the two-piece pi/2 has a 6e-33 tail error)
  MEASURED (MI355X | emulator): sin 1.04e-16 | 5.6e-17, cos 1.08e-16 | 5.6e-17."""
  x, rs, rc = _sincos_large_in()
  o = run('sincos', F64, [x])
  return [m_abs('f64 sin |x|<=1e5', o[0], rs, 2.0 ** -52, x), m_abs('f64 cos |x|<=1e5', o[1], rc, 2.0 ** -52, x)]


def case_sincos_f32(run):
  """|x| <= 1e4 (the header's range): absolute 2^-23 (simulated 8.8e-8); the points with |x| <= 20 and |result| >= 2^-10
  additionally 2 ulp (simulated 1.47).
  The results BELOW 2^-10 at |x| <= 20 (the f32 values nearest to k pi/2, |k| <= 13: next to a zero the result is the reduced
  argument itself) are held to 2 ulp as well.  That is what the third piece of pi/2 is for, and the only place where it shows
  (k 5.4e-15 against results of 1e-8 ... 1e-6): the first fused step of the reduction is exact (x and k P1 are multiples of 2^-23,
  their difference is small), the second and the third round once each, the kernel's last fused step once more - three half ulps.
  MEASURED (MI355X | emulator): absolute sin 8.9e-8 | 3.2e-8, cos 8.6e-8 | 3.2e-8; |x| <= 20: sin 1.32 | 0.56, cos 1.37 | 0.56 ulp;
  next to a zero 0.48 | 0.48 ulp (without the third piece: 18 ulp)."""
  x, rs, rc = _sincos_f32_in()
  o = run('sincos', F32, [x])
  near = np.abs(x) <= 20
  big_s, big_c = np.abs(rs[0]) >= 2.0 ** -10, np.abs(rc[0]) >= 2.0 ** -10
  assert (near & ~big_s).sum() >= 14 and (near & ~big_c).sum() >= 13           # (the multiples of pi/2 are among the inputs)
  return [m_abs('f32 sin |x|<=1e4', o[0], rs, 2.0 ** -23, x), m_abs('f32 cos |x|<=1e4', o[1], rc, 2.0 ** -23, x),
          m_ulp('f32 sin |x|<=20', o[0], rs, F32, 2.0, x, near & big_s), m_ulp('f32 cos |x|<=20', o[1], rc, F32, 2.0, x, near & big_c),
          m_ulp('f32 sin next to a zero', o[0], rs, F32, 2.0, x, near & ~big_s),
          m_ulp('f32 cos next to a zero', o[1], rc, F32, 2.0, x, near & ~big_c)]


# ---- sinc_cos ------------------------------------------------------------------------------------------------------
def library_side(x2):
  """the side of sinc_cos' switch an argument is on, as the header takes it: f32 compares the bits with those of 1/16, f64
  the HIGH WORD with 1/16's - so the doubles in (1/16, 1/16 (1 + 2^-20)) still take the Taylor side"""
  if x2.dtype == F32:
    return x2.view(np.int32) > 0x3d800000
  return (x2.view(np.int64) >> 32) > 0x3fb00000


def _one_side(x2, side):
  """every block of 64 (the last one filled with the last element) lies on one side: the switch is taken from lane 0"""
  assert (library_side(x2) == side).all()
  return x2


def _sinc_ref(x2):
  mp = _mp()
  return (ref1(lambda v: mp.sin(mp.sqrt(v)) / mp.sqrt(v) if v > 0 else mp.mpf(1), x2), ref1(lambda v: mp.cos(mp.sqrt(v)), x2))


@functools.lru_cache(None)
def _sinc_taylor_in(dtype):
  r = _rng(5)
  sixteenth = dtype(1.0 / 16)
  edges = [0.0, 1e-300 if dtype == F64 else 1e-30, sixteenth]
  if dtype == F64:
    edges.append(np.nextafter(sixteenth, 1.0))
  x2 = np.concatenate([r.uniform(0, 1.0 / 16, NPTS - 2048), 10.0 ** r.uniform(-20, -1.3, 2040), edges]).astype(dtype)
  return (_one_side(x2, False),) + _sinc_ref(x2)


@functools.lru_cache(None)
def _sinc_library_in(dtype):
  r = _rng(6)
  if dtype == F64:
    first = np.array([0x3fb0000100000000 + i for i in range(4)], np.int64).view(F64)
  else:
    first = np.array([0x3d800001 + i for i in range(4)], np.int32).view(F32)
  x2 = np.concatenate([first.astype(F64), r.uniform(1.0 / 16 + 1e-6, 100, NPTS - 64), [100.0]]).astype(dtype)
  return (_one_side(x2, True),) + _sinc_ref(x2)


def case_sinc_taylor(run, dtype):
  """x2 in [0, 1/16] with 0, 1e-300 and exactly 1/16.  f64: 1 ulp each (simulated 0.51).  f32: 2 ulp (the header: truncation
  5e-11 / 3e-9, the rest is the round-off of four / five fused steps)
  MEASURED (MI355X | emulator): f64 sinc 0.51 | 0.50, cos 0.51 | 0.52 ulp; f32 sinc 0.51 | 1.40, cos 0.51 | 0.52 ulp."""
  x2, rs, rc = _sinc_taylor_in(dtype)
  o = run('sinc_cos', dtype, [x2])
  bar = 1.0 if dtype == F64 else 2.0
  t = _name(dtype)
  return [m_ulp(t + ' sinc Taylor', o[0], rs, dtype, bar, x2), m_ulp(t + ' cos Taylor', o[1], rc, dtype, bar, x2)]


def case_sinc_library(run, dtype):
  """x2 in (1/16, 100] from the first values above the switch.  The bar is DERIVED from the bars of the parts, with
  eps = 2^-52 / 2^-23, x = sqrt(x2), B_sqrt = 2 / 1 ulp, B_rcp = 1 ulp, A = sincos' absolute bar 2^-52 / 2^-23:
    the argument's error   dx  = B_sqrt eps x                (an ulp of x is at most eps x)
    cos:                   dx + A                            (slope of cos <= 1)
    sinc = sin(x) rcp(x):  (dx + A) / x + |sinc| (B_rcp + 1) eps     (rcp's bar, and the product's own rounding)
  MEASURED (MI355X | emulator): as a fraction of the bar: f64 sinc 0.41 | 0.20, cos 0.40 | 0.22; f32 sinc 0.53 | 0.38, cos 0.62 | 0.43."""
  x2, rs, rc = _sinc_library_in(dtype)
  o = run('sinc_cos', dtype, [x2])
  eps = EPS[dtype]
  x = np.sqrt(x2.astype(F64))
  dx = (2.0 if dtype == F64 else 1.0) * eps * x
  t = _name(dtype)
  return [m_ratio(t + ' sinc library', abs_err(o[0], rs), (dx + eps) / x + np.abs(rs[0]) * 2.0 * eps, x2),
          m_ratio(t + ' cos library', abs_err(o[1], rc), dx + eps, x2)]


# ---- atan2 / asin / exp --------------------------------------------------------------------------------------------
def _atan2_ref(y, x):
  mp = _mp()
  vals = []
  for a, b in zip(y, x):
    a, b = float(a), float(b)
    if a == 0.0:   # (mpmath has no signed zero)
      v = mp.mpf(0) if (b > 0 or b == 0) else mp.pi
      vals.append(-v if math.copysign(1.0, a) < 0 else v)
    else:
      vals.append(mp.atan2(mp.mpf(a), mp.mpf(b)))
  return dd(vals)


@functools.lru_cache(None)
def _atan2_in(dtype):
  r = _rng(7)
  n = NPTS - 64
  th, rad = r.uniform(-np.pi, np.pi, n), 10.0 ** r.uniform(-3, 3, n)
  y, x = list(rad * np.sin(th)), list(rad * np.cos(th))
  for q in (1e-3, 1.0, 1e3):
    for sy, sx in ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1)):   # (both axes, the four diagonals)
      y.append(sy * q); x.append(sx * q)
  y += [0.0, 0.0, -0.0]; x += [0.0, -1.0, -1.0]
  y, x = np.array(y).astype(dtype), np.array(x).astype(dtype)
  return y, x, _atan2_ref(y, x)


def _angle_bar_f32(ref):
  """the f32 atan2's bar: the polynomial's 1.5e-7 rad plus one f32 ulp of |reference| (the octant fix-ups round once more)"""
  return 1.5e-7 + ulp_of(ref, F32)


def case_atan2(run, dtype):
  """angles over the full circle at radii 1e-3 ... 1e3, both axes, the diagonals, (0, 0), (+-0, -1).  f32: 1.5e-7 + one f32 ulp
  of |reference| (simulated: 0.73 of that; v_rcp_f32 adds about 3e-8).  f64 (a library call): 4 ulp.
  MEASURED (MI355X | emulator): f32 0.75 | 0.61 of the bar (2.93e-7 rad near -pi on the MI355X); f64 1.43 | 0.50 ulp."""
  y, x, ref = _atan2_in(dtype)
  o = run('atan2', dtype, [y, x])[0]
  assert o[-3] == 0.0 and o[-2] > 3.14 and o[-1] < -3.14                    # ((0, 0) -> 0; (+-0, -1) -> +-pi)
  pts = list(zip(y, x))
  if dtype == F32:
    return [m_ratio('f32 atan2', abs_err(o, ref), _angle_bar_f32(ref), pts)]
  return [m_ulp('f64 atan2', o, ref, F64, 4.0, pts)]


@functools.lru_cache(None)
def _asin_in(dtype):
  r = _rng(8)
  lim = dtype(0.99999)
  while abs(float(lim)) > 0.99999:
    lim = np.nextafter(lim, dtype(0))
  x = list(r.uniform(-0.99999, 0.99999, NPTS - 128).astype(dtype)) + [lim, -lim, dtype(0), dtype(1e-20), dtype(-1e-20)]
  if dtype == F64:
    for k in range(10, 53):   # (cos_of_asin is written to survive this cancellation)
      x += [1 - 2.0 ** -k, -(1 - 2.0 ** -k)]
  x = np.array(x, dtype)
  x = x[np.abs(x.astype(F64)) <= (1.0 if dtype == F64 else 0.99999)]
  mp = _mp()
  return x, ref1(mp.asin, x), ref1(lambda v: mp.sqrt((1 - v) * (1 + v)), x)


def case_asin(run, dtype):
  """|x| <= 0.99999 (all that euler_component passes); f64 also 1 - 2^-k, k = 10 ... 52.  f32: asin as atan2, cos_of_asin 2 ulp.
  f64: 4 ulp both.  |x| = 1 gives exactly +-half_pi() and 0.
  MEASURED (MI355X | emulator): f32 asin 0.82 | 0.33 of the bar, cos_of_asin 1.10 | 0.81 ulp; f64 asin 2.52 | 0.50, cos_of_asin 1.77 | 1.16 ulp."""
  x, ra, rc = _asin_in(dtype)
  o = run('asin', dtype, [np.concatenate([x, [1, -1]]).astype(dtype)])
  half_pi = dtype(np.pi / 2)
  assert o[0, -2] == half_pi and o[0, -1] == -half_pi and o[1, -2] == 0 and o[1, -1] == 0
  a, c = o[0, :-2], o[1, :-2]
  if dtype == F32:
    return [m_ratio('f32 asin', abs_err(a, ra), _angle_bar_f32(ra), x), m_ulp('f32 cos_of_asin', c, rc, F32, 2.0, x)]
  return [m_ulp('f64 asin', a, ra, F64, 4.0, x), m_ulp('f64 cos_of_asin', c, rc, F64, 4.0, x)]


@functools.lru_cache(None)
def _exp_in(dtype):
  x = np.concatenate([_rng(9).uniform(-90, 0, NPTS - 64), [0.0, -90.0, -1e-10, -1.0]]).astype(dtype)
  return x, ref1(_mp().exp, x)


def case_exp(run, dtype):
  """x in [-90, 0] (the gaussian tolerance's range).  f32: relative 2^-23 (1 + |x|) - the rounding of the argument's scaling,
  |x| 2^-24 twice, plus 1 ulp of v_exp_f32.  f64 (a library call): 4 ulp.
  MEASURED (MI355X | emulator): f32 0.59 | 0.27 of the bar; f64 0.76 | 0.50 ulp.  (Before Real<float>::exp handled denormal results the MI355X gave 0
  for x < -87.34: 9.5e4 times the bar.)"""
  x, ref = _exp_in(dtype)
  o = run('exp', dtype, [x])[0]
  if dtype == F32:
    return [m_ratio('f32 exp', abs_err(o, ref), np.abs(ref[0]) * 2.0 ** -23 * (1 + np.abs(x.astype(F64))), x)]
  return [m_ulp('f64 exp', o, ref, F64, 4.0, x)]


# ---- exact semantics ---------------------------------------------------------------------------------------------
def case_exact(run, dtype):
  """clamp, min, max, abs, floor on finite inputs with lo <= hi equal numpy AS VALUES: lo == hi, +-0, the largest finite values,
  x far outside the bounds"""
  r = _rng(10)
  big = float(np.finfo(dtype).max)
  n = 1024
  a, b = r.normal(0, 10, n), r.normal(0, 10, n)
  lo, hi = np.minimum(a, b), np.maximum(a, b)
  x = r.normal(0, 20, n)
  x[:64] *= 1e20                                                             # (far outside)
  hi[64:128] = lo[64:128]                                                    # (lo == hi)
  x[128:160] = lo[128:160]; x[160:192] = hi[160:192]                         # (on a bound)
  sp = [(0.0, -0.0, 0.0), (-0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (-0.0, -1.0, 1.0), (big, -big, big), (-big, -big, big), (big, -1.0, 1.0),
        (-big, -1.0, 1.0), (1.0, -big, -big), (1.0, big, big), (0.5, -big, big), (-2.5, -big, 0.0), (2.5, 0.0, big), (-0.5, -1.0, 0.0)]
  x = np.concatenate([x, [s[0] for s in sp]]).astype(dtype)
  lo = np.concatenate([lo, [s[1] for s in sp]]).astype(dtype)
  hi = np.concatenate([hi, [s[2] for s in sp]]).astype(dtype)
  assert (lo <= hi).all()
  o = run('exact', dtype, [x, lo, hi])
  for got, want, what in zip(o, (np.clip(x, lo, hi), np.minimum(x, lo), np.maximum(x, lo), np.abs(x), np.floor(x)),
                             ('clamp', 'min', 'max', 'abs', 'floor')):
    assert np.array_equal(got, want), what
  assert not np.signbit(o[3]).any()


def _round_fraction(v, dtype):
  """the exact rational v rounded to dtype (nearest; no ties among these inputs)"""
  f = dtype(float(v))
  cands = [np.nextafter(f, dtype(-np.inf)), f, np.nextafter(f, dtype(np.inf))]
  return min(cands, key=lambda c: abs(Fraction(float(c)) - v))


def case_fma(run, dtype):
  """ONE rounding: random operands, and c = -round(a b), where the result is the product's rounding error itself"""
  r = _rng(11)
  n = 512
  a = (_signs(r, n) * 10.0 ** r.uniform(-3, 3, n)).astype(dtype)
  b = (_signs(r, n) * 10.0 ** r.uniform(-3, 3, n)).astype(dtype)
  c = (_signs(r, n) * 10.0 ** r.uniform(-3, 3, n)).astype(dtype)
  c[: n // 2] = -(a[: n // 2] * b[: n // 2])
  want = np.array([_round_fraction(Fraction(float(p)) * Fraction(float(q)) + Fraction(float(s)), dtype) for p, q, s in zip(a, b, c)], dtype)
  assert (want[: n // 2] != 0).sum() > n // 4                               # (an unfused a b + c gives 0 there)
  assert np.array_equal(run('fma', dtype, [a, b, c])[0], want)


def case_floor_int(run, dtype):
  """(int)floor(x) over the grid coordinates of the terrain lookup (clamped to [0, nx - 1] before the conversion): the integers,
  their neighbours, random points"""
  k = np.arange(0, 4097, dtype=F64)
  x = np.concatenate([k, np.nextafter(k.astype(dtype), dtype(-1)).astype(F64)[1:], np.nextafter(k.astype(dtype), dtype(1e9)).astype(F64),
                      _rng(12).uniform(0, 4096, 1024), [-0.0]]).astype(dtype)
  got = run('floor_int', dtype, [x])[0]
  assert np.array_equal(got, np.floor(x)) and got.min() == 0 and got.max() == 4096


def case_finite(run, dtype):
  """false for NaN and +-inf, true for 0, denormals and +-max: what the diverged-robot guard depends on"""
  fi = np.finfo(dtype)
  x = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, fi.smallest_subnormal, -fi.smallest_subnormal,
                np.nextafter(fi.tiny, dtype(0)), fi.tiny, fi.max, -fi.max, 1.0, -1.0], dtype)
  bits = np.dtype(dtype).itemsize * 8
  u = {32: np.uint32, 64: np.uint64}[bits]
  nans = np.array([0x7fc00001, 0xffc00000, 0x7f800001] if bits == 32 else [0x7ff8000000000001, 0xfff8000000000000, 0x7ff0000000000001], u).view(dtype)
  x = np.concatenate([x, nans])
  want = np.array([0, 0, 0, 0] + [1] * 10 + [0, 0, 0], dtype)
  assert np.array_equal(run('finite', dtype, [x])[0], want)


def case_constants(run, dtype):
  """big(), half_pi() and half_ulp() bit for bit: 1e300 / 3e38, pi/2 rounded to T, 2^-53 / 2^-24 (the f64 ones are built from
  two pinned 32-bit halves)"""
  o = run('constants', dtype, [np.zeros(64, dtype)])
  want = [dtype(1e300 if dtype == F64 else 3e38), dtype(np.pi / 2), dtype(2.0 ** (-53 if dtype == F64 else -24))]
  u = np.uint64 if dtype == F64 else np.uint32
  for got, w, what in zip(o, want, ('big', 'half_pi', 'half_ulp')):
    assert (got.view(u) == np.array([w], dtype).view(u)[0]).all(), what


MATH_CASES = {
    'roots-f64': lambda run: case_roots(run, F64), 'roots-f32': lambda run: case_roots(run, F32),
    'sincos-f64-small': case_sincos_f64_small, 'sincos-f64-large': case_sincos_f64_large, 'sincos-f32': case_sincos_f32,
    'sinc-taylor-f64': lambda run: case_sinc_taylor(run, F64), 'sinc-taylor-f32': lambda run: case_sinc_taylor(run, F32),
    'sinc-library-f64': lambda run: case_sinc_library(run, F64), 'sinc-library-f32': lambda run: case_sinc_library(run, F32),
    'atan2-f64': lambda run: case_atan2(run, F64), 'atan2-f32': lambda run: case_atan2(run, F32),
    'asin-f64': lambda run: case_asin(run, F64), 'asin-f32': lambda run: case_asin(run, F32),
    'exp-f64': lambda run: case_exp(run, F64), 'exp-f32': lambda run: case_exp(run, F32),
}
EXACT_CASES = {'exact': case_exact, 'fma': case_fma, 'floor_int': case_floor_int, 'finite': case_finite, 'constants': case_constants}


# ---- moves ---------------------------------------------------------------------------------------------------------
N = BLOCKS * 64
LANE = np.tile(np.arange(64), BLOCKS)


def _data(dtype, seed):
  r = _rng(seed)
  if dtype == I32:
    return r.integers(-2 ** 31, 2 ** 31, N).astype(I32)
  return (_signs(r, N) * 10.0 ** r.uniform(-8, 8, N)).astype(dtype)


def _bits(a):
  return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, want, what):
  assert np.array_equal(_bits(np.ascontiguousarray(got)), _bits(np.ascontiguousarray(want))), what


def _gather(x, src):
  """lane l of every block gets its block's lane src[l] (src: [N] lanes)"""
  return x.reshape(BLOCKS, 64)[np.arange(N) // 64, src]


def move_readlane(run, dtype):
  x = _data(dtype, 20)
  o = run('readlane', dtype, [x])
  for j in range(64):
    _same(o[j], _gather(x, np.full(N, j)), 'lane %d' % j)


def move_halves16(run, dtype):
  x = _data(dtype, 21)
  o = run('halves16', dtype, [x])
  _same(o[0], _gather(x, LANE ^ 8), 'wave_other_half16')
  _same(o[1], _gather(x, LANE | 8), 'wave_from_lower_half16 (the lanes 8..15 of the row)')
  _same(o[2], _gather(x, LANE & ~8), 'wave_from_upper_half16 (the lanes 0..7 of the row)')


def move_below(run, dtype):
  x = _data(dtype, 22)
  o = run('below', dtype, [x])
  for k, (n, row) in enumerate(((1, True), (2, True), (1, False), (2, False))):
    has = ((LANE & 15) if row else LANE) >= n
    want = np.where(has, _gather(x, np.maximum(LANE - n, 0)), dtype(0))      # (lanes without a source read 0)
    _same(o[k], want, ('wave_lane_below<%d>' if row else 'wave_slot_below<%d>') % n)


def move_lower_half32(run, dtype):
  x = _data(dtype, 23)
  _same(run('lower_half32', dtype, [x])[0], _gather(x, LANE & 31), 'wave_from_lower_half32')


def _perms(seed):
  r = _rng(seed)
  p = np.concatenate([r.permutation(64) for _ in range(BLOCKS)])
  p[:64] = np.arange(64)            # (the identity, a reversal and a rotation among the random ones)
  p[64:128] = 63 - np.arange(64)
  p[128:192] = (np.arange(64) + 17) % 64
  return p


def move_push(run, dtype):
  x, dst = _data(dtype, 24), _perms(25)
  want = np.empty_like(x)
  want.reshape(BLOCKS, 64)[np.arange(N) // 64, dst] = x
  _same(run('push', dtype, [x, dst.astype(dtype)])[0], want, 'wave_push')


def move_pull(run, dtype):
  x = _data(dtype, 26)
  src = _perms(27)
  _same(run('pull', dtype, [x, src.astype(dtype)])[0], _gather(x, src), 'wave_pull (permutations)')
  rep = _rng(28).integers(0, 64, N)                                         # (repeated sources; one block all from one lane)
  rep[:64] = 41
  _same(run('pull', dtype, [x, rep.astype(dtype)])[0], _gather(x, rep), 'wave_pull (repeated sources)')


def move_ballot(run):
  r = _rng(29)
  p = (r.random((BLOCKS, 64)) < 0.5).astype(I32)
  p[0] = 0
  p[1] = 1
  for b, lane in ((2, 0), (3, 31), (4, 32), (5, 63)):
    p[b] = 0
    p[b, lane] = 1
  p[6] = (r.random(64) < 0.05)
  p[7] = (r.random(64) < 0.95)
  p[8] *= 77                                                                 # (any non-zero value is true)
  o = run('ballot', I32, [p.reshape(-1)]).reshape(4, BLOCKS, 64)
  set_ = p != 0
  mask = (set_.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
  assert np.array_equal(o[0].view(np.uint32), np.repeat((mask & np.uint64(0xffffffff)).astype(np.uint32)[:, None], 64, 1)), 'wave_ballot (low word)'
  assert np.array_equal(o[1].view(np.uint32), np.repeat((mask >> np.uint64(32)).astype(np.uint32)[:, None], 64, 1)), 'wave_ballot (high word)'
  assert np.array_equal(o[2], np.cumsum(set_, axis=1) - set_), 'wave_count_below'
  assert np.array_equal(o[3], np.tile(np.arange(64), (BLOCKS, 1))), 'wave_fresh_lane'


# ---- sums ----------------------------------------------------------------------------------------------------------
SUM_PROBES = ('sum_basic', 'reduce_rows', 'reduce_rows_lds')


def sum_inputs(dtype, integer):
  r = _rng(30 if integer else 31)
  if integer:
    return [r.integers(-1024, 1025, N).astype(dtype) for _ in range(8)]
  return [(_signs(r, N) * 10.0 ** r.uniform(-8, 8, N)).astype(dtype) for _ in range(8)]


def sum_run(run, dtype, integer):
  """-> {probe: outputs} for the sum probes that exist in dtype"""
  ins = sum_inputs(dtype, integer)
  out = {'sum_basic': run('sum_basic', dtype, ins[:1]), 'reduce_rows': run('reduce_rows', dtype, ins)}
  if dtype == F64:
    out['reduce_rows_lds'] = run('reduce_rows_lds', dtype, ins)
  return out


def _members(kind):
  """[64, k] lanes that a lane's sum runs over"""
  lane = np.arange(64)
  if kind == 'legs':
    return np.stack([lane ^ m for m in (0, 16, 32, 48)], 1)
  if kind == 'row':
    return (lane & 48)[:, None] + np.arange(16)[None, :]
  return np.tile(np.arange(64), (64, 1))


def _check_sum(got, x, kind, dtype, integer, what):
  xb = x.reshape(BLOCKS, 64).astype(F64)
  terms = xb[:, _members(kind)]                                              # [blocks, 64, k]
  got = got.reshape(BLOCKS, 64).astype(F64)
  if integer:
    assert np.array_equal(got, terms.sum(axis=2)), what                     # (|v| <= 1024: every association is exact)
    return 0.0
  want = np.array([[math.fsum(t) for t in blk] for blk in terms])
  bound = 64 * EPS[dtype] * np.abs(terms).sum(axis=2)
  assert (np.abs(got - want) <= bound).all(), what
  if kind == 'all':   # (a wave-uniform result: the same bits in every lane)
    assert (got == got[:, :1]).all(), what + ': not uniform'
  return float((np.abs(got - want) / bound).max())


def sum_check(outs, dtype, integer):
  """every lane of every output against the sum over its members (exact for integers; within 64 eps sum|x| of fsum otherwise)"""
  ins = sum_inputs(dtype, integer)
  t = _name(dtype)
  o = outs['sum_basic']
  for k, kind in enumerate(('legs', 'row', 'all')):
    _check_sum(o[k], ins[0], kind, dtype, integer, '%s wave_sum_%s' % (t, ('legs', 'group16', 'all')[k]))
  for probe in SUM_PROBES[1:]:
    if probe in outs:
      for i in range(8):
        _check_sum(outs[probe][i], ins[i], 'all' if i < 6 else 'row', dtype, integer, '%s wave_%s %s[%d]' % (t, probe, 'zy'[i >= 6], i % 6))


def sum_same_bits(a, b, dtype):
  """two builds' results for the same real input, bit for bit"""
  assert a.keys() == b.keys()
  for probe in a:
    for k in range(a[probe].shape[0]):
      _same(a[probe][k], b[probe][k], '%s %s output %d: the two builds associate differently' % (_name(dtype), probe, k))


# ---- RowDot --------------------------------------------------------------------------------------------------------
def rowdot_check(run, dtype):
  """both forms of RowDot<T>::dot within 8 eps sum|terms| of the exact dot product; with same = 1 the three-argument form (f64)
  equals the two-argument form bit for bit"""
  mp = _mp()
  r = _rng(32)
  v = [(r.normal(0, 1, N) * 10.0 ** r.uniform(-2, 2, N)).astype(dtype) for _ in range(16)]
  same = (r.random(N) < 0.5).astype(dtype)
  o = run('rowdot', dtype, v + [same])
  prod = np.array([[mp.mpf(float(v[i][k])) * mp.mpf(float(v[8 + i][k])) for i in range(8)] for k in range(N)], dtype=object)
  mag = np.array([[abs(float(p)) for p in row] for row in prod])
  eps = EPS[dtype]
  full = np.array([float(mp.fsum(row)) for row in prod])
  assert (np.abs(o[0].astype(F64) - full) <= 8 * eps * mag.sum(axis=1)).all(), 'dot(rg, rh)'
  if dtype == F64:
    part = np.array([float(mp.fsum(row[:6]) + (mp.fsum(row[6:]) if s else 0)) for row, s in zip(prod, same)])
    assert (np.abs(o[1] - part) <= 8 * eps * (mag[:, :6].sum(axis=1) + same * mag[:, 6:].sum(axis=1))).all(), 'dot(rg, rh, same)'
    on = same == 1
    assert on.sum() > N // 4 and (~on).sum() > N // 4
    _same(o[1][on], o[0][on], 'dot(rg, rh, 1) != dot(rg, rh)')
