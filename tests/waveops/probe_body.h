// probe_body.h — TEST-ONLY straight-line probes of the wave-ops layer, written ONCE for two builds:
//   tests/waveops/waveops_probe.hip     includes gym_solo_amd/csrc/solo_wave_ops.h (the GPU's definitions),
//   tests/emu/emu_waveops_harness.cpp   includes tests/emu/wave_emu.h (the CPU emulator's restatement).
// Only names that both headers provide are used, the way the kernels themselves are written.  One workgroup is one
// 64-lane wave; a probe reads element block_id() * 64 + lane_id() of each of its `nin` input planes (plane p starts at
// in + p * n, n = 64 * blocks) and writes the same element of each of its `nout` output planes.  No loops over data, no
// waiting on anybody.  Integer arguments (lanes, predicates) travel as values of T.
//
// SOLO_WAVEOPS_PROBES is the list: X(id, name, nin, nout, types) - types: 1 float, 2 double, 4 int.  tests/waveops_cases.py
// reads the ids, the plane counts and the types from THIS list, so the buffers it allocates are the ones the probes index.
#pragma once

// (primitives the emulator does not have are compiled out of its build and checked against numpy alone)
#ifdef SOLO_WAVEOPS_EMU
#define SOLO_WAVEOPS_PROBES_GPU_ONLY(X)
#else
#define SOLO_WAVEOPS_PROBES_GPU_ONLY(X) X(16, lower_half32, 1, 1, 6)
#endif
#define SOLO_WAVEOPS_PROBES(X) \
  X(1, sqrt_rsqrt, 1, 2, 3)    \
  X(2, rcp, 1, 1, 3)           \
  X(3, sincos, 1, 2, 3)        \
  X(4, sinc_cos, 1, 2, 3)      \
  X(5, atan2, 2, 1, 3)         \
  X(6, asin, 1, 2, 3)          \
  X(7, exp, 1, 1, 3)           \
  X(8, exact, 3, 5, 3)         \
  X(9, fma, 3, 1, 3)           \
  X(10, floor_int, 1, 1, 3)    \
  X(11, finite, 1, 1, 3)       \
  X(12, constants, 1, 3, 3)    \
  X(13, readlane, 1, 64, 7)    \
  X(14, halves16, 1, 3, 3)     \
  X(15, below, 1, 4, 3)        \
  SOLO_WAVEOPS_PROBES_GPU_ONLY(X) \
  X(17, push, 2, 1, 7)         \
  X(18, pull, 2, 1, 3)         \
  X(19, ballot, 1, 4, 4)       \
  X(20, sum_basic, 1, 3, 3)    \
  X(21, reduce_rows, 8, 8, 3)  \
  X(22, reduce_rows_lds, 8, 8, 2) \
  X(23, rowdot, 17, 2, 3)

namespace solo {

#define SOLO_PROBE_ARGS const T* __restrict__ in, T* __restrict__ out, int n
#define SOLO_PROBE_IDX const int idx = block_id() * 64 + lane_id()

// the f64 polynomial coefficients, staged into LDS as solo_step_body.h stages them (the emulator has no table)
template <typename T> __device__ __forceinline__ const T* probe_math_table() {
  __shared__ T s_math[Real<T>::kTabSize > 0 ? Real<T>::kTabSize : 1];
  if constexpr (Real<T>::kTabSize > 0) {
    const int lane0 = lane_id();
    const T math_w = wave_math_table<T>(lane0 < Real<T>::kTabSize ? lane0 : 0);
    if (lane0 < Real<T>::kTabSize) s_math[lane0] = math_w;
    wave_sync();
  }
  return s_math;
}

// ---- Real<T> ---------------------------------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ void probe_sqrt_rsqrt(SOLO_PROBE_ARGS) {
  SOLO_PROBE_IDX;
  const T x = in[idx];
  out[idx] = Real<T>::sqrt(x);
  out[n + idx] = Real<T>::rsqrt(x);
}
template <typename T> __device__ __forceinline__ void probe_rcp(SOLO_PROBE_ARGS) {
  SOLO_PROBE_IDX;
  out[idx] = Real<T>::rcp(in[idx]);
}
template <typename T> __device__ __forceinline__ void probe_sincos(SOLO_PROBE_ARGS) {
  SOLO_PROBE_IDX;
  const T* tab = probe_math_table<T>();
  T s, c;
  Real<T>::sincos(in[idx], &s, &c, tab);
  out[idx] = s;
  out[n + idx] = c;
}
// (the switch inside sinc_cos is taken from lane 0: the caller keeps a block's 64 arguments on one side of it)
template <typename T> __device__ __forceinline__ void probe_sinc_cos(SOLO_PROBE_ARGS) {
  SOLO_PROBE_IDX;
  const T* tab = probe_math_table<T>();
  T s, c;
  Real<T>::sinc_cos(in[idx], &s, &c, tab);
  out[idx] = s;
  out[n + idx] = c;
}
template <typename T> __device__ __forceinline__ void probe_atan2(SOLO_PROBE_ARGS) {
  SOLO_PROBE_IDX;
  out[idx] = Real<T>::atan2(in[idx], in[n + idx]);
}
template <typename T> __device__ __forceinline__ void probe_asin(SOLO_PROBE_ARGS) {
  SOLO_PROBE_IDX;
  const T x = in[idx];
  out[idx] = Real<T>::asin(x);
  out[n + idx] = Real<T>::cos_of_asin(x);
}
template <typename T> __device__ __forceinline__ void probe_exp(SOLO_PROBE_ARGS) {
  SOLO_PROBE_IDX;
  out[idx] = Real<T>::exp(in[idx]);
}
// in: x, lo, hi -> clamp(x, lo, hi), min(x, lo), max(x, lo), abs(x), floor(x)
template <typename T> __device__ __forceinline__ void probe_exact(SOLO_PROBE_ARGS) {
  SOLO_PROBE_IDX;
  const T x = in[idx], lo = in[n + idx], hi = in[2 * n + idx];
  out[idx] = Real<T>::clamp(x, lo, hi);
  out[n + idx] = Real<T>::min(x, lo);
  out[2 * n + idx] = Real<T>::max(x, lo);
  out[3 * n + idx] = Real<T>::abs(x);
  out[4 * n + idx] = Real<T>::floor(x);
}
template <typename T> __device__ __forceinline__ void probe_fma(SOLO_PROBE_ARGS) {
  SOLO_PROBE_IDX;
  out[idx] = Real<T>::fma(in[idx], in[n + idx], in[2 * n + idx]);
}
// the terrain lookup's cell index: floor, then the int conversion (solo_step_kernel.h)
template <typename T> __device__ __forceinline__ void probe_floor_int(SOLO_PROBE_ARGS) {
  SOLO_PROBE_IDX;
  const int gi = (int)Real<T>::floor(in[idx]);
  out[idx] = T(gi);
}
template <typename T> __device__ __forceinline__ void probe_finite(SOLO_PROBE_ARGS) {
  SOLO_PROBE_IDX;
  out[idx] = Real<T>::finite(in[idx]) ? T(1) : T(0);
}
template <typename T> __device__ __forceinline__ void probe_constants(SOLO_PROBE_ARGS) {
  SOLO_PROBE_IDX;
  out[idx] = Real<T>::big();
  out[n + idx] = Real<T>::half_pi();
  out[2 * n + idx] = Real<T>::half_ulp();
}

// ---- moves -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int probe_readlane_any(int x, int lane) { return wave_readlane_int(x, lane); }
__device__ __forceinline__ float probe_readlane_any(float x, int lane) { return wave_readlane(x, lane); }
__device__ __forceinline__ double probe_readlane_any(double x, int lane) { return wave_readlane(x, lane); }
__device__ __forceinline__ int probe_push_any(int x, int dst) { return wave_push_int(x, dst); }
__device__ __forceinline__ float probe_push_any(float x, int dst) { return wave_push(x, dst); }
__device__ __forceinline__ double probe_push_any(double x, int dst) { return wave_push(x, dst); }

// plane j: the value of lane j in every lane, j a constant after unrolling
template <typename T> __device__ __forceinline__ void probe_readlane(SOLO_PROBE_ARGS) {
  SOLO_PROBE_IDX;
  const T x = in[idx];
#pragma unroll
  for (int j = 0; j < 64; ++j) out[j * n + idx] = probe_readlane_any(x, j);
}
template <typename T> __device__ __forceinline__ void probe_halves16(SOLO_PROBE_ARGS) {
  SOLO_PROBE_IDX;
  const T x = in[idx];
  out[idx] = wave_other_half16(x);
  out[n + idx] = wave_from_lower_half16(x);
  out[2 * n + idx] = wave_from_upper_half16(x);
}
template <typename T> __device__ __forceinline__ void probe_below(SOLO_PROBE_ARGS) {
  SOLO_PROBE_IDX;
  const T x = in[idx];
  out[idx] = wave_lane_below<1>(x);
  out[n + idx] = wave_lane_below<2>(x);
  out[2 * n + idx] = wave_slot_below<1>(x);
  out[3 * n + idx] = wave_slot_below<2>(x);
}
#ifndef SOLO_WAVEOPS_EMU   // (the emulator has no wave_from_lower_half32: the column build that uses it is GPU-only)
template <typename T> __device__ __forceinline__ void probe_lower_half32(SOLO_PROBE_ARGS) {
  SOLO_PROBE_IDX;
  out[idx] = wave_from_lower_half32(in[idx]);
}
#endif
// in: x, dst (a permutation of the lanes)
template <typename T> __device__ __forceinline__ void probe_push(SOLO_PROBE_ARGS) {
  SOLO_PROBE_IDX;
  out[idx] = probe_push_any(in[idx], (int)in[n + idx] & 63);
}
// in: x, src (any lanes, repeats allowed)
template <typename T> __device__ __forceinline__ void probe_pull(SOLO_PROBE_ARGS) {
  SOLO_PROBE_IDX;
  out[idx] = wave_pull(in[idx], (int)in[n + idx] & 63);
}
// in: predicate -> the ballot's low and high words, the set bits below this lane, the lane number from v_mbcnt
template <typename T> __device__ __forceinline__ void probe_ballot(SOLO_PROBE_ARGS) {
  SOLO_PROBE_IDX;
  const unsigned long long m = wave_ballot(in[idx] != T(0));
  out[idx] = (T)(unsigned)(m & 0xffffffffull);
  out[n + idx] = (T)(unsigned)(m >> 32);
  out[2 * n + idx] = (T)wave_count_below(m);
  out[3 * n + idx] = (T)wave_fresh_lane();
}

// ---- sums ------------------------------------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ void probe_sum_basic(SOLO_PROBE_ARGS) {
  SOLO_PROBE_IDX;
  const T x = in[idx];
  out[idx] = wave_sum_legs(x);
  out[n + idx] = wave_sum_group16(x);
  out[2 * n + idx] = wave_sum_all(x);
}
// in: z0..z5, y0, y1 -> the same order (z wave-uniform, y per 16-lane row)
template <typename T> __device__ __forceinline__ void probe_reduce_rows(SOLO_PROBE_ARGS) {
  SOLO_PROBE_IDX;
  T z[6], y[2];
#pragma unroll
  for (int i = 0; i < 6; ++i) z[i] = in[i * n + idx];
  y[0] = in[6 * n + idx]; y[1] = in[7 * n + idx];
  wave_reduce_rows(z, y);
#pragma unroll
  for (int i = 0; i < 6; ++i) out[i * n + idx] = z[i];
  out[6 * n + idx] = y[0]; out[7 * n + idx] = y[1];
}
template <typename T> __device__ __forceinline__ void probe_reduce_rows_lds(SOLO_PROBE_ARGS) {
  SOLO_PROBE_IDX;
  __shared__ T s_scratch[kReduceScratch];
  T z[6], y[2];
#pragma unroll
  for (int i = 0; i < 6; ++i) z[i] = in[i * n + idx];
  y[0] = in[6 * n + idx]; y[1] = in[7 * n + idx];
  wave_reduce_rows_lds(z, y, s_scratch, lane_id());
#pragma unroll
  for (int i = 0; i < 6; ++i) out[i * n + idx] = z[i];
  out[6 * n + idx] = y[0]; out[7 * n + idx] = y[1];
}
// in: own g0..g5, h0, h1; other rg0..rg5, rh0, rh1; same -> dot(rg, rh), dot(rg, rh, same) (f64 only: the f32 bank has no
// slot space, RowDot<float> no three-argument form)
template <typename T> __device__ __forceinline__ void probe_rowdot(SOLO_PROBE_ARGS) {
  SOLO_PROBE_IDX;
  alignas(16) T own[8];
  alignas(16) T other[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) { own[i] = in[i * n + idx]; other[i] = in[(8 + i) * n + idx]; }
  RowDot<T> d;
  d.set(own, own + 6);
  out[idx] = d.dot(other, other + 6);
  if constexpr (sizeof(T) == 8) out[n + idx] = d.dot(other, other + 6, in[16 * n + idx]);
  else out[n + idx] = T(0);
}

#undef SOLO_PROBE_ARGS
#undef SOLO_PROBE_IDX

}  // namespace solo
