// waveops_probe.hip — TEST-ONLY GPU build of tests/waveops/probe_body.h over gym_solo_amd/csrc/solo_wave_ops.h: one kernel
// per (probe, type), one wave per workgroup, launched by solo_waveops_probe().  Built as
// gym_solo_amd/csrc/libsolo_waveops_probe.so (`make -C gym_solo_amd/csrc test-libs`); tests/test_gpu_waveops.py loads it.
// Never part of the product library.
#include "solo_wave_ops.h"
#include "probe_body.h"

namespace {

#define X(id, name, nin, nout, types)                                                                        \
  template <typename T> __global__ __launch_bounds__(64) void k_##name(const T* in, T* out, int n) {         \
    solo::probe_##name<T>(in, out, n);                                                                       \
  }                                                                                                          \
  struct K_##name {                                                                                          \
    template <typename T> static void launch(const void* in, void* out, int blocks, hipStream_t stream) {    \
      hipLaunchKernelGGL(k_##name<T>, dim3(blocks), dim3(64), 0, stream, (const T*)in, (T*)out, blocks * 64); \
    }                                                                                                        \
  };
SOLO_WAVEOPS_PROBES(X)
#undef X

// a (probe, type) pair outside the probe's type list is never instantiated
template <typename K, typename T, bool ON> struct Launch {
  static int go(const void* in, void* out, int blocks, hipStream_t stream) {
    K::template launch<T>(in, out, blocks, stream);
    return (int)hipGetLastError();
  }
};
template <typename K, typename T> struct Launch<K, T, false> {
  static int go(const void*, void*, int, hipStream_t) { return -2; }
};

}  // namespace

// probe: an id of SOLO_WAVEOPS_PROBES; dtype: 0 float, 1 double, 2 int32; in_dev / out_dev: the probe's nin / nout planes
// of 64 * blocks elements each.  Returns the HIP status of the launch (-1: no such probe, -2: not for this type).
extern "C" int solo_waveops_probe(int probe, int dtype, const void* in_dev, void* out_dev, int blocks, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (blocks <= 0 || dtype < 0 || dtype > 2) return -1;
  switch (probe) {
#define X(id, name, nin, nout, types)                                                                \
    case id:                                                                                         \
      if (dtype == 0) return Launch<K_##name, float, ((types) & 1) != 0>::go(in_dev, out_dev, blocks, s);  \
      if (dtype == 1) return Launch<K_##name, double, ((types) & 2) != 0>::go(in_dev, out_dev, blocks, s); \
      return Launch<K_##name, int, ((types) & 4) != 0>::go(in_dev, out_dev, blocks, s);
    SOLO_WAVEOPS_PROBES(X)
#undef X
  }
  return -1;
}
