// emu_waveops_harness.cpp — TEST-ONLY CPU build of tests/waveops/probe_body.h over wave_emu.h: the probes that
// tests/waveops/waveops_probe.hip runs on the GPU, executed lane by lane on the fibre emulator over host pointers.
// tests/test_emu_waveops.py checks the emulator's primitives with it; tests/test_gpu_waveops.py compares the GPU's real-valued
// sums with its results bit for bit.
#include "wave_emu.h"
#define SOLO_WAVEOPS_EMU 1
#include "../waveops/probe_body.h"

namespace {

template <typename T> using ProbeFn = void (*)(const T*, T*, int);

template <typename T> int run(ProbeFn<T> fn, const void* in, void* out, int blocks) {
  const T* i = (const T*)in;
  T* o = (T*)out;
  const int n = blocks * 64;
  for (int b = 0; b < blocks; ++b) solo::WaveEmu::get().run_block(b, blocks, [&]() { fn(i, o, n); });
  return 0;
}

// a (probe, type) pair outside the probe's type list is never instantiated
#define X(id, name, nin, nout, types) \
  struct K_##name { template <typename T> static ProbeFn<T> fn() { return &solo::probe_##name<T>; } };
SOLO_WAVEOPS_PROBES(X)
#undef X

template <typename K, typename T, bool ON> struct Launch {
  static int go(const void* in, void* out, int blocks) { return run<T>(K::template fn<T>(), in, out, blocks); }
};
template <typename K, typename T> struct Launch<K, T, false> {
  static int go(const void*, void*, int) { return -2; }
};

}  // namespace

// the GPU library's entry point over HOST pointers (`stream` is ignored); -1 also for the probes this build leaves out
extern "C" int solo_waveops_probe(int probe, int dtype, const void* in, void* out, int blocks, void* /*stream*/) {
  if (blocks <= 0 || dtype < 0 || dtype > 2) return -1;
  switch (probe) {
#define X(id, name, nin, nout, types)                                                                               \
    case id:                                                                                                        \
      if (dtype == 0) return Launch<K_##name, float, ((types) & 1) != 0>::go(in, out, blocks);    \
      if (dtype == 1) return Launch<K_##name, double, ((types) & 2) != 0>::go(in, out, blocks);   \
      return Launch<K_##name, int, ((types) & 4) != 0>::go(in, out, blocks);
    SOLO_WAVEOPS_PROBES(X)
#undef X
  }
  return -1;
}
