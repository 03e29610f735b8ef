// emu_push_ubsan_main.cpp — TEST-ONLY: a stand-alone program around emu_push_harness.cpp, for a sanitizer build of the
// push kernels on the CPU wave emulator (tests/test_emu_push.py builds it with -fsanitize=undefined and runs it).
// argv[1]: the call as raw bytes (written by the test: SoloConfig, SoloModel, SoloProgram, int32 has_control, SoloControl,
// int32 {dtype, n, k, decimation}, double values[SOLO_MAX_TERMS], then doubles: state [n][32], snapshot [n][32], actions [k][n][12],
// targets [n][12], params [n][4], actuators [n][SOLO_ACTUATOR_WIDTH], wrench [n][SOLO_WRENCH_WIDTH]).  Runs ONE recording rollout of k control steps and then one
// physics-only launch under the first action row, and writes to argv[2]: doubles state, targets, obs_out, reward_out; int32
// term_count [n][4]; uint8 done_out [k][n], term_fired [n].
#include "emu_push_harness.cpp"

#include <cstdio>

template <class X>
static bool get(FILE* f, X* x, size_t cnt = 1) { return fread(x, sizeof(X), cnt, f) == cnt; }
template <class X>
static bool put(FILE* f, const X* x, size_t cnt) { return fwrite(x, sizeof(X), cnt, f) == cnt; }

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s call.bin out.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  static SoloConfig cfg; static SoloModel mdl; static SoloProgram prog; static SoloControl ctl;
  int32_t has_ctl = 0, head[4] = {0, 0, 0, 0};
  double values[SOLO_MAX_TERMS];
  if (!get(f, &cfg) || !get(f, &mdl) || !get(f, &prog) || !get(f, &has_ctl) || !get(f, &ctl) || !get(f, head, 4) || !get(f, values, SOLO_MAX_TERMS)) return 2;
  const int dtype = head[0], n = head[1], k = head[2], decimation = head[3];
  if (n < 1 || n > 64 || k < 1 || k > 64 || prog.num_obs < 1) return 2;
  std::vector<double> state((size_t)n * SOLO_STATE_STRIDE), snapshot(state.size()), actions((size_t)k * n * SOLO_NUM_JOINTS),
      targets((size_t)n * SOLO_NUM_JOINTS), params((size_t)n * 4), actuators((size_t)n * SOLO_ACTUATOR_WIDTH), wrench((size_t)n * SOLO_WRENCH_WIDTH);
  if (!get(f, state.data(), state.size()) || !get(f, snapshot.data(), snapshot.size()) || !get(f, actions.data(), actions.size()) ||
      !get(f, targets.data(), targets.size()) || !get(f, params.data(), params.size()) || !get(f, actuators.data(), actuators.size()) ||
      !get(f, wrench.data(), wrench.size())) return 2;
  fclose(f);
  const int D = prog.num_obs;
  std::vector<double> obs_out((size_t)k * n * D), reward_out((size_t)k * n), obs((size_t)n * D), reward((size_t)n),
      stats((size_t)SOLO_STATS_SHARDS * SOLO_STATS_WIDTH, 0.0);
  std::vector<uint8_t> done_out((size_t)k * n), done((size_t)n), fired((size_t)n);
  std::vector<int32_t> term_count((size_t)n * SOLO_MAX_TERMS, 0);
  char name[96];
  int rc = solo_emu_push_call(&cfg, &mdl, &prog, has_ctl ? &ctl : nullptr, dtype, n, k, 0, decimation, SOLO_STEP_ALL, state.data(), snapshot.data(),
                             actions.data(), targets.data(), params.data(), obs_out.data(), reward_out.data(), done_out.data(), obs.data(),
                             reward.data(), done.data(), term_count.data(), stats.data(), values, fired.data(), actuators.data(), wrench.data(), name, 96);
  if (rc) return 3;
  printf("%s\n", name);
  rc = solo_emu_push_call(&cfg, &mdl, &prog, has_ctl ? &ctl : nullptr, dtype, n, 1, 1, decimation, SOLO_STEP_PHYSICS, state.data(), snapshot.data(),
                         actions.data(), targets.data(), params.data(), nullptr, nullptr, nullptr, obs.data(), reward.data(), done.data(),
                         term_count.data(), stats.data(), values, fired.data(), actuators.data(), wrench.data(), name, 96);
  if (rc) return 3;
  printf("%s\n", name);
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  const bool ok = put(o, state.data(), state.size()) && put(o, targets.data(), targets.size()) && put(o, obs_out.data(), obs_out.size()) &&
                  put(o, reward_out.data(), reward_out.size()) && put(o, term_count.data(), term_count.size()) &&
                  put(o, done_out.data(), done_out.size()) && put(o, fired.data(), fired.size());
  return fclose(o) == 0 && ok ? 0 : 2;
}
