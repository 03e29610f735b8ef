// emu_roll_check.cpp — TEST-ONLY, stand-alone: the fused-segment rollouts of tests/test_emu_roll.py, built with
// -fsanitize=address,undefined (the test builds and runs it; never loaded into Python).  emu_roll_harness.cpp sizes the record
// scratch at exactly record_reals(n, S) - one segment per robot - so a record addressed by the launch's step is a heap overflow here.
//   emu_roll_check CALL.bin
// CALL.bin: SoloConfig, SoloModel, SoloProgram (raw structs; the config's dtype is the precision), int32 {n, cases, kmax},
// int32 [cases][3] = {steps_per_launch, k, rollout_streams}, then doubles: state [n][32], params [n][4], targets [n][12], actions
// [kmax][n][12], and int32 term_count [n][SOLO_MAX_TERMS].  Every case runs from that start twice - solo_emu_rollout (the launches of
// before) and solo_emu_roll_rollout with fused segments - and exit status 0 = the two agree bit for bit in every case: recorded
// obs / reward / done, the view, state, counters, targets and statistics.
#include "emu_roll_harness.cpp"

#include <cstdio>
#include <cstring>

template <class V>
static bool take(FILE* f, V* out, size_t count) { return fread(out, sizeof(V), count, f) == count; }

struct World {
  std::vector<double> state, snapshot, targets, params, obs, reward, stats, warm, obs_out, reward_out;
  std::vector<uint8_t> done, done_out;
  std::vector<int32_t> term;
  bool same(const World& o) const {
    return state == o.state && targets == o.targets && obs == o.obs && reward == o.reward && done == o.done && term == o.term &&
           stats == o.stats && obs_out == o.obs_out && reward_out == o.reward_out && done_out == o.done_out;
  }
};

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s CALL.bin\n", argv[0]); return 2; }
  static SoloConfig base;
  static SoloModel mdl;
  static SoloProgram prog;
  FILE* f = fopen(argv[1], "rb");
  int32_t head[3];
  if (!f || !take(f, &base, 1) || !take(f, &mdl, 1) || !take(f, &prog, 1) || !take(f, head, 3)) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  const int n = head[0], cases = head[1], kmax = head[2], D = prog.num_obs;
  std::vector<int32_t> spec((size_t)cases * 3);
  World start;
  start.state.resize((size_t)n * SOLO_STATE_STRIDE); start.params.resize((size_t)n * 4); start.targets.resize((size_t)n * SOLO_NUM_JOINTS);
  std::vector<double> acts((size_t)kmax * n * SOLO_NUM_JOINTS);
  start.term.resize((size_t)n * SOLO_MAX_TERMS);
  if (!take(f, spec.data(), spec.size()) || !take(f, start.state.data(), start.state.size()) || !take(f, start.params.data(), start.params.size()) ||
      !take(f, start.targets.data(), start.targets.size()) || !take(f, acts.data(), acts.size()) || !take(f, start.term.data(), start.term.size())) {
    fprintf(stderr, "%s is too short\n", argv[1]);
    return 2;
  }
  fclose(f);
  start.snapshot = start.state;
  start.obs.assign((size_t)n * D, 0.0); start.reward.assign((size_t)n, 0.0); start.done.assign((size_t)n, 0);
  start.stats.assign((size_t)SOLO_STATS_SHARDS * SOLO_STATS_WIDTH, 0.0); start.warm.assign((size_t)n * 64, 0.0);
  for (int c = 0; c < cases; ++c) {
    SoloConfig cfg = base;
    cfg.steps_per_launch = spec[3 * c]; cfg.rollout_streams = spec[3 * c + 2];
    const int k = spec[3 * c + 1];
    World plain = start, fused = start;
    for (World* w : {&plain, &fused}) { w->obs_out.assign((size_t)k * n * D, 0.0); w->reward_out.assign((size_t)k * n, 0.0); w->done_out.assign((size_t)k * n, 0); }
    if (solo_emu_rollout(&cfg, &mdl, &prog, cfg.dtype, n, k, plain.state.data(), plain.snapshot.data(), acts.data(), plain.targets.data(),
                         plain.params.data(), plain.obs_out.data(), plain.reward_out.data(), plain.done_out.data(), plain.obs.data(),
                         plain.reward.data(), plain.done.data(), plain.term.data(), plain.stats.data(), SOLO_STEP_ALL, nullptr, plain.warm.data()))
      return 1;
    int32_t info[8];
    char names[256];
    if (solo_emu_roll_rollout(&cfg, &mdl, &prog, cfg.dtype, n, k, fused.state.data(), fused.snapshot.data(), acts.data(), fused.targets.data(),
                              fused.params.data(), fused.obs_out.data(), fused.reward_out.data(), fused.done_out.data(), fused.obs.data(),
                              fused.reward.data(), fused.done.data(), fused.term.data(), fused.stats.data(), SOLO_STEP_ALL, 1, info, names, 256))
      return 1;
    const bool ok = fused.same(plain) && info[4] > 0 && info[6] > 0 && strstr(names, "solo_roll_kernel") != nullptr && solo_emu_take_fault() == 0;
    printf("S %d K %d streams %d: fuse %d, %d launches (%d segmented), %s: %s\n", spec[3 * c], k, spec[3 * c + 2], info[4], info[5], info[6], names,
           ok ? "equals the unfused rollout" : "DIFFERS");
    if (!ok) return 1;
  }
  return 0;
}
