// emu_pacing_check.cpp — TEST-ONLY, stand-alone: the paced rollouts of tests/test_emu_progress_pacing.py, built with
// -fsanitize=address,undefined (the test builds and runs it; never loaded into Python).  emu_pacing_harness.cpp sizes the progress
// block at exactly progress_ints(plan) counters and the record scratch at one segment per robot.
//   emu_pacing_check CALL.bin
// CALL.bin: the layout of emu_roll_check.cpp - SoloConfig, SoloModel, SoloProgram (raw structs; the config's dtype is the precision),
// int32 {n, cases, kmax}, int32 [cases][3] = {steps_per_launch, k, rollout_streams}, then doubles: state [n][32], params [n][4],
// targets [n][12], actions [kmax][n][12], and int32 term_count [n][SOLO_MAX_TERMS].  Every case runs from that start twice - with a
// null block and with the block wired - and exit status 0 = the two agree bit for bit in every case (recorded obs / reward / done,
// the view, state, counters, targets, statistics), every launch of the paced run was wired, and the block holds n in the counters
// of the segments that have a successor and 0 elsewhere.
#include "emu_pacing_harness.cpp"

#include <cstdio>
#include <cstring>

template <class V>
static bool take(FILE* f, V* out, size_t count) { return fread(out, sizeof(V), count, f) == count; }

struct World {
  std::vector<double> state, snapshot, targets, params, obs, reward, stats, obs_out, reward_out;
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
  start.stats.assign((size_t)SOLO_STATS_SHARDS * SOLO_STATS_WIDTH, 0.0);
  for (int c = 0; c < cases; ++c) {
    SoloConfig cfg = base;
    cfg.steps_per_launch = spec[3 * c]; cfg.rollout_streams = spec[3 * c + 2];
    const int k = spec[3 * c + 1];
    World off = start, on = start;
    int32_t info[2][8], block[2][kMaxFusedSegments];
    int which = 0;
    for (World* w : {&off, &on}) {
      w->obs_out.assign((size_t)k * n * D, 0.0); w->reward_out.assign((size_t)k * n, 0.0); w->done_out.assign((size_t)k * n, 0);
      if (solo_emu_pacing_rollout(&cfg, &mdl, &prog, cfg.dtype, n, k, w->state.data(), w->snapshot.data(), acts.data(), w->targets.data(),
                                  w->params.data(), w->obs_out.data(), w->reward_out.data(), w->done_out.data(), w->obs.data(),
                                  w->reward.data(), w->done.data(), w->term.data(), w->stats.data(), SOLO_STEP_ALL, which, info[which], block[which]))
        return 1;
      ++which;
    }
    const int segments = (k + spec[3 * c] - 1) / spec[3 * c];
    bool counted = true;
    for (int s = 0; s < kMaxFusedSegments; ++s) counted = counted && block[0][s] == 0 && block[1][s] == (s < segments - 1 ? n : 0);
    const bool ok = on.same(off) && info[1][4] > 0 && info[1][6] == info[1][5] && info[0][6] == 0 && counted && solo_emu_take_fault() == 0;
    printf("S %d K %d streams %d: fuse %d, %d launches (%d wired), counters %d %d %d: %s\n", spec[3 * c], k, spec[3 * c + 2], info[1][4], info[1][5],
           info[1][6], block[1][0], block[1][1], block[1][2], ok ? "equals the run with a null block" : "DIFFERS");
    if (!ok) return 1;
  }
  return 0;
}
