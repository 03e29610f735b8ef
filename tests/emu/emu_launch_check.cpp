// emu_launch_check.cpp — TEST-ONLY, stand-alone: the whole-rollout cases of tests/test_launch_plan.py and the queue sizing
// sweep, built with -fsanitize=address,undefined (make asan).  The emulator allocates the record scratch and the migration
// queues at exactly the sizes the engine does (solo_launch.h), so a launch wired past its region is a heap overflow here.
//   python tests/test_launch_plan.py DIR ; emu_launch_check DIR      (make asan-check does both)
// reads DIR/config.bin, model.bin, program.bin (the raw structs); exit status 0 = every rollout equals its single steps.
#include "emu_harness.cpp"

#include <cstdio>
#include <cstring>

template <class S>
static bool load(const std::string& path, S* out) {
  FILE* f = fopen(path.c_str(), "rb");
  const bool ok = f != nullptr && fread(out, sizeof(S), 1, f) == 1;
  if (f) fclose(f);
  if (!ok) fprintf(stderr, "cannot read %s\n", path.c_str());
  return ok;
}

static constexpr int N = 8;

// the buffers of tests/emu_kernel.py's EmuEngine
struct World {
  std::vector<double> state, snapshot, targets, params, obs, reward, stats, warm;
  std::vector<uint8_t> done;
  std::vector<int32_t> term;
  World(const SoloConfig& cfg, int D)
      : state(N * SOLO_STATE_STRIDE), targets(N * SOLO_NUM_JOINTS), params(N * 4), obs(N * D), reward(N),
        stats(SOLO_STATS_SHARDS * SOLO_STATS_WIDTH), warm(N * 64), done(N), term(N * SOLO_MAX_TERMS) {
    for (int e = 0; e < N; ++e) {
      for (int a = 0; a < 3; ++a) state[e * SOLO_STATE_STRIDE + SOLO_S_POS + a] = cfg.start_pos[a];
      for (int a = 0; a < 4; ++a) state[e * SOLO_STATE_STRIDE + SOLO_S_QUAT + a] = cfg.start_quat[a];
      params[e * 4] = cfg.lateral_friction;
      params[e * 4 + 1] = 1.0;
    }
    snapshot = state;
  }
  bool same(const World& o) const {
    return state == o.state && targets == o.targets && obs == o.obs && reward == o.reward && done == o.done && term == o.term;
  }
};

static int step(const SoloConfig& cfg, const SoloModel& mdl, const SoloProgram& prog, World& w, const double* act, uint32_t flags) {
  return solo_emu_step(&cfg, &mdl, &prog, cfg.dtype, N, w.state.data(), w.snapshot.data(), act, w.targets.data(), w.params.data(),
                       w.obs.data(), w.reward.data(), w.done.data(), w.term.data(), w.stats.data(), flags, nullptr, w.warm.data());
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s DIR\n", argv[0]); return 2; }
  static SoloConfig base;
  static SoloModel mdl;
  static SoloProgram prog;
  const std::string dir = argv[1];
  if (!load(dir + "/config.bin", &base) || !load(dir + "/model.bin", &mdl) || !load(dir + "/program.bin", &prog)) return 2;
  const int D = prog.num_obs;

  long long cases = 0;
  if (solo_emu_queue_sweep(260, 16, &cases) != 0) { fprintf(stderr, "queue sizing: a launch does not fit its region\n"); return 1; }
  printf("queue sizing sweep: %lld launches fit\n", cases);

  struct Case { const char* name; int k, spl, streams, migrate; uint32_t flags; };
  const Case all[] = {{"a", 23, 7, 2, -1, SOLO_STEP_ALL}, {"b", 22, 7, 2, -1, SOLO_STEP_ALL}, {"c1", 193, 128, 1, 1, SOLO_STEP_ALL},
                      {"c2", 193, 128, 2, 1, SOLO_STEP_ALL}, {"d", 23, 7, 2, -1, SOLO_STEP_PHYSICS | SOLO_STEP_DONE}};
  std::vector<double> acts((size_t)193 * N * SOLO_NUM_JOINTS);
  unsigned long long seed = 11;
  for (double& a : acts) {
    seed = seed * 6364136223846793005ull + 1442695040888963407ull;
    a = -6.0 + 12.0 * (double)(seed >> 11) / 9007199254740992.0;
  }
  for (int dtype : {(int)SOLO_F64, (int)SOLO_F32}) {
    SoloConfig cfg = base;
    cfg.dtype = dtype;
    World start(cfg, D);
    std::vector<double> settle(N * SOLO_NUM_JOINTS);
    for (int i = 0; i < N * SOLO_NUM_JOINTS; ++i) settle[i] = cfg.settle_targets[i % SOLO_NUM_JOINTS] / cfg.action_scale;
    for (int s = 0; s < 40; ++s) if (step(cfg, mdl, prog, start, settle.data(), SOLO_STEP_PHYSICS)) return 1;
    start.snapshot = start.state;
    for (const Case& c : all) {
      World single = start, whole = start;
      std::vector<double> obs((size_t)c.k * N * D), rew((size_t)c.k * N), obs1, rew1;
      std::vector<uint8_t> done((size_t)c.k * N), done1;
      for (int s = 0; s < c.k; ++s) {
        if (step(cfg, mdl, prog, single, acts.data() + (size_t)s * N * SOLO_NUM_JOINTS, c.flags)) return 1;
        obs1.insert(obs1.end(), single.obs.begin(), single.obs.end());
        rew1.insert(rew1.end(), single.reward.begin(), single.reward.end());
        done1.insert(done1.end(), single.done.begin(), single.done.end());
      }
      SoloConfig geo = cfg;
      geo.steps_per_launch = c.spl; geo.rollout_streams = c.streams; geo.migrate_steps = c.migrate;
      if (solo_emu_rollout(&geo, &mdl, &prog, dtype, N, c.k, whole.state.data(), whole.snapshot.data(), acts.data(), whole.targets.data(),
                           whole.params.data(), obs.data(), rew.data(), done.data(), whole.obs.data(), whole.reward.data(), whole.done.data(),
                           whole.term.data(), whole.stats.data(), c.flags, nullptr, whole.warm.data()))
        return 1;
      const bool outputs = (c.flags & SOLO_STEP_OBS) != 0;
      const bool ok = whole.same(single) && done == done1 && (!outputs || (obs == obs1 && rew == rew1)) && solo_emu_take_fault() == 0;
      printf("%s %s: %s\n", dtype == SOLO_F32 ? "f32" : "f64", c.name, ok ? "equals its single steps" : "DIFFERS");
      if (!ok) return 1;
    }
  }
  return 0;
}
