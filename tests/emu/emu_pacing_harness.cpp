// emu_pacing_harness.cpp — TEST-ONLY: progress pacing of the segmented launch (solo_roll_kernel, solo_step_body.h's segment boundary)
// on the CPU wave emulator, next to the kernels of emu_harness.cpp.  emu_roll_harness.cpp's rollout - the engine's launch policy
// with PlanInput::fuse set, for_each_launch, wire_launch, choose_kernel - with ONE difference: EngineBuffers::progress points at a
// block of kMaxFusedSegments counters (zeroed in front of the rollout, as the engine does) or is null.  The emulator runs a launch's
// waves one after the other, each through all its segments, so a wave's rank at every boundary is its position in the issue order:
// launch-major, slice-minor, block by block - deterministic.  Built by the tests that use it with the flags of tests/emu/Makefile.
#include "emu_harness.cpp"

// info (int32 [8], or null): the plan {S, launches, slices, migrate, fuse}, the kernel launches issued, those wired to the block, and
// whether the view was copied.  progress_out (int32 [kMaxFusedSegments], or null): the block after the rollout (zeros without one)
template <typename T>
static int run_paced(const EmuCall& c, bool paced, int32_t* info, int32_t* progress_out) {
  const SoloConfig* cfg = c.cfg;
  const int n = c.n, k = c.k;
  const uint32_t flags = c.flags;
  std::string err;
  if (int rc = validate_model(*c.mdl, &err)) { fprintf(stderr, "emu: %s\n", err.c_str()); return rc; }
  static KParams<T> P;
  pack_params<T>(*cfg, *c.mdl, &P);
  int D = 0;
  if (c.prog) {
    if (int rc = pack_program<T>(*c.prog, &P, &err)) { fprintf(stderr, "emu: %s\n", err.c_str()); return rc; }
    D = c.prog->num_obs;
  }
  pack_terrain<T>(nullptr, &P);
  P.decimation = 1;
  for (int t = 0; t < SOLO_MAX_TERMS; ++t) P.term_value[t] = T(0);
  P.term_fired = nullptr; P.contact = nullptr; P.contact_traj = nullptr; P.contact_traj_steps = 0;
  PlanInput in{n, sizeof(T), n, cfg->steps_per_launch, cfg->rollout_streams, cfg->migrate_steps, false, false, k, flags};
  in.fuse = true;
  const Plan plan = make_plan(in);
  if (plan.migrate != 0 || cfg->solver_residual_threshold > 0) return (int)SOLO_ERR_INVALID_ARG;
  const size_t ns = (size_t)n * SOLO_STATE_STRIDE;
  std::vector<T> st = conv<T>(c.state, ns), snap = conv<T>(c.snapshot ? c.snapshot : c.state, ns);
  std::vector<T> tg = conv<T>(c.targets, (size_t)n * SOLO_NUM_JOINTS), par = conv<T>(c.params, (size_t)n * 4);
  std::vector<T> ob = conv<T>(c.obs, (size_t)n * (D > 0 ? D : 1)), rew = conv<T>(c.reward, (size_t)n);
  g_last_cost.assign((size_t)n, 0);
  const bool records = leaves_records(flags);
  std::vector<T> traj(records ? record_reals(n, plan.S) : 0);
  std::vector<T> act = conv<T>(c.actions, (size_t)k * n * SOLO_NUM_JOINTS);
  std::vector<T> ob_out((flags & SOLO_STEP_OBS) && c.obs_out ? (size_t)k * n * D : 0), rew_out((flags & SOLO_STEP_REWARD) && c.reward_out ? (size_t)k * n : 0);
  // the block at EXACTLY the size the engine allocates: a counter indexed past a launch's segments is a heap overflow here
  std::vector<int32_t> progress(paced ? progress_ints(plan) : 0, 0);
  EngineBuffers<T> e;
  e.state = st.data(); e.snapshot = snap.data(); e.targets = tg.data(); e.params = par.data(); e.obs = ob.data(); e.reward = rew.data();
  e.done = c.done; e.term_count = c.term_count; e.stats = c.stats;
  e.terrain = nullptr; e.order = nullptr; e.cost = g_last_cost.data(); e.warm = nullptr; e.fault = &g_fault;
  e.traj = traj.empty() ? nullptr : traj.data(); e.traj_steps = plan.S; e.queue = nullptr; e.queue_len = 0;
  e.n = n; e.obs_dim = D;
  e.progress = progress.empty() ? nullptr : progress.data();
  const RolloutArgs<T> args{act.data(), (long long)n * SOLO_NUM_JOINTS, k, flags, ob_out.empty() ? nullptr : ob_out.data(),
                            rew_out.empty() ? nullptr : rew_out.data(), (flags & SOLO_STEP_DONE) ? c.done_out : nullptr};
  const KParams<T>* Pp = &P;
  int launches = 0, wired = 0;
  const int rc = for_each_launch(plan, n, k, [&](const Launch& l) {
    KBuffers<T> B;
    QueueInit q;
    if (!wire_launch(plan, args, e, l, &B, &q) || q.ints > 0) return (int)SOLO_ERR_INVALID_ARG;
    const KernelId id = choose_kernel(false, false, false, false, false, flags, 1, false, false, false, B.seg_steps > 0);   // (Engine::enqueue)
    ++launches;
    wired += B.progress != nullptr;
    if (B.progress != nullptr && B.progress != e.progress) return (int)SOLO_ERR_INVALID_ARG;   // (every slice: the SAME block)
    with_step_kernel<T>(id, [&](StepKernel<T> kernel) {
      for (int b = 0; b < l.count; ++b) WaveEmu::get().run_block(b, l.count, [&]() { kernel(Pp, B); });
    });
    return 0;
  });
  if (rc) return rc;
  const bool copy = tail_needs_copy<T>(plan, k, flags);
  if (copy) {
    if (args.obs_out) for (size_t i = 0; i < (size_t)n * D; ++i) ob[i] = ob_out[(size_t)(k - 1) * n * D + i];
    if (args.reward_out) for (size_t i = 0; i < (size_t)n; ++i) rew[i] = rew_out[(size_t)(k - 1) * n + i];
    if (args.done_out) for (size_t i = 0; i < (size_t)n; ++i) e.done[i] = args.done_out[(size_t)(k - 1) * n + i];
  }
  if (info) { info[0] = plan.S; info[1] = plan.launches; info[2] = plan.slices; info[3] = plan.migrate; info[4] = plan.fuse; info[5] = launches; info[6] = wired; info[7] = copy; }
  if (progress_out) for (int i = 0; i < kMaxFusedSegments; ++i) progress_out[i] = i < (int)progress.size() ? progress[(size_t)i] : 0;
  back(c.state, st); back(c.targets, tg);
  if (flags & SOLO_STEP_OBS) { back(c.obs, ob); back(c.obs_out, ob_out); }
  if (flags & SOLO_STEP_REWARD) { back(c.reward, rew); back(c.reward_out, rew_out); }
  return 0;
}

// solo_emu_rollout's arguments (position control, flat ground, no warm start), then: paced (0: a null block), info, progress_out
extern "C" int solo_emu_pacing_rollout(const SoloConfig* cfg, const SoloModel* mdl, const SoloProgram* prog, int dtype, int n, int k, double* state,
                                       const double* snapshot, const double* actions, double* targets, const double* params, double* obs_out,
                                       double* reward_out, uint8_t* done_out, double* obs, double* reward, uint8_t* done, int32_t* term_count,
                                       double* stats, uint32_t flags, int paced, int32_t* info, int32_t* progress_out) {
  EmuCall c;
  c.cfg = cfg; c.mdl = mdl; c.prog = prog; c.n = n; c.k = k; c.flags = flags;
  c.state = state; c.snapshot = snapshot; c.actions = actions; c.targets = targets; c.params = params;
  c.obs_out = obs_out; c.reward_out = reward_out; c.done_out = done_out;
  c.obs = obs; c.reward = reward; c.done = done; c.term_count = term_count; c.stats = stats;
  return dtype == SOLO_F32 ? run_paced<float>(c, paced != 0, info, progress_out) : run_paced<double>(c, paced != 0, info, progress_out);
}

// the wiring of a rollout of k steps under the policy (fuse: PlanInput::fuse), without running it: out [max][3] = {slice, segmented,
// which block the launch got: 0 = none, 1 = the engine's, 2 = another pointer} per launch in issue order, then what
// for_each_geometry's plans need of the block: *geometry_ints = the largest progress_ints over the geometries of up to k steps;
// returns the number of launches
extern "C" int solo_emu_pacing_wiring(const SoloConfig* cfg, int dtype, int n, int k, uint32_t flags, int fuse, int32_t* out, int max, int32_t* plan_out,
                                      int32_t* geometry_ints) {
  PlanInput in{n, dtype == SOLO_F32 ? sizeof(float) : sizeof(double), n, cfg->steps_per_launch, cfg->rollout_streams, cfg->migrate_steps, false, false, k, flags};
  in.fuse = fuse != 0;
  const Plan plan = make_plan(in);
  if (plan_out) { plan_out[0] = plan.S; plan_out[1] = plan.launches; plan_out[2] = plan.slices; plan_out[3] = plan.fuse; plan_out[4] = (int32_t)progress_ints(plan); plan_out[5] = rollout_is_paced(plan, k); }
  static int32_t block[kMaxFusedSegments];
  static double dummy[4];
  EngineBuffers<double> e{};
  e.traj = dummy; e.traj_steps = plan.S; e.n = n; e.obs_dim = 1; e.progress = block;
  const RolloutArgs<double> args{dummy, 0, k, flags, nullptr, nullptr, nullptr};
  int count = 0;
  for_each_launch(plan, n, k, [&](const Launch& l) {
    KBuffers<double> B;
    QueueInit q;
    wire_launch(plan, args, e, l, &B, &q);
    if (count < max) { out[3 * count] = l.slice; out[3 * count + 1] = B.seg_steps > 0; out[3 * count + 2] = B.progress == nullptr ? 0 : (B.progress == block ? 1 : 2); }
    ++count;
    return 0;
  });
  size_t most = 0;
  for_each_geometry(in, k, [&](const Plan& p) { most = progress_ints(p) > most ? progress_ints(p) : most; return 0; });
  if (geometry_ints) *geometry_ints = (int32_t)most;
  return count;
}
