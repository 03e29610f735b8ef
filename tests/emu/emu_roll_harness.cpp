// emu_roll_harness.cpp — TEST-ONLY: fused segments (solo_roll_kernel: solo_step_body.h's kSegments) on the CPU wave emulator, next to
// the kernels of emu_harness.cpp.  One emulated rollout under the engine's launch policy WITH PlanInput::fuse set, as the engine
// sets it: make_plan decides, for_each_launch yields the fused launches, wire_launch sets KBuffers::seg_steps, choose_kernel picks the
// kernel.  The record scratch holds exactly record_reals(n, S) reals - ONE segment per robot, what the engine allocates - so a record
// indexed by the launch's step instead of the segment's is a heap overflow here (emu_roll_check.cpp runs these cases under
// AddressSanitizer).  The same rollout WITHOUT fused segments is solo_emu_rollout of emu_harness.cpp - the twin of
// tests/test_emu_roll.py.  Built by the tests that use it with the flags of tests/emu/Makefile.
#include "emu_harness.cpp"

// info (int32 [8], or null): the plan {S, launches, slices, migrate, fuse}, the kernel launches issued, the segmented ones among
// them, and whether the view was copied (tail_needs_copy).  names (or null): the kernels launched, in order, each once, ';'-separated
template <typename T>
static int run_roll(const EmuCall& c, bool fuse, int32_t* info, char* names, int names_len) {
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
  const bool resid = cfg->solver_residual_threshold > 0;
  PlanInput in{n, sizeof(T), n, cfg->steps_per_launch, cfg->rollout_streams, cfg->migrate_steps, false, false, k, flags};
  in.fuse = fuse && !resid;   // (Engine::plan_input)
  const Plan plan = make_plan(in);
  if (plan.migrate != 0) return (int)SOLO_ERR_INVALID_ARG;   // (this harness wires no queue)
  const size_t ns = (size_t)n * SOLO_STATE_STRIDE;
  std::vector<T> st = conv<T>(c.state, ns), snap = conv<T>(c.snapshot ? c.snapshot : c.state, ns);
  std::vector<T> tg = conv<T>(c.targets, (size_t)n * SOLO_NUM_JOINTS), par = conv<T>(c.params, (size_t)n * 4);
  std::vector<T> ob = conv<T>(c.obs, (size_t)n * (D > 0 ? D : 1)), rew = conv<T>(c.reward, (size_t)n);
  g_last_cost.assign((size_t)n, 0);
  // the record scratch at EXACTLY the size the engine allocates: S steps per robot, however many steps a fused launch has
  const bool records = leaves_records(flags);
  std::vector<T> traj(records ? record_reals(n, plan.S) : 0);
  std::vector<T> act = conv<T>(c.actions, (size_t)k * n * SOLO_NUM_JOINTS);
  std::vector<T> ob_out((flags & SOLO_STEP_OBS) && c.obs_out ? (size_t)k * n * D : 0), rew_out((flags & SOLO_STEP_REWARD) && c.reward_out ? (size_t)k * n : 0);
  EngineBuffers<T> e;
  e.state = st.data(); e.snapshot = snap.data(); e.targets = tg.data(); e.params = par.data(); e.obs = ob.data(); e.reward = rew.data();
  e.done = c.done; e.term_count = c.term_count; e.stats = c.stats;
  e.terrain = nullptr; e.order = nullptr; e.cost = g_last_cost.data(); e.warm = nullptr; e.fault = &g_fault;
  e.traj = traj.empty() ? nullptr : traj.data(); e.traj_steps = plan.S; e.queue = nullptr; e.queue_len = 0;
  e.n = n; e.obs_dim = D;
  const RolloutArgs<T> args{act.data(), (long long)n * SOLO_NUM_JOINTS, k, flags, ob_out.empty() ? nullptr : ob_out.data(),
                            rew_out.empty() ? nullptr : rew_out.data(), (flags & SOLO_STEP_DONE) ? c.done_out : nullptr};
  const KParams<T>* Pp = &P;
  std::string launched;
  int launches = 0, segmented = 0;
  const int rc = for_each_launch(plan, n, k, [&](const Launch& l) {
    KBuffers<T> B;
    QueueInit q;
    if (!wire_launch(plan, args, e, l, &B, &q) || q.ints > 0) return (int)SOLO_ERR_INVALID_ARG;
    const KernelId id = choose_kernel(false, false, false, resid, false, flags, 1, false, false, false, B.seg_steps > 0);   // (Engine::enqueue)
    const std::string name = kernel_name(id, sizeof(T));
    if (launched.find(name) == std::string::npos) launched += (launched.empty() ? "" : ";") + name;
    ++launches;
    segmented += B.seg_steps > 0;
    with_step_kernel<T>(id, [&](StepKernel<T> kernel) {
      for (int b = 0; b < l.count; ++b) WaveEmu::get().run_block(b, l.count, [&]() { kernel(Pp, B); });
    });
    return 0;
  });
  if (rc) return rc;
  const bool copy = tail_needs_copy<T>(plan, k, flags);
  if (copy) {   // (what Engine::rollout copies into the view when the last launch could not write it there)
    if (args.obs_out) for (size_t i = 0; i < (size_t)n * D; ++i) ob[i] = ob_out[(size_t)(k - 1) * n * D + i];
    if (args.reward_out) for (size_t i = 0; i < (size_t)n; ++i) rew[i] = rew_out[(size_t)(k - 1) * n + i];
    if (args.done_out) for (size_t i = 0; i < (size_t)n; ++i) e.done[i] = args.done_out[(size_t)(k - 1) * n + i];
  }
  if (info) { info[0] = plan.S; info[1] = plan.launches; info[2] = plan.slices; info[3] = plan.migrate; info[4] = plan.fuse; info[5] = launches; info[6] = segmented; info[7] = copy; }
  if (names) snprintf(names, (size_t)names_len, "%s", launched.c_str());
  back(c.state, st); back(c.targets, tg);
  if (flags & SOLO_STEP_OBS) { back(c.obs, ob); back(c.obs_out, ob_out); }
  if (flags & SOLO_STEP_REWARD) { back(c.reward, rew); back(c.reward_out, rew_out); }
  return 0;
}

// solo_emu_rollout's arguments (position control, flat ground, no warm start), then: fuse (what Engine::plan_input sets), info, names
extern "C" int solo_emu_roll_rollout(const SoloConfig* cfg, const SoloModel* mdl, const SoloProgram* prog, int dtype, int n, int k, double* state,
                                     const double* snapshot, const double* actions, double* targets, const double* params, double* obs_out,
                                     double* reward_out, uint8_t* done_out, double* obs, double* reward, uint8_t* done, int32_t* term_count,
                                     double* stats, uint32_t flags, int fuse, int32_t* info, char* names, int names_len) {
  EmuCall c;
  c.cfg = cfg; c.mdl = mdl; c.prog = prog; c.n = n; c.k = k; c.flags = flags;
  c.state = state; c.snapshot = snapshot; c.actions = actions; c.targets = targets; c.params = params;
  c.obs_out = obs_out; c.reward_out = reward_out; c.done_out = done_out;
  c.obs = obs; c.reward = reward; c.done = done; c.term_count = term_count; c.stats = stats;
  return dtype == SOLO_F32 ? run_roll<float>(c, fuse != 0, info, names, names_len) : run_roll<double>(c, fuse != 0, info, names, names_len);
}

// make_plan with PlanInput::fuse: out = {S, launches, slices, migrate, fuse}
extern "C" void solo_emu_roll_plan(const SoloConfig* cfg, int dtype, int n, int resident, int ctl_active, int sensing, int k, uint32_t flags,
                                   int decimation, int state_terms, int actuators, int wrench, int fuse, int32_t* out) {
  PlanInput in{n, dtype == SOLO_F32 ? sizeof(float) : sizeof(double), resident, cfg->steps_per_launch, cfg->rollout_streams,
               cfg->migrate_steps, ctl_active != 0, sensing != 0, k, flags};
  in.decimation = decimation; in.state_terms = state_terms != 0; in.actuators = actuators != 0; in.wrench = wrench != 0; in.fuse = fuse != 0;
  const Plan p = make_plan(in);
  out[0] = p.S; out[1] = p.launches; out[2] = p.slices; out[3] = p.migrate; out[4] = p.fuse;
}

// the distinct plans for_each_geometry visits for rollouts of up to k steps (what solo_engine_reserve prepares for):
// out [max][5] = {S, launches, slices, migrate, fuse} each; returns their number
extern "C" int solo_emu_roll_geometries(const SoloConfig* cfg, int dtype, int n, int resident, int k, uint32_t flags, int fuse, int32_t* out, int max) {
  PlanInput in{n, dtype == SOLO_F32 ? sizeof(float) : sizeof(double), resident, cfg->steps_per_launch, cfg->rollout_streams,
               cfg->migrate_steps, false, false, k, flags};
  in.fuse = fuse != 0;
  int count = 0;
  for_each_geometry(in, k, [&](const Plan& p) {
    if (count < max) { int32_t* o = out + 5 * count; o[0] = p.S; o[1] = p.launches; o[2] = p.slices; o[3] = p.migrate; o[4] = p.fuse; }
    ++count;
    return 0;
  });
  return count;
}
