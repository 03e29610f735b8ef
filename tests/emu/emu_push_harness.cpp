// emu_push_harness.cpp — TEST-ONLY: external base wrenches (solo_push_kernel: solo_step_body.h's kPush) on the CPU wave emulator,
// next to the kernels of emu_harness.cpp and emu_actuator_harness.cpp.  One emulated engine call - a single-step launch or a whole
// rollout under the engine's launch policy - with the engine's base wrench block [n][SOLO_WRENCH_WIDTH] and, as in the engine, the
// actuator block or the all-ones block that stands for "off".  EmuCall has no field for either block, so the runner that wires
// them lives here (run_push: emu_actuator_harness.cpp's run_act with KParams::wrench, PlanInput::wrench and choose_kernel's last
// argument); a call WITHOUT a wrench block goes through solo_emu_act_call - the kernels of before, the twin of
// tests/test_emu_push.py.  Built by the tests that use it with the flags of tests/emu/Makefile.
#include "emu_actuator_harness.cpp"

#include <cstddef>

template <typename T>
static int run_push(const EmuCall& c, const double* actuators, const double* wrench) {
  const SoloConfig* cfg = c.cfg;
  const int n = c.n, k = c.k;
  const uint32_t flags = c.flags;
  std::string err;
  if (int rc = validate_model(*c.mdl, &err)) { fprintf(stderr, "emu: %s\n", err.c_str()); return rc; }
  // (what solo_engine_set_base_wrench and solo_engine_set_actuators check before a block goes on - the wrench TABLE is the
  // setter's to validate, solo_emu_push_validate: the block a launch reads may hold an in-place write, which nobody validates;
  // without an actuator block the push kernels read all ones: Engine::point_actuators)
  std::vector<T> wr_block = conv<T>(wrench, (size_t)n * SOLO_WRENCH_WIDTH);
  if (int rc = base_wrench_conflict(*cfg, c.contact != nullptr, &err)) { fprintf(stderr, "emu: %s\n", err.c_str()); return rc; }
  std::vector<T> act_block = actuators ? conv<T>(actuators, (size_t)n * SOLO_ACTUATOR_WIDTH) : std::vector<T>((size_t)n * SOLO_ACTUATOR_WIDTH, T(1));
  if (actuators) {
    if (int rc = actuators_conflict(*cfg, c.contact != nullptr, &err)) { fprintf(stderr, "emu: %s\n", err.c_str()); return rc; }
    if (int rc = validate_actuators<T>(act_block.data(), n, &err)) { fprintf(stderr, "emu: %s\n", err.c_str()); return rc; }
  }
  static KParams<T> P;
  pack_params<T>(*cfg, *c.mdl, &P);
  int D = 0;
  if (c.prog) {
    if (int rc = pack_program<T>(*c.prog, &P, &err)) { fprintf(stderr, "emu: %s\n", err.c_str()); return rc; }
    D = c.prog->num_obs;
  }
  if (c.ctl) pack_control<T>(*cfg, *c.ctl, &P);
  pack_terrain<T>(c.terrain, &P);
  P.decimation = c.decimation;
  for (int t = 0; t < SOLO_MAX_TERMS; ++t) P.term_value[t] = c.term_values ? (T)c.term_values[t] : T(0);
  P.term_fired = c.term_fired;
  P.actuators = act_block.data();
  P.wrench = wr_block.data();
  const bool ctl_active = c.ctl != nullptr && c.ctl->mode != SOLO_CTRL_POSITION;
  const bool state_terms = c.prog != nullptr && program_reads_state(*c.prog);
  PlanInput in{n, sizeof(T), n, cfg->steps_per_launch, cfg->rollout_streams, cfg->migrate_steps, ctl_active, false, k, flags};
  in.decimation = c.decimation;
  in.state_terms = state_terms;
  in.actuators = actuators != nullptr;
  in.wrench = true;
  const Plan plan = c.single ? Plan{1, 1, 1, 0} : make_plan(in);
  if (plan.migrate != 0) return (int)SOLO_ERR_INVALID_ARG;   // (these launches never migrate)
  const size_t ns = (size_t)n * SOLO_STATE_STRIDE;
  std::vector<T> st = conv<T>(c.state, ns), snap = conv<T>(c.snapshot ? c.snapshot : c.state, ns);
  std::vector<T> tg = conv<T>(c.targets, (size_t)n * SOLO_NUM_JOINTS), par = conv<T>(c.params, (size_t)n * 4);
  std::vector<T> ob = conv<T>(c.obs, (size_t)n * (D > 0 ? D : 1)), rew = conv<T>(c.reward, (size_t)n);
  std::vector<T> terr = conv<T>(c.terrain ? c.terrain->heights : nullptr, c.terrain ? (size_t)c.terrain->nx * c.terrain->ny : 0);
  std::vector<uint8_t> done_own(c.done ? 0 : (size_t)n, 0);
  std::vector<int32_t> term_own(c.term_count ? 0 : (size_t)n * SOLO_MAX_TERMS, 0);
  g_last_cost.assign((size_t)n, 0);
  const bool records = leaves_records(flags);
  std::vector<T> traj(records ? record_reals(n, plan.S) : 0);
  P.contact = nullptr; P.contact_traj = nullptr; P.contact_traj_steps = 0;
  std::vector<T> act = conv<T>(c.actions, c.actions ? (size_t)k * n * SOLO_NUM_JOINTS : 0);
  std::vector<T> ob_out((flags & SOLO_STEP_OBS) && c.obs_out ? (size_t)k * n * D : 0), rew_out((flags & SOLO_STEP_REWARD) && c.reward_out ? (size_t)k * n : 0);
  EngineBuffers<T> e;
  e.state = st.data(); e.snapshot = snap.data(); e.targets = tg.data(); e.params = par.data(); e.obs = ob.data(); e.reward = rew.data();
  e.done = c.done ? c.done : done_own.data(); e.term_count = c.term_count ? c.term_count : term_own.data(); e.stats = c.stats;
  e.terrain = terr.empty() ? nullptr : terr.data(); e.order = nullptr; e.cost = g_last_cost.data();
  e.warm = nullptr; e.fault = &g_fault;
  e.traj = traj.empty() ? nullptr : traj.data(); e.traj_steps = plan.S; e.queue = nullptr; e.queue_len = 0;
  e.n = n; e.obs_dim = D;
  const RolloutArgs<T> args{act.empty() ? nullptr : act.data(), (!c.single && !act.empty()) ? (long long)n * SOLO_NUM_JOINTS : 0, k, flags,
                            ob_out.empty() ? nullptr : ob_out.data(), rew_out.empty() ? nullptr : rew_out.data(),
                            (flags & SOLO_STEP_DONE) ? c.done_out : nullptr};
  const KParams<T>* Pp = &P;
  std::string launched;
  const int rc = for_each_launch(plan, n, k, [&](const Launch& l) {
    KBuffers<T> B;
    QueueInit q;
    if (!wire_launch(plan, args, e, l, &B, &q) || q.ints > 0) return (int)SOLO_ERR_INVALID_ARG;
    const KernelId id = choose_kernel(false, ctl_active, false, false, false, flags, c.decimation, state_terms, actuators != nullptr, true);
    launched = kernel_name(id, sizeof(T));
    with_step_kernel<T>(id, [&](StepKernel<T> kernel) {
      for (int b = 0; b < l.count; ++b) WaveEmu::get().run_block(b, l.count, [&]() { kernel(Pp, B); });
    });
    return 0;
  });
  if (rc) return rc;
  if (c.kernel_name) snprintf(c.kernel_name, (size_t)c.kernel_name_len, "%s", launched.c_str());
  if (!c.single && tail_needs_copy<T>(plan, k, flags)) {
    if (args.obs_out) for (size_t i = 0; i < (size_t)n * D; ++i) ob[i] = ob_out[(size_t)(k - 1) * n * D + i];
    if (args.reward_out) for (size_t i = 0; i < (size_t)n; ++i) rew[i] = rew_out[(size_t)(k - 1) * n + i];
    if (args.done_out) for (size_t i = 0; i < (size_t)n; ++i) e.done[i] = args.done_out[(size_t)(k - 1) * n + i];
  }
  back(c.state, st); back(c.targets, tg);
  if (flags & SOLO_STEP_OBS) { back(c.obs, ob); back(c.obs_out, ob_out); }
  if (flags & SOLO_STEP_REWARD) { back(c.reward, rew); back(c.reward_out, rew_out); }
  return 0;
}

// solo_emu_act_call with the base wrench block [n][SOLO_WRENCH_WIDTH] as one more argument in front of the name (null = off: that
// call itself).  actuators: the actuator block, or null = off.
extern "C" int solo_emu_push_call(const SoloConfig* cfg, const SoloModel* mdl, const SoloProgram* prog, const SoloControl* ctl, int dtype,
                                  int n, int k, int single, int decimation, uint32_t flags, double* state, const double* snapshot,
                                  const double* actions, double* targets, const double* params, double* obs_out, double* reward_out,
                                  uint8_t* done_out, double* obs, double* reward, uint8_t* done, int32_t* term_count, double* stats,
                                  const double* term_values, uint8_t* term_fired, const double* actuators, const double* wrench, char* name,
                                  int name_len) {
  // (a launch the push kernels do not take - it does not step the physics - keeps its kernel)
  if (wrench == nullptr || choose_kernel(false, false, false, false, false, flags, decimation, false, actuators != nullptr, true).family != KERNEL_PUSH)
    return solo_emu_act_call(cfg, mdl, prog, ctl, dtype, n, k, single, decimation, flags, state, snapshot, actions, targets, params, obs_out,
                             reward_out, done_out, obs, reward, done, term_count, stats, term_values, term_fired, actuators, name, name_len);
  EmuCall c;
  c.cfg = cfg; c.mdl = mdl; c.prog = prog; c.ctl = ctl; c.n = n; c.k = single ? 1 : k; c.flags = flags; c.single = single != 0;
  c.state = state; c.snapshot = snapshot; c.actions = actions; c.targets = targets; c.params = params;
  c.obs_out = obs_out; c.reward_out = reward_out; c.done_out = done_out;
  c.obs = obs; c.reward = reward; c.done = done; c.term_count = term_count; c.stats = stats;
  c.decimation = decimation; c.term_values = term_values; c.term_fired = term_fired; c.kernel_name = name; c.kernel_name_len = name_len;
  return dtype == SOLO_F32 ? run_push<float>(c, actuators, wrench) : run_push<double>(c, actuators, wrench);
}

// what solo_engine_set_base_wrench checks (solo_launch.h): the table's values in the engine's precision, and the configurations
// a block does not run with; 0, or the status - msg: the error text
extern "C" int solo_emu_push_validate(const double* table, int n, int dtype, char* msg, int msg_len) {
  std::string err;
  int rc;
  if (dtype == SOLO_F32) { const std::vector<float> v = conv<float>(table, (size_t)n * SOLO_WRENCH_WIDTH); rc = validate_base_wrench<float>(v.data(), n, &err); }
  else rc = validate_base_wrench<double>(table, n, &err);
  if (msg) snprintf(msg, (size_t)msg_len, "%s", err.c_str());
  return rc;
}
extern "C" int solo_emu_push_conflict(const SoloConfig* cfg, int sensing, char* msg, int msg_len) {
  std::string err;
  const int rc = base_wrench_conflict(*cfg, sensing != 0, &err);
  if (msg) snprintf(msg, (size_t)msg_len, "%s", err.c_str());
  return rc;
}

// make_plan / choose_kernel with a base wrench block (tests/test_push_host.py); wrench < 0: the call WITHOUT the new argument
extern "C" void solo_emu_push_plan(const SoloConfig* cfg, int dtype, int n, int resident, int ctl_active, int sensing, int k, uint32_t flags,
                                   int decimation, int state_terms, int actuators, int wrench, int32_t* out) {
  PlanInput in{n, dtype == SOLO_F32 ? sizeof(float) : sizeof(double), resident, cfg->steps_per_launch, cfg->rollout_streams,
               cfg->migrate_steps, ctl_active != 0, sensing != 0, k, flags};
  in.decimation = decimation;
  in.state_terms = state_terms != 0;
  in.actuators = actuators != 0;
  if (wrench >= 0) in.wrench = wrench != 0;
  const Plan p = make_plan(in);
  out[0] = p.S; out[1] = p.launches; out[2] = p.slices; out[3] = p.migrate;
}
extern "C" int solo_emu_push_choose_kernel(int sensing, int ctl_active, int settling, int resid, int has_queue, uint32_t flags, int decimation,
                                           int state_terms, int actuators, int wrench, int dtype, int32_t* out, char* name, int name_len) {
  const KernelId id = wrench < 0 ? choose_kernel(sensing != 0, ctl_active != 0, settling != 0, resid != 0, has_queue != 0, flags, decimation, state_terms != 0, actuators != 0)
                                 : choose_kernel(sensing != 0, ctl_active != 0, settling != 0, resid != 0, has_queue != 0, flags, decimation, state_terms != 0, actuators != 0, wrench != 0);
  out[0] = id.family; out[1] = id.full; out[2] = id.resid; out[3] = id.migrate; out[4] = id.ctl;
  return snprintf(name, (size_t)name_len, "%s", kernel_name(id, dtype == SOLO_F32 ? sizeof(float) : sizeof(double)).c_str());
}

// the offsets of KParams<T>'s members behind the tables (tests/test_push_abi.py: appending `wrench` moved none of them), and its size
extern "C" void solo_emu_push_kparams_offsets(int dtype, int64_t* out) {
  auto fill = [&](auto tag) {
    using K = KParams<decltype(tag)>;
    out[0] = (int64_t)offsetof(K, mu_base); out[1] = (int64_t)offsetof(K, ctl); out[2] = (int64_t)offsetof(K, contact);
    out[3] = (int64_t)offsetof(K, contact_traj); out[4] = (int64_t)offsetof(K, contact_traj_steps); out[5] = (int64_t)offsetof(K, decimation);
    out[6] = (int64_t)offsetof(K, term_value); out[7] = (int64_t)offsetof(K, term_fired); out[8] = (int64_t)offsetof(K, actuators);
    out[9] = (int64_t)offsetof(K, wrench); out[10] = (int64_t)sizeof(K);
  };
  if (dtype == SOLO_F32) fill(float()); else fill(double());
}
