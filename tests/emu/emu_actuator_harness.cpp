// emu_actuator_harness.cpp — TEST-ONLY: actuator randomisation (solo_act_kernel: solo_step_body.h's kAct) on the CPU wave
// emulator, next to the kernels of emu_harness.cpp.  One emulated engine call - a single-step launch or a whole rollout under the
// engine's launch policy - with the engine's actuator block [n][SOLO_ACTUATOR_WIDTH].  EmuCall has no field for the block, so the
// runner that wires it lives here (run_act: emu_harness.cpp's run with KParams::actuators, PlanInput::actuators and
// choose_kernel's last argument); a call WITHOUT a block goes through emu_harness.cpp's own runner - the kernels of before, the
// twin of tests/test_emu_actuators.py.  Built by the tests that use it with the flags of tests/emu/Makefile.
#include "emu_harness.cpp"

template <typename T>
static int run_act(const EmuCall& c, const double* actuators) {
  const SoloConfig* cfg = c.cfg;
  const int n = c.n, k = c.k;
  const uint32_t flags = c.flags;
  std::string err;
  if (int rc = validate_model(*c.mdl, &err)) { fprintf(stderr, "emu: %s\n", err.c_str()); return rc; }
  // (what solo_engine_set_actuators checks before a block goes on)
  std::vector<T> act_block = conv<T>(actuators, (size_t)n * SOLO_ACTUATOR_WIDTH);
  if (int rc = actuators_conflict(*cfg, c.contact != nullptr, &err)) { fprintf(stderr, "emu: %s\n", err.c_str()); return rc; }
  if (int rc = validate_actuators<T>(act_block.data(), n, &err)) { fprintf(stderr, "emu: %s\n", err.c_str()); return rc; }
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
  const bool ctl_active = c.ctl != nullptr && c.ctl->mode != SOLO_CTRL_POSITION;
  const bool state_terms = c.prog != nullptr && program_reads_state(*c.prog);
  PlanInput in{n, sizeof(T), n, cfg->steps_per_launch, cfg->rollout_streams, cfg->migrate_steps, ctl_active, false, k, flags};
  in.decimation = c.decimation;
  in.state_terms = state_terms;
  in.actuators = true;
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
    const KernelId id = choose_kernel(false, ctl_active, false, false, false, flags, c.decimation, state_terms, true);
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

// single != 0: solo_engine_step (one launch of one control step; actions [n][12], or null: the robots' targets stay); else
// solo_engine_rollout_record over k control steps (actions [k][n][12]; obs_out [k][n][D], reward_out [k][n], done_out [k][n]).
// obs / reward / done / term_count / term_fired: the engine's view.  actuators: the block [n][SOLO_ACTUATOR_WIDTH], or null = off.
// name: the kernel the (last) launch ran.
extern "C" int solo_emu_act_call(const SoloConfig* cfg, const SoloModel* mdl, const SoloProgram* prog, const SoloControl* ctl, int dtype,
                                 int n, int k, int single, int decimation, uint32_t flags, double* state, const double* snapshot,
                                 const double* actions, double* targets, const double* params, double* obs_out, double* reward_out,
                                 uint8_t* done_out, double* obs, double* reward, uint8_t* done, int32_t* term_count, double* stats,
                                 const double* term_values, uint8_t* term_fired, const double* actuators, char* name, int name_len) {
  EmuCall c;
  c.cfg = cfg; c.mdl = mdl; c.prog = prog; c.ctl = ctl; c.n = n; c.k = single ? 1 : k; c.flags = flags; c.single = single != 0;
  c.state = state; c.snapshot = snapshot; c.actions = actions; c.targets = targets; c.params = params;
  c.obs_out = obs_out; c.reward_out = reward_out; c.done_out = done_out;
  c.obs = obs; c.reward = reward; c.done = done; c.term_count = term_count; c.stats = stats;
  c.decimation = decimation; c.term_values = term_values; c.term_fired = term_fired; c.kernel_name = name; c.kernel_name_len = name_len;
  if (actuators == nullptr) return run(dtype, c);
  // (a launch the actuator kernels do not take - it neither steps the physics nor evaluates a state termination - keeps its kernel)
  const bool state_terms = prog != nullptr && program_reads_state(*prog);
  if (choose_kernel(false, false, false, false, false, flags, decimation, state_terms, true).family != KERNEL_ACT) return run(dtype, c);
  return dtype == SOLO_F32 ? run_act<float>(c, actuators) : run_act<double>(c, actuators);
}

// what solo_engine_set_actuators checks (solo_launch.h): the table's values in the engine's precision, and the configurations a
// block does not run with; 0, or the status - msg: the error text
extern "C" int solo_emu_act_validate(const double* table, int n, int dtype, char* msg, int msg_len) {
  std::string err;
  int rc;
  if (dtype == SOLO_F32) { const std::vector<float> v = conv<float>(table, (size_t)n * SOLO_ACTUATOR_WIDTH); rc = validate_actuators<float>(v.data(), n, &err); }
  else rc = validate_actuators<double>(table, n, &err);
  if (msg) snprintf(msg, (size_t)msg_len, "%s", err.c_str());
  return rc;
}
extern "C" int solo_emu_act_conflict(const SoloConfig* cfg, int sensing, char* msg, int msg_len) {
  std::string err;
  const int rc = actuators_conflict(*cfg, sensing != 0, &err);
  if (msg) snprintf(msg, (size_t)msg_len, "%s", err.c_str());
  return rc;
}

// make_plan / choose_kernel with an actuator block (tests/test_actuators_host.py); actuators < 0: the call WITHOUT the new argument
extern "C" void solo_emu_act_plan(const SoloConfig* cfg, int dtype, int n, int resident, int ctl_active, int sensing, int k, uint32_t flags,
                                  int decimation, int state_terms, int actuators, int32_t* out) {
  PlanInput in{n, dtype == SOLO_F32 ? sizeof(float) : sizeof(double), resident, cfg->steps_per_launch, cfg->rollout_streams,
               cfg->migrate_steps, ctl_active != 0, sensing != 0, k, flags};
  in.decimation = decimation;
  in.state_terms = state_terms != 0;
  if (actuators >= 0) in.actuators = actuators != 0;
  const Plan p = make_plan(in);
  out[0] = p.S; out[1] = p.launches; out[2] = p.slices; out[3] = p.migrate;
}
extern "C" int solo_emu_act_choose_kernel(int sensing, int ctl_active, int settling, int resid, int has_queue, uint32_t flags, int decimation,
                                          int state_terms, int actuators, int dtype, int32_t* out, char* name, int name_len) {
  const KernelId id = actuators < 0 ? choose_kernel(sensing != 0, ctl_active != 0, settling != 0, resid != 0, has_queue != 0, flags, decimation, state_terms != 0)
                                    : choose_kernel(sensing != 0, ctl_active != 0, settling != 0, resid != 0, has_queue != 0, flags, decimation, state_terms != 0, actuators != 0);
  out[0] = id.family; out[1] = id.full; out[2] = id.resid; out[3] = id.migrate; out[4] = id.ctl;
  return snprintf(name, (size_t)name_len, "%s", kernel_name(id, dtype == SOLO_F32 ? sizeof(float) : sizeof(double)).c_str());
}
