// emu_terms_harness.cpp — TEST-ONLY: state terminations (solo_term_kernel: solo_step_body.h's kDecim and
// kTerms) on the CPU wave emulator, next to the kernels of emu_harness.cpp.  One emulated engine call - a single-step
// launch or a whole rollout under the engine's launch policy - with `decimation` physics steps per control step, the thresholds
// of solo_engine_set_term_values and the engine's term_fired record.  A program without a state kind runs the kernels
// emu_harness.cpp / emu_decimation_harness.cpp run (the twin of tests/test_emu_terms.py).  Built by the tests that use it with the
// flags of tests/emu/Makefile.
#include "emu_harness.cpp"

// single != 0: solo_engine_step (one launch of one control step; actions [n][12], or null: the robots' targets stay); else
// solo_engine_rollout_record over k control steps (actions [k][n][12]; obs_out [k][n][D], reward_out [k][n], done_out [k][n]).
// obs / reward / done / term_count / term_fired: the engine's view.  term_values: [SOLO_MAX_TERMS] or null = zeros.  name: the
// kernel the (last) launch ran.
extern "C" int solo_emu_terms_call(const SoloConfig* cfg, const SoloModel* mdl, const SoloProgram* prog, const SoloControl* ctl, int dtype,
                                   int n, int k, int single, int decimation, uint32_t flags, double* state, const double* snapshot,
                                   const double* actions, double* targets, const double* params, double* obs_out, double* reward_out,
                                   uint8_t* done_out, double* obs, double* reward, uint8_t* done, int32_t* term_count, double* stats,
                                   const double* term_values, uint8_t* term_fired, char* name, int name_len) {
  EmuCall c;
  c.cfg = cfg; c.mdl = mdl; c.prog = prog; c.ctl = ctl; c.n = n; c.k = single ? 1 : k; c.flags = flags; c.single = single != 0;
  c.state = state; c.snapshot = snapshot; c.actions = actions; c.targets = targets; c.params = params;
  c.obs_out = obs_out; c.reward_out = reward_out; c.done_out = done_out;
  c.obs = obs; c.reward = reward; c.done = done; c.term_count = term_count; c.stats = stats;
  c.decimation = decimation; c.term_values = term_values; c.term_fired = term_fired; c.kernel_name = name; c.kernel_name_len = name_len;
  return run(dtype, c);
}

// pack_program's validation alone (tests/test_terms_abi.py): 0, or the status it returns; msg: its error text
extern "C" int solo_emu_terms_validate(const SoloProgram* prog, char* msg, int msg_len) {
  static KParams<double> P;
  std::string err;
  const int rc = pack_program<double>(*prog, &P, &err);
  if (msg) snprintf(msg, (size_t)msg_len, "%s", err.c_str());
  return rc;
}

// make_plan / choose_kernel with a state termination in the program (tests/test_terms_host.py)
extern "C" void solo_emu_terms_plan(const SoloConfig* cfg, int dtype, int n, int resident, int ctl_active, int k, uint32_t flags, int decimation,
                                    int state_terms, int32_t* out) {
  PlanInput in{n, dtype == SOLO_F32 ? sizeof(float) : sizeof(double), resident, cfg->steps_per_launch, cfg->rollout_streams,
               cfg->migrate_steps, ctl_active != 0, false, k, flags};
  in.decimation = decimation;
  in.state_terms = state_terms != 0;
  const Plan p = make_plan(in);
  out[0] = p.S; out[1] = p.launches; out[2] = p.slices; out[3] = p.migrate;
}
extern "C" int solo_emu_terms_choose_kernel(int sensing, int ctl_active, int settling, int resid, int has_queue, uint32_t flags, int decimation,
                                            int state_terms, int dtype, int32_t* out, char* name, int name_len) {
  const KernelId id = choose_kernel(sensing != 0, ctl_active != 0, settling != 0, resid != 0, has_queue != 0, flags, decimation, state_terms != 0);
  out[0] = id.family; out[1] = id.full; out[2] = id.resid; out[3] = id.migrate; out[4] = id.ctl;
  return snprintf(name, (size_t)name_len, "%s", kernel_name(id, dtype == SOLO_F32 ? sizeof(float) : sizeof(double)).c_str());
}
