// emu_decimation_harness.cpp — TEST-ONLY: control decimation (solo_decim_kernel: solo_step_body.h's kDecim) on the
// CPU wave emulator, next to the kernels of emu_harness.cpp.  One emulated engine call - a single-step launch or a whole
// rollout under the engine's launch policy - with `decimation` physics steps per control step; decimation = 1 runs the kernels
// emu_harness.cpp runs (the twin of tests/test_emu_decimation.py).  Built by tests/test_emu_decimation.py with the flags of
// tests/emu/Makefile.
#include "emu_harness.cpp"

// single != 0: solo_engine_step (one launch of one control step; actions [n][12]); else solo_engine_rollout_record over k control
// steps (actions [k][n][12]; obs_out [k][n][D], reward_out [k][n], done_out [k][n]).  obs / reward / done / term_count: the
// engine's view.  name: the kernel the (last) launch ran.
extern "C" int solo_emu_decim_call(const SoloConfig* cfg, const SoloModel* mdl, const SoloProgram* prog, const SoloControl* ctl, int dtype,
                                   int n, int k, int single, int decimation, uint32_t flags, double* state, const double* snapshot,
                                   const double* actions, double* targets, const double* params, double* obs_out, double* reward_out,
                                   uint8_t* done_out, double* obs, double* reward, uint8_t* done, int32_t* term_count, double* stats,
                                   char* name, int name_len) {
  EmuCall c;
  c.cfg = cfg; c.mdl = mdl; c.prog = prog; c.ctl = ctl; c.n = n; c.k = single ? 1 : k; c.flags = flags; c.single = single != 0;
  c.state = state; c.snapshot = snapshot; c.actions = actions; c.targets = targets; c.params = params;
  c.obs_out = obs_out; c.reward_out = reward_out; c.done_out = done_out;
  c.obs = obs; c.reward = reward; c.done = done; c.term_count = term_count; c.stats = stats;
  c.decimation = decimation; c.kernel_name = name; c.kernel_name_len = name_len;
  return run(dtype, c);
}

// make_plan / choose_kernel with a decimation (tests/test_decimation_host.py; emu_harness.cpp's entry points pass none)
extern "C" void solo_emu_decim_plan(const SoloConfig* cfg, int dtype, int n, int resident, int ctl_active, int sensing, int k, uint32_t flags,
                                    int decimation, int32_t* out) {
  PlanInput in{n, dtype == SOLO_F32 ? sizeof(float) : sizeof(double), resident, cfg->steps_per_launch, cfg->rollout_streams,
               cfg->migrate_steps, ctl_active != 0, sensing != 0, k, flags};
  in.decimation = decimation;
  const Plan p = make_plan(in);
  out[0] = p.S; out[1] = p.launches; out[2] = p.slices; out[3] = p.migrate;
}
extern "C" int solo_emu_decim_choose_kernel(int sensing, int ctl_active, int settling, int resid, int has_queue, uint32_t flags, int decimation,
                                            int dtype, int32_t* out, char* name, int name_len) {
  const KernelId id = choose_kernel(sensing != 0, ctl_active != 0, settling != 0, resid != 0, has_queue != 0, flags, decimation);
  out[0] = id.family; out[1] = id.full; out[2] = id.resid; out[3] = id.migrate; out[4] = id.ctl;
  return snprintf(name, (size_t)name_len, "%s", kernel_name(id, dtype == SOLO_F32 ? sizeof(float) : sizeof(double)).c_str());
}
