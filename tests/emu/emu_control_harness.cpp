// emu_control_harness.cpp — TEST-ONLY: the joint-control step kernels (solo_ctl_step_kernel, solo_step_body.h) on the CPU
// wave emulator, next to the position-control kernel of emu_harness.cpp.  Physics-only launches (stepSimulation) of
// `steps` fused steps; built by tests/test_emu_control.py with the flags of tests/emu/Makefile.
#include "emu_harness.cpp"

template <typename T>
static int run_ctl(const SoloConfig* cfg, const SoloModel* mdl, const SoloControl* ctl, int n, int steps, double* state,
                   const double* snapshot, const double* actions, double* targets, const double* params, double* stats) {
  std::string err;
  if (int rc = validate_model(*mdl, &err)) { fprintf(stderr, "emu: %s\n", err.c_str()); return rc; }
  static KParams<T> P;
  pack_params<T>(*cfg, *mdl, &P);
  // (as Engine::set_control packs it)
  P.ctl.mode = ctl->mode;
  for (int d = 0; d < SOLO_NUM_DOF; ++d) { P.ctl.kp[d] = (T)ctl->kp[d]; P.ctl.kd[d] = (T)ctl->kd[d]; }
  P.ctl.action_scale = (T)(ctl->mode == SOLO_CTRL_POSITION ? cfg->action_scale : ctl->action_scale);
  for (int j = 0; j < SOLO_NUM_JOINTS; ++j) P.ctl.reset_cmd[j] = (T)(ctl->mode == SOLO_CTRL_TORQUE ? 0.0 : cfg->settle_targets[j]);
  auto conv = [](const double* src, size_t cnt) {
    std::vector<T> v(cnt);
    for (size_t i = 0; i < cnt; ++i) v[i] = (T)src[i];
    return v;
  };
  std::vector<T> st = conv(state, (size_t)n * SOLO_STATE_STRIDE), snap = conv(snapshot, (size_t)n * SOLO_STATE_STRIDE);
  std::vector<T> tg = conv(targets, (size_t)n * SOLO_NUM_JOINTS), par = conv(params, (size_t)n * 4);
  std::vector<T> act;
  if (actions) act = conv(actions, (size_t)steps * n * SOLO_NUM_JOINTS);
  std::vector<uint8_t> done((size_t)n, 0);
  std::vector<int32_t> term((size_t)n * SOLO_MAX_TERMS, 0), cost((size_t)n, 0);
  KBuffers<T> B;
  B.terrain = nullptr; B.order = nullptr; B.cost = cost.data();
  B.state = st.data(); B.snapshot = snap.data(); B.targets = tg.data();
  B.actions = actions ? act.data() : nullptr; B.params = par.data();
  B.traj = nullptr; B.obs_inline = B.reward_inline = nullptr; B.obs_rec = B.reward_rec = nullptr;
  B.obs_rec_stride = B.reward_rec_stride = 0; B.obs_from = 0;
  B.view_obs = B.view_reward = nullptr; B.view_done = nullptr;
  B.done = done.data(); B.term_count = term.data(); B.stats = stats;
  B.num_envs = n; B.flags = SOLO_STEP_PHYSICS; B.env_base = 0; B.count = n; B.steps = steps;
  B.action_stride = (long long)n * SOLO_NUM_JOINTS; B.done_stride = 0;
  B.queue = nullptr; B.q_rings = 1; B.q_chunk = 0; B.fault = &g_fault; B.warm = nullptr;
  const KParams<T>* Pp = &P;
  for (int b = 0; b < n; ++b)
    WaveEmu::get().run_block(b, n, [&]() {
      if (ctl->mode == SOLO_CTRL_POSITION) solo_step_kernel<T, false, false>(Pp, B);
      else solo_ctl_step_kernel<T, false>(Pp, B);
    });
  for (size_t i = 0; i < st.size(); ++i) state[i] = (double)st[i];
  for (size_t i = 0; i < tg.size(); ++i) targets[i] = (double)tg[i];
  return 0;
}

extern "C" int solo_emu_ctl_rollout(const SoloConfig* cfg, const SoloModel* mdl, const SoloControl* ctl, int dtype, int n,
                                    int steps, double* state, const double* snapshot, const double* actions, double* targets,
                                    const double* params, double* stats) {
  if (dtype == SOLO_F32) return run_ctl<float>(cfg, mdl, ctl, n, steps, state, snapshot, actions, targets, params, stats);
  return run_ctl<double>(cfg, mdl, ctl, n, steps, state, snapshot, actions, targets, params, stats);
}
