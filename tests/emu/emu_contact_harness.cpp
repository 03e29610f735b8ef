// emu_contact_harness.cpp — TEST-ONLY: the contact-sensing step kernels (solo_contact_kernel, solo_step_body.h with
// SOLO_BODY_CONTACT) on the CPU wave emulator.  Physics-only launches (stepSimulation) of `steps` fused steps in position,
// torque or PD control, on the flat plane or a heightfield; returns the contact record of the last step.  Built by
// tests/test_emu_contact.py with the flags of tests/emu/Makefile.
#include "emu_harness.cpp"

template <typename T>
static int run_contact(const SoloConfig* cfg, const SoloModel* mdl, const SoloControl* ctl, const SoloTerrain* terrain, int n,
                       int steps, double* state, const double* actions, double* targets, const double* params, double* stats,
                       double* contact) {
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
  // (as Engine::set_terrain packs it)
  std::vector<T> heights;
  if (terrain) {
    heights = conv(terrain->heights, (size_t)terrain->nx * terrain->ny);
    P.c.terr_nx = terrain->nx; P.c.terr_ny = terrain->ny;
    P.c.terr_inv_cell = (T)(1.0 / terrain->cell);
    P.c.terr_ox = (T)terrain->origin[0]; P.c.terr_oy = (T)terrain->origin[1];
  }
  std::vector<T> st = conv(state, (size_t)n * SOLO_STATE_STRIDE), snap = st;
  std::vector<T> tg = conv(targets, (size_t)n * SOLO_NUM_JOINTS), par = conv(params, (size_t)n * 4);
  std::vector<T> act;
  if (actions) act = conv(actions, (size_t)steps * n * SOLO_NUM_JOINTS);
  std::vector<T> rec((size_t)n * SOLO_MAX_SPHERES * SOLO_CONTACT_WIDTH, T(0));
  P.contact = rec.data();
  P.contact_traj = nullptr;
  P.contact_traj_steps = 0;
  std::vector<uint8_t> done((size_t)n, 0);
  std::vector<int32_t> term((size_t)n * SOLO_MAX_TERMS, 0), cost((size_t)n, 0);
  KBuffers<T> B;
  B.terrain = terrain ? heights.data() : nullptr; B.order = nullptr; B.cost = cost.data();
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
      if (ctl->mode == SOLO_CTRL_POSITION) solo_contact_kernel<T, false, false>(Pp, B);
      else solo_contact_kernel<T, false, true>(Pp, B);
    });
  for (size_t i = 0; i < st.size(); ++i) state[i] = (double)st[i];
  for (size_t i = 0; i < tg.size(); ++i) targets[i] = (double)tg[i];
  for (size_t i = 0; i < rec.size(); ++i) contact[i] = (double)rec[i];
  return 0;
}

extern "C" int solo_emu_contact_rollout(const SoloConfig* cfg, const SoloModel* mdl, const SoloControl* ctl, const SoloTerrain* terrain,
                                        int dtype, int n, int steps, double* state, const double* actions, double* targets,
                                        const double* params, double* stats, double* contact) {
  if (dtype == SOLO_F32) return run_contact<float>(cfg, mdl, ctl, terrain, n, steps, state, actions, targets, params, stats, contact);
  return run_contact<double>(cfg, mdl, ctl, terrain, n, steps, state, actions, targets, params, stats, contact);
}
