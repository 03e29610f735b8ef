// emu_contact_harness.cpp — TEST-ONLY: the contact-sensing step kernels (solo_contact_kernel: solo_step_body.h's
// kContact) on the CPU wave emulator.  Physics-only rollouts (stepSimulation) of `steps` steps in position,
// torque or PD control, on the flat plane or a heightfield; returns the contact record of the last step.  Built by
// tests/test_emu_contact.py with the flags of tests/emu/Makefile.
#include "emu_harness.cpp"

extern "C" int solo_emu_contact_rollout(const SoloConfig* cfg, const SoloModel* mdl, const SoloControl* ctl, const SoloTerrain* terrain,
                                        int dtype, int n, int steps, double* state, const double* actions, double* targets,
                                        const double* params, double* stats, double* contact) {
  EmuCall c;
  c.cfg = cfg; c.mdl = mdl; c.ctl = ctl; c.terrain = terrain; c.n = n; c.k = steps;
  c.state = state; c.actions = actions; c.targets = targets; c.params = params; c.stats = stats; c.contact = contact;
  return run(dtype, c);
}
