// emu_control_harness.cpp — TEST-ONLY: the joint-control step kernels (solo_ctl_step_kernel, solo_step_body.h) on the CPU
// wave emulator, next to the position-control kernel of emu_harness.cpp.  Physics-only rollouts (stepSimulation) of
// `steps` steps in the given control mode; built by tests/test_emu_control.py with the flags of tests/emu/Makefile.
#include "emu_harness.cpp"

extern "C" int solo_emu_ctl_rollout(const SoloConfig* cfg, const SoloModel* mdl, const SoloControl* ctl, int dtype, int n,
                                    int steps, double* state, const double* snapshot, const double* actions, double* targets,
                                    const double* params, double* stats) {
  EmuCall c;
  c.cfg = cfg; c.mdl = mdl; c.ctl = ctl; c.n = n; c.k = steps;
  c.state = state; c.snapshot = snapshot; c.actions = actions; c.targets = targets; c.params = params; c.stats = stats;
  return run(dtype, c);
}
