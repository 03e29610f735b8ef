// emu_harness.cpp — TEST-ONLY: runs the product kernel source (solo_step_kernel.h) on the CPU
// wave emulator.  Built by tests/emu/Makefile into libsolo_emu.so and driven from pytest.
#include "wave_emu.h"

#ifdef SOLO_EMU_TRACE
// DIAGNOSTIC variant (make trace): records every lane's impulse / candidate after each Gauss-Seidel
// sweep of the LAST emulated robot-step, for tools/analyse_slow_steps.py
static double g_trace_lam[64][64], g_trace_v[64][64];
static unsigned long long g_trace_pend[64];
static int g_trace_sweeps = 0;
#define SOLO_PGS_SWEEP_HOOK(it, pend, lam, v)                                       \
  do {                                                                              \
    if ((it) < 64) {                                                                \
      g_trace_lam[(it)][solo::lane_id()] = (double)(lam);                           \
      g_trace_v[(it)][solo::lane_id()] = (double)(v);                               \
      g_trace_pend[(it)] = (pend);                                                  \
      g_trace_sweeps = (it) + 1;                                                    \
    }                                                                               \
  } while (0)
extern "C" int solo_emu_trace(double* lam, double* v, unsigned long long* pend) {
  for (int i = 0; i < 64 * 64; ++i) { lam[i] = (&g_trace_lam[0][0])[i]; v[i] = (&g_trace_v[0][0])[i]; }
  for (int i = 0; i < 64; ++i) pend[i] = g_trace_pend[i];
  return g_trace_sweeps;
}
#endif

#include "../../gym_solo_amd/csrc/solo_step_kernel.h"
#include "../../gym_solo_amd/csrc/solo_launch.h"

#include <string>
#include <vector>

using namespace solo;

// Gauss-Seidel sweeps each robot ran in the last emulated launch (view.cost of the engine)
static std::vector<int32_t> g_last_cost;
static int32_t g_fault = 0;      // the engine's fault word (KBuffers::fault), as the emulator sees it
static int g_sabotage = 0;
extern "C" int solo_emu_last_cost(int32_t* out, int n) {
  const int m = (int)g_last_cost.size() < n ? (int)g_last_cost.size() : n;
  for (int i = 0; i < m; ++i) out[i] = g_last_cost[i];
  return m;
}

// the step kernel's workgroup -> robot map (solo_kernel_params.h), for tests/test_emu_kernel.py
extern "C" int solo_emu_xcd_contiguous(int b, int count) { return solo::xcd_contiguous(b, count); }

// One emulated engine call over the driver's buffers (doubles, whatever the kernel's precision; null = not used).
// single: solo_engine_step - one launch of one step; else a rollout of k steps under the engine's launch policy (every robot
// has a wave slot: the emulator has no such limit).  obs_out / reward_out / done_out: the [k][n][.] buffers of a recording
// rollout; obs / reward / done: the engine's view.  ctl: the joint control mode in force (null = position control);
// contact: contact sensing is on, and this is its record [n][16][4].  decimation: physics steps per control step (what
// solo_engine_set_decimation uploads; k counts control steps); term_values: what solo_engine_set_term_values uploads
// ([SOLO_MAX_TERMS], null = zeros) and term_fired [n]: the engine's record of which termination fired.  A decimation > 1 or a
// program with a state termination selects the decimation / termination kernels, whose launches never migrate.
// kernel_name (kernel_name_len bytes, or null): receives the name of the kernel the last launch ran.
struct EmuCall {
  const SoloConfig* cfg = nullptr;
  const SoloModel* mdl = nullptr;
  const SoloProgram* prog = nullptr;
  const SoloControl* ctl = nullptr;
  const SoloTerrain* terrain = nullptr;
  int n = 0, k = 1;
  uint32_t flags = SOLO_STEP_PHYSICS;
  bool single = false;
  double* state = nullptr;
  const double* snapshot = nullptr;
  const double* actions = nullptr;
  double* targets = nullptr;
  const double* params = nullptr;
  double *obs_out = nullptr, *reward_out = nullptr;
  uint8_t* done_out = nullptr;
  double *obs = nullptr, *reward = nullptr;
  uint8_t* done = nullptr;
  int32_t* term_count = nullptr;
  double *stats = nullptr, *warm = nullptr, *contact = nullptr;
  int decimation = 1;
  const double* term_values = nullptr;
  uint8_t* term_fired = nullptr;
  char* kernel_name = nullptr;
  int kernel_name_len = 0;
};

template <typename T>
static std::vector<T> conv(const double* src, size_t cnt) {
  std::vector<T> v(cnt, T(0));
  if (src) for (size_t i = 0; i < cnt; ++i) v[i] = (T)src[i];
  return v;
}
template <typename T>
static void back(double* dst, const std::vector<T>& v) {
  if (dst) for (size_t i = 0; i < v.size(); ++i) dst[i] = (double)v[i];
}

template <typename T>
static int run(const EmuCall& c) {
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
  if (c.ctl) pack_control<T>(*cfg, *c.ctl, &P);
  pack_terrain<T>(c.terrain, &P);
  P.decimation = c.decimation;
  for (int t = 0; t < SOLO_MAX_TERMS; ++t) P.term_value[t] = c.term_values ? (T)c.term_values[t] : T(0);
  P.term_fired = c.term_fired;
  const bool ctl_active = c.ctl != nullptr && c.ctl->mode != SOLO_CTRL_POSITION, sensing = c.contact != nullptr;
  const bool state_terms = c.prog != nullptr && program_reads_state(*c.prog);
  PlanInput in{n, sizeof(T), n, cfg->steps_per_launch, cfg->rollout_streams, cfg->migrate_steps, ctl_active, sensing, k, flags};
  in.decimation = c.decimation;
  in.state_terms = state_terms;
  const Plan plan = c.single ? Plan{1, 1, 1, 0} : make_plan(in);
  // the engine's buffers ...
  const size_t ns = (size_t)n * SOLO_STATE_STRIDE;
  std::vector<T> st = conv<T>(c.state, ns), snap = conv<T>(c.snapshot ? c.snapshot : c.state, ns);
  std::vector<T> tg = conv<T>(c.targets, (size_t)n * SOLO_NUM_JOINTS), par = conv<T>(c.params, (size_t)n * 4);
  std::vector<T> ob = conv<T>(c.obs, (size_t)n * (D > 0 ? D : 1)), rew = conv<T>(c.reward, (size_t)n);
  std::vector<T> wrm = conv<T>(c.warm, c.warm != nullptr && cfg->solver_warm_start > 0 ? (size_t)n * 64 : 0);
  std::vector<T> terr = conv<T>(c.terrain ? c.terrain->heights : nullptr, c.terrain ? (size_t)c.terrain->nx * c.terrain->ny : 0);
  std::vector<T> rec = conv<T>(c.contact, sensing ? (size_t)n * SOLO_MAX_SPHERES * SOLO_CONTACT_WIDTH : 0);
  std::vector<uint8_t> done_own(c.done ? 0 : (size_t)n, 0);
  std::vector<int32_t> term_own(c.term_count ? 0 : (size_t)n * SOLO_MAX_TERMS, 0);
  g_last_cost.assign((size_t)n, 0);
  // ... its scratch, at EXACTLY the sizes the engine allocates (solo_launch.h: a wiring error is a heap overflow here) ...
  const bool records = leaves_records(flags);
  std::vector<T> traj(records ? record_reals(n, plan.S) : 0), foot(sensing && records ? foot_force_reals(n, plan.S) : 0);
  std::vector<int32_t> queue(queue_ints(n, plan));
  P.contact = sensing ? rec.data() : nullptr;
  P.contact_traj = foot.empty() ? nullptr : foot.data();
  P.contact_traj_steps = foot.empty() ? 0 : plan.S;
  // ... and the caller's: actions [k][n][12], the outputs of a recording rollout
  std::vector<T> act = conv<T>(c.actions, c.actions ? (size_t)k * n * SOLO_NUM_JOINTS : 0);
  std::vector<T> ob_out((flags & SOLO_STEP_OBS) && c.obs_out ? (size_t)k * n * D : 0), rew_out((flags & SOLO_STEP_REWARD) && c.reward_out ? (size_t)k * n : 0);
  EngineBuffers<T> e;
  e.state = st.data(); e.snapshot = snap.data(); e.targets = tg.data(); e.params = par.data(); e.obs = ob.data(); e.reward = rew.data();
  e.done = c.done ? c.done : done_own.data(); e.term_count = c.term_count ? c.term_count : term_own.data(); e.stats = c.stats;
  e.terrain = terr.empty() ? nullptr : terr.data(); e.order = nullptr; e.cost = g_last_cost.data();
  e.warm = wrm.empty() ? nullptr : wrm.data(); e.fault = &g_fault;
  e.traj = traj.empty() ? nullptr : traj.data(); e.traj_steps = plan.S; e.queue = queue.empty() ? nullptr : queue.data(); e.queue_len = queue.size();
  e.n = n; e.obs_dim = D;
  const RolloutArgs<T> args{act.empty() ? nullptr : act.data(), (!c.single && !act.empty()) ? (long long)n * SOLO_NUM_JOINTS : 0, k, flags,
                            ob_out.empty() ? nullptr : ob_out.data(), rew_out.empty() ? nullptr : rew_out.data(),
                            (flags & SOLO_STEP_DONE) ? c.done_out : nullptr};
  const KParams<T>* Pp = &P;
  std::string launched;
  // the launches in the engine's issue order, one after the other; per launch one emulated wavefront per robot, one after the
  // other too (so the first wave of a migrating launch drains every ring it can reach)
  const int rc = for_each_launch(plan, n, k, [&](const Launch& l) {
    KBuffers<T> B;
    QueueInit q;
    if (!wire_launch(plan, args, e, l, &B, &q)) { fprintf(stderr, "emu: the migration queue of a launch does not fit its slice's region\n"); return (int)SOLO_ERR_INVALID_ARG; }
    if (q.ints > 0) {
      if (l.count == 16) B.q_rings = q.rings = 8;  // (16 robots: eight rings of two, so that the CPU suite walks several rings too)
      for (size_t i = 0; i < q.ints; ++i) migration_queue_init(q.q, i, q.lo, q.count, q.rings, q.steps, q.chunk, q.order);
      // FAULT INJECTION (tests/test_emu_kernel.py): ring 0's tail starts one slot too far - its first chunk-1 slot is never
      // published, the wave that holds that slot's ticket must give up (bounded wait), count itself and set the fault word
      if (g_sabotage) q.q[16] += 1;
    }
    const KernelId id = choose_kernel(sensing, ctl_active, false, cfg->solver_residual_threshold > 0, B.queue != nullptr, flags, c.decimation, state_terms);
    if ((id.family == KERNEL_DECIM || id.family == KERNEL_TERM) && q.ints > 0) return (int)SOLO_ERR_INVALID_ARG;   // (these launches never migrate)
    launched = kernel_name(id, sizeof(T));
    with_step_kernel<T>(id, [&](StepKernel<T> kernel) {
      for (int b = 0; b < l.count; ++b) WaveEmu::get().run_block(b, l.count, [&]() { kernel(Pp, B); });
    });
    return 0;
  });
  if (rc) return rc;
  if (c.kernel_name) snprintf(c.kernel_name, (size_t)c.kernel_name_len, "%s", launched.c_str());
  // (what Engine::rollout copies into the view when the last launch could not write it there)
  if (!c.single && tail_needs_copy<T>(plan, k, flags)) {
    if (args.obs_out) for (size_t i = 0; i < (size_t)n * D; ++i) ob[i] = ob_out[(size_t)(k - 1) * n * D + i];
    if (args.reward_out) for (size_t i = 0; i < (size_t)n; ++i) rew[i] = rew_out[(size_t)(k - 1) * n + i];
    if (args.done_out) for (size_t i = 0; i < (size_t)n; ++i) e.done[i] = args.done_out[(size_t)(k - 1) * n + i];
  }
  back(c.state, st); back(c.targets, tg); back(c.warm, wrm); back(c.contact, rec);
  if (flags & SOLO_STEP_OBS) { back(c.obs, ob); back(c.obs_out, ob_out); }
  if (flags & SOLO_STEP_REWARD) { back(c.reward, rew); back(c.reward_out, rew_out); }
  return 0;
}

static int run(int dtype, const EmuCall& c) { return dtype == SOLO_F32 ? run<float>(c) : run<double>(c); }

// solo_engine_step: one launch of one step; obs [n][D], reward [n], done [n] are the engine's view
extern "C" int solo_emu_step(const SoloConfig* cfg, const SoloModel* mdl, const SoloProgram* prog,
                             int dtype, int n, double* state, const double* snapshot,
                             const double* actions, double* targets, const double* params,
                             double* obs, double* reward, uint8_t* done, int32_t* term_count,
                             double* stats, uint32_t flags, const SoloTerrain* terrain, double* warm) {
  EmuCall c;
  c.cfg = cfg; c.mdl = mdl; c.prog = prog; c.terrain = terrain; c.n = n; c.flags = flags; c.single = true;
  c.state = state; c.snapshot = snapshot; c.actions = actions; c.targets = targets; c.params = params;
  c.obs = obs; c.reward = reward; c.done = done; c.term_count = term_count; c.stats = stats; c.warm = warm;
  return run(dtype, c);
}

// solo_engine_rollout / solo_engine_rollout_record: a WHOLE rollout of k steps, cut into launches and slices by the engine's
// launch policy.  actions [k][n][12]; obs_out [k][n][D], reward_out [k][n], done_out [k][n] (each may be null: not recorded);
// obs / reward / done: the engine's view, which ends up with the last step's outputs
extern "C" int solo_emu_rollout(const SoloConfig* cfg, const SoloModel* mdl, const SoloProgram* prog,
                                int dtype, int n, int k, double* state, const double* snapshot,
                                const double* actions, double* targets, const double* params,
                                double* obs_out, double* reward_out, uint8_t* done_out,
                                double* obs, double* reward, uint8_t* done, int32_t* term_count,
                                double* stats, uint32_t flags, const SoloTerrain* terrain, double* warm) {
  EmuCall c;
  c.cfg = cfg; c.mdl = mdl; c.prog = prog; c.terrain = terrain; c.n = n; c.k = k; c.flags = flags;
  c.state = state; c.snapshot = snapshot; c.actions = actions; c.targets = targets; c.params = params;
  c.obs_out = obs_out; c.reward_out = reward_out; c.done_out = done_out;
  c.obs = obs; c.reward = reward; c.done = done; c.term_count = term_count; c.stats = stats; c.warm = warm;
  return run(dtype, c);
}

// ---- the launch planning itself (solo_launch.h), for tests/test_launch_plan.py --------------------------------------------
// make_plan: out = {S, launches, slices, migrate}
extern "C" void solo_emu_plan(const SoloConfig* cfg, int dtype, int n, int resident, int ctl_active, int sensing, int k, uint32_t flags, int32_t* out) {
  const Plan p = make_plan(PlanInput{n, dtype == SOLO_F32 ? sizeof(float) : sizeof(double), resident, cfg->steps_per_launch, cfg->rollout_streams,
                                     cfg->migrate_steps, ctl_active != 0, sensing != 0, k, flags});
  out[0] = p.S; out[1] = p.launches; out[2] = p.slices; out[3] = p.migrate;
}
// choose_kernel: out = {family, full, resid, migrate, ctl}; returns the length of the rendered name written to `name`
extern "C" int solo_emu_choose_kernel(int sensing, int ctl_active, int settling, int resid, int has_queue, uint32_t flags, int dtype, int32_t* out,
                                      char* name, int name_len) {
  const KernelId id = choose_kernel(sensing != 0, ctl_active != 0, settling != 0, resid != 0, has_queue != 0, flags);
  out[0] = id.family; out[1] = id.full; out[2] = id.resid; out[3] = id.migrate; out[4] = id.ctl;
  return snprintf(name, (size_t)name_len, "%s", kernel_name(id, dtype == SOLO_F32 ? sizeof(float) : sizeof(double)).c_str());
}
// the queue ints a launch of `steps` steps of `count` robots needs, under a plan of S steps per launch migrating every
// `migrate`; *region: the ints its slice's region holds
extern "C" long long solo_emu_queue_ints(int S, int migrate, int steps, int count, long long* region) {
  const Plan p{S, 1, 1, migrate};
  *region = (long long)kQueueHeader + (long long)count * queue_slots_per_robot(p);
  return (long long)migration_queue_ints(count, steps, migration_chunk_steps(steps, migrate));
}
// ... swept over every S <= max_S, migrate <= S and steps <= S: the number of launches whose queue does not fit
extern "C" long long solo_emu_queue_sweep(int max_S, int count, long long* cases) {
  long long misfits = 0, region;
  *cases = 0;
  for (int S = 1; S <= max_S; ++S)
    for (int m = 1; m <= S; ++m)
      for (int steps = 1; steps <= S; ++steps, ++*cases) misfits += solo_emu_queue_ints(S, m, steps, count, &region) > region;
  return misfits;
}

// the fault word a wave sets when it gives up waiting for a ring slot (and clears it); fault injection on / off
extern "C" int solo_emu_take_fault(void) { const int f = g_fault; g_fault = 0; return f; }
extern "C" void solo_emu_sabotage_queue(int on) { g_sabotage = on; }
