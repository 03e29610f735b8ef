// solo_engine.hip — implementation of the C-ABI in include/solo_engine.h for gfx950.
// Host logic only: buffer ownership, allocation, streams, events, validation, parameter upload.  The arithmetic is in
// solo_step_kernel.h; what is launched, in which order and on which buffers is planned in solo_launch.h, which the CPU
// emulator compiles too.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

// the GPU build constructs the f64 Delassus columns two per pass (solo_wave_ops.h: ColumnBank<double>::build_pair);
// -DSOLO_F64_PAIR_BUILD=0: the single-column build, the twin tests/test_gpu_pair_build.py compares it with bit for bit
#ifndef SOLO_F64_PAIR_BUILD
#define SOLO_F64_PAIR_BUILD 1
#endif
// ... and four per pass in the steps with at most 16 live rows (ColumnBank<double>::build_quad; it rides on the paired build's
// operand hand-over, so it is off wherever that is); -DSOLO_F64_QUAD_BUILD=0: the pair-only twin
// tests/test_gpu_quad_build.py compares it with bit for bit
#ifndef SOLO_F64_QUAD_BUILD
#define SOLO_F64_QUAD_BUILD SOLO_F64_PAIR_BUILD
#endif
#include "solo_wave_ops.h"
#include "solo_pgs_gfx950.h"  // (defines SOLO_PGS_GFX950: the f32 Gauss-Seidel loop of the step kernel in assembly)
#include "solo_step_kernel.h"
#include "solo_launch.h"

// TRANSLATION UNITS (round 4).  The product library is this file compiled TWICE (Makefile): -DSOLO_TU_F32 = the C ABI and
// the f32 engine, -DSOLO_TU_F64 = the f64 engine alone, with `-mllvm -disable-machine-licm`: the f64 step kernel lives on
// exactly 128 VGPRs (four waves per SIMD since round 5; round 4: 168 and three), and what machine LICM hoists out of its step loop (LDS base addresses, flags)
// it then has to SPILL - scratch reloads inside the step, each behind an s_waitcnt vmcnt(0) that also waits for the
// step's freshly issued action load.  Without the pass: 0 VGPR spills, +3 ... 5 % (profiles/round4_ab.log); the f32
// kernels (0 spills either way) are 1 ... 3 % faster WITH it, hence two units.  Without either macro (the test and
// diagnostic builds) everything is one unit, as before.
namespace solo_engine_detail {

struct EngineBase {
  virtual ~EngineBase() {}
  virtual int set_program(const SoloProgram* p) = 0;
  virtual int reset(const uint8_t* mask, hipStream_t s) = 0;
  virtual int settle(hipStream_t s) = 0;
  virtual int set_targets(const void* a, hipStream_t s) = 0;
  virtual int step(const void* a, uint32_t flags, hipStream_t s) = 0;
  virtual int rollout(const void* a, int k, uint32_t flags, void* obs_out, void* reward_out, void* done_out, hipStream_t s) = 0;
  virtual int view(SoloStateView* v) = 0;
  virtual int set_params(int which, const void* p, hipStream_t s) = 0;
  virtual int set_terrain(const SoloTerrain* t, hipStream_t s) = 0;
  virtual int set_order(const int32_t* order, hipStream_t s) = 0;
  virtual int time_step(const void* a, uint32_t flags, int reps, hipStream_t s, double* ms) = 0;
  virtual int time_rollout(const void* a, int k, uint32_t flags, void* obs_out, void* reward_out, void* done_out, hipStream_t s, double* ms) = 0;
  virtual int plan(int k, SoloLaunchPlan* out) = 0;
  virtual int reserve(int k, uint32_t flags) = 0;
  virtual int check_fault() = 0;
  virtual const char* kernel_name() = 0;
  virtual int debug_progress(int32_t* host) = 0;
  virtual int set_control(const SoloControl* c, hipStream_t s) = 0;
  virtual int get_control(SoloControl* out) = 0;
  virtual int set_contact_sensing(int32_t enable, hipStream_t s) = 0;
  virtual int get_contacts(void** out) = 0;
  virtual int set_decimation(int32_t d) = 0;
  virtual int get_decimation(int32_t* out) = 0;
  virtual int set_term_values(const double* values) = 0;
  virtual int get_term_fired(void** out) = 0;
  virtual int set_actuators(const void* per_env, hipStream_t s) = 0;
  virtual int get_actuators(void** out) = 0;
  virtual int set_base_wrench(const void* per_env, hipStream_t s) = 0;
  virtual int get_base_wrench(void** out) = 0;
  std::string err;
};

#define HIP_TRY(expr)                                                                 \
  do {                                                                                \
    hipError_t e_ = (expr);                                                           \
    if (e_ != hipSuccess) {                                                           \
      err = std::string(#expr) + ": " + hipGetErrorString(e_);                        \
      return SOLO_ERR_HIP;                                                            \
    }                                                                                 \
  } while (0)

constexpr size_t kStatsBytes = (size_t)SOLO_STATS_SHARDS * SOLO_STATS_WIDTH * sizeof(double);

template <typename T>
struct Engine final : EngineBase {
  SoloConfig cfg;
  SoloModel model;
  int n = 0, device = 0, obs_dim = 0;
  bool have_program = false;
  SoloControl control{};      // the joint control mode in force (solo_engine_set_control); hparams.ctl is its packed form
  bool settling = false;      // (the settle loop is position-controlled in every mode)
  solo::KParams<T> hparams;
  solo::KParams<T>* dparams = nullptr;
  T *state = nullptr, *snapshot = nullptr, *targets = nullptr, *params = nullptr, *obs = nullptr,
    *reward = nullptr, *settle_actions = nullptr, *warm = nullptr;  // (warm: the warm-start cache [N][64], SoloStateView::warm)
  // per-launch scratch: the step records [N][S][32] a fused launch leaves for its own output epilogue
  // (S = steps per launch)
  T* traj = nullptr;
  uint8_t* done = nullptr;
  int32_t* term_count = nullptr;
  int32_t *order = nullptr, *cost = nullptr;  // launch order (null = identity), per-robot sweeps of the last launch
  bool use_order = false;
  double* stats = nullptr;
  T* terrain = nullptr;
  int32_t* queue = nullptr;   // robot-migration queues of the launches in flight (one region per rollout slice), or null
  size_t queue_ints = 0;      // (allocated lazily, for the geometry of the rollout at hand)
  int traj_steps = 0;         // steps the record scratch `traj` holds per robot (allocated lazily)
  // progress pacing (solo_launch.h): the counters the waves of a paced rollout's segmented launches rank themselves with - ONE block
  // for all slices, allocated with the scratch of the first fused plan, zeroed on the caller's stream in front of every paced rollout
  int32_t* progress = nullptr;
  int32_t* fault_host = nullptr;  // pinned host word a wave that gives up waiting sets (SOLO_ERR_INCOMPLETE), device-visible
  int32_t* fault_dev = nullptr;
  // contact sensing (solo_engine_set_contact_sensing): the record [N][16][4] (allocated on first use) and the foot forces of
  // every step of a fused launch that leaves records, [N][contact_traj_steps][4] (sized with the record scratch)
  bool sensing = false;
  T *contact = nullptr, *contact_traj = nullptr;
  // control decimation (solo_engine_set_decimation): physics steps per control step; hparams.decimation is what the kernels read
  int decimation = 1;
  // state terminations (solo_engine_set_term_values / set_program): the thresholds per termination slot (hparams.term_value is
  // what the kernels read), whether the program in force holds a state kind (solo_term_kernel), and which termination fired [N]
  double term_values[SOLO_MAX_TERMS] = {0, 0, 0, 0};
  bool state_terms = false;
  uint8_t* term_fired = nullptr;
  // actuator randomisation (solo_engine_set_actuators): the block [N][SOLO_ACTUATOR_WIDTH] (allocated on first use), and whether
  // it is on (solo_act_kernel; hparams.actuators is what the kernels read)
  T* actuators = nullptr;
  bool act_on = false;
  // external base wrenches (solo_engine_set_base_wrench): the block [N][SOLO_WRENCH_WIDTH] (allocated on first use), whether it
  // is on (solo_push_kernel; hparams.wrench is what the kernels read), and the all-ones actuator block the push kernels - actuator
  // kernels, all of them - read while the actuator block is off (point_actuators)
  T* wrench = nullptr;
  bool wrench_on = false;
  T* act_ones = nullptr;
#ifdef SOLO_STAMPS
  unsigned long long* stamps = nullptr;
#endif

  ~Engine() override {
    (void)hipSetDevice(device);
    for (int g = 0; g < kMaxStreams; ++g) {
      if (sub[g]) (void)hipStreamDestroy(sub[g]);
      if (ev_join[g]) (void)hipEventDestroy(ev_join[g]);
    }
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    for (void* p : {(void*)dparams, (void*)state, (void*)snapshot, (void*)targets, (void*)params,
                    (void*)obs, (void*)reward, (void*)settle_actions, (void*)done,
                    (void*)term_count, (void*)order, (void*)cost, (void*)stats, (void*)terrain, (void*)traj, (void*)queue, (void*)warm, (void*)contact, (void*)contact_traj, (void*)term_fired, (void*)actuators, (void*)wrench, (void*)act_ones, (void*)progress})
      if (p) (void)hipFree(p);
    if (fault_host) (void)hipHostFree(fault_host);
  }

  int init(const SoloConfig& c, const SoloModel& m, int num_envs, int dev) {
    cfg = c; model = m; n = num_envs; device = dev;
    HIP_TRY(hipSetDevice(device));
    solo::pack_params<T>(cfg, model, &hparams);
    control.mode = SOLO_CTRL_POSITION;
    control.action_scale = cfg.action_scale;
    const size_t ns = (size_t)n * SOLO_STATE_STRIDE;
    HIP_TRY(hipMalloc((void**)&dparams, sizeof(hparams)));
    HIP_TRY(hipMalloc((void**)&state, ns * sizeof(T)));
    HIP_TRY(hipMalloc((void**)&snapshot, ns * sizeof(T)));
    HIP_TRY(hipMalloc((void**)&targets, (size_t)n * SOLO_NUM_JOINTS * sizeof(T)));
    HIP_TRY(hipMalloc((void**)&settle_actions, (size_t)n * SOLO_NUM_JOINTS * sizeof(T)));
    HIP_TRY(hipMalloc((void**)&params, (size_t)n * 4 * sizeof(T)));
    HIP_TRY(hipMalloc((void**)&obs, (size_t)n * SOLO_MAX_OBS * sizeof(T)));
    HIP_TRY(hipMalloc((void**)&reward, (size_t)n * sizeof(T)));
    HIP_TRY(hipMalloc((void**)&done, (size_t)n));
    HIP_TRY(hipMalloc((void**)&term_count, (size_t)n * SOLO_MAX_TERMS * sizeof(int32_t)));
    HIP_TRY(hipMalloc((void**)&stats, kStatsBytes));
    HIP_TRY(hipMalloc((void**)&order, (size_t)n * sizeof(int32_t)));
    HIP_TRY(hipMalloc((void**)&cost, (size_t)n * sizeof(int32_t)));
    HIP_TRY(hipMemset(cost, 0, (size_t)n * sizeof(int32_t)));
    HIP_TRY(hipMalloc((void**)&warm, (size_t)n * 64 * sizeof(T)));
    HIP_TRY(hipMemset(warm, 0, (size_t)n * 64 * sizeof(T)));
    HIP_TRY(hipHostMalloc((void**)&fault_host, sizeof(int32_t), hipHostMallocMapped));
    *fault_host = 0;
    HIP_TRY(hipHostGetDevicePointer((void**)&fault_dev, fault_host, 0));
    HIP_TRY(hipMemset(obs, 0, (size_t)n * SOLO_MAX_OBS * sizeof(T)));
    HIP_TRY(hipMemset(reward, 0, (size_t)n * sizeof(T)));
    HIP_TRY(hipMemset(done, 0, (size_t)n));
    HIP_TRY(hipMalloc((void**)&term_fired, (size_t)n));
    HIP_TRY(hipMemset(term_fired, 0, (size_t)n));
    hparams.term_fired = term_fired;
    HIP_TRY(hipMemset(term_count, 0, (size_t)n * SOLO_MAX_TERMS * sizeof(int32_t)));
    HIP_TRY(hipMemset(stats, 0, kStatsBytes));
#ifdef SOLO_STAMPS
    HIP_TRY(hipMalloc((void**)&stamps, (size_t)n * 32 * sizeof(unsigned long long)));
    HIP_TRY(hipMemset(stamps, 0, (size_t)n * 32 * sizeof(unsigned long long)));
#endif
    std::vector<T> hp((size_t)n * 4, T(0));
    std::vector<T> ha((size_t)n * SOLO_NUM_JOINTS);
    for (int e = 0; e < n; ++e) {
      hp[(size_t)e * 4 + 0] = (T)cfg.lateral_friction;
      hp[(size_t)e * 4 + 1] = T(1);
      // settle targets are absolute radians; the kernel multiplies actions by action_scale
      for (int j = 0; j < SOLO_NUM_JOINTS; ++j)
        ha[(size_t)e * SOLO_NUM_JOINTS + j] = (T)(cfg.settle_targets[j] / cfg.action_scale);
    }
    HIP_TRY(hipMemcpy(params, hp.data(), hp.size() * sizeof(T), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(settle_actions, ha.data(), ha.size() * sizeof(T), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dparams, &hparams, sizeof(hparams), hipMemcpyHostToDevice));
    return settle(nullptr);
  }

  using Plan = solo::Plan;
  using Args = solo::RolloutArgs<T>;
  static constexpr int kMaxStreams = solo::kMaxStreams;

  // one thread per element of a utility kernel's array
  template <class K, class... A>
  static void launch_flat(K kernel, size_t total, hipStream_t s, A... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, args...);
  }

  // the buffers a launch is wired to (solo::wire_launch), as they are now
  solo::EngineBuffers<T> wiring() const {
    solo::EngineBuffers<T> e;
    e.state = state; e.snapshot = snapshot; e.targets = targets; e.params = params; e.obs = obs; e.reward = reward;
    e.done = done; e.term_count = term_count; e.stats = stats; e.terrain = terrain; e.order = use_order ? order : nullptr;
    e.cost = cost; e.warm = cfg.solver_warm_start > 0 ? warm : nullptr; e.fault = fault_dev;
    e.traj = traj; e.traj_steps = traj_steps; e.queue = queue; e.queue_len = queue_ints; e.n = n; e.obs_dim = obs_dim;
    e.progress = progress;
#ifdef SOLO_STAMPS
    e.stamps = stamps;
#endif
    return e;
  }

  int launch(const T* actions, uint32_t flags, hipStream_t s) {
    // one 64-lane workgroup (= one wavefront) per robot, one env step
    return rollout_impl(Plan{1, 1, 1, 0}, Args{actions, 0, 1, flags, nullptr, nullptr, nullptr}, s, nullptr, nullptr);
  }

  // (SOLO_ERR_INCOMPLETE, sticky: a wave of an earlier migrating launch gave up waiting - a plain read of a pinned host word)
  int check_fault() override {
    if (fault_host != nullptr && *(volatile int32_t*)fault_host != 0) {
      err = "a wave of an earlier launch with robot migration gave up waiting for its robot: some robots were not stepped through that launch (internal error)";
      return SOLO_ERR_INCOMPLETE;
    }
    return SOLO_OK;
  }

  int settle(hipStream_t s) override {
    if (int rc = check_fault()) return rc;
    HIP_TRY(hipSetDevice(device));
    const int total = n * SOLO_STATE_STRIDE;
    launch_flat(solo::solo_init_kernel<T>, total, s, state, targets,
                (T)cfg.start_pos[0], (T)cfg.start_pos[1], (T)cfg.start_pos[2], (T)cfg.start_quat[0],
                (T)cfg.start_quat[1], (T)cfg.start_quat[2], (T)cfg.start_quat[3], n);
    HIP_TRY(hipGetLastError());
    // the snapshot doubles as the divergence fallback during the settle loop itself
    HIP_TRY(hipMemcpyAsync(snapshot, state, (size_t)total * sizeof(T), hipMemcpyDeviceToDevice, s));
    // (the settle loop starts from an empty warm-start cache too: a second settle - after a terrain or parameter change -
    // must not depend on what was simulated before)
    HIP_TRY(hipMemsetAsync(warm, 0, (size_t)n * 64 * sizeof(T), s));
    // the settle loop repeats one action: action stride 0 inside the fused launches (position control in every mode), as
    // one chain on the caller's stream whatever the rollout policy says about slices
    // (... and in PHYSICS steps whatever the control decimation: `settling` also keeps the launches on the position kernels)
    settling = true;
    Plan settle_plan = make_plan(cfg.settle_steps, SOLO_STEP_PHYSICS);
    settle_plan.slices = 1;
    const int rc_settle = rollout_impl(settle_plan, Args{settle_actions, 0, cfg.settle_steps, SOLO_STEP_PHYSICS, nullptr, nullptr, nullptr}, s, nullptr, nullptr);
    settling = false;
    if (rc_settle) return rc_settle;
    // (a torque / PD mode's robots are then commanded to its reset command)
    if (ctl_active()) {
      launch_flat(solo::solo_set_command_kernel<T>, (size_t)n * SOLO_NUM_JOINTS, s, dparams, targets, (const uint8_t*)nullptr, n);
      HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(snapshot, state, (size_t)total * sizeof(T), hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemsetAsync(term_count, 0, (size_t)n * SOLO_MAX_TERMS * sizeof(int32_t), s));
    HIP_TRY(hipMemsetAsync(warm, 0, (size_t)n * 64 * sizeof(T), s));  // (the snapshot starts from an empty warm-start cache)
    HIP_TRY(hipMemsetAsync(stats, 0, kStatsBytes, s));
    if (contact) HIP_TRY(hipMemsetAsync(contact, 0, contact_bytes(), s));   // (every robot was reset)
    HIP_TRY(hipStreamSynchronize(s));
    return SOLO_OK;
  }
  size_t contact_bytes() const { return (size_t)n * SOLO_MAX_SPHERES * SOLO_CONTACT_WIDTH * sizeof(T); }
  // (of a SoloProgram or of its packed form: the foot-force sources are the last SOLO_NUM_LEGS of the enumeration)
  template <class Obs>
  static bool reads_foot_force(const Obs* obs, int num_obs) {
    for (int i = 0; i < num_obs && i < SOLO_MAX_OBS; ++i)
      if (obs[i].src >= SOLO_SRC_FOOT_FORCE && obs[i].src < SOLO_SRC_FOOT_FORCE + SOLO_NUM_LEGS) return true;
    return false;
  }

  int set_program(const SoloProgram* p) override {
    HIP_TRY(hipSetDevice(device));
    solo::KParams<T> tmp = hparams;
    if (int rc = solo::pack_program<T>(*p, &tmp, &err)) return rc;
    if (!sensing && reads_foot_force(p->obs, p->num_obs)) { err = "the observation program reads a foot-force source: turn contact sensing on first (solo_engine_set_contact_sensing)"; return SOLO_ERR_INVALID_ARG; }
    const bool reads_state = solo::program_reads_state(*p);
    if (reads_state) {   // (validated before anything is touched: a rejected program leaves the previous one in force)
      if (cfg.migrate_steps > 0) { err = "state terminations do not support robot migration (migrate_steps > 0)"; return SOLO_ERR_INVALID_ARG; }
      if (cfg.solver_residual_threshold > 0) { err = "state terminations do not support solver_residual_threshold > 0"; return SOLO_ERR_INVALID_ARG; }
      if (cfg.solver_warm_start > 0) { err = "state terminations do not support solver_warm_start > 0"; return SOLO_ERR_INVALID_ARG; }
      if (sensing) { err = "state terminations do not support contact sensing: turn it off first"; return SOLO_ERR_INVALID_ARG; }
    }
    hparams = tmp;
    state_terms = reads_state;
    obs_dim = p->num_obs;
    have_program = true;
    // uploads are rare (registration time): a blocking copy keeps later launches ordered
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(dparams, &hparams, sizeof(hparams), hipMemcpyHostToDevice));
    return SOLO_OK;
  }

  int reset(const uint8_t* mask, hipStream_t s) override {
    if (int rc = check_fault()) return rc;
    HIP_TRY(hipSetDevice(device));
    const int total = n * SOLO_STATE_STRIDE;
    launch_flat(solo::solo_reset_kernel<T>, total, s, dparams, state, snapshot, targets, term_count, warm, mask, n);
    HIP_TRY(hipGetLastError());
    if (ctl_active()) {  // (a torque / PD mode's reset command instead of the settle pose: same stream, behind the restore)
      launch_flat(solo::solo_set_command_kernel<T>, (size_t)n * SOLO_NUM_JOINTS, s, dparams, targets, mask, n);
      HIP_TRY(hipGetLastError());
    }
    if (contact) {   // (contact sensing: a reset robot reads zeros until its next physics step)
      launch_flat(solo::solo_contact_zero_kernel<T>, (size_t)n * SOLO_MAX_SPHERES * SOLO_CONTACT_WIDTH, s, contact, mask, n);
      HIP_TRY(hipGetLastError());
    }
    return SOLO_OK;
  }

  int set_targets(const void* a, hipStream_t s) override {
    if (!a) { err = "actions must not be NULL"; return SOLO_ERR_INVALID_ARG; }
    HIP_TRY(hipSetDevice(device));
    const int total = n * SOLO_NUM_JOINTS;
    launch_flat(solo::solo_set_targets_kernel<T>, total, s, (const T*)a, targets, (T)(ctl_active() ? control.action_scale : cfg.action_scale), total);
    HIP_TRY(hipGetLastError());
    return SOLO_OK;
  }

  int check_flags(uint32_t flags) {
    if ((flags & SOLO_STEP_ALL) == 0 || (flags & ~(SOLO_STEP_ALL | SOLO_STEP_AUTO_RESET))) { err = "bad step flags"; return SOLO_ERR_INVALID_ARG; }
    if ((flags & (SOLO_STEP_OBS | SOLO_STEP_REWARD | SOLO_STEP_DONE)) && !have_program) {
      err = "no observation/reward/termination program registered";
      return SOLO_ERR_NO_PROGRAM;
    }
    // mirrors the ValueErrors of obs.py:138-139, rewards.py:115-116, termination.py:43-44
    if ((flags & SOLO_STEP_OBS) && hparams.c.num_obs == 0) { err = "Need to register at least one observation instance"; return SOLO_ERR_NO_PROGRAM; }
    if ((flags & SOLO_STEP_REWARD) && hparams.c.num_reward_ops == 0) { err = "Need to register at least one reward instance"; return SOLO_ERR_NO_PROGRAM; }
    if ((flags & SOLO_STEP_DONE) && hparams.c.num_terms == 0) { err = "Need to register at least one termination instance"; return SOLO_ERR_NO_PROGRAM; }
    return SOLO_OK;
  }

  int step(const void* a, uint32_t flags, hipStream_t s) override {
    if (int rc = check_fault()) return rc;
    if (int rc = check_flags(flags)) return rc;
    HIP_TRY(hipSetDevice(device));
    return launch((const T*)a, flags, s);
  }

  // ---- the launch policy is solo::make_plan (solo_launch.h); what it reads of this engine:
  static constexpr int kWavesPerSimd = solo::kWavesPerSimd<T>;
  int resident_robots() const {
    hipDeviceProp_t p;
    const int cus = (hipGetDeviceProperties(&p, device) == hipSuccess && p.multiProcessorCount > 0) ? p.multiProcessorCount : 256;
    return cus * 4 * kWavesPerSimd;
  }
  int resident_cache = 0;
  solo::PlanInput plan_input(int k, uint32_t flags) {
    if (resident_cache == 0) resident_cache = resident_robots();
    // (fused segments - solo_roll_kernel - with the default solver, outside the settle loop)
    return {n, sizeof(T), resident_cache, cfg.steps_per_launch, cfg.rollout_streams, cfg.migrate_steps, ctl_active(), sensing, k, flags,
            settling ? 1 : decimation, state_terms, act_on, wrench_on, !settling && !(cfg.solver_residual_threshold > 0)};
  }
  Plan make_plan(int k, uint32_t flags) { return solo::make_plan(plan_input(k, flags)); }
  // the record scratch of fused launches and the migration queues are sized for the rollout at hand (a larger one grows them:
  // the one hidden device synchronisation of the stream-ordered calls - include/solo_engine.h "LAZY SCRATCH"; solo_engine_reserve
  // does it ahead of time)
  int ensure_scratch(const Plan& p, uint32_t flags) {
    const bool records = solo::leaves_records(flags);
    if (records && p.S > traj_steps) {
      HIP_TRY(hipDeviceSynchronize());
      if (traj) { (void)hipFree(traj); traj = nullptr; traj_steps = 0; }
      HIP_TRY(hipMalloc((void**)&traj, solo::record_reals(n, p.S) * sizeof(T)));
      traj_steps = p.S;
      if (contact_traj) { (void)hipFree(contact_traj); contact_traj = nullptr; }
    }
    if (sensing && records && contact_traj == nullptr && traj_steps > 0) {   // (the foot forces per step, sized like the records)
      HIP_TRY(hipDeviceSynchronize());
      HIP_TRY(hipMalloc((void**)&contact_traj, solo::foot_force_reals(n, traj_steps) * sizeof(T)));
      hparams.contact_traj = contact_traj;
      hparams.contact_traj_steps = traj_steps;
      HIP_TRY(hipMemcpy(dparams, &hparams, sizeof(hparams), hipMemcpyHostToDevice));
    }
    const size_t need = solo::queue_ints(n, p);
    if (need > queue_ints) {
      HIP_TRY(hipDeviceSynchronize());
      if (queue) { (void)hipFree(queue); queue = nullptr; queue_ints = 0; }
      HIP_TRY(hipMalloc((void**)&queue, need * sizeof(int32_t)));
      queue_ints = need;
    }
    if (solo::progress_ints(p) > 0 && progress == nullptr) {   // (a fresh allocation: nothing in flight uses it)
      HIP_TRY(hipMalloc((void**)&progress, solo::progress_ints(p) * sizeof(int32_t)));
      HIP_TRY(hipMemset(progress, 0, solo::progress_ints(p) * sizeof(int32_t)));
    }
    return SOLO_OK;
  }

  // the arguments of a rollout over the caller's buffers: actions [K][N][12], outputs only where their flag is set
  Args rollout_args(const void* a, int k, uint32_t flags, void* obs_out, void* reward_out, void* done_out) const {
    return Args{(const T*)a, a ? (long long)n * SOLO_NUM_JOINTS : 0, k, flags, (flags & SOLO_STEP_OBS) ? (T*)obs_out : nullptr,
                (flags & SOLO_STEP_REWARD) ? (T*)reward_out : nullptr, (flags & SOLO_STEP_DONE) ? (uint8_t*)done_out : nullptr};
  }

  int rollout(const void* a, int k, uint32_t flags, void* obs_out, void* reward_out, void* done_out, hipStream_t s) override {
    if (int rc = check_fault()) return rc;
    if (int rc = check_flags(flags)) return rc;
    if (k == 0) return SOLO_OK;  // an empty rollout is a no-op
    if (!a || k < 0) { err = "rollout needs actions [K][N][12]"; return SOLO_ERR_INVALID_ARG; }
    const Plan plan = make_plan(k, flags);
    const Args args = rollout_args(a, k, flags, obs_out, reward_out, done_out);
    rolled = false;   // (kernel_name: did this rollout run segmented launches?)
    if (int rc = rollout_impl(plan, args, s, nullptr, nullptr)) return rc;
    // (the view's last step of the recording rollouts whose last launch does not write it: solo::tail_needs_copy)
    if (!solo::tail_needs_copy<T>(plan, k, flags)) return SOLO_OK;
    if (args.obs_out)
      HIP_TRY(hipMemcpyAsync(obs, args.obs_out + (size_t)(k - 1) * n * obs_dim, (size_t)n * obs_dim * sizeof(T), hipMemcpyDeviceToDevice, s));
    if (args.reward_out)
      HIP_TRY(hipMemcpyAsync(reward, args.reward_out + (size_t)(k - 1) * n, (size_t)n * sizeof(T), hipMemcpyDeviceToDevice, s));
    if (args.done_out)
      HIP_TRY(hipMemcpyAsync(done, args.done_out + (size_t)(k - 1) * n, (size_t)n, hipMemcpyDeviceToDevice, s));
    return SOLO_OK;
  }

  // enqueues the launches of a rollout (solo::for_each_launch): one chain on the caller's stream, or one chain per slice on
  // the engine's own streams, forked from and joined into the caller's.
  // t0 / t1 (optional, [groups] each): timing events recorded around every slice's launch chain, on
  // the stream that chain is launched on
  int rollout_impl(const Plan& plan, const Args& args, hipStream_t s, hipEvent_t* t0, hipEvent_t* t1) {
    HIP_TRY(hipSetDevice(device));
    const int groups = plan.slices;
    if (int rc = ensure_scratch(plan, args.flags)) return rc;   // (before any timing event is recorded)
    // (progress pacing: the block is zeroed in front of the fork - every slice's launch counts into it; a captured rollout re-zeroes it at every replay)
    if (progress != nullptr && solo::rollout_is_paced(plan, args.k)) HIP_TRY(hipMemsetAsync(progress, 0, solo::progress_ints(plan) * sizeof(int32_t), s));
    if (groups == 1) {
      if (t0) HIP_TRY(hipEventRecord(t0[0], s));
    } else {
      if (int rc = ensure_streams(groups)) return rc;
      HIP_TRY(hipEventRecord(ev_fork, s));
      for (int g = 0; g < groups; ++g) {
        HIP_TRY(hipStreamWaitEvent(sub[g], ev_fork, 0));
        if (t0) HIP_TRY(hipEventRecord(t0[g], sub[g]));
      }
    }
    const solo::EngineBuffers<T> wired = wiring();
    const bool resid = cfg.solver_residual_threshold > 0;
    if (int rc = solo::for_each_launch(plan, n, args.k, [&](const solo::Launch& l) { return enqueue(plan, args, wired, l, resid, groups == 1 ? s : sub[l.slice]); }))
      return rc;
    if (groups == 1) {
      if (t1) HIP_TRY(hipEventRecord(t1[0], s));
      return SOLO_OK;
    }
    for (int g = 0; g < groups; ++g) {
      if (t1) HIP_TRY(hipEventRecord(t1[g], sub[g]));
      HIP_TRY(hipEventRecord(ev_join[g], sub[g]));
      HIP_TRY(hipStreamWaitEvent(s, ev_join[g], 0));
    }
    return SOLO_OK;
  }

  // one launch: its work queue's initialisation when its robots migrate, then the step kernel, one wave per robot
  int enqueue(const Plan& plan, const Args& args, const solo::EngineBuffers<T>& wired, const solo::Launch& l, bool resid, hipStream_t s) {
    solo::KBuffers<T> b;
    solo::QueueInit q;
    if (!solo::wire_launch(plan, args, wired, l, &b, &q)) {
      err = "internal error: the migration queue of a launch does not fit its slice's region";
      return SOLO_ERR_INVALID_ARG;
    }
    if (q.ints > 0) {
      launch_flat(solo::solo_queue_init_kernel, q.ints, s, q.q, q.ints, q.lo, q.count, q.rings, q.steps, q.chunk, q.order);
      HIP_TRY(hipGetLastError());
    }
    const solo::KParams<T>* params_dev = dparams;
    const bool segmented = b.seg_steps > 0;   // (a fused launch: solo_roll_kernel)
    if (segmented) rolled = true;
    solo::with_step_kernel<T>(solo::choose_kernel(sensing, ctl_active(), settling, resid, b.queue != nullptr, args.flags, decimation, state_terms, act_on, wrench_on, segmented),
                              [&](solo::StepKernel<T> k) { hipLaunchKernelGGL(k, dim3(l.count), dim3(64), 0, s, params_dev, b); });
    HIP_TRY(hipGetLastError());
    return SOLO_OK;
  }

  hipStream_t sub[kMaxStreams] = {};
  hipEvent_t ev_fork = nullptr, ev_join[kMaxStreams] = {};
  int ensure_streams(int groups) {
    if (!ev_fork) HIP_TRY(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
    for (int g = 0; g < groups; ++g) {
      if (!sub[g]) HIP_TRY(hipStreamCreateWithFlags(&sub[g], hipStreamNonBlocking));
      if (!ev_join[g]) HIP_TRY(hipEventCreateWithFlags(&ev_join[g], hipEventDisableTiming));
    }
    return SOLO_OK;
  }

  // runs a rollout with hipEvents around every slice's chain, each on the stream its chain is launched on, and reports the
  // AVERAGE launch duration over all slices and launches (the statistic rocprofv3 --stats gives for the kernel)
  int timed(const Plan& plan, const Args& args, hipStream_t s, double* ms) {
    struct Events {  // destroyed on every path out of this function
      hipEvent_t e[2 * kMaxStreams] = {};
      ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    } ev;
    for (hipEvent_t& x : ev.e) HIP_TRY(hipEventCreate(&x));
    hipEvent_t *e0 = ev.e, *e1 = ev.e + kMaxStreams;
    if (int rc = rollout_impl(plan, args, s, e0, e1)) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    double total = 0;
    for (int g = 0; g < plan.slices; ++g) {
      float t = 0;
      HIP_TRY(hipEventElapsedTime(&t, e0[g], e1[g]));
      total += t;
    }
    *ms = total / plan.slices / plan.launches;   // (fused segments: plan.launches counts the S-step segments - the figure stays "per S steps")
    return SOLO_OK;
  }

  int time_step(const void* a, uint32_t flags, int reps, hipStream_t s, double* ms) override {
    if (int rc = check_flags(flags)) return rc;
    if (reps <= 0 || !ms) { err = "reps must be positive"; return SOLO_ERR_INVALID_ARG; }
    HIP_TRY(hipSetDevice(device));
    // (reps launches of the CONFIGURED steps per launch - one step when that is left to the engine: solo_engine_time_rollout
    // times a rollout of a given length with the engine's own geometry)
    const int S = cfg.steps_per_launch > 1 ? cfg.steps_per_launch : 1;
    Plan plan = make_plan(reps * S, flags);
    plan.fuse = 0;   // (reps LAUNCHES: never fused into segments of one)
    if (cfg.steps_per_launch == -1) {   // (reps launches of ONE step, whatever the engine would choose for a rollout of reps steps - on ONE chain, whatever reps is)
      plan.S = 1; plan.launches = reps; plan.migrate = 0;
      if (cfg.rollout_streams == -1) plan.slices = 1;
    }
    rolled = false;
    return timed(plan, rollout_args(a, reps * S, flags, nullptr, nullptr, nullptr), s, ms);
  }

  int time_rollout(const void* a, int k, uint32_t flags, void* obs_out, void* reward_out, void* done_out, hipStream_t s, double* ms) override {
    if (int rc = check_flags(flags)) return rc;
    if (k <= 0 || !ms) { err = "num_steps must be positive"; return SOLO_ERR_INVALID_ARG; }
    HIP_TRY(hipSetDevice(device));
    rolled = false;
    return timed(make_plan(k, flags), rollout_args(a, k, flags, obs_out, reward_out, done_out), s, ms);
  }

  int reserve(int k, uint32_t flags) override {
    if (k <= 0) { err = "num_steps must be positive"; return SOLO_ERR_INVALID_ARG; }
    if (int rc = check_flags(flags)) return rc;
    HIP_TRY(hipSetDevice(device));
    // (every distinct geometry of the rollouts of up to k steps under this configuration)
    return solo::for_each_geometry(plan_input(k, flags), k, [&](const Plan& p) {
      if (int rc = ensure_scratch(p, flags)) return rc;
      return p.slices > 1 ? ensure_streams(p.slices) : (int)SOLO_OK;
    });
  }

  int plan(int k, SoloLaunchPlan* out) override {
    if (k <= 0 || !out) { err = "num_steps must be positive"; return SOLO_ERR_INVALID_ARG; }
    HIP_TRY(hipSetDevice(device));
    const Plan p = make_plan(k, SOLO_STEP_ALL);
    out->steps_per_launch = p.S; out->launches = p.launches; out->slices = p.slices;
    out->migrate_steps = (p.migrate > 0 && p.S > p.migrate) ? solo::migration_chunk_steps(p.S, p.migrate) : 0;
    out->waves_per_simd = kWavesPerSimd; out->resident_robots = resident_cache;
    return SOLO_OK;
  }

  int set_terrain(const SoloTerrain* t, hipStream_t s) override {
    // (validated before anything is touched: a rejected call leaves the previous ground in force)
    if (t && (t->nx < 2 || t->ny < 2 || !(t->cell > 0) || !t->heights || (long long)t->nx * t->ny > (1ll << 26))) {
      err = "terrain needs nx, ny >= 2, cell > 0 and a heights array";
      return SOLO_ERR_INVALID_ARG;
    }
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipDeviceSynchronize());
    if (terrain) { (void)hipFree(terrain); terrain = nullptr; }
    solo::pack_terrain<T>(nullptr, &hparams);
    if (t) {
      const size_t cnt = (size_t)t->nx * t->ny;
      std::vector<T> h(cnt);
      for (size_t i = 0; i < cnt; ++i) h[i] = (T)t->heights[i];
      HIP_TRY(hipMalloc((void**)&terrain, cnt * sizeof(T)));
      HIP_TRY(hipMemcpy(terrain, h.data(), cnt * sizeof(T), hipMemcpyHostToDevice));
      solo::pack_terrain<T>(t, &hparams);
    }
    HIP_TRY(hipMemcpy(dparams, &hparams, sizeof(hparams), hipMemcpyHostToDevice));
    return settle(s);
  }

  int set_order(const int32_t* o, hipStream_t s) override {
    HIP_TRY(hipSetDevice(device));
    if (o == nullptr) { use_order = false; return SOLO_OK; }
    // The step kernel uses order[slot] as the robot index of every buffer it addresses, and the output epilogues
    // of a rollout slice read the records of that slice's robots: the table is validated here, once per upload
    // (a rare call; blocking) - a permutation of [0, N) that maps every rollout slice onto itself.
    std::vector<int32_t> h((size_t)n);
    HIP_TRY(hipMemcpyAsync(h.data(), o, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    std::vector<uint8_t> seen((size_t)n, 0);
    const int groups = solo::max_slices(n, cfg.rollout_streams);
    for (int g = 0; g < groups; ++g) {
      const int lo = (int)((long long)n * g / groups), hi = (int)((long long)n * (g + 1) / groups);
      for (int i = lo; i < hi; ++i) {
        const int32_t e = h[(size_t)i];
        if (e < lo || e >= hi || seen[(size_t)e]) {
          err = "launch order must be a permutation of [0, num_envs) that keeps every rollout slice's robots in that slice";
          return SOLO_ERR_INVALID_ARG;
        }
        seen[(size_t)e] = 1;
      }
    }
    HIP_TRY(hipMemcpyAsync(order, h.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));  // (h goes out of scope)
    use_order = true;
    return SOLO_OK;
  }

  int view(SoloStateView* v) override {
    v->num_envs = n;
    v->dtype = sizeof(T) == 4 ? SOLO_F32 : SOLO_F64;
    v->state_stride = SOLO_STATE_STRIDE;
    v->obs_dim = obs_dim;
    v->state = state; v->snapshot = snapshot; v->targets = targets; v->obs = obs; v->reward = reward;
    v->done = done; v->term_count = term_count; v->params = params; v->stats = stats; v->cost = cost; v->warm = warm;
    return SOLO_OK;
  }

  int set_params(int which, const void* p, hipStream_t s) override {
    if (which < 0 || which > 1 || !p) { err = "which must be 0 (friction) or 1 (base mass scale)"; return SOLO_ERR_INVALID_ARG; }
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMemcpy2DAsync(params + which, 4 * sizeof(T), p, sizeof(T), sizeof(T), n, hipMemcpyDeviceToDevice, s));
    return SOLO_OK;
  }

  bool ctl_active() const { return control.mode != SOLO_CTRL_POSITION; }

  int get_control(SoloControl* out) override { *out = control; return SOLO_OK; }

  int set_control(const SoloControl* c, hipStream_t s) override {
    // (validated before anything is touched: a rejected call leaves the previous mode in force)
    if (c->mode != SOLO_CTRL_POSITION && c->mode != SOLO_CTRL_TORQUE && c->mode != SOLO_CTRL_PD) { err = "control mode must be SOLO_CTRL_POSITION, SOLO_CTRL_TORQUE or SOLO_CTRL_PD"; return SOLO_ERR_INVALID_ARG; }
    if (c->reserved0 != 0) { err = "SoloControl::reserved0 must be 0"; return SOLO_ERR_INVALID_ARG; }
    for (int d = 0; d < SOLO_NUM_DOF; ++d)
      if (!(c->kp[d] >= 0 && c->kp[d] < INFINITY && c->kd[d] >= 0 && c->kd[d] < INFINITY)) { err = "PD gains must be finite and >= 0"; return SOLO_ERR_INVALID_ARG; }
    if (!(c->action_scale > 0 && c->action_scale < INFINITY)) { err = "action_scale must be finite and positive"; return SOLO_ERR_INVALID_ARG; }
    if (c->mode != SOLO_CTRL_POSITION) {
      if (cfg.solver_residual_threshold > 0) { err = "torque / PD control does not support solver_residual_threshold > 0"; return SOLO_ERR_INVALID_ARG; }
      if (cfg.solver_warm_start > 0) { err = "torque / PD control does not support solver_warm_start > 0"; return SOLO_ERR_INVALID_ARG; }
      if (cfg.migrate_steps > 0) { err = "torque / PD control does not support robot migration (migrate_steps > 0)"; return SOLO_ERR_INVALID_ARG; }
    }
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipDeviceSynchronize());
    control = *c;
    if (c->mode == SOLO_CTRL_POSITION) control.action_scale = cfg.action_scale;   // (position mode keeps the configuration's scale)
    solo::pack_control<T>(cfg, control, &hparams);
    HIP_TRY(hipMemcpy(dparams, &hparams, sizeof(hparams), hipMemcpyHostToDevice));
    // every robot's command becomes the mode's reset command
    launch_flat(solo::solo_set_command_kernel<T>, (size_t)n * SOLO_NUM_JOINTS, s, dparams, targets, (const uint8_t*)nullptr, n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    return SOLO_OK;
  }

  int get_contacts(void** out) override { *out = sensing ? (void*)contact : nullptr; return SOLO_OK; }

  int set_contact_sensing(int32_t enable, hipStream_t s) override {
    // (validated before anything is touched: a rejected call leaves sensing as it was)
    if (enable) {
      if (cfg.solver_residual_threshold > 0) { err = "contact sensing does not support solver_residual_threshold > 0"; return SOLO_ERR_INVALID_ARG; }
      if (cfg.solver_warm_start > 0) { err = "contact sensing does not support solver_warm_start > 0"; return SOLO_ERR_INVALID_ARG; }
      if (cfg.migrate_steps > 0) { err = "contact sensing does not support robot migration (migrate_steps > 0)"; return SOLO_ERR_INVALID_ARG; }
      if (decimation > 1) { err = "contact sensing does not support control decimation (decimation > 1)"; return SOLO_ERR_INVALID_ARG; }
      if (state_terms) { err = "contact sensing does not support state terminations: register a program without them first"; return SOLO_ERR_INVALID_ARG; }
      if (act_on) { err = "contact sensing does not support actuator randomisation: turn it off first (solo_engine_set_actuators(NULL))"; return SOLO_ERR_INVALID_ARG; }
      if (wrench_on) { err = "contact sensing does not support base wrenches: turn them off first (solo_engine_set_base_wrench(NULL))"; return SOLO_ERR_INVALID_ARG; }
    } else if (reads_foot_force(hparams.obs, hparams.c.num_obs)) {
      err = "the observation program reads a foot-force source: register one without it before turning contact sensing off";
      return SOLO_ERR_INVALID_ARG;
    }
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipDeviceSynchronize());
    if (enable) {
      if (contact == nullptr) HIP_TRY(hipMalloc((void**)&contact, contact_bytes()));
      HIP_TRY(hipMemsetAsync(contact, 0, contact_bytes(), s));
      hparams.contact = contact;
      HIP_TRY(hipMemcpy(dparams, &hparams, sizeof(hparams), hipMemcpyHostToDevice));
      HIP_TRY(hipStreamSynchronize(s));
    }
    sensing = enable != 0;
    return SOLO_OK;
  }

  int get_decimation(int32_t* out) override { *out = decimation; return SOLO_OK; }

  int set_decimation(int32_t d) override {
    // (validated before anything is touched: a rejected call leaves the previous decimation in force)
    if (d < 1 || d > SOLO_MAX_DECIMATION) { err = "decimation must be in [1, 64]"; return SOLO_ERR_INVALID_ARG; }
    if (d > 1) {
      if (cfg.migrate_steps > 0) { err = "control decimation does not support robot migration (migrate_steps > 0)"; return SOLO_ERR_INVALID_ARG; }
      if (cfg.solver_residual_threshold > 0) { err = "control decimation does not support solver_residual_threshold > 0"; return SOLO_ERR_INVALID_ARG; }
      if (cfg.solver_warm_start > 0) { err = "control decimation does not support solver_warm_start > 0"; return SOLO_ERR_INVALID_ARG; }
      if (sensing) { err = "control decimation does not support contact sensing: turn it off first"; return SOLO_ERR_INVALID_ARG; }
    }
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipDeviceSynchronize());
    decimation = d;
    hparams.decimation = d;
    HIP_TRY(hipMemcpy(dparams, &hparams, sizeof(hparams), hipMemcpyHostToDevice));
    return SOLO_OK;
  }

  int get_term_fired(void** out) override { *out = term_fired; return SOLO_OK; }

  int set_term_values(const double* values) override {
    // (validated before anything is touched: a rejected call leaves the previous thresholds in force)
    for (int t = 0; t < SOLO_MAX_TERMS; ++t)
      if (values[t] != values[t]) { err = "termination thresholds must not be NaN"; return SOLO_ERR_INVALID_ARG; }
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipDeviceSynchronize());
    for (int t = 0; t < SOLO_MAX_TERMS; ++t) { term_values[t] = values[t]; hparams.term_value[t] = (T)values[t]; }
    HIP_TRY(hipMemcpy(dparams, &hparams, sizeof(hparams), hipMemcpyHostToDevice));
    return SOLO_OK;
  }

  int get_actuators(void** out) override { *out = act_on ? (void*)actuators : nullptr; return SOLO_OK; }

  int set_actuators(const void* per_env, hipStream_t s) override {
    HIP_TRY(hipSetDevice(device));
    if (per_env == nullptr) {   // off: the kernels of before
      HIP_TRY(hipDeviceSynchronize());
      act_on = false;
      return point_actuators();
    }
    // (validated before anything is touched - the table with one device-to-host copy, as set_order validates its own: a rejected
    // call leaves the previous block, or "off", in force)
    if (int rc = solo::actuators_conflict(cfg, sensing, &err)) return rc;
    const size_t cnt = (size_t)n * SOLO_ACTUATOR_WIDTH;
    std::vector<T> h(cnt);
    HIP_TRY(hipMemcpyAsync(h.data(), per_env, cnt * sizeof(T), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (int rc = solo::validate_actuators<T>(h.data(), n, &err)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    if (actuators == nullptr) HIP_TRY(hipMalloc((void**)&actuators, cnt * sizeof(T)));
    if ((const void*)actuators != per_env) HIP_TRY(hipMemcpy(actuators, h.data(), cnt * sizeof(T), hipMemcpyHostToDevice));
    act_on = true;
    return point_actuators();
  }

  // what the kernels read as the actuator block (the device is idle): the block while it is on, else the all-ones block - the
  // push kernels are actuator kernels, and all ones equal "off" bit for bit (null until either exists: no kernel reads it then)
  int point_actuators() {
    const T* want = act_on ? actuators : act_ones;
    if (hparams.actuators != want) {
      hparams.actuators = want;
      HIP_TRY(hipMemcpy(dparams, &hparams, sizeof(hparams), hipMemcpyHostToDevice));
    }
    return SOLO_OK;
  }

  int get_base_wrench(void** out) override { *out = wrench_on ? (void*)wrench : nullptr; return SOLO_OK; }

  int set_base_wrench(const void* per_env, hipStream_t s) override {
    HIP_TRY(hipSetDevice(device));
    if (per_env == nullptr) {   // off: the kernels of before
      HIP_TRY(hipDeviceSynchronize());
      wrench_on = false;
      return SOLO_OK;
    }
    // (validated before anything is touched, as set_actuators validates its own: a rejected call leaves the previous block, or
    // "off", in force)
    if (int rc = solo::base_wrench_conflict(cfg, sensing, &err)) return rc;
    const size_t cnt = (size_t)n * SOLO_WRENCH_WIDTH;
    std::vector<T> h(cnt);
    HIP_TRY(hipMemcpyAsync(h.data(), per_env, cnt * sizeof(T), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (int rc = solo::validate_base_wrench<T>(h.data(), n, &err)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    if (act_ones == nullptr) {
      const std::vector<T> ones((size_t)n * SOLO_ACTUATOR_WIDTH, T(1));
      HIP_TRY(hipMalloc((void**)&act_ones, ones.size() * sizeof(T)));
      HIP_TRY(hipMemcpy(act_ones, ones.data(), ones.size() * sizeof(T), hipMemcpyHostToDevice));
    }
    if (wrench == nullptr) {
      HIP_TRY(hipMalloc((void**)&wrench, cnt * sizeof(T)));
      hparams.wrench = wrench;
      HIP_TRY(hipMemcpy(dparams, &hparams, sizeof(hparams), hipMemcpyHostToDevice));
    }
    if ((const void*)wrench != per_env) HIP_TRY(hipMemcpy(wrench, h.data(), cnt * sizeof(T), hipMemcpyHostToDevice));
    wrench_on = true;
    return point_actuators();
  }

  // (the instantiation of a full launch whose robots do not migrate - every launch of up to 4096 robots under the engine's own
  // policy; a migrating launch's last template argument is `true`; solo_roll_kernel while the engine's last rollout ran fused
  // segments and the configuration still would)
  // (the progress block as the last paced rollout left it, zeros while there is none: solo_engine_debug_progress)
  int debug_progress(int32_t* host) override {
    for (int i = 0; i < solo::kMaxFusedSegments; ++i) host[i] = 0;
    if (progress == nullptr) return SOLO_OK;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(host, progress, solo::kMaxFusedSegments * sizeof(int32_t), hipMemcpyDeviceToHost));
    return SOLO_OK;
  }
  std::string name;
  bool rolled = false;
  const char* kernel_name() override {
    name = solo::kernel_name(solo::choose_kernel(sensing, ctl_active(), false, cfg.solver_residual_threshold > 0, false, SOLO_STEP_ALL, decimation, state_terms, act_on, wrench_on, rolled), sizeof(T));
    return name.c_str();
  }
};

// the f64 engine's factory: the one entry point of its translation unit (null = out of host memory; *rc = init's status)
EngineBase* make_engine_f64(const SoloConfig& cfg, const SoloModel& model, int32_t num_envs, int32_t device_id, int* rc);
#ifndef SOLO_TU_F32
EngineBase* make_engine_f64(const SoloConfig& cfg, const SoloModel& model, int32_t num_envs, int32_t device_id, int* rc) {
  auto* e = new (std::nothrow) Engine<double>();
  *rc = e ? e->init(cfg, model, num_envs, device_id) : (int)SOLO_ERR_HIP;
  return e;
}
#endif

}  // namespace solo_engine_detail

#ifndef SOLO_TU_F64  // ---- the C ABI (and the f32 engine) ----
using namespace solo_engine_detail;

namespace {

thread_local std::string g_create_error;

int check_config(const SoloConfig* c, std::string* err) {
  auto fail = [&](const char* s) { *err = s; return (int)SOLO_ERR_INVALID_ARG; };
  if (c->abi_version != SOLO_ABI_VERSION) return fail("abi_version mismatch");
  if (c->dtype != SOLO_F32 && c->dtype != SOLO_F64) return fail("dtype must be SOLO_F32 or SOLO_F64");
  if (!(c->dt > 0)) return fail("dt must be positive");
  if (c->solver_iterations < 1 || c->solver_iterations > 10000) return fail("solver_iterations out of range");
  if (c->solver_ulp_tolerance < 0 || c->solver_ulp_tolerance > (1 << 20)) return fail("solver_ulp_tolerance out of range");
  if (!(c->solver_residual_threshold >= 0)) return fail("solver_residual_threshold must be >= 0");
  if (c->settle_steps < 0 || c->settle_steps > 100000) return fail("settle_steps out of range");
  if (c->steps_per_launch < -1 || c->steps_per_launch > 100000) return fail("steps_per_launch out of range (-1 = the engine chooses)");
  if (c->rollout_streams < -1 || c->rollout_streams > 64) return fail("rollout_streams out of range (-1 = the engine chooses)");
  if (!(c->solver_warm_start >= 0 && c->solver_warm_start <= 1)) return fail("solver_warm_start must be in [0, 1]");
  if (c->solver_warm_start > 0 && !(c->solver_residual_threshold > 0)) return fail("solver_warm_start needs solver_residual_threshold > 0");
  if (c->migrate_steps < -1 || c->migrate_steps > 100000) return fail("migrate_steps out of range (-1 = the engine chooses)");
  if (c->reserved0 != 0) return fail("reserved0 must be 0");
  // (restitution: accepted, and without effect - see include/solo_engine.h: Bullet combines it with the ground's, which is 0)
  if (!(c->restitution >= 0 && c->restitution <= 1)) return fail("restitution must be in [0, 1] (gym_solo configs.py:23)");
  if (!(c->action_scale > 0)) return fail("action_scale must be positive");
  if (c->lateral_friction < 0 || c->contact_margin < 0 || c->contact_erp < 0) return fail("negative contact parameter");
  if (!(c->base_lateral_friction >= 0)) return fail("base_lateral_friction must be >= 0");
  return SOLO_OK;
}

}  // namespace

struct SoloEngine { EngineBase* impl; };

extern "C" {

#ifdef SOLO_STAMPS
// DIAGNOSTIC build only: copies the [N][32] s_memtime stamps of the last launch to the host.
int solo_engine_debug_stamps(SoloEngine* eng, unsigned long long* host, int is_f32) {
  if (!eng || !eng->impl) return SOLO_ERR_INVALID_ARG;
  (void)hipDeviceSynchronize();
  if (is_f32) { auto* e = static_cast<Engine<float>*>(eng->impl); return hipMemcpy(host, e->stamps, (size_t)e->n * 256, hipMemcpyDeviceToHost) == hipSuccess ? 0 : SOLO_ERR_HIP; }
  auto* e = static_cast<Engine<double>*>(eng->impl);
  return hipMemcpy(host, e->stamps, (size_t)e->n * 256, hipMemcpyDeviceToHost) == hipSuccess ? 0 : SOLO_ERR_HIP;
}
#endif

// DIAGNOSTIC (not part of include/solo_engine.h; tests/test_gpu_progress_pacing.py): the kMaxFusedSegments counters of the progress
// block as the last paced rollout left them, copied to the host behind a device synchronisation
int solo_engine_debug_progress(SoloEngine* eng, int32_t* host) {
  if (!eng || !eng->impl || !host) return SOLO_ERR_INVALID_ARG;
  return eng->impl->debug_progress(host);
}

int solo_abi_version(void) { return SOLO_ABI_VERSION; }
const char* solo_last_create_error(void) { return g_create_error.c_str(); }

int solo_engine_create(const SoloConfig* cfg, const SoloModel* model, int32_t num_envs, int32_t device_id,
                       SoloEngine** out) {
  if (!cfg || !model || !out) { g_create_error = "NULL argument"; return SOLO_ERR_INVALID_ARG; }
  *out = nullptr;
  if (num_envs < 1 || num_envs > (1 << 24)) { g_create_error = "num_envs out of range"; return SOLO_ERR_INVALID_ARG; }
  if (int rc = check_config(cfg, &g_create_error)) return rc;
  if (int rc = solo::validate_model(*model, &g_create_error)) return rc;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0) {
    g_create_error = "no HIP device visible: the Solo8 engine has no CPU fallback";
    return SOLO_ERR_NO_DEVICE;
  }
  if (device_id < 0 || device_id >= count) { g_create_error = "device_id out of range"; return SOLO_ERR_INVALID_ARG; }
  EngineBase* impl = nullptr;
  int rc;
  if (cfg->dtype == SOLO_F32) {
    auto* e = new (std::nothrow) Engine<float>();
    impl = e;
    rc = e ? e->init(*cfg, *model, num_envs, device_id) : SOLO_ERR_HIP;
  } else {
    impl = make_engine_f64(*cfg, *model, num_envs, device_id, &rc);
  }
  if (rc != SOLO_OK) {
    g_create_error = impl ? impl->err : "out of host memory";
    delete impl;
    return rc;
  }
  *out = new SoloEngine{impl};
  return SOLO_OK;
}

int solo_engine_destroy(SoloEngine* eng) {
  if (!eng) return SOLO_ERR_INVALID_ARG;
  delete eng->impl;
  delete eng;
  return SOLO_OK;
}

// (SOLO_ERR_INCOMPLETE is sticky: EVERY entry point that takes the engine checks the fault word first - ADVICE r5)
static int eng_fault(SoloEngine* eng) { return eng && eng->impl ? eng->impl->check_fault() : (int)SOLO_ERR_INVALID_ARG; }
#define ENG_CALL(expr) (eng_fault(eng) != SOLO_OK ? eng_fault(eng) : (eng->impl->expr))

int solo_engine_set_program(SoloEngine* eng, const SoloProgram* prog) {
  if (!prog) return SOLO_ERR_INVALID_ARG;
  return ENG_CALL(set_program(prog));
}
int solo_engine_reset(SoloEngine* eng, const uint8_t* mask_dev, void* stream) { return ENG_CALL(reset(mask_dev, (hipStream_t)stream)); }
int solo_engine_settle(SoloEngine* eng, void* stream) { return ENG_CALL(settle((hipStream_t)stream)); }
int solo_engine_set_targets(SoloEngine* eng, const void* a, void* stream) { return ENG_CALL(set_targets(a, (hipStream_t)stream)); }
int solo_engine_step(SoloEngine* eng, const void* a, uint32_t flags, void* stream) { return ENG_CALL(step(a, flags, (hipStream_t)stream)); }
int solo_engine_rollout(SoloEngine* eng, const void* a, int32_t k, uint32_t flags, void* stream) {
  return ENG_CALL(rollout(a, k, flags, nullptr, nullptr, nullptr, (hipStream_t)stream));
}
int solo_engine_rollout_record(SoloEngine* eng, const void* a, int32_t k, uint32_t flags, void* obs_out, void* reward_out,
                               void* done_out, void* stream) {
  return ENG_CALL(rollout(a, k, flags, obs_out, reward_out, done_out, (hipStream_t)stream));
}
int solo_engine_get_view(SoloEngine* eng, SoloStateView* out) {
  if (!out) return SOLO_ERR_INVALID_ARG;
  return ENG_CALL(view(out));
}
int solo_engine_set_params(SoloEngine* eng, int32_t which, const void* p, void* stream) { return ENG_CALL(set_params(which, p, (hipStream_t)stream)); }
int solo_engine_set_terrain(SoloEngine* eng, const SoloTerrain* t, void* stream) { return ENG_CALL(set_terrain(t, (hipStream_t)stream)); }
int solo_engine_set_order(SoloEngine* eng, const int32_t* o, void* stream) { return ENG_CALL(set_order(o, (hipStream_t)stream)); }
const char* solo_engine_kernel_name(SoloEngine* eng) { return eng && eng->impl ? eng->impl->kernel_name() : ""; }
int solo_engine_set_control(SoloEngine* eng, const SoloControl* ctl, void* stream) {
  if (!ctl) return SOLO_ERR_INVALID_ARG;
  return ENG_CALL(set_control(ctl, (hipStream_t)stream));
}
int solo_engine_get_control(SoloEngine* eng, SoloControl* out) {
  if (!out) return SOLO_ERR_INVALID_ARG;
  return ENG_CALL(get_control(out));
}
int solo_engine_set_contact_sensing(SoloEngine* eng, int32_t enable, void* stream) { return ENG_CALL(set_contact_sensing(enable, (hipStream_t)stream)); }
int solo_engine_get_contacts(SoloEngine* eng, void** contact_dev) {
  if (!contact_dev) return SOLO_ERR_INVALID_ARG;
  return ENG_CALL(get_contacts(contact_dev));
}
int solo_engine_time_step(SoloEngine* eng, const void* a, uint32_t flags, int32_t reps, void* stream, double* ms) {
  return ENG_CALL(time_step(a, flags, reps, (hipStream_t)stream, ms));
}
int solo_engine_time_rollout(SoloEngine* eng, const void* a, int32_t k, uint32_t flags, void* obs_out, void* reward_out, void* done_out,
                             void* stream, double* ms) {
  return ENG_CALL(time_rollout(a, k, flags, obs_out, reward_out, done_out, (hipStream_t)stream, ms));
}
int solo_engine_plan(SoloEngine* eng, int32_t k, SoloLaunchPlan* out) { return ENG_CALL(plan(k, out)); }
int solo_engine_reserve(SoloEngine* eng, int32_t k, uint32_t flags) { return ENG_CALL(reserve(k, flags)); }
int solo_engine_set_decimation(SoloEngine* eng, int32_t decimation) { return ENG_CALL(set_decimation(decimation)); }
int solo_engine_get_decimation(SoloEngine* eng, int32_t* out) {
  if (!out) return SOLO_ERR_INVALID_ARG;
  return ENG_CALL(get_decimation(out));
}
int solo_engine_set_term_values(SoloEngine* eng, const double* values) {
  if (!values) return SOLO_ERR_INVALID_ARG;
  return ENG_CALL(set_term_values(values));
}
int solo_engine_get_term_fired(SoloEngine* eng, void** fired_dev) {
  if (!fired_dev) return SOLO_ERR_INVALID_ARG;
  return ENG_CALL(get_term_fired(fired_dev));
}
int solo_engine_set_actuators(SoloEngine* eng, const void* per_env_dev, void* stream) { return ENG_CALL(set_actuators(per_env_dev, (hipStream_t)stream)); }
int solo_engine_get_actuators(SoloEngine* eng, void** dev) {
  if (!dev) return SOLO_ERR_INVALID_ARG;
  return ENG_CALL(get_actuators(dev));
}
int solo_engine_set_base_wrench(SoloEngine* eng, const void* per_env_dev, void* stream) { return ENG_CALL(set_base_wrench(per_env_dev, (hipStream_t)stream)); }
int solo_engine_get_base_wrench(SoloEngine* eng, void** dev) {
  if (!dev) return SOLO_ERR_INVALID_ARG;
  return ENG_CALL(get_base_wrench(dev));
}
const char* solo_engine_last_error(SoloEngine* eng) { return eng && eng->impl ? eng->impl->err.c_str() : "invalid engine handle"; }

}  // extern "C"
#endif  // !SOLO_TU_F64
