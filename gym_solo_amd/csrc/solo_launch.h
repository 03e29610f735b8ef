// solo_launch.h — from "a rollout of K steps with these flags" to a sequence of kernel launches: the launch policy, the choice
// of the step-kernel instantiation, the KBuffers wiring of every launch and the packing of the control block and the terrain.
// Host-only, plain C++17, no HIP runtime call: the engine (solo_engine.hip) enqueues what this header plans, and the CPU
// emulator (tests/emu/emu_harness.cpp) executes the same plan, so the CPU suite runs the product's wiring.
// Include after solo_step_kernel.h (with_step_kernel names the kernels).
#pragma once

#include <string>

#include "solo_kernel_params.h"

namespace solo {

constexpr int kMaxStreams = 8;   // the most slices (internal HIP streams) of a rollout

// ---- THE LAUNCH POLICY (round 5: it was bench.py's).  A rollout of k steps runs as `launches` fused launches of S steps
//      per slice, `slices` independent launch chains, robots migrating every `migrate` steps of a launch (0: never).
//      Configured values are taken as they are; -1 = the engine chooses, from what was measured on the benchmark workload
//      (profiles/round5_launch_policy_f32_8192.log, profiles/round5_baseline_configs_f64.log):
//        * S = min(k, 250): the state record never leaves LDS inside a launch, and 250 steps average out the robots'
//          unequal solver costs (1.8e8 env-steps/s against 1.2e8 at 20 steps per launch, f64);
//        * two slices when the rollout takes several launches (one slice's launch boundary and tail overlap the other's
//          work: +1 ... 2 %), one when it is a single launch (halves of a single launch only shorten each other's tails);
//          a rollout that FUSES into one launch per slice has no boundaries left to overlap, and was measured both ways with progress
//          pacing on (profiles/progress_pacing_ab.log, 4096 robots, 3000 steps, two calls): f64 2.2509e8 / 2.2476e8 on two slices
//          against 2.2446e8 / 2.2523e8 on one (+0.3 % and -0.2 %, A/A spread 0.04 ... 0.5 %), f32 4.1006e8 / 4.1039e8 against
//          4.0981e8 / 4.0923e8 (+0.1 % / +0.3 %, spread 0.0 ... 0.3 %) - no side wins by three spreads in both precisions: two stay;
//        * no migration while every robot of a launch has a wave slot of its own - 4096 robots: four waves on each of the
//          1024 SIMDs in BOTH precisions since round 5 (f64 round 4: three - 3072 slots - and migration was worth +16 %):
//          with all robots resident a hand-over only costs; beyond that, in f64, two chunks per launch (several launches:
//          chunks of 25 steps on ONE chain) let the waves that finish early take over the robots that started late
//          (f32: never - measured slower).
//      CONTROL DECIMATION (PlanInput::decimation = D > 1; solo_engine_set_decimation): k, S and every other count are CONTROL
//      steps of D physics steps each.  S = min(k, max(1, 250 / D)) keeps a launch's physics length at what was measured
//      (DESIGN.md section 11 has the measurement for D = 4), and robots never migrate (-1 resolves to 0; an explicit value is
//      rejected by the setters).  The same holds while the program has a state termination or an actuator or a base wrench block
//      is on.
//      FUSED SEGMENTS (Plan::fuse; PlanInput::fuse switches the policy on - the engine does, the emulator harnesses of the other
//      kernels do not): a launch boundary is a barrier for its slice - launch j + 1 cannot start before the slowest robot of
//      launch j has finished, and at 4096 robots, all resident, nothing else can use the wave slots that wait (a wave lives
//      1.24 ... 1.28 x the mean at S = 250: profiles/fused_segments_tail_parent.log).  Nothing of the boundary is needed by the
//      result, so up to kMaxFusedSegments consecutive S-step launches of a slice run as ONE launch of solo_roll_kernel, whose waves
//      run the output epilogue after every S steps and go on: `launches` still counts the S-step SEGMENTS per slice, for_each_launch
//      yields one Launch per group of `fuse` of them.  Only the plain position-control step with the default solver, on rollouts
//      of several launches of at least two steps that leave records; everything else keeps its launches (fuse = 0).
//      PROGRESS PACING (KBuffers::progress; solo_step_body.h, the segment boundary): a rollout that is ONE fused launch per slice
//      (k <= fuse x S) shares one block of kMaxFusedSegments counters between its slices; at the end of segment s a wave counts
//      itself in counter s and learns its rank among all robots of the rollout, which sets its issue priority for the next segment.
//      The engine owns the block (progress_ints; allocated with the scratch, zeroed in front of the rollout) and hands it over in
//      EngineBuffers::progress; a rollout of several fused launches per slice - whose launches would count into the same counters
//      at different times - and every unfused plan get none, and a launch without the block runs as it did before it existed.
constexpr int kMaxFusedSegments = 16;   // segments per kernel launch: 4000 steps at S = 250, below 0.1 s at today's rate - a barrier that rare costs what none costs
struct Plan { int S, launches, slices, migrate; int fuse = 0; };

// what the policy reads: the batch, the precision, the robots with a wave slot of their own on the device (the emulator has
// no such limit: it passes n), SoloConfig's three geometry fields, what is switched on, and the rollout
struct PlanInput {
  int n;
  size_t real_bytes;   // sizeof(T)
  int resident;
  int32_t steps_per_launch, rollout_streams, migrate_steps;
  bool ctl_active, sensing;
  int k;
  uint32_t flags;
  int decimation = 1;   // physics steps per control step (k and steps_per_launch count control steps)
  bool state_terms = false;   // the program holds a state termination (solo_term_kernel: its robots never migrate)
  bool actuators = false;     // an actuator block is on (solo_act_kernel: its robots never migrate)
  bool wrench = false;        // a base wrench block is on (solo_push_kernel: its robots never migrate)
  bool fuse = false;          // the caller runs fused segments (solo_roll_kernel) where the policy allows them (the engine: with the default solver)
};

inline bool leaves_records(uint32_t flags);

inline Plan make_plan(const PlanInput& in) {
  const int n = in.n, k = in.k;
  const uint32_t flags = in.flags;
  // steps per fused launch, capped so that the records of one launch stay below 2^32 elements (the step kernel
  // addresses them with 32-bit offsets; at 4096 robots that is 32768 steps)
  const long long cap = ((1ll << 32) - 1) / ((long long)n * SOLO_STATE_STRIDE);
  const int decim = in.decimation > 1 ? in.decimation : 1;
  const int S_auto = 250 / decim > 1 ? 250 / decim : 1;
  long long want = in.steps_per_launch == -1 ? (k < S_auto ? k : S_auto) : (in.steps_per_launch > 1 ? in.steps_per_launch : 1);
  if (want > k && k > 0) want = k;
  Plan p;
  p.S = (int)(want < cap ? want : (cap > 1 ? cap : 1));
  if (p.S < 1) p.S = 1;
  p.launches = (k + p.S - 1) / p.S;
  const bool physics_only = flags == SOLO_STEP_PHYSICS;   // (stepSimulation-only launches - the settle loop - never migrate: their robots are in step)
  int streams = in.rollout_streams == -1 ? (p.launches > 1 ? 2 : 1) : in.rollout_streams;
  streams = streams < 1 ? 1 : (streams > kMaxStreams ? kMaxStreams : streams);
  p.migrate = 0;
#ifndef SOLO_STAMPS   // (never in the diagnostic stamps builds, whose per-wave stamps assume one robot per wave)
  if (decim > 1 || in.state_terms || in.actuators || in.wrench) p.migrate = 0;
  else if (in.migrate_steps > 0) p.migrate = in.migrate_steps;
  else if (in.migrate_steps == -1 && !physics_only && (flags & SOLO_STEP_PHYSICS) && p.S >= 8 && !in.ctl_active && !in.sensing) {   // (the control modes and contact sensing never migrate)
    // (8192 robots, f64, profiles/round5_baseline_configs_f64.log: one launch of 20 steps 1.485e8 in two chunks against
    // 1.474e8 without; 1000 steps 1.995e8 as one chain in chunks of 25 against 1.956e8 on two slices, 1.76e8 on one chain)
    // f32 at 8192 robots: migration costs 2.6 % (K = 20) / 3.8 % (1000 steps) - its robot-steps are short against a
    // hand-over (profiles/round5_launch_policy_f32_8192.log): f64 only
    if (n > in.resident && in.real_bytes == 8) {
      if (p.launches == 1) p.migrate = (p.S + 1) / 2;
      else if (p.S >= 50) { p.migrate = 25; if (in.rollout_streams == -1) streams = 1; }
    }
  }
#endif
  p.slices = (streams > 1 && n >= 2 * streams) ? streams : 1;
  // fused segments: several launches of the plain position-control step (S = 1 keeps its single-step launches and their
  // in-place outputs), whose flags leave records - the epilogue is what a segment ends with - and step the physics
  p.fuse = 0;
#if !defined(SOLO_STAMPS) || defined(SOLO_STAMPS_LIGHT)   // (never in the stamps builds with per-step accumulators)
  if (in.fuse && p.launches > 1 && p.S > 1 && p.migrate == 0 && !in.ctl_active && !in.sensing && decim == 1 && !in.state_terms &&
      !in.actuators && !in.wrench && leaves_records(flags) && (flags & SOLO_STEP_PHYSICS))
    p.fuse = p.launches < kMaxFusedSegments ? p.launches : kMaxFusedSegments;
#endif
  return p;
}

// progress pacing: the counters a plan needs of the engine (0: none), and whether a rollout of k steps under it is paced
static_assert(kMaxFusedSegments == kProgressCounters, "one counter per segment of a fused launch");
inline size_t progress_ints(const Plan& p) { return p.fuse > 0 ? (size_t)kMaxFusedSegments : 0; }
inline bool rollout_is_paced(const Plan& p, int k) { return p.fuse > 0 && k <= p.fuse * p.S; }

// the most slices a rollout can be cut into under this configuration (what a launch order has to respect)
inline int max_slices(int n, int32_t rollout_streams) {
  const int streams = rollout_streams == -1 ? 2 : (rollout_streams < 1 ? 1 : (rollout_streams > kMaxStreams ? kMaxStreams : rollout_streams));
  return (streams > 1 && n >= 2 * streams) ? streams : 1;
}

// the robots [lo, hi) of slice g of `groups`
inline int slice_begin(int n, int g, int groups) { return (int)((long long)n * g / groups); }

// ints of the migration queue per robot (its sweep counter + its ring slots), for EVERY launch of a chain whose launches
// fuse up to S steps: the chunk count is not monotone in the step count - migration_chunk_steps stretches the chunks of a
// launch that would need more than 127 (a ring slot has 7 bits for the chunk index), so a ragged last launch of fewer steps
// can need MORE chunks than the full ones (S = 128, migrate 1: 64 chunks of 2; a 65-step tail: 65 chunks of 1) - but no
// launch ever has more than min(127, ceil(S / migrate)) (the regions were sized and strided for the S-step
// launch's count, and such a tail wrote past its slice's region).  The same expression sizes the allocation and strides
// the slices' regions (wire_launch), which asserts that every launch's queue fits.
inline int queue_slots_per_robot(const Plan& p) {
  const int chunks = migration_chunks(p.S, p.migrate);
  return 1 + (chunks < 127 ? chunks : 127);
}

// ---- what a plan needs of the lazily sized scratch: the step records [N][S][32] of launches that leave records (any
//      observation or reward output), the foot forces of those steps [N][S][4] (contact sensing), and the migration queues
//      (a header per possible slice + every robot's slots), in ints; 0 = no queue
inline bool leaves_records(uint32_t flags) { return (flags & (SOLO_STEP_OBS | SOLO_STEP_REWARD)) != 0; }
inline size_t record_reals(int n, int steps) { return (size_t)steps * (size_t)n * SOLO_STATE_STRIDE; }
inline size_t foot_force_reals(int n, int steps) { return (size_t)steps * (size_t)n * 4; }
inline size_t queue_ints(int n, const Plan& p) {
  return p.migrate > 0 ? (size_t)kMaxStreams * kQueueHeader + (size_t)n * (size_t)queue_slots_per_robot(p) : 0;
}

// every rollout of up to k steps under one configuration: steps per launch grow with the rollout up to the cap, and the
// migration policy depends on the number of launches - the geometries of 1 .. k steps reduce to a handful.  f(plan) for each
// distinct one; stops at the first non-zero status and returns it.
template <class F>
inline int for_each_geometry(PlanInput in, int k, F&& f) {
  // (the slices belong to the geometry - a rollout of one launch runs on one slice, the same S over several launches on
  // two, and whoever prepares for the geometries has to see both; so do the fused segments)
  int last_S = -1, last_m = -1, last_slices = -1, last_fuse = -1;
  for (int kk = 1; kk <= k; kk = (kk < 512 ? kk + 1 : (kk * 2 < k ? kk * 2 : (kk == k ? k + 1 : k)))) {
    in.k = kk;
    const Plan p = make_plan(in);
    if (p.S == last_S && p.migrate == last_m && p.slices == last_slices && p.fuse == last_fuse) continue;
    last_S = p.S; last_m = p.migrate; last_slices = p.slices; last_fuse = p.fuse;
    if (int rc = f(p)) return rc;
  }
  return 0;
}

// ---- THE KERNEL CHOICE.  One step-kernel instantiation: solo_step_kernel<T, full, resid, migrate> (position control),
//      solo_ctl_step_kernel<T, full> (torque / PD), solo_contact_kernel<T, full, ctl> (contact sensing, in every mode) or
//      solo_decim_kernel<T, full, ctl> (control decimation, in every mode) or solo_term_kernel<T, full, ctl> (a program with a
//      state termination, in every mode and with any decimation) or solo_act_kernel<T, full, ctl> (an actuator block is on, in
//      every mode, with any decimation and any program) or solo_push_kernel<T, full, ctl> (a base wrench block is on: the
//      actuator kernel's body plus the wrench), or solo_roll_kernel<T> (a SEGMENTED launch of the full position-control step with the
//      default solver: wire_launch set KBuffers::seg_steps).
enum KernelFamily : int { KERNEL_STEP = 0, KERNEL_CTL = 1, KERNEL_CONTACT = 2, KERNEL_DECIM = 3, KERNEL_TERM = 4, KERNEL_ACT = 5, KERNEL_PUSH = 6, KERNEL_ROLL = 7 };
struct KernelId {
  KernelFamily family;
  bool full, resid, migrate, ctl;
};

// stepSimulation-only calls (settle loop, client.stepSimulation()) run the physics-only instantiation: no termination code,
// and a separate name in profiles; pybullet's residual threshold, an opt-in, is a kernel instantiation of its own (the
// default kernels carry none of it), and so is robot migration - always the full kernel: kFull only selects code.  The
// contact-sensing and torque / PD kernels never run with the residual threshold, warm start or a queue (set_control and
// set_contact_sensing reject the configurations), and never in the settle loop, which is position-controlled in every mode.
// The decimation kernels (decimation > 1) run every launch that steps the physics outside the settle loop - the settle loop
// stays in physics steps, and a launch without SOLO_STEP_PHYSICS has nothing to decimate -, never with any of the above
// (set_decimation rejects the configurations).
// The termination kernels (the program holds a state termination) run every launch outside the settle loop that steps the
// physics or evaluates the terminations - with D >= 1 substeps, so in place of the decimation kernels too -, never with the
// residual threshold, warm start, a queue or contact sensing (set_program rejects the configurations).
// The actuator kernels (solo_engine_set_actuators: a block is on) run every launch outside the settle loop that steps the physics
// or evaluates state terminations - with D >= 1 substeps and any program, so in place of the termination, decimation, control and
// position kernels -, never with the residual threshold, warm start, a queue or contact sensing (set_actuators rejects the
// configurations).  A launch that only evaluates a program without a state kind reads no motor: it keeps its kernel.
// The push kernels (solo_engine_set_base_wrench: a block is on) run every launch outside the settle loop that steps the physics -
// the actuator kernel's body plus the wrench, so in place of every family above, with the actuator block on or off (off: the
// engine points KParams::actuators at an all-ones block) -, never with the residual threshold, warm start, a queue or contact
// sensing (set_base_wrench rejects the configurations).  A launch without SOLO_STEP_PHYSICS applies no force: it keeps its kernel.
// The roll kernel runs the launches that make_plan fused (segmented: the launch has more steps than a segment) - where every
// family above would have chosen solo_step_kernel<T, true, false, false>, and nowhere else.
inline KernelId choose_kernel(bool sensing, bool ctl_active, bool settling, bool resid, bool has_queue, uint32_t flags, int decimation = 1,
                              bool state_terms = false, bool actuators = false, bool wrench = false, bool segmented = false) {
  const bool full = flags != SOLO_STEP_PHYSICS;
  if (wrench && !settling && (flags & SOLO_STEP_PHYSICS)) return {KERNEL_PUSH, full, false, false, ctl_active};
  if (actuators && !settling && ((flags & SOLO_STEP_PHYSICS) || (state_terms && (flags & SOLO_STEP_DONE)))) return {KERNEL_ACT, full, false, false, ctl_active};
  if (state_terms && !settling && (flags & (SOLO_STEP_PHYSICS | SOLO_STEP_DONE))) return {KERNEL_TERM, full, false, false, ctl_active};
  if (decimation > 1 && !settling && (flags & SOLO_STEP_PHYSICS)) return {KERNEL_DECIM, full, false, false, ctl_active};
  if (sensing && !settling) return {KERNEL_CONTACT, full, false, false, ctl_active};
  if (ctl_active && !settling) return {KERNEL_CTL, full, false, false, true};
  if (has_queue) return {KERNEL_STEP, true, resid, true, false};
  if (segmented && full && !resid) return {KERNEL_ROLL, true, false, false, false};
  return {KERNEL_STEP, full, resid, false, false};
}

// the kernel's name as profilers print it (solo_engine_kernel_name)
inline std::string kernel_name(const KernelId& id, size_t real_bytes) {
  const auto b = [](bool v) { return v ? ", true" : ", false"; };
  const std::string real = real_bytes == 4 ? "float" : "double";
  switch (id.family) {
    case KERNEL_CONTACT: return "solo_contact_kernel<" + real + b(id.full) + b(id.ctl) + ">";
    case KERNEL_CTL: return "solo_ctl_step_kernel<" + real + b(id.full) + ">";
    case KERNEL_DECIM: return "solo_decim_kernel<" + real + b(id.full) + b(id.ctl) + ">";
    case KERNEL_TERM: return "solo_term_kernel<" + real + b(id.full) + b(id.ctl) + ">";
    case KERNEL_ACT: return "solo_act_kernel<" + real + b(id.full) + b(id.ctl) + ">";
    case KERNEL_PUSH: return "solo_push_kernel<" + real + b(id.full) + b(id.ctl) + ">";
    case KERNEL_ROLL: return "solo_roll_kernel<" + real + ">";
    default: return "solo_step_kernel<" + real + b(id.full) + b(id.resid) + b(id.migrate) + ">";
  }
}

// THE ONE SWITCH: the only place that spells the step-kernel instantiations (twenty-nine per precision).  f(kernel) receives the
// kernel as a function pointer: the engine launches it, the emulator calls it.
template <typename T>
using StepKernel = void (*)(const KParams<T>*, KBuffers<T>);

template <typename T, class F>
inline void with_step_kernel(const KernelId& id, F&& f) {
  StepKernel<T> k;
  if (id.family == KERNEL_CONTACT) {
    if (id.ctl) k = !id.full ? solo_contact_kernel<T, false, true> : solo_contact_kernel<T, true, true>;
    else k = !id.full ? solo_contact_kernel<T, false, false> : solo_contact_kernel<T, true, false>;
  } else if (id.family == KERNEL_DECIM) {
    if (id.ctl) k = !id.full ? solo_decim_kernel<T, false, true> : solo_decim_kernel<T, true, true>;
    else k = !id.full ? solo_decim_kernel<T, false, false> : solo_decim_kernel<T, true, false>;
  } else if (id.family == KERNEL_TERM) {
    if (id.ctl) k = !id.full ? solo_term_kernel<T, false, true> : solo_term_kernel<T, true, true>;
    else k = !id.full ? solo_term_kernel<T, false, false> : solo_term_kernel<T, true, false>;
  } else if (id.family == KERNEL_ACT) {
    if (id.ctl) k = !id.full ? solo_act_kernel<T, false, true> : solo_act_kernel<T, true, true>;
    else k = !id.full ? solo_act_kernel<T, false, false> : solo_act_kernel<T, true, false>;
  } else if (id.family == KERNEL_PUSH) {
    if (id.ctl) k = !id.full ? solo_push_kernel<T, false, true> : solo_push_kernel<T, true, true>;
    else k = !id.full ? solo_push_kernel<T, false, false> : solo_push_kernel<T, true, false>;
  } else if (id.family == KERNEL_CTL) {
    k = !id.full ? solo_ctl_step_kernel<T, false> : solo_ctl_step_kernel<T, true>;
  } else if (id.family == KERNEL_ROLL) {
    k = solo_roll_kernel<T>;
  } else if (id.migrate) {
    k = id.resid ? solo_step_kernel<T, true, true, true> : solo_step_kernel<T, true, false, true>;
  } else if (!id.full) {
    k = id.resid ? solo_step_kernel<T, false, true> : solo_step_kernel<T, false, false>;
  } else {
    k = id.resid ? solo_step_kernel<T, true, true> : solo_step_kernel<T, true, false>;
  }
  f(k);
}

// ---- THE WIRING.  The buffers of the engine a launch is wired to ...
template <typename T>
struct EngineBuffers {
  T *state, *snapshot, *targets, *params;
  T *obs, *reward;            // the view [N][D] / [N] / [N]: the last step's outputs
  uint8_t* done;
  int32_t* term_count;
  double* stats;
  const T* terrain;           // or null
  const int32_t* order;       // the launch order in force, or null = identity
  int32_t* cost;
  T* warm;                    // the warm-start cache, or null = off
  int32_t* fault;
  T* traj;                    // the record scratch: traj_steps steps per robot
  int traj_steps;
  int32_t* queue;             // the migration queues: queue_len ints
  size_t queue_len;
  int n, obs_dim;
#ifdef SOLO_STAMPS
  unsigned long long* stamps;
#endif
  int32_t* progress = nullptr;   // the progress block of paced rollouts (progress_ints counters), or null = never paced
};

// ... the arguments of a rollout (act_stride: elements between the actions of consecutive steps - 0 repeats one action;
// the three outputs: the caller's [K][N][.] buffers of a recording rollout, each null when its flag is not set) ...
template <typename T>
struct RolloutArgs {
  const T* act;
  long long act_stride;
  int k;
  uint32_t flags;
  T *obs_out, *reward_out;
  uint8_t* done_out;
};

// ... and one launch of it: steps [i, i + steps) of robots [lo, lo + count), which are slice `slice` of the batch.
// final_chunk: the launch ends the rollout - a RECORDING rollout then has its epilogue also leave the last step's
// observation / reward / done in the engine's view (what three device-to-device copies after the chain used to do: ~15 us
// of a 0.4 ms 20-step rollout)
struct Launch {
  int i, steps, lo, count, slice;
  bool final_chunk;
};

// the most steps of one kernel launch under a plan: S, or plan.fuse segments of S steps
inline int launch_span(const Plan& plan) { return plan.fuse > 0 ? plan.fuse * plan.S : plan.S; }

// the launches of a whole rollout in issue order: launch-major, slice-minor.  Robots are independent, so the batch can be cut
// into plan.slices slices that advance through the K steps as independent launch chains (the engine: on their own HIP
// streams - one slice's kernel boundary / tail overlaps the other slices' work).  f(launch) for each; stops at the first
// non-zero status and returns it.
template <class F>
inline int for_each_launch(const Plan& plan, int n, int k, F&& f) {
  // (fused segments: one launch per group of plan.fuse S-step segments - wire_launch tells the kernel the segment length)
  const int S = launch_span(plan), groups = plan.slices;
  for (int i = 0; i < k; i += S)
    for (int g = 0; g < groups; ++g) {
      const int lo = slice_begin(n, g, groups), hi = slice_begin(n, g + 1, groups);
      if (int rc = f(Launch{i, (k - i < S) ? (k - i) : S, lo, hi - lo, g, i + S >= k})) return rc;
    }
  return 0;
}

// the work queue a migrating launch needs initialised in front of it (migration_queue_init for every i < ints); ints = 0: none
struct QueueInit {
  int32_t* q;
  size_t ints;
  int lo, count, rings, steps, chunk;
  const int32_t* order;
};

// fills the KBuffers of launch l (one wave per robot, l.steps fused steps; the kernel's output epilogue evaluates the step
// records the robot left).  false: the launch's migration queue does not fit its slice's region (never: see
// queue_slots_per_robot).
template <typename T>
inline bool wire_launch(const Plan& plan, const RolloutArgs<T>& a, const EngineBuffers<T>& e, const Launch& l, KBuffers<T>* out, QueueInit* qi) {
  const int n = e.n, i = l.i, steps = l.steps;
  const uint32_t flags = a.flags;
  KBuffers<T>& b = *out;
  b.state = e.state; b.snapshot = e.snapshot; b.targets = e.targets; b.actions = a.act ? a.act + (size_t)i * a.act_stride : nullptr;
  b.params = e.params; b.traj = nullptr; b.obs_inline = b.reward_inline = nullptr; b.done = e.done; b.term_count = e.term_count;
  b.obs_rec = b.reward_rec = b.view_obs = b.view_reward = nullptr; b.view_done = nullptr; b.obs_rec_stride = b.reward_rec_stride = 0; b.obs_from = 0;
  b.stats = e.stats; b.terrain = e.terrain; b.order = e.order; b.cost = e.cost; b.num_envs = n; b.flags = flags;
  b.env_base = l.lo; b.count = l.count; b.steps = steps;
  b.action_stride = a.act_stride; b.done_stride = 0;
  b.queue = nullptr; b.q_rings = 1; b.q_chunk = 0;
  b.fault = e.fault;
  b.warm = e.warm;
  // a launch of more steps than a segment (fused segments: for_each_launch) runs them S at a time, each segment on the
  // launch's region of the record scratch, which holds e.traj_steps >= S steps per robot as for any launch of S steps
  b.seg_steps = steps > plan.S ? plan.S : 0;
  // (progress pacing: every slice's launch of a rollout that is one fused launch per slice counts into the SAME block)
  b.progress = (b.seg_steps > 0 && rollout_is_paced(plan, a.k)) ? e.progress : nullptr;
#ifdef SOLO_STAMPS
  b.stamps = e.stamps;
#endif
  if (a.done_out) { b.done = a.done_out + (size_t)i * n; b.done_stride = n; }
  const bool want_obs = (flags & SOLO_STEP_OBS) != 0, want_reward = (flags & SOLO_STEP_REWARD) != 0;
  // a single-step launch (closed-loop step(), or a rollout with steps_per_launch = 1) evaluates its outputs
  // lane-parallel over the items of the one step; every other launch leaves records, which the robot's wave
  // evaluates after its last step (the output epilogue of the step kernel): where they go -
  const bool inline_outputs = steps == 1 && (want_obs || want_reward) && kInlineOutputs<T, true>;
  if (inline_outputs) {
    if (want_obs) b.obs_inline = a.obs_out ? a.obs_out + (size_t)i * n * e.obs_dim : e.obs;
    if (want_reward) b.reward_inline = a.reward_out ? a.reward_out + (size_t)i * n : e.reward;
  } else if (want_obs || want_reward) {
    // (the launch's own region of the record scratch, indexed by robot - first robot of the launch: the slices of
    // a rollout run side by side with DIFFERENT step counts when one of them is already in its ragged last launch -
    // indexed by absolute robot x steps of the launch their regions overlapped: a race that round 4's warm-start
    // test caught, tests/test_gpu_warm_start.py)
    b.traj = e.traj + (size_t)l.lo * (size_t)e.traj_steps * SOLO_STATE_STRIDE;
    // a recording rollout keeps every step ([K][N][.] buffers of the caller) and its last launch also leaves the
    // last step in the engine's view; otherwise only the last step's observation / reward / done stay in the view
    const bool tail_to_view = l.final_chunk;
    if (want_obs) {
      if (a.obs_out) { b.obs_rec = a.obs_out + (size_t)i * n * e.obs_dim; b.obs_rec_stride = (long long)n * e.obs_dim; if (tail_to_view) b.view_obs = e.obs; }
      else b.view_obs = e.obs;
    }
    if (want_reward) {
      if (a.reward_out) { b.reward_rec = a.reward_out + (size_t)i * n; b.reward_rec_stride = n; if (tail_to_view) b.view_reward = e.reward; }
      else b.view_reward = e.reward;
    }
    if (a.done_out && (flags & SOLO_STEP_DONE) && tail_to_view) b.view_done = e.done;
  }
  // robot migration: a launch of more than one chunk of steps gets a work queue (its own region per rollout slice:
  // the slices' launches run side by side), initialised in front of the step kernel; eight rings -
  // one per XCD - when the robots divide evenly, else one
  // (stepSimulation-only launches - the settle loop, client.stepSimulation() - keep the physics-only instantiation:
  // their robots are in step with each other, there is nothing to balance, and in profiles the settle loop stays a
  // kernel of its own instead of inflating the measured one's average)
  qi->ints = 0;
  if (plan.migrate > 0 && steps > plan.migrate && (flags & SOLO_STEP_PHYSICS) && flags != SOLO_STEP_PHYSICS) {
    const int chunk = migration_chunk_steps(steps, plan.migrate);
    b.q_chunk = chunk;
    b.q_rings = migration_rings(l.count);
    b.queue = e.queue + (size_t)l.slice * kQueueHeader + (size_t)l.lo * (size_t)queue_slots_per_robot(plan);
    const size_t ints = migration_queue_ints(l.count, steps, chunk);
    if (ints > (size_t)kQueueHeader + (size_t)l.count * (size_t)queue_slots_per_robot(plan) ||
        (size_t)(b.queue - e.queue) + ints > e.queue_len)   // (never: queue_slots_per_robot bounds every launch of <= S steps)
      return false;
    *qi = QueueInit{b.queue, ints, l.lo, l.count, b.q_rings, steps, chunk, e.order};
  }
  return true;
}

// The engine's view always ends up with the LAST step's outputs, also when every step was recorded: the last launch's
// epilogue writes them (wire_launch).  True for the recording rollouts that have to copy them out of the caller's buffers
// instead: those whose last launch is a single-step launch with in-place outputs (steps_per_launch = 1, or a one-step
// remainder of the launches - not of the segments inside a fused launch), and those that asked for neither observations nor rewards - their launches leave no records (no epilogue runs),
// the step kernel writes the done flags straight into the caller's [K][N] buffer.
template <typename T>
inline bool tail_needs_copy(const Plan& plan, int k, uint32_t flags) {
  // (fused segments: the ragged last SEGMENT of a launch goes through that launch's epilogue, a one-step one too - only a
  // last LAUNCH of one step evaluates in place)
  const int span = launch_span(plan);
  const int last_steps = (k % span == 0) ? span : k % span;
  return !leaves_records(flags) || (last_steps == 1 && kInlineOutputs<T, true>);
}

// ---- THE PACKING of the joint control mode (solo_engine_set_control) and of the heightfield ground (solo_engine_set_terrain;
//      null = the flat plane) into the parameter block; the heights themselves travel in KBuffers::terrain
template <typename T>
inline void pack_control(const SoloConfig& cfg, const SoloControl& c, KParams<T>* P) {
  CtlConst<T>& k = P->ctl;
  k.mode = c.mode;
  for (int d = 0; d < SOLO_NUM_DOF; ++d) { k.kp[d] = (T)c.kp[d]; k.kd[d] = (T)c.kd[d]; }
  k.action_scale = (T)(c.mode == SOLO_CTRL_POSITION ? cfg.action_scale : c.action_scale);   // (position mode keeps the configuration's scale)
  for (int j = 0; j < SOLO_NUM_JOINTS; ++j) k.reset_cmd[j] = (T)(c.mode == SOLO_CTRL_TORQUE ? 0.0 : cfg.settle_targets[j]);
}

// ---- ACTUATOR RANDOMISATION (solo_engine_set_actuators): what the setter checks before anything is touched.  The block's values
//      [n][SOLO_ACTUATOR_WIDTH], on the host: finite and >= 0 (the reserved column is kept as uploaded, and held to the same rule) ...
template <typename T>
inline int validate_actuators(const T* host, int n, std::string* err) {
  for (size_t i = 0; i < (size_t)n * SOLO_ACTUATOR_WIDTH; ++i)
    if (!(host[i] >= T(0) && host[i] < (T)INFINITY)) {
      if (err) *err = "actuator scales must be finite and >= 0 (robot " + std::to_string(i / SOLO_ACTUATOR_WIDTH) + ", column " + std::to_string(i % SOLO_ACTUATOR_WIDTH) + ")";
      return SOLO_ERR_INVALID_ARG;
    }
  return SOLO_OK;
}
// ... and the configurations a block does not run with (the actuator kernels carry none of that code)
inline int actuators_conflict(const SoloConfig& cfg, bool sensing, std::string* err) {
  auto fail = [&](const char* s) { if (err) *err = s; return (int)SOLO_ERR_INVALID_ARG; };
  if (cfg.migrate_steps > 0) return fail("actuator randomisation does not support robot migration (migrate_steps > 0)");
  if (cfg.solver_residual_threshold > 0) return fail("actuator randomisation does not support solver_residual_threshold > 0");
  if (cfg.solver_warm_start > 0) return fail("actuator randomisation does not support solver_warm_start > 0");
  if (sensing) return fail("actuator randomisation does not support contact sensing: turn it off first");
  return SOLO_OK;
}

// ---- EXTERNAL BASE WRENCHES (solo_engine_set_base_wrench): what the setter checks before anything is touched.  The block's
//      values [n][SOLO_WRENCH_WIDTH], on the host, in the engine's precision: finite, of either sign (a value that overflowed
//      the precision arrives as an infinity; the reserved columns are kept as uploaded, and held to the same rule) ...
template <typename T>
inline int validate_base_wrench(const T* host, int n, std::string* err) {
  for (size_t i = 0; i < (size_t)n * SOLO_WRENCH_WIDTH; ++i)
    if (!(host[i] > -(T)INFINITY && host[i] < (T)INFINITY)) {
      if (err) *err = "base wrench values must be finite (robot " + std::to_string(i / SOLO_WRENCH_WIDTH) + ", column " + std::to_string(i % SOLO_WRENCH_WIDTH) + ")";
      return SOLO_ERR_INVALID_ARG;
    }
  return SOLO_OK;
}
// ... and the configurations a block does not run with (the push kernels carry none of that code)
inline int base_wrench_conflict(const SoloConfig& cfg, bool sensing, std::string* err) {
  auto fail = [&](const char* s) { if (err) *err = s; return (int)SOLO_ERR_INVALID_ARG; };
  if (cfg.migrate_steps > 0) return fail("base wrenches do not support robot migration (migrate_steps > 0)");
  if (cfg.solver_residual_threshold > 0) return fail("base wrenches do not support solver_residual_threshold > 0");
  if (cfg.solver_warm_start > 0) return fail("base wrenches do not support solver_warm_start > 0");
  if (sensing) return fail("base wrenches do not support contact sensing: turn it off first");
  return SOLO_OK;
}

template <typename T>
inline void pack_terrain(const SoloTerrain* t, KParams<T>* P) {
  P->c.terr_nx = P->c.terr_ny = 0;
  if (t == nullptr) return;
  P->c.terr_nx = t->nx; P->c.terr_ny = t->ny;
  P->c.terr_inv_cell = (T)(1.0 / t->cell);
  P->c.terr_ox = (T)t->origin[0]; P->c.terr_oy = (T)t->origin[1];
}

}  // namespace solo
