// solo_step_body.h — the body of the fused step kernels: solo::step_body, ONE function template that every step kernel of
// solo_step_kernel.h calls, and nothing else.  What a kernel is, is its template arguments:
//   solo_step_kernel<T, kFull, kResid, kMigrate>    position control                      (kCtl = kContact = kDecim = kTerms = false)
//   solo_ctl_step_kernel<T, kFull>                  torque / PD                           (kCtl)
//   solo_contact_kernel<T, kFull, kCtl>             contact sensing                       (kContact)
//   solo_decim_kernel<T, kFull, kCtl>               control decimation                    (kDecim)
//   solo_term_kernel<T, kFull, kCtl>                state terminations                    (kDecim and kTerms)
//   solo_act_kernel<T, kFull, kCtl>                 actuator randomisation                (kDecim, kTerms and kAct)
//   solo_push_kernel<T, kFull, kCtl>                external base wrenches                (kDecim, kTerms, kAct and kPush)
//   solo_roll_kernel<T>                             position control, segmented launch    (kFull and kSegments, nothing else)
// with kResid = kMigrate = false in all but the first.  A feature that is off compiles none of its code (if constexpr), and
// the variables that only a feature writes are dead without it.
// solo_step_kernel.h includes this header - once, behind physics_solve / physics_finish and in front of the kernels - and
// provides everything it names; like that header it relies on the translation unit for the wave primitives.
// (tests/emu/Makefile and tests/emu_kernel.py's staleness check list this file: an edit rebuilds the emulator library.)
#pragma once

namespace solo {

// Pin / Bin: the calling kernel's own parameters (Bin by reference to the kernel's by-value block: wave_cold_args reads the
// rarely used fields from the kernel's argument segment - one pointer, then that block).
template <typename T, bool kFull, bool kResid, bool kMigrate, bool kCtl, bool kContact, bool kDecim, bool kTerms, bool kAct = false, bool kPush = false, bool kSegments = false>
__device__ __forceinline__ void step_body(const KParams<T>* Pin, const KBuffers<T>& Bin) {
  static_assert(!kTerms || kDecim, "the termination kernels run the substep loop");
  static_assert(!kAct || (kTerms && !kContact && !kResid && !kMigrate), "the actuator kernels are termination kernels: slot 25 of s_leg is theirs, and no robot migrates");
  static_assert(!kPush || kAct, "the push kernels are actuator kernels: their body plus the wrench");
  static_assert(!kSegments || (kFull && !kResid && !kMigrate && !kCtl && !kContact && !kDecim && !kTerms && !kAct && !kPush), "the segmented kernel is the full position-control step: every other family needs its own register check");
  KBuffers<T> B = Bin;
  if (!kFull) B.flags = SOLO_STEP_PHYSICS;
  using R = Real<T>;
  __shared__ T s_state[SOLO_STATE_STRIDE];
  // ONE block: the whitened row vectors [64][kRS], their joint-space parts by leg slot [64][4 legs x 2] (see
  // physics_solve; zero except the row's own leg) and the per-row geometry [64][centre 3, radius] - the output epilogue
  // (where all three are dead) uses it as its 1024-value scratch
  constexpr int kRS = ColumnBank<T>::kRowStride;
  constexpr int kRowsReals = kRowBlockReals<T>;
  // (the geometry table has one entry per SPHERE - a contact's three rows share it - and an all-zero entry for the rows
  // that have none: as [64 rows][4] it was 2 KB of the f64 kernel's 13.2 KB, and 13.2 KB round up to eleven LDS
  // allocation granules of 1280 B: ELEVEN workgroups per CU where the registers allow twelve - round 5)
  constexpr int kGeoRows = SOLO_MAX_SPHERES + 1;
  __shared__ T s_blk[kRowsReals + kGeoRows * 4];
  static_assert(kRowsReals >= SOLO_MAX_REWARD_OPS * (kRowsReals / SOLO_MAX_REWARD_OPS < 32 ? kRowsReals / SOLO_MAX_REWARD_OPS : 32), "the output epilogue's scratch");
  T* const s_rowvec = s_blk;
  T (*const s_hext)[8] = ColumnBank<T>::kCompact ? nullptr : reinterpret_cast<T (*)[8]>(s_blk + 64 * kRS);
  __shared__ unsigned char s_rowleg[64];  // (slot space: the leg of every slot's row)
  T (*const s_rowgeo)[4] = reinterpret_cast<T (*)[4]>(s_blk + kRowsReals);
  __shared__ int32_t s_rowtype[64];  // (StepTables::rowtype)
  __shared__ T s_keep[32];
  __shared__ T s_leg[4][kLegSlots];
  // termination (termination.py:38-83), one lane per termination (lanes >= SOLO_MAX_TERMS: never fire):
  // s_cnt = TimeBased step counters, s_termlim = the count above which lane t fires (-1: always - a
  // Constant(True) -, INT_MAX: never), s_termtick = 1 for the lanes whose counter ticks (TimeBased)
  // (SOLO_MAX_TERMS entries each: as [64] they were 768 B for four live entries)
  __shared__ int s_cnt[SOLO_MAX_TERMS];
  __shared__ int s_termlim[SOLO_MAX_TERMS];
  __shared__ int s_termtick[SOLO_MAX_TERMS];
  // per-lane constant tables, staged ONCE per launch (a launch fuses many steps): the steps then
  // read them from LDS instead of paying a global-load latency each
  __shared__ LegConst<T> s_legc[4];
  __shared__ StepConst<T> s_const;          // the scalars a step reads (see solo_kernel_params.h)
  // coefficient table of Real<T>'s polynomials (f64 only: see Real<double>::sincos; f32 uses instruction literals)
  __shared__ T s_math[Real<T>::kTabSize > 0 ? Real<T>::kTabSize : 1];
  // CONTACT SENSING (kContact: solo_contact_kernel; every other kernel compiles none of it).  Its LDS: the
  // ground normal under each sphere [16][3] (heightfield only) - in f64 the tail of the row-vector block, which nothing
  // touches from the row phase to the end of the step (the f64 kernel's LDS is exactly eight granules, 10240 B), in f32 an
  // array of its own - and the foot normal forces of the step in the free slot 25 of s_leg.
  T* s_cnrm = nullptr;
  if constexpr (kContact) {
    static_assert(kReduceScratch + 3 * SOLO_MAX_SPHERES <= kRowBlockReals<double>, "the f64 ground normals fit the row-vector block");
    __shared__ T s_cnrm_own[3 * SOLO_MAX_SPHERES];
    if constexpr (sizeof(T) == 8) s_cnrm = s_blk + kReduceScratch;
    else s_cnrm = s_cnrm_own;
  }
  static_assert(kLegSlots == 26, "contact sensing keeps the foot forces in slot 25 of s_leg");
  // CONTROL DECIMATION (kDecim: solo_decim_kernel; every other kernel compiles none of it): a step of the
  // step loop is a CONTROL step - KParams::decimation physics steps under one action row, then ONE termination tick, record,
  // output evaluation and auto-reset.  The count is wave-uniform and re-read from the parameter block where it is used (a
  // scalar load): nothing of it lives in a vector register across physics_solve.
  // STATE TERMINATIONS (kTerms, next to kDecim: solo_term_kernel; every other kernel compiles none of it):
  // SOLO_T_HEIGHT_BELOW / SOLO_T_TILT_ABOVE test the state record after the control step's last physics step against
  // KParams::term_value[t], with term_param[t] as a grace count on a counter that ticks like a TimeBased one.  No LDS of their
  // own (the f64 kernel sits on exactly eight granules): s_termtick holds the lane's KIND here - whether a counter ticks is a
  // function of it -, and the threshold is loaded from the parameter block behind the control step's last physics_solve, so no
  // register pair lives across the solve.  The index of the termination that fired travels in bits >= 2 of the event word.
  // ACTUATOR RANDOMISATION (kAct, next to kDecim and kTerms: solo_act_kernel; every other kernel compiles none of it): the robot's
  // row of KParams::actuators is loaded with the prologue's other loads and staged ONCE per launch where the LDS has room (the
  // f64 kernel sits on exactly eight granules): the torque limit's scale in s_keep[30], the PD position gains' in s_keep[31], the
  // PD velocity gains' in slot 25 of every leg's s_leg row (free without contact sensing).  physics_solve reads them where
  // the motor rows use them: nothing of it lives in a vector register across the solve.  A program WITHOUT a state kind runs this
  // kernel too: its termination lanes then behave as the kernels' without kTerms, and KParams::term_fired is left alone.
  // EXTERNAL BASE WRENCHES (kPush, next to kDecim, kTerms and kAct: solo_push_kernel; every other kernel compiles none of it): no
  // LDS and no staging - the robot's row of KParams::wrench is wave-uniform and constant over the launch, and physics_solve loads
  // its six components from device memory every physics step, in front of the base-level sum that hides the latency, and adds
  // them where the base body's right-hand side is formed.  The row's address is formed at the call; nothing of the wrench lives
  // in a vector register across the solve.

  // (kAct: does the program hold a state kind?  From the staged kinds, where the answer is used - only then is term_fired written)
  auto state_program = [&]() -> bool {
    bool r = false;
#pragma unroll
    for (int t = 0; t < SOLO_MAX_TERMS; ++t) r = r || solo_term_kind_reads_state(s_termtick[t]);
    return r;
  };
  const int lane0 = lane_id();
  const int slot = block_id() + B.env_base;
  if (slot >= B.num_envs) return;
  // (wave_cold_args assumes the kernel's parameter layout - one pointer, then this block: checked on
  // two fields, so that a changed signature traps instead of reading garbage)
  if (wave_cold_args(Bin)->num_envs != B.num_envs || wave_cold_args(Bin)->steps != B.steps) __builtin_trap();
  // workgroup -> robot: the cost-balanced launch order if one is set (solo_engine_set_order: dispatch position ->
  // robot), else the XCD-contiguous map (xcd_contiguous, solo_kernel_params.h: the robots whose waves share an L2 are
  // neighbours in the batch, so their rows of the [step][robot][.] arrays complete each other's cache lines there)
  const int32_t* order = wave_cold_args(Bin)->order;
  // A TASK = one robot and a range of the launch's steps.  kMigrate = false: this workgroup's robot, all steps.
  // kMigrate (SoloConfig::migrate_steps; the queue: solo_kernel_params.h): chunks of q_chunk steps of whichever robot
  // is ready next, taken from the ring of this wave's XCD first - the wave loops over tasks until the rings hold no
  // ticket, and a robot moves from wave to wave as its record in device memory.  A kernel instantiation of its own:
  // the one-robot-per-wave kernels keep their straight-line code.
  int32_t* const queue = kMigrate ? wave_cold_args(Bin)->queue : nullptr;
  int env = 0, step_begin = 0, step_end = B.steps;
  bool last_chunk = true;   // this task ends the robot's launch: output epilogue, final bookkeeping
  int q_ring = 0, q_rings_left = 0, q_sweeps = 0, q_chunk_at = 0;
  int next_ticket = 0;      // the next task's ticket, taken with the publication of the previous one (see the end of the task loop)
  bool have_next = false;
  // kSegments (solo_roll_kernel): the task loop below also runs once per SEGMENT of seg_len steps of this wave's own robot - the
  // step loop, then the output epilogue on the record scratch of one segment - until step_end reaches B.steps.  Only the first
  // segment loads the tables, the state record and the counters (they stay in LDS), only the last one stores them; the priority
  // history (carry_sweeps over carry_steps steps) runs on across the segments.
  int seg_len = B.steps, carry_sweeps = 0, carry_steps = 0;
  if constexpr (kSegments) {
    const int seg = wave_cold_args(Bin)->seg_steps;   // (0: the launch is one segment)
    if (seg > 0 && seg < B.steps) seg_len = seg;
    step_end = seg_len;
    last_chunk = step_end == B.steps;
  }
  if constexpr (!kMigrate) env = order != nullptr ? wave_uniform(order[slot]) : B.env_base + xcd_contiguous(block_id(), B.count);
  else {
    // home ring: one of the rings of this wave's XCD (q_rings = 8 x rings per XCD, or 1)
    const int per_xcd = B.q_rings >= 8 ? B.q_rings >> 3 : 1;
    q_ring = B.q_rings >= 8 ? (wave_xcc_id() & 7) * per_xcd + (block_id() >> 3) % per_xcd : 0;
    q_rings_left = B.q_rings;
  }
#ifdef SOLO_STAMPS
  B.stamp_row = env;
#ifndef SOLO_STAMPS_LIGHT   // (the light build keeps the product's LDS footprint - 10240 B in f64: sixteen workgroups per CU - and its residency)
  __shared__ unsigned long long s_acc[17];
  if (lane0 < 17) s_acc[lane0] = lane0 == 16 ? __builtin_amdgcn_s_memtime() : 0ull;
  B.acc = s_acc;
  wave_sync();
#endif
#endif
  SOLO_STAMP(B, 0);
  // episodic statistics are sharded over SOLO_STATS_SHARDS rows: all robots of a batch finish
  // their episodes in the same step, and same-address atomics serialise at ~12 ns each
  // (the rarely touched buffers are re-read from the kernarg segment where they are used: wave_cold_args)
#define SOLO_STATS_ROW (wave_cold_args(Bin)->stats + (size_t)(env % SOLO_STATS_SHARDS) * SOLO_STATS_WIDTH)

  const KParams<T>* __restrict__ const P0 = Pin;
  // ---- the per-launch tables (per-leg / per-row / per-step constants, the polynomial coefficients): loaded ...
  constexpr int kLegWords = (int)(sizeof(LegConst<T>) * 4 / sizeof(T)), kLegLoads = (kLegWords + 63) / 64;
  constexpr int kConstWords = (int)(sizeof(StepConst<T>) / sizeof(int32_t)), kConstLoads = (kConstWords + 63) / 64;
  T leg_w[kLegLoads];
  int32_t const_w[kConstLoads];
  RowConst<T> row_w;
  T math_w = T(0);
  auto load_tables = [&]() {
    const T* leg_src = reinterpret_cast<const T*>(P0->leg);
    const int32_t* const_src = reinterpret_cast<const int32_t*>(&P0->c);
#pragma unroll
    for (int j = 0; j < kLegLoads; ++j) leg_w[j] = (lane0 + 64 * j < kLegWords) ? leg_src[lane0 + 64 * j] : T(0);
    row_w = P0->row[lane0];
#pragma unroll
    for (int j = 0; j < kConstLoads; ++j) const_w[j] = (lane0 + 64 * j < kConstWords) ? const_src[lane0 + 64 * j] : 0;
    if constexpr (Real<T>::kTabSize > 0) math_w = wave_math_table<T>(lane0 < Real<T>::kTabSize ? lane0 : 0);
  };
  // ... and staged into LDS
  auto store_tables = [&]() {
    T* leg_dst = reinterpret_cast<T*>(s_legc);
    int32_t* const_dst = reinterpret_cast<int32_t*>(&s_const);
#pragma unroll
    for (int j = 0; j < kLegLoads; ++j) if (lane0 + 64 * j < kLegWords) leg_dst[lane0 + 64 * j] = leg_w[j];
    const bool has_geo = row_w.type >= ROW_NORMAL && row_w.type <= ROW_TAN2;   // (row_w.dof: the row's model sphere)
    s_rowtype[lane0] = row_w.type | (row_w.body << 4) | ((has_geo ? row_w.dof : SOLO_MAX_SPHERES) << 8) | (leg_sum_entry(lane0 < 27 ? lane0 : 0) << 16);
    if (row_w.type == ROW_NORMAL) {
#pragma unroll
      for (int i = 0; i < 3; ++i) s_rowgeo[row_w.dof][i] = row_w.center[i];
      s_rowgeo[row_w.dof][3] = row_w.radius;
    }
    if (lane0 < 4) s_rowgeo[SOLO_MAX_SPHERES][lane0] = T(0);
#pragma unroll
    for (int j = 0; j < kConstLoads; ++j) if (lane0 + 64 * j < kConstWords) const_dst[lane0 + 64 * j] = const_w[j];
    if constexpr (Real<T>::kTabSize > 0) { if (lane0 < Real<T>::kTabSize) s_math[lane0] = math_w; }
  };
  // the termination tables, from the staged constants
  auto make_term_tables = [&]() {
    const int tl = lane0 & (SOLO_MAX_TERMS - 1);
    const int kind = s_const.term_kind[tl], param = s_const.term_param[tl];
    const bool mine = lane0 < s_const.num_terms;  // (num_terms <= SOLO_MAX_TERMS)
    if constexpr (kTerms) {
      // (a state kind: the grace count is the limit of its counter; s_termtick = the kind, 0 - SOLO_T_PERPETUAL - beyond the program)
      if (lane0 < SOLO_MAX_TERMS) {
        s_termlim[lane0] = (mine && (kind == SOLO_T_TIME || solo_term_kind_reads_state(kind))) ? param : ((mine && kind == SOLO_T_CONST && param != 0) ? -1 : 0x7fffffff);
        s_termtick[lane0] = mine ? kind : SOLO_T_PERPETUAL;
      }
    } else {
      if (lane0 < SOLO_MAX_TERMS) {
        s_termlim[lane0] = (mine && kind == SOLO_T_TIME) ? param : ((mine && kind == SOLO_T_CONST && param != 0) ? -1 : 0x7fffffff);
        s_termtick[lane0] = (mine && kind == SOLO_T_TIME) ? 1 : 0;
      }
    }
  };
  if constexpr (kMigrate) {  // once per wave, in front of the task loop
    load_tables();
    store_tables();
    wave_sync();
    make_term_tables();
  }
  do {  // ---- the task loop (kMigrate; else one pass)
  if constexpr (kMigrate) {
    // a ticket of the current ring; a ring without tickets sends the wave on to the next one, and a whole round of
    // empty rings ends it
    const int chunks = migration_chunks(B.steps, B.q_chunk), per_ring = B.count / B.q_rings, ring_len = per_ring * chunks;
    int32_t* const ring_slots = queue + kQueueHeader + (size_t)B.count;
    // (a ticket is taken when the wave is FREE - at the earliest together with the publication of its previous task,
    // below -, never while it still works: a ticket reserved during the last step of a task is matched with a robot in
    // reservation order, not in the order waves become free, and waves then wait for "their" robot while others are
    // ready - measured: slower at every chunk length)
    int ticket = ring_len;
    bool tried = false;
    if (have_next) { ticket = next_ticket; tried = true; have_next = false; }
    for (;;) {
      if (ticket < ring_len) break;
      if (tried) { if (--q_rings_left <= 0) break; q_ring = q_ring + 1 == B.q_rings ? 0 : q_ring + 1; }
      // (the ring the wave is on: one read-modify-write - one device-scope round trip; a ring it walks on to at the
      // end of a launch is first looked at with a load: read-modify-writes of one address serialise at ~12 ns each,
      // and every wave ends by walking over every ring)
      if (lane0 == 0) {
        ticket = tried ? wave_atomic_load(queue + q_ring * 32) : 0;
        if (ticket < ring_len) ticket = wave_atomic_add(queue + q_ring * 32, 1);
      }
      ticket = wave_readlane_int(ticket, 0);
      tried = true;
    }
    if (ticket >= ring_len) break;
    // the slot of that ticket: published already unless more waves ask than robots are ready (the end of a launch).
    // BOUNDED wait: a wave that gives up counts itself in slot 6 of the statistics and leaves (never observed; a
    // launch must not hang on a bug)
    int ready = -1;
    for (int spin = 0; spin < SOLO_QUEUE_SPINS; ++spin) {
      if (lane0 == 0) ready = wave_atomic_load(ring_slots + (size_t)q_ring * ring_len + ticket);
      ready = wave_readlane_int(ready, 0);
      if (ready >= 0) break;
      wave_backoff();
    }
    if (ready < 0) {   // (the host finds the word set at its next call: SOLO_ERR_INCOMPLETE)
      if (lane0 == 0) { stats_add(&wave_cold_args(Bin)->stats[6], 1.0); if (wave_cold_args(Bin)->fault != nullptr) wave_fault_set(wave_cold_args(Bin)->fault); }
      break;
    }
    wave_acquire_device();  // (orders the loads of the robot's record and counters behind the poll)
    // the slot says which robot and which of its chunks: everything else is loaded in ONE round trip below
    env = B.env_base + (ready & 0xffffff);
    q_chunk_at = ready >> 24;
    step_begin = q_chunk_at * B.q_chunk;
    step_end = step_begin + B.q_chunk < B.steps ? step_begin + B.q_chunk : B.steps;
    last_chunk = step_end == B.steps;
  }
  const size_t rec = (size_t)env * SOLO_STATE_STRIDE;
  const bool first_seg = !kSegments || step_begin == 0;   // (kSegments: what is loaded once per launch is loaded in the first segment)
  // (lane = row keeps the joint-space parts of dead legs' slots at zero - they are written once: here, and again after
  // an output epilogue has used the block as scratch; slot space rewrites all eight every step)
  if constexpr (!ColumnBank<T>::kCompact) {
#pragma unroll
    for (int i = 0; i < 8; ++i) s_hext[lane0][i] = T(0);
  }
  // ---- the prologue's global loads, ALL ISSUED BEFORE THE FIRST ONE IS WAITED FOR (written as copy loops
  //      and load-then-store pairs they were eight exposed round trips to memory, one after the other:
  //      nothing in a fused launch, 17 % of a closed-loop step, which is a launch of its own)
  if constexpr (!kMigrate) { if (first_seg) load_tables(); }
  T state_w = T(0);
  int count_w = 0;
  if constexpr (kMigrate) {  // (what a robot travels as is read and written with device-coherent accesses: solo_wave_ops.h)
    if (lane0 < SOLO_STATE_STRIDE) state_w = wave_load_shared(wave_cold_args(Bin)->state + rec + lane0);
    if (lane0 < SOLO_MAX_TERMS) count_w = wave_atomic_load(wave_cold_args(Bin)->term_count + (size_t)env * SOLO_MAX_TERMS + lane0);
  } else if (first_seg) {
    if (lane0 < SOLO_STATE_STRIDE) state_w = wave_cold_args(Bin)->state[rec + lane0];
    if (lane0 < SOLO_MAX_TERMS) count_w = wave_cold_args(Bin)->term_count[(size_t)env * SOLO_MAX_TERMS + lane0];
  }
  // (contact sensing: the foot forces the record holds - what a launch without physics observes)
  T foot_w = T(0);
  if constexpr (kContact) { if (lane0 < 4) foot_w = P0->contact[((size_t)env * SOLO_MAX_SPHERES + 4 * lane0 + 1) * SOLO_CONTACT_WIDTH + 3]; }
  const T mu = wave_cold_args(Bin)->params[(size_t)env * 4 + 0];
  const T mass_scale = wave_cold_args(Bin)->params[(size_t)env * 4 + 1];
  const T mu_base = P0->mu_base;
  T act_w = T(1);   // (kAct) lane c < 3: column c of the robot's actuator row
  if constexpr (kAct) { if (lane0 < 3) act_w = P0->actuators[(size_t)env * SOLO_ACTUATOR_WIDTH + lane0]; }
  // issue priority (see physics_solve): a closed-loop step() is a launch of ONE step - it has no history
  // of its own, and its slowest robot, one that runs all the sweeps, decides how long the step takes.  A
  // robot's Gauss-Seidel cost is persistent, so such a launch starts from the sweep count of the robot's
  // previous step (fused launches build their own history: seeded the same way they were 4 % slower)
  int hist_w = 0, prio_steps = 0;
  // (control decimation: the cost of the robot's previous CONTROL step is the sweeps of its prio_unit physics steps)
  int prio_unit = 1;
  if constexpr (kDecim) prio_unit = wave_uniform(P0->decimation);
  if (B.steps == 1) {
    const int32_t* cost = wave_cold_args(Bin)->cost;
    if ((B.flags & SOLO_STEP_PHYSICS) && cost != nullptr) { hist_w = cost[env]; prio_steps = prio_unit; }
  }
  if constexpr (kMigrate) {  // (a migrating robot brings its history along: its sweeps so far in this launch)
    if (lane0 == 0) hist_w = wave_atomic_load(queue + kQueueHeader + (env - B.env_base));
    hist_w = wave_readlane_int(hist_w, 0);
    prio_steps = step_begin;
  }
  if constexpr (kSegments) { if (!first_seg) { hist_w = carry_sweeps; prio_steps = carry_steps; } }   // (the history of the segments behind it)
  // ---- ... and into LDS: the per-leg / per-row / per-step tables, the state record, the TimeBased counters
  //      (kept in scalar registers next to the termination program they cost 25 SGPR spills in the step loop)
  {
    if constexpr (!kMigrate) { if (first_seg) store_tables(); }
    if (first_seg) {
      if (lane0 < SOLO_STATE_STRIDE) s_state[lane0] = state_w;
      if (lane0 < SOLO_MAX_TERMS) s_cnt[lane0] = count_w;
    }
    // f64: the robot's friction coefficient and base-mass scale wait in LDS, not in two register pairs held across the
    // whole step loop (the f64 kernel lives on 168 VGPRs: see physics_solve, "PARK EARLY")
    if constexpr (sizeof(T) == 8) { if (lane0 == 0) { s_keep[27] = mu; s_keep[28] = mass_scale; } }
    if (lane0 == 0) s_keep[29] = mu_base;   // (the base link's own friction coefficient: physics_solve)
    if constexpr (kContact) { if (lane0 < 4) s_leg[lane0][25] = foot_w; }
    if constexpr (kAct) {
      if (lane0 < 2) s_keep[30 + lane0] = act_w;   // (SOLO_ACT_TORQUE_LIMIT, SOLO_ACT_KP)
      const T act_kd = wave_readlane(act_w, SOLO_ACT_KD);
      if (lane0 < 4) s_leg[lane0][25] = act_kd;
    }
  }
  int prio_sweeps = wave_uniform(hist_w);
  const int hist_sweeps = kMigrate ? 0 : prio_sweeps;   // (kSegments: re-based at every segment's start - cost[env] stays the sweeps of the last seg_len steps)
  int prio_rot = (prio_steps + wave_slot_id()) % 3;  // the rotation's phase (advanced once per step)
  // (a migrating robot's history is its sweeps over the prio_steps steps it has behind it in this launch; a single-step
  // launch's the sweeps of the robot's previous step)
  if (prio_steps > 0 && first_seg) wave_set_priority_level(prio_sweeps > kPrioSweeps<T> * (kMigrate ? prio_steps : prio_unit) ? 3 : wave_slot_id() % 3);
  wave_sync();
  if constexpr (!kMigrate) { if (first_seg) make_term_tables(); }
  // The auto-reset belongs to a step that advanced the simulation (or asks for it explicitly): a
  // query-only launch - TerminationFactory.is_terminated() outside step(), termination.py:38-50 - never
  // mutates the physics state.
  const bool may_restart = (B.flags & SOLO_STEP_DONE) && (B.flags & (SOLO_STEP_PHYSICS | SOLO_STEP_AUTO_RESET)) &&
                           wave_uniform(s_const.auto_reset) != 0;

  // B.steps consecutive env steps of THIS robot in one launch: the state record stays in LDS,
  // only actions come in and the step records / done flags go out per step.  Robots are independent, so
  // no wave ever waits for another one; a launch lasts as long as its slowest robot's SUM over
  // the steps, which averages out the contact-count imbalance between robots.
  wave_sync();  // the staged tables, the state record and the counters are in LDS
#pragma unroll 1
  for (int step = step_begin; step < step_end; ++step) {
    const StepConst<T>& C = s_const;  // (LDS: re-read every step, nothing carried across the step loop in registers)
    // per-lane address arithmetic stays in the step instead of being hoisted out of the fused step loop and kept live
    // across it (spills).  kLean (f64: the kernel lives on exactly 168 VGPRs, and what it spilled was reloaded from
    // scratch INSIDE the step - behind an s_waitcnt vmcnt(0) that also waited for the step's freshly issued action
    // load): the lane number itself is computed here (solo_wave_ops.h: wave_fresh_lane), "are there actions?" is a compare
    // on two scalar registers here instead of a flag parked in a vector register across the loop (only the test is
    // opaque: through an opaque pointer the loads became flat loads), the target's finiteness is looked at where the
    // target is used (physics_solve) instead of keeping it to the end of the step, and physics_finish re-derives its
    // LDS addresses.  f32 (0 spills without any of it, 1 % slower with it) keeps its code.
    constexpr bool kLean = sizeof(T) == 8;
    int lane = kLean ? wave_fresh_lane() : wave_opaque_lane(lane0);
    const bool have_actions = kLean ? wave_opaque_bits((unsigned long long)B.actions) != 0ull : B.actions != nullptr;
    const T* const actions = have_actions ? B.actions : nullptr;
    const StepTables<T> tabs = {s_legc, s_rowtype, s_rowgeo};
    // setJointMotorControlArray (solo8v2vanilla.py:87-90): every motor lane fetches the target of ITS
    // joint straight from global memory.  The value is consumed when the motor rows are built,
    // thousands of cycles into the step, so the load's latency is never waited for (funnelled
    // through LDS at the top of the step - or prefetched a step ahead into a register the compiler
    // then copies at once - it cost an exposed global-memory round trip per step).
    // (f64, round 5: the load is issued INSIDE physics_solve, behind the leg phase - the step's register peak - and still
    // ~3000 cycles in front of its use; at the top of the step its register pair was the first thing the 128-VGPR kernel
    // spilled)
    bool motor_lane = (s_rowtype[lane] & 15) == ROW_MOTOR;
    // (the robot's motor targets are written from several chunks - the last step's action, an auto-reset's settle pose -
    // and read back when a launch brings no actions: device-coherent accesses in a migrating launch, like its record)
    auto fetch_target = [&](int ln) -> T {   // action de-normalisation (solo8v2vanilla.py:84-85) included
      const size_t tgt_at = (size_t)env * SOLO_NUM_JOINTS + (size_t)(3 * (ln >> 4) + (ln & 15));  // pybullet joint index
      T raw_target = T(0);
      if ((ln & 15) < 2) {   // (the motor rows: k = 0, 1 of every leg - solo_kernel_params.h)
        if (actions != nullptr) raw_target = actions[(size_t)step * B.action_stride + tgt_at];
        else if constexpr (kMigrate) raw_target = wave_load_shared(wave_cold_args(Bin)->targets + tgt_at);
        else raw_target = wave_cold_args(Bin)->targets[tgt_at];
      }
      return raw_target * (actions != nullptr ? step_action_scale<T, kCtl>(s_const, P0) : T(1));
    };
    if (actions != nullptr && step == B.steps - 1 && lane < SOLO_NUM_JOINTS) {  // the view's targets: all 12 entries
      const T tv = actions[(size_t)step * B.action_stride + (size_t)env * SOLO_NUM_JOINTS + lane] * step_action_scale<T, kCtl>(C, P0);
      if constexpr (kMigrate) wave_store_shared(wave_cold_args(Bin)->targets + (size_t)env * SOLO_NUM_JOINTS + lane, tv);
      else wave_cold_args(Bin)->targets[(size_t)env * SOLO_NUM_JOINTS + lane] = tv;
    }

    // the warm-start cache (SoloConfig::solver_warm_start; residual-threshold kernels only): this lane's row's impulse at
    // the end of the robot's previous step, fetched now and used when the rows are built
    T* const warm_row = kResid ? wave_cold_args(Bin)->warm : nullptr;   // (wave-uniform; null = off)
    T warm_in = T(0);
    if constexpr (kResid) if (warm_row != nullptr && (B.flags & SOLO_STEP_PHYSICS)) {
      if constexpr (kMigrate) warm_in = wave_load_shared(warm_row + (size_t)env * 64 + lane);
      else warm_in = warm_row[(size_t)env * 64 + lane];
    }
    SOLO_STAMP(B, 1);
    bool diverged = false;
    T term_thr = T(0);   // (kTerms) lane t < SOLO_MAX_TERMS: the threshold of termination t (loaded below, behind the substep's physics_solve)
    // THE SUBSTEP LOOP (kDecim; every other kernel: ONE pass, see the break at its end): the control step's physics steps, all under action row
    // `step`; the motor rows are rebuilt (PD: the law re-evaluated) from the fresh state every time.  A substep that diverges
    // ends the control step: restored and counted once.
    int substeps = 1;
    if constexpr (kDecim) substeps = wave_uniform(P0->decimation);
#pragma unroll 1
    for (int sub = 0; sub < substeps; ++sub) {
    // (the lane is re-derived behind an opaque statement every substep, as at the top of every step: what is computed from a
    // lane that is invariant across the substeps - ~60 lane masks in f32 - is otherwise hoisted in front of this loop and spilled)
    if constexpr (kDecim) lane = kLean ? wave_fresh_lane() : wave_opaque_lane(lane0);
    if (B.flags & SOLO_STEP_PHYSICS) {
      const T my_target = kLean ? T(0) : fetch_target(lane);
      bool target_bad = false;  // (set on a motor lane whose target is not finite)
      int row_at;  // where this lane's constraint row sits in s_rowvec / s_hext (its lane, or its slot: see physics_solve)
      // (the pipelined column build: the default-solver kernels whose robots do not migrate - the others, with a value or two more
      // live across the step, would reload them from scratch inside it)
      const T lam = physics_solve<T, kResid, !kResid && !kMigrate, kCtl, kContact, kAct, kPush>(C, B, tabs, s_state, my_target, fetch_target, s_rowvec, s_hext, s_rowleg, s_keep, s_leg, s_math, mu, mass_scale, lane, row_at, target_bad, prio_sweeps, prio_steps, prio_rot,
                                             warm_in, kResid && warm_row != nullptr, kCtl ? &P0->ctl : nullptr, s_cnrm,
                                             kPush ? P0->wrench + (size_t)env * SOLO_WRENCH_WIDTH : nullptr);
      if constexpr (kResid) if (warm_row != nullptr) {
        if constexpr (kMigrate) wave_store_shared(warm_row + (size_t)env * 64 + lane, lam);
        else warm_row[(size_t)env * 64 + lane] = lam;
      }
      if constexpr (kLean) lane = wave_fresh_lane();   // (nothing lane-derived lives across physics_solve)
      // the thresholds, re-read every substep where the last one's is used: issued here, the load flies during physics_finish,
      // and the value of the previous substep is dead at the top of the next (nothing of it lives across physics_solve)
      if constexpr (kTerms) term_thr = P0->term_value[lane & (SOLO_MAX_TERMS - 1)];
      if constexpr (kContact) {
        // THE CONTACT RECORD: lam is the impulse of the row THIS lane built (lane = row, solo_kernel_params.h: a sphere's
        // normal, tangent-1 and tangent-2 rows on three neighbouring lanes of its leg's 16-lane row).  Each contact lane
        // turns its impulse into a world-frame force along its row's direction (flat plane: world z / x / y; heightfield:
        // the normal parked by the row phase, t1 = world x projected into the tangent plane, t2 = n x t1 - the row phase's
        // expressions), and the sphere's tangent-2 lane sums the three (two DPP shifts within the row).  A dead row's
        // impulse is 0, so is its force.
        const int rt = s_rowtype[lane] & 15, ck = lane & 15;
        const bool crow = rt >= ROW_NORMAL && rt <= ROW_TAN2;
        const T f = crow ? lam * C.inv_dt : T(0);
        T dx = rt == ROW_TAN1 ? T(1) : T(0), dy = rt == ROW_TAN2 ? T(1) : T(0), dz = rt == ROW_NORMAL ? T(1) : T(0);
        if (B.terrain != nullptr) {
          const T* cn = s_cnrm + 3 * (4 * (lane >> 4) + (crow ? (ck - 2) / 3 : 0));
          const V3<T> nw = {cn[0], cn[1], cn[2]};
          const T itn = R::rsqrt(T(1) - nw.x * nw.x);
          const V3<T> t1w = {(T(1) - nw.x * nw.x) * itn, -nw.x * nw.y * itn, -nw.x * nw.z * itn};
          const V3<T> t2w = cross(nw, t1w);
          const V3<T> dw = rt == ROW_NORMAL ? nw : (rt == ROW_TAN1 ? t1w : t2w);
          dx = dw.x; dy = dw.y; dz = dw.z;
        }
        const T fx = f * dx, fy = f * dy, fz = f * dz;
        const T cf_x = (fx + wave_lane_below<1>(fx)) + wave_lane_below<2>(fx);
        const T cf_y = (fy + wave_lane_below<1>(fy)) + wave_lane_below<2>(fy);
        const T cf_z = (fz + wave_lane_below<1>(fz)) + wave_lane_below<2>(fz);
        const T cf_n = wave_lane_below<2>(f);
        // (written at once - held across physics_finish they cost the f64 kernel scratch reloads inside the step; a robot
        // that this step restores or restarts has its entries zeroed again below, by the same lanes)
        if (rt == ROW_TAN2) {
          const int sph = 4 * (lane >> 4) + (ck - 2) / 3;
          T* const out = P0->contact + ((size_t)env * SOLO_MAX_SPHERES + sph) * SOLO_CONTACT_WIDTH;
          out[0] = cf_x; out[1] = cf_y; out[2] = cf_z; out[3] = cf_n;
          if ((sph & 3) == 1) s_leg[sph >> 2][25] = cf_n;
        }
      }
      physics_finish<T>(C, s_state, s_rowvec, s_keep, s_leg, s_math, lam, lane, row_at);
      // a robot whose state went non-finite - or that was handed a non-finite target, which the
      // solver's clamps would otherwise swallow silently - is restored from its snapshot and counted
      const bool bad = (lane < SOLO_S_RETURN && !R::finite(s_state[lane & 31])) || (kLean ? target_bad : (motor_lane && !R::finite(my_target)));
      diverged = wave_ballot(bad) != 0ull;
      if (diverged) {
        if constexpr (kResid) if (warm_row != nullptr) {  // (a restored robot starts from zero impulses)
          if constexpr (kMigrate) wave_store_shared(warm_row + (size_t)env * 64 + lane, T(0));
          else warm_row[(size_t)env * 64 + lane] = T(0);
        }
        if (lane < SOLO_S_RETURN) s_state[lane] = wave_cold_args(Bin)->snapshot[rec + lane];
        if (lane == 0) stats_add(&SOLO_STATS_ROW[5], 1.0);
        wave_sync();
      }
    }
    // (without kDecim the pass leaves through this break unconditionally: no back edge is ever emitted, and the optimiser sees
    // the straight-line step - left to delete a loop of trip count 1 itself, it allocated the f32 kernels' registers differently)
    if (!kDecim || diverged) break;
    }  // the substep loop

    SOLO_STAMP(B, 10);
    // ---- termination: OR with short-circuit, per-env TimeBased counters (termination.py:38-83).
    //      Lane t evaluates termination t on its own counter; once an earlier termination fires, the
    //      later ones are not ticked (termination.py:46-48).  Branch-free: ~14 instructions.
    bool done = false;
    int fired_index = 0;   // (kTerms) wave-uniform: 0 = none, else 1 + the index of the first termination that fired
    if constexpr (kTerms) {
      // (a launch without physics - a query - evaluates the terminations too: its load is here, behind the substep loop, so that no
      // path that defines the threshold joins another one inside the loop)
      if (!(B.flags & SOLO_STEP_PHYSICS)) term_thr = P0->term_value[lane & (SOLO_MAX_TERMS - 1)];
      // (state kinds: lane t also tests the state record - after a diverged robot's restore, before the auto-reset; c = 1 - 2 (qx^2 +
      // qy^2) with explicit fused multiply-adds, as euler_component: every inlined copy and the emulator give the same bits)
      if (B.flags & SOLO_STEP_DONE) {
        const int tl = lane & (SOLO_MAX_TERMS - 1);
        const bool term_lane = lane < SOLO_MAX_TERMS;
        const int old = s_cnt[tl], kind = s_termtick[tl];
        const T z = s_state[SOLO_S_POS + 2], qx = s_state[SOLO_S_QUAT], qy = s_state[SOLO_S_QUAT + 1];
        const T upz = R::fma(T(-2), R::fma(qx, qx, qy * qy), T(1));
        const bool holds = kind == SOLO_T_HEIGHT_BELOW ? z < term_thr : (kind == SOLO_T_TILT_ABOVE ? upz < term_thr : true);
        const unsigned long long fired = wave_ballot(term_lane && old + 1 > s_termlim[tl] && holds);
        done = fired != 0ull;
        const int first = done ? __builtin_ctzll(fired) : 63;  // wave-uniform
        const bool ticks = kind == SOLO_T_TIME || solo_term_kind_reads_state(kind);
        if (term_lane) s_cnt[tl] = old + ((ticks && lane <= first) ? 1 : 0);
        fired_index = done ? first + 1 : 0;
      }
    } else {
      if (B.flags & SOLO_STEP_DONE) {
        const int tl = lane & (SOLO_MAX_TERMS - 1);
        const bool term_lane = lane < SOLO_MAX_TERMS;
        const int old = s_cnt[tl];
        const unsigned long long fired = wave_ballot(term_lane && old + 1 > s_termlim[tl]);
        done = fired != 0ull;
        const int first = done ? __builtin_ctzll(fired) : 63;  // wave-uniform
        if (term_lane) s_cnt[tl] = old + ((s_termtick[tl] != 0 && lane <= first) ? 1 : 0);
      }
    }
    const int fired_bits = fired_index << 2;   // (the event word: kEventDone | kEventRestart | fired_index << 2; 0 without kTerms)
    const bool restart = may_restart && (done || diverged);
    if constexpr (kContact) {
      // a robot this step restores or restarts reads zeros (the record, and the foot forces of this step's observations);
      // then the foot forces go out per step of a launch that leaves records: KParams::contact_traj, the output epilogue's
      if (diverged || restart) {
        const int rt = s_rowtype[lane] & 15, sph = 4 * (lane >> 4) + ((lane & 15) - 2) / 3;
        if (rt == ROW_TAN2) {
          T* const out = P0->contact + ((size_t)env * SOLO_MAX_SPHERES + sph) * SOLO_CONTACT_WIDTH;
          // (a zero the compiler cannot see: a constant zero tuple for these stores was hoisted out of the step loop and spilled)
          const T zr = T(wave_opaque_lane(0));
          out[0] = zr; out[1] = zr; out[2] = zr; out[3] = zr;
          if ((sph & 3) == 1) s_leg[sph >> 2][25] = zr;
        }
      }
      wave_sync();
      if (B.traj != nullptr && lane < 4)
        P0->contact_traj[((size_t)env * P0->contact_traj_steps + step) * 4 + lane] = s_leg[lane][25];
    }
    // ---- the step's record for the output epilogue (end of this kernel): the state after the step, before
    //      an auto-reset, as ONE coalesced 32-real store; slot 31 carries the step's event bits (the
    //      epilogue turns them into the done flags and the episodic bookkeeping: no byte stores here)
    if (B.traj != nullptr) {
      const T ev = T((done ? kEventDone : 0) | (restart ? kEventRestart : 0) | fired_bits);
      const T word = s_state[lane & (SOLO_STATE_STRIDE - 1)];
      if (lane < SOLO_STATE_STRIDE)
        B.traj[(unsigned)(kSegments ? (env - B.env_base) * seg_len + (step - step_begin) : (env - B.env_base) * B.steps + step) * (unsigned)SOLO_STATE_STRIDE + (unsigned)lane] = lane == SOLO_S_SPARE ? ev : word;
    }
    // closed-loop step() = a single-step launch: its outputs are evaluated right here with the
    // same per-item functions the output epilogue uses (no second launch on the critical path of a
    // policy loop) - lane i takes observation element i / reward leaf i, lane 0 folds the reward
    // (both precisions - kInlineOutputs is kFull; physics-only instantiations compile none of it)
    if constexpr (kInlineOutputs<T, kFull>) if (B.obs_inline != nullptr || B.reward_inline != nullptr) {
      // lane i's observation element / reward instruction come from the parameter block in global memory:
      // loaded HERE so that the loads fly while the Euler angles are computed
      // (loaded where they are used they were three exposed round trips at the end of every closed-loop step)
      const int n_obs = wave_uniform(C.num_obs), n_rops = wave_uniform(C.num_reward_ops);
      // (lanes beyond a program load its entry 0 - one more address in an already issued load - and never use it)
      const ObsElemK<T> prog_obs = P0->obs[lane < n_obs ? lane : 0];
      const RewardInstrK<T> prog_reward = P0->reward[lane < n_rops ? lane : 0];
      // the three Euler angles on three LANES, one atan2 for all of them (solo_outputs.h: euler_component - the function the
      // output epilogue calls per angle, so the two paths agree bit for bit), broadcast to the wave
      const T angle = euler_component<T>(lane < 3 ? lane : 0, s_state[SOLO_S_QUAT], s_state[SOLO_S_QUAT + 1], s_state[SOLO_S_QUAT + 2], s_state[SOLO_S_QUAT + 3]);
      const T roll = wave_readlane(angle, 0), pitch = wave_readlane(angle, 1), yaw = wave_readlane(angle, 2);
      if (B.obs_inline != nullptr && lane < n_obs) {
        if constexpr (kContact) B.obs_inline[(size_t)env * n_obs + lane] = observation_value_foot<T>(prog_obs, s_state, roll, pitch, yaw, &s_leg[0][25], kLegSlots);
        else B.obs_inline[(size_t)env * n_obs + lane] = observation_value<T>(prog_obs, s_state, roll, pitch, yaw);
      }
      if (B.reward_inline != nullptr) {
        // lane i holds instruction i and its value: the leaves are evaluated lane-parallel, the
        // combining instructions (SCALE / ADD / MUL over earlier values, three-address form) in
        // program order with wave-uniform v_readlane broadcasts - no LDS, and no chain of dependent
        // scalar loads of the program on lane 0 (~14 x 250 cycles at the end of every closed-loop step)
        const RewardInstrK<T>& ri = prog_reward;  // (lanes >= n_rops hold a copy of instruction 0: evaluated, never read)
        T myval = reward_is_leaf(ri.op) ? reward_leaf<T>(ri, s_state, roll, pitch) : T(0);
        for (int i = 0; i < n_rops; ++i) {
          const int op = wave_readlane_int(ri.op, i);
          if (reward_is_leaf(op)) continue;                      // (wave-uniform)
          const int src = wave_readlane_int(ri.src, i);
          const T x0 = wave_readlane(myval, src & 255), x1 = wave_readlane(myval, (src >> 8) & 255);
          const T res = op == SOLO_R_SCALE ? wave_readlane(ri.a, i) * x0 : (op == SOLO_R_ADD ? x0 + x1 : x0 * x1);
          myval = (lane == i) ? res : myval;
        }
        const T reward_value = wave_readlane(myval, n_rops - 1);
        if (lane == 0) {
          const T r = reward_value;
          B.reward_inline[env] = r;
          if (B.flags & SOLO_STEP_DONE) {
            // episodic return / length live in the record's slots 29, 30: loaded with the state in the
            // prologue, updated here in LDS, stored with the state at the end of the launch
            const uint8_t ev = (uint8_t)((done ? kEventDone : 0) | (restart ? kEventRestart : 0));
            accumulate_returns<T>(s_state, &ev, 0, &r, 0, 1, SOLO_STATS_ROW, [](double* p, double x) { stats_add(p, x); });
          }
        }
      }
    }
    SOLO_STAMP(B, 11);
    if (B.flags & SOLO_STEP_DONE) {
      if (restart) {
        wave_sync();  // the record above is read from the old state first
        if (lane < SOLO_S_RETURN) s_state[lane] = wave_cold_args(Bin)->snapshot[rec + lane];
        if (lane < SOLO_MAX_TERMS) s_cnt[lane] = 0;
        if constexpr (kResid) if (warm_row != nullptr) {  // (... and so does a robot that starts a new episode)
          if constexpr (kMigrate) wave_store_shared(warm_row + (size_t)env * 64 + lane, T(0));
          else warm_row[(size_t)env * 64 + lane] = T(0);
        }
        // reset() leaves the motors commanded to the settle pose (solo8v2vanilla.py:127-136); kCtl: to the mode's reset command
        if (lane < SOLO_NUM_JOINTS) {
          if constexpr (kMigrate) wave_store_shared(wave_cold_args(Bin)->targets + (size_t)env * SOLO_NUM_JOINTS + lane, step_reset_command<T, kCtl>(C, P0, lane));
          else wave_cold_args(Bin)->targets[(size_t)env * SOLO_NUM_JOINTS + lane] = step_reset_command<T, kCtl>(C, P0, lane);
        }
      }
      // (a launch that leaves records has its done flags written by the output epilogue, from slot 31; one that keeps
      // only the view's flag - done_stride = 0 - writes the LAST step's: in a migrating launch the steps of a robot run
      // on waves of different XCDs, whose L2s would write their plain stores to the one byte back in any order)
      if (B.traj == nullptr && lane == 0 && (B.done_stride != 0 || step == B.steps - 1)) B.done[(size_t)step * B.done_stride + env] = done ? 1 : 0;
      if constexpr (kTerms) { if (B.traj == nullptr && lane == 0 && step == B.steps - 1 && (!kAct || state_program())) P0->term_fired[env] = (uint8_t)fired_index; }   // (the launch's last control step)
    }
    SOLO_STAMP(B, 12);
    wave_sync();  // this step's LDS state is complete before the next step reads it
  }
  SOLO_STAMP(B, 13);
  const int lane1 = sizeof(T) == 8 ? wave_fresh_lane() : wave_opaque_lane(lane0);  // re-derive the addresses instead of keeping them live
  // ---- THE OUTPUT EPILOGUE (round 3): the launch's observations, rewards, done flags and episodic bookkeeping,
  //      evaluated by the robot's own wave from the records it left, 32 steps per pass with LANE = STEP - one pass
  //      costs what one item costs (~450 instructions), whatever the number of steps in it: 0.2 % of a 250-step
  //      launch, 3 % of a 20-step one, and a wave that finishes early does this while the launch waits for its slowest
  //      robot anyway.  Rounds 1-2 ran two more kernels after the launch (one thread per robot-step; 15 + 5 us and two
  //      launch gaps per 0.36-ms 20-step rollout in f32, 44 + 6 us in f64); the per-item functions are the same
  //      (solo_outputs.h), so are the results, bit for bit.  The records are re-read from global memory (this wave
  //      wrote them: L2-resident, its own robot's are contiguous); the reward program's values live in the row-vector
  //      block of LDS, which is dead by now; lane 0 then folds the pass's rewards into the episodic accumulators in
  //      step order (accumulate_returns: the additions stay sequential).
  //      With robot migration every chunk's wave does this for the steps of ITS chunk (it reads only records it wrote
  //      itself; the episodic accumulators travel in the robot's record) and goes on to its next task afterwards - so
  //      the scratch stays clear of the per-launch tables (25 steps per pass in f64: kRowBlockReals<double> = 800).
  if constexpr (kFull) if (B.traj != nullptr) {
    wave_fence_global();  // this wave's record stores before its loads of them
    SOLO_STAMP_E(B, 1);
    const auto A = wave_cold_args(Bin);
    const int n_obs = wave_uniform(s_const.num_obs), n_rops = wave_uniform(s_const.num_reward_ops);
    constexpr int kPass = kRowsReals / SOLO_MAX_REWARD_OPS < 32 ? kRowsReals / SOLO_MAX_REWARD_OPS : 32;
    static_assert(kPass >= 16 && sizeof(T) * 32 >= (size_t)kPass, "the output epilogue's scratch");
    T* const val = s_blk;                                            // [n_rops][kPass]: the row vectors' block (dead here)
    uint8_t* const ev_bytes = reinterpret_cast<uint8_t*>(s_keep);    // (the parked factors are dead too)
    // (kSegments: the scratch holds ONE segment per robot, indexed from the segment's first step; everything else is indexed by the absolute step)
    const T* const my_traj = B.traj + (size_t)(env - B.env_base) * (size_t)(kSegments ? seg_len : B.steps) * SOLO_STATE_STRIDE;
    const bool want_reward = (B.flags & SOLO_STEP_REWARD) != 0;
    const bool bookkeeping = want_reward && (B.flags & SOLO_STEP_DONE) != 0;
    T* const obs_rec = A->obs_rec; T* const reward_rec = A->reward_rec;
    T* const view_obs = A->view_obs; T* const view_reward = A->view_reward; uint8_t* const view_done = A->view_done;
    const long long obs_stride = A->obs_rec_stride, reward_stride = A->reward_rec_stride;
    const int obs_from = A->obs_from;
    for (int base = step_begin; base < step_end; base += kPass) {
      const int k = base + lane1;
      if (lane1 < kPass && k < step_end) {
        const T* rec = my_traj + (size_t)(kSegments ? k - step_begin : k) * SOLO_STATE_STRIDE;
        const bool last = k == B.steps - 1;
        const int ev = (int)rec[SOLO_S_SPARE];
        ev_bytes[lane1] = (uint8_t)ev;
        if (B.flags & SOLO_STEP_DONE) {
          if (B.done_stride != 0 || last) B.done[(size_t)k * B.done_stride + env] = (uint8_t)(ev & kEventDone);
          if (view_done != nullptr && last) view_done[env] = (uint8_t)(ev & kEventDone);
          if constexpr (kTerms) { if (last && (!kAct || state_program())) P0->term_fired[env] = (uint8_t)(ev >> 2); }   // (which termination fired: bits >= 2 of the event word)
        }
        SOLO_STAMP_E(B, 2);
        T roll, pitch, yaw;
        euler_from_quat<T>(rec[SOLO_S_QUAT], rec[SOLO_S_QUAT + 1], rec[SOLO_S_QUAT + 2], rec[SOLO_S_QUAT + 3], &roll, &pitch, &yaw);
        SOLO_STAMP_E(B, 3);
        if (B.flags & SOLO_STEP_OBS) {
          T* o_rec = (obs_rec != nullptr && k >= obs_from) ? obs_rec + (size_t)k * obs_stride + (size_t)env * n_obs : nullptr;
          T* o_view = (view_obs != nullptr && last) ? view_obs + (size_t)env * n_obs : nullptr;
          if (o_rec != nullptr || o_view != nullptr)
            for (int i = 0; i < n_obs; ++i) {
              T x;
              if constexpr (kContact) x = observation_value_foot<T>(P0->obs[i], rec, roll, pitch, yaw, P0->contact_traj + ((size_t)env * P0->contact_traj_steps + k) * 4, 1);
              else x = observation_value<T>(P0->obs[i], rec, roll, pitch, yaw);
              if (o_rec != nullptr) o_rec[i] = x;
              if (o_view != nullptr) o_view[i] = x;
            }
        }
        SOLO_STAMP_E(B, 4);
        if (want_reward) {
          const T rv = eval_reward<T>(P0, rec, roll, pitch, val + lane1, kPass);
          if (reward_rec != nullptr) reward_rec[(size_t)k * reward_stride + env] = rv;
          if (view_reward != nullptr && last) view_reward[env] = rv;
        }
        SOLO_STAMP_E(B, 5);
      }
      wave_sync();
      SOLO_STAMP_E(B, 6);
      if (bookkeeping && lane1 == 0) {
        const int cnt = step_end - base < kPass ? step_end - base : kPass;
        accumulate_returns<T>(s_state, ev_bytes, 1, val + (size_t)(n_rops - 1) * kPass, 1, cnt, SOLO_STATS_ROW,
                              [](double* p, double x) { stats_add(p, x); });
      }
      wave_sync();
      SOLO_STAMP_E(B, 7);
    }
  }
  // (kSegments: the counters, the cost and the record go out once, after the last segment)
  if ((B.flags & SOLO_STEP_DONE) && lane1 < SOLO_MAX_TERMS && (!kSegments || last_chunk)) {
    if constexpr (kMigrate) wave_atomic_store(wave_cold_args(Bin)->term_count + (size_t)env * SOLO_MAX_TERMS + lane1, s_cnt[lane1]);
    else wave_cold_args(Bin)->term_count[(size_t)env * SOLO_MAX_TERMS + lane1] = s_cnt[lane1];
  }
  if ((B.flags & SOLO_STEP_PHYSICS) && lane1 == 0 && last_chunk) { int32_t* cost = wave_cold_args(Bin)->cost; if (cost != nullptr) cost[env] = prio_sweeps - hist_sweeps; }
  // (slots SOLO_S_RETURN.. of the record: the episodic accumulators, kept by whichever path evaluated the rewards)
  const bool own_returns = (B.flags & SOLO_STEP_REWARD) && (B.flags & SOLO_STEP_DONE) &&
                           (B.traj != nullptr || (kInlineOutputs<T, kFull> && B.reward_inline != nullptr));
  if (lane1 < (own_returns ? SOLO_S_SPARE : SOLO_S_RETURN) && (!kSegments || last_chunk)) {
    if constexpr (kMigrate) wave_store_shared(wave_cold_args(Bin)->state + rec + lane1, s_state[lane1]);
    else wave_cold_args(Bin)->state[rec + lane1] = s_state[lane1];
  }
  SOLO_STAMP(B, 14);
#if defined(SOLO_STAMPS) && defined(SOLO_STAMPS_LIGHT)
  // (the light build's slot 13: the robot's Gauss-Seidel sweeps over all segments of the launch so far - tools/gpu_tail.py)
  if constexpr (kSegments) { if (lane1 == 0) B.stamps[(size_t)B.stamp_row * 32 + 13] = (unsigned long long)pace_sweeps(prio_sweeps); }
#endif
#if defined(SOLO_STAMPS) && !defined(SOLO_STAMPS_LIGHT)
  wave_sync();
  if (lane1 < 16) B.stamps[(size_t)env * 32 + 16 + lane1] = s_acc[lane1];
#endif
  if constexpr (kMigrate) {
    // hand the robot on (unless this was its last chunk): its history, then - when the device-coherent stores of its
    // record and counters above have completed - its number and next chunk into the next free slot of its ring (whoever
    // holds that slot's ticket continues it).  The slot's index and the wave's OWN next ticket are two independent
    // read-modify-writes: both are issued here, in front of the one wait that the stores need anyway - a hand-over is
    // a chain of device-scope round trips (~1.8 us each under load), and this takes two of the five off it.
    const int chunks = migration_chunks(B.steps, B.q_chunk), ring_len = (B.count / B.q_rings) * chunks;
    int at = 0, nt = 0;
    if (lane1 == 0) {
      if (!last_chunk) {
        wave_atomic_store(queue + kQueueHeader + (env - B.env_base), prio_sweeps);
        at = wave_atomic_add(queue + q_ring * 32 + 16, 1);
      }
      nt = wave_atomic_add(queue + q_ring * 32, 1);
    }
    wave_release_device();
    if (!last_chunk && lane1 == 0)
      wave_atomic_store(queue + kQueueHeader + (size_t)B.count + (size_t)q_ring * ring_len + at, (env - B.env_base) | ((q_chunk_at + 1) << 24));
    next_ticket = wave_readlane_int(nt, 0);
    have_next = true;
  }
  if constexpr (kMigrate) wave_sync();  // (the next task's prologue rewrites the LDS record)
  if constexpr (kSegments) {
    if (last_chunk) break;
    wave_fence_global();  // this segment's epilogue has its record loads behind it before the next segment's steps overwrite the scratch
    carry_sweeps = prio_sweeps; carry_steps = prio_steps;
#if SOLO_ROLL_PACING
    // PROGRESS PACING (KBuffers::progress, null = off): the wave counts itself in the counter of the segment it has just ended - one
    // relaxed device-scope read-modify-write, no wave ever waits for another - and what comes back is its rank among ALL robots of
    // the rollout, whichever slice they run in.  The rank sets the wave's issue priority for its next segment through the sweep
    // history that both priority tests read (physics_solve: `prio_sweeps > kPrioSweeps<T> * prio_steps`): a bias of +/- kPaceBias
    // holds the test one way or the other for a whole segment - the last quarter is pinned to level 3 like a robot of many
    // sweeps, the first quarter is kept off the pin, the middle half keeps its own history.  No register of its own in the step
    // loop: the bias lives in the high bits of the history (the true count stays below kPaceBias: pace_sweeps takes it back out
    // in front of the next one), and cost[env] is a difference inside one segment, which the bias cancels out of.
    if (int32_t* const progress = wave_cold_args(Bin)->progress) {
      int rank = 0;
      const int seg_at = step_begin / seg_len;   // (the segment just ended; below kProgressCounters - a launch has at most that many)
      if (lane1 == 0) rank = wave_atomic_add(progress + (seg_at < kProgressCounters ? seg_at : kProgressCounters - 1), 1);
      rank = wave_readlane_int(rank, 0);
      carry_sweeps = pace_sweeps(prio_sweeps) + pace_bias(rank, B.num_envs);
    }
#endif
    step_begin += seg_len;
    step_end = step_begin + seg_len < B.steps ? step_begin + seg_len : B.steps;
    last_chunk = step_end == B.steps;
  }
  } while (kMigrate || kSegments);  // the task loop
#undef SOLO_STATS_ROW
}

}  // namespace solo
