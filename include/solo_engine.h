/* solo_engine.h — C-ABI of the MI355X batched Solo8 physics engine.
 *
 * This is the drop-in boundary for the ONE hot path of WPI-MMR/gym_solo:
 * the per-step pybullet call sequence issued by Solo8VanillaEnv.step()
 *   client.setJointMotorControlArray(...)   gym_solo/envs/solo8v2vanilla.py:87-90
 *   client.stepSimulation()                 gym_solo/envs/solo8v2vanilla.py:91
 *   client.getBasePositionAndOrientation    gym_solo/core/obs.py:268, rewards.py:232,264,370
 *   client.getBaseVelocity                  gym_solo/core/obs.py:273, rewards.py:334
 *   client.getJointState                    gym_solo/core/obs.py:354, rewards.py:298
 * plus the obs/reward/termination reductions (obs.py:130-159, rewards.py:104-118,
 * termination.py:38-50) and the reset/settle loop (solo8v2vanilla.py:104-143),
 * for N independent robots at once.
 *
 * The reference binds pybullet through `pybullet_utils.bullet_client.BulletClient`
 * (solo8_base_env.py:34-35).  A maintainer replaces that object by a ctypes stub
 * over this header; no torch / C++ type crosses the boundary:
 * plain pointers (device pointers are `void*`), sizes and PODs only.
 *
 * Conventions
 *  - return value: 0 = SOLO_OK, negative = SoloStatus error; text via
 *    solo_engine_last_error().
 *  - one engine handle per GPU / process; NOT thread-safe per handle; all work
 *    is enqueued on the caller-provided HIP stream (NULL = default stream), no
 *    hidden device synchronisation except where stated.
 *  - device buffers are owned by the engine and exposed zero-copy through
 *    SoloStateView; pointers passed IN (actions, masks, params) are borrowed.
 *  - `real` below means float (dtype SOLO_F32) or double (SOLO_F64) as chosen at
 *    create time; every device buffer of the engine uses that type.
 */
#ifndef SOLO_ENGINE_H_
#define SOLO_ENGINE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SOLO_ABI_VERSION 7  /* 2: SOLO_STEP_AUTO_RESET; query-only launches never auto-reset; reset restores the motor targets
                               3: SoloConfig::solver_residual_threshold
                               4: SoloConfig::migrate_steps, SoloConfig::solver_warm_start, SoloStateView::warm
                               5: -1 = "the engine chooses" for steps_per_launch / rollout_streams / migrate_steps (the measured
                                  launch policy lives in the engine: solo_engine_plan reports it), solo_engine_time_rollout,
                                  SOLO_ERR_INCOMPLETE
                               6: SoloConfig::base_lateral_friction (the base link keeps its own friction: the reference's
                                  changeDynamics loop never reaches link -1), solo_engine_reserve
                               7: joint control modes: SoloControl, solo_engine_set_control / solo_engine_get_control
                                  (+ contact sensing - solo_engine_set_contact_sensing / get_contacts, SOLO_SRC_FOOT_FORCE -:
                                  new calls and constants only, no struct changed, so the version stays 7; control
                                  decimation - solo_engine_set_decimation / get_decimation - the same way, and so do
                                   the state terminations: SOLO_T_HEIGHT_BELOW / SOLO_T_TILT_ABOVE,
                                   solo_engine_set_term_values / solo_engine_get_term_fired, and the per-robot actuator
                                   block: SOLO_ACTUATOR_WIDTH, solo_engine_set_actuators / solo_engine_get_actuators, and the
                                   per-robot base wrench block: SOLO_WRENCH_WIDTH, solo_engine_set_base_wrench /
                                   solo_engine_get_base_wrench) */

/* ---- fixed Solo8 dimensions -------------------------------------------- */
#define SOLO_NUM_LEGS 4
#define SOLO_NUM_DOF 8        /* actuated revolute joints (HFE, KFE per leg)          */
#define SOLO_NUM_JOINTS 12    /* pybullet joint count incl. 4 fixed ANKLE joints:      */
                              /* gym_solo/envs/test_solo8v2vanilla.py:57               */
#define SOLO_NUM_BODIES 9     /* base + 8 moving links (feet are welded to lower legs) */
#define SOLO_NV 14            /* velocity dofs: 6 (floating base) + 8                  */
#define SOLO_MAX_SPHERES 16   /* collision primitives (sphere vs ground)               */
#define SOLO_STATE_STRIDE 32  /* reals per env record (one 128-B line in f32)          */
#define SOLO_MAX_OBS 64       /* observation elements per env                          */
#define SOLO_MAX_REWARD_OPS 32
#define SOLO_MAX_TERMS 4
#define SOLO_STATS_SHARDS 64  /* episodic statistics are accumulated in 64 rows (sum them) */
#define SOLO_STATS_WIDTH 8

/* env record layout (reals), AoS so that one wavefront reads its robot's whole
 * state as ONE coalesced 128-B (f32) / 256-B (f64) line: */
#define SOLO_S_POS 0      /* base CoM position, world            [3] */
#define SOLO_S_QUAT 3     /* base orientation xyzw (pybullet)    [4] */
#define SOLO_S_Q 7        /* joint angles, dof order             [8] */
#define SOLO_S_ANGVEL 15  /* base angular velocity, world frame  [3] */
#define SOLO_S_LINVEL 18  /* base linear velocity, world frame   [3] */
#define SOLO_S_QD 21      /* joint velocities                    [8] */
#define SOLO_S_RETURN 29  /* episodic return accumulator             */
#define SOLO_S_EPLEN 30   /* episode length accumulator              */
#define SOLO_S_SPARE 31
/* The quaternion of a state the caller writes (the state view, a checkpoint) is taken to be UNIT to the rounding of T and is
 * used as stored: the step forms the base rotation from its components (r00 = 1 - 2 (qy qy + qz qz), ...) without
 * renormalising on load, so a quaternion that is off unit by e in |q|^2 gives a "rotation" off orthogonal by the same order
 * (a unit quaternion rounded to f32: e <= 2^-23).  Every step WRITES q+ = exp(dt w / 2) (x) q renormalised (one rsqrt of the
 * four squares), so the stored quaternion never drifts from unit by more than that product's rounding. */

typedef enum SoloStatus {
  SOLO_OK = 0,
  SOLO_ERR_INVALID_ARG = -1, /* -> ValueError in the Python facade */
  SOLO_ERR_HIP = -2,         /* -> RuntimeError                    */
  SOLO_ERR_UNSUPPORTED_MODEL = -3,
  SOLO_ERR_NO_PROGRAM = -4,  /* step() without a reward / obs / termination registered:
                                mirrors the ValueErrors of rewards.py:115-116, obs.py:138-139,
                                termination.py:43-44 */
  SOLO_ERR_NO_DEVICE = -5,
  SOLO_ERR_INCOMPLETE = -6   /* a wave of an EARLIER launch with robot migration gave up waiting for its robot (a bounded
                                wait that a correct queue never exhausts): some robots were not stepped through that
                                launch.  Sticky: every later call on the handle that takes the engine (everything but
                                destroy, last_error and kernel_name) returns it.  An internal error - never observed -
                                surfaced instead of returned as SOLO_OK; the count is slot 6 of the statistics. */
} SoloStatus;

typedef enum SoloDType { SOLO_F32 = 0, SOLO_F64 = 1 } SoloDType;

/* ---- robot model (DATA, not code: both the engine and the CPU oracle take it) */
typedef struct SoloModel {
  /* body 0 = base; body 1+j = link moved by dof j.  dof order:
   * FL_HFE, FL_KFE, FR_HFE, FR_KFE, HL_HFE, HL_KFE, HR_HFE, HR_KFE. */
  int32_t parent[SOLO_NUM_DOF];            /* parent BODY index of dof j's link         */
  double joint_origin[SOLO_NUM_DOF][3];    /* joint frame origin, in parent body frame  */
  double joint_axis[SOLO_NUM_DOF][3];      /* unit axis (Solo8: all +y)                 */
  double mass[SOLO_NUM_BODIES];
  double com[SOLO_NUM_BODIES][3];          /* in body frame; base com must be 0         */
  double inertia[SOLO_NUM_BODIES][6];      /* about com, body axes: xx yy zz xy xz yz   */
  int32_t num_spheres;
  int32_t sphere_body[SOLO_MAX_SPHERES];
  double sphere_center[SOLO_MAX_SPHERES][3]; /* in body frame */
  double sphere_radius[SOLO_MAX_SPHERES];
  /* dof j <-> pybullet joint index (for getJointState facade), and the 12 names */
  int32_t dof_to_joint[SOLO_NUM_DOF];
  /* URDF joint limits [rad] (the reference's getJointInfo fixture pins -10 / +10,
   * gym_solo/core/test_obs_observations.py:123-162 columns 8-9): unilateral rows next to the motors
   * ([recalled] btMultiBodyJointLimitConstraint).  lower < upper required. */
  double joint_lower[SOLO_NUM_DOF];
  double joint_upper[SOLO_NUM_DOF];
} SoloModel;

/* ---- physics / env configuration (gym_solo/core/configs.py:8-38) -------- */
typedef struct SoloConfig {
  int32_t abi_version;       /* = SOLO_ABI_VERSION */
  int32_t dtype;             /* SoloDType */
  double dt;                 /* configs.py:10  (1e-3), one substep: solo8_base_env.py:39-41 */
  double gravity[3];         /* configs.py:17 */
  double motor_torque_limit; /* configs.py:12  -> impulse clamp +-limit*dt per step */
  double motor_kp;           /* pybullet POSITION_CONTROL default positionGain 0.1 [recalled] */
  double motor_kd;           /* pybullet POSITION_CONTROL default velocityGain 1.0 [recalled] */
  double linear_damping;     /* configs.py:21 */
  double angular_damping;    /* configs.py:22 */
  double lateral_friction;   /* configs.py:24 (x plane friction 1.0): the collision spheres of links 0..11 - the legs.  The
                                reference's changeDynamics loop runs over range(getNumJoints) (solo8v2vanilla.py:157-163) and so
                                never reaches the base link (-1): see base_lateral_friction */
  double restitution;        /* configs.py:23, passed to changeDynamics for links 0..11 (solo8v2vanilla.py:158-163).  In [0, 1];
                                WITHOUT EFFECT here, as in the reference: Bullet gives a contact the PRODUCT of its two bodies'
                                restitutions ([recalled] btManifoldResult::calculateCombinedRestitution), and the ground the
                                reference loads - pybullet_data's plane.urdf, solo8_base_env.py:47 - declares none (0) */
  double contact_erp;        /* penetration recovery rate (Bullet erp2 0.2 [recalled]) */
  double contact_margin;     /* spheres closer than this to the ground create rows */
  double joint_limit_margin; /* a joint closer than this [rad] to one of its limits gets that limit's row
                                (a speculative unilateral row: exact as long as |qd| dt < margin) */
  int32_t solver_iterations; /* Bullet default 50 [recalled] */
  int32_t settle_steps;      /* solo8v2vanilla.py:130 (500) */
  double start_pos[3];       /* configs.py:15 */
  double start_quat[4];      /* from configs.py:16 euler */
  double settle_targets[SOLO_NUM_JOINTS]; /* solo8v2vanilla.py:21-34, pybullet joint order */
  double action_scale;       /* normalize_actions ? max_motor_rotation : 1 (solo8v2vanilla.py:84-85) */
  int32_t auto_reset;        /* 1: envs whose `done` fires are restored from the snapshot in-kernel */
  int32_t steps_per_launch;  /* rollouts / settle fuse this many consecutive env steps of each robot
                                into one kernel launch (state stays in LDS); 0 or 1 = one step;
                                -1 = the engine chooses (a rollout of K steps: launches of min(K, 250) steps) */
  int32_t rollout_streams;   /* rollouts cut the batch into this many slices that advance as
                                independent launch chains on internal HIP streams (0/1 = off);
                                -1 = the engine chooses (two slices when a rollout takes more than one launch) */
  int32_t solver_ulp_tolerance; /* k: a Gauss-Seidel row whose clamped candidate differs from its impulse by
                                at most k half-ulps relative to the impulse (|d| <= k * 2^-24 |lam| in f32,
                                k * 2^-53 |lam| in f64) is left untouched, and a sweep that changes no row
                                ends the iteration early.  0 = only an exact fixed point ends it (then
                                identical to always running solver_iterations sweeps); 2 also stops last-bit limit
                                cycles, which otherwise keep ~3% of the robots iterating to the cap.  Host defaults
                                (gym_solo_amd/core/configs.py): 2 in f32, 512 in f64 - 5.7e-14 relative, half of the
                                rounding noise between two f64 formulations of one step; measured in round 6: rest
                                behaviour and parity against 50 plain sweeps unchanged, 12 % fewer sweeps.
                                Negative values are rejected. */
  double solver_residual_threshold; /* pybullet's solverResidualThreshold ([recalled] documented default 1e-7, set in
                                PhysicsServerCommandProcessor::createEmptyDynamicsWorld; the reference never changes it;
                                the host default here is 0 = off - gym_solo_amd/core/configs.py says why):
                                the iteration ends after the first sweep in which max over the rows of
                                (delta impulse x A_rr)^2 - the squared velocity-level change, [recalled]
                                btMultiBodyConstraintSolver::solveSingleIteration / resolveSingleConstraintRowGeneric
                                returning deltaImpulse / jacDiagABInv - is <= this value.  0 = never (every sweep that
                                still changes a row runs, up to solver_iterations).  Negative values are rejected. */
  int32_t migrate_steps;     /* c > 0: a fused launch of more than c steps hands its robots from wave to wave every c
                                steps through a work queue in device memory (the robot's 256-B record travels; any idle
                                wave continues any robot), so that the launch ends when the WORK is done and not when
                                the unluckiest SIMD's robots are.  Scheduling only: results are bit-identical.  0 = off
                                (one wave steps one robot through the whole launch).  -1 = the engine chooses: off while
                                every robot of a launch has a wave slot of its own (4096 robots: four waves on each of
                                the chip's 1024 SIMDs, in both precisions since round 5), else - in f64 - two chunks per
                                launch (chunks of 25 steps in a rollout of several launches); f32 never (measured slower) -
                                solo_engine_plan reports it. */
  int32_t reserved0;         /* (padding; must be 0) */
  double solver_warm_start;  /* f in (0, 1]: the Gauss-Seidel iteration of a step STARTS from f x the impulses the previous
                                step ended with (every row: motors, joint limits, contacts - clamped to the row's bounds
                                of this step, the friction rows to mu x their contact's starting normal impulse; a row
                                that was not live in the previous step starts at 0; a reset / auto-reset / restored robot
                                starts at 0).  [recalled] Bullet warm-starts its rigid-body contacts with
                                m_warmstartingFactor 0.85; whether the btMultiBody path the reference runs on does is
                                not known here.  An OPT-IN, and only together with solver_residual_threshold > 0 (the pair
                                is what makes pybullet's early exit leave a resting robot at rest: DESIGN.md section 4).
                                0 = off (every step starts from zero impulses).  The cache - SoloStateView::warm, 64 reals
                                per robot, the step kernel's lane layout - costs 2 x 64 reals of memory traffic per
                                env-step, reported separately from the path's algorithmic bytes. */
  double base_lateral_friction; /* friction of the BASE link's collision spheres (model spheres attached to body 0).  The
                                reference sets lateralFriction with changeDynamics for links 0 .. 11 only
                                (solo8v2vanilla.py:157-163: `for joint in range(joint_cnt)`), so the base keeps what loadURDF
                                gave it: [recalled] pybullet's default 0.5 (x plane.urdf's 1.0).  Neither
                                SoloConfig::lateral_friction nor solo_engine_set_params(0, ...) touches it: with the
                                reference's 0.5 the two coincide, with any other leg friction (BASELINE configs[3]'s
                                per-robot values) the belly keeps 0.5.  Host default 0.5; negative values are rejected. */
} SoloConfig;

/* ---- fused observation / reward / termination programs ------------------ */
/* Source vector the obs program indexes (per env, computed in-kernel):
 *   [0..2] euler xyz  [3..5] base lin vel  [6..8] base ang vel
 *   [9..20] joint angle by pybullet joint index (fixed joints = 0)
 *   [21..32] joint velocity by pybullet joint index
 *   [33..35] base position  [36..39] quaternion xyzw  [40] constant 1.0
 *   [41..44] normal contact force [N] on the foot sphere of leg 0..3 (model sphere 4l+1) in THIS step: needs
 *            contact sensing (solo_engine_set_contact_sensing) */
#define SOLO_SRC_EULER 0
#define SOLO_SRC_LINVEL 3
#define SOLO_SRC_ANGVEL 6
#define SOLO_SRC_JPOS 9
#define SOLO_SRC_JVEL 21
#define SOLO_SRC_POS 33
#define SOLO_SRC_QUAT 36
#define SOLO_SRC_ONE 40
#define SOLO_SRC_FOOT_FORCE 41
#define SOLO_SRC_COUNT 45

typedef struct SoloObsElem {
  int32_t src;      /* index into the source vector */
  int32_t flags;    /* bit0: clip to [lo,hi]; bit1: normalise 2(a-nlo)/(nhi-nlo)-1 (obs.py:149-152) */
  double scale;     /* e.g. 180/pi for degrees (obs.py:277-279, 358) */
  double lo, hi;    /* clip bounds (obs.py:282, 361) */
  double nlo, nhi;  /* normalisation bounds: the float32 Box bounds widened to double */
} SoloObsElem;

/* reward program: postfix (RPN) over a small value stack */
typedef enum SoloRewardOp {
  SOLO_R_CONST = 0,        /* push a                                              */
  SOLO_R_UPRIGHT = 1,      /* push (-pi/2)*pitch/(-pi/2)^2      rewards.py:221-234 */
  SOLO_R_FLAT_TORSO = 2,   /* push tol(sqrt(tx^2+ty^2),(-a,a),b) rewards.py:256-269 */
  SOLO_R_TORSO_HEIGHT = 3, /* push tol(z,(a-b,a+b),c)            rewards.py:362-373 */
  SOLO_R_HORIZ_SPEED = 4,  /* push tol(|vxy|,(a-b,a+b),c)        rewards.py:326-338 */
  SOLO_R_SMALL_CONTROL = 5,/* push tol(mean12|qd|,(0,0),a)       rewards.py:290-301 */
  SOLO_R_SCALE = 6,        /* top *= a                                            */
  SOLO_R_ADD = 7,          /* pop b, pop a, push a+b                              */
  SOLO_R_MUL = 8           /* pop b, pop a, push a*b                              */
} SoloRewardOp;

typedef struct SoloRewardInstr {
  int32_t op;
  int32_t pad;
  double a, b, c;
} SoloRewardInstr;

typedef enum SoloTermKind {
  SOLO_T_PERPETUAL = 0,  /* termination.py:86-97  */
  SOLO_T_TIME = 1,       /* termination.py:59-83  */
  SOLO_T_CONST = 2,      /* testing.py DummyTermination: fixed flag */
  /* state terminations (see "state terminations" below): functions of the robot's state record after the control step;
     term_param = a grace count, the threshold comes from solo_engine_set_term_values */
  SOLO_T_HEIGHT_BELOW = 3, /* fires when state[SOLO_S_POS + 2] < value (WORLD z, also over a heightfield) */
  SOLO_T_TILT_ABOVE = 4    /* fires when 1 - 2 (qx^2 + qy^2) < value = cos(max tilt) */
} SoloTermKind;

typedef struct SoloProgram {
  int32_t num_obs;
  int32_t num_reward_ops;
  int32_t num_terms;
  int32_t pad;
  SoloObsElem obs[SOLO_MAX_OBS];
  SoloRewardInstr reward[SOLO_MAX_REWARD_OPS];
  int32_t term_kind[SOLO_MAX_TERMS];
  int32_t term_param[SOLO_MAX_TERMS]; /* max_step_delta / flag */
} SoloProgram;

/* ---- ground: the reference loads pybullet_data's flat `plane.urdf` (solo8_base_env.py:47);
 * BASELINE configs[4] asks for inclined / stair terrain.  A heightfield z = h(x, y): inside the
 * grid rectangle (borders included) the bilinear interpolant of the cell's four grid heights, and
 * outside it h(x, y) = h(x and y each clamped to the rectangle), so the ground has zero slope along
 * a clamped axis; every collision sphere collides with the tangent plane of that surface under its
 * centre. ------------------------------------------------------------------------------------- */
typedef struct SoloTerrain {
  int32_t nx, ny;          /* grid points along x and y (>= 2 each)                       */
  double cell;             /* grid spacing [m]                                            */
  double origin[2];        /* world (x, y) of grid point (0, 0)                           */
  const double* heights;   /* HOST pointer, [ny][nx] row-major (y major), copied by the call */
} SoloTerrain;

/* ---- zero-copy view of engine-owned device buffers ----------------------- */
typedef struct SoloStateView {
  int32_t num_envs;
  int32_t dtype;        /* SoloDType of every `real` buffer               */
  int32_t state_stride; /* = SOLO_STATE_STRIDE                            */
  int32_t obs_dim;      /* D of the current program (0 if none)           */
  void* state;          /* real  [N][SOLO_STATE_STRIDE]                   */
  void* snapshot;       /* real  [N][SOLO_STATE_STRIDE] post-settle state */
  void* targets;        /* real  [N][12] last motor targets (radians)     */
  void* obs;            /* real  [N][D]                                   */
  void* reward;         /* real  [N]                                      */
  void* done;           /* uint8 [N]                                      */
  void* term_count;     /* int32 [N][SOLO_MAX_TERMS]                      */
  void* params;         /* real  [N][4]: lateral friction, base-mass scale, 2 spare */
  void* stats;          /* double[SOLO_STATS_SHARDS][8], sum over the shard axis: sum return, sum return^2,
                           episodes, sum length, (unused), diverged robots restored, waves of migrating launches that
                           gave up waiting (row 0 only; non-zero = SOLO_ERR_INCOMPLETE), 1 spare */
  void* cost;           /* int32 [N]: Gauss-Seidel sweeps each robot ran in the LAST launch that stepped it
                           (its cost is persistent within an episode): input of solo_engine_set_order */
  void* warm;           /* real  [N][64]: the impulses every robot's last step ended with, one per constraint row in the
                           step kernel's lane layout (solo_kernel_params.h) - the warm-start cache of
                           SoloConfig::solver_warm_start; all zero while that is off */
} SoloStateView;

typedef struct SoloEngine SoloEngine;

/* flags of solo_engine_step */
#define SOLO_STEP_PHYSICS 1u  /* A3+A4: motors + stepSimulation */
#define SOLO_STEP_OBS 2u      /* A5-A7  */
#define SOLO_STEP_REWARD 4u   /* A8-A11 */
#define SOLO_STEP_DONE 8u     /* A12 (+ auto-reset when configured) */
#define SOLO_STEP_ALL 15u
/* The in-kernel auto-reset (cfg.auto_reset) acts in launches that carry SOLO_STEP_PHYSICS: a
 * query-only launch (TerminationFactory.is_terminated() outside step(), termination.py:38-50)
 * never mutates the simulation.  A caller that evaluates `done` in a launch of its own AFTER the
 * physics launch (a Python-side observation / reward in between) adds this bit to let that launch
 * restore the robots whose `done` fires. */
#define SOLO_STEP_AUTO_RESET 16u

/* BulletClient(connection_mode) + setGravity + setPhysicsEngineParameter + loadURDF x2
 * (solo8_base_env.py:34-48).  Allocates device buffers, uploads the model, places every
 * robot at start_pos and runs the settle loop (solo8v2vanilla.py:124-136) to build the
 * reset snapshot.  Synchronises the device once. */
int solo_engine_create(const SoloConfig* cfg, const SoloModel* model, int32_t num_envs,
                       int32_t device_id, SoloEngine** out);
/* client.disconnect()  (solo8_base_env.py:150-152) */
int solo_engine_destroy(SoloEngine* eng);
/* register_observation / register_reward / register_termination, compiled
 * (obs.py:109-128, rewards.py:91-102, termination.py:28-36) */
int solo_engine_set_program(SoloEngine* eng, const SoloProgram* prog);
/* resetSimulation + reload + settle (solo8v2vanilla.py:104-143): restores the snapshot for
 * envs with mask[i] != 0 (mask NULL = all) and clears their termination counters. */
int solo_engine_reset(SoloEngine* eng, const uint8_t* mask_dev, void* stream);
/* re-run the settle loop from the start pose for every env and refresh the snapshot
 * (needed after solo_engine_set_params). Synchronises the stream. */
int solo_engine_settle(SoloEngine* eng, void* stream);
/* setJointMotorControlArray(..., POSITION_CONTROL, targetPositions=a, forces=limit)
 * (solo8v2vanilla.py:87-90).  actions_dev: real [N][12] in pybullet joint order
 * (entries 2,5,8,11 = fixed ANKLE joints are ignored); multiplied by action_scale. */
int solo_engine_set_targets(SoloEngine* eng, const void* actions_dev, void* stream);
/* One env step for all N robots (solo8v2vanilla.py:72-102).  actions_dev may be NULL
 * (keep the last targets).  flags: SOLO_STEP_*.  One kernel launch. */
int solo_engine_step(SoloEngine* eng, const void* actions_dev, uint32_t flags, void* stream);
/* K consecutive env steps with per-step actions real [K][N][12] (open-loop rollout, used by
 * bench.py): ceil(K / steps_per_launch) launches enqueued back-to-back; the view's obs / reward /
 * done hold the LAST step's values afterwards.  With cfg.rollout_streams = G > 1 the batch is cut
 * into G slices that advance as independent launch chains on G internal HIP streams, forked from
 * / joined into `stream` (robots are independent: one slice's launch boundary and tail overlap
 * the other slices' work). */
int solo_engine_rollout(SoloEngine* eng, const void* actions_dev, int32_t num_steps,
                        uint32_t flags, void* stream);
/* Same, but every step's outputs are kept: obs_out real [K][N][D], reward_out real [K][N],
 * done_out uint8 [K][N] (caller-owned device buffers; a NULL pointer = that output is not recorded).
 * The engine's view holds the last step's outputs afterwards in either case.  This is what an RL
 * rollout collector reads. */
int solo_engine_rollout_record(SoloEngine* eng, const void* actions_dev, int32_t num_steps,
                               uint32_t flags, void* obs_out, void* reward_out, void* done_out,
                               void* stream);
int solo_engine_get_view(SoloEngine* eng, SoloStateView* out);
/* changeDynamics(lateralFriction=...) per env + base-mass randomisation
 * (solo8v2vanilla.py:158-163; BASELINE config 4).  which: 0 = friction, 1 = base mass scale.
 * per_env_dev: real [N]. */
int solo_engine_set_params(SoloEngine* eng, int32_t which, const void* per_env_dev, void* stream);
/* Replaces loadURDF('plane.urdf') (solo8_base_env.py:47): NULL = the flat plane z = 0.  Re-runs the
 * settle loop (the reset snapshot depends on the ground).  Synchronises the device. */
int solo_engine_set_terrain(SoloEngine* eng, const SoloTerrain* terrain, void* stream);
/* Launch order of the robots (cost-balanced scheduling): order_dev int32 [N], a permutation of 0..N-1
 * that maps workgroup b of a launch to robot order[b]; NULL = the engine's own map (each of the 8 XCDs of the
 * chip steps a contiguous eighth of the launch's robots, so that neighbouring robots' rows of the [K][N][.]
 * arrays meet in one L2: HBM traffic, not results).  With cfg.rollout_streams = G
 * the positions [N g / G, N (g+1) / G) must hold a permutation of the same robot range (every slice
 * keeps its robots).  Results do not depend on the order (robots are independent); it matters when
 * N exceeds the 4096 resident waves of the chip: dispatching the costliest robots first (view.cost,
 * descending) keeps the tail of a launch short.  Copied into an engine-owned buffer.  The table is
 * VALIDATED on upload (one device-to-host copy, synchronises `stream`): anything but such a permutation
 * returns SOLO_ERR_INVALID_ARG and leaves the previous order in force. */
int solo_engine_set_order(SoloEngine* eng, const int32_t* order_dev, void* stream);
/* name of the dominant kernel (for rocprof cross-checks) and its last launch geometry: the full step kernel of the
 * configuration in force - or solo_roll_kernel<T> when the engine's last rollout (or solo_engine_time_rollout) ran FUSED SEGMENTS
 * (below, at SoloLaunchPlan) and the configuration still would. */
const char* solo_engine_kernel_name(SoloEngine* eng);
/* Times a rollout of reps * steps_per_launch steps - the CONFIGURED steps per launch; one step per launch when that is
 * left to the engine (solo_engine_time_rollout times a rollout with the engine's own geometry) - as solo_engine_rollout
 * runs it (same slicing, same fused launches; the step kernel, its output epilogue included) with hipEvents
 * recorded ON THE STREAMS THE KERNELS ARE LAUNCHED ON (every slice's internal stream when
 * rollout_streams > 1, else `stream`) and returns the mean milliseconds per LAUNCH over all slices;
 * one launch covers N / max(1, rollout_streams) robots x steps_per_launch steps.
 * actions_dev: real [reps * steps_per_launch][N][12] or NULL. */
int solo_engine_time_step(SoloEngine* eng, const void* actions_dev, uint32_t flags,
                          int32_t reps, void* stream, double* ms_per_launch);
/* The launch geometry a rollout of num_steps steps runs with (what -1 = "the engine chooses" resolved to, or the
 * configured values): the measured launch policy is the engine's, not the caller's. */
typedef struct SoloLaunchPlan {
  int32_t steps_per_launch;  /* env steps fused into one launch (the last launch of a slice may be shorter) */
  int32_t launches;          /* launches per slice; with FUSED SEGMENTS: steps_per_launch-step segments per slice (below) */
  int32_t slices;            /* independent launch chains (batch slices on internal HIP streams) */
  int32_t migrate_steps;     /* steps per migration chunk of a launch, 0 = no robot migration */
  int32_t waves_per_simd;    /* resident step-kernel waves per SIMD in this precision (4) */
  int32_t resident_robots;   /* robots with a wave slot of their own on this device: waves_per_simd x SIMDs */
} SoloLaunchPlan;
int solo_engine_plan(SoloEngine* eng, int32_t num_steps, SoloLaunchPlan* out);
/* FUSED SEGMENTS.  A rollout of several launches in plain position control with the default solver (no robot migration, contact
 * sensing, decimation, state termination, actuator or wrench block; steps_per_launch >= 2; flags with SOLO_STEP_PHYSICS and
 * observations or rewards) runs up to 16 consecutive launches of a slice as ONE kernel launch (solo_roll_kernel): every wave runs
 * its robot's output epilogue after each steps_per_launch steps and goes on with the next segment instead of waiting at a launch
 * boundary for the slice's slowest robot.  Scheduling only: results are bit-identical, the record scratch stays
 * [N][steps_per_launch][32], and SoloLaunchPlan reports what it reported before (its `launches` are those segments);
 * solo_engine_time_rollout still divides by them, solo_engine_time_step always times separate launches. */
/* LAZY SCRATCH.  The per-launch record scratch of fused launches ([N][steps_per_launch][32] reals: 0.5 GB for 8192 robots x
 * 250 steps in f64) and the robot-migration queues are sized for the largest rollout geometry seen so far: the FIRST
 * rollout / step / time_* call of a larger geometry synchronises the DEVICE, frees and re-allocates them (never shrinks) -
 * the one hidden synchronisation of the otherwise stream-ordered calls, not legal inside a HIP stream capture, and the
 * place where an out-of-memory surfaces (SOLO_ERR_HIP) after create.  solo_engine_reserve does that work NOW for rollouts
 * of num_steps steps with these flags (and every shorter one under the same configuration): latency-sensitive or
 * graph-capturing callers call it once after solo_engine_set_program; later calls within the reserved geometry allocate
 * nothing and synchronise nothing.  Synchronises the device when it grows something. */
int solo_engine_reserve(SoloEngine* eng, int32_t num_steps, uint32_t flags);
/* Times ONE rollout of num_steps steps exactly as solo_engine_rollout_record runs it (solo_engine_plan's geometry; the
 * output buffers as there: NULL = that output is not recorded) with hipEvents recorded on the streams the kernels are
 * launched on; returns the mean milliseconds per LAUNCH over all slices and launches.  actions_dev: real [num_steps][N][12]. */
int solo_engine_time_rollout(SoloEngine* eng, const void* actions_dev, int32_t num_steps, uint32_t flags,
                             void* obs_out, void* reward_out, void* done_out, void* stream, double* ms_per_launch);
/* ---- joint control modes (setJointMotorControlArray's controlMode, solo8v2vanilla.py:87-90) ------------------------
 * What the motors do with the command of each actuated joint (set_targets / the actions of step and rollout):
 *  - SOLO_CTRL_POSITION (the default): pybullet's POSITION_CONTROL motor row with cfg.motor_kp / motor_kd, command =
 *    action x cfg.action_scale [rad] - the kernels of every earlier ABI, unchanged.
 *  - SOLO_CTRL_TORQUE: tau_j = clamp(action_j x action_scale, +-cfg.motor_torque_limit) [N m].
 *  - SOLO_CTRL_PD: explicit PD from the state at the START of each step (the ODRI motor-driver board; pybullet's
 *    PD_CONTROL with target velocity 0): tau_j = clamp(kp_j (action_j x action_scale - q_j) - kd_j qd_j, +-limit).
 * tau enters the step as a fixed joint impulse tau dt: the motor rows of the Gauss-Seidel iteration are pinned at
 * lo = hi = tau dt (they are solved first in every sweep, so the impulse is in place from the first sweep on and never
 * moves); contact and joint-limit rows are solved as in position mode.  A non-finite command restores the robot from
 * its snapshot and counts it (stats slot 5), as a non-finite target does in position mode.
 * The settle loop and the reset snapshot stay POSITION-controlled in every mode (as in the reference), so
 * set_control does not re-settle.  reset(), the in-kernel auto-reset and set_control itself leave every affected
 * robot's command at its mode's RESET COMMAND: 0 N m in torque mode, the settle pose (cfg.settle_targets, as reset
 * writes it) in position and PD modes.  The command buffer (SoloStateView::targets) holds radians in position / PD
 * mode and N m in torque mode.
 * NOT supported together with a torque / PD mode: robot migration (solo_engine_plan resolves migrate_steps to 0;
 * an explicit cfg.migrate_steps > 0 is rejected), cfg.solver_residual_threshold > 0 and cfg.solver_warm_start > 0:
 * solo_engine_set_control returns SOLO_ERR_INVALID_ARG for each. */
typedef enum SoloControlMode { SOLO_CTRL_POSITION = 0, SOLO_CTRL_TORQUE = 1, SOLO_CTRL_PD = 2 } SoloControlMode;
typedef struct SoloControl {
  int32_t mode;          /* SoloControlMode */
  int32_t reserved0;     /* = 0 */
  double kp[SOLO_NUM_DOF];  /* PD position gains [N m / rad] >= 0, dof order (engine-wide); read in PD mode only */
  double kd[SOLO_NUM_DOF];  /* PD velocity gains [N m s / rad] >= 0, dof order */
  double action_scale;   /* > 0: command = action x action_scale (torque / PD modes; position mode uses cfg.action_scale) */
} SoloControl;
/* Switches the joint control mode of every robot (validated first: a rejected call changes nothing) and sets every
 * robot's command to the mode's reset command.  Synchronises the device (like set_terrain); not legal inside a
 * stream capture - and a HIP graph captured BEFORE the call keeps launching the previous mode's kernel on commands now in
 * the new mode's units (N m in torque mode): re-capture graphs after switching.  solo_engine_kernel_name names the control kernel (solo_ctl_step_kernel) while a torque / PD mode
 * is active. */
int solo_engine_set_control(SoloEngine* eng, const SoloControl* ctl, void* stream);
/* The control mode in force (after create: SOLO_CTRL_POSITION with zero gains and cfg.action_scale). */
int solo_engine_get_control(SoloEngine* eng, SoloControl* out);
/* ---- contact sensing (pybullet getContactPoints(bodyA=robot)) ----------------------------------------------------------
 * The per-step CONTACT RECORD: real [N][SOLO_MAX_SPHERES][SOLO_CONTACT_WIDTH], one entry per model collision sphere:
 *   [0..2] the world-frame force on the robot at that sphere, f = (lam_n n + lam_t1 t1 + lam_t2 t2) / dt [N], where lam
 *          are the impulses the step's Gauss-Seidel iteration ended with on the sphere's normal and two friction rows and
 *          n, t1, t2 the directions those rows used: on the flat plane n = world z, t1 = world x, t2 = world y; on a
 *          heightfield n is the normal of the tangent plane under the sphere centre, t1 world x projected into that
 *          plane (normalised) and t2 = n x t1;
 *   [3]    the normal force lam_n / dt (>= 0).
 * The three rows act at the sphere's CONTACT POINT x = c - r n - c the sphere centre at the start of the step, r its radius, n
 * the ground normal under the centre (the same n on which the rows' directions are built): their Jacobians are those of the
 * velocity of the body-fixed point at x, and the force above is applied there.
 * A sphere without a contact row in the step reads all zeros.  Every launch that carries SOLO_STEP_PHYSICS writes the
 * record of the robots it steps (fused launches too: the record then holds the launch's LAST step); the settle loop
 * does not.  A robot that is reset - solo_engine_reset, the settle loop, the in-kernel auto-reset, the restore of a
 * diverged robot - reads zeros until its next physics step.  The record is not part of the state: a resumed run
 * recomputes it with its next step.  The observation sources SOLO_SRC_FOOT_FORCE + l hold column 3 of the record for
 * sphere 4l+1 of THIS step, in every output path (zero on a step that reset the robot).
 * NOT supported together with robot migration (cfg.migrate_steps > 0; the engine's own policy never migrates while
 * sensing is on), cfg.solver_residual_threshold > 0 or cfg.solver_warm_start > 0: SOLO_ERR_INVALID_ARG. */
#define SOLO_CONTACT_WIDTH 4
/* enable != 0: turns sensing on (allocates the record on first use and zeroes it; synchronises the device); the physics
 * launches then run the sensing kernels (solo_contact_kernel: the same step, bit for bit, plus the record).  0: off -
 * rejected while the registered observation program reads a SOLO_SRC_FOOT_FORCE source.  Re-capture HIP graphs after
 * switching. */
int solo_engine_set_contact_sensing(SoloEngine* eng, int32_t enable, void* stream);
/* *contact_dev = the device pointer of the record (engine-owned), or NULL while sensing is off. */
int solo_engine_get_contacts(SoloEngine* eng, void** contact_dev);
/* ---- control decimation ------------------------------------------------------------------------------------------------
 * decimation = D, 1 <= D <= SOLO_MAX_DECIMATION (after create: 1).  With D > 1 every step of every interface is a CONTROL
 * STEP: D consecutive physics steps of cfg.dt under the same action row, in ONE launch (solo_decim_kernel) - the motor rows
 * are rebuilt from the fresh state every physics step (PD mode: the law is re-evaluated; torque mode: tau stays constant).
 * Terminations are evaluated ONCE, after the last physics step: TimeBased counters, the episode length and every step count
 * of this ABI (rollout's K and its K rows of outputs, solo_engine_plan / solo_engine_reserve, cfg.steps_per_launch and the
 * record scratch) count control steps, and the episodic return sums one reward per control step.  A control step in which a
 * physics step diverges (non-finite state or command) ends at that physics step: the robot is restored from its snapshot
 * once, counted once (stats slot 5) and treated as a diverged step is with D = 1.  SoloStateView::cost stays in Gauss-Seidel
 * sweeps (of the D physics steps).  Launches without SOLO_STEP_PHYSICS, the settle loop (physics steps, position kernels),
 * reset and the snapshot are untouched, and with D = 1 the engine launches exactly the kernels it launches without this call.
 * The engine's own launch policy fuses min(K, max(1, 250 / D)) control steps per launch.
 * Configuration, not state: a checkpoint is restored into an engine with the same decimation.
 * D > 1 is NOT supported together with robot migration (solo_engine_plan resolves migrate_steps to 0; an explicit
 * cfg.migrate_steps > 0 is rejected), cfg.solver_residual_threshold > 0, cfg.solver_warm_start > 0 or contact sensing:
 * SOLO_ERR_INVALID_ARG for each, and solo_engine_set_contact_sensing(1) is rejected while D > 1.
 * Synchronises the device; not legal inside a stream capture, and a HIP graph captured BEFORE the call keeps launching the
 * previous kernel: re-capture graphs after the call. */
#define SOLO_MAX_DECIMATION 64
int solo_engine_set_decimation(SoloEngine* eng, int32_t decimation);
int solo_engine_get_decimation(SoloEngine* eng, int32_t* decimation);
/* ---- state terminations ---------------------------------------------------------------------------------------------------
 * Two termination kinds that read the robot's state record, in the ordered termination list next to the others (same OR /
 * short-circuit rule, SOLO_MAX_TERMS stays 4):
 *   SOLO_T_HEIGHT_BELOW  the condition is state[SOLO_S_POS + 2] < value: the base's WORLD z, also over a heightfield (the
 *                        height above the ground under the base is not what is compared)
 *   SOLO_T_TILT_ABOVE    the condition is c < value with c = 1 - 2 (qx^2 + qy^2), the world-z component of the body z axis:
 *                        value = cos(max tilt), computed by the host in double
 * value = values[t] of solo_engine_set_term_values for termination slot t (after create: 0 for every slot), converted to the
 * engine's precision; call it BEFORE solo_engine_set_program.  term_param[t] >= 0 is a GRACE COUNT: the termination's counter
 * term_count[:, t] ticks on every evaluation exactly as a SOLO_T_TIME counter does (not once an earlier termination has fired;
 * cleared by reset, auto-reset and a restore), and the termination fires when old + 1 > grace AND the condition holds.
 * The condition is evaluated once per control step, on the state after the step's last physics step (after a diverged robot
 * has been restored, before the auto-reset).  A fired state termination is a `done` like any other: event bits, auto-reset,
 * episodic statistics; with auto-reset off it keeps firing while the condition holds.  A launch with SOLO_STEP_DONE and
 * without SOLO_STEP_PHYSICS evaluates and ticks, as it does for SOLO_T_TIME.
 * WHICH ONE FIRED: uint8 [N] (solo_engine_get_term_fired), 0 = none, else 1 + the index of the first termination that fired -
 * written for the LAST control step of every launch that carries SOLO_STEP_DONE, while the program holds a state kind.  The
 * done flags stay 0 / 1.  Recording rollouts do not record it per step.
 * While the program holds a state kind the engine launches solo_term_kernel (in every control mode, with any decimation), and
 * only then.  NOT supported together with robot migration (solo_engine_plan resolves migrate_steps to 0; an explicit
 * cfg.migrate_steps > 0 is rejected), cfg.solver_residual_threshold > 0, cfg.solver_warm_start > 0 or contact sensing:
 * solo_engine_set_program returns SOLO_ERR_INVALID_ARG for each, and solo_engine_set_contact_sensing(1) is rejected while such
 * a program is registered.  The thresholds are configuration, not state (a checkpoint carries the counters, not them).
 * solo_engine_set_term_values synchronises the device; a HIP graph captured BEFORE a program change keeps launching the
 * previous kernel: re-capture graphs after it. */
int solo_engine_set_term_values(SoloEngine* eng, const double values[SOLO_MAX_TERMS]);
/* *fired_dev = the device pointer of the uint8 [N] record (engine-owned; zeros until a launch writes it). */
int solo_engine_get_term_fired(SoloEngine* eng, void** fired_dev);
/* ---- actuator randomisation ---------------------------------------------------------------------------------------------
 * The per-robot ACTUATOR BLOCK: real [N][SOLO_ACTUATOR_WIDTH], engine-owned, all ones when first switched on:
 *   [SOLO_ACT_TORQUE_LIMIT]  s:   the scale of the torque limit (every mode)
 *   [SOLO_ACT_KP]            a_p: the scale of every PD position gain (PD mode only)
 *   [SOLO_ACT_KD]            a_d: the scale of every PD velocity gain (PD mode only)
 *   [3]                      reserved: ignored by the kernels, kept as uploaded
 * Position mode: the motor rows' impulse clamp is +-(motor_torque_limit dt x s) - the uniform bound, in the engine's precision,
 * multiplied once.  Torque mode: tau = clamp(command, +-(motor_torque_limit x s)).  PD mode: tau = clamp((kp_j x a_p)(command
 * - q_j) - (kd_j x a_d) qd_j, +-(motor_torque_limit x s)): the scaled gains are formed first, then the law is evaluated as it
 * is without the block.  That order is part of the contract: with power-of-two scales a robot equals, bit for bit, a robot of
 * an engine created with the scaled limit and gains.  Evaluated every physics step (D times per control step under
 * decimation).  Values must be finite and >= 0 (0: a dead motor / a zero gain).
 * While a block is on, every launch outside the settle loop that steps the physics or evaluates state terminations runs
 * solo_act_kernel (every control mode, any decimation, programs with or without state terminations; solo_engine_kernel_name
 * names it); with an all-ones block it computes what the kernel it replaces computes, bit for bit.  The settle loop and the
 * reset snapshot do not read the block (nothing is re-settled), and solo_engine_reset, the in-kernel auto-reset and the
 * restore of a diverged robot leave it untouched, as they leave the friction coefficients.  Configuration, not state: a
 * checkpoint does not carry it, and one restored into an engine with the same block continues bit for bit.
 * NOT supported together with robot migration (solo_engine_plan resolves migrate_steps to 0 while a block is on; an explicit
 * cfg.migrate_steps > 0 is rejected), cfg.solver_residual_threshold > 0, cfg.solver_warm_start > 0 or contact sensing:
 * SOLO_ERR_INVALID_ARG for each, and solo_engine_set_contact_sensing(1) is rejected while a block is on. */
#define SOLO_ACTUATOR_WIDTH 4
#define SOLO_ACT_TORQUE_LIMIT 0
#define SOLO_ACT_KP 1
#define SOLO_ACT_KD 2
/* per_env_dev: real [N][SOLO_ACTUATOR_WIDTH] in device memory, copied into the engine's block (validated first, with one
 * device-to-host copy that synchronises the stream: a table with a NaN, an infinity or a negative value returns
 * SOLO_ERR_INVALID_ARG and leaves the previous block - or "off" - in force); NULL = off: the engine launches exactly the
 * kernels it launched before the first call.  In-place writes through solo_engine_get_actuators' pointer are not validated:
 * the caller's responsibility, as with SoloStateView::params.  Synchronises the device; not legal inside a stream capture,
 * and a HIP graph captured BEFORE an on / off switch keeps launching the previous kernel: re-capture graphs after it. */
int solo_engine_set_actuators(SoloEngine* eng, const void* per_env_dev, void* stream);
/* *dev = the device pointer of the block (engine-owned), or NULL while off. */
int solo_engine_get_actuators(SoloEngine* eng, void** dev);
/* ---- external base wrenches (pushes) -------------------------------------------------------------------------------------
 * The per-robot BASE WRENCH BLOCK: real [N][SOLO_WRENCH_WIDTH], engine-owned, all zeros when first switched on:
 *   [SOLO_WRENCH_FORCE  .. + 2]  f [N],   world frame, applied at the base link's centre of mass (SOLO_S_POS: validate_model
 *                                         requires the base frame to be the CoM frame)
 *   [SOLO_WRENCH_TORQUE .. + 2]  n [N m], world frame
 *   [6], [7]                     reserved: ignored by the kernels, kept as uploaded
 * While a block is on, EVERY PHYSICS STEP adds the wrench to the generalised force of the unconstrained update, next to
 * gravity and link damping - in every launch outside the settle loop that carries SOLO_STEP_PHYSICS, and in each of the D
 * substeps of a control step under decimation: u* = u + dt M^-1 (tau - h + Q) with Q = (n, f, 0_8) on the world-frame base
 * coordinates.  In the base frame the kernels work in that is rhs[0..2] += R^T n, rhs[3..5] += R^T f, with R the base rotation
 * at the START of the step (the one gravity is rotated with); each component of R^T v is fma(r2i, v.z, fma(r1i, v.y, r0i v.x)),
 * in that order.  The contact, joint-limit and motor rows are then solved from that u* as without a block: a push against a
 * standing robot is resisted by friction because the solver sees it.  The wrench is constant in the WORLD frame until the block
 * is changed: it does not rotate with the base and no step clears it (pybullet's applyExternalForce, which is cleared after
 * one stepSimulation and takes an application point, is a different contract and not offered).
 * While a block is on, every launch outside the settle loop that steps the physics runs solo_push_kernel (every control mode,
 * any decimation, programs with or without state terminations, the actuator block on or off; solo_engine_kernel_name names
 * it); with an all-zero block it computes what the kernel it replaces computes (as numbers: a zero that is added may change
 * the sign of a zero).  The settle loop and the reset snapshot do not read the block (nothing is re-settled), and
 * solo_engine_reset, the in-kernel auto-reset and the restore of a diverged robot leave it untouched, as they leave the
 * friction coefficients and the actuator block.  Configuration, not state: a checkpoint does not carry it, and one restored
 * into an engine with the same block continues bit for bit.
 * NOT supported together with robot migration (solo_engine_plan resolves migrate_steps to 0 while a block is on; an explicit
 * cfg.migrate_steps > 0 is rejected), cfg.solver_residual_threshold > 0, cfg.solver_warm_start > 0 or contact sensing:
 * SOLO_ERR_INVALID_ARG for each, and solo_engine_set_contact_sensing(1) is rejected while a block is on. */
#define SOLO_WRENCH_WIDTH 8
#define SOLO_WRENCH_FORCE 0
#define SOLO_WRENCH_TORQUE 3
/* per_env_dev: real [N][SOLO_WRENCH_WIDTH] in device memory, copied into the engine's block (validated first, with one
 * device-to-host copy that synchronises the stream: a table with a NaN or an infinity returns SOLO_ERR_INVALID_ARG and leaves
 * the previous block - or "off" - in force); NULL = off: the engine launches exactly the kernels it launched before.
 * Synchronises the device; not legal inside a stream capture, and a HIP graph captured BEFORE an on / off switch keeps launching
 * the previous kernel: re-capture graphs after it. */
int solo_engine_set_base_wrench(SoloEngine* eng, const void* per_env_dev, void* stream);
/* *dev = the device pointer of the block (engine-owned), or NULL while off.  The pointer is STABLE while the block stays on
 * (calls of solo_engine_set_base_wrench with a table included), and the kernels read the block at every launch: an in-place
 * write through it is picked up by the next launch, and by an already captured graph.  Such writes are not validated: a
 * non-finite one makes the state non-finite, and the robot is restored and counted in slot 5 of the statistics like any
 * diverged robot. */
int solo_engine_get_base_wrench(SoloEngine* eng, void** dev);
const char* solo_engine_last_error(SoloEngine* eng);
/* library-level: last error of a failed create (eng == NULL) */
const char* solo_last_create_error(void);
int solo_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SOLO_ENGINE_H_ */
