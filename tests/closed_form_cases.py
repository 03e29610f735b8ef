"""Closed forms of the CONSTRAINT rows - Coulomb friction, the saturated POSITION_CONTROL motor, the penetration
push-out - that hold whatever the solver's inner workings are ("pin the constraint rows with closed forms that do
not go through the oracle's step").  Each case is a set of initial states plus a checker of the state(s) a `stepSimulation`
(gym_solo/envs/solo8v2vanilla.py:87-91) leaves; tests/test_oracle_physics.py holds the CPU oracle to them (a few robots),
tests/test_gpu_closed_forms.py the HIP engine (4096 robots, through the C-ABI).  The checkers use Newton's law, Coulomb's law
and the model's masses / geometry only; of the oracle they use the KINEMATIC helpers (`momentum`, and `step_debug`'s CRBA
mass matrix M(q)) as measuring devices, never a step's result.

Conventions: state records [N, 32] (include/solo_engine.h), world-frame base velocities, generalised velocity
u = [R^T w, R^T v, qd] (base-body coordinates)."""
import numpy as np

from gym_solo_amd import abi
from gym_solo_amd.model import Solo8Model

THETA = np.radians(10.0)                                    # helpers.incline_terrain(10): h = tan(theta) x, uphill = +x
N_SLOPE = np.array([-np.sin(THETA), 0.0, np.cos(THETA)])    # ground normal
T1_SLOPE = np.array([np.cos(THETA), 0.0, np.sin(THETA)])    # world x projected into the tangent plane: UP the slope
VEL = (slice(abi.S_ANGVEL, abi.S_ANGVEL + 3), slice(abi.S_LINVEL, abi.S_LINVEL + 3), slice(abi.S_QD, abi.S_QD + 8))
NV = abi.NV


# ---- precision: inputs on the format's grid, and a rounding budget u n S next to every residual ------------------------------
# The closed forms hold whatever the solver does, so what an engine of dtype T leaves of them is ROUNDING: each checker below
# returns, with each residual, the budget u n S - u the unit roundoff of T, S the sum of the absolute values of the terms the
# identity adds (evaluated here, in f64), n the number of roundings on the longest path from the stored inputs to the stored
# outputs that enter the identity, COUNTED from gym_solo_amd/csrc/solo_step_kernel.h (the statements named below; one rounding per
# + - x of T, no contraction assumed - the emulator is built with -ffp-contract=off, a fused multiply-add only removes one -, and
# the bars tests/waveops_cases.py holds the header's math to: rsqrt, rcp, sqrt 1 ulp = 2 u, sincos 2 ulp = 4 u).  No count comes
# from a run of a kernel.  float64 callers that pass no dtype get what they always got.
def unit_roundoff(dtype):
  return 2.0 ** -24 if np.dtype(dtype) == np.float32 else 2.0 ** -53


def on_grid(a, dtype='float64'):
  """`a` rounded to the engine's dtype (what the engine holds of it), as float64"""
  return np.asarray(a, dtype=np.float64).astype(np.dtype(dtype)).astype(np.float64)


def model_on_grid(ma, dtype='float64'):
  """a copy of the SoloModel with every real rounded to dtype: the masses and the geometry the kernel computes with"""
  import ctypes as C
  out = type(ma)()
  C.memmove(C.addressof(out), C.addressof(ma), C.sizeof(ma))
  for name in ('joint_origin', 'joint_axis', 'mass', 'com', 'inertia', 'sphere_center', 'sphere_radius', 'joint_lower', 'joint_upper'):
    a = np.ctypeslib.as_array(getattr(out, name))
    a[...] = on_grid(a, dtype)
  return out


def unit_pose(s):
  """the state(s) with the quaternion normalised: the POSE a stored quaternion stands for.  The step uses the stored quaternion
  as it is (solo_step_kernel.h: r00 = 1 - 2 (qy qy + qz qz), ...; include/solo_engine.h, "state layout"); what that costs is in
  the budgets (ROUNDINGS['quat_*'])."""
  s = np.array(s, dtype=np.float64, copy=True)
  q = s[..., abi.S_QUAT:abi.S_QUAT + 4]
  s[..., abi.S_QUAT:abi.S_QUAT + 4] = q / np.linalg.norm(q, axis=-1, keepdims=True)
  return s


def constants_on_grid(ca, dtype='float64'):
  """the configuration's reals as make_params (solo_kernel_params.h) hands them to the kernel: dt, gravity, the damping
  coefficient rounded; motor_impulse = T(limit dt), erp_over_dt = T(erp / dt) rounded once from the f64 product / quotient"""
  class K:
    pass
  k = K()
  k.dt = float(on_grid(ca.dt, dtype))
  k.gravity = on_grid(list(ca.gravity), dtype)
  k.limit_dt = float(on_grid(ca.motor_torque_limit * ca.dt, dtype))
  k.erp_over_dt = float(on_grid(ca.contact_erp / ca.dt, dtype))
  k.linear_damping = float(on_grid(ca.linear_damping, dtype))
  k.u = unit_roundoff(dtype)
  return k


# n, per building block, with the statements of solo_step_kernel.h it counts (S of a rotated vector is its 1-norm: |R_ij| <= 1)
_R = {
  # one component of R v or R^T v from the stored quaternion and the stored v.  An entry of R: 1 - 2 (a + b) with a + b <= 1 -
  # two products, a sum, (x 2 exact), a difference: <= 5 u absolute; 2 (ab -+ cd): <= 3 u.  The component: three products, two
  # sums (gamma_3).  5 + 3
  'rotate': 8,
  # a velocity through one step: vb = R^T v, ub = vb + dt xb (physics_solve), ub + z, vn = R ub (physics_finish): 2 x rotate + 2
  'pass': 18,
  # the stored quaternion is used as it is, |q|^2 = 1 + e: R_k = (1 + e) R - e I, so R_k R_k^T v = v + 2 e v - e (R + R^T) v to
  # first order: 4 |e| |v|.  A unit quaternion rounded to T: every component off by u relative, e <= 2 u
  'quat_user': 8,
  # ... and one the kernel wrote (physics_finish: nn = rsqrt(nx nx + ny ny + nz nz + nw nw), nx nn, ...): the sum of four squares
  # 4 u, halved by the root, the root itself 2 u - a common factor 1 + 4 u, squared - and one product per component: e <= 10 u
  'quat_kernel': 40,
  # an entry of the joint-space inertia from the stored joint angles: q1 + q2 (1), sincos (4), o2 = o1 + roty (3 + 1), c = ob + roty
  # (3 + 1), r = c - o (1), mB dot(t, t) (1 + 5), + I[1] (1), both_halves (1) - the rotated inertia I (6) is the shorter branch
  'kin': 22,
  # through the factored inverse inertia (Cholesky of the four 2x2 leg blocks and of the 6x6 base Schur complement = Cholesky of
  # the 14 x 14 M in the order legs, base; the whitened rows ghat, hhat and physics_finish's back substitution are its solves):
  # counting that path is impractical - the backward-error bound of a Cholesky factor-and-solve of dimension d = NV = 14 instead,
  # |dM| <= gamma_(3 d + 1) |M| (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Theorem 10.4), plus one u per
  # elimination stage: the pivots are 1-ulp rsqrt's times a product where the theorem has a correctly rounded root and quotient
  'factor_solve': 3 * NV + 1 + NV,
  # a bias force from the stored velocities (physics_solve, "bias forces of the leg"): wB (1), wB2 (5), dot(wB, r) wB - wB2 r (3),
  # the sums of a_c (3), - gb + dB v_c (2), mB (1), r x F (3), + N.y (1), both_halves (1)
  'bias': 20,
  # what a unilateral / motor row's right-hand side costs: C = limit - q or the distance (1 ... 3), x inv_dt (1), inv_dt = T(1 / dt)
  # itself (1), and the Gauss-Seidel iteration ends within solver_ulp_tolerance = 2 half-ulps of the impulse
  'row_rhs': 7,
}
# n, per identity: the ONE table (DESIGN.md section 6 repeats it)
ROUNDINGS = {
  # M (u_post - u_pre) against +- limit dt / 0 (motor rows) and M (u_post - u_free) (limit row): M formed (kin), applied inverted
  # (factor_solve), the base part of u read back in the body frame of the pose (rotate + quat_user)
  'motor_clamp': _R['kin'] + _R['factor_solve'] + _R['rotate'] + _R['quat_user'],
  'limit_impulse': _R['kin'] + _R['factor_solve'] + _R['rotate'] + _R['quat_user'],
  # the joint's rate against min(free rate, C / dt): the row's right-hand side, and its solution through the same factors
  'limit_rate': _R['kin'] + _R['factor_solve'] + _R['row_rhs'],
  # the contact point's velocity v + w x arm against erp d / dt: the arm from the pose (rotate + quat_user, kin does not enter: a
  # base sphere), the row's right-hand side (the distance z + n . c - r: 3 of row_rhs), the solve, and v, w back in the world frame
  'push_out': _R['factor_solve'] + 2 * _R['rotate'] + _R['quat_user'] + _R['row_rhs'],
  # momenta of one step (Coulomb, free fall of a tumbling robot, the motors' internal impulses): every body's velocity is the base's
  # (pass + quat) plus the joint rates' share, which go through the dynamics (kin, bias, factor_solve)
  'momentum_step_user': _R['pass'] + _R['quat_user'] + _R['kin'] + _R['bias'] + _R['factor_solve'],
  'momentum_step_kernel': _R['pass'] + _R['quat_kernel'] + _R['kin'] + _R['bias'] + _R['factor_solve'],
  # a step of the k-step free fall (no rotation, no joint motion: the base velocity alone).  |v|: pass + quat_kernel (the first step
  # renormalises the quaternion); g dt: gravity into the base frame (rotate), m0 gb ... through the solve, dt xb (1)
  'free_fall_v': _R['pass'] + _R['quat_kernel'],
  'free_fall_g': _R['rotate'] + _R['bias'] + _R['factor_solve'] + 1,
  # the damped translation: as free fall, with kl (1 + sqrt(v . v)) v for g (dot 5, sqrt 2, 1 +, two products: + 10)
  'damping_v': _R['pass'] + _R['quat_user'],
  'damping_f': _R['rotate'] + _R['bias'] + _R['factor_solve'] + 1 + 10,
  # the air identity engine(S, tau) - oracle_off(S) = dt (fd(S, tau) - fd(S, 0)): the state's own velocity through a step (pass +
  # quat_user) and everything the dynamics add to it - the bias forces and M^-1 tau dt through kin and the factors
  'air_u': _R['pass'] + _R['quat_user'] + _R['kin'] + _R['bias'] + _R['factor_solve'],
}


def budget(dtype, name, S):
  """u n S"""
  return unit_roundoff(dtype) * ROUNDINGS[name] * S


def quat_about_y(angle):
  return np.array([0.0, np.sin(angle / 2), 0.0, np.cos(angle / 2)])


def rot(q):
  x, y, z, w = q
  return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                   [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                   [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def with_velocities(pre, post):
  """the configuration of `pre` with the velocities of `post`: the momentum of THAT state minus the momentum of `pre` is
  the impulse the step applied (a step changes velocities at the configuration it started from)"""
  s = pre.copy()
  for sl in VEL:
    s[sl] = post[sl]
  return s


class Kinematics:
  """The oracle's KINEMATIC helpers as measuring devices on the model the engine of `dtype` holds (model_on_grid), at the pose
  the state stands for (unit_pose): total and per-body momenta, centres of mass, the CRBA mass matrix.  Never a step's result."""

  def __init__(self, ca, ma, dtype='float64'):
    from oracle import solo_oracle as so
    self.dtype = dtype
    self.ma = model_on_grid(ma, dtype)
    import ctypes as C
    self.ca = type(ca)()
    C.memmove(C.addressof(self.ca), C.addressof(ca), C.sizeof(ca))
    for a in range(3):
      self.ca.gravity[a] = float(on_grid(ca.gravity[a], dtype))
    self.ph = so.OraclePhysics(self.ca, self.ma)
    self.masses = np.array(list(self.ma.mass))
    self.total_mass = float(self.masses.sum())
    self._single = []
    for b in range(abi.NUM_BODIES):     # body b alone: the model with every other mass and inertia zeroed
      one = model_on_grid(self.ma)
      for o in range(abi.NUM_BODIES):
        if o != b:
          one.mass[o] = 0.0
          for i in range(6):
            one.inertia[o][i] = 0.0
      self._single.append(so.OraclePhysics(ca, one))

  def momentum(self, s):
    """(linear [3], angular about the world origin [3])"""
    lin, ang, _ = self.ph.momentum(np.ascontiguousarray(unit_pose(s)))
    return lin.copy(), ang.copy()

  def body_momenta(self, s):
    """per body: (m_i v_i [9, 3], its angular momentum about the world origin [9, 3])"""
    s = np.ascontiguousarray(unit_pose(s))
    out = [one.momentum(s) for one in self._single]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])

  def body_coms(self, s):
    """world positions of the nine centres of mass [9, 3]: body b alone, translating at e_x / e_y, has the angular momentum
    c_b x m_b e about the origin"""
    p = np.ascontiguousarray(unit_pose(s))
    for sl in VEL:
      p[sl] = 0.0
    c = np.zeros((abi.NUM_BODIES, 3))
    for axis in (0, 1):
      p[VEL[1]] = np.eye(3)[axis]
      for b, one in enumerate(self._single):
        ang = one.momentum(p)[1] / self.masses[b]
        if axis == 0:
          c[b, 2], c[b, 1] = ang[1], -ang[2]
        else:
          c[b, 0] = ang[2]
    return c

  def mass_matrix(self, s):
    return np.array(self.ph.step_debug(np.ascontiguousarray(unit_pose(s)), np.zeros(8)).M).reshape(NV, NV)

  def free_momentum_change(self, pre, dt):
    """the linear momentum the step adds WITHOUT its constraint rows, at the configuration of `pre`: the momentum of u + dt a_0,
    a_0 the oracle's forward dynamics without joint torques (gravity and the velocity-product forces; m g dt for a robot at rest or
    in pure translation), minus the momentum of u"""
    s = np.ascontiguousarray(unit_pose(pre))
    a0 = self.ph.forward_dynamics(s.copy(), np.zeros(abi.NUM_DOF))[0]
    R = rot(s[abi.S_QUAT:abi.S_QUAT + 4])
    u0 = _gen_velocity(s, s)
    u = u0 + dt * a0
    u[3:6] += dt * np.cross(u0[:3], u0[3:6])   # (the oracle's accelerations are spatial: + w x v for the base origin's classical one)
    t = s.copy()
    t[VEL[0]], t[VEL[1]], t[VEL[2]] = R @ u[:3], R @ u[3:6], u[6:]
    return self.momentum(t)[0] - self.momentum(s)[0]

  def momenta_about_com(self, pre, post):
    """The momenta of the velocities of `post` at the configuration of `pre`, the angular one about the centre of mass, and
    the sums of absolute terms they are made of: (lin, ang_com, S_lin, S_ang)"""
    s = with_velocities(unit_pose(pre), post)
    lin_b, ang_b = self.body_momenta(s)
    coms = self.body_coms(s)
    com = (self.masses[:, None] * coms).sum(axis=0) / self.total_mass
    lin, ang = lin_b.sum(axis=0), ang_b.sum(axis=0)
    spin = ang_b - np.cross(coms, lin_b)
    S_ang = np.abs(spin).sum() + (np.abs(coms - com).sum(axis=1) * np.abs(lin_b).sum(axis=1)).sum()
    return lin, ang - np.cross(com, lin), float(np.abs(lin_b).sum()), float(S_ang)


# ---- (a) Coulomb on the incline ------------------------------------------------------------------------------------------
def standing_on_incline(n, lift=1e-3):
  """n robots standing (all joints 0: the motors hold the pose against targets 0) on the 10-degree incline, the base pitched
  with the slope so that the four feet meet the ground together; nothing but the feet is near the ground."""
  model = Solo8Model()
  st = np.zeros((n, abi.STATE_STRIDE))
  st[:, abi.S_POS:abi.S_POS + 3] = N_SLOPE * (0.32 + model.foot_radius + lift)
  st[:, abi.S_QUAT:abi.S_QUAT + 4] = quat_about_y(-THETA)
  return st


def incline_frictions(n, seed=0):
  """per-robot friction: the first half slides (mu < tan 10 deg = 0.176), the second half sticks"""
  rng = np.random.default_rng(seed)
  return np.concatenate([rng.uniform(0.02, 0.15, n // 2), rng.uniform(0.25, 1.0, n - n // 2)])


def check_coulomb_step(momentum, pre, post, mu, dt, g=9.81):
  """One step of one robot on the incline, every foot sliding DOWN the slope (friction rows along t1 saturated at + mu x
  their normal impulse): contact i applies lam_i (n + mu t1) + (its t2 impulse) t2, so the component of the step's total
  external impulse along w = t1 - mu n - perpendicular to all of that - is gravity's alone:
      (p_after - p_before) . w = - m g dt (sin theta - mu cos theta)
  however the normal load is shared between the feet.  Returns (measured, expected)."""
  m = Solo8Model().total_mass
  dp = momentum(with_velocities(pre, post)) - momentum(pre)
  w = T1_SLOPE - mu * N_SLOPE
  return float(dp @ w), -m * g * dt * (np.sin(THETA) - mu * np.cos(THETA))


# the distance of a leg's sphere to the heightfield's tangent plane from the stored state (physics_solve, "constraint rows"): the sphere
# in base coordinates (q1 + q2, sincos, two roty + sums: 13), cwz = z + n . cb (rotate + 1), the bilinear height and the normal (gu, fu:
# 4; hh0: 7; hx, hy, rsqrt: 3 + 2 of the longest branch), (cwz - hh0) nw.z - radius (3), and the stored quaternion (quat_kernel)
_R['contact_distance'] = 13 + _R['rotate'] + 1 + 16 + 3 + _R['quat_kernel']
ROUNDINGS['contact_distance'] = _R['contact_distance']


def rest_budget(kin, state, K, slope=np.tan(THETA)):
  """What rounding leaves of "at rest on the ground", as a momentum: a contact row's right-hand side is its distance x 1 / dt (or
  erp / dt), and the distance is a cancellation of the base height, the sphere's offset from the base, the ground's height under it and
  the radius - u n of THAT sum, through 1 / dt, is a velocity the solver gives the robot.  Returns u n m / dt max over the spheres of
  (|z| + |c_z - z| + |h(c_x)| + r), n = ROUNDINGS['contact_distance']."""
  s = np.ascontiguousarray(unit_pose(state))
  c = kin.ph.sphere_centers(s)
  r = np.array(list(kin.ma.sphere_radius))[:len(c)]
  z = s[abi.S_POS + 2]
  S = (abs(z) + np.abs(c[:, 2] - z) + np.abs(slope * c[:, 0]) + r).max()
  return budget(kin.dtype, 'contact_distance', kin.total_mass * S / K.dt)


def check_coulomb_step_budgeted(kin, pre, post, mu, K, count='momentum_step_kernel'):
  """check_coulomb_step at the precision of kin.dtype: mu, dt = K.dt and g = K.gravity as the engine holds them, the masses of
  the rounded model.  Returns (measured, expected, budget): S = the nine bodies' |m_i v_i| entering both momenta, projected with
  |w|, plus gravity's own term; n = ROUNDINGS[count] (momentum_step_kernel: the pose was written by the kernel)."""
  w = T1_SLOPE - mu * N_SLOPE
  lin_pre = kin.body_momenta(pre)[0]
  lin_post = kin.body_momenta(with_velocities(pre, post))[0]
  dp = lin_post.sum(axis=0) - lin_pre.sum(axis=0)
  want = float(kin.total_mass * K.dt * (K.gravity @ w))
  S = float(((np.abs(lin_pre) + np.abs(lin_post)) @ np.abs(w)).sum() + kin.total_mass * K.dt * (np.abs(K.gravity) @ np.abs(w)))
  return float(dp @ w), want, budget(kin.dtype, count, S)


# ---- (b) the saturated motor row -----------------------------------------------------------------------------------------
def floating_at_rest(n, seed=1, dtype='float64'):
  """n robots afloat (no contact) AT REST in random poses - no velocity, so no velocity-product forces: with zero gravity
  the only thing that acts in a step is the joint motors - and motor targets [n, 12]: per dof either FAR away (+-3 ... 6 rad:
  the row's target velocity kp (q* - q) / dt is hundreds of rad/s, far beyond what +-limit dt of impulse can give: saturated)
  or the joint's own angle (target velocity 0: the row holds the joint still with whatever impulse that takes)."""
  rng = np.random.default_rng(seed)
  st = np.zeros((n, abi.STATE_STRIDE))
  st[:, abi.S_POS + 2] = 2.0
  q = rng.normal(size=(n, 4))
  st[:, abi.S_QUAT:abi.S_QUAT + 4] = q / np.linalg.norm(q, axis=1, keepdims=True)
  st[:, abi.S_Q:abi.S_Q + 8] = rng.uniform(-1.5, 1.5, (n, 8))
  far = rng.random((n, 8)) < 0.6
  sign = np.where(rng.random((n, 8)) < 0.5, -1.0, 1.0)
  tgt = st[:, abi.S_Q:abi.S_Q + 8] + np.where(far, sign * rng.uniform(3.0, 6.0, (n, 8)), 0.0)
  st = on_grid(st, dtype)                                  # (dtype: the state as the engine holds it; a holding row's target
  tgt = np.where(far, on_grid(tgt, dtype), st[:, abi.S_Q:abi.S_Q + 8])   #  is the joint's STORED angle)
  acts = np.zeros((n, abi.NUM_JOINTS))
  for d in range(abi.NUM_DOF):
    acts[:, 3 * (d // 2) + d % 2] = tgt[:, d]
  return st, acts, far, sign


def _gen_velocity(pose, s):
  """u = [R^T w, R^T v, qd] of the velocities of `s` in the base frame of `pose` (its quaternion normalised)"""
  R = rot(unit_pose(pose)[abi.S_QUAT:abi.S_QUAT + 4])
  return np.concatenate([R.T @ s[VEL[0]], R.T @ s[VEL[1]], s[VEL[2]]])


def worst(pairs):
  """of (residual, budget) pairs - scalars or arrays - the one with the largest residual / budget: (residual, budget)"""
  best = (0.0, 1.0)
  for r, b in pairs:
    r, b = np.atleast_1d(np.asarray(r, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    b = np.broadcast_to(b, r.shape)
    if r.size == 0:
      continue
    i = int(np.argmax(np.where(b > 0, r / np.where(b > 0, b, 1.0), np.where(r > 0, np.inf, 0.0))))
    if (r[i] > 0 and b[i] <= 0) or r[i] * best[1] > best[0] * b[i]:
      best = (float(r[i]), float(b[i]))
  return best


def check_motor_clamp_budgeted(M, pre, post, far, sign, limit_dt, dtype='float64'):
  """M(q) du = J^T lam: with motor rows only, the generalised impulse of a step is 0 on the six base rows and lam_j on joint j.
  A row with a far target is SATURATED: lam_j = + limit dt towards the target.  A row whose target is the joint's own angle
  wants the joint at rest after the step (target velocity 0, kd = 1) and gets there unless the bound stops it
  (complementarity of a box-constrained row): either qd_j = 0 with |lam_j| <= limit dt, or lam_j = - sign(qd_j) limit dt.
  M: the CRBA mass matrix at `pre` (kinematics, not a step); limit_dt as the engine holds it.
  Budgets: impulse rows u n (|M| |u_post| + |M| |u_pre|) per row (limit dt is handed over on the engine's grid: it rounds nothing), n = ROUNDINGS['motor_clamp']; a holding joint's
  rate u n (|M^-1| |M du| + |u_pre|) - the terms its velocity is the sum of.  NO absolute threshold classifies a holding row: it
  is INSIDE its bound if |lam| < limit dt - budget (then |qd| <= its rate budget), otherwise it sits at the bound, against the
  motion where the joint moves by more than its rate budget.
  Returns {'base' | 'saturated' | 'holding inside' | 'holding at bound': (worst residual, its budget)} and the masks (inside, at
  bound).  (In f64 the rate of a row inside its bound is the Gauss-Seidel iteration's convergence, not rounding - oracle and kernel
  alike leave up to 4e-12 rad/s on the f64 tests' seeds -: the f64 callers, check_motor_clamp, do not hold it to this budget.)"""
  up, u0 = _gen_velocity(pre, post), _gen_velocity(pre, pre)
  imp = M @ (up - u0)
  bud = budget(dtype, 'motor_clamp', np.abs(M) @ (np.abs(up) + np.abs(u0)))
  rate_bud = budget(dtype, 'motor_clamp', np.abs(np.linalg.inv(M)) @ np.abs(imp) + np.abs(u0))[6:]
  lam, qd, jb = imp[6:], post[VEL[2]], bud[6:]
  inside = ~far & (np.abs(lam) < limit_dt - jb)
  at_bound = ~far & ~inside
  moving = np.abs(qd) > rate_bud
  res_bound = np.where(moving, np.abs(lam + np.sign(qd) * limit_dt), np.abs(np.abs(lam) - limit_dt))
  out = {'base': worst([(np.abs(imp[:6]), bud[:6])]),
         'saturated': worst([(np.abs(lam[far] - sign[far] * limit_dt), jb[far])]),
         'holding inside': worst([(np.abs(qd[inside]), rate_bud[inside])]),
         'holding at bound': worst([(res_bound[at_bound], jb[at_bound])])}
  return out, inside, at_bound


def check_motor_clamp(M, pre, post, far, sign, limit_dt):
  """The float64 callers' form: the worst violations (base rows, saturated rows, holding rows) in impulse units, and how many holding
  rows held / were at their bound - the expressions they always were (a row that holds may not exceed its bound, one at its bound sits
  there against the motion), under check_motor_clamp_budgeted's classification."""
  _, held, stopped = check_motor_clamp_budgeted(M, pre, post, far, sign, limit_dt)
  R = rot(pre[abi.S_QUAT:abi.S_QUAT + 4])
  def gen(s):
    return np.concatenate([R.T @ s[VEL[0]], R.T @ s[VEL[1]], s[VEL[2]]])
  imp = M @ (gen(post) - gen(pre))
  lam, qd = imp[6:], post[VEL[2]]
  worst_hold = 0.0
  if held.any():
    worst_hold = max(worst_hold, float(np.maximum(np.abs(lam[held]) - limit_dt, 0.0).max()))
  if stopped.any():
    worst_hold = max(worst_hold, float(np.abs(lam[stopped] + np.sign(qd[stopped]) * limit_dt).max()))
  return (float(np.abs(imp[:6]).max()), float(np.abs(lam[far] - sign[far] * limit_dt).max()) if far.any() else 0.0, worst_hold,
          int(held.sum()), int(stopped.sum()))


# ---- (c) the penetration push-out (erp) ----------------------------------------------------------------------------------
def belly_corner_penetrating(n, seed=2, dtype='float64'):
  """n robots AT REST, legs pointing up (nothing of a leg near the ground), the base rolled and pitched (0.12 ... 0.3 rad each,
  either sign) so that ONE bottom corner sphere of the base is the lowest point, penetrating the flat ground by d (0.05 ... 2 mm,
  per robot).  Returns (states, actions, depths, per robot: that sphere's centre in the base frame, the radius).
  dtype: everything as an engine of that dtype holds it, and the depth RECOMPUTED from the rounded height, the pose the rounded
  quaternion stands for and the rounded sphere (at 0.05 mm the depth moves by 1e-4 relative when z is rounded to f32)."""
  model = Solo8Model()
  rng = np.random.default_rng(seed)
  base = [(c, r) for b, c, r in model.spheres() if b == 0]
  st = np.zeros((n, abi.STATE_STRIDE))
  d = rng.uniform(5e-5, 2e-3, n)
  centres = np.zeros((n, 3))
  for e in range(n):
    roll, pitch = rng.uniform(0.12, 0.3, 2) * np.where(rng.random(2) < 0.5, -1.0, 1.0)
    cr, sr, cp, sp = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2)
    q = np.array([sr * cp, cr * sp, -sr * sp, cr * cp])              # pybullet's getQuaternionFromEuler(roll, pitch, 0)
    zs = [(rot(q) @ c)[2] - r for c, r in base]
    low = int(np.argmin(zs))
    centres[e] = base[low][0]
    st[e, abi.S_QUAT:abi.S_QUAT + 4] = q
    st[e, abi.S_POS + 2] = -d[e] - zs[low]
  st[:, abi.S_Q:abi.S_Q + 8] = np.tile([np.pi, 0.0], 4)              # legs straight up
  acts = np.zeros((n, abi.NUM_JOINTS))
  for leg in range(4):
    acts[:, 3 * leg] = np.pi
  radius = model.base_sphere_radius
  if np.dtype(dtype) != np.float64:
    st, acts, centres, radius = on_grid(st, dtype), on_grid(acts, dtype), on_grid(centres, dtype), float(on_grid(radius, dtype))
    pose = unit_pose(st)
    d = np.array([-(st[e, abi.S_POS + 2] + (rot(pose[e, abi.S_QUAT:abi.S_QUAT + 4]) @ centres[e])[2] - radius) for e in range(n)])
  return st, acts, d, centres, radius


def contact_point_velocity(post, pre, centre, radius):
  """world velocity, after the step, of the body-fixed point that was the sphere's contact point (centre - r z) at `pre`"""
  R = rot(pre[abi.S_QUAT:abi.S_QUAT + 4])
  arm = R @ centre - radius * np.array([0.0, 0.0, 1.0])
  return post[VEL[1]] + np.cross(post[VEL[0]], arm)


_R['distance'] = 18   # z + n . c - r: an entry of n from the quaternion (5), the dot product (3), two sums (2), quat_user (8)
ROUNDINGS['push_out_distance'] = _R['distance']


def check_push_out_budgeted(pre, post, centre, radius, d, erp_over_dt, dtype='float64'):
  """The contact point leaves the ground at erp d / dt, without tangential velocity.  Returns ((|v_z - erp d / dt|, budget),
  (max |v_xy|, budget)): S = |v| + |w x arm| + erp d / dt (1-norms of the terms), n = ROUNDINGS['push_out'] - plus what the
  distance itself is a cancellation of, erp / dt (|z| + |n . c| + r), n = ROUNDINGS['push_out_distance']: d is 0.05 ... 2 mm
  out of a height, an offset and a radius of 0.1 m each."""
  pose = unit_pose(pre)
  R = rot(pose[abi.S_QUAT:abi.S_QUAT + 4])
  arm = R @ centre - radius * np.array([0.0, 0.0, 1.0])
  v = post[VEL[1]] + np.cross(post[VEL[0]], arm)
  want = erp_over_dt * d
  w = np.abs(post[VEL[0]])
  S = np.abs(post[VEL[1]]).sum() + (w.sum() * np.abs(arm).sum() - w @ np.abs(arm)) + want   # (the six products of w x arm)
  S_d = erp_over_dt * (abs(pre[abi.S_POS + 2]) + np.abs(R[2] * centre).sum() + radius)
  b = budget(dtype, 'push_out', S) + budget(dtype, 'push_out_distance', S_d)
  return (abs(v[2] - want), b), (float(np.abs(v[:2]).max()), b)


# ---- (d) the base link keeps its own friction ------------------------------------------------------------------------------
def belly_on_incline(n, lift=5e-4):
  """n robots AT REST lying on the four bottom corner spheres of the base (legs straight up) on the 10-degree incline, the
  base pitched with the slope: the only contacts are the BASE link's.  gym_solo sets lateralFriction for links 0 .. 11 only
  (solo8v2vanilla.py:157-163): with lateral_friction = 0.1 < tan 10 deg the belly still has 0.5 and the robot stays."""
  model = Solo8Model()
  hz, r = model.base_sphere_half_extents[2], model.base_sphere_radius
  st = np.zeros((n, abi.STATE_STRIDE))
  st[:, abi.S_POS:abi.S_POS + 3] = N_SLOPE * (hz + r + lift)
  st[:, abi.S_QUAT:abi.S_QUAT + 4] = quat_about_y(-THETA)
  st[:, abi.S_Q:abi.S_Q + 8] = np.tile([np.pi, 0.0], 4)
  acts = np.zeros((n, abi.NUM_JOINTS))
  for leg in range(4):
    acts[:, 3 * leg] = np.pi
  return st, acts


# ---- (e) the joint-limit row ([recalled] btMultiBodyJointLimitConstraint; limits: the reference's getJointInfo fixture) -------
def joints_running_into_limits(n, limit=10.0, margin=0.5, seed=4, dtype='float64'):
  """n robots afloat, no gravity, motors WITHOUT torque (motor_torque_limit = 0: their rows are pinned to zero impulse), at rest
  but for ONE joint per robot, which sits C inside a limit (0.01 ... 0.3 rad, within joint_limit_margin) and moves towards it at s
  rad/s - some slow enough to stay inside within the step (s dt < C: the row must do NOTHING), some fast enough to cross it (the
  row must stop them at the speed that just reaches the limit, C / dt).  Returns (states, dof, side (+1 upper / -1 lower), C, s)."""
  rng = np.random.default_rng(seed)
  st = np.zeros((n, abi.STATE_STRIDE))
  st[:, abi.S_POS + 2] = 2.0
  q = rng.normal(size=(n, 4))
  st[:, abi.S_QUAT:abi.S_QUAT + 4] = q / np.linalg.norm(q, axis=1, keepdims=True)
  st[:, abi.S_Q:abi.S_Q + 8] = rng.uniform(-1.5, 1.5, (n, 8))
  dof = rng.integers(0, 8, n)
  side = np.where(rng.random(n) < 0.5, -1.0, 1.0)
  c = rng.uniform(0.01, 0.3, n)
  fast = rng.random(n) < 0.6
  s = np.where(fast, rng.uniform(1.2, 4.0, n), rng.uniform(0.05, 0.9, n)) * c / 1e-3   # relative to C / dt (dt = 1e-3)
  st[np.arange(n), abi.S_Q + dof] = side * (limit - c)
  st[np.arange(n), abi.S_QD + dof] = side * s
  if np.dtype(dtype) != np.float64:   # (as the engine holds it; the distance to the limit RECOMPUTED from the rounded angle)
    st = on_grid(st, dtype)
    c = limit - np.abs(st[np.arange(n), abi.S_Q + dof])
    s = np.abs(st[np.arange(n), abi.S_QD + dof])
  return st, dof, side, c, s


def check_joint_limit_budgeted(M, pre, post, free, dof, side, c, inv_dt, dtype='float64'):
  """The joint's rate TOWARDS its limit after the step is min(what it would be without the row, C / dt) - a unilateral row in
  speculative form: it acts only if the joint would cross the limit within the step, and then leaves it exactly ON the limit - and
  what the row adds to the step's generalised impulse, M(q) (u_post - u_free), is zero everywhere but on that joint's row, where it
  pushes AWAY from the limit.  `free` = the state after the same step from the same state with the limits far away (a single moving
  joint has velocity-product forces: they are in both).  M: the CRBA mass matrix at `pre`; C / dt = c inv_dt as the row forms it.
  Budgets: the rate u n (|rate_free| + |rate_post| + C / dt), n = ROUNDINGS['limit_rate']; the impulse rows
  u n (|M| |u_post| + |M| |u_free|), n = ROUNDINGS['limit_impulse'].  The row ACTED if its impulse is above its budget.
  Returns ((rate error, budget), (largest off-row impulse, its budget), (sign violation, budget), whether the row acted)."""
  up, uf = _gen_velocity(pre, post), _gen_velocity(pre, free)
  imp = M @ (up - uf)                           # what the limit row added to the step
  bud = budget(dtype, 'limit_impulse', np.abs(M) @ (np.abs(up) + np.abs(uf)))
  towards_free = side * free[abi.S_QD + dof]    # the rate towards the limit without the row
  towards = side * post[abi.S_QD + dof]
  want = min(towards_free, c * inv_dt)
  rate_bud = budget(dtype, 'limit_rate', abs(towards_free) + abs(towards) + c * inv_dt)
  lam = -side * imp[6 + dof]                    # the row's impulse, counted AWAY from the limit
  off = worst([(np.abs(np.delete(imp, 6 + dof)), np.delete(bud, 6 + dof))])
  return (abs(towards - want), rate_bud), off, (max(0.0, -lam), bud[6 + dof]), bool(lam > bud[6 + dof])


def check_joint_limit_against_free(M, pre, post, free, dof, side, c, dt):
  """check_joint_limit_budgeted for a float64 engine, in the form its first callers take:
  (rate error, largest off-row impulse, sign violation, whether the row acted)."""
  R = rot(pre[abi.S_QUAT:abi.S_QUAT + 4])
  def gen(s):
    return np.concatenate([R.T @ s[VEL[0]], R.T @ s[VEL[1]], s[VEL[2]]])
  imp = M @ (gen(post) - gen(free))
  towards_free = side * free[abi.S_QD + dof]
  towards = side * post[abi.S_QD + dof]
  want = min(towards_free, c / dt)
  lam = -side * imp[6 + dof]
  off = np.abs(np.delete(imp, 6 + dof)).max()
  acted = check_joint_limit_budgeted(M, pre, post, free, dof, side, c, 1.0 / dt)[3]   # (by the budget, not by an absolute threshold)
  return abs(towards - want), off, max(0.0, -lam), acted


# ---- (f) link damping ([recalled] btMultiBody: - m v k (1 + |v|) per link; configs.py:21-22 set k for every link) ------------------
def translating_afloat(n, seed=6, dtype='float64'):
  """n robots afloat in random poses, no gravity, no joint motion, no rotation: every link moves with the same velocity v0, so the
  total damping force is - m_total k (1 + |v0|) v0 and one explicit-Euler step leaves v0 (1 - dt k (1 + |v0|)), nothing else."""
  rng = np.random.default_rng(seed)
  st = np.zeros((n, abi.STATE_STRIDE))
  st[:, abi.S_POS + 2] = 2.0
  q = rng.normal(size=(n, 4))
  st[:, abi.S_QUAT:abi.S_QUAT + 4] = q / np.linalg.norm(q, axis=1, keepdims=True)
  st[:, abi.S_Q:abi.S_Q + 8] = rng.uniform(-1.5, 1.5, (n, 8))
  st[:, abi.S_LINVEL:abi.S_LINVEL + 3] = rng.uniform(-3.0, 3.0, (n, 3))
  acts = np.zeros((n, abi.NUM_JOINTS))
  for d in range(abi.NUM_DOF):
    acts[:, 3 * (d // 2) + d % 2] = st[:, abi.S_Q + d]     # the motors hold the pose (nothing for them to do)
  return on_grid(st, dtype), on_grid(acts, dtype)


def check_damped_translation_budgeted(M, pre, post, K, dtype='float64'):
  """One step of a pure translation leaves v0 (1 - dt k (1 + |v0|)) and nothing else.  Every link feels - m_i k (1 + |v0|) v0,
  in generalised coordinates - k (1 + |v0|) M u0, so the step adds - dt k (1 + |v0|) M^-1 (M u0) to u0 = [0, R^T v0, 0].
  Budgets: u (n_v |u0| + n_f dt k (1 + |v0|) |M^-1| |M| |u0|) per coordinate (ROUNDINGS['damping_v'], ['damping_f']); the base's
  world velocity carries the 1-norm of its three rows.  Returns ((|v - want|, budget), (|w|, budget), (|qd|, budget))."""
  v0 = pre[VEL[1]]
  speed = np.linalg.norm(v0)
  want = v0 * (1 - K.dt * K.linear_damping * (1 + speed))
  u0 = _gen_velocity(pre, pre)
  S_f = K.dt * K.linear_damping * (1 + speed) * (np.abs(np.linalg.inv(M)) @ (np.abs(M) @ np.abs(u0)))
  b = budget(dtype, 'damping_v', np.abs(u0)) + budget(dtype, 'damping_f', S_f)
  return (worst([(np.abs(post[VEL[1]] - want), b[3:6].sum())]), worst([(np.abs(post[VEL[0]]), b[0:3].sum())]),
          worst([(np.abs(post[VEL[2]]), b[6:])]))


# ---- (g) free fall and the momenta of one step in the air ----------------------------------------------------------------------
def afloat(st, rng, spin):
  """robots lifted above the ground (they fall 0.4 m at most in these tests), random joint angles; optionally moving in every
  coordinate (tests/test_gpu_closed_forms.py's _afloat)"""
  n = st.shape[0]
  st[:, abi.S_POS + 2] = rng.uniform(2.0, 3.0, n)
  st[:, abi.S_Q:abi.S_Q + 8] = rng.uniform(-1.5, 1.5, (n, 8))
  st[:, abi.S_LINVEL:abi.S_LINVEL + 3] = rng.uniform(-1.0, 1.0, (n, 3))
  st[:, abi.S_QD:abi.S_QD + 8] = 0.0
  st[:, abi.S_ANGVEL:abi.S_ANGVEL + 3] = 0.0
  if spin:
    st[:, abi.S_QD:abi.S_QD + 8] = rng.uniform(-3.0, 3.0, (n, 8))
    st[:, abi.S_ANGVEL:abi.S_ANGVEL + 3] = rng.uniform(-2.0, 2.0, (n, 3))
    q = rng.normal(size=(n, 4))
    st[:, abi.S_QUAT:abi.S_QUAT + 4] = q / np.linalg.norm(q, axis=1, keepdims=True)
  return st


def free_fall_closed_form(st0, k, K, dtype='float64'):
  """Semi-implicit Euler free fall without rotation or joint motion: v_k = v0 + g k dt, p_k = p0 + v0 k dt + g dt^2 k (k + 1) / 2,
  with dt and g as the engine holds them.  Budgets, per robot: v: u k (n_v max|v| + n_g |g| dt) (ROUNDINGS['free_fall_v'],
  ['free_fall_g']; max|v| <= |v0| + |g| k dt, 1-norms); p: every p += dt v rounds twice on |p| and carries dt x the velocity's
  error of that step: u k 2 max|p| + k dt (the v budget).  Returns (v_k, p_k, budget_v [n], budget_p [n])."""
  v0, p0 = st0[:, VEL[1]], st0[:, abi.S_POS:abi.S_POS + 3]
  g, dt, u = K.gravity, K.dt, unit_roundoff(dtype)
  vmax = np.abs(v0).sum(axis=1) + np.abs(g).sum() * k * dt
  bud_v = u * k * (ROUNDINGS['free_fall_v'] * vmax + ROUNDINGS['free_fall_g'] * np.abs(g).sum() * dt)
  pmax = np.abs(p0).sum(axis=1) + k * dt * vmax
  bud_p = u * k * 2 * pmax + k * dt * bud_v
  return v0 + g * k * dt, p0 + v0 * k * dt + g * dt * dt * k * (k + 1) / 2, bud_v, bud_p


def check_momenta_of_a_step(kin, pre, post_a, post_b, impulse, count='momentum_step_user'):
  """Linear momentum and angular momentum about the centre of mass of the velocities of `post_a` and of `post_b`, both at the
  configuration of `pre`: (a) - (b) = (impulse [3], 0).  post_b = pre with impulse = m g dt: one step of free fall of a tumbling
  robot; post_b = the same step with the motors off, impulse 0: the motors' impulses are internal.  S = the nine bodies' |m_i v_i|
  (and |I_i w_i| + |c_i - c| |m_i v_i|) of both sides plus |impulse|.  Returns ((linear residual, budget), (angular, budget))."""
  la, aa, Sla, Saa = kin.momenta_about_com(pre, post_a)
  lb, ab, Slb, Sab = kin.momenta_about_com(pre, post_b)
  return ((float(np.abs(la - lb - impulse).max()), budget(kin.dtype, count, Sla + Slb + np.abs(impulse).sum())),
          (float(np.abs(aa - ab).max()), budget(kin.dtype, count, Saa + Sab)))


# ---- (h) contact sensing: the recorded forces are the step's external impulse ------------------------------------------------------
# the record against the momenta of the step: those (momentum_step_kernel), and the record's own path - lam d into the world frame
# (rotate), x inv_dt (1, and T(1 / dt) itself 1), the sum of a sphere's three rows (2)
ROUNDINGS['contact_record'] = ROUNDINGS['momentum_step_kernel'] + _R['rotate'] + 4


def check_contact_record_budgeted(kin, pre, post, record, K):
  """Newton for the robot as a whole, at the configuration the step started from: the sum over the 16 spheres of the recorded world
  force x dt = the step's momentum change - what the step adds without its rows (Kinematics.free_momentum_change: m g dt for a robot
  at rest or in rigid translation; the motors' impulses are internal).  record [16, 4].
  S = the nine bodies' |m_i v_i| of both momenta + m |g| dt + sum |f_s| dt.  Returns (residual, budget)."""
  lin_pre = kin.body_momenta(pre)[0]
  lin_post = kin.body_momenta(with_velocities(pre, post))[0]
  f = np.asarray(record, dtype=np.float64)[:, :3]
  free = kin.free_momentum_change(pre, K.dt)
  res = np.abs(f.sum(axis=0) * K.dt - (lin_post.sum(axis=0) - lin_pre.sum(axis=0) - free)).max()
  S = np.abs(lin_pre).sum() + np.abs(lin_post).sum() + kin.total_mass * K.dt * np.abs(K.gravity).sum() + np.abs(f).sum() * K.dt
  return float(res), budget(kin.dtype, 'contact_record', S)


# ---- (i) the solved contact rows, per row: Newton on all fourteen rows of M du = J^T lam and the conditions of a unilateral row
#      with a friction box (tests/kkt_cases.py: the checkers; the counts are here, in the ONE table) ----------------------------------
# a leg sphere's contact arm x - p_j from the stored state (physics_solve, "constraint rows"): the sphere in base coordinates (q1 + q2,
# sincos, two roty + sums: 13, as in contact_distance), nloc = R^T nw on a heightfield (rotate), - radius x nloc (2), - p_j (1)
_R['leg_arm'] = 13 + _R['rotate'] + 2 + 1
# ... and the row's hip / knee column dot(d, ycross(x - p_j)): the arm, the direction d = R^T dw (rotate) of a tangent whose world
# components come from the normal (t1: 1 - nx nx 2, rsqrt 2, a product 1, x nx ny 1: 6; t2 = n x t1: + 3), two products and a sum
_R['leg_column'] = _R['leg_arm'] + _R['rotate'] + 9 + 3
# J^T lam of one contact into a generalised coordinate: a product per row, the sum of the sphere's three rows (the way of that
# impulse through the whitened rows and physics_finish's back substitution is factor_solve's)
_R['jt_lambda'] = 3
# a component of the recorded force (solo_step_body.h, "THE CONTACT RECORD"): a tangent's world component from the parked normal
# (9, as above), f = lam x inv_dt (1, and T(1 / dt) itself 1), f d (1), the sum of the sphere's three rows (2)
_R['record_force'] = 9 + 2 + 1 + 2
# the ground normal under a sphere centre from the stored state: contact_distance's path (the sphere in the world, the cell, the
# slopes, rsqrt) without the last three operations - counted as the whole of it
_R['ground_normal'] = _R['contact_distance']
# rho = M (u_post - u_free) - sum_s J_s^T f_s dt, per generalised coordinate: both velocities through a step (momentum_step_kernel),
# the contact Jacobian's longest column, J^T lam, the recorded force
ROUNDINGS['kkt_newton'] = ROUNDINGS['momentum_step_kernel'] + _R['leg_column'] + _R['jt_lambda'] + _R['record_force']
# f . n = entry 3: the recorded force, and how far the kernel's n is from unit (three squares and two sums halved by the root 3, rsqrt 2)
ROUNDINGS['kkt_normal'] = _R['record_force'] + 5
# |f . t| <= mu x entry 3: the recorded force, lim = mu x lam_n (1), entry 3 = lam_n x inv_dt (1)
ROUNDINGS['kkt_cone'] = _R['record_force'] + 2
# a contact row's velocity J_r u_post: u_post (momentum_step_kernel) and the row's longest column
ROUNDINGS['kkt_row'] = ROUNDINGS['momentum_step_kernel'] + _R['leg_column']
# ... and its right-hand side - d / dt or - erp d / dt: the distance (contact_distance) and row_rhs
ROUNDINGS['kkt_rhs'] = _R['contact_distance'] + _R['row_rhs']
# a position-mode motor row's rate against kp (q* - q) / dt + (1 - kd) u*_j: the joint's rate through the factors (limit_rate) and
# u*_j's bias forces
ROUNDINGS['kkt_motor'] = ROUNDINGS['limit_rate'] + _R['bias']


# ---- (j) the free dynamics and the pose update against the kinematics-only reference (tests/dynamics_cases.py: the reference and
#      the checkers; the counts are here, in the ONE table) -------------------------------------------------------------------------
# what air_u's bias does not count of a link's damping force (physics_solve, "bias forces of the leg": dB = kl (1 + sqrt(dot(v_c,
# v_c))), dB v_c; eB likewise): the dot product 5, halved by the root and the root's 2, 1 +, kl x, x v_c - damping_f's + 10
_R['damping_norm'] = 10
# the base's own mass and inertia: m0 = C.base_mass x mass_scale, I0[i] = C.base_I[i] x mass_scale (physics_solve, "the base body itself")
_R['mass_scale'] = 1
# |x+ - x - dt xdd_ref| per generalised coordinate, from a state the caller wrote / one the kernel wrote: the air identity's path
# with the damping's norm and the mass scale, which that identity - a DIFFERENCE of two steps under one damping and scale 1 - never met
ROUNDINGS['dyn_user'] = ROUNDINGS['air_u'] + _R['damping_norm'] + _R['mass_scale']
ROUNDINGS['dyn_kernel'] = ROUNDINGS['dyn_user'] - _R['quat_user'] + _R['quat_kernel']
# a component of q+ = normalise(exp(dt w+ / 2) (x) q) from the stored w+ and q (physics_finish), every component carrying S = 1, for
# x = |w+| dt / 2 <= 1; one count per side of sinc_cos' switch at x^2 = 1 / 16 (two code paths).  In units of u, absolute:
#   the argument x^2 = T(0.25) dt dt dot(wn, wn): the dot product 5, two products 2 (x 0.25 is exact): 7 relative
#   dw = cos x at the bars of tests/waveops_cases.py.  Taylor side (x <= 1 / 4): 2 ulp = 4 of a value <= 1 (f32; f64 1 ulp), the
#     argument through |x^2 cos'(x^2)| = x^2 sinc / 2 <= 1 / 32: + 1 = 5.  Library side (1 / 4 < x <= 1): (B_sqrt x + 1) eps <= 3 eps
#     = 6 (f64: B_sqrt = 2 ulp; f32 4), the argument through x^2 / 2 <= 1 / 2: + 4 = 10
#   a component of dv = wn (T(0.5) dt sinc x) (x 0.5 exact), at most sin x.  Taylor side: sinc 4 relative, the argument through
#     x^2 / 6: < 1, two products 2, of sin(1 / 4) < 1 / 4: 2.  Library side: sinc's bar (B_sqrt + 1 / x + 2) eps times the component's
#     |w| dt / 2 <= x: (B_sqrt x + 1 + 2 x) eps <= 5 eps = 10 (f64; f32 8), two products 2, the argument through x^2 / 6: 2 = 14
#   the Hamilton product: a component of it takes dw's error times one component of the unit q and dv's times the three others, at most
#     sqrt(a_w^2 + 3 a_v^2) - sqrt(25 + 12) < 7 | sqrt(100 + 588) < 27 - and its own four products and three sums, gamma_4 of
#     sum |d_i q_j| <= |d| |q| = 1: 4
#   the renormalisation: the sum of four squares gamma_5 halved by the root 3, rsqrt 1 ulp = 2, nx nn 1: 6
# (The stored q needs not be unit: the reference normalises the same product.)
ROUNDINGS['quat_update_taylor'] = 7 + 4 + 6
ROUNDINGS['quat_update_library'] = 27 + 4 + 6
# p+ = p + dt v+ and q_j+ = q_j + dt qd_j+ from the stored v+, qd+: the product and the sum, on |p| + dt |v+|
ROUNDINGS['pose_update'] = 2
