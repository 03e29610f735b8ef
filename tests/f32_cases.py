"""The closed forms of tests/closed_form_cases.py as CASES an engine of any precision runs: tests/test_emu_closed_forms_f32.py
(the f32 kernel source on the CPU emulator, 6 ... 24 robots) and tests/test_gpu_closed_forms_f32.py (the HIP engine, 256 robots)
share the generators, the checkers and the budgets through here.  An engine is driven through a small adapter X:
X.make(ca, ma, n, terrain=None, friction=None), X.put(e, state), X.get(e) -> float64 [n, 32], X.step(e, acts [n, 12]),
X.rollout(e, acts [k, n, 12]) (one fused launch sequence, physics only), X.diverged(e), X.close(e), X.n_small / X.n_large.

A case returns a REPORT: a list of (label, residual, budget, unit) - the worst residual / budget of each identity over the
batch; assert_within_budget holds every residual to its budget.  Single-step identities run either as one launch (fused = False)
or as the LAST step of a fused 3-step rollout, the checked state taken before that step from a twin engine (fused = True)."""
import numpy as np

import closed_form_cases as cf
from gym_solo_amd import abi
from helpers import incline_terrain, make_abi

REST = 1.5e-4   # m/s: what the reference's own rest test allows (test_solo8v2vanilla.py:77-104, 6 decimals over 10 steps)

BASE_FRICTION = [(0.1, 0.5, False), (0.1, 0.1, True), (0.9, 0.1, True)]
MULTI_STEP = ['free_fall_200', 'coulomb_incline'] + ['base_friction[%g-%g]' % (a, b) for a, b, _ in BASE_FRICTION]
SINGLE_STEP = ['free_fall_tumbling', 'motors_internal', 'motor_rows', 'push_out', 'joint_limit', 'damping']
# as the last step of a fused rollout: all but the push-out, which HAS no fused form.  A unilateral row only acts while the sphere
# leaves more slowly than erp d / dt, and after a first push-out step it does not (it left at erp d0 / dt > erp d1 / dt): from the
# second step on the closed form is an inequality.  Nor can lead steps bring a robot INTO the ground for the last one: the contact
# rows are speculative (a sphere within the margin may approach at distance / dt at most), so a step ends ON the ground, never inside
# it - penetration exists only as a state the caller writes.  (motor_rows leads in with two steps that command the joints' own
# angles: nothing moves.)
FUSED = [c for c in SINGLE_STEP if c != 'push_out']
CASES = MULTI_STEP + SINGLE_STEP


def show(where, case, report):
  for label, res, bud, unit in report:
    print('%s | %s | %s: worst residual / budget %.3g (%.3e of %.3e %s)' % (where, case, label, res / bud if bud > 0 else np.inf, res, bud, unit))


def assert_within_budget(report):
  bad = [(label, res, bud, unit) for label, res, bud, unit in report if not res <= bud]
  assert not bad, bad


def _entry(label, pairs, unit):
  res, bud = cf.worst(pairs)
  return (label, res, bud, unit)


def _hold_actions(st):
  a = np.zeros((st.shape[0], abi.NUM_JOINTS))
  for d in range(abi.NUM_DOF):
    a[:, 3 * (d // 2) + d % 2] = st[:, abi.S_Q + d]
  return a


def _last_step(X, e, twin, st, acts, fused, lead=None):
  """(checked state, state after the checked step) of engine e: the step alone, or the last of a fused 3-step rollout whose first two
  steps take `lead` (default: the same actions) - the checked state then comes from `twin`, an engine like e"""
  X.put(e, st)
  if not fused:
    X.step(e, acts)
    return st.copy(), X.get(e)
  lead = acts if lead is None else lead
  X.put(twin, st)
  X.rollout(twin, np.stack([lead, lead]))
  X.rollout(e, np.stack([lead, lead, acts]))
  return X.get(twin), X.get(e)


def run(case, X, dtype, fused=False):
  if case.startswith('base_friction'):
    leg_mu, base_mu = (float(x) for x in case[len('base_friction['):-1].split('-'))
    slides = [s for a, b, s in BASE_FRICTION if (a, b) == (leg_mu, base_mu)][0]
    return base_friction(X, dtype, leg_mu, base_mu, slides)
  return globals()[case](X, dtype, fused) if case in SINGLE_STEP else globals()[case](X, dtype)


# ---- free fall --------------------------------------------------------------------------------------------------------------------
def free_fall_200(X, dtype, k=200):
  """200 steps from poses without spin, motors without torque, no damping: base v and p against the closed form"""
  ca, ma = make_abi(dtype, linear_damping=0.0, angular_damping=0.0, motor_torque_limit=0.0)
  n = X.n_large
  e = X.make(ca, ma, n)
  K = cf.constants_on_grid(ca, dtype)
  st0 = cf.on_grid(cf.afloat(X.get(e), np.random.default_rng(5), spin=False), dtype)
  X.put(e, st0)
  X.rollout(e, np.zeros((k, n, 12)))
  st = X.get(e)
  v, p, bud_v, bud_p = cf.free_fall_closed_form(st0, k, K, dtype)
  report = [_entry('v after %d steps' % k, [(np.abs(st[:, cf.VEL[1]] - v).max(axis=1), bud_v)], 'm/s'),
            _entry('p after %d steps' % k, [(np.abs(st[:, abi.S_POS:abi.S_POS + 3] - p).max(axis=1), bud_p)], 'm')]
  assert X.diverged(e) == 0
  X.close(e)
  return report


def free_fall_tumbling(X, dtype, fused):
  """One step from a spinning, tumbling state: gravity changes the total momentum by m g dt and the angular momentum about the CoM
  not at all.  As an identity of the SCHEME this is a statement about the pair of steps with and without gravity from one state:
  u_g - u_0 = dt M^-1 Q_g exactly, and the momenta of that difference are (m g dt, 0).  (The momentum of ONE tumbling step changes by
  m g dt only up to the first-order integration error of semi-implicit Euler - tests/test_oracle_physics.py's
  test_momentum_conservation_zero_gravity (b) - which is 5.6e-4 kg m/s here in f64 and f32 alike: no rounding budget can hold it.)"""
  kw = dict(linear_damping=0.0, angular_damping=0.0, motor_torque_limit=0.0)
  ca, ma = make_abi(dtype, **kw)
  ca_0, _ = make_abi(dtype, gravity=(0., 0., 0.), **kw)
  n = X.n_large
  e, e0, twin = X.make(ca, ma, n), X.make(ca_0, ma, n), (X.make(ca, ma, n) if fused else None)
  K, kin = cf.constants_on_grid(ca, dtype), cf.Kinematics(ca, ma, dtype)
  st = cf.on_grid(cf.afloat(X.get(e), np.random.default_rng(6), spin=True), dtype)
  zero = np.zeros((n, 12))
  pre, post = _last_step(X, e, twin, st, zero, fused)
  X.put(e0, pre)
  X.step(e0, zero)
  post_0 = X.get(e0)
  count = 'momentum_step_kernel' if fused else 'momentum_step_user'
  lin, ang = [], []
  for i in range(n):
    a, b = cf.check_momenta_of_a_step(kin, pre[i], post[i], post_0[i], kin.total_mass * K.dt * K.gravity, count)
    lin.append(a); ang.append(b)
  assert X.diverged(e) == 0 and X.diverged(e0) == 0
  for x in (e, e0, twin):
    X.close(x)
  return [_entry('linear momentum: gravity adds m g dt', lin, 'kg m/s'), _entry('angular momentum about the CoM: gravity adds none', ang, 'kg m^2/s')]


def motors_internal(X, dtype, fused):
  """no gravity, no damping, no contact: the on / off pair of one step leaves the same linear and angular momentum"""
  kw = dict(gravity=(0., 0., 0.), linear_damping=0.0, angular_damping=0.0)
  ca, ma = make_abi(dtype, **kw)
  ca_off, _ = make_abi(dtype, motor_torque_limit=0.0, **kw)
  n = X.n_large
  on, off, twin = X.make(ca, ma, n), X.make(ca_off, ma, n), (X.make(ca, ma, n) if fused else None)
  kin = cf.Kinematics(ca, ma, dtype)
  rng = np.random.default_rng(9)
  st = cf.on_grid(cf.afloat(X.get(on), rng, spin=True), dtype)
  acts = cf.on_grid(rng.uniform(-2 * np.pi, 2 * np.pi, (n, 12)), dtype)
  pre, post_on = _last_step(X, on, twin, st, acts, fused)
  X.put(off, pre)
  X.step(off, acts)
  post_off = X.get(off)
  assert np.abs(post_on[:, cf.VEL[2]] - post_off[:, cf.VEL[2]]).max() > 1.0   # the motors did act
  count = 'momentum_step_kernel' if fused else 'momentum_step_user'
  lin, ang = [], []
  for i in range(n):
    a, b = cf.check_momenta_of_a_step(kin, pre[i], post_on[i], post_off[i], np.zeros(3), count)
    lin.append(a); ang.append(b)
  assert X.diverged(on) == 0 and X.diverged(off) == 0
  for e in (on, off, twin):
    X.close(e)
  return [_entry('linear momentum, motors on - off', lin, 'kg m/s'), _entry('angular momentum, motors on - off', ang, 'kg m^2/s')]


# ---- Coulomb ------------------------------------------------------------------------------------------------------------------------
def coulomb_incline(X, dtype, lead=250, checked=3, early=40):
  """standing on the 10-degree incline, per-robot friction: the slide identity on three checked steps after 250, the slide a rigid
  translation with a = g (sin theta - mu cos theta) over them, the sticking robots at rest.  (A sticking robot's friction rows are not
  saturated, so its contact impulse does not drop out of dp . w: that identity says "at rest", and its budget carries what rounding
  leaves of rest - closed_form_cases.rest_budget.)
  And ONE checked step EARLY in the slide (after `early` steps: landed, hardly moving): the budget grows with the slide's speed
  through the sum of |m_i v_i|, a wrong friction limit's defect - mu' m g cos(theta) dt per step - does not, so the early step is
  where a small one shows.  Its "does slide" guard is half of what the closed form gives after `early` steps, a dt early / 2."""
  ca, ma = make_abi(dtype, linear_damping=0.0, angular_damping=0.0)
  n = X.n_small
  mus = cf.on_grid(cf.incline_frictions(n, seed=5), dtype)
  e = X.make(ca, ma, n, terrain=incline_terrain(10.0), friction=mus)
  K, kin = cf.constants_on_grid(ca, dtype), cf.Kinematics(ca, ma, dtype)
  X.put(e, cf.on_grid(cf.standing_on_incline(n), dtype))
  zero = np.zeros((n, 12))
  slides = mus < np.tan(cf.THETA)
  g = -K.gravity[2]
  accel = g * (np.sin(cf.THETA) - mus * np.cos(cf.THETA))
  X.rollout(e, np.zeros((early, n, 12)))
  pre = X.get(e)
  X.step(e, zero)
  post = X.get(e)
  slide_early = []
  for i in np.flatnonzero(slides):
    got, want, bud = cf.check_coulomb_step_budgeted(kin, pre[i], post[i], mus[i], K)
    assert kin.momentum(post[i])[0] @ cf.T1_SLOPE / kin.total_mass < -0.5 * accel[i] * early * K.dt
    slide_early.append((abs(got - want), bud))
  X.rollout(e, np.zeros((lead - early - 1, n, 12)))
  slide, stick, rest, rigid = [], [], [], []
  first = X.get(e)
  acc = np.zeros(n)
  pre = first
  for k in range(checked):
    X.step(e, zero)
    post = X.get(e)
    for i in range(n):
      got, want, bud = cf.check_coulomb_step_budgeted(kin, pre[i], post[i], mus[i], K)
      if slides[i]:
        assert kin.momentum(post[i])[0] @ cf.T1_SLOPE < -0.05
        slide.append((abs(got - want), bud))
        acc[i] += bud
      else:
        stick.append((abs(got), bud + np.abs(cf.T1_SLOPE - mus[i] * cf.N_SLOPE).sum() * cf.rest_budget(kin, pre[i], K)))
        rest.append(np.abs(kin.momentum(post[i])[0]).max() / kin.total_mass)
    pre = post
  # the slide as a rigid translation: along t1 the friction is mu x the normal load of a robot that does not accelerate into the
  # ground, so dp . t1 = dp . w + mu dp . n = - m a dt per step with dp . n = 0 - each of the two held to the accumulated budget
  for i in np.flatnonzero(slides):
    dp = kin.momentum(post[i])[0] - kin.momentum(first[i])[0]
    rigid.append((abs(dp @ cf.T1_SLOPE + kin.total_mass * accel[i] * checked * K.dt), (1 + mus[i]) * acc[i]))
  assert X.diverged(e) == 0
  X.close(e)
  assert max(rest) < REST, max(rest)
  return [_entry('slide identity, step %d' % (early + 1), slide_early, 'kg m/s'), _entry('slide identity', slide, 'kg m/s'), _entry('sticking feet', stick, 'kg m/s'),
          _entry('rigid translation over %d steps' % checked, rigid, 'kg m/s')]


def base_friction(X, dtype, leg_mu, base_mu, slides, lead=119, early=20):
  """lying on the base link's four bottom spheres on the incline: the base link keeps base_lateral_friction whatever the legs'
  coefficient - Coulomb's identity with the BASE coefficient where it slides, at rest where it holds; where it slides also on one
  step EARLY in the slide (see coulomb_incline)"""
  ca, ma = make_abi(dtype, lateral_friction=leg_mu, base_lateral_friction=base_mu, linear_damping=0.0, angular_damping=0.0)
  n = X.n_small
  e = X.make(ca, ma, n, terrain=incline_terrain(10.0), friction=np.full(n, leg_mu))
  K, kin = cf.constants_on_grid(ca, dtype), cf.Kinematics(ca, ma, dtype)
  mu = float(cf.on_grid(base_mu, dtype))
  st, acts = cf.belly_on_incline(n)
  st, acts = cf.on_grid(st, dtype), cf.on_grid(acts, dtype)
  X.put(e, st)
  report = []
  if slides:
    accel = -K.gravity[2] * (np.sin(cf.THETA) - mu * np.cos(cf.THETA))
    X.rollout(e, np.broadcast_to(acts, (early,) + acts.shape).copy())
    pre = X.get(e)
    X.step(e, acts)
    post = X.get(e)
    first = []
    for i in range(n):
      got, want, bud = cf.check_coulomb_step_budgeted(kin, pre[i], post[i], mu, K)
      assert kin.momentum(post[i])[0] @ cf.T1_SLOPE / kin.total_mass < -0.5 * accel * early * K.dt
      first.append((abs(got - want), bud))
    report.append(_entry('base link slides, step %d' % (early + 1), first, 'kg m/s'))
    X.rollout(e, np.broadcast_to(acts, (lead - early - 1,) + acts.shape).copy())
  else:
    X.rollout(e, np.broadcast_to(acts, (lead,) + acts.shape).copy())
  pre = X.get(e)
  X.step(e, acts)
  post = X.get(e)
  pairs = []
  for i in range(n):
    got, want, bud = cf.check_coulomb_step_budgeted(kin, pre[i], post[i], mu, K)
    v = kin.momentum(post[i])[0] / kin.total_mass
    if slides:
      assert v @ cf.T1_SLOPE < -0.05
      pairs.append((abs(got - want), bud))
    else:
      assert np.abs(v).max() < REST
      pairs.append((abs(got), bud + np.abs(cf.T1_SLOPE - mu * cf.N_SLOPE).sum() * cf.rest_budget(kin, pre[i], K)))
  assert X.diverged(e) == 0
  X.close(e)
  return report + [_entry('base link %s' % ('slides' if slides else 'holds'), pairs, 'kg m/s')]


def contact_record(X, dtype, lead=250):
  """contact sensing, robots settled or sliding on the incline, damping off: the sum over the 16 spheres of the recorded world force
  x dt = the step's momentum change - m g dt - more exactly, minus what the step adds without its rows (Kinematics.free_momentum_change):
  the sticking robots' transient is still decaying after 250 steps, and its velocity-product term, m w^2 r dt = 2e-15 kg m/s, is three
  times the f64 budget of a robot at rest.  X.step_record(e, acts) -> the record [n, 16, 4] of that step."""
  ca, ma = make_abi(dtype, linear_damping=0.0, angular_damping=0.0)
  n = X.n_small
  mus = cf.on_grid(cf.incline_frictions(n, seed=5), dtype)
  e = X.make(ca, ma, n, terrain=incline_terrain(10.0), friction=mus)
  K, kin = cf.constants_on_grid(ca, dtype), cf.Kinematics(ca, ma, dtype)
  X.put(e, cf.on_grid(cf.standing_on_incline(n), dtype))
  X.rollout(e, np.zeros((lead, n, 12)))
  pre = X.get(e)
  rec = X.step_record(e, np.zeros((n, 12)))
  post = X.get(e)
  slides = mus < np.tan(cf.THETA)
  weight = -kin.total_mass * K.gravity[2]
  assert np.all(rec[:, :, 3].sum(axis=1) > 0.5 * weight)     # (every robot stands on the ground)
  pairs = {True: [], False: []}
  for i in range(n):
    pairs[bool(slides[i])].append(cf.check_contact_record_budgeted(kin, pre[i], post[i], rec[i], K))
  assert X.diverged(e) == 0
  X.close(e)
  return [_entry('recorded impulse, sliding robots', pairs[True], 'kg m/s'), _entry('recorded impulse, sticking robots', pairs[False], 'kg m/s')]


# ---- the rows -----------------------------------------------------------------------------------------------------------------------
def motor_rows(X, dtype, fused):
  """afloat at rest, no gravity: M du of one step is 0 on the base rows, + limit dt on the saturated rows, and a holding row rests
  or sits at its bound against the motion (fused: the first two steps command the joints' own angles - nothing moves)"""
  ca, ma = make_abi(dtype, gravity=(0., 0., 0.), linear_damping=0.0, angular_damping=0.0)
  n = X.n_large
  e, twin = X.make(ca, ma, n), (X.make(ca, ma, n) if fused else None)
  K, kin = cf.constants_on_grid(ca, dtype), cf.Kinematics(ca, ma, dtype)
  st, acts, far, sign = cf.floating_at_rest(n, dtype=dtype)
  pre, post = _last_step(X, e, twin, st, acts, fused, lead=_hold_actions(st))
  out = {}
  held = stopped = 0
  for i in range(n):
    o, inside, at_bound = cf.check_motor_clamp_budgeted(kin.mass_matrix(pre[i]), pre[i], post[i], far[i], sign[i], K.limit_dt, dtype)
    for key, pair in o.items():
      out.setdefault(key, []).append(pair)
    held += int(inside.sum()); stopped += int(at_bound.sum())
  assert held > 0 and stopped > 0, (held, stopped)
  assert X.diverged(e) == 0
  for x in (e, twin):
    X.close(x)
  return [_entry(key + ' rows' if key != 'holding inside' else 'holding rows inside their bound (rate)', pairs,
                 'rad/s' if key == 'holding inside' else 'N m s') for key, pairs in out.items()]


def _depth(pre, centre, radius):
  R = cf.rot(cf.unit_pose(pre)[abi.S_QUAT:abi.S_QUAT + 4])
  return -(pre[abi.S_POS + 2] + (R @ centre)[2] - radius)


def push_out(X, dtype, fused):
  """at rest, one base sphere 0.05 ... 2 mm inside the flat ground: the contact point leaves at erp d / dt, no tangential velocity"""
  ca, ma = make_abi(dtype)
  n = X.n_large
  e, twin = X.make(ca, ma, n), (X.make(ca, ma, n) if fused else None)
  K = cf.constants_on_grid(ca, dtype)
  st, acts, d, centres, radius = cf.belly_corner_penetrating(n, dtype=dtype)
  pre, post = _last_step(X, e, twin, st, acts, fused)
  vz, vxy = [], []
  for i in range(n):
    depth = _depth(pre[i], centres[i], radius) if fused else d[i]
    assert depth > 0
    a, b = cf.check_push_out_budgeted(pre[i], post[i], centres[i], radius, depth, K.erp_over_dt, dtype)
    vz.append(a); vxy.append(b)
  assert X.diverged(e) == 0
  for x in (e, twin):
    X.close(x)
  return [_entry('push-out velocity', vz, 'm/s'), _entry('tangential velocity', vxy, 'm/s')]


def joint_limit(X, dtype, fused):
  """one joint per robot running into its limit, against the far-limits twin: the rate, the off-row impulse, the sign"""
  from gym_solo_amd.model import Solo8Model
  ca, ma = make_abi(dtype, gravity=(0., 0., 0.), linear_damping=0.0, angular_damping=0.0, motor_torque_limit=0.0)
  far = Solo8Model().to_abi()
  for j in range(abi.NUM_DOF):
    far.joint_lower[j], far.joint_upper[j] = -1e3, 1e3
  n = X.n_large
  e, free, twin = X.make(ca, ma, n), X.make(ca, far, n), (X.make(ca, ma, n) if fused else None)
  kin = cf.Kinematics(ca, ma, dtype)
  inv_dt = float(cf.on_grid(1.0 / ca.dt, dtype))
  st, dof, side, c, s = cf.joints_running_into_limits(n, margin=ca.joint_limit_margin, dtype=dtype)
  zero = np.zeros((n, 12))
  pre, post = _last_step(X, e, twin, st, zero, fused)
  X.put(free, pre)
  X.step(free, zero)
  post_free = X.get(free)
  rate, off, sign, acted = [], [], [], 0
  for i in range(n):
    ci = 10.0 - abs(pre[i, abi.S_Q + dof[i]])     # (the distance to the limit of the CHECKED state)
    if ci <= 0:
      continue   # (fused: a joint the first steps left ON its limit to rounding is pushed back with the erp - another closed form)
    r, o, sg, on = cf.check_joint_limit_budgeted(kin.mass_matrix(pre[i]), pre[i], post[i], post_free[i], dof[i], side[i], ci, inv_dt, dtype)
    rate.append(r); off.append(o); sign.append(sg)
    acted += int(on)
  assert acted > 0, (acted, len(rate))   # (some rows did act in the checked step)
  assert X.diverged(e) == 0 and X.diverged(free) == 0
  for x in (e, free, twin):
    X.close(x)
  return [_entry('rate towards the limit', rate, 'rad/s'), _entry('off-row impulse', off, 'N m s'), _entry('impulse sign', sign, 'N m s')]


def damping(X, dtype, fused):
  """a pure translation afloat, no gravity: one step leaves v0 (1 - dt k (1 + |v0|)) and nothing else"""
  ca, ma = make_abi(dtype, gravity=(0., 0., 0.))
  n = X.n_large
  e, twin = X.make(ca, ma, n), (X.make(ca, ma, n) if fused else None)
  K, kin = cf.constants_on_grid(ca, dtype), cf.Kinematics(ca, ma, dtype)
  st, acts = cf.translating_afloat(n, dtype=dtype)
  pre, post = _last_step(X, e, twin, st, acts, fused)
  v, w, qd = [], [], []
  for i in range(n):
    a, b, c = cf.check_damped_translation_budgeted(kin.mass_matrix(pre[i]), pre[i], post[i], K, dtype)
    v.append(a); w.append(b); qd.append(c)
  assert X.diverged(e) == 0
  for x in (e, twin):
    X.close(x)
  return [_entry('translation', v, 'm/s'), _entry('base rotation', w, 'rad/s'), _entry('joint rates', qd, 'rad/s')]


# ---- the air identity of tests/control_cases.py (torque and PD mode; the emulator's control harness) -----------------------------------
def air_identity_emu(mode, dtype, run_ctl, control, n=32):
  """engine(S, tau) - oracle_off(S) = dt (fd(S, tau) - fd(S, 0)), the oracle stepping from the f32-rounded S with the rounded model
  and dt.  Budget per coordinate: u n (dt |M^-1| (|tau terms| + |M a0|) + |u|), n = ROUNDINGS['air_u']."""
  import ctypes as C
  from control_cases import air_states, rotation
  from gym_solo_amd.model import DOF_TO_JOINT
  from oracle import solo_oracle as so
  ca, ma = make_abi(dtype)
  K = cf.constants_on_grid(ca, dtype)
  def rounded(**kw):
    c, _ = make_abi(dtype, **kw)
    c.dt = K.dt
    return c
  mg = cf.model_on_grid(ma, dtype)
  rng = np.random.default_rng(11 if mode == 'torque' else 12)
  S = cf.on_grid(air_states(rng, n), dtype)
  L = float(cf.on_grid(ca.motor_torque_limit, dtype))
  a = np.zeros((n, abi.NUM_JOINTS))
  if mode == 'torque':
    tau = cf.on_grid(rng.uniform(-0.99 * L, 0.99 * L, (n, abi.NUM_DOF)), dtype)
    a[:, DOF_TO_JOINT] = tau
    terms = np.abs(tau)
    ctl = control(abi.CTRL_TORQUE)
  else:
    kp, kd = cf.on_grid(rng.uniform(1.0, 4.0, abi.NUM_DOF), dtype), cf.on_grid(rng.uniform(0.01, 0.05, abi.NUM_DOF), dtype)
    a = cf.on_grid(rng.uniform(-3, 3, (n, abi.NUM_JOINTS)), dtype)
    q, qd = S[:, abi.S_Q:abi.S_Q + 8], S[:, abi.S_QD:abi.S_QD + 8]
    raw = kp * (a[:, DOF_TO_JOINT] - q) - kd * qd
    tau = np.clip(raw, -L, L)
    terms = np.abs(kp * (a[:, DOF_TO_JOINT] - q)) + np.abs(kd * qd)
    ctl = control(abi.CTRL_PD, kp, kd)
  got = S.copy()
  run_ctl(ca, ma, ctl, got, a[None])
  ref = cf.unit_pose(S)
  so.OraclePhysics(rounded(motor_torque_limit=0.0), mg).step(ref, np.zeros((n, abi.NUM_JOINTS)))
  ph = so.OraclePhysics(rounded(), mg)
  Rt = np.transpose(rotation(cf.unit_pose(S)[:, abi.S_QUAT:abi.S_QUAT + 4]), (0, 2, 1))
  pairs_qd, pairs_tw = [], []
  for e in range(n):
    pose = cf.unit_pose(S[e])
    a_tau = ph.forward_dynamics(pose.copy(), tau[e])[0]
    a_0 = ph.forward_dynamics(pose.copy(), np.zeros(abi.NUM_DOF))[0]
    want = K.dt * (a_tau - a_0)
    M = np.array(ph.step_debug(pose.copy(), np.zeros(8)).M).reshape(abi.NV, abi.NV)
    d = np.concatenate([Rt[e] @ (got[e, cf.VEL[0]] - ref[e, cf.VEL[0]]), Rt[e] @ (got[e, cf.VEL[1]] - ref[e, cf.VEL[1]]),
                        got[e, cf.VEL[2]] - ref[e, cf.VEL[2]]])
    gen_terms = np.concatenate([np.zeros(6), terms[e]])
    u0 = np.concatenate([Rt[e] @ S[e, cf.VEL[0]], Rt[e] @ S[e, cf.VEL[1]], S[e, cf.VEL[2]]])
    Sj = K.dt * (np.abs(np.linalg.inv(M)) @ (gen_terms + np.abs(M @ a_0))) + np.abs(u0)
    bud = cf.budget(dtype, 'air_u', Sj)
    pairs_qd.append((np.abs(d - want)[6:], bud[6:]))
    pairs_tw.append((np.abs(d - want)[:6], np.concatenate([np.full(3, bud[0:3].sum()), np.full(3, bud[3:6].sum())])))
  assert np.abs(got[:, cf.VEL[2]] - ref[:, cf.VEL[2]]).max() > 1e-3   # (tau did something)
  return [_entry('joint rates', pairs_qd, 'rad/s'), _entry('base twist', pairs_tw, 'rad/s | m/s')]
