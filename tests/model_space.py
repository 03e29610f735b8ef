"""Points of the MODEL space `validate_model` admits (gym_solo_amd/csrc/solo_kernel_params.h), shared by the oracle, emulator
(CPU) and GPU parity tests the way tests/config_space.py shares points of the configuration space.

The built-in Solo8Model is a very special point of that family: no Ixy / Ixz anywhere, a diagonal base inertia, knee origin
x = 0, mirrored legs, +-10 rad limits and both leg spheres on the LOWER link - so pack_params' xy / xz copies, the full 6 x 6
composite inertia of leg_sum_entry, the BODY_UPPER sphere transform and the per-leg table indices only ever saw zeros or one
branch.  `random_model(seed)` moves every one of them at once; the named edge models move ONE thing each, so a failure
points at a term; `invalid_models()` holds one mutation per rejection clause of validate_model.

The helpers at the end are the conditions that keep a parity test from passing vacuously, all evaluated on the ORACLE's
trajectory: how many spheres have live contact rows, whether an upper-link sphere touches, whether a joint sits inside the
limit margin while the robot is in contact."""
import numpy as np

from gym_solo_amd import abi
from gym_solo_amd.model import DOF_TO_JOINT, LinkInertial, Solo8Model, model_to_abi

RANDOM_SEEDS = (0, 1, 2)
EDGE_MODELS = ('offdiag_base', 'offdiag_legs', 'knee_x', 'asymmetric', 'upper_spheres', 'tight_limits')


class TableModel:
  """A Solo8-family model as explicit per-body tables, with the accessor interface model_to_abi takes.  `lowers` are the
  lower legs WITH their welded feet."""

  def __init__(self, source=None):
    m = source or Solo8Model()
    copy = lambda li: LinkInertial(float(li.mass), np.array(li.com, dtype=np.float64), np.array(li.inertia, dtype=np.float64))
    self._base = copy(m.base())
    self.uppers = [copy(m.upper(leg)) for leg in range(abi.NUM_LEGS)]
    self.lowers = [copy(m.lower_with_foot(leg)) for leg in range(abi.NUM_LEGS)]
    self.hips = [np.array(m.hip_origin(leg), dtype=np.float64) for leg in range(abi.NUM_LEGS)]
    self.knees = [np.array(m.knee_origin(leg), dtype=np.float64) for leg in range(abi.NUM_LEGS)]
    self._spheres = [(int(b), np.array(c, dtype=np.float64), float(r)) for b, c, r in m.spheres()]
    self.limits = [(float(lo), float(hi)) for lo, hi in m.joint_limits()]

  def base(self): return self._base
  def upper(self, leg): return self.uppers[leg]
  def lower_with_foot(self, leg): return self.lowers[leg]
  def hip_origin(self, leg): return self.hips[leg]
  def knee_origin(self, leg): return self.knees[leg]
  def spheres(self): return list(self._spheres)
  def joint_limits(self): return list(self.limits)

  def bodies(self):
    """the nine bodies in C-ABI order: base, then upper / lower of every leg"""
    out = [self._base]
    for leg in range(abi.NUM_LEGS):
      out += [self.uppers[leg], self.lowers[leg]]
    return out

  @property
  def total_mass(self):
    return sum(b.mass for b in self.bodies())

  def to_abi(self):
    return model_to_abi(self)


def _rotation(axis, angle):
  """Rodrigues: rotation by `angle` about `axis`"""
  a = np.asarray(axis, dtype=np.float64)
  a = a / np.linalg.norm(a)
  K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
  return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def _tilt(li, axis, angle, scale=(1.0, 1.0, 1.0)):
  """the body's inertia tensor with its principal values rescaled and its principal axes rotated: symmetric, positive
  definite whatever the rotation"""
  w, V = np.linalg.eigh(li.inertia)
  R = _rotation(axis, angle)
  I = R @ (V @ np.diag(w * np.asarray(scale)) @ V.T) @ R.T
  li.inertia = 0.5 * (I + I.T)


def _random_axis(rng):
  """a unit axis with every component at least 0.3 in magnitude: the rotation mixes all three pairs of axes"""
  a = rng.uniform(0.3, 1.0, 3) * rng.choice([-1.0, 1.0], 3)
  return a / np.linalg.norm(a)


def random_model(seed):
  """Every table of the model at a random point, the four legs drawn independently (no mirroring): masses x U(0.7, 1.4); link
  CoMs and hip / knee origins +-1 cm in all three components (the base CoM stays 0, as validate_model demands); every inertia
  tensor - the base's included - rotated by about 0.3 rad about a generic axis with its principal values x U(0.7, 1.4), so all
  six components are non-zero; sphere centres +-5 mm, radii x U(0.8, 1.2); sphere 4l of one leg moved to the UPPER link;
  per-joint limits (-U(2, 10), +U(2, 10))."""
  rng = np.random.default_rng(1000 + seed)
  m = TableModel()
  for k, body in enumerate(m.bodies()):
    body.mass *= rng.uniform(0.7, 1.4)
    if k > 0:
      body.com = body.com + rng.uniform(-0.01, 0.01, 3)
    _tilt(body, _random_axis(rng), rng.uniform(0.25, 0.35), rng.uniform(0.7, 1.4, 3))
  for leg in range(abi.NUM_LEGS):
    m.hips[leg] = m.hips[leg] + rng.uniform(-0.01, 0.01, 3)
    m.knees[leg] = m.knees[leg] + rng.uniform(-0.01, 0.01, 3)
  up = int(rng.integers(abi.NUM_LEGS))
  for s, (body, centre, radius) in enumerate(m._spheres):
    if s == 4 * up:   # the knee sphere of one leg rides on the upper link, at the knee joint's origin
      body, centre = 1 + 2 * up, m.knees[up].copy()
    m._spheres[s] = (body, centre + rng.uniform(-0.005, 0.005, 3), radius * rng.uniform(0.8, 1.2))
  m.limits = [(-rng.uniform(2.0, 10.0), rng.uniform(2.0, 10.0)) for _ in range(abi.NUM_DOF)]
  return m


def edge_model(name):
  """The default model with ONE thing changed (see EDGE_MODELS)."""
  m = TableModel()
  if name == 'offdiag_base':        # only the base has Ixy, Ixz, Iyz != 0
    _tilt(m.base(), (0.5, -0.6, 0.62), 0.3)
  elif name == 'offdiag_legs':      # only the links have them, every link its own axis
    rng = np.random.default_rng(3)
    for body in m.bodies()[1:]:
      _tilt(body, _random_axis(rng), 0.3)
  elif name == 'knee_x':            # knee origin x and link CoM x at +-1 cm (both are 0 / 1e-5 in the default model)
    for leg in range(abi.NUM_LEGS):
      s = 1.0 if leg in (0, 3) else -1.0
      m.knees[leg][0] = 0.01 * s
      m.uppers[leg].com[0] = -0.01 * s
      m.lowers[leg].com[0] = 0.01 * s
  elif name == 'asymmetric':        # one leg 1.4 x heavier and 1 cm longer than the others
    leg = 2
    for body in (m.uppers[leg], m.lowers[leg]):
      body.mass *= 1.4
      body.inertia = body.inertia * 1.4
    m.knees[leg][2] -= 0.01
  elif name == 'upper_spheres':
    # sphere 4l of every leg on the UPPER link, 1 cm above its lower end (the knee joint) and 8 mm off the link's axis, on the
    # side that faces the ground in the folded settle pose (HFE = +pi/2 in front turns the link's +x down, -pi/2 behind its
    # -x): the folded leg lies at the hip's height, 0.026 m, and the default knee sphere (radius 0.0195 m) on the axis stays
    # 6.5 mm above the ground there - 8 mm off the axis the sphere carries the leg
    for leg in range(abi.NUM_LEGS):
      _, _, radius = m._spheres[4 * leg]
      m._spheres[4 * leg] = (1 + 2 * leg, m.knees[leg] + np.array([0.008 if leg < 2 else -0.008, 0.0, 0.01]), radius)
  elif name == 'tight_limits':      # KFE limits +-2.5 rad: the settle pose's +-pi knee targets push into them
    for leg in range(abi.NUM_LEGS):
      m.limits[2 * leg + 1] = (-2.5, 2.5)
  else:
    raise KeyError(name)
  return m


def get_model(case):
  """'default' | 'seed<k>' | the name of an edge model -> model"""
  if case == 'default':
    return Solo8Model()
  if case.startswith('seed'):
    return random_model(int(case[4:]))
  return edge_model(case)


ALL_CASES = tuple('seed%d' % s for s in RANDOM_SEEDS) + EDGE_MODELS   # the random seeds, then the edge models


# ---- models validate_model must reject: one mutation of the C-ABI struct per clause ---------------------------------------
def _hfe_parent(ma): ma.parent[4] = 3
def _kfe_parent(ma): ma.parent[3] = 0
def _joint_axis(ma): ma.joint_axis[5][1], ma.joint_axis[5][0] = 0.0, 1.0
def _base_com(ma): ma.com[0][2] = 1e-3
def _num_spheres(ma): ma.num_spheres = 12
def _limits(ma): ma.joint_lower[6] = ma.joint_upper[6]
def _leg_sphere_on_another_leg(ma): ma.sphere_body[5] = 2          # the foot sphere of leg 1 on the lower link of leg 0
def _base_sphere_on_a_leg(ma): ma.sphere_body[10] = 6              # a base-box corner of leg 2 on that leg's lower link


def invalid_models():
  """[(mutation of an abi.SoloModel, fragment of validate_model's message)], one per clause"""
  return [(_hfe_parent, 'HFE link must hang off the base'),
          (_kfe_parent, 'KFE link must hang off its HFE link'),
          (_joint_axis, '+y joint axes'),
          (_base_com, 'base CoM frame'),
          (_num_spheres, 'expected 16 collision spheres'),
          (_limits, 'lower < upper'),
          (_leg_sphere_on_another_leg, 'must be attached to leg l'),
          (_base_sphere_on_a_leg, 'must be attached to the base')]


# ---- the conditions that keep a parity test from passing vacuously (on the oracle's trajectory) --------------------------
class Liveness:
  """Accumulates, over the (robot, step) pairs it is shown, what the ORACLE's step has live: call see() with the state BEFORE
  the step and the step's actions."""

  def __init__(self, ph, ma, ca):
    self.ph, self.ma, self.ca = ph, ma, ca
    self.pairs = self.rich = self.upper = self.limit_and_contact = 0
    self.rows = []
    self.upper_spheres = [s for s in range(abi.MAX_SPHERES) if ma.sphere_body[s] != 0 and ma.sphere_body[s] % 2 == 1]
    self.lower = np.array(list(ma.joint_lower))
    self.high = np.array(list(ma.joint_upper))

  def see(self, st, actions, params=None, every=1):
    """every: look at every k-th robot only"""
    scaled = np.asarray(actions, dtype=np.float64) * self.ca.action_scale
    for e in range(0, st.shape[0], every):
      dbg = self.ph.step_debug(st[e].copy(), scaled[e][DOF_TO_JOINT].copy(), None if params is None else params[e].copy())
      touching = set(np.ctypeslib.as_array(dbg.row_sphere)[:dbg.num_rows].tolist()) - {-1}
      q = st[e, abi.S_Q:abi.S_Q + abi.NUM_DOF]
      near = bool((np.minimum(q - self.lower, self.high - q) < self.ca.joint_limit_margin).any())
      self.pairs += 1
      self.rich += len(touching) >= 3
      self.upper += any(s in touching for s in self.upper_spheres)
      self.limit_and_contact += near and len(touching) >= 1
      self.rows.append(dbg.num_rows)

  def check(self, case):
    """the issue's section 5: >= 75 % of the pairs with three or more touching spheres; on upper_spheres an upper-link sphere
    touching in >= 10 %; on tight_limits a joint inside the limit margin while a sphere touches in >= 10 %"""
    assert self.pairs > 0
    assert self.rich >= 0.75 * self.pairs, (case, self.rich, self.pairs)
    if case == 'upper_spheres':
      assert self.upper >= 0.10 * self.pairs, (case, self.upper, self.pairs)
    if case == 'tight_limits':
      assert self.limit_and_contact >= 0.10 * self.pairs, (case, self.limit_and_contact, self.pairs)

  def __str__(self):
    return '{} robot-steps: {} with >= 3 touching spheres, {} with an upper-link sphere touching, {} at a limit in contact, rows {}..{}'.format(
      self.pairs, self.rich, self.upper, self.limit_and_contact, min(self.rows), max(self.rows))


def upper_sphere_touches(ph, ma, ca, st):
  """does a sphere that rides on an UPPER link sit within the contact margin of the flat ground in state st [32]?"""
  z = ph.sphere_centers(np.ascontiguousarray(st).copy())[:, 2] - np.array(list(ma.sphere_radius))
  return any(z[s] < ca.contact_margin for s in range(abi.MAX_SPHERES) if ma.sphere_body[s] != 0 and ma.sphere_body[s] % 2 == 1)
