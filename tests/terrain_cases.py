"""The heightfield ground (include/solo_engine.h, SoloTerrain) pinned to its DOCUMENTED contract, shared by the CPU oracle
(tests/test_oracle_physics.py), the product kernel source on the emulator (tests/test_emu_kernel.py) and the HIP engine
(tests/test_gpu_terrain.py) in the way closed_form_cases.py is shared.

What the header says: inside the grid rectangle the ground is the bilinear interpolant of the cell's four heights; outside it
is h(x, y) with x and y each clamped to the rectangle, so it has no slope along a clamped axis; a sphere collides with the
tangent plane of that surface under its centre.  Two independent statements of it live here, neither derived from the oracle's
`ground_at`, the kernel's heightfield branch or `contact_cases.gaps`:

  * `saddle_truth`: a surface h = a + b x + c y + e x y sampled on ANY grid is reproduced exactly by bilinear interpolation, so
    inside the grid the truth is h(x, y) and grad h = (b + e y, c + e x) - no cell index, no stride, no origin arithmetic.
  * `ground_reference`: the words of the header in numpy longdouble, for grids without a closed form (the random grid).

The PROBE generalises closed_form_cases.belly_corner_penetrating / contact_point_velocity to any ground and any (x, y): a robot
at rest (gravity 0), legs straight up, the base rolled and pitched by 0.12 ... 0.3 rad RELATIVE TO THE LOCAL TANGENT PLANE so that
one bottom corner sphere of the base is the lowest point, its centre over the probe point and its tangent-plane distance
(z - h) n_z - r = -d (d = 0.05 ... 2 mm).  After one step the body-fixed point centre - r n moves at (contact_erp d / dt) n and has no
tangential velocity: the direction gives both slope components, the magnitude gives d and so the height.  One robot per probe,
256 robots per batch, every robot at its own (x, y)."""
import numpy as np

from gym_solo_amd import abi
from gym_solo_amd.model import Solo8Model
from closed_form_cases import VEL, rot

LD = np.longdouble
BATCH = 256

# The bars.  f64: the project's push-out bar (closed_form_cases: 1e-11 m/s on every velocity component of the contact point).
# f32, measured then fixed (the reference evaluated at the f32-ROUNDED state and the f32-rounded heights, so that only the
# kernel's own arithmetic counts): the emulated f32 kernel's worst error over the probes is 5.2e-5 (saddle 7x19), 3.8e-5
# (saddle 33x5), 9.0e-5 (saddle 2x2), 1.0e-4 (saddle 2x9), 7.8e-6 m/s (random 11x6); the worst, 1.0e-4, x 4 = 4e-4 m/s.  What it
# is made of: the bias is contact_erp dist / dt = 200 / s x dist, and dist comes out of a cancellation of world coordinates of
# up to 5 m (ulp 2.4e-7 ... 4.8e-7 m) taken through slopes of up to 0.4 and of heights of up to 1.5 m (ulp 1.2e-7 m):
# a few 1e-7 m x 200 / s.  (The random grid's heights are centimetres: its error is ten times smaller.)
BARS = {'float64': 1e-11, 'float32': 4e-4}
# the recorded contact force of the probed sphere (contact sensing on): contact_cases.BARS' force bars
FORCE_BARS = {'float64': 1e-6, 'float32': 0.5}


# ---- the two statements of the ground --------------------------------------------------------------------------------------------
def heights_of(terrain):
  return np.ctypeslib.as_array(terrain.heights, shape=(terrain.ny * terrain.nx,)).reshape(terrain.ny, terrain.nx)


def _rectangle(terrain):
  ox, oy, c = LD(terrain.origin[0]), LD(terrain.origin[1]), LD(terrain.cell)
  return ox, ox + (terrain.nx - 1) * c, oy, oy + (terrain.ny - 1) * c


def _normal(hx, hy):
  n = np.array([-hx, -hy, LD(1)], dtype=LD)
  return n / np.sqrt(hx * hx + hy * hy + LD(1))


def ground_reference(terrain, x, y, cell=None, clamped=None, heights=None):
  """(h, n) of the ground under the world point (x, y), from the words of the header, in longdouble: clamp the point to the
  grid rectangle, find the cell, interpolate bilinearly, take the gradient with zero slope along a clamped axis.
  cell = (i, j): use THAT cell's bilinear patch (a point on a grid line belongs to both neighbours); clamped = (bool, bool):
  decide by hand which axes count as clamped (a point on the border, to rounding); heights: another [ny, nx] array (the
  f32-rounded grid an f32 engine holds)."""
  H = heights_of(terrain) if heights is None else heights
  x0, x1, y0, y1 = _rectangle(terrain)
  c = LD(terrain.cell)
  x, y = LD(x), LD(y)
  xc, yc = min(max(x, x0), x1), min(max(y, y0), y1)
  if clamped is None:
    clamped = (xc != x, yc != y)
  u, v = (xc - x0) / c, (yc - y0) / c
  if cell is None:
    cell = (min(int(np.floor(u)), terrain.nx - 2), min(int(np.floor(v)), terrain.ny - 2))
  i, j = cell
  fu, fv = u - i, v - j
  h00, h10, h01, h11 = LD(H[j, i]), LD(H[j, i + 1]), LD(H[j + 1, i]), LD(H[j + 1, i + 1])
  h = (1 - fu) * (1 - fv) * h00 + fu * (1 - fv) * h10 + (1 - fu) * fv * h01 + fu * fv * h11
  hx = LD(0) if clamped[0] else ((1 - fv) * (h10 - h00) + fv * (h11 - h01)) / c
  hy = LD(0) if clamped[1] else ((1 - fu) * (h01 - h00) + fu * (h11 - h10)) / c
  return h, _normal(hx, hy)


def saddle_truth(coef, terrain, x, y, clamped=None):
  """(h, n) of h = a + b x + c y + e x y continued outside the grid rectangle as the header says - no cell, no index"""
  a, b, c, e = (LD(t) for t in coef)
  x0, x1, y0, y1 = _rectangle(terrain)
  x, y = LD(x), LD(y)
  xc, yc = min(max(x, x0), x1), min(max(y, y0), y1)
  if clamped is None:
    clamped = (xc != x, yc != y)
  h = a + b * xc + c * yc + e * xc * yc
  return h, _normal(LD(0) if clamped[0] else b + e * yc, LD(0) if clamped[1] else c + e * xc)


# ---- the grids -----------------------------------------------------------------------------------------------------------------
class Grid:
  def __init__(self, name, nx, ny, cell, origin, coef=None, heights=None, dyadic=False):
    self.name, self.coef, self.dyadic = name, coef, dyadic
    if coef is not None:
      xs, ys = origin[0] + cell * np.arange(nx), origin[1] + cell * np.arange(ny)
      a, b, c, e = coef
      heights = a + b * xs[None, :] + c * ys[:, None] + e * xs[None, :] * ys[:, None]
    self.terrain = abi.make_terrain(heights, cell, origin)

  def truth(self, x, y, cell=None, clamped=None, f32=False):
    if self.coef is not None and cell is None:
      return saddle_truth(self.coef, self.terrain, x, y, clamped)
    H = heights_of(self.terrain)
    return ground_reference(self.terrain, x, y, cell, clamped, H.astype(np.float32).astype(np.float64) if f32 else None)


def _random_heights(nx=11, ny=6, cell=0.07, seed=17, steepest=0.5):
  h = np.random.default_rng(seed).standard_normal((ny, nx))
  slope = max(np.abs(np.diff(h, axis=0)).max(), np.abs(np.diff(h, axis=1)).max()) / cell
  return h * (steepest / slope) * (1 - 1e-12)


_GRIDS = {}


def grid(name):
  """The grids, all small: analytic saddles (b, c, e != 0, slopes <= 0.4 over the rectangle) and one random grid (steepest cell
  slope <= 0.5).  saddle_2x2 and saddle_2x9 have dyadic cells, origins and coefficients: their heights and borders are EXACT in
  binary, and their borders lie well inside the binade [2, 4), where a sphere centre can be put on them exactly (_lands_exactly)."""
  if name not in _GRIDS:
    _GRIDS[name] = {
      'saddle_7x19': lambda: Grid(name, 7, 19, 0.13, (-0.31, 2.4), coef=(0.05, 0.6, -0.33, -0.11)),     # the world origin lies outside
      'saddle_33x5': lambda: Grid(name, 33, 5, 0.02, (-5.0, -0.04), coef=(1.2, 0.3, 1.4, 0.25)),
      'saddle_2x2': lambda: Grid(name, 2, 2, 0.5, (2.5, -3.5), coef=(0.25, -0.75, 0.5, -0.125), dyadic=True),     # a single cell
      'saddle_2x9': lambda: Grid(name, 2, 9, 0.125, (-3.25, 2.5), coef=(-0.5, 0.625, -0.625, -0.125), dyadic=True),
      'random_11x6': lambda: Grid(name, 11, 6, 0.07, (0.4, -1.3), heights=_random_heights()),
    }[name]()
  return _GRIDS[name]


GRID_NAMES = ('saddle_7x19', 'saddle_33x5', 'saddle_2x2', 'saddle_2x9', 'random_11x6')


def steepest_slope(g):
  """the largest |dh/dx|, |dh/dy| over the rectangle (a saddle's are linear in the other coordinate: at the corners)"""
  if g.coef is None:
    H, c = heights_of(g.terrain), g.terrain.cell
    return max(np.abs(np.diff(H, axis=0)).max(), np.abs(np.diff(H, axis=1)).max()) / c
  x0, x1, y0, y1 = (float(t) for t in _rectangle(g.terrain))
  _, b, c, e = g.coef
  return max(max(abs(b + e * y) for y in (y0, y1)), max(abs(c + e * x) for x in (x0, x1)))


# ---- the probe points ----------------------------------------------------------------------------------------------------------
class Probe:
  """kind: 'inside' | 'border' (exactly on it: the cell's slope) | 'border~' (on it to rounding: the cell's slope or the clamped
  one) | 'outside' | 'line' (on interior grid lines: any adjacent cell) | 'far' (+-1e12 m)"""
  def __init__(self, kind, x, y, uv=None):
    self.kind, self.x, self.y, self.uv = kind, float(x), float(y), uv


def probe_points(g, seed=0, far=False):
  t = g.terrain
  nx, ny, c, ox, oy = t.nx, t.ny, t.cell, t.origin[0], t.origin[1]
  rng = np.random.default_rng([seed, nx, ny])
  def inner(n):   # a coordinate in cells, at least 1e-6 cell away from any grid line
    while True:
      u = rng.uniform(0, n - 1)
      if abs(u - round(u)) > 1e-6:
        return u
  X, Y = (lambda u: ox + u * c), (lambda v: oy + v * c)
  if far:   # +-1e12 m on one axis (the conversion clamp), the other axis inside and outside
    out = []
    for big in (-1e12, 1e12):
      for w in (inner(nx), -3.3, nx + 1.7):
        out.append(Probe('far', X(w), big))
      for w in (inner(ny), -2.6, ny + 0.9):
        out.append(Probe('far', big, Y(w)))
    return out
  out = []
  # one point in each of the four corner cells (cell indices 0 and nx - 2 / ny - 2)
  for iu in (0, nx - 2):
    for jv in (0, ny - 2):
      out.append(Probe('inside', X(iu + rng.uniform(0.05, 0.95)), Y(jv + rng.uniform(0.05, 0.95))))
  # exactly on the border: the four edges and the four corners
  bk = 'border' if g.dyadic else 'border~'
  for u in (0, nx - 1):
    out.append(Probe(bk, X(u), Y(inner(ny)), (u, None)))
  for v in (0, ny - 1):
    out.append(Probe(bk, X(inner(nx)), Y(v), (None, v)))
  for u in (0, nx - 1):
    for v in (0, ny - 1):
      out.append(Probe(bk, X(u), Y(v), (u, v)))
  # outside on all eight sides, 0.3 cell, 10 cells and 1000 m away
  for dist in (0.3 * c, 10 * c, 1000.0):
    for sx in (-1, 0, 1):
      for sy in (-1, 0, 1):
        if sx == 0 and sy == 0:
          continue
        x = X(inner(nx)) if sx == 0 else (ox - dist if sx < 0 else X(nx - 1) + dist)
        y = Y(inner(ny)) if sy == 0 else (oy - dist if sy < 0 else Y(ny - 1) + dist)
        out.append(Probe('outside', x, y))
  # exactly on interior grid lines (x, y, and a grid point)
  for rep in range(3):
    if nx > 2:
      u = int(rng.integers(1, nx - 1))
      out.append(Probe('line', X(u), Y(inner(ny)), (u, None)))
    if ny > 2:
      v = int(rng.integers(1, ny - 1))
      out.append(Probe('line', X(inner(nx)), Y(v), (None, v)))
    if nx > 2 and ny > 2:
      out.append(Probe('line', X(int(rng.integers(1, nx - 1))), Y(int(rng.integers(1, ny - 1))), (-1, -1)))
  for p in out:
    if p.kind == 'line':   # (the grid line(s) the point lies on, from the point itself)
      u, v = round((p.x - ox) / c), round((p.y - oy) / c)
      p.uv = (u if p.uv[0] is not None else None, v if p.uv[1] is not None else None)
  while len(out) < BATCH:
    out.append(Probe('inside', X(inner(nx)), Y(inner(ny))))
  return out


def _another(g, p, rng):
  """a fresh probe of p's kind: inside, or on interior grid lines along the same axes"""
  t = g.terrain
  def inner(n):
    while True:
      u = rng.uniform(0, n - 1)
      if abs(u - round(u)) > 1e-6:
        return u
  if p.kind == 'inside':
    return Probe('inside', t.origin[0] + inner(t.nx) * t.cell, t.origin[1] + inner(t.ny) * t.cell)
  u = int(rng.integers(1, t.nx - 1)) if p.uv[0] is not None else None
  v = int(rng.integers(1, t.ny - 1)) if p.uv[1] is not None else None
  return Probe('line', t.origin[0] + (inner(t.nx) if u is None else u) * t.cell, t.origin[1] + (inner(t.ny) if v is None else v) * t.cell, (u, v))


def truths(g, p, x, y, f32=False):
  """the legitimate (h, n) of the ground under probe p, evaluated at (x, y): one, or - where rounding decides - several"""
  t = g.terrain
  if p.kind == 'line':
    # the kernel multiplies by 1 / cell and the oracle divides (0.15 / 0.05 = 2.9999999999999996, 0.15 * 20 = 3.0): the point is
    # in either cell next to the line (four next to a grid point); the height is the same, the normal is not
    u, v = p.uv
    ci = [u - 1, u] if u is not None else [None]
    cj = [v - 1, v] if v is not None else [None]
    i0 = min(int(np.floor((LD(x) - LD(t.origin[0])) / LD(t.cell))), t.nx - 2)
    j0 = min(int(np.floor((LD(y) - LD(t.origin[1])) / LD(t.cell))), t.ny - 2)
    return [g.truth(x, y, cell=(i0 if i is None else i, j0 if j is None else j), clamped=(False, False), f32=f32) for i in ci for j in cj]
  if p.kind == 'border~':
    u, v = p.uv
    return [g.truth(x, y, clamped=(cx, cy), f32=f32) for cx in ((False, True) if u is not None else (False,)) for cy in ((False, True) if v is not None else (False,))]
  if p.kind == 'border':
    return [g.truth(x, y, clamped=(False, False), f32=f32)]
  return [g.truth(x, y, f32=f32)]


# ---- the probe pose ------------------------------------------------------------------------------------------------------------
def _qmul(a, b):
  ax, ay, az, aw = a
  bx, by, bz, bw = b
  return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                   aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def _tilt_to(n):
  """the smallest rotation that takes world z to n, as a quaternion"""
  n = np.asarray(n, dtype=np.float64)
  axis = np.array([-n[1], n[0], 0.0])
  s = np.linalg.norm(axis)
  if s < 1e-300:
    return np.array([0.0, 0.0, 0.0, 1.0])
  ang = np.arctan2(s, n[2])
  return np.concatenate([axis / s * np.sin(ang / 2), [np.cos(ang / 2)]])


def _centre_ld(st, centre):
  """world centre of a base sphere from a state record, in longdouble (the rotation matrix of closed_form_cases.rot)"""
  R = rot(st[abi.S_QUAT:abi.S_QUAT + 4].astype(LD))
  return st[abi.S_POS:abi.S_POS + 3].astype(LD) + R @ centre.astype(LD)


def _lands_exactly(st, centre, axis, target, f32):
  """Exactly ON the border: the centre coordinate the step computes, pos + R[axis] . c in ITS precision, must BE the border
  coordinate whatever the order of its additions and whether or not products are fused.  Border, position and every partial
  sum lie in one binade ([2, 4)), so each addition rounds to that binade's grid of 1 ulp: the result is pos + (the terms
  rounded to the grid, in some grouping).  Accepted: every grouping gives the border, and no term or partial sum is within
  0.2 ulp of a rounding tie (the roundings of the matrix entries and products are worth < 0.1 ulp there)."""
  T = np.float32 if f32 else np.float64
  R = rot(st[abi.S_QUAT:abi.S_QUAT + 4].astype(T))
  a, b, c = (LD(R[axis, k]) * LD(T(centre[k])) for k in range(3))
  ulp = LD(np.spacing(T(abs(float(target)))))
  want = (LD(target) - LD(st[abi.S_POS + axis])) / ulp
  if want != np.rint(want):
    return False
  sums = [t / ulp for t in (a, b, c, a + b, b + c, a + c, a + b + c)]
  if any(abs(abs(t - np.floor(t) - LD(0.5))) < 0.2 for t in sums):
    return False
  G = np.rint
  a, b, c, ab, bc, ac, abc = sums
  return all(t == want for t in (G(a) + G(b) + G(c), G(ab) + G(c), G(a) + G(bc), G(ac) + G(b), G(abc)))


class ProbeBatch:
  pass


def make_batch(g, dtype='float64', far=False, seed=0, margin=0.005):
  """256 probes of grid g as one batch (or the +-1e12 m probes, a batch of their own).  f32: probes farther than 4 m OUTSIDE the
  grid (1000 m, 1e12 m) are left out - f32 resolves 1e-4 m there - and the batch is topped up with inside points; the states are
  rounded to f32 (the engine would), and every expectation is evaluated at the rounded state."""
  model = Solo8Model()
  f32 = dtype == 'float32'
  rnd = (lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)) if f32 else (lambda a: np.asarray(a, dtype=np.float64))
  rng = np.random.default_rng([seed, 99, int(far)])
  sph = model.spheres()
  base = [(k, c, r) for k, (b, c, r) in enumerate(sph) if b == 0]
  radius = model.base_sphere_radius
  pts = probe_points(g, seed, far)
  if f32:
    x0, x1, y0, y1 = (float(t) for t in _rectangle(g.terrain))
    near = [p for p in pts if max(x0 - p.x, p.x - x1, y0 - p.y, p.y - y1) <= 4.0]
    extra = [p for p in probe_points(g, seed + 1) if p.kind == 'inside']
    pts = (near + extra)[:BATCH] if not far else []
  n = len(pts)
  B = ProbeBatch()
  B.grid, B.dtype, B.probes, B.radius = g, dtype, pts, radius
  B.states = np.zeros((n, abi.STATE_STRIDE))
  B.centres, B.sphere, B.depth = np.zeros((n, 3)), np.zeros(n, dtype=int), np.zeros(n)
  B.acts = np.zeros((n, abi.NUM_JOINTS))
  for leg in range(4):
    B.acts[:, 3 * leg] = np.pi
  for e in range(n):
   for redraw in range(60):
    p = pts[e]
    h, nrm = truths(g, p, p.x, p.y, f32)[0]
    nrm64 = nrm.astype(np.float64)
    for attempt in range(40000 if p.kind == 'border' else 400):
      d = rng.uniform(5e-5, 2e-3)
      roll, pitch = rng.uniform(0.12, 0.3, 2) * np.where(rng.random(2) < 0.5, -1.0, 1.0)
      cr, sr, cp, sp = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2)
      ql = np.array([sr * cp, cr * sp, -sr * sp, cr * cp])
      if attempt >= 100:   # rough ground: also turn the base about the local normal, until the rest of it clears the bumps
        yaw = rng.uniform(-np.pi, np.pi)
        ql = _qmul(np.array([0.0, 0.0, np.sin(yaw / 2), np.cos(yaw / 2)]), ql)
      zs = [(rot(ql) @ c)[2] - r for _, c, r in base]
      low = int(np.argmin(zs))
      k, centre, _ = base[low]
      q = rnd(_qmul(_tilt_to(nrm64), ql))
      arm = rot(q.astype(LD)) @ centre.astype(LD)
      cw = np.array([LD(p.x), LD(p.y), h + (LD(radius) - LD(d)) / nrm[2]])
      st = np.zeros(abi.STATE_STRIDE)
      st[abi.S_QUAT:abi.S_QUAT + 4] = q
      st[abi.S_POS:abi.S_POS + 3] = rnd((cw - arm).astype(np.float64))
      st[abi.S_Q:abi.S_Q + 8] = rnd(np.tile([np.pi, 0.0], 4))
      if p.kind == 'border' and not all(w is None or _lands_exactly(st, centre, a, cw[a], f32) for a, w in enumerate(p.uv)):
        continue
      # every other sphere is farther than the contact margin from its own tangent plane (reference and numpy only)
      ok = True
      for kk, (b, c, r) in enumerate(sph):
        if kk == k:
          continue
        if b == 0:
          w = _centre_ld(st, c)
        else:   # legs straight up: the leg spheres sit ABOVE the base; a bound is enough: the base origin's height minus the reach
          continue
        hh, nn = g.truth(w[0], w[1], f32=f32)
        if (w[2] - hh) * nn[2] - r < 2 * margin:
          ok = False
          break
      if ok:
        break
    else:
      # no base fits there (the bottom of a V between two bumps of the random grid): another point of the same kind
      if p.kind not in ('inside', 'line') or redraw == 59:
        raise RuntimeError('no pose for probe %d of %s (%s at %g, %g)' % (e, g.name, p.kind, p.x, p.y))
      pts[e] = _another(g, p, rng)
      continue
    B.states[e], B.centres[e], B.sphere[e], B.depth[e] = st, centre, k, d
    break
  return B


def leg_spheres_clear(ph, B, margin):
  """the leg spheres too (through the oracle's KINEMATICS, a measuring device): every sphere but the probed one is farther than
  the contact margin from its own tangent plane"""
  sph = Solo8Model().spheres()
  for e in range(len(B.probes)):
    c = ph.sphere_centers(B.states[e].copy())
    for k, (b, _, r) in enumerate(sph):
      if k == B.sphere[e]:
        continue
      hh, nn = B.grid.truth(c[k, 0], c[k, 1])
      if not (c[k, 2] - float(hh)) * float(nn[2]) - r > margin:
        return False
  return True


def check(B, post, erp, dt):
  """per probe: the largest component of (velocity of the body-fixed contact point after the step) - (erp d / dt) n, against the
  best of the probe's legitimate grounds; d is re-derived from the state the step started from.  Returns errors [n]."""
  f32 = B.dtype == 'float32'
  err = np.zeros(len(B.probes))
  B.normal = np.zeros((len(B.probes), 3))   # per probe: the normal of the ground that fitted best ...
  B.inside = np.zeros(len(B.probes))        # ... and how deep the sphere is inside THAT tangent plane (0: it does not penetrate it)
  for e, p in enumerate(B.probes):
    st = B.states[e]
    cw = _centre_ld(st, B.centres[e])
    exact_xy = not f32 or p.kind == 'border'    # (f32: the ground under the ROUNDED state's centre; on the border it is the border)
    x, y = (LD(p.x), LD(p.y)) if exact_xy else (cw[0], cw[1])
    R = rot(st[abi.S_QUAT:abi.S_QUAT + 4])
    best = np.inf
    for h, n in truths(B.grid, p, x, y, f32):
      dist = (cw[2] - h) * n[2] - LD(B.radius)
      n64 = n.astype(np.float64)
      want = n64 * (erp * max(0.0, -float(dist)) / dt)
      arm = R @ B.centres[e] - B.radius * n64
      got = post[e][VEL[1]] + np.cross(post[e][VEL[0]], arm)
      this = float(np.abs(got - want).max())
      if this < best:
        best, B.normal[e], B.inside[e] = this, n64, max(0.0, -float(dist))
    err[e] = best
  return err


def summary(B, err):
  kinds = sorted(set(p.kind for p in B.probes))
  return '%s %s: %d probes, worst %.2e m/s (%s)' % (B.grid.name, B.dtype, len(err), err.max() if len(err) else 0.0, ', '.join(
    '%s %.1e' % (k, max(err[i] for i, p in enumerate(B.probes) if p.kind == k)) for k in kinds))


_BATCHES = {}


def batch(name, dtype='float64', far=False):
  """make_batch, built once per (grid, precision) and shared by the oracle, emulator and GPU tests (read-only)"""
  key = (name, dtype, far)
  if key not in _BATCHES:
    _BATCHES[key] = make_batch(grid(name), dtype, far)
  return _BATCHES[key]


# ---- dynamic cases -------------------------------------------------------------------------------------------------------------
def scattered(g, ph, pose, n, seed=0, beyond=3.0, clearance=2e-3):
  """n copies of the state `pose` (a settle snapshot), each at its own (x, y): scattered over the grid and up to `beyond` cells
  across all four borders, at the height at which its lowest sphere is `clearance` above its own tangent plane (the reference
  and the oracle's kinematics only) - dropped from the settle pose."""
  t = g.terrain
  rng = np.random.default_rng([seed, 7, t.nx])
  radii = [r for _, _, r in Solo8Model().spheres()]
  st = np.tile(pose, (n, 1))
  for e in range(n):
    st[e, abi.S_POS] = t.origin[0] + rng.uniform(-beyond, t.nx - 1 + beyond) * t.cell
    st[e, abi.S_POS + 1] = t.origin[1] + rng.uniform(-beyond, t.ny - 1 + beyond) * t.cell
    st[e, abi.S_POS + 2] = 0.0
    c = ph.sphere_centers(st[e].copy())
    lift = -np.inf
    for k, r in enumerate(radii):
      h, nn = g.truth(c[k, 0], c[k, 1])
      lift = max(lift, float(h + (r + clearance) / nn[2]) - c[k, 2])
    st[e, abi.S_POS + 2] = lift
  return st


def ambiguous(g, centres, eps=1e-9):
  """a sphere centre within eps cell of a grid line (border lines included): 1 / cell against a division may put it in either
  cell, so kernel and oracle may legitimately disagree from this step on"""
  t = g.terrain
  for a, n in ((0, t.nx), (1, t.ny)):
    u = (centres[:, a] - t.origin[a]) / t.cell
    k = np.rint(u)
    if np.any((np.abs(u - k) < eps) & (k >= 0) & (k <= n - 1)):
      return True
  return False


def oracle_trajectory(g, ph, st0, acts):
  """the oracle's trajectory from st0 under acts [K, N, 12] and, per robot, the first step at which a sphere centre is ambiguous
  (K: never) - robot-steps from that step on are skipped"""
  st = st0.copy()
  n = st.shape[0]
  first = np.full(n, len(acts))
  for k, a in enumerate(acts):
    for e in range(n):
      if first[e] == len(acts) and ambiguous(g, ph.sphere_centers(st[e].copy())):
        first[e] = k
    ph.step(st, a, threads=4)
  return st, first


def shelf_states(ph_flat, n, seed=0):
  """settled robots beyond the +x edge of helpers.incline_terrain() (the grid ends at x = 1.575 m), at several y inside and
  outside the grid: on the level shelf h = tan(10 deg) x 1.575.  Returns (states on the flat plane z = 0, the same raised by the
  shelf, the actions that hold the settle pose: under them the robots are AT REST)."""
  rng = np.random.default_rng([seed, 31])
  st = np.tile(ph_flat.settle(1), (n, 1))
  st[:, abi.S_POS] = rng.uniform(2.5, 5.0, n)
  st[:, abi.S_POS + 1] = rng.uniform(-2.5, 2.5, n)
  up = st.copy()
  up[:, abi.S_POS + 2] += shelf_height()
  hold = np.tile(np.array(list(ph_flat.cfg.settle_targets)), (n, 1)) / ph_flat.cfg.action_scale
  return st, up, hold


def momentum_gain(ph, pre, post):
  """per robot, the horizontal linear momentum a step added (the oracle's `momentum` helper: kinematics, a measuring device)"""
  return np.array([ph.momentum(post[i].copy())[0][:2] - ph.momentum(pre[i].copy())[0][:2] for i in range(pre.shape[0])])


def shelf_case(step_flat, step_shelf, ph, n, seed=0):
  """The shelf is a flat plane.  step_flat / step_shelf(state [n, 32], actions) -> the state after one step on the flat plane / on
  the incline heightfield.  Returns (worst |state difference| after 40 random-action steps with the shelf state lowered by the
  border height, worst horizontal momentum gained per step by robots AT REST holding the settle pose, worst difference per step
  between the shelf's and the flat plane's horizontal momentum gain under ZERO actions - the folded robots stand up, and their
  feet push them about on either ground alike)."""
  from helpers import random_actions
  a, b, hold = shelf_states(ph, n, seed)
  rest, moving_flat, moving = b.copy(), a.copy(), b.copy()
  rng = np.random.default_rng([seed, 5])
  for k in range(40):
    act = random_actions(rng, n)
    a, b = step_flat(a, act), step_shelf(b, act)
  b[:, abi.S_POS + 2] -= shelf_height()
  gain = rel = 0.0
  zero = np.zeros((n, abi.NUM_JOINTS))
  for k in range(40):
    post = step_shelf(rest, hold)
    gain = max(gain, float(np.abs(momentum_gain(ph, rest, post)).max()))
    rest = post
    pf, ps = step_flat(moving_flat, zero), step_shelf(moving, zero)
    rel = max(rel, float(np.abs(momentum_gain(ph, moving, ps) - momentum_gain(ph, moving_flat, pf)).max()))
    moving_flat, moving = pf, ps
  return float(np.abs(a[:, :29] - b[:, :29]).max()), gain, rel


def shelf_height():
  """the border height of helpers.incline_terrain(): its last grid value"""
  from helpers import incline_terrain
  return float(heights_of(incline_terrain())[0, -1])


_SETTLED = {}


def settled_on(name):
  """(ca, ma, oracle on the grid, the oracle's settle snapshot [32] on it) - settled where every engine settles, at the world
  origin: OUTSIDE saddle_7x19 and random_11x6"""
  if name not in _SETTLED:
    from helpers import make_abi
    from oracle import solo_oracle as so
    ca, ma = make_abi('float64')
    ph = so.OraclePhysics(ca, ma, terrain=grid(name).terrain)
    _SETTLED[name] = (ca, ma, ph, ph.settle(1)[0])
  return _SETTLED[name]
