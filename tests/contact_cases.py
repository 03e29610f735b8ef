"""Shared case of the contact-sensing parity tests on the GPU (tests/test_gpu_contact.py on the built-in model,
tests/test_gpu_model_space.py on models with another sphere -> link layout): one step's per-sphere record against the CPU
oracle's impulses (OraclePhysics.step_debug)."""
import numpy as np

from gym_solo_amd import abi
from helpers import incline_terrain, make_abi, random_actions, stairs_terrain


def rot(q):
  x, y, z, w = q
  return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                   [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                   [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def oracle_forces(dbg, state, dt):
  """[16, 4] from the oracle's rows: sum over the sphere's rows of lam_r R J_r[3:6] / dt, and the normal row's lam / dt
  (the first row of a sphere is its normal row)."""
  out = np.zeros((abi.MAX_SPHERES, 4))
  R = rot(state[abi.S_QUAT:abi.S_QUAT + 4])
  seen = set()
  for r in range(dbg.num_rows):
    s = dbg.row_sphere[r]
    if s < 0:
      continue
    d = R @ np.array([dbg.J[r][3], dbg.J[r][4], dbg.J[r][5]])
    out[s, :3] += dbg.lam[r] * d / dt
    if s not in seen:
      out[s, 3] = dbg.lam[r] / dt
      seen.add(s)
  return out, seen


def flail(torch, eng, rng, steps=30):
  for _ in range(steps):
    a = torch.as_tensor(random_actions(rng, eng.num_envs, 0.6), device='cuda', dtype=eng.tdtype)
    eng.step(a, abi.STEP_PHYSICS)


# The f32 bar, derived: the step's penetration bias is -dist / dt, and dist comes out of a cancellation of world positions of
# ~0.3 m, rounded at 2^-24 x 0.3 m = 2e-8 m in f32.  A velocity error of 2e-8 m / dt, applied to the robot's 1.9 kg within one
# step, is a force error of 1.9 x 2e-8 / dt^2 = 0.04 N per rounding; a few such roundings meet in one sphere's rows, and the
# state itself - the oracle steps the f32 state widened to f64 - is exact.  Bar: 0.5 N (about 3 % of the robot's weight).
# The f64 bar is the issue's estimate, 1e-6 N.  Rows within 1e-9 m (f64) / 1e-5 m (f32) of the contact margin are skipped:
# rounding decides whether they exist.
BARS = {'float64': (1e-6, 1e-9), 'float32': (0.5, 1e-5)}


def gaps(ph, ma, terrain, st):
  """per sphere: the distance to the ground the step's rows use (flat: z - r; heightfield: along the tangent plane's normal)"""
  c = ph.sphere_centers(st.copy())
  r = np.array(list(ma.sphere_radius))
  if terrain is None:
    return c[:, 2] - r
  h = np.ctypeslib.as_array(terrain.heights, shape=(terrain.ny * terrain.nx,)).reshape(terrain.ny, terrain.nx)
  out = np.zeros(len(r))
  for s in range(len(r)):
    gu0, gv0 = (c[s, 0] - terrain.origin[0]) / terrain.cell, (c[s, 1] - terrain.origin[1]) / terrain.cell
    gu, gv = np.clip(gu0, 0, terrain.nx - 1), np.clip(gv0, 0, terrain.ny - 1)   # outside the grid: the clamped point's height ...
    i, j = min(int(np.floor(gu)), terrain.nx - 2), min(int(np.floor(gv)), terrain.ny - 2)
    fu, fv = gu - i, gv - j
    h00, h10, h01, h11 = h[j, i], h[j, i + 1], h[j + 1, i], h[j + 1, i + 1]
    hh = (1 - fu) * (1 - fv) * h00 + fu * (1 - fv) * h10 + (1 - fu) * fv * h01 + fu * fv * h11
    hx = 0.0 if gu != gu0 else ((1 - fv) * (h10 - h00) + fv * (h11 - h01)) / terrain.cell   # ... and no slope along a clamped axis
    hy = 0.0 if gv != gv0 else ((1 - fu) * (h01 - h00) + fu * (h11 - h10)) / terrain.cell
    out[s] = (c[s, 2] - hh) / np.sqrt(hx * hx + hy * hy + 1) - r[s]
  return out


def one_step_parity_against_step_debug(torch, ground, dtype, ma, n, every=4, flail_steps=30):
  """f_s = sum over the sphere's rows of lam_r d_r / dt on every `every`-th of n robots, half of them with their own friction
  and base mass, after `flail_steps` flailing steps; asserts the bar of BARS and returns (the set of spheres that touched somewhere, the engine's count of diverged robots)"""
  from gym_solo_amd.engine import Engine
  from oracle import solo_oracle as so
  from gym_solo_amd.model import DOF_TO_JOINT
  ca, _ = make_abi(dtype)
  ca64, _ = make_abi('float64')
  bar, amb = BARS[dtype]
  terrain = {'flat': None, 'incline': incline_terrain(), 'stairs': stairs_terrain()}[ground]
  eng = Engine(ca, ma, n)
  N = n
  if terrain is not None:
    eng.set_terrain(terrain)
  rng = np.random.default_rng(7)
  params = eng.params.cpu().numpy().copy()
  half = np.arange(N) % 2 == 1
  params[half, 0] = rng.uniform(0.3, 1.2, half.sum())
  params[half, 1] = rng.uniform(0.8, 1.3, half.sum())
  eng.set_params(abi.PARAM_FRICTION, torch.as_tensor(params[:, 0].copy(), device='cuda', dtype=eng.tdtype))
  eng.set_params(abi.PARAM_BASE_MASS_SCALE, torch.as_tensor(params[:, 1].copy(), device='cuda', dtype=eng.tdtype))
  params = eng.params.cpu().numpy().astype(np.float64)   # (as the engine holds them)
  eng.set_contact_sensing(True)
  flail(torch, eng, rng, flail_steps)
  st = eng.state.cpu().numpy().astype(np.float64)
  tg = eng.targets.cpu().numpy().astype(np.float64)
  eng.step(None, abi.STEP_PHYSICS)
  got = eng.contacts.cpu().numpy().astype(np.float64)
  ph = so.OraclePhysics(ca64, ma, terrain=terrain)
  worst, touching, checked, touched = 0.0, 0, 0, set()
  for e in range(0, N, every):
    dbg = ph.step_debug(st[e].copy(), tg[e][DOF_TO_JOINT].copy(), params[e].copy())
    want, live = oracle_forces(dbg, st[e], ca.dt)
    gap = gaps(ph, ma, terrain, st[e])
    for s in range(abi.MAX_SPHERES):
      if abs(gap[s] - ca.contact_margin) < amb:
        continue
      if s not in live:
        assert np.all(got[e, s] == 0), (e, s, got[e, s])
      worst = max(worst, float(np.max(np.abs(got[e, s] - want[s]))))
    touching += len(live)
    touched |= set(live)
    checked += 1
  print('contact parity ({}, {}): {} robots, {} touching spheres, worst |df| = {:.3e} N (bar {:g})'.format(
    ground, dtype, checked, touching, worst, bar))
  assert touching > checked          # (robots on the ground, most with several spheres)
  assert worst < bar
  diverged = float(eng.stats.cpu().numpy()[5])
  eng.close()
  return touched, diverged
