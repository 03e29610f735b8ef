"""The heightfield ground of the HIP engine against its documented contract (include/solo_engine.h, SoloTerrain; the reference and
the cases: tests/terrain_cases.py - an analytic surface and a longdouble restatement of the header's words, not the oracle's
ground_at), and what follows from it dynamically.

  A. probes: 256 robots per grid, every robot over its own point (lanes and waves gather different cells) - inside, in the corner
     cells, exactly on the border, outside on all eight sides, on interior grid lines, and at +-1e12 m in a batch of their own - in
     f64 and f32, and with contact sensing on;
  B. the shelf beyond the incline's edge is a flat plane; parity with the oracle where no test stood before (scattered over a grid
     that does not contain the world origin, across its borders); fused = single launches on that batch; replacing a terrain.
"""
import numpy as np
import pytest

from gym_solo_amd import abi
import terrain_cases as tc
from helpers import incline_terrain, make_abi, random_actions

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def torch():
  import torch
  if not torch.cuda.is_available():
    pytest.fail('GPU tests need a visible MI355X')
  return torch


def _engine(ca, ma, n, terrain=None):
  from gym_solo_amd.engine import Engine
  eng = Engine(ca, ma, n)
  if terrain is not None:
    eng.set_terrain(terrain)
  return eng


def _put(torch, eng, st):
  eng.state.copy_(torch.as_tensor(st, device='cuda').to(eng.tdtype))


def _step(torch, eng, acts, flags=abi.STEP_PHYSICS):
  eng.step(torch.as_tensor(acts, device='cuda').to(eng.tdtype), flags)


def _probe(torch, name, dtype, far=False, sensing=False):
  ca, ma = make_abi(dtype, gravity=(0., 0., 0.), settle_steps=1)
  B = tc.batch(name, dtype, far)
  eng = _engine(ca, ma, len(B.probes), B.grid.terrain)
  if sensing:
    eng.set_contact_sensing(True)
  _put(torch, eng, B.states)
  assert np.array_equal(eng.state.cpu().numpy().astype(np.float64), B.states)     # (f32: the states are f32 numbers already)
  _step(torch, eng, B.acts)
  post = eng.state.cpu().numpy().astype(np.float64)
  rec = eng.contacts.cpu().numpy().astype(np.float64) if sensing else None
  assert float(eng.stats.cpu().numpy()[5]) == 0
  eng.close()
  err = tc.check(B, post, ca.contact_erp, ca.dt)
  print('gpu ' + tc.summary(B, err))
  assert err.max() < tc.BARS[dtype], tc.summary(B, err)
  return B, rec


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('name', tc.GRID_NAMES)
def test_heightfield_probes(torch, name, dtype):
  """after one step the contact point of the one penetrating sphere leaves along the REFERENCE normal at contact_erp d / dt: 1e-11
  m/s per component in f64, 4e-4 in f32 (terrain_cases.BARS)"""
  _probe(torch, name, dtype)


@pytest.mark.parametrize('name', tc.GRID_NAMES)
def test_heightfield_probes_at_1e12_metres(torch, name):
  """+-1e12 m on one axis, the other inside and outside the grid: the point is clamped in real arithmetic before the conversion"""
  B, _ = _probe(torch, name, 'float64', far=True)
  assert len(B.probes) == 12


@pytest.mark.parametrize('name,dtype', [('saddle_7x19', 'float64'), ('random_11x6', 'float32')])
def test_heightfield_probes_with_contact_sensing(torch, name, dtype):
  """The record of the probed sphere: f = lam_n n + friction, and entry 3 is lam_n / dt - so f . n_reference equals entry 3 (a
  wrong recorded normal shows to first order through the friction part), and where the tangential part vanishes f is parallel
  to the reference normal and entry 3 is |f|; every other sphere's record is zero."""
  B, rec = _probe(torch, name, dtype, sensing=True)
  bar = tc.FORCE_BARS[dtype]
  worst, pushed = 0.0, 0
  for e in range(len(B.probes)):
    f, fn, n = rec[e, B.sphere[e], :3], rec[e, B.sphere[e], 3], B.normal[e]
    # A probe on a grid line or (to rounding) on the border has several legitimate grounds, and under the one the step took the
    # sphere may not reach its tangent plane (the check of the velocities expects no push-out there): no force to look at.
    # Everywhere else the sphere is at least 0.05 mm inside and is pushed out with newtons.
    if B.inside[e] > 2e-5:
      assert fn > 0.1, (e, B.probes[e].kind, fn, B.inside[e])
      pushed += 1
    elif B.inside[e] == 0:
      assert fn == 0, (e, B.probes[e].kind, fn)
    assert B.inside[e] > 2e-5 or B.probes[e].kind in ('line', 'border~'), (e, B.probes[e].kind)
    worst = max(worst, abs(f @ n - fn))
    tang = f - (f @ n) * n
    if np.linalg.norm(tang) < bar:
      assert np.linalg.norm(np.cross(f, n)) < bar and abs(np.linalg.norm(f) - fn) < 2 * bar
    others = np.delete(rec[e], B.sphere[e], axis=0)
    assert np.all(others == 0), e
  assert pushed >= len(B.probes) - 16
  print('gpu sensing on %s %s: worst |f . n - f_n| = %.2e N (bar %g)' % (name, dtype, worst, bar))
  assert worst < bar


def test_the_shelf_beyond_the_incline_is_a_flat_plane(torch):
  """64 robots (lateral_friction 0.05) beyond the +x edge of the incline, at several y: 40 random-action steps equal those of a
  flat-plane engine from the same states lowered by the border height (1e-9); at rest they gain no horizontal momentum (1e-12 kg
  m/s per step), and under zero actions they gain what they gain on the flat plane (tests/terrain_cases.py: shelf_case)."""
  from oracle import solo_oracle as so
  ca, ma = make_abi('float64', lateral_friction=0.05, settle_steps=1)
  n = 64
  engines = _engine(ca, ma, n), _engine(ca, ma, n, incline_terrain())
  def stepper(eng):
    def step(st, act):
      _put(torch, eng, st)
      _step(torch, eng, act)
      return eng.state.cpu().numpy()
    return step
  ca500, _ = make_abi('float64', lateral_friction=0.05)
  state, gain, rel = tc.shelf_case(stepper(engines[0]), stepper(engines[1]), so.OraclePhysics(ca500, ma), n)
  print('gpu shelf: state %.2e, momentum at rest %.2e, against flat %.2e' % (state, gain, rel))
  for eng in engines:
    eng.close()
  assert state < 1e-9 and gain < 1e-12 and rel < 1e-12


@pytest.mark.parametrize('name', ['saddle_7x19', 'random_11x6'])
def test_parity_where_nobody_stood(torch, name):
  """f64 engine against the oracle: the settle snapshot on a grid that does not contain the world origin, then 256 robots
  scattered over the grid and across its four borders, dropped from the settle pose, 40 random-action steps, at 1e-9.  Robot-steps
  with a sphere centre within 1e-9 cell of a grid line are skipped (kernel: x 1 / cell, oracle: / cell) - at most 1 %."""
  ca, ma, ph, snap = tc.settled_on(name)
  g = tc.grid(name)
  n, k = 256, 40
  eng = _engine(ca, ma, n, g.terrain)
  got_snap = eng.snapshot.cpu().numpy()
  err_snap = np.abs(got_snap[:, :29] - snap[None, :29]).max()
  st0 = tc.scattered(g, ph, snap, n)
  rng = np.random.default_rng(8)
  acts = [random_actions(rng, n) for _ in range(k)]
  want, first = tc.oracle_trajectory(g, ph, st0, acts)
  _put(torch, eng, st0)
  for a in acts:
    _step(torch, eng, a)
  got = eng.state.cpu().numpy()
  diverged = float(eng.stats.cpu().numpy()[5])
  eng.close()
  keep = first == k
  skipped = int((k - first).sum())
  err = np.abs(got[keep, :29] - want[keep, :29]).max()
  outside = ((st0[:, 0] < g.terrain.origin[0]).sum(), (st0[:, 1] < g.terrain.origin[1]).sum())
  print('gpu parity on %s: snapshot %.2e, 40 steps %.2e over %d robots, %d robot-steps skipped' % (name, err_snap, err, keep.sum(), skipped))
  assert min(outside) > 5 and diverged == 0
  assert skipped <= 0.01 * n * k
  assert err_snap < 1e-9 and err < 1e-9


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_fused_equals_single_steps_on_the_scattered_batch(torch, dtype):
  """one fused 20-step launch with recorded outputs, the same on two slices, and 20 single launches: bit-identical"""
  from test_env_host import make_env
  from gym_solo_amd.workloads import register_benchmark_workload
  env = make_env()
  register_benchmark_workload(env, max_steps=1000)
  env._ensure_program()
  prog = env.engine.program
  _, ma, ph, snap = tc.settled_on('saddle_7x19')
  g = tc.grid('saddle_7x19')
  n, k = 256, 20
  st0 = tc.scattered(g, ph, snap, n, seed=1)
  tdt = torch.float32 if dtype == 'float32' else torch.float64
  acts = torch.as_tensor(np.random.default_rng(2).uniform(-6, 6, (k, n, 12)), device='cuda').to(tdt)
  out = []
  for spl, streams in ((20, 1), (20, 2), (1, 1)):
    ca, _ = make_abi(dtype, steps_per_launch=spl, rollout_streams=streams, settle_steps=1)
    eng = _engine(ca, ma, n, g.terrain)
    eng.set_program(prog)
    _put(torch, eng, st0)
    if spl > 1:
      assert eng.plan(k)['launches'] == 1 and eng.plan(k)['slices'] == streams
      obs, rew, done = eng.rollout(acts, abi.STEP_ALL, record=True)
    else:
      o, r, d = [], [], []
      for i in range(k):
        eng.step(acts[i], abi.STEP_ALL)
        o.append(eng.obs.clone()); r.append(eng.reward.clone()); d.append(eng.done.clone())
      obs, rew, done = torch.stack(o), torch.stack(r), torch.stack(d)
    torch.cuda.synchronize()
    out.append((obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy(), eng.state.cpu().numpy()))
    eng.close()
  for other in out[1:]:
    for a, b in zip(out[0], other):
      np.testing.assert_array_equal(a, b)
  assert np.isfinite(out[0][3][:, :29]).all()


def test_replacing_a_terrain(torch):
  """set_terrain with 64 x 64, then 7 x 19, then 2 x 2, then 33 x 5 on ONE engine: after each call the snapshot and 20 steps are
  bit-identical to a fresh engine given that terrain directly (a stale nx, ny, origin or buffer would show); then None: the flat
  snapshot."""
  ca, ma = make_abi('float64')
  n = 64
  eng = _engine(ca, ma, n)
  flat = eng.snapshot.clone()
  rng = np.random.default_rng(4)
  acts = [torch.as_tensor(random_actions(rng, n), device='cuda') for _ in range(20)]
  for terrain in (incline_terrain(), tc.grid('saddle_7x19').terrain, tc.grid('saddle_2x2').terrain, tc.grid('saddle_33x5').terrain):
    eng.set_terrain(terrain)
    fresh = _engine(ca, ma, n, terrain)
    assert torch.equal(eng.snapshot, fresh.snapshot), (terrain.nx, terrain.ny)
    for e in (eng, fresh):
      e.reset()
      for a in acts:
        e.step(a, abi.STEP_PHYSICS)
    torch.cuda.synchronize()
    assert torch.equal(eng.state, fresh.state), (terrain.nx, terrain.ny)
    fresh.close()
  eng.set_terrain(None)
  assert torch.equal(eng.snapshot, flat)
  eng.close()
