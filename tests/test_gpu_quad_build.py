"""The four-column f64 build (gym_solo_amd/csrc/solo_wave_ops.h: ColumnBank<double>::build_quad - four Delassus columns per
pass on the wave's four 16-lane quarters, in the steps with at most 16 live rows) against the paired build and the single-column
build, ON THE GPU and BIT FOR BIT: the product library, libsolo_hip_pair_only.so (the same sources with
-DSOLO_F64_QUAD_BUILD=0) and libsolo_hip_single_build.so (-DSOLO_F64_PAIR_BUILD=0) run the same float64 workloads in one fresh
process each; every result must be identical - a bank entry is the same multiply / fused multiply-add sequence on the same
operands whichever quarter computes it.

The robots are PLACED, twelve kinds of 16 (place()): so that the first step of every kind has a known number of live rows L -
8, 11, 14 (the quad schedule: 2, 3, 4 passes), 17, 20 (the pair schedule), 44 (the overflow path, no column built), and with
joints inside the limit margin 9, 12, 15 and 16 (L is then no 8 + 3 t: the quarter mask, the own-lane zero and the `while
n_live > 4 q` of the schedule at L = 4 q and 4 q + 1; 16 / 17 is the boundary between the two schedules) - and two kinds that
drop onto the ground within a few steps, so that their L crosses 16 between consecutive steps of ONE launch (what the lanes
16 .. 31 hold goes from a copy of the lanes 0 .. 15 back to rows of their own).  The host counts L of every robot-step from the
recorded states (live_rows of tests/test_gpu_pair_build.py) and the tests assert that each of these occurred.

Launch kinds: single steps (default solver; residual threshold 1e-7: kernels of their own), a fused 20-step launch, the same 20
steps as single-step launches (whose recorded states give the L of every step of the fused launch: the two end in the same bits),
a solo_roll_kernel rollout of three segments of four steps, contact sensing and torque control."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'gym_solo_amd', 'csrc')
KINDS, PER_KIND = 12, 16
N, STEPS, FUSED, SEG = KINDS * PER_KIND, 12, 20, 4
# live rows of the FIRST step of a robot of kind k (None: not pinned - the two kinds that drop)
FIRST_L = (8, 11, 14, 17, 20, 44, 9, 12, 15, 16, None, None)


def place(base, ph, radius, cfg):
  """[N, STATE_STRIDE] from one settled state.  Kind k = robot // PER_KIND; within a kind the robots differ by a little height
  (less than the safety of the contact counts) so that no two run the same numbers.
  0: lifted.  1 - 4: the base rolled and pitched a little, which puts its four lowest spheres at four heights (2 mm and more
  apart), and lowered until exactly 1 .. 4 of them are inside the contact margin.  5: lying flat on base and legs (12 spheres).
  6 - 9: lifted, with 1, 4, 7, 8 joints inside the margin of their limit (+-10 rad).  10: level, the lowest spheres 3 mm above
  the margin.  11: tilted as 1 - 4, the lowest sphere 2 mm above the margin."""
  from gym_solo_amd import abi
  st = np.repeat(base[None], N, axis=0).copy()
  st[:, abi.S_ANGVEL:abi.S_QD + 8] = 0.0
  jitter = np.linspace(0.0, 2e-4, PER_KIND)
  tilted = base.copy()
  quat = np.array([0.010, 0.0125, 0.0, 1.0])                       # (x, y, z, w): roll 0.02 rad, pitch 0.025 rad
  tilted[abi.S_QUAT:abi.S_QUAT + 4] = quat / np.linalg.norm(quat)
  level = base.copy()
  level[abi.S_QUAT:abi.S_QUAT + 4] = (0.0, 0.0, 0.0, 1.0)
  clear_t = np.sort(ph.sphere_centers(tilted)[:, 2] - radius)
  clear_l = np.sort(ph.sphere_centers(level)[:, 2] - radius)
  assert (np.diff(clear_t[:5]) > 1.5e-3).all(), clear_t[:5]        # (0.7 mm inside the margin, the next sphere 0.6 mm and more outside, jitter included)
  kind = lambda k: slice(k * PER_KIND, (k + 1) * PER_KIND)
  st[kind(0), abi.S_POS + 2] += 0.3 + jitter
  for t in (1, 2, 3, 4):
    st[kind(t)] = tilted
    st[kind(t), abi.S_POS + 2] -= clear_t[t - 1] - (cfg.contact_margin - 7e-4) - jitter
  st[kind(5), abi.S_Q:abi.S_Q + 8] = np.array([np.pi / 2, 0, np.pi / 2, 0, -np.pi / 2, 0, -np.pi / 2, 0])
  st[kind(5), abi.S_POS + 2] = 0.021 - jitter
  for k, limited in ((6, 1), (7, 4), (8, 7), (9, 8)):
    st[kind(k), abi.S_POS + 2] += 0.3 + jitter
    st[kind(k), abi.S_Q:abi.S_Q + limited] = np.where(np.arange(limited) % 2 == 0, 9.8, -9.8)
  st[kind(10)] = level
  st[kind(10), abi.S_POS + 2] -= clear_l[0] - (cfg.contact_margin + 3e-3) - jitter
  st[kind(11)] = tilted
  st[kind(11), abi.S_POS + 2] -= clear_t[0] - (cfg.contact_margin + 2e-3) - jitter
  return st


_WORKER = r'''
import sys, os
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, 'tests'))
import numpy as np, torch
from gym_solo_amd import abi
from gym_solo_amd.engine import Engine
from helpers import make_abi
from oracle import solo_oracle as so
import bench
import test_gpu_quad_build as tq
out = sys.argv[1]
N, STEPS, FUSED, SEG = tq.N, tq.STEPS, tq.FUSED, tq.SEG
res = {}
placed = None

# ---- single steps, every state kept: the default solver, then pybullet's residual threshold (kernels of their own)
for case, resid in (('step', 0.0), ('resid', 1e-7)):
  ca, ma = make_abi('float64', settle_steps=100, solver_residual_threshold=resid)
  eng = Engine(ca, ma, N)
  if placed is None:
    ph = so.OraclePhysics(ca, ma)
    radius = np.array([ma.sphere_radius[i] for i in range(ma.num_spheres)])
    placed = torch.as_tensor(tq.place(eng.state[0].cpu().numpy(), ph, radius, ca), device='cuda')
  eng.state.copy_(placed)
  acts = torch.as_tensor(np.random.default_rng(5).uniform(-6, 6, (STEPS, N, 12)), device='cuda', dtype=torch.float64)
  states = torch.empty(STEPS + 1, N, abi.STATE_STRIDE, device='cuda', dtype=torch.float64)
  cost = torch.zeros(N, device='cuda', dtype=torch.int64)
  for i in range(STEPS):
    states[i].copy_(eng.state)
    eng.step(acts[i], abi.STEP_PHYSICS)
    cost += eng.cost
  states[STEPS].copy_(eng.state)
  torch.cuda.synchronize()
  res[case + '_states'] = states.cpu().numpy()
  res[case + '_cost'] = cost.cpu().numpy()
  eng.close()

# ---- launches of the benchmark's environment from the placed states: one fused launch of 20 recorded steps, the same steps as
#      20 launches (every state kept), three fused segments of four steps in one launch, contact sensing, torque control
def launch(case, k, prepare=None, **kw):
  env = bench.build_env(N, 0, 'float64', **kw)
  eng = env.engine
  if prepare is not None:
    prepare(eng)
  eng.state.copy_(placed)
  g = torch.Generator(device='cuda').manual_seed(77)
  acts = (torch.rand(k, N, 12, device='cuda', dtype=torch.float64, generator=g) * 2 - 1) * (2 * np.pi)
  if case == 'replay':
    states = torch.empty(k, N, abi.STATE_STRIDE, device='cuda', dtype=torch.float64)
    for i in range(k):
      states[i].copy_(eng.state)
      eng.step(acts[i], abi.STEP_ALL)
    res['replay_states'] = states.cpu().numpy()
  else:
    o = eng.rollout(acts, abi.STEP_ALL, out=eng.rollout_buffers(k))
    torch.cuda.synchronize()
    res.update({case + '_obs': o[0].cpu().numpy(), case + '_reward': o[1].cpu().numpy(), case + '_done': o[2].cpu().numpy(),
                case + '_plan': np.array([eng.plan(k)[f] for f in ('steps_per_launch', 'launches', 'migrate_steps')])})
  torch.cuda.synchronize()
  res[case + '_state'] = eng.state.cpu().numpy()
  res[case + '_kernel'] = np.frombuffer(eng.kernel_name.encode(), dtype=np.uint8)
  if case == 'contact':
    res['contact_record'] = eng.contacts.cpu().numpy()
  env._close()

launch('fused', FUSED, steps_per_launch=FUSED, rollout_streams=1, migrate_steps=0)
launch('replay', FUSED, steps_per_launch=1, rollout_streams=1, migrate_steps=0)
launch('roll', 3 * SEG, steps_per_launch=SEG, rollout_streams=1, migrate_steps=0)
launch('contact', FUSED, lambda eng: eng.set_contact_sensing(True), steps_per_launch=FUSED, rollout_streams=1, migrate_steps=0)
launch('torque', FUSED, lambda eng: eng.set_control('torque', action_scale=0.3), steps_per_launch=FUSED, rollout_streams=1, migrate_steps=0)
np.savez(out, **res)
'''

ROLLOUT = ('obs', 'reward', 'done', 'state')
CASES = {'step': ('states', 'cost'), 'resid': ('states', 'cost'), 'fused': ROLLOUT, 'replay': ('states', 'state'), 'roll': ROLLOUT,
         'contact': ROLLOUT + ('record',), 'torque': ROLLOUT}
KERNEL = {'fused': b'solo_step_kernel<double', 'replay': b'solo_step_kernel<double', 'roll': b'solo_roll_kernel<double>',
          'contact': b'solo_contact_kernel<double', 'torque': b'solo_ctl_step_kernel<double'}
LIBS = {'quad': 'libsolo_hip.so', 'pair': 'libsolo_hip_pair_only.so', 'single': 'libsolo_hip_single_build.so'}


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
  """The workloads on the three libraries: ONE fresh process per library (SOLO_HIP_LIB is read at import), shared by the tests."""
  tmp = tmp_path_factory.mktemp('quad_build')
  got = {}
  for name, lib in LIBS.items():
    lib = os.path.join(CSRC, lib)
    assert os.path.isfile(lib), 'build it: make -C gym_solo_amd/csrc test-libs (or __graft_entry__.build())'
    out = str(tmp / (name + '.npz'))
    subprocess.run([sys.executable, '-c', _WORKER % {'root': ROOT}, out], check=True, env=dict(os.environ, SOLO_HIP_LIB=lib), timeout=300)
    got[name] = dict(np.load(out))
  return got


@pytest.fixture(scope='module')
def counter():
  """L of one state, as the step kernel counts it (the host's count: tests/test_gpu_pair_build.py)"""
  from helpers import make_abi
  from oracle import solo_oracle as so
  from test_gpu_pair_build import live_rows
  ca, ma = make_abi('float64', settle_steps=100)
  ph = so.OraclePhysics(ca, ma)
  radius = np.array([ma.sphere_radius[i] for i in range(ma.num_spheres)])
  return lambda states: np.array([[live_rows(ph, radius, ca, np.ascontiguousarray(s)) for s in step] for step in states])


@pytest.mark.parametrize('other', ['pair', 'single'])
@pytest.mark.parametrize('case', sorted(CASES))
def test_quad_build_equals_the_other_builds_bit_for_bit(runs, case, other):
  a, b = runs['quad'], runs[other]
  for field in CASES[case]:
    k = case + '_' + field
    assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype
    assert a[k].tobytes() == b[k].tobytes(), 'the quad build and the %s build differ in %r' % (other, k)
    assert np.isfinite(a[k]).all()
  if case in ('step', 'resid'):
    assert a[case + '_cost'].max() > 0   # (sweeps were counted)
  else:
    assert a[case + '_kernel'].tobytes() == b[case + '_kernel'].tobytes() and KERNEL[case] in a[case + '_kernel'].tobytes()
  if case in ('fused', 'contact', 'torque'):
    assert tuple(int(x) for x in a[case + '_plan']) == (FUSED, 1, 0)   # (one launch)
  if case == 'roll':
    assert tuple(int(x) for x in a['roll_plan']) == (SEG, 3, 0)        # (three segments of SEG steps, which the roll kernel runs as one launch)


def test_single_steps_cover_both_schedules_the_limit_rows_and_the_overflow_path(runs, counter):
  for case in ('step', 'resid'):
    L = counter(runs['quad'][case + '_states'][:-1])   # (the states the STEPS steps started in)
    seen = sorted(set(L.ravel().tolist()))
    print('%s: live rows per robot-step: %s' % (case, ' '.join('%d:%d' % (x, (L == x).sum()) for x in seen)))
    for k, want in enumerate(FIRST_L):
      if want is not None:
        assert (L[0, k * PER_KIND:(k + 1) * PER_KIND] == want).all(), (case, k, want, L[0, k * PER_KIND:(k + 1) * PER_KIND])
    for want in (8, 11, 14, 17, 20):          # (quad schedule: 2, 3, 4 passes; pair schedule)
      assert want in seen
    assert 9 in seen and 12 in seen           # (joint-limit rows: L = 4 q + 1 and 4 q)
    assert 16 in seen and 17 in seen          # (the boundary between the two schedules)
    assert any(x > 32 for x in seen)          # (the overflow path)


def test_live_rows_cross_16_inside_the_fused_launch(runs, counter):
  r = runs['quad']
  assert r['replay_state'].tobytes() == r['fused_state'].tobytes()   # (the recorded states ARE the fused launch's)
  L = counter(r['replay_states'])
  up = ((L[:-1] <= 16) & (L[1:] > 16)).any(axis=0)
  down = ((L[:-1] > 16) & (L[1:] <= 16)).any(axis=0)
  print('robots whose live rows cross 16 inside the launch: %d upwards, %d downwards, %d both ways' % (up.sum(), down.sum(), (up & down).sum()))
  assert up.sum() >= PER_KIND   # (at the least the kind that is dropped level: 3 mm of free fall, then four spheres at once)
