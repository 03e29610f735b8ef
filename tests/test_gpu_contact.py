"""GPU suite of contact sensing (solo_engine_set_contact_sensing, solo_contact_kernel) through the C-ABI on the MI355X.

  1. one-step per-sphere parity against the CPU oracle's impulses (OraclePhysics.step_debug): f_s = sum over the sphere's
     rows of lam_r d_r / dt, d_r = the base-translation block of the row's Jacobian rotated to world - on the flat plane,
     the 10-degree incline and the stairs, half the robots with their own friction and base mass;
  2. a closed form that does not depend on the oracle: a settled robot on flat ground carries its weight;
  3. sensing changes no physics: fused rollouts with auto-reset are bit-identical with sensing on and off, in every mode;
  4. the foot-force observations of every step of a recorded fused rollout equal column 3 of that step's record taken by
     single-step launches (zeros on the steps that restart a robot);
  5. the rejection rules, and the record after reset / restore;
  6. 8192 robots (more than the chip's wave slots) give the records of two runs of 4096;
  7. closed forms on the 10-degree incline: a sticking robot's forces sum to -m g, a sliding foot's friction is mu times its
     normal force, uphill.
"""
import numpy as np
import pytest

from gym_solo_amd import abi
import contact_cases as cc
from helpers import incline_terrain, make_abi, random_actions, stairs_terrain

pytestmark = pytest.mark.gpu

N = 4096
DT = 1e-3


@pytest.fixture(scope='module')
def torch():
  import torch
  if not torch.cuda.is_available():
    pytest.fail('GPU tests need a visible MI355X')
  return torch


def _engine(ca, ma, n=N):
  from gym_solo_amd.engine import Engine
  return Engine(ca, ma, n)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('ground', ['flat', 'incline', 'stairs'])
def test_one_step_parity_against_step_debug(torch, ground, dtype):
  cc.one_step_parity_against_step_debug(torch, ground, dtype, make_abi(dtype)[1], N, every=4)


def test_settled_robot_carries_its_weight(torch):
  """Closed form: a robot holding its settle pose on flat ground - sum over the spheres of the record = (0, 0, m g)."""
  ca, ma = make_abi('float64')
  eng = _engine(ca, ma)
  eng.set_contact_sensing(True)
  eng.step(None, abi.STEP_PHYSICS)
  f = eng.contacts.cpu().numpy()
  total = f[:, :, :3].sum(axis=1)
  mg = -float(np.sum(list(ma.mass))) * ca.gravity[2]
  rel = np.abs(total - np.array([0.0, 0.0, mg])) / mg
  print('settled: sum f = {}, m g = {:.6f}, worst relative error {:.3e}'.format(total[0], mg, rel.max()))
  assert rel.max() < 1e-6
  assert np.all(f[:, :, 3] >= 0)


def _workload_env(dtype, n, mode, sensing, max_steps=50, foot=False):
  from gym_solo_amd.core import obs as solo_obs
  from gym_solo_amd.envs.solo8v2vanilla import Solo8VanillaConfig, Solo8VanillaEnv
  from gym_solo_amd.workloads import register_benchmark_workload
  cfg = Solo8VanillaConfig()
  cfg.dtype, cfg.num_envs, cfg.auto_reset = dtype, n, True
  cfg.control_mode = mode
  if mode == 'pd':
    cfg.pd_kp, cfg.pd_kd = 3.0, 0.05
  cfg.contact_sensing = sensing
  env = Solo8VanillaEnv(config=cfg)
  register_benchmark_workload(env, max_steps=max_steps)
  if foot:
    env.obs_factory.register_observation(solo_obs.FootContact(env.robot))
    env.obs_factory.register_observation(solo_obs.FootContact(env.robot, binary=True))
  env._ensure_program()
  return env


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('mode', ['position', 'torque', 'pd'])
def test_sensing_changes_no_physics(torch, dtype, mode):
  rng = np.random.default_rng(3)
  scale = 1.0 if mode == 'torque' else 0.5
  acts = torch.as_tensor(random_actions(rng, N, scale)[None].repeat(200, 0) * rng.uniform(0.5, 1.0, (200, 1, 1)),
                         device='cuda', dtype=torch.float64 if dtype == 'float64' else torch.float32)
  out = {}
  for sensing in (False, True):
    env = _workload_env(dtype, N, mode, sensing)
    rec = env.engine.rollout(acts, abi.STEP_ALL, record=True)
    env.engine.synchronize()
    out[sensing] = [t.cpu().numpy() for t in rec] + [env.engine.state.cpu().numpy()]
    if sensing:
      assert env.engine.kernel_name.startswith('solo_contact_kernel')
  assert out[True][2].any()   # (episodes ended inside the rollout: auto-resets ran)
  for a, b in zip(out[False], out[True]):
    np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_foot_observations_equal_the_record_of_each_step(torch, dtype):
  rng = np.random.default_rng(5)
  k, n = 30, N
  # (the benchmark's U(+-2 pi) targets, fresh every step: the legs swing down and the feet hit the ground - from the folded
  # settle pose the robot rests on its knees and its base)
  acts = torch.as_tensor(np.stack([random_actions(rng, n) for _ in range(k)]), device='cuda',
                         dtype=torch.float64 if dtype == 'float64' else torch.float32)
  acts[10, 7, 0] = float('nan')   # (robot 7 diverges in step 10 and is restored: it reads zeros there)
  env = _workload_env(dtype, n, 'position', True, max_steps=12, foot=True)
  eng = env.engine
  start = eng.state.clone()
  obs, _, done = eng.rollout(acts, abi.STEP_ALL, record=True)
  obs, done = obs.cpu().numpy(), done.cpu().numpy()
  # the same steps as single-step launches from the same start
  eng.state.copy_(start)
  eng.term_count.zero_()
  eng.reset(None)
  eng.state.copy_(start)
  for j in range(k):
    eng.step(acts[j], abi.STEP_ALL)
    rec = eng.contacts.cpu().numpy()
    foot = np.clip(rec[:, 1::4, 3], 0.0, 100.0)
    binary = np.clip(rec[:, 1::4, 3] * np.asarray(1e9, dtype=rec.dtype), 0.0, 1.0)
    np.testing.assert_array_equal(obs[j][:, -8:-4], foot)
    np.testing.assert_array_equal(obs[j][:, -4:], binary)
    np.testing.assert_array_equal(eng.obs.cpu().numpy()[:, -8:], np.concatenate([foot, binary], axis=1))
    if j == 10:
      assert np.all(obs[j][7, -8:] == 0) and np.all(rec[7] == 0)
    np.testing.assert_array_equal(eng.done.cpu().numpy(), done[j])
    if done[j].any():
      assert np.all(rec[done[j].astype(bool)] == 0)   # (a robot that auto-resets reads zeros)
  assert done.any()
  assert (obs[:, :, -8:-4] > 0).any() and (obs[:, :, -4:] == 1).any()
  assert eng.stats.cpu().numpy()[5] >= 1
  # the Python path reads the same record, in both modes
  np.testing.assert_array_equal(env.obs_factory._observations[-2].compute().cpu().numpy(), foot)
  np.testing.assert_array_equal(env.obs_factory._observations[-1].compute().cpu().numpy(), binary)


def test_rejections_and_resets(torch):
  from gym_solo_amd.envs.solo8v2vanilla import Solo8VanillaConfig
  for kw in (dict(migrate_steps=5), dict(solver_residual_threshold=1e-7), dict(solver_residual_threshold=1e-7, solver_warm_start=0.5)):
    ca, ma = make_abi('float64', **kw)
    eng = _engine(ca, ma, 64)
    with pytest.raises(ValueError):
      eng.set_contact_sensing(True)
    with pytest.raises(ValueError):
      eng.contacts
  ca, ma = make_abi('float64')
  eng = _engine(ca, ma, 64)
  prog = abi.SoloProgram()
  prog.num_obs = 1
  prog.obs[0].src = abi.SRC_FOOT_FORCE + 2
  prog.obs[0].scale = 1.0
  with pytest.raises(ValueError):
    eng.set_program(prog)            # (sensing off)
  eng.set_contact_sensing(True)
  assert np.all(eng.contacts.cpu().numpy() == 0)
  eng.set_program(prog)
  with pytest.raises(ValueError):
    eng.set_contact_sensing(False)   # (the program reads a foot force)
  eng.step(None, abi.STEP_PHYSICS | abi.STEP_OBS)
  c = eng.contacts.cpu().numpy()
  assert (c[:, :, 3].sum(axis=1) > 0).all()   # (settled robots stand on the ground)
  np.testing.assert_array_equal(eng.obs.cpu().numpy()[:, 0], c[:, 9, 3])
  mask = torch.zeros(64, dtype=torch.uint8, device='cuda')
  mask[::2] = 1
  eng.reset(mask)
  c2 = eng.contacts.cpu().numpy()
  assert np.all(c2[::2] == 0)
  np.testing.assert_array_equal(c2[1::2], c[1::2])
  eng.step(None, abi.STEP_OBS)       # (no physics: the record stands, the observation reads it)
  np.testing.assert_array_equal(eng.obs.cpu().numpy()[:, 0], c2[:, 9, 3])
  # a diverged robot is restored and reads zeros
  bad = (eng.targets / ca.action_scale).contiguous()   # (the others keep holding their pose: they stay on the ground)
  bad[3, 0] = float('nan')
  eng.step(bad, abi.STEP_PHYSICS)
  c3 = eng.contacts.cpu().numpy()
  assert np.all(c3[3] == 0) and c3[np.arange(64) != 3].any()
  assert eng.stats.cpu().numpy()[5] == 1
  eng.set_program(abi.SoloProgram())
  eng.set_contact_sensing(False)
  with pytest.raises(ValueError):
    eng.contacts


def test_8192_robots_give_the_records_of_two_runs_of_4096(torch):
  ca, ma = make_abi('float64')
  rng = np.random.default_rng(11)
  acts = random_actions(rng, 2 * N, 0.5)
  rec = {}
  for n in (2 * N, N):
    eng = _engine(ca, ma, n)
    eng.set_contact_sensing(True)
    for part in range(2 * N // n):
      eng.reset(None)
      a = torch.as_tensor(acts[part * n:(part + 1) * n], device='cuda')
      for _ in range(20):
        eng.step(a, abi.STEP_PHYSICS)
      rec[(n, part)] = eng.contacts.cpu().numpy()
  np.testing.assert_array_equal(rec[(2 * N, 0)][:N], rec[(N, 0)])
  np.testing.assert_array_equal(rec[(2 * N, 0)][N:], rec[(N, 1)])


def test_checkpoint_resume_is_bit_for_bit_with_sensing(torch):
  ca, ma = make_abi('float64')
  rng = np.random.default_rng(13)
  acts = torch.as_tensor(random_actions(rng, N, 0.5)[None].repeat(40, 0), device='cuda')
  a = _engine(ca, ma)
  a.set_contact_sensing(True)
  a.rollout(acts[:20], abi.STEP_PHYSICS)
  ckpt = (a.state.clone(), a.targets.clone())
  a.rollout(acts[20:], abi.STEP_PHYSICS)
  b = _engine(ca, ma)
  b.set_contact_sensing(True)
  b.state.copy_(ckpt[0]); b.targets.copy_(ckpt[1])
  b.rollout(acts[20:], abi.STEP_PHYSICS)
  np.testing.assert_array_equal(a.state.cpu().numpy(), b.state.cpu().numpy())
  np.testing.assert_array_equal(a.contacts.cpu().numpy(), b.contacts.cpu().numpy())


def test_closed_forms_on_the_incline(torch):
  """10-degree incline, no damping, per-robot friction (closed_form_cases): after the landing, a robot whose friction holds
  it (mu > tan theta) is at rest and its contact forces sum to -m g as a world vector, which pins the basis and the signs; on
  a robot that slides, every touching foot's friction force along the slope is mu times its normal force and points UP the
  slope, and the sideways forces cancel over the robot."""
  import closed_form_cases as cf
  from gym_solo_amd.model import Solo8Model
  ca, ma = make_abi('float64', linear_damping=0.0, angular_damping=0.0, settle_steps=10)
  eng = _engine(ca, ma)
  eng.set_terrain(incline_terrain(10.0))
  mus = cf.incline_frictions(N, seed=3)
  eng.set_params(abi.PARAM_FRICTION, torch.as_tensor(mus, device='cuda'))
  eng.state.copy_(torch.as_tensor(cf.standing_on_incline(N), device='cuda'))
  eng.set_contact_sensing(True)
  zero = torch.zeros(N, 12, device='cuda', dtype=torch.float64)
  eng.rollout(zero.expand(300, N, 12).contiguous(), abi.STEP_PHYSICS)
  f = eng.contacts.cpu().numpy()
  mg = Solo8Model().total_mass * 9.81
  slides = mus < np.tan(cf.THETA)
  total = f[~slides, :, :3].sum(axis=1)
  stick_err = np.abs(total - np.array([0.0, 0.0, mg])).max() / mg
  fn = f[slides, :, 3]
  along = f[slides, :, :3] @ cf.T1_SLOPE
  touching = fn > 0
  slide_err = np.abs(along - mus[slides, None] * fn)[touching].max() / mg
  print('incline: sticking sum f - (0, 0, m g): {:.3e} of m g; sliding |f.t1 - mu fn|: {:.3e} of m g, {} touching feet'.format(
    stick_err, slide_err, touching.sum()))
  assert touching.sum() >= 4 * slides.sum() * 0.9     # (the sliding robots stand on their feet)
  assert np.all(along[touching] > 0)                   # (uphill)
  assert slide_err < 1e-9
  # (the sideways rows - t2 = world y on this slope - are not saturated: the feet push against each other, which only the sum
  # over the robot pins)
  assert np.abs(f[slides, :, 1].sum(axis=1)).max() < 1e-9 * mg
  assert stick_err < 1e-6

