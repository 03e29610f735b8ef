"""The OUTPUT EPILOGUE of the step kernels (gym_solo_amd/csrc/solo_step_body.h: lane = step, ``pass_steps`` steps per
pass, the reward program's values strided through LDS, lane 0 folding each pass into the episodic accumulators) against
host references that are pinned to the upstream project's own vectors - the golden file
tests/golden/obs_reward_golden.npz and the numpy reductions of oracle/solo_oracle.py (tests/test_oracle_golden.py) in
float64.  Never against the in-place path of single-step launches, which is what every older output test compares with.

  A. no physics: the golden states (and synthetic gimbal-pole orientations) go through ONE fused launch of K steps - the
     step loop leaves the unchanged state as every step's record -, K around the pass length; with an in-launch auto-reset
     from a snapshot of OTHER golden states the lanes of one wave hold different states (divergent gimbal / tolerance /
     clip branches).
  B. physics rollouts with non-benchmark programs: the per-step states come from a twin engine that runs single
     STEP_PHYSICS launches (no output code at all, the host applies the TimeBased schedule with masked resets), the
     expected outputs from the oracle's reductions of those states.
  C. the episodic return / length / statistics after those rollouts against a host loop over the recorded rewards.

Shared by the CPU suite (product kernel source on the wave emulator) and the GPU suite (HIP engine through the C ABI);
every body takes ``make_env(config=..., **kw)``.  The bars are golden_cases.tolerances, unchanged."""
import os
import re

import numpy as np

import golden_cases as gc
from gym_solo_amd import abi
from gym_solo_amd.core import obs as solo_obs
from gym_solo_amd.core import rewards
from gym_solo_amd.core import termination as terms
from gym_solo_amd.envs.solo8v2vanilla import Solo8VanillaConfig
from oracle import solo_oracle as so

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'gym_solo_amd', 'csrc')


def pass_steps(dtype):
  """kPass of the output epilogue, derived from the kernel source the way the kernel derives it: the row-vector block
  (kRowBlockReals<T>, solo_step_kernel.h - in f64 it depends on the waves per SIMD the kernel is built for) divided by
  SOLO_MAX_REWARD_OPS, at most 32 (solo_step_body.h: `constexpr int kPass`, under its static_assert "the output
  epilogue's scratch").  32 in f32; in f64 25 for the product build (four waves per SIMD, 800 reals) and 28 for the
  three- / two-wave A/B builds (896 reals)."""
  kernel = open(os.path.join(CSRC, 'solo_step_kernel.h')).read()
  body = open(os.path.join(CSRC, 'solo_step_body.h')).read()
  assert 'constexpr int kPass = kRowsReals / SOLO_MAX_REWARD_OPS < 32 ? kRowsReals / SOLO_MAX_REWARD_OPS : 32;' in body
  assert 'constexpr int kRowsReals = kRowBlockReals<T>;' in body
  waves = int(re.search(r'#ifndef SOLO_F64_WAVES\s*\n#define SOLO_F64_WAVES (\d+)', kernel).group(1))
  m = re.search(r'constexpr int kRowBlockReals = sizeof\(T\) == 4 \? ([0-9 *+]+) : \(SOLO_F64_WAVES >= 4 \? (\d+) : (\d+)\);', kernel)
  reals = eval(m.group(1)) if dtype == 'float32' else int(m.group(2) if waves >= 4 else m.group(3))  # (digits, * and + only)
  return min(32, reals // abi.MAX_REWARD_OPS)


def launch_lengths(dtype):
  """Steps per launch around the pass length: 2, one below / at / above one pass, two passes + 1 - for the pass length of
  the source at hand, and for the values 28 (f64) / 32 (f32) whatever the source says (a three-wave f64 build)."""
  out = set()
  for p in {pass_steps(dtype), 28 if dtype == 'float64' else 32}:
    out |= {2, p - 1, p, p + 1, 2 * p + 1}
  return sorted(out)


def _cfg(dtype, n, **kw):
  cfg = Solo8VanillaConfig()
  cfg.dtype, cfg._dtype_pinned, cfg.num_envs, cfg._num_envs_pinned = dtype, True, n, True
  cfg.settle_steps = 0   # every state is loaded by the test
  for k, v in kw.items():
    setattr(cfg, k, v)
  return cfg


def _to(env, a):
  import torch
  s = env.engine.state
  return torch.as_tensor(np.ascontiguousarray(a)).to(device=s.device, dtype=s.dtype)


def _load(env, name, a):
  import torch
  t = getattr(env.engine, name)
  t.copy_(torch.as_tensor(np.ascontiguousarray(a)).to(device=t.device, dtype=t.dtype))
  env.client.state_version += 1


def _sync(env):
  env.engine.synchronize()


def _has_view(env):
  """The HIP engine leaves the last step's outputs in its view; the emulator's driver has no view of a rollout."""
  return env.engine.kernel_name != 'emulated'


def _rollout(env, actions, flags):
  """One recording rollout into NaN / 0xff-poisoned buffers: (obs [K,N,D], reward [K,N], done [K,N]) as float64 / uint8."""
  k = actions.shape[0]
  out = env.engine.rollout_buffers(k)
  out[0].fill_(float('nan')); out[1].fill_(float('nan')); out[2].fill_(255)
  env.engine.rollout(actions, flags, out=out)
  _sync(env)
  return gc._np(out[0]).astype(np.float64), gc._np(out[1]).astype(np.float64), gc._np(out[2]).copy()


def _zeros(env, k):
  return _to(env, np.zeros((k, env.num_envs, abi.NUM_JOINTS)))


def _check(got, want, tol, what):
  assert got.shape == want.shape, (what, got.shape, want.shape)
  err = np.abs(got - want)
  bad = ~(err <= tol)   # (a NaN - a row nobody wrote - fails)
  if bad.any():
    at = np.unravel_index(np.nanargmax(np.where(bad, np.where(np.isnan(err), np.inf, err / np.maximum(tol, 1e-300)), 0)), err.shape)
    raise AssertionError('%s: %d values off, worst at %s: got %r want %r (tol %.3g)' % (what, bad.sum(), at, got[at], want[at], tol[at]))


ANGLE_OBS = ('imu_rad', 'imu_deg', 'bench')
ANGLE_REW = ('upright', 'flat_torso', 'flat_torso_default', 'composite', 'weighted3')


def _reward_tol(dtype, g, want, name, z):
  tol = gc.tolerances(dtype, g, want, angle_derived=name in ANGLE_REW)
  if dtype == 'float32' and name == 'hard_step':
    # (golden_cases.case_reward: inputs within f32 rounding of a step's edge may land on the other side)
    edge = np.minimum(np.abs(z - 0.2), np.abs(z - 0.4)) < 1e-6
    tol = np.where(edge, 1.0, tol)
  return tol


# ---- A. golden states straight through the epilogue ----------------------------------------------------------------------
def golden_pairs():
  """Every observation program x normalize, each with one of the reward programs, so that every entry of golden_cases.REW
  occurs: (obs name, normalize, reward name)."""
  rew = sorted(gc.REW)
  combos = [(o, nrm) for o in sorted(gc.OBS) for nrm in (False, True)]
  assert len(combos) >= len(rew)
  return [(o, nrm, rew[i % len(rew)]) for i, (o, nrm) in enumerate(combos)]


def case_golden_through_epilogue(make_env, obs_name, normalize, rew_name, dtype):
  """The 256 golden states, one fused launch of K steps without physics for every K of launch_lengths: each of the K
  recorded rows, and the engine's view, equal the fixture."""
  g = gc.gold()
  st = gc.golden_state(g)
  n = st.shape[0]
  env = make_env(config=_cfg(dtype, n), normalize_observations=normalize)
  for o in gc.OBS[obs_name](env.robot):
    env.obs_factory.register_observation(o)
  for w, r in gc.REW[rew_name](env):
    env.reward_factory.register_reward(w, r)
  env._ensure_program()
  assert env._fused['obs'] and env._fused['reward']
  gc._load_state(env, st)
  want_o = g[('obsn_' if normalize else 'obs_') + obs_name]
  want_r = g['rew_' + rew_name]
  tol_o = gc.tolerances(dtype, g, want_o, angle_derived=obs_name in ANGLE_OBS)
  tol_r = _reward_tol(dtype, g, want_r, rew_name, g['pos'][:, 2])
  lengths = launch_lengths(dtype)
  assert pass_steps(dtype) + 1 in lengths and 2 * pass_steps(dtype) + 1 in lengths
  for k in lengths:
    assert env.engine.plan(k)['steps_per_launch'] == k and env.engine.plan(k)['launches'] == 1
    if _has_view(env):
      env.engine.obs.fill_(float('nan')); env.engine.reward.fill_(float('nan'))
    obs, rew, _ = _rollout(env, _zeros(env, k), abi.STEP_OBS | abi.STEP_REWARD)
    assert obs.shape == (k, n, want_o.shape[1])
    for s in range(k):
      _check(obs[s], want_o, tol_o, 'K = %d, observations of step %d' % (k, s))
      _check(rew[s], want_r, tol_r, 'K = %d, rewards of step %d' % (k, s))
    if _has_view(env):
      _check(gc._np(env.engine.obs).astype(np.float64), want_o, tol_o, 'K = %d, the view\'s observations' % k)
      _check(gc._np(env.engine.reward).astype(np.float64), want_r, tol_r, 'K = %d, the view\'s rewards' % k)
    np.testing.assert_array_equal(gc._np(env.engine.state).astype(np.float64)[:, :abi.S_RETURN],
                                  st[:, :abi.S_RETURN].astype(np.float32 if dtype == 'float32' else np.float64).astype(np.float64))
  env._close()


def _sarg(q):
  return -2 * (q[:, 0] * q[:, 2] - q[:, 3] * q[:, 1])


def pole_orientations():
  """16 unit quaternions whose sarg is within 1e-6 of +1 (8) and of -1 (8): pitch = +-(pi/2 - d), d = 0 ... 1.3e-3,
  with arbitrary roll and yaw - all of them inside the gimbal branches of getEulerFromQuaternion (|sarg| >= 0.99999)."""
  from gym_solo_amd.core.configs import euler_to_quat
  rng = np.random.default_rng(5)
  out = []
  for sign in (1.0, -1.0):
    for d in (0.0, 1e-8, 1e-5, 1e-4, 3e-4, 6e-4, 1e-3, 1.3e-3):
      out.append(euler_to_quat((rng.uniform(-3, 3), sign * (0.5 * np.pi - d), rng.uniform(-3, 3))))
  q = np.array(out)
  q /= np.linalg.norm(q, axis=1, keepdims=True)
  s = _sarg(q)
  assert (np.abs(s) >= 1 - 1e-6).all() and (s[:8] > 0).all() and (s[8:] < 0).all()
  return q


ROLL = 97


def divergent_batch():
  """(before [288, 32], after [288, 32]): rows 0..255 the golden states and the golden states rolled by 97 rows; rows
  256..271 the synthetic pole orientations (on golden rows' other fields) before a regular golden state; rows 272..287
  the other way round."""
  g = gc.gold()
  st = gc.golden_state(g)
  n = st.shape[0]
  pole = np.abs(_sarg(g['quat'])) >= 0.99999
  idx = np.flatnonzero(pole)
  # the fixture holds two gimbal-pole states; rolled by 97 rows each is once the state before and once the state after
  # the restore, next to a regular one: four pole / regular pairs on neighbouring lanes
  assert len(idx) == 2
  for i in idx:
    assert not pole[(i + ROLL) % n] and not pole[(i - ROLL) % n]
  regular = st[np.flatnonzero(~pole)[:16]]
  syn = regular.copy()
  syn[:, abi.S_QUAT:abi.S_QUAT + 4] = pole_orientations()
  before = np.concatenate([st, syn, regular])
  after = np.concatenate([np.roll(st, -ROLL, axis=0), regular, syn])
  assert (after[:n] == st[(np.arange(n) + ROLL) % n]).all()
  return before, after


def restart_steps(dtype):
  """TimeBased(m): inside a pass, and on the last lane of one (for the source's pass length and for 28 / 32)."""
  return sorted({7, pass_steps(dtype) - 1, (28 if dtype == 'float64' else 32) - 1})


def case_divergent_lanes(make_env, obs_name, normalize, rew_name, dtype, m):
  """One launch of 2 passes + 1 steps without physics, TimeBased(m) with the in-launch auto-reset, the snapshot holding
  OTHER states than the state buffer: steps 0 .. m of a robot record its loaded state, the later steps its snapshot's -
  neighbouring lanes of one wave evaluate a gimbal-pole and a regular orientation, in- and out-of-bounds heights.
  Expected: the fixture's vectors for the golden rows, the oracle's reductions for the synthetic pole orientations."""
  g = gc.gold()
  before, after = divergent_batch()
  n = before.shape[0]
  env = make_env(config=_cfg(dtype, n, auto_reset=True), normalize_observations=normalize)
  for o in gc.OBS[obs_name](env.robot):
    env.obs_factory.register_observation(o)
  for w, r in gc.REW[rew_name](env):
    env.reward_factory.register_reward(w, r)
  env.termination_factory.register_termination(terms.TimeBasedTermination(m))
  env._ensure_program()
  assert env._fused == dict(obs=True, reward=True, done=True)
  import test_oracle_golden as tog
  rew_spec = {'composite': [(1, tog.COMPOSITE)],
              'weighted3': [(0.25, ('upright',)), (-2.0, ('small_control', 10)), (3.0, ('torso_height', 0.33698, 0.025, 0.15))]}
  rspec = rew_spec.get(rew_name) or [(1, tog.REW[rew_name])]

  def expected(states, rolled):
    ng = g['quat'].shape[0]
    gold_o, gold_r = g[('obsn_' if normalize else 'obs_') + obs_name], g['rew_' + rew_name]
    if rolled:
      gold_o, gold_r = np.roll(gold_o, -ROLL, axis=0), np.roll(gold_r, -ROLL, axis=0)
    o = np.concatenate([gold_o, so.observations(states[ng:], tog.OBS[obs_name], normalize_obs=normalize)])
    r = np.concatenate([gold_r, so.factory_reward(states[ng:], rspec)])
    # (the oracle's reductions ARE the fixture on the golden rows: pinned by tests/test_oracle_golden.py, re-checked here)
    np.testing.assert_allclose(so.observations(states[:ng], tog.OBS[obs_name], normalize_obs=normalize), gold_o, rtol=0, atol=1e-13)
    gg = {'quat': states[:, abi.S_QUAT:abi.S_QUAT + 4]}
    return (o, gc.tolerances(dtype, gg, o, angle_derived=obs_name in ANGLE_OBS),
            r, _reward_tol(dtype, gg, r, rew_name, states[:, abi.S_POS + 2]))

  exp = {False: expected(before, False), True: expected(after, True)}
  k = 2 * max(pass_steps(dtype), 28 if dtype == 'float64' else 32) + 1
  assert m < k // 2 and env.engine.plan(k)['launches'] == 1
  _load(env, 'state', before)
  _load(env, 'snapshot', after)
  obs, rew, done = _rollout(env, _zeros(env, k), abi.STEP_OBS | abi.STEP_REWARD | abi.STEP_DONE | abi.STEP_AUTO_RESET)
  for s in range(k):
    o, to, r, tr = exp[s > m]
    _check(obs[s], o, to, 'TimeBased(%d), observations of step %d' % (m, s))
    _check(rew[s], r, tr, 'TimeBased(%d), rewards of step %d' % (m, s))
    np.testing.assert_array_equal(done[s], np.full(n, 1 if (s + 1) % (m + 1) == 0 else 0, dtype=np.uint8), err_msg='step %d' % s)
  # the restore happened (the record is taken before it), and the view holds the last step
  T = np.float32 if dtype == 'float32' else np.float64
  np.testing.assert_array_equal(gc._np(env.engine.state).astype(np.float64)[:, :abi.S_RETURN], after[:, :abi.S_RETURN].astype(T).astype(np.float64))
  if _has_view(env):
    np.testing.assert_array_equal(gc._np(env.engine.obs).astype(np.float64), obs[-1])
    np.testing.assert_array_equal(gc._np(env.engine.reward).astype(np.float64), rew[-1])
    np.testing.assert_array_equal(gc._np(env.engine.done), done[-1])
  # C on a schedule nobody needs physics for: return / length / statistics from the recorded rewards, in step order
  _check_bookkeeping(env, dtype, rew, done, np.zeros(n), np.zeros(n), np.zeros(abi.STATS_WIDTH))
  env._close()


def _random_tree_factory(rng):
  """The generator of tests/test_emu_golden.py's random reward trees (same draws in the same order)."""
  def leaf(env):
    r, k = env.robot, rng.integers(0, 5)
    return [lambda: rewards.UprightReward(r),
            lambda: rewards.FlatTorsoReward(r, hard_margin=float(rng.uniform(0, .3)), soft_margin=float(rng.uniform(0, 2))),
            lambda: rewards.TorsoHeightReward(r, float(rng.uniform(.1, .4)), float(rng.uniform(0, .1)), float(rng.uniform(0, .3))),
            lambda: rewards.HorizontalMoveSpeedReward(r, float(rng.uniform(0, 2)), float(rng.uniform(0, .5)), float(rng.uniform(0, 3))),
            lambda: rewards.SmallControlReward(r, margin=float(rng.uniform(0, 12)))][k]()

  def tree(env, depth):
    if depth == 0 or rng.random() < 0.3:
      return leaf(env)
    if rng.random() < 0.5:
      node = rewards.AdditiveReward()
      node.client = env.client
      for _ in range(rng.integers(1, 4)):
        node.add_term(float(rng.uniform(-2, 2)), tree(env, depth - 1))
      return node
    return rewards.MultiplicitiveReward(float(rng.uniform(-2, 2)), *[tree(env, depth - 1) for _ in range(rng.integers(1, 4))])

  def register(env):
    for _ in range(rng.integers(1, 4)):
      env.reward_factory.register_reward(float(rng.uniform(-3, 3)), tree(env, 2))
  return register


def case_random_trees_through_epilogue(make_env):
  """The 20 seeded random reward trees of test_random_reward_trees_fused_vs_reference_semantics (same seed, same draws)
  through fused f64 launches of 29 and of pass_steps + 1 steps, every recorded row against get_reward_python() at
  rtol = atol = 1e-12; then the generator goes on until a tree compiles to exactly SOLO_MAX_REWARD_OPS instructions (the
  last row of the epilogue's LDS block), which is checked the same way."""
  g = gc.gold()
  st = gc.golden_state(g)[:32]
  rng = np.random.default_rng(11)
  register = _random_tree_factory(rng)
  done, full, tries = 0, 0, 0
  lengths = sorted({29, pass_steps('float64') + 1})
  while done < 20 or full < 1:
    tries += 1
    assert tries < 4000, 'no tree of exactly %d instructions' % abi.MAX_REWARD_OPS
    env = make_env(config=_cfg('float64', st.shape[0]))
    register(env)
    ops = len(env.reward_factory.program())
    if not env.reward_factory.fusable() or (done >= 20 and ops != abi.MAX_REWARD_OPS):
      env._close()
      continue
    env._ensure_program()
    assert env._fused['reward'] and env.engine.program.num_reward_ops == ops
    gc._load_state(env, st)
    python = gc._np(env.reward_factory.get_reward_python()).astype(np.float64)
    for k in lengths:
      _, rew, _ = _rollout(env, _zeros(env, k), abi.STEP_REWARD)
      for s in range(k):
        np.testing.assert_allclose(rew[s], python, rtol=1e-12, atol=1e-12, err_msg='tree %d (%d instructions), K = %d, step %d' % (done, ops, k, s))
    done += 1
    full += ops == abi.MAX_REWARD_OPS
    env._close()
  assert full >= 1


WIDE = ('imu_rad', 'imu_deg', 'imu_rad', 'enc_rad', 'enc_deg_clip', 'enc_clip')   # 3 x 9 + 3 x 12 = 63 elements


def case_widest_observation_program(make_env, dtype, normalize):
  """63 of SOLO_MAX_OBS = 64 elements (9 a + 12 b = 64 has no solution) through launches around the pass length."""
  g = gc.gold()
  st = gc.golden_state(g)
  env = make_env(config=_cfg(dtype, st.shape[0]), normalize_observations=normalize)
  for name in WIDE:
    for o in gc.OBS[name](env.robot):
      env.obs_factory.register_observation(o)
  env._ensure_program()
  assert env._fused['obs'] and env.engine.program.num_obs == 63 == abi.MAX_OBS - 1
  gc._load_state(env, st)
  want = np.concatenate([g[('obsn_' if normalize else 'obs_') + name] for name in WIDE], axis=1)
  tol = np.concatenate([gc.tolerances(dtype, g, g[('obsn_' if normalize else 'obs_') + name], angle_derived=name in ANGLE_OBS)
                        for name in WIDE], axis=1)
  p = pass_steps(dtype)
  for k in (p - 1, p + 1, 2 * p + 1):
    obs, _, _ = _rollout(env, _zeros(env, k), abi.STEP_OBS)
    for s in range(k):
      _check(obs[s], want, tol, 'K = %d, step %d' % (k, s))
  env._close()


def case_full_observation_program_with_foot_forces(make_env, dtype, normalize):
  """SOLO_MAX_OBS = 64 elements on the contact-sensing kernel: 4 x TorsoIMU + 2 x MotorEncoder + FootContact.  A launch
  without physics observes the foot forces the contact record holds: written here (below, inside and above the clip)."""
  g = gc.gold()
  st = gc.golden_state(g)
  n = st.shape[0]
  env = make_env(config=_cfg(dtype, n), normalize_observations=normalize)
  names = ('imu_rad', 'imu_deg', 'imu_deg', 'imu_rad', 'enc_deg_clip', 'enc_clip')
  for name in names:
    for o in gc.OBS[name](env.robot):
      env.obs_factory.register_observation(o)
  env.obs_factory.register_observation(solo_obs.FootContact(env.robot, max_force=20.))
  env._ensure_program()
  assert env._fused['obs'] and env.engine.program.num_obs == abi.MAX_OBS and env.engine.contact_sensing
  gc._load_state(env, st)
  force = np.random.default_rng(8).uniform(-5, 30, (n, 4))
  T = np.float32 if dtype == 'float32' else np.float64
  force = force.astype(T).astype(np.float64)
  contacts = np.zeros((n, abi.MAX_SPHERES, abi.CONTACT_WIDTH))
  contacts[:, 1::4, 3] = force
  c = env.engine.contacts
  c.copy_(_to(env, contacts))
  feet = np.clip(force, 0.0, 20.0)
  if normalize:
    feet = so.normalize(feet, np.zeros(4), np.full(4, 20.0))
  pre = 'obsn_' if normalize else 'obs_'
  want = np.concatenate([g[pre + name] for name in names] + [feet], axis=1)
  tol = np.concatenate([gc.tolerances(dtype, g, g[pre + name], angle_derived=name in ANGLE_OBS) for name in names] +
                       [gc.tolerances(dtype, g, feet, angle_derived=False)], axis=1)
  p = pass_steps(dtype)
  for k in (p, p + 1, 2 * p + 1):
    obs, _, _ = _rollout(env, _zeros(env, k), abi.STEP_OBS)
    for s in range(k):
      _check(obs[s], want, tol, 'K = %d, step %d' % (k, s))
  env._close()


# ---- B / C. physics rollouts against the host reductions of a twin's states ------------------------------------------------
OBS_SPEC = {
  'imu_rad': ('torso_imu', {}),
  'imu_deg': ('torso_imu', dict(degrees=True, max_lin_velocity=5, max_angular_velocity=200.)),
  'enc_rad': ('motor_encoder', {}),
  'enc_deg_clip': ('motor_encoder', dict(degrees=True, max_rotation=100.)),
  'enc_clip': ('motor_encoder', dict(max_rotation=3.0)),
}
STAND = ('multiplicative', 1, [
  ('additive', [(0.5, ('flat_torso', .1, np.pi)), (0.5, ('torso_height', 0.33698, 0.025, 0.15))]),
  ('small_control', 10), ('horizontal_speed', 0, .5, 3)])
REWARD_SPEC = {
  'weighted3': [(0.25, ('upright',)), (-2.0, ('small_control', 10)), (3.0, ('torso_height', 0.33698, 0.025, 0.15))],
  'composite': [(1, STAND)],
  'hard_step+speed': [(1, ('torso_height', 0.3, 0.1, 0.0)), (1, ('horizontal_speed', 1, .1, .5))],
}


def build_observation(env, name):
  kind, kw = OBS_SPEC[name]
  return {'torso_imu': solo_obs.TorsoIMU, 'motor_encoder': solo_obs.MotorEncoder}[kind](env.robot, **kw)


def build_reward(env, node):
  """A reward object of gym_solo_amd.core.rewards from the oracle's tree notation (oracle/solo_oracle.py: reward_node)."""
  r, kind = env.robot, node[0]
  if kind == 'upright':
    return rewards.UprightReward(r)
  if kind == 'flat_torso':
    return rewards.FlatTorsoReward(r, hard_margin=node[1], soft_margin=node[2])
  if kind == 'small_control':
    return rewards.SmallControlReward(r, margin=node[1])
  if kind == 'horizontal_speed':
    return rewards.HorizontalMoveSpeedReward(r, node[1], hard_margin=node[2], soft_margin=node[3])
  if kind == 'torso_height':
    return rewards.TorsoHeightReward(r, node[1], node[2], node[3])
  if kind == 'additive':
    out = rewards.AdditiveReward()
    out.client = env.client
    for c, t in node[1]:
      out.add_term(c, build_reward(env, t))
    return out
  if kind == 'multiplicative':
    return rewards.MultiplicitiveReward(node[1], *[build_reward(env, t) for t in node[2]])
  raise KeyError(kind)


def _program_length(weighted):
  """Instructions the host compiler makes of a weighted list of trees (rewards.py: program())."""
  def ops(node):
    if node[0] == 'additive':
      return sum(ops(t) + 1 for _, t in node[1]) + len(node[1]) - 1
    if node[0] == 'multiplicative':
      return sum(ops(t) for t in node[2]) + len(node[2]) - 1 + 1
    return 1
  return sum(ops(t) + 1 for _, t in weighted) + len(weighted) - 1


def full_length_tree():
  """A seeded random weighted list of trees, in the oracle's notation, that compiles to exactly SOLO_MAX_REWARD_OPS."""
  rng = np.random.default_rng(23)

  def leaf():
    k = rng.integers(0, 5)
    return [lambda: ('upright',),
            lambda: ('flat_torso', float(rng.uniform(0, .3)), float(rng.uniform(.1, 2))),
            lambda: ('torso_height', float(rng.uniform(.1, .4)), float(rng.uniform(0, .1)), float(rng.uniform(0, .3))),
            lambda: ('horizontal_speed', float(rng.uniform(0, 2)), float(rng.uniform(0, .5)), float(rng.uniform(0, 3))),
            lambda: ('small_control', float(rng.uniform(.5, 12)))][k]()

  def tree(depth):
    if depth == 0 or rng.random() < 0.3:
      return leaf()
    if rng.random() < 0.5:
      return ('additive', [(float(rng.uniform(-2, 2)), tree(depth - 1)) for _ in range(rng.integers(1, 4))])
    return ('multiplicative', float(rng.uniform(-2, 2)), [tree(depth - 1) for _ in range(rng.integers(1, 4))])

  for _ in range(4000):
    weighted = [(float(rng.uniform(-3, 3)), tree(2)) for _ in range(rng.integers(1, 4))]
    if _program_length(weighted) == abi.MAX_REWARD_OPS:
      return weighted
  raise AssertionError('no tree of %d instructions' % abi.MAX_REWARD_OPS)


def start_states(dtype, n, seed):
  """n different robots near the settled pose (the oracle's settle loop), perturbed: joint angles, base height, tilt and
  a small twist - on the ground within a few steps, every robot on a trajectory of its own."""
  from helpers import make_abi
  ca, ma = make_abi('float64')
  st = np.tile(so.OraclePhysics(ca, ma).settle(1), (n, 1))
  st[:, abi.S_RETURN:] = 0
  rng = np.random.default_rng(seed)
  st[:, abi.S_Q:abi.S_Q + abi.NUM_DOF] += rng.uniform(-0.4, 0.4, (n, abi.NUM_DOF))
  st[:, abi.S_POS + 2] += rng.uniform(0.0, 0.03, n)
  st[:, abi.S_POS:abi.S_POS + 2] += rng.uniform(-1, 1, (n, 2))
  tilt = rng.uniform(-0.5, 0.5, (n, 3))
  from gym_solo_amd.core.configs import euler_to_quat
  st[:, abi.S_QUAT:abi.S_QUAT + 4] = [euler_to_quat(t) for t in tilt]
  st[:, abi.S_LINVEL:abi.S_LINVEL + 3] = rng.uniform(-0.5, 0.5, (n, 3))
  st[:, abi.S_ANGVEL:abi.S_ANGVEL + 3] = rng.uniform(-1, 1, (n, 3))
  st[:, abi.S_QD:abi.S_QD + abi.NUM_DOF] = rng.uniform(-3, 3, (n, abi.NUM_DOF))
  T = np.float32 if dtype == 'float32' else np.float64
  return st.astype(T).astype(np.float64)


PERIOD = 10   # TimeBased(PERIOD - 1): episodes of 10 steps


def staggered_counters(dtype, n, spl):
  """Initial TimeBased counters per robot so that, with episodes of PERIOD steps, some robot of the batch ends an episode
  at each of these steps of the first launch: the last lane of a pass, the first lane of the next (for the source's pass
  length and for 28 / 32), the launch's last step - and robot 0 (counter 0) twice within every pass."""
  wanted = [0]
  for p in (pass_steps(dtype), 28 if dtype == 'float64' else 32):
    for w in (p - 1, p):
      if w < spl:
        wanted.append((PERIOD - 1 - w) % PERIOD)
  wanted.append((PERIOD - 1 - (spl - 1)) % PERIOD)
  wanted = list(dict.fromkeys(wanted))
  assert n >= len(wanted), 'the batch is too small for the schedule'
  return np.array([wanted[i % len(wanted)] for i in range(n)], dtype=np.int32)


def _assert_schedule_covers(dtype, done, spl):
  """From the expected done flags alone: an episode end at pass position kPass - 1, at kPass, at the launch's last step
  and two within one pass."""
  first = done[:spl].astype(bool)
  p = pass_steps(dtype)
  if p < spl:
    assert first[p - 1].any() and first[p].any()
  assert first[spl - 1].any()
  assert (first[:min(p, spl)].sum(axis=0) >= 2).any()


def case_physics_rollout(make_env, dtype, n, spl, k, obs_names, normalize, reward, flags=abi.STEP_ALL, seed=0, streams=1,
                         migrate=0, extra=None, action_scale=2 * np.pi):
  """A fused recording rollout with in-kernel auto-reset against the oracle's reductions of a twin engine's states (module
  docstring, B), the episodic bookkeeping against a host loop over the recorded rewards (C)."""
  import torch
  extra = dict(extra or {})
  T = np.float32 if dtype == 'float32' else np.float64
  want_done = bool(flags & abi.STEP_DONE)
  weighted = REWARD_SPEC[reward] if isinstance(reward, str) else reward

  env = make_env(config=_cfg(dtype, n, auto_reset=True, steps_per_launch=spl, rollout_streams=streams, migrate_steps=migrate, **extra),
                 normalize_observations=normalize)
  for name in obs_names:
    env.obs_factory.register_observation(build_observation(env, name))
  for w, node in weighted:
    env.reward_factory.register_reward(w, build_reward(env, node))
  env.termination_factory.register_termination(terms.TimeBasedTermination(PERIOD - 1))
  env._ensure_program()
  assert env._fused == dict(obs=True, reward=True, done=True)
  assert env.engine.program.num_reward_ops == _program_length(weighted)
  plan = env.engine.plan(k)
  assert plan['steps_per_launch'] == spl and plan['launches'] == -(-k // spl)
  twin = make_env(config=_cfg(dtype, n, auto_reset=False, **extra))
  if 'control_mode' in extra:
    assert env.engine.control['mode'] == twin.engine.control['mode'] == extra['control_mode']
  if extra.get('contact_sensing'):
    assert env.engine.contact_sensing

  start = start_states(dtype, n, seed)
  count = staggered_counters(dtype, n, spl) if want_done else np.zeros(n, dtype=np.int32)
  tc = np.zeros((n, abi.MAX_TERMS), dtype=np.int32)
  tc[:, 0] = count
  ret0, len0 = np.arange(n) * 0.25, np.arange(n) % 7.0   # (the accumulators a launch finds in the record)
  for e in (env, twin):
    _load(e, 'state', start)
    _load(e, 'snapshot', start)
  st0 = start.copy()
  st0[:, abi.S_RETURN], st0[:, abi.S_EPLEN] = ret0, len0
  _load(env, 'state', st0)
  env.engine.term_count.copy_(torch.as_tensor(tc).to(env.engine.term_count.device))
  stats0 = gc._np(env.engine.stats).astype(np.float64).copy()
  rng = np.random.default_rng(100 + seed)
  acts = rng.uniform(-action_scale, action_scale, (k, n, abi.NUM_JOINTS)).astype(T).astype(np.float64)

  # the twin: one STEP_PHYSICS launch per step, the host keeps the TimeBased counters and resets with a mask
  states = np.zeros((k, n, abi.STATE_STRIDE))
  done_want = np.zeros((k, n), dtype=np.uint8)
  a_t = _to(twin, acts)
  for s in range(k):
    twin.engine.step(a_t[s], abi.STEP_PHYSICS)
    _sync(twin)
    states[s] = gc._np(twin.engine.state).astype(np.float64)
    if want_done:
      count += 1
      fired = count > PERIOD - 1
      done_want[s] = fired
      if fired.any():
        twin.engine.reset(torch.as_tensor(fired.astype(np.uint8)).to(twin.engine.state.device))
        count[fired] = 0
  assert np.isfinite(states).all()
  if want_done:
    _assert_schedule_covers(dtype, done_want, spl)

  obs, rew, done = _rollout(env, _to(env, acts), flags)
  # the premise of the bars: the two runs' physics is bit-identical (if not, that is a finding of its own - stop here)
  _sync(twin)
  np.testing.assert_array_equal(gc._np(env.engine.state).astype(np.float64)[:, :abi.S_RETURN],
                                gc._np(twin.engine.state).astype(np.float64)[:, :abi.S_RETURN])
  assert gc._np(env.engine.stats)[5] == 0   # (nobody diverged)
  flat = states.reshape(k * n, abi.STATE_STRIDE)
  gg = {'quat': flat[:, abi.S_QUAT:abi.S_QUAT + 4]}
  if flags & abi.STEP_OBS:
    want = so.observations(flat, [OBS_SPEC[name] for name in obs_names], normalize_obs=normalize)
    tol = gc.tolerances(dtype, gg, want, angle_derived=any(OBS_SPEC[name][0] == 'torso_imu' for name in obs_names))
    _check(obs.reshape(k * n, -1), want, tol, 'observations [step x robot]')
  if flags & abi.STEP_REWARD:
    want = so.factory_reward(flat, weighted)
    tol = gc.tolerances(dtype, gg, want, angle_derived=True)
    if dtype == 'float32' and reward == 'hard_step+speed':
      z = flat[:, abi.S_POS + 2]
      tol = np.where(np.minimum(np.abs(z - 0.2), np.abs(z - 0.4)) < 1e-6, 1.0, tol)
    _check(rew.reshape(k * n), want, tol, 'rewards [step x robot]')
  if want_done:
    np.testing.assert_array_equal(done, done_want)
    np.testing.assert_array_equal(gc._np(env.engine.term_count)[:, 0], count)
  if _has_view(env):
    if flags & abi.STEP_OBS:
      np.testing.assert_array_equal(gc._np(env.engine.obs).astype(np.float64), obs[-1])
    if flags & abi.STEP_REWARD:
      np.testing.assert_array_equal(gc._np(env.engine.reward).astype(np.float64), rew[-1])
    if want_done:
      np.testing.assert_array_equal(gc._np(env.engine.done), done[-1])
  if (flags & abi.STEP_REWARD) and want_done:
    _check_bookkeeping(env, dtype, rew, done_want, ret0, len0, stats0)
  else:
    # no bookkeeping: slots 29, 30 of the records and the statistics do not move
    got = gc._np(env.engine.state).astype(np.float64)
    np.testing.assert_array_equal(got[:, abi.S_RETURN], ret0.astype(T).astype(np.float64))
    np.testing.assert_array_equal(got[:, abi.S_EPLEN], len0.astype(T).astype(np.float64))
    np.testing.assert_array_equal(gc._np(env.engine.stats).astype(np.float64), stats0)
  env._close()
  twin._close()


def _check_bookkeeping(env, dtype, rew, done, ret0, len0, stats0):
  """C: SOLO_S_RETURN / SOLO_S_EPLEN equal a host loop over the recorded rewards and the event schedule in step order, in
  the engine's precision (IEEE scalar adds: bit equality); the statistics (double atomics in any robot order) at 1e-12."""
  T = np.float32 if dtype == 'float32' else np.float64
  k, n = rew.shape
  ret, ln = ret0.astype(T), len0.astype(T)
  stats = np.zeros(4)
  one = T(1)
  for s in range(k):
    ret = (ret + rew[s].astype(T)).astype(T)
    ln = (ln + one).astype(T)
    ended = done[s].astype(bool)   # (auto-reset on: every done step restarts)
    x = ret[ended].astype(np.float64)
    stats += [x.sum(), (x * x).sum(), ended.sum(), ln[ended].astype(np.float64).sum()]
    ret[ended] = 0
    ln[ended] = 0
  got = gc._np(env.engine.state).astype(np.float64)
  np.testing.assert_array_equal(got[:, abi.S_RETURN], ret.astype(np.float64))
  np.testing.assert_array_equal(got[:, abi.S_EPLEN], ln.astype(np.float64))
  got_stats = gc._np(env.engine.stats).astype(np.float64) - stats0
  np.testing.assert_allclose(got_stats[:4], stats, rtol=1e-12, atol=0)
  assert got_stats[2] == done.astype(bool).sum()
