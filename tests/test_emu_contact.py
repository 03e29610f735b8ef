"""The contact-sensing step kernels (solo_contact_kernel) on the CPU wave emulator - the product kernel source, run without a
GPU (tests/emu/emu_contact_harness.cpp, built here with the flags of tests/emu/Makefile) - in position, torque and PD
control, on the flat plane, the 10-degree incline and the stairs:
  (a) one-step per-sphere parity: from identical states the record equals f_s = sum over the sphere's rows of lam_r d_r / dt
      from OraclePhysics.step_debug (d_r: the base-translation block of the row's Jacobian, rotated to world; first confirmed
      on flat ground, where the normal is world z).  Torque and PD run the oracle identity of tests/test_emu_control.py: a
      saturated torque s L (PD: kp = 1e3, kd = 0, targets s 1e3 rad) is the oracle's position motor driven to saturation;
  (b) the spheres with a non-zero record are the ones with a live contact row in the oracle's step;
  (c) a robot in the air reads all zeros."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from gym_solo_amd import abi
from gym_solo_amd.model import DOF_TO_JOINT
from helpers import incline_terrain, make_abi, stairs_terrain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, 'tests', 'emu')
N = 12
MODES = ('position', 'torque', 'pd')


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
  out = str(tmp_path_factory.mktemp('emu_contact') / 'libsolo_emu_contact.so')
  # (the flags of tests/emu/Makefile's libsolo_emu.so)
  subprocess.check_call(['g++', '-O2', '-g', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-Wall', '-Wno-unknown-pragmas',
                         '-Wno-unused-variable', '-Wno-unused-but-set-variable', '-Wno-unused-function', '-DSOLO_QUEUE_SPINS=64',
                         '-o', out, os.path.join(EMU, 'emu_contact_harness.cpp')])
  lib = C.CDLL(out)
  lib.solo_emu_contact_rollout.restype = C.c_int
  lib.solo_emu_contact_rollout.argtypes = [C.POINTER(abi.SoloConfig), C.POINTER(abi.SoloModel), C.POINTER(abi.SoloControl),
                                           C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6
  return lib


def _dp(a):
  assert a.dtype == np.float64 and a.flags['C_CONTIGUOUS']
  return a.ctypes.data


def _control(mode, kp=None, kd=None, action_scale=1.0):
  c = abi.SoloControl()
  c.mode, c.action_scale = mode, action_scale
  for d in range(abi.NUM_DOF):
    c.kp[d] = 0.0 if kp is None else kp[d]
    c.kd[d] = 0.0 if kd is None else kd[d]
  return c


def _step(lib, ca, ma, ctl, terrain, state, actions, params):
  """one physics-only step with actions [N, 12] (the motor commands); state [N, 32] in place; returns the record [N, 16, 4]"""
  n = state.shape[0]
  a = np.ascontiguousarray(actions[None], dtype=np.float64)
  targets = np.zeros((n, abi.NUM_JOINTS))
  stats = np.zeros((abi.STATS_SHARDS, abi.STATS_WIDTH))
  rec = np.zeros((n, abi.MAX_SPHERES, abi.CONTACT_WIDTH))
  rc = lib.solo_emu_contact_rollout(C.byref(ca), C.byref(ma), C.byref(ctl), C.addressof(terrain) if terrain is not None else None,
                                    ca.dtype, n, 1, _dp(state), _dp(a), _dp(targets), _dp(params), _dp(stats), _dp(rec))
  assert rc == 0
  assert stats[:, 5].sum() == 0   # (nothing diverged)
  return rec


def _rot(q):
  x, y, z, w = q
  return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                   [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                   [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _oracle_forces(dbg, state, dt):
  out = np.zeros((abi.MAX_SPHERES, 4))
  rot = _rot(state[abi.S_QUAT:abi.S_QUAT + 4])
  live = {}
  for r in range(dbg.num_rows):
    s = dbg.row_sphere[r]
    if s < 0:
      continue
    d = rot @ np.array([dbg.J[r][3], dbg.J[r][4], dbg.J[r][5]])
    out[s, :3] += dbg.lam[r] * d / dt
    if s not in live:   # (the first row of a sphere is its normal row)
      out[s, 3] = dbg.lam[r] / dt
      live[s] = d
  return out, live


def _ground_states(ph, ca, n, seed):
  """robots on the ground in flailing poses: the oracle's settle, then a few steps of random targets"""
  st = np.tile(ph.settle(1), (n, 1))
  rng = np.random.default_rng(seed)
  for _ in range(15):
    ph.step(st, rng.uniform(-0.6, 0.6, (n, abi.NUM_JOINTS)) / ca.action_scale)
  return st


def _oracle_after(ph, st0, tg, params):
  out = st0.copy()
  for e in range(out.shape[0]):
    ph.step_debug(out[e], tg[e][DOF_TO_JOINT].copy(), params[e].copy())
  return out


@pytest.mark.parametrize('ground', ['flat', 'incline', 'stairs'])
def test_one_step_record_parity_and_live_set(lib, ground):
  _one_step_record_parity_and_live_set(lib, ground, make_abi('float64')[1])


@pytest.mark.parametrize('ground', ['flat', 'incline'])
@pytest.mark.parametrize('case', ['upper_spheres', 'seed0'])
def test_one_step_record_parity_and_live_set_on_model(lib, ground, case):
  """(a), (b) on models whose sphere -> link layout is not the default's (tests/model_space.py): sphere 4l of every leg on the
  UPPER link, and a random model (one knee sphere on an upper link, every sphere moved and resized) - the record's sphere ->
  link mapping and its forces must follow the model; an upper-link sphere is among the touching ones"""
  import model_space
  ma = model_space.get_model(case).to_abi()
  upper = [s for s in range(abi.MAX_SPHERES) if ma.sphere_body[s] != 0 and ma.sphere_body[s] % 2 == 1]
  assert _one_step_record_parity_and_live_set(lib, ground, ma) & set(upper)


def _one_step_record_parity_and_live_set(lib, ground, ma):
  """returns the set of spheres that touched on some robot"""
  from oracle import solo_oracle as so
  ca, _ = make_abi('float64')
  touched = set()
  terrain = {'flat': None, 'incline': incline_terrain(), 'stairs': stairs_terrain()}[ground]
  ph = so.OraclePhysics(ca, ma, terrain=terrain)
  st0 = _ground_states(ph, ca, N, seed=3)
  params = np.zeros((N, 4))
  params[:, 0], params[:, 1] = ca.lateral_friction, 1.0
  params[N // 2:, 0], params[N // 2:, 1] = 0.4, 1.15   # (half the robots with their own friction and base mass)
  L = ca.motor_torque_limit
  sgn = np.random.default_rng(4).choice([-1.0, 1.0], (N, abi.NUM_JOINTS))
  worst, touching = 0.0, 0
  for mode in MODES:
    if mode == 'position':
      acts = np.random.default_rng(5).uniform(-0.6, 0.6, (N, abi.NUM_JOINTS))
      ctl, tg = _control(abi.CTRL_POSITION, action_scale=ca.action_scale), acts * ca.action_scale
    elif mode == 'torque':
      ctl, acts, tg = _control(abi.CTRL_TORQUE), sgn * L, sgn * 1e3
    else:
      ctl, acts, tg = _control(abi.CTRL_PD, np.full(8, 1e3), np.zeros(8)), sgn * 1e3, sgn * 1e3
    st = st0.copy()
    rec = _step(lib, ca, ma, ctl, terrain, st, acts, params)
    for e in range(N):
      dbg = ph.step_debug(st0[e].copy(), tg[e][DOF_TO_JOINT].copy(), params[e].copy())
      want, live = _oracle_forces(dbg, st0[e], ca.dt)
      if ground == 'flat':
        for d in live.values():   # (the reading of the Jacobian, confirmed where the basis is known: the normal is z)
          np.testing.assert_allclose(d, [0.0, 0.0, 1.0], atol=1e-12)
      for s in range(abi.MAX_SPHERES):
        if s not in live:
          assert np.all(rec[e, s] == 0), (mode, e, s, rec[e, s])     # (b)
        elif want[s, 3] > 1e-9:
          assert rec[e, s, 3] > 0, (mode, e, s)                       # (b)
      worst = max(worst, float(np.abs(rec[e] - want).max()))
      touching += len(live)
      touched |= set(live)
    # (the step itself is the oracle's: the identity holds)
    np.testing.assert_allclose(st[:, :abi.S_RETURN], _oracle_after(ph, st0, tg, params)[:, :abi.S_RETURN], rtol=0, atol=1e-9)
  print('emu contact parity ({}): worst |df| = {:.3e} N over {} touching sphere-steps'.format(ground, worst, touching))
  assert touching > 3 * N
  assert worst < 1e-6
  return touched


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_a_robot_in_the_air_reads_zeros(lib, dtype):
  from oracle import solo_oracle as so
  ca, ma = make_abi(dtype)
  ph = so.OraclePhysics(make_abi('float64')[0], ma)
  st = np.tile(ph.settle(1), (N, 1))
  st[:, abi.S_POS + 2] += 1.0
  params = np.zeros((N, 4))
  params[:, 0], params[:, 1] = ca.lateral_friction, 1.0
  for mode, m in (('position', abi.CTRL_POSITION), ('torque', abi.CTRL_TORQUE), ('pd', abi.CTRL_PD)):
    ctl = _control(m, np.full(8, 2.0), np.full(8, 0.05), ca.action_scale if mode == 'position' else 1.0)
    rec = _step(lib, ca, ma, ctl, None, st.copy(), np.random.default_rng(2).uniform(-1, 1, (N, abi.NUM_JOINTS)), params)
    assert np.all(rec == 0), mode
