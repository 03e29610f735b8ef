"""The joint-control step kernels (solo_ctl_step_kernel: torque / PD) on the CPU wave emulator - the product kernel
source, run without a GPU (tests/emu/emu_control_harness.cpp, built here with the flags of tests/emu/Makefile).
  (a) zero torque == OraclePhysics with motor_torque_limit = 0, 60 steps from the settled snapshot (the robot collapses:
      contact rows live);
  (b) saturated torque tau = s L (s = +-1 per robot, step and joint) == the oracle's position motors driven to saturation
      (targets s 1e3 rad), 60 steps on the ground, half the robots with their own friction and base mass;
  (c) arbitrary torque in the air (random q, qd, base twist and orientation; no contact or limit row live):
      engine_torque(S, tau) - oracle_motors_off(S) == dt (fd(S, tau) - fd(S, 0)) with the oracle's independent CRBA / RNEA
      forward dynamics - for torque commands and for the PD law at random gains (tau computed on the host from S);
  (d) a PD step == a torque step fed the PD law's torque computed on the host from the same state;
  (e) position mode through the new harness == tests/emu_kernel.py's driver, bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from gym_solo_amd import abi
from gym_solo_amd.model import DOF_TO_JOINT
from control_cases import air_identity_errors, air_states
from helpers import make_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, 'tests', 'emu')
N = 32


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
  out = str(tmp_path_factory.mktemp('emu_ctl') / 'libsolo_emu_control.so')
  # (the flags of tests/emu/Makefile's libsolo_emu.so)
  subprocess.check_call(['g++', '-O2', '-g', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-Wall', '-Wno-unknown-pragmas',
                         '-Wno-unused-variable', '-Wno-unused-but-set-variable', '-Wno-unused-function', '-DSOLO_QUEUE_SPINS=64',
                         '-o', out, os.path.join(EMU, 'emu_control_harness.cpp')])
  lib = C.CDLL(out)
  lib.solo_emu_ctl_rollout.restype = C.c_int
  lib.solo_emu_ctl_rollout.argtypes = [C.POINTER(abi.SoloConfig), C.POINTER(abi.SoloModel), C.POINTER(abi.SoloControl), C.c_int,
                                       C.c_int, C.c_int] + [C.c_void_p] * 6
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


def _run(lib, ca, ma, ctl, state, actions, params=None):
  """actions [K, N, 12]: one fused physics-only launch of K steps; state [N, 32] in place."""
  n = state.shape[0]
  a = np.ascontiguousarray(actions, dtype=np.float64)
  snapshot = state.copy()
  targets = np.zeros((n, abi.NUM_JOINTS))
  if params is None:
    params = np.zeros((n, 4))
    params[:, 0], params[:, 1] = ca.lateral_friction, 1.0
  stats = np.zeros((abi.STATS_SHARDS, abi.STATS_WIDTH))
  rc = lib.solo_emu_ctl_rollout(C.byref(ca), C.byref(ma), C.byref(ctl), ca.dtype, n, a.shape[0], _dp(state), _dp(snapshot), _dp(a),
                                _dp(targets), _dp(params), _dp(stats))
  assert rc == 0
  assert stats[:, 5].sum() == 0   # (nothing diverged)
  return state


@pytest.fixture(scope='module')
def settled():
  from oracle import solo_oracle as so
  ca, ma = make_abi('float64')
  return np.tile(so.OraclePhysics(ca, ma).settle(1), (N, 1))


MODEL_CASES = ['seed0', 'seed1', 'offdiag_legs']   # (tests/model_space.py; the tests without a model parameter run the default)


def _model(case):
  import model_space
  return model_space.get_model(case).to_abi()


def test_zero_torque_equals_oracle_with_motors_off(lib, settled):
  _zero_torque_equals_oracle_with_motors_off(lib, settled, make_abi('float64')[1])


@pytest.mark.parametrize('case', MODEL_CASES)
def test_zero_torque_equals_oracle_with_motors_off_on_model(lib, case):
  """(a) on random models and on off-diagonal link inertias, from that model's own settled snapshot"""
  from oracle import solo_oracle as so
  ma = _model(case)
  _zero_torque_equals_oracle_with_motors_off(lib, np.tile(so.OraclePhysics(make_abi('float64')[0], ma).settle(1), (N, 1)), ma)


def _zero_torque_equals_oracle_with_motors_off(lib, settled, ma):
  from oracle import solo_oracle as so
  ca, _ = make_abi('float64')
  ca0, _ = make_abi('float64', motor_torque_limit=0.0)
  st = settled.copy()
  _run(lib, ca, ma, _control(abi.CTRL_TORQUE), st, np.zeros((60, N, abi.NUM_JOINTS)))
  ref = settled.copy()
  ph = so.OraclePhysics(ca0, ma)
  tg = np.tile(np.array(list(ca.settle_targets)), (N, 1))
  for _ in range(60):
    ph.step(ref, tg)
  assert ref[:, abi.S_POS + 2].max() < 0.2
  np.testing.assert_allclose(st[:, :abi.S_RETURN], ref[:, :abi.S_RETURN], rtol=0, atol=1e-9)


def test_pd_step_equals_torque_step_fed_the_host_torque(lib, settled):
  ca, ma = make_abi('float64')
  rng = np.random.default_rng(5)
  kp, kd = rng.uniform(1.0, 4.0, abi.NUM_DOF), rng.uniform(0.01, 0.05, abi.NUM_DOF)
  pd, tq = _control(abi.CTRL_PD, kp, kd), _control(abi.CTRL_TORQUE)
  L = ca.motor_torque_limit
  st = settled.copy()
  settle = np.array(list(ca.settle_targets))
  worst = 0.0
  for k in range(30):
    a = settle[None, :] + rng.uniform(-0.5, 0.5, (N, abi.NUM_JOINTS))
    S = st.copy()
    _run(lib, ca, ma, pd, st, a[None])
    if k % 10 == 0:
      q, qd = S[:, abi.S_Q:abi.S_Q + 8], S[:, abi.S_QD:abi.S_QD + 8]
      tau = np.clip(kp * (a[:, DOF_TO_JOINT] - q) - kd * qd, -L, L)
      tj = np.zeros((N, abi.NUM_JOINTS))
      tj[:, DOF_TO_JOINT] = tau
      _run(lib, ca, ma, tq, S, tj[None])
      worst = max(worst, np.abs(S[:, :abi.S_RETURN] - st[:, :abi.S_RETURN]).max())
  assert worst <= 1e-13, worst


def test_position_mode_through_the_new_harness_is_bit_identical(lib, settled):
  from emu_kernel import EmuEngine
  ca, ma = make_abi('float64')
  rng = np.random.default_rng(1)
  acts = rng.uniform(-6, 6, (10, 8, abi.NUM_JOINTS))
  st = settled[:8].copy()
  _run(lib, ca, ma, _control(abi.CTRL_POSITION, action_scale=ca.action_scale), st, acts)
  e = EmuEngine(ca, ma, 8)
  e.state[:] = settled[:8]
  e.snapshot[:] = settled[:8]
  e.rollout(acts, abi.STEP_PHYSICS)
  np.testing.assert_array_equal(st, e.state)


def _limit_distance(ma, st):
  q = st[:, abi.S_Q:abi.S_Q + abi.NUM_DOF]
  lo, hi = np.array(list(ma.joint_lower)), np.array(list(ma.joint_upper))
  return np.min(np.minimum(q - lo, hi - q))


def test_saturated_torque_equals_oracle_with_saturated_motors(lib, settled):
  from oracle import solo_oracle as so
  ca, ma = make_abi('float64')
  rng = np.random.default_rng(3)
  params = np.zeros((N, 4))
  params[:, 0], params[:, 1] = ca.lateral_friction, 1.0
  half = np.arange(N) % 2 == 1
  params[half, 0] = rng.uniform(0.2, 1.2, half.sum())
  params[half, 1] = rng.uniform(0.7, 1.3, half.sum())
  s = rng.choice([-1.0, 1.0], (60, N, abi.NUM_JOINTS))
  st = settled.copy()
  _run(lib, ca, ma, _control(abi.CTRL_TORQUE), st, s * ca.motor_torque_limit, params)
  ref = settled.copy()
  ph = so.OraclePhysics(ca, ma)
  for k in range(60):
    ph.step(ref, s[k] * 1e3 / ca.action_scale, params)
    assert _limit_distance(ma, ref) > ca.joint_limit_margin   # (limit rows interleave with motor rows: none may be live)
  np.testing.assert_allclose(st[:, :abi.S_RETURN], ref[:, :abi.S_RETURN], rtol=0, atol=1e-9)


@pytest.mark.parametrize('mode', ['torque', 'pd'])
def test_arbitrary_torque_in_the_air_equals_forward_dynamics(lib, mode):
  _arbitrary_torque_in_the_air(lib, mode, make_abi('float64')[1], own_limits=False)


@pytest.mark.parametrize('mode', ['torque', 'pd'])
@pytest.mark.parametrize('case', MODEL_CASES)
def test_arbitrary_torque_in_the_air_equals_forward_dynamics_on_model(lib, mode, case):
  """(c) on random models and on off-diagonal link inertias: nothing but the inertia terms acts, so this is the sharpest check
  of them (1e-12; the random models' joint limits are at least 2 rad out, the air states' angles up to 3 rad - a live limit
  row would break the identity, so the angles are drawn inside the model's own limits)"""
  _arbitrary_torque_in_the_air(lib, mode, _model(case))


def _arbitrary_torque_in_the_air(lib, mode, ma, own_limits=True):
  from oracle import solo_oracle as so
  ca, _ = make_abi('float64')
  ca0, _ = make_abi('float64', motor_torque_limit=0.0)
  rng = np.random.default_rng(11 if mode == 'torque' else 12)
  S = air_states(rng, N, ma if own_limits else None, ca.joint_limit_margin)
  L = ca.motor_torque_limit
  if mode == 'torque':
    tau = rng.uniform(-0.99 * L, 0.99 * L, (N, abi.NUM_DOF))
    a = np.zeros((N, abi.NUM_JOINTS))
    a[:, DOF_TO_JOINT] = tau
    ctl = _control(abi.CTRL_TORQUE)
  else:
    kp, kd = rng.uniform(1.0, 4.0, abi.NUM_DOF), rng.uniform(0.01, 0.05, abi.NUM_DOF)
    a = rng.uniform(-3, 3, (N, abi.NUM_JOINTS))
    q, qd = S[:, abi.S_Q:abi.S_Q + 8], S[:, abi.S_QD:abi.S_QD + 8]
    tau = np.clip(kp * (a[:, DOF_TO_JOINT] - q) - kd * qd, -L, L)
    ctl = _control(abi.CTRL_PD, kp, kd)
  got = S.copy()
  _run(lib, ca, ma, ctl, got, a[None])
  ref = S.copy()
  ph0 = so.OraclePhysics(ca0, ma)
  ph0.step(ref, np.zeros((N, abi.NUM_JOINTS)))
  worst_qd, worst_twist = air_identity_errors(S, got, ref, tau, so.OraclePhysics(ca, ma), ca.dt)
  assert worst_qd <= 1e-12 and worst_twist <= 1e-12, (worst_qd, worst_twist)
  assert np.abs(got[:, abi.S_QD:abi.S_QD + 8] - ref[:, abi.S_QD:abi.S_QD + 8]).max() > 1e-3   # (tau did something)
