"""tests/dynamics_cases.py on the CPU: the kinematics-only reference validated against ITSELF (Newton-Euler for the robot as a whole
and the power balance along its own solution, without forming M; longdouble against mpmath at 50 digits), then the oracle held to
it - forward_dynamics (both outputs: CRBA + RNEA and ABA) on every model of the family, one oracle step in the air in position mode
(the motors are internal, against an M the oracle did not supply), and the pose update of its quat_integrate.  Every test prints the
worst residual / budget."""
import numpy as np
import pytest

import closed_form_cases as cf
import dynamics_cases as dc
from gym_solo_amd import abi
from oracle import solo_oracle as so


class Oracle:
  """dynamics_cases' engine interface on the CPU oracle (float64, position mode: it has no other)"""

  def open(self, ca, ma, n, mode, scales, gains=None, actuators=None):
    assert mode == 'position' and actuators is None
    params = np.zeros((n, 4))
    params[:, 0], params[:, 1] = ca.lateral_friction, scales
    return so.OraclePhysics(ca, ma), params

  def run(self, h, state, acts):
    ph, params = h
    st = np.ascontiguousarray(state, dtype=np.float64).copy()
    for a in acts:
      ph.step(st, a, params)
    assert np.isfinite(st).all()
    return st

  def close(self, h):
    pass


def _torques(G, rng, n):
  return rng.uniform(-0.99 * G.limit, 0.99 * G.limit, (n, abi.NUM_DOF))


@pytest.mark.parametrize('damping', [True, False], ids=['damped', 'undamped'])
@pytest.mark.parametrize('model', dc.MODELS)
def test_the_reference_satisfies_newton_euler_and_the_power_balance(model, damping):
  """six equations for the robot as a whole and d/dt of the kinetic energy, along x_0 + xd t + xdd t^2 / 2 with the reference's own
  xdd: 1e-16 of the sum of the absolute terms each"""
  kw = {} if damping else dict(linear_damping=0.0, angular_damping=0.0)
  ca, ma, G, S, scales, rng = dc.case_setup('float64', model, 8, 31, **kw)
  tau = _torques(G, rng, 8)
  A = dc.Algebra()
  acc = dc.accelerations(A, G.ma, G.K, S, tau, scales)
  lin, ang, power = dc.newton_euler_residuals(A, G.ma, G.K, S, tau, scales, acc.xdd)
  print('reference | %s | Newton %.1e, Euler %.1e, power %.1e of the sum of absolute terms' % (model, lin.max(), ang.max(), power.max()))
  assert lin.max() < 1e-16 and ang.max() < 1e-16 and power.max() < 1e-16


@pytest.mark.parametrize('model', ['default', 'seed0'])
def test_the_longdouble_reference_agrees_with_mpmath_at_50_digits(model):
  """the same jets on mpmath numbers, 5 states per model: xdd agrees to 1e-3 of the f64 budget of the dynamics residual"""
  import mpmath
  n = 5
  ca, ma, G, S, scales, rng = dc.case_setup('float64', model, n, 32)
  tau = _torques(G, rng, n)
  A = dc.Algebra()
  acc = dc.accelerations(A, G.ma, G.K, S, tau, scales)
  with mpmath.workdps(50):
    B = dc.Algebra(mpmath)
    ref = dc.accelerations(B, G.ma, G.K, S, tau, scales)
    diff = B.f64(abs(_to_mp(B, acc.xdd) - ref.xdd))
    lin, ang, power = dc.newton_euler_residuals(B, G.ma, G.K, S, tau, scales, ref.xdd)
  S_k = A.f64(abs(acc.xd) + A.num(G.K.dt) * dc._mv(abs(acc.Minv), acc.terms))
  bud = dc._blocks(cf.budget('float64', 'dyn_user', S_k))
  worst = (G.K.dt * diff / bud).max()
  print('reference | %s | longdouble against mpmath: %.2e of the f64 budget; mpmath Newton %.1e, Euler %.1e, power %.1e' % (
    model, worst, lin.max(), ang.max(), power.max()))
  assert worst < 1e-3
  assert max(lin.max(), ang.max(), power.max()) < 1e-40


def _to_mp(B, a):
  """a longdouble array as mpmath numbers, exactly (high and low float64 parts)"""
  hi = np.asarray(a, dtype=np.float64)
  lo = np.asarray(a - hi.astype(np.longdouble), dtype=np.float64)
  return B.num(hi) + B.num(lo)


@pytest.mark.parametrize('model', dc.MODELS)
def test_forward_dynamics_against_the_reference(model):
  """both outputs (CRBA + RNEA, ABA) in world coordinates against xdd_ref at the f64 budget of a step: random airborne states,
  damping on, random tau, base-mass scale U(0.8, 1.2)"""
  n = 12
  ca, ma, G, S, scales, rng = dc.case_setup('float64', model, n, 33)
  tau = _torques(G, rng, n)
  ph = so.OraclePhysics(ca, ma)
  pose = cf.unit_pose(S)
  out = [ph.forward_dynamics(pose[e].copy(), tau[e], float(scales[e])) for e in range(n)]
  report = []
  for k, name in enumerate(('CRBA + RNEA', 'ABA')):
    xdd = dc.oracle_world_accelerations(S, np.array([o[k] for o in out]))
    A = dc.Algebra()
    acc = dc.accelerations(A, G.ma, G.K, S, tau, scales)
    res = A.f64(A.num(G.K.dt) * abs(A.num(xdd) - acc.xdd))
    bud = dc._blocks(cf.budget('float64', 'dyn_user', A.f64(abs(acc.xd) + A.num(G.K.dt) * dc._mv(abs(acc.Minv), acc.terms))))
    report += [dc._entry(name + ', joint rates', [(res[:, 6:], bud[:, 6:])], 'rad/s'), dc._entry(name + ', base twist', [(res[:, :6], bud[:, :6])], 'rad/s | m/s')]
  dc.show('oracle', 'forward_dynamics, ' + model, report)
  dc.assert_within_budget(report)


@pytest.mark.parametrize('model', ['default', 'seed0'])
def test_one_oracle_step_in_position_mode_keeps_the_motors_internal(model):
  report = dc.position(Oracle(), 'float64', model, 12)
  dc.show('oracle', 'position, ' + model, report)
  dc.assert_within_budget(report)


def test_the_oracles_pose_update():
  report = dc.pose(Oracle(), 'float64', 4, mode='position')
  dc.show('oracle', 'pose', report)
  dc.assert_within_budget(report)
