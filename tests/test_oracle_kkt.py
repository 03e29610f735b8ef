"""tests/kkt_cases.py on the CPU oracle: the measuring device validated against the oracle's own kinematics, then the oracle's
solved step - the first thing held to the per-row conditions - in scenarios (a) ... (e), position mode (the oracle has no other).
The oracle runs solver_iterations plain sweeps and keeps no sweep count: a robot-step takes the conditional checks if ONE MORE
sweep moves no impulse by more than k half-ulps (k = the f64 engine's solver_ulp_tolerance) - what "the iteration left through no
row pending" means for the kernels."""
import ctypes as C

import numpy as np
import pytest

import contact_cases
import kkt_cases as kc
from gym_solo_amd import abi
from gym_solo_amd.model import DOF_TO_JOINT

N = {'saddle': 64}    # (robots per scenario, 16 unless listed: on the saddle one robot in five holds, and a holding robot rarely converges)


class Oracle:
  """kkt_cases' engine interface on the CPU oracle (float64)"""

  def make(self, case):
    from oracle import solo_oracle as so
    self.case = case
    self.ph = so.OraclePhysics(case.ca, case.ma, terrain=case.terrain)
    more = type(case.ca)()
    C.memmove(C.addressof(more), C.addressof(case.ca), C.sizeof(more))
    more.solver_iterations = case.ca.solver_iterations + 1
    self.more = so.OraclePhysics(more, case.ma, terrain=case.terrain)
    self.params = np.zeros((case.n, 4))
    self.params[:, 0], self.params[:, 1] = case.mus, case.scales
    return self

  def put(self, e, st):
    self.state = st.copy()

  def get(self, e):
    return self.state.copy()

  def rollout(self, e, acts):
    for a in acts:
      self.ph.step(self.state, a, self.params, threads=4)

  def sense(self, e):
    pass

  def step_record(self, e, act):
    ca = self.case.ca
    rec = np.zeros((self.case.n, abi.MAX_SPHERES, abi.CONTACT_WIDTH))
    cost = np.zeros(self.case.n, dtype=np.int32)
    tol = ca.solver_ulp_tolerance * 2.0 ** -53
    for i in range(self.case.n):
      tg = (act[i] * ca.action_scale)[DOF_TO_JOINT].copy()
      pre = self.state[i].copy()
      dbg = self.ph.step_debug(self.state[i], tg, self.params[i].copy())     # (steps the robot in place)
      rec[i] = contact_cases.oracle_forces(dbg, pre, ca.dt)[0]
      again = self.more.step_debug(pre.copy(), tg, self.params[i].copy())
      a, b = np.array(list(dbg.lam))[:dbg.num_rows], np.array(list(again.lam))[:dbg.num_rows]
      cost[i] = ca.solver_iterations - int((np.abs(a - b) <= tol * np.abs(a)).all())
    return rec, cost

  def diverged(self, e):
    return 0 if np.isfinite(self.state).all() else 1

  def close(self, e):
    pass


@pytest.mark.parametrize('ground', ['flat', 'incline', 'saddle'])
def test_the_measuring_device_against_the_oracles_kinematics(ground):
  """sphere centres against OraclePhysics.sphere_centers to 1e-15, the point-velocity rows against step_debug's J to 1e-14, on
  states of the flailing scenario (base and leg spheres live) and of the upper-link model"""
  from oracle import solo_oracle as so
  name = {'flat': 'belly', 'incline': 'incline', 'saddle': 'saddle'}[ground]
  rows = 0
  for scen in (name, 'upper') if ground == 'flat' else (name,):
    case = kc.make_case(scen, 'float64', 6)
    X = Oracle()
    X.make(case)
    X.put(X, case.states)
    X.rollout(X, case.acts[:120])
    worst_c, worst_j, n_rows = kc.validate_device(X.ph, case.ma, case.terrain, X.state)
    print('device vs oracle kinematics (%s): centres %.1e m, %d Jacobian rows %.1e' % (scen, worst_c, n_rows, worst_j))
    assert worst_c < 1e-15 and worst_j < 1e-14
    rows += n_rows
  assert rows >= 30


@pytest.mark.parametrize('name', kc.SCENARIOS)
def test_the_oracles_step_satisfies_newton_and_complementarity_per_row(name):
  case = kc.make_case(name, 'float64', N.get(name, 16))
  R = kc.evaluate(case, kc.collect(Oracle(), case), k_tol=case.ca.solver_ulp_tolerance, k_clamp=0)   # (the oracle always clamps)
  kc.show('oracle', case, R)
  kc.assert_holds(case, R)
