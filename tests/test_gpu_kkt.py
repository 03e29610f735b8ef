"""tests/kkt_cases.py on the HIP engine, through the C-ABI: Newton on all fourteen rows of M du = J^T lam and the per-row
complementarity conditions of the solved contact rows, read from the state before a step, the state after it, the contact record
and view.cost - f64 and f32, 256 robots, position control in scenarios (a) ... (e), torque control on (a) and (b).  Every step of
the schedule runs on the engine: one fused physics-only launch to the first sampled step, sensing on, then one-step STEP_PHYSICS
launches with fused launches in between.  The start states are the CPU oracle's settle snapshot (a state, not a result under test);
nothing else of the oracle's step enters.  Each test prints, per check, the worst residual / budget."""
import numpy as np
import pytest

import kkt_cases as kc
from gym_solo_amd import abi

pytestmark = pytest.mark.gpu

N = 256


class Hip:
  """kkt_cases' engine interface on the HIP engine"""

  def __init__(self):
    import torch
    if not torch.cuda.is_available():
      pytest.fail('GPU tests need a visible MI355X')
    self.torch = torch

  def _t(self, e, a):
    return self.torch.as_tensor(np.ascontiguousarray(a), device='cuda', dtype=e.tdtype)

  def make(self, case):
    from gym_solo_amd.engine import Engine
    case.ca.settle_steps = 1     # (the case puts its own states)
    e = Engine(case.ca, case.ma, case.n)
    if case.terrain is not None:
      e.set_terrain(case.terrain)
    e.set_params(abi.PARAM_FRICTION, self._t(e, case.mus))
    e.set_params(abi.PARAM_BASE_MASS_SCALE, self._t(e, case.scales))
    if case.mode == 'torque':
      e.set_control('torque')
    return e

  def put(self, e, st):
    e.state.copy_(self._t(e, st))

  def get(self, e):
    return e.state.cpu().numpy().astype(np.float64)

  def rollout(self, e, acts):
    if len(acts):
      e.rollout(self._t(e, acts), abi.STEP_PHYSICS)

  def sense(self, e):
    e.set_contact_sensing(True)

  def step_record(self, e, act):
    e.step(self._t(e, act), abi.STEP_PHYSICS)
    return e.contacts.cpu().numpy().astype(np.float64), e.cost.cpu().numpy().copy()

  def diverged(self, e):
    return float(e.stats.cpu().numpy()[5])

  def close(self, e):
    e.close()


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('name,mode', [(s, 'position') for s in kc.SCENARIOS] + [(s, 'torque') for s in kc.TORQUE_SCENARIOS])
def test_the_engine_satisfies_newton_and_complementarity_per_row(name, mode, dtype):
  case = kc.make_case(name, dtype, N, mode)
  R = kc.evaluate(case, kc.collect(Hip(), case), k_tol=case.ca.solver_ulp_tolerance)
  kc.show('MI355X', case, R)
  kc.assert_holds(case, R)
