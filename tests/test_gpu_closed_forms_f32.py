"""The closed forms of tests/closed_form_cases.py on the FLOAT32 HIP engine: the cases, checkers and rounding budgets of
tests/test_emu_closed_forms_f32.py (tests/f32_cases.py) at 256 robots per case, one engine per case - the f32 kernels' own
Gauss-Seidel loop in assembly (solo_pgs_gfx950.h) and solo_wave_ops.h's Real<float> held to Newton's and Coulomb's laws, not to
the oracle's step.  Every single-step identity runs twice: as a launch of its own, and as the last step of a fused 3-step
rollout with the checked state taken before that step from a twin engine.  Each test prints, per identity, the worst
residual / budget and the worst residual in its unit; no robot may diverge (stats[5] == 0).  Plus the contact-sensing identity
(sum of the recorded forces x dt = the step's momentum change - m g dt) in both precisions."""
import numpy as np
import pytest

import f32_cases as fc
from gym_solo_amd import abi

pytestmark = pytest.mark.gpu

N = 256


class Hip:
  """f32_cases' engine interface on the HIP engine"""
  n_small = n_large = N

  def __init__(self, sensing=False):
    import torch
    if not torch.cuda.is_available():
      pytest.fail('GPU tests need a visible MI355X')
    self.torch, self.sensing = torch, sensing

  def _t(self, e, a):
    return self.torch.as_tensor(np.ascontiguousarray(a), device='cuda', dtype=e.tdtype)

  def make(self, ca, ma, n, terrain=None, friction=None):
    from gym_solo_amd.engine import Engine
    ca.settle_steps = 1     # (every case puts its own states)
    e = Engine(ca, ma, n)
    if terrain is not None:
      e.set_terrain(terrain)
    if friction is not None:
      e.set_params(abi.PARAM_FRICTION, self._t(e, friction))
    if self.sensing:
      e.set_contact_sensing(True)
    return e

  def put(self, e, st):
    e.state.copy_(self._t(e, st))

  def get(self, e):
    return e.state.cpu().numpy().astype(np.float64)

  def step(self, e, acts):
    e.step(self._t(e, acts), abi.STEP_PHYSICS)

  def rollout(self, e, acts):
    e.rollout(self._t(e, acts), abi.STEP_PHYSICS)

  def step_record(self, e, acts):
    self.step(e, acts)
    return e.contacts.cpu().numpy().astype(np.float64)

  def diverged(self, e):
    return float(e.stats.cpu().numpy()[5])

  def close(self, e):
    if e is not None:
      e.close()


@pytest.mark.parametrize('case', fc.MULTI_STEP)
def test_closed_form_on_the_f32_engine(case):
  report = fc.run(case, Hip(), 'float32')
  fc.show('MI355X f32', case, report)
  fc.assert_within_budget(report)


@pytest.mark.parametrize('case,fused', [(c, False) for c in fc.SINGLE_STEP] + [(c, True) for c in fc.FUSED])
def test_single_step_closed_form_on_the_f32_engine(case, fused):
  report = fc.run(case, Hip(), 'float32', fused)
  fc.show('MI355X f32', case + (' (last of a fused rollout of 3)' if fused else ' (one launch)'), report)
  fc.assert_within_budget(report)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_recorded_contact_forces_are_the_momentum_change(dtype):
  report = fc.contact_record(Hip(sensing=True), dtype)
  fc.show('MI355X ' + dtype, 'contact record', report)
  fc.assert_within_budget(report)
