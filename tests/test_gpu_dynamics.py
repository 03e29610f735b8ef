"""tests/dynamics_cases.py on the HIP engine, through the C-ABI, f64 and f32, 256 robots per case: the free dynamics of one step in
torque mode (A: every model of the family, damping on and off, and through the actuator block - solo_act_kernel), PD mode (B) and
position mode (C), three chained one-step launches and the same steps as one fused launch (D), and the pose update (E), against the
kinematics-only reference in longdouble.  Nothing of the CPU oracle enters.  Every test prints the worst residual / budget."""
import numpy as np
import pytest

import dynamics_cases as dc
from gym_solo_amd import abi

pytestmark = pytest.mark.gpu

N = 256
DTYPES = ['float64', 'float32']


class Hip:
  """dynamics_cases' engine interface on the HIP engine"""

  def __init__(self):
    import torch
    if not torch.cuda.is_available():
      pytest.fail('GPU tests need a visible MI355X')
    self.torch = torch

  def _t(self, e, a):
    return self.torch.as_tensor(np.ascontiguousarray(a), device='cuda', dtype=e.tdtype)

  def open(self, ca, ma, n, mode, scales, gains=None, actuators=None):
    from gym_solo_amd.engine import Engine
    ca.settle_steps = 1     # (the case puts its own states)
    e = Engine(ca, ma, n)
    e.set_params(abi.PARAM_BASE_MASS_SCALE, self._t(e, scales))
    if mode != 'position':
      kp, kd = (dc.joint_actions(np.asarray(g)) for g in gains) if gains is not None else (None, None)
      e.set_control(mode, kp=kp, kd=kd, action_scale=1.0)
    if actuators is not None:
      e.set_actuators(self._t(e, actuators))
      assert e.kernel_name.startswith('solo_act_kernel')
    return e

  def run(self, e, state, acts):
    e.state.copy_(self._t(e, state))
    if len(acts) == 1:
      e.step(self._t(e, acts[0]), abi.STEP_PHYSICS)
    else:
      e.rollout(self._t(e, acts), abi.STEP_PHYSICS)
    assert float(e.stats.cpu().numpy()[5]) == 0     # (no robot was restored)
    return e.state.cpu().numpy().astype(np.float64)

  def close(self, e):
    e.close()


def _hold(dtype, case, report):
  dc.show('MI355X ' + dtype, case, report)
  dc.assert_within_budget(report)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('model', dc.MODELS)
def test_torque_step_on_every_model(model, dtype):
  _hold(dtype, 'torque, ' + model, dc.torque(Hip(), dtype, model, N))


@pytest.mark.parametrize('dtype', DTYPES)
def test_torque_step_without_damping(dtype):
  _hold(dtype, 'torque, damping 0', dc.torque(Hip(), dtype, 'default', N, damping=False))


@pytest.mark.parametrize('dtype', DTYPES)
def test_torque_step_through_the_actuator_block(dtype):
  _hold(dtype, 'torque, actuator block', dc.torque_actuators(Hip(), dtype, N))


@pytest.mark.parametrize('dtype', DTYPES)
def test_pd_step(dtype):
  _hold(dtype, 'pd', dc.pd(Hip(), dtype, N))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('model', ['default', 'seed0'])
def test_position_step_keeps_the_motors_internal(model, dtype):
  _hold(dtype, 'position, ' + model, dc.position(Hip(), dtype, model, N))


@pytest.mark.parametrize('dtype', DTYPES)
def test_three_chained_steps_and_their_fused_twin(dtype):
  _hold(dtype, 'chained', dc.chained(Hip(), dtype, N))


@pytest.mark.parametrize('dtype', DTYPES)
def test_pose_update(dtype):
  _hold(dtype, 'pose', dc.pose(Hip(), dtype, 37))     # (37 robots per spin: 259)
