"""tests/dynamics_cases.py on the PRODUCT kernel source (CPU emulator), f64 and f32: the free dynamics of one step in torque mode
(A: every model of the family, damping on and off, and through the actuator block), PD mode (B) and position mode (C), three chained
launches and their fused twin (D), and the pose update (E) against the kinematics-only reference.  Torque and PD launches go through
emu_kernel.control_rollout, the actuator block through emu_actuator.ActSim, position mode through EmuEngine.  Every test prints the
worst residual / budget; tests/test_gpu_dynamics.py runs the same cases on the HIP engine."""
import numpy as np
import pytest

import dynamics_cases as dc
import emu_kernel
from gym_solo_amd import abi

DTYPES = ['float64', 'float32']
N = {'float64': 16, 'float32': 16}
N_FAMILY = 8          # (per model of the family and dtype, and in the chained case)


class Emu:
  """dynamics_cases' engine interface on the emulator"""

  def open(self, ca, ma, n, mode, scales, gains=None, actuators=None):
    params = np.zeros((n, 4))
    params[:, 0], params[:, 1] = ca.lateral_friction, scales
    h = dict(ca=ca, ma=ma, n=n, mode=mode, params=params, actuators=actuators)
    if mode != 'position':
      kp, kd = gains if gains is not None else (None, None)
      h['ctl'] = emu_kernel.control_block(abi.CTRL_TORQUE if mode == 'torque' else abi.CTRL_PD, kp, kd)
    return h

  def run(self, h, state, acts):
    st = np.ascontiguousarray(state, dtype=np.float64).copy()
    if h['actuators'] is not None:
      import emu_actuator
      from test_emu_terms import program
      sim = emu_actuator.ActSim(emu_actuator.load(), h['ca'], h['ma'], h['n'], program([(abi.T_TIME, 1000)]), st, None, h['ctl'], 1)
      sim.params[:] = h['params']
      sim.set_actuators(h['actuators'])
      assert len(acts) == 1
      sim.step(acts[0], abi.STEP_PHYSICS)
      assert sim.kernel.startswith('solo_act_kernel') and sim.stats[:, 5].sum() == 0
      return sim.state.copy()
    if h['mode'] == 'position':
      e = emu_kernel.EmuEngine(h['ca'], h['ma'], h['n'])
      e.state[:], e.snapshot[:], e.params[:] = st, st, h['params']
      if len(acts) == 1:
        e.step(acts[0], abi.STEP_PHYSICS)
      else:
        e.rollout(acts, abi.STEP_PHYSICS, record=False)
      assert e.stats[:, 5].sum() == 0
      return e.state.copy()
    return emu_kernel.control_rollout(h['ca'], h['ma'], h['ctl'], st, acts, h['params'])

  def close(self, h):
    pass


def _hold(where, case, report):
  dc.show(where, case, report)
  dc.assert_within_budget(report)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('model', dc.MODELS)
def test_torque_step_on_every_model(model, dtype):
  _hold('emu ' + dtype, 'torque, ' + model, dc.torque(Emu(), dtype, model, N[dtype] if model == 'default' else N_FAMILY))


@pytest.mark.parametrize('dtype', DTYPES)
def test_torque_step_without_damping(dtype):
  _hold('emu ' + dtype, 'torque, damping 0', dc.torque(Emu(), dtype, 'default', N[dtype], damping=False))


@pytest.mark.parametrize('dtype', DTYPES)
def test_torque_step_through_the_actuator_block(dtype):
  _hold('emu ' + dtype, 'torque, actuator block', dc.torque_actuators(Emu(), dtype, N[dtype]))


@pytest.mark.parametrize('dtype', DTYPES)
def test_pd_step(dtype):
  _hold('emu ' + dtype, 'pd', dc.pd(Emu(), dtype, N[dtype]))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('model', ['default', 'seed0'])
def test_position_step_keeps_the_motors_internal(model, dtype):
  _hold('emu ' + dtype, 'position, ' + model, dc.position(Emu(), dtype, model, N[dtype]))


@pytest.mark.parametrize('dtype', DTYPES)
def test_three_chained_steps_and_their_fused_twin(dtype):
  _hold('emu ' + dtype, 'chained', dc.chained(Emu(), dtype, N_FAMILY))


@pytest.mark.parametrize('dtype', DTYPES)
def test_pose_update(dtype):
  _hold('emu ' + dtype, 'pose', dc.pose(Emu(), dtype, 4))
