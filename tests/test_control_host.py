"""Host side of the joint control modes (no GPU): configuration validation, the action space per mode, gain conversion
from joint order to dof order, and the pybullet facade's mapping of TORQUE_CONTROL / PD_CONTROL onto Engine calls."""
import numpy as np
import pytest

from gym_solo_amd import abi
from gym_solo_amd.core.configs import control_settings
from gym_solo_amd.engine import Engine
from gym_solo_amd.envs.solo8v2vanilla import Solo8VanillaConfig, Solo8VanillaEnv
from gym_solo_amd.model import DOF_TO_JOINT


def _cfg(**kw):
  c = Solo8VanillaConfig()
  for k, v in kw.items():
    setattr(c, k, v)
  return c


def test_config_defaults_and_validation():
  c = Solo8VanillaConfig()
  assert (c.control_mode, c.pd_kp, c.pd_kd) == ('position', None, None)
  assert control_settings(c) == ('position', None, None, None)
  assert control_settings(_cfg(control_mode='torque')) == ('torque', None, None, 1.0)
  assert control_settings(_cfg(control_mode='torque', motor_torque_limit=3.0), normalize_actions=True) == ('torque', None, None, 3.0)
  mode, kp, kd, scale = control_settings(_cfg(control_mode='pd', pd_kp=2.0, pd_kd=0.1))
  assert (mode, kp, kd, scale) == ('pd', 2.0, 0.1, None)
  with pytest.raises(ValueError):
    control_settings(_cfg(control_mode='pd'))                        # no default gains
  with pytest.raises(ValueError):
    control_settings(_cfg(control_mode='pd', pd_kp=1.0))
  with pytest.raises(ValueError):
    control_settings(_cfg(control_mode='velocity'))
  for bad in (-1.0, np.nan, np.inf, [1.0] * 11, [1.0] * 11 + [-0.5]):
    with pytest.raises(ValueError):
      control_settings(_cfg(control_mode='pd', pd_kp=bad, pd_kd=0.1))
    with pytest.raises(ValueError):
      control_settings(_cfg(control_mode='pd', pd_kp=1.0, pd_kd=bad))


def _env_without_engine(normalize, **kw):
  """The action-space logic of Solo8VanillaEnv on an instance that never created an engine."""
  from gym_solo_amd import spaces
  env = object.__new__(Solo8VanillaEnv)
  env.config = _cfg(**kw)
  env._normalize = normalize
  env._action_space = spaces.Box(-env.config.max_motor_rotation, env.config.max_motor_rotation, shape=(12,))
  return env


@pytest.mark.parametrize('normalize', [False, True])
def test_action_space_per_mode(normalize):
  pos = _env_without_engine(normalize).action_space
  pd = _env_without_engine(normalize, control_mode='pd', pd_kp=1.0, pd_kd=0.1).action_space
  tq = _env_without_engine(normalize, control_mode='torque', motor_torque_limit=2.5).action_space
  assert tq.shape == pd.shape == pos.shape == (12,)
  np.testing.assert_array_equal(pd.high, pos.high)   # PD keeps position mode's space and scaling
  np.testing.assert_array_equal(pd.low, pos.low)
  if normalize:
    np.testing.assert_array_equal(tq.high, np.ones(12))
    np.testing.assert_array_equal(tq.low, -np.ones(12))
  else:
    np.testing.assert_array_equal(tq.high, np.full(12, 2.5, dtype=np.float32))
    np.testing.assert_array_equal(tq.low, np.full(12, -2.5, dtype=np.float32))
    np.testing.assert_array_equal(pos.high, np.full(12, np.float32(2 * np.pi)))


def test_gain_conversion_joint_to_dof_order():
  g = np.arange(12, dtype=np.float64) * 0.5
  d = Engine.gains_to_dof(g, 'kp')
  assert d == [float(g[j]) for j in DOF_TO_JOINT]
  assert DOF_TO_JOINT == [0, 1, 3, 4, 6, 7, 9, 10]   # (the ANKLE entries 2, 5, 8, 11 are ignored)
  g2 = g.copy()
  g2[[2, 5, 8, 11]] = 99.0
  assert Engine.gains_to_dof(g2, 'kp') == d
  assert Engine.gains_to_dof(3.0, 'kp') == [3.0] * 8
  assert Engine.gains_to_dof(None, 'kp') == [0.0] * 8
  for bad in (-1.0, np.nan, [1.0] * 8, [[1.0] * 12]):
    with pytest.raises(ValueError):
      Engine.gains_to_dof(bad, 'kp')


class _FakeEngine:
  """Records what the facade asks of the engine (the real Engine needs a GPU)."""
  gains_to_dof = staticmethod(Engine.gains_to_dof)

  def __init__(self):
    from helpers import make_abi
    self.cfg, _ = make_abi('float64')
    self.num_envs = 3
    self.calls = []
    self._control = {'mode': 'position', 'kp': [0.0] * 8, 'kd': [0.0] * 8, 'action_scale': self.cfg.action_scale}

  @property
  def control(self):
    return dict(self._control)

  def set_control(self, mode, kp=None, kd=None, action_scale=None):
    self.calls.append(('set_control', mode))
    self._control = {'mode': mode, 'kp': self.gains_to_dof(kp, 'kp'), 'kd': self.gains_to_dof(kd, 'kd'),
                     'action_scale': float(action_scale if action_scale is not None else self.cfg.action_scale)}

  def set_targets(self, a):
    self.calls.append(('set_targets', a))


def _client():
  from gym_solo_amd.client import BatchedBulletClient
  from gym_solo_amd.model import Solo8Model
  eng = _FakeEngine()
  c = BatchedBulletClient(eng, Solo8Model())
  c.as_actions = lambda a: np.asarray(a)   # (the real one moves the actions to the engine's device)
  return c, eng


def test_facade_constants_and_mapping():
  from gym_solo_amd import client as p
  assert (p.TORQUE_CONTROL, p.POSITION_CONTROL, p.PD_CONTROL) == (1, 2, 3)
  c, eng = _client()
  tau = np.full(12, 0.3)
  c.setJointMotorControlArray(1, range(12), p.TORQUE_CONTROL, forces=tau)
  c.setJointMotorControlArray(1, range(12), p.TORQUE_CONTROL, forces=tau)
  assert [x[0] for x in eng.calls] == ['set_control', 'set_targets', 'set_targets']   # (set_control only on a change)
  assert eng.control['mode'] == 'torque' and eng.control['action_scale'] == 1.0
  eng.calls.clear()
  c.setJointMotorControlArray(1, range(12), p.PD_CONTROL, targetPositions=np.zeros(12), positionGains=2.0, velocityGains=0.1)
  c.setJointMotorControlArray(1, range(12), p.PD_CONTROL, targetPositions=np.zeros(12), positionGains=2.0, velocityGains=0.1,
                              targetVelocities=np.zeros(12))
  c.setJointMotorControlArray(1, range(12), p.PD_CONTROL, targetPositions=np.zeros(12), positionGains=3.0, velocityGains=0.1)
  assert [x[0] for x in eng.calls] == ['set_control', 'set_targets', 'set_targets', 'set_control', 'set_targets']
  assert eng.control['kp'] == [3.0] * 8 and eng.control['kd'] == [0.1] * 8
  eng.calls.clear()
  c.setJointMotorControlArray(1, range(12), p.POSITION_CONTROL, targetPositions=np.zeros(12), forces=eng.cfg.motor_torque_limit)
  assert [x[0] for x in eng.calls] == ['set_control', 'set_targets'] and eng.control['mode'] == 'position'


def test_facade_errors():
  from gym_solo_amd import client as p
  c, eng = _client()
  with pytest.raises(ValueError):
    c.setJointMotorControlArray(1, range(12), p.PD_CONTROL, targetPositions=np.zeros(12), positionGains=1.0,
                                velocityGains=0.1, targetVelocities=np.ones(12))
  with pytest.raises(ValueError):
    c.setJointMotorControlArray(1, range(12), p.PD_CONTROL, targetPositions=np.zeros(12))   # gains missing
  with pytest.raises(ValueError):
    c.setJointMotorControlArray(1, range(12), p.PD_CONTROL, targetPositions=np.zeros(12), positionGains=-1.0, velocityGains=0.1)
  with pytest.raises(ValueError):
    c.setJointMotorControlArray(1, range(12), p.TORQUE_CONTROL)                              # no torques
  for mode in (0, 4, 5):   # VELOCITY_CONTROL, STABLE_PD_CONTROL, ... [recalled]
    with pytest.raises(ValueError):
      c.setJointMotorControlArray(1, range(12), mode, targetPositions=np.zeros(12))
  assert eng.calls == []
