"""Batched termination conditions — counterpart of gym_solo/core/termination.py.

Same classes, names and error behaviour.  ``is_terminated()`` returns a ``[N]`` bool tensor
when the termination is attached to an engine (one counter per env, kept on the device and
ticked inside the fused step kernel), and keeps the reference's scalar semantics when used
stand-alone (the reference's unit tests: test_termination_conditions.py:4-38).
"""
from abc import ABC, abstractmethod
import math

from gym_solo_amd import abi


class Termination(ABC):
  @abstractmethod
  def reset(self):
    """Resets the state of the termination condition"""
    pass

  @abstractmethod
  def is_terminated(self):
    """Determines when an episode should terminate"""
    pass

  def program(self):
    """(kind, param) for the fused kernel, or None if this termination is Python-only."""
    return None


class TerminationFactory:
  def __init__(self):
    """termination.py:19-26"""
    self._terminations = []
    self._use_or = True
    self._engine_env = None  # set by the env: enables the fused, per-env path

  def register_termination(self, *terminations):
    """termination.py:28-36"""
    self._terminations.extend(terminations)
    if self._engine_env is not None:
      for t in terminations:
        if isinstance(t, StateTermination) and t._client is None:
          t.client = self._engine_env.client   # (the Python fallback reads the engine's state through it)
      self._engine_env._mark_dirty()

  def fusable(self):
    return (0 < len(self._terminations) <= abi.MAX_TERMS
            and all(t.program() is not None for t in self._terminations))

  def program(self):
    return [t.program() for t in self._terminations]

  def values(self):
    """The threshold of every termination slot (0 for the kinds that have none): Engine.set_term_values"""
    return [float(getattr(t, 'value', 0.0)) for t in self._terminations]

  def has_state_termination(self):
    return any(isinstance(t, StateTermination) for t in self._terminations)

  def fired(self):
    """Which termination ended each robot's last evaluated step: an ``[N]`` uint8 tensor, 0 = none, else 1 + the index (in
    registration order) of the first termination that fired.  Attached to an env; on the fused path it is the engine's
    ``term_fired`` (written by every launch that evaluates the terminations while a Height / TiltTermination is registered)."""
    if self._engine_env is None:
      raise ValueError('fired() needs the factory of an env')
    return self._engine_env._terminations_fired()

  def is_terminated(self):
    """OR over the registered conditions with short-circuit (termination.py:38-50).

    Stand-alone (no engine): exactly the reference's scalar loop.  Attached to an env: the
    per-env evaluation happens in the fused kernel; see Solo8VanillaEnv.step."""
    if not self._terminations:
      raise ValueError('Need to register at least one termination instance')
    if self._engine_env is not None:
      return self._engine_env._evaluate_terminations()
    for termination in self._terminations:
      if termination.is_terminated():
        return True
    return False

  def reset(self):
    """termination.py:52-56"""
    for termination in self._terminations:
      termination.reset()


class TimeBasedTermination(Termination):
  """termination.py:59-83: terminated once step_delta exceeds max_step_delta."""

  def __init__(self, max_step_delta: int):
    self.max_step_delta = max_step_delta
    self.reset()

  def reset(self):
    self.step_delta = 0

  def is_terminated(self) -> bool:
    self.step_delta += 1
    return self.step_delta > self.max_step_delta

  def program(self):
    return (abi.T_TIME, int(self.max_step_delta))


class PerpetualTermination(Termination):
  """termination.py:86-97: never terminates."""

  def reset(self):
    pass

  def is_terminated(self) -> bool:
    return False

  def program(self):
    return (abi.T_PERPETUAL, 0)


class StateTermination(Termination):
  """A termination that is a function of each robot's state after the step (Height / TiltTermination): per robot, with a grace
  period of ``after_steps`` evaluations at the start of every episode - the termination's counter ticks on every evaluation,
  exactly as a TimeBasedTermination's does (not once an earlier termination of the factory has fired), is cleared by a reset,
  and the termination fires when the counter exceeds ``after_steps`` AND the condition holds.  The grace period matters: the
  reset snapshot of the default configuration lies on its belly (z = 0.026 m) and stands up within ~120 steps.

  Registered with an env they run inside the fused step kernel (``program()``: solo_term_kernel; thresholds through
  Engine.set_term_values).  When the factory is not fusable (a Python-only termination next to them) they are evaluated with
  torch from the engine's state - the same formula in the engine's precision, the same tick rule - as an ``[N]`` bool tensor."""
  kind = None

  def __init__(self, robot, value, after_steps=0):
    if isinstance(after_steps, bool) or int(after_steps) != after_steps or int(after_steps) < 0:
      raise ValueError('after_steps must be an integer >= 0: {!r}'.format(after_steps))
    self.robot = robot
    self.value = float(value)
    self.after_steps = int(after_steps)
    self._client = None
    self._count = None   # [N] int32 on the state's device (Python path), or an int before the first evaluation

  @property
  def client(self):
    if self._client is None:
      raise ValueError('PyBullet client needs to be set')
    return self._client

  @client.setter
  def client(self, client):
    self._client = client

  def reset(self):
    self._count = None

  def reset_where(self, mask):
    """Clears the counters of the robots whose flag is set (a partial reset)"""
    if self._count is not None:
      self._count[mask.to(self._count.device).bool()] = 0

  @abstractmethod
  def condition(self, pos, quat):
    """[N] bool: the state condition, from base position [N, 3] and orientation quaternion [N, 4] (x, y, z, w)"""
    pass

  def is_terminated_where(self, active=None):
    """One evaluation: ticks the counters of the robots in ``active`` ([N] bool; None = all) and returns the ``[N]`` bool flags
    (False outside ``active``)."""
    import torch
    pos, quat = self.client.getBasePositionAndOrientation(self.robot)
    eng = getattr(self.client, 'engine', None)
    if eng is not None and eng.cfg.dtype == abi.F32:   # (the engine's precision, whatever the tensors of its state are held in)
      pos, quat = pos.to(torch.float32), quat.to(torch.float32)
    cond = self.condition(pos, quat)
    if self._count is None:
      self._count = torch.zeros(cond.shape[0], dtype=torch.int32, device=cond.device)
    old = self._count
    fires = (old + 1 > self.after_steps) & cond
    if active is not None:
      fires = fires & active
      self._count = old + active.to(torch.int32)
    else:
      self._count = old + 1
    return fires

  def is_terminated(self):
    return self.is_terminated_where(None)

  def program(self):
    return (self.kind, self.after_steps)


class HeightTermination(StateTermination):
  """Ends a robot's episode when its base is lower than ``min_height`` [m]: WORLD z, also over a heightfield."""
  kind = abi.T_HEIGHT_BELOW

  def __init__(self, robot, min_height, after_steps=0):
    if not math.isfinite(float(min_height)):
      raise ValueError('min_height must be finite: {!r}'.format(min_height))
    super().__init__(robot, float(min_height), after_steps)
    self.min_height = float(min_height)

  def condition(self, pos, quat):
    return pos[:, 2] < pos.new_tensor(self.value)


class TiltTermination(StateTermination):
  """Ends a robot's episode when its body z axis is tilted by more than ``max_tilt`` [rad], 0 < max_tilt < pi, from world z:
  c = 1 - 2 (qx^2 + qy^2) < cos(max_tilt) (the threshold is computed here, in double)."""
  kind = abi.T_TILT_ABOVE

  def __init__(self, robot, max_tilt, after_steps=0):
    if not (0.0 < float(max_tilt) < math.pi):
      raise ValueError('max_tilt must be in (0, pi) radians: {!r}'.format(max_tilt))
    super().__init__(robot, math.cos(float(max_tilt)), after_steps)
    self.max_tilt = float(max_tilt)

  def condition(self, pos, quat):
    qx, qy = quat[:, 0], quat[:, 1]
    return 1 - 2 * (qx * qx + qy * qy) < quat.new_tensor(self.value)
