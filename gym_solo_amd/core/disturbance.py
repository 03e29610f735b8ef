"""Host-side disturbance schedules on top of the engine's base wrench block (Engine.set_base_wrench / Engine.base_wrench;
include/solo_engine.h "external base wrenches").  The engine applies whatever the block holds, every physics step; a schedule
only decides WHEN the block changes, with torch operations on the engine's device that never synchronise - so it runs inside a
training loop, between launches, at the cost of a handful of small kernels per control step."""
import math


class RandomPushes:
  """Random pushes of the base link, per robot: after a pause of ``interval = (lo, hi)`` control steps (an integer drawn
  uniformly, both ends included) a robot is pushed for ``duration`` control steps, then left alone for the next pause.

  A push is a HORIZONTAL world-frame force of uniformly distributed direction and a magnitude uniform in [0, max_force] [N],
  and a world-frame torque uniform in the ball of radius ``max_torque`` [N m]; both are held unchanged for the whole push (the
  engine applies them every physics step of every control step) and are zero between pushes.

  ``tick()`` advances the schedule by ONE control step: call it once after every engine step (Solo8VanillaEnv.step does when the
  schedule is its ``disturbance``).  It works on per-robot countdown tensors and writes the block in place through
  ``engine.base_wrench`` - the engine documents that the next launch, and an already captured graph, read such writes - with no
  synchronisation and no transfer to the host.  Resets do not touch the timers: a push is a property of the world, not of the
  episode.

  The engine's block must be on when the schedule is created (it is switched on here, all zeros, if it is off) and must stay on;
  ``generator`` is a torch.Generator of the engine's device (None: the default one)."""

  def __init__(self, engine, interval, duration, max_force, max_torque=0.0, generator=None):
    import torch
    lo, hi = int(interval[0]), int(interval[1])
    if lo < 1 or hi < lo:
      raise ValueError('interval must be (lo, hi) with 1 <= lo <= hi control steps: {!r}'.format(interval))
    if int(duration) < 1:
      raise ValueError('duration must be at least one control step: {!r}'.format(duration))
    if not (max_force >= 0 and math.isfinite(max_force) and max_torque >= 0 and math.isfinite(max_torque)):
      raise ValueError('max_force and max_torque must be finite and >= 0')
    self.engine = engine
    self.lo, self.hi, self.duration = lo, hi, int(duration)
    self.max_force, self.max_torque = float(max_force), float(max_torque)
    self.generator = generator
    if engine.base_wrench is None:
      engine.set_base_wrench({})
    self.block = engine.base_wrench   # (zero copy, and stable while the block stays on)
    self.device, self.dtype = self.block.device, self.block.dtype
    n = self.block.shape[0]
    self._torch = torch
    # the control steps left in the robot's current phase, and whether that phase is a push
    self.count = self._pause(n)
    self.active = torch.zeros(n, dtype=torch.bool, device=self.device)

  def _pause(self, n):
    return self._torch.randint(self.lo, self.hi + 1, (n,), generator=self.generator, device=self.device)

  def _draw(self, n):
    """[n, 6]: (force, torque) of a new push"""
    torch = self._torch
    u = torch.rand(n, 3, generator=self.generator, device=self.device, dtype=self.dtype)
    g = torch.randn(n, 3, generator=self.generator, device=self.device, dtype=self.dtype)
    angle, mag = (2.0 * math.pi) * u[:, 0], self.max_force * u[:, 1]
    force = torch.stack((mag * torch.cos(angle), mag * torch.sin(angle), torch.zeros_like(mag)), dim=1)
    radius = self.max_torque * u[:, 2] ** (1.0 / 3.0)
    torque = g * (radius / g.norm(dim=1).clamp_min(1e-30)).unsqueeze(1)
    return torch.cat((force, torque), dim=1)

  def tick(self):
    torch = self._torch
    n = self.count.shape[0]
    self.count -= 1
    expired = self.count <= 0
    start, stop = expired & ~self.active, expired & self.active
    # (every tick draws for every robot: the stream of random numbers, and the work, do not depend on who expired)
    fresh, pause = self._draw(n), self._pause(n)
    w = self.block[:, :6]
    w.copy_(torch.where(start.unsqueeze(1), fresh, torch.where(stop.unsqueeze(1), torch.zeros_like(fresh), w)))
    self.count = torch.where(start, torch.full_like(self.count, self.duration), torch.where(stop, pause, self.count))
    self.active = self.active ^ expired
