"""Host side of contact sensing (no GPU): FootContact's labels, space and binary mode, its fused program against its
Python path on a stand-in client, the pybullet facade's sphere -> link mapping, and the configuration field."""
import numpy as np
import pytest

from gym_solo_amd import abi
from gym_solo_amd.client import BatchedBulletClient
from gym_solo_amd.core.obs import FootContact
from gym_solo_amd.envs.solo8v2vanilla import Solo8VanillaConfig


class _Client:
  """getContactPoints of a batch of 3 robots with made-up normal forces."""
  def __init__(self, fn):
    self.fn = fn

  def getContactPoints(self, bodyA=None):
    return {'linkIndexA': list(BatchedBulletClient.SPHERE_LINKS), 'normalForce': self.fn, 'force': np.zeros(self.fn.shape + (3,))}


def _fused(elems, fn):
  """What the kernel does with the program (solo_outputs.h observation_value_foot): source x scale, then the clip."""
  out = np.zeros((fn.shape[0], len(elems)))
  for i, e in enumerate(elems):
    v = fn[:, 4 * (e['src'] - abi.SRC_FOOT_FORCE) + 1] * e['scale']
    out[:, i] = np.minimum(np.maximum(v, e['lo']), e['hi']) if e['clip'] else v
  return out


def test_labels_space_and_program():
  o = FootContact(0)
  assert o.labels == ['FL_foot_force', 'FR_foot_force', 'HL_foot_force', 'HR_foot_force']
  np.testing.assert_array_equal(o.observation_space.low, np.zeros(4))
  np.testing.assert_array_equal(o.observation_space.high, np.full(4, 100.))
  assert [e['src'] for e in o.program()] == [41, 42, 43, 44]
  b = FootContact(0, binary=True, max_force=7.)
  assert b.labels == ['FL_foot_contact', 'FR_foot_contact', 'HL_foot_contact', 'HR_foot_contact']
  np.testing.assert_array_equal(b.observation_space.high, np.ones(4))
  assert all(e['clip'] and e['lo'] == 0 and e['hi'] == 1 for e in b.program())
  with pytest.raises(ValueError):
    FootContact(0, max_force=0)


@pytest.mark.parametrize('binary', [False, True])
def test_python_path_equals_fused_program(binary):
  rng = np.random.default_rng(0)
  fn = np.where(rng.random((3, 16)) < 0.5, 0.0, rng.uniform(0, 300, (3, 16)))
  fn[0, 1] = 1e-6    # (a barely touching foot: 1 in binary mode)
  o = FootContact(0, binary=binary, max_force=50.)
  o.client = _Client(fn)
  got = o.compute()
  np.testing.assert_array_equal(got, _fused(o.program(), fn))
  if binary:
    np.testing.assert_array_equal(got, (fn[:, 1::4] > 0).astype(float))
  assert got.shape == (3, 4)


class _Engine:
  contact_sensing = True

  def __init__(self):
    self.contacts = np.zeros((2, abi.MAX_SPHERES, abi.CONTACT_WIDTH))


def test_facade_rejects_the_filters_it_does_not_support():
  client = object.__new__(BatchedBulletClient)
  client.engine = _Engine()
  out = client.getContactPoints(bodyA=0)
  assert out['normalForce'].shape == (2, 16) and out['force'].shape == (2, 16, 3)
  for kw in (dict(bodyB=1), dict(linkIndexA=2), dict(linkIndexB=-1)):
    with pytest.raises(ValueError):
      client.getContactPoints(bodyA=0, **kw)


def test_binary_mode_below_one_nanonewton_is_proportional():
  o = FootContact(0, binary=True)
  fn = np.zeros((1, 16))
  fn[0, 1::4] = [0.0, 2.5e-10, 1e-9, 5.0]
  o.client = _Client(fn)
  np.testing.assert_allclose(o.compute(), [[0.0, 0.25, 1.0, 1.0]])


def test_facade_sphere_links_and_config():
  links = BatchedBulletClient.SPHERE_LINKS
  assert len(links) == abi.MAX_SPHERES
  for l in range(4):
    assert links[4 * l] == 3 * l + 1        # knee sphere: the lower leg (the KFE joint's link)
    assert links[4 * l + 1] == 3 * l + 2    # foot sphere: the foot welded to it (the fixed ANKLE joint's link)
    assert links[4 * l + 2] == links[4 * l + 3] == -1   # base corners
  assert Solo8VanillaConfig().contact_sensing is False
  from gym_solo_amd.model import Solo8Model
  m = Solo8Model().to_abi()
  for l in range(4):   # (the model's spheres sit on the bodies the mapping names)
    assert m.sphere_body[4 * l] == m.sphere_body[4 * l + 1] == 2 + 2 * l   # (the lower leg carries the foot)
    assert m.sphere_body[4 * l + 2] == m.sphere_body[4 * l + 3] == 0
