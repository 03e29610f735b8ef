"""Progress pacing of the segmented launch ON THE GPU (solo_roll_kernel's segment boundary: a wave counts itself in the engine's
progress block and takes its issue priority for the next segment from its rank).  Pacing is scheduling: every value a caller can
see equals, BIT FOR BIT, the twin library built with -DSOLO_ROLL_PACING=0 (libsolo_hip_no_pacing.so: the roll kernel as it was
before) and eight single-step launches; the block holds what the waves counted; a captured rollout re-zeroes it at every replay.

128 robots, steps_per_launch = 3, K = 8: segments of 3, 3 and 2 steps (a ragged last one), on two slices - two launches sharing
the block - and on one; f64 and f32; TimeBased(7) with auto-reset on staggered counters.  Every rollout runs twice in a row.  The
statistics shards are zeroed in front of every rollout: 128 robots share 64 rows, a robot ends exactly one episode in eight steps, and
two additions onto zero commute - a third would depend on the order in which the waves arrive.

The regression guard: 64 robots, K = 6, S = 3, TimeBased(4) with auto-reset on counters 0 .. 4 - resets inside a segment, on a
segment's last step and on the next one's first - against the twin.

One fresh process per library (SOLO_HIP_LIB is read at import), shared by the tests."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'gym_solo_amd', 'csrc')
N, S, K = 128, 3, 8
DTYPES = ('float64', 'float32')
FIELDS = ('obs_rec', 'reward_rec', 'done_rec', 'obs', 'reward', 'done', 'state', 'term_count', 'targets', 'stats')

_WORKER = r'''
import sys, os, ctypes as C
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, 'tests'))
import numpy as np, torch
from gym_solo_amd import abi
from gym_solo_amd.envs.solo8v2vanilla import Solo8VanillaConfig, Solo8VanillaEnv
from gym_solo_amd.workloads import register_benchmark_workload
out = sys.argv[1]
N, S, K = %(n)d, %(s)d, %(k)d
res = {}

def make_env(dtype, n, max_steps, **geometry):
  cfg = Solo8VanillaConfig()
  cfg.dtype, cfg.num_envs, cfg.auto_reset = dtype, n, True
  for key, value in geometry.items():
    setattr(cfg, key, value)
  env = Solo8VanillaEnv(config=cfg, copy_outputs=False)
  register_benchmark_workload(env, max_steps=max_steps)   # TimeBased(max_steps)
  env._ensure_program()
  return env

def progress(eng):
  buf = np.full(16, -1, dtype=np.int32)
  eng.lib.solo_engine_debug_progress.argtypes = [C.c_void_p, C.c_void_p]
  eng.lib.solo_engine_debug_progress.restype = C.c_int
  assert eng.lib.solo_engine_debug_progress(eng._h, buf.ctypes.data) == 0
  return buf

def keep(tag, eng, rec):
  eng.synchronize()
  got = dict(obs_rec=rec[0], reward_rec=rec[1], done_rec=rec[2], obs=eng.obs, reward=eng.reward, done=eng.done, state=eng.state,
             term_count=eng.term_count, targets=eng.targets, stats=eng.stats_shards, cost=eng.cost)
  for k, v in got.items():
    res[tag + '/' + k] = v.detach().cpu().numpy().copy()
  res[tag + '/progress'] = progress(eng)
  res[tag + '/kernel'] = np.frombuffer(eng.kernel_name.encode(), dtype=np.uint8)

for dtype in ('float64', 'float32'):
  tdt = torch.float32 if dtype == 'float32' else torch.float64
  g = torch.Generator(device='cuda').manual_seed(53)
  acts = (torch.rand(2, K, N, 12, device='cuda', dtype=tdt, generator=g) * 2 - 1) * 6.28
  tc = torch.zeros(N, 4, device='cuda', dtype=torch.int32)
  tc[:, 0] = torch.arange(N, device='cuda', dtype=torch.int32) %% 8
  # ---- two rollouts in a row: on two slices, on one, and as eight single-step launches
  for name, geometry in (('two', dict(steps_per_launch=S, rollout_streams=2)), ('one', dict(steps_per_launch=S, rollout_streams=1)),
                         ('single', dict(steps_per_launch=1, rollout_streams=1))):
    env = make_env(dtype, N, 7, **geometry)
    eng = env.engine
    eng.term_count.copy_(tc)
    for rep in range(2):
      eng.stats_shards.zero_()
      keep('%%s/%%s/%%d' %% (dtype, name, rep), eng, eng.rollout(acts[rep], abi.STEP_ALL, record=True))
    res['%%s/%%s/plan' %% (dtype, name)] = np.array([eng.plan(K)[k] for k in ('steps_per_launch', 'launches', 'slices')])
    env._close()
  # ---- the never-run rollout on two slices, captured after reserve(K) and replayed twice
  env = make_env(dtype, N, 7, steps_per_launch=S, rollout_streams=2)
  eng = env.engine
  eng.term_count.copy_(tc)
  static = torch.zeros(K, N, 12, device='cuda', dtype=tdt)
  bufs = eng.rollout_buffers(K)
  eng.reserve(K)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    eng.rollout(static, abi.STEP_ALL, out=bufs)
  for rep in range(2):
    eng.stats_shards.zero_()
    static.copy_(acts[rep])
    graph.replay()
    keep('%%s/graph/%%d' %% (dtype, rep), eng, bufs)
  env._close()
  # ---- the regression guard: resets inside a segment and on both sides of a boundary
  env = make_env(dtype, 64, 4, steps_per_launch=S, rollout_streams=2)
  eng = env.engine
  tg = torch.zeros(64, 4, device='cuda', dtype=torch.int32)
  tg[:, 0] = torch.arange(64, device='cuda', dtype=torch.int32) %% 5
  eng.term_count.copy_(tg)
  keep('%%s/guard/0' %% dtype, eng, eng.rollout(acts[0][:6, :64].contiguous(), abi.STEP_ALL, record=True))
  env._close()
np.savez(out, **res)
'''


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
  import torch
  if not torch.cuda.is_available():
    pytest.fail('GPU tests need a visible MI355X')
  libs = {'paced': os.path.join(CSRC, 'libsolo_hip.so'), 'twin': os.path.join(CSRC, 'libsolo_hip_no_pacing.so')}
  assert os.path.isfile(libs['twin']), 'build it: make -C gym_solo_amd/csrc test-libs (or __graft_entry__.build())'
  tmp = tmp_path_factory.mktemp('progress_pacing')
  got = {}
  for name, lib in libs.items():
    out = str(tmp / (name + '.npz'))
    subprocess.run([sys.executable, '-c', _WORKER % {'root': ROOT, 'n': N, 's': S, 'k': K}, out], check=True,
                   env=dict(os.environ, SOLO_HIP_LIB=lib), timeout=240)
    got[name] = dict(np.load(out))
  return got


def same(a, b, tag_a, tag_b, fields):
  for f in fields:
    x, y = a[tag_a + '/' + f], b[tag_b + '/' + f]
    assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), '%s against %s: %s differs' % (tag_a, tag_b, f)


@pytest.mark.parametrize('slices', ['two', 'one'])
@pytest.mark.parametrize('dtype', DTYPES)
def test_paced_equals_the_twin_and_single_steps(runs, dtype, slices):
  paced, twin = runs['paced'], runs['twin']
  real = 'double' if dtype == 'float64' else 'float'
  assert paced['%s/%s/plan' % (dtype, slices)].tolist() == [S, 3, 2 if slices == 'two' else 1]
  for rep in range(2):
    tag = '%s/%s/%d' % (dtype, slices, rep)
    assert paced[tag + '/kernel'].tobytes().decode() == 'solo_roll_kernel<%s>' % real == twin[tag + '/kernel'].tobytes().decode()
    same(paced, twin, tag, tag, FIELDS + ('cost',))                                # the roll kernel without pacing
    same(paced, paced, tag, '%s/single/%d' % (dtype, rep), FIELDS)                  # eight launches of one step
    same(twin, twin, tag, '%s/single/%d' % (dtype, rep), FIELDS)
    done = paced[tag + '/done_rec'].astype(bool)
    assert done.any() and not done.all(axis=0).any() and paced[tag + '/stats'].any()


@pytest.mark.parametrize('slices', ['two', 'one'])
@pytest.mark.parametrize('dtype', DTYPES)
def test_the_block_holds_what_the_waves_counted(runs, dtype, slices):
  """counters 0 and 1 = all 128 robots - both slices count into ONE block -, the last segment counts nothing, and the second rollout
  in a row starts from zero again; the twin's kernel never touches the block"""
  for rep in range(2):
    tag = '%s/%s/%d' % (dtype, slices, rep)
    assert runs['paced'][tag + '/progress'].tolist() == [N, N] + [0] * 14, tag
    assert runs['twin'][tag + '/progress'].tolist() == [0] * 16, tag
    assert runs['paced']['%s/single/%d/progress' % (dtype, rep)].tolist() == [0] * 16


@pytest.mark.parametrize('dtype', DTYPES)
def test_a_captured_never_run_rollout_replays_like_eager(runs, dtype):
  paced = runs['paced']
  for rep in range(2):
    tag = '%s/graph/%d' % (dtype, rep)
    same(paced, paced, tag, '%s/two/%d' % (dtype, rep), FIELDS + ('cost',))
    same(paced, runs['twin'], tag, tag, FIELDS + ('cost',))
    assert paced[tag + '/progress'].tolist() == [N, N] + [0] * 14, tag      # (re-zeroed inside the graph)


@pytest.mark.parametrize('dtype', DTYPES)
def test_resets_around_a_boundary_equal_the_twin(runs, dtype):
  tag = '%s/guard/0' % dtype
  same(runs['paced'], runs['twin'], tag, tag, FIELDS + ('cost',))
  assert runs['paced'][tag + '/progress'].tolist() == [64] + [0] * 15
  done = runs['paced'][tag + '/done_rec'].astype(bool)
  ends = np.flatnonzero(done.any(axis=1))
  assert {1, 2, 3}.issubset(set(ends.tolist()))   # inside the first segment, on its last step, on the next one's first
