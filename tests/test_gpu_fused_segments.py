"""Fused segments on the GPU (solo_roll_kernel: consecutive S-step launches of a rollout slice as ONE launch whose waves run the
output epilogue after every S steps): bit for bit against an engine that runs every step as a launch of its own
(steps_per_launch = 1: no record scratch, no epilogue, in-place outputs), the kernel names the engine reports, and the capture of a
never-run 600-step rollout after reserve()."""
import numpy as np
import pytest

from epilogue_cases import pass_steps

pytestmark = pytest.mark.gpu

N = 64


def make_env(dtype, n, max_steps, **geometry):
  import torch
  if not torch.cuda.is_available():
    pytest.fail('GPU tests need a visible MI355X')
  from gym_solo_amd.envs.solo8v2vanilla import Solo8VanillaConfig, Solo8VanillaEnv
  from gym_solo_amd.workloads import register_benchmark_workload
  cfg = Solo8VanillaConfig()
  cfg.dtype, cfg.num_envs, cfg.auto_reset = dtype, n, True
  for key, value in geometry.items():
    setattr(cfg, key, value)
  env = Solo8VanillaEnv(config=cfg, copy_outputs=False)
  register_benchmark_workload(env, max_steps=max_steps)   # TimeBased(max_steps)
  env._ensure_program()
  return env


def cases(dtype):
  p = pass_steps(dtype)
  return [(3, 10), (p + 1, 2 * (p + 1) + 1), (2, 17 * 2 + 1)]   # (the last one crosses kMaxFusedSegments = 16: two launches per slice)


_REFERENCE = {}


def inputs(dtype):
  """actions [max K][N][12] and the staggered TimeBased counters (0 .. 7), per precision; the single-step engine's results per K"""
  import torch
  if dtype not in _REFERENCE:
    tdt = torch.float32 if dtype == 'float32' else torch.float64
    g = torch.Generator(device='cuda').manual_seed(31)
    kmax = max(k for _, k in cases(dtype))
    acts = (torch.rand(kmax, N, 12, device='cuda', dtype=tdt, generator=g) * 2 - 1) * 6.28
    tc = torch.zeros(N, 4, device='cuda', dtype=torch.int32)
    tc[:, 0] = torch.arange(N, device='cuda', dtype=torch.int32) % 8
    _REFERENCE[dtype] = (acts, tc, {})
  return _REFERENCE[dtype]


def everything(eng, rec):
  eng.synchronize()
  out = dict(obs_rec=rec[0], reward_rec=rec[1], done_rec=rec[2], obs=eng.obs, reward=eng.reward, done=eng.done, state=eng.state,
             term_count=eng.term_count, targets=eng.targets, stats=eng.stats_shards)
  return {k: v.detach().cpu().numpy().copy() for k, v in out.items()}


def run(dtype, k, **geometry):
  from gym_solo_amd import abi
  acts, tc, _ = inputs(dtype)
  env = make_env(dtype, N, 7, **geometry)
  eng = env.engine
  eng.term_count.copy_(tc)
  got = everything(eng, eng.rollout(acts[:k], abi.STEP_ALL, record=True))
  name, plan = eng.kernel_name, eng.plan(k)
  env._close()
  return got, name, plan


def single_steps(dtype, k):
  """steps_per_launch = 1 on one chain: computed once per (precision, K), shared"""
  ref = inputs(dtype)[2]
  if k not in ref:
    got, name, plan = run(dtype, k, steps_per_launch=1, rollout_streams=1)
    assert plan['steps_per_launch'] == 1 and plan['launches'] == k and name.startswith('solo_step_kernel<')
    ref[k] = got
  return ref[k]


@pytest.mark.parametrize('streams', [1, 2])
@pytest.mark.parametrize('which', [0, 1, 2], ids=['S3-K10', 'Spass+1-K2S+1', 'S2-K35'])
@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_fused_segments_equal_single_step_launches(dtype, which, streams):
  S, K = cases(dtype)[which]
  want = single_steps(dtype, K)
  got, name, plan = run(dtype, K, steps_per_launch=S, rollout_streams=streams)
  assert name == 'solo_roll_kernel<%s>' % ('double' if dtype == 'float64' else 'float')
  # (the report is the one of before: S-step segments per slice)
  assert plan['steps_per_launch'] == S and plan['launches'] == -(-K // S) and plan['slices'] == streams and plan['migrate_steps'] == 0
  for key in want:   # (the statistics too: 64 robots on 64 shards - every robot's episodes add up in its own row, in step order)
    np.testing.assert_array_equal(got[key], want[key], err_msg=key)
  done = want['done_rec'].astype(bool)
  ends = np.flatnonzero(done.any(axis=1))
  assert any(s % S == S - 1 and s != K - 1 for s in ends) and any(s % S == 0 and s > 0 for s in ends) and done[K - 1].any()


def test_the_other_kernels_keep_their_names():
  """a K = 20 rollout is one launch of the step kernel; a torque-control engine keeps the control kernel over several launches; and
  after a fused rollout a single-launch rollout reports the step kernel again"""
  import torch
  from gym_solo_amd import abi
  env = make_env('float64', N, 7)
  eng = env.engine
  acts = torch.zeros(300, N, 12, device='cuda', dtype=torch.float64)
  assert eng.kernel_name == 'solo_step_kernel<double, true, false, false>'
  eng.rollout(acts[:20], abi.STEP_ALL)
  assert eng.kernel_name == 'solo_step_kernel<double, true, false, false>' and eng.plan(20)['launches'] == 1
  eng.rollout(acts, abi.STEP_ALL)                       # 250 + 50 on two slices
  assert eng.kernel_name == 'solo_roll_kernel<double>' and eng.plan(300)['steps_per_launch'] == 250
  eng.rollout(acts[:20], abi.STEP_ALL)
  assert eng.kernel_name == 'solo_step_kernel<double, true, false, false>'
  eng.rollout(acts, abi.STEP_ALL)
  eng.set_control('torque')
  assert eng.kernel_name == 'solo_ctl_step_kernel<double, true>'
  eng.rollout(acts, abi.STEP_ALL)
  assert eng.kernel_name == 'solo_ctl_step_kernel<double, true>'
  eng.synchronize()
  env._close()


def test_a_never_run_600_step_rollout_is_capturable_after_reserve():
  """256 robots, the engine's own geometry: segments of 250, 250 and 100 steps on two slices.  reserve(600) has to prepare the
  two-slice geometry - its streams - although the 250-step single launch in front of it has the same S (for_each_geometry compares
  the slices too); the captured rollout's replays equal an eager engine's rollouts bit for bit."""
  import torch
  from gym_solo_amd import abi
  eager, captured = make_env('float64', 256, 99), make_env('float64', 256, 99)
  n, k = 256, 600
  assert captured.engine.plan(k) == dict(captured.engine.plan(k), steps_per_launch=250, launches=3, slices=2, migrate_steps=0)
  g = torch.Generator(device='cuda').manual_seed(17)
  static = torch.zeros(k, n, 12, device='cuda', dtype=torch.float64)
  out = captured.engine.rollout_buffers(k)
  captured.engine.reserve(k)                 # (the captured engine has never launched a rollout)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    captured.engine.rollout(static, abi.STEP_ALL, out=out)
  assert captured.engine.kernel_name == 'solo_roll_kernel<double>'
  for rep in range(2):
    acts = (torch.rand(k, n, 12, device='cuda', dtype=torch.float64, generator=g) * 2 - 1) * 6.28
    want = eager.engine.rollout(acts, abi.STEP_ALL, record=True)
    static.copy_(acts)
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(want, out):
      assert torch.equal(x, y), rep
    assert torch.equal(eager.engine.state, captured.engine.state), rep
    assert torch.equal(eager.engine.obs, captured.engine.obs) and torch.equal(eager.engine.done, captured.engine.done), rep
  assert bool(out[2].any())
  for env in (eager, captured):
    env._close()
