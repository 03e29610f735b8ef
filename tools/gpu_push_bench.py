"""GPU MEASUREMENT: what the external base wrenches cost (solo_push_kernel) against the kernel the engine launches for the same
configuration without a block, and against solo_act_kernel (the body the push kernels add the wrench to), at 4096 robots in f64 and
f32, position and PD control, on the benchmark workload (TorsoIMU + MotorEncoder, the stand reward, TimeBased(1000), auto-reset), as
recorded rollouts of plan(20): one launch of 20 steps with every output recorded.  Two blocks: ALL ZEROS - the motion is the replaced
kernel's (checked here too), so the ratio is the kernel's own cost - and a RANDOM block (horizontal force components up to 24.5 N -
about the robot's weight -, torque components up to 1 N m), whose ratio also carries what the pushed robots' different motion costs the solver.  One process; every timed region
starts from reset(), is bracketed by HIP events on the launch stream, and the series alternate round after round; medians over the
rounds are reported, with an A/A pair (the zero-block push kernel measured twice per round) to show the spread of the run.
  python tools/gpu_push_bench.py [--rounds 20] [--out profiles/push_bench.log]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--n', type=int, default=4096)
  ap.add_argument('--steps', type=int, default=20)
  ap.add_argument('--rounds', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  import numpy as np
  import torch
  from gym_solo_amd import abi
  from gym_solo_amd.envs.solo8v2vanilla import Solo8VanillaConfig, Solo8VanillaEnv
  from gym_solo_amd.workloads import register_benchmark_workload
  rng = np.random.default_rng(0)
  kp, kd = rng.uniform(1.0, 4.0, 12), rng.uniform(0.01, 0.05, 12)
  n, k = args.n, args.steps

  def make(dtype, mode):
    cfg = Solo8VanillaConfig()
    cfg.dtype, cfg.num_envs, cfg.auto_reset = dtype, n, True
    if mode == 'pd':
      cfg.control_mode, cfg.pd_kp, cfg.pd_kd = 'pd', kp, kd
    env = Solo8VanillaEnv(config=cfg)
    register_benchmark_workload(env, max_steps=1000)
    env._ensure_program()
    env.engine.reserve(k)
    return env

  def timed(eng, fn):
    eng.reset()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)

  def compare(series):
    ts = {name: [] for name in series}
    for rnd in range(args.warmup + args.rounds):
      for name, thunk in series.items():
        ms = thunk()
        if rnd >= args.warmup:
          ts[name].append(ms)
    return {name: statistics.median(v) for name, v in ts.items()}

  lines = []

  def emit(rec):
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)

  for dtype in ('float64', 'float32'):
    tdt = torch.float64 if dtype == 'float64' else torch.float32
    for mode in ('position', 'pd'):
      zero, rnd, act, old = make(dtype, mode), make(dtype, mode), make(dtype, mode), make(dtype, mode)
      zero.engine.set_base_wrench({})
      g = torch.Generator(device='cuda').manual_seed(1)
      w = torch.zeros(n, abi.WRENCH_WIDTH, device='cuda', dtype=tdt)
      w[:, 0:2] = (torch.rand(n, 2, device='cuda', dtype=tdt, generator=g) * 2 - 1) * (2.5 * 9.81)
      w[:, 3:6] = torch.rand(n, 3, device='cuda', dtype=tdt, generator=g) * 2 - 1
      rnd.engine.set_base_wrench(w)
      act.engine.set_actuators(torch.ones(n, abi.ACTUATOR_WIDTH, device='cuda', dtype=tdt))
      r = torch.rand(k, n, 12, device='cuda', dtype=tdt, generator=g) * 2 - 1
      settle = torch.as_tensor(np.array(list(zero.engine.cfg.settle_targets)), device='cuda', dtype=tdt)
      acts = ((r * 6.28) if mode == 'position' else (settle + 0.6 * r)).contiguous()
      envs = {'A': zero, 'A2': zero, 'R': rnd, 'ACT': act, 'B': old}
      outs = {name: e.engine.rollout_buffers(k) for name, e in envs.items() if name != 'A2'}
      outs['A2'] = outs['A']
      series = {name: (lambda e=e, o=outs[name]: timed(e.engine, lambda: e.engine.rollout(acts, abi.STEP_ALL, out=o))) for name, e in envs.items()}
      med = compare(series)
      same = all(torch.equal(x, y) for x, y in zip(outs['A'], outs['B'])) and torch.equal(zero.engine.state, old.engine.state)
      emit({'dtype': dtype, 'mode': mode, 'num_envs': n, 'steps': k, 'rounds': args.rounds, 'kernel': zero.engine.kernel_name,
            'replaces': old.engine.kernel_name, 'plan': zero.engine.plan(k), 'ms_push_zero_block': med['A'], 'ms_push_zero_block_again': med['A2'],
            'ms_push_random_block': med['R'], 'ms_act_kernel': med['ACT'], 'ms_replaced_kernel': med['B'],
            'aa_spread': abs(med['A'] - med['A2']) / med['A'], 'push_zero_over_replaced': med['A'] / med['B'],
            'push_random_over_replaced': med['R'] / med['B'], 'push_zero_over_act': med['A'] / med['ACT'], 'same_results_zero_block': bool(same)})
      for e in (zero, rnd, act, old):
        e._close()
  if args.out:
    with open(args.out, 'w') as f:
      f.write('# tools/gpu_push_bench.py: HIP-event medians over %d alternating rounds, one process; A/A = the zero-block push kernel twice\n' % args.rounds)
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
