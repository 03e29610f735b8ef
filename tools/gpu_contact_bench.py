"""GPU MEASUREMENT: what contact sensing costs, at 4096 robots in f64 and f32, on the benchmark workload (TorsoIMU +
MotorEncoder, the stand reward, TimeBased) with the driver geometry (engine.plan(20): rollouts of 20 steps, every step's
outputs recorded).  Three variants on ONE engine per precision, alternating round after round:
  off    sensing off (the product kernels, solo_step_kernel);
  on     sensing on, the same program (solo_contact_kernel: the record is written, nothing reads it);
  foot   sensing on, FootContact added to the program (four more observation elements read the foot forces).
Each timed region is one rollout measured with HIP events (solo_engine_time_rollout, as bench.py's kernel time) after a
warm-up; the median of the repeats is reported, with the slowdown against `off`.
  python tools/gpu_contact_bench.py [--rounds 30] [--out profiles/contact_sensing_bench.log]"""
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
  ap.add_argument('--k', type=int, default=20)
  ap.add_argument('--rounds', type=int, default=30)
  ap.add_argument('--warmup', type=int, default=5)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  import torch
  from gym_solo_amd import abi
  from gym_solo_amd.core.obs import FootContact
  from gym_solo_amd.envs.solo8v2vanilla import Solo8VanillaConfig, Solo8VanillaEnv
  from gym_solo_amd.workloads import register_benchmark_workload
  lines = []
  for dtype in ('float64', 'float32'):
    tdt = torch.float64 if dtype == 'float64' else torch.float32
    cfg = Solo8VanillaConfig()
    cfg.dtype, cfg.num_envs, cfg.auto_reset = dtype, args.n, True
    env = Solo8VanillaEnv(config=cfg)
    register_benchmark_workload(env, max_steps=1000)
    env._ensure_program()
    eng = env.engine
    p_base = eng.program
    env.obs_factory.register_observation(FootContact(env.robot))   # (turns sensing on)
    env._ensure_program()
    p_foot = eng.program
    g = torch.Generator(device='cuda').manual_seed(1)
    acts = ((torch.rand(args.k, args.n, 12, device='cuda', dtype=tdt, generator=g) * 2 - 1) * 6.28).contiguous()
    plan = eng.plan(args.k)
    variants = ('off', 'on', 'foot')
    bufs, kernels, times = {}, {}, {v: [] for v in variants}

    def select(v):
      if v == 'off':
        eng.set_program(p_base)
        eng.set_contact_sensing(False)
      else:
        eng.set_contact_sensing(True)
        eng.set_program(p_foot if v == 'foot' else p_base)
      if v not in bufs:
        bufs[v] = eng.rollout_buffers(args.k)
        kernels[v] = eng.kernel_name
    for rnd in range(args.warmup + args.rounds):
      for v in variants:
        select(v)
        eng.reset()
        ms = eng.time_rollout(acts, abi.STEP_ALL, out=bufs[v]) * plan['launches']
        if rnd >= args.warmup:
          times[v].append(ms)
    base = statistics.median(times['off'])
    for v in variants:
      ts = times[v]
      med = statistics.median(ts)
      rec = {'dtype': dtype, 'variant': v, 'num_envs': args.n, 'steps': args.k, 'plan': plan, 'repeats': len(ts),
             'ms_per_rollout_median': med, 'ms_min': min(ts), 'ms_max': max(ts),
             'env_steps_per_s': args.n * args.k / (med * 1e-3), 'slowdown_vs_off': med / base - 1.0, 'kernel': kernels[v]}
      lines.append(json.dumps(rec))
      print(lines[-1], flush=True)
    env._close()
  if args.out:
    with open(args.out, 'w') as f:
      f.write('# tools/gpu_contact_bench.py: HIP-event time of one recorded rollout (median over rounds, variants alternating)\n')
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
