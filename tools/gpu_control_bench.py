"""GPU MEASUREMENT: env-steps/s of the three joint control modes (position, torque, PD) at 4096 robots in f64 and f32, on
the benchmark workload (TorsoIMU + MotorEncoder, the stand reward, TimeBased) with the driver geometry (engine.plan(20):
rollouts of 20 steps, every step's outputs recorded).  One process and ONE engine per precision; the modes alternate
round after round (solo_engine_set_control between the timed regions), each timed region is a rollout measured with HIP
events (solo_engine_time_rollout, as bench.py's kernel time) after a warm-up, and the median of the repeats is reported.
Two workloads:
  own        every mode on its own action distribution (position: U(+-2 pi) targets; torque: U(+-2.5) N m; PD: the settle
             pose + U(+-0.6) rad) - different motions, different contact sets;
  saturated  the SAME motion in every mode: per robot, step and joint a sign s; position mode targets s 1e3 rad (every
             motor row saturates at +-limit dt), torque mode tau = s L, PD mode kp = 1e3, kd = 0 and targets s 1e3 rad (the
             clamp gives s L) - identities (b) / (d) of tests/test_gpu_control.py: the kernels' own cost, side by side.
  python tools/gpu_control_bench.py [--rounds 30] [--out profiles/control_modes_bench.log]"""
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
  import numpy as np
  import torch
  from gym_solo_amd import abi
  from gym_solo_amd.envs.solo8v2vanilla import Solo8VanillaConfig, Solo8VanillaEnv
  from gym_solo_amd.workloads import register_benchmark_workload
  rng = np.random.default_rng(0)
  kp, kd = rng.uniform(1.0, 4.0, 12), rng.uniform(0.01, 0.05, 12)
  lines = []
  for dtype in ('float64', 'float32'):
    tdt = torch.float64 if dtype == 'float64' else torch.float32
    cfg = Solo8VanillaConfig()
    cfg.dtype, cfg.num_envs, cfg.auto_reset = dtype, args.n, True
    env = Solo8VanillaEnv(config=cfg)
    register_benchmark_workload(env, max_steps=1000)
    env._ensure_program()
    eng = env.engine
    g = torch.Generator(device='cuda').manual_seed(1)
    settle = torch.as_tensor(np.array(list(eng.cfg.settle_targets)), device='cuda', dtype=tdt)
    r = torch.rand(args.k, args.n, 12, device='cuda', dtype=tdt, generator=g) * 2 - 1
    sgn = torch.where(r < 0, -1.0, 1.0).to(tdt)
    L = float(eng.cfg.motor_torque_limit)
    work = {
      'own': ({'position': (r * 6.28).contiguous(), 'torque': (r * 2.5).contiguous(), 'pd': (settle + 0.6 * r).contiguous()},
              (kp, kd)),
      'saturated': ({'position': (sgn * 1e3).contiguous(), 'torque': (sgn * L).contiguous(), 'pd': (sgn * 1e3).contiguous()},
                    (np.full(12, 1e3), np.zeros(12))),
    }
    bufs = eng.rollout_buffers(args.k)
    modes = ('position', 'torque', 'pd')
    plan = eng.plan(args.k)
    times = {(w, m): [] for w in work for m in modes}
    for rnd in range(args.warmup + args.rounds):
      for w, (acts, (wkp, wkd)) in work.items():
        for m in modes:
          eng.set_control(m, kp=wkp if m == 'pd' else None, kd=wkd if m == 'pd' else None)
          eng.reset()
          ms = eng.time_rollout(acts[m], abi.STEP_ALL, out=bufs) * plan['launches']
          if rnd >= args.warmup:
            times[(w, m)].append(ms)
    for (w, m), ts in times.items():
      med = statistics.median(ts)
      rec = {'dtype': dtype, 'workload': w, 'mode': m, 'num_envs': args.n, 'steps': args.k, 'plan': plan, 'repeats': len(ts),
             'ms_per_rollout_median': med, 'ms_min': min(ts), 'ms_max': max(ts),
             'env_steps_per_s': args.n * args.k / (med * 1e-3), 'kernel': None}
      eng.set_control(m, kp=kp if m == 'pd' else None, kd=kd if m == 'pd' else None)
      rec['kernel'] = eng.kernel_name
      lines.append(json.dumps(rec))
      print(lines[-1], flush=True)
    env._close()
  if args.out:
    with open(args.out, 'w') as f:
      f.write('# tools/gpu_control_bench.py: HIP-event time of one recorded rollout (median over rounds, modes alternating)\n')
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
