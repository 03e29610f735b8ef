"""GPU MEASUREMENT: what the state terminations cost (solo_term_kernel) against the kernel they replace, at 4096 robots in f64
and f32 on the benchmark workload (TorsoIMU + MotorEncoder, the stand reward, TimeBased(1000), auto-reset), as recorded rollouts
of plan(20): one launch of 20 control steps with every output recorded.  One process; every timed region starts from reset(), is
bracketed by HIP events on the launch stream, and the series of a comparison alternate round after round; medians over the
rounds are reported, with an A/A pair (the termination kernel measured twice per round) to show the spread of the run.
  (a) parity   [Height(-1e9), Tilt(cos = -2), TimeBased(1000)] - thresholds that never fire, so the motion is the same - against
               [Perpetual, Perpetual, TimeBased(1000)] on the kernel it replaces: solo_step_kernel (position, D = 1),
               solo_ctl_step_kernel (PD, D = 1), solo_decim_kernel (position, D = 4);
  (b) falls    the same workload over `--long` consecutive rollouts of 20 without a reset in between, with a tilt limit taken from
               the workload - the median over the robots of their largest tilt in a closed-loop run of the same actions on the
               time-only program, so that about half of the robots end an episode early - against the time-only program: the ms per
               rollout, the episodes ended and the Gauss-Seidel sweeps per robot-step of the last rollout (Engine.cost).
  python tools/gpu_terms_bench.py [--rounds 20] [--out profiles/terms_bench.log]"""
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
  ap.add_argument('--long', type=int, default=10, help='consecutive rollouts per timed region of (b)')
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  import numpy as np
  import torch
  from gym_solo_amd import abi
  from gym_solo_amd.core import termination as terms
  from gym_solo_amd.envs.solo8v2vanilla import Solo8VanillaConfig, Solo8VanillaEnv
  from gym_solo_amd.workloads import register_benchmark_workload
  rng = np.random.default_rng(0)
  kp, kd = rng.uniform(1.0, 4.0, 12), rng.uniform(0.01, 0.05, 12)
  n, k = args.n, args.steps

  def make(dtype, mode, D, members):
    cfg = Solo8VanillaConfig()
    cfg.dtype, cfg.num_envs, cfg.auto_reset = dtype, n, True
    if mode == 'pd':
      cfg.control_mode, cfg.pd_kp, cfg.pd_kd = 'pd', kp, kd
    env = Solo8VanillaEnv(config=cfg, decimation=D)
    register_benchmark_workload(env, max_steps=1000)
    env.termination_factory._terminations = []
    env.termination_factory.register_termination(*members(env))
    env._ensure_program()
    env.engine.reserve(k)
    return env

  def never(env):
    tilt = terms.TiltTermination(env.robot, 1.0)
    tilt.value = -2.0   # (cos = -2: out of reach)
    return [terms.HeightTermination(env.robot, -1e9), tilt, terms.TimeBasedTermination(1000)]

  def plain(env):
    return [terms.PerpetualTermination(), terms.PerpetualTermination(), terms.TimeBasedTermination(1000)]

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
    for mode, D in (('position', 1), ('pd', 1), ('position', 4)):
      new, old = make(dtype, mode, D, never), make(dtype, mode, D, plain)
      g = torch.Generator(device='cuda').manual_seed(1)
      r = torch.rand(k, n, 12, device='cuda', dtype=tdt, generator=g) * 2 - 1
      settle = torch.as_tensor(np.array(list(new.engine.cfg.settle_targets)), device='cuda', dtype=tdt)
      acts = ((r * 6.28) if mode == 'position' else (settle + 0.6 * r)).contiguous()
      out_new, out_old = new.engine.rollout_buffers(k), old.engine.rollout_buffers(k)
      run_new = lambda: timed(new.engine, lambda: new.engine.rollout(acts, abi.STEP_ALL, out=out_new))
      run_old = lambda: timed(old.engine, lambda: old.engine.rollout(acts, abi.STEP_ALL, out=out_old))
      med = compare({'A': run_new, 'A2': run_new, 'B': run_old})
      same = all(torch.equal(x, y) for x, y in zip(out_new, out_old)) and torch.equal(new.engine.state, old.engine.state)
      emit({'part': 'a_parity', 'dtype': dtype, 'mode': mode, 'D': D, 'num_envs': n, 'control_steps': k, 'rounds': args.rounds,
            'kernel': new.engine.kernel_name, 'replaces': old.engine.kernel_name, 'plan': new.engine.plan(k), 'ms_term_kernel': med['A'],
            'ms_term_kernel_again': med['A2'], 'ms_replaced_kernel': med['B'], 'aa_spread': abs(med['A'] - med['A2']) / med['A'],
            'term_over_replaced': med['A'] / med['B'], 'same_results': bool(same)})
      new._close(); old._close()
    # (b) a tilt limit from the workload over `long` consecutive rollouts, position control, D = 1
    time_only = make(dtype, 'position', 1, lambda e: [terms.TimeBasedTermination(1000)])
    g = torch.Generator(device='cuda').manual_seed(2)
    long_acts = [((torch.rand(k, n, 12, device='cuda', dtype=tdt, generator=g) * 2 - 1) * 6.28).contiguous() for _ in range(args.long)]
    # (the limit: every robot's smallest c = 1 - 2 (qx^2 + qy^2) over the same steps run closed loop, then the median of them)
    time_only.engine.reset()
    lowest = torch.ones(n, device='cuda', dtype=tdt)
    for a in long_acts:
      for i in range(k):
        time_only.engine.step(a[i].contiguous(), abi.STEP_ALL)
        q = time_only.engine.state[:, abi.S_QUAT:abi.S_QUAT + 2]
        lowest = torch.minimum(lowest, 1 - 2 * (q * q).sum(dim=1))
    cos_limit = float(lowest.median().item())

    def falling(env):
      tilt = terms.TiltTermination(env.robot, 1.0)
      tilt.value = cos_limit
      return [tilt, terms.TimeBasedTermination(1000)]

    fall = make(dtype, 'position', 1, falling)
    outs = {id(e): e.engine.rollout_buffers(k) for e in (fall, time_only)}

    def chain(env):
      def go():
        for a in long_acts:
          env.engine.rollout(a, abi.STEP_ALL, out=outs[id(env)])
      return go

    def sweeps(env):
      return float(env.engine.cost.double().mean().item()) / k

    stat = {}
    for name, env in (('tilt', fall), ('time_only', time_only)):
      env.engine.reset()
      env.engine.stats_shards.zero_()
      chain(env)()
      env.engine.synchronize()
      stat[name] = dict(episodes=float(env.engine.stats[2].item()), sweeps_per_robot_step_last_rollout=sweeps(env))
    med = compare({'A': lambda: timed(fall.engine, chain(fall)), 'A2': lambda: timed(fall.engine, chain(fall)),
                   'B': lambda: timed(time_only.engine, chain(time_only))})
    emit({'part': 'b_falls', 'dtype': dtype, 'mode': 'position', 'D': 1, 'num_envs': n, 'control_steps': k * args.long, 'rounds': args.rounds,
          'cos_max_tilt': cos_limit, 'max_tilt_rad': float(np.arccos(max(-1.0, min(1.0, cos_limit)))), 'kernel': fall.engine.kernel_name, 'against': time_only.engine.kernel_name,
          'ms_per_rollout_tilt': med['A'] / args.long, 'ms_per_rollout_tilt_again': med['A2'] / args.long,
          'ms_per_rollout_time_only': med['B'] / args.long, 'aa_spread': abs(med['A'] - med['A2']) / med['A'],
          'tilt_over_time_only': med['A'] / med['B'], 'episodes_ended_tilt': stat['tilt']['episodes'],
          'episodes_ended_time_only': stat['time_only']['episodes'],
          'sweeps_per_robot_step_tilt': stat['tilt']['sweeps_per_robot_step_last_rollout'],
          'sweeps_per_robot_step_time_only': stat['time_only']['sweeps_per_robot_step_last_rollout']})
    fall._close(); time_only._close()
  if args.out:
    with open(args.out, 'w') as f:
      f.write('# tools/gpu_terms_bench.py: HIP-event medians over %d alternating rounds, one process; A/A = the termination kernel twice\n' % args.rounds)
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
