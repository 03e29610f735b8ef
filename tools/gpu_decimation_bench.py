"""GPU MEASUREMENT: control decimation (Engine.set_decimation, solo_decim_kernel) against what a user had without it, at 4096
robots in f64 and f32, position and PD control, D in {1, 2, 4, 10}, on the benchmark workload (TorsoIMU + MotorEncoder, the
stand reward, TimeBased(1000), auto-reset).  One process; per precision and mode one decimated engine and one D = 1 engine (the
TWIN: the kernels as they were before decimation).  Every timed region starts from reset(), is bracketed by HIP events on
the launch stream, and the series of a comparison alternate round after round; medians over the rounds are reported, with an
A/A pair (the decimated series measured twice per round) to show the spread of the run.
  (a) closed   ms per CONTROL step of `steps` decimated step() calls (one launch each) against the twin sequence: per control
               step D - 1 step(STEP_PHYSICS) launches and one step(STEP_ALL);
  (b) fused    a recorded rollout of 20 control steps against the workaround: an undecimated recorded rollout of 20 D steps
               with every action row repeated D times (D times the records, D times the epilogue work - and not the same
               episode bookkeeping);
  (c) policy   1000 control steps at D = 4 under the engine's own plan (S = 250 / D control steps per launch) against
               steps_per_launch = 250 control steps.
  python tools/gpu_decimation_bench.py [--rounds 20] [--out profiles/decimation_bench.log]"""
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
  ap.add_argument('--steps', type=int, default=20, help='control steps per timed region of (a) and (b)')
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

  def make(dtype, mode, **kw):
    cfg = Solo8VanillaConfig()
    cfg.dtype, cfg.num_envs, cfg.auto_reset = dtype, n, True
    if mode == 'pd':
      cfg.control_mode, cfg.pd_kp, cfg.pd_kd = 'pd', kp, kd
    for key, v in kw.items():
      setattr(cfg, key, v)
    env = Solo8VanillaEnv(config=cfg)
    register_benchmark_workload(env, max_steps=1000)
    env._ensure_program()
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
    """series: {name: thunk returning ms}; alternating rounds -> {name: median ms}"""
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
      dec, twin = make(dtype, mode), make(dtype, mode)
      d_eng, t_eng = dec.engine, twin.engine
      g = torch.Generator(device='cuda').manual_seed(1)
      r = torch.rand(k, n, 12, device='cuda', dtype=tdt, generator=g) * 2 - 1
      settle = torch.as_tensor(np.array(list(d_eng.cfg.settle_targets)), device='cuda', dtype=tdt)
      acts = ((r * 6.28) if mode == 'position' else (settle + 0.6 * r)).contiguous()
      rows = [acts[i].contiguous() for i in range(k)]
      for D in (1, 2, 4, 10):
        d_eng.set_decimation(D)
        d_eng.reserve(k)
        t_eng.reserve(k * D)
        repeated = acts.repeat_interleave(D, dim=0).contiguous()
        out_d, out_t = d_eng.rollout_buffers(k), t_eng.rollout_buffers(k * D)

        def closed_dec():
          for a in rows:
            d_eng.step(a, abi.STEP_ALL)

        def closed_twin():
          for a in rows:
            for _ in range(D - 1):
              t_eng.step(a, abi.STEP_PHYSICS)
            t_eng.step(a, abi.STEP_ALL)

        med = compare({'A': lambda: timed(d_eng, closed_dec), 'A2': lambda: timed(d_eng, closed_dec), 'B': lambda: timed(t_eng, closed_twin)})
        emit({'part': 'a_closed_loop', 'dtype': dtype, 'mode': mode, 'D': D, 'num_envs': n, 'control_steps': k, 'rounds': args.rounds,
              'kernel': d_eng.kernel_name, 'ms_per_control_step_decimated': med['A'] / k, 'ms_per_control_step_decimated_again': med['A2'] / k,
              'ms_per_control_step_twin': med['B'] / k, 'aa_spread': abs(med['A'] - med['A2']) / med['A'], 'twin_over_decimated': med['B'] / med['A']})
        med = compare({'A': lambda: timed(d_eng, lambda: d_eng.rollout(acts, abi.STEP_ALL, out=out_d)),
                       'A2': lambda: timed(d_eng, lambda: d_eng.rollout(acts, abi.STEP_ALL, out=out_d)),
                       'B': lambda: timed(t_eng, lambda: t_eng.rollout(repeated, abi.STEP_ALL, out=out_t))})
        emit({'part': 'b_fused', 'dtype': dtype, 'mode': mode, 'D': D, 'num_envs': n, 'control_steps': k, 'rounds': args.rounds,
              'plan_decimated': d_eng.plan(k), 'plan_workaround': t_eng.plan(k * D), 'ms_rollout_decimated': med['A'],
              'ms_rollout_decimated_again': med['A2'], 'ms_rollout_workaround': med['B'], 'aa_spread': abs(med['A'] - med['A2']) / med['A'],
              'workaround_over_decimated': med['B'] / med['A'],
              'env_control_steps_per_s': n * k / (med['A'] * 1e-3), 'physics_steps_per_s': n * k * D / (med['A'] * 1e-3)})
        del out_d, out_t, repeated
      dec._close(); twin._close()
    # (c) the launch policy at D = 4: 1000 control steps, position control
    auto, wide = make(dtype, 'position'), make(dtype, 'position', steps_per_launch=250)
    for e in (auto, wide):
      e.engine.set_decimation(4)
      e.engine.reserve(1000)
    g = torch.Generator(device='cuda').manual_seed(2)
    long_acts = ((torch.rand(1000, n, 12, device='cuda', dtype=tdt, generator=g) * 2 - 1) * 6.28).contiguous()
    med = compare({'A': lambda: timed(auto.engine, lambda: auto.engine.rollout(long_acts, abi.STEP_ALL)),
                   'A2': lambda: timed(auto.engine, lambda: auto.engine.rollout(long_acts, abi.STEP_ALL)),
                   'B': lambda: timed(wide.engine, lambda: wide.engine.rollout(long_acts, abi.STEP_ALL))})
    emit({'part': 'c_launch_policy', 'dtype': dtype, 'D': 4, 'num_envs': n, 'control_steps': 1000, 'rounds': args.rounds,
          'plan_default': auto.engine.plan(1000), 'plan_250': wide.engine.plan(1000), 'ms_default': med['A'], 'ms_default_again': med['A2'],
          'ms_250': med['B'], 'aa_spread': abs(med['A'] - med['A2']) / med['A'], 's250_over_default': med['B'] / med['A'],
          'physics_steps_per_s_default': n * 4000 / (med['A'] * 1e-3), 'physics_steps_per_s_250': n * 4000 / (med['B'] * 1e-3)})
    auto._close(); wide._close()
  if args.out:
    with open(args.out, 'w') as f:
      f.write('# tools/gpu_decimation_bench.py: HIP-event medians over %d alternating rounds, one process; A/A = the decimated series twice\n' % args.rounds)
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
