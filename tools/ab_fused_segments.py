"""Same-call A/B/A of engine-library builds for the fused-segments change (boxes differ by 2-3 %: only numbers from ONE call compare).
Every library runs in a child process of its own (SOLO_HIP_LIB is read at import), the libraries alternate, ROUNDS rounds:

  python tools/ab_fused_segments.py [--rounds 2] [--repeats 6] PARENT.so THIS.so PARENT_COPY.so

Workloads (bench.py's environment, 4096 robots, the engine's own geometry; env-steps/s by wall clock, device sync on both sides):
f64: rollouts of 3000 and of 1000 steps, a rollout of 20 steps, the closed loop (20 single-step launches); f32: 3000 and 20.
Prints every sample, then per workload the median of all repeats of every library, the A/A spread (|first - third| / first) and the
second library's gain over the first in units of that spread."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = {'float64': ('k3000', 'k1000', 'k20', 'closed'), 'float32': ('k3000', 'k20')}


def child(spec):
  sys.path.insert(0, ROOT)
  import torch
  import bench
  from gym_solo_amd import abi
  dtype, n = spec['dtype'], 4096
  tdt = torch.float32 if dtype == 'float32' else torch.float64
  out = {}
  for leg in LEGS[dtype]:
    closed = leg == 'closed'
    k = 20 if closed else int(leg[1:])
    env = bench.build_env(n, 0, dtype, steps_per_launch=1 if closed else -1, rollout_streams=1 if closed else -1, migrate_steps=0 if closed else -1)
    eng = env.engine
    gen = torch.Generator(device='cuda').manual_seed(1234)
    bench.desynchronise_episodes(eng, gen)
    pool = lambda steps: (torch.rand(steps, n, abi.NUM_JOINTS, device='cuda', dtype=tdt, generator=gen) * 2 - 1) * 6.283185307179586
    bufs = None if closed else eng.rollout_buffers(k)
    def run(a):
      if closed:
        for i in range(a.shape[0]):
          eng.step(a[i], abi.STEP_ALL)
      else:
        eng.rollout(a, abi.STEP_ALL, out=bufs)
    a = pool(k)
    for _ in range(5 if k == 20 else 1):   # warm-up
      run(a)
    samples = []
    for _ in range(spec['repeats'] * (5 if k == 20 else 1)):
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      run(a)
      torch.cuda.synchronize()
      samples.append(n * k / (time.perf_counter() - t0))
    out[leg] = {'samples': samples, 'kernel': eng.kernel_name, 'plan': None if closed else eng.plan(k)}
    env._close()
  print('AB_RESULT ' + json.dumps(out), flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=2)
  ap.add_argument('--repeats', type=int, default=6, help='timed repeats per workload inside a child (20-step workloads: five times as many)')
  ap.add_argument('libs', nargs=3)
  args = ap.parse_args()
  samples = {}   # (dtype, leg) -> [samples of library i]
  kernels = {}
  for rnd in range(args.rounds):
    for dtype in ('float64', 'float32'):
      for i, lib in enumerate(args.libs):
        env = dict(os.environ, SOLO_HIP_LIB=os.path.abspath(lib), SOLO_AB_CHILD=json.dumps({'dtype': dtype, 'repeats': args.repeats}))
        try:
          res = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        except subprocess.TimeoutExpired:
          print('%s: TIMEOUT' % lib, flush=True)
          raise SystemExit(1)   # (a hung GPU step: no further GPU step in this call)
        line = [l for l in res.stdout.decode().splitlines() if l.startswith('AB_RESULT ')]
        if res.returncode != 0 or not line:
          print('%s: FAILED rc=%d\n%s' % (lib, res.returncode, res.stderr.decode()[-2000:]), flush=True)
          raise SystemExit(1)
        for leg, r in json.loads(line[0][len('AB_RESULT '):]).items():
          samples.setdefault((dtype, leg), [[], [], []])[i] += r['samples']
          kernels[(dtype, leg, i)] = r['kernel']
          print('round %d %-8s %-7s lib %d (%s) %s: %s' % (rnd, dtype, leg, i, os.path.basename(lib), r['kernel'], ' '.join('%.4g' % s for s in r['samples'])), flush=True)
  print('---- medians of %d rounds (env-steps/s); library 0 = %s, 1 = %s, 2 = %s' % ((args.rounds,) + tuple(args.libs)))
  for (dtype, leg), per_lib in samples.items():
    m = [statistics.median(s) for s in per_lib]
    spread = abs(m[0] - m[2]) / m[0]
    gain = m[1] / m[0] - 1
    print('%-8s %-7s n=%3d each: %.4g  %.4g  %.4g ; A/A spread %.2f %% ; library 1 against 0: %+.2f %% = %.1f spreads ; kernel of library 1: %s' % (
      dtype, leg, len(per_lib[0]), m[0], m[1], m[2], 100 * spread, 100 * gain, gain / spread if spread > 0 else float('inf'), kernels[(dtype, leg, 1)]), flush=True)


if __name__ == '__main__':
  if os.environ.get('SOLO_AB_CHILD'):
    child(json.loads(os.environ['SOLO_AB_CHILD']))
  else:
    main()
