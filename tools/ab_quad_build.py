"""Same-call A/B of engine-library builds for the four-column f64 Delassus build (ColumnBank<double>::build_quad; boxes differ by
2-3 %: only numbers from ONE call compare).  Every library runs in a child process of its own (SOLO_HIP_LIB is read at import), the
libraries alternate, ROUNDS rounds:

  python tools/ab_quad_build.py [--rounds 2] [--repeats 6] PARENT.so libsolo_hip.so libsolo_hip_pair_only.so PARENT_COPY.so

The first and the last library are the A/A pair (the parent commit's library and a second copy of it); everything between them is a
candidate (this tree's library, and its pair-only twin - the parent's kernels instruction for instruction: the null check).

Workloads (bench.py's environment, 4096 robots, f64 - the f32 kernels are the parent's byte for byte; env-steps/s by wall clock,
device sync on both sides): rollouts of 3000 steps under the engine's own geometry (bench.py --steps 3000), of 20 steps, and the
closed loop (20 single-step launches).
Prints every sample, then per workload the median of all repeats of every library, the A/A spread (|first - last| / first), every
candidate's gain over both parents in units of that spread, and whether any parent sample reaches the candidate's lowest."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = {'float64': ('k3000', 'k20', 'closed')}


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
  ap.add_argument('libs', nargs='+')
  args = ap.parse_args()
  if not 3 <= len(args.libs) <= 5:
    ap.error('PARENT.so, one to three candidates, PARENT_COPY.so')
  nl = len(args.libs)
  samples = {}   # (dtype, leg) -> [samples of library i]
  kernels = {}
  for rnd in range(args.rounds):
    for dtype in sorted(LEGS):
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
          samples.setdefault((dtype, leg), [[] for _ in range(nl)])[i] += r['samples']
          kernels[(dtype, leg, i)] = r['kernel']
          print('round %d %-8s %-7s lib %d (%s) %s %s: %s' % (rnd, dtype, leg, i, os.path.basename(lib), r['kernel'], 'slices %s' % (r['plan'] or {}).get('slices'),
                                                              ' '.join('%.5g' % s for s in r['samples'])), flush=True)
  print('---- medians of %d rounds (env-steps/s); libraries: %s' % (args.rounds, ', '.join('%d = %s' % (i, l) for i, l in enumerate(args.libs))))
  for (dtype, leg), per_lib in samples.items():
    m = [statistics.median(s) for s in per_lib]
    spread = abs(m[0] - m[-1]) / m[0]
    print('%-8s %-7s n=%3d each: %s ; A/A spread %.2f %%' % (dtype, leg, len(per_lib[0]), '  '.join('%.5g' % x for x in m), 100 * spread), flush=True)
    for c in range(1, nl - 1):
      gains = [m[c] / m[0] - 1, m[c] / m[-1] - 1]
      reach = max(max(per_lib[0]), max(per_lib[-1])) >= min(per_lib[c])
      print('      library %d against the parents: %+.2f %% / %+.2f %% = %.1f / %.1f spreads ; a parent sample reaches its lowest: %s ; kernel %s' % (
        c, 100 * gains[0], 100 * gains[1], gains[0] / spread if spread > 0 else float('inf'), gains[1] / spread if spread > 0 else float('inf'),
        'yes' if reach else 'no', kernels[(dtype, leg, c)]), flush=True)


if __name__ == '__main__':
  if os.environ.get('SOLO_AB_CHILD'):
    child(json.loads(os.environ['SOLO_AB_CHILD']))
  else:
    main()
