"""DIAGNOSTIC: how unequal are the robots of one fused launch, and how much of the launch is tail?
Uses the light stamp build (make -C gym_solo_amd/csrc stamps_light): one stamp at each wave's
start and end, nothing per step.
usage: gpu_tail.py [--dtype float64,float32] [--geometry 4096x2,2048x1] [--rollout K] [steps_per_launch ...]
  --geometry  robots x rollout streams, one run each (default: $N robots, or 4096, on one and on two streams)
  --rollout   steps of the measured rollout (default: steps_per_launch - ONE fused launch per slice).  A longer rollout
              that the engine runs as one segmented launch per slice (solo_roll_kernel) has ONE wave life per robot, the
              whole rollout; run as separate launches, the stamps are those of the last launch.
Per run, next to the totals: the wave life by XCC, CU and SIMD, by SLICE (mean, p99, max, and when the slice's last wave ended),
its rank correlation with the robot's Gauss-Seidel sweeps over a segmented launch (slot 13 of the light build), and by wave slot % 3
(the phase of the priority rotation).  SOLO_HIP_LIB selects the stamps build (e.g. one made with -DSOLO_ROLL_PACING=0)."""
import argparse, sys, os, ctypes as C
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault('SOLO_HIP_LIB', os.path.join(ROOT, 'gym_solo_amd', 'csrc', 'libsolo_hip_stamps_light.so'))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np, torch
from gym_solo_amd import abi
from bench import build_env
ap = argparse.ArgumentParser()
ap.add_argument('--dtype', default='float32')
ap.add_argument('--geometry', default=None)
ap.add_argument('--rollout', type=int, default=0)
ap.add_argument('spl', nargs='*', type=int)
args = ap.parse_args()
n_env = int(os.environ.get('N', '4096'))
geometries = [tuple(int(x) for x in g.split('x')) for g in args.geometry.split(',')] if args.geometry else [(n_env, 1), (n_env, 2)]
for dtype in args.dtype.split(','):
 tdtype = getattr(torch, dtype)
 for spl in args.spl or (250, 20, 1):
  for n, streams in geometries:
    k = args.rollout if args.rollout > 0 else spl
    env = build_env(n, 0, dtype, steps_per_launch=spl, rollout_streams=streams)
    eng = env.engine
    g = torch.Generator(device='cuda').manual_seed(99)
    acts = (torch.rand(500 + k, n, 12, device='cuda', dtype=tdtype, generator=g) * 2 - 1) * (2 * np.pi)
    eng.rollout(acts[:500], abi.STEP_ALL)                      # into the flailing steady state
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    eng.rollout(acts[500:], abi.STEP_ALL)                      # ONE fused launch per slice (--rollout: see above)
    e1.record(); torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    buf = np.zeros((n, 32), dtype=np.uint64)
    eng.lib.solo_engine_debug_stamps.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    assert eng.lib.solo_engine_debug_stamps(eng._h, buf.ctypes.data, 1 if dtype == 'float32' else 0) == 0
    t0 = buf[:, 0].astype(np.int64); t1 = buf[:, 14].astype(np.int64)
    life = (t1 - t0)
    # (only per-wave DIFFERENCES are used)
    print('%s S=%d K=%d streams=%d N=%d kernel %s: rollout %.3f ms = %.2f us/step ; wave life (ticks): mean %.0f p99 %.0f max %.0f ; max/mean %.3f ; p99/mean %.3f ; per step pct 1/50/90/99/max = %s' % (
      dtype, spl, k, streams, n, eng.kernel_name, ms, ms * 1e3 / k, life.mean(), np.percentile(life, 99), life.max(), life.max() / life.mean(),
      np.percentile(life, 99) / life.mean(), (np.percentile(life, [1, 50, 90, 99, 100]) / spl).astype(int).tolist()), flush=True)
    hw = (buf[:, 15] >> 28).astype(np.int64); xcc = ((buf[:, 15] >> 24) & 0xf).astype(np.int64)
    simd = (hw >> 4) & 3; cu = (hw >> 8) & 0xf; sh = (hw >> 12) & 1; se = (hw >> 13) & 7
    print('    by XCC: ' + ' '.join('%d:%d/%.0f' % (x, (xcc == x).sum(), life[xcc == x].mean() / spl) for x in np.unique(xcc)))
    cuid = ((xcc * 8 + se) * 2 + sh) * 16 + cu
    u, inv = np.unique(cuid, return_inverse=True)
    cnt = np.bincount(inv); cmean = np.bincount(inv, weights=life / spl) / cnt
    print('    CUs used %d ; waves per CU min/max %d/%d ; per-CU mean life: min %.0f p50 %.0f max %.0f ; corr(waves on CU, mean life) %.2f' % (
      len(u), cnt.min(), cnt.max(), cmean.min(), np.median(cmean), cmean.max(), np.corrcoef(cnt, cmean)[0, 1] if cnt.std() > 0 else 0))
    sid = cuid * 4 + simd
    u2, inv2 = np.unique(sid, return_inverse=True)
    cnt2 = np.bincount(inv2)
    print('    SIMDs used %d ; waves per SIMD histogram %s ; mean life by waves-on-SIMD: %s' % (
      len(u2), np.bincount(cnt2).tolist(), {int(c): int((life / spl)[cnt2[inv2] == c].mean()) for c in np.unique(cnt2)}), flush=True)
    # where the spread comes from: the slice a wave ran in (robots [n g / streams, n (g + 1) / streams): solo_launch.h), the robot's own
    # work (slot 13 of the light build: its Gauss-Seidel sweeps over the whole segmented launch) and the wave slot's phase of the
    # priority rotation (HW_ID's wave id = wave_slot_id())
    first = t0.min()
    for gi in range(streams):
      m = slice(n * gi // streams, n * (gi + 1) // streams)
      print('    slice %d: wave life mean %.0f p99 %.0f max %.0f ; max/mean %.3f ; its last wave ended %.3f ms after the first start' % (
        gi, life[m].mean(), np.percentile(life[m], 99), life[m].max(), life[m].max() / life[m].mean(), (t1[m].max() - first) / 1e5))
    sweeps = buf[:, 13].astype(np.int64)
    if 'roll_kernel' in eng.kernel_name and sweeps.any():
      rank = lambda x: np.argsort(np.argsort(x, kind='stable'), kind='stable').astype(np.float64)
      late = life >= np.percentile(life, 75)
      print('    rank correlation (wave life, robot sweeps over the rollout) %.3f ; sweeps per step: mean %.2f, of the slowest quarter %.2f, of the fastest quarter %.2f' % (
        np.corrcoef(rank(life), rank(sweeps))[0, 1], sweeps.mean() / k, sweeps[late].mean() / k, sweeps[life <= np.percentile(life, 25)].mean() / k))
    phase = (hw & 0xf) % 3
    print('    wave life by wave slot % 3: ' + ' '.join('%d:%d/%.0f' % (p, (phase == p).sum(), life[phase == p].mean() / spl) for p in np.unique(phase)), flush=True)
    env._close()
