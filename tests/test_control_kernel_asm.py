"""The joint-control kernels (solo_ctl_step_kernel<T, kFull>: torque / PD modes) meet the product's budget in the
generated gfx950 assembly (hipcc cross-compiles without a GPU): 128 VGPRs or fewer (four waves per SIMD: 4096 f64 robots
resident), at most 16 spills, no scratch access inside the step loop, the register-index rule of the whole file - and
the twelve solo_step_kernel instantiations are still there, under their own names."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASM = os.path.join(ROOT, 'gym_solo_amd', 'csrc', 'solo_engine.gfx950.s')
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def _asm():
  subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'gym_solo_amd', 'csrc'), 'asm'], stderr=subprocess.DEVNULL)
  return open(ASM).read()


def _step_loop_scratch(body):
  """(scratch accesses inside the step loop, instructions of the step loop, all scratch accesses) of one kernel body: the
  step loop is the depth-1 loop (the compiler's loop annotations) that contains the Gauss-Seidel loop, i.e. the first
  s_set_gpr_idx_on - as tools/step_body_scratch.py finds it for solo_step_kernel."""
  blocks, cur = [], {'label': None, 'loops': {}, 'lines': []}
  for line in body.split('\n'):
    lab = re.match(r'^(\.LBB\d+_\d+):(.*)$', line)
    if lab:
      blocks.append(cur)
      cur = {'label': lab.group(1)[2:], 'loops': {}, 'lines': []}
      line = lab.group(2)
    ann = re.search(r';\s+(?:in Loop: Header=|Parent Loop )(BB\d+_\d+) Depth=(\d+)', line)
    if ann and not cur['lines']:
      cur['loops'][ann.group(1)] = int(ann.group(2))
    hdr = re.search(r';\s*=>\s*This (?:Inner )?Loop Header: Depth=(\d+)', line)
    if hdr and not cur['lines']:
      cur['loops'][cur['label']] = int(hdr.group(1))
    if re.match(r'^\s+[a-z]\w+', line) and not line.strip().startswith('.'):
      cur['lines'].append(line.strip())
  blocks.append(cur)
  solver = next(b for b in blocks if any(l.startswith('s_set_gpr_idx_on') for l in b['lines']))
  loop = [h for h, d in solver['loops'].items() if d == 1]
  assert len(loop) == 1, solver['loops']
  inside = [b for b in blocks if loop[0] in b['loops']]
  scratch = lambda l: l.startswith('scratch_')
  return (sum(scratch(l) for b in inside for l in b['lines']), sum(len(b['lines']) for b in inside),
          sum(scratch(l) for b in blocks for l in b['lines']))


def test_control_kernels_resource_budget():
  text = _asm()
  found = {}
  for m in re.finditer(r'- \.agpr_count:.*?\.name:\s+(\S+)\n.*?\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)', text, re.S):
    k = re.search(r'solo_ctl_step_kernelI(\w)Lb(\d)EE', m.group(1))
    if k:
      found[(k.group(1), int(k.group(2)))] = (int(m.group(2)), int(m.group(3)))
  assert sorted(found) == [('d', 0), ('d', 1), ('f', 0), ('f', 1)], sorted(found)
  bodies = {}
  for m in re.finditer(r'^(_ZN4solo20solo_ctl_step_kernelI(\w)Lb(\d)EE\w*):.*?\n(.*?)^\.Lfunc_end', text, re.S | re.M):
    bodies[(m.group(2), int(m.group(3)))] = m.group(4)
  assert sorted(bodies) == sorted(found)
  for key, (vgprs, spills) in found.items():
    assert vgprs <= 128, (key, vgprs)
    assert spills <= 16, (key, spills)
    in_loop, loop_len, total = _step_loop_scratch(bodies[key])
    assert in_loop == 0, (key, in_loop, total)
    assert loop_len > 2000, (key, loop_len)   # (the loop found IS the step loop)


def test_register_index_rule_and_the_position_kernels_are_still_twelve():
  import check_gpr_idx
  text = _asm()
  n, errors = check_gpr_idx.check(ASM)
  assert not errors, '\n'.join(errors)
  names = set(re.findall(r'^(_ZN4solo16solo_step_kernelI\w+):', text, re.M))
  assert len(names) == 12, sorted(names)
  assert all(re.search(r'I[fd]Lb\dELb\dELb\dEE', s) for s in names), sorted(names)
  assert len(set(re.findall(r'^(_ZN4solo20solo_ctl_step_kernelI\w+):', text, re.M))) == 4
