"""The contact-sensing kernels (solo_contact_kernel<T, kFull, kCtl>) meet the product's budget in the generated gfx950
assembly (hipcc cross-compiles without a GPU): all eight instantiations are there under their own name, at 128 VGPRs or
fewer with at most 16 spills, no scratch access inside the step loop, at most 10240 B of LDS (one 1280-B granule more
costs the f64 kernel its fourth wave per SIMD), and the register-index rule of the whole file holds.  The position and
control kernels are still twelve and four."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_control_kernel_asm import ASM, _asm, _step_loop_scratch  # noqa: E402


def test_contact_kernels_resource_budget():
  text = _asm()
  found = {}
  for m in re.finditer(r'- \.agpr_count:.*?\.group_segment_fixed_size:\s+(\d+)\n.*?\.name:\s+(\S+)\n.*?\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)', text, re.S):
    k = re.search(r'solo_contact_kernelI(\w)Lb(\d)ELb(\d)EE', m.group(2))
    if k:
      found[(k.group(1), int(k.group(2)), int(k.group(3)))] = (int(m.group(3)), int(m.group(4)), int(m.group(1)))
  want = sorted((t, f, c) for t in 'df' for f in (0, 1) for c in (0, 1))
  assert sorted(found) == want, sorted(found)
  bodies = {}
  for m in re.finditer(r'^(_ZN4solo19solo_contact_kernelI(\w)Lb(\d)ELb(\d)EE\w*):.*?\n(.*?)^\.Lfunc_end', text, re.S | re.M):
    bodies[(m.group(2), int(m.group(3)), int(m.group(4)))] = m.group(5)
  assert sorted(bodies) == want
  for key, (vgprs, spills, lds) in found.items():
    assert vgprs <= 128, (key, vgprs)
    assert spills <= 16, (key, spills)
    assert lds <= 10240, (key, lds)
    in_loop, loop_len, total = _step_loop_scratch(bodies[key])
    assert in_loop == 0, (key, in_loop, total)
    assert loop_len > 2000, (key, loop_len)   # (the loop found IS the step loop)


def test_register_index_rule_and_the_other_kernels_keep_their_names():
  import check_gpr_idx
  text = _asm()
  n, errors = check_gpr_idx.check(ASM)
  assert not errors, '\n'.join(errors)
  assert len(set(re.findall(r'^(_ZN4solo16solo_step_kernelI\w+):', text, re.M))) == 12
  assert len(set(re.findall(r'^(_ZN4solo20solo_ctl_step_kernelI\w+):', text, re.M))) == 4
  assert len(set(re.findall(r'^(_ZN4solo19solo_contact_kernelI\w+):', text, re.M))) == 8
