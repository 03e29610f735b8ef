"""The eight instantiations of solo_push_kernel<T, kFull, kCtl> (external base wrenches) in the generated gfx950 assembly (hipcc
cross-compiles without a GPU): their names, their budget - the actuator kernels': at most 128 VGPRs and 16 VGPR spills, the LDS of
solo_act_kernel for the same arguments exactly (the wrench has no LDS of its own: it is loaded where it is used), NO scratch access
inside the substep loop, the register-index rule - and the 12 / 4 / 8 / 8 / 8 / 8 counts of the other families.  The helpers are
tests/test_term_kernel_asm.py's: kernel names and the resource metadata, nothing else."""
import os
import sys

from test_term_kernel_asm import ROOT, _kernels, asm, substep_loop  # noqa: F401 - asm is the module-scoped fixture

FAMILY = 'solo_push_kernel'


def test_the_eight_instantiations_and_their_budget(asm):
  k = _kernels(asm, FAMILY)
  assert sorted(k) == sorted('%sLb%dELb%d' % (t, full, ctl) for t in 'fd' for full in (0, 1) for ctl in (0, 1)), sorted(k)
  for args, (body, meta, _) in k.items():
    assert meta is not None, args
    print(args, meta)
    assert meta['vgprs'] <= 128, (args, meta)
    assert meta['spills'] <= 16, (args, meta)
    header, loop, big = substep_loop(body)
    # the loop found IS the substep loop: depth 2, inside the step loop (depth 1), which holds little else
    assert loop['depth'] == 2 and len(big) == 2, (args, big)
    outer = big[loop['parent']]
    assert outer['depth'] == 1 and outer['instructions'] - loop['instructions'] < 1500, (args, big)
    assert loop['scratch'] == 0, (args, loop)
    assert 's_set_gpr_idx_on' in body   # (the Gauss-Seidel loops sit inside it)


def test_no_lds_beyond_the_actuator_kernels(asm):
  """the wrench is read from device memory where the base body's right-hand side is formed: the footprint is the actuator kernels'
  exactly (f64: eight granules, 10240 B)"""
  push, act = _kernels(asm, FAMILY), _kernels(asm, 'solo_act_kernel')
  for args in push:
    assert push[args][1]['lds'] == act[args][1]['lds'], args
    if args[0] == 'd':
      assert push[args][1]['lds'] == 10240, (args, push[args][1])


def test_register_index_rule_in_the_push_kernels(asm, tmp_path):
  sys.path.insert(0, os.path.join(ROOT, 'tools'))
  import check_gpr_idx
  k = _kernels(asm, FAMILY)
  switches = 0
  for args, (body, _, mangled) in k.items():
    f = tmp_path / (args + '.s')
    f.write_text(mangled + 'E:\n' + body)
    n, errors = check_gpr_idx.check(str(f))
    assert not errors, '\n'.join(errors)
    switches += n
  assert switches >= 8 * 8


def test_the_other_families_keep_their_counts(asm):
  assert len(_kernels(asm, 'solo_step_kernel')) == 12
  assert len(_kernels(asm, 'solo_ctl_step_kernel')) == 4
  assert len(_kernels(asm, 'solo_contact_kernel')) == 8
  assert len(_kernels(asm, 'solo_decim_kernel')) == 8
  assert len(_kernels(asm, 'solo_term_kernel')) == 8
  assert len(_kernels(asm, 'solo_act_kernel')) == 8
