"""The eight instantiations of solo_decim_kernel<T, kFull, kCtl> in the generated gfx950 assembly (hipcc cross-compiles without
a GPU): their names, their budget - 128 VGPRs, at most 16 VGPR spills, 10240 B (f64) / 6240 B (f32) of LDS, NO scratch access
inside the substep loop, the register-index rule - and the 12 / 4 / 8 counts of the other families.

The substep loop is found through the compiler's loop annotations, as tools/step_body_scratch.py finds the step loop - that
helper looks at one fixed depth and attributes a block only to the loop whose header its annotation names, so the finder of a
NESTED loop lives here: the loop tree is built from the headers' "Parent Loop" lines, a loop's instructions include those of
the loops inside it, and the substep loop is the innermost loop of more than 2000 instructions."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'gym_solo_amd', 'csrc')


@pytest.fixture(scope='module')
def asm():
  subprocess.check_call(['make', '-s', '-C', CSRC, 'asm'], stderr=subprocess.DEVNULL)
  return open(os.path.join(CSRC, 'solo_engine.gfx950.s')).read()


def loops_of(body):
  """{header: dict(depth, parent, instructions, scratch)} of one function body, inner loops included in their parents"""
  blocks, cur = [], {'label': None, 'own': None, 'lines': [], 'parents': {}}
  for line in body.split('\n'):
    lab = re.match(r'^(?:\.L(BB\d+_\d+)|; %bb\.\d+):(.*)$', line)   # (a labelled block, or one that is only fallen into)
    if lab:
      blocks.append(cur)
      cur = {'label': lab.group(1), 'own': None, 'lines': [], 'parents': {}}
      line = lab.group(2)
    if not cur['lines']:
      m = re.search(r';\s+in Loop: Header=(BB\d+_\d+) Depth=(\d+)', line)
      if m:
        cur['own'] = (m.group(1), int(m.group(2)))
      m = re.search(r';\s+Parent Loop (BB\d+_\d+) Depth=(\d+)', line)
      if m:
        cur['parents'][int(m.group(2))] = m.group(1)
      m = re.search(r';\s*=>\s*This (?:Inner )?Loop Header: Depth=(\d+)', line)
      if m:
        cur['own'] = (cur['label'], int(m.group(1)))
    if re.match(r'^\s+[a-z]\w+', line) and not line.strip().startswith('.'):
      cur['lines'].append(line.strip())
  blocks.append(cur)
  loops = {}
  for b in blocks:   # the tree: a header names all its ancestors
    if b['own'] and b['own'][0] == b['label']:
      h, d = b['own']
      loops[h] = dict(depth=d, parent=b['parents'].get(d - 1), instructions=0, scratch=0)
  for b in blocks:
    h = b['own'][0] if b['own'] else None
    while h is not None:
      loops[h]['instructions'] += len(b['lines'])
      loops[h]['scratch'] += sum(l.startswith('scratch_') for l in b['lines'])
      h = loops[h]['parent']
  return loops


def substep_loop(body):
  big = {h: l for h, l in loops_of(body).items() if l['instructions'] > 2000}
  h = max(big, key=lambda x: big[x]['depth'])
  return h, big[h], big


def _kernels(asm, name):
  """{template arguments: (body, metadata dict)} of a kernel family"""
  out = {}
  for m in re.finditer(r'^(_ZN4solo\d+%sI(\w+?)E)E\w*:.*?\n(.*?)^\.Lfunc_end' % name, asm, re.S | re.M):
    out[m.group(2)] = [m.group(3), None, m.group(1)]
  for m in re.finditer(r'- \.agpr_count:.*?\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+)\n.*?\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)', asm, re.S):
    for args, entry in out.items():
      if m.group(2).startswith(entry[2]):
        entry[1] = dict(lds=int(m.group(1)), vgprs=int(m.group(3)), spills=int(m.group(4)))
  return out


def test_the_eight_instantiations_and_their_budget(asm):
  k = _kernels(asm, 'solo_decim_kernel')
  assert sorted(k) == sorted('%sLb%dELb%d' % (t, full, ctl) for t in 'fd' for full in (0, 1) for ctl in (0, 1)), sorted(k)
  for args, (body, meta, _) in k.items():
    assert meta is not None, args
    assert meta['vgprs'] <= 128, (args, meta)
    assert meta['spills'] <= 16, (args, meta)
    assert meta['lds'] <= (10240 if args[0] == 'd' else 6240), (args, meta)
    header, loop, big = substep_loop(body)
    # the loop found IS the substep loop: depth 2, inside the step loop (depth 1), which holds little else
    assert loop['depth'] == 2 and len(big) == 2, (args, big)
    outer = big[loop['parent']]
    assert outer['depth'] == 1 and outer['instructions'] - loop['instructions'] < 1500, (args, big)
    assert loop['scratch'] == 0, (args, loop)
    assert 's_set_gpr_idx_on' in body   # (the Gauss-Seidel loops sit inside it)


def test_the_finder_sees_a_nested_loop():
  body = '\n'.join(['.LBB0_1:   ; =>This Loop Header: Depth=1', '\ts_nop 0', '\tscratch_load_dword v0, off, off',
                    '.LBB0_2:   ;   Parent Loop BB0_1 Depth=1', '     ; =>  This Inner Loop Header: Depth=2'] + ['\tv_mov_b32 v1, v2'] * 2001 +
                   ['; %bb.3:   ;   in Loop: Header=BB0_2 Depth=2', '\tscratch_store_dword off, v1, off', '\ts_cbranch_scc1 .LBB0_2',
                    '; %bb.4:   ;   in Loop: Header=BB0_1 Depth=1', '\ts_cbranch_scc1 .LBB0_1', ''])
  header, loop, big = substep_loop(body)
  assert header == 'BB0_2' and loop['depth'] == 2 and loop['scratch'] == 1 and loop['instructions'] == 2003
  assert big['BB0_1']['instructions'] == 2006 and big['BB0_1']['scratch'] == 2


def test_register_index_rule_in_the_decimation_kernels(asm, tmp_path):
  sys.path.insert(0, os.path.join(ROOT, 'tools'))
  import check_gpr_idx
  k = _kernels(asm, 'solo_decim_kernel')
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
