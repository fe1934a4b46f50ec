#!/usr/bin/env python
"""Two device-assembly files of one unit (hipcc build.FLAGS --cuda-device-only -S), kernel by kernel: the instruction stream (comments,
directives, the __hip_cuid symbol and the function number in block labels removed) and the resources of the kernel descriptors.

    python tools/exp/same_code.py parent.s branch.s > record.json

Per kernel `code` is one of
  equal                                 the same lines
  operand order or register names only  the same opcodes in the same order; lines that differ hold the same operands once register
                                        numbers are dropped and the operands sorted
  reordered, same opcode histogram      the same count of every opcode (s_nop and s_waitcnt counted apart: their number follows the order)
  different                             anything else, with the opcodes whose counts moved
"""
import collections
import json
import re
import sys

FIELDS = ('vgpr_count', 'sgpr_count', 'group_segment_fixed_size', 'private_segment_fixed_size')
PADDING = ('s_nop', 's_waitcnt')


def kernels(path):
    """{mangled name: {'lines': [...], 'occupancy': n, FIELDS...}}"""
    out, name, meta = {}, None, {}
    for raw in open(path):
        m = re.match(r'(_Z\w+):', raw)
        if m and name is None:
            name = m.group(1)
            out[name] = {'lines': []}
            continue
        if name is not None:
            if re.match(r'\.Lfunc_end\d+:', raw):
                name, last = None, name
                continue
            line = re.sub(r'\.LBB\d+_', '.LBB_', raw.split(';')[0]).strip()
            if line and (not line.startswith('.') or line.endswith(':')):
                out[name]['lines'].append(re.sub(r'\s+', ' ', line))
            continue
        m = re.match(r'; Occupancy: (\d+)', raw)
        if m:
            out[last]['occupancy'] = int(m.group(1))
        m = re.match(r'\s+\.(\w+):\s+(\S+)', raw)          # the metadata note: fields in alphabetical order, .name among them
        if m:
            if m.group(1) == 'name':
                meta['name'] = m.group(2)
            elif m.group(1) in FIELDS:
                meta[m.group(1)] = int(m.group(2))
            if m.group(1) == 'vgpr_count':
                out[meta.pop('name')].update(meta)
                meta = {}
    return out


def opcode(line):
    return line.split(' ', 1)[0]


def operands(line):
    rest = line.split(' ', 1)[1] if ' ' in line else ''
    rest = re.sub(r'\b([vsa])\[(\d+):(\d+)\]', lambda m: f'{m.group(1)}x{int(m.group(3)) - int(m.group(2)) + 1}', rest)
    rest = re.sub(r'\b([vsa])\d+\b', r'\1', rest)
    return sorted(t.strip() for t in rest.split(','))


def histogram(lines):
    return collections.Counter(opcode(ln) for ln in lines if not ln.endswith(':'))


def compare(a, b):
    res = {'instructions': [sum(histogram(a['lines']).values()), sum(histogram(b['lines']).values())]}
    for f in FIELDS + ('occupancy',):
        res[f] = a[f] if a[f] == b[f] else [a[f], b[f]]
    res['resources_equal_to_parent'] = all(a[f] == b[f] for f in FIELDS + ('occupancy',))
    la, lb = a['lines'], b['lines']
    if la == lb:
        res['code'] = 'equal'
        res['instructions'] = res['instructions'][0]
        return res
    ha, hb = histogram(la), histogram(lb)
    if [opcode(x) for x in la] == [opcode(x) for x in lb] and all(operands(x) == operands(y) for x, y in zip(la, lb)):
        res['code'] = 'operand order or register names only'
        res['lines_that_differ'] = sum(x != y for x, y in zip(la, lb))
        return res
    for h in (ha, hb):
        res.setdefault('padding', []).append({p: h.pop(p, 0) for p in PADDING})
    if ha == hb:
        res['code'] = 'reordered, same opcode histogram'
    else:
        res['code'] = 'different'
        res['opcode_counts_that_moved'] = {k: [ha.get(k, 0), hb.get(k, 0)] for k in sorted(set(ha) | set(hb)) if ha.get(k, 0) != hb.get(k, 0)}
    return res


if __name__ == '__main__':
    parent, branch = kernels(sys.argv[1]), kernels(sys.argv[2])
    per_kernel = {k: compare(parent[k], branch[k]) for k in parent if k in branch}
    print(json.dumps({'kernels': len(per_kernel), 'only_in_parent': sorted(set(parent) - set(branch)), 'only_in_branch': sorted(set(branch) - set(parent)),
                      'by_result': dict(collections.Counter(v['code'] for v in per_kernel.values())),
                      'resources_equal_in_every_kernel': all(v['resources_equal_to_parent'] for v in per_kernel.values()),
                      'per_kernel': per_kernel}, indent=1))
