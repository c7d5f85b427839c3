"""Issue budget of the headline K-step kernel from its gfx950 ISA.

    python scripts/issue_budget.py [--kernel NAME_SUBSTRING] [--json OUT]

Compiles csrc/optimize_lr_persist.hip to assembly (the product flags of
custom_envs_amd/build.py), cuts out the benchmark instance
(optimize_lr_persist_ws_kernel<3,4,false>), finds the row waves' and the
epilogue waves' step loops (the two loops that hold an s_barrier), and counts
per step, by issue class: f64 MFMA, f64 VALU, 32-bit VALU, transcendental
VALU (v_rcp_*, v_log_*, ...: priced apart), LDS, VMEM, SALU, s_waitcnt and
s_nop.  The row loop has three bodies behind the |u| bound's tiers (lr_tier:
batched reciprocals, clamp-free, clamped); the one that runs on the
benchmark data (the fewest reciprocals, then the fewest f64 VALU) is counted
with the blocks around the bodies, and priced beside round 6's counts.

The per-class costs ("Issue budget") turn the counts into
time: they are measured, not assumed (profiles/r06_mfma_overlap.jsonl and
profiles/archive/r01_f64_costs.jsonl).
"""
import argparse
import collections
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'custom_envs_amd', 'csrc', 'optimize_lr_persist.hip')


def compile_asm(defines=()):
    out = os.path.join(tempfile.mkdtemp(), 'lp.s')
    cmd = ['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-x', 'hip', '-O3', '-std=c++17',
           '-I', os.path.join(ROOT, 'include'), '-mllvm', '-amdgpu-mfma-vgpr-form=1',
           '--offload-device-only', '-S', SRC, '-o', out] + ['-D' + d for d in defines]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    return open(out).read().split('\n')


def kernel_body(lines, name):
    starts = [i for i, l in enumerate(lines) if l.startswith('_Z') and l.split()[0].endswith(':')
              and name in l]
    if not starts:
        raise SystemExit('kernel %s not found' % name)
    s = starts[0]
    e = next(i for i in range(s, len(lines)) if lines[i].strip().startswith('s_endpgm'))
    return lines[s:e + 1]


def classify(op):
    if op.startswith('v_mfma'):
        return 'mfma'
    if op.startswith('ds_'):
        return 'lds'
    if op.startswith(('global_', 'buffer_', 'flat_', 'scratch_')):
        return 'vmem'
    if op.startswith('s_waitcnt'):
        return 'waitcnt'
    if op.startswith('s_nop'):
        return 'nop'
    if op.startswith('s_'):
        return 'salu'
    if op.startswith(TRANS):
        return 'trans'
    if op.startswith('v_'):
        return 'valu64' if 'f64' in op else 'valu32'
    return 'other'


# Transcendental VALU operations: quarter-rate or slower, counted apart from
# the ordinary f64 / 32-bit classes.  v_rcp_f64 measured 16.76 cycles per
# instruction with one wave per SIMD (profiles/archive/r01_f64_costs.jsonl).
TRANS = ('v_rcp_', 'v_rsq_', 'v_sqrt_', 'v_log_', 'v_exp_', 'v_sin_', 'v_cos_')

# ns per instruction ("Issue budget"): the 16x16x4 f64 MFMA
# 27.6, the 4x4x4 one 0.26 of it, f64 VALU 2.35, 32-bit VALU 2.0,
# transcendental 16.8 cycles at 2.16 GHz
COST_NS = {'mfma16': 27.6, 'mfma4': 27.6 * 0.26, 'valu64': 2.35, 'valu32': 2.0, 'trans': 16.8 / 2.16}
# round 6's tree (CE_LR_TLOG=0, CE_LR_RCPB=0) by the same classes: its 325
# f64 VALU held 16 v_rcp_f64, its 138 32-bit VALU one v_log_f32
ROUND6 = {'mfma16': 12, 'mfma4': 48, 'valu64': 309, 'valu32': 137, 'trans': 17}
# round 9's tree (the table log, one reciprocal per four values), before the
# miss shift register and the high-word tie prefilter
# (profiles/r09_issue_budget.json)
ROUND9 = {'mfma16': 12, 'mfma4': 48, 'valu64': 312, 'valu32': 123, 'trans': 5}


def budget(counts, ops):
    """The counted classes priced: (class -> count, class -> us, total us)."""
    n4 = sum(n for op, n in ops.items() if op.startswith('v_mfma_f64_4x4x4'))
    n = {'mfma16': counts.get('mfma', 0) - n4, 'mfma4': n4, 'valu64': counts.get('valu64', 0),
         'valu32': counts.get('valu32', 0), 'trans': counts.get('trans', 0)}
    us = {k: n[k] * COST_NS[k] * 1e-3 for k in n}
    return n, us, sum(us.values())


def count(body, a, b):
    c, ops = collections.Counter(), collections.Counter()
    for line in body[a:b]:
        t = line.strip()
        if not t or t.startswith(('.', ';')) or t.endswith(':'):
            continue
        op = t.split()[0]
        c[classify(op)] += 1
        ops[op] += 1
    return dict(c), dict(ops.most_common())


def loops(body):
    """(header index, back-branch index) of every loop: a label whose name a
    later branch targets."""
    labels = {l.split()[0][:-1]: i for i, l in enumerate(body) if re.match(r'^\.LBB\w+:', l.strip())}
    out = []
    for i, l in enumerate(body):
        m = re.match(r'\s*s_(?:cbranch_\w+|branch)\s+(\.LBB\w+)', l)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            out.append((labels[m.group(1)], i))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kernel', default='optimize_lr_persist_ws_kernelILi3ELi4ELb0E')
    ap.add_argument('--define', action='append', default=[])
    ap.add_argument('--json')
    args = ap.parse_args()
    body = kernel_body(compile_asm(args.define), args.kernel)
    # the step loops: outermost loops containing an s_barrier
    cand = []
    for h, b in loops(body):
        if any('s_barrier' in body[i] for i in range(h, b + 1)):
            cand.append((h, b))
    outer = [x for x in cand if not any(y != x and y[0] <= x[0] and x[1] <= y[1] for y in cand)]
    outer.sort()
    res = {'kernel': args.kernel, 'loops': []}
    for h, b in outer:
        whole, ops = count(body, h, b + 1)
        res['loops'].append({'lines': [h, b], 'per_step': whole, 'ops': ops})
    # the row loop: the one with MFMAs; split its two row bodies (the blocks
    # with 28 MFMAs each) from the rest
    for lp in res['loops']:
        lp['role'] = 'row' if lp['per_step'].get('mfma', 0) else 'epilogue'
    row = next((lp for lp in res['loops'] if lp['role'] == 'row'), None)
    if row:
        h, b = row['lines']
        blocks, cur = [], None
        for i in range(h, b + 1):
            if re.match(r'^\.LBB\w+:', body[i].strip()):
                if cur:
                    blocks.append(cur)
                cur = [i, i]
            elif cur:
                cur[1] = i
        if cur:
            blocks.append(cur)
        info = [(blk, count(body, blk[0], blk[1] + 1)[0]) for blk in blocks]
        mf = [(blk, c) for blk, c in info if c.get('mfma', 0) >= 20]
        # the body that runs on the benchmark data: the heavy block with the
        # fewest reciprocals (batched, CE_LR_RCPB), then the fewest f64 VALU
        # (no clamp)
        mf.sort(key=lambda x: (x[1].get('trans', 0), x[1].get('valu64', 0)))
        if mf:
            bounded = mf[0]
            # the hot path: the blocks ahead of the first row body and the
            # blocks after the last block with an MFMA (the tie re-walk,
            # never taken on the benchmark data, sits between)
            first = min(i for i, (blk, c) in enumerate(info) if c.get('mfma', 0) >= 20)
            last = max(i for i, (blk, c) in enumerate(info) if c.get('mfma', 0) > 0)
            rest = collections.Counter()
            for blk, c in info[:first] + info[last + 1:]:
                rest.update(c)
            total = collections.Counter(bounded[1])
            total.update(rest)
            hot_ops = collections.Counter()
            for blk, c in [bounded] + info[:first] + info[last + 1:]:
                hot_ops.update(count(body, blk[0], blk[1] + 1)[1])
            row['bounded_body'] = bounded[1]
            row['outside_bodies'] = dict(rest)
            row['per_step_bounded'] = dict(total)
            n, us, tot = budget(total, hot_ops)
            row['budget'] = {'counts': n, 'us': us, 'total_us': tot}
    txt = json.dumps(res, indent=1)
    if args.json:
        with open(args.json, 'w') as fh:
            fh.write(txt)
    for lp in res['loops']:
        print(lp['role'], 'per step:', lp.get('per_step_bounded', lp['per_step']))
        if 'bounded_body' in lp:
            print('   bounded row body:', lp['bounded_body'])
            print('   around it       :', lp['outside_bodies'])
        if 'budget' in lp:
            keys = ('mfma16', 'mfma4', 'valu64', 'valu32', 'trans')
            r6 = {k: ROUND6[k] * COST_NS[k] * 1e-3 for k in keys}
            r9 = {k: ROUND9[k] * COST_NS[k] * 1e-3 for k in keys}
            print('   budget, us      : ' + ' '.join('%8s' % k for k in keys) + '    total')
            for name, n, us in (('round 6', ROUND6, r6), ('round 9', ROUND9, r9),
                                ('this tree', lp['budget']['counts'], lp['budget']['us'])):
                print('   %-10s count: ' % name + ' '.join('%8d' % n[k] for k in keys))
                print('   %-10s    us: ' % name + ' '.join('%8.3f' % us[k] for k in keys)
                      + ' %8.3f' % sum(us[k] for k in keys))
    return 0


if __name__ == '__main__':
    sys.exit(main())
