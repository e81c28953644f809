#!/usr/bin/env python3
# -*- coding: utf-8 -*-
"""Prologue census of the step kernels: what stands between kernel entry and the first weight (or K) loads.

Builds la_kernels.hip and la_attn1.hip of a source tree to gfx950 assembly with the flags of csrc/build.sh plus
`--cuda-device-only -S` (no GPU involved), for the bf16 and the fp16 product library, and for every kernel of the
single-sequence step walks the code from the entry to the first wide vector load (dwordx2 / dwordx4: a weight, x or K
fragment).  Where the code branches, the cheapest way through is taken — that is the dense launch: no expert routing,
no lab knob, a K-range magic the launcher could compute.  Per kernel it prints

    scalar loads issued, scalar waits (an s_waitcnt on lgkmcnt with a scalar load outstanding), division expansions
    (v_rcp_iflag_f32 / v_rcp_f32 of the integer-division sequences), and the kernel-argument offsets the loads read.

The first instructions of a kernel built with kernel-argument preload are a compatibility header (loads of the preloaded
arguments for firmware that does not preload, then a branch to the 256-byte aligned real entry); hardware that preloads
skips it, and so does the census.  A report, not a test:

    python scripts/prologue_census.py [--src painlessinferenceacceleration_amd/csrc] [--label branch] > census.txt
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wall', '-Wno-unused-function', '-mllvm',
         '-amdgpu-kernarg-preload-count=16', '--cuda-device-only', '-S', '-x', 'hip']
# (launch, file, mangled-name prefix): the template arguments behind the prefix may grow, the leading ones name the kernel
KERNELS = [
    ('QKV        k_gemm64r<2,3,8,8,0>', 'la_kernels', r'_Z9k_gemm64rILi2ELi3ELi8ELi8ELi0E'),
    ('gate/up    k_gemm64r<4,1,4,8,0>', 'la_kernels', r'_Z9k_gemm64rILi4ELi1ELi4ELi8ELi0E(Lb0E)?E'),
    ('lm_head    k_gemm64r<4,2,4,8,0>', 'la_kernels', r'_Z9k_gemm64rILi4ELi2ELi4ELi8ELi0E'),
    ('o_proj     k_gemm64<2,0,8,8>', 'la_kernels', r'_Z8k_gemm64ILi2ELi0ELi8ELi8E(Lb0E)?E'),
    ('down       k_gemm64<2,0,8,4>', 'la_kernels', r'_Z8k_gemm64ILi2ELi0ELi8ELi4E(Lb0E)?E'),
    ('attention  k_tree_attn1<false,4,0>', 'la_attn1', r'_Z12k_tree_attn1ILb0ELi4ELi0EE'),
    ('attention  k_tree_attn1<false,1,0>', 'la_attn1', r'_Z12k_tree_attn1ILb0ELi1ELi0EE'),
    ('row norm   k_row_norm<4,false>', 'la_kernels', r'_Z10k_row_normILi4ELb0EE'),
]
WIDE = re.compile(r'^(global|buffer|flat)_load_dwordx[24]\b')
SLOAD = re.compile(r'^s_(buffer_)?load_dword')
DIV = re.compile(r'^v_rcp_(iflag_)?f32')


def functions(path):
    """{symbol: [(label or None, mnemonic, operands)]} of an assembly file"""
    out, cur = {}, None
    for line in open(path):
        line = line.split(';')[0].rstrip()
        if not line:
            continue
        m = re.match(r'^(_Z\w+):', line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        if line.startswith('.Lfunc_end'):
            cur = None
            continue
        m = re.match(r'^(\.LBB\w+):', line)
        if m:
            cur.append((m.group(1), None, None))
            continue
        s = line.strip()
        if s.startswith('.'):
            continue
        parts = s.split(None, 1)
        cur.append((None, parts[0], parts[1] if len(parts) > 1 else ''))
    return out


def census(ins):
    labels = {lab: i for i, (lab, _, _) in enumerate(ins) if lab}
    start = 0
    for i, (_, op, arg) in enumerate(ins[:12]):        # the preload compatibility header
        if op == 's_branch':
            start = labels[arg.strip()]
            break
        if op is not None and not (SLOAD.match(op) or op == 's_waitcnt'):
            break
    sys.setrecursionlimit(100000)
    memo = {}

    def walk(i, pending, seen):
        """cheapest (waits + divisions, loads, waits, divisions, offsets) from instruction i to the first wide vector load"""
        key = (i, pending)
        if key in memo:
            return memo[key]
        loads = waits = divs = 0
        offs = []
        best = None
        while i < len(ins):
            lab, op, arg = ins[i]
            i += 1
            if op is None:
                continue
            if WIDE.match(op):
                best = (0, 0, 0, 0, [])
                break
            if op == 's_endpgm':
                break
            if SLOAD.match(op):
                loads += 1
                pending = True
                offs.append(arg.split(',')[-1].strip())
            elif op == 's_waitcnt' and 'lgkmcnt' in arg and pending:
                waits += 1
                pending = False
            elif DIV.match(op):
                divs += 1
            elif op == 's_branch' or op.startswith('s_cbranch'):
                tgt = labels[arg.strip()]
                ways = []
                if op != 's_cbranch_execz' and tgt not in seen:           # exec is never empty here
                    ways.append(walk(tgt, pending, seen | {tgt}))
                if op not in ('s_branch', 's_cbranch_execnz'):
                    ways.append(walk(i, pending, seen))
                ways = [w for w in ways if w is not None]
                best = min(ways, key=lambda w: (w[0], w[1])) if ways else None
                break
        if best is not None:
            best = (best[0] + waits + divs, best[1] + loads, best[2] + waits, best[3] + divs, offs + best[4])
        memo[key] = best
        return best

    return walk(start, False, frozenset())


def main():
    ap = argparse.ArgumentParser()
    here = os.path.dirname(os.path.abspath(__file__))
    ap.add_argument('--src', default=os.path.join(here, '..', 'painlessinferenceacceleration_amd', 'csrc'))
    ap.add_argument('--label', default='branch')
    a = ap.parse_args()
    for lib, extra in (('bf16 product library', []), ('fp16 product library', ['-DLA_DTYPE=1'])):
        with tempfile.TemporaryDirectory() as tmp:
            procs = []
            for f in ('la_kernels', 'la_attn1'):
                procs.append(subprocess.Popen([HIPCC] + FLAGS + extra + [os.path.join(a.src, f + '.hip'), '-o', os.path.join(tmp, f + '.s')],
                                              stderr=subprocess.DEVNULL))
            for p in procs:
                if p.wait() != 0:
                    sys.exit('hipcc failed')
            fns = {f: functions(os.path.join(tmp, f + '.s')) for f in ('la_kernels', 'la_attn1')}
        print(f'== {a.label}: {lib}')
        print(f'{"launch / kernel":<38} {"s_loads":>7} {"s_waits":>7} {"divisions":>9}  kernel-argument offsets loaded')
        for name, f, pat in KERNELS:
            syms = [s for s in fns[f] if re.match(pat, s)]
            if len(syms) != 1:
                print(f'{name:<38} (symbol not found: {len(syms)} matches)')
                continue
            r = census(fns[f][syms[0]])
            if r is None:
                print(f'{name:<38} (no wide vector load reached)')
                continue
            print(f'{name:<38} {r[1]:>7} {r[2]:>7} {r[3]:>9}  {" ".join(r[4]) or "-"}')
        print()


if __name__ == '__main__':
    main()
