# -*- coding: utf-8 -*-
"""The kernel launches of the multi-block step, dispatch for dispatch, at the layer shapes of the benchmarked models — the record
that pins the launch forms of csrc/la_mb_forms.h (profiles/mb_launch_forms_trace.txt, tests/golden/mb_launch_forms.json).

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python scripts/mb_launch_trace.py run [--lab] --tuples OUT/tuples.json
        one-layer engines (Llama-2-7B, 13B, Mistral-7B, Mixtral with gathered experts, Qwen2 with bias; the row plan of this device's
        CU count); per engine one eager mstep with 1..8 blocks, one wide-tree pass (128 rows) and one prefill chain (200 tokens).
        Writes the input tuple of every multi-block GEMM the passes make, in launch order (what la_mb_select is asked).
    python scripts/mb_launch_trace.py normalise TRACE.csv
        -> one line per dispatch of this library's kernels: name with template arguments | grid in workgroups | workgroup | LDS bytes
           (LDS_Block_Size as rocprofv3 reports it: the static part, so 0 for the GEMMs, whose LDS is all dynamic)
    python scripts/mb_launch_trace.py fixture --product TUPLES TRACE.csv --lab TUPLES TRACE.csv > tests/golden/mb_launch_forms.json
        pairs tuple i with the i-th multi-block GEMM dispatch of a trace (the PARENT's: the commit before the selector existed); the
        LDS bytes of a case follow from the traced kernel's template arguments (form_lds)
"""
import argparse
import csv
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPI = ('SLAB', 'SWIGLU', 'QKV', 'LOGITS')
FIELDS = ('kind', 'nblk', 'n_wg', 'ksplit', 'K16', 'N', 'R', 'planned', 'gu_interleaved', 'ex_n', 'nblk_dev', 'bias')


def gemm_tuples(eng, nblk):
    """Input tuples (la_mb_forms.h MbFormIn) of the GEMMs of one mstep over nblk blocks of a ONE-layer engine, in launch order:
    what la_engine.cpp's enqueue of the multi-block step hands lk_mb_gemm (resolve_cfg's K splits included)."""
    s = eng.shape
    qkv_n, hidden, ffn, vocab = (s.n_heads + 2 * s.n_kv_heads) * 128, s.hidden, s.ffn, s.vocab
    wg_qkv, wg_gu, wg_lm = eng.balanced_wg
    moe = s.n_experts > 0
    cus = wg_gu if wg_gu > 0 else 256
    k = cus // (hidden // 64)
    auto_ks = 4 if moe else (4 if k >= 4 else k if k >= 1 else 1)

    def fit_ks(ks, k16):
        return next((v for v in (8, 6, 4, 3, 2, 1) if v <= ks and (v == 1 or k16 // v >= 4)), 1)
    o_ks, down_ks = fit_ks(auto_ks, s.n_heads * 128 // 16), fit_ks(auto_ks, ffn // 16)

    def t(kind, n_wg, ksplit, K, N, R, planned, gu=0, ex_n=0, nblk_dev=0, bias=0):
        return dict(zip(FIELDS, (kind, nblk, n_wg, ksplit, K // 16, N, R, planned, gu, ex_n, nblk_dev, bias)))

    def gate_up(**kw):
        return t(1, wg_gu, 1, hidden, ffn, ffn // wg_gu, 1, **kw) if wg_gu else t(1, ffn // 64, 1, hidden, ffn, 64, 0, gu=1, **kw)
    out = []
    q_wg = eng.qkv_mb_wg if (eng.qkv_mb_wg and nblk >= 3) else wg_qkv
    bias = int(bool(getattr(s, 'qkv_bias', False)))
    out.append(t(2, q_wg, 1, hidden, qkv_n, qkv_n // 2 // q_wg, 1, bias=bias) if q_wg else t(2, qkv_n // 64, 1, hidden, qkv_n, 32, 0, bias=bias))
    out.append(t(0, hidden // 64, o_ks, s.n_heads * 128, hidden, 0, 0))
    if moe and nblk >= 2:               # gathered experts, all of a stage in one launch
        out.append(gate_up(ex_n=s.n_experts, nblk_dev=1))
        out.append(t(0, hidden // 64, down_ks // 2 if down_ks >= 2 else 1, ffn, hidden, 0, 0, ex_n=s.n_experts, nblk_dev=1))
    elif moe:
        for _ in range(s.n_experts):
            out.append(gate_up())
            out.append(t(0, hidden // 64, down_ks, ffn, hidden, 0, 0))
    else:
        out.append(gate_up())
        out.append(t(0, hidden // 64, down_ks, ffn, hidden, 0, 0))
    out.append(t(3, wg_lm, 1, hidden, vocab, vocab // wg_lm, 1) if wg_lm else t(3, vocab // 128, 1, hidden, vocab, 128, 0))
    return out


def run(args):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from painlessinferenceacceleration_amd.llama_engine import LlamaShape, LlamaVerifyEngine, random_weights
    from oracle.tiny import random_tree
    tuples = []
    for name in ('llama2_7b', 'llama2_13b', 'mistral_7b', 'mixtral_8x7b', 'qwen2_7b'):
        shape = getattr(LlamaShape, name)()
        shape.n_layers = 1
        sd = random_weights(shape, seed=0, device='cuda:0', decisive=True)
        eng = LlamaVerifyEngine(shape, sd, max_length=512, n_slots=8, max_blocks=8, consume_state_dict=True, lab=args.lab)
        rs = np.random.RandomState(0)
        passes = []

        def trees(n):
            return [(b, rs.randint(3, shape.vocab, size=64).astype(np.int32), random_tree(rs, 64)[1], 0, 1) for b in range(n)]
        for nblk in range(1, 9):
            eng.mstep(trees(nblk), eager=True)
            passes.append(nblk)
        eng.reset()
        ids = rs.randint(3, shape.vocab, size=128).astype(np.int32)
        chain = np.zeros((128, 2), dtype=np.uint64)           # a 128-row chain as a wide tree: row i sees rows 0..i
        for i in range(128):
            chain[i, 0] = (1 << min(i + 1, 64)) - 1
            chain[i, 1] = (1 << (i - 63)) - 1 if i >= 64 else 0
        eng.tstep(ids, chain, eager=True)
        passes.append(2)
        eng.reset()
        eng.mprefill(0, rs.randint(3, shape.vocab, size=200).tolist(), eager=True)
        passes.append(4)
        torch.cuda.synchronize()
        for nblk in passes:
            tuples += [dict(x, model=name) for x in gemm_tuples(eng, nblk)]
        del eng, sd
        torch.cuda.empty_cache()
    with open(args.tuples, 'w') as f:
        json.dump(tuples, f)
    print('passes done, %d GEMM tuples' % len(tuples))


def dispatches(path):
    """[(kernel name, (gx, gy, gz) in workgroups, (wx, wy, wz), LDS bytes)] of this library's kernels (k_*), in dispatch order."""
    with open(path, newline='') as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r['Dispatch_Id']))
    lds_col = 'LDS_Block_Size' if 'LDS_Block_Size' in rows[0] else 'Group_Segment_Size'
    out = []
    for r in rows:
        name = re.sub(r'^void\s+', '', r['Kernel_Name']).replace(' [clone .kd]', '').replace('.kd', '')
        name = re.sub(r'\(.*\)$', '', name)
        if not name.startswith('k_'):
            continue
        wg = tuple(int(r['Workgroup_Size_' + a]) for a in 'XYZ')
        grid = tuple(int(r['Grid_Size_' + a]) // w for a, w in zip('XYZ', wg))
        out.append((name, grid, wg, int(r[lds_col])))
    return out


def form_name(kernel):
    """'k_gemm_wide<4, 2, 0, 0, 2, 4>' -> 'WIDE<4,2,SLAB,0,2,0,0>' (the name strings of kMbForms); None for any other kernel."""
    m = re.match(r'^k_gemm_(mb|wide|fatd|fat)<(.*)>$', kernel)
    if not m:
        return None
    fam = m.group(1).upper()
    a = [{'true': 1, 'false': 0}.get(x.strip(), x.strip()) for x in m.group(2).split(',')]
    a = [int(x) for x in a]
    if fam == 'FATD':
        a = [a[0], a[1], 1, 0, 0, 0, 0]
    n = {'MB': 5, 'WIDE': 5, 'FAT': 7, 'FATD': 7}[fam]
    a = (a[:n] + [0] * 7)[:7]
    return '%s<%d,%d,%s,%d,%d,%d,%d>' % (fam, a[0], a[1], EPI[a[2]], a[3], a[4], a[5], a[6])


def form_lds(form):
    """Dynamic LDS bytes of a form from its template arguments, by the geometry of the kernels (the 64 KiB reduction buffer of k_gemm_mb, WideGeom, FatGeom,
    LA_FATD_LDS of la_mblock.hip): rocprofv3's LDS_Block_Size column holds the static LDS only, 0 for every one of these kernels."""
    fam, rest = form.split('<')
    a = rest.rstrip('>').split(',')
    rbv, tw, rpw = int(a[0]), int(a[1]), int(a[5])
    if fam == 'MB':
        return max(2 * 4 * tw * 1024, 65536)
    if fam == 'WIDE':
        return 4 * (2 * rbv + 2 * (8 // (rbv // 2)) * tw) * 1024
    if fam == 'FAT':
        stage = 2 * rbv + 2 * (4 // (rbv // rpw)) * tw
        return (4 if 4 * stage * 1024 <= 144 * 1024 else 3) * stage * 1024
    return 96 * 1024


def fixture(args):
    out = {}
    for key, (tuples_path, trace) in (('product', args.product), ('lab', args.lab)):
        with open(tuples_path) as f:
            tuples = json.load(f)
        gemms = [d for d in dispatches(trace) if form_name(d[0])]
        assert len(gemms) == len(tuples), (key, len(gemms), len(tuples))
        seen, cases = set(), []
        for t, (name, grid, wg, lds) in zip(tuples, gemms):
            k = tuple(t[f] for f in FIELDS)
            if k in seen:
                continue
            seen.add(k)
            cases.append({'in': {f: t[f] for f in FIELDS}, 'model': t['model'], 'form': form_name(name), 'grid': list(grid), 'lds': form_lds(form_name(name))})
        out[key] = cases
    json.dump(out, sys.stdout, indent=0)
    sys.stdout.write('\n')


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest='cmd', required=True)
    r = sub.add_parser('run')
    r.add_argument('--lab', action='store_true', help='the lab libraries (default knobs) instead of the product libraries')
    r.add_argument('--tuples', required=True)
    n = sub.add_parser('normalise')
    n.add_argument('trace')
    fx = sub.add_parser('fixture')
    fx.add_argument('--product', nargs=2, required=True, metavar=('TUPLES', 'TRACE'))
    fx.add_argument('--lab', nargs=2, required=True, metavar=('TUPLES', 'TRACE'))
    args = ap.parse_args()
    if args.cmd == 'run':
        run(args)
    elif args.cmd == 'normalise':
        for name, grid, wg, lds in dispatches(args.trace):
            print('%s | grid %d,%d,%d | workgroup %d,%d,%d | LDS %d' % ((name,) + grid + wg + (lds,)))
    else:
        fixture(args)


if __name__ == '__main__':
    main()
