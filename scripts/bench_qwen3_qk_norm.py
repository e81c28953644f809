# -*- coding: utf-8 -*-
"""Cost of the Qwen3 per-head q / k RMSNorm + RoPE stage (la_qk_norm_rope, csrc/la_qknorm.hip: one small launch per layer behind the QKV
launch) on the verify step: a Qwen3-8B-shaped random-init model (36 layers, hidden 4096, 32 / 8 heads, head_dim 128, ffn 12288, vocab
151936) timed with the stage (shape.qk_norm) and with the same weights and the stage off (the QKV launches then apply RoPE themselves),
at bs=1 (the 64-row step, verify only) and bs=8 (la_llama_mstep, 8 x 64 rows, forward only).  Variants are built one at a time and
alternated (norm, plain, norm, plain, ...) so that drift of the box shows up as spread; each adds the la_llama_profile class times of
one 64-row step (the stage is counted under `other`).

    timeout -k 10 900 python scripts/bench_qwen3_qk_norm.py --iters 30 --rounds 3 --out profiles/qwen3_qk_norm.json && \\
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d results/qk_norm_trace -o qk -- \\
        python scripts/bench_qwen3_qk_norm.py --kernel-run && \\
    python scripts/bench_qwen3_qk_norm.py --merge-kernel-stats results/qk_norm_trace --out profiles/qwen3_qk_norm.json

The rocprofv3 command is a run of its own (kernel trace only, no counters): one engine with the stage, 20 64-row steps and
20 8-block steps; the last command (no GPU) reads the per-dispatch durations of k_qk_norm_rope, and of the other small per-layer
launches of the same trace for comparison, from the result database and merges them into the JSON.
"""
import argparse
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CLASSES = ('qkv', 'o', 'gateup', 'down', 'lm_head', 'attn', 'other')
COMPARE = ('k_qk_norm_rope', 'k_tree_attn1', 'k_row_norm', 'k_mb_row_norm', 'k_mb_tree_attn')


def _time(fn, iters, warmup=5):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / iters * 1e3


def _engine(qk_norm, n_layers, seed=0):
    import torch
    from painlessinferenceacceleration_amd.llama_engine import LlamaShape, LlamaVerifyEngine, random_weights
    shape = LlamaShape.qwen3_8b()
    shape.n_layers = n_layers
    sd = random_weights(shape, seed=seed, device='cuda:0')                  # the same weights for both variants
    if not qk_norm:
        shape.qk_norm = False
        sd = {k: v for k, v in sd.items() if '_norm.weight' not in k or 'self_attn' not in k}
    eng = LlamaVerifyEngine(shape, sd, max_length=1024, consume_state_dict=True, n_slots=8, max_blocks=8)
    del sd
    torch.cuda.empty_cache()
    return shape, eng


def _inputs(shape, eng):
    from oracle.tiny import random_tree
    rs = np.random.RandomState(1)
    for b in range(8):
        eng.mprefill(b, rs.randint(3, shape.vocab, size=200).tolist())
    _, rows = random_tree(rs, 64)                       # (slot 0 hands its 200 keys to the single-sequence step as well)
    ids = rs.randint(3, shape.vocab, size=64).astype(np.int32)
    return ids, rows


def run_variant(qk_norm, iters, n_layers):
    import torch
    shape, eng = _engine(qk_norm, n_layers)
    ids, rows = _inputs(shape, eng)
    bs1 = _time(lambda: eng.verify_only(ids, rows), iters)
    prof = eng.profile(ids, rows, iters=3)
    blocks = [(b, ids, rows, 2, 16) for b in range(8)]
    bs8 = _time(lambda: eng.mstep(blocks), iters)
    logits = eng.mlogits()[:64].float().cpu()
    del eng
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return bs1, bs8, prof, bool(torch.isfinite(logits).all())


def kernel_run(n_layers, iters=20):
    """what the rocprofv3 run traces: the stage inside captured 64-row steps and inside 8-block steps"""
    import torch
    shape, eng = _engine(True, n_layers)
    ids, rows = _inputs(shape, eng)
    for _ in range(iters):
        eng.verify_only(ids, rows)
    blocks = [(b, ids, rows, 2, 16) for b in range(8)]
    for _ in range(iters):
        eng.mstep(blocks)
    torch.cuda.synchronize()


def merge_kernel_stats(trace_dir, out_path):
    """per-dispatch durations from the rocprofv3 result database (<dir>/**/*_results.db, table `kernels`); k_qk_norm_rope also split by
    the block count of its grid: 40 head slots x 1 block in the 64-row step, x 8 in the 8-block passes"""
    import sqlite3
    rows = {}
    for path in glob.glob(os.path.join(trace_dir, '**', '*_results.db'), recursive=True):
        db = sqlite3.connect(path)
        for name in COMPARE:
            d = np.array([(e - s_) / 1e3 for s_, e in db.execute(
                "select start, end from kernels where name like ? order by start", (f'%{name}%',))])
            if len(d):
                rows[name] = {'calls': len(d), 'average_us': round(float(d.mean()), 3), 'median_us': round(float(np.median(d)), 3),
                              'min_us': round(float(d.min()), 3), 'max_us': round(float(d.max()), 3)}
        # the stage by grid: blockIdx.y = the 64-row block, so grid y = 1 in the 64-row step and 8 in the 8-block passes
        cols = [c[0] for c in db.execute('select * from kernels limit 1').description]
        ycol = next((c for c in cols if 'grid' in c.lower() and c.lower().endswith('y')), None)
        for nblk in ((1, 8) if ycol else ()):
            d = np.array([(e - s_) / 1e3 for s_, e in db.execute(
                f"select start, end from kernels where name like '%k_qk_norm_rope%' and {ycol} = ? order by start", (nblk,))])
            if len(d):
                rows[f'k_qk_norm_rope_{64 * nblk}_rows'] = {
                    'calls': len(d), 'average_us': round(float(d.mean()), 3), 'median_us': round(float(np.median(d)), 3),
                    'min_us': round(float(d.min()), 3), 'max_us': round(float(d.max()), 3)}
    assert 'k_qk_norm_rope' in rows, f'no k_qk_norm_rope dispatch in the trace under {trace_dir}'
    out = json.load(open(out_path)) if out_path and os.path.exists(out_path) else {}
    out['kernel_trace'] = {'tool': 'rocprofv3 --kernel-trace --stats (a run of its own: --kernel-run, 20 64-row steps + 20 8-block steps)', **rows}
    for k, v in rows.items():
        print(f'{k:28s} calls {v["calls"]:6d}  mean {v["average_us"]:9.3f} us  median {v["median_us"]:9.3f} us  min {v["min_us"]:9.3f} us  max {v["max_us"]:9.3f} us')
    if out_path:
        with open(out_path, 'w') as f:
            json.dump(out, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--layers', type=int, default=36)
    ap.add_argument('--out', default='')
    ap.add_argument('--kernel-run', action='store_true')
    ap.add_argument('--merge-kernel-stats', default='')
    args = ap.parse_args()
    if args.merge_kernel_stats:
        return merge_kernel_stats(args.merge_kernel_stats, args.out)
    import torch
    assert torch.cuda.is_available(), 'needs an MI355X'
    if args.kernel_run:
        return kernel_run(args.layers)
    res = {t: {'bs1_ms': [], 'bs8_ms': [], 'class_ms': [], 'launches': None} for t in ('qk_norm', 'plain')}
    for _ in range(args.rounds):
        for tag in ('qk_norm', 'plain'):
            bs1, bs8, prof, finite = run_variant(tag == 'qk_norm', args.iters, args.layers)
            assert finite
            cls = {c: round(float(prof['ms'][c]), 4) for c in CLASSES}
            res[tag]['bs1_ms'].append(round(bs1, 4))
            res[tag]['bs8_ms'].append(round(bs8, 4))
            res[tag]['class_ms'].append(cls)
            res[tag]['launches'] = {c: int(prof['launches'][c]) for c in CLASSES}
            print(tag, f'bs1 {bs1:.3f} ms/step  bs8 {bs8:.3f} ms/step', cls, flush=True)
    out = {'model': 'Qwen3-8B shape, random init, bf16; bs1 = 64-row verify step, bs8 = 8 x 64-row mstep', 'n_layers': args.layers,
           'iters': args.iters, **res}
    for k in ('bs1_ms', 'bs8_ms'):
        a, b = np.median(res['qk_norm'][k]), np.median(res['plain'][k])
        out[k.replace('_ms', '_stage_cost_ms')] = round(float(a - b), 4)
        out[k.replace('_ms', '_stage_cost_us_per_layer')] = round(1e3 * float(a - b) / args.layers, 3)
        out[k.replace('_ms', '_stage_cost_pct')] = round(100.0 * float(a - b) / float(b), 3)
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f_:
            json.dump(out, f_, indent=1)


if __name__ == '__main__':
    main()
