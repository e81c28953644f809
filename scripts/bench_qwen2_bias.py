# -*- coding: utf-8 -*-
"""Cost of the Qwen2 q/k/v bias on the verify step: a 32-layer Qwen2.5-7B-shaped random-init model (hidden 3584, 28 / 4 heads,
ffn 18944, vocab 152064) timed with the bias (shape.qkv_bias, one lane-ordered vector per QKV launch) and with the same shape and the
bias pointer NULL, at bs=1 (the 64-row step, verify only) and bs=8 (la_llama_mstep, 8 x 64 rows, forward only).  Variants are built
one at a time and alternated (bias, null, bias, null, ...) so that drift of the box shows up as spread.

    python scripts/bench_qwen2_bias.py --iters 50 --rounds 2 [--out profiles/qwen2_bias_cost.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.tiny import random_tree  # noqa: E402
from painlessinferenceacceleration_amd.llama_engine import LlamaShape, LlamaVerifyEngine, random_weights  # noqa: E402


def _time(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / iters * 1e3


def run_variant(with_bias, iters, n_layers, seed=0):
    shape = LlamaShape.qwen2_7b()
    shape.n_layers = n_layers
    sd = random_weights(shape, seed=seed, device='cuda:0')
    if not with_bias:
        shape.qkv_bias = False
        sd = {k: v for k, v in sd.items() if not k.endswith('.bias')}
    eng = LlamaVerifyEngine(shape, sd, max_length=1024, n_slots=8, max_blocks=8, consume_state_dict=True)
    del sd
    rs = np.random.RandomState(1)
    for b in range(8):
        eng.mprefill(b, rs.randint(3, shape.vocab, size=200).tolist())
    _, rows = random_tree(rs, 64)
    ids = rs.randint(3, shape.vocab, size=64).astype(np.int32)
    eng.reset()
    eng.prefill(rs.randint(3, shape.vocab, size=200).tolist())
    bs1 = _time(lambda: eng.verify_only(ids, rows), iters)
    blocks = [(b, ids, rows, 2, 16) for b in range(8)]
    bs8 = _time(lambda: eng.mstep(blocks), iters)
    logits = eng.mlogits()[:64].float().cpu()
    del eng
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return bs1, bs8, bool(torch.isfinite(logits).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--layers', type=int, default=32)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    res = {'bias': {'bs1_ms': [], 'bs8_ms': []}, 'null': {'bs1_ms': [], 'bs8_ms': []}}
    for _ in range(args.rounds):
        for tag in ('bias', 'null'):
            bs1, bs8, finite = run_variant(tag == 'bias', args.iters, args.layers)
            assert finite
            res[tag]['bs1_ms'].append(round(bs1, 4))
            res[tag]['bs8_ms'].append(round(bs8, 4))
            print(tag, f'bs1 {bs1:.3f} ms/step  bs8 {bs8:.3f} ms/step', flush=True)
    out = {'model': 'Qwen2.5-7B shape, random init, bf16', 'n_layers': args.layers, 'iters': args.iters, **res}
    for k in ('bs1_ms', 'bs8_ms'):
        b, n = np.median(res['bias'][k]), np.median(res['null'][k])
        out[k.replace('_ms', '_bias_cost_pct')] = round(100.0 * (b - n) / n, 3)
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
