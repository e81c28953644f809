# -*- coding: utf-8 -*-
"""FP8 (e4m3fn) weight-only projections against bf16 at the Llama-2-7B shape (32 layers, random init), bs=1, 64-row verify steps.
Variants are built one at a time and alternated (bf16, fp8, bf16, fp8, ...) on one box, with the step timing of
scripts/bench_qwen2_bias.py, and each adds the la_llama_profile class times (qkv / o / gate-up / down) of one step.

    python scripts/bench_fp8_weights.py --iters 50 --rounds 2 [--out profiles/fp8_weights.json]
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

CLASSES = ('qkv', 'o', 'gateup', 'down', 'lm_head', 'attn', 'other')


def _time(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / iters * 1e3


def run_variant(fmt, iters, n_layers, seed=0):
    shape = LlamaShape.llama2_7b()
    shape.n_layers = n_layers
    sd = random_weights(shape, seed=seed, device='cuda:0')
    eng = LlamaVerifyEngine(shape, sd, max_length=1024, consume_state_dict=True, weight_format=fmt)
    del sd
    rs = np.random.RandomState(1)
    _, rows = random_tree(rs, 64)
    ids = rs.randint(3, shape.vocab, size=64).astype(np.int32)
    eng.prefill(rs.randint(3, shape.vocab, size=200).tolist())
    ms = _time(lambda: eng.verify_only(ids, rows), iters)
    prof = eng.profile(ids, rows, iters=3)
    logits = eng.logits()[:64].float().cpu()
    del eng
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return ms, prof, bool(torch.isfinite(logits).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--layers', type=int, default=32)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    res = {'bf16': {'step_ms': [], 'class_ms': []}, 'fp8': {'step_ms': [], 'class_ms': []}}
    for _ in range(args.rounds):
        for tag in ('bf16', 'fp8'):
            ms, prof, finite = run_variant('fp8' if tag == 'fp8' else None, args.iters, args.layers)
            assert finite
            cls = {c: round(float(prof['ms'][c]), 4) for c in CLASSES}
            res[tag]['step_ms'].append(round(ms, 4))
            res[tag]['class_ms'].append(cls)
            print(tag, f'{ms:.3f} ms/step', cls, flush=True)
    out = {'model': 'Llama-2-7B shape, random init, bs=1, 64-row verify step', 'n_layers': args.layers, 'iters': args.iters, **res}
    b, f = np.median(res['bf16']['step_ms']), np.median(res['fp8']['step_ms'])
    out['fp8_over_bf16_step'] = round(float(f / b), 4)
    for c in ('qkv', 'o', 'gateup', 'down'):
        cb = np.median([r[c] for r in res['bf16']['class_ms']])
        cf = np.median([r[c] for r in res['fp8']['class_ms']])
        out[f'fp8_over_bf16_{c}'] = round(float(cf / cb), 4) if cb > 0 else None
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f_:
            json.dump(out, f_, indent=1)


if __name__ == '__main__':
    main()
