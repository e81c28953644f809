# -*- coding: utf-8 -*-
"""What do_sample costs at the Llama-2-7B shape (32 layers, decisive random init), bs=1, 64-row trees on a warm trie.
Three legs, alternated `--rounds` times on one box in one process, every leg one lookahead_generation request of `--new` tokens:

    a  greedy, no processor                       (the fused greedy step, native loop: the headline path)
    b  do_sample on the device                    (csrc/la_sample.hip: temperature 0.8, top_k 50, top_p 0.95, sample_seed given)
    c  do_sample on the host walk                 (the same warpers, sample_seed absent: verify_only + softmax + multinomial + commit)

Reported per leg and round: ms per step (mean of the per-step times behind the prefill), accepted tokens per step, tokens per
second; medians over the rounds and the ratios b / c and b / a.  Leg c is the path leg b replaces; leg a only shows the delta of
the stage.  Legs b and c draw with different random numbers, so their tokens (and accept lengths) differ; leg b repeats its tokens
round after round (asserted).

    timeout -k 10 900 python scripts/bench_device_sampling.py --rounds 3 --out profiles/device_sampling.json && \\
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d results/samp_trace_32000 -o samp -- \\
        python scripts/bench_device_sampling.py --kernel-rows 32000 && \\
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d results/samp_trace_152064 -o samp -- \\
        python scripts/bench_device_sampling.py --kernel-rows 152064 && \\
    python scripts/bench_device_sampling.py --merge-kernel-stats results/samp_trace_32000,results/samp_trace_152064 \\
        --out profiles/device_sampling.json

The rocprofv3 commands are runs of their own (kernel trace only, no counters): 64 rows of N(0, 2) logits through la_sample_rows,
2 x 200 launches per setting (the flagship setting, top_p alone, no filter); the last command (no GPU) reads the per-dispatch
durations from the result databases and merges them into the JSON and profiles/device_sampling_kernel_stats.txt.
"""
import argparse
import ctypes as C
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TEMPERATURE, TOP_K, TOP_P, SEED = 0.8, 50, 0.95, 7
LEGS = {'a': 'greedy, no processor', 'b': f'do_sample on the device (T {TEMPERATURE}, top_k {TOP_K}, top_p {TOP_P})',
        'c': 'do_sample on the host walk (same warpers, no sample_seed)'}


KERNEL_SETTINGS = (('flagship', (TOP_K, TOP_P)), ('top_p_only', (0, TOP_P)), ('no_filter', (0, 1.0)))
KERNEL_ITERS = 200


def merge_kernel_stats(trace_dirs, out_path):
    """per-dispatch durations of k_sample_rows from the rocprofv3 result databases (<dir>/*_results.db, table `kernels`), split by the
    setting order of kernel_rows: 2 x KERNEL_ITERS launches per setting"""
    import sqlite3
    rows, text = {}, []
    for trace_dir in trace_dirs.split(','):
        vocab = trace_dir.rstrip('/').split('_')[-1]
        for path in glob.glob(os.path.join(trace_dir, '**', '*_results.db'), recursive=True):
            db = sqlite3.connect(path)
            d = np.array([(e - s_) / 1e3 for s_, e in db.execute(
                "select start, end from kernels where name like '%k_sample_rows%' order by start")])
            per = 2 * KERNEL_ITERS
            assert len(d) == per * len(KERNEL_SETTINGS), (path, len(d))
            for i, (name, (k, p)) in enumerate(KERNEL_SETTINGS):
                g = d[i * per:(i + 1) * per]
                rows[f'k_sample_rows_vocab_{vocab}_{name}'] = {
                    'top_k': k, 'top_p': p, 'calls': len(g), 'average_us': round(float(g.mean()), 3),
                    'min_us': round(float(g.min()), 3), 'max_us': round(float(g.max()), 3)}
                text.append(f'k_sample_rows  vocab {vocab:>6}  64 rows  bf16  T {TEMPERATURE}  top_k {k:>2}  top_p {p:<4}  '
                            f'calls {len(g)}  mean {g.mean():8.3f} us  min {g.min():8.3f} us  max {g.max():8.3f} us')
    assert rows, f'no k_sample_rows dispatch in the traces under {trace_dirs}'
    out = json.load(open(out_path)) if out_path and os.path.exists(out_path) else {}
    out['kernel_trace'] = {'tool': 'rocprofv3 --kernel-trace --stats (runs of their own: --kernel-rows VOCAB, 64 rows of N(0, 2) bf16 logits)',
                           **rows}
    print('\n'.join(text))
    if out_path:
        with open(out_path, 'w') as f:
            json.dump(out, f, indent=1)
        with open(os.path.splitext(out_path)[0] + '_kernel_stats.txt', 'w') as f:
            f.write('rocprofv3 --kernel-trace --stats, one run per vocabulary (scripts/bench_device_sampling.py --kernel-rows VOCAB)\n')
            f.write('\n'.join(text) + '\n')


def kernel_rows(vocab, iters=KERNEL_ITERS):
    """64 rows of N(0, 2) bf16 logits through la_sample_rows: the flagship setting, then top_k off, then no filter at all"""
    import torch
    from painlessinferenceacceleration_amd import _lib
    assert torch.cuda.is_available(), 'needs an MI355X'
    lib = _lib.lib
    g = torch.Generator(device='cuda:0').manual_seed(0)
    lg = (torch.randn(64, vocab, generator=g, device='cuda:0') * 2).to(torch.bfloat16)
    pos = torch.arange(64, dtype=torch.int32, device='cuda:0')
    zi = torch.zeros(64, dtype=torch.int32, device='cuda:0')
    zl = torch.zeros(64, dtype=torch.int64, device='cuda:0')
    tok = torch.zeros(64, dtype=torch.int32, device='cuda:0')
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {}
    for name, (k, p) in KERNEL_SETTINGS:
        for timed in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                rc = lib.la_sample_rows(st, C.c_void_p(lg.data_ptr()), vocab, 64, C.c_void_p(pos.data_ptr()), 0, SEED, TEMPERATURE, k, p,
                                        None, C.c_void_p(zi.data_ptr()), C.c_void_p(zl.data_ptr()), None, C.c_void_p(tok.data_ptr()), None)
                assert rc == 0, rc
            torch.cuda.synchronize()
            if timed:
                res[name] = round((time.perf_counter() - t0) / iters * 1e6, 2)
    print(json.dumps({'vocab': vocab, 'us_per_launch_host_clock': res}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--legs', default='abc')
    ap.add_argument('--new', type=int, default=256, help='generated tokens per request')
    ap.add_argument('--prompt', type=int, default=96)
    ap.add_argument('--layers', type=int, default=32)
    ap.add_argument('--out', default='')
    ap.add_argument('--merge-kernel-stats', default='', metavar='DIR[,DIR]')
    ap.add_argument('--kernel-rows', type=int, default=0, metavar='VOCAB')
    args = ap.parse_args()
    if args.merge_kernel_stats:
        return merge_kernel_stats(args.merge_kernel_stats, args.out)
    if args.kernel_rows:
        return kernel_rows(args.kernel_rows)

    import torch
    from transformers import LogitsProcessorList, TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    from painlessinferenceacceleration_amd.llama_engine import LlamaShape
    from painlessinferenceacceleration_amd.lookahead_cache import LookaheadCache
    from painlessinferenceacceleration_amd.modeling_llama import LlamaForCausalLM
    assert torch.cuda.is_available(), 'needs an MI355X'
    shape = LlamaShape.llama2_7b()
    shape.n_layers = args.layers
    model = LlamaForCausalLM.random_init(shape, seed=0, max_length=args.prompt + args.new + 128, decisive=True, eos_token_id=None)
    rs = np.random.RandomState(2)
    prompt = torch.tensor([rs.randint(3, shape.vocab, size=args.prompt).tolist()])
    procs = LogitsProcessorList([TemperatureLogitsWarper(TEMPERATURE), TopKLogitsWarper(TOP_K), TopPLogitsWarper(TOP_P)])
    caches = {leg: LookaheadCache() for leg in LEGS}          # one trie per token stream; each is warmed by an untimed request

    def request(leg):
        model.lookahead_cache = caches[leg]
        dk = {'use_lookahead': True, 'decoding_length': 64, 'branch_length': 12, 'stop_words': {}, 'do_sample': leg != 'a'}
        if leg == 'b':
            dk['sample_seed'] = SEED
        torch.manual_seed(0)                                  # leg c draws from torch's global generator
        n0 = model.engine.sample_launches()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.lookahead_generation(prompt, logits_processor=None if leg == 'a' else procs, stopping_criteria=args.prompt + args.new,
                                         eos_token_id=[None], return_dict_in_generate=True, decoding_kwargs=dk)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        assert (model.engine.sample_launches() > n0) == (leg == 'b'), 'the stage runs in leg b and only there'
        fts, edls = out.kwargs['fts'][1:], out.kwargs['edls'][1:]
        n_new = out.sequences.shape[1] - args.prompt
        return {'ms_per_step': round(float(np.mean(fts)) * 1e3, 4), 'accepted_per_step': round(float(np.mean(edls)), 3),
                'steps': len(fts), 'tok_per_s': round(sum(edls) / float(np.sum(fts)), 1), 'wall_s': round(wall, 4),
                'new_tokens': int(n_new)}, out.sequences[0].tolist()

    legs = [c for c in args.legs if c in LEGS]
    for leg in legs:
        request(leg)                                       # warm-up: trie, graph capture, code objects
    res = {leg: [] for leg in legs}
    toks = {}
    for r in range(args.rounds):
        for leg in legs:
            stats, seq = request(leg)
            res[leg].append(stats)
            toks.setdefault(leg, seq)
            if leg != 'c':
                assert toks[leg] == seq, f'leg {leg}: tokens changed between rounds'
            print(leg, LEGS[leg], stats, flush=True)
    out = json.load(open(args.out)) if args.out and os.path.exists(args.out) else {}
    out.update({'model': f'Llama-2-7B shape, {args.layers} layers, decisive random init, bs=1, decoding_length 64, branch_length 12, warm trie',
                'sampling': {'temperature': TEMPERATURE, 'top_k': TOP_K, 'top_p': TOP_P, 'sample_seed': SEED},
                'prompt_tokens': args.prompt, 'new_tokens': args.new, 'rounds': args.rounds,
                'device': torch.cuda.get_device_name(0), 'legs': {leg: {'what': LEGS[leg], 'runs': res[leg]} for leg in legs}})
    med = {leg: {k: float(np.median([x[k] for x in res[leg]])) for k in ('ms_per_step', 'accepted_per_step', 'tok_per_s')} for leg in legs}
    spread = {leg: round(float((max(x['ms_per_step'] for x in res[leg]) - min(x['ms_per_step'] for x in res[leg])) / med[leg]['ms_per_step']), 4)
              for leg in legs}
    out['median'] = med
    out['ms_per_step_spread_over_rounds'] = spread
    if 'b' in med and 'c' in med:
        out['b_over_c_ms_per_step'] = round(med['b']['ms_per_step'] / med['c']['ms_per_step'], 4)
        out['b_over_c_tok_per_s'] = round(med['b']['tok_per_s'] / med['c']['tok_per_s'], 4)
        out['condition_b_ms_per_step_below_c'] = bool(med['b']['ms_per_step'] < med['c']['ms_per_step'])
    if 'b' in med and 'a' in med:
        out['b_over_a_ms_per_step'] = round(med['b']['ms_per_step'] / med['a']['ms_per_step'], 4)
        out['stage_delta_ms_per_step'] = round(med['b']['ms_per_step'] - med['a']['ms_per_step'], 4)
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
