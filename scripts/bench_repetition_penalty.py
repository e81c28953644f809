# -*- coding: utf-8 -*-
"""What a repetition penalty costs at the Llama-2-7B shape (32 layers, decisive random init), bs=1, 64-token trees on a warm trie.
Three legs, alternated `--rounds` times on one box in one process, every leg one lookahead_generation request of `--new` tokens:

    a  no processor                                  (the fused greedy step, native loop: the headline path)
    b  RepetitionPenaltyLogitsProcessor(1.05) on the device  (csrc/la_penalty.hip: penalised argmax + the same fused path)
    c  the same processor on the host walk           (decoding_kwargs['device_processors'] = False: verify_only + pick() + commit)

Reported per leg and round: ms per step (mean of the per-step times behind the prefill), accepted tokens per step, tokens per
second; medians over the rounds and the ratios b / c and b / a.  Legs b and c emit the same tokens (asserted).

    timeout -k 10 900 python scripts/bench_repetition_penalty.py --rounds 3 --out profiles/repetition_penalty.json && \\
    timeout -k 10 600 rocprofv3 --kernel-trace --stats -d results/pen_trace -o pen -- \\
        python scripts/bench_repetition_penalty.py --legs b --rounds 1 && \\
    python scripts/bench_repetition_penalty.py --merge-kernel-stats results/pen_trace --out profiles/repetition_penalty.json

The second command is a run of its own (kernel trace only, no counters): its timings are not used, only the per-kernel durations of
k_pen_argmax / k_pen_update; the third (no GPU) merges them into the JSON.
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PENALTY = 1.05
LEGS = {'a': 'no processor', 'b': f'penalty {PENALTY} on the device', 'c': f'penalty {PENALTY} on the host walk'}


def merge_kernel_stats(trace_dir, out_path):
    rows = {}
    for path in glob.glob(os.path.join(trace_dir, '**', '*kernel_stats.csv'), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                name = r.get('Name', '')
                if 'k_pen_' in name:
                    key = 'k_pen_argmax' if 'k_pen_argmax' in name else 'k_pen_update'
                    rows[key] = {'calls': int(r['Calls']), 'average_us': round(float(r['AverageNs']) / 1e3, 3),
                                 'min_us': round(float(r['MinNs']) / 1e3, 3), 'max_us': round(float(r['MaxNs']) / 1e3, 3)}
    assert rows, f'no k_pen_* kernel in the stats under {trace_dir}'
    out = json.load(open(out_path)) if out_path and os.path.exists(out_path) else {}
    out['kernel_trace'] = {'tool': 'rocprofv3 --kernel-trace --stats (a run of its own, leg b)', **rows}
    print(json.dumps(out['kernel_trace']))
    if out_path:
        with open(out_path, 'w') as f:
            json.dump(out, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--legs', default='abc')
    ap.add_argument('--new', type=int, default=256, help='generated tokens per request')
    ap.add_argument('--prompt', type=int, default=96)
    ap.add_argument('--layers', type=int, default=32)
    ap.add_argument('--out', default='')
    ap.add_argument('--merge-kernel-stats', default='', metavar='DIR')
    args = ap.parse_args()
    if args.merge_kernel_stats:
        return merge_kernel_stats(args.merge_kernel_stats, args.out)

    import torch
    from transformers import LogitsProcessorList, RepetitionPenaltyLogitsProcessor
    from painlessinferenceacceleration_amd.llama_engine import LlamaShape
    from painlessinferenceacceleration_amd.lookahead_cache import LookaheadCache
    from painlessinferenceacceleration_amd.modeling_llama import LlamaForCausalLM
    assert torch.cuda.is_available(), 'needs an MI355X'
    shape = LlamaShape.llama2_7b()
    shape.n_layers = args.layers
    model = LlamaForCausalLM.random_init(shape, seed=0, max_length=args.prompt + args.new + 128, decisive=True, eos_token_id=None)
    rs = np.random.RandomState(2)
    prompt = torch.tensor([rs.randint(3, shape.vocab, size=args.prompt).tolist()])
    procs = LogitsProcessorList([RepetitionPenaltyLogitsProcessor(PENALTY)])
    # one trie per token stream (the penalty changes tokens): legs b and c share theirs; each is warmed by an untimed request
    caches = {'a': LookaheadCache(), 'b': LookaheadCache()}
    caches['c'] = caches['b']

    def request(leg):
        model.lookahead_cache = caches[leg]
        dk = {'use_lookahead': True, 'decoding_length': 64, 'branch_length': 12, 'stop_words': {}, 'device_processors': leg != 'c'}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.lookahead_generation(prompt, logits_processor=None if leg == 'a' else procs, stopping_criteria=args.prompt + args.new,
                                         eos_token_id=[None], return_dict_in_generate=True, decoding_kwargs=dk)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
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
            assert toks[leg] == seq, f'leg {leg}: tokens changed between rounds'
            print(leg, LEGS[leg], stats, flush=True)
    if 'b' in toks and 'c' in toks:
        assert toks['b'] == toks['c'], 'device path and host walk emitted different tokens'
    out = {'model': f'Llama-2-7B shape, {args.layers} layers, decisive random init, bs=1, decoding_length 64, branch_length 12, warm trie',
           'penalty': PENALTY, 'prompt_tokens': args.prompt, 'new_tokens': args.new, 'rounds': args.rounds,
           'device': torch.cuda.get_device_name(0), 'legs': {leg: {'what': LEGS[leg], 'runs': res[leg]} for leg in legs}}
    med = {leg: {k: float(np.median([x[k] for x in res[leg]])) for k in ('ms_per_step', 'accepted_per_step', 'tok_per_s')} for leg in legs}
    spread = {leg: round(float((max(x['ms_per_step'] for x in res[leg]) - min(x['ms_per_step'] for x in res[leg])) / med[leg]['ms_per_step']), 4)
              for leg in legs}
    out['median'] = med
    out['ms_per_step_spread_over_rounds'] = spread
    if 'b' in med and 'c' in med:
        out['b_over_c_ms_per_step'] = round(med['b']['ms_per_step'] / med['c']['ms_per_step'], 4)
        out['b_over_c_tok_per_s'] = round(med['b']['tok_per_s'] / med['c']['tok_per_s'], 4)
    if 'b' in med and 'a' in med:
        out['b_over_a_ms_per_step'] = round(med['b']['ms_per_step'] / med['a']['ms_per_step'], 4)
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
