# -*- coding: utf-8 -*-
"""What top-N log-probabilities cost at the Llama-2-7B shape (32 layers, decisive random init), bs=1, 64-row trees on a warm trie.
Four legs, alternated `--rounds` times on one box in one process, every leg one lookahead_generation request of `--new` tokens:

    a  greedy, stages off                          (the fused greedy step, native loop: the headline path)
    b  greedy, decoding_kwargs['output_logprobs']  (k_logprob_rows behind the accept scan of every step)
    c  greedy, decoding_kwargs['top_logprobs'] = 5 (b + k_top_logprob_rows: csrc/la_logprob.hip)
    d  greedy, decoding_kwargs['top_logprobs'] = 20

Reported per leg and round: ms per step (mean of the per-step times behind the prefill), accepted tokens per step, tokens per
second; medians over the rounds and every leg's ratio to a.  There is no pass bar: the cost is reported next to the scalar stage's
(profiles/device_logprobs.json).  All legs emit the same tokens (asserted).

    timeout -k 10 900 python scripts/bench_top_logprobs.py --rounds 3 --out profiles/top_logprobs.json && \\
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d results/tlp_trace_32000 -o tlp -- \\
        python scripts/bench_top_logprobs.py --kernel-rows 32000 && \\
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d results/tlp_trace_152064 -o tlp -- \\
        python scripts/bench_top_logprobs.py --kernel-rows 152064 && \\
    python scripts/bench_top_logprobs.py --merge-kernel-stats results/tlp_trace_32000,results/tlp_trace_152064 \\
        --out profiles/top_logprobs.json

The rocprofv3 commands are runs of their own (kernel trace only, no counters): N(0, 2) logits through la_top_logprob_rows with n = 5
and 20 and 1, 7 and 13 rows (the rows a step keeps: the root alone, a typical accept, branch_length + 1), 2 x 200 launches per
setting; the last command (no GPU) reads the per-dispatch durations from the result databases and merges them into the JSON and
profiles/top_logprobs_kernel_stats.txt.
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

LEGS = {'a': 'greedy, stages off', 'b': 'greedy, output_logprobs (the scalar stage in every step)',
        'c': 'greedy, top_logprobs = 5 (scalar stage + top-N stage in every step)', 'd': 'greedy, top_logprobs = 20'}
TOP = {'c': 5, 'd': 20}
KERNEL_N = (5, 20)
KERNEL_ROWS = (1, 7, 13)
KERNEL_ITERS = 200


def merge_kernel_stats(trace_dirs, out_path):
    """per-dispatch durations of k_top_logprob_rows from the rocprofv3 result databases (<dir>/*_results.db, table `kernels`), split by
    the (n, row count) settings of kernel_rows: 2 x KERNEL_ITERS launches per setting"""
    import sqlite3
    rows, text = {}, []
    for trace_dir in trace_dirs.split(','):
        vocab = trace_dir.rstrip('/').split('_')[-1]
        for path in glob.glob(os.path.join(trace_dir, '**', '*_results.db'), recursive=True):
            db = sqlite3.connect(path)
            d = np.array([(e - s_) / 1e3 for s_, e in db.execute(
                "select start, end from kernels where name like '%k_top_logprob_rows%' order by start")])
            per = 2 * KERNEL_ITERS
            assert len(d) == per * len(KERNEL_ROWS) * len(KERNEL_N), (path, len(d))
            i = 0
            for n in KERNEL_N:
                for kept in KERNEL_ROWS:
                    g = d[i * per:(i + 1) * per]
                    i += 1
                    rows[f'k_top_logprob_rows_vocab_{vocab}_n_{n}_rows_{kept}'] = {
                        'n': n, 'kept_rows': kept, 'calls': len(g), 'average_us': round(float(g.mean()), 3),
                        'min_us': round(float(g.min()), 3), 'max_us': round(float(g.max()), 3)}
                    text.append(f'k_top_logprob_rows  vocab {vocab:>6}  n {n:>2}  {kept:>2} kept rows  bf16  calls {len(g)}  '
                                f'mean {g.mean():8.3f} us  min {g.min():8.3f} us  max {g.max():8.3f} us')
    assert rows, f'no k_top_logprob_rows dispatch in the traces under {trace_dirs}'
    out = json.load(open(out_path)) if out_path and os.path.exists(out_path) else {}
    out['kernel_trace'] = {'tool': 'rocprofv3 --kernel-trace --stats (runs of their own: --kernel-rows VOCAB, N(0, 2) bf16 logits)', **rows}
    print('\n'.join(text))
    if out_path:
        with open(out_path, 'w') as f:
            json.dump(out, f, indent=1)
        with open(os.path.splitext(out_path)[0] + '_kernel_stats.txt', 'w') as f:
            f.write('rocprofv3 --kernel-trace --stats, one run per vocabulary (scripts/bench_top_logprobs.py --kernel-rows VOCAB)\n')
            f.write('\n'.join(text) + '\n')


def kernel_rows(vocab, iters=KERNEL_ITERS):
    """N(0, 2) bf16 logits through la_top_logprob_rows with n = 5 and 20 and 1, 7 and 13 rows: the workgroups that work in a step are
    its kept rows"""
    import torch
    from painlessinferenceacceleration_amd import _lib
    assert torch.cuda.is_available(), 'needs an MI355X'
    lib = _lib.lib
    g = torch.Generator(device='cuda:0').manual_seed(0)
    lg = (torch.randn(64, vocab, generator=g, device='cuda:0') * 2).to(torch.bfloat16)
    ids = torch.zeros((64, 20), dtype=torch.int32, device='cuda:0')
    vals = torch.zeros((64, 20), dtype=torch.float32, device='cuda:0')
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {}
    for n in KERNEL_N:
        for kept in KERNEL_ROWS:
            for timed in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(iters):
                    rc = lib.la_top_logprob_rows(st, C.c_void_p(lg.data_ptr()), vocab, kept, n, C.c_void_p(ids.data_ptr()),
                                                 C.c_void_p(vals.data_ptr()))
                    assert rc == 0, rc
                torch.cuda.synchronize()
                if timed:
                    res[f'n_{n}_rows_{kept}'] = round((time.perf_counter() - t0) / iters * 1e6, 2)
    print(json.dumps({'vocab': vocab, 'us_per_launch_host_clock': res}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
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
    from painlessinferenceacceleration_amd.llama_engine import LlamaShape
    from painlessinferenceacceleration_amd.lookahead_cache import LookaheadCache
    from painlessinferenceacceleration_amd.modeling_llama import LlamaForCausalLM
    assert torch.cuda.is_available(), 'needs an MI355X'
    shape = LlamaShape.llama2_7b()
    shape.n_layers = args.layers
    model = LlamaForCausalLM.random_init(shape, seed=0, max_length=args.prompt + args.new + 128, decisive=True, eos_token_id=None)
    rs = np.random.RandomState(2)
    prompt = torch.tensor([rs.randint(3, shape.vocab, size=args.prompt).tolist()])
    caches = {leg: LookaheadCache() for leg in LEGS}          # one trie per leg; each is warmed by an untimed request

    def request(leg):
        model.lookahead_cache = caches[leg]
        dk = {'use_lookahead': True, 'decoding_length': 64, 'branch_length': 12, 'stop_words': {}}
        if leg == 'b':
            dk['output_logprobs'] = True
        if leg in TOP:
            dk['top_logprobs'] = TOP[leg]
        n0 = model.engine.logprob_launches()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.lookahead_generation(prompt, stopping_criteria=args.prompt + args.new, eos_token_id=[None],
                                         return_dict_in_generate=True, decoding_kwargs=dk)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        assert (model.engine.logprob_launches() > n0) == (leg != 'a'), 'the stages run in legs b, c, d and only there'
        fts, edls = out.kwargs['fts'][1:], out.kwargs['edls'][1:]
        n_new = out.sequences.shape[1] - args.prompt
        if leg != 'a':
            lps = out.kwargs['logprobs']
            assert len(lps) == n_new and all(np.isfinite(x) and x <= 0 for x in lps)
        if leg in TOP:
            tops = out.kwargs['top_logprobs']
            assert len(tops) == n_new and all(len(row) == TOP[leg] for row in tops)
            assert [row[0][0] for row in tops] == out.sequences[0].tolist()[args.prompt:], 'entry 0 is the greedy token'
        return {'ms_per_step': round(float(np.mean(fts)) * 1e3, 4), 'accepted_per_step': round(float(np.mean(edls)), 3),
                'steps': len(fts), 'tok_per_s': round(sum(edls) / float(np.sum(fts)), 1), 'wall_s': round(wall, 4),
                'new_tokens': int(n_new)}, out.sequences[0].tolist()

    for leg in LEGS:
        request(leg)                                       # warm-up: trie, graph capture, code objects
    res = {leg: [] for leg in LEGS}
    toks = None
    for r in range(args.rounds):
        for leg in LEGS:
            stats, seq = request(leg)
            res[leg].append(stats)
            toks = seq if toks is None else toks
            assert toks == seq, f'leg {leg}: the tokens differ from the first request'
            print(leg, LEGS[leg], stats, flush=True)
    out = json.load(open(args.out)) if args.out and os.path.exists(args.out) else {}
    out.update({'model': f'Llama-2-7B shape, {args.layers} layers, decisive random init, bs=1, decoding_length 64, branch_length 12, warm trie',
                'prompt_tokens': args.prompt, 'new_tokens': args.new, 'rounds': args.rounds,
                'device': torch.cuda.get_device_name(0), 'legs': {leg: {'what': LEGS[leg], 'runs': res[leg]} for leg in LEGS}})
    med = {leg: {k: float(np.median([x[k] for x in res[leg]])) for k in ('ms_per_step', 'accepted_per_step', 'tok_per_s')} for leg in LEGS}
    out['median'] = med
    out['ms_per_step_spread_over_rounds'] = {
        leg: round(float((max(x['ms_per_step'] for x in res[leg]) - min(x['ms_per_step'] for x in res[leg])) / med[leg]['ms_per_step']), 4)
        for leg in LEGS}
    out['over_a_ms_per_step'] = {leg: round(med[leg]['ms_per_step'] / med['a']['ms_per_step'], 4) for leg in 'bcd'}
    out['delta_ms_per_step_over_a'] = {leg: round(med[leg]['ms_per_step'] - med['a']['ms_per_step'], 4) for leg in 'bcd'}
    out['top_n_delta_ms_per_step_over_b'] = {leg: round(med[leg]['ms_per_step'] - med['b']['ms_per_step'], 4) for leg in 'cd'}
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
