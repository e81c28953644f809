# -*- coding: utf-8 -*-
"""ORACLE tooling (build container only): the REFERENCE's own CPU loop as bench.py's `cpu_baseline` leg of kind "reference"
(oracle/reference_cpu.py::reference_lookahead_loop) on the tiny decisive model, recorded so that
tests/test_bench_helpers_cpu.py can hold the port (kind "port") to it without the reference present.

Writes tests/golden/cpu_baseline_reference_leg.json: the leg's emitted tokens and its per-step draft / accept means (no timings).
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'tests', 'golden', 'cpu_baseline_reference_leg.json')
KEYS = ('kind', 'verify_steps', 'cores', 'dtype', 'tokens', 'mean_accept_len', 'mean_draft_len')


def leg_inputs():
    """-> (shape, fp32 state dict, 40-token prompt, prompt + 60 greedy tokens, 6 noisy copies of the continuation for the trie)"""
    import bench
    from oracle import llama_oracle as lo
    from tests.tiny_model import tiny_decisive_weights, tiny_shape
    s = tiny_shape()
    sd = tiny_decisive_weights(0, torch.float32)
    prompt = bench.phrase_prompt(7, 40, s.vocab)
    model = lo.OracleLlama(s, sd)
    seq = list(prompt)
    lg, past = model.forward(torch.tensor(seq), torch.tril(torch.ones((40, 40), dtype=torch.long)), None)
    for _ in range(60):
        t = int(lg[-1].float().argmax())
        seq.append(t)
        lg, past = model.forward(torch.tensor([t]), torch.ones((1, len(seq)), dtype=torch.long), past)
    copies = bench.noisy_copies(prompt[-2:] + seq[40:], 6, 0.3, s.vocab, seed=99)
    return s, sd, prompt, seq, copies


def main():
    from oracle import reference_cpu
    assert reference_cpu.reference_available(), 'needs the reference sources'
    s, sd, prompt, _, copies = leg_inputs()
    ref = reference_cpu.reference_lookahead_loop(s, sd, prompt, copies, 12, 64, verify_steps=4, threads=2, dtype=torch.float32)
    assert ref['value'] > 0
    with open(OUT, 'w') as f:
        json.dump({k: ref[k] for k in KEYS}, f, separators=(',', ':'))
    print('wrote', OUT, {k: ref[k] for k in KEYS if k != 'tokens'}, len(ref['tokens']), 'tokens')


if __name__ == '__main__':
    main()
