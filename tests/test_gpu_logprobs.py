# -*- coding: utf-8 -*-
"""GPU: per-token log-probabilities on the device (csrc/la_logprob.hip) against the numpy fp64 model of tests/logprob_model.py.

Bound of every value against the fp64 model on the SAME stored logits: 1e-4 + 2^-22 |lp| (logprob_model.bound_device: the
integer-mass bound V * 2^-32 <= 3.5e-5 that tests/test_logprobs_cpu.py checks on the CPU, plus a margin for the ulps of expf / logf).
Lookahead against no-draft (section 6): |dlp| <= 4 * TOL * max|logit| of the position — each path's logits row is within
TOL * max|logit| of the oracle's (tests/test_gpu_e2e.py), and lp is 2-Lipschitz in the sup norm of the row."""
import numpy as np
import pytest
import torch

from oracle import llama_oracle as lo
from painlessinferenceacceleration_amd import _lib
from painlessinferenceacceleration_amd._lib import check
from painlessinferenceacceleration_amd.llama_engine import LlamaVerifyEngine
from painlessinferenceacceleration_amd.lookahead_cache import LookaheadCache
from painlessinferenceacceleration_amd.modeling_llama import LlamaForCausalLM
from painlessinferenceacceleration_amd.modeling_llama_batch import LlamaForCausalLM as BatchLlama
from tests import logprob_model as lm
from tests.gpu_utils import DEV, ptr, sp
from tests.test_gpu_e2e import TOL
from tests.tiny_model import tiny_decisive_weights, tiny_shape, tiny_weights

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
IDS = ['bf16', 'fp16']
ONE = np.array([1], dtype=np.uint64)
WORST = {'rows': 0.0, 'steps': 0.0, 'doors': 0.0}      # worst measured error / bound (rows, steps) and |dlp| (doors) of the session: printed


def _name(dtype):
    return str(dtype).replace('torch.', '')


# ------------------------------------------------------------------------------------------------ 1. the row stage alone
_ROWS = {}


def _rows(V, dtype):
    """the planted rows of one (vocab, dtype) and their fp64 values, computed once"""
    key = (V, dtype)
    if key not in _ROWS:
        rows, toks = lm.planted_rows(V, _name(dtype), n_rows=64)
        _ROWS[key] = (rows, toks, lm.logprob_f64(rows, toks))
    return _ROWS[key]


def _run_rows(lib, lg_dev, toks):
    n = lg_dev.shape[0]
    d_tok = torch.from_numpy(np.asarray(toks, dtype=np.int32)).to(DEV)
    out = torch.full((64,), 7.0, dtype=torch.float32, device=DEV)
    check(lib.la_logprob_rows(sp(), ptr(lg_dev), lg_dev.shape[1], n, ptr(d_tok), ptr(out)), 'logprob_rows')
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert (out[n:] == 7.0).all()                                              # rows past n_rows store nothing
    return out[:n]


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('n_rows', [1, 64])
@pytest.mark.parametrize('V', [512, 32000, 152064])
def test_row_stage_equals_the_fp64_model(V, n_rows, dtype):
    lib = _lib.lib_for(dtype)
    rows, toks, want = _rows(V, dtype)
    lg = torch.from_numpy(rows[:n_rows]).to(dtype)
    assert (lg.float().numpy() == rows[:n_rows]).all()                         # the rows are values of the storage type
    lg_dev = lg.to(DEV).contiguous()
    got = _run_rows(lib, lg_dev, toks[:n_rows])
    err, bound = np.abs(got.astype(np.float64) - want[:n_rows]), lm.bound_device(want[:n_rows])
    WORST['rows'] = max(WORST['rows'], float((err / bound).max()))
    print(f'V={V} n_rows={n_rows} {_name(dtype)}: worst err {err.max():.3e}, worst err / bound {(err / bound).max():.3e} '
          f'(session {WORST["rows"]:.3e})')
    assert np.all(np.isfinite(got)) and np.all(err <= bound), (err, bound)
    again = _run_rows(lib, lg_dev, toks[:n_rows])
    assert got.tobytes() == again.tobytes()                                    # the same bits on every run
    if n_rows == 64:                                                           # ... and at every row index
        perm = np.random.RandomState(1).permutation(64)
        moved = _run_rows(lib, lg_dev[torch.from_numpy(perm).to(DEV)].contiguous(), toks[perm])
        assert moved.tobytes() == got[perm].tobytes()
        tok_out = toks.copy()
        tok_out[0], tok_out[1] = -1, V                                         # a token outside the row: NaN, nothing read
        bad = _run_rows(lib, lg_dev, tok_out)
        assert np.isnan(bad[:2]).all() and bad[2:].tobytes() == got[2:].tobytes()


# ------------------------------------------------------------------------------------------------ 2. the stage inside the steps
def _sd(dtype):
    return {k: v.to(dtype) for k, v in tiny_weights(0, torch.float32).items()}


def _planted_tree(root, cont, k, depth, rs, vocab):
    """Rows root, main_1, sib_1, main_2, sib_2, ...: the main chain carries the greedy continuation `cont` for k depths and then
    leaves it; every depth has a wrong sibling, so dropped rows share their position with kept ones.  -> ids, uint64 row masks."""
    def wrong(t):
        w = int(rs.randint(3, vocab))
        return w if w != t else (w + 1 - 3) % (vocab - 3) + 3
    ids, rm = [int(root)], [1]
    chain = 1
    for d in range(1, depth + 1):
        good = int(cont[d - 1])
        main = len(ids)
        ids.append(good if d <= k else wrong(good))
        rm.append(chain | (1 << main))
        ids.append(wrong(good))
        rm.append(chain | (1 << (main + 1)))
        chain |= 1 << main
    return np.asarray(ids, dtype=np.int32), np.asarray(rm, dtype=np.uint64)


def _depths(rm):
    return [bin(int(m)).count('1') - 1 for m in rm]


def _mask_matrix(rm):
    T = len(rm)
    return np.array([[(int(rm[i]) >> j) & 1 for j in range(T)] for i in range(T)], dtype=np.int64)


def _model_rows(lg_rows, toks):
    """the fp64 model on rows of the engine's own logits buffer"""
    return lm.logprob_f64(lg_rows.float().cpu().numpy(), np.asarray(toks, dtype=np.int64))


def _check_positions(eng, slot, expected, first, n=160):
    """the slot's log from position `first` on: the expected value (within the bound) where a token was emitted, NaN elsewhere"""
    log = eng.logprobs(slot, first, n)
    for p in range(first, first + n):
        if p in expected:
            err, bound = abs(float(log[p - first]) - expected[p]), float(lm.bound_device(expected[p]))
            WORST['steps'] = max(WORST['steps'], err / bound)
            assert np.isfinite(log[p - first]) and err <= bound, (slot, p, float(log[p - first]), expected[p])
        else:
            assert np.isnan(log[p - first]), (slot, p, float(log[p - first]))


def _verify_tree(ids, rm, words, limit, emitted, lg_rows, nk, expected):
    """the step's output against the host accept walk over its ARGMAX words; the kept rows' values join `expected`"""
    want, rows = lo.accept_scan_limited(ids.tolist(), _mask_matrix(rm), [int(w) for w in words], limit)
    assert list(emitted) == want, (emitted, want)
    dep = _depths(rm)
    vals = _model_rows(lg_rows[rows], [words[r] for r in rows])
    for i, r in enumerate(rows):
        assert dep[r] == i
        assert nk + i + 1 not in expected
        expected[nk + i + 1] = float(vals[i])
    siblings = [r for r in range(len(ids)) if r not in rows and dep[r] in [dep[q] for q in rows]]
    return len(rows), len(siblings)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_stage_inside_the_single_step(dtype):
    shape = tiny_shape()
    eng = LlamaVerifyEngine(shape, _sd(dtype), max_length=512)
    rs = np.random.RandomState(4)
    prompt = rs.randint(3, shape.vocab, size=70).tolist()                      # two prefill blocks
    # stage off (section 4): ordinary steps launch nothing of the stage and leave the log NaN; they also give the greedy continuation
    tok = eng.prefill(prompt, fast=False)
    cont = [tok]
    for _ in range(16):
        cont.append(eng.step(np.asarray(cont[-1:], dtype=np.int32), ONE)[0][0])
    assert eng.logprob_launches() == 0 and np.isnan(eng.logprobs(0, 0, 200)).all()
    eng.reset()
    eng.set_logprobs(True)
    assert eng.prefill(prompt, fast=False) == tok
    assert eng.logprob_launches() == 2
    expected = {70: float(_model_rows(eng.logits()[5:6], [tok])[0])}           # row (70 - 1) % 64 chooses the token at index 70
    _check_positions(eng, 0, expected, 70)
    at = 0                                                                     # cont[at] = the newest token of the sequence
    for step, (k, eager) in enumerate([(3, False), (2, True), (1, False)]):
        ids, rm = _planted_tree(cont[at], cont[at + 1:], k, 6, rs, shape.vocab)
        nk = eng.n_keys
        toks, n = eng.step(ids.copy(), rm.copy(), eager=eager)
        words = eng.state().cpu().numpy()[_lib.LA_ST_ARGMAX:_lib.LA_ST_ARGMAX + len(ids)]
        kept, sib = _verify_tree(ids, rm, words, 64, toks, eng.logits()[:len(ids)], nk, expected)
        assert kept == n and kept >= k + 1 and sib >= 1, (step, kept, sib)     # the planted chain was accepted; a dropped sibling shares a position
        _check_positions(eng, 0, expected, 70)
        at += len(toks)
        assert toks == cont[at - len(toks) + 1:at + 1], step
    # a forward-only step (mode 2) stores nothing
    before = eng.logprobs(0, 0, 300).tobytes()
    ids, rm = _planted_tree(cont[at], cont[at + 1:], 2, 6, rs, shape.vocab)
    eng.verify_only(ids, rm)
    assert eng.logprobs(0, 0, 300).tobytes() == before
    eng.set_logprobs(False)
    n = eng.logprob_launches()
    eng.commit([0])
    eng.step(np.asarray(cont[at + 1:at + 2], dtype=np.int32), ONE)
    assert eng.logprob_launches() == n and eng.logprobs(0, 0, 300).tobytes() == before      # off again: the stage is not launched
    print(f'single step {_name(dtype)}: worst err / bound so far {WORST["steps"]:.3e}')


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('multi', [False, True], ids=['bstep', 'mstep'])
def test_stage_inside_the_batch_steps(multi, dtype):
    """bstep: two slots at different cursors + one slot in prefill mode in ONE block; mstep: two blocks; bprefill / mprefill of a
    70-token prompt (slot 0) before them"""
    shape = tiny_shape()
    eng = LlamaVerifyEngine(shape, _sd(dtype), max_length=256, n_slots=3, max_blocks=2 if multi else 0)
    rs = np.random.RandomState(6 + multi)
    lens = [70, 22]
    prompts = {b: rs.randint(3, shape.vocab, size=lens[b]).tolist() for b in range(2)}
    late = rs.randint(3, shape.vocab, size=20).tolist()                        # slot 2's prompt: prefilled inside the tree step (bstep)
    prefill = eng.mprefill_many if multi else eng.bprefill_many

    def last_rows():
        """after the prefill: (logits buffer, {slot: row of the prompt's last token})"""
        if multi:            # pass 1 = slot 0's two pieces (blocks 0 and 1), pass 2 = slot 1's piece (block 0; block 1 is left as it was)
            return eng.mlogits(), {0: 64 + lens[0] - 64 - 1, 1: lens[1] - 1}
        base = eng.bstep_rows()                     # the second block: slot 0's last 6 rows, then slot 1's chain
        return eng.logits(), {0: base[0] + lens[0] - 64 - 1, 1: base[1] + lens[1] - 1}

    def one_token_steps(seqs, n):
        for _ in range(n):
            segs = [(b, np.asarray(seqs[b][-1:], dtype=np.int32), ONE, 0, 1) for b in range(2)]
            out = dict(zip(range(2), eng.mstep(segs))) if multi else eng.bstep(segs)
            for b in range(2):
                seqs[b].append(out[b][0])

    # stage off: the greedy continuations, nothing launched, the log stays NaN
    first = prefill(prompts)
    cont = {b: [first[b]] for b in range(2)}
    one_token_steps(cont, 10)
    assert eng.logprob_launches() == 0 and all(np.isnan(eng.logprobs(b, 0, 200)).all() for b in range(3))
    eng.reset_slot(-1)
    eng.set_logprobs(True)
    assert prefill(prompts) == first
    # the first generated token of every prompt whose last row is still readable
    lg, rows = last_rows()
    expected = {b: {} for b in range(3)}
    for b, r in rows.items():
        expected[b][lens[b]] = float(_model_rows(lg[r:r + 1], [first[b]])[0])
        _check_positions(eng, b, expected[b], lens[b])
    # one tree step: slot 0 and slot 1 at their own cursors (+ bstep: slot 2 as a prefill chain in the same block)
    segs = []
    for b, k in ((0, 3), (1, 1)):
        ids, rm = _planted_tree(cont[b][0], cont[b][1:], k, 6, rs, shape.vocab)
        segs.append((b, ids, rm, 0, 16))
    nk = list(eng.slot_keys)
    if multi:
        out = dict(zip(range(2), eng.mstep(segs)))
        lg, base = eng.mlogits(), {0: 0, 1: 64}
        am = eng.mout().cpu().numpy()[_lib.LA_MOUT_ARGMAX:]
    else:
        segs.append((2, np.asarray(late, dtype=np.int32), eng._CHAIN[:len(late)], 1, 1))
        out = eng.bstep(segs)
        lg, base = eng.logits(), eng.bstep_rows()
        am = eng.bstate().cpu().numpy()[_lib.LA_BST_ARGMAX:]
    for b, ids, rm, mode, limit in segs[:2]:
        T = len(ids)
        kept, sib = _verify_tree(ids, rm, am[base[b]:base[b] + T], limit, out[b], lg[base[b]:base[b] + T], nk[b], expected[b])
        assert kept >= 2 and sib >= 1, (b, kept, sib)
    if not multi:
        r = base[2] + len(late) - 1
        assert out[2] == [int(am[r])]
        expected[2][len(late)] = float(_model_rows(lg[r:r + 1], [am[r]])[0])
    for b in range(3):
        _check_positions(eng, b, expected[b], [lens[0], lens[1], len(late)][b])
    # forward only (mode 2): nothing stored
    before = [eng.logprobs(b, 0, 200).tobytes() for b in range(3)]
    segs2 = [(b, np.asarray(cont[b][:1], dtype=np.int32), ONE, 2, 1) for b in range(2)]
    if multi:
        eng.mstep(segs2)
    else:
        eng.bstep(segs2)
    assert [eng.logprobs(b, 0, 200).tobytes() for b in range(3)] == before
    eng.set_logprobs(False)
    print(f'{"mstep" if multi else "bstep"} {_name(dtype)}: worst err / bound so far {WORST["steps"]:.3e}')


# ------------------------------------------------------------------------------------------------ 3, 5, 6. the loops
# The decisive tiny model (the residual stream stays on the token embedding, so a position's logits do not depend on the tree and
# lookahead == no-draft holds token for token) with lm_head scaled by 1/8 (exact in both types): the top logit leads by ~2.4 instead
# of ~19, so the log-probabilities are values around -0.5, not zeros.
def _sd_decisive(dtype):
    sd = tiny_decisive_weights(0, dtype)
    sd['lm_head.weight'] = sd['lm_head.weight'] * 0.125
    return sd


def _warm_trie(rows):
    cache = LookaheadCache()
    for row in rows:
        cache.put([int(t) for t in row], branch_length=13, mode='output', idx=-1)
    return cache


def _lists():
    from transformers import (LogitsProcessorList, RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper, TopKLogitsWarper,
                              TopPLogitsWarper)
    return {'greedy': None, 'penalty': LogitsProcessorList([RepetitionPenaltyLogitsProcessor(1.3)]),
            'sampling': LogitsProcessorList([TemperatureLogitsWarper(0.8), TopKLogitsWarper(20), TopPLogitsWarper(0.9)])}


DK = {'use_lookahead': True, 'decoding_length': 64, 'branch_length': 12, 'stop_words': {}}
_MODELS = {}


def _model(dtype):
    if dtype not in _MODELS:
        _MODELS[dtype] = LlamaForCausalLM(tiny_shape(), _sd_decisive(dtype), max_length=512, eos_token_id=None)
    return _MODELS[dtype]


def _finite_nonpositive(lps, n):
    return len(lps) == n and all(np.isfinite(x) and x <= 0 for x in lps)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_native_loop_and_interpreter_loop_give_the_same_bits(dtype):
    model = _model(dtype)
    rs = np.random.RandomState(3)
    prompt = torch.tensor([rs.randint(3, model.engine.shape.vocab, size=50).tolist()])
    n_new = 48
    plain = model.greedy_search(prompt, 50 + n_new, eos_token_id=None)[0].tolist()
    runs = {}
    for native in (True, False):
        model.lookahead_cache = _warm_trie([plain[49:]])
        n0 = model.engine.logprob_launches()
        out = model.lookahead_generation(prompt, stopping_criteria=50 + n_new, eos_token_id=[None], return_dict_in_generate=True,
                                         decoding_kwargs=dict(DK, native_loop=native, output_logprobs=True))
        seq, lps = out.sequences[0].tolist(), out.kwargs['logprobs']
        assert _finite_nonpositive(lps, len(seq) - 50) and model.engine.logprob_launches() > n0 and not model.engine.logprobs_on
        assert np.mean(out.kwargs['edls'][1:]) > 2, out.kwargs['edls']         # drafts were accepted: several kept rows per step
        runs[native] = (seq, np.asarray(lps, dtype=np.float32).tobytes(), out.kwargs['edls'])
    assert runs[True] == runs[False]
    assert runs[True][0][:50 + n_new] == plain[:len(runs[True][0])][:50 + n_new]


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('which', ['greedy', 'penalty', 'sampling'])
def test_tokens_do_not_change_with_the_stage_on(which, dtype):
    model = _model(dtype)
    rs = np.random.RandomState(5)
    prompt = torch.tensor([rs.randint(3, model.engine.shape.vocab, size=40).tolist()])
    procs = _lists()[which]
    seqs = {}
    for on in (False, True):
        model.lookahead_cache = LookaheadCache()
        dk = dict(DK, do_sample=which == 'sampling', sample_seed=7)
        if on:
            dk['output_logprobs'] = True
        n0 = model.engine.logprob_launches()
        out = model.lookahead_generation(prompt, logits_processor=procs, stopping_criteria=40 + 24, eos_token_id=[None],
                                         return_dict_in_generate=True, decoding_kwargs=dk)
        seqs[on] = out.sequences[0].tolist()
        assert (model.engine.logprob_launches() > n0) == on
        if on:
            assert _finite_nonpositive(out.kwargs['logprobs'], len(seqs[on]) - 40)
        else:
            assert 'logprobs' not in out.kwargs
    assert seqs[True] == seqs[False]
    if which != 'greedy':
        assert (model.engine.penalty_launches() if which == 'penalty' else model.engine.sample_launches()) > 0


def _no_draft_bs1(eng, prompt, n_new):
    """the engine calls of greedy_search with the stage on -> (tokens, max |logit| of the row every token was chosen from)"""
    eng.reset()
    eng.set_logprobs(True)
    toks, peak = [eng.prefill(prompt)], [float(eng.logits()[(len(prompt) - 1) % 64].float().abs().max())]
    while len(toks) < n_new:
        toks.append(eng.step(np.asarray(toks[-1:], dtype=np.int32), ONE)[0][0])
        peak.append(float(eng.logits()[0].float().abs().max()))
    lps = eng.logprobs(0, len(prompt), n_new)
    eng.set_logprobs(False)
    return toks, peak, lps


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_front_doors_bs1(dtype):
    model = _model(dtype)
    eng = model.engine
    rs = np.random.RandomState(8)
    P, n_new = 45, 40
    prompt = torch.tensor([rs.randint(3, eng.shape.vocab, size=P).tolist()])
    toks, peak, lps0 = _no_draft_bs1(eng, prompt[0].tolist(), n_new)
    seq_g, lps_g = model.greedy_search(prompt, P + n_new, eos_token_id=None, output_logprobs=True)
    assert seq_g[0].tolist() == prompt[0].tolist() + toks
    assert np.asarray(lps_g, dtype=np.float32).tobytes() == lps0.tobytes()     # the no-draft comparator IS those engine calls
    model.lookahead_cache = _warm_trie([seq_g[0].tolist()[P - 1:]])
    ref = model.lookahead_generation(prompt, stopping_criteria=P + n_new, eos_token_id=[None], return_dict_in_generate=True,
                                     decoding_kwargs=dict(DK))
    for door in ('lookahead_generation', 'generate'):
        model.lookahead_cache = _warm_trie([seq_g[0].tolist()[P - 1:]])
        if door == 'generate':
            out = model.generate(prompt, max_new_tokens=n_new, return_dict_in_generate=True, decoding_kwargs=dict(DK, output_logprobs=True))
        else:
            out = model.lookahead_generation(prompt, stopping_criteria=P + n_new, eos_token_id=[None], return_dict_in_generate=True,
                                             decoding_kwargs=dict(DK, output_logprobs=True))
        seq, lps = out.sequences[0].tolist(), out.kwargs['logprobs']
        assert seq == ref.sequences[0].tolist() and seq[:P + n_new] == seq_g[0].tolist()[:len(seq)]
        assert _finite_nonpositive(lps, len(seq) - P) and np.mean(out.kwargs['edls'][1:]) > 2
        for i in range(min(len(lps), n_new)):
            d = abs(lps[i] - float(lps0[i]))
            WORST['doors'] = max(WORST['doors'], d)
            assert d <= 4 * TOL * peak[i], (door, i, lps[i], float(lps0[i]), peak[i])
    print(f'bs=1 {_name(dtype)}: worst |dlp| lookahead vs no-draft so far {WORST["doors"]:.3e} (bound >= {4 * TOL * min(peak):.3e})')


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('max_blocks', [0, 2], ids=['cursor', 'multiblock'])
def test_front_doors_batch_of_two_left_padded_prompts(max_blocks, dtype):
    """cursor: the whole batch shares one 64-row block (bstep).  multiblock: an engine with two blocks, one 64-row budget per sample and
    a trie with three wrong 11-token branches behind every position, so the two trees together pass 64 rows and the steps are
    mstep_async passes (counted)."""
    model = BatchLlama(tiny_shape(), _sd_decisive(dtype), max_length=512, max_batch=4, eos_token_id=None, max_blocks=max_blocks)
    eng = model.engine
    rs = np.random.RandomState(15)
    lens, n_new = [40, 20], 32                 # (every prompt is one chain of one prefill pass: every last row stays readable)
    P = max(lens)
    ids = np.zeros((2, P), dtype=np.int64)
    am = np.zeros((2, P), dtype=np.int64)
    for b, n in enumerate(lens):
        ids[b, P - n:] = rs.randint(3, eng.shape.vocab, size=n)
        am[b, P - n:] = 1
    t_ids, t_am = torch.from_numpy(ids), torch.from_numpy(am)
    # the no-draft run, call by call (the calls of greedy_search), for the max |logit| of every position
    prompts = {b: ids[b, P - lens[b]:].tolist() for b in range(2)}
    eng.reset_slot(-1)
    eng.set_logprobs(True)
    if max_blocks:                             # one pass: slot 0's chain in block 0, slot 1's in block 1
        first = eng.mprefill_many(prompts)
        lg, base = eng.mlogits(), {0: 0, 1: 64}
    else:
        first = eng.bprefill_many(prompts)
        lg, base = eng.logits(), eng.bstep_rows()
    toks = {b: [first[b]] for b in range(2)}
    peak = {b: [float(lg[base[b] + lens[b] - 1].float().abs().max())] for b in range(2)}
    while len(toks[0]) < n_new:
        out = eng.bstep([(b, np.asarray(toks[b][-1:], dtype=np.int32), ONE, 0, 1) for b in range(2)])
        lg, base = eng.logits(), eng.bstep_rows()
        for b in range(2):
            toks[b].append(out[b][0])
            peak[b].append(float(lg[base[b]].float().abs().max()))
    lps0 = [eng.logprobs(b, lens[b], n_new) for b in range(2)]
    eng.set_logprobs(False)
    seq_g, lps_g = model.greedy_search(t_ids, P + n_new, attention_mask=t_am, eos_token_id=None, output_logprobs=True)
    seq_g = seq_g.cpu().numpy()
    for b in range(2):
        assert seq_g[b, P:].tolist() == toks[b]
        assert np.asarray(lps_g[b], dtype=np.float32).tobytes() == lps0[b].tobytes()
    warm = [seq_g[b, P - 1:] for b in range(2)]
    extra = {}
    if max_blocks:
        extra = {'per_sample_budget': True}
        for b in range(2):
            for i in range(P, P + n_new):
                warm += [seq_g[b, i - 1:i + 1].tolist() + rs.randint(3, eng.shape.vocab, size=11).tolist() for _ in range(3)]
    passes = [0]
    if max_blocks:
        queue = eng.mstep_async

        def counted(group, **kw):
            passes[0] += 1
            return queue(group, **kw)
        eng.mstep_async = counted

    def run(door, on):
        model.lookahead_cache = _warm_trie(warm)
        dk = dict(DK, output_logprobs=True, **extra) if on else dict(DK, **extra)
        if door == 'generate':
            return model.generate(input_ids=t_ids, attention_mask=t_am, max_new_tokens=n_new, eos_token_id=[None], pad_token_id=0,
                                  return_dict_in_generate=True, decoding_kwargs=dk)
        return model.lookahead_generation(t_ids, stopping_criteria=P + n_new, eos_token_id=[None], pad_token_id=0,
                                          return_dict_in_generate=True, attention_mask=t_am, decoding_kwargs=dk)

    ref = run('lookahead_generation', False)
    assert 'logprobs' not in ref.kwargs
    for door in ('lookahead_generation', 'generate'):
        n0 = passes[0]
        out = run(door, True)
        got = out.sequences.cpu().numpy()
        assert got.tolist() == ref.sequences.cpu().numpy().tolist()
        w = min(got.shape[1], P + n_new)
        assert got[:, :w].tolist() == seq_g[:, :w].tolist()
        assert np.mean(out.kwargs['edls'][2:]) > 2
        assert (passes[0] > n0) == bool(max_blocks), (door, passes)            # multiblock: the steps were mstep_async passes
        for b in range(2):
            lps = out.kwargs['logprobs'][b]
            assert _finite_nonpositive(lps, got.shape[1] - P)
            for i in range(min(len(lps), n_new)):
                d = abs(lps[i] - float(lps0[b][i]))
                WORST['doors'] = max(WORST['doors'], d)
                assert d <= 4 * TOL * peak[b][i], (door, b, i, lps[i], float(lps0[b][i]), peak[b][i])
        assert not eng.logprobs_on
    print(f'batch {"multiblock" if max_blocks else "cursor"} {_name(dtype)}: worst |dlp| lookahead vs no-draft so far {WORST["doors"]:.3e}')


# ------------------------------------------------------------------------------------------------ 7. wide trees
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_wide_tree_pass_with_the_stage_on_is_refused(dtype):
    """a missing kernel is an error, not a silent fall-back: the multi-block step has no wide-tree form of the stage"""
    shape = tiny_shape()
    eng = LlamaVerifyEngine(shape, _sd(dtype), max_length=512, n_slots=1, max_blocks=2)
    rs = np.random.RandomState(1)
    eng.mprefill(0, rs.randint(3, shape.vocab, size=20).tolist())
    eng.set_logprobs(True)
    rmw = np.zeros((100, 2), dtype=np.uint64)
    ids = rs.randint(3, shape.vocab, size=100).astype(np.int32)
    anc = 0
    for r in range(100):
        anc |= 1 << r
        rmw[r, 0], rmw[r, 1] = anc & 0xFFFFFFFFFFFFFFFF, anc >> 64
    with pytest.raises(AssertionError):                                        # LA_E_ARG
        eng.tstep(ids, rmw, mode=0)
    assert 'log-probabilities' in _lib.last_error()
    eng.set_logprobs(False)
    eng.reset_slot(-1)
    eng.mprefill(0, rs.randint(3, shape.vocab, size=20).tolist())
    toks, _ = eng.tstep(ids, rmw, mode=0)                                      # off again: the wide pass runs
    assert len(toks) >= 1
