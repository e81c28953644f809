# -*- coding: utf-8 -*-
"""Every step form of the engine (step / bstep / mstep / mstep_trie / decode_native / profile / the wide-tree pass; captured and
eager; the long-context graph) under every combination of the three row stages (repetition penalty, sampling, log-probabilities),
pinned bit for bit: tests/golden/step_form_digests.json holds, for each case and after each of three seeded steps with planted
trees (built as tests/test_gpu_logprobs.py builds them), the emitted tokens, a sha256 of the header words the form publishes, the
ARGMAX words and a sha256 of the logits of the live rows, sha256 of every active slot's penalty bitmap and log-probability log, and
the three launch counters (as increments since the case's prefill began).

The fixture was recorded (record_all() below) on an MI355X from the commit BEFORE the step driver of csrc/la_engine.cpp was
reorganised (one row-stage tail, one step-graph cache), twice in separate processes, the second with the allocator's memory
pre-filled with a non-zero byte: every digest agreed, so no case reads memory it did not write and none had to be narrowed further
than the live rows the digests cover from the start.  The module uses the Python API of that commit only, so it runs unchanged
there.  The plans depend on the CU count, which the fixture stores: on another device the tests fail rather than skip."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from painlessinferenceacceleration_amd import _lib
from painlessinferenceacceleration_amd.device_trie import DeviceTrie
from painlessinferenceacceleration_amd.llama_engine import LlamaShape, LlamaVerifyEngine, random_weights
from painlessinferenceacceleration_amd.lookahead_cache import LookaheadCache
from tests.test_gpu_attn_census import _split_partials_tail
from tests.test_gpu_logprobs import _planted_tree
from tests.tiny_model import TINY_MOE, moe_shape, moe_weights, tiny_shape, tiny_weights

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'step_form_digests.json')
ONE = np.array([1], dtype=np.uint64)
PENALTY, SEED, TEMPERATURE, TOP_K, TOP_P = 1.3, 7, 0.8, 20, 0.9
STAGES = {'off': (), 'pen': ('pen',), 'samp': ('samp',), 'pen_samp': ('pen', 'samp'), 'lp': ('lp',), 'all': ('pen', 'samp', 'lp')}
LENS = [70, 22, 20]                # prompt lengths of slots 0, 1, 2 (slot 0: two prefill blocks)
N_CONT = 40                        # tokens of the no-draft continuation the trees are planted from
KS = (3, 2, 1)                     # planted depth of the three steps


def _sha(t):
    if torch.is_tensor(t):
        t = t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy()
    return hashlib.sha256(np.ascontiguousarray(t).tobytes()).hexdigest()


def set_stages(eng, names):
    eng.set_repetition_penalty(PENALTY if 'pen' in names else 1.0)
    eng.set_sampling('samp' in names, seed=SEED, temperature=TEMPERATURE, top_k=TOP_K, top_p=TOP_P)
    eng.set_logprobs('lp' in names)


def _counters(eng):
    return [eng.penalty_launches(), eng.sample_launches(), eng.logprob_launches()]


def _common(eng, slots, base):
    return {'pen': [_sha(eng.penalty_context(s)) for s in slots], 'lp': [_sha(eng.logprobs(s, 0, eng.max_keys)) for s in slots],
            'counters': [a - b for a, b in zip(_counters(eng), base)]}


def _single_digest(eng, T, base):
    st = eng.state().cpu().numpy()
    d = {'hdr': _sha(st[:_lib.LA_ST_OUTTOK + 64]), 'argmax': st[_lib.LA_ST_ARGMAX:_lib.LA_ST_ARGMAX + T].tolist(), 'logits': _sha(eng.logits()[:T])}
    d.update(_common(eng, [0], base))
    return d


def _batch_digest(eng, rows, slots, base):
    st = eng.bstate().cpu().numpy()
    d = {'hdr': _sha(st[:_lib.LA_BST_DST]), 'argmax': st[_lib.LA_BST_ARGMAX:_lib.LA_BST_ARGMAX + rows].tolist(), 'logits': _sha(eng.logits()[:rows])}
    d.update(_common(eng, slots, base))
    return d


def _mblock_digest(eng, Ts, slots, base):
    st, lg = eng.mout().cpu().numpy(), eng.mlogits()
    live = [r for b, T in enumerate(Ts) for r in range(64 * b, 64 * b + T)]
    d = {'hdr': _sha(st[:_lib.LA_MOUT_DST]), 'argmax': [int(st[_lib.LA_MOUT_ARGMAX + r]) for r in live],
         'logits': _sha(lg[torch.tensor(live, device=lg.device)])}
    d.update(_common(eng, sorted(set(slots)), base))
    return d


def _prompts(eng, n, seed):
    rs = np.random.RandomState(seed)
    return {b: rs.randint(3, eng.shape.vocab, size=LENS[b]).tolist() for b in range(n)}


# ------------------------------------------------------------------------------------------------ the forms
# Every run_* takes an engine whose stages are set, finds the no-draft continuation of its prompts under those stages with one-token
# steps of the same form (the planted chains are then accepted whatever the stages pick), resets the engine, and records the prefill
# and three tree steps.
def run_single(eng, eager=False, prompt_len=LENS[0], hooks=None, seed=11, split_evidence=False):
    """split_evidence (fresh engines only): whether the key-split attention has written its partials yet joins the digest"""
    rs = np.random.RandomState(seed)
    prompt = rs.randint(3, eng.shape.vocab, size=prompt_len).tolist()
    cont = [eng.prefill(prompt, fast=False, eager=eager)]
    while len(cont) < N_CONT:
        cont.append(eng.step(np.asarray(cont[-1:], dtype=np.int32), ONE, eager=eager)[0][0])
    eng.reset()
    base = _counters(eng)
    out = [{'first': eng.prefill(prompt, fast=False, eager=eager)}]
    at, last = 0, out[0]['first']
    for i, k in enumerate(KS):
        if hooks and i in hooks:
            hooks[i]()
        ids, rm = _planted_tree(last, cont[at + 1:], k, 6, rs, eng.shape.vocab)
        toks, n = eng.step(ids.copy(), rm.copy(), eager=eager)
        d = {'toks': toks, 'n': n}
        d.update(_single_digest(eng, len(ids), base))
        if split_evidence:
            d['split_partials'] = bool(_split_partials_tail(eng).abs().max() > 0)
        out.append(d)
        at, last = at + len(toks), toks[-1]
    return out


def _run_slots(eng, n_active, multi, eager, seed):
    prompts = _prompts(eng, n_active, seed)
    rs = np.random.RandomState(seed + 1)
    slots = list(range(n_active))
    prefill = eng.mprefill_many if multi else eng.bprefill_many

    def launch(segs):
        if multi:
            return dict(zip(slots, eng.mstep(segs, eager=eager)))
        return eng.bstep(segs, eager=eager)

    first = prefill(prompts, eager=eager)
    cont = {b: [first[b]] for b in slots}
    while len(cont[0]) < N_CONT:
        got = launch([(b, np.asarray(cont[b][-1:], dtype=np.int32), ONE, 0, 1) for b in slots])
        for b in slots:
            cont[b].append(got[b][0])
    eng.reset()
    return prompts, rs, slots, prefill, launch, cont


def run_slots(eng, n_active, multi, eager=False, seed=21):
    """bstep (one shared block) or mstep (one block per slot) over n_active slots"""
    prompts, rs, slots, prefill, launch, cont = _run_slots(eng, n_active, multi, eager, seed)
    base = _counters(eng)
    first = prefill(prompts, eager=eager)
    out = [{'first': [first[b] for b in slots]}]
    at, last = {b: 0 for b in slots}, dict(first)
    for i in range(len(KS)):
        segs = []
        for b in slots:
            ids, rm = _planted_tree(last[b], cont[b][at[b] + 1:], KS[(i + b) % len(KS)], 6, rs, eng.shape.vocab)
            segs.append((b, ids, rm, 0, 16))
        got = launch(segs)
        d = {'toks': [got[b] for b in slots]}
        if multi:
            d.update(_mblock_digest(eng, [len(s[1]) for s in segs], slots, base))
        else:
            d.update(_batch_digest(eng, sum(len(s[1]) for s in segs), slots, base))
        out.append(d)
        for b in slots:
            at[b], last[b] = at[b] + len(got[b]), got[b][-1]
    return out


def run_trie(eng, seed=31):
    """mstep_trie: two slots, the drafts taken on the device from a trie that holds both continuations"""
    prompts, rs, slots, prefill, launch, cont = _run_slots(eng, 2, True, False, seed)
    cache = LookaheadCache()
    for b in slots:
        cache.put([prompts[b][-1]] + cont[b], branch_length=13, mode='output', idx=-1)
    dt = DeviceTrie(cache, idxs=slots)
    base = _counters(eng)
    first = prefill(prompts)
    out = [{'first': [first[b] for b in slots]}]
    seqs = {b: [prompts[b][-1], first[b]] for b in slots}
    for _ in range(len(KS)):
        with torch.cuda.stream(eng.stream):
            dt.hier_get_dev([seqs[b][-2:] for b in slots], idxs=slots, decoding_length=64, branch_length=12, min_input_size=0,
                            min_output_size=32, mode='mix')
            toks, Ts = eng.mstep_trie(dt, 0, slots, [16] * len(slots), [seqs[b][-1] for b in slots])
        d = {'toks': toks, 'Ts': Ts}
        d.update(_mblock_digest(eng, Ts, slots, base))
        out.append(d)
        for b in slots:
            seqs[b] += toks[b]
    return out


def run_native(eng, seed=41):
    """la_lookahead_decode for a dozen tokens over a trie that holds the continuation"""
    rs = np.random.RandomState(seed)
    prompt = rs.randint(3, eng.shape.vocab, size=LENS[0]).tolist()
    cont = [eng.prefill(prompt, fast=False)]
    while len(cont) < N_CONT:
        cont.append(eng.step(np.asarray(cont[-1:], dtype=np.int32), ONE)[0][0])
    eng.reset()
    base = _counters(eng)
    cache = LookaheadCache()
    cache.put(prompt[-1:] + cont, branch_length=13, mode='output', idx=-1)
    first = eng.prefill(prompt, fast=False)
    new, dls, edls, _, _, fin = eng.decode_native(cache, prompt + [first], len(prompt) + 1 + 12, decoding_length=16, branch_length=4)
    d = {'first': first, 'toks': new, 'dls': dls, 'edls': edls, 'finished': fin}
    d.update(_single_digest(eng, dls[-1], base))
    return [d]


def run_profile(eng, seed=51):
    rs = np.random.RandomState(seed)
    prompt = rs.randint(3, eng.shape.vocab, size=LENS[0]).tolist()
    base = _counters(eng)
    first = eng.prefill(prompt, fast=False)
    ids, rm = _planted_tree(first, rs.randint(3, eng.shape.vocab, size=8).tolist(), 2, 6, rs, eng.shape.vocab)
    launches = eng.profile(ids.copy(), rm.copy(), iters=2)['launches']
    d = {'first': first, 'launches': launches}
    d.update(_single_digest(eng, len(ids), base))
    return [d]


def _wide_tree(vocab, seed=61):
    rs = np.random.RandomState(seed)
    rmw = np.zeros((100, 2), dtype=np.uint64)
    anc = 0
    for r in range(100):
        anc |= 1 << r
        rmw[r, 0], rmw[r, 1] = anc & 0xFFFFFFFFFFFFFFFF, anc >> 64
    return rs.randint(3, vocab, size=20).tolist(), rs.randint(3, vocab, size=100).astype(np.int32), rmw


def run_wide(eng):
    """stages off: one 100-row pass through tstep"""
    prompt, ids, rmw = _wide_tree(eng.shape.vocab)
    base = _counters(eng)
    first = eng.mprefill(0, prompt)
    toks, n = eng.tstep(ids, rmw, mode=0)
    d = {'first': first, 'toks': toks, 'n': n}
    d.update(_mblock_digest(eng, [64, 36], [0, 0], base))
    return [d]


def run_wide_refusal(eng):
    """a stage on: the pass is refused -> the error text"""
    prompt, ids, rmw = _wide_tree(eng.shape.vocab)
    eng.mprefill(0, prompt)
    with pytest.raises(AssertionError):
        eng.tstep(ids, rmw, mode=0)
    # the engine's own library: _lib.last_error() joins the texts every loaded build (fp16, lab) still holds from earlier tests
    return [{'error': eng._lib.la_last_error().decode('utf-8', 'replace'), 'counters': _counters(eng)}]


# ------------------------------------------------------------------------------------------------ the shapes
def _tiny_sd(dtype=torch.bfloat16):
    return {k: v.to(dtype) for k, v in tiny_weights(0, torch.float32).items()}


def _hd64():
    return LlamaShape(1, 256, 4, 2, 512, 512, 1e-5, head_dim=64, qkv_bias=True)


def _llama7b_layer():
    return LlamaShape(1, 4096, 32, 32, 11008, 32000)


def _tiny(**kw):
    return LlamaVerifyEngine(tiny_shape(), _tiny_sd(), **kw)


def _run_epoch(eng):
    """the capture epoch changes in the middle of the sequence: step 2 runs the first layer only (la_debug_set key 13), step 3 all again"""
    try:
        return run_single(eng, hooks={1: lambda: _lib.debug_set(13, 1), 2: lambda: _lib.debug_set(13, 0)})
    finally:
        _lib.debug_set(13, 0)


# form -> (engine factory, runner): one fresh engine per case
TINY_FORMS = {
    'step': (lambda: _tiny(max_length=512), lambda e: run_single(e, split_evidence=True)),
    'step_eager': (lambda: _tiny(max_length=512), lambda e: run_single(e, eager=True)),
    # 2 kv heads: the key-split graph from 5468 - 64 committed keys on; the prompt ends past that point
    'step_long': (lambda: _tiny(max_length=5800), lambda e: run_single(e, prompt_len=5440, split_evidence=True)),
    'step_epoch': (lambda: _tiny(max_length=512), _run_epoch),
    'bstep1': (lambda: _tiny(max_length=256, n_slots=3), lambda e: run_slots(e, 1, False)),
    'bstep1_eager': (lambda: _tiny(max_length=256, n_slots=3), lambda e: run_slots(e, 1, False, eager=True)),
    'bstep3': (lambda: _tiny(max_length=256, n_slots=3), lambda e: run_slots(e, 3, False)),
    'bstep3_eager': (lambda: _tiny(max_length=256, n_slots=3), lambda e: run_slots(e, 3, False, eager=True)),
    'mstep1': (lambda: _tiny(max_length=256, n_slots=2, max_blocks=2), lambda e: run_slots(e, 1, True)),
    'mstep1_eager': (lambda: _tiny(max_length=256, n_slots=2, max_blocks=2), lambda e: run_slots(e, 1, True, eager=True)),
    'mstep2': (lambda: _tiny(max_length=256, n_slots=2, max_blocks=2), lambda e: run_slots(e, 2, True)),
    'mstep2_eager': (lambda: _tiny(max_length=256, n_slots=2, max_blocks=2), lambda e: run_slots(e, 2, True, eager=True)),
    'mstep_trie': (lambda: _tiny(max_length=256, n_slots=2, max_blocks=2), run_trie),
    'decode_native': (lambda: _tiny(max_length=512), run_native),
    'profile': (lambda: _tiny(max_length=512), run_profile),
}


def _moe():
    return LlamaVerifyEngine(moe_shape(TINY_MOE), moe_weights(TINY_MOE, 3, torch.bfloat16), max_length=256, n_slots=2, max_blocks=2)


def _fp8():
    return LlamaVerifyEngine(_hd64(), random_weights(_hd64(), 2, device='cpu', dtype=torch.bfloat16), max_length=512, weight_format='fp8')


_ENGINE_7B = {}


def _llama7b(dtype):
    """ONE engine per dtype for all cases of the 7B layer (0.9 GB of weights)"""
    if dtype not in _ENGINE_7B:
        _ENGINE_7B.clear()
        torch.cuda.empty_cache()
        sd = random_weights(_llama7b_layer(), 5, device='cpu', dtype=dtype)
        _ENGINE_7B[dtype] = LlamaVerifyEngine(_llama7b_layer(), sd, max_length=256, n_slots=3)
    return _ENGINE_7B[dtype]


CASES = {}          # name -> (engine factory, stage names, runner)
for _form, (_make, _run) in TINY_FORMS.items():
    for _st in STAGES:
        CASES[f'tiny/{_form}/{_st}'] = (_make, _st, _run)
CASES['tiny/wide/off'] = (lambda: _tiny(max_length=512, n_slots=1, max_blocks=2), 'off', run_wide)
for _st in ('pen', 'samp', 'lp', 'all'):
    CASES[f'tiny/wide/{_st}'] = (lambda: _tiny(max_length=512, n_slots=1, max_blocks=2), _st, run_wide_refusal)
for _st in ('off', 'lp'):
    CASES[f'moe/step/{_st}'] = (_moe, _st, run_single)
    CASES[f'moe/mstep1/{_st}'] = (_moe, _st, lambda e: run_slots(e, 1, True))
    CASES[f'moe/mstep2/{_st}'] = (_moe, _st, lambda e: run_slots(e, 2, True))
for _st in ('off', 'all'):
    CASES[f'hd64_gqa_bias_fp8/step/{_st}'] = (_fp8, _st, run_single)
    CASES[f'hd64_gqa_bias_fp8/step_eager/{_st}'] = (_fp8, _st, lambda e: run_single(e, eager=True))
# the balanced lm_head (la_rowplan has a plan from this shape on): the fused tail, with the log-probability launch between tail and commit
for _dt, _dn in ((torch.bfloat16, 'bf16'), (torch.float16, 'fp16')):
    for _st in ('off', 'lp', 'all'):
        CASES[f'llama7b_layer_{_dn}/step/{_st}'] = (lambda d=_dt: _llama7b(d), _st, run_single)
        CASES[f'llama7b_layer_{_dn}/step_eager/{_st}'] = (lambda d=_dt: _llama7b(d), _st, lambda e: run_single(e, eager=True))
        CASES[f'llama7b_layer_{_dn}/bstep3/{_st}'] = (lambda d=_dt: _llama7b(d), _st, lambda e: run_slots(e, 3, False))


def run_on(eng, st, run):
    """one case on an engine, fresh or used: from a reset, with the stages of `st` on, all of them off again afterwards"""
    eng.reset()
    set_stages(eng, STAGES[st])
    try:
        return run(eng)
    finally:
        set_stages(eng, ())


def run_case(name):
    make, st, run = CASES[name]
    return run_on(make(), st, run)


def record_all():
    """the fixture's content, from whatever tree this runs in"""
    cases = {name: run_case(name) for name in CASES}
    return {'cu_count': int(torch.cuda.get_device_properties(0).multi_processor_count),
            'balanced_wg': {'tiny': [int(x) for x in _tiny(max_length=128).balanced_wg],
                            'llama7b_layer': [int(x) for x in _llama7b(torch.float16).balanced_wg]},
            'cases': cases}


@pytest.fixture(scope='module')
def golden():
    with open(FIXTURE) as f:
        g = json.load(f)
    assert sorted(g['cases']) == sorted(CASES)
    return g


def _same(got, want, what):
    got = json.loads(json.dumps(got))
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (what, i, {k: (a.get(k), b.get(k)) for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)})


def test_device_is_the_one_the_fixture_was_recorded_on(golden):
    assert torch.cuda.get_device_properties(0).multi_processor_count == golden['cu_count'], \
        'the GEMM plans deal rows out per CU: the digests hold for the recorded CU count only'


@pytest.mark.parametrize('name', list(CASES))
def test_step_form_matches_the_recorded_digests(golden, name):
    assert torch.cuda.get_device_properties(0).multi_processor_count == golden['cu_count']
    _same(run_case(name), golden['cases'][name], name)


def test_the_recorded_cases_are_what_they_were_chosen_for(golden):
    c = golden['cases']
    # no plan at the tiny shape (no fused tail, no balanced launches), all three at the 7B layer
    assert golden['balanced_wg']['tiny'] == [0, 0, 0] and all(golden['balanced_wg']['llama7b_layer'])
    for name, steps in c.items():
        form, st = name.split('/')[1:]
        if form == 'wide' and st != 'off':
            continue
        want = [int('pen' in STAGES[st]), int('samp' in STAGES[st]), int('lp' in STAGES[st])]
        last = steps[-1]['counters']
        assert [int(x > 0) for x in last] == want, (name, last)
        if form != 'profile':                          # (a profiled step counts its log-probability launch only)
            assert len(set(x for x in last if x)) <= 1, (name, last)
        if form not in ('decode_native', 'profile', 'wide', 'mstep_trie'):
            assert all(len(s['argmax']) >= 13 for s in steps[1:]), name                 # 13-row planted trees
    assert c['tiny/profile/all'][0]['counters'] == [2, 2, 4]                            # two prefill steps, two profiled ones
    # drafts were accepted; the sampled / penalised picks differ from the greedy ones; the epoch change and the stage show
    assert all(s['n'] >= 2 for s in c['tiny/step/off'][1:]) and all(s['n'] >= 2 for s in c['tiny/step/all'][1:])
    assert c['tiny/step/off'] != c['tiny/step/samp']
    # the engine's own evidence of the attention form: no split partials below the threshold, partials past it
    for st in STAGES:
        assert not any(s['split_partials'] for s in c[f'tiny/step/{st}'][1:]) and all(s['split_partials'] for s in c[f'tiny/step_long/{st}'][1:])
        assert len(c[f'tiny/decode_native/{st}'][0]['dls']) >= 2 and len(c[f'tiny/decode_native/{st}'][0]['toks']) >= 12
    assert {k: v for k, v in c['tiny/step/off'][1].items() if k != 'split_partials'} == c['tiny/step_epoch/off'][1] and c['tiny/step/off'][2]['logits'] != c['tiny/step_epoch/off'][2]['logits']
    assert c['tiny/step/off'][1]['lp'] != c['tiny/step/lp'][1]['lp'] and c['tiny/step/off'][1]['pen'] != c['tiny/step/pen'][1]['pen']
    assert 'sampling' in c['tiny/wide/samp'][0]['error'] and 'sampling' in c['tiny/wide/all'][0]['error']
    assert 'log-probabilities' in c['tiny/wide/lp'][0]['error'] and 'repetition penalty' in c['tiny/wide/pen'][0]['error']


@pytest.mark.parametrize('form', ['step', 'bstep3'])
def test_switching_the_stages_recaptures(golden, form):
    """ONE engine through off, all, off, all: every segment gives what a fresh engine in that state gives (the fixture's digests).
    Not the multi-block forms: their header digest covers the whole LA_MOUT_* block up to DST, and the OUTTOK words past a block's
    NOUT keep what an earlier pass left there (no reset clears them), so on a used engine it differs from a fresh one's — on the
    commit the fixture was recorded from as well (mstep2: 'hdr' alone differed, every other digest agreed)."""
    make, _, run = CASES[f'tiny/{form}/off']
    eng = make()
    for st in ('off', 'all', 'off', 'all'):
        _same(run_on(eng, st, run), golden['cases'][f'tiny/{form}/{st}'], (form, st))


@pytest.mark.parametrize('st', ['off', 'all'])
def test_new_pinned_blocks_recapture(golden, st):
    """other staging blocks handed to step in the middle of a sequence: captured again over them, the same results"""
    eng = _tiny(max_length=512)
    kept = []

    def swap():
        kept.append((eng.host_in, eng.host_out, eng.host_bin, eng.host_bout))      # the old blocks stay allocated
        old = eng.host_in.data_ptr()
        eng._alloc_host_blocks()
        assert eng.host_in.data_ptr() != old
    _same(run_on(eng, st, lambda e: run_single(e, hooks={1: swap}, split_evidence=True)), golden['cases'][f'tiny/step/{st}'], st)
