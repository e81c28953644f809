# -*- coding: utf-8 -*-
"""-m gpu: the repetition penalty as a stage of the device step (csrc/la_penalty.hip) — kernel arithmetic and the row stage against
torch / transformers bit for bit, the fused penalised step against verify_only + the host walk + commit bit for bit (single
sequence, cursor batch, multi-block), the loops on the device path against the host walk (device_processors=False) and against
the reference goldens, the fallbacks, and "off means off".

Every comparison of tokens, cursors and logits is exact.  The only tolerance is the near-tie clause of the reference goldens, taken
from tests/test_gpu_batch.py (TOL): a bf16 engine follows an fp32 reference run up to the first position where the fp32 oracle's
penalised top-2 gap is at most 2 * TOL * max|logit|."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import llama_oracle as lo
from painlessinferenceacceleration_amd import _lib
from painlessinferenceacceleration_amd._lib import check
from painlessinferenceacceleration_amd.llama_engine import LlamaShape, LlamaVerifyEngine, random_weights
from painlessinferenceacceleration_amd.lookahead_cache import LookaheadCache
from painlessinferenceacceleration_amd.modeling_llama import LlamaForCausalLM
from painlessinferenceacceleration_amd.modeling_llama_batch import LlamaForCausalLM as BatchLlama
from painlessinferenceacceleration_amd.pretrained_model import _parents_of
from tests.gpu_utils import DEV, ptr, random_tree, sp
from tests.test_gpu_batch import TOL
from tests.test_gpu_e2e import _bf16_sd
from tests.tiny_model import GOLDEN, tiny_shape, tiny_weights

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
ONE = np.array([1], dtype=np.uint64)


def _procs(p):
    from transformers import LogitsProcessorList, RepetitionPenaltyLogitsProcessor
    return LogitsProcessorList([RepetitionPenaltyLogitsProcessor(float(p))])


def _pen_word(p):
    return torch.tensor([p], dtype=torch.float32, device=DEV)


# ------------------------------------------------------------------------------------------------ 1. arithmetic, exhaustive
@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
def test_penalised_value_equals_torch_for_every_16_bit_pattern(dtype):
    """every finite pattern of the storage type x p in {1.05, 1.3, 2.0, 0.8, 1.0}: the kernel's penalised value == torch.where(x < 0,
    x * p, x / p) on a 16-bit tensor (the call transformers' processor makes), bit for bit"""
    lib = _lib.lib_for(dtype)
    x = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype).to(DEV)
    finite = torch.isfinite(x.float())
    assert int(finite.sum()) in (65536 - 2 * 128, 65536 - 2 * 1024)          # bf16: 7 mantissa bits of inf / nan; fp16: 10
    for p in (1.05, 1.3, 2.0, 0.8, 1.0):
        out, pw = torch.empty_like(x), _pen_word(p)
        check(lib.la_penalty_transform(sp(), ptr(x), x.numel(), ptr(pw), ptr(out)), 'penalty_transform')
        torch.cuda.synchronize()
        ref = torch.where(x < 0, x * p, x / p)
        bad = (out.view(torch.int16) != ref.view(torch.int16)) & finite
        cpu = torch.where(x.cpu() < 0, x.cpu() * p, x.cpu() / p)
        print(f'[{dtype}] p={p}: kernel != torch(device) on {int(bad.sum())} finite patterns; torch(device) != torch(cpu) on '
              f'{int(((cpu.view(torch.int16) != ref.cpu().view(torch.int16)) & finite.cpu()).sum())}')
        assert int(bad.sum()) == 0, (p, x[bad][:8], out[bad][:8], ref[bad][:8])


# ------------------------------------------------------------------------------------------------ 2. row stage against HF
def _bitmap(tokens, vocab):
    bits = np.zeros(vocab // 32, dtype=np.uint32)
    t = np.unique(np.asarray(tokens, dtype=np.int64))
    np.bitwise_or.at(bits, t >> 5, (np.uint32(1) << (t & 31).astype(np.uint32)))
    return bits


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
@pytest.mark.parametrize('V', [512, 32000, 152064])
def test_row_stage_equals_hf_processor_argmax_on_every_row(V, dtype):
    lib = _lib.lib_for(dtype)
    rs = np.random.RandomState(V % 1000)
    T = 64
    checked = tie_rows = 0
    for case, density in enumerate([0.0, 1.0, 0.02, 0.4, 0.1]):
        p = [1.3, 1.05, 2.0, 0.8, 1.3][case]
        procs = _procs(p)
        if density == 0.0:
            ctx = np.zeros(0, dtype=np.int64)
        elif density == 1.0:
            ctx = np.arange(V, dtype=np.int64)
        else:
            ctx = np.nonzero(rs.rand(V) < density)[0].astype(np.int64)
        member = np.zeros(V, dtype=bool)
        member[ctx] = True
        _, rows = random_tree(rs, T)
        ids = rs.randint(0, V, size=T).astype(np.int32)
        lg = torch.from_numpy(rs.standard_normal((T, V)).astype(np.float32) * 2).to(dtype)
        if case == 2:
            lg = lg - 30                                    # an all-negative case: members are MULTIPLIED
        # planted ties, row by row: a run of equal values above the noise straddling members and non-members; and a penalised
        # member landing exactly on a non-member's value, the non-member at a lower index (even rows) or a higher one (odd rows)
        for r in range(T):
            path = [int(ids[a]) for a in range(T) if (int(rows[r]) >> a) & 1]
            mem_r = member.copy()
            mem_r[path] = True
            mem_idx, non_idx = np.nonzero(mem_r)[0], np.nonzero(~mem_r)[0]
            top = torch.tensor(9.0 if case != 2 else -9.0).to(dtype)
            if r % 4 < 2 and len(non_idx) >= 3:
                run = rs.choice(non_idx, 3, replace=False).tolist() + (rs.choice(mem_idx, 2).tolist() if len(mem_idx) else [])
                for t in run:
                    lg[r, t] = top
                tie_rows += 1
            elif len(mem_idx) and len(non_idx):
                m = int(mem_idx[rs.randint(len(mem_idx))])
                raw = torch.tensor(12.0 if case != 2 else -7.0).to(dtype)
                pen = torch.where(raw < 0, raw * p, raw / p)            # the member's value after the penalty, in the storage type
                cand = non_idx[non_idx < m] if r % 2 == 0 else non_idx[non_idx > m]
                if len(cand) == 0:
                    cand = non_idx
                n = int(cand[rs.randint(len(cand))])
                lg[r, m] = raw
                lg[r, n] = pen
                lg[r, int(path[0])] = torch.maximum(lg[r, int(path[0])], top)      # and a member on the row's own path near the top
                tie_rows += 1
        lg = lg.to(DEV).contiguous()
        d_bits = torch.from_numpy(_bitmap(ctx, V).view(np.int32)).to(DEV)
        d_ids = torch.from_numpy(ids).to(DEV)
        d_rm = torch.from_numpy(np.asarray(rows, dtype=np.uint64).view(np.int64)).to(DEV)
        out, pw = torch.full((T,), -1, dtype=torch.int32, device=DEV), _pen_word(p)
        check(lib.la_penalty_argmax(sp(), ptr(lg), V, T, ptr(d_bits), ptr(d_ids), ptr(d_rm), ptr(pw), ptr(out)), 'penalty_argmax')
        torch.cuda.synchronize()
        got = out.cpu().tolist()
        ctx_dev = torch.from_numpy(ctx).to(DEV)
        for r in range(T):
            path = [int(ids[a]) for a in range(T) if (int(rows[r]) >> a) & 1]
            full = torch.cat([ctx_dev, torch.tensor(path, dtype=torch.long, device=DEV)])[None]
            want = int(procs(full, lg[r][None].clone()).argmax(-1)[0])
            assert got[r] == want, (V, dtype, case, r, got[r], want)
            checked += 1
    assert checked == 5 * T and tie_rows > 3 * T


# ------------------------------------------------------------------------------------------------ helpers of the step / loop tests
def _chain_tree(rs, root, chain, vocab, max_rows=64):
    """DFS-ordered tree: root, then the chain tokens one below the other, every chain node with a random leaf sibling before or
    after it -> (ids int32[T], rowmask uint64[T])"""
    ids, masks = [int(root)], [1]
    parent_row = 0
    for tok in chain:
        if len(ids) + 2 > max_rows:
            break
        first_leaf = rs.rand() < 0.5
        order = ['leaf', 'chain'] if first_leaf else ['chain']
        chain_row = None
        for kind in order:
            r = len(ids)
            ids.append(int(rs.randint(3, vocab)) if kind == 'leaf' else int(tok))
            masks.append(masks[parent_row] | (1 << r))
            if kind == 'chain':
                chain_row = r
        parent_row = chain_row
    return np.asarray(ids, dtype=np.int32), np.asarray(masks, dtype=np.uint64)


def _host_step(eng, seq, ids, rowmask, procs):
    """engine B: verify_only + the host walk of pretrained_model._lookahead_generation + commit -> emitted tokens"""
    T = len(ids)
    eng.verify_only(ids, rowmask)
    parent = _parents_of(rowmask, T)
    cur, live, rows, toks = 0, {0}, [0], []
    while True:
        ctx = torch.tensor([seq + toks], dtype=torch.long, device=eng.device)
        t = int(torch.argmax(procs(ctx, eng.logits()[cur][None].clone()), dim=-1)[0])
        toks.append(t)
        nxt = [j for j in range(1, T) if parent[j] in live and int(ids[j]) == t]
        if not nxt:
            break
        cur, live = nxt[0], set(nxt)
        rows.append(cur)
    eng.commit(rows)
    return toks


def _context_tokens(eng, slot=0):
    words = eng.penalty_context(slot).cpu().numpy().view(np.uint32)
    return {32 * w + b for w in np.nonzero(words)[0] for b in range(32) if (int(words[w]) >> b) & 1}


class Spy(object):
    """counts the forward-only (mode 2) steps an engine is asked for: verify_only, and the mode word of bstep / mstep / tstep"""

    def __init__(self, monkeypatch, eng):
        self.mode2 = 0
        self.fused = 0

        def wrap(name, modes_of):
            if not hasattr(eng, name):
                return
            inner = getattr(eng, name)

            def f(*a, **k):
                for md in modes_of(*a, **k):
                    if md == 2:
                        self.mode2 += 1
                    else:
                        self.fused += 1
                return inner(*a, **k)
            monkeypatch.setattr(eng, name, f)
        wrap('verify_only', lambda *a, **k: [2])
        wrap('step_async', lambda ids, rowmask, mode=0, eager=False: [] if mode == 2 else [mode])      # verify_only counted above
        wrap('decode_native', lambda *a, **k: [0])
        wrap('bstep', lambda segments, eager=False: [sg[3] for sg in segments])
        wrap('mstep_async', lambda blocks, eager=False: [b[3] for b in blocks])
        wrap('mstep_trees', lambda trees, eager=False: [t[3] for t in trees])
        wrap('tstep', lambda ids, rowmask, slot=0, mode=0, limit=None, eager=False: [mode])


# ------------------------------------------------------------------------------------------------ 3. step equivalence, bit-exact
@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
def test_fused_penalised_step_equals_verify_only_host_walk_commit(dtype):
    p = 1.3
    procs = _procs(p)
    shape = tiny_shape()
    sd = {k: v.to(dtype) for k, v in tiny_weights(0, torch.float32).items()}
    rs = np.random.RandomState(5)
    prompt = rs.randint(3, shape.vocab, size=90).tolist()               # two prefill blocks
    # a scout run on the host path tells which continuation the trees should carry to be accepted several tokens deep
    scout = LlamaForCausalLM(shape, dict(sd), max_length=512, eos_token_id=None)
    truth = scout.greedy_search(torch.tensor([prompt]), 90 + 80, eos_token_id=None, logits_processor=procs,
                                device_processors=False)[0].tolist()
    del scout
    A = LlamaVerifyEngine(shape, dict(sd), max_length=512)
    B = LlamaVerifyEngine(shape, dict(sd), max_length=512)
    A.set_repetition_penalty(p)
    launches0 = A.penalty_launches()
    tok_a = A.prefill(prompt)
    B.prefill(prompt, fast=False)
    ctx = torch.tensor([prompt], dtype=torch.long, device=DEV)
    tok_b = int(torch.argmax(procs(ctx, B.logits()[(len(prompt) - 1) % 64][None].clone()), dim=-1)[0])
    assert tok_a == tok_b == truth[90]
    assert _context_tokens(A) == set(prompt) | {tok_a}
    seq = prompt + [tok_a]
    deep = 0
    for step in range(8):
        if step % 2 == 0:
            ids, rm = _chain_tree(rs, seq[-1], truth[len(seq):len(seq) + 12], shape.vocab)
        else:
            T = int(rs.randint(2, 64))
            _, rm = random_tree(rs, T)
            ids = np.concatenate([[seq[-1]], rs.randint(3, shape.vocab, size=T - 1)]).astype(np.int32)
        eager = step == 5
        toks_a, n_a = A.step(ids.copy(), rm.copy(), eager=eager)
        toks_b = _host_step(B, seq, ids, rm, procs)
        assert toks_a == toks_b, (step, toks_a, toks_b)
        assert A.n_keys == B.n_keys and n_a == len(toks_b)
        assert torch.equal(A.logits()[:len(ids)], B.logits()[:len(ids)])
        seq += toks_a
        assert _context_tokens(A) == set(seq), step
        deep = max(deep, len(toks_a))
    print('deepest accept:', deep)
    assert deep >= 3, deep                                                 # trees were accepted several tokens deep
    assert A.penalty_launches() - launches0 == 2 + 8                       # two prefill blocks + eight steps ran the stage
    # one further plain step: identical KV caches
    A.set_repetition_penalty(1.0)
    nxt = np.asarray(seq[-1:], dtype=np.int32)
    ta, _ = A.step(nxt, ONE)
    tb, _ = B.step(nxt, ONE)
    assert ta == tb and torch.equal(A.logits()[:1], B.logits()[:1])
    assert A.penalty_launches() - launches0 == 10                          # off again: the stage is not launched


def _padded(prompts, pad=0):
    P = max(len(p) for p in prompts)
    ids = np.full((len(prompts), P), pad, dtype=np.int64)
    am = np.zeros((len(prompts), P), dtype=np.int64)
    for b, p in enumerate(prompts):
        ids[b, P - len(p):] = p
        am[b, P - len(p):] = 1
    return ids, am


@pytest.mark.parametrize('multi', [False, True], ids=['bstep-2-slots', 'mstep-3-blocks'])
def test_fused_penalised_batch_step_equals_mode2_host_walk_commit(multi):
    """cursor batch with two slots sharing a 64-row block (one prompt left-padded) / multi-block step with three blocks: engine A
    runs the fused penalised step, engine B the forward-only step + the existing batch host walk (_sequential_walk) + b/mcommit"""
    p = 1.3
    procs = _procs(p)
    shape = tiny_shape()
    sd = _bf16_sd()
    rs = np.random.RandomState(9 + multi)
    B_ = 3 if multi else 2
    lens = [30, 22, 27][:B_]
    prompts = [rs.randint(3, shape.vocab, size=n).tolist() for n in lens]
    ids0, am = _padded(prompts)
    scout = BatchLlama(shape, dict(sd), max_length=256, max_batch=B_, eos_token_id=None, max_blocks=B_ if multi else 0)
    truth = scout.greedy_search(torch.from_numpy(ids0), ids0.shape[1] + 60, attention_mask=torch.from_numpy(am), eos_token_id=None,
                                logits_processor=procs, device_processors=False).cpu().numpy()
    del scout
    mk = dict(max_length=256, n_slots=B_, max_blocks=B_ if multi else 0)
    A = LlamaVerifyEngine(shape, dict(sd), **mk)
    Bh = LlamaVerifyEngine(shape, dict(sd), **mk)
    A.set_repetition_penalty(p)
    rows = [ids0[b].tolist() for b in range(B_)]                     # padded-coordinate rows: what the walk hands the processor
    for b in range(B_):
        A.seed_penalty_context(b, rows[b])
    pd = {b: prompts[b] for b in range(B_)}
    if multi:
        first_a = A.mprefill_many(pd)
        Bh.mprefill_many(pd)
        lg = Bh.mlogits()
        base = {b: 64 * b for b in range(B_)}                          # one block per prompt (all shorter than 64 tokens)
    else:
        first_a = A.bprefill_many(pd)
        Bh.bprefill_many(pd)
        lg, base = Bh.logits(), Bh.bstep_rows()

    def pick(ctx_ids, row):
        ctx = torch.tensor([ctx_ids], dtype=torch.long, device=DEV)
        return int(torch.argmax(procs(ctx, row[None].clone()), dim=-1)[0])

    for b in range(B_):
        assert first_a[b] == pick(rows[b], lg[base[b] + lens[b] - 1]), b
        rows[b].append(first_a[b])
        assert _context_tokens(A, b) == set(rows[b]), b                # pads included
    deep = 0
    for step in range(6):
        segs = []
        for b in range(B_):
            if multi:
                room = 64
            else:
                room = 64 // B_
            if (step + b) % 2 == 0:
                chain = truth[b, len(rows[b]):len(rows[b]) + 8].tolist()
                ids, rm = _chain_tree(rs, rows[b][-1], chain, shape.vocab, max_rows=room)
            else:
                T = int(rs.randint(1, room + 1))
                _, rm = random_tree(rs, T)
                ids = np.concatenate([[rows[b][-1]], rs.randint(3, shape.vocab, size=T - 1)]).astype(np.int32)
            segs.append((b, ids, np.asarray(rm, dtype=np.uint64)))
        limit = 16
        if multi:
            out_a = dict(zip(range(B_), A.mstep([(b, i, r, 0, limit) for b, i, r in segs])))
            Bh.mstep([(b, i, r, 2, limit) for b, i, r in segs])
            lg, base = Bh.mlogits(), {b: 64 * b for b in range(B_)}
            assert torch.equal(lg[:64 * B_], A.mlogits()[:64 * B_])
        else:
            out_a = A.bstep([(b, i, r, 0, limit) for b, i, r in segs])
            Bh.bstep([(b, i, r, 2, limit) for b, i, r in segs])
            lg, base = Bh.logits(), Bh.bstep_rows()
            assert torch.equal(lg, A.logits())
        kept = {}
        for b, ids, rm in segs:
            toks, keep_rows = BatchLlama._sequential_walk(rows[b], (b, ids, rm, 2, limit), lg, base[b], pick)
            assert out_a[b] == toks, (multi, step, b, out_a[b], toks)
            kept[b] = keep_rows
            rows[b] += toks
            deep = max(deep, len(toks))
        if multi:
            Bh.mcommit([kept[b] for b in range(B_)])
        else:
            Bh.bcommit(kept)
        assert A.slot_keys == Bh.slot_keys, (multi, step)
        for b in range(B_):
            assert _context_tokens(A, b) == set(rows[b]), (step, b)
    assert deep >= 3, deep
    A.set_repetition_penalty(1.0)
    nxt = [(b, np.asarray(rows[b][-1:], dtype=np.int32), ONE, 0, 1) for b in range(B_)]
    if multi:
        a, c = A.mstep(nxt), Bh.mstep(nxt)
        assert a == c and torch.equal(A.mlogits()[:64 * B_:64], Bh.mlogits()[:64 * B_:64])
    else:
        a, c = A.bstep(nxt), Bh.bstep(nxt)
        assert a == c and torch.equal(A.logits()[:B_], Bh.logits()[:B_])


def test_wide_tree_pass_with_the_penalty_on_is_refused():
    """a missing kernel is an error, not a silent fall-back: the multi-block step has no wide-tree form of the stage"""
    shape = tiny_shape()
    eng = LlamaVerifyEngine(shape, _bf16_sd(), max_length=512, n_slots=1, max_blocks=2)
    rs = np.random.RandomState(1)
    eng.mprefill(0, rs.randint(3, shape.vocab, size=20).tolist())
    eng.set_repetition_penalty(1.3)
    rmw = np.zeros((100, 2), dtype=np.uint64)
    ids = rs.randint(3, shape.vocab, size=100).astype(np.int32)
    anc = [1]
    for r in range(1, 100):
        anc.append(anc[r - 1] | (1 << r))                               # a 100-row chain: rows 64.. have ancestors in block 0
    for r in range(100):
        rmw[r, 0] = anc[r] & 0xFFFFFFFFFFFFFFFF
        rmw[r, 1] = anc[r] >> 64
    with pytest.raises(AssertionError):
        eng.tstep(ids, rmw, mode=0)
    eng.set_repetition_penalty(1.0)
    eng.reset_slot(-1)
    eng.mprefill(0, rs.randint(3, shape.vocab, size=20).tolist())
    toks, _ = eng.tstep(ids, rmw, mode=0)                               # off again: the wide pass runs
    assert len(toks) >= 1


# ------------------------------------------------------------------------------------------------ 4. loop equivalence
def _decisive_model(max_blocks=0, decisive=True):
    shape = tiny_shape()
    sd = random_weights(shape, seed=2, device='cpu', decisive=True) if decisive else _bf16_sd()
    return shape, LlamaForCausalLM(shape, sd, max_length=512, eos_token_id=None, max_blocks=max_blocks)


@pytest.mark.parametrize('p,decisive', [(1.05, True), (1.3, True), (1.3, False)], ids=['1.05-decisive', '1.3-decisive', '1.3-tiny'])
def test_loop_on_the_device_path_equals_the_host_walk_bs1(monkeypatch, p, decisive):
    """decisive weights: long accepts, and lookahead == plain decoding holds token for token; the plain tiny model: the penalty
    changes many tokens (a random LM loops), device path == host walk still holds exactly"""
    shape, model = _decisive_model(decisive=decisive)
    procs = _procs(p)
    rs = np.random.RandomState(3)
    prompt = torch.tensor([rs.randint(3, shape.vocab, size=50).tolist()])
    n_new = 150
    spy = Spy(monkeypatch, model.engine)
    plain_dev = model.greedy_search(prompt, 50 + n_new, eos_token_id=None, logits_processor=procs)[0].tolist()
    assert spy.mode2 == 0 and spy.fused > 0
    plain_host = model.greedy_search(prompt, 50 + n_new, eos_token_id=None, logits_processor=procs, device_processors=False)[0].tolist()
    assert spy.mode2 > 0
    assert plain_dev == plain_host
    free = model.greedy_search(prompt, 50 + n_new, eos_token_id=None)[0].tolist()
    print(f'p={p}: tokens changed by the penalty: {sum(a != b for a, b in zip(plain_dev, free))} of {n_new}')
    if not decisive:
        assert plain_dev != free                                          # the penalty does act on this model
    for mode in ('hier', 'par', 'one'):
        for native in (True, False):
            runs = {}
            for dev in (True, False):
                model.lookahead_cache = LookaheadCache()
                outs = []
                for rep in range(2):                                      # the second request finds a warm trie: long accepts
                    dk = {'use_lookahead': True, 'decoding_mode': mode, 'decoding_length': 64, 'branch_length': 12, 'stop_words': {},
                          'native_loop': native, 'device_processors': dev}
                    before = spy.mode2
                    out = model.lookahead_generation(prompt, logits_processor=procs, stopping_criteria=50 + n_new, eos_token_id=[None],
                                                     return_dict_in_generate=True, decoding_kwargs=dk)
                    if dev:
                        assert spy.mode2 == before, (mode, native)        # never a forward-only step: no silent fall-back
                    else:
                        assert spy.mode2 > before
                    outs.append((out.sequences[0].tolist(), out.kwargs['dls'], out.kwargs['edls']))
                runs[dev] = outs
                assert model.engine.repetition_penalty == 1.0
            for rep in range(2):
                assert runs[True][rep] == runs[False][rep], (mode, native, rep)
                seq = runs[True][rep][0]
                if decisive:
                    assert seq[:50 + n_new] == plain_dev[:len(seq)][:50 + n_new], (mode, native, rep)
            if decisive and mode == 'hier':
                assert np.mean(runs[True][1][2][1:]) > 2, runs[True][1][2]


@pytest.mark.parametrize('bs', [2, 3])
@pytest.mark.parametrize('multi', [False, True], ids=['default-budget', 'per-sample-budget'])
def test_loop_on_the_device_path_equals_the_host_walk_batch(monkeypatch, bs, multi):
    p = 1.05
    procs = _procs(p)
    shape = tiny_shape()
    sd = random_weights(shape, seed=2, device='cpu', decisive=True)
    model = BatchLlama(shape, dict(sd), max_length=512, max_batch=4, eos_token_id=None, max_blocks=4 if multi else 0)
    rs = np.random.RandomState(13 + bs)
    lens = [60, 47, 31][:bs]
    ids, am = _padded([rs.randint(3, shape.vocab, size=n).tolist() for n in lens])
    P, n_new = ids.shape[1], 100
    t_ids, t_am = torch.from_numpy(ids), torch.from_numpy(am)
    spy = Spy(monkeypatch, model.engine)
    plain_dev = model.greedy_search(t_ids, P + n_new, attention_mask=t_am, eos_token_id=None, logits_processor=procs).cpu().numpy()
    assert spy.mode2 == 0 and spy.fused > 0
    plain_host = model.greedy_search(t_ids, P + n_new, attention_mask=t_am, eos_token_id=None, logits_processor=procs,
                                     device_processors=False).cpu().numpy()
    assert spy.mode2 > 0 and plain_dev.tolist() == plain_host.tolist()
    runs = {}
    for dev in (True, False):
        model.lookahead_cache = LookaheadCache()
        outs = []
        for rep in range(2):
            dk = {'use_lookahead': True, 'decoding_length': 64, 'branch_length': 12, 'stop_words': {}, 'per_sample_budget': multi,
                  'device_processors': dev}
            before = spy.mode2
            out = model.lookahead_generation(t_ids, logits_processor=procs, stopping_criteria=P + n_new, eos_token_id=[None],
                                             pad_token_id=0, return_dict_in_generate=True, attention_mask=t_am, decoding_kwargs=dk)
            assert (spy.mode2 == before) if dev else (spy.mode2 > before)
            outs.append((out.sequences.cpu().numpy().tolist(), out.kwargs['dls'], out.kwargs['edls']))
        runs[dev] = outs
        assert model.engine.repetition_penalty == 1.0
    for rep in range(2):
        assert runs[True][rep] == runs[False][rep], rep
        got = np.asarray(runs[True][rep][0])
        w = min(got.shape[1], plain_dev.shape[1], P + n_new)
        assert got[:, :w].tolist() == plain_dev[:, :w].tolist(), rep
    assert np.mean(runs[True][1][2][bs:]) > 1.5


# ------------------------------------------------------------------------------------------------ 5. reference goldens
def test_device_path_vs_reference_golden_bs1(monkeypatch):
    """tests/golden/llama_tiny_fp32_rep.npz (penalty 1.3, recorded from the reference in fp32) through the device path of a bf16
    engine: the clause of test_gpu_batch.py::test_batch_processor_run_vs_reference_golden, with its TOL"""
    g = np.load(os.path.join(GOLDEN, 'llama_tiny_fp32_rep.npz'))
    shape = tiny_shape()
    model = LlamaForCausalLM(shape, _bf16_sd(), max_length=256)
    oracle = lo.OracleLlama(shape, tiny_weights(0, torch.float32))
    procs = _procs(float(g['penalty']))
    prompt = g['prompt'].tolist()
    spy = Spy(monkeypatch, model.engine)
    whole = 0
    for r in range(2):
        dk = {'use_lookahead': True, 'decoding_mode': 'hier', 'decoding_length': 64, 'branch_length': 12, 'max_query_length': 2,
              'stop_words': {}}
        out = model.lookahead_generation(torch.tensor([prompt]), logits_processor=procs, stopping_criteria=len(prompt) + 64,
                                         eos_token_id=2, return_dict_in_generate=True, decoding_kwargs=dk)
        assert spy.mode2 == 0
        ref, got = g[f'r{r}_sequences'].tolist(), out.sequences[0].tolist()
        if got == ref:
            assert out.kwargs['dls'] == g[f'r{r}_dls'].tolist() and out.kwargs['edls'] == g[f'r{r}_edls'].tolist()
            whole += 1
            continue
        w = min(len(got), len(ref))
        assert got[:w] != ref[:w], 'one run is a strict prefix of the other'
        i = next(k for k in range(w) if got[k] != ref[k])
        ctx = ref[:i]
        lg, _ = oracle.forward(torch.tensor(ctx), torch.tril(torch.ones((len(ctx), len(ctx)), dtype=torch.long)), None)
        sc = procs(torch.tensor([ctx]), lg[-1:].float().clone())[0]
        top = torch.topk(sc, 2).values
        assert float(top[0] - top[1]) <= 2 * TOL * float(lg[-1].float().abs().max()), (r, i)
        break                                  # the trie of the second request depends on the first one's tokens
    print('bs=1 processor requests identical to the reference run end to end:', whole, 'of 2')


def test_device_path_vs_reference_golden_batch(monkeypatch):
    g = np.load(os.path.join(GOLDEN, 'llama_tiny_batch_fp32_rep.npz'))
    shape, sd = tiny_shape(), _bf16_sd()
    oracle = lo.OracleLlama(shape, tiny_weights(0, torch.float32))
    procs = _procs(float(g['penalty']))
    whole = 0
    for name in ('b2', 'b3pad'):
        bs, dl, max_new = [int(x) for x in g[f'{name}_cfg']]
        model = BatchLlama(shape, dict(sd), max_length=256, max_batch=4, max_blocks=0)
        spy = Spy(monkeypatch, model.engine)
        ids, am = torch.from_numpy(g[f'{name}_ids']), torch.from_numpy(g[f'{name}_am'])
        P = ids.shape[1]
        dk = {'use_lookahead': True, 'decoding_mode': 'hier', 'decoding_length': dl, 'branch_length': 12, 'stop_words': {}}
        out = model.lookahead_generation(ids, logits_processor=procs, stopping_criteria=P + max_new, eos_token_id=2, pad_token_id=0,
                                         return_dict_in_generate=True, attention_mask=am, decoding_kwargs=dk)
        assert spy.mode2 == 0 and spy.fused > 0, name
        ref, got = g[f'{name}_r0_sequences'], out.sequences.cpu().numpy()
        if got.shape == ref.shape and bool((got == ref).all()):
            assert out.kwargs['dls'] == g[f'{name}_r0_dls'].tolist() and out.kwargs['edls'] == g[f'{name}_r0_edls'].tolist()
            whole += 1
            continue
        for b in range(bs):
            w = min(got.shape[1], ref.shape[1])
            diff = np.nonzero(got[b, :w] != ref[b, :w])[0]
            if len(diff) == 0:
                continue
            i = int(diff[0])
            ctx = [int(t) for t, m in zip(ref[b, :P], am[b]) if m] + ref[b, P:i].tolist()
            lg, _ = oracle.forward(torch.tensor(ctx), torch.tril(torch.ones((len(ctx), len(ctx)), dtype=torch.long)), None)
            sc = procs(torch.from_numpy(ref[b:b + 1, :i]), lg[-1:].float().clone())[0]
            top = torch.topk(sc, 2).values
            assert float(top[0] - top[1]) <= 2 * TOL * float(lg[-1].float().abs().max()), (name, b, i)
    print('batch processor cases identical to the reference run end to end on the device path:', whole, 'of 2')


# ------------------------------------------------------------------------------------------------ 6. fallbacks
def test_everything_else_keeps_the_host_walk(monkeypatch):
    from transformers import (LogitsProcessorList, NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor, StoppingCriteria,
                              StoppingCriteriaList, MaxLengthCriteria)

    class Sub(RepetitionPenaltyLogitsProcessor):
        pass

    shape, model = _decisive_model(max_blocks=2)
    eng = model.engine
    rs = np.random.RandomState(4)
    prompt = torch.tensor([rs.randint(3, shape.vocab, size=50).tolist()])
    spy = Spy(monkeypatch, eng)
    launches0 = eng.penalty_launches()

    def run(procs, dev, **extra):
        dk = {'use_lookahead': True, 'decoding_length': extra.pop('decoding_length', 64), 'branch_length': 12, 'stop_words': {},
              'device_processors': dev, 'do_sample': extra.pop('do_sample', False)}
        model.lookahead_cache = LookaheadCache()
        torch.manual_seed(0)
        out = model.lookahead_generation(prompt, logits_processor=procs, stopping_criteria=50 + 60, eos_token_id=[None],
                                         return_dict_in_generate=True, decoding_kwargs=dk, **extra)
        return out

    cases = [
        ('two processors', LogitsProcessorList([RepetitionPenaltyLogitsProcessor(1.3), NoRepeatNGramLogitsProcessor(3)]), {}),
        ('subclass', LogitsProcessorList([Sub(1.3)]), {}),
        ('do_sample', _procs(1.3), {'do_sample': True}),
        ('output_scores', _procs(1.3), {'output_scores': True}),
        ('wide tree', _procs(1.3), {'decoding_length': 128}),
    ]
    for name, procs, extra in cases:
        before = spy.mode2
        a = run(procs, True, **dict(extra))
        assert spy.mode2 > before, name                                   # the host walk ran
        b = run(procs, False, **dict(extra))
        assert a.sequences.tolist() == b.sequences.tolist() and a.kwargs['dls'] == b.kwargs['dls'] and a.kwargs['edls'] == b.kwargs['edls'], name
        if name == 'output_scores':
            assert len(a.scores) == len(b.scores) and all(torch.equal(x, y) for x, y in zip(a.scores, b.scores))
        assert eng.repetition_penalty == 1.0
    assert eng.penalty_launches() == launches0                            # none of them touched the device stage

    # the penalty is cleared after a request that raised
    class Boom(StoppingCriteria):
        def __call__(self, input_ids, scores, **kw):
            if input_ids.shape[1] > 70:
                raise RuntimeError('boom')
            return False

    crit = StoppingCriteriaList([MaxLengthCriteria(50 + 60), Boom()])
    with pytest.raises(RuntimeError, match='boom'):
        model.lookahead_generation(prompt, logits_processor=_procs(1.3), stopping_criteria=crit, eos_token_id=[None],
                                   return_dict_in_generate=True,
                                   decoding_kwargs={'use_lookahead': True, 'decoding_length': 64, 'branch_length': 12, 'stop_words': {}})
    assert eng.penalty_launches() > launches0                             # that request did run on the device stage ...
    assert eng.repetition_penalty == 1.0                                  # ... and left it switched off
    n = eng.penalty_launches()
    model.lookahead_cache = LookaheadCache()
    model.lookahead_generation(prompt, stopping_criteria=50 + 30, eos_token_id=[None],
                               decoding_kwargs={'use_lookahead': True, 'decoding_length': 64, 'branch_length': 12, 'stop_words': {}})
    assert eng.penalty_launches() == n


def test_batch_request_with_wide_trees_keeps_the_host_walk(monkeypatch):
    """the b3pad256 case of the batch golden (decoding_length 256 on a 4-block engine: a sample's tree may span several blocks): the
    whole request takes the host walk and gives what it gives with device_processors=False"""
    g = np.load(os.path.join(GOLDEN, 'llama_tiny_batch_fp32_rep.npz'))
    shape, sd = tiny_shape(), _bf16_sd()
    procs = _procs(float(g['penalty']))
    bs, dl, max_new = [int(x) for x in g['b3pad256_cfg']]
    ids, am = torch.from_numpy(g['b3pad256_ids']), torch.from_numpy(g['b3pad256_am'])
    outs = []
    for dev in (True, False):
        model = BatchLlama(shape, dict(sd), max_length=256, max_batch=4, max_blocks=4)
        spy = Spy(monkeypatch, model.engine)
        dk = {'use_lookahead': True, 'decoding_mode': 'hier', 'decoding_length': dl, 'branch_length': 12, 'stop_words': {},
              'device_processors': dev}
        out = model.lookahead_generation(ids, logits_processor=procs, stopping_criteria=ids.shape[1] + max_new, eos_token_id=2,
                                         pad_token_id=0, return_dict_in_generate=True, attention_mask=am, decoding_kwargs=dk)
        assert spy.mode2 > 0 and model.engine.penalty_launches() == 0
        outs.append((out.sequences.tolist(), out.kwargs['dls'], out.kwargs['edls']))
    assert outs[0] == outs[1]


@pytest.mark.parametrize('stage', ['penalty', 'sampling'])
@pytest.mark.parametrize('batch', [False, True], ids=['bs1', 'batch-of-2'])
def test_request_that_raises_leaves_no_stage_behind(batch, stage):
    """a request with the penalty / sampling stage on is ended by a raising StoppingCriteria after its first step (lookahead loop and
    plain loop): the next request on the same model, with no processor, emits exactly what a fresh model emits and launches no stage"""
    from transformers import (LogitsProcessorList, MaxLengthCriteria, RepetitionPenaltyLogitsProcessor, StoppingCriteria,
                              StoppingCriteriaList, TemperatureLogitsWarper, TopKLogitsWarper)

    class Boom(StoppingCriteria):
        def __call__(self, input_ids, scores, **kw):
            raise RuntimeError('boom')

    shape, sd = tiny_shape(), _bf16_sd()
    rs = np.random.RandomState(21)
    n_new = 8
    if batch:
        ids_np, am_np = _padded([rs.randint(3, shape.vocab, size=n).tolist() for n in (17, 11)])
        ids, extra = torch.from_numpy(ids_np), {'attention_mask': torch.from_numpy(am_np)}

        def make():
            return BatchLlama(shape, dict(sd), max_length=256, max_batch=2, eos_token_id=None, max_blocks=0)
    else:
        ids, extra = torch.tensor([rs.randint(3, shape.vocab, size=17).tolist()]), {}

        def make():
            return LlamaForCausalLM(shape, dict(sd), max_length=256, eos_token_id=None)
    P = ids.shape[1]
    sampling = stage == 'sampling'
    procs = LogitsProcessorList([RepetitionPenaltyLogitsProcessor(1.3)] + ([TemperatureLogitsWarper(0.8), TopKLogitsWarper(20)] if sampling else []))
    dk = {'use_lookahead': True, 'decoding_length': 64, 'branch_length': 12, 'stop_words': {}}

    def plain(model):
        model.lookahead_cache = LookaheadCache()
        la = model.lookahead_generation(ids, stopping_criteria=P + n_new, eos_token_id=[None], pad_token_id=0, decoding_kwargs=dict(dk), **extra)
        return la.tolist(), model.greedy_search(ids, P + n_new, eos_token_id=None, **extra).tolist()

    want = plain(make())
    model = make()
    eng = model.engine
    launches = eng.sample_launches if sampling else eng.penalty_launches
    crit = StoppingCriteriaList([MaxLengthCriteria(P + n_new), Boom()])
    for entry in ('lookahead', 'plain'):
        n0 = launches()
        with pytest.raises(RuntimeError, match='boom'):
            if entry == 'lookahead':
                model.lookahead_generation(ids, logits_processor=procs, stopping_criteria=crit, eos_token_id=[None], pad_token_id=0,
                                           decoding_kwargs=dict(dk, do_sample=sampling, **({'sample_seed': 7} if sampling else {})), **extra)
            else:
                model.greedy_search(ids, P + n_new, eos_token_id=None, logits_processor=procs, do_sample=sampling, stopping_criteria=crit,
                                    sample_seed=7 if sampling else None, **extra)
        assert launches() > n0, entry                                     # the request did run on the device stage ...
        assert eng.repetition_penalty == 1.0 and not getattr(eng, 'sampling', False), entry      # ... and left it switched off
        counts = (eng.penalty_launches(), eng.sample_launches())
        assert plain(model) == want, entry
        assert (eng.penalty_launches(), eng.sample_launches()) == counts, entry


# ------------------------------------------------------------------------------------------------ 7. off means off
def test_without_a_processor_the_stage_is_never_launched():
    shape, model = _decisive_model()
    rs = np.random.RandomState(6)
    prompt = torch.tensor([rs.randint(3, shape.vocab, size=50).tolist()])
    dk = {'use_lookahead': True, 'decoding_length': 64, 'branch_length': 12, 'stop_words': {}}
    for native in (True, False):
        model.lookahead_generation(prompt, stopping_criteria=50 + 100, eos_token_id=[None], decoding_kwargs=dict(dk, native_loop=native))
    model.greedy_search(prompt, 50 + 20, eos_token_id=None)
    assert model.engine.penalty_launches() == 0 and model.engine.repetition_penalty == 1.0
    bm = BatchLlama(shape, random_weights(shape, seed=2, device='cpu', decisive=True), max_length=512, max_batch=2, eos_token_id=None)
    ids = torch.from_numpy(rs.randint(3, shape.vocab, size=(2, 40)).astype(np.int64))
    bm.lookahead_generation(ids, stopping_criteria=40 + 40, eos_token_id=[None], pad_token_id=0, decoding_kwargs=dict(dk))
    assert bm.engine.penalty_launches() == 0


# ------------------------------------------------------------------------------------------------ 8. full size
def test_full_size_llama7b_penalty_on_the_device_path(monkeypatch):
    """32-layer Llama-2-7B shape, decisive random init, penalty 1.05, 64 new tokens: lookahead on the device path == plain decoding
    with the penalty, and drafts are still accepted (mean edls > 2, the bound of test_sequential_processor_path_on_device)"""
    shape = LlamaShape.llama2_7b()
    model = LlamaForCausalLM.random_init(shape, seed=0, max_length=512, decisive=True, eos_token_id=None)
    procs = _procs(1.05)
    rs = np.random.RandomState(2)
    prompt = torch.tensor([rs.randint(3, 32000, size=96).tolist()])
    n_new = 64
    spy = Spy(monkeypatch, model.engine)
    plain = model.greedy_search(prompt, 96 + n_new, eos_token_id=None, logits_processor=procs)[0].tolist()
    dk = {'use_lookahead': True, 'decoding_length': 64, 'branch_length': 12, 'stop_words': {}}
    model.lookahead_cache = LookaheadCache()
    for rep in range(2):
        out = model.lookahead_generation(prompt, logits_processor=procs, stopping_criteria=96 + n_new, eos_token_id=[None],
                                         return_dict_in_generate=True, decoding_kwargs=dict(dk))
        seq = out.sequences[0].tolist()
        assert seq[:96 + n_new] == plain[:len(seq)][:96 + n_new], rep
    assert spy.mode2 == 0 and model.engine.penalty_launches() > 0
    assert np.mean(out.kwargs['edls'][1:]) > 2, out.kwargs['edls']
