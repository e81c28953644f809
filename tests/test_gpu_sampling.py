# -*- coding: utf-8 -*-
"""GPU: sampling on the device (csrc/la_sample.hip) against the numpy fp64 model of tests/sampling_model.py.

Margins (derived, not fitted):
  DELTA = 1e-4   the top-p threshold key k* of the kernel must satisfy, in fp64, M_>(k*) < top_p + DELTA and M_>=(k*) >= top_p - DELTA.
                 The kernel's fixed-point mass accumulation is exact; what is left is fp32 expf and z rounding, ~1e-6 relative.
  GAP = 1e-3     rows whose fp64 top-1 / top-2 gap of z + g is below GAP are left out of the token comparison (the fp32 error of
                 x / T + g at |score| <~ 100 is ~1e-5); at most 1 % of the rows of a case may be left out (asserted).
The top-k threshold key is compared exactly, always."""
import ctypes as C

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
from tests import sampling_model as sm
from tests.gpu_utils import DEV, ptr, random_tree, sp
from tests.tiny_model import tiny_decisive_weights, tiny_shape, tiny_weights

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
DELTA, GAP = 1e-4, 1e-3
ONE = np.array([1], dtype=np.uint64)
SLACK = {'worst': -1.0}          # worst observed top-p slack over the session: max(M_> - top_p, top_p - M_>=), <= 0 when fp64 agrees
                                 # outright (printed; recorded in profiles/device_sampling.json)


def _bits_dev(lib, seed, stream, position, vocab):
    out = torch.zeros(vocab, dtype=torch.int32, device=DEV)
    check(lib.la_sample_bits(sp(), C.c_uint64(seed), stream, position, vocab, ptr(out)), 'sample_bits')
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. the Philox words
@pytest.mark.parametrize('V', [512, 152064])
def test_sample_bits_equal_the_model_word_for_word(V):
    lib = _lib.lib
    seen = []
    for seed in (7, 0xDEADBEEFCAFEF00D):
        for position in (1, 4097):
            for stream in (0, 5):
                got = _bits_dev(lib, seed, stream, position, V)
                assert (got == sm.sample_bits(seed, stream, position, V)).all(), (seed, position, stream)
                seen.append(got)
    for i in range(len(seen)):
        for j in range(i):
            assert (seen[i] != seen[j]).mean() > 0.99               # another seed, position or stream: other words


# ------------------------------------------------------------------------------------------------ 2. the row stage
def _bitmap(tokens, vocab):
    bits = np.zeros(vocab // 32, dtype=np.uint32)
    t = np.unique(np.asarray(tokens, dtype=np.int64))
    np.bitwise_or.at(bits, t >> 5, (np.uint32(1) << (t & 31).astype(np.uint32)))
    return bits


def _unique_max(lg):
    """one more storage step on the first maximum of every row whose maximum is tied: top_k = 1 then has one survivor"""
    bits = lg.view(torch.int16)
    for r in range(lg.shape[0]):
        mx = lg[r].max()
        idx = torch.nonzero(lg[r] == mx)[:, 0]
        if len(idx) > 1:
            assert float(mx) > 0
            bits[r, idx[0]] += 1
    return lg


_REF = {}


def _reference(V, dtype):
    """logits N(0, 2) in the storage type, positions, tree, context — and the Philox words of every row — once per (V, dtype)"""
    key = (V, dtype)
    if key not in _REF:
        rs = np.random.RandomState(V % 997 + (1 if dtype == torch.float16 else 0))
        T = 64
        lg = _unique_max(torch.from_numpy(rs.standard_normal((T, V)).astype(np.float32) * 2).to(dtype))
        pos = rs.randint(0, 5000, size=T).astype(np.int32)
        seed, stream = 0x1234567887654321, 3
        words = np.stack([sm.sample_bits(seed, stream, int(p) + 1, V) for p in pos])
        _, rowmask = random_tree(rs, T)
        ids = rs.randint(0, V, size=T).astype(np.int32)
        ctx = np.nonzero(rs.rand(V) < 0.05)[0]
        _REF[key] = dict(lg=lg, bits=sm.torch_bits(lg)[0], name=sm.torch_bits(lg)[1], pos=pos, seed=seed, stream=stream,
                         gumbel=sm.gumbel_of(words), rowmask=np.asarray(rowmask, dtype=np.uint64), ids=ids, ctx=ctx)
    return _REF[key]


def _run_rows(lib, lg_dev, V, pos, stream, seed, temperature, top_k, top_p, pen=None):
    T = lg_dev.shape[0]
    d_pos = torch.from_numpy(np.asarray(pos, dtype=np.int32)).to(DEV)
    tok = torch.full((T,), -1, dtype=torch.int32, device=DEV)
    info = torch.full((T, 4), -1, dtype=torch.int32, device=DEV)
    if pen is None:
        d_ids = torch.zeros(T, dtype=torch.int32, device=DEV)
        d_rm = torch.zeros(T, dtype=torch.int64, device=DEV)
        d_bits = d_pw = None
    else:
        d_bits = torch.from_numpy(_bitmap(pen['ctx'], V).view(np.int32)).to(DEV)
        d_ids = torch.from_numpy(pen['ids']).to(DEV)
        d_rm = torch.from_numpy(pen['rowmask'].view(np.int64)).to(DEV)
        d_pw = torch.tensor([pen['penalty']], dtype=torch.float32, device=DEV)
    check(lib.la_sample_rows(sp(), ptr(lg_dev), V, T, ptr(d_pos), stream, C.c_uint64(seed), temperature, top_k, top_p, ptr(d_bits),
                             ptr(d_ids), ptr(d_rm), ptr(d_pw), ptr(tok), ptr(info)), 'sample_rows')
    torch.cuda.synchronize()
    return tok.cpu().numpy(), info.cpu().numpy()


def _check_rows(bits, name, gumbel, temperature, top_k, top_p, tok, info, what):
    """every row of one call against the model -> number of rows left out by the GAP rule"""
    T, V = bits.shape
    left_out = 0
    Tf = float(np.float32(temperature))
    for r in range(T):
        keys = sm.keys_of(bits[r], name)
        kk, kp, kept_n = int(info[r, 0]), int(info[r, 1]), int(info[r, 2])
        assert kk == sm.topk_key(keys, top_k), (what, r, kk)
        surv = np.nonzero(keys >= max(kk, 1))[0]
        ks = keys[surv]
        z = sm.key_to_f64(ks, name) / Tf
        if top_p < 1.0:
            m = np.exp(z - z.max())
            above, at_or_above = m[ks > kp].sum() / m.sum(), m[ks >= kp].sum() / m.sum()
            assert kp > 0 and above < top_p + DELTA and at_or_above >= top_p - DELTA, (what, r, kp, above, at_or_above)
            SLACK['worst'] = max(SLACK['worst'], above - top_p, top_p - at_or_above)
        else:
            assert kp == 0, (what, r)
        sel = ks >= max(kk, kp, 1)
        assert kept_n == int(sel.sum()) and kept_n >= 1, (what, r, kept_n, int(sel.sum()))
        cand = surv[sel]
        score = z[sel] + gumbel[r][cand]
        order = np.argsort(-score, kind='stable')
        gap = score[order[0]] - score[order[1]] if len(order) > 1 else np.inf
        t = int(tok[r])
        assert t in set(cand.tolist()), (what, r, t)
        if gap < GAP:
            left_out += 1
            continue
        assert t == int(cand[order[0]]), (what, r, t, int(cand[order[0]]), gap)
    return left_out


GRID = [(t, k, p) for t in (0.7, 1.0) for k in (0, 1, 50) for p in (1.0, 0.9)]


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
@pytest.mark.parametrize('V', [512, 32000, 152064])
def test_row_stage_equals_the_model(V, dtype):
    lib = _lib.lib_for(dtype)
    ref = _reference(V, dtype)
    lg_dev = ref['lg'].to(DEV).contiguous()
    left_out = rows = 0
    for temperature, top_k, top_p in GRID:
        tok, info = _run_rows(lib, lg_dev, V, ref['pos'], ref['stream'], ref['seed'], temperature, top_k, top_p)
        n = _check_rows(ref['bits'], ref['name'], ref['gumbel'], temperature, top_k, top_p, tok, info, (V, temperature, top_k, top_p))
        if top_k == 1:
            assert n == 0 and (tok == ref['lg'].float().argmax(-1).numpy()).all()      # the plain argmax, no row left out
        left_out += n
        rows += len(tok)
    # the penalty variant: context bitmap + the path tokens of every row, penalised and rounded to the storage type first
    penalty = 1.3
    pen_bits = ref['bits'].copy()
    for r in range(64):
        members = np.zeros(V, dtype=bool)
        members[ref['ctx']] = True
        members[[int(ref['ids'][a]) for a in range(64) if (int(ref['rowmask'][r]) >> a) & 1]] = True
        pen_bits[r] = sm.penalised_bits(ref['bits'][r], ref['name'], members, penalty)
    assert (pen_bits != ref['bits']).any()
    tok, info = _run_rows(lib, lg_dev, V, ref['pos'], ref['stream'], ref['seed'], 0.7, 50, 0.9,
                          pen=dict(ctx=ref['ctx'], ids=ref['ids'], rowmask=ref['rowmask'], penalty=penalty))
    left_out += _check_rows(pen_bits, ref['name'], ref['gumbel'], 0.7, 50, 0.9, tok, info, (V, 'penalty'))
    rows += 64
    print(f'V={V} {ref["name"]}: {left_out} of {rows} rows left out by the gap rule; worst top-p slack so far {SLACK["worst"]:.3e}')
    assert left_out <= rows // 100


# ------------------------------------------------------------------------------------------------ 3. determinism
@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
def test_row_stage_is_a_function_of_its_inputs(dtype):
    lib = _lib.lib_for(dtype)
    V = 32000
    ref = _reference(V, dtype)
    lg_dev = ref['lg'].to(DEV).contiguous()
    args = (ref['stream'], ref['seed'], 0.8, 50, 0.95)
    tok_a, info_a = _run_rows(lib, lg_dev, V, ref['pos'], *args)
    tok_b, info_b = _run_rows(lib, lg_dev, V, ref['pos'], *args)
    assert (tok_a == tok_b).all() and (info_a == info_b).all()
    # the same logits rows at other row indices, with their positions: the same tokens
    perm = np.random.RandomState(1).permutation(64)
    tok_c, info_c = _run_rows(lib, lg_dev[torch.from_numpy(perm).to(DEV)].contiguous(), V, ref['pos'][perm], *args)
    assert (tok_c == tok_a[perm]).all() and (info_c == info_a[perm]).all()
    # another position, stream or seed: the filter is the same, the draws are not
    for other in (dict(pos=ref['pos'] + 1), dict(stream=ref['stream'] + 1), dict(seed=ref['seed'] + 1)):
        tok_d, info_d = _run_rows(lib, lg_dev, V, other.get('pos', ref['pos']), other.get('stream', ref['stream']),
                                  other.get('seed', ref['seed']), 0.8, 50, 0.95)
        assert (info_d == info_a).all() and (tok_d != tok_a).mean() > 0.5, other.keys()


# ------------------------------------------------------------------------------------------------ 4. the stage inside the step
PARAMS = dict(seed=7, temperature=0.8, top_k=20, top_p=0.9)


def _sd(dtype):
    return {k: v.to(dtype) for k, v in tiny_weights(0, torch.float32).items()}


def _model_words(lg_rows, positions, stream, dtype, params=PARAMS):
    """the kernel under test as the unit entry: tokens of plain rows at (position, stream) — compared with the numpy model in section 2"""
    lib = _lib.lib_for(dtype)
    tok, _ = _run_rows(lib, lg_rows.contiguous(), lg_rows.shape[1], positions, stream, params['seed'], params['temperature'],
                       params['top_k'], params['top_p'])
    return tok


def _expect_words(lg_rows, positions, stream, dtype, got, params=PARAMS):
    """ARGMAX words of live rows == the numpy model on the rows' logits (GAP rule: a marginal row may differ, and is counted)"""
    bits, name = sm.torch_bits(lg_rows)
    V = bits.shape[1]
    marginal = 0
    for r in range(len(bits)):
        kk, kp, kept = sm.filter_row(bits[r], name, params['temperature'], params['top_k'], params['top_p'])
        keys = sm.keys_of(bits[r], name)
        m, _ = sm.masses(keys, name, params['temperature'], kk)
        edge = min(abs(sm.mass_above(keys, m, kp) - params['top_p']), abs(sm.mass_above(keys, m, kp, strict=False) - params['top_p']))
        t, gap = sm.pick(bits[r], name, params['temperature'], kept, sm.sample_bits(params['seed'], stream, int(positions[r]) + 1, V))
        if gap < GAP or edge < DELTA:
            marginal += 1
            continue
        assert int(got[r]) == t, (r, int(got[r]), t, gap, edge)
    return marginal


def _depths(rowmask):
    return np.array([bin(int(m)).count('1') - 1 for m in rowmask], dtype=np.int32)


def _mask_matrix(rowmask):
    T = len(rowmask)
    return np.array([[(int(rowmask[i]) >> j) & 1 for j in range(T)] for i in range(T)], dtype=np.int64)


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
def test_stage_inside_the_single_step(dtype):
    shape = tiny_shape()
    eng = LlamaVerifyEngine(shape, _sd(dtype), max_length=512)
    rs = np.random.RandomState(4)
    prompt = rs.randint(3, shape.vocab, size=90).tolist()                 # two prefill blocks
    eng.set_sampling(True, **PARAMS)
    n0 = eng.sample_launches()
    tok = eng.prefill(prompt, fast=False)
    row = (len(prompt) - 1) % 64
    # prefill: only the last row emits, at position = prompt length
    lg = eng.logits()[row:row + 1].clone()
    assert tok == int(_model_words(lg, [len(prompt) - 1], 0, dtype)[0])
    marginal = _expect_words(lg, [len(prompt) - 1], 0, dtype, [tok])
    seq = prompt + [tok]
    for step in range(4):
        T = int(rs.randint(2, 65)) if step else 64
        _, rm = random_tree(rs, T)
        rm = np.asarray(rm, dtype=np.uint64)
        ids = np.concatenate([[seq[-1]], rs.randint(3, shape.vocab, size=T - 1)]).astype(np.int32)
        nk = eng.n_keys
        toks, n = eng.step(ids.copy(), rm.copy(), eager=(step == 2))
        words = eng.state().cpu().numpy()[_lib.LA_ST_ARGMAX:_lib.LA_ST_ARGMAX + T]
        positions = nk + _depths(rm)
        lg = eng.logits()[:T].clone()
        assert (words == _model_words(lg, positions, 0, dtype)).all(), step
        marginal += _expect_words(lg, positions, 0, dtype, words)
        want, rows = lo.accept_scan(ids.tolist(), _mask_matrix(rm), words.tolist())
        assert toks == want and n == len(rows), (step, toks, want)
        assert eng.n_keys == nk + len(rows)
        seq += toks
    assert marginal <= 2, marginal
    assert eng.sample_launches() - n0 == 2 + 4
    eng.set_sampling(False)
    eng.step(np.asarray(seq[-1:], dtype=np.int32), ONE)
    assert eng.sample_launches() - n0 == 6                                # off again: the stage is not launched


@pytest.mark.parametrize('multi', [False, True], ids=['bstep-2-slots', 'mstep-3-blocks'])
def test_stage_inside_the_batch_steps(multi):
    dtype = torch.bfloat16
    shape = tiny_shape()
    B = 3 if multi else 2
    eng = LlamaVerifyEngine(shape, _sd(dtype), max_length=256, n_slots=B, max_blocks=B if multi else 0)
    rs = np.random.RandomState(6 + multi)
    lens = [30, 22, 27][:B]
    prompts = {b: rs.randint(3, shape.vocab, size=lens[b]).tolist() for b in range(B)}
    for b in range(B):
        eng.sampling_stream(b, b)
    eng.set_sampling(True, **PARAMS)
    first = eng.mprefill_many(prompts) if multi else eng.bprefill_many(prompts)
    lg = eng.mlogits() if multi else eng.logits()
    base = {b: 64 * b for b in range(B)} if multi else eng.bstep_rows()
    marginal = 0
    for b in range(B):
        row = lg[base[b] + lens[b] - 1][None].clone()
        assert first[b] == int(_model_words(row, [lens[b] - 1], b, dtype)[0]), b
        marginal += _expect_words(row, [lens[b] - 1], b, dtype, [first[b]])
    seqs = {b: prompts[b] + [first[b]] for b in range(B)}
    for step in range(3):
        segs = []
        for b in range(B):
            T = int(rs.randint(1, (64 if multi else 64 // B) + 1))
            _, rm = random_tree(rs, T)
            ids = np.concatenate([[seqs[b][-1]], rs.randint(3, shape.vocab, size=T - 1)]).astype(np.int32)
            segs.append((b, ids, np.asarray(rm, dtype=np.uint64), 0, 16))
        nk = list(eng.slot_keys)
        if multi:
            out = dict(zip(range(B), eng.mstep(segs)))
            lg, base = eng.mlogits(), {b: 64 * b for b in range(B)}
            am = eng.mout().cpu().numpy()[_lib.LA_MOUT_ARGMAX:]
        else:
            out = eng.bstep(segs)
            lg, base = eng.logits(), eng.bstep_rows()
            am = eng.bstate().cpu().numpy()[_lib.LA_BST_ARGMAX:]
        for b, ids, rm, _, limit in segs:
            T = len(ids)
            words = am[base[b]:base[b] + T]
            positions = nk[b] + _depths(rm)
            rows_lg = lg[base[b]:base[b] + T].clone()
            assert (words == _model_words(rows_lg, positions, b, dtype)).all(), (step, b)
            marginal += _expect_words(rows_lg, positions, b, dtype, words)
            want, rows = lo.accept_scan_limited(ids.tolist(), _mask_matrix(rm), words.tolist(), limit)
            assert list(out[b]) == want, (step, b, out[b], want)
            assert eng.slot_keys[b] == nk[b] + len(rows)
            seqs[b] += want
    assert marginal <= 2, marginal
    eng.set_sampling(False)


# ------------------------------------------------------------------------------------------------ 5. lookahead == no-draft
# The invariant is "the same logits give the same tokens, whatever the trees were".  The 16-bit logits of a position are NOT the same
# bits in a T = 1 step and in a tree step on the pure random-init tiny model (measured on the MI355X: 38 of 39 rows differ, by up to
# 0.055 — the attention sums run in another order; llama_engine.random_weights documents the same for greedy decoding), and one
# storage step on a logit moves a Gumbel score by ~1e-2, enough to flip a draw now and then.  So these tests run the tiny model of
# tests/tiny_model.py with its decisive weights, as the greedy "lookahead == plain" tests of this suite do — the residual stream stays
# on the token embedding, so a position's logits do not depend on the tree — and with lm_head scaled by 1/8 (exact in bf16): the
# decisive head alone leads by ~19 logits, under which every draw is the argmax; at 1/8 the top logit leads by ~2.4, the top token
# holds roughly half of the mass under temperature 0.8 / top_k 20 / top_p 0.9, and the sequence is a random walk.  The tests assert
# that (another seed gives another sequence, and the sequence is not the greedy one).
def _sd_decisive():
    sd = tiny_decisive_weights(0, torch.bfloat16)
    sd['lm_head.weight'] = sd['lm_head.weight'] * 0.125
    return sd


def _warpers(penalty=None):
    from transformers import (LogitsProcessorList, RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper, TopKLogitsWarper,
                              TopPLogitsWarper)
    pre = [RepetitionPenaltyLogitsProcessor(penalty)] if penalty else []
    return LogitsProcessorList(pre + [TemperatureLogitsWarper(0.8), TopKLogitsWarper(20), TopPLogitsWarper(0.9)])


def _warm_trie(rows):
    cache = LookaheadCache()
    for row in rows:
        cache.put([int(t) for t in row], branch_length=13, mode='output', idx=-1)
    return cache


@pytest.mark.parametrize('penalty', [None, 1.3], ids=['plain', 'penalty-1.3'])
def test_lookahead_equals_no_draft_bs1(penalty):
    shape = tiny_shape()
    model = LlamaForCausalLM(shape, _sd_decisive(), max_length=512, eos_token_id=None)
    eng = model.engine
    rs = np.random.RandomState(3)
    prompt = torch.tensor([rs.randint(3, shape.vocab, size=50).tolist()])
    n_new, procs = 48, _warpers(penalty)
    n0 = eng.sample_launches()
    plain = model.greedy_search(prompt, 50 + n_new, eos_token_id=None, logits_processor=procs, do_sample=True, sample_seed=7)[0].tolist()
    assert eng.sample_launches() > n0 and not eng.sampling
    assert plain == model.greedy_search(prompt, 50 + n_new, eos_token_id=None, logits_processor=procs, do_sample=True, sample_seed=7)[0].tolist()
    other = model.greedy_search(prompt, 50 + n_new, eos_token_id=None, logits_processor=procs, do_sample=True, sample_seed=8)[0].tolist()
    greedy = model.greedy_search(prompt, 50 + n_new, eos_token_id=None)[0].tolist()
    assert other != plain and plain != greedy and len(set(plain[50:])) > 8     # the seed matters: this is sampling, not an argmax
    for native in ((True, False) if penalty is None else (True,)):
        for decoding_length in (16, 64):
            model.lookahead_cache = _warm_trie([plain[49:]])
            dk = {'use_lookahead': True, 'decoding_length': decoding_length, 'branch_length': 12, 'stop_words': {}, 'native_loop': native,
                  'do_sample': True, 'sample_seed': 7}
            out = model.lookahead_generation(prompt, logits_processor=procs, stopping_criteria=50 + n_new, eos_token_id=[None],
                                             return_dict_in_generate=True, decoding_kwargs=dk)
            seq = out.sequences[0].tolist()
            assert seq[:50 + n_new] == plain[:len(seq)][:50 + n_new], (native, decoding_length)
            edls = out.kwargs['edls']
            print(f'native={native} decoding_length={decoding_length}: mean edls {np.mean(edls[1:]):.2f}')
            assert np.mean(edls[1:]) > 2, edls                             # drafts were accepted: the comparison is not vacuous
            assert not eng.sampling and eng.repetition_penalty == 1.0


@pytest.mark.parametrize('bs', [2, 3])
@pytest.mark.parametrize('multi', [False, True], ids=['cursor', 'multi-block'])
def test_lookahead_equals_no_draft_batch(bs, multi):
    shape = tiny_shape()
    model = BatchLlama(shape, _sd_decisive(), max_length=512, max_batch=4, eos_token_id=None, max_blocks=4 if multi else 0)
    rs = np.random.RandomState(13 + bs)
    lens = [60, 47, 31][:bs]
    P = max(lens)
    ids = np.zeros((bs, P), dtype=np.int64)
    am = np.zeros((bs, P), dtype=np.int64)
    for b, n in enumerate(lens):
        ids[b, P - n:] = rs.randint(3, shape.vocab, size=n)
        am[b, P - n:] = 1
    t_ids, t_am = torch.from_numpy(ids), torch.from_numpy(am)
    n_new, procs = 48, _warpers()
    n0 = model.engine.sample_launches()
    plain = model.greedy_search(t_ids, P + n_new, attention_mask=t_am, eos_token_id=None, logits_processor=procs, do_sample=True,
                                sample_seed=7).cpu().numpy()
    assert model.engine.sample_launches() > n0
    assert len({tuple(plain[b, P:].tolist()) for b in range(bs)}) == bs     # stream = batch index: the rows draw differently
    model.lookahead_cache = _warm_trie([plain[b, P - 1:] for b in range(bs)])
    dk = {'use_lookahead': True, 'decoding_length': 64, 'branch_length': 12, 'stop_words': {}, 'per_sample_budget': multi,
          'do_sample': True, 'sample_seed': 7}
    out = model.lookahead_generation(t_ids, logits_processor=procs, stopping_criteria=P + n_new, eos_token_id=[None], pad_token_id=0,
                                     return_dict_in_generate=True, attention_mask=t_am, decoding_kwargs=dk)
    got = out.sequences.cpu().numpy()
    w = min(got.shape[1], plain.shape[1], P + n_new)
    assert got[:, :w].tolist() == plain[:, :w].tolist()
    edls = out.kwargs['edls']
    print(f'bs={bs} multi={multi}: mean edls {np.mean(edls[bs:]):.2f}')
    assert np.mean(edls[bs:]) > 2, edls
    assert not model.engine.sampling


# ------------------------------------------------------------------------------------------------ 6. the front door
def test_front_door_takes_the_stage_only_with_a_sample_seed(monkeypatch):
    shape = tiny_shape()
    model = LlamaForCausalLM(shape, _sd_decisive(), max_length=512, eos_token_id=None)
    eng = model.engine
    rs = np.random.RandomState(5)
    prompt = torch.tensor([rs.randint(3, shape.vocab, size=40).tolist()])
    calls = [0]
    inner = torch.multinomial

    def spy(*a, **k):
        calls[0] += 1
        return inner(*a, **k)
    monkeypatch.setattr(torch, 'multinomial', spy)
    kw = dict(max_new_tokens=12, do_sample=True, temperature=0.8, top_k=20, top_p=0.9)
    # plain greedy: neither stage
    model.generate(prompt, max_new_tokens=12, decoding_kwargs={'use_lookahead': True, 'decoding_length': 16, 'stop_words': {}})
    assert eng.sample_launches() == 0 and eng.penalty_launches() == 0 and calls[0] == 0
    # without the key, or with device_processors=False: the host walk
    model.generate(prompt, decoding_kwargs={'use_lookahead': True, 'decoding_length': 16, 'stop_words': {}}, **kw)
    assert eng.sample_launches() == 0 and calls[0] > 0
    before = calls[0]
    model.generate(prompt, decoding_kwargs={'use_lookahead': True, 'decoding_length': 16, 'stop_words': {}, 'sample_seed': 7,
                                            'device_processors': False}, **kw)
    assert eng.sample_launches() == 0 and calls[0] > before
    # with the key: the device stage, and no host draw
    before = calls[0]
    a = model.generate(prompt, decoding_kwargs={'use_lookahead': True, 'decoding_length': 16, 'stop_words': {}, 'sample_seed': 7}, **kw)
    assert eng.sample_launches() > 0 and calls[0] == before
    # the no-draft front door with the same seed: the same tokens
    n = eng.sample_launches()
    b = model.generate(prompt, decoding_kwargs={'sample_seed': 7}, **kw)
    assert eng.sample_launches() > n and calls[0] == before
    assert a[0].tolist() == b[0].tolist()
    assert eng.penalty_launches() == 0 and not eng.sampling


# ------------------------------------------------------------------------------------------------ 7. wide trees
def test_wide_tree_pass_with_sampling_on_is_refused():
    """a missing kernel is an error, not a silent fall-back: the multi-block step has no wide-tree form of the stage"""
    shape = tiny_shape()
    eng = LlamaVerifyEngine(shape, _sd(torch.bfloat16), max_length=512, n_slots=1, max_blocks=2)
    rs = np.random.RandomState(1)
    eng.mprefill(0, rs.randint(3, shape.vocab, size=20).tolist())
    eng.set_sampling(True, **PARAMS)
    rmw = np.zeros((100, 2), dtype=np.uint64)
    ids = rs.randint(3, shape.vocab, size=100).astype(np.int32)
    anc = [1]
    for r in range(1, 100):
        anc.append(anc[r - 1] | (1 << r))
    for r in range(100):
        rmw[r, 0] = anc[r] & 0xFFFFFFFFFFFFFFFF
        rmw[r, 1] = anc[r] >> 64
    with pytest.raises(AssertionError):
        eng.tstep(ids, rmw, mode=0)
    assert 'sampling' in _lib.last_error()
    eng.set_sampling(False)
    eng.reset_slot(-1)
    eng.mprefill(0, rs.randint(3, shape.vocab, size=20).tolist())
    toks, _ = eng.tstep(ids, rmw, mode=0)                                   # off again: the wide pass runs
    assert len(toks) >= 1


def test_batch_request_with_wide_trees_keeps_the_host_walk(monkeypatch):
    shape = tiny_shape()
    model = BatchLlama(shape, _sd(torch.bfloat16), max_length=256, max_batch=4, eos_token_id=None, max_blocks=4)
    rs = np.random.RandomState(2)
    t_ids = torch.from_numpy(rs.randint(3, shape.vocab, size=(2, 30)).astype(np.int64))
    calls = [0]
    inner = torch.multinomial

    def spy(*a, **k):
        calls[0] += 1
        return inner(*a, **k)
    monkeypatch.setattr(torch, 'multinomial', spy)
    dk = {'use_lookahead': True, 'decoding_length': 256, 'branch_length': 12, 'stop_words': {}, 'do_sample': True, 'sample_seed': 7}
    model.lookahead_generation(t_ids, logits_processor=_warpers(), stopping_criteria=30 + 10, eos_token_id=[None], pad_token_id=0,
                               return_dict_in_generate=True, attention_mask=torch.ones_like(t_ids), decoding_kwargs=dk)
    assert model.engine.sample_launches() == 0 and calls[0] > 0
