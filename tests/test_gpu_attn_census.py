# -*- coding: utf-8 -*-
"""Attention visibility census on the MI355X (pytest -m gpu): every step path runs the census model of tests/census.py and the
residual stream it leaves (engine.hidden() / engine.mhidden()) is compared, row by row and head by head, with the integer rule
expected_visible — an exact statement of WHICH keys each row read.  Product libraries throughout.  Every test prints its number of
(row, head) checks and the worst deviation against the 0.25 bar (pytest -s)."""
import numpy as np
import pytest
import torch

from oracle import llama_oracle as lo
from oracle.tiny import random_tree
from painlessinferenceacceleration_amd.llama_engine import LlamaShape, LlamaVerifyEngine, random_weights
from tests.census import BAR, CensusModel, CensusStats, census_check, expected_visible

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
SIZES = (1, 2, 17, 33, 63, 64)


def _tree(rs, T, tokens):
    """random T-row tree over `tokens` -> (ids int32 [T], rowmask uint64 [T])"""
    _, rows = random_tree(rs, T)
    return np.asarray(tokens)[rs.randint(len(tokens), size=T)].astype(np.int32), np.asarray(rows, dtype=np.uint64)


def _check_single(cm, eng, keys, ids, rm, what, st):
    """the last single-sequence block (T rows; the 64 - T unused rows carry their diagonal bit and token 0) over context `keys`"""
    T = len(ids)
    assert eng.n_keys == len(keys), (what, eng.n_keys, len(keys))
    masks = [int(rm[t]) if t < T else (1 << t) for t in range(64)]
    row_tok = [int(x) for x in ids] + [0] * (64 - T)
    vis = expected_visible(len(keys), masks, cm.window)
    census_check(cm, eng.hidden(), row_tok, vis, list(keys) + row_tok, what, st)


def _check_rows(cm, h, keys, ids, masks, what, st):
    """rows of one slot's tree / chain (h [R, hidden]) over the slot's committed `keys`; masks: Python ints over the same rows"""
    vis = expected_visible(len(keys), masks, cm.window)
    fresh = [int(x) for x in ids] + [0] * (vis.shape[1] - len(keys) - len(ids))
    census_check(cm, h, [int(x) for x in ids], vis, list(keys) + fresh, what, st)


# ================================================================================================ single sequence, dense walk
WINDOWS = [(0, False), (33, False), (33, True), (40, False), (40, True), (64, False), (64, True), (100, False), (100, True)]


def _dense_walk(cm, dtype, kv_ring, st, seed, stops=38, inc=17):
    """context 0 -> (stops - 1) * inc keys in steps of inc (17: every residue mod 32, every tile count 0 .. 20, 221 / 238 on the two
    sides of the early-first-tile threshold); at every stop one step on a random tree, tree sizes cycling over SIZES, eager and
    graph steps alternating every six stops"""
    eng = LlamaVerifyEngine(cm.shape(), cm.weights(dtype), max_length=stops * inc + 64, kv_ring=kv_ring)
    rs = np.random.RandomState(seed)
    toks = np.arange(cm.vocab)
    keys, residues = [], set()
    for i in range(stops):
        eager = (i // 6) % 2 == 1
        residues.add(len(keys) % 32)
        T = SIZES[i % len(SIZES)]
        what = f'step {cm.nh}/{cm.nkv} hd {cm.hd} window {cm.window} ring {kv_ring} {dtype} nkeys {len(keys)} T {T} eager {eager}'
        ids, rm = _tree(rs, T, toks)
        eng.verify_only(ids, rm, eager=eager)
        _check_single(cm, eng, keys, ids, rm, what, st)
        if T < inc:                                  # too few rows to keep inc of them: a full tree feeds the context
            T = 64
            ids, rm = _tree(rs, T, toks)
            eng.verify_only(ids, rm, eager=eager)
            _check_single(cm, eng, keys, ids, rm, what + ' (feeder)', st)
        rows = [0] + sorted(int(r) for r in 1 + rs.permutation(T - 1)[:inc - 1])
        eng.commit(rows)
        keys += [int(ids[r]) for r in rows]
    assert residues == set(range(32)) and len(keys) >= 600
    if kv_ring:
        assert len(keys) >= 2 * eng.max_keys, 'the ring must wrap at least twice'
    del eng
    torch.cuda.empty_cache()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('nh,nkv,hd', [(2, 2, 128), (4, 2, 128), (6, 3, 128), (2, 2, 64), (2, 2, 96)])
def test_single_sequence_dense_walk(nh, nkv, hd, dtype):
    """verify_only + commit on 2 / 2, 4 / 2 (GQA) and 6 / 3 heads (the other block-id map), head_dim 64 / 96 in padded lanes: the
    window horizon, skipped tiles and ring slots at every nkeys residue.  head_dim 128 takes all nine (window, ring) combinations;
    head_dim 64 / 96 deliberately three of them (no window, a ringed window, a plain window): the lanes only pad the same kernels'
    Q / K / V fragments with zeros, the window and ring arithmetic does not see head_dim."""
    st = CensusStats(f'single-sequence dense walk {nh}/{nkv} hd {hd} {dtype}')
    windows = WINDOWS if hd == 128 else [(0, False), (40, True), (100, False)]
    for k, (window, ring) in enumerate(windows):
        _dense_walk(CensusModel(nh, nkv, head_dim=hd, window=window), dtype, ring, st, seed=100 * nh + k)
    print(st)
    assert st.worst < BAR


# ================================================================================================ fused accept and compaction
@pytest.mark.parametrize('dtype', DTYPES)
def test_fused_accept_single_step(dtype):
    """step(): the permutation head makes the accept walk follow the successor chain planted in the tree; the emitted tokens are the
    chain, and the next step's census shows exactly the accepted rows as new committed keys, none of the rejected"""
    cm = CensusModel(4, 2, lm_head='perm')
    st = CensusStats(f'fused accept, step {dtype}')
    eng = LlamaVerifyEngine(cm.shape(), cm.weights(dtype), max_length=512)
    rs = np.random.RandomState(4)
    prompt = rs.randint(0, cm.vocab, size=50).tolist()
    root = eng.prefill(prompt)
    assert root == cm.succ(prompt[-1])
    keys = list(prompt)
    for i, (depth, T) in enumerate([(0, 1), (1, 2), (3, 17), (7, 33), (10, 63), (0, 64), (15, 64), (5, 17), (12, 64)]):
        ids, rm = cm.chain_tree(rs, root, depth, T)
        toks, n = eng.step(ids, rm, eager=(i % 2 == 1))
        assert toks == cm.chain(root, depth + 1) and n == depth + 1, (i, toks, cm.chain(root, depth + 1), n)
        # the block itself saw the context before the commit
        masks = [int(rm[t]) if t < T else (1 << t) for t in range(64)]
        row_tok = [int(x) for x in ids] + [0] * (64 - T)
        census_check(cm, eng.hidden(), row_tok, expected_visible(len(keys), masks, 0), keys + row_tok, f'fused step {i}', st)
        keys = keys + [int(x) for x in ids[:depth + 1]]          # the root and the accepted chain rows, nothing else
        assert eng.n_keys == len(keys)
        root = toks[-1]
    ids, rm = _tree(rs, 64, np.arange(cm.vocab))
    eng.verify_only(ids, rm)
    _check_single(cm, eng, keys, ids, rm, 'after the fused steps', st)
    print(st)
    del eng
    torch.cuda.empty_cache()


@pytest.mark.parametrize('window', [0, 40])
@pytest.mark.parametrize('dtype', DTYPES)
def test_cursor_batch_isolation_accept_and_commit(dtype, window):
    """bstep: 2 to 4 of 4 slots share the block (slot 1 idle every other step, slot 2 joins twice) with unequal contexts and disjoint class
    groups — a key of a foreign slot would show as a count in a foreign class; fused accept along planted chains (mode 0), prefill
    chains (mode 1) and forward-only + bcommit (mode 2) compact per slot"""
    cm = CensusModel(4, 2, lm_head='perm', window=window)
    st = CensusStats(f'bstep window {window} {dtype}')
    eng = LlamaVerifyEngine(cm.shape(), cm.weights(dtype), max_length=512, n_slots=4)
    rs = np.random.RandomState(9 + window)
    gt = {s: cm.group_tokens(s) for s in range(4)}
    prompts = {0: gt[0][rs.randint(len(gt[0]), size=70)].tolist(), 1: gt[1][rs.randint(len(gt[1]), size=5)].tolist(),
               2: gt[2][rs.randint(len(gt[2]), size=33)].tolist(), 3: gt[3][rs.randint(len(gt[3]), size=150)].tolist()}
    first = eng.bprefill_many(prompts)
    keys = {s: list(p) for s, p in prompts.items()}
    roots = {s: first[s] for s in prompts}
    for s in prompts:
        assert first[s] == cm.succ(prompts[s][-1]) and eng.slot_keys[s] == len(keys[s])
    plans = [((0, 20, 0), (1, 1, 0), (3, 30, 0)), ((3, 33, 2), (0, 17, 2)), ((0, 2, 0), (1, 40, 1), (3, 22, 0)),
             ((3, 63, 0),), ((1, 17, 2), (0, 30, 2), (3, 17, 2)), ((0, 31, 0), (3, 33, 0)), ((1, 10, 0), (0, 10, 1), (3, 44, 0)),
             ((0, 16, 0), (1, 9, 0), (2, 17, 0), (3, 22, 0)), ((2, 20, 2), (0, 10, 2), (1, 14, 2), (3, 20, 2)), ((2, 5, 0), (3, 40, 0))]
    for i, plan in enumerate(plans):
        segs, want = [], {}
        for s, T, mode in plan:
            if mode == 0:
                depth = min(T - 1, int(rs.randint(0, 12)))
                ids, rm = cm.chain_tree(rs, roots[s], depth, T, gt[s])
                want[s] = depth
            elif mode == 1:
                ids, rm = gt[s][rs.randint(len(gt[s]), size=T)].astype(np.int32), eng._CHAIN[:T]
            else:
                ids, rm = _tree(rs, T, gt[s])
            segs.append((s, ids, rm, mode, 1 if mode == 1 else 16))
        out = eng.bstep(segs, eager=(i % 2 == 1))
        h = eng.hidden()
        base = eng.bstep_rows()
        kept = {}
        for s, ids, rm, mode, _ in segs:
            T = len(ids)
            _check_rows(cm, h[base[s]:base[s] + T], keys[s], ids, [int(x) for x in rm], f'bstep {i} slot {s} mode {mode}', st)
            if mode == 0:
                assert out[s] == cm.chain(roots[s], want[s] + 1), (i, s, out[s])
                keys[s] += [int(x) for x in ids[:want[s] + 1]]
                roots[s] = out[s][-1]
            elif mode == 1:
                assert out[s] == [cm.succ(ids[-1])]
                keys[s] += [int(x) for x in ids]
                roots[s] = out[s][0]
            else:
                kept[s] = [0] + sorted(int(r) for r in 1 + rs.permutation(T - 1)[:min(T - 1, 9)])
                keys[s] += [int(ids[r]) for r in kept[s]]
        if kept:
            eng.bcommit(kept)
        for s in keys:
            assert eng.slot_keys[s] == len(keys[s]), (i, s)
    # a last forward-only block: every slot's context is what the accepts / commits above left, nothing else
    segs = [(s, *_tree(rs, 16, gt[s]), 2, 16) for s in (3, 1, 2, 0)]
    eng.bstep(segs)
    base = eng.bstep_rows()
    for s, ids, rm, _, _ in segs:
        _check_rows(cm, eng.hidden()[base[s]:base[s] + 16], keys[s], ids, [int(x) for x in rm], f'bstep final slot {s}', st)
    print(st)
    del eng
    torch.cuda.empty_cache()


@pytest.mark.parametrize('B', [2, 5, 8])
@pytest.mark.parametrize('dtype', DTYPES)
def test_multi_block_mixed_modes_isolation_and_commit(dtype, B):
    """mstep with B blocks of B slots: verify trees (fused accept along planted chains), forward-only trees and prefill chains in ONE
    pass, slots on disjoint class groups; all-forward-only passes + mcommit compact per slot"""
    cm = CensusModel(4, 2, lm_head='perm')
    st = CensusStats(f'mstep B {B} {dtype}')
    eng = LlamaVerifyEngine(cm.shape(), cm.weights(dtype), max_length=512, n_slots=B, max_blocks=B)
    rs = np.random.RandomState(20 + B)
    gt = [cm.group_tokens(s) for s in range(B)]
    keys = [gt[s][rs.randint(len(gt[s]), size=int(rs.randint(1, 100)))].tolist() for s in range(B)]
    roots = []
    for s in range(B):
        tok = eng.mprefill(s, keys[s])
        assert tok == cm.succ(keys[s][-1])
        roots.append(tok)
    for i in range(6):
        all_fwd = i in (2, 4)
        blocks, want = [], {}
        for s in range(B):
            mode = 2 if all_fwd else (s + i) % 3
            T = SIZES[(s + 2 * i) % len(SIZES)]
            if mode == 0:
                want[s] = min(T - 1, int(rs.randint(0, 14)))
                ids, rm = cm.chain_tree(rs, roots[s], want[s], T, gt[s])
            elif mode == 1:
                ids, rm = gt[s][rs.randint(len(gt[s]), size=T)].astype(np.int32), eng._CHAIN[:T]
            else:
                ids, rm = _tree(rs, T, gt[s])
            blocks.append((s, ids, rm, mode, 1 if mode == 1 else 16))
        out = eng.mstep(blocks, eager=(i % 2 == 1))
        h = eng.mhidden()
        kept = []
        for b, (s, ids, rm, mode, _) in enumerate(blocks):
            T = len(ids)
            _check_rows(cm, h[64 * b:64 * b + T], keys[s], ids, [int(x) for x in rm], f'mstep pass {i} block {b} mode {mode}', st)
            if mode == 0:
                assert out[b] == cm.chain(roots[s], want[s] + 1), (i, b, out[b])
                keys[s] += [int(x) for x in ids[:want[s] + 1]]
                roots[s] = out[b][-1]
            elif mode == 1:
                assert out[b] == [cm.succ(ids[-1])]
                keys[s] += [int(x) for x in ids]
                roots[s] = out[b][0]
            elif all_fwd:
                kept.append([0] + sorted(int(r) for r in 1 + rs.permutation(T - 1)[:min(T - 1, 11)]))
                keys[s] += [int(ids[r]) for r in kept[-1]]
        if all_fwd:
            eng.mcommit(kept)
        for s in range(B):
            assert eng.slot_keys[s] == len(keys[s]), (i, s)
    blocks = [(s, *_tree(rs, 64, gt[s]), 2, 16) for s in reversed(range(B))]
    eng.mstep(blocks)
    for b, (s, ids, rm, _, _) in enumerate(blocks):
        _check_rows(cm, eng.mhidden()[64 * b:64 * b + 64], keys[s], ids, [int(x) for x in rm], f'mstep final block {b}', st)
    print(st)
    del eng
    torch.cuda.empty_cache()


@pytest.mark.parametrize('dtype', DTYPES)
def test_multi_block_prefill_chains_are_causal_across_blocks(dtype):
    """mprefill of 64, 130 and 700 tokens (max_blocks 4: up to 256 rows per pass, the 700-token prompt in three passes): a row sees
    the committed keys, the earlier blocks of its chain in the pass and the rows before it in its own block"""
    cm = CensusModel(4, 2)
    st = CensusStats(f'mprefill chains {dtype}')
    eng = LlamaVerifyEngine(cm.shape(), cm.weights(dtype), max_length=1024, n_slots=3, max_blocks=4)
    rs = np.random.RandomState(31)
    for slot, P in ((0, 64), (1, 130), (2, 700)):
        prompt = rs.randint(0, cm.vocab, size=P).tolist()
        done = 0
        for s0 in range(0, P, 256):
            piece = prompt[s0:s0 + 256]
            blocks = [(slot, np.asarray(piece[j:j + 64], dtype=np.int32), eng._CHAIN[:len(piece[j:j + 64])], 1, 1) for j in range(0, len(piece), 64)]
            eng.mstep(blocks)
            n = len(piece)
            _check_rows(cm, eng.mhidden()[:n], prompt[:done], piece, [(2 << r) - 1 for r in range(n)], f'mprefill P {P} pass at {s0}', st)
            done += n
            assert eng.slot_keys[slot] == done
        ids, rm = _tree(rs, 64, np.arange(cm.vocab))
        eng.mstep([(slot, ids, rm, 2, 16)])
        _check_rows(cm, eng.mhidden()[:64], prompt, ids, [int(x) for x in rm], f'tree after mprefill P {P}', st)
    print(st)
    del eng
    torch.cuda.empty_cache()


def _wide_tree(rs, T, tokens):
    """random DFS tree of T <= 256 rows with ancestors in earlier blocks -> (ids, uint64 [T][W] words, Python-int masks)"""
    masks, stack = [1], [0]
    for i in range(1, T):
        while len(stack) > 1 and rs.rand() < 0.3:
            stack.pop()
        p = stack[-1]
        masks.append(masks[p] | (1 << i))
        stack.append(i)
    W = (T + 63) // 64
    rm = np.array([[(m >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range(W)] for m in masks], dtype=np.uint64)
    return np.asarray(tokens)[rs.randint(len(tokens), size=T)].astype(np.int32), rm, masks


@pytest.mark.parametrize('dtype', DTYPES)
def test_wide_trees_see_their_ancestors_in_earlier_blocks(dtype):
    """tstep at T = 65, 128, 200, 256 (LA_MIN_XMASK words over the earlier blocks) + tcommit; then mstep_trees with three wide trees
    of three slots in one pass + mcommit_trees; window 0 and 40"""
    for window in (0, 40):
        cm = CensusModel(4, 2, window=window)
        st = CensusStats(f'wide trees window {window} {dtype}')
        eng = LlamaVerifyEngine(cm.shape(), cm.weights(dtype), max_length=1024, n_slots=3, max_blocks=8)
        rs = np.random.RandomState(41 + window)
        gt = [cm.group_tokens(s) for s in range(3)]
        keys = [gt[s][rs.randint(len(gt[s]), size=n)].tolist() for s, n in enumerate((90, 33, 7))]
        for s in range(3):
            eng.mprefill(s, keys[s])
        for T in (65, 128, 200, 256):
            ids, rm, masks = _wide_tree(rs, T, gt[0])
            eng.tstep(ids, rm, slot=0, mode=2)
            _check_rows(cm, eng.mhidden()[:T], keys[0], ids, masks, f'tstep T {T} window {window}', st)
            # keep one root-to-leaf path: the deepest row's ancestors, in order
            deep = max(range(T), key=lambda r: bin(masks[r]).count('1'))
            path = [j for j in range(T) if (masks[deep] >> j) & 1][:20]
            eng.tcommit(path, T)
            keys[0] += [int(ids[r]) for r in path]
            assert eng.slot_keys[0] == len(keys[0])
        trees = [(s, *_wide_tree(rs, T, gt[s])) for s, T in ((2, 130), (0, 64), (1, 200))]
        eng.mstep_trees([(s, ids, rm, 2, 16) for s, ids, rm, _ in trees])
        b0, kept = 0, []
        for s, ids, rm, masks in trees:
            T = len(ids)
            _check_rows(cm, eng.mhidden()[64 * b0:64 * b0 + T], keys[s], ids, masks, f'mstep_trees slot {s} T {T} window {window}', st)
            b0 += (T + 63) // 64
            deep = max(range(T), key=lambda r: bin(masks[r]).count('1'))
            kept.append([j for j in range(T) if (masks[deep] >> j) & 1][:20])
            keys[s] += [int(ids[r]) for r in kept[-1]]
        eng.mcommit_trees(kept, [len(t[1]) for t in trees])
        blocks = [(s, *_tree(rs, 64, gt[s]), 2, 16) for s in range(3)]
        eng.mstep(blocks)
        for b, (s, ids, rm, _, _) in enumerate(blocks):
            assert eng.slot_keys[s] == len(keys[s])
            _check_rows(cm, eng.mhidden()[64 * b:64 * b + 64], keys[s], ids, [int(x) for x in rm], f'after the wide commits, slot {s}', st)
        print(st)
        del eng
        torch.cuda.empty_cache()


# ================================================================================== product head counts, the long-context graph
def _split_partials_tail(eng):
    """The last n_heads * 64 floats of lpart, the softmax denominators that ONLY the key-split attention (k_tree_attn) writes: the
    workspace is carved ... | opart | mpart | lpart | cand_val | cand_idx | state | ... (la_engine.cpp::carve, 256-byte aligned), so the
    tail of lpart ends 2 * cand * 256 bytes before the state block, cand = max(vocab / 32 * 4, 8 * lm_head workgroups).  Zero from
    the start (the workspace is zero-filled) until the first step on the key-split graph."""
    from painlessinferenceacceleration_amd import _lib
    cand = max(eng.shape.vocab // 32 * 4, eng.balanced_wg[2] * 8)
    end = eng._lib.la_llama_buffer(eng._h, 1) - eng.workspace.data_ptr() - 2 * cand * 256
    n = eng.shape.n_heads * 256
    assert _lib.LA_ST_WORDS > 0 and end - n > 0
    return eng.workspace[end - n:end].view(torch.float32)


def long_context_walk(cm, dtype, start, stop, st, seed=0):
    """ONE generation from `start` to past `stop` keys (no reset): verify_only on a 64-row tree + commit of 1 .. 64 rows, a census at
    every step.  -> [(n_keys, split partials written so far)] per step: what the ENGINE reports about the graph it replayed."""
    eng = LlamaVerifyEngine(cm.shape(), cm.weights(dtype), max_length=stop + 128)
    rs = np.random.RandomState(seed)
    toks = np.arange(cm.vocab)
    keys = rs.randint(0, cm.vocab, size=start).tolist()
    eng.prefill(keys)
    seen = []
    commits = (1, 64, 17, 33, 63, 2, 48, 31)
    i = 0
    while len(keys) <= stop:
        ids, rm = _tree(rs, 64, toks)
        eng.verify_only(ids, rm, eager=(i % 5 == 4))
        seen.append((len(keys), bool(_split_partials_tail(eng).abs().max() > 0)))
        _check_single(cm, eng, keys, ids, rm, f'long context {cm.nh}/{cm.nkv} {dtype} nkeys {len(keys)}', st)
        n = commits[i % len(commits)]
        rows = [0] + sorted(int(r) for r in 1 + rs.permutation(63)[:n - 1])
        eng.commit(rows)
        keys += [int(ids[r]) for r in rows]
        i += 1
    del eng
    torch.cuda.empty_cache()
    return seen


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('nh,nkv,start,stop', [(32, 32, 1000, 1700), (32, 8, 1000, 1700), (40, 40, 800, 1400)])
def test_product_head_counts_across_the_long_context_switch(nh, nkv, start, stop, dtype):
    """One-layer census models at the product head counts.  The single-sequence step replays the single-launch attention while
    n_keys + 64 <= attn_thr = 2800000 / (ceil(n_kv / 8) * 512) (1367 at 32 kv heads, 1093 at 40) and the key-split graph past it: the walk
    crosses that point inside one generation; where it crosses is read from the split partials the engine leaves (lpart stays zero
    until k_tree_attn runs), not from this formula.  At 8 kv heads the threshold is 5468 keys: this walk stays on the single-launch form of
    the GQA block-id map (the Mistral-window test below goes past 5468)."""
    cm = CensusModel(nh, nkv)
    st = CensusStats(f'product heads {nh}/{nkv} ({cm.layout}) {start} -> {stop} keys {dtype}')
    seen = long_context_walk(cm, dtype, start, stop, st)
    split = [n for n, wrote in seen if wrote]
    single = [n for n, wrote in seen if not wrote]
    print(f'[census] {nh}/{nkv} {dtype}: single-launch steps at {single[:1]}..{single[-1:]} keys, key-split partials from {split[:1]} keys on')
    if nkv >= 32:
        # the engine's own evidence of the switch: no split partials while the single-launch graph runs, partials from the first
        # step past the threshold; at least four census steps on each side, in one generation
        assert len(single) >= 4 and len(split) >= 4 and max(single) < min(split), seen
        assert 900 < min(split) < stop - 200, seen
    else:
        assert not split, seen
    print(st)
    assert st.worst < BAR


@pytest.mark.parametrize('dtype', DTYPES)
def test_two_layer_random_model_32_heads_context_1500_vs_oracle(dtype):
    """A two-layer random-weight model at 32 / 32 heads (head_dim 128; hidden / ffn / vocab small: only the head count matters to the
    attention forms) from 1250 to 1500+ keys in one generation: logits against the oracle at every step, on both sides of the switch
    to the key-split graph, under the bar of test_gpu_e2e.py"""
    from tests.test_gpu_e2e import TOL, _check_rows as check_logits, _mask_from_rows
    shape = LlamaShape(2, 1024, 32, 32, 2048, 2048, 1e-5, head_dim=128)
    sd = random_weights(shape, seed=5, std=0.02, device='cpu', dtype=dtype)
    eng = LlamaVerifyEngine(shape, sd, max_length=1700)
    oracle = lo.OracleLlama(shape, sd)
    rs = np.random.RandomState(15)
    P = 1250
    prompt = rs.randint(3, shape.vocab, size=P).tolist()
    eng.prefill(prompt)
    _, past = oracle.forward(torch.tensor(prompt), torch.tril(torch.ones((P, P), dtype=torch.long)), None)
    nk, sides = P, set()
    while nk < 1500 + 40:
        T = 64
        _, rows = random_tree(rs, T)
        ids = rs.randint(3, shape.vocab, size=T).astype(np.int32)
        eng.verify_only(ids, rows)
        full = torch.cat([torch.ones((T, nk), dtype=torch.long), torch.from_numpy(_mask_from_rows(rows, T))], 1)
        lg, new_past = oracle.forward(torch.tensor(ids.tolist()), full, past)
        check_logits(eng.logits(), lg, range(T), f'32-head model at {nk} keys', tol=TOL)
        sides.add(nk + 64 > 1367)
        keep = [0] + sorted(int(r) for r in 1 + rs.permutation(T - 1)[:39])
        eng.commit(keep)
        idx = torch.tensor(list(range(nk)) + [nk + r for r in keep], dtype=torch.long)
        past = [(k[:, idx], v[:, idx]) for k, v in new_past]
        nk += len(keep)
        assert eng.n_keys == nk
    assert sides == {False, True}
    del eng
    torch.cuda.empty_cache()


# ================================================================================================ the real Mistral window
@pytest.mark.parametrize('kv_ring', [False, True])
@pytest.mark.parametrize('dtype', DTYPES)
def test_mistral_window_4096_single_step_and_eight_blocks(dtype, kv_ring):
    """32 / 8 heads, sliding_window 4096 (BASELINE config 3), with the O(window) ring and without: the context grows past 9400
    positions (two laps of the 4672-key ring) through mprefill chains of 512 tokens; a dozen stops, at each a single-sequence step
    (past 5404 keys: on the key-split graph) and an 8-block mstep over 8 slots of unequal contexts"""
    cm = CensusModel(32, 8, window=4096)
    st = CensusStats(f'Mistral window 4096 ring {kv_ring} {dtype}')
    sd = cm.weights(dtype)
    e1 = LlamaVerifyEngine(cm.shape(), sd, max_length=10200, n_slots=1, max_blocks=8, kv_ring=kv_ring)
    e8 = LlamaVerifyEngine(cm.shape(), sd, max_length=10200, n_slots=8, max_blocks=8, kv_ring=kv_ring)
    rs = np.random.RandomState(77)
    toks = np.arange(cm.vocab)
    keys1, keys8 = [], [[] for _ in range(8)]
    lead = [int(x) for x in rs.randint(1, 300, size=8)]                    # unequal contexts
    for stop in range(12):
        grow = rs.randint(0, cm.vocab, size=790 + stop).tolist()
        e1.prefill(grow)
        keys1 += grow
        ids, rm = _tree(rs, SIZES[stop % len(SIZES)], toks)
        e1.verify_only(ids, rm, eager=(stop % 4 == 3))
        _check_single(cm, e1, keys1, ids, rm, f'Mistral single step at {len(keys1)} keys', st)
        for s in range(8):
            more = rs.randint(0, cm.vocab, size=790 + stop + (lead[s] if stop == 0 else 0)).tolist()
            e8.mprefill(s, more)
            keys8[s] += more
        blocks = [(s, *_tree(rs, SIZES[(s + stop) % len(SIZES)], toks), 2, 16) for s in range(8)]
        e8.mstep(blocks)
        for b, (s, ids, rm, _, _) in enumerate(blocks):
            assert e8.slot_keys[s] == len(keys8[s])
            # at most 4160 visible keys over 1024 classes: the histogram helper asserts every count <= 32
            _check_rows(cm, e8.mhidden()[64 * b:64 * b + len(ids)], keys8[s], ids, [int(x) for x in rm],
                        f'Mistral mstep block {b} at {len(keys8[s])} keys', st)
    assert len(keys1) > 9400 and min(len(k) for k in keys8) > 9400
    if kv_ring:
        assert len(keys1) >= 2 * e1.max_keys and e8.max_keys == 4672
    print(st)
    assert st.worst < BAR
    del e1, e8
    torch.cuda.empty_cache()
