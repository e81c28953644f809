# -*- coding: utf-8 -*-
"""MoE routing census on the MI355X (pytest -m gpu): every step path runs the census model of tests/moe_census.py, and the residual
stream it leaves (engine.hidden() / engine.mhidden()) and the routing weights (route_weights() / mroute_weights()) are compared for
EQUALITY with the rule MoeCensusModel.expected — an exact statement of which experts ran on which row, with what weight, folded in
what order.  Product libraries (bf16 and fp16) throughout; the lab forms run on the lab build.  Every test prints one [moe census] line:
the live rows, (row, expert) cells and routing weights it checked (pytest -s)."""
import functools

import numpy as np
import pytest
import torch

from oracle.tiny import random_tree
from painlessinferenceacceleration_amd.llama_engine import LlamaVerifyEngine
from tests import gpu_utils as gu
from tests.moe_census import MoeCensusModel, MoeCensusStats, census_check

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
SHAPES = [(8, 2), (8, 1), (8, 4), (4, 3), (2, 2), (1, 1), (8, 5), (8, 8)]      # (8, 5), (8, 8): the per-expert loop on the 64-row step
C_WIDE = 384                                                                     # classes of the multi-block models: up to 384 live rows

# Planted rows per WINDOW group j (experts j .. j + top_k - 1 mod E) and the rows per expert they add up to: the 64-row block edges of
# the gathered path (0, 1, 63, 64, 65, 128, 129 rows), expert 0 receiving nothing wherever the shape allows it
PLANTS = {
    (8, 2): ([0, 1, 62, 2, 63, 65, 64, 0], [0, 1, 63, 64, 65, 128, 129, 64]),
    (8, 1): ([0, 1, 63, 64, 65, 0, 0, 0], [0, 1, 63, 64, 65, 0, 0, 0]),
    (8, 4): ([0, 1, 62, 1, 64, 0, 0, 0], [0, 1, 63, 64, 128, 127, 65, 64]),
    (4, 3): ([0, 65, 0, 0], [0, 65, 65, 65]),
    (2, 2): ([129], [129, 129]),
    (1, 1): ([129], [129]),
    (8, 5): ([0, 1, 63, 65, 0, 0, 0, 0], [0, 1, 64, 129, 129, 129, 128, 65]),
    (8, 8): ([129], [129] * 8),
}


@functools.lru_cache(maxsize=2)
def _model(E, top_k, dtype, C=128, layers=1):
    plant = PLANTS[(E, top_k)][0] if C == C_WIDE else None
    cm = MoeCensusModel(E, top_k, dtype, C=C, plant=plant, layers=layers)
    return cm, cm.weights()


def _engine(cm, sd, **kw):
    return LlamaVerifyEngine(cm.shape(), dict(sd), max_length=512, **kw)


def _rows(rs, T):
    return np.asarray(random_tree(rs, T)[1], dtype=np.uint64)


def _split(R, nblk):
    """R rows over nblk blocks of 1 .. 64 rows: full blocks first"""
    assert nblk <= R <= 64 * nblk
    sizes, left = [1] * nblk, R - nblk
    for i in range(nblk):
        add = min(63, left)
        sizes[i] += add
        left -= add
    return sizes


def _check_single(cm, eng, tokens, what, st):
    """the last 64-row block of the single-sequence / cursor-batch step: len(tokens) live rows, dead rows after them"""
    census_check(cm, eng.hidden(), eng.route_weights(), tokens, what, st, n_dead=64 - len(tokens))


def _check_blocks(cm, eng, per_block, what, st):
    h, rw = eng.mhidden(), eng.mroute_weights()
    for b, toks in enumerate(per_block):
        census_check(cm, h[64 * b:64 * b + 64], rw[:, 64 * b:64 * b + 64], toks, f'{what} block {b} (T {len(toks)})', st, n_dead=64 - len(toks))


def _mstep(cm, eng, rs, tokens, sizes, what, st, eager=False):
    """one forward-only multi-block pass: block b = sizes[b] of `tokens` as a random tree of slot b"""
    assert sum(sizes) == len(tokens)
    per_block, blocks, at = [], [], 0
    for b, T in enumerate(sizes):
        per_block.append(tokens[at:at + T])
        blocks.append((b, tokens[at:at + T], _rows(rs, T), 2, 16))
        at += T
    eng.mstep(blocks, eager=eager)
    _check_blocks(cm, eng, per_block, f'{what} nblk {len(sizes)} eager {eager}', st)


# ================================================================================================ 64-row step, cursor batch
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('E,top_k', SHAPES)
def test_single_sequence_step_and_cursor_batch(E, top_k, dtype):
    """prefill (two chains: 64 + 6 rows), then step / verify_only at T = 1, 33, 64, graph and eager; a step that leaves expert 0 idle; bstep
    with 4 slots sharing the block; (8, 2): balanced and classic GEMM grids"""
    cm, sd = _model(E, top_k, dtype)
    st = MoeCensusStats(f'step + bstep E {E} top_k {top_k} {dtype}')
    rs = np.random.RandomState(100 * E + top_k)
    for balanced in ((True, False) if (E, top_k) == (8, 2) else (True,)):
        eng = _engine(cm, sd, balanced=balanced)
        what = f'E {E} top_k {top_k} {dtype} balanced {balanced}'
        prompt = cm.draw_mixed(rs, 70)
        eng.prefill(prompt.tolist())
        _check_single(cm, eng, prompt[64:], f'prefill tail, {what}', st)
        for i, T in enumerate((1, 33, 64, 64, 33, 1)):
            eager = i >= 3
            tokens = cm.draw_mixed(rs, T)
            if i % 2:
                eng.verify_only(tokens, _rows(rs, T), eager=eager)
            else:
                eng.step(tokens, _rows(rs, T), eager=eager)
            _check_single(cm, eng, tokens, f'step T {T} eager {eager}, {what}', st)
        if top_k < E:
            # expert 0 receives nothing (the window groups that do not hold it): on the per-expert loop of top_k > 4 the FIRST launch,
            # which zero-fills the accumulator, then has no row of its own
            tokens = cm.draw(rs, {j: 8 for j in range(E) if 0 not in [(j + i) % E for i in range(top_k)]})
            assert cm.expert_counts(tokens)[0] == 0 and len(tokens) >= 8
            for eager in (False, True):
                eng.verify_only(tokens, _rows(rs, len(tokens)), eager=eager)
                _check_single(cm, eng, tokens, f'expert 0 idle, eager {eager}, {what}', st)
        del eng
        eng = _engine(cm, sd, balanced=balanced, n_slots=4)
        eng.bprefill_many({slot: cm.draw_mixed(rs, 3 + 2 * slot).tolist() for slot in range(4)})
        for i, sizes in enumerate(((20, 1, 30, 13), (17, 5), (1, 1, 1, 1))):
            tokens = cm.draw_mixed(rs, sum(sizes))
            segs, at = [], 0
            for slot, n in enumerate(sizes):
                segs.append((slot, tokens[at:at + n], _rows(rs, n), 2, 16))
                at += n
            eng.bstep(segs, eager=(i == 1))
            _check_single(cm, eng, tokens, f'bstep {sizes}, {what}', st)
        del eng
        torch.cuda.empty_cache()
    print(st)


# ================================================================================================ multi-block step
def _multi_block_walk(cm, sd, st, what, balanced=True, nblks=(1, 2, 3, 5, 8), planted=True):
    E, top_k = cm.E, cm.k
    eng = _engine(cm, sd, balanced=balanced, n_slots=8, max_blocks=8)
    rs = np.random.RandomState(1000 + 10 * E + top_k)
    # mprefill chain, P = 130: blocks of 64, 64 and 2 rows of slot 0 in one pass
    prompt = cm.draw_mixed(rs, 130)
    eng.mprefill(0, prompt.tolist())
    _check_blocks(cm, eng, [prompt[0:64], prompt[64:128], prompt[128:]], f'mprefill P 130, {what}', st)
    for s in range(1, 8):
        eng.mprefill(s, cm.draw_mixed(rs, 3 + s).tolist())
    mixes = {1: [(64,), (40,), (1,)], 2: [(64, 1), (40, 64)], 3: [(40, 64, 1)], 5: [(64, 40, 1, 64, 40)], 8: [(64, 40, 1, 64, 40, 1, 64, 40)]}
    for nblk in nblks:
        for i, sizes in enumerate(mixes[nblk]):
            for eager in (False, True):
                _mstep(cm, eng, rs, cm.draw_mixed(rs, sum(sizes)), list(sizes), what, st, eager=eager)
    if planted:
        # the planted counts: rows per window group as PLANTS says, in the fewest blocks of {2, 3, 5, 8} that hold them
        plant, counts = PLANTS[(E, top_k)]
        tokens = cm.draw(rs, {j: n for j, n in enumerate(plant) if n})
        assert cm.expert_counts(tokens) == counts, (cm.expert_counts(tokens), counts)
        nblk = min(n for n in (2, 3, 5, 8) if 64 * n >= len(tokens))
        for eager in (False, True):
            _mstep(cm, eng, rs, tokens, _split(len(tokens), nblk), f'planted {counts}, {what}', st, eager=eager)
        if top_k < E and E > 2:
            # all live rows at once: 128 rows that every one routes to expert x (the window groups x - top_k + 1 .. x hold it)
            x = max(range(E), key=lambda e: counts[e])
            pool = {j: plant[j] for j in range(E) if x in [(j + i) % E for i in range(top_k)] and plant[j]}
            tokens = cm.draw(rs, pool)
            if len(tokens) >= 128:
                tokens = tokens[:128]
                assert cm.expert_counts(tokens)[x] == 128
                _mstep(cm, eng, rs, tokens, [64, 64], f'all 128 live rows to expert {x}, {what}', st)
    # one wide tree: T = 100, two blocks of one slot
    T = 100
    masks, stack = [1], [0]
    for i in range(1, T):
        while len(stack) > 1 and rs.rand() < 0.3:
            stack.pop()
        masks.append(masks[stack[-1]] | (1 << i))
        stack.append(i)
    rm = np.array([[(m >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range(2)] for m in masks], dtype=np.uint64)
    tokens = cm.draw_mixed(rs, T)
    eng.mstep_trees([(3, tokens, rm, 2, 16)])
    _check_blocks(cm, eng, [tokens[:64], tokens[64:]], f'wide tree T 100, {what}', st)
    del eng
    torch.cuda.empty_cache()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('E,top_k', SHAPES)
def test_multi_block_step_prefill_chain_and_wide_tree(E, top_k, dtype):
    """mstep (graph and la_llama_mstep_eager) at 1 block (the ungathered form) and 2, 3, 5, 8 blocks (gathered, merged launches; top_k > 4:
    the per-expert launches) with 64, 40 and 1 rows per block — dead rows in every pass; the planted per-expert counts; the mprefill chain
    of 130 tokens; a 100-row tree through mstep_trees.  (8, 5) and (8, 8) route a row to more than four experts: every one of them must
    show in the row's lanes, on the multi-block paths as on the 64-row step."""
    cm, sd = _model(E, top_k, dtype, C=C_WIDE)
    st = MoeCensusStats(f'mstep + mprefill + wide tree E {E} top_k {top_k} {dtype}')
    _multi_block_walk(cm, sd, st, f'E {E} top_k {top_k} {dtype}')
    print(st)


@pytest.mark.parametrize('dtype', DTYPES)
def test_multi_block_step_on_the_classic_gemm_grids(dtype):
    """balanced=False on the (8, 2) shape"""
    cm, sd = _model(8, 2, dtype, C=C_WIDE)
    st = MoeCensusStats(f'mstep, classic grids, E 8 top_k 2 {dtype}')
    _multi_block_walk(cm, sd, st, f'E 8 top_k 2 {dtype} balanced False', balanced=False, nblks=(1, 2, 5))
    print(st)


# ================================================================================================ stale scratch
@pytest.mark.parametrize('dtype', DTYPES)
def test_no_stale_expert_scratch_after_a_step_that_routed_elsewhere(dtype):
    """A step that sends all of its 65 rows to experts {5, 6}, then a step on the same engine whose 3 rows go to {2, 3} and {3, 4}: the lane
    blocks of 5 and 6 must read exactly 0 (nothing of the first step's slabs, lists or positions survives), on the gathered form (2 blocks),
    the ungathered form (1 block) and the 64-row step."""
    cm, sd = _model(8, 2, dtype, C=C_WIDE)
    st = MoeCensusStats(f'stale scratch {dtype}')
    eng = _engine(cm, sd, n_slots=2, max_blocks=2)
    rs = np.random.RandomState(77)
    for s in range(2):
        eng.mprefill(s, cm.draw_mixed(rs, 5).tolist())
    for sizes_a, sizes_b in (((64, 1), (2, 1)), ((64,), (3,))):
        first = cm.draw(rs, {5: sum(sizes_a)})
        c = cm.expert_counts(first)
        assert c[5] == c[6] == sum(sizes_a) and sum(c) == 2 * sum(sizes_a)
        _mstep(cm, eng, rs, first, list(sizes_a), 'stale scratch, first step', st)
        second = cm.draw(rs, {2: 2, 3: 1})
        c = cm.expert_counts(second)
        assert c[5] == c[6] == 0 and c[2:5] == [2, 3, 1]
        _mstep(cm, eng, rs, second, list(sizes_b), 'stale scratch, second step', st)
    first, second = cm.draw(rs, {5: 64}), cm.draw(rs, {2: 2, 3: 1})
    eng.verify_only(first, _rows(rs, 64))
    _check_single(cm, eng, first, 'stale scratch, 64-row step, first', st)
    eng.verify_only(second, _rows(rs, 3))
    _check_single(cm, eng, second, 'stale scratch, 64-row step, second', st)
    print(st)
    del eng
    torch.cuda.empty_cache()


# ================================================================================================ layer indexing
@pytest.mark.parametrize('dtype', DTYPES)
def test_two_layers_per_layer_expert_pointers_and_route_weights(dtype):
    """Two layers: layer 0's experts have down = 0 (it adds nothing) behind a router table of its own; the census is read after layer 1 and the
    routing weights of BOTH layers are checked — the per-layer expert pointers, strides and the route_w offset."""
    cm, sd = _model(8, 2, dtype, C=C_WIDE, layers=2)
    assert not torch.equal(cm.w[0], cm.w[1])
    st = MoeCensusStats(f'two layers {dtype}')
    eng = _engine(cm, sd, n_slots=3, max_blocks=3)
    rs = np.random.RandomState(5)
    for s in range(3):
        eng.mprefill(s, cm.draw_mixed(rs, 4).tolist())
    for sizes in ((64,), (64, 40), (40, 64, 1)):
        _mstep(cm, eng, rs, cm.draw_mixed(rs, sum(sizes)), list(sizes), 'two layers', st)
    for T in (64, 33, 1):
        tokens = cm.draw_mixed(rs, T)
        eng.verify_only(tokens, _rows(rs, T))
        _check_single(cm, eng, tokens, f'two layers, step T {T}', st)
    print(st)
    del eng
    torch.cuda.empty_cache()


# ================================================================================================ lab forms
@pytest.mark.usefixtures('lab_build')
@pytest.mark.parametrize('knob,value', [(16, 1), (16, 4), (16, 5), (22, 1), (22, 2), (22, 4)])
def test_lab_forms_of_the_multi_block_moe_against_the_rule(knob, value):
    """la_lab_set key 16 (bit 0: per-expert launches + the unfused accumulate / norm pair; bit 2: plan and gather as two launches) and key 22
    (K splits of the gathered experts' down projection): the same mstep cases, each form against the RULE, not against another form"""
    cm, sd = _model(8, 2, torch.bfloat16, C=C_WIDE)
    st = MoeCensusStats(f'lab knob {knob} = {value}')
    with gu.debug_knob(knob, value):
        _multi_block_walk(cm, sd, st, f'knob {knob} = {value}')
    print(st)
