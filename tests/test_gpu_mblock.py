# -*- coding: utf-8 -*-
"""-m gpu: the multi-block step (la_llama_mstep / la_mb_gemm, csrc/la_mblock.hip) through the C ABI.

Every block of a multi-block step is one sequence's full 64-row verify block (or one 64-token piece of a prompt), so parity
is defined per sequence: block b of an M = 64*B row step must reproduce what the bs=1 oracle computes for that
sequence alone — logits within the tolerance of test_gpu_e2e.py (2e-2 * max|logit| per row, argmax wherever the gap is
decisive), accept walk / commit plan / cursors bit-exact given the device's argmax rows."""
import os

import numpy as np
import pytest
import torch

from oracle import llama_oracle as lo
from painlessinferenceacceleration_amd import _lib
from painlessinferenceacceleration_amd._lib import check, lib
from painlessinferenceacceleration_amd.llama_engine import LlamaShape, LlamaVerifyEngine, random_weights, rope_tables
from tests import gpu_utils as gu
from tests.gpu_utils import DEV, ptr, random_tree, sp
from tests.test_gpu_e2e import TOL, _bf16_sd, _check_rows, _mask_from_rows
from tests.tiny_model import tiny_shape

pytestmark = pytest.mark.gpu

# ONE tolerance: the stated 2e-2 of max|logit| per row (TOL, tests/test_gpu_e2e.py), asserted for every row of every layer-shape test
# (7B / 13B / Mistral / Mixtral slices).  On the TINY seeded model (hidden 256, weights std 0.08, ~3-ulp top-2 gaps) two CORRECT bf16
# summation orders are themselves 0.021-0.022 apart in the tail: measured on MI355X over 15 prompts (scripts/gpu_mb_diag.py) the 64-row path
# AND the multi-block path sit at max 0.0211 / 0.0221 of max|logit| from the bf16 CPU oracle (mean 0.012 both, < 2 % of rows above 2e-2) and
# within 0.013 of each other.  So the tiny-model checks of this file keep TOL per row and allow a TAIL: at most TAIL_FRAC of a check's rows
# between TOL and TOL_TAIL, none beyond — instead of a second, looser tolerance.
TOL_TAIL = 3e-2
TAIL_FRAC = 0.10
TINY = dict(tol=TOL, tail_tol=TOL_TAIL, tail_frac=TAIL_FRAC)


def bf(t):
    return t.to(torch.bfloat16)


def _pack_blocks(x):
    """[nblk*64][K] -> nblk consecutive 64-row XP images"""
    return torch.cat([gu.pack_x(x[b * 64:(b + 1) * 64].contiguous()) for b in range(x.shape[0] // 64)])


def _mb(kind, wp, xp, N, K, nblk, n_wg=0, ksplit=1, slabs=None, slab_rows=0, act=None, logits=None, cv=None, ci=None, pos=None,
        rc=None, rs_=None, qf=None, kf=None, vf=None, nh=0, nkv=0):
    check(lib.la_mb_gemm(sp(), kind, ptr(wp), ptr(xp), N, K, nblk, n_wg, ksplit, ptr(slabs), slab_rows, ptr(act), ptr(logits), ptr(cv),
                         ptr(ci), ptr(pos), ptr(rc), ptr(rs_), ptr(qf), ptr(kf), ptr(vf), nh, nkv), 'mb_gemm')
    torch.cuda.synchronize()


@pytest.mark.parametrize('nblk', [1, 2, 3, 4, 8])
@pytest.mark.parametrize('N,K,ks', [(256, 512, 1), (4096, 1376, 4), (512, 11008, 4)])
def test_mb_slab_gemm(nblk, N, K, ks):
    g = torch.Generator(device=DEV).manual_seed(N + nblk)
    x = bf(torch.randn(nblk * 64, K, generator=g, device=DEV))
    w = bf(torch.randn(N, K, generator=g, device=DEV) * 0.05)
    rows = (nblk if nblk <= 2 else (nblk + 3) // 4 * 4) * 64
    slabs = torch.full((ks, rows, N), float('nan'), dtype=torch.float32, device=DEV)
    _mb(0, gu.pack_weight(w), _pack_blocks(x), N, K, nblk, ksplit=ks, slabs=slabs, slab_rows=rows)
    got = slabs[:, :nblk * 64].sum(0)
    ref = x.double() @ w.double().t()
    assert gu.rel_err(got, ref) < 2e-3, gu.rel_err(got, ref)


@pytest.mark.parametrize('nblk', [1, 2, 4, 5, 8])
@pytest.mark.parametrize('F,K,nwg', [(512, 256, 0), (11008, 512, 256), (688, 512, 16), (13824, 1024, 256)])
def test_mb_swiglu_gemm_planned_and_classic(nblk, F, K, nwg):
    g = torch.Generator(device=DEV).manual_seed(F + nblk)
    x = bf(torch.randn(nblk * 64, K, generator=g, device=DEV))
    wg = bf(torch.randn(F, K, generator=g, device=DEV) * 0.05)
    wu = bf(torch.randn(F, K, generator=g, device=DEV) * 0.05)
    wp = gu.pack_planned(1, [wg, wu], nwg) if nwg else gu.pack_weight(wg, wu)
    act = torch.zeros(8 * 64 * F, dtype=torch.bfloat16, device=DEV)
    _mb(1, wp, _pack_blocks(x), F, K, nblk, n_wg=nwg, act=act)
    for b in range(nblk):
        got = gu.from_packed(act[b * 64 * F:(b + 1) * 64 * F], gu.xp_index(F)).float()
        xb = x[b * 64:(b + 1) * 64].float()
        gg, uu = bf(xb @ wg.float().t()), bf(xb @ wu.float().t())
        ref = bf(bf(torch.nn.functional.silu(gg.float())).float() * uu.float()).float()
        assert gu.rel_err(got, ref) < 2e-2, (b, gu.rel_err(got, ref))
        assert float((got != ref).float().mean()) < 0.02


@pytest.mark.parametrize('nblk', [1, 3, 4, 8])
@pytest.mark.parametrize('V,K,nwg', [(512, 256, 0), (32000, 512, 256)])
def test_mb_logits_gemm_and_argmax(nblk, V, K, nwg):
    g = torch.Generator(device=DEV).manual_seed(V + nblk)
    x = bf(torch.randn(nblk * 64, K, generator=g, device=DEV))
    w = bf(torch.randn(V, K, generator=g, device=DEV) * 0.05)
    wp = gu.pack_planned(0, [w], nwg) if nwg else gu.pack_weight(w)
    n_tiles = 4 * (nwg if nwg else V // 128)
    logits = torch.zeros(8 * 64, V, dtype=torch.bfloat16, device=DEV)
    cv = torch.zeros(8 * n_tiles * 64, dtype=torch.float32, device=DEV)
    ci = torch.zeros(8 * n_tiles * 64, dtype=torch.int32, device=DEV)
    _mb(3, wp, _pack_blocks(x), V, K, nblk, n_wg=nwg, logits=logits, cv=cv, ci=ci)
    lg = logits[:nblk * 64].float()
    assert gu.rel_err(lg, x.double() @ w.double().t()) < 1e-2
    # argmax candidates reduce to the first maximum of the stored bf16 row (torch.argmax tie rule on CPU)
    cvv = cv.view(8, n_tiles, 64)[:nblk].cpu()
    cii = ci.view(8, n_tiles, 64)[:nblk].cpu()
    lf = lg.cpu()
    for b in range(nblk):
        for t in range(0, 64, 7):
            row = lf[b * 64 + t]
            best = float(row.max())
            exp = int((row == best).nonzero()[0])
            cand = [(float(cvv[b, i, t]), int(cii[b, i, t])) for i in range(n_tiles)]
            mv = max(c[0] for c in cand)
            assert mv == best and min(c[1] for c in cand if c[0] == mv) == exp


@pytest.mark.parametrize('nblk', [1, 2, 4, 6, 8])
@pytest.mark.parametrize('nh,nkv,nwg', [(2, 2, 0), (32, 32, 256), (8, 2, 32), (40, 40, 256), (32, 8, 256)])
def test_mb_qkv_gemm_equals_single_block_kernel(nblk, nh, nkv, nwg):
    """Fragments written by the multi-block QKV launch == the single-block balanced / classic kernel run per block (same
    rounding points; the fp32 sums differ by the K split, so a small fraction of elements moves by one bf16 ulp)."""
    K = 512
    N = (nh + 2 * nkv) * 128
    g = torch.Generator(device=DEV).manual_seed(nh * 7 + nkv + nblk)
    x = bf(torch.randn(nblk * 64, K, generator=g, device=DEV))
    w = bf(torch.randn(N, K, generator=g, device=DEV) * 0.05)
    pos = torch.randint(0, 900, (nblk * 64,), generator=g, device=DEV, dtype=torch.int32)
    rc, rs_ = rope_tables(128, 1024, 10000.0, DEV)
    if nwg:
        wp = gu.pack_planned(2, [w], nwg)
    else:
        perm = np.zeros(N, dtype=np.int32)
        check(lib.la_qkv_row_perm(nh, nkv, perm.ctypes.data_as(_lib.pi32)), 'perm')
        wp = gu.pack_weight(w[torch.from_numpy(perm.astype(np.int64)).to(DEV)].contiguous())
    qf = torch.zeros(8 * nh * 8192, dtype=torch.bfloat16, device=DEV)
    kf = torch.zeros(8 * nkv * 8192, dtype=torch.bfloat16, device=DEV)
    vf = torch.zeros(8 * nkv * 8192, dtype=torch.bfloat16, device=DEV)
    xp = _pack_blocks(x)
    _mb(2, wp, xp, N, K, nblk, n_wg=nwg, pos=pos, rc=rc, rs_=rs_, qf=qf, kf=kf, vf=vf, nh=nh, nkv=nkv)
    for b in range(nblk):
        q1 = torch.zeros(nh * 8192, dtype=torch.bfloat16, device=DEV)
        k1 = torch.zeros(nkv * 8192, dtype=torch.bfloat16, device=DEV)
        v1 = torch.zeros(nkv * 8192, dtype=torch.bfloat16, device=DEV)
        xb = xp[b * 64 * K:(b + 1) * 64 * K]
        pb = pos[b * 64:(b + 1) * 64].contiguous()
        if nwg:
            check(lib.la_gemm64r_qkv(sp(), ptr(wp), ptr(xb), nh, nkv, K, nwg, ptr(pb), ptr(rc), ptr(rs_), ptr(q1), ptr(k1), ptr(v1)), 'qkv_r')
        else:
            check(lib.la_gemm64_qkv(sp(), ptr(wp), ptr(xb), nh, nkv, K, ptr(pb), ptr(rc), ptr(rs_), ptr(q1), ptr(k1), ptr(v1), 0), 'qkv')
        torch.cuda.synchronize()
        for a, ref, name in ((qf[b * nh * 8192:(b + 1) * nh * 8192], q1, 'q'), (kf[b * nkv * 8192:(b + 1) * nkv * 8192], k1, 'k'),
                             (vf[b * nkv * 8192:(b + 1) * nkv * 8192], v1, 'v')):
            assert gu.rel_err(a.float(), ref.float()) < 1e-2, (b, name)
            assert float((a != ref).float().mean()) < 0.02, (b, name)


def _oracle_seq(oracle, prompt):
    P = len(prompt)
    lg, past = oracle.forward(torch.tensor(prompt), torch.tril(torch.ones((P, P), dtype=torch.long)), None)
    return lg, past


@pytest.mark.parametrize('B', [2, 4, 5, 8])
def test_mstep_every_block_matches_its_bs1_oracle_run(B):
    """B sequences with different prompt lengths, each with its own 64-row random tree in ONE multi-block step: logits of
    block b vs the oracle run on sequence b alone, accept walk and commit plan bit-exact given the device argmax, then a second
    step on the committed caches (checks the KV rows the first step kept)."""
    shape = tiny_shape()
    sd = _bf16_sd(1)
    eng = LlamaVerifyEngine(shape, sd, max_length=384, n_slots=B, max_blocks=B)
    oracle = lo.OracleLlama(shape, sd)
    rs = np.random.RandomState(B)
    prompts = [rs.randint(3, shape.vocab, size=int(rs.randint(5, 150))).tolist() for _ in range(B)]
    pasts, nk = [], []
    for b, p in enumerate(prompts):
        tok = eng.mprefill(b, p)
        lg, past = _oracle_seq(oracle, p)
        _check_rows(eng.mlogits()[((len(p) - 1) // 64 % eng.max_blocks) * 64:][:(len(p) - 1) % 64 + 1],
                    lg[(len(p) - 1) // 64 * 64:], range((len(p) - 1) % 64 + 1), f'prefill {b}', **TINY)
        assert eng.slot_keys[b] == len(p)
        pasts.append(past)
        nk.append(len(p))
        prompts[b] = p + [tok]
    for step in range(2):
        blocks, trees = [], []
        for b in range(B):
            T = int(rs.randint(1, 65)) if b else 64
            _, rows = random_tree(rs, T)
            ids = np.concatenate([[prompts[b][-1]], rs.randint(3, shape.vocab, size=T - 1)]).astype(np.int32)
            blocks.append((b, ids, rows, 0, 16))
            trees.append((ids, rows, T))
        outs = eng.mstep(blocks, eager=(step == 1))
        mo = eng.mout().cpu().numpy()
        for b in range(B):
            ids, rows, T = trees[b]
            mask = _mask_from_rows(rows, T)
            full = torch.cat([torch.ones((T, nk[b]), dtype=torch.long), torch.from_numpy(mask)], 1)
            lg, past_all = oracle.forward(torch.tensor(ids.tolist()), full, pasts[b])
            _check_rows(eng.mlogits()[b * 64:b * 64 + T], lg, range(T), f'step {step} block {b}', **TINY)
            am = mo[_lib.LA_MOUT_ARGMAX + 64 * b:_lib.LA_MOUT_ARGMAX + 64 * b + T].tolist()
            exp_toks, exp_rows = lo.accept_scan(ids.tolist(), mask, am)
            exp_toks, exp_rows = exp_toks[:16], exp_rows[:16]
            assert outs[b] == exp_toks, (step, b)
            dst = mo[_lib.LA_MOUT_DST + 64 * b:_lib.LA_MOUT_DST + 64 * b + 64]
            want = np.full(64, -1, dtype=np.int64)
            for d, r in enumerate(exp_rows):
                want[r] = b * eng.max_keys + nk[b] + d
            assert dst.tolist() == want.tolist(), (step, b)
            keep = list(range(nk[b])) + [nk[b] + r for r in exp_rows]
            idx = torch.tensor(keep, dtype=torch.long)
            pasts[b] = [(k[:, idx], v[:, idx]) for k, v in past_all]
            nk[b] += len(exp_rows)
            assert eng.slot_keys[b] == nk[b]
            prompts[b] = prompts[b] + exp_toks


@pytest.mark.parametrize('P', [64, 130, 512, 700])
def test_mprefill_chain_equals_oracle_and_feeds_the_single_sequence_step(P):
    """A prompt as ONE chain of 64-row blocks per pass (blocks see the fresh keys of the earlier blocks of the chain), then a
    tree step on the classic single-sequence path on top of the cache the chain committed."""
    shape = tiny_shape()
    sd = _bf16_sd(2)
    eng = LlamaVerifyEngine(shape, sd, max_length=1024, n_slots=1, max_blocks=8)
    oracle = lo.OracleLlama(shape, sd)
    rs = np.random.RandomState(P)
    prompt = rs.randint(3, shape.vocab, size=P).tolist()
    tok = eng.mprefill(0, prompt)
    lg, past = _oracle_seq(oracle, prompt)
    last = (P - 1) // 64
    nb_last_pass = last % 8
    rows = (P - 1) % 64 + 1
    _check_rows(eng.mlogits()[nb_last_pass * 64:nb_last_pass * 64 + rows], lg[last * 64:], range(rows), 'chain', **TINY)
    top = torch.topk(lg[-1].float(), 2).values
    if float(top[0] - top[1]) > 4 * TOL * float(lg[-1].float().abs().max()):
        assert tok == int(lg[-1].float().argmax())
    assert eng.n_keys == P
    T = 64
    _, trows = random_tree(rs, T)
    ids = np.concatenate([[tok], rs.randint(3, shape.vocab, size=T - 1)]).astype(np.int32)
    eng.step(ids, trows, mode=0)
    full = torch.cat([torch.ones((T, P), dtype=torch.long), torch.from_numpy(_mask_from_rows(trows, T))], 1)
    lg2, _ = oracle.forward(torch.tensor(ids.tolist()), full, past)
    _check_rows(eng.logits(), lg2, range(T), 'tree after chain', **TINY)


def test_mstep_llama7b_layer_shapes_vs_oracle():
    """Two layers at the Llama-2-7B layer shape (balanced weight images, K = 4096 / 11008), 4 sequences x 64 rows."""
    shape = LlamaShape(2, 4096, 32, 32, 11008, 32000, 1e-5)
    sd = random_weights(shape, seed=5, device='cpu')
    eng = LlamaVerifyEngine(shape, sd, max_length=256, n_slots=4, max_blocks=4)
    assert all(eng.balanced_wg), eng.balanced_wg
    oracle = lo.OracleLlama(shape, sd)
    rs = np.random.RandomState(3)
    blocks, refs = [], []
    for b in range(4):
        p = rs.randint(3, shape.vocab, size=int(rs.randint(20, 100))).tolist()
        tok = eng.mprefill(b, p)
        _, past = _oracle_seq(oracle, p)
        T = 64 if b == 0 else int(rs.randint(8, 65))
        _, rows = random_tree(rs, T)
        ids = np.concatenate([[tok], rs.randint(3, shape.vocab, size=T - 1)]).astype(np.int32)
        blocks.append((b, ids, rows, 0, 16))
        full = torch.cat([torch.ones((T, len(p)), dtype=torch.long), torch.from_numpy(_mask_from_rows(rows, T))], 1)
        refs.append((oracle.forward(torch.tensor(ids.tolist()), full, past)[0], T))
    eng.mstep(blocks)
    for b, (lg, T) in enumerate(refs):
        _check_rows(eng.mlogits()[b * 64:b * 64 + T], lg, range(T), f'7B-shape block {b}')


def test_mstep_mixtral_blocks_track_the_64_row_path():
    """Sparse-MoE MLP in the multi-block step (router fused into the post-attention norm over M rows, per-expert GEMMs over all
    rows with the skip for unused experts, weighted accumulation in expert order): every block of a 3-sequence step must track
    the 64-row engine path run on that sequence alone.  The two paths share every rounding point but sum K in a different
    order, so a near-tie router row may flip an expert (tests/test_gpu_moe.py): the bulk of the rows sits at bf16 noise and the
    routing weights agree on almost all (row, layer) pairs."""
    from tests.tiny_model import moe_shape, moe_weights, TINY_MOE
    shape = moe_shape(TINY_MOE)
    sd = {k: v.to(torch.bfloat16) for k, v in moe_weights(TINY_MOE, seed=3).items()}
    B = 3
    engm = LlamaVerifyEngine(shape, dict(sd), max_length=256, n_slots=B, max_blocks=B)
    eng1 = LlamaVerifyEngine(shape, dict(sd), max_length=256)
    rs = np.random.RandomState(8)
    blocks, refs = [], []
    for b in range(B):
        p = rs.randint(3, shape.vocab, size=int(rs.randint(10, 90))).tolist()
        eng1.reset()
        tok1 = eng1.prefill(p, fast=False)
        tokm = engm.mprefill(b, p)
        T = int(rs.randint(20, 65))
        _, rows = random_tree(rs, T)
        ids = np.concatenate([[tok1], rs.randint(3, shape.vocab, size=T - 1)]).astype(np.int32)
        eng1.step(ids, rows, mode=2)
        refs.append((eng1.logits()[:T].float().cpu().clone(), T, tok1 == tokm))
        blocks.append((b, ids, rows, 0, 16))
    engm.mstep(blocks)
    agree = []
    for b, (ref, T, same_first) in enumerate(refs):
        got = engm.mlogits()[b * 64:b * 64 + T].float().cpu()
        err = (got - ref).abs().max(1).values / ref.abs().max(1).values
        agree.append(float((err < TOL).float().mean()))
        assert float(err.median()) < TOL, (b, err)
    assert np.mean(agree) >= 0.8, agree


def test_mstep_moe_every_expert_receives_every_row():
    """Gathered MoE worst case: 2 experts, top-2 -> each expert's list is ALL rows of the step (4 blocks = two 128-row passes of
    the expert GEMMs, positions == rows).  No routing decision can flip here, so every block must sit at bf16 noise of the 64-row
    engine path run on that sequence alone."""
    from tests.tiny_model import moe_shape, moe_weights, TINY_MOE
    cfg = dict(TINY_MOE, n_experts=2, top_k=2)
    shape = moe_shape(cfg)
    sd = {k: v.to(torch.bfloat16) for k, v in moe_weights(cfg, seed=5).items()}
    B = 4
    engm = LlamaVerifyEngine(shape, dict(sd), max_length=256, n_slots=B, max_blocks=B)
    eng1 = LlamaVerifyEngine(shape, dict(sd), max_length=256)
    rs = np.random.RandomState(11)
    blocks, refs = [], []
    for b in range(B):
        p = rs.randint(3, shape.vocab, size=int(rs.randint(10, 90))).tolist()
        eng1.reset()
        tok1 = eng1.prefill(p, fast=False)
        engm.mprefill(b, p)
        T = 64 if b == 0 else int(rs.randint(20, 65))
        _, rows = random_tree(rs, T)
        ids = np.concatenate([[tok1], rs.randint(3, shape.vocab, size=T - 1)]).astype(np.int32)
        eng1.step(ids, rows, mode=2)
        refs.append((eng1.logits()[:T].float().cpu().clone(), T))
        blocks.append((b, ids, rows, 0, 16))
    engm.mstep(blocks)
    for b, (ref, T) in enumerate(refs):
        got = engm.mlogits()[b * 64:b * 64 + T].float().cpu()
        err = (got - ref).abs().max(1).values / ref.abs().max(1).values
        assert float((err < TOL).float().mean()) >= 1.0 - TAIL_FRAC and float(err.max()) < TOL_TAIL and float(err.median()) < 0.75 * TOL, (b, err)


@pytest.mark.usefixtures('lab_build')
@pytest.mark.parametrize('nblk', [2, 3, 4, 5, 7, 8])
def test_mb_paired_wide_form_is_bitwise_the_unpaired_one(nblk):
    """la_debug_set key 6: the slab and QKV launches of the wide family with TWO weight regions x HALF the token blocks per
    workgroup (RBV = 4 wave grid, grid.z = token halves).  Every output element is the same chain of MFMAs over the same operands
    in the same order, so slabs and Q / K / V fragments must equal the unpaired launch bit for bit — classic and planned images,
    MHA and GQA shapes, K splits."""
    rc, rs_ = rope_tables(128, 1024, 10000.0, DEV)
    default_form = lib.la_lab_get(6)
    try:
        for N, K, ks in ((4096, 1376, 4), (512, 2048, 1), (5120, 512, 4)):
            g = torch.Generator(device=DEV).manual_seed(N + nblk)
            x = bf(torch.randn(nblk * 64, K, generator=g, device=DEV))
            wp = gu.pack_weight(bf(torch.randn(N, K, generator=g, device=DEV) * 0.05))
            rows = (nblk + 3) // 4 * 4 * 64
            outs = []
            for pair in (0, 1, 33, 33 + 8192 + 16384, 1025):   # 24609 = the fat slab launch with one K split per XCD on any grid (xcd_map: the same tiles under other workgroup ids); 1025 = one region x 256 rows per workgroup at <= 4 blocks (fat waves of 2 x 2 tiles); 33 = round 5: the paired launch as four fat waves (k_gemm_fat; 1376 / 4 = 86 k-tiles per split: even)
                check(lib.la_lab_set(6, pair), 'debug_set')
                slabs = torch.full((ks, rows, N), float('nan'), dtype=torch.float32, device=DEV)
                _mb(0, wp, _pack_blocks(x), N, K, nblk, ksplit=ks, slabs=slabs, slab_rows=rows)
                outs.append(slabs[:, :nblk * 64].clone())
            assert all(torch.equal(outs[0], o) for o in outs[1:]), (N, K, ks)
        for nh, nkv, nwg in ((32, 32, 256), (32, 8, 256), (40, 40, 256), (8, 2, 32), (2, 2, 0)):
            K = 512
            N = (nh + 2 * nkv) * 128
            g = torch.Generator(device=DEV).manual_seed(nh * 7 + nkv + nblk)
            x = bf(torch.randn(nblk * 64, K, generator=g, device=DEV))
            w = bf(torch.randn(N, K, generator=g, device=DEV) * 0.05)
            pos = torch.randint(0, 900, (nblk * 64,), generator=g, device=DEV, dtype=torch.int32)
            if nwg:
                wp = gu.pack_planned(2, [w], nwg)
            else:
                perm = np.zeros(N, dtype=np.int32)
                check(lib.la_qkv_row_perm(nh, nkv, perm.ctypes.data_as(_lib.pi32)), 'perm')
                wp = gu.pack_weight(w[torch.from_numpy(perm.astype(np.int64)).to(DEV)].contiguous())
            outs = []
            for pair in (0, 1, 5, 33, 257 + 512, 257 + 4096):      # 4353 = one region x 128 rows per workgroup at <= 4 blocks (n_wg <= 128: the GQA / classic images here); 769 = round 5: ONE region x 256 rows per workgroup as fat waves of 2 x 2 tiles; 5 = paired + the QUAD form of the QKV launch (taken at >= 7 blocks of a GQA shape); 33 = fat waves (round 5)
                check(lib.la_lab_set(6, pair), 'debug_set')
                qf = torch.zeros(8 * nh * 8192, dtype=torch.bfloat16, device=DEV)
                kf = torch.zeros(8 * nkv * 8192, dtype=torch.bfloat16, device=DEV)
                vf = torch.zeros(8 * nkv * 8192, dtype=torch.bfloat16, device=DEV)
                _mb(2, wp, _pack_blocks(x), N, K, nblk, n_wg=nwg, pos=pos, rc=rc, rs_=rs_, qf=qf, kf=kf, vf=vf, nh=nh, nkv=nkv)
                outs.append((qf, kf, vf))
            for o in outs[1:]:
                for a_, b_ in zip(outs[0], o):
                    assert torch.equal(a_, b_), (nh, nkv, nwg)
        # gate/up + SwiGLU on planned images: two regions {G0, G1, U0, U1} x 2 per workgroup (RBV = 8 wave grid)
        for F, K in ((11008, 512), (13824, 1024), (14336, 256)):
            g = torch.Generator(device=DEV).manual_seed(F + nblk)
            x = bf(torch.randn(nblk * 64, K, generator=g, device=DEV))
            wg_ = bf(torch.randn(F, K, generator=g, device=DEV) * 0.05)
            wu_ = bf(torch.randn(F, K, generator=g, device=DEV) * 0.05)
            wp = gu.pack_planned(1, [wg_, wu_], 256)
            outs = []
            for pair in (0, 3, 17, 17 + 2048, 65 + 128):     # 2065 = the fat pair staged through registers (STG form); 17 = round 5: the pair of regions as FOUR fat waves (k_gemm_fat, 4 x TW accumulator tiles per wave); 193 = ONE region x all token blocks as four fat waves (bit 6; bit 7: at every block count)
                check(lib.la_lab_set(6, pair), 'debug_set')
                act = torch.zeros(8 * 64 * F, dtype=torch.bfloat16, device=DEV)
                _mb(1, wp, _pack_blocks(x), F, K, nblk, n_wg=256, act=act)
                outs.append(act)
            assert all(torch.equal(outs[0], o) for o in outs[1:]), (F, K)
            assert float(outs[0][:nblk * 64 * F].float().abs().sum()) > 0
    finally:
        lib.la_lab_set(6, default_form)


@pytest.mark.usefixtures('lab_build')
@pytest.mark.parametrize('nblk', [5, 6, 7, 8])
def test_mb_direct_weight_gateup_is_bitwise_the_fat_launch(nblk):
    """la_lab_set key 35 (k_gemm_fatd, the default at 5-8 blocks): the paired gate/up launch with the weight fragments streamed straight
    into MFMA operand registers (four waves = four {gate, up} row-block pairs x all 6 / 8 token tiles; only x goes through LDS).  Same MFMA
    chain per output element as k_gemm_fat (knob 35 = 0): the activation image must be equal bit for bit — three model shapes, short and
    long reductions."""
    assert lib.la_lab_get(35) == 1
    try:
        for F, K in ((11008, 512), (13824, 1024), (14336, 256), (14336, 4096), (11008, 128), (11008, 5120 + 96), (13824, 32), (14336, 1120), (11008, 2048 + 64), (13824, 96)):
            g = torch.Generator(device=DEV).manual_seed(F + K + nblk)
            x = bf(torch.randn(nblk * 64, K, generator=g, device=DEV))
            wg_ = bf(torch.randn(F, K, generator=g, device=DEV) * 0.05)
            wu_ = bf(torch.randn(F, K, generator=g, device=DEV) * 0.05)
            wp = gu.pack_planned(1, [wg_, wu_], 256)
            outs = []
            for knob in (0, 1):
                check(lib.la_lab_set(35, knob), 'lab_set')
                act = torch.full((8 * 64 * F,), -1.0, dtype=torch.bfloat16, device=DEV)
                _mb(1, wp, _pack_blocks(x), F, K, nblk, n_wg=256, act=act)
                torch.cuda.synchronize()
                outs.append(act)
            assert torch.equal(outs[0], outs[1]), (F, K)
            assert float(outs[0][:nblk * 64 * F].float().abs().sum()) > 0
    finally:
        lib.la_lab_set(35, 1)


@pytest.mark.usefixtures('lab_build')
@pytest.mark.parametrize('nblk', [5, 6, 7, 8])
def test_mb_x_direct_slab_launch_is_bitwise_the_fat_launch(nblk):
    """la_lab_set key 36 (k_gemm_fat, STG = 2, the default): in the slab launch at 5-8 blocks (one row group: the four waves share the weight
    row-blocks, each owns two token tiles) the x fragments go straight into MFMA operand registers and only the weights go through the LDS ring.
    Same MFMA chain per output element as the LDS-DMA form (knob 36 = 0): the fp32 split-K slabs must be equal bit for bit — K splits 1-4, stage
    counts with and without a remainder, with and without the one-K-split-per-XCD mapping."""
    assert lib.la_lab_get(36) == 1
    form = lib.la_lab_get(6)
    try:
        for N, K, ks in ((4096, 4096, 4), (4096, 5504, 4), (4096, 14336, 4), (5120, 5120, 3), (512, 512, 2), (1024, 64, 2), (256, 2048 + 32, 1)):
            g = torch.Generator(device=DEV).manual_seed(N + K + nblk)
            x = bf(torch.randn(nblk * 64, K, generator=g, device=DEV))
            wp = gu.pack_weight(bf(torch.randn(N, K, generator=g, device=DEV) * 0.05))
            rows = (nblk + 3) // 4 * 4 * 64
            outs = []
            for knob, pair in ((0, form), (1, form), (1, form & ~8192), (1, form | 16384)):
                check(lib.la_lab_set(36, knob), 'lab_set')
                check(lib.la_lab_set(6, pair), 'lab_set')
                slabs = torch.full((ks, rows, N), float('nan'), dtype=torch.float32, device=DEV)
                _mb(0, wp, _pack_blocks(x), N, K, nblk, ksplit=ks, slabs=slabs, slab_rows=rows)
                torch.cuda.synchronize()
                outs.append(slabs[:, :nblk * 64].clone())
            assert not torch.isnan(outs[0]).any()
            assert all(torch.equal(outs[0], o) for o in outs[1:]), (N, K, ks)
    finally:
        lib.la_lab_set(36, 1)
        lib.la_lab_set(6, form)


@pytest.mark.usefixtures('lab_build')
@pytest.mark.parametrize('nblk', [3, 4, 6, 8])
def test_mb_wide_schedules_are_bitwise_identical(nblk):
    """la_lab_set key 24: the round-4 schedule of k_gemm_wide (buffer-addressed LDS-DMA pieces; one fragment read after every MFMA at
    >= 3 token tiles per wave) runs the same MFMAs on the same operands in the same order as the round-2 schedule: slabs, Q / K / V
    fragments and SwiGLU activations must be equal bit for bit — classic and planned images, odd K ranges (half stages), K splits."""
    rc, rs_ = rope_tables(128, 1024, 10000.0, DEV)
    default_sched = lib.la_lab_get(24)
    assert default_sched == 1
    try:
        for N, K, ks in ((4096, 1376, 4), (512, 2048, 1), (5120, 528, 3)):        # 1376 / 4 and 528 / 3 k-tiles: odd ranges
            g = torch.Generator(device=DEV).manual_seed(N + nblk)
            x = bf(torch.randn(nblk * 64, K, generator=g, device=DEV))
            wp = gu.pack_weight(bf(torch.randn(N, K, generator=g, device=DEV) * 0.05))
            rows = (nblk + 3) // 4 * 4 * 64
            outs = []
            for sch in (0, 1):
                check(lib.la_lab_set(24, sch), 'lab_set')
                slabs = torch.full((ks, rows, N), float('nan'), dtype=torch.float32, device=DEV)
                _mb(0, wp, _pack_blocks(x), N, K, nblk, ksplit=ks, slabs=slabs, slab_rows=rows)
                outs.append(slabs[:, :nblk * 64].clone())
            assert torch.equal(outs[0], outs[1]), (N, K, ks)
            assert bool(torch.isfinite(outs[0]).all())
        for nh, nkv, nwg in ((32, 32, 256), (32, 8, 256), (8, 2, 32), (2, 2, 0)):
            K = 528
            N = (nh + 2 * nkv) * 128
            g = torch.Generator(device=DEV).manual_seed(nh * 7 + nkv + nblk)
            x = bf(torch.randn(nblk * 64, K, generator=g, device=DEV))
            w = bf(torch.randn(N, K, generator=g, device=DEV) * 0.05)
            pos = torch.randint(0, 900, (nblk * 64,), generator=g, device=DEV, dtype=torch.int32)
            if nwg:
                wp = gu.pack_planned(2, [w], nwg)
            else:
                perm = np.zeros(N, dtype=np.int32)
                check(lib.la_qkv_row_perm(nh, nkv, perm.ctypes.data_as(_lib.pi32)), 'perm')
                wp = gu.pack_weight(w[torch.from_numpy(perm.astype(np.int64)).to(DEV)].contiguous())
            outs = []
            for sch in (0, 1):
                check(lib.la_lab_set(24, sch), 'lab_set')
                qf = torch.zeros(8 * nh * 8192, dtype=torch.bfloat16, device=DEV)
                kf = torch.zeros(8 * nkv * 8192, dtype=torch.bfloat16, device=DEV)
                vf = torch.zeros(8 * nkv * 8192, dtype=torch.bfloat16, device=DEV)
                _mb(2, wp, _pack_blocks(x), N, K, nblk, n_wg=nwg, pos=pos, rc=rc, rs_=rs_, qf=qf, kf=kf, vf=vf, nh=nh, nkv=nkv)
                outs.append((qf, kf, vf))
            for a_, b_ in zip(outs[0], outs[1]):
                assert torch.equal(a_, b_), (nh, nkv, nwg)
        for F, K in ((11008, 528), (14336, 256)):
            g = torch.Generator(device=DEV).manual_seed(F + nblk)
            x = bf(torch.randn(nblk * 64, K, generator=g, device=DEV))
            wp = gu.pack_planned(1, [bf(torch.randn(F, K, generator=g, device=DEV) * 0.05), bf(torch.randn(F, K, generator=g, device=DEV) * 0.05)], 256)
            outs = []
            for sch in (0, 1):
                check(lib.la_lab_set(24, sch), 'lab_set')
                act = torch.zeros(8 * 64 * F, dtype=torch.bfloat16, device=DEV)
                _mb(1, wp, _pack_blocks(x), F, K, nblk, n_wg=256, act=act)
                outs.append(act)
            assert torch.equal(outs[0], outs[1]), (F, K)
            assert float(outs[0][:nblk * 64 * F].float().abs().sum()) > 0
    finally:
        lib.la_lab_set(24, default_sched)


def _random_wide_tree(rs, T, chain_len):
    """T rows (parent index < row index), multiword ancestor masks uint64[T][ceil(T/64)].  Rows 0, 3, 6, ... form one long chain
    (so that it crosses the 64-row block boundaries); every other row hangs below a random earlier row."""
    W = (T + 63) // 64
    chain = [r for r in range(0, T, 3)][:chain_len]
    parent = [-1] * T
    for k in range(1, len(chain)):
        parent[chain[k]] = chain[k - 1]
    on_chain = set(chain)
    for r in range(1, T):
        if r not in on_chain:
            parent[r] = int(rs.randint(0, r))
    anc = [0] * T
    for r in range(T):
        anc[r] = (anc[parent[r]] if parent[r] >= 0 else 0) | (1 << r)
    rm = np.zeros((T, W), dtype=np.uint64)
    for r in range(T):
        for w in range(W):
            rm[r, w] = (anc[r] >> (64 * w)) & 0xFFFFFFFFFFFFFFFF
    mask = np.array([[(anc[i] >> j) & 1 for j in range(T)] for i in range(T)], dtype=np.int64)
    return parent, chain, rm, mask


@pytest.mark.parametrize('T,chain_len', [(65, 20), (128, 36), (200, 45), (256, 40)])
def test_wide_tree_step_matches_oracle(T, chain_len):
    """Trees wider than a block (the reference's decoding_length=128 / branch_length=32 setting, README.md:100; grid search up to
    256, benchmarks/benchmark.py:256-288): rows 64 p .. of the tree are block p of one multi-block pass, later blocks see the
    earlier ones under their ancestor words (LA_MIN_XMASK).  Logits of EVERY tree row vs the oracle forward under the full
    [T][ctx + T] mask (positions = ctx + depth), the cross-block accept walk / emitted tokens / kept rows bit-exact given the
    device's argmax rows (<= LA_MOUT_TOKS tokens), and a second step on top of the cache the first one committed."""
    shape = tiny_shape()
    sd = _bf16_sd(5)
    eng = LlamaVerifyEngine(shape, sd, max_length=512, n_slots=1, max_blocks=4)
    oracle = lo.OracleLlama(shape, sd)
    rs = np.random.RandomState(T)
    P = 7                  # a SHORT context: the tree's own keys carry most of the attention mass, so a wrong visibility bit shows
    prompt = rs.randint(3, shape.vocab, size=P).tolist()
    tok = eng.mprefill(0, prompt)
    _, past = _oracle_seq(oracle, prompt)
    nk = P
    for step in range(2):
        parent, chain, rm, mask = _random_wide_tree(rs, T, chain_len)
        ids = np.concatenate([[tok], rs.randint(3, shape.vocab, size=T - 1)]).astype(np.int32)
        full = torch.cat([torch.ones((T, nk), dtype=torch.long), torch.from_numpy(mask)], 1)
        # make the long chain the DEVICE's own greedy continuation: forward-only passes (mode 2: nothing committed); a row's
        # logits depend on its ancestors only, so fixing the chain top-down converges in len(chain) passes
        for k in range(len(chain) - 1):
            eng.tstep(ids, rm, mode=2)
            ids[chain[k + 1]] = int(eng.mout()[_lib.LA_MOUT_ARGMAX + chain[k]])
        assert eng.slot_keys[0] == nk
        lg, past_all = oracle.forward(torch.tensor(ids.tolist()), full, past)
        toks, kept = eng.tstep(ids, rm, mode=0, eager=(step == 1))
        got = eng.mlogits()[:T]
        # per-row bound 4e-2 (SHORT context on purpose: the tree's own handful of bf16 keys carry the softmax mass, DESIGN 4 'One tolerance' (2); deep chain rows sit at ~3e-2) AND a mean bound that a
        # systematically wrong mask cannot meet; the later blocks are held to the same numbers as block 0
        gf, rf = got.float().cpu(), lg.float()
        rel = ((gf - rf).abs().amax(-1) / rf.abs().amax(-1)).numpy()
        assert rel.max() <= 4e-2 and rel.mean() <= 1.5e-2, (T, step, float(rel.max()), float(rel.mean()), int(rel.argmax()))
        if T > 64:
            assert rel[64:].mean() <= 1.5e-2 and rel[64:].max() <= 4e-2, (float(rel[64:].mean()), float(rel[64:].max()))
        mo = eng.mout().cpu().numpy()
        am = [int(mo[_lib.LA_MOUT_ARGMAX + r]) for r in range(T)]
        assert am == got.float().argmax(-1).cpu().tolist()
        exp_toks, exp_rows = lo.accept_scan(ids.tolist(), mask, am)
        exp_toks, exp_rows = exp_toks[:_lib.LA_MOUT_TOKS], exp_rows[:_lib.LA_MOUT_TOKS]
        assert toks == exp_toks and kept == len(exp_rows), (step, len(toks), len(exp_toks))
        if step == 0:
            assert len(exp_rows) > 16 and (max(exp_rows) >= 64 or T == 65)     # the walk crosses blocks and the old 16-token limit
        nb = (T + 63) // 64
        want = np.full(64 * nb, -1, dtype=np.int64)
        for d, r in enumerate(exp_rows):
            want[r] = nk + d
        assert mo[_lib.LA_MOUT_DST:_lib.LA_MOUT_DST + 64 * nb].tolist() == want.tolist()
        idx = torch.tensor(list(range(nk)) + [nk + r for r in exp_rows], dtype=torch.long)
        past = [(k[:, idx], v[:, idx]) for k, v in past_all]
        nk += len(exp_rows)
        assert eng.slot_keys[0] == nk
        tok = exp_toks[-1]


@pytest.mark.parametrize('Ts', [(100, 150), (65, 64, 130), (256, 200)])
def test_several_wide_trees_in_one_pass_match_oracle(Ts):
    """A batch whose per-sample trees are wider than a block (bat_get gives every sample (decoding_length // bs) // bs rows, any
    size: lookahead_cache.py:534-541): LlamaVerifyEngine.mstep_trees packs several sequences' trees — ceil(T / 64) consecutive
    blocks each, mode 0 + LA_MODE_TREE_PIECE — into ONE pass.  Per sequence: logits of every tree row vs the oracle forward under
    that sequence's own past and full mask, the cross-block accept walk / emitted tokens / commit plan bit-exact given the device's
    argmax rows, cursors; a second step on top of what the first one committed."""
    shape = tiny_shape()
    sd = _bf16_sd(9)
    n = len(Ts)
    nblk = sum((T + 63) // 64 for T in Ts)
    eng = LlamaVerifyEngine(shape, sd, max_length=768, n_slots=n, max_blocks=nblk)
    oracle = lo.OracleLlama(shape, sd)
    rs = np.random.RandomState(sum(Ts))
    pasts, nks, toks0 = [], [], []
    for i in range(n):
        prompt = rs.randint(3, shape.vocab, size=7 + 3 * i).tolist()
        toks0.append(eng.mprefill(i, prompt))
        pasts.append(_oracle_seq(oracle, prompt)[1])
        nks.append(len(prompt))
    for step in range(2):
        trees, meta = [], []
        for i, T in enumerate(Ts):
            parent, chain, rm, mask = _random_wide_tree(rs, T, min(30, T // 3))
            ids = np.concatenate([[toks0[i]], rs.randint(3, shape.vocab, size=T - 1)]).astype(np.int32)
            trees.append([i, ids, rm, 0, _lib.LA_MOUT_TOKS])
            meta.append((chain, mask))
        # make every tree's long chain the device's own greedy continuation (forward-only passes of the whole batch, nothing committed)
        for k in range(max(len(m[0]) for m in meta) - 1):
            eng.mstep_trees([(t[0], t[1], t[2], 2, t[4]) for t in trees])
            mo = eng.mout().cpu().numpy()
            b0 = 0
            for t, (chain, _) in zip(trees, meta):
                if k + 1 < len(chain):
                    t[1][chain[k + 1]] = int(mo[_lib.LA_MOUT_ARGMAX + 64 * b0 + chain[k]])
                b0 += (len(t[1]) + 63) // 64
        assert [eng.slot_keys[i] for i in range(n)] == nks
        out = eng.mstep_trees([tuple(t) for t in trees], eager=(step == 1))
        got_all = eng.mlogits()
        mo = eng.mout().cpu().numpy()
        b0 = 0
        for i, (t, (chain, mask)) in enumerate(zip(trees, meta)):
            ids, T = t[1], len(t[1])
            nb = (T + 63) // 64
            full = torch.cat([torch.ones((T, nks[i]), dtype=torch.long), torch.from_numpy(mask)], 1)
            lg, past_all = oracle.forward(torch.tensor(ids.tolist()), full, pasts[i])
            gf, rf = got_all[64 * b0:64 * b0 + T].float().cpu(), lg.float()
            rel = ((gf - rf).abs().amax(-1) / rf.abs().amax(-1)).numpy()
            assert rel.max() <= 4e-2 and rel.mean() <= 1.5e-2, (Ts, i, step, float(rel.max()), float(rel.mean()))
            am = [int(mo[_lib.LA_MOUT_ARGMAX + 64 * b0 + r]) for r in range(T)]
            assert am == gf.argmax(-1).tolist()
            exp_toks, exp_rows = lo.accept_scan(ids.tolist(), mask, am)
            exp_toks, exp_rows = exp_toks[:_lib.LA_MOUT_TOKS], exp_rows[:_lib.LA_MOUT_TOKS]
            assert out[i] == exp_toks, (Ts, i, step, len(out[i]), len(exp_toks))
            if step == 0 and T > 64:
                assert len(exp_rows) > 8
            want = np.full(64 * nb, -1, dtype=np.int64)
            for d, r in enumerate(exp_rows):
                want[r] = i * eng._capacity() + nks[i] + d             # main-cache key rows are slot-major
            assert mo[_lib.LA_MOUT_DST + 64 * b0:_lib.LA_MOUT_DST + 64 * (b0 + nb)].tolist() == want.tolist(), (Ts, i, step)
            idx = torch.tensor(list(range(nks[i])) + [nks[i] + r for r in exp_rows], dtype=torch.long)
            pasts[i] = [(k[:, idx], v[:, idx]) for k, v in past_all]
            nks[i] += len(exp_rows)
            assert eng.slot_keys[i] == nks[i]
            toks0[i] = exp_toks[-1]
            b0 += nb


def test_wide_tree_host_commit_equals_device_commit():
    """Sequential accept path on a wide tree (logits processors / sampling: tstep(mode=2) = forward only, the host walks the
    tree over the logits rows, tcommit(rows) moves the kept K/V rows of all the tree's blocks, la_llama_mcommit): keeping the
    rows the device walk keeps must leave the SAME cache — the next step's logits are bitwise equal."""
    shape = tiny_shape()
    sd = _bf16_sd(6)
    T = 150
    rs = np.random.RandomState(11)
    prompt = rs.randint(3, shape.vocab, size=40).tolist()
    parent, chain, rm, mask = _random_wide_tree(rs, T, 30)
    engs = [LlamaVerifyEngine(shape, sd, max_length=512, n_slots=1, max_blocks=3) for _ in range(2)]
    tok = [e.mprefill(0, prompt) for e in engs]
    assert tok[0] == tok[1]
    ids = np.concatenate([[tok[0]], rs.randint(3, shape.vocab, size=T - 1)]).astype(np.int32)
    for k in range(len(chain) - 1):
        engs[0].tstep(ids, rm, mode=2)
        ids[chain[k + 1]] = int(engs[0].mout()[_lib.LA_MOUT_ARGMAX + chain[k]])
    toks, kept = engs[0].tstep(ids, rm, mode=0)
    assert kept > 16
    engs[1].tstep(ids, rm, mode=2)
    am = engs[1].mlogits()[:T].float().argmax(-1).cpu().tolist()
    exp_toks, exp_rows = lo.accept_scan(ids.tolist(), mask, am)
    assert exp_toks[:_lib.LA_MOUT_TOKS] == toks
    engs[1].tcommit(exp_rows[:_lib.LA_MOUT_TOKS], T)
    assert engs[1].slot_keys[0] == engs[0].slot_keys[0] == 40 + kept
    nxt = np.concatenate([[toks[-1]], rs.randint(3, shape.vocab, size=70)]).astype(np.int32)
    _, _, rm2, _ = _random_wide_tree(rs, 71, 5)
    for e in engs:
        e.tstep(nxt, rm2, mode=2)
    assert torch.equal(engs[0].mlogits()[:71], engs[1].mlogits()[:71])


# ---- round 3: the multi-block step at the BENCHMARKED shapes against the oracle (2-layer slices, stated 2e-2) ---------------
def _window_prefill(oracle, prompt):
    """The prompt through the oracle in 64-token chains, as the engine's blocks: the oracle applies shape.sliding_window to the
    COMMITTED keys of a call (positions come from the mask row sums, so the rule cannot be written into the mask itself);
    inside a 64-token piece the window (>= 64) never bites."""
    past, nk, lg = None, 0, None
    for s0 in range(0, len(prompt), 64):
        blk = prompt[s0:s0 + 64]
        n = len(blk)
        full = torch.cat([torch.ones((n, nk), dtype=torch.long), torch.tril(torch.ones((n, n), dtype=torch.long))], 1)
        lg, past = oracle.forward(torch.tensor(blk), full, past)
        nk += n
    return lg, past


def test_mstep_mistral_shape_b8_window_ring_paired_launches_vs_oracle():
    """BASELINE config 3 as the driver benchmarks it, two layers deep: Mistral-7B layer shape (GQA 32 / 8 heads, ffn 14336,
    Mistral RMSNorm flavour, models/mistral/modeling_mistral.py:236-318), B = 8 sequences -> 512 rows in one pass (wide GEMMs
    with the paired QKV / slab launches, the default), sliding window with the KV cache as a RING (cfg.kv_ring), contexts
    shorter than, crossing and far beyond the window, two of them long enough to wrap the ring.  Every block vs the oracle run
    on that sequence alone (window rule included), then a second step over the caches the first one committed."""
    torch.set_num_threads(8)
    W = 160
    shape = LlamaShape(2, 4096, 32, 8, 14336, 32000, 1e-5, norm_cast_first=True, sliding_window=W)
    sd = random_weights(shape, seed=9, device='cpu')
    B = 8
    eng = LlamaVerifyEngine(shape, sd, max_length=1200, n_slots=B, max_blocks=B, kv_ring=True)
    assert eng.kv_ring and eng.max_keys == 736
    assert _lib.lab_get(6) & 1, 'the paired wide launches are the default (csrc/la_knobs.h: the lab build reports the product default)'
    oracle = lo.OracleLlama(shape, sd)
    rs = np.random.RandomState(21)
    lens = [40, 150, 170, 300, 90, 800, 230, 1000]          # < W, ~W, > W, >> W; 800 / 1000 wrap the 736-row ring
    pasts, nk, last = [], [], []
    for b, P in enumerate(lens):
        p = rs.randint(3, shape.vocab, size=P).tolist()
        tok = eng.mprefill(b, p)
        lg, past = _window_prefill(oracle, p)
        top = torch.topk(lg[-1].float(), 2).values
        if float(top[0] - top[1]) > 4 * TOL * float(lg[-1].float().abs().max()):
            assert tok == int(lg[-1].float().argmax()), b
        pasts.append(past); nk.append(P); last.append(tok)
    for step in range(2):
        blocks, trees = [], []
        for b in range(B):
            T = 64 if b in (0, 5) else int(rs.randint(8, 65))
            _, rows = random_tree(rs, T)
            ids = np.concatenate([[last[b]], rs.randint(3, shape.vocab, size=T - 1)]).astype(np.int32)
            blocks.append((b, ids, rows, 0, 16))
            trees.append((ids, rows, T))
        outs = eng.mstep(blocks)
        mo = eng.mout().cpu().numpy()
        for b in range(B):
            ids, rows, T = trees[b]
            mask = _mask_from_rows(rows, T)
            full = torch.cat([torch.ones((T, nk[b]), dtype=torch.long), torch.from_numpy(mask)], 1)
            lg, past_all = oracle.forward(torch.tensor(ids.tolist()), full, pasts[b])
            _check_rows(eng.mlogits()[b * 64:b * 64 + T], lg, range(T), f'Mistral-shape step {step} block {b} (ctx {nk[b]})')
            am = mo[_lib.LA_MOUT_ARGMAX + 64 * b:_lib.LA_MOUT_ARGMAX + 64 * b + T].tolist()
            exp_toks, exp_rows = lo.accept_scan(ids.tolist(), mask, am)
            assert outs[b] == exp_toks[:16], (step, b)
            idx = torch.tensor(list(range(nk[b])) + [nk[b] + r for r in exp_rows[:16]], dtype=torch.long)
            pasts[b] = [(k[:, idx], v[:, idx]) for k, v in past_all]
            nk[b] += len(exp_rows[:16])
            last[b] = exp_toks[:16][-1]
            assert eng.slot_keys[b] == nk[b]


def test_mstep_llama13b_shape_b4_vs_oracle():
    """BASELINE config 4's per-GPU share, two layers deep: Llama-2-13B layer shape (hidden 5120 -> 3 K splits of the slab GEMMs,
    40 heads -> one key split and no combine launch at 4 blocks, ffn 13824), 4 sequences x 64 rows = 256 rows per pass."""
    torch.set_num_threads(8)
    shape = LlamaShape(2, 5120, 40, 40, 13824, 32000, 1e-5)
    sd = random_weights(shape, seed=10, device='cpu')
    eng = LlamaVerifyEngine(shape, sd, max_length=512, n_slots=4, max_blocks=4)
    oracle = lo.OracleLlama(shape, sd)
    rs = np.random.RandomState(22)
    blocks, refs = [], []
    for b in range(4):
        p = rs.randint(3, shape.vocab, size=int(rs.randint(30, 330))).tolist()
        tok = eng.mprefill(b, p)
        _, past = _oracle_seq(oracle, p)
        T = 64 if b == 0 else int(rs.randint(8, 65))
        _, rows = random_tree(rs, T)
        ids = np.concatenate([[tok], rs.randint(3, shape.vocab, size=T - 1)]).astype(np.int32)
        blocks.append((b, ids, rows, 0, 16))
        full = torch.cat([torch.ones((T, len(p)), dtype=torch.long), torch.from_numpy(_mask_from_rows(rows, T))], 1)
        refs.append((oracle.forward(torch.tensor(ids.tolist()), full, past)[0], T))
    eng.mstep(blocks)
    for b, (lg, T) in enumerate(refs):
        _check_rows(eng.mlogits()[b * 64:b * 64 + T], lg, range(T), f'13B-shape block {b}')


def test_mstep_mixtral_gathered_experts_vs_oracle_with_forced_routing():
    """BASELINE config 5's path — the multi-block Mixtral step with GATHERED experts (k_moe_plan_mb / k_moe_gather_mb, rows packed
    per expert, MixtralSparseMoeBlock.forward, models/mixtral/modeling_mixtral.py:692-759) — against the ORACLE, not against the
    repo's own 64-row path: top-k routing is discontinuous, so (as tests/test_gpu_moe.py does for the 64-row path) ALL rows of
    every block are compared with the oracle re-run under the engine's own routing (forced_routing = the step's per-layer routing
    weights), and on decisively routed rows the engine must pick the oracle's experts."""
    from tests.tiny_model import moe_shape, moe_weights, TINY_MOE
    shape = moe_shape(TINY_MOE)
    sd = {k: v.to(torch.bfloat16) for k, v in moe_weights(TINY_MOE, seed=3).items()}
    B = 4
    eng = LlamaVerifyEngine(shape, dict(sd), max_length=256, n_slots=B, max_blocks=B)
    oracle = lo.OracleLlama(shape, sd)
    rs = np.random.RandomState(23)
    blocks, seqs = [], []
    for b in range(B):
        p = rs.randint(3, shape.vocab, size=int(rs.randint(10, 60))).tolist()
        tok = eng.mprefill(b, p)
        # the prompt's routing as the engine decided it (one block): the oracle's cache is built under the SAME routing, so an
        # expert flipped on a prompt row cannot leak into the tree rows through the K/V they attend to
        rwp = eng.mroute_weights()[:, :len(p), :shape.n_experts].cpu().clone()
        T = 64 if b == 0 else int(rs.randint(20, 65))
        _, rows = random_tree(rs, T)
        ids = np.concatenate([[tok], rs.randint(3, shape.vocab, size=T - 1)]).astype(np.int32)
        blocks.append((b, ids, rows, 0, 16))
        seqs.append((p, ids, rows, T, rwp))
    eng.mstep(blocks)
    rw = eng.mroute_weights().cpu()                                       # [L][512][8]
    n_dec = n_all = 0
    for b, (p, ids, rows, T, rwp) in enumerate(seqs):
        P = len(p)
        _, past = oracle.forward(torch.tensor(p), torch.tril(torch.ones((P, P), dtype=torch.long)), None,
                                 forced_routing=[rwp[li] for li in range(shape.n_layers)])
        full = torch.cat([torch.ones((T, P), dtype=torch.long), torch.from_numpy(_mask_from_rows(rows, T))], 1)
        lg_own, _ = oracle.forward(torch.tensor(ids.tolist()), full, past)
        trace = [rl.clone() for rl in oracle.router_trace]
        forced = [rw[li, 64 * b:64 * b + T, :shape.n_experts] for li in range(shape.n_layers)]
        lg_forced, _ = oracle.forward(torch.tensor(ids.tolist()), full, past, forced_routing=forced)
        got = eng.mlogits()[64 * b:64 * b + T].float().cpu()
        err = (got - lg_forced.float()).abs().amax(-1) / lg_forced.float().abs().amax(-1)
        assert float(err.max()) <= TOL_TAIL and float((err <= TOL).float().mean()) >= 1.0 - TAIL_FRAC, (b, float(err.max()), int(err.argmax()))
        decisive = []                                                     # rows routed with a margin in EVERY layer (oracle)
        for t in range(T):
            ok = True
            for rl in trace:
                srt = torch.sort(torch.softmax(rl[t].float(), -1), descending=True).values
                ok = ok and float(srt[shape.top_k - 1] - srt[shape.top_k]) > 0.05
            if ok:
                decisive.append(t)
        n_dec += len(decisive); n_all += T
        for li, rl in enumerate(trace):
            sel = torch.topk(torch.softmax(rl.float(), -1), shape.top_k, -1).indices
            for t in decisive:
                mine = sorted(int(e) for e in torch.nonzero(forced[li][t]).flatten())
                assert mine == sorted(sel[t].tolist()), (b, li, t)
    assert n_dec >= 0.25 * n_all


def test_mstep_mixtral8x7b_layer_shape_gathered_experts_vs_oracle_with_forced_routing():
    """BASELINE config 5 at its REAL layer shape, two layers deep: hidden 4096, GQA 32 / 8 heads, ffn 14336, 8 experts top-2
    (MixtralSparseMoeBlock.forward, models/mixtral/modeling_mixtral.py:692-759), B = 4 sequences x 64 rows = 256 rows per pass —
    the gathered-expert launches the driver times (k_moe_plan_mb / k_moe_gather_mb, merged per-stage expert launches
    k_gemm_mb<..., EX = true>, k_moe_accum_norm_mb).  Same method as the tiny-shape test above, at the STATED tolerance (2e-2):
    every row of every block vs the oracle re-run under the engine's own per-layer routing (prompt and tree), and on rows the
    oracle routes decisively the engine must pick the oracle's experts.  Weights: plain random init (std 0.02, every projection),
    NOT the permutation LM — an expert's output carries its full weight here, so a wrong row list / weight / expert shows."""
    torch.set_num_threads(min(16, os.cpu_count() or 8))
    shape = LlamaShape(2, 4096, 32, 8, 14336, 32000, 1e-5, rope_theta=1e6, n_experts=8, top_k=2, norm_cast_first=True)
    sd = random_weights(shape, seed=12, device='cpu')
    B = 4
    eng = LlamaVerifyEngine(shape, dict(sd), max_length=256, n_slots=B, max_blocks=B)
    oracle = lo.OracleLlama(shape, sd)
    rs = np.random.RandomState(24)
    blocks, seqs = [], []
    for b in range(B):
        p = rs.randint(3, shape.vocab, size=int(rs.randint(20, 64))).tolist()       # one prefill block per prompt
        tok = eng.mprefill(b, p)
        rwp = eng.mroute_weights()[:, :len(p), :shape.n_experts].cpu().clone()
        T = 64 if b < 2 else int(rs.randint(30, 65))
        _, rows = random_tree(rs, T)
        ids = np.concatenate([[tok], rs.randint(3, shape.vocab, size=T - 1)]).astype(np.int32)
        blocks.append((b, ids, rows, 0, 16))
        seqs.append((p, ids, rows, T, rwp))
    eng.mstep(blocks)
    rw = eng.mroute_weights().cpu()
    n_dec = n_all = 0
    worst = 0.0
    hit = torch.zeros(shape.n_layers, shape.n_experts)
    for b, (p, ids, rows, T, rwp) in enumerate(seqs):
        P = len(p)
        _, past = oracle.forward(torch.tensor(p), torch.tril(torch.ones((P, P), dtype=torch.long)), None,
                                 forced_routing=[rwp[li] for li in range(shape.n_layers)])
        full = torch.cat([torch.ones((T, P), dtype=torch.long), torch.from_numpy(_mask_from_rows(rows, T))], 1)
        oracle.forward(torch.tensor(ids.tolist()), full, past)
        trace = [rl.clone() for rl in oracle.router_trace]
        forced = [rw[li, 64 * b:64 * b + T, :shape.n_experts] for li in range(shape.n_layers)]
        lg_forced, _ = oracle.forward(torch.tensor(ids.tolist()), full, past, forced_routing=forced)
        got = eng.mlogits()[64 * b:64 * b + T].float().cpu()
        err = (got - lg_forced.float()).abs().amax(-1) / lg_forced.float().abs().amax(-1)
        worst = max(worst, float(err.max()))
        assert float(err.max()) <= TOL, (b, float(err.max()), int(err.argmax()))
        for li in range(shape.n_layers):
            w = forced[li]
            assert bool(((w != 0).sum(-1) == shape.top_k).all()), (b, li)              # every live row: exactly top_k experts
            assert float((w.sum(-1) - 1).abs().max()) < 2e-2, (b, li)                  # renormalised weights (bf16)
            hit[li] += (w != 0).sum(0).float()
        for t in range(T):
            ok = True
            for rl in trace:
                srt = torch.sort(torch.softmax(rl[t].float(), -1), descending=True).values
                ok = ok and float(srt[shape.top_k - 1] - srt[shape.top_k]) > 0.02
            if not ok:
                continue
            n_dec += 1
            for li, rl in enumerate(trace):
                sel = torch.topk(torch.softmax(rl[t].float(), -1), shape.top_k, -1).indices
                mine = sorted(int(e) for e in torch.nonzero(forced[li][t]).flatten())
                assert mine == sorted(sel.tolist()), (b, li, t)
        n_all += T
    print(f'[Mixtral-8x7B layer shape, 256 rows] max rel err vs oracle (forced routing) {worst:.4f}; decisively routed rows '
          f'{n_dec}/{n_all}; rows per expert, layer 0: {hit[0].int().tolist()}')
    assert n_dec >= 0.25 * n_all
    assert bool((hit > 0).all()), 'every expert of every layer received rows (the gathered path ran for all of them)'


@pytest.mark.usefixtures('lab_build')
def test_merged_expert_launch_forms_agree():
    """la_lab_set key 25: the merged-expert launches of the gathered MoE step.  One workgroup per CU (0) and two per CU with 4 weight tiles
    in flight (bits 0 / 1) run the same MFMA chain per output element and sum the K parts in the same fixed order: bit-identical logits.
    The round-5 forms with TWO adjacent weight regions per workgroup (bits 2 / 3: half the x traffic and LDS reads per weight byte) give a
    wave a longer K range (gate/up: the whole K in one accumulator chain instead of two K parts; down: two parts instead of four), i.e.
    another — equally valid, deterministic — fp32 summation order: same routing (the router runs before the experts), logits within bf16 noise of the other forms (1e-2 of max|logit| per row; the stated tolerance vs the oracle is 2e-2 and is asserted for
    whatever form is the default by test_mstep_mixtral8x7b_layer_shape_gathered_experts_vs_oracle_with_forced_routing)."""
    shape = LlamaShape(1, 4096, 32, 8, 14336, 32000, 1e-5, rope_theta=1e6, n_experts=8, top_k=2, norm_cast_first=True)
    sd = random_weights(shape, seed=13, device='cpu')
    B = 4
    default_form = lib.la_lab_get(25)
    outs = {}
    try:
        for form in (0, 1, 3, 4, 8, 12):
            check(_lib.lab_set(25, form), 'lab_set')
            eng = LlamaVerifyEngine(shape, dict(sd), max_length=256, n_slots=B, max_blocks=B)
            rs = np.random.RandomState(31)
            blocks = []
            for b in range(B):
                p = rs.randint(3, shape.vocab, size=int(rs.randint(20, 64))).tolist()
                tok = eng.mprefill(b, p)
                T = 64 if b < 2 else int(rs.randint(30, 65))
                _, rows = random_tree(rs, T)
                ids = np.concatenate([[tok], rs.randint(3, shape.vocab, size=T - 1)]).astype(np.int32)
                blocks.append((b, ids, rows, 0, 16))
            toks = eng.mstep(blocks)
            outs[form] = (eng.mlogits()[:B * 64].clone(), eng.mroute_weights().clone(), toks)
            del eng
    finally:
        _lib.lab_set(25, default_form)
    ref = outs[0]
    assert bool(torch.isfinite(ref[0].float()).all()) and float(ref[0].float().abs().max()) > 0
    for form in (1, 3):
        assert torch.equal(outs[form][0], ref[0]) and torch.equal(outs[form][1], ref[1]) and outs[form][2] == ref[2], form
    for form in (4, 8, 12):
        lg = outs[form][0].float()
        err = (lg - ref[0].float()).abs().amax(-1) / ref[0].float().abs().amax(-1).clamp_min(1e-6)
        assert torch.equal(outs[form][1], ref[1]), form                      # routing weights: identical (the router precedes the experts)
        assert float(err.max()) <= 1e-2, (form, float(err.max()))


@pytest.mark.usefixtures('lab_build')
def test_moe_plan_gather_one_launch_is_bitwise_the_two_launch_form():
    """la_lab_set key 16 bit 2: the expert plan (rows per expert, ascending) and the gather of each expert's packed activation blocks as ONE
    launch (round 5 default: every workgroup derives its expert's row list itself) vs the round-3 pair of launches.  Integer work in front
    of the same GEMMs: logits, routing weights and emitted tokens must be equal bit for bit — full blocks, ragged last blocks, 2-4 blocks."""
    shape = LlamaShape(1, 4096, 32, 8, 14336, 32000, 1e-5, rope_theta=1e6, n_experts=8, top_k=2, norm_cast_first=True)
    sd = random_weights(shape, seed=17, device='cpu')
    default_form = lib.la_lab_get(16)
    assert default_form == 0
    try:
        for B in (2, 3, 4):
            outs = {}
            for form in (0, 4):
                check(_lib.lab_set(16, form), 'lab_set')
                eng = LlamaVerifyEngine(shape, dict(sd), max_length=256, n_slots=B, max_blocks=B)
                rs = np.random.RandomState(37 + B)
                blocks = []
                for b in range(B):
                    p = rs.randint(3, shape.vocab, size=int(rs.randint(20, 64))).tolist()
                    tok = eng.mprefill(b, p)
                    T = 64 if b == 0 else int(rs.randint(5, 65))
                    _, rows = random_tree(rs, T)
                    ids = np.concatenate([[tok], rs.randint(3, shape.vocab, size=T - 1)]).astype(np.int32)
                    blocks.append((b, ids, rows, 0, 16))
                toks = eng.mstep(blocks)
                outs[form] = (eng.mlogits()[:B * 64].clone(), eng.mroute_weights().clone(), toks)
                del eng
            assert bool(torch.isfinite(outs[0][0].float()).all()) and float(outs[0][0].float().abs().max()) > 0
            assert torch.equal(outs[0][0], outs[4][0]) and torch.equal(outs[0][1], outs[4][1]) and outs[0][2] == outs[4][2], B
    finally:
        _lib.lab_set(16, default_form)


def test_every_product_gemm_form_launches_and_matches_torch():
    """One small launch per row of the product build's table of GEMM forms (csrc/la_mb_forms.h; tests/mb_form_cases.py lists them and
    tests/test_mb_forms_cpu.py asserts that each case selects the form it names) against the fp32 torch reference, at the tolerance this
    file uses for the kind: a row with another kernel's LDS size, block size or kernel pointer fails to launch or computes garbage."""
    from tests.mb_form_cases import FORM_CASES
    from tests.test_gpu_kernels import _rope_ref
    rc, rs_ = rope_tables(128, 1024, 10000.0, DEV)
    for form, kind, nblk, K, shp in FORM_CASES:
        g = torch.Generator(device=DEV).manual_seed(nblk * 1000 + K + kind)
        x = bf(torch.randn(nblk * 64, K, generator=g, device=DEV))
        xp = _pack_blocks(x)
        if kind == 0:
            N = shp
            w = bf(torch.randn(N, K, generator=g, device=DEV) * 0.05)
            rows = (nblk if nblk <= 2 else (nblk + 3) // 4 * 4) * 64
            slabs = torch.full((1, rows, N), float('nan'), dtype=torch.float32, device=DEV)
            _mb(0, gu.pack_weight(w), xp, N, K, nblk, ksplit=1, slabs=slabs, slab_rows=rows)
            assert gu.rel_err(slabs[0, :nblk * 64], x.double() @ w.double().t()) < 2e-3, form
        elif kind == 1:
            F, nwg = shp
            wg = bf(torch.randn(F, K, generator=g, device=DEV) * 0.05)
            wu = bf(torch.randn(F, K, generator=g, device=DEV) * 0.05)
            act = torch.zeros(8 * 64 * F, dtype=torch.bfloat16, device=DEV)
            _mb(1, gu.pack_planned(1, [wg, wu], nwg) if nwg else gu.pack_weight(wg, wu), xp, F, K, nblk, n_wg=nwg, act=act)
            got = gu.from_packed(act[:nblk * 64 * F].view(nblk, 64 * F), gu.xp_index(F)).float()
            gg, uu = bf(x.float() @ wg.float().t()), bf(x.float() @ wu.float().t())
            ref = bf(bf(torch.nn.functional.silu(gg.float())).float() * uu.float()).float().view(nblk, 64, F)
            assert gu.rel_err(got, ref) < 2e-2, form
            assert float((got != ref).float().mean()) < 0.02, form
        elif kind == 2:
            nh, nkv, nwg = shp
            N = (nh + 2 * nkv) * 128
            w = bf(torch.randn(N, K, generator=g, device=DEV) * 0.05)
            pos = torch.randint(0, 900, (nblk * 64,), generator=g, device=DEV, dtype=torch.int32)
            if nwg:
                wp = gu.pack_planned(2, [w], nwg)
            else:
                perm = np.zeros(N, dtype=np.int32)
                check(lib.la_qkv_row_perm(nh, nkv, perm.ctypes.data_as(_lib.pi32)), 'perm')
                wp = gu.pack_weight(w[torch.from_numpy(perm.astype(np.int64)).to(DEV)].contiguous())
            qf = torch.zeros(8 * nh * 8192, dtype=torch.bfloat16, device=DEV)
            kf = torch.zeros(8 * nkv * 8192, dtype=torch.bfloat16, device=DEV)
            vf = torch.zeros(8 * nkv * 8192, dtype=torch.bfloat16, device=DEV)
            _mb(2, wp, xp, N, K, nblk, n_wg=nwg, pos=pos, rc=rc, rs_=rs_, qf=qf, kf=kf, vf=vf, nh=nh, nkv=nkv)
            qkv = x.float() @ w.float().t()
            q = _rope_ref(qkv[:, :nh * 128].reshape(-1, nh, 128), pos.long())
            k = _rope_ref(qkv[:, nh * 128:(nh + nkv) * 128].reshape(-1, nkv, 128), pos.long())
            v = qkv[:, (nh + nkv) * 128:].reshape(-1, nkv, 128)
            for b in range(nblk):
                rows = slice(b * 64, (b + 1) * 64)
                got_q = gu.from_packed(qf[b * nh * 8192:(b + 1) * nh * 8192].view(nh, 8192), gu.rf_index(64)).transpose(0, 1)
                got_k = gu.from_packed(kf[b * nkv * 8192:(b + 1) * nkv * 8192].view(nkv, 8192), gu.rf_index(64)).transpose(0, 1)
                got_v = gu.from_packed(vf[b * nkv * 8192:(b + 1) * nkv * 8192].view(nkv, 8192), gu.vf_index(64)).transpose(0, 1)
                for got, ref, name in ((got_q, q[rows], 'q'), (got_k, k[rows], 'k'), (got_v, v[rows], 'v')):
                    assert gu.rel_err(got.float(), ref) < 1e-2, (form, b, name)
        else:
            V, nwg = shp
            w = bf(torch.randn(V, K, generator=g, device=DEV) * 0.05)
            n_tiles = 4 * (nwg if nwg else V // 128)
            logits = torch.zeros(8 * 64, V, dtype=torch.bfloat16, device=DEV)
            cv = torch.zeros(8 * n_tiles * 64, dtype=torch.float32, device=DEV)
            ci = torch.zeros(8 * n_tiles * 64, dtype=torch.int32, device=DEV)
            _mb(3, gu.pack_planned(0, [w], nwg) if nwg else gu.pack_weight(w), xp, V, K, nblk, n_wg=nwg, logits=logits, cv=cv, ci=ci)
            assert gu.rel_err(logits[:nblk * 64].float(), x.double() @ w.double().t()) < 1e-2, form
