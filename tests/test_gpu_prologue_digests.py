# -*- coding: utf-8 -*-
"""The prologues of the single-sequence step's kernels (K range of a split, wave ranges, block decomposition of the attention launch,
expert addressing) pinned bit for bit at the smallest shapes at which they can go wrong: tests/golden/prologue_digests.json holds a
sha256 of every output buffer, recorded (record_all() below) on an MI355X from the libraries of the commit BEFORE the prologues were
reworked (no division, no scalar round trip before the first load).  A prologue that hands a wave another K range, another row block or
another head changes the fp32 summation order or the bytes themselves, so every digest moves.

  slab launches   la_gemm64_slab, N in {64, 96} (rb 2 / rb 1), K16 in {16, 26, 29} x ksplit in {1, 2, 3, 4, 6} wherever K16 / ksplit >= 4
                  (remainders in both bounds of a split), the 4-wave and the 8-wave instantiation; la_gemm64_slab_fp8 the same at N = 64
                  (the fp8 entry point takes whole 64-row groups only)
  planned         hidden 256: QKV nh = 4, nkv = 2 with and without bias, SwiGLU F = 352, logits V = 1000 (bf16), QKV and SwiGLU in fp8
                  (the planned lm_head has no fp8 form); the classic launches of the same epilogues ride along
  attention       la_tree_attn (the single-launch kernel), nh = 8 with nkv in {8, 2} (sharers on one XCD / linear block order),
                  1, 33, 225 and 300 committed keys, V's head dims over 4 workgroups (the product default) and over 1 (lab knob 37 = 0);
                  plus 6 heads over 2 kv heads: a group size that is no power of two
  experts         the routed launch (one launch per expert, lab knob 16 = 1) and the merged-expert launch with E = 3 have no per-kernel
                  entry point: they run inside a one-layer Mixtral-shaped engine whose third router row is the mean of the other two, so
                  no row ever routes to expert 2 (its workgroups return at once)

The module uses only API of the commit the fixture was recorded from.  Plans and forms depend on the CU count, which the fixture stores."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from painlessinferenceacceleration_amd import _lib
from painlessinferenceacceleration_amd._lib import check, lib
from painlessinferenceacceleration_amd.llama_engine import LlamaVerifyEngine, quantize_fp8, rope_tables
from tests import gpu_utils as gu
from tests.gpu_utils import DEV, ptr, sp
from tests.test_gpu_fp8 import pack8, pack_planned8
from tests.tiny_model import TINY_MOE, moe_shape, moe_weights

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'prologue_digests.json')
K16S, KSPLITS = (16, 26, 29), (1, 2, 3, 4, 6)
WAVES = {64: {4: 2, 8: 2 | 3 << 8}, 96: {4: 1, 8: 1 | 1 << 8}}          # N -> waves -> the rb argument (row-blocks | variant << 8)
HIDDEN = 256


def _sha(*ts):
    h = hashlib.sha256()
    for t in ts:
        h.update(np.ascontiguousarray(t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy()).tobytes())
    return h.hexdigest()


def _randn(rs, *shape, scale=1.0):
    return torch.from_numpy((rs.standard_normal(shape) * scale).astype(np.float32)).to(DEV)


def _bf(t):
    return t.to(torch.bfloat16)


def slab_digests(fp8):
    out = {}
    for N in ((64,) if fp8 else (64, 96)):
        for K16 in K16S:
            K = 16 * K16
            rs = np.random.RandomState(1000 * N + K16)
            x, w = _bf(_randn(rs, 64, K)), _randn(rs, N, K, scale=0.05)
            xp = gu.pack_x(x)
            if fp8:
                q, s = quantize_fp8(w * torch.logspace(-1, 1, N, device=DEV)[:, None])
                wp = pack8(lib, q)
            else:
                wp = gu.pack_weight(_bf(w))
            for ks in KSPLITS:
                if K16 // ks < 4:
                    continue
                for waves, rb in WAVES[N].items():
                    slabs = torch.full((ks, 64, N), float('nan'), dtype=torch.float32, device=DEV)
                    if fp8:
                        check(lib.la_gemm64_slab_fp8(sp(), ptr(wp), ptr(xp), N, K, rb, ks, ptr(slabs), ptr(s)), 'slab8')
                    else:
                        check(lib.la_gemm64_slab(sp(), ptr(wp), ptr(xp), N, K, rb, ks, ptr(slabs)), 'slab')
                    torch.cuda.synchronize()
                    assert not torch.isnan(slabs).any()
                    out[f'N{N}/K16_{K16}/ks{ks}/w{waves}'] = _sha(slabs)
    return out


def _qkv_case(rs, nh, nkv):
    N = (nh + 2 * nkv) * 128
    x, w = _bf(_randn(rs, 64, HIDDEN)), _randn(rs, N, HIDDEN, scale=0.05)
    bias = _bf(_randn(rs, N, scale=0.5))
    pos = torch.from_numpy(rs.randint(0, 900, size=64).astype(np.int32)).to(DEV)
    rc, rsn = rope_tables(128, 1024, 10000.0, DEV)
    return N, x, w, bias, pos, rc, rsn


def planned_digests():
    out = {}
    nh, nkv, nwg = 4, 2, 16
    rs = np.random.RandomState(7)
    N, x, w, bias, pos, rc, rsn = _qkv_case(rs, nh, nkv)
    xp = gu.pack_x(x)
    q8, s8 = quantize_fp8(w)
    bufs = lambda: [torch.zeros(n * 8192, dtype=torch.bfloat16, device=DEV) for n in (nh, nkv, nkv)]
    perm = np.zeros(N, dtype=np.int32)
    check(lib.la_qkv_row_perm(nh, nkv, perm.ctypes.data_as(_lib.pi32)), 'perm')
    wperm = _bf(w)[torch.from_numpy(perm.astype(np.int64)).to(DEV)].contiguous()
    images = {'planned': gu.pack_planned(2, [_bf(w)], nwg), 'planned_fp8': pack_planned8(lib, 2, [q8], nwg), 'classic': gu.pack_weight(wperm)}
    for b in (None, bias):
        tag = 'bias' if b is not None else 'nobias'
        for form, wp in images.items():
            o = bufs()
            if form == 'planned':
                check(lib.la_gemm64r_qkv_bias(sp(), ptr(wp), ptr(xp), nh, nkv, HIDDEN, nwg, ptr(pos), ptr(rc), ptr(rsn), *[ptr(t) for t in o], ptr(b)), 'qkv_r')
            elif form == 'planned_fp8':
                check(lib.la_gemm64r_qkv_fp8(sp(), ptr(wp), ptr(xp), nh, nkv, HIDDEN, nwg, ptr(pos), ptr(rc), ptr(rsn), *[ptr(t) for t in o], ptr(b), ptr(s8)), 'qkv8_r')
            else:
                check(lib.la_gemm64_qkv_bias(sp(), ptr(wp), ptr(xp), nh, nkv, HIDDEN, ptr(pos), ptr(rc), ptr(rsn), *[ptr(t) for t in o], 0, ptr(b)), 'qkv')
            torch.cuda.synchronize()
            out[f'qkv/{form}/{tag}'] = _sha(*o)
    # SwiGLU, F = 352 over 8 workgroups (44 rows each: a partial second row block)
    F, nwg = 352, 8
    rs = np.random.RandomState(8)
    x, wg, wu = _bf(_randn(rs, 64, HIDDEN)), _randn(rs, F, HIDDEN, scale=0.05), _randn(rs, F, HIDDEN, scale=0.05)
    xp = gu.pack_x(x)
    (qg, sg), (qu, su) = quantize_fp8(wg), quantize_fp8(wu)
    sc = torch.cat([sg, su]).contiguous()
    for form in ('planned', 'planned_fp8', 'classic'):
        act = torch.zeros(64 * F, dtype=torch.bfloat16, device=DEV)
        if form == 'planned':
            wp = gu.pack_planned(1, [_bf(wg), _bf(wu)], nwg)
            check(lib.la_gemm64r_swiglu(sp(), ptr(wp), ptr(xp), F, HIDDEN, nwg, ptr(act)), 'swiglu_r')
        elif form == 'planned_fp8':
            wp = pack_planned8(lib, 1, [qg, qu], nwg)
            check(lib.la_gemm64r_swiglu_fp8(sp(), ptr(wp), ptr(xp), F, HIDDEN, nwg, ptr(act), ptr(sc)), 'swiglu8_r')
        else:
            wp = gu.pack_weight(_bf(wg), _bf(wu))
            check(lib.la_gemm64_swiglu(sp(), ptr(wp), ptr(xp), F, HIDDEN, ptr(act), 0), 'swiglu')
        torch.cuda.synchronize()
        out[f'swiglu/{form}'] = _sha(act)
    # logits, V = 1000 over 8 workgroups (125 rows each); the classic two-row-block launch takes whole 64-row groups: V = 960
    rs = np.random.RandomState(9)
    x = _bf(_randn(rs, 64, HIDDEN))
    xp = gu.pack_x(x)
    for form, V, nwg in (('planned', 1000, 8), ('classic', 960, 0)):
        w = _bf(_randn(rs, V, HIDDEN, scale=0.05))
        n_tiles = nwg if nwg else V // 64 * 2
        logits = torch.zeros(64, V, dtype=torch.bfloat16, device=DEV)
        cv = torch.zeros(max(n_tiles, 8) * 8 * 64, dtype=torch.float32, device=DEV)
        ci = torch.zeros(max(n_tiles, 8) * 8 * 64, dtype=torch.int32, device=DEV)
        state = torch.zeros(_lib.LA_ST_WORDS, dtype=torch.int32, device=DEV)
        if nwg:
            wp = gu.pack_planned(0, [w], nwg)
            check(lib.la_gemm64r_logits(sp(), ptr(wp), ptr(xp), V, HIDDEN, nwg, ptr(logits), ptr(cv), ptr(ci)), 'logits_r')
        else:
            wp = gu.pack_weight(w)
            check(lib.la_gemm64_logits(sp(), ptr(wp), ptr(xp), V, HIDDEN, 2, ptr(logits), ptr(cv), ptr(ci)), 'logits')
        check(lib.la_argmax_finalize(sp(), ptr(cv), ptr(ci), n_tiles, ptr(state)), 'argmax')
        torch.cuda.synchronize()
        out[f'logits/{form}'] = _sha(logits, cv[:n_tiles * 64], ci[:n_tiles * 64], state[_lib.LA_ST_ARGMAX:_lib.LA_ST_ARGMAX + 64])
    return out


ATTN_CASES = [(8, 8), (8, 2), (6, 2)]
ATTN_KEYS = (1, 33, 225, 300)


def attn_digests():
    """DV = 4: the product library's default form; DV = 1: the lab build with knob 37 = 0"""
    out = {}
    lab = _lib.lab_lib_for(torch.bfloat16)
    max_keys = 512
    for nh, nkv in ATTN_CASES:
        rs = np.random.RandomState(100 * nh + nkv)
        q = _bf(_randn(rs, nh, 64, 128))
        kmain, vmain = _bf(_randn(rs, nkv, max_keys, 128)), _bf(_randn(rs, nkv, max_keys, 128))
        kfr, vfr = _bf(_randn(rs, nkv, 64, 128)), _bf(_randn(rs, nkv, 64, 128))
        _, rows = gu.random_tree(rs, 64)
        rm = torch.from_numpy(np.array([int(r) for r in rows], dtype=np.uint64).view(np.int64)).to(DEV)
        qf = gu.to_packed(q, gu.rf_index(64), 8192).reshape(-1)
        km = gu.to_packed(kmain, gu.rf_index(max_keys), max_keys * 128).reshape(-1)
        vm = gu.to_packed(vmain, gu.vf_index(max_keys), max_keys * 128).reshape(-1)
        kf = gu.to_packed(kfr, gu.rf_index(64), 8192).reshape(-1)
        vf = gu.to_packed(vfr, gu.vf_index(64), 8192).reshape(-1)
        part = [torch.zeros(nh * 64 * 128, dtype=torch.float32, device=DEV), torch.zeros(nh * 64, dtype=torch.float32, device=DEV),
                torch.zeros(nh * 64, dtype=torch.float32, device=DEV)]
        for nkeys in (ATTN_KEYS if nh == 8 else (225,)):
            state = torch.zeros(_lib.LA_ST_WORDS, dtype=torch.int32, device=DEV)
            state[_lib.LA_ST_NKEYS] = nkeys
            for dv, L in ((4, lib), (1, lab)):
                o = torch.zeros(64 * nh * 128, dtype=torch.bfloat16, device=DEV)
                old = lab.la_lab_get(37)
                try:
                    if dv == 1:
                        check(lab.la_lab_set(37, 0), 'lab_set')
                    check(L.la_tree_attn(sp(), ptr(qf), ptr(km), ptr(vm), ptr(kf), ptr(vf), ptr(rm), ptr(state), nh, nkv, max_keys, 1,
                                         *[ptr(t) for t in part], ptr(o)), 'tree_attn')
                    torch.cuda.synchronize()
                finally:
                    lab.la_lab_set(37, old)
                assert float(part[0].abs().max()) == 0.0, 'the single-launch form writes no split partials'
                out[f'nh{nh}_nkv{nkv}/keys{nkeys}/dv{dv}'] = _sha(o)
    return out


def expert_digests():
    """merged: the product engine (one grid over the 3 experts); routed: the lab engine with one launch per expert and stage"""
    cfg = dict(TINY_MOE, n_layers=1, n_experts=3, top_k=1, ffn=352)
    sd = moe_weights(cfg, 5, torch.bfloat16)
    gate = sd['model.layers.0.block_sparse_moe.gate.weight'].float()
    gate[2] = 0.5 * (gate[0] + gate[1])               # the mean of two logits is never the largest: nobody routes to expert 2
    sd['model.layers.0.block_sparse_moe.gate.weight'] = gate.to(torch.bfloat16)
    rs = np.random.RandomState(3)
    prompt = rs.randint(3, cfg['vocab'], size=20).tolist()
    out = {}
    for form in ('merged', 'routed'):
        old = _lib.lab_get(16)
        try:
            if form == 'routed':
                check(_lib.lab_set(16, 1), 'lab_set')
            eng = LlamaVerifyEngine(moe_shape(cfg), dict(sd), max_length=256, lab=(form == 'routed'))
            tok = eng.prefill(prompt, fast=False)
            first = _sha(eng.logits()[:len(prompt)])
            ids = np.array([tok, prompt[3], prompt[4]], dtype=np.int32)
            toks, n = eng.step(ids, np.array([1, 3, 7], dtype=np.uint64))
            out[form] = {'tok': int(tok), 'prefill_logits': first, 'toks': [int(t) for t in toks], 'n': int(n), 'step_logits': _sha(eng.logits()[:3])}
            del eng
        finally:
            if form == 'routed':
                _lib.lab_set(16, old)
    return out


GROUPS = {'slab_bf16': lambda: slab_digests(False), 'slab_fp8': lambda: slab_digests(True), 'planned': planned_digests,
          'attention': attn_digests, 'experts': expert_digests}


def record_all():
    """the fixture's content, from whatever libraries lie beside the package"""
    d = {name: fn() for name, fn in GROUPS.items()}
    d['cu_count'] = int(torch.cuda.get_device_properties(0).multi_processor_count)
    return d


@pytest.fixture(scope='module')
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_holds_the_cases_it_was_chosen_for(golden):
    n_slab = sum(1 for K16 in K16S for ks in KSPLITS if K16 // ks >= 4) * 2
    assert len(golden['slab_bf16']) == 2 * n_slab and len(golden['slab_fp8']) == n_slab and n_slab == 28
    assert len(golden['attention']) == 2 * (2 * len(ATTN_KEYS) + 1)
    assert sorted(golden['experts']) == ['merged', 'routed']
    # forms that must differ do: another K split is another summation order
    assert golden['slab_bf16']['N64/K16_26/ks3/w4'] != golden['slab_bf16']['N64/K16_26/ks4/w4']
    assert golden['planned']['qkv/planned/bias'] != golden['planned']['qkv/planned/nobias']


@pytest.mark.parametrize('group', list(GROUPS))
def test_prologue_digests_match_the_recorded_ones(golden, group):
    assert torch.cuda.get_device_properties(0).multi_processor_count == golden['cu_count'], \
        'plans and attention forms follow the CU count: the digests hold for the recorded one only'
    got = json.loads(json.dumps(GROUPS[group]()))
    want = golden[group]
    assert sorted(got) == sorted(want)
    diff = [k for k in sorted(want) if got[k] != want[k]]
    assert not diff, (group, len(diff), diff[:8])
