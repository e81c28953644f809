# -*- coding: utf-8 -*-
"""-m gpu, lab build: the single-launch tree attention with V's head dims split over DV workgroups (csrc/la_attn1.hip, la_lab_set key 37)
must be BYTE-equal to the (SL = 2, DV = 1) form it replaces — a workgroup that owns 4 / DV of the 32-dim blocks of V computes the same
scores and softmax and sends every output element through the same fp32 operations; only which workgroup stores which columns of
o_proj's operand differs (and, with a ring, when a tile's loads are issued).  Equality, not a tolerance: the bar needs no derivation."""
import numpy as np
import pytest
import torch

from painlessinferenceacceleration_amd import _lib
from painlessinferenceacceleration_amd._lib import lib, check
from painlessinferenceacceleration_amd.llama_engine import LlamaShape, LlamaVerifyEngine, random_weights
from tests import gpu_utils as gu
from tests.gpu_utils import DEV, ptr, sp, random_tree
from tests.tiny_model import tiny_shape, tiny_weights

pytestmark = pytest.mark.gpu
KEY = 37
# (DV, ring tiles) pairs the lab build instantiates (ATTN1_FORMS in csrc/la_attn1.hip), each at every slice count SL
KERNELS = ((2, 0), (4, 0), (2, 2), (4, 2), (4, 3))
SLICES = (1, 2, 4)


def _form(sl, dv, nkb):
    return dv | (sl << 4) | (nkb << 8)


def _forms_that_fit(nh):
    """The launcher takes a form only where nh * 2 * SL * DV workgroups fit one per CU; anything else runs the DV = 1 kernel, and
    comparing that with itself would prove nothing."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return [(sl, dv, nkb) for dv, nkb in KERNELS for sl in SLICES if nh * 2 * sl * dv <= cus]


def test_every_kernel_of_the_lab_build_is_reached_at_the_7b_shape():
    fit = _forms_that_fit(32)
    assert {(dv, nkb) for _, dv, nkb in fit} == set(KERNELS) and (1, 4, 3) in fit and (2, 2, 0) in fit
    assert all(dv == 2 and sl == 1 for sl, dv, _ in _forms_that_fit(40)) or torch.cuda.get_device_properties(0).multi_processor_count > 256    # 40 heads: no DV = 4


@pytest.mark.parametrize('nh,nkv,dtype', [(32, 32, torch.bfloat16), (32, 8, torch.bfloat16), (32, 8, torch.float16), (4, 2, torch.bfloat16),
                                          (6, 3, torch.bfloat16)])
@pytest.mark.usefixtures('lab_build')
def test_dv_forms_store_the_bytes_of_the_dv1_form(nh, nkv, dtype):
    """lk_tree_attn1 through la_tree_attn (C ABI) on seeded inputs: the 7B shape (32 / 32 heads), GQA 32 / 8 (sharers of a kv head on
    one XCD), few heads (every SL x DV fits; 6 / 3: nkv not a multiple of 8, the other block-id map); contexts on both sides of the
    226 keys where the early first tile starts to be used, up to more tiles than any ring is deep, and trees of fewer than 64 rows
    (the unused rows carry their own diagonal bit, as the engine writes them)."""
    lab = _lib.lab_lib_for(dtype)
    max_keys = 2048
    g = torch.Generator(device=DEV).manual_seed(nh * 64 + nkv)

    def rnd(*shape):
        return torch.randn(*shape, generator=g, device=DEV).to(dtype)
    q, kmain, vmain = rnd(nh, 64, 128), rnd(nkv, max_keys, 128), rnd(nkv, max_keys, 128)
    kfr, vfr = rnd(nkv, 64, 128), rnd(nkv, 64, 128)
    qf = gu.to_packed(q, gu.rf_index(64), 8192).reshape(-1)
    km = gu.to_packed(kmain, gu.rf_index(max_keys), max_keys * 128).reshape(-1)
    vm = gu.to_packed(vmain, gu.vf_index(max_keys), max_keys * 128).reshape(-1)
    kf = gu.to_packed(kfr, gu.rf_index(64), 8192).reshape(-1)
    vf = gu.to_packed(vfr, gu.vf_index(64), 8192).reshape(-1)
    part = torch.zeros(nh * 64 * 128, dtype=torch.float32, device=DEV)       # the single-launch form writes no partials
    forms = _forms_that_fit(nh)
    assert forms
    old = lab.la_lab_get(KEY), lab.la_lab_get(17)
    try:
        check(lab.la_lab_set(17, 1), 'lab_set')
        for nkeys, T in ((0, 64), (5, 3), (70, 64), (225, 64), (226, 17), (333, 40), (640, 64), (990, 64), (1500, 33), (2040, 64)):
            rs = np.random.RandomState(nkeys + T)
            _, rows = random_tree(rs, T)
            rowmask = np.array([int(rows[t]) if t < T else (1 << t) for t in range(64)], dtype=np.uint64)
            rm = torch.from_numpy(rowmask.view(np.int64)).to(DEV)
            state = torch.zeros(_lib.LA_ST_WORDS, dtype=torch.int32, device=DEV)
            state[_lib.LA_ST_NKEYS] = nkeys

            def run(form):
                check(lab.la_lab_set(KEY, form), 'lab_set')
                out = torch.full((64 * nh * 128,), 77, dtype=dtype, device=DEV)      # every element must be stored by some workgroup
                check(lab.la_tree_attn(sp(), ptr(qf), ptr(km), ptr(vm), ptr(kf), ptr(vf), ptr(rm), ptr(state), nh, nkv, max_keys, 8,
                                       ptr(part), ptr(part), ptr(part), ptr(out)), 'tree_attn')
                torch.cuda.synchronize()
                return out.view(torch.int16)
            ref = run(0)
            assert not torch.equal(ref, torch.full_like(ref, ref[0].item()))
            for sl, dv, nkb in forms:
                got = run(_form(sl, dv, nkb))
                assert torch.equal(got, ref), (nkeys, T, sl, dv, nkb, int((got != ref).sum()))
    finally:
        lab.la_lab_set(KEY, old[0])
        lab.la_lab_set(17, old[1])


def _steps(eng, prompt_len, n_steps, seed, vocab):
    """reset + prefill + n_steps steps (random trees; every third a chain, which commits all its rows): (tokens, logits) of each."""
    eng.reset()
    rs = np.random.RandomState(seed)
    out = [(eng.prefill(rs.randint(3, vocab, size=prompt_len).tolist()), eng.logits().clone())]
    for step in range(n_steps):
        T = 64 if step % 2 == 0 else int(rs.randint(1, 64))
        _, rows = random_tree(rs, T)
        ids = rs.randint(3, vocab, size=T).astype(np.int32)
        toks = eng.step(ids, eng._CHAIN[:T], mode=1) if step % 3 == 2 else eng.step(ids, rows)
        out.append((toks, eng.logits()[:T].clone()))
    return out


def _same_steps(eng, forms, prompt_len, n_steps, seed, vocab):
    """One lab engine under every form in turn (a knob change captures the step graph again)."""
    assert forms
    with gu.debug_knob(KEY, 0):
        ref = _steps(eng, prompt_len, n_steps, seed, vocab)
    for sl, dv, nkb in forms:
        with gu.debug_knob(KEY, _form(sl, dv, nkb)):
            got = _steps(eng, prompt_len, n_steps, seed, vocab)
        for i, ((tr, lr), (tg, lg)) in enumerate(zip(ref, got)):
            assert tr == tg and torch.equal(lr, lg), (sl, dv, nkb, i)
    return ref


@pytest.mark.usefixtures('lab_build')
def test_whole_step_7b_shape_two_layers():
    """Three steps of a 2-layer model of the Llama-2-7B shape (the spec condition holds from the first step: 300 committed keys):
    logits and accepted tokens byte-equal under every form the shape takes."""
    shape = LlamaShape(2, 4096, 32, 32, 11008, 32000, 1e-5)
    sd = random_weights(shape, seed=3, device=DEV, decisive=True)
    eng = LlamaVerifyEngine(shape, sd, max_length=1024)
    assert eng.lab
    _same_steps(eng, _forms_that_fit(32), 300, 3, 5, shape.vocab)


@pytest.mark.parametrize('case', ['head_dim_64', 'head_dim_96', 'window', 'window_ring', 'short'])
@pytest.mark.usefixtures('lab_build')
def test_whole_step_narrow_heads_window_and_ring(case):
    """The paths the C ABI of the kernel does not parametrise, through the engine: heads of 64 / 96 dims in padded 128-feature lanes
    (another softmax scale; GQA), a sliding window (masked tiles, skipped tiles, no early first tile) with a linear cache and with the
    KV ring (ring-slot addressing of every request), and contexts below 226 keys (the early tile is requested but not used)."""
    if case.startswith('head_dim'):
        shape = LlamaShape(2, 256, 4, 2, 512, 512, 1e-5, head_dim=int(case[-2:]))
        sd = random_weights(shape, seed=7, device='cpu')
        kw, P, n = {}, 250, 6
    else:
        shape = tiny_shape()
        sd = {k: v.to(torch.bfloat16) for k, v in tiny_weights(4, torch.float32).items()}
        kw, P, n = {}, 40, 6
        if case != 'short':
            shape.sliding_window = 100
            kw, P, n = ({'kv_ring': True} if case == 'window_ring' else {}), 150, 36      # the context passes the ring size several times
    eng = LlamaVerifyEngine(shape, sd, max_length=2048, **kw)
    assert eng.lab
    _same_steps(eng, _forms_that_fit(shape.n_heads), P, n, 11, shape.vocab)
    if case == 'window_ring':
        assert eng.n_keys > 2 * eng.max_keys          # the ring wrapped
