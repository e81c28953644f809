# -*- coding: utf-8 -*-
"""FP8 (e4m3fn) weight-only projections on the MI355X: the conversion (exhaustive), the packers, every fp8 entry point against fp64
torch on W' = s * q and bit for bit against its 16-bit counterpart on e4m3-grid weights, and the engine end to end."""
import numpy as np
import pytest
import torch

from oracle import llama_oracle as lo
from painlessinferenceacceleration_amd import _lib
from painlessinferenceacceleration_amd._lib import check
from painlessinferenceacceleration_amd.llama_engine import (LlamaShape, LlamaVerifyEngine, dequantize_fp8, quantize_fp8,
                                                            random_weights, rope_tables)
from tests import gpu_utils as gu
from tests.gpu_utils import DEV, ptr, sp, random_tree
from tests.qwen2_oracle import OracleQwen2
from tests.tiny_model import tiny_shape, tiny_weights

pytestmark = pytest.mark.gpu
TOL = 2e-2                  # tests/test_gpu_e2e.py
DTYPES = [torch.bfloat16, torch.float16]


def _u8(q):
    return q.view(torch.uint8).contiguous()


def pack8(L, q, q2=None):
    n, k = q.shape
    out = torch.empty((2 if q2 is not None else 1) * n * k, dtype=torch.uint8, device=DEV)
    a, b = _u8(q), (_u8(q2) if q2 is not None else None)
    check(L.la_pack_weight_fp8(sp(), ptr(a), ptr(b) if b is not None else None, n, k, 1 if b is not None else 0, ptr(out)), 'pack8')
    torch.cuda.synchronize()
    return out


def _plan(L, kind, n_rows, nwg):
    n = L.la_rowplan(kind, n_rows, nwg, None)
    assert n > 0
    plan = np.zeros(n, dtype=np.int32)
    assert L.la_rowplan(kind, n_rows, nwg, plan.ctypes.data_as(_lib.pi32)) == n
    return torch.from_numpy(plan).to(DEV)


def pack_planned8(L, kind, mats, nwg):
    mats = [_u8(m) for m in mats]
    n_rows, K = mats[0].shape
    plan = _plan(L, kind, n_rows, nwg)
    out = torch.empty(L.la_planned_elems(kind, n_rows, K, nwg), dtype=torch.uint8, device=DEV)
    check(L.la_pack_planned_fp8(sp(), ptr(mats[0]), ptr(mats[1]) if len(mats) > 1 else None, ptr(plan), kind, n_rows, K, nwg,
                                ptr(out)), 'pack_planned8')
    torch.cuda.synchronize()
    return out


def pack16(L, kind, mats, nwg=0):
    """16-bit image of the same values (bit copies: the 16-bit packers move bits, whatever the storage type)"""
    if nwg == 0:
        return gu.pack_weight(*mats)
    n_rows, K = mats[0].shape
    plan = _plan(L, kind, n_rows, nwg)
    out = torch.empty(L.la_planned_elems(kind, n_rows, K, nwg), dtype=mats[0].dtype, device=DEV)
    check(L.la_pack_planned(sp(), ptr(mats[0]), ptr(mats[1]) if len(mats) > 1 else None, ptr(plan), kind, n_rows, K, nwg, ptr(out)), 'pp')
    torch.cuda.synchronize()
    return out


def pack_x(L, x):
    out = torch.empty_like(x).reshape(-1)
    check(L.la_pack_x(sp(), ptr(x), x.shape[1], ptr(out)), 'pack_x')
    return out


def _rand_q(n, k, g, scale_spread=True):
    w = torch.randn(n, k, generator=g, device=DEV) * 0.05
    if scale_spread:
        w = w * torch.logspace(-1, 1, n, device=DEV)[:, None]
    return quantize_fp8(w)


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('rb', [2, 2 | 3 << 8])
def test_conversion_is_exact_for_every_finite_e4m3_code(dtype, rb):
    """An image holding every finite e4m3 code (subnormals and -0 included), unit scales, one-hot x rows: the slab returns the
    values exactly."""
    L = _lib.lib_for(dtype)
    codes = torch.tensor([c for c in range(256) if (c & 0x7f) != 0x7f], dtype=torch.uint8)
    N, K = 256, 64
    flat = codes.repeat((N * K + len(codes) - 1) // len(codes))[:N * K]
    q = flat.reshape(K, N).t().contiguous().to(DEV).view(torch.float8_e4m3fn)        # column t holds codes t*256 .. t*256+255
    assert len(set(flat.tolist())) == 254
    x = torch.eye(64, K, dtype=dtype, device=DEV)
    scale = torch.ones(N, dtype=torch.float32, device=DEV)
    slabs = torch.full((1, 64, N), float('nan'), dtype=torch.float32, device=DEV)
    wp, xp = pack8(L, q), pack_x(L, x)
    check(L.la_gemm64_slab_fp8(sp(), ptr(wp), ptr(xp), N, K, rb, 1, ptr(slabs), ptr(scale)), 'slab8')
    torch.cuda.synchronize()
    assert torch.equal(slabs[0], q.float().t())


@pytest.mark.parametrize('dtype', DTYPES)
def test_pack_layouts_match_the_16bit_order_with_1_byte_elements(dtype):
    L = _lib.lib_for(dtype)
    g = torch.Generator(device=DEV).manual_seed(0)
    q, _ = _rand_q(96, 64, g)
    # WP8 tile (nb, kb) of 512 bytes: lane = n%32 + 32*((k%16)/8), byte e = k%8
    n = np.arange(96)[:, None]; k = np.arange(64)[None, :]
    idx = torch.from_numpy((((n >> 5) * 4 + (k >> 4)) * 512 + ((n & 31) + 32 * ((k >> 3) & 1)) * 8 + (k & 7)).astype(np.int64)).to(DEV)
    img = pack8(L, q)
    assert torch.equal(img[idx], _u8(q))
    # both image kinds: byte i of the fp8 image == low byte of element i of the 16-bit image of the codes
    for kind, mats, nwg in [(1, [q, _rand_q(96, 64, g)[0]], 2), (2, [_rand_q(3 * 128, 64, g)[0]], 16), (0, [q], 1)]:
        codes16 = [_u8(m).to(torch.int16).view(dtype) for m in mats]
        if nwg == 1:
            img8 = pack8(L, *mats)
            img16 = pack16(L, 0, codes16)
        else:
            img8 = pack_planned8(L, kind, mats, nwg)
            img16 = pack16(L, kind, codes16, nwg)
        assert img8.numel() == img16.numel()
        assert torch.equal(img8.to(torch.int16), img16.view(torch.int16) & 0xff)
    # gate/up interleave
    q2 = _rand_q(96, 64, g)[0]
    assert torch.equal(pack8(L, q, q2).to(torch.int16),
                       pack16(L, 0, [_u8(q).to(torch.int16).view(dtype), _u8(q2).to(torch.int16).view(dtype)]).view(torch.int16))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('N,K,rb,ks', [(4096, 4096, 2 | 3 << 8, 4), (4096, 11008, 2, 4), (512, 1104, 2, 3), (256, 4096, 2, 1),
                                       (5120, 5120, 2 | 3 << 8, 3)])
def test_slab_fp8_vs_fp64(N, K, rb, ks, dtype):
    L = _lib.lib_for(dtype)
    g = torch.Generator(device=DEV).manual_seed(N + K)
    x = torch.randn(64, K, generator=g, device=DEV).to(dtype)
    q, s = _rand_q(N, K, g)
    slabs = torch.full((ks, 64, N), float('nan'), dtype=torch.float32, device=DEV)
    wp, xp = pack8(L, q), pack_x(L, x)
    check(L.la_gemm64_slab_fp8(sp(), ptr(wp), ptr(xp), N, K, rb, ks, ptr(slabs), ptr(s)), 'slab8')
    torch.cuda.synchronize()
    ref = x.double() @ dequantize_fp8(q, s).double().t()
    assert gu.rel_err(slabs.sum(0), ref) < 2e-3, gu.rel_err(slabs.sum(0), ref)


def _swiglu_ref(x, wg, wu, dt):
    gg, uu = (x.double() @ wg.double().t()).to(dt), (x.double() @ wu.double().t()).to(dt)
    return (torch.nn.functional.silu(gg.float()).to(dt).float() * uu.float()).to(dt).float()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('F,K,nwg', [(1024, 512, 0), (11008, 4096, 0), (688, 512, 16), (11008, 4096, 256), (14336, 4096, 256)])
def test_swiglu_fp8_vs_fp64(F, K, nwg, dtype):
    L = _lib.lib_for(dtype)
    g = torch.Generator(device=DEV).manual_seed(F + nwg)
    x = torch.randn(64, K, generator=g, device=DEV).to(dtype)
    (qg, sg), (qu, su) = _rand_q(F, K, g), _rand_q(F, K, g)
    sc = torch.cat([sg, su]).contiguous()
    act = torch.zeros(64 * F, dtype=dtype, device=DEV)
    xp = pack_x(L, x)
    if nwg:
        wp = pack_planned8(L, 1, [qg, qu], nwg)
        check(L.la_gemm64r_swiglu_fp8(sp(), ptr(wp), ptr(xp), F, K, nwg, ptr(act), ptr(sc)), 'swiglu8r')
    else:
        wp = pack8(L, qg, qu)
        check(L.la_gemm64_swiglu_fp8(sp(), ptr(wp), ptr(xp), F, K, ptr(act), ptr(sc)), 'swiglu8')
    torch.cuda.synchronize()
    got = gu.from_packed(act, gu.xp_index(F)).float()
    ref = _swiglu_ref(x, dequantize_fp8(qg, sg), dequantize_fp8(qu, su), dtype)
    assert gu.rel_err(got, ref) < 2e-2, gu.rel_err(got, ref)


def _qkv_inputs(nh, nkv, K, seed, bias, dtype=torch.bfloat16):
    g = torch.Generator(device=DEV).manual_seed(seed)
    N = (nh + 2 * nkv) * 128
    x = torch.randn(64, K, generator=g, device=DEV).to(dtype)
    q, s = _rand_q(N, K, g)
    b = (torch.randn(N, generator=g, device=DEV) * 0.5).to(dtype) if bias else None
    pos = torch.randint(0, 900, (64,), generator=g, device=DEV, dtype=torch.int32)
    return x, q, s, b, pos


def _qkv_bufs(nh, nkv, dt=torch.bfloat16):
    return [torch.zeros(n * 8192, dtype=dt, device=DEV) for n in (nh, nkv, nkv)]


@pytest.mark.parametrize('nh,nkv,nwg,bias', [(32, 32, 256, False), (32, 8, 256, False), (28, 4, 256, True), (8, 2, 32, True),
                                             (32, 32, 0, False), (28, 4, 0, True), (40, 40, 256, False)])
@pytest.mark.parametrize('dtype', DTYPES)
def test_qkv_fp8_vs_fp64(nh, nkv, nwg, bias, dtype):
    """Reference: the fp64 product with W' in fp32 slabs through the 16-bit la_qkv_post(_bias) (the same bias, rounding and RoPE)."""
    L = _lib.lib_for(dtype)
    K = 512
    N = (nh + 2 * nkv) * 128
    x, q, s, b, pos = _qkv_inputs(nh, nkv, K, nh * 7 + nkv, bias, dtype)
    rc, rs_ = rope_tables(128, 1024, 10000.0, DEV, dtype)
    xp = pack_x(L, x)
    got = _qkv_bufs(nh, nkv, dtype)
    if nwg:
        wp = pack_planned8(L, 2, [q], nwg)
        check(L.la_gemm64r_qkv_fp8(sp(), ptr(wp), ptr(xp), nh, nkv, K, nwg, ptr(pos), ptr(rc), ptr(rs_), *[ptr(t) for t in got],
                                   ptr(b) if bias else None, ptr(s)), 'qkv8r')
    else:
        perm = np.zeros(N, dtype=np.int32)
        check(L.la_qkv_row_perm(nh, nkv, perm.ctypes.data_as(_lib.pi32)), 'perm')
        wp = pack8(L, q.view(torch.uint8).index_select(0, torch.from_numpy(perm.astype(np.int64)).to(DEV)).view(torch.float8_e4m3fn))
        sl = s                                                          # lane-ordered, whatever the row order of the image
        check(L.la_gemm64_qkv_fp8(sp(), ptr(wp), ptr(xp), nh, nkv, K, ptr(pos), ptr(rc), ptr(rs_), *[ptr(t) for t in got],
                                  ptr(b) if bias else None, ptr(sl)), 'qkv8')
    ref = _qkv_bufs(nh, nkv, dtype)
    slabs = (x.double() @ dequantize_fp8(q, s).double().t()).float().reshape(1, 64, N).contiguous()
    check(L.la_qkv_post_bias(sp(), ptr(slabs), 1, nh, nkv, ptr(pos), ptr(rc), ptr(rs_), *[ptr(t) for t in ref],
                             ptr(b) if bias else None), 'post')
    torch.cuda.synchronize()
    for a, r, name in zip(got, ref, 'qkv'):
        assert gu.rel_err(a.float(), r.float()) < 1e-2, (name, gu.rel_err(a.float(), r.float()))


# ---- bit for bit against the 16-bit launches: e4m3-grid weights, unit scales ---------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_every_fp8_launch_equals_its_16bit_launch_on_grid_weights(dtype):
    L = _lib.lib_for(dtype)
    g = torch.Generator(device=DEV).manual_seed(11)
    K = 1024
    x = torch.randn(64, K, generator=g, device=DEV).to(dtype)
    xp = pack_x(L, x)
    one = lambda n: torch.ones(n, dtype=torch.float32, device=DEV)      # noqa: E731
    # slab, both forms, 1-4 K splits
    N = 512
    q, _ = _rand_q(N, K, g)
    w16 = q.float().to(dtype)
    for rb in (2, 2 | 3 << 8):
        for ks in (1, 2, 3, 4):
            a = torch.zeros(ks, 64, N, device=DEV); b = torch.zeros(ks, 64, N, device=DEV)
            wp8, wp16 = pack8(L, q), pack16(L, 0, [w16])
            check(L.la_gemm64_slab_fp8(sp(), ptr(wp8), ptr(xp), N, K, rb, ks, ptr(a), ptr(one(N))), 'slab8')
            check(L.la_gemm64_slab(sp(), ptr(wp16), ptr(xp), N, K, rb, ks, ptr(b)), 'slab')
            torch.cuda.synchronize()
            assert torch.equal(a, b), (rb, ks)
    # swiglu: classic and balanced
    F = 688
    qg, qu = _rand_q(F, K, g)[0], _rand_q(F, K, g)[0]
    for nwg in (0, 16):
        a = torch.zeros(64 * F, dtype=dtype, device=DEV); b = torch.zeros_like(a)
        if nwg:
            wp8, wp16 = pack_planned8(L, 1, [qg, qu], nwg), pack16(L, 1, [qg.float().to(dtype), qu.float().to(dtype)], nwg)
            check(L.la_gemm64r_swiglu_fp8(sp(), ptr(wp8), ptr(xp), F, K, nwg, ptr(a), ptr(one(2 * F))), 'sw8r')
            check(L.la_gemm64r_swiglu(sp(), ptr(wp16), ptr(xp), F, K, nwg, ptr(b)), 'swr')
        else:
            F2 = 672
            a = a[:64 * F2]; b = b[:64 * F2]
            wp8, wp16 = pack8(L, qg[:F2], qu[:F2]), gu.pack_weight(qg[:F2].float().to(dtype), qu[:F2].float().to(dtype))
            check(L.la_gemm64_swiglu_fp8(sp(), ptr(wp8), ptr(xp), F2, K, ptr(a), ptr(one(2 * F2))), 'sw8')
            check(L.la_gemm64_swiglu(sp(), ptr(wp16), ptr(xp), F2, K, ptr(b), 0), 'sw')
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), nwg
    # qkv: classic and balanced, with and without the bias
    nh, nkv = 8, 2
    N = (nh + 2 * nkv) * 128
    q, _ = _rand_q(N, K, g)
    bias = (torch.randn(N, generator=g, device=DEV) * 0.5).to(dtype)
    pos = torch.randint(0, 900, (64,), generator=g, device=DEV, dtype=torch.int32)
    rc, rs_ = rope_tables(128, 1024, 10000.0, DEV, dtype)
    perm = np.zeros(N, dtype=np.int32)
    check(L.la_qkv_row_perm(nh, nkv, perm.ctypes.data_as(_lib.pi32)), 'perm')
    pi = torch.from_numpy(perm.astype(np.int64)).to(DEV)
    for nwg in (0, 32):
        for bb in (None, bias):
            a, b = _qkv_bufs(nh, nkv, dtype), _qkv_bufs(nh, nkv, dtype)
            if nwg:
                wp8, wp16 = pack_planned8(L, 2, [q], nwg), pack16(L, 2, [q.float().to(dtype)], nwg)
                check(L.la_gemm64r_qkv_fp8(sp(), ptr(wp8), ptr(xp), nh, nkv, K, nwg, ptr(pos), ptr(rc), ptr(rs_), *[ptr(t) for t in a],
                                           ptr(bb) if bb is not None else None, ptr(one(N))), 'q8r')
                check(L.la_gemm64r_qkv_bias(sp(), ptr(wp16), ptr(xp), nh, nkv, K, nwg, ptr(pos), ptr(rc), ptr(rs_), *[ptr(t) for t in b],
                                            ptr(bb) if bb is not None else None), 'qr')
            else:
                qp = q.view(torch.uint8).index_select(0, pi).view(torch.float8_e4m3fn)
                wp8, wp16 = pack8(L, qp), gu.pack_weight(qp.float().to(dtype))
                check(L.la_gemm64_qkv_fp8(sp(), ptr(wp8), ptr(xp), nh, nkv, K, ptr(pos), ptr(rc), ptr(rs_), *[ptr(t) for t in a],
                                          ptr(bb) if bb is not None else None, ptr(one(N))), 'q8')
                check(L.la_gemm64_qkv_bias(sp(), ptr(wp16), ptr(xp), nh, nkv, K, ptr(pos), ptr(rc), ptr(rs_), *[ptr(t) for t in b], 0,
                                           ptr(bb) if bb is not None else None), 'q')
            torch.cuda.synchronize()
            for u, v in zip(a, b):
                assert torch.equal(u.view(torch.int16), v.view(torch.int16)), (nwg, bb is not None)


# ---- engine ---------------------------------------------------------------------------------------------------------------------
def _mask(rows, T):
    return np.array([[(int(rows[i]) >> j) & 1 for j in range(T)] for i in range(T)], dtype=np.int64)


def _check_rows(got, ref, rows, what, tol=TOL):
    got, ref = got.float().cpu(), ref.float().cpu()
    worst = 0.0
    for t in rows:
        err = float((got[t] - ref[t]).abs().max()) / float(ref[t].abs().max())
        worst = max(worst, err)
        top = torch.topk(ref[t], 2).values
        if float(top[0] - top[1]) > 2 * err * float(ref[t].abs().max()) and err <= tol:
            assert int(got[t].argmax()) == int(ref[t].argmax()), f'{what}: row {t} argmax'
    assert worst <= tol, f'{what}: {worst:.4g} > {tol}'
    return worst


def _pow2_fp8_sd(sd):
    """(pre-quantized state dict, the bf16 state dict of W') with PER-ROW power-of-two scales: s[n] = 2^round(log2(amax / 448)), so
    that W' = s * q is exact in bf16 and the oracle computes with W' itself (arbitrary scales would give it bf16(W') instead, a
    second rounding of the weights the engine does not make)"""
    sd8, ref = {}, {}
    for k, v in sd.items():
        if k.endswith('_proj.weight') and k.startswith('model.layers.'):
            w = v.float()
            amax = w.abs().amax(1).clamp_min(1e-30)
            s = torch.pow(2.0, torch.round(torch.log2(amax / 448.0)))
            q = (w / s[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn)
            sd8[k], sd8[k[:-len('weight')] + 'weight_scale'] = q, s
            ref[k] = dequantize_fp8(q, s).to(torch.bfloat16)
            assert torch.equal(ref[k].float(), dequantize_fp8(q, s))
        else:
            sd8[k] = ref[k] = v.to(torch.bfloat16) if v.is_floating_point() else v
    return sd8, ref


def _run_vs_oracle(shape, sd, oracle, P, seed, what, **kw):
    eng = LlamaVerifyEngine(shape, dict(sd), max_length=512, **kw)
    assert eng.weight_format == 'fp8'
    rs = np.random.RandomState(seed)
    prompt = rs.randint(3, shape.vocab, size=P).tolist()
    tok = eng.prefill(prompt)                                     # 64-token steps (max_blocks = 0)
    lg0, past = oracle.forward(torch.tensor(prompt), torch.tril(torch.ones((P, P), dtype=torch.long)), None)
    last = (P - 1) // 64 * 64
    _check_rows(eng.logits()[:P - last], lg0[last:], range(P - last), what + ' prefill')
    T = 64
    _, rows = random_tree(rs, T)
    ids = np.concatenate([[tok], rs.randint(3, shape.vocab, size=T - 1)]).astype(np.int32)
    eng.step(ids, rows)
    full = torch.cat([torch.ones((T, P), dtype=torch.long), torch.from_numpy(_mask(rows, T))], 1)
    lg, _ = oracle.forward(torch.tensor(ids.tolist()), full, past)
    return eng, _check_rows(eng.logits(), lg, range(T), what + ' tree'), (prompt, ids, rows, lg)


@pytest.mark.parametrize('balanced', [True, False])
def test_tiny_engine_fp8_vs_oracle_on_dequantized_weights(balanced):
    shape = tiny_shape()
    sd8, ref = _pow2_fp8_sd(tiny_weights(0))
    _run_vs_oracle(shape, sd8, lo.OracleLlama(shape, ref), 150, 0, 'tiny', balanced=balanced)


def test_control_scales_forced_to_one_are_far_off():
    shape = tiny_shape()
    sd8, ref = _pow2_fp8_sd(tiny_weights(0))
    oracle = lo.OracleLlama(shape, ref)
    bad = dict(sd8)
    for k in list(bad):
        if k.endswith('.weight_scale'):
            bad[k] = torch.tensor(1.0)
    eng = LlamaVerifyEngine(shape, bad, max_length=512)
    assert eng.weight_format == 'fp8'
    rs = np.random.RandomState(0)
    prompt = rs.randint(3, shape.vocab, size=64).tolist()
    eng.prefill(prompt)
    lg0, _ = oracle.forward(torch.tensor(prompt), torch.tril(torch.ones((64, 64), dtype=torch.long)), None)
    got, ref = eng.logits()[:64].float().cpu(), lg0.float()
    err = float((got - ref).abs().max() / ref.abs().max())
    assert err > 10 * TOL, err


@pytest.mark.parametrize('name', ['llama2-7b', 'llama2-13b', 'mistral-7b', 'qwen2-7b'])
def test_real_layer_shapes_two_layers_fp8_vs_oracle(name):
    shape = {'llama2-7b': LlamaShape.llama2_7b, 'llama2-13b': LlamaShape.llama2_13b, 'mistral-7b': LlamaShape.mistral_7b,
             'qwen2-7b': LlamaShape.qwen2_7b}[name]()
    shape.n_layers = 2
    sd8, ref = _pow2_fp8_sd(random_weights(shape, seed=3, std=0.02, device='cpu'))
    oracle = OracleQwen2(shape, ref) if name == 'qwen2-7b' else lo.OracleLlama(shape, ref)
    eng, err, _ = _run_vs_oracle(shape, sd8, oracle, 40, 6, name)
    print(name, 'fp8 tree rel err', err, 'balanced', eng.balanced_wg)


def test_whole_step_bitwise_equals_bf16_engine_on_grid_weights():
    """Projections on the e4m3 grid with unit weight_scale: the fp8 engine IS the bf16 engine, bit for bit (graph step, eager
    step, prefill, sequential commit)."""
    shape = tiny_shape()
    sd = {k: v.to(torch.bfloat16) for k, v in tiny_weights(2).items()}
    sd8, sd16 = {}, {}
    for k, v in sd.items():
        if k.endswith('_proj.weight') and k.startswith('model.layers.'):
            q = quantize_fp8(v.float())[0]
            sd8[k], sd8[k[:-len('weight')] + 'weight_scale'] = q, torch.tensor(1.0)
            sd16[k] = q.float().to(torch.bfloat16)
        else:
            sd8[k] = sd16[k] = v
    rs = np.random.RandomState(3)
    prompt = rs.randint(3, shape.vocab, size=100).tolist()
    _, rows = random_tree(rs, 48)
    ids = rs.randint(3, shape.vocab, size=48).astype(np.int32)
    for kw in (dict(), dict(balanced=False)):
        outs = []
        for s in (sd8, sd16):
            eng = LlamaVerifyEngine(shape, dict(s), max_length=512, **kw)
            tok = eng.prefill(prompt)
            ids[0] = tok
            toks, n = eng.step(ids.copy(), rows)
            lg = eng.logits().clone()
            toks2, _ = eng.step(np.array([toks[-1]] + ids[1:].tolist(), dtype=np.int32), rows, eager=True)
            outs.append((tok, toks, n, lg, toks2, eng.logits().clone(), eng.weight_format))
        assert outs[0][6] == 'fp8' and outs[1][6] is None
        for a, b in zip(outs[0][:6], outs[1][:6]):
            assert (torch.equal(a, b) if torch.is_tensor(a) else a == b), kw


def test_cursor_batch_fp8_vs_oracle():
    """n_slots > 1: two sequences in one 64-row block share the fp8 launches; each segment's logits against the oracle on W'."""
    shape = tiny_shape()
    sd8, ref = _pow2_fp8_sd(tiny_weights(0))
    oracle = lo.OracleLlama(shape, ref)
    eng = LlamaVerifyEngine(shape, dict(sd8), max_length=512, n_slots=2)
    assert eng.weight_format == 'fp8'
    rs = np.random.RandomState(5)
    prompts = [rs.randint(3, shape.vocab, size=n).tolist() for n in (70, 45)]
    segs, refs = [], []
    for slot, pr in enumerate(prompts):
        tok = eng.bprefill(slot, pr)
        P = len(pr)
        lg0, past = oracle.forward(torch.tensor(pr), torch.tril(torch.ones((P, P), dtype=torch.long)), None)
        assert tok == int(lg0[-1].float().argmax())
        T = 32
        _, rows = random_tree(rs, T)
        ids = np.concatenate([[tok], rs.randint(3, shape.vocab, size=T - 1)]).astype(np.int32)
        segs.append((slot, ids, np.asarray(rows, dtype=np.uint64), 0, 16))
        full = torch.cat([torch.ones((T, P), dtype=torch.long), torch.from_numpy(_mask(rows, T))], 1)
        refs.append(oracle.forward(torch.tensor(ids.tolist()), full, past)[0])
    eng.bstep(segs)
    first = eng.bstep_rows()
    got = eng.logits()[:64].clone()
    # W' is exact in bf16 here, so the fp8 cursor batch IS the bf16 one on W', bit for bit; against the oracle, the tiny seeded model's
    # bf16 tail allowance of tests/test_gpu_mblock.py (TOL_TAIL = 3e-2) applies
    e16 = LlamaVerifyEngine(shape, dict(ref), max_length=512, n_slots=2)
    for slot, pr in enumerate(prompts):
        e16.bprefill(slot, pr)
    e16.bstep(segs)
    assert torch.equal(got, e16.logits()[:64])
    for slot, lg in enumerate(refs):
        _check_rows(got[first[slot]:first[slot] + 32], lg, range(32), f'bstep slot {slot}', tol=3e-2)


def test_sequential_commit_fp8_equals_the_fused_accept():
    """The sequential path (forward-only step, then commit of the accepted rows) leaves the same KV cache as the fused accept: the next
    step's logits are bitwise those of the engine that took the fused path, and both match the oracle."""
    shape = tiny_shape()
    sd8, ref = _pow2_fp8_sd(tiny_weights(1))
    oracle = lo.OracleLlama(shape, ref)
    rs = np.random.RandomState(8)
    prompt = rs.randint(3, shape.vocab, size=70).tolist()
    T = 48
    _, rows = random_tree(rs, T)
    a = LlamaVerifyEngine(shape, dict(sd8), max_length=512)
    b = LlamaVerifyEngine(shape, dict(sd8), max_length=512)
    tok = a.prefill(prompt)
    assert b.prefill(prompt) == tok
    ids = np.concatenate([[tok], rs.randint(3, shape.vocab, size=T - 1)]).astype(np.int32)
    toks, n = b.step(ids, rows)
    kept = b.state().cpu().numpy()[72:72 + n].tolist()
    a.verify_only(ids, rows)
    a.commit(kept)
    assert a.n_keys == b.n_keys == len(prompt) + n
    _, rows2 = random_tree(rs, 40)
    ids2 = np.concatenate([[toks[-1]], rs.randint(3, shape.vocab, size=39)]).astype(np.int32)
    a.step(ids2, rows2)
    b.step(ids2, rows2)
    assert torch.equal(a.logits()[:40], b.logits()[:40])
    seq = prompt + [int(ids[r]) for r in kept]
    C = len(seq)
    mask = torch.cat([torch.ones((40, C), dtype=torch.long), torch.from_numpy(_mask(rows2, 40))], 1)
    lg, _ = oracle.forward(torch.tensor(seq + ids2.tolist()), torch.cat([torch.cat([torch.tril(torch.ones((C, C), dtype=torch.long)),
                                                                                   torch.zeros((C, 40), dtype=torch.long)], 1), mask], 0), None)
    _check_rows(a.logits()[:40], lg[C:], range(40), 'after commit')


def test_tiny_head_dim_64_gqa_fp8_vs_oracle():
    """head_dim 64 (heads spread over padded 128-feature lanes: q/k/v rows and o_proj columns moved as bytes, padding scales 1) with GQA,
    balanced and classic images."""
    shape = LlamaShape(2, 256, 4, 2, 512, 512, 1e-5, head_dim=64)
    sd8, ref = _pow2_fp8_sd(random_weights(shape, seed=7, device='cpu'))
    assert sd8['model.layers.0.self_attn.q_proj.weight'].shape == (4 * 64, 256)
    for balanced in (True, False):
        _run_vs_oracle(shape, sd8, lo.OracleLlama(shape, ref), 100, 2, f'hd64 balanced={balanced}', balanced=balanced)


def test_generate_from_hf_fp8_equals_greedy_and_transformers():
    transformers = pytest.importorskip('transformers')
    from painlessinferenceacceleration_amd.modeling_llama import LlamaForCausalLM
    cfg = transformers.LlamaConfig(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
                                   num_key_value_heads=2, max_position_embeddings=1024, rms_norm_eps=1e-5, tie_word_embeddings=False)
    torch.manual_seed(0)
    hf = transformers.LlamaForCausalLM(cfg).eval()
    with torch.no_grad():                           # decisive: large logits margins, so bf16 / fp8 numerics cannot flip a token
        hf.lm_head.weight.mul_(8.0)
    model = LlamaForCausalLM.from_hf(hf, weight_format='fp8', max_length=512, dtype=torch.bfloat16)
    rs = np.random.RandomState(0)
    prompt = rs.randint(3, 512, size=40).tolist()
    def gen(m, la):
        return m.generate(input_ids=torch.tensor([prompt]), max_new_tokens=48, pad_token_id=2, eos_token_id=None,
                          decoding_kwargs={'use_lookahead': la, 'decoding_length': 64, 'branch_length': 12})[0].tolist()
    la, gr = gen(model, True), gen(model, False)
    assert la == gr
    # transformers' greedy tokens on the CPU with W' loaded
    hf2 = transformers.LlamaForCausalLM(cfg).eval()
    dq = {}
    for k, v in hf.state_dict().items():
        dq[k] = dequantize_fp8(*quantize_fp8(v.float())) if (k.endswith('_proj.weight') and 'layers.' in k) else v
    hf2.load_state_dict(dq)
    with torch.no_grad():
        ref = hf2.generate(torch.tensor([prompt]), max_new_tokens=48, do_sample=False, pad_token_id=0, eos_token_id=None)[0].tolist()
    # bf16 activations against fp32 transformers on W': every token agrees up to the first position where transformers' own top-2 gap
    # is a near-tie (below 1 % of its largest logit), and that position is past the first 24 new tokens
    for i in range(len(prompt), len(ref)):
        if la[i] != ref[i]:
            with torch.no_grad():
                lg = hf2(torch.tensor([ref[:i]])).logits[0, -1].float()
            top = torch.topk(lg, 2).values
            assert float(top[0] - top[1]) < 1e-2 * float(lg.abs().max()), (i, la[len(prompt):], ref[len(prompt):])
            assert i - len(prompt) >= 24, (i, la[len(prompt):], ref[len(prompt):])
            break
    # a pre-quantized state dict of the same q / s gives the same tokens
    sd8 = {}
    for k, v in hf.state_dict().items():
        if k.endswith('_proj.weight') and 'layers.' in k:
            q, s = quantize_fp8(v.float())
            sd8[k], sd8[k[:-len('weight')] + 'weight_scale'] = q, s
        else:
            sd8[k] = v
    from painlessinferenceacceleration_amd.llama_engine import LlamaShape as _S, legacy_state_dict
    shape = _S.from_hf(cfg)
    m2 = LlamaForCausalLM(shape, legacy_state_dict(sd8, shape), max_length=512, dtype=torch.bfloat16)
    assert m2.engine.weight_format == 'fp8'
    assert gen(m2, True) == la


def test_full_size_llama7b_fp8_lookahead_equals_greedy_and_half_the_bytes():
    """32-layer Llama-2-7B-shaped decisive model in fp8: lookahead output == greedy output; the projection images, scales included,
    take <= 0.51x the bytes of the bf16 engine's (measured sizes of the packed images, LlamaVerifyEngine.weight_bytes); lm_head and
    the embedding are unchanged."""
    from painlessinferenceacceleration_amd.modeling_llama import LlamaForCausalLM
    shape = LlamaShape.llama2_7b()
    sizes = {}
    for fmt in (None, 'fp8'):
        model = LlamaForCausalLM.random_init(shape, seed=0, decisive=True, max_length=512, weight_format=fmt)
        assert model.engine.weight_format == fmt
        sizes[fmt] = dict(model.engine.weight_bytes)
        if fmt == 'fp8':
            rs = np.random.RandomState(0)
            prompt = rs.randint(3, shape.vocab, size=64).tolist()

            def gen(la):
                return model.generate(input_ids=torch.tensor([prompt]), max_new_tokens=64, pad_token_id=2, eos_token_id=None,
                                      decoding_kwargs={'use_lookahead': la, 'decoding_length': 64, 'branch_length': 12})[0].tolist()
            gr = gen(False)
            assert gen(True) == gr and len(gr) == 128
        del model
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    r = sizes['fp8']['projections'] / sizes[None]['projections']
    print('projection image bytes fp8 / bf16:', r, sizes)
    assert r <= 0.51, r
    assert sizes['fp8']['lm_head'] == sizes[None]['lm_head'] and sizes['fp8']['embed'] == sizes[None]['embed']


def test_create_refuses_max_blocks_and_mixtral_shapes():
    shape = tiny_shape()
    sd = {k: v.to(torch.bfloat16) for k, v in tiny_weights(0).items()}
    with pytest.raises(ValueError, match='max_blocks'):
        LlamaVerifyEngine(shape, dict(sd), max_length=256, weight_format='fp8', max_blocks=2)
    mx = LlamaShape(2, 256, 2, 2, 512, 512, 1e-5, n_experts=4, top_k=2)
    with pytest.raises(ValueError, match='MoE'):
        LlamaVerifyEngine(mx, random_weights(mx, device='cpu'), max_length=256, weight_format='fp8')
