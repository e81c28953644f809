# -*- coding: utf-8 -*-
"""-m gpu: the Qwen2 family — q/k/v bias in every QKV epilogue (la_gemm64r_qkv_bias, la_gemm64_qkv_bias, la_qkv_post_bias,
la_mb_gemm_bias) and the engine / wrappers built on it.

* kernels: x W^T + b in fp32, rounded once to the storage type, then RoPE in storage-type arithmetic (F.linear with a bias +
  apply_rotary_pos_emb) — for GQA and MHA, head_dim 128 and 64 (padding lanes), the balanced, classic and multi-block images,
  1-4 K splits on the unfused path, 1-8 blocks, both dtypes.  A NULL bias and an all-zero bias are BITWISE the entry points
  without the suffix;
* engine: a tiny Qwen2 vs tests/qwen2_oracle.py through step, the cursor batch, mstep, prefill chains and the other QKV forms;
  the real Qwen2.5-7B / Qwen2-0.5B layer shapes; the front door (from_hf + generate) vs transformers greedy; and a sensitivity
  control (the same model without its biases is far outside the tolerance)."""
import numpy as np
import pytest
import torch

from painlessinferenceacceleration_amd import _lib
from painlessinferenceacceleration_amd._lib import check
from painlessinferenceacceleration_amd.llama_engine import LlamaShape, LlamaVerifyEngine, random_weights, rope_tables
from tests import gpu_utils as gu
from tests.gpu_utils import DEV, ptr, random_tree, sp
from tests.qwen2_oracle import OracleQwen2
from tests.test_gpu_e2e import TOL, _check_rows, _mask_from_rows

pytestmark = pytest.mark.gpu

TINY = dict(tol=TOL, tail_tol=3e-2, tail_frac=0.10)      # the tiny-model tail documented in tests/test_gpu_mblock.py
DTYPES = [torch.bfloat16, torch.float16]


# ------------------------------------------------------------------------------------------------------------------- kernels
def _lanes(t, n_h, hd):
    """[n_h * hd, ...] -> [n_h * 128, ...]: la_head_lane_map (feature d -> lane d, d + hd/2 -> lane 64 + d, zeros elsewhere)"""
    if hd == 128:
        return t
    src = np.zeros(128, dtype=np.int32)
    check(_lib.lib.la_head_lane_map(hd, src.ctypes.data_as(_lib.pi32)), 'lane_map')
    s = torch.from_numpy(src.astype(np.int64)).to(t.device)
    idx = (torch.arange(n_h, device=t.device)[:, None] * hd + s.clamp(min=0)[None, :]).reshape(-1)
    keep = (s >= 0).repeat(n_h).to(t.dtype)
    out = t.index_select(0, idx)
    return out * keep.reshape([-1] + [1] * (t.dim() - 1))


class _Case(object):
    """One QKV projection in 128-feature lanes: x [nblk*64, K], W [(nh+2nkv)*128, K], lane-ordered bias, RoPE tables, positions."""

    def __init__(self, nh, nkv, hd, dt, nblk=1, K=512, seed=0):
        g = torch.Generator(device=DEV).manual_seed(seed * 131 + nh * 7 + nkv + hd + nblk)
        self.nh, self.nkv, self.hd, self.dt, self.nblk, self.K = nh, nkv, hd, dt, nblk, K
        self.N = (nh + 2 * nkv) * 128
        self.x = (torch.randn(nblk * 64, K, generator=g, device=DEV)).to(dt)
        ws, bs = [], []
        for n in (nh, nkv, nkv):
            ws.append(_lanes((torch.randn(n * hd, K, generator=g, device=DEV) * 0.05).to(dt), n, hd))
            b = torch.randn(n * hd, generator=g, device=DEV) * 0.3
            b[::5] *= 10.0                                   # a few large entries, as trained Qwen2 K biases
            bs.append(_lanes(b.to(dt)[:, None], n, hd)[:, 0])
        self.w = torch.cat(ws).contiguous()
        self.bias = torch.cat(bs).contiguous()
        self.zero = torch.zeros_like(self.bias)
        self.pos = torch.randint(0, 900, (nblk * 64,), generator=g, device=DEV, dtype=torch.int32)
        rc, rs_ = rope_tables(hd, 1024, 1e6, DEV, dt)
        if hd < 128:
            c = torch.ones((1024, 64), dtype=dt, device=DEV)
            s = torch.zeros((1024, 64), dtype=dt, device=DEV)
            c[:, :hd // 2], s[:, :hd // 2] = rc, rs_
            rc, rs_ = c, s
        self.rc, self.rs = rc.contiguous(), rs_.contiguous()
        self.xp = torch.cat([gu.pack_x(self.x[b * 64:(b + 1) * 64].contiguous()) for b in range(nblk)])
        # x W^T in fp32 by the library's own split-K GEMM (same matrix cores; one K split): the reference then differs from every QKV
        # form by the fp32 summation order only.  (A float64 matmul would not do for float16: the matrix cores' fp32 sums sit ~1e-4
        # relative from the exact value, half a float16 ulp, which moves ~15 % of the rounded elements.)
        L = _lib.lib_for(dt)
        wp = gu.pack_weight(self.w.view(torch.bfloat16))
        self.acc = torch.zeros(nblk, 64, self.N, dtype=torch.float32, device=DEV)
        for b in range(nblk):
            check(L.la_gemm64_slab(sp(), ptr(wp), ptr(self.xp[b * 64 * K:(b + 1) * 64 * K]), self.N, K, 2, 1, ptr(self.acc[b])), 'slab')
        torch.cuda.synchronize()
        self.acc = self.acc.reshape(nblk * 64, self.N)

    def outs(self):
        nb = self.nblk
        return (torch.zeros(nb * self.nh * 8192, dtype=torch.bfloat16, device=DEV),
                torch.zeros(nb * self.nkv * 8192, dtype=torch.bfloat16, device=DEV),
                torch.zeros(nb * self.nkv * 8192, dtype=torch.bfloat16, device=DEV))

    def ref(self, with_bias=True):
        """per block: q, k [64, heads, 128] after RoPE, v [64, nkv, 128] in the storage type"""
        dt = self.dt
        y = self.acc + self.bias.float() if with_bias else self.acc        # fp32 epilogue, one rounding (F.linear with a bias)
        y = y.to(dt)
        out = []
        for b in range(self.nblk):
            yb = y[b * 64:(b + 1) * 64]
            p = self.pos[b * 64:(b + 1) * 64].long()
            cos = torch.cat([self.rc[p], self.rc[p]], -1)[:, None]
            sin = torch.cat([self.rs[p], self.rs[p]], -1)[:, None]

            def rope(t):
                return (t * cos) + (torch.cat((-t[..., 64:], t[..., :64]), -1) * sin)
            q = yb[:, :self.nh * 128].view(64, self.nh, 128)
            k = yb[:, self.nh * 128:(self.nh + self.nkv) * 128].view(64, self.nkv, 128)
            v = yb[:, (self.nh + self.nkv) * 128:].view(64, self.nkv, 128)
            out.append((rope(q), rope(k), v))
        return out

    def unpack(self, qf, kf, vf, b):
        nh, nkv, dt = self.nh, self.nkv, self.dt
        return (gu.from_packed(qf.view(dt)[b * nh * 8192:(b + 1) * nh * 8192].view(nh, 8192), gu.rf_index(64)).transpose(0, 1),
                gu.from_packed(kf.view(dt)[b * nkv * 8192:(b + 1) * nkv * 8192].view(nkv, 8192), gu.rf_index(64)).transpose(0, 1),
                gu.from_packed(vf.view(dt)[b * nkv * 8192:(b + 1) * nkv * 8192].view(nkv, 8192), gu.vf_index(64)).transpose(0, 1))

    def check(self, res, what):
        """res['bias'] vs the reference with the bias, res['null'] vs the one without.  V (no RoPE) must match all but the fp32
        summation-order moves (< 3 % of elements by one ulp).  Q / K: the RoPE of the float16 build sits one ulp from torch's float16
        eager arithmetic on ~18 % of elements with or without a bias (bias-free kernels of the parent, unchanged here), so the bar is
        the SAME as the bias-free launch's own distance to its reference, + 3 %."""
        ref, ref0 = self.ref(True), self.ref(False)
        for b in range(self.nblk):
            got, got0 = self.unpack(*res['bias'], b), self.unpack(*res['null'], b)
            for g_, g0, r, r0, name in zip(got, got0, ref[b], ref0[b], 'qkv'):
                err = gu.rel_err(g_.float(), r.float())
                assert err < 1e-2, (what, b, name, err)
                frac, frac0 = float((g_ != r).float().mean()), float((g0 != r0).float().mean())
                assert frac < 0.03 + (frac0 if name != 'v' else 0.0), (what, b, name, frac, frac0)
                assert gu.rel_err(r0.float(), r.float()) > 5e-2, 'the case cannot see the bias'


def _three(fn, case):
    """fn(bias_ptr, qf, kf, vf) with the bias, NULL and all-zero; the bias-free entry point is `fn(None, ...)` with bias=False"""
    res = {}
    for tag, b in (('bias', case.bias), ('null', None), ('zero', case.zero)):
        o = case.outs()
        fn(b, *o)
        torch.cuda.synchronize()
        res[tag] = o
    return res


def _bitwise(a, b, what):
    for x, y, name in zip(a, b, 'qkv'):
        assert torch.equal(x, y), (what, name, int((x != y).sum()))


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('nh,nkv,hd,nwg', [(3, 1, 128, 16), (4, 4, 128, 32), (5, 1, 128, 32), (8, 2, 64, 32), (4, 4, 64, 32)])
def test_gemm64r_qkv_bias(dt, nh, nkv, hd, nwg):
    L = _lib.lib_for(dt)
    c = _Case(nh, nkv, hd, dt)
    wp = gu.pack_planned(2, [c.w.view(torch.bfloat16)], nwg)

    def run(b, qf, kf, vf):
        check(L.la_gemm64r_qkv_bias(sp(), ptr(wp), ptr(c.xp), nh, nkv, c.K, nwg, ptr(c.pos), ptr(c.rc), ptr(c.rs), ptr(qf), ptr(kf),
                                    ptr(vf), ptr(b)), 'qkv_r_bias')
    r = _three(run, c)
    plain = c.outs()
    check(L.la_gemm64r_qkv(sp(), ptr(wp), ptr(c.xp), nh, nkv, c.K, nwg, ptr(c.pos), ptr(c.rc), ptr(c.rs), *map(ptr, plain)), 'qkv_r')
    torch.cuda.synchronize()
    _bitwise(r['null'], plain, 'null')
    _bitwise(r['zero'], plain, 'zero')
    c.check(r, 'gemm64r')


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('nh,nkv,hd', [(2, 2, 128), (8, 2, 128), (4, 2, 64)])
def test_gemm64_qkv_bias_classic_image(dt, nh, nkv, hd):
    L = _lib.lib_for(dt)
    c = _Case(nh, nkv, hd, dt)
    perm = np.zeros(c.N, dtype=np.int32)
    check(L.la_qkv_row_perm(nh, nkv, perm.ctypes.data_as(_lib.pi32)), 'perm')
    wp = gu.pack_weight(c.w[torch.from_numpy(perm.astype(np.int64)).to(DEV)].contiguous().view(torch.bfloat16))

    def run(b, qf, kf, vf):
        check(L.la_gemm64_qkv_bias(sp(), ptr(wp), ptr(c.xp), nh, nkv, c.K, ptr(c.pos), ptr(c.rc), ptr(c.rs), ptr(qf), ptr(kf), ptr(vf),
                                   0, ptr(b)), 'qkv_bias')
    r = _three(run, c)
    plain = c.outs()
    check(L.la_gemm64_qkv(sp(), ptr(wp), ptr(c.xp), nh, nkv, c.K, ptr(c.pos), ptr(c.rc), ptr(c.rs), *map(ptr, plain), 0), 'qkv')
    torch.cuda.synchronize()
    _bitwise(r['null'], plain, 'null')
    _bitwise(r['zero'], plain, 'zero')
    c.check(r, 'gemm64')


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('ks', [1, 2, 3, 4])
@pytest.mark.parametrize('nh,nkv,hd', [(2, 2, 128), (8, 2, 64)])
def test_qkv_post_bias_adds_once_to_the_sum_of_the_splits(dt, ks, nh, nkv, hd):
    L = _lib.lib_for(dt)
    c = _Case(nh, nkv, hd, dt, K=768)
    wp = gu.pack_weight(c.w.view(torch.bfloat16))
    slabs = torch.zeros(ks, 64, c.N, dtype=torch.float32, device=DEV)
    check(L.la_gemm64_slab(sp(), ptr(wp), ptr(c.xp), c.N, c.K, 2, ks, ptr(slabs)), 'slab')

    def run(b, qf, kf, vf):
        check(L.la_qkv_post_bias(sp(), ptr(slabs), ks, nh, nkv, ptr(c.pos), ptr(c.rc), ptr(c.rs), ptr(qf), ptr(kf), ptr(vf), ptr(b)),
              'post_bias')
    r = _three(run, c)
    plain = c.outs()
    check(L.la_qkv_post(sp(), ptr(slabs), ks, nh, nkv, ptr(c.pos), ptr(c.rc), ptr(c.rs), *map(ptr, plain)), 'post')
    torch.cuda.synchronize()
    _bitwise(r['null'], plain, 'null')
    _bitwise(r['zero'], plain, 'zero')
    c.check(r, f'post ks={ks}')


# (nh, nkv, hd, n_wg): classic image (0), balanced images (one workgroup per CU: R = 12 / 30 / 24 pairs), and the fuller multi-block image
# (cfg.qkv_mb_wg: 96 workgroups x 32 pairs) — RoPE groups of 4, 2 and 1 rows per store
MB_IMAGES = [(2, 2, 128, 0), (8, 2, 128, 0), (32, 8, 128, 256), (32, 8, 128, 96), (40, 40, 128, 256), (14, 2, 64, 48), (4, 2, 64, 0)]


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('nblk', [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize('nh,nkv,hd,nwg', MB_IMAGES)
def test_mb_gemm_bias(dt, nblk, nh, nkv, hd, nwg):
    L = _lib.lib_for(dt)
    c = _Case(nh, nkv, hd, dt, nblk=nblk)
    if nwg:
        wp = gu.pack_planned(2, [c.w.view(torch.bfloat16)], nwg)
    else:
        perm = np.zeros(c.N, dtype=np.int32)
        check(L.la_qkv_row_perm(nh, nkv, perm.ctypes.data_as(_lib.pi32)), 'perm')
        wp = gu.pack_weight(c.w[torch.from_numpy(perm.astype(np.int64)).to(DEV)].contiguous().view(torch.bfloat16))

    def mb(b, qf, kf, vf, fn=L.la_mb_gemm_bias):
        args = [sp(), 2, ptr(wp), ptr(c.xp), c.N, c.K, nblk, nwg, 1, None, 0, None, None, None, None, ptr(c.pos), ptr(c.rc), ptr(c.rs),
                ptr(qf), ptr(kf), ptr(vf), nh, nkv]
        check(fn(*args, ptr(b)) if fn is L.la_mb_gemm_bias else fn(*args), 'mb_gemm')
    r = _three(mb, c)
    plain = c.outs()
    mb(None, *plain, fn=L.la_mb_gemm)
    torch.cuda.synchronize()
    _bitwise(r['null'], plain, 'null')
    _bitwise(r['zero'], plain, 'zero')
    c.check(r, f'mb nblk={nblk} nwg={nwg}')


def test_bias_arguments_are_checked():
    L = _lib.lib
    c = _Case(2, 2, 128, torch.bfloat16)
    qf, kf, vf = c.outs()
    wp = gu.pack_planned(2, [c.w], 16)
    odd = c.bias[1:]                                            # not 8-byte aligned
    assert L.la_gemm64r_qkv_bias(sp(), ptr(wp), ptr(c.xp), 2, 2, c.K, 16, ptr(c.pos), ptr(c.rc), ptr(c.rs), ptr(qf), ptr(kf), ptr(vf),
                                 ptr(odd)) == -1
    # a bias on a GEMM kind that has no q/k/v epilogue is refused, never ignored
    slabs = torch.zeros(1, 64, 256, dtype=torch.float32, device=DEV)
    w0 = gu.pack_weight(c.w[:256].contiguous())
    assert L.la_mb_gemm_bias(sp(), 0, ptr(w0), ptr(c.xp), 256, c.K, 1, 0, 1, ptr(slabs), 64, None, None, None, None, None, None, None,
                             None, None, None, 0, 0, ptr(c.bias)) == -1


@pytest.mark.usefixtures('lab_build')
def test_lab_variant_without_epilogue_refuses_a_bias():
    """The measurement build of the wide launch without an epilogue (lab key 4 = 4) would drop the bias: LA_E_ARG instead."""
    lab = _lib.lab_lib_for('bfloat16')
    c = _Case(8, 2, 128, torch.bfloat16, nblk=4)
    wp = gu.pack_planned(2, [c.w], 32)
    qf, kf, vf = c.outs()
    args = [sp(), 2, ptr(wp), ptr(c.xp), c.N, c.K, 4, 32, 1, None, 0, None, None, None, None, ptr(c.pos), ptr(c.rc), ptr(c.rs),
            ptr(qf), ptr(kf), ptr(vf), 8, 2]
    with gu.debug_knob(4, 4):
        assert lab.la_mb_gemm_bias(*args, ptr(c.bias)) == -1


# -------------------------------------------------------------------------------------------------------------------- engine
def _tiny(hd=128, layers=2):
    if hd == 128:
        return LlamaShape(layers, 256, 2, 1, 512, 512, 1e-6, rope_theta=1e6, norm_cast_first=True, qkv_bias=True)
    return LlamaShape(layers, 256, 4, 2, 512, 512, 1e-6, rope_theta=1e6, head_dim=64, norm_cast_first=True, qkv_bias=True)


def _sd(shape, seed=3, dt=torch.bfloat16, tied=False):
    sd = random_weights(shape, seed=seed, std=0.08, dtype=torch.float32)
    sd = {k: v.to(dt) for k, v in sd.items()}
    if tied:
        sd['lm_head.weight'] = sd['model.embed_tokens.weight']
    return sd


def _tree(rs, T, vocab):
    _, rows = random_tree(rs, T)
    return rs.randint(3, vocab, size=T).astype(np.int32), rows


def _oracle_tree(oracle, past, nkeys, ids, rows):
    T = len(ids)
    mask = _mask_from_rows(rows, T)
    full = torch.cat([torch.ones((T, nkeys), dtype=torch.long), torch.from_numpy(mask)], 1)
    lg, _ = oracle.forward(torch.tensor(np.asarray(ids).tolist()), full, past)
    return lg


@pytest.mark.parametrize('hd,tied', [(128, False), (64, True)])
@pytest.mark.parametrize('kw', [dict(), dict(balanced=False), dict(gemm_cfg=[0, -1]), dict(fuse=2)],
                         ids=['balanced', 'classic', 'unfused_post', 'fused_norm'])
def test_engine_step_and_prefill_chain_match_the_oracle(hd, tied, kw):
    shape = _tiny(hd)
    sd = _sd(shape, tied=tied)
    oracle = OracleQwen2(shape, sd)
    eng = LlamaVerifyEngine(shape, dict(sd), max_length=384, **kw)
    rs = np.random.RandomState(hd)
    prompt = rs.randint(3, shape.vocab, size=150).tolist()             # a prefill chain of three 64-row blocks
    tok = eng.prefill(prompt)
    P = len(prompt)
    lg0, past = oracle.forward(torch.tensor(prompt), torch.tril(torch.ones((P, P), dtype=torch.long)), None)
    _check_rows(eng.logits()[:(P - 1) % 64 + 1], lg0[(P - 1) // 64 * 64:], range((P - 1) % 64 + 1), 'prefill', **TINY)
    ids, rows = _tree(rs, 64, shape.vocab)
    eng.verify_only(ids, rows)
    ref = _oracle_tree(oracle, past, P, ids, rows)
    _check_rows(eng.logits()[:64], ref, range(64), f'tree {kw}', **TINY)


@pytest.mark.parametrize('B', [2, 4, 8])
def test_mstep_and_cursor_batch_match_the_oracle(B):
    shape = _tiny(128)
    sd = _sd(shape, seed=5)
    oracle = OracleQwen2(shape, sd)
    eng = LlamaVerifyEngine(shape, dict(sd), max_length=384, n_slots=B, max_blocks=B)
    rs = np.random.RandomState(B)
    prompts = [rs.randint(3, shape.vocab, size=int(rs.randint(5, 60))).tolist() for _ in range(B)]
    pasts = []
    for b, p in enumerate(prompts):
        eng.mprefill(b, p)
        P = len(p)
        lg, past = oracle.forward(torch.tensor(p), torch.tril(torch.ones((P, P), dtype=torch.long)), None)
        _check_rows(eng.mlogits()[:P], lg, range(P), f'mprefill {b}', **TINY)
        pasts.append(past)
    trees = [_tree(rs, 64, shape.vocab) for _ in range(B)]
    eng.mstep([(b, trees[b][0], trees[b][1], 2, 16) for b in range(B)])
    got = eng.mlogits()
    for b in range(B):
        ref = _oracle_tree(oracle, pasts[b], len(prompts[b]), *trees[b])
        _check_rows(got[b * 64:(b + 1) * 64], ref, range(64), f'mstep block {b}', **TINY)
    # the cursor batch (la_llama_bstep): every slot prefilled through the 64-row step
    engb = LlamaVerifyEngine(shape, dict(sd), max_length=384, n_slots=B)
    for b, p in enumerate(prompts[:2]):
        engb.bprefill(b, p)
        P = len(p)
        lg, _ = oracle.forward(torch.tensor(p), torch.tril(torch.ones((P, P), dtype=torch.long)), None)
        _check_rows(engb.logits()[:P], lg, range(P), f'bprefill {b}', **TINY)


def test_sensitivity_control_without_the_biases_is_far_off():
    shape = _tiny(128)
    sd = _sd(shape, seed=7)
    oracle = OracleQwen2(shape, sd)
    sd0 = {k: (torch.zeros_like(v) if k.endswith('.bias') else v) for k, v in sd.items()}
    rs = np.random.RandomState(1)
    prompt = rs.randint(3, shape.vocab, size=48).tolist()
    P = len(prompt)
    ref, _ = oracle.forward(torch.tensor(prompt), torch.tril(torch.ones((P, P), dtype=torch.long)), None)
    errs = []
    for s in (sd, sd0):
        eng = LlamaVerifyEngine(shape, dict(s), max_length=256)
        eng.prefill(prompt)
        got = eng.logits()[:P].float().cpu()
        errs.append(max(float((got[i] - ref[i].float()).abs().max() / ref[i].float().abs().max()) for i in range(P)))
        del eng
    assert errs[0] < 3e-2 and errs[1] > 0.2, errs


@pytest.mark.parametrize('preset', ['qwen2_7b', 'qwen2_0_5b'])
def test_real_layer_shapes_two_layers(preset):
    shape = getattr(LlamaShape, preset)()
    shape.n_layers = 2
    sd = random_weights(shape, seed=2, device=DEV)
    if preset == 'qwen2_0_5b':
        sd['lm_head.weight'] = sd['model.embed_tokens.weight']
    cpu = {k: v.cpu() for k, v in sd.items()}
    oracle = OracleQwen2(shape, cpu)
    eng = LlamaVerifyEngine(shape, sd, max_length=256, n_slots=2, max_blocks=2)
    rs = np.random.RandomState(3)
    prompt = rs.randint(3, shape.vocab, size=40).tolist()
    eng.prefill(prompt)
    P = len(prompt)
    assert P <= 64
    lg0, past = oracle.forward(torch.tensor(prompt), torch.tril(torch.ones((P, P), dtype=torch.long)), None)
    _check_rows(eng.logits()[:P], lg0, range(P), f'{preset} prefill', **TINY)
    ids, rows = _tree(rs, 64, shape.vocab)
    eng.verify_only(ids, rows)
    ref = _oracle_tree(oracle, past, P, ids, rows)
    _check_rows(eng.logits()[:64], ref, range(64), f'{preset} tree', **TINY)


def _hf_qwen2_decisive(dt):
    import transformers
    torch.manual_seed(0)
    cfg = transformers.Qwen2Config(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
                                   num_key_value_heads=1, rms_norm_eps=1e-6, rope_theta=1e6, max_position_embeddings=1024,
                                   pad_token_id=0, bos_token_id=1, eos_token_id=2, tie_word_embeddings=False,
                                   attn_implementation='eager')
    m = transformers.Qwen2ForCausalLM(cfg).eval()
    sd = m.state_dict()
    with torch.no_grad():
        for k in sd:
            if k.endswith('o_proj.weight') or k.endswith('down_proj.weight'):
                sd[k].mul_(0.005)
            elif k.endswith('.bias'):
                sd[k].copy_(torch.randn_like(sd[k]) * 0.5)
        order = 3 + torch.randperm(512 - 3)
        perm = torch.arange(512)
        perm[order] = torch.roll(order, -1)
        head = torch.empty_like(sd['model.embed_tokens.weight'])
        head[perm] = sd['model.embed_tokens.weight']
        sd['lm_head.weight'].copy_(head)
    m = m.to(dt).float()                   # weights rounded to the engine's dtype once; the HF reference runs them in fp32
    return m


@pytest.mark.parametrize('dt', DTYPES)
def test_front_door_generate_gives_hf_greedy_tokens(dt):
    from painlessinferenceacceleration_amd import BatchQwen2ForCausalLM, Qwen2ForCausalLM
    hf = _hf_qwen2_decisive(dt)
    input_ids = torch.randint(3, 512, (1, 20), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        ref = hf.generate(input_ids, max_new_tokens=48, do_sample=False, pad_token_id=0, eos_token_id=None)[0].tolist()
    model = Qwen2ForCausalLM.from_hf(hf, max_length=256, dtype=dt)
    assert model.engine.dtype == dt and model.shape.qkv_bias
    dk = {'use_lookahead': True, 'decoding_length': 64, 'branch_length': 12}
    for _ in range(2):                     # the second run drafts from the trie the first one filled
        out = model.generate(input_ids=input_ids.cuda(), attention_mask=torch.ones_like(input_ids).cuda(), max_new_tokens=48,
                             pad_token_id=0, eos_token_id=None, decoding_kwargs=dict(dk), return_dict_in_generate=True)
        assert out.sequences[0].tolist() == ref
        assert sum(out.kwargs['edls']) == len(ref) - 20
    del model
    four = torch.randint(3, 512, (4, 20), generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        ref4 = [hf.generate(four[i:i + 1], max_new_tokens=32, do_sample=False, pad_token_id=0, eos_token_id=None)[0].tolist() for i in range(4)]
    bm = BatchQwen2ForCausalLM.from_hf(hf, max_length=256, max_batch=4, dtype=dt)
    out4 = bm.generate(input_ids=four.cuda(), attention_mask=torch.ones_like(four).cuda(), max_new_tokens=32, pad_token_id=2,
                       eos_token_id=None, decoding_kwargs=dk)
    assert [o.tolist() for o in out4] == ref4
