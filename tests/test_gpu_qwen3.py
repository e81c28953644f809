# -*- coding: utf-8 -*-
"""-m gpu: the Qwen3 family — the per-head q / k RMSNorm + RoPE stage (la_qk_norm_rope, csrc/la_qknorm.hip) and the engine / wrappers
built on it.

* kernel: in place on packed QF / fresh KF fragments, against torch on the same device with the stage's rounding points
  (n = storage(f * rsqrt(mean(f^2) + eps)), y = storage(w * n), rotate-half RoPE of y in storage-type arithmetic), both dtypes, 1 and 3
  blocks, GQA and MHA head counts; V, guard bytes and the blocks past nblk stay bit-identical; an all-zero row stays zero;
* engine: a tiny Qwen3 vs tests/qwen3_oracle.py through step + a prefill chain on every QKV launch form, the cursor batch, mstep
  at 2 and 5 blocks, a 150-row wide tree (tstep), tied and untied heads, both dtypes; the real Qwen3-8B / Qwen3-0.6B layer shapes; fp8 weights; the front door
  (from_hf + generate) vs transformers greedy; and a sensitivity control (the same weights without the stage are far outside)."""
import functools

import numpy as np
import pytest
import torch

from painlessinferenceacceleration_amd import _lib
from painlessinferenceacceleration_amd._lib import check
from painlessinferenceacceleration_amd.llama_engine import LlamaShape, LlamaVerifyEngine, random_weights, rope_tables
from tests import gpu_utils as gu
from tests.gpu_utils import DEV, ptr, random_tree, sp
from tests.qwen3_oracle import OracleQwen3
from tests.test_gpu_e2e import TOL, _check_rows
from tests.test_gpu_qwen2 import TINY, _Case, _oracle_tree, _tree

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
EPS = 1e-6


# ------------------------------------------------------------------------------------------------------------------- kernel
class _NormCase(object):
    """Packed q / k / v tiles of nblk 64-row blocks (+ one block past nblk and guard words around every buffer, all random bits), the
    norm weights, positions and RoPE tables of one la_qk_norm_rope call."""
    GUARD = 4096

    def __init__(self, nh, nkv, dt, nblk, seed=0):
        g = torch.Generator(device=DEV).manual_seed(seed * 977 + nh * 13 + nkv * 5 + nblk)
        self.nh, self.nkv, self.dt, self.nblk = nh, nkv, dt, nblk

        def tiles(n):
            # per-token rms from 1e-4 to 10 (log-uniform): below sqrt(eps) the eps term carries the result
            scale = 10.0 ** (torch.rand(nblk, n, 64, 1, generator=g, device=DEV) * 5.0 - 4.0)
            return (torch.randn(nblk, n, 64, 128, generator=g, device=DEV) * scale).to(dt)
        self.q, self.k, self.v = tiles(nh), tiles(nkv), tiles(nkv)
        self.q[0, 0, 5] = 0                                     # an all-zero row in a q head and in a k head
        self.k[nblk - 1, nkv - 1, 63] = 0

        def weight():                                           # mixed signs, magnitudes 0.1 ... 4
            mag = 0.1 * 40.0 ** torch.rand(128, generator=g, device=DEV)
            sign = torch.where(torch.rand(128, generator=g, device=DEV) < 0.5, -1.0, 1.0)
            return (mag * sign).to(dt).contiguous()
        self.qw, self.kw = weight(), weight()
        self.pos = torch.randint(0, 900, (nblk * 64,), generator=g, device=DEV, dtype=torch.int32)
        self.rc, self.rs = rope_tables(128, 1024, 1e6, DEV, dt)

        def buf(dense, index, heads):
            """[guard | nblk blocks | one more block | guard] of random bits with the packed tiles in the first nblk blocks"""
            n = heads * 8192
            raw = torch.randint(-32768, 32767, (2 * self.GUARD + (nblk + 1) * n,), generator=g, device=DEV, dtype=torch.int16)
            raw[self.GUARD:self.GUARD + nblk * n] = gu.to_packed(dense, index, 8192).reshape(-1).view(torch.int16)
            return raw
        self.qbuf, self.kbuf = buf(self.q, gu.rf_index(64), nh), buf(self.k, gu.rf_index(64), nkv)
        self.vbuf = buf(self.v, gu.vf_index(64), nkv)

    def tiles_of(self, raw, heads):
        n = heads * 8192
        flat = raw[self.GUARD:self.GUARD + self.nblk * n].view(self.dt).view(self.nblk, heads, 8192)
        return gu.from_packed(flat, gu.rf_index(64))            # [nblk, heads, 64, 128]

    def outside(self, raw, heads):
        n = self.nblk * heads * 8192
        return torch.cat([raw[:self.GUARD], raw[self.GUARD + n:]])

    def run(self, L):
        G = self.GUARD * 2                                      # bytes
        check(L.la_qk_norm_rope(sp(), self.qbuf.data_ptr() + G, self.kbuf.data_ptr() + G, self.nblk, self.nh, self.nkv, ptr(self.qw),
                                ptr(self.kw), EPS, ptr(self.pos), ptr(self.rc), ptr(self.rs)), 'qk_norm_rope')
        torch.cuda.synchronize()

    def ref(self, x, w):
        """[nblk, heads, 64, 128] -> the same after norm + RoPE, every rounding where the stage rounds"""
        dt = self.dt
        f = x.float()
        n = (f * torch.rsqrt(f.pow(2).mean(-1, keepdim=True) + EPS)).to(dt)
        y = w * n
        p = self.pos.long().view(self.nblk, 1, 64)
        cos = torch.cat([self.rc[p], self.rc[p]], -1)
        sin = torch.cat([self.rs[p], self.rs[p]], -1)
        return (y * cos) + (torch.cat((-y[..., 64:], y[..., :64]), -1) * sin)


@functools.lru_cache(maxsize=None)
def _parent_rope_share(dt):
    """Share of q / k elements of la_gemm64r_qkv (unchanged here) that are not bit-identical to its torch reference at this dtype: the
    RoPE of the float16 build sits one ulp from torch's eager arithmetic on a sizeable share (tests/test_gpu_qwen2.py::_Case.check)."""
    L = _lib.lib_for(dt)
    c = _Case(4, 2, 128, dt)
    wp = gu.pack_planned(2, [c.w.view(torch.bfloat16)], 32)
    o = c.outs()
    check(L.la_gemm64r_qkv(sp(), ptr(wp), ptr(c.xp), 4, 2, c.K, 32, ptr(c.pos), ptr(c.rc), ptr(c.rs), *map(ptr, o)), 'qkv_r')
    torch.cuda.synchronize()
    got, ref = c.unpack(*o, 0), c.ref(False)[0]
    diff = sum(int((g_ != r).sum()) for g_, r in zip(got[:2], ref[:2]))
    return diff / float(sum(r.numel() for r in ref[:2]))


@pytest.mark.parametrize('dt', DTYPES, ids=['bf16', 'fp16'])
@pytest.mark.parametrize('nblk', [1, 3])
@pytest.mark.parametrize('nh,nkv', [(4, 2), (5, 5)])
def test_qk_norm_rope_kernel(dt, nblk, nh, nkv):
    L = _lib.lib_for(dt)
    c = _NormCase(nh, nkv, dt, nblk)
    rms = c.q.float().pow(2).mean(-1).sqrt()
    assert float(rms[rms > 0].min()) < 1e-3 and float(rms.max()) > 3.0, 'the case spans both sides of sqrt(eps)'
    before = [b.clone() for b in (c.qbuf, c.kbuf, c.vbuf)]
    c.run(L)
    # exact: V, the guard words and the block past nblk of every buffer
    assert torch.equal(c.vbuf, before[2])
    assert torch.equal(c.outside(c.qbuf, nh), c.outside(before[0], nh)) and torch.equal(c.outside(c.kbuf, nkv), c.outside(before[1], nkv))
    share0 = _parent_rope_share(dt)
    eps_dt = torch.finfo(dt).eps
    n_diff = n_all = 0
    for name, raw, heads, x, w in (('q', c.qbuf, nh, c.q, c.qw), ('k', c.kbuf, nkv, c.k, c.kw)):
        got, ref = c.tiles_of(raw, heads), c.ref(x, w)
        assert bool(torch.isfinite(got.float()).all())
        # hard cap per (token, head) vector: a one-ulp move of n passes two more roundings and a rotation with |c| + |s| <= sqrt(2),
        # about 4.3 ulps of the vector's largest magnitude; 6
        err = (got.float() - ref.float()).abs().amax(-1)
        cap = 6.0 * eps_dt * ref.float().abs().amax(-1)
        worst = float((err / cap.clamp_min(1e-30)).max())
        print(f'{name}: worst |got - ref| / (6 eps max|ref|) = {worst:.3f}')
        assert bool((err <= cap).all()), (name, worst)
        n_diff += int((got != ref).sum())
        n_all += ref.numel()
        zero = (x == 0).all(-1)
        assert int(zero.sum()) == 1 and bool((got[zero].float() == 0).all()), 'an all-zero row stays zero'
        # the case can see the stage: the input itself is far from the result
        assert gu.rel_err(x.float(), ref.float()) > 0.5
    share = n_diff / float(n_all)
    print(f'not bit-identical: {share:.4f}; la_gemm64r_qkv against its own reference: {share0:.4f}')
    assert share <= share0 + 0.03, f'not bit-identical: {share:.4f} of the elements; la_gemm64r_qkv against its own reference: {share0:.4f}'


def test_qk_norm_rope_arguments_are_checked():
    L = _lib.lib
    c = _NormCase(2, 2, torch.bfloat16, 1)
    G = c.GUARD * 2
    good = [sp(), c.qbuf.data_ptr() + G, c.kbuf.data_ptr() + G, 1, 2, 2, ptr(c.qw), ptr(c.kw), EPS, ptr(c.pos), ptr(c.rc), ptr(c.rs)]
    for i in (1, 2, 6, 7, 9, 10, 11):                            # every pointer: NULL is LA_E_ARG
        bad = list(good)
        bad[i] = None
        assert L.la_qk_norm_rope(*bad) == -1, i
    for nblk in (0, -1, _lib.LA_MB_MAX + 1):
        bad = list(good)
        bad[3] = nblk
        assert L.la_qk_norm_rope(*bad) == -1, nblk
    bad = list(good)
    bad[6] = c.qw.data_ptr() + 2                                 # the weights are read with 16-byte loads
    assert L.la_qk_norm_rope(*bad) == -1
    before = c.qbuf.clone()
    torch.cuda.synchronize()
    assert torch.equal(c.qbuf, before), 'a refused call launches nothing'
    check(L.la_qk_norm_rope(*good), 'qk_norm_rope')
    torch.cuda.synchronize()


# -------------------------------------------------------------------------------------------------------------------- engine
def _tiny(layers=2, qk_norm=True):
    return LlamaShape(layers, 256, 4, 2, 512, 512, 1e-6, rope_theta=1e6, head_dim=128, norm_cast_first=True, qk_norm=qk_norm)


def _sd(shape, seed=3, dt=torch.bfloat16, tied=False):
    sd = random_weights(shape, seed=seed, std=0.08, dtype=torch.float32)
    sd = {k: v.to(dt) for k, v in sd.items()}
    if tied:
        sd['lm_head.weight'] = sd['model.embed_tokens.weight']
    return sd


@pytest.mark.parametrize('kw,dt,tied', [(dict(), torch.bfloat16, False), (dict(), torch.float16, True),
                                        (dict(balanced=False), torch.bfloat16, True), (dict(balanced=False), torch.float16, False),
                                        (dict(gemm_cfg=[0, -1]), torch.bfloat16, False)],
                         ids=['balanced-bf16', 'balanced-fp16-tied', 'classic-bf16-tied', 'classic-fp16', 'unfused_post-bf16'])
def test_engine_step_and_prefill_chain_match_the_oracle(kw, dt, tied):
    shape = _tiny()
    sd = _sd(shape, dt=dt, tied=tied)
    oracle = OracleQwen3(shape, sd)
    eng = LlamaVerifyEngine(shape, dict(sd), max_length=384, **kw)
    assert eng.dtype == dt
    rs = np.random.RandomState(17)
    prompt = rs.randint(3, shape.vocab, size=150).tolist()             # a prefill chain of three 64-row blocks
    eng.prefill(prompt)
    P = len(prompt)
    lg0, past = oracle.forward(torch.tensor(prompt), torch.tril(torch.ones((P, P), dtype=torch.long)), None)
    _check_rows(eng.logits()[:(P - 1) % 64 + 1], lg0[(P - 1) // 64 * 64:], range((P - 1) % 64 + 1), 'prefill', **TINY)
    ids, rows = _tree(rs, 64, shape.vocab)
    toks, _ = eng.step(ids, rows)                                      # the captured graph
    ref = _oracle_tree(oracle, past, P, ids, rows)
    _check_rows(eng.logits()[:64], ref, range(64), f'tree {kw}', **TINY)
    assert len(toks) >= 1


@pytest.mark.parametrize('B', [2, 5])
def test_mstep_matches_the_oracle(B):
    shape = _tiny()
    sd = _sd(shape, seed=5)
    oracle = OracleQwen3(shape, sd)
    eng = LlamaVerifyEngine(shape, dict(sd), max_length=384, n_slots=B, max_blocks=B)
    rs = np.random.RandomState(B)
    prompts = [rs.randint(3, shape.vocab, size=int(rs.randint(5, 60))).tolist() for _ in range(B)]
    prompts[0] = rs.randint(3, shape.vocab, size=64 * (B - 1) + 9).tolist()       # a prefill chain over all B blocks of one pass
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


def test_cursor_batch_matches_the_oracle():
    B = 3
    shape = _tiny()
    sd = _sd(shape, seed=6)
    oracle = OracleQwen3(shape, sd)
    eng = LlamaVerifyEngine(shape, dict(sd), max_length=384, n_slots=B)
    rs = np.random.RandomState(8)
    prompts = [rs.randint(3, shape.vocab, size=n).tolist() for n in (70, 23, 41)]
    pasts = []
    for b, p in enumerate(prompts):
        eng.bprefill(b, p)
        P = len(p)
        lg, past = oracle.forward(torch.tensor(p), torch.tril(torch.ones((P, P), dtype=torch.long)), None)
        last = (P - 1) // 64 * 64
        _check_rows(eng.logits()[:P - last], lg[last:], range(P - last), f'bprefill {b}', **TINY)
        pasts.append(past)
    # one block shared by the three sequences: 21 + 22 + 21 rows
    sizes = [21, 22, 21]
    trees = [_tree(rs, n, shape.vocab) for n in sizes]
    eng.bstep([(b, trees[b][0], trees[b][1], 2, 16) for b in range(B)])
    got = eng.logits()
    row = 0
    for b in range(B):
        ref = _oracle_tree(oracle, pasts[b], len(prompts[b]), *trees[b])
        _check_rows(got[row:row + sizes[b]], ref, range(sizes[b]), f'bstep slot {b}', **TINY)
        row += sizes[b]


def test_sensitivity_control_without_the_stage_is_far_off():
    shape = _tiny()
    sd = _sd(shape, seed=7)
    oracle = OracleQwen3(shape, sd)
    plain = _tiny(qk_norm=False)
    sd0 = {k: v for k, v in sd.items() if '_norm.weight' not in k or 'self_attn' not in k}     # the same weights, the stage off
    rs = np.random.RandomState(1)
    prompt = rs.randint(3, shape.vocab, size=48).tolist()
    P = len(prompt)
    ref, _ = oracle.forward(torch.tensor(prompt), torch.tril(torch.ones((P, P), dtype=torch.long)), None)
    ids, rows = _tree(rs, 64, shape.vocab)
    errs, launches = [], []
    for sh, s in ((shape, sd), (plain, sd0)):
        eng = LlamaVerifyEngine(sh, dict(s), max_length=256)
        eng.prefill(prompt)
        got = eng.logits()[:P].float().cpu()
        errs.append(max(float((got[i] - ref[i].float()).abs().max() / ref[i].float().abs().max()) for i in range(P)))
        launches.append(eng.profile(ids, rows, iters=1)['launches'])
        del eng
    assert errs[0] < 3e-2 and errs[1] > 10 * TOL, errs
    # the stage is one KC_OTHER launch per layer behind the QKV launch, and nothing else moved
    assert launches[0]['other'] == launches[1]['other'] + shape.n_layers, launches
    assert all(launches[0][k] == launches[1][k] for k in launches[0] if k != 'other'), launches


@pytest.mark.parametrize('preset', ['qwen3_8b', 'qwen3_0_6b'])
def test_real_layer_shapes_two_layers(preset):
    shape = getattr(LlamaShape, preset)()
    shape.n_layers = 2
    sd = random_weights(shape, seed=2, device=DEV)
    if preset == 'qwen3_0_6b':
        sd['lm_head.weight'] = sd['model.embed_tokens.weight']
    cpu = {k: v.cpu() for k, v in sd.items()}
    oracle = OracleQwen3(shape, cpu)
    eng = LlamaVerifyEngine(shape, sd, max_length=256, n_slots=3, max_blocks=3)
    rs = np.random.RandomState(3)
    prompt = rs.randint(3, shape.vocab, size=40).tolist()
    eng.prefill(prompt)
    P = len(prompt)
    lg0, past = oracle.forward(torch.tensor(prompt), torch.tril(torch.ones((P, P), dtype=torch.long)), None)
    _check_rows(eng.logits()[:P], lg0, range(P), f'{preset} prefill', **TINY)
    ids, rows = _tree(rs, 64, shape.vocab)
    eng.verify_only(ids, rows)
    ref = _oracle_tree(oracle, past, P, ids, rows)
    _check_rows(eng.logits()[:64], ref, range(64), f'{preset} tree', **TINY)
    # three blocks in one pass (the multi-block step's own QKV image where the shape has one): every block carries the same tree
    eng.reset()
    for b in range(3):
        eng.mprefill(b, prompt)
    eng.mstep([(b, ids, rows, 2, 16) for b in range(3)])
    got = eng.mlogits()
    print(preset, 'balanced', eng.balanced_wg, 'qkv_mb_wg', eng.qkv_mb_wg)
    for b in range(3):
        _check_rows(got[b * 64:(b + 1) * 64], ref, range(64), f'{preset} mstep block {b}', **TINY)


def test_fp8_weights_with_the_stage_vs_oracle_on_dequantized_weights():
    """weight_format='fp8' (pre-quantized projections with power-of-two row scales, tests/test_gpu_fp8.py::_pow2_fp8_sd, so that the oracle
    computes with the dequantized weights themselves) + the stage, on the single-sequence step: the QKV GEMMs are the fp8 launches of
    before, run with the identity tables.  The tiny model and its bar are those of the 16-bit engine tests above."""
    from tests.test_gpu_fp8 import _pow2_fp8_sd
    shape = _tiny()
    sd8, ref = _pow2_fp8_sd(random_weights(shape, seed=4, std=0.08, dtype=torch.float32))
    assert sd8['model.layers.0.self_attn.q_norm.weight'].dtype == torch.bfloat16
    oracle = OracleQwen3(shape, ref)
    eng = LlamaVerifyEngine(shape, dict(sd8), max_length=384)
    assert eng.weight_format == 'fp8'
    rs = np.random.RandomState(2)
    prompt = rs.randint(3, shape.vocab, size=100).tolist()
    eng.prefill(prompt)
    P = len(prompt)
    lg0, past = oracle.forward(torch.tensor(prompt), torch.tril(torch.ones((P, P), dtype=torch.long)), None)
    _check_rows(eng.logits()[:P - 64], lg0[64:], range(P - 64), 'fp8 prefill', **TINY)
    ids, rows = _tree(rs, 64, shape.vocab)
    eng.step(ids, rows)
    _check_rows(eng.logits()[:64], _oracle_tree(oracle, past, P, ids, rows), range(64), 'fp8 tree', **TINY)
    del eng
    # control: the same fp8 weights without the stage are far off
    sd0 = {k: v for k, v in sd8.items() if '_norm.weight' not in k or 'self_attn' not in k}
    eng = LlamaVerifyEngine(_tiny(qk_norm=False), sd0, max_length=384)
    assert eng.weight_format == 'fp8'
    eng.prefill(prompt[:64])
    got = eng.logits()[:64].float().cpu()
    assert float((got - lg0[:64].float()).abs().max() / lg0[:64].float().abs().max()) > 10 * TOL


def test_wide_tree_step_matches_the_oracle():
    """tstep: a 150-row tree over three blocks of one pass (later blocks see the earlier ones under their ancestor words).  Every row's
    logits against the oracle under the full [T][ctx + T] mask, to the bar tests/test_gpu_mblock.py::test_wide_tree_step_matches_oracle
    states for this path (4e-2 per row, 1.5e-2 mean), then the accept walk given the device's argmax rows."""
    from oracle import llama_oracle as lo
    from tests.test_gpu_mblock import _random_wide_tree
    shape = _tiny()
    sd = _sd(shape, seed=9)
    oracle = OracleQwen3(shape, sd)
    eng = LlamaVerifyEngine(shape, dict(sd), max_length=512, n_slots=1, max_blocks=4)
    rs = np.random.RandomState(150)
    prompt = rs.randint(3, shape.vocab, size=40).tolist()
    tok = eng.mprefill(0, prompt)
    P = len(prompt)
    _, past = oracle.forward(torch.tensor(prompt), torch.tril(torch.ones((P, P), dtype=torch.long)), None)
    T = 150
    _, _, rm, mask = _random_wide_tree(rs, T, 30)
    ids = np.concatenate([[tok], rs.randint(3, shape.vocab, size=T - 1)]).astype(np.int32)
    full = torch.cat([torch.ones((T, P), dtype=torch.long), torch.from_numpy(mask)], 1)
    lg, _ = oracle.forward(torch.tensor(ids.tolist()), full, past)
    toks, kept = eng.tstep(ids, rm, mode=0)
    gf, rf = eng.mlogits()[:T].float().cpu(), lg.float()
    rel = ((gf - rf).abs().amax(-1) / rf.abs().amax(-1)).numpy()
    print('wide tree rel err: max', float(rel.max()), 'mean', float(rel.mean()))
    assert rel.max() <= 4e-2 and rel.mean() <= 1.5e-2, (float(rel.max()), float(rel.mean()), int(rel.argmax()))
    assert rel[64:].max() <= 4e-2 and rel[64:].mean() <= 1.5e-2
    mo = eng.mout().cpu().numpy()
    am = [int(mo[_lib.LA_MOUT_ARGMAX + r]) for r in range(T)]
    exp_toks, exp_rows = lo.accept_scan(ids.tolist(), mask, am)
    assert toks == exp_toks[:_lib.LA_MOUT_TOKS] and kept == min(len(exp_rows), _lib.LA_MOUT_TOKS)


def test_create_refuses_what_the_stage_does_not_serve():
    """Second line behind the host checks: la_llama_create_qk_norm itself never serves a model without the norm, and la_llama_create
    on the same config and weights is the model WITHOUT the stage (its structs did not change)."""
    import ctypes as C
    shape = _tiny()
    eng = LlamaVerifyEngine(shape, _sd(shape), max_length=256)
    L = eng._lib
    nbytes = L.la_llama_workspace_bytes(C.byref(eng._cfg))
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    w = _lib.LlamaWeightsC()
    w.embed, w.lm_head, w.final_norm = eng.embed.data_ptr(), eng.embed.data_ptr(), eng.embed.data_ptr()
    w.rope_cos, w.rope_sin = eng.rope_cos.data_ptr(), eng.rope_sin.data_ptr()
    w.layers = C.cast(eng._layers, C.POINTER(_lib.LlamaLayerWeightsC))

    def qk(**over):
        q = _lib.QkNormWeightsC()
        q.q_norm, q.k_norm = (C.cast(a, C.POINTER(_lib.vp)) for a in eng._qk_arrays)
        q.rope_cos_id, q.rope_sin_id = eng.rope_cos_id.data_ptr(), eng.rope_sin_id.data_ptr()
        for k, v in over.items():
            setattr(q, k, v)
        return q

    def create(cfg, q):
        return L.la_llama_create_qk_norm(C.byref(cfg), C.byref(w), C.byref(q) if q is not None else None, ws.data_ptr(), nbytes)
    assert not create(eng._cfg, None) and 'null' in _lib.last_error()
    assert not create(eng._cfg, qk(rope_cos_id=None)) and 'identity' in _lib.last_error()
    short = (_lib.vp * shape.n_layers)(eng._qk_arrays[1][0], None)
    assert not create(eng._cfg, qk(k_norm=C.cast(short, C.POINTER(_lib.vp)))) and 'k_norm' in _lib.last_error()        # a layer without its k_norm
    odd = (_lib.vp * shape.n_layers)(*[p + 2 for p in eng._qk_arrays[0]])
    assert not create(eng._cfg, qk(q_norm=C.cast(odd, C.POINTER(_lib.vp)))) and 'aligned' in _lib.last_error()
    for field, value, word in (('head_dim', 64, 'head_dim'), ('fuse', 2, 'fuse'), ('fuse', -4, 'fuse')):
        bad = _lib.LlamaConfigC.from_buffer_copy(eng._cfg)
        setattr(bad, field, value)
        assert not create(bad, qk()) and word in _lib.last_error(), field
    h = create(eng._cfg, qk())
    assert h
    L.la_llama_destroy(h)
    h = L.la_llama_create(C.byref(eng._cfg), C.byref(w), ws.data_ptr(), nbytes)           # the plain entry point: no stage, no refusal
    assert h
    L.la_llama_destroy(h)


def _hf_qwen3_decisive(dt):
    import transformers
    torch.manual_seed(0)
    cfg = transformers.Qwen3Config(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                                   num_key_value_heads=2, head_dim=128, rms_norm_eps=1e-6, rope_theta=1e6, max_position_embeddings=1024,
                                   pad_token_id=0, bos_token_id=1, eos_token_id=2, tie_word_embeddings=False,
                                   attn_implementation='eager')
    m = transformers.Qwen3ForCausalLM(cfg).eval()
    sd = m.state_dict()
    with torch.no_grad():
        for k in sd:
            if k.endswith('o_proj.weight') or k.endswith('down_proj.weight'):
                sd[k].mul_(0.005)
            elif k.endswith('q_norm.weight') or k.endswith('k_norm.weight'):
                sd[k].copy_(0.2 + 2.0 * torch.rand_like(sd[k]))
        order = 3 + torch.randperm(512 - 3)
        perm = torch.arange(512)
        perm[order] = torch.roll(order, -1)
        head = torch.empty_like(sd['model.embed_tokens.weight'])
        head[perm] = sd['model.embed_tokens.weight']
        sd['lm_head.weight'].copy_(head)
    return m.to(dt).float()                # weights rounded to the engine's dtype once; the HF reference runs them in fp32


@pytest.mark.parametrize('dt', DTYPES, ids=['bf16', 'fp16'])
def test_front_door_generate_gives_hf_greedy_tokens(dt):
    from painlessinferenceacceleration_amd import BatchQwen3ForCausalLM, Qwen3ForCausalLM
    hf = _hf_qwen3_decisive(dt)
    input_ids = torch.randint(3, 512, (1, 20), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        ref = hf.generate(input_ids, max_new_tokens=48, do_sample=False, pad_token_id=0, eos_token_id=None)[0].tolist()
    model = Qwen3ForCausalLM.from_hf(hf, max_length=256, dtype=dt)
    assert model.engine.dtype == dt and model.shape.qk_norm and not model.shape.qkv_bias
    plain = model.generate(input_ids=input_ids.cuda(), attention_mask=torch.ones_like(input_ids).cuda(), max_new_tokens=48,
                           pad_token_id=0, eos_token_id=None, decoding_kwargs={'use_lookahead': False}, return_dict_in_generate=True)
    assert plain.sequences[0].tolist() == ref                   # no drafts
    dk = {'use_lookahead': True, 'decoding_length': 64, 'branch_length': 12}
    for _ in range(2):                     # the second run drafts from the trie the first one filled
        out = model.generate(input_ids=input_ids.cuda(), attention_mask=torch.ones_like(input_ids).cuda(), max_new_tokens=48,
                             pad_token_id=0, eos_token_id=None, decoding_kwargs=dict(dk), return_dict_in_generate=True)
        assert out.sequences[0].tolist() == ref
        assert sum(out.kwargs['edls']) == len(ref) - 20
    assert max(out.kwargs['edls']) > 1, 'the drafts were never accepted'
    del model
    three = torch.randint(3, 512, (3, 20), generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        ref3 = [hf.generate(three[i:i + 1], max_new_tokens=32, do_sample=False, pad_token_id=0, eos_token_id=None)[0].tolist() for i in range(3)]
    bm = BatchQwen3ForCausalLM.from_hf(hf, max_length=256, max_batch=3, dtype=dt)
    out3 = bm.generate(input_ids=three.cuda(), attention_mask=torch.ones_like(three).cuda(), max_new_tokens=32, pad_token_id=2,
                       eos_token_id=None, decoding_kwargs=dk)
    assert [o.tolist() for o in out3] == ref3
