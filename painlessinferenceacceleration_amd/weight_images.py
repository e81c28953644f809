# -*- coding: utf-8 -*-
"""Weight images — what LlamaVerifyEngine hands la_llama_create: every projection of a state dict repacked into MFMA-fragment order
(la_pack_weight / la_pack_planned and their fp8 twins), plus the vectors that travel with them (fp8 row scales, the Qwen2 q/k/v
bias, the Qwen3 q/k norms, the norms).  Host side only: torch allocates and moves, the pack kernels live in liblookahead_hip.so.  WeightPacker is the one
place that calls la_pack_* and la_rowplan; pack_layer turns one decoder layer into its LlamaLayerWeightsC."""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from ._lib import check

FP8_MAX = 448.0          # largest finite e4m3fn value


def quantize_fp8(w):
    """Per-output-row symmetric FP8 (OCP e4m3fn) quantization: s[n] = amax(|W[n, :]|) / 448, q = clamp(W / s, -448, 448) in e4m3fn,
    so that W'[n][k] = s[n] * q[n][k].  A row whose amax is 0 (lane padding) gets s = 1 and q = 0.  The clamp matters: torch's cast
    gives NaN above ~464 rather than saturating, and W / s can round just past 448.  -> (q float8_e4m3fn [N, K], s float32 [N])."""
    w = w.float()
    amax = w.abs().amax(dim=1)
    s = torch.where(amax > 0, amax / FP8_MAX, torch.ones_like(amax))
    q = (w / s[:, None]).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn)
    return q, s


def dequantize_fp8(q, s):
    """W' = s[n] * q[n][k] in fp32 (what an fp8 engine computes with)."""
    return q.float() * s.float().reshape(-1, 1)


def fp8_row_scale(scale, n_rows, name):
    """A checkpoint's weight_scale -> fp32 [n_rows]: a scalar per tensor is broadcast to the rows, [N] / [N, 1] is per channel."""
    scale = scale.detach().float().reshape(-1)
    if scale.numel() == 1:
        return scale.expand(n_rows).clone()
    if scale.numel() != n_rows:
        raise ValueError(f'{name}: {scale.numel()} scales for {n_rows} rows (per-tensor or per-output-row scales only)')
    return scale.clone()


def to_lanes(w, n_h, dim, lane_src):
    """[n_h * head_dim, K] rows (dim 0) or [N, n_h * head_dim] columns (dim 1) -> the same with 128 lanes per head: lane l of a head
    holds its feature lane_src[l] (la_head_lane_map), exact zeros where lane_src[l] < 0.  16-bit weights, the bias vector (as one
    column) and fp8 bytes (uint8) all go through here; head_dim 128 is handed back as it is."""
    hd = int((lane_src >= 0).sum())
    if hd == 128:
        return w
    src = torch.from_numpy(lane_src.astype(np.int64)).to(w.device)
    idx = (torch.arange(n_h, device=w.device)[:, None] * hd + src.clamp(min=0)[None, :]).reshape(-1)
    keep = (src >= 0).repeat(n_h)
    shape_ = [1, 1]
    shape_[dim] = -1
    return w.index_select(dim, idx) * keep.reshape(shape_).to(w.dtype)


def fp8_lanes(q, s, n_h, dim, lane_src):
    """The 128-feature lanes (la_head_lane_map) of an fp8 projection of a model with head_dim < 128: q (uint8 view of the e4m3fn
    bytes: torch has no fp8 multiply) rows (dim 0: q / k / v) or columns (dim 1: o_proj) spread over the lanes, zero on padding
    lanes; s (fp32 per output row) follows the rows, padding rows get s = 1; s = None (a 16-bit matrix) stays None.  -> (q, s)."""
    q2 = to_lanes(q, n_h, dim, lane_src)
    if s is not None and dim == 0 and q2 is not q:
        keep = torch.from_numpy(np.tile(lane_src >= 0, n_h)).to(s.device)
        s = torch.where(keep, to_lanes(s.reshape(-1, 1), n_h, 0, lane_src).reshape(-1), torch.ones((), dtype=s.dtype, device=s.device))
    return q2, s


def qkv_mb_workgroups(n_heads, n_kv_heads, balanced_wg0, max_blocks, head_dim):
    """Workgroups of the SECOND QKV image, which the multi-block step (192-512 rows, MFMA-bound) reads, or 0 = none.  balanced_wg0:
    workgroups of the balanced QKV plan (one per CU; 0 = no plan); head_dim: the lane width of the images (128 in every engine).
    When the one-workgroup-per-CU plan leaves the 32-row MFMA blocks less than 60 % full (GQA: Mistral / Mixtral 24 rows = 12 RoPE
    pairs per workgroup), a second image over pairs / 32 workgroups (every block full; 50 MB per layer at the Mistral shape) serves
    that path: Mistral bs=8 11.26 -> 10.45 ms per step (scripts/gpu_qkv_wg_ab.sh, profiles/r03_qkv_mb_plan.txt) ... or leaves a
    pair count per workgroup that is no multiple of 4 (Llama-2-13B: 30): the RoPE epilogue then stores 4-byte pieces and 1/16 of the
    MFMA rows are padding; 240 full workgroups instead: 13B bs=4 10.57 -> 10.45 ms, bs=8 16.00 -> 15.60.  LA_QKV_MB_WG overrides
    the choice (0 = off), not the conditions on a count; the caller confirms that la_rowplan has a plan for it."""
    if not (max_blocks > 1 and balanced_wg0 and head_dim == 128):
        return 0
    pairs = (n_heads + 2 * n_kv_heads) * head_dim // 2
    per_wg = pairs // balanced_wg0
    want = pairs // 32 if (pairs % 32 == 0 and (per_wg / 32.0 < 0.6 or (per_wg % 4 != 0 and pairs // 32 >= 0.9 * balanced_wg0))) else 0
    if os.environ.get('LA_QKV_MB_WG') is not None:
        want = int(os.environ['LA_QKV_MB_WG'])
    ok = want > 0 and want % 16 == 0 and want < balanced_wg0 and pairs % want == 0 and pairs // want <= 32
    return want if ok else 0


class WeightPacker(object):
    """Builds the images of one engine: the library, the engine's stream, device and 16-bit type, the balanced row plans, the list
    that keeps every device tensor alive (the engine's _keep) and the bytes of the images (+ fp8 scales) built so far (nbytes: the
    engine's weight_bytes).  An image is 16-bit or fp8 by the element type of its source: uint8 = e4m3fn bytes."""

    def __init__(self, lib, stream, device, dtype):
        self.lib, self.stream, self.device, self.dtype = lib, stream, device, dtype
        self.sp = C.c_void_p(stream.cuda_stream)
        self.keep, self.nbytes = [], 0
        self.plans, self.plan_kinds = {}, {}
        self.qk_norms = []          # (q_norm, k_norm) device pointers per layer of a Qwen3 model (pack_layer)

    def add_plan(self, slot, kind, n_rows, nwg):
        """la_rowplan deals the rows of a GEMM out to nwg workgroups: ask for the plan's size, then fill it.  -> False: the shape is
        not balanceable (classic grid)"""
        n = self.lib.la_rowplan(kind, n_rows, nwg, None)
        if n <= 0:
            return False
        plan = np.zeros(n, dtype=np.int32)
        check(min(self.lib.la_rowplan(kind, n_rows, nwg, plan.ctypes.data_as(_lib.pi32)), 0), 'rowplan')
        self.plans[slot] = torch.from_numpy(plan).to(self.device)
        self.plan_kinds[slot] = (kind, n_rows, nwg)
        return True

    def hold(self, t, dtype=None):
        """a tensor the engine reads as it is (norm, bias, router, embedding), kept on the device in the 16-bit type; not counted"""
        t = t.to(device=self.device, dtype=dtype or self.dtype).contiguous()
        self.keep.append(t)
        return t

    def hold_scales(self, t):
        """the fp32 row scales of an fp8 image: kept, and counted with the images"""
        t = self.hold(t, torch.float32)
        self.nbytes += t.numel() * t.element_size()
        return t

    def _image(self, mats, n_elems, pack16, pack8, *args):
        """one image of n_elems elements from one or two source matrices by pack16 or (uint8 sources) pack8, called on the engine's
        stream as pack(stream, source 0, source 1 or None, *args, destination)"""
        fp8 = mats[0].dtype == torch.uint8
        pack = pack8 if fp8 else pack16
        mats = [m.to(device=self.device, dtype=torch.uint8 if fp8 else self.dtype).contiguous() for m in mats]
        out = torch.empty(n_elems, dtype=torch.uint8 if fp8 else self.dtype, device=self.device)
        torch.cuda.synchronize(self.device)          # the sources were produced on torch's stream
        check(pack(self.sp, mats[0].data_ptr(), mats[1].data_ptr() if len(mats) > 1 else None, *args, out.data_ptr()), pack.__name__[3:])
        self.stream.synchronize()                    # the sources may be freed by the caller right after
        self.keep.append(out)
        self.nbytes += out.numel() * out.element_size()
        return out

    def plain(self, w, w2=None):
        """la_pack_weight(_fp8): w [N, K], or w and w2 (gate and up) interleaved into one image"""
        n, k = w.shape
        mats = [w] if w2 is None else [w, w2]
        return self._image(mats, len(mats) * n * k, self.lib.la_pack_weight, self.lib.la_pack_weight_fp8, n, k, len(mats) - 1)

    def planned(self, slot, mats):
        """la_pack_planned(_fp8): compact workgroup-major packing by the row plan `slot`"""
        kind, n_rows, nwg = self.plan_kinds[slot]
        K = mats[0].shape[1]
        return self._image(mats, self.lib.la_planned_elems(kind, n_rows, K, nwg), self.lib.la_pack_planned, self.lib.la_pack_planned_fp8,
                           self.plans[slot].data_ptr(), kind, n_rows, K, nwg)

    def planned_or_plain(self, slot, mats):
        return self.planned(slot, mats) if slot in self.plans else self.plain(*mats)


class StateDictSource(object):
    """Reads an HF-named state dict; consume=True pops what it reads (the caller's dict shrinks as the device images grow)."""

    def __init__(self, state_dict, consume, device, fp8):
        self.sd, self.consume, self.device, self.fp8 = state_dict, consume, device, fp8

    def take(self, name):
        return self.sd.pop(name) if self.consume else self.sd[name]

    def projection(self, name, on_device=False):
        """projection `name` (…/q_proj etc.) -> (matrix, None) as stored (on_device: moved there in its stored type; otherwise the
        packer moves and converts it in one step, which a CPU fp32 checkpoint wants), or for an fp8 engine (q as uint8 [N, K],
        s fp32 [N]) on the device: the checkpoint's own e4m3fn bytes and weight_scale, or quantize_fp8 of a 16/32-bit weight"""
        w = self.take(name + '.weight')
        if not self.fp8:
            return (w.to(self.device) if on_device else w), None
        if w.dtype == torch.float8_e4m3fn:
            q, sc = w.to(self.device), fp8_row_scale(self.take(name + '.weight_scale'), w.shape[0], name).to(self.device)
        else:
            q, sc = quantize_fp8(w.to(self.device))
        if self.consume:
            self.sd.pop(name + '.input_scale', None)        # activations stay 16-bit (W8A16)
        return q.view(torch.uint8).contiguous(), sc.float().contiguous()


def qkv_bias_vector(src, prefix, shape, lane_src):
    """One lane-ordered vector [q heads | k heads | v heads] x 128 lanes (zeros on padding lanes): the layout every QKV epilogue
    reads, whatever the row order of the weight image (la_gemm64_qkv_bias)"""
    try:
        bq, bk, bv = (src.take(prefix + f'self_attn.{n}_proj.bias') for n in 'qkv')
    except KeyError as e:
        raise ValueError(f'shape.qkv_bias is set but the state dict has no {e.args[0]}') from None
    return torch.cat([to_lanes(b.to(src.device).reshape(-1, 1), n_h, 0, lane_src).reshape(-1)
                      for b, n_h in ((bq, shape.n_heads), (bk, shape.n_kv_heads), (bv, shape.n_kv_heads))])


def stack_experts(packer, src, prefix, n_experts):
    """The expert images of a Mixtral layer at equal spacing in ONE buffer per projection, which lets the engine run all experts of a
    stage in a single launch (la_engine.cpp: ex_merged).  -> (gate/up, down) as void* [n_experts]; the per-expert images are
    dropped from the kept list once copied (their bytes stay counted: the buffers hold the same images)."""
    gu, dn = (_lib.vp * n_experts)(), (_lib.vp * n_experts)()
    gu_all = dn_all = None
    for e in range(n_experts):
        q = prefix + f'block_sparse_moe.experts.{e}.'
        one_gu = packer.planned_or_plain(1, [src.take(q + 'w1.weight'), src.take(q + 'w3.weight')])
        one_dn = packer.plain(src.take(q + 'w2.weight'))
        if gu_all is None:
            gstride = (one_gu.numel() + 63) // 64 * 64
            dstride = (one_dn.numel() + 63) // 64 * 64
            gu_all = torch.zeros(n_experts * gstride, dtype=packer.dtype, device=packer.device)
            dn_all = torch.zeros(n_experts * dstride, dtype=packer.dtype, device=packer.device)
        gu_all[e * gstride:e * gstride + one_gu.numel()].copy_(one_gu)
        dn_all[e * dstride:e * dstride + one_dn.numel()].copy_(one_dn)
        gu[e] = gu_all.data_ptr() + 2 * e * gstride
        dn[e] = dn_all.data_ptr() + 2 * e * dstride
        packer.keep[:] = [t for t in packer.keep if t is not one_gu and t is not one_dn]
    torch.cuda.synchronize(packer.device)
    packer.keep.extend([gu, dn, gu_all, dn_all])
    return gu, dn


def pack_layer(packer, src, shape, i, L, lane_src, qkv_perm):
    """Decoder layer i of the state dict -> the fields of L (LlamaLayerWeightsC).  fp8 differs from 16-bit only in what
    src.projection hands back: uint8 sources (which select the fp8 pack entry points) with fp32 row scales, which follow their rows
    through the lanes and the concatenations into the <image>_scale fields.  qkv_perm: the row order of a QKV image that has no
    plan (la_qkv_row_perm: each workgroup owns RoPE pairs), None = rows as concatenated (the unfused QKV)."""
    p = f'model.layers.{i}.'

    def put(field, image, scales):
        setattr(L, field, image.data_ptr())
        if scales is not None:
            setattr(L, field + '_scale', packer.hold_scales(scales).data_ptr())

    def cat(vs):
        return None if vs[0] is None else torch.cat(vs)

    if getattr(shape, 'qkv_bias', False):
        L.qkv_bias = packer.hold(qkv_bias_vector(src, p, shape, lane_src)).data_ptr()
    # rows of [Wq;Wk;Wv]; the QKV scale vector stays lane-ordered (slot * 128 + lane) whatever row order the image gets, like the bias
    parts = [fp8_lanes(*src.projection(p + f'self_attn.{n}_proj', True), n_h, 0, lane_src)
             for n, n_h in (('q', shape.n_heads), ('k', shape.n_kv_heads), ('v', shape.n_kv_heads))]
    qkv, s_qkv = torch.cat([w for w, _ in parts], 0), cat([s for _, s in parts])
    del parts
    if 0 in packer.plans:
        put('wqkv', packer.planned(0, [qkv]), s_qkv)
        if 'qkv_mb' in packer.plans:
            L.wqkv_mb = packer.planned('qkv_mb', [qkv]).data_ptr()
    else:
        put('wqkv', packer.plain(qkv if qkv_perm is None else qkv.index_select(0, qkv_perm)), s_qkv)
    del qkv
    wo, s_o = fp8_lanes(*src.projection(p + 'self_attn.o_proj', bool((lane_src < 0).any())), shape.n_heads, 1, lane_src)
    put('wo', packer.plain(wo), s_o)
    del wo                               # every source is freed where it always was: the images keep their places in memory
    if shape.n_experts > 0:
        L.router = packer.hold(src.take(p + 'block_sparse_moe.gate.weight')).data_ptr()
        gu, dn = stack_experts(packer, src, p, shape.n_experts)
        L.ex_gateup = C.cast(gu, C.POINTER(_lib.vp))
        L.ex_down = C.cast(dn, C.POINTER(_lib.vp))
    else:
        (wg, s_g), (wu, s_u) = src.projection(p + 'mlp.gate_proj'), src.projection(p + 'mlp.up_proj')
        put('wgateup', packer.planned_or_plain(1, [wg, wu]), cat([s_g, s_u]))
        del wg, wu
        wd, s_d = src.projection(p + 'mlp.down_proj')
        put('wdown', packer.plain(wd), s_d)
        del wd
    if getattr(shape, 'qk_norm', False):
        # not fields of L: la_llama_create_qk_norm takes them as one array per norm (LlamaVerifyEngine)
        packer.qk_norms.append((packer.hold(src.take(p + 'self_attn.q_norm.weight')).data_ptr(),
                                packer.hold(src.take(p + 'self_attn.k_norm.weight')).data_ptr()))
    L.norm1 = packer.hold(src.take(p + 'input_layernorm.weight')).data_ptr()
    L.norm2 = packer.hold(src.take(p + 'post_attention_layernorm.weight')).data_ptr()
    torch.cuda.synchronize(packer.device)
