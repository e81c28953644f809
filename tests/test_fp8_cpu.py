# -*- coding: utf-8 -*-
"""FP8 (e4m3fn) weight-only quantization: the load-time quantizer and every refusal, on the CPU (no GPU needed: the engine checks
its weight format before it looks for a device)."""
import pytest
import torch

import numpy as np

from painlessinferenceacceleration_amd.llama_engine import (FP8_MAX, LlamaShape, LlamaVerifyEngine, check_weight_format,
                                                            dequantize_fp8, fp8_lanes, fp8_row_scale, quantize_fp8, random_weights)
from painlessinferenceacceleration_amd import modeling_llama_batch, modeling_qwen2


def _e4m3_step(v):
    """spacing of the e4m3 grid at |v| (normals: 2^(e - 3); subnormals: 2^-9)"""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -6)))
    return torch.pow(2.0, e - 3)


def test_quantizer_row_amax_maps_to_448_and_error_is_half_a_step():
    g = torch.Generator().manual_seed(0)
    w = torch.randn(96, 256, generator=g) * torch.logspace(-3, 1, 96)[:, None]
    q, s = quantize_fp8(w)
    assert q.dtype == torch.float8_e4m3fn and s.dtype == torch.float32 and s.shape == (96,)
    qa = q.float().abs().amax(1)
    assert torch.equal(qa, torch.full_like(qa, FP8_MAX))
    wq = dequantize_fp8(q, s)
    # |W' - W| <= half an e4m3 step of each element (in the scaled domain): relative 2^-4 for normals
    err = (w / s[:, None] - q.float()).abs()
    assert bool((err <= 0.5 * _e4m3_step(w / s[:, None]) + 1e-6).all())
    normal = (w / s[:, None]).abs() >= 2.0 ** -6
    assert bool(((wq - w).abs()[normal] <= (2.0 ** -4) * w.abs()[normal] + 1e-12).all())


def test_quantizer_zero_rows_and_no_nan_at_the_row_amax():
    w = torch.zeros(4, 64)
    w[1, 3] = 5.0
    w[2] = -1e4                      # every element at the row amax (the cast would give NaN past ~464 without the clamp)
    w[3, :] = torch.linspace(-7, 7, 64)
    q, s = quantize_fp8(w)
    assert float(s[0]) == 1.0 and bool((q[0].float() == 0).all())
    assert not torch.isnan(q.float()).any()
    assert float(q[1, 3].float()) == FP8_MAX and float(q[2, 0].float()) == -FP8_MAX
    assert torch.allclose(dequantize_fp8(q, s)[2], w[2])


def test_prequantized_scales_per_tensor_and_per_channel_give_the_same_rows():
    g = torch.Generator().manual_seed(1)
    q = (torch.randn(32, 64, generator=g) * 40).clamp(-448, 448).to(torch.float8_e4m3fn)
    one = fp8_row_scale(torch.tensor(0.0125), 32, 'x')
    chan = fp8_row_scale(torch.full((32,), 0.0125), 32, 'x')
    col = fp8_row_scale(torch.full((32, 1), 0.0125), 32, 'x')
    assert torch.equal(one, chan) and torch.equal(chan, col)
    assert torch.equal(dequantize_fp8(q, one), dequantize_fp8(q, col))
    with pytest.raises(ValueError):
        fp8_row_scale(torch.ones(31), 32, 'x')


def _lane_src(head_dim):
    """la_head_lane_map restated: lane j carries feature d = j % 64 of the first half (j < 64) or of the second (j >= 64), -1 past it"""
    half = head_dim // 2
    return np.array([(j & 63) if (j & 63) < half and j < 64 else half + (j & 63) if (j & 63) < half else -1 for j in range(128)],
                    dtype=np.int32)


@pytest.mark.parametrize('head_dim', [128, 64])
def test_qkv_scales_follow_the_rows_through_the_lanes_and_the_concatenation(head_dim):
    """q / k / v rows spread over the 128-feature lanes and concatenated: row slot * 128 + lane of the lane-ordered scale vector is the
    scale of the source row of that lane (1 on padding lanes), and the e4m3 bytes move with it; o_proj columns move, its scales stay."""
    nh, nkv, K = 3, 1, 32
    src = _lane_src(head_dim)
    g = torch.Generator().manual_seed(2)
    parts, want_q, want_s = [], [], []
    for n_h in (nh, nkv, nkv):
        q, s = quantize_fp8(torch.randn(n_h * head_dim, K, generator=g) * torch.rand(n_h * head_dim, 1, generator=g))
        qq, ss = fp8_lanes(q.view(torch.uint8), s, n_h, 0, src)
        parts.append((qq, ss))
        for h in range(n_h):
            for lane in range(128):
                r = h * head_dim + int(src[lane])
                want_q.append(q.view(torch.uint8)[r] if src[lane] >= 0 else torch.zeros(K, dtype=torch.uint8))
                want_s.append(float(s[r]) if src[lane] >= 0 else 1.0)
    q_all = torch.cat([a for a, _ in parts], 0)
    s_all = torch.cat([b for _, b in parts])
    assert q_all.shape == ((nh + 2 * nkv) * 128, K) and s_all.shape == ((nh + 2 * nkv) * 128,)
    assert torch.equal(q_all, torch.stack(want_q)) and torch.equal(s_all, torch.tensor(want_s))
    qo, so = quantize_fp8(torch.randn(64, nh * head_dim, generator=g))
    qo8, so8 = fp8_lanes(qo.view(torch.uint8), so, nh, 1, src)
    assert torch.equal(so8, so) and qo8.shape == (64, nh * 128)
    for h in range(nh):
        for lane in range(128):
            col = qo8[:, h * 128 + lane]
            assert torch.equal(col, qo.view(torch.uint8)[:, h * head_dim + int(src[lane])] if src[lane] >= 0 else torch.zeros_like(col))


def _tiny():
    return LlamaShape(2, 128, 2, 2, 256, 256, 1e-5)


def _fp8_sd(shape, per_tensor=True, drop=None, seed=0):
    sd = random_weights(shape, seed=seed, device='cpu')
    for k in list(sd):
        if k.startswith('model.layers.') and k.endswith('_proj.weight'):
            q, s = quantize_fp8(sd[k])
            sd[k] = q
            sd[k[:-len('weight')] + 'weight_scale'] = s.max().reshape(()) if per_tensor else s
            sd[k[:-len('weight')] + 'input_scale'] = torch.tensor(1.0)
    if drop:
        del sd[drop]
    return sd


def test_weight_format_selection():
    shape = _tiny()
    assert check_weight_format(shape, random_weights(shape, device='cpu')) is None
    assert check_weight_format(shape, random_weights(shape, device='cpu'), 'fp8') == 'fp8'
    assert check_weight_format(shape, _fp8_sd(shape)) == 'fp8'                     # the tensor format selects fp8 by itself
    assert check_weight_format(shape, _fp8_sd(shape, per_tensor=False), 'fp8') == 'fp8'


@pytest.mark.parametrize('case', ['no_scale', 'blockwise', 'mixed', 'explicit16', 'moe', 'max_blocks', 'fuse', 'unfused_qkv',
                                  'gemm_variant', 'bad_name', 'scale_on_16bit', 'fp8_lm_head', 'fp8_experts', 'e5m2'])
def test_refusals_raise_before_any_gpu_check(case):
    shape = _tiny()
    kw = {}
    if case == 'no_scale':
        sd = _fp8_sd(shape, drop='model.layers.1.mlp.down_proj.weight_scale')
    elif case == 'blockwise':
        sd = _fp8_sd(shape)
        sd['model.layers.0.self_attn.q_proj.weight_scale_inv'] = sd.pop('model.layers.0.self_attn.q_proj.weight_scale')
    elif case == 'mixed':
        sd = _fp8_sd(shape)
        sd['model.layers.0.mlp.up_proj.weight'] = sd['model.layers.0.mlp.up_proj.weight'].to(torch.bfloat16)
        del sd['model.layers.0.mlp.up_proj.weight_scale']
    elif case == 'explicit16':
        sd, kw = _fp8_sd(shape), dict(weight_format='bf16')
    elif case == 'moe':
        shape = LlamaShape(2, 128, 2, 2, 256, 256, 1e-5, n_experts=4, top_k=2)
        sd, kw = random_weights(shape, device='cpu'), dict(weight_format='fp8')
    elif case == 'max_blocks':
        sd, kw = random_weights(shape, device='cpu'), dict(weight_format='fp8', max_blocks=2)
    elif case == 'fuse':
        sd, kw = random_weights(shape, device='cpu'), dict(weight_format='fp8', fuse=1)
    elif case == 'unfused_qkv':
        sd, kw = random_weights(shape, device='cpu'), dict(weight_format='fp8', gemm_cfg=[2, -1])
    elif case == 'gemm_variant':
        sd, kw = random_weights(shape, device='cpu'), dict(weight_format='fp8', gemm_cfg=[0, 0, 1])
    elif case == 'bad_name':
        sd, kw = random_weights(shape, device='cpu'), dict(weight_format='int4')
    elif case == 'fp8_lm_head':          # 16-bit projections, an fp8 lm_head: no fp8 consumer, refused rather than cast
        sd = random_weights(shape, device='cpu')
        sd['lm_head.weight'], sd['lm_head.weight_scale'] = quantize_fp8(sd['lm_head.weight'])
    elif case == 'fp8_experts':          # fp8 MoE experts next to 16-bit attention projections
        shape = LlamaShape(2, 128, 2, 2, 256, 256, 1e-5, n_experts=4, top_k=2)
        sd = random_weights(shape, device='cpu')
        k = next(k for k in sd if k.endswith('experts.0.w1.weight'))
        sd[k], sd[k[:-len('weight')] + 'weight_scale'] = quantize_fp8(sd[k])
    elif case == 'e5m2':
        sd = _fp8_sd(shape)
        k = 'model.layers.0.mlp.down_proj.weight'
        sd[k] = sd[k].float().to(torch.float8_e5m2)
    else:
        sd = random_weights(shape, device='cpu')
        sd['model.layers.0.mlp.up_proj.weight_scale'] = torch.tensor(1.0)
    with pytest.raises(ValueError):
        LlamaVerifyEngine(shape, sd, max_length=128, **kw)


def test_batch_front_doors_refuse_fp8():
    shape = _tiny()
    with pytest.raises(ValueError, match='batch'):
        modeling_llama_batch.LlamaForCausalLM(shape, random_weights(shape, device='cpu'), weight_format='fp8')
    with pytest.raises(ValueError):        # a pre-quantized state dict through the batch path: multi-block, refused as well
        modeling_llama_batch.LlamaForCausalLM(shape, _fp8_sd(shape))
    assert issubclass(modeling_qwen2.BatchQwen2ForCausalLM, modeling_llama_batch.LlamaForCausalLM)
