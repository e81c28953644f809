# -*- coding: utf-8 -*-
"""LlamaVerifyEngine — host-side owner of the device memory behind la_llama_* (the verify forward).

Plumbing only: torch allocates HBM (weights repacked into MFMA-fragment order, KV caches, scratch),
provides the stream and pinned staging buffers; every kernel of the step is hand-written HIP inside
liblookahead_hip.so (csrc/la_kernels.hip, csrc/la_engine.cpp).  There is no torch fallback: without a
GPU the constructor raises.

Reference counterpart: LlamaForCausalLM.forward under the rank-4 mask hook
(lookahead/lookahead/models/llama/modeling_llama.py:544-677, 710-794), called once per verify step
from lookahead_generation (common/pretrained_model.py:1176-1181).
"""
import ctypes as C
import math
import re

import numpy as np
import torch

from . import _lib
from ._lib import lib, check
from .weight_images import (FP8_MAX, StateDictSource, WeightPacker, dequantize_fp8, fp8_lanes, fp8_row_scale,  # noqa: F401 — re-exported
                            pack_layer, qkv_mb_workgroups, quantize_fp8, to_lanes)


class LlamaShape(object):
    """The fields of LlamaConfig the path uses."""

    def __init__(self, n_layers=32, hidden=4096, n_heads=32, n_kv_heads=None, ffn=11008, vocab=32000,
                 rms_eps=1e-5, rope_theta=10000.0, head_dim=None, n_experts=0, top_k=2, norm_cast_first=False, sliding_window=0,
                 qkv_bias=False, qk_norm=False):
        self.n_layers, self.hidden, self.n_heads = n_layers, hidden, n_heads
        # Qwen3: q_norm / k_norm, an RMSNorm over the head_dim features of every q and k head between the projection and RoPE
        # (one device stage behind every QKV launch, csrc/la_qknorm.hip); the projections carry no bias
        self.qk_norm = bool(qk_norm)
        # Qwen2 (Qwen1.5 / Qwen2 / Qwen2.5): q_proj / k_proj / v_proj carry a bias (qwen2/modeling_qwen2.py:234-237), added in the
        # fp32 epilogue of every QKV launch; o_proj and the MLP have none
        self.qkv_bias = bool(qkv_bias)
        self.n_experts, self.top_k = n_experts, top_k       # > 0: Mixtral sparse-MoE MLP
        # RMSNorm flavour: False = LlamaRMSNorm (one rounding), True = Mistral/MixtralRMSNorm (normalised value rounded
        # to the activation dtype before the weight multiply, mixtral/modeling_mixtral.py:160-165)
        self.norm_cast_first = bool(norm_cast_first)
        # 0 = full attention (what the reference's lookahead path does for every family); > 0 = sliding window (extension)
        self.sliding_window = int(sliding_window)
        self.n_kv_heads = n_kv_heads if n_kv_heads is not None else n_heads
        self.ffn, self.vocab, self.rms_eps, self.rope_theta = ffn, vocab, rms_eps, rope_theta
        self.head_dim = head_dim if head_dim is not None else hidden // n_heads

    @classmethod
    def llama2_7b(cls):
        return cls(32, 4096, 32, 32, 11008, 32000, 1e-5)

    @classmethod
    def llama2_13b(cls):
        return cls(40, 5120, 40, 40, 13824, 32000, 1e-5)

    @classmethod
    def mistral_7b(cls):
        return cls(32, 4096, 32, 8, 14336, 32000, 1e-5, rope_theta=10000.0, norm_cast_first=True)

    @classmethod
    def mixtral_8x7b(cls):
        return cls(32, 4096, 32, 8, 14336, 32000, 1e-5, rope_theta=1e6, n_experts=8, top_k=2, norm_cast_first=True)

    @classmethod
    def qwen2_7b(cls):
        """Qwen2.5-7B (Qwen2-7B: the same layer shape)"""
        return cls(28, 3584, 28, 4, 18944, 152064, 1e-6, rope_theta=1e6, norm_cast_first=True, qkv_bias=True)

    @classmethod
    def qwen2_0_5b(cls):
        """Qwen2-0.5B / Qwen2.5-0.5B: head_dim 64, tied embeddings (lm_head = embed_tokens)"""
        return cls(24, 896, 14, 2, 4864, 151936, 1e-6, rope_theta=1e6, norm_cast_first=True, qkv_bias=True)

    @classmethod
    def qwen3_8b(cls):
        """Qwen3-8B"""
        return cls(36, 4096, 32, 8, 12288, 151936, 1e-6, rope_theta=1e6, head_dim=128, norm_cast_first=True, qk_norm=True)

    @classmethod
    def qwen3_0_6b(cls):
        """Qwen3-0.6B: n_heads * head_dim = 2048 != hidden, tied embeddings (lm_head = embed_tokens)"""
        return cls(28, 1024, 16, 8, 3072, 151936, 1e-6, rope_theta=1e6, head_dim=128, norm_cast_first=True, qk_norm=True)

    @classmethod
    def from_hf(cls, cfg):
        """LlamaConfig / MistralConfig / MixtralConfig of transformers 4.3x (the reference's pins) or 5.x (rope_theta moved
        into cfg.rope_parameters)."""
        rope_theta = getattr(cfg, 'rope_theta', None)
        if rope_theta is None:
            rp = getattr(cfg, 'rope_parameters', None) or {}
            rope_theta = rp.get('rope_theta', 10000.0) if isinstance(rp, dict) else getattr(rp, 'rope_theta', 10000.0)
        scaling = getattr(cfg, 'rope_scaling', None)
        if scaling and (scaling.get('rope_type', scaling.get('type', 'default')) not in ('default', None)):
            raise NotImplementedError(f'rope_scaling {scaling} is not supported by the RoPE tables of this path')
        head_dim = getattr(cfg, 'head_dim', None) or cfg.hidden_size // cfg.num_attention_heads
        kind = getattr(cfg, 'model_type', 'llama')
        if kind == 'qwen3' and getattr(cfg, 'attention_bias', False):
            raise ValueError('qwen3 with attention_bias=True: the o_proj bias has no consumer here; refusing to drop it')
        return cls(cfg.num_hidden_layers, cfg.hidden_size, cfg.num_attention_heads,
                   getattr(cfg, 'num_key_value_heads', None), cfg.intermediate_size, cfg.vocab_size,
                   cfg.rms_norm_eps, float(rope_theta), head_dim=head_dim,
                   n_experts=getattr(cfg, 'num_local_experts', 0) or 0, top_k=getattr(cfg, 'num_experts_per_tok', 2),
                   norm_cast_first=kind in ('mistral', 'mixtral', 'qwen2', 'qwen3'),
                   qkv_bias=kind == 'qwen2', qk_norm=kind == 'qwen3')

    def n_params_no_embed(self):
        hd = self.head_dim
        mlp = 3 * self.ffn * self.hidden * max(self.n_experts, 1) + self.n_experts * self.hidden
        per_layer = (self.n_heads + 2 * self.n_kv_heads) * hd * self.hidden + self.n_heads * hd * self.hidden \
            + mlp + 2 * self.hidden + (self.n_heads + 2 * self.n_kv_heads) * hd * int(self.qkv_bias) + 2 * hd * int(self.qk_norm)
        return self.n_layers * per_layer + self.hidden + self.vocab * self.hidden


def legacy_state_dict(sd, shape):
    """HF-named state dict -> the transformers-4.36 parameter names the engine consumes (the reference's model files:
    block_sparse_moe.gate / experts.{e}.w1|w3|w2, mixtral/modeling_mixtral.py:668-759).  transformers 5.x stores the experts of
    a layer fused: mlp.gate.weight [E, hidden], mlp.experts.gate_up_proj [E, 2*ffn, hidden] (gate rows first),
    mlp.experts.down_proj [E, hidden, ffn]; tied lm_head falls back to the embedding."""
    out = {}
    for k, v in sd.items():
        v = v.detach()
        if shape.n_experts > 0 and k.endswith('.mlp.gate.weight'):
            out[k.replace('.mlp.gate.weight', '.block_sparse_moe.gate.weight')] = v
        elif shape.n_experts > 0 and k.endswith('.mlp.experts.gate_up_proj'):
            p = k[:-len('mlp.experts.gate_up_proj')] + 'block_sparse_moe.experts.'
            for e in range(shape.n_experts):
                out[f'{p}{e}.w1.weight'] = v[e, :shape.ffn]
                out[f'{p}{e}.w3.weight'] = v[e, shape.ffn:]
        elif shape.n_experts > 0 and k.endswith('.mlp.experts.down_proj'):
            p = k[:-len('mlp.experts.down_proj')] + 'block_sparse_moe.experts.'
            for e in range(shape.n_experts):
                out[f'{p}{e}.w2.weight'] = v[e]
        else:
            out[k] = v
    if 'lm_head.weight' not in out:
        out['lm_head.weight'] = out['model.embed_tokens.weight']
    return out


def load_hf_checkpoint(model_dir):
    """(transformers config, HF-named state dict on CPU) of a checkpoint directory: config.json plus *.safetensors (sharded or
    not) or pytorch_model*.bin — what LlamaForCausalLM.from_pretrained(model_dir, ...) of the reference's examples resolves
    (examples/llama_example.py:19-24).  Tensors are read shard by shard; nothing is instantiated as an nn.Module."""
    import glob
    import json
    import os
    from transformers import AutoConfig
    cfg = AutoConfig.from_pretrained(model_dir)
    sd = {}
    # consolidated*.safetensors (Mistral / Mixtral repos ship them NEXT to the HF shards, under other key names) would double
    # the host memory and leave keys nobody consumes
    st_files = sorted(f for f in glob.glob(os.path.join(model_dir, '*.safetensors'))
                      if not os.path.basename(f).startswith('consolidated'))
    idx = os.path.join(model_dir, 'model.safetensors.index.json')
    if os.path.exists(idx):
        names = sorted(set(json.load(open(idx))['weight_map'].values()))
        st_files = [os.path.join(model_dir, n) for n in names]
    if st_files:
        from safetensors import safe_open
        for f in st_files:
            with safe_open(f, framework='pt', device='cpu') as fh:
                for k in fh.keys():
                    sd[k] = fh.get_tensor(k)
    else:
        bins = sorted(glob.glob(os.path.join(model_dir, 'pytorch_model*.bin')))
        if not bins:
            raise FileNotFoundError(f'no *.safetensors or pytorch_model*.bin under {model_dir}')
        for f in bins:
            sd.update(torch.load(f, map_location='cpu', weights_only=True))
    return cfg, sd


def rope_tables(head_dim, max_pos, theta, device, dtype=torch.bfloat16):
    """cos/sin exactly as LlamaRotaryEmbedding.forward (modeling_llama.py:93-126): fp32 outer product,
    cos()/sin() in fp32, cast to the activation dtype (bfloat16 or float16).  Only the first head_dim/2 columns are stored
    (emb = cat(freqs, freqs))."""
    inv_freq = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.int64).float() / head_dim))
    pos = torch.arange(max_pos, dtype=torch.int64).float()
    freqs = (inv_freq[:, None].float() @ pos[None, :].float()).transpose(0, 1)      # [max_pos, hd/2]
    return freqs.cos().to(dtype).to(device).contiguous(), freqs.sin().to(dtype).to(device).contiguous()


def random_weights(shape, seed=0, std=0.02, device='cpu', dtype=torch.bfloat16, decisive=False):
    """Random-init weights in HF Llama naming (initializer_range=0.02, norms = 1), generated layer by layer on
    `device` (no checkpoints are available).

    decisive=True builds the synthetic "permutation LM" used by bench.py: same shapes and byte counts, but
    o_proj / down_proj are drawn with std 1e-4 (the residual stream stays dominated by the token embedding) and
    lm_head[pi(t)] = embed[t] for a fixed random permutation pi, so greedy decoding has a logit margin of several
    units instead of the ~3 bf16 ulps of a pure random-init model.  With pure random init, greedy and tree-verify
    decoding legitimately drift apart after ~20 tokens in bf16 (the reference README warns of the same in fp16/bf16,
    lookahead/README.md:45), which would make a trie warmed on the greedy continuation useless."""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    hd = shape.head_dim

    def w(n, k, s=std):
        return (torch.randn(n, k, generator=g, device=device, dtype=torch.float32) * s).to(dtype)

    out_std = 1e-4 if decisive else std
    sd = {'model.embed_tokens.weight': w(shape.vocab, shape.hidden)}
    for i in range(shape.n_layers):
        p = f'model.layers.{i}.'
        sd[p + 'self_attn.q_proj.weight'] = w(shape.n_heads * hd, shape.hidden)
        sd[p + 'self_attn.k_proj.weight'] = w(shape.n_kv_heads * hd, shape.hidden)
        sd[p + 'self_attn.v_proj.weight'] = w(shape.n_kv_heads * hd, shape.hidden)
        sd[p + 'self_attn.o_proj.weight'] = w(shape.hidden, shape.n_heads * hd, out_std)
        if getattr(shape, 'qkv_bias', False):
            # trained Qwen2 biases are mostly small with a few large K entries (|b| of several units): draw the same kind, so that a
            # lost or misplaced bias changes the tokens
            for nm, n in (('q_proj', shape.n_heads * hd), ('k_proj', shape.n_kv_heads * hd), ('v_proj', shape.n_kv_heads * hd)):
                b = torch.randn(n, generator=g, device=device, dtype=torch.float32) * 0.1
                if nm == 'k_proj':
                    big = torch.rand(n, generator=g, device=device) < 0.1
                    b = torch.where(big, torch.randn(n, generator=g, device=device, dtype=torch.float32) * 4.0, b)
                sd[p + f'self_attn.{nm}.bias'] = b.to(dtype)
        if getattr(shape, 'qk_norm', False):
            # away from 1, so that a lost or swapped norm weight changes the tokens
            for nm in ('q_norm', 'k_norm'):
                sd[p + f'self_attn.{nm}.weight'] = (0.2 + 2.0 * torch.rand(hd, generator=g, device=device, dtype=torch.float32)).to(dtype)
        if shape.n_experts > 0:                      # HF Mixtral naming (w1 = gate, w3 = up, w2 = down)
            sd[p + 'block_sparse_moe.gate.weight'] = w(shape.n_experts, shape.hidden)
            for e in range(shape.n_experts):
                q = p + f'block_sparse_moe.experts.{e}.'
                sd[q + 'w1.weight'] = w(shape.ffn, shape.hidden)
                sd[q + 'w3.weight'] = w(shape.ffn, shape.hidden)
                sd[q + 'w2.weight'] = w(shape.hidden, shape.ffn, out_std)
        else:
            sd[p + 'mlp.gate_proj.weight'] = w(shape.ffn, shape.hidden)
            sd[p + 'mlp.up_proj.weight'] = w(shape.ffn, shape.hidden)
            sd[p + 'mlp.down_proj.weight'] = w(shape.hidden, shape.ffn, out_std)
        sd[p + 'input_layernorm.weight'] = torch.ones(shape.hidden, device=device, dtype=dtype)
        sd[p + 'post_attention_layernorm.weight'] = torch.ones(shape.hidden, device=device, dtype=dtype)
    sd['model.norm.weight'] = torch.ones(shape.hidden, device=device, dtype=dtype)
    if decisive:
        # pi fixes the special ids 0..2 and is ONE cycle over [3, V): a sequence that starts from ordinary tokens never
        # emits token 0, whose drafts the reference mis-roots (`match_token_id or self.token_id`, lookahead_cache.py:129,
        # H1g), and never repeats itself within V-3 tokens (a short cycle would turn the warm-up text periodic)
        order = 3 + torch.randperm(shape.vocab - 3, generator=g, device=device)
        perm = torch.arange(shape.vocab, device=device)
        perm[order] = torch.roll(order, -1)
        head = torch.empty_like(sd['model.embed_tokens.weight'])
        head[perm] = sd['model.embed_tokens.weight']          # lm_head[pi(t)] = embed[t]
        sd['lm_head.weight'] = head
    else:
        sd['lm_head.weight'] = w(shape.vocab, shape.hidden)
    return sd


def check_biases(shape, state_dict):
    """The q/k/v bias of a Qwen2 shape (shape.qkv_bias) is applied in the QKV epilogues; any other bias — Llama's attention_bias=True
    puts one on o_proj too, mlp_bias=True on the MLP — has no kernel here and is REFUSED rather than dropped: dropping it would
    silently compute another model."""
    qkv = re.compile(r'\.self_attn\.[qkv]_proj\.bias$')
    for k in (state_dict or {}):
        if k.endswith('.bias') and not (getattr(shape, 'qkv_bias', False) and qkv.search(k)):
            why = 'q/k/v biases need a shape with qkv_bias=True (Qwen2)' if qkv.search(k) else 'only q_proj / k_proj / v_proj biases are supported'
            raise ValueError(f'the state dict carries {k}: {why}; refusing to drop it')


def check_qk_norm(shape, state_dict):
    """q_norm / k_norm weights and shape.qk_norm (Qwen3) come together: a state dict that carries them under a shape without the stage
    would run as a Llama and silently drop them, a shape with the stage needs every layer's pair.  Both are REFUSED."""
    sd = state_dict or {}
    norm = re.compile(r'\.self_attn\.[qk]_norm\.weight$')
    have = [k for k in sd if norm.search(k)]
    if not getattr(shape, 'qk_norm', False):
        if have:
            raise ValueError(f'the state dict carries {have[0]}: q/k norms need a shape with qk_norm=True (Qwen3); refusing to drop it')
        return
    if int(shape.head_dim) != 128:
        raise ValueError(f'qk_norm with head_dim={shape.head_dim}: the q / k norm stage serves head_dim 128 only')
    if getattr(shape, 'n_experts', 0) > 0:
        raise ValueError('qk_norm: MoE models are not served with the q / k norm stage')
    if sd:
        for i in range(shape.n_layers):
            for nm in ('q_norm', 'k_norm'):
                k = f'model.layers.{i}.self_attn.{nm}.weight'
                if k not in sd:
                    raise ValueError(f'shape.qk_norm is set but the state dict has no {k}')
                if sd[k].numel() != shape.head_dim:
                    raise ValueError(f'{k}: {sd[k].numel()} values for head_dim {shape.head_dim}')


PROJECTIONS = ('self_attn.q_proj', 'self_attn.k_proj', 'self_attn.v_proj', 'self_attn.o_proj', 'mlp.gate_proj', 'mlp.up_proj',
               'mlp.down_proj')
_W16_NAMES = ('storage', 'bf16', 'bfloat16', 'fp16', 'float16')


def check_weight_format(shape, state_dict, weight_format=None, gemm_cfg=None, fuse=0, max_blocks=0):
    """-> 'fp8' or None (the storage type).  weight_format=None: the state dict decides — float8_e4m3fn projections with their
    <proj>.weight_scale select fp8 by themselves; 'fp8' quantizes 16/32-bit projections at load (quantize_fp8).  Everything the fp8
    launches cannot serve is REFUSED here, before any GPU is needed (la_llama_create refuses the same cases as a second line)."""
    if weight_format is not None and weight_format != 'fp8' and weight_format not in _W16_NAMES:
        raise ValueError(f"weight_format={weight_format!r}: None, 'fp8' or a 16-bit name {_W16_NAMES}")
    sd = state_dict or {}
    blockwise = [k for k in sd if k.endswith('.weight_scale_inv')]
    if blockwise:
        raise ValueError(f'{blockwise[0]}: block-wise fp8 scales (128x128 blocks) are not supported; per-tensor or per-row weight_scale only')
    kinds = {}
    for k, v in sd.items():
        if any(k.endswith(f'.{p}.weight') for p in PROJECTIONS) and k.startswith('model.layers.'):
            kinds.setdefault(v.dtype == torch.float8_e4m3fn, k)
            if v.dtype == torch.float8_e4m3fn and k[:-len('weight')] + 'weight_scale' not in sd:
                raise ValueError(f'{k} is float8_e4m3fn but the state dict has no {k[:-len("weight")]}weight_scale')
        elif k.endswith('.weight_scale') and k[:-len('_scale')] in sd and sd[k[:-len('_scale')]].dtype != torch.float8_e4m3fn:
            raise ValueError(f'{k} belongs to a {sd[k[:-len("_scale")]].dtype} weight: scales come with float8_e4m3fn weights only')
    # every other 8-bit float tensor (lm_head, embedding, norms, MoE experts, another fp8 encoding) has no fp8 consumer: the 16-bit
    # path would cast it to the storage type without its scale, i.e. compute another model
    f8 = tuple(getattr(torch, n) for n in ('float8_e4m3fn', 'float8_e5m2', 'float8_e4m3fnuz', 'float8_e5m2fnuz') if hasattr(torch, n))
    for k, v in sd.items():
        if torch.is_tensor(v) and v.dtype in f8 and not (v.dtype == torch.float8_e4m3fn and k.startswith('model.layers.')
                                                         and any(k.endswith(f'.{p}.weight') for p in PROJECTIONS)):
            raise ValueError(f'{k} is {v.dtype}: fp8 weights are supported for the q/k/v, o, gate/up and down projections only '
                             '(OCP e4m3fn with weight_scale); refusing to cast it without its scale')
    if len(kinds) > 1:
        raise ValueError(f'mixed weight formats: {kinds[True]} is float8_e4m3fn, {kinds[False]} is not; the projections must share one format')
    pre = kinds.get(True) is not None
    if pre and weight_format in _W16_NAMES:
        raise ValueError(f'weight_format={weight_format!r} but the projections are float8_e4m3fn ({kinds[True]}); they are not dequantized silently')
    fmt = 'fp8' if (pre or weight_format == 'fp8') else None
    if fmt is None:
        return None
    if getattr(shape, 'n_experts', 0) > 0:
        raise ValueError('fp8 weights: MoE (Mixtral) experts have no fp8 launch')
    if max_blocks > 1:
        raise ValueError('fp8 weights: the multi-block step (max_blocks > 1) has no fp8 launch')
    if fuse:
        raise ValueError('fp8 weights: the fused norm / role-fused launches (fuse != 0) have no fp8 form')
    g = list(gemm_cfg or []) + [0] * 8
    if g[1] < 0:
        raise ValueError('fp8 weights: the unfused QKV (gemm_cfg[1] < 0) has no fp8 launch')
    if (g[0] >> 8) != 0 or g[2] not in (0, 2, 2 | 3 << 8) or g[4] not in (0, 2, 2 | 3 << 8) or g[7] != 0:
        raise ValueError(f'fp8 weights: only the default GEMM plan has fp8 launches (gemm_cfg={list(gemm_cfg)})')
    if shape.hidden % 64:
        raise ValueError('fp8 weights: hidden must be a multiple of 64')
    return fmt


DEFAULT_LAB = False      # engines created without lab=... take the product library; the lab_build fixture of tests/conftest.py flips it for a variant test


class LlamaVerifyEngine(object):
    """One GPU: packed weights + KV cache + the captured step graph.  n_slots = 1: one sequence (the bs=1 loop).
    n_slots > 1: the cursor-batch path — every slot owns a max_keys region of the KV cache and the 64 rows of a
    verify block are shared by the active slots (bstep).

    The weight images are built by weight_images.py (WeightPacker, pack_layer).  Three step families share the engine, each with its
    own pinned input / result block: the single-sequence step (step / verify_only / commit: _fill writes LA_IN_*, step_finish and
    commit read LA_ST_*), the cursor batch (bstep / bcommit: LA_BIN_* written and LA_BST_* read in place) and the multi-block step
    (mstep / mstep_trie / tstep / mstep_trees and their commits: _put_block / _put_trees write LA_MIN_*, _mlaunch queues the pass,
    _mout_read decodes LA_MOUT_*, _mcommit keeps rows)."""

    def __init__(self, shape, state_dict, max_length=2048, device='cuda:0', attn_split=0, gemm_cfg=None,
                 consume_state_dict=False, balanced=True, n_slots=1, fuse=0, max_blocks=0, kv_ring=False, dtype=None, lab=None,
                 weight_format=None):
        check_biases(shape, state_dict)
        check_qk_norm(shape, state_dict)
        if getattr(shape, 'qk_norm', False) and fuse:
            raise ValueError('qk_norm: the fused norm / role-fused launches (fuse != 0) are not served with the q / k norm stage')
        # weight_format: None (the state dict decides) or 'fp8' — W8A16, see check_weight_format / quantize_fp8
        self.weight_format = check_weight_format(shape, state_dict, weight_format, gemm_cfg, fuse, max_blocks)
        w8 = self.weight_format == 'fp8'
        if not torch.cuda.is_available():
            raise RuntimeError('LlamaVerifyEngine needs an MI355X: the verify step has no CPU fallback')
        # The engine computes in the checkpoint's own 16-bit type: bfloat16 (BASELINE) or float16 (what the reference's examples and
        # benchmarks load, benchmarks/llama_benchmark.py:27) — one library build per type (_lib.lib_for), never a silent conversion.
        # dtype=None: the dtype of the state dict's lm_head (fp32 state dicts run as bfloat16, as before).
        if dtype is None:
            dtype = state_dict['lm_head.weight'].dtype if state_dict and 'lm_head.weight' in state_dict else torch.bfloat16
            if dtype not in (torch.bfloat16, torch.float16):
                dtype = torch.bfloat16
        self.dtype = dtype
        # lab=True: the LAB build of the same sources (measurement knobs / A/B switches, _lib.lab_set) instead of the product library
        self.lab = DEFAULT_LAB if lab is None else bool(lab)
        self._lib = _lib.lab_lib_for(dtype) if self.lab else _lib.lib_for(dtype)
        self.shape = shape
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        self.kv_ring = bool(kv_ring)
        if self.kv_ring:
            # sliding-window ring (extension, SURVEY H3 / BASELINE config 3): KV memory O(window) per sequence instead of O(max_length)
            win = int(getattr(shape, 'sliding_window', 0))
            assert win > 0, 'kv_ring needs shape.sliding_window > 0'
            self.max_keys = int(math.ceil((win + 64 * max(int(max_blocks), 1) + 64) / 32.0)) * 32
            self.max_pos = max_length + 64 + 64 + 2      # _capacity() = max_length + 65, as the linear cache admits
        else:
            self.max_keys = int(math.ceil((max_length + 64 + 1) / 32.0)) * 32
            self.max_pos = self.max_keys + 64
        # a dedicated non-default stream: hipStreamBeginCapture is illegal on the legacy NULL stream that
        # torch.cuda.current_stream() returns by default
        self.stream = torch.cuda.Stream(self.device)
        # Every kernel lays a head out as a 128-feature lane (RoPE pairs (d, d + 64), 8192-element Q / K / V fragments).  A model whose
        # heads are narrower (LlamaAttention is shape-generic, modeling_llama.py:189-308) runs in the same lanes: its q / k / v rows and
        # o_proj columns are spread over the lanes by la_head_lane_map (feature d -> lane d, its rotary partner d + hd/2 -> lane 64 + d,
        # zeros elsewhere) BEFORE packing (weight_images.to_lanes); zero lanes add exact zeros to every dot product, and cfg.head_dim —
        # the real one — sets the softmax scale.  hd below is the LANE width every size is computed from.
        self.head_dim = int(shape.head_dim)
        if not (8 <= self.head_dim <= 128 and self.head_dim % 2 == 0):
            raise ValueError(f'head_dim={self.head_dim}: even values from 8 to 128 are supported (128-feature lanes)')
        hd = 128
        lane_src = np.zeros(128, dtype=np.int32)
        check(self._lib.la_head_lane_map(self.head_dim, lane_src.ctypes.data_as(_lib.pi32)), 'head_lane_map')
        self._lane_src = lane_src
        packer = WeightPacker(self._lib, self.stream, self.device, self.dtype)
        self._keep = packer.keep
        src = StateDictSource(state_dict, consume_state_dict, self.device, w8)

        # Balanced GEMMs: one workgroup per CU, rows dealt out by la_rowplan (0 = shape not balanceable -> classic grid); the
        # multi-block step may get a second QKV image over fewer, fuller workgroups (qkv_mb_workgroups)
        self.qkv_fused = not (gemm_cfg and len(gemm_cfg) > 1 and gemm_cfg[1] < 0)
        n_cu = torch.cuda.get_device_properties(self.device).multi_processor_count
        n_qkv = (shape.n_heads + 2 * shape.n_kv_heads) * hd
        self.balanced_wg = [0, 0, 0]
        if balanced and self.qkv_fused:
            for slot, (kind, n_rows) in enumerate([(2, n_qkv), (1, shape.ffn), (0, shape.vocab)]):
                if packer.add_plan(slot, kind, n_rows, n_cu):
                    self.balanced_wg[slot] = n_cu
        want = qkv_mb_workgroups(shape.n_heads, shape.n_kv_heads, self.balanced_wg[0], max_blocks, hd)
        self.qkv_mb_wg = want if want and packer.add_plan('qkv_mb', 2, n_qkv, want) else 0

        # rows of [Wq;Wk;Wv] are gathered so that each GEMM workgroup owns RoPE pairs (d, d+64): the QKV epilogue
        # applies RoPE and writes the attention fragments itself (la_gemm64_qkv)
        perm_np = np.zeros(n_qkv, dtype=np.int32)
        check(self._lib.la_qkv_row_perm(shape.n_heads, shape.n_kv_heads, perm_np.ctypes.data_as(_lib.pi32)), 'qkv_row_perm')
        qkv_perm = torch.from_numpy(perm_np.astype(np.int64)).to(self.device) if self.qkv_fused else None
        layers = (_lib.LlamaLayerWeightsC * shape.n_layers)()
        for i in range(shape.n_layers):
            pack_layer(packer, src, shape, i, layers[i], lane_src, qkv_perm)
        self._layers = layers
        self.embed = packer.hold(src.take('model.embed_tokens.weight'))
        self.rope_cos, self.rope_sin = rope_tables(self.head_dim, self.max_pos, shape.rope_theta, self.device, self.dtype)
        if self.head_dim < 128:          # 64 columns per position: the lanes past head_dim / 2 only ever meet zeros
            padc = torch.ones((self.max_pos, 64), dtype=self.dtype, device=self.device)
            pads = torch.zeros((self.max_pos, 64), dtype=self.dtype, device=self.device)
            padc[:, :self.head_dim // 2] = self.rope_cos
            pads[:, :self.head_dim // 2] = self.rope_sin
            self.rope_cos, self.rope_sin = padc.contiguous(), pads.contiguous()
        w = _lib.LlamaWeightsC()
        w.embed = self.embed.data_ptr()
        proj_bytes = packer.nbytes
        w.lm_head = packer.planned_or_plain(2, [src.take('lm_head.weight')]).data_ptr()
        # device bytes of the weights the step streams: projection images (fp8: with their scales), lm_head image, embedding
        self.weight_bytes = {'projections': proj_bytes, 'lm_head': packer.nbytes - proj_bytes,
                             'embed': self.embed.numel() * self.embed.element_size()}
        w.final_norm = packer.hold(src.take('model.norm.weight')).data_ptr()
        w.rope_cos, w.rope_sin = self.rope_cos.data_ptr(), self.rope_sin.data_ptr()
        if getattr(shape, 'qk_norm', False):
            # the QKV launches of a qk_norm model run with identity tables (cos = 1, sin = 0) and leave the rounded projection output;
            # la_qk_norm_rope behind them normalises and applies the real tables
            self.rope_cos_id, self.rope_sin_id = torch.ones_like(self.rope_cos), torch.zeros_like(self.rope_sin)
        w.layers = C.cast(layers, C.POINTER(_lib.LlamaLayerWeightsC))
        torch.cuda.synchronize(self.device)

        cfg = _lib.LlamaConfigC()
        cfg.n_layers, cfg.hidden, cfg.n_heads, cfg.n_kv_heads = shape.n_layers, shape.hidden, shape.n_heads, shape.n_kv_heads
        cfg.head_dim, cfg.ffn, cfg.vocab = self.head_dim, shape.ffn, shape.vocab
        cfg.max_keys, cfg.max_pos, cfg.attn_split, cfg.rms_eps = self.max_keys, self.max_pos, attn_split, shape.rms_eps
        for i, v in enumerate(gemm_cfg or []):
            cfg.gemm_cfg[i] = int(v)
        for i in range(3):
            cfg.balanced_wg[i] = self.balanced_wg[i]
        assert 1 <= n_slots <= _lib.LA_MAX_SEQ
        self.n_slots = int(n_slots)
        cfg.n_slots = self.n_slots
        cfg.n_experts, cfg.top_k = shape.n_experts, shape.top_k
        cfg.norm_cast_first = int(shape.norm_cast_first)
        cfg.qkv_mb_wg = int(self.qkv_mb_wg)
        cfg.fuse = int(fuse)
        assert 0 <= max_blocks <= _lib.LA_MB_MAX
        self.max_blocks = int(max_blocks) if max_blocks > 1 else 0
        cfg.max_blocks = self.max_blocks
        cfg.sliding_window = int(getattr(shape, 'sliding_window', 0))
        cfg.kv_ring = int(self.kv_ring)
        cfg.weight_format = 1 if w8 else 0
        self._cfg = cfg
        nbytes = self._lib.la_llama_workspace_bytes(C.byref(cfg))
        if nbytes <= 0:
            raise _lib.LookaheadHipError(f'la_llama_workspace_bytes: {_lib.last_error()}')
        self.workspace = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        if getattr(shape, 'qk_norm', False):
            qk = _lib.QkNormWeightsC()
            self._qk_arrays = [(_lib.vp * shape.n_layers)(*[pair[i] for pair in packer.qk_norms]) for i in (0, 1)]
            qk.q_norm, qk.k_norm = (C.cast(a, C.POINTER(_lib.vp)) for a in self._qk_arrays)
            qk.rope_cos_id, qk.rope_sin_id = self.rope_cos_id.data_ptr(), self.rope_sin_id.data_ptr()
            self._h = self._lib.la_llama_create_qk_norm(C.byref(cfg), C.byref(w), C.byref(qk), self.workspace.data_ptr(), nbytes)
        else:
            self._h = self._lib.la_llama_create(C.byref(cfg), C.byref(w), self.workspace.data_ptr(), nbytes)
        if not self._h:
            raise _lib.LookaheadHipError(f'la_llama_create: {_lib.last_error()}')
        self._alloc_host_blocks()
        self.slot_keys = [0] * self.n_slots
        self.n_keys = 0
        self.repetition_penalty = 1.0
        self._pen_ctx = {}
        self.sampling = False
        self.logprobs_on = False
        self.top_logprobs_n = 0
        self.reset()

    def _alloc_host_blocks(self):
        """the pinned input / result blocks of the three step families and their numpy views (row masks as uint64)"""
        def pinned(words):
            t = torch.zeros(words, dtype=torch.int32).pin_memory()
            return t, t.numpy()
        self.host_in, self._in_np = pinned(_lib.LA_IN_WORDS)
        self.host_out, self._out_np = pinned(_lib.LA_ST_OUTTOK + 64)
        self._in_rm = self._in_np[_lib.LA_IN_ROWMASK:_lib.LA_IN_ROWMASK + 128].view(np.uint64)
        self.host_bin, self._bin_np = pinned(_lib.LA_BIN_WORDS)
        self.host_bout, self._bout_np = pinned(_lib.LA_BST_DST)
        self._bin_rm = self._bin_np[_lib.LA_BIN_ROWMASK:_lib.LA_BIN_ROWMASK + 128].view(np.uint64)
        if self.max_blocks:
            self.host_min, self._min_np = pinned(_lib.LA_MIN_WORDS)
            self.host_mout, self._mout_np = pinned(_lib.LA_MOUT_DST)
            self._min_rm = self._min_np[_lib.LA_MIN_ROWMASK:_lib.LA_MIN_ROWMASK + 2 * 64 * _lib.LA_MB_MAX].view(np.uint64)
            self._min_xm = self._min_np[_lib.LA_MIN_XMASK:_lib.LA_MIN_XMASK + 2 * 3 * 64 * _lib.LA_MB_MAX].view(np.uint64).reshape(_lib.LA_MB_MAX * 64, 3)

    def __del__(self):
        h = getattr(self, '_h', None)
        if h:
            self._lib.la_llama_destroy(h)
            self._h = None

    # ------------------------------------------------------------------------------------------------
    def _sp(self):
        return C.c_void_p(self.stream.cuda_stream)

    def _capacity(self):
        """keys a sequence may hold: the cache size, or (ring) whatever the RoPE tables cover"""
        return self.max_pos - 65 if self.kv_ring else self.max_keys

    def reset(self):
        check(self._lib.la_llama_reset(self._h, self._sp()), 'llama_reset')
        self.n_keys = 0
        self.slot_keys = [0] * self.n_slots
        self._pen_ctx = {}

    # ---- repetition penalty on the device (csrc/la_penalty.hip) -------------------------------------------------------------
    def set_repetition_penalty(self, penalty):
        """transformers' RepetitionPenaltyLogitsProcessor(penalty) as a stage of every verify step (step / decode_native / bstep /
        mstep, first token after a prefill included): the penalised argmax of every live tree row is taken on the device and the
        fused accept walk runs on it, emitting what the host walk over verify_only + commit emits.  1.0 = off (the default: the
        steps launch exactly what they launch without this stage).  The context set of a slot is seeded by prefill / bprefill /
        mprefill (the prompt, or what seed_penalty_context recorded for the slot) and kept current on the device afterwards."""
        penalty = float(penalty)
        check(self._lib.la_llama_set_repetition_penalty(self._h, self._sp(), penalty), 'set_repetition_penalty')
        self.repetition_penalty = penalty

    def seed_penalty_context(self, slot, tokens):
        """The context set of `slot` := set(tokens), now, and again from the same tokens when the slot's next prefill reaches the
        pass that holds the prompt's last row (a prefill chain emits a token per pass; only the last one is read).  The batch loops
        hand the left-padded row here, pads included: that is what the reference's walk hands the processor."""
        tokens = [int(x) for x in tokens]
        self._pen_ctx[int(slot)] = tokens
        self._pen_seed(int(slot), tokens)

    def _pen_seed(self, slot, tokens):
        arr = np.ascontiguousarray(tokens, dtype=np.int32)
        check(self._lib.la_llama_penalty_seed(self._h, self._sp(), int(slot), arr.ctypes.data_as(_lib.pi32), len(arr)), 'penalty_seed')

    def _pen_seed_final(self, slot, prompt_ids):
        """before the prefill pass that holds the last row of `slot`'s prompt (no-op while the penalty is off)"""
        if self.repetition_penalty != 1.0:
            self._pen_seed(slot, self._pen_ctx.pop(slot, prompt_ids))

    def penalty_launches(self):
        """steps launched with the penalty stage since the engine was created"""
        return int(self._lib.la_llama_penalty_launches(self._h))

    # ---- sampling on the device (csrc/la_sample.hip) ------------------------------------------------------------------------
    def set_sampling(self, enabled, seed=0, temperature=1.0, top_k=0, top_p=1.0):
        """do_sample as a stage of every verify step (step / decode_native / bstep / mstep, first token after a prefill included):
        the seeded temperature / top-k / top-p token of every live tree row is drawn on the device where the argmax went, and the
        fused accept walk runs on it.  The draw depends on (seed, stream of the slot, position, token) only, so the same seed gives
        the same sequence with and without drafts.  Off (the default): the steps launch exactly what they launch without the
        stage.  With set_repetition_penalty on as well, the stage penalises the context members first.  top_k 0 / top_p 1.0: off."""
        check(self._lib.la_llama_set_sampling(self._h, self._sp(), 1 if enabled else 0, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                              float(temperature), int(top_k), float(top_p)), 'set_sampling')
        self.sampling = bool(enabled)

    def sampling_stream(self, slot, stream_id):
        """the stream word of `slot` (default: the slot index): what tells the sequences of one seed apart"""
        check(self._lib.la_llama_sampling_stream(self._h, self._sp(), int(slot), int(stream_id) & 0xFFFFFFFF), 'sampling_stream')

    def sample_launches(self):
        """steps launched with the sampling stage since the engine was created"""
        return int(self._lib.la_llama_sample_launches(self._h))

    # ---- log-probabilities on the device (csrc/la_logprob.hip) --------------------------------------------------------------
    def set_logprobs(self, enabled):
        """The model's own log-softmax value of every token a step emits (raw logits: before any penalty, temperature or filter),
        taken on the device after the accept scan of every step form (step / decode_native / bstep / mstep, first token after a
        prefill included) and kept in a position-indexed log per slot; read it with logprobs().  Off (the default): the steps
        launch exactly what they launch without the stage."""
        check(self._lib.la_llama_set_logprobs(self._h, self._sp(), 1 if enabled else 0), 'set_logprobs')
        self.logprobs_on = bool(enabled)

    def logprobs(self, slot, first_pos, n):
        """np.float32[n]: the log-probabilities of the tokens at positions first_pos .. first_pos + n of `slot`'s unpadded
        sequence (NaN: no step with the stage on emitted a token there since the slot's last reset).  Waits for the stream."""
        out = np.empty(int(n), dtype=np.float32)
        check(self._lib.la_llama_logprobs_read(self._h, self._sp(), int(slot), int(first_pos), int(n), out.ctypes.data_as(_lib.pf32)),
              'logprobs_read')
        return out

    def set_top_logprobs(self, n):
        """The top-N list of the log-probability stage: n = 0 (the default) off, 1 .. 20 = for every token a step emits while
        set_logprobs(True), the n tokens with the largest raw logits (value descending, then id ascending) with their
        log-probabilities, kept in a position-indexed log per slot next to the scalar one; read it with top_logprobs().  The log is
        allocated by the first call with n > 0; switching n drops the captured graphs."""
        check(self._lib.la_llama_set_top_logprobs(self._h, self._sp(), int(n)), 'set_top_logprobs')
        self.top_logprobs_n = int(n)

    def top_logprobs(self, slot, first_pos, n_pos):
        """-> (ids int32 [n_pos][n], vals float32 [n_pos][n]): the top-N log of `slot` from position first_pos on (positions are
        indices in the unpadded sequence, as logprobs(); (-1, NaN): nothing emitted there)"""
        n = getattr(self, 'top_logprobs_n', 0)
        assert n > 0, 'top_logprobs: the stage is off (set_top_logprobs(n))'
        ids = np.empty((int(n_pos), n), dtype=np.int32)
        vals = np.empty((int(n_pos), n), dtype=np.float32)
        check(self._lib.la_llama_top_logprobs_read(self._h, self._sp(), int(slot), int(first_pos), int(n_pos),
                                                   ids.ctypes.data_as(_lib.pi32), vals.ctypes.data_as(_lib.pf32)), 'top_logprobs_read')
        return ids, vals

    def logprob_launches(self):
        """steps launched with the log-probability stage since the engine was created"""
        return int(self._lib.la_llama_logprob_launches(self._h))

    def penalty_context(self, slot=0):
        """uint32 [vocab / 32]: the context bitmap of `slot` (bit t of word t // 32 <=> token t is in the set)"""
        words = self.shape.vocab // 32
        return self._view(15, self.n_slots * words * 4, torch.int32).view(self.n_slots, words)[slot]

    # ---- cursor batch ------------------------------------------------------------------------------------
    def reset_slot(self, slot):
        check(self._lib.la_llama_reset_slot(self._h, self._sp(), int(slot)), 'reset_slot')
        if slot < 0:
            self.slot_keys = [0] * self.n_slots
            self._pen_ctx = {}
        else:
            self.slot_keys[slot] = 0
            self._pen_ctx.pop(slot, None)

    def bstep(self, segments, eager=False):
        """One verify block shared by several sequences.  segments: list of (slot, ids, local_rowmask, mode, limit);
        local_rowmask bit j of row i = tree row i sees tree row j OF THE SAME SEGMENT.  Rows are laid out segment after
        segment (sum of lengths <= 64).  -> {slot: list of emitted tokens}."""
        a = self._bin_np
        a[_lib.LA_BIN_SEQ:_lib.LA_BIN_SEQ + 64] = -1
        a[_lib.LA_BIN_MODE:_lib.LA_BIN_MODE + 16] = 0
        a[_lib.LA_BIN_LIMIT:_lib.LA_BIN_LIMIT + 16] = 16
        row = 0
        seen = set()
        self._bstep_first = {}
        for slot, ids, rowmask, mode, limit in segments:
            n = len(ids)
            assert 0 <= slot < self.n_slots and slot not in seen and n >= 1, 'one segment per slot'
            seen.add(slot)
            self._bstep_first[slot] = row
            assert row + n <= _lib.LA_TREE_MAX, 'a verify block holds 64 rows'
            assert self.slot_keys[slot] + n <= self._capacity(), 'KV cache capacity of the slot exceeded'
            a[_lib.LA_BIN_IDS + row:_lib.LA_BIN_IDS + row + n] = ids
            self._bin_rm[row:row + n] = np.asarray(rowmask, dtype=np.uint64) << np.uint64(row)
            a[_lib.LA_BIN_SEQ + row:_lib.LA_BIN_SEQ + row + n] = slot
            a[_lib.LA_BIN_MODE + slot] = mode
            a[_lib.LA_BIN_LIMIT + slot] = max(1, min(16, int(limit)))
            row += n
        a[_lib.LA_BIN_T] = row
        fn = self._lib.la_llama_bstep_eager if eager else self._lib.la_llama_bstep
        check(fn(self._h, self._sp(), self.host_bin.data_ptr(), self.host_bout.data_ptr()), 'llama_bstep')
        self.stream.synchronize()
        o = self._bout_np
        out = {}
        for slot in seen:
            n_out = int(o[_lib.LA_BST_NOUT + slot])
            self.slot_keys[slot] = int(o[_lib.LA_BST_NKEYS + slot])
            out[slot] = o[_lib.LA_BST_OUTTOK + 16 * slot:_lib.LA_BST_OUTTOK + 16 * slot + n_out].tolist()
        return out

    def bstep_rows(self):
        """{slot: first block row} of the last bstep (segments are laid out one after another)."""
        return dict(self._bstep_first)

    def bcommit(self, kept):
        """After a bstep whose segments ran in mode 2 (forward only): kept = {slot: [local tree rows to keep, root first]};
        their K/V move to the slot's cursor (la_llama_bcommit), cursors advance."""
        keep = np.full(64, -1, dtype=np.int32)
        for slot, rows in kept.items():
            base = self._bstep_first[slot]
            for k, r in enumerate(rows):
                keep[base + int(r)] = k
            assert self.slot_keys[slot] + len(rows) <= self._capacity(), 'KV cache capacity of the slot exceeded'
        check(self._lib.la_llama_bcommit(self._h, self._sp(), keep.ctypes.data_as(_lib.pi32), self.host_bout.data_ptr()), 'llama_bcommit')
        for slot in kept:
            self.slot_keys[slot] = int(self._bout_np[_lib.LA_BST_NKEYS + slot])

    def mcommit(self, kept):
        """After an mstep whose blocks ran in mode 2: kept = list (one entry per block, block order) of the tree rows to keep,
        root first (la_llama_mcommit)."""
        slots = self._mstep_slots
        assert len(kept) == len(slots)
        self._mcommit(enumerate(kept), len(kept), slots)

    def bprefill(self, slot, prompt_ids, eager=False):
        """Prompt of one slot as chains of <= 64 rows; -> first generated token."""
        prompt_ids = [int(x) for x in prompt_ids]
        tok = None
        for s in range(0, len(prompt_ids), 64):
            blk = prompt_ids[s:s + 64]
            if s + 64 >= len(prompt_ids):
                self._pen_seed_final(slot, prompt_ids)
            tok = self.bstep([(slot, np.asarray(blk, dtype=np.int32), self._CHAIN[:len(blk)], 1, 1)], eager=eager)[slot][0]
        return tok

    def bprefill_many(self, prompts, eager=False):
        """prompts: {slot: token list}.  The chains of all slots are packed greedily into shared 64-row blocks (a
        slot contributes one contiguous run per block and continues in the next).  -> {slot: first generated token}."""
        todo = {s: [int(x) for x in p] for s, p in prompts.items()}
        assert all(len(p) > 0 for p in todo.values())
        done, first = {s: 0 for s in todo}, {}
        order = sorted(todo)
        while any(done[s] < len(todo[s]) for s in order):
            segments, room = [], _lib.LA_TREE_MAX
            for s in order:
                left = len(todo[s]) - done[s]
                if left == 0 or room == 0:
                    continue
                n = min(left, room)
                segments.append((s, np.asarray(todo[s][done[s]:done[s] + n], dtype=np.int32), self._CHAIN[:n], 1, 1))
                done[s] += n
                room -= n
                if done[s] == len(todo[s]):
                    self._pen_seed_final(s, todo[s])
            out = self.bstep(segments, eager=eager)
            for s, _, _, _, _ in segments:
                if done[s] == len(todo[s]):
                    first[s] = out[s][0]
        return first

    # ---- multi-block step: every block is a full 64-row verify block of its own (la_llama_mstep) ---------------------
    # the host protocol, once: _put_block / _put_trees write LA_MIN_*, _mlaunch queues the pass, _mout_read decodes LA_MOUT_*, _mcommit keeps rows
    @staticmethod
    def _limit(limit):
        return max(1, min(_lib.LA_MOUT_TOKS, int(limit)))

    def _put_block(self, b, slot, ids, own, mode, lim, ancestors=()):
        """block b of the pass: its table entry, ids, the row-mask words over its own rows and (LA_MODE_TREE_PIECE) the ancestor words
        over the earlier blocks of its tree"""
        a, n = self._min_np, len(ids)
        a[_lib.LA_MIN_BLK + 4 * b:_lib.LA_MIN_BLK + 4 * b + 4] = (slot, n, mode, lim)
        a[_lib.LA_MIN_IDS + 64 * b:_lib.LA_MIN_IDS + 64 * b + n] = ids
        self._min_rm[64 * b:64 * b + n] = own
        for q, words in enumerate(ancestors):
            self._min_xm[64 * b:64 * b + n, q] = words

    @staticmethod
    def _tree(ids, rowmask):
        """-> (ids int32[T], row masks uint64[T][W], blocks of the tree)"""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        rm = np.asarray(rowmask, dtype=np.uint64)
        return ids, rm[:, None] if rm.ndim == 1 else rm, (len(ids) + 63) // 64

    def _put_trees(self, trees, b=0):
        """trees: (slot, ids int32[T], row masks uint64[T][W], mode, limit word), laid out from block b on: rows 64 p .. 64 p + 63 of a
        tree form its block p — block 0 in `mode`, the others as LA_MODE_TREE_PIECE; word p of a row's mask is its own-block word,
        the words q < p its ancestor words over the earlier blocks; a mask with fewer words stands for zeros.  Sets the block count
        of the pass.  -> [(first block, blocks)] per tree"""
        spans = []
        for slot, ids, rm, mode, lim in trees:
            T, W = rm.shape
            nb = (T + 63) // 64
            spans.append((b, nb))
            for p in range(nb):
                rows = slice(64 * p, min(T, 64 * p + 64))
                self._put_block(b, slot, ids[rows], rm[rows, p] if p < W else 0, mode if p == 0 else _lib.LA_MODE_TREE_PIECE, lim,
                                [rm[rows, q] if q < W else 0 for q in range(p)])
                b += 1
        self._min_np[_lib.LA_MIN_NBLK] = b
        return spans

    def _mlaunch(self, eager):
        fn = self._lib.la_llama_mstep_eager if eager else self._lib.la_llama_mstep
        check(fn(self._h, self._sp(), self.host_min.data_ptr(), self.host_mout.data_ptr()), 'llama_mstep')

    def _mout_keys(self, slots):
        """the cursors of the slots that took part in the pass (or the commit), from the result header"""
        for slot in slots:
            self.slot_keys[slot] = int(self._mout_np[_lib.LA_MOUT_NKEYS + slot])
        if 0 in slots:
            self.n_keys = self.slot_keys[0]

    def _mout_read(self, slots, blocks):
        """the result header of a finished pass: new cursors of `slots` -> the emitted tokens of each block in `blocks`"""
        self._mout_keys(slots)
        o = self._mout_np
        return [o[_lib.LA_MOUT_OUTTOK + _lib.LA_MOUT_TOKS * b:_lib.LA_MOUT_OUTTOK + _lib.LA_MOUT_TOKS * b + int(o[_lib.LA_MOUT_NOUT + b])].tolist()
                for b in blocks]

    def _mcommit(self, kept_at, n_blocks, slots):
        """kept_at: (first block of a tree, its rows to keep, root first) -> keep[64 * block + row] = place on the kept path, -1 = drop
        (la_llama_mcommit over the n_blocks blocks of the last pass), then the new cursors"""
        keep = np.full(64 * n_blocks, -1, dtype=np.int32)
        for b0, rows in kept_at:
            for k, r in enumerate(rows):
                keep[64 * b0 + int(r)] = k
        check(self._lib.la_llama_mcommit(self._h, self._sp(), n_blocks, keep.ctypes.data_as(_lib.pi32), self.host_mout.data_ptr()),
              'llama_mcommit')
        self._mout_keys(slots)

    def mstep(self, blocks, eager=False):
        """blocks: list of (slot, ids, rowmask, mode, limit) — one sequence's draft tree each (mode 0), or consecutive
        64-token pieces of one prompt (mode 1, same slot: a causal chain; every piece but the last holds 64 rows).
        All blocks run in ONE pass over the weights (M = 64 * len(blocks) rows).  -> list of emitted token lists.
        = mstep_async + mstep_finish."""
        self.mstep_async(blocks, eager=eager)
        return self.mstep_finish()

    def mstep_async(self, blocks, eager=False):
        """Queue the multi-block pass (input block H2D, captured graph, result header D2H) and return at once: the host is free —
        the previous step's trie update (LookaheadCache.stream_put_many), the accepted-token gather of an N-rank job
        (AcceptedTokenGather.finish_into_trie), bookkeeping — until mstep_finish()."""
        assert self.max_blocks and 1 <= len(blocks) <= self.max_blocks, 'engine was created with max_blocks < len(blocks)'
        self._min_np[_lib.LA_MIN_NBLK] = len(blocks)
        used, rows = {}, {}
        for b, (slot, ids, rowmask, mode, limit) in enumerate(blocks):
            n = len(ids)
            assert 0 <= slot < self.n_slots and 1 <= n <= 64
            prev = used.get(slot)
            assert prev is None or (mode == 1 and prev == (1, 64)), 'several blocks of one slot must form a prefill chain of full blocks'
            used[slot] = (mode, n)
            rows[slot] = rows.get(slot, 0) + n
            self._put_block(b, slot, ids, rowmask, mode, self._limit(limit))
        self._mstep_slots = [blk[0] for blk in blocks]
        for slot, n in rows.items():
            assert self.slot_keys[slot] + n <= self._capacity(), 'KV cache capacity of the slot exceeded'
        self._mlaunch(eager)
        self._mstep_pending = (len(blocks), list(rows))

    def mstep_finish(self):
        """Wait for the pass queued by mstep_async -> list of emitted token lists (block order)."""
        nb, slots = self._mstep_pending
        self._mstep_pending = None
        self.stream.synchronize()
        return self._mout_read(slots, range(nb))

    def mstep_trie(self, dev_trie, q0, slots, limits, last_tokens, put_idxs=None, put_branch_length=None):
        """One multi-block verify step whose drafts are the results of the LAST dev_trie.hier_get_dev(...) launch, taken on the
        device: block b = query q0 + b of that launch (ids / row masks / count stay in HBM; nothing but the result header crosses
        PCIe).  The trie kernels must have been queued on this engine's stream.  slots / limits / last_tokens: per block.
        put_idxs: the trie slot (batch index) of each block — the step's accepted tokens are then inserted into the DEVICE trie
        image by the device, straight from the step's output block (DeviceTrie.stream_put_dev, queued behind the step; the host
        waits for the result header only and must dev_trie.replay() the same tokens before its next trie update).
        -> (emitted token lists, draft lengths).  = mstep_trie_async + mstep_trie_finish."""
        self.mstep_trie_async(dev_trie, q0, slots, limits, last_tokens, put_idxs, put_branch_length)
        return self.mstep_trie_finish()

    def mstep_trie_async(self, dev_trie, q0, slots, limits, last_tokens, put_idxs=None, put_branch_length=None):
        """Queue the chained step (and the device-side trie update behind it) and return at once: the host is free — e.g. to
        replay the PREVIOUS step's trie update on its own trie (DeviceTrie.replay) — until mstep_trie_finish()."""
        nb = len(slots)
        assert self.max_blocks and 1 <= nb <= self.max_blocks
        assert getattr(dev_trie, 'rows', 64) == 64, 'the chained step reads 64-row result blocks (DeviceTrie(max_rows=64), decoding_length <= 64)'
        arr = lambda v: (C.c_int32 * nb)(*[int(x) for x in v])
        check(self._lib.la_llama_mstep_trie(self._h, self._sp(), nb, arr(slots), arr([self._limit(x) for x in limits]), arr(last_tokens),
                                      C.c_void_p(dev_trie.out_ids.data_ptr() + 4 * 64 * q0), C.c_void_p(dev_trie.out_rm.data_ptr() + 8 * 64 * q0),
                                      C.c_void_p(dev_trie.out_n.data_ptr() + 4 * q0), self.host_mout.data_ptr()), 'llama_mstep_trie')
        self._trie_wait = None
        if put_idxs is not None:
            ev = getattr(self, '_hdr_event', None)
            if ev is None:
                ev = self._hdr_event = torch.cuda.Event()
            ev.record(self.stream)                      # behind the D2H of the result header
            mo = getattr(self, '_mout_ptr', None)
            if mo is None:
                mo = self._mout_ptr = self.mout().data_ptr()
            with torch.cuda.stream(self.stream):
                dev_trie.stream_put_dev(mo + 4 * _lib.LA_MOUT_OUTTOK, _lib.LA_MOUT_TOKS, mo + 4 * _lib.LA_MOUT_NOUT, put_idxs,
                                        put_branch_length)
            self._trie_wait = ev
        self._trie_slots = list(slots)

    def mstep_trie_finish(self):
        """Wait for the result header of the step queued by mstep_trie_async -> (emitted token lists, draft lengths)."""
        if self._trie_wait is not None:
            self._trie_wait.synchronize()
        else:
            self.stream.synchronize()
        slots = self._mstep_slots = list(self._trie_slots)
        toks = self._mout_read(slots, range(len(slots)))
        return toks, [int(self._mout_np[_lib.LA_MOUT_T + b]) for b in range(len(slots))]

    # ---- wide trees: one sequence's tree of up to LA_TREE_WIDE_MAX rows as consecutive blocks of one multi-block pass -------
    def tstep(self, ids, rowmask, slot=0, mode=0, limit=None, eager=False):
        """One verify step of ONE sequence whose draft tree may be wider than a 64-row block (the reference grid-searches
        decoding_length up to 256 and publishes its best numbers at decoding_length=128, branch_length=32: README.md:100,
        benchmarks/benchmark.py:256-288).  ids int32[T], rowmask uint64[T] or uint64[T][W] (word w of row i = tree columns
        64 w ...; W >= the tree's blocks): rows 64 p .. 64 p + 63 form block p of the pass — block 0 in `mode` (0 verify / 2 forward
        only), the others as LA_MODE_TREE_PIECE with their ancestor words over the earlier blocks in LA_MIN_XMASK.  limit=None:
        LA_MOUT_TOKS.  -> (emitted tokens, keys kept)."""
        ids, rm, nb = self._tree(ids, rowmask)
        T = len(ids)
        assert 1 <= T <= _lib.LA_TREE_WIDE_MAX and nb <= min(self.max_blocks, 4), \
            f'a {T}-row tree needs an engine created with max_blocks >= {nb} (has {self.max_blocks}; at most 4 blocks per tree)'
        assert rm.shape[1] >= nb, f'a {T}-row tree needs {nb} mask words per row (got {rm.shape[1]})'
        assert 0 <= slot < self.n_slots and mode in (0, 2)
        assert self.slot_keys[slot] + T <= self._capacity(), 'KV cache capacity of the slot exceeded'
        self._put_trees([(slot, ids, rm, mode, self._limit(_lib.LA_MOUT_TOKS if limit is None else limit))])
        self._mstep_slots = [slot] * nb
        self._mlaunch(eager)
        self.stream.synchronize()
        before = self.slot_keys[slot]
        toks, = self._mout_read([slot], [0])
        return toks, self.slot_keys[slot] - before

    def mstep_trees(self, trees, eager=False):
        """Several sequences' draft trees in ONE pass, each tree of up to LA_TREE_WIDE_MAX rows (a batch whose per-sample budget
        exceeds a 64-row block: the reference's bat_get hands every sample (decoding_length // bs) // bs rows, any size,
        lookahead_cache.py:534-541).  trees: list of (slot, ids int32[T], rowmask uint64[T] or uint64[T][W], mode 0 / 2, limit):
        a tree occupies ceil(T / 64) consecutive blocks of the pass (block 0 in `mode`, the others LA_MODE_TREE_PIECE), one tree
        per slot, all blocks together <= max_blocks.  -> list of emitted token lists (tree order)."""
        laid, slots, b = [], [], 0
        for slot, ids, rowmask, mode, limit in trees:
            ids, rm, nb = self._tree(ids, rowmask)
            T = len(ids)
            assert 1 <= T <= _lib.LA_TREE_WIDE_MAX and nb <= 4, f'a tree holds 1..{_lib.LA_TREE_WIDE_MAX} rows (got {T})'
            assert 0 <= slot < self.n_slots and slot not in slots and mode in (0, 2), 'one tree per slot, mode 0 or 2'
            assert self.slot_keys[slot] + T <= self._capacity(), 'KV cache capacity of the slot exceeded'
            slots.append(slot)
            laid.append((slot, ids, rm, mode, self._limit(limit)))
            b += nb
        assert self.max_blocks and 1 <= b <= self.max_blocks, f'{b} blocks in one pass need an engine created with max_blocks >= {b}'
        spans = self._put_trees(laid)
        self._mstep_slots = [slot for slot, (_, nb) in zip(slots, spans) for _ in range(nb)]
        self._mlaunch(eager)
        self.stream.synchronize()
        return self._mout_read(slots, [b0 for b0, _ in spans])

    def mcommit_trees(self, kept, n_rows):
        """After mstep_trees(mode 2): kept[i] = the tree rows of tree i to keep (root first, path order), n_rows[i] = its row count
        — the host-walked sequential accept path for several (possibly wide) trees of one pass (la_llama_mcommit)."""
        nbs = [(int(n) + 63) // 64 for n in n_rows]
        firsts = [sum(nbs[:i]) for i in range(len(nbs))]
        self._mcommit(zip(firsts, kept), sum(nbs), set(self._mstep_slots))

    def tcommit(self, rows, n_rows):
        """After tstep(mode=2) over an n_rows-row tree: keep the tree rows `rows` (root first, path order) — the host-walked
        sequential accept path on a wide tree (la_llama_mcommit over the tree's blocks)."""
        self._mcommit([(0, rows)], (int(n_rows) + 63) // 64, self._mstep_slots[:1])

    def mprefill(self, slot, prompt_ids, eager=False):
        """Prompt of one slot in passes of up to max_blocks x 64 tokens (one pass over the weights each); -> first
        generated token.  Slot 0 hands its cursor to the single-sequence step as well (la_llama_set_nkeys)."""
        prompt_ids = [int(x) for x in prompt_ids]
        tok = None
        per = 64 * self.max_blocks
        for s in range(0, len(prompt_ids), per):
            piece = prompt_ids[s:s + per]
            blocks = [(slot, np.asarray(piece[i:i + 64], dtype=np.int32), self._CHAIN[:len(piece[i:i + 64])], 1, 1)
                      for i in range(0, len(piece), 64)]
            if s + per >= len(prompt_ids):
                self._pen_seed_final(slot, prompt_ids)
            tok = self.mstep(blocks, eager=eager)[-1][0]
        if slot == 0:
            check(self._lib.la_llama_set_nkeys(self._h, self._sp(), 0, self.slot_keys[0]), 'set_nkeys')
            self.n_keys = self.slot_keys[0]
        return tok

    def mprefill_many(self, prompts, eager=False):
        """prompts: {slot: token list}.  The 64-token pieces of all prompts are dealt, slot after slot, into passes of up to
        max_blocks blocks (one pass over the weights each); a slot whose prompt spans several passes continues from its
        committed keys.  -> {slot: first generated token}."""
        todo = {s: [int(x) for x in p] for s, p in prompts.items()}
        assert all(len(p) > 0 for p in todo.values())
        pieces = []                                   # (slot, piece, is_last)
        for s in sorted(todo):
            p = todo[s]
            for i in range(0, len(p), 64):
                pieces.append((s, p[i:i + 64], i + 64 >= len(p)))
        first = {}
        for i in range(0, len(pieces), self.max_blocks):
            group = pieces[i:i + self.max_blocks]
            for s, _, last in group:
                if last:
                    self._pen_seed_final(s, todo[s])
            out = self.mstep([(s, np.asarray(pc, dtype=np.int32), self._CHAIN[:len(pc)], 1, 1) for s, pc, _ in group], eager=eager)
            for (s, _, last), toks in zip(group, out):
                if last:
                    first[s] = toks[0]
        if 0 in todo:
            check(self._lib.la_llama_set_nkeys(self._h, self._sp(), 0, self.slot_keys[0]), 'set_nkeys')
            self.n_keys = self.slot_keys[0]
        return first

    def mlogits(self):
        """bf16 [max_blocks * 64][vocab] of the last multi-block step (row = 64 * block + tree row)."""
        return self._view(11, _lib.LA_MB_MAX * 64 * self.shape.vocab * 2, self.dtype).view(_lib.LA_MB_MAX * 64, self.shape.vocab)

    def mhidden(self):
        """[max_blocks * 64][hidden]: the residual stream of the last multi-block step after the last layer (row = 64 * block + tree
        row) — the multi-block twin of hidden()."""
        return self._view(13, _lib.LA_MB_MAX * 64 * self.shape.hidden * 2, self.dtype).view(_lib.LA_MB_MAX * 64, self.shape.hidden)

    def mout(self):
        return self._view(12, _lib.LA_MOUT_WORDS * 4, torch.int32)

    def bstate(self):
        return self._view(8, _lib.LA_BST_WORDS * 4, torch.int32)

    def _fill(self, ids, rowmask, mode):
        T = len(ids)
        assert 1 <= T <= _lib.LA_TREE_MAX
        assert self.n_keys + T <= self._capacity(), 'KV cache capacity exceeded'
        a = self._in_np
        a[_lib.LA_IN_T] = T
        a[_lib.LA_IN_MODE] = mode
        a[_lib.LA_IN_NKEYS_HINT] = self.n_keys               # host-side hint: which tree-attention form the step graph uses
        a[_lib.LA_IN_IDS:_lib.LA_IN_IDS + T] = ids
        self._in_rm[:T] = rowmask

    def step_async(self, ids, rowmask, mode=0, eager=False):
        """Enqueue one block (tree of T<=64 tokens) on the current stream; results land in host_out."""
        self._fill(ids, rowmask, mode)
        fn = self._lib.la_llama_step_eager if eager else self._lib.la_llama_step
        self._eager_pending = bool(eager)
        check(fn(self._h, self._sp(), self.host_in.data_ptr(), self.host_out.data_ptr()), 'llama_step')

    def step(self, ids, rowmask, mode=0, eager=False):
        """-> list of emitted tokens (accepted path + bonus), list of accepted tree rows."""
        self.step_async(ids, rowmask, mode, eager)
        return self.step_finish()

    def _wait(self):
        # captured step: the last kernel writes the result block into pinned host memory and bumps its sequence word, which
        # la_llama_wait polls (no D2H copy command, no sleep on the stream); eager steps use copies + a stream sync
        if getattr(self, '_eager_pending', False):
            self.stream.synchronize()
        else:
            check(self._lib.la_llama_wait(self._h, self._sp()), 'llama_wait')

    def step_finish(self):
        """Wait for the block enqueued by step_async and return its result (host work can run in between)."""
        self._wait()
        o = self._out_np
        n_out = int(o[_lib.LA_ST_NOUT])
        self.n_keys = int(o[_lib.LA_ST_NKEYS])
        return o[_lib.LA_ST_OUTTOK:_lib.LA_ST_OUTTOK + n_out].tolist(), int(o[_lib.LA_ST_NCOMMIT])

    def decode_native(self, cache, seq, max_length, eos_ids=(), decoding_length=64, branch_length=12, max_query_length=2,
                      mode=_lib.LA_MODE_MIX, idx=0, max_steps=1 << 30):
        """Run verify steps in the native loop (la_lookahead_decode: trie query -> captured graph -> trie update, no
        interpreter in between) until max_length / eos / max_steps.  `seq` = prompt + first generated token, already
        prefilled.  -> (new tokens, dls, edls, fts, qts, finished)."""
        p = _lib.DecodeParamsC()
        p.decoding_length, p.branch_length, p.max_query_length = int(decoding_length), int(branch_length), int(max_query_length)
        p.mode, p.idx, p.max_length = int(mode), int(idx), int(max_length)
        eos_ids = [int(e) for e in eos_ids if e is not None]
        if len(eos_ids) > 8:
            raise ValueError('decode_native: la_decode_params holds at most 8 eos ids (the interpreter loop has no such limit)')
        p.n_eos = len(eos_ids)
        for i, e in enumerate(eos_ids):
            p.eos[i] = e
        cap = max(1, min(int(max_steps), max(int(max_length) - len(seq), 0) + 1))
        p.max_steps = cap
        buf = np.zeros(max(int(max_length), len(seq)) + 32, dtype=np.int32)
        buf[:len(seq)] = seq
        n = C.c_int32(len(seq))
        dls = np.zeros(cap, dtype=np.int32)
        edls = np.zeros(cap, dtype=np.int32)
        fts = np.zeros(cap, dtype=np.float64)
        qts = np.zeros(cap, dtype=np.float64)
        steps, fin = C.c_int32(0), C.c_int32(0)
        dp = C.POINTER(C.c_double)
        check(self._lib.la_lookahead_decode(self._h, cache._h, self._sp(), C.byref(p), buf.ctypes.data_as(_lib.pi32), C.byref(n),
                                      self.host_in.data_ptr(), self.host_out.data_ptr(), dls.ctypes.data_as(_lib.pi32),
                                      edls.ctypes.data_as(_lib.pi32), C.byref(steps), C.byref(fin),
                                      fts.ctypes.data_as(dp), qts.ctypes.data_as(dp)), 'lookahead_decode')
        k = steps.value
        self.n_keys = int(self._out_np[_lib.LA_ST_NKEYS]) if k else self.n_keys
        return (buf[len(seq):n.value].tolist(), dls[:k].tolist(), edls[:k].tolist(), fts[:k].tolist(), qts[:k].tolist(),
                bool(fin.value))

    def verify_only(self, ids, rowmask, eager=False):
        """Forward of one block without the device accept walk (mode 2): logits() holds one row per tree token, nothing is
        committed until commit()."""
        self.step_async(ids, rowmask, mode=2, eager=eager)
        self._wait()

    def commit(self, rows):
        """Keep the K/V of tree rows `rows` (root first) of the last verify_only block."""
        arr = np.ascontiguousarray(rows, dtype=np.int32)
        assert self.n_keys + len(arr) <= self._capacity(), 'KV cache capacity exceeded'
        check(self._lib.la_llama_commit(self._h, self._sp(), arr.ctypes.data_as(_lib.pi32), len(arr), self.host_out.data_ptr()),
              'llama_commit')
        self.n_keys = int(self._out_np[_lib.LA_ST_NKEYS])

    _CHAIN = np.array([(2 << t) - 1 for t in range(63)] + [0xFFFFFFFFFFFFFFFF], dtype=np.uint64)

    def prefill(self, prompt_ids, eager=False, fast=None):
        """Process the prompt; returns the first generated token (argmax of the last prompt row,
        pretrained_model.py:783-798).  fast (default: engines created with max_blocks > 1, prompts of more than one block):
        chains of up to max_blocks x 64 tokens per pass over the weights (la_llama_mstep); otherwise 64-token steps, whose
        last block's logits stay readable through logits()."""
        prompt_ids = [int(x) for x in prompt_ids]
        if fast is None:
            fast = bool(self.max_blocks) and len(prompt_ids) > 64
        if fast:
            return self.mprefill(0, prompt_ids, eager=eager)
        tok = None
        for s in range(0, len(prompt_ids), 64):
            blk = prompt_ids[s:s + 64]
            if s + 64 >= len(prompt_ids):
                self._pen_seed_final(0, prompt_ids)
            toks, _ = self.step(np.asarray(blk, dtype=np.int32), self._CHAIN[:len(blk)], mode=1, eager=eager)
            tok = toks[0]
        return tok

    # ---- introspection for parity tests ----------------------------------------------------------------
    def _view(self, which, nbytes, dtype):
        ptr = self._lib.la_llama_buffer(self._h, which)
        off = ptr - self.workspace.data_ptr()
        return self.workspace[off:off + nbytes].view(dtype)

    def logits(self):
        """bf16 [64][vocab] of the last block (row t = tree token t)."""
        return self._view(0, 64 * self.shape.vocab * 2, self.dtype).view(64, self.shape.vocab)

    def state(self):
        return self._view(1, _lib.LA_ST_WORDS * 4, torch.int32)

    def hidden(self):
        return self._view(2, 64 * self.shape.hidden * 2, self.dtype).view(64, self.shape.hidden)

    def route_weights(self):
        """fp32 [n_layers][64][8]: routing weight of every (layer, block row, expert) of the last block (0 = not routed)."""
        L = self.shape.n_layers
        return self._view(9, L * 64 * _lib.LA_MOE_MAX_E * 4, torch.float32).view(L, 64, _lib.LA_MOE_MAX_E)

    def mroute_weights(self):
        """fp32 [n_layers][LA_MB_MAX * 64][8]: routing weights of the last multi-block step (row = 64 * block + block row)"""
        L = self.shape.n_layers
        return self._view(14, L * _lib.LA_MB_MAX * 64 * _lib.LA_MOE_MAX_E * 4, torch.float32).view(L, _lib.LA_MB_MAX * 64, _lib.LA_MOE_MAX_E)

    def profile_gateup(self, iters=5):
        """mean ms of one gate/up launch, every layer's launch back to back inside one HIP-event pair (la_llama_profile_gateup)"""
        ms = C.c_float(0)
        check(self._lib.la_llama_profile_gateup(self._h, self._sp(), int(iters), C.byref(ms)), 'profile_gateup')
        return float(ms.value)

    def profile(self, ids, rowmask, iters=3):
        """HIP-event timing per kernel class (see la_llama_profile)."""
        self._fill(ids, rowmask, 0)
        ms = (C.c_float * 8)()
        launches = (C.c_int32 * 7)()
        check(self._lib.la_llama_profile(self._h, self._sp(), self.host_in.data_ptr(), int(iters), ms, launches), 'profile')
        names = ['qkv', 'o', 'gateup', 'down', 'lm_head', 'attn', 'other']
        return {'ms': {n: ms[i] for i, n in enumerate(names)}, 'ms_step': ms[7],
                'launches': {n: launches[i] for i, n in enumerate(names)}}
