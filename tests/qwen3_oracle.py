# -*- coding: utf-8 -*-
"""Test oracle: the Qwen3 (dense) tree forward on CPU, in the dtype of the weights — transformers' models/qwen3/modeling_qwen3.py.

Qwen3 is tests/qwen2_oracle.py's decoder without the q/k/v bias and with q_norm / k_norm: the cast-first RMSNorm (oracle.llama_oracle._rms
with cast_first) over the head_dim features of every q and k head, on the [1, T, heads, head_dim] views of the rounded projection output,
BEFORE the transpose and RoPE (Qwen3Attention.forward).  `qk_norm=False` skips the two norms (the sensitivity controls); the signature is
OracleLlama's, so oracle.llama_oracle.lookahead_generate / greedy_generate drive it unchanged.  Sliding window: off."""
import math

import torch

from oracle.llama_oracle import _rms, _rope_cos_sin, _rot_half


class OracleQwen3(object):
    """Functional Qwen3 over a HF-named state dict.  KV cache: list of (k, v), each [n_kv, C, hd]."""

    def __init__(self, shape, state_dict, qk_norm=True):
        self.s = shape
        self.w = state_dict
        self.dtype = state_dict['lm_head.weight'].dtype
        self.qk_norm = qk_norm

    @torch.no_grad()
    def forward(self, ids, mask, past):
        """ids: LongTensor [T]; mask: 0/1 LongTensor [T, C+T]; past: None or list of (k, v).  -> logits [T, V], new past."""
        s, w, dt = self.s, self.w, self.dtype
        T, hd, nh, nkv = ids.shape[0], s.head_dim, s.n_heads, s.n_kv_heads
        lin = torch.nn.functional.linear
        h = w['model.embed_tokens.weight'][ids][None]
        mask4 = mask[None, None]
        pos = torch.sum(mask4, dim=-1).squeeze(1) - 1
        bias = (1.0 - mask4.to(dt)) * torch.finfo(dt).min
        cos, sin = _rope_cos_sin(pos[0], hd, s.rope_theta, dt)
        cos, sin = cos[None, None], sin[None, None]
        new_past = []
        for i in range(s.n_layers):
            p = f'model.layers.{i}.'
            x = _rms(h, w[p + 'input_layernorm.weight'], s.rms_eps, True)
            q = lin(x, w[p + 'self_attn.q_proj.weight']).view(1, T, nh, hd)
            k = lin(x, w[p + 'self_attn.k_proj.weight']).view(1, T, nkv, hd)
            if self.qk_norm:
                q = _rms(q, w[p + 'self_attn.q_norm.weight'], s.rms_eps, True)
                k = _rms(k, w[p + 'self_attn.k_norm.weight'], s.rms_eps, True)
            q, k = q.transpose(1, 2), k.transpose(1, 2)
            v = lin(x, w[p + 'self_attn.v_proj.weight']).view(1, T, nkv, hd).transpose(1, 2)
            q = (q * cos) + (_rot_half(q) * sin)
            k = (k * cos) + (_rot_half(k) * sin)
            if past is not None:
                k = torch.cat([past[i][0][None], k], dim=2)
                v = torch.cat([past[i][1][None], v], dim=2)
            new_past.append((k[0], v[0]))
            kk, vv = k, v
            if nkv != nh:
                rep = nh // nkv
                kk = k[:, :, None].expand(1, nkv, rep, k.shape[2], hd).reshape(1, nh, -1, hd)
                vv = v[:, :, None].expand(1, nkv, rep, v.shape[2], hd).reshape(1, nh, -1, hd)
            att = torch.matmul(q, kk.transpose(2, 3)) / math.sqrt(hd)
            att = att + bias
            att = torch.max(att, torch.tensor(torch.finfo(att.dtype).min))
            att = torch.softmax(att, dim=-1, dtype=torch.float32).to(dt)
            o = torch.matmul(att, vv).transpose(1, 2).reshape(1, T, nh * hd)
            h = h + lin(o, w[p + 'self_attn.o_proj.weight'])
            x = _rms(h, w[p + 'post_attention_layernorm.weight'], s.rms_eps, True)
            g = torch.nn.functional.silu(lin(x, w[p + 'mlp.gate_proj.weight']))
            u = lin(x, w[p + 'mlp.up_proj.weight'])
            h = h + lin(g * u, w[p + 'mlp.down_proj.weight'])
        h = _rms(h, w['model.norm.weight'], s.rms_eps, True)
        return lin(h, w['lm_head.weight'])[0], new_past
