# -*- coding: utf-8 -*-
"""Test oracle: the Qwen2 tree forward (lookahead/lookahead/models/qwen2/modeling_qwen2.py) on CPU, in the dtype of the weights.

Qwen2 is the Llama decoder with a bias on q_proj / k_proj / v_proj (:234-237, F.linear with a bias: one rounding of x W^T + b) and
the cast-first RMSNorm (:82-96, the Mistral flavour of oracle.llama_oracle._rms).  The lookahead hook is Llama's (position = sum of
the mask row - 1, additive mask, :997-1000), so `forward(ids, mask, past)` has the signature of oracle.llama_oracle.OracleLlama and
oracle.llama_oracle.lookahead_generate / greedy_generate drive it unchanged.  Sliding window: off, as on the reference's lookahead
path."""
import math

import torch

from oracle.llama_oracle import _rms, _rope_cos_sin, _rot_half


class OracleQwen2(object):
    """Functional Qwen2 over a HF-named state dict.  KV cache: list of (k, v), each [n_kv, C, hd]."""

    def __init__(self, shape, state_dict):
        self.s = shape
        self.w = state_dict
        self.dtype = state_dict['lm_head.weight'].dtype

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
            q = lin(x, w[p + 'self_attn.q_proj.weight'], w.get(p + 'self_attn.q_proj.bias')).view(1, T, nh, hd).transpose(1, 2)
            k = lin(x, w[p + 'self_attn.k_proj.weight'], w.get(p + 'self_attn.k_proj.bias')).view(1, T, nkv, hd).transpose(1, 2)
            v = lin(x, w[p + 'self_attn.v_proj.weight'], w.get(p + 'self_attn.v_proj.bias')).view(1, T, nkv, hd).transpose(1, 2)
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
