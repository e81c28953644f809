# -*- coding: utf-8 -*-
"""Qwen2 wrappers on the MI355X verify engine: the surface of lookahead/lookahead/models/qwen2/modeling_qwen2.py (a bs=1 driver in
the reference, the model of examples/qwen1.5_example.py).  Qwen1.5, Qwen2 and Qwen2.5 checkpoints share the architecture: the Llama
decoder with

* a bias on q_proj / k_proj / v_proj (modeling_qwen2.py:234-237), added in fp32 inside every QKV launch before the rounding and RoPE
  (la_gemm64_qkv_bias; o_proj and the MLP carry none, and the engine refuses a state dict that has one);
* the Mistral RMSNorm flavour (the normalised value is rounded to the activation dtype before the weight multiply, :82-96);
* tied embeddings on the small models (legacy_state_dict falls back to embed_tokens), rms_norm_eps 1e-6, rope_theta 1e6.

The lookahead hook is Llama's (position = sum of the mask row - 1, additive 4-D mask, :997-1000), so the trie, accept and commit code
is shared.  Sliding window stays OFF, as on the reference's lookahead path (the 4-D mask is passed in as is).

BatchQwen2ForCausalLM is the same over modeling_llama_batch.LlamaForCausalLM (the multi-block step): an extension, the reference has no
Qwen2 batch model.
"""
from .llama_engine import LlamaShape
from .modeling_llama import LlamaForCausalLM
from .modeling_llama_batch import LlamaForCausalLM as _BatchLlamaForCausalLM


def _qwen2_shape(cls, cfg):
    kind = getattr(cfg, 'model_type', type(cfg).__name__)
    if kind != 'qwen2':
        raise ValueError(f'{cls.__name__}: the checkpoint is a {kind} model; only model_type "qwen2" (Qwen1.5 / Qwen2 / Qwen2.5) loads '
                         f'here (Qwen2-MoE and Qwen v1 are other architectures)')
    shape = LlamaShape.from_hf(cfg)
    assert shape.qkv_bias and shape.norm_cast_first
    return shape


class _Qwen2Family(object):
    _default_shape = staticmethod(LlamaShape.qwen2_7b)

    @classmethod
    def _shape_of(cls, cfg, kw):
        return _qwen2_shape(cls, cfg)

    @classmethod
    def random_init(cls, shape=None, **kw):
        shape = shape or cls._default_shape()
        if not shape.qkv_bias:
            raise ValueError(f'{cls.__name__}.random_init: a Qwen2 shape has qkv_bias=True (LlamaShape.qwen2_7b / qwen2_0_5b)')
        return super().random_init(shape, **kw)


class Qwen2ForCausalLM(_Qwen2Family, LlamaForCausalLM):
    pass


class BatchQwen2ForCausalLM(_Qwen2Family, _BatchLlamaForCausalLM):
    pass
