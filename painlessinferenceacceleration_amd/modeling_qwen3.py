# -*- coding: utf-8 -*-
"""Qwen3 (dense: 0.6B ... 32B) wrappers on the MI355X verify engine.  An extension: the reference has no Qwen3 model; the architecture is
transformers' models/qwen3/modeling_qwen3.py, the Qwen2 decoder with

* NO bias on q_proj / k_proj / v_proj, and instead q_norm / k_norm: an RMSNorm over the 128 features of every q and k head, applied to
  the rounded projection output before RoPE (Qwen3Attention.forward).  No QKV workgroup holds a whole head, so the norm is one device
  stage behind every QKV launch (la_qk_norm_rope, csrc/la_qknorm.hip): the QKV launch runs with identity RoPE tables, the stage
  normalises and applies the real ones;
* head_dim 128 whatever hidden / n_heads is (Qwen3-0.6B: 16 heads x 128 over hidden 1024);
* the cast-first RMSNorm everywhere (the q / k norms included), tied embeddings on the small models, rms_norm_eps 1e-6, rope_theta 1e6.

The lookahead hook is Llama's, so the trie, accept and commit code is shared.  Sliding window stays OFF, as for Qwen2.  A checkpoint
with attention_bias=True is refused (LlamaShape.from_hf), and so is a state dict whose q_norm / k_norm weights do not match the shape
(llama_engine.check_qk_norm): a Qwen3 checkpoint never runs as a Llama with its norms dropped.  Qwen3-MoE is another architecture.

BatchQwen3ForCausalLM is the same over modeling_llama_batch.LlamaForCausalLM (the multi-block step).
"""
from .llama_engine import LlamaShape
from .modeling_llama import LlamaForCausalLM
from .modeling_llama_batch import LlamaForCausalLM as _BatchLlamaForCausalLM


def _qwen3_shape(cls, cfg):
    kind = getattr(cfg, 'model_type', type(cfg).__name__)
    if kind != 'qwen3':
        raise ValueError(f'{cls.__name__}: the checkpoint is a {kind} model; only model_type "qwen3" (Qwen3 dense) loads here '
                         f'(Qwen3-MoE and Qwen2 are other architectures)')
    shape = LlamaShape.from_hf(cfg)
    assert shape.qk_norm and shape.norm_cast_first and not shape.qkv_bias
    return shape


class _Qwen3Family(object):
    _default_shape = staticmethod(LlamaShape.qwen3_8b)

    @classmethod
    def _shape_of(cls, cfg, kw):
        return _qwen3_shape(cls, cfg)

    @classmethod
    def random_init(cls, shape=None, **kw):
        shape = shape or cls._default_shape()
        if not shape.qk_norm:
            raise ValueError(f'{cls.__name__}.random_init: a Qwen3 shape has qk_norm=True (LlamaShape.qwen3_8b / qwen3_0_6b)')
        return super().random_init(shape, **kw)


class Qwen3ForCausalLM(_Qwen3Family, LlamaForCausalLM):
    pass


class BatchQwen3ForCausalLM(_Qwen3Family, _BatchLlamaForCausalLM):
    pass
