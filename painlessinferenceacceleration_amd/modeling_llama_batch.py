# -*- coding: utf-8 -*-
"""Batch LlamaForCausalLM on the MI355X verify engine: the wrapper surface of
lookahead/lookahead/models/llama/modeling_llama_batch.py (generate / lookahead_generation over [bs, P] prompts with
per-sample cursors) with the forward living in liblookahead_hip.so (la_llama_bstep)."""
from .llama_engine import LlamaVerifyEngine
from .modeling_llama import _LlamaWrapper
from .pretrained_model_batch import LookaheadPreTrainedModel


class LlamaForCausalLM(_LlamaWrapper, LookaheadPreTrainedModel):
    def __init__(self, shape, state_dict, max_length=2048, max_batch=8, device='cuda:0', eos_token_id=2, pad_token_id=0,
                 attn_split=0, gemm_cfg=None, consume_state_dict=False, balanced=True, max_blocks=None, kv_ring=False, dtype=None,
                 weight_format=None):
        if weight_format is not None:
            # the batch path runs the multi-block step, which has no fp8 launch (the single-sequence LlamaForCausalLM has)
            raise ValueError(f'weight_format={weight_format!r}: the batch models run the multi-block step, which has 16-bit weights only; '
                             'fp8 weights run on the single-sequence models (modeling_llama.LlamaForCausalLM, Qwen2ForCausalLM)')
        self.engine = LlamaVerifyEngine(shape, state_dict, max_length=max_length, device=device, attn_split=attn_split,
                                        gemm_cfg=gemm_cfg, consume_state_dict=consume_state_dict, balanced=balanced,
                                        n_slots=max_batch,
                                        max_blocks=min(max_batch, 8) if max_blocks is None else max_blocks, kv_ring=kv_ring, dtype=dtype)
        self._finish_init(shape, device, eos_token_id, pad_token_id)
