# -*- coding: utf-8 -*-
"""painlessinferenceacceleration_amd — MI355X-native LOOKAHEAD trie-draft / tree-verify decoding.

Drop-in surface (reference: alipay/PainlessInferenceAcceleration, lookahead/):
    LookaheadCache                         lookahead/common/lookahead_cache.py
    LookaheadPreTrainedModel.lookahead_generation   lookahead/common/pretrained_model.py
    LlamaForCausalLM                       lookahead/models/llama/modeling_llama.py
    modeling_llama_batch.LlamaForCausalLM  lookahead/models/llama/modeling_llama_batch.py (bs>1, cursor batch)
    Qwen2ForCausalLM                       lookahead/models/qwen2/modeling_qwen2.py (Qwen1.5 / Qwen2 / Qwen2.5; BatchQwen2ForCausalLM: bs>1)
    Qwen3ForCausalLM                       Qwen3 dense (transformers models/qwen3/modeling_qwen3.py; BatchQwen3ForCausalLM: bs>1): an
                                           extension, the reference has no Qwen3 model
All compute lives in liblookahead_hip.so (csrc/, hand-written gfx950 HIP + the native trie).
"""
from ._lib import LIB_PATH, LookaheadHipError  # noqa: F401  (raises at import if the library is not built)
from .lookahead_cache import LookaheadCache  # noqa: F401
from .lookahead_generation_utils import (GenerationMode, LookaheadDecoderOnlyOutput,  # noqa: F401
                                         LookaheadGenerationConfig)

__all__ = ['LookaheadCache', 'GenerationMode', 'LookaheadDecoderOnlyOutput', 'LookaheadGenerationConfig',
           'LookaheadHipError', 'LIB_PATH']


def __getattr__(name):          # torch-dependent pieces are imported lazily
    if name in ('LlamaForCausalLM',):
        from .modeling_llama import LlamaForCausalLM
        return LlamaForCausalLM
    if name in ('BatchLlamaForCausalLM',):
        from .modeling_llama_batch import LlamaForCausalLM
        return LlamaForCausalLM
    if name in ('Qwen2ForCausalLM', 'BatchQwen2ForCausalLM'):
        from . import modeling_qwen2
        return getattr(modeling_qwen2, name)
    if name in ('Qwen3ForCausalLM', 'BatchQwen3ForCausalLM'):
        from . import modeling_qwen3
        return getattr(modeling_qwen3, name)
    if name in ('LookaheadPreTrainedModel',):
        from .pretrained_model import LookaheadPreTrainedModel
        return LookaheadPreTrainedModel
    if name in ('LlamaVerifyEngine', 'LlamaShape'):
        from . import llama_engine
        return getattr(llama_engine, name)
    raise AttributeError(name)
