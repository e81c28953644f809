# -*- coding: utf-8 -*-
"""CPU (not gpu): the Qwen3 family on the host side — config mapping and the family check, the Qwen3 oracle (tests/qwen3_oracle.py)
against the transformers eager forward in fp32, its relation to the Qwen2 oracle, its lookahead loop, the refusal of q/k norm weights
that do not match the shape (in both directions), and the C surface of the new stage ."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import llama_oracle as lo
from painlessinferenceacceleration_amd import _lib
from painlessinferenceacceleration_amd.llama_engine import LlamaShape, LlamaVerifyEngine, legacy_state_dict, random_weights
from tests.qwen2_oracle import OracleQwen2
from tests.qwen3_oracle import OracleQwen3


def _qwen3(n_kv=2, tied=False, seed=11, **extra):
    import transformers
    torch.manual_seed(seed)
    kw = dict(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
              num_key_value_heads=n_kv, head_dim=128, rms_norm_eps=1e-6, max_position_embeddings=1024, rope_theta=1e6, pad_token_id=0,
              bos_token_id=1, eos_token_id=2, tie_word_embeddings=tied, attn_implementation='eager')
    kw.update(extra)
    cfg = transformers.Qwen3Config(**kw)
    m = transformers.Qwen3ForCausalLM(cfg).eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.dim() >= 2:
                p.mul_(4.0)
            elif n.endswith('q_norm.weight') or n.endswith('k_norm.weight'):       # redrawn away from 1
                p.copy_(0.2 + 2.0 * torch.rand_like(p))
    return m


def _fp32_sd(m, shape):
    return {k: v.float() for k, v in legacy_state_dict(m.state_dict(), shape).items()}


def test_config_mapping():
    import transformers
    cfg = transformers.Qwen3Config(vocab_size=151936, hidden_size=4096, intermediate_size=12288, num_hidden_layers=36,
                                   num_attention_heads=32, num_key_value_heads=8, head_dim=128, rms_norm_eps=1e-6, rope_theta=1e6,
                                   tie_word_embeddings=False)
    s = LlamaShape.from_hf(cfg)
    assert s.qk_norm and s.norm_cast_first and not s.qkv_bias and s.rms_eps == 1e-6 and s.rope_theta == 1e6
    ref = LlamaShape.qwen3_8b()
    assert (ref.n_layers, ref.hidden, ref.n_heads, ref.n_kv_heads, ref.head_dim, ref.ffn, ref.vocab) == (36, 4096, 32, 8, 128, 12288, 151936)
    assert vars(s) == vars(ref)
    small = LlamaShape.qwen3_0_6b()
    assert (small.n_layers, small.hidden, small.n_heads, small.n_kv_heads, small.head_dim, small.ffn, small.vocab) == \
        (28, 1024, 16, 8, 128, 3072, 151936)
    assert small.qk_norm and small.n_heads * small.head_dim != small.hidden
    cfg06 = transformers.Qwen3Config(vocab_size=151936, hidden_size=1024, intermediate_size=3072, num_hidden_layers=28,
                                     num_attention_heads=16, num_key_value_heads=8, head_dim=128, rms_norm_eps=1e-6, rope_theta=1e6,
                                     tie_word_embeddings=True)
    assert vars(LlamaShape.from_hf(cfg06)) == vars(small)
    # tied head -> legacy_state_dict takes lm_head from the embedding
    m = _qwen3(tied=True)
    sd = legacy_state_dict(m.state_dict(), LlamaShape.from_hf(m.config))
    assert torch.equal(sd['lm_head.weight'], sd['model.embed_tokens.weight'])
    # the norms enter the parameter count: 2 * 128 per layer
    plain = LlamaShape.qwen3_8b()
    plain.qk_norm = False
    assert ref.n_params_no_embed() - plain.n_params_no_embed() == 36 * 256
    # attention_bias=True: the o_proj bias has no consumer
    with pytest.raises(ValueError, match='attention_bias'):
        LlamaShape.from_hf(transformers.Qwen3Config(attention_bias=True))
    # other families are unchanged
    assert not LlamaShape.from_hf(transformers.LlamaConfig()).qk_norm
    assert not LlamaShape.from_hf(transformers.Qwen2Config()).qk_norm and LlamaShape.from_hf(transformers.Qwen2Config()).qkv_bias
    assert not LlamaShape().qk_norm and not LlamaShape.qwen2_7b().qk_norm


def test_family_check_of_the_wrappers():
    import transformers
    from painlessinferenceacceleration_amd import BatchQwen3ForCausalLM, Qwen2ForCausalLM, Qwen3ForCausalLM
    for cls in (Qwen3ForCausalLM, BatchQwen3ForCausalLM):
        assert cls._shape_of(_qwen3().config, {}).qk_norm
        with pytest.raises(ValueError, match='qwen3'):
            cls._shape_of(transformers.LlamaConfig(), {})
        with pytest.raises(ValueError, match='qwen3_moe'):
            cls._shape_of(transformers.Qwen3MoeConfig(), {})
        with pytest.raises(ValueError, match='qwen2'):
            cls._shape_of(transformers.Qwen2Config(), {})
        with pytest.raises(ValueError, match='attention_bias'):
            cls._shape_of(transformers.Qwen3Config(attention_bias=True), {})
        with pytest.raises(NotImplementedError, match='rope_scaling'):
            cls._shape_of(transformers.Qwen3Config(rope_scaling={'rope_type': 'yarn', 'factor': 4.0, 'rope_theta': 1e6}), {})
        with pytest.raises(ValueError, match='qk_norm'):
            cls.random_init(LlamaShape.qwen2_7b())
    with pytest.raises(ValueError, match='qwen3'):
        Qwen2ForCausalLM._shape_of(_qwen3().config, {})


@pytest.mark.parametrize('n_kv', [2, 4])
def test_oracle_matches_transformers_fp32(n_kv):
    m = _qwen3(n_kv=n_kv, tied=n_kv == 4)
    shape = LlamaShape.from_hf(m.config)
    orc = OracleQwen3(shape, _fp32_sd(m, shape))
    ids = torch.from_numpy(np.random.RandomState(3).randint(3, 512, size=40)).long()
    mask = torch.tril(torch.ones((40, 40), dtype=torch.long))
    m32 = m.float()
    with torch.no_grad():
        ref = m32(ids[None]).logits[0]
    got, _ = orc.forward(ids, mask, None)
    err = float((got - ref).abs().max() / ref.abs().max())
    assert err <= 1e-5, err
    # the norms are visible: without them the logits move far beyond that
    lg0, _ = OracleQwen3(shape, orc.w, qk_norm=False).forward(ids, mask, None)
    assert float((lg0 - ref).abs().max() / ref.abs().max()) > 1e-2


def test_oracle_without_the_norms_is_qwen2_and_unit_weights_are_not():
    """The norm with all weights 1 still normalises: only SKIPPING it gives the bias-free Qwen2 forward (bitwise)."""
    m = _qwen3()
    shape = LlamaShape.from_hf(m.config)
    sd = {k: v.to(torch.bfloat16) for k, v in legacy_state_dict(m.state_dict(), shape).items()}
    ones = {k: (torch.ones_like(v) if re.search(r'[qk]_norm\.weight$', k) else v) for k, v in sd.items()}
    ids = torch.from_numpy(np.random.RandomState(5).randint(3, 512, size=24)).long()
    mask = torch.tril(torch.ones((24, 24), dtype=torch.long))
    q2, _ = OracleQwen2(shape, sd).forward(ids, mask, None)
    skipped, _ = OracleQwen3(shape, sd, qk_norm=False).forward(ids, mask, None)
    assert torch.equal(skipped, q2)
    unit, _ = OracleQwen3(shape, ones).forward(ids, mask, None)
    assert float((unit.float() - q2.float()).abs().max() / q2.float().abs().max()) > 1e-2


def test_oracle_lookahead_loop_gives_hf_greedy_tokens():
    from painlessinferenceacceleration_amd.lookahead_cache import LookaheadCache
    m = _qwen3().float()
    shape = LlamaShape.from_hf(m.config)
    orc = OracleQwen3(shape, _fp32_sd(m, shape))
    rs = np.random.RandomState(9)
    prompt = rs.randint(3, 512, size=20).tolist()
    n_new = 24
    seq = list(prompt)
    with torch.no_grad():
        for _ in range(n_new):
            seq.append(int(m(torch.tensor([seq])).logits[0, -1].argmax()))
    cache = LookaheadCache(eos_ids=[None])
    cache.put(seq[len(prompt) - 1:], branch_length=13, mode='output', idx=-1)
    out = lo.lookahead_generate(orc, cache, prompt, max_length=len(prompt) + n_new, eos_token_id=None)
    assert out['sequences'][:len(seq)] == seq
    assert sum(out['edls']) == len(out['sequences']) - len(prompt)
    assert max(out['edls']) > 1, 'the drafts were never accepted: the loop did not exercise tree verification'


def test_norm_weights_and_shape_must_agree():
    """Both refusals come before any GPU is needed."""
    from painlessinferenceacceleration_amd.modeling_llama import LlamaForCausalLM
    m = _qwen3()
    shape = LlamaShape.from_hf(m.config)
    sd = legacy_state_dict(m.state_dict(), shape)
    # a Qwen3 state dict under a shape without the stage (the silent-Llama hole): refused
    plain = LlamaShape.from_hf(m.config)
    plain.qk_norm = False
    with pytest.raises(ValueError, match=r'q_norm\.weight.*refusing to drop it'):
        LlamaVerifyEngine(plain, dict(sd))
    with pytest.raises(ValueError, match=r'q_norm\.weight.*refusing to drop it'):
        LlamaForCausalLM(plain, dict(sd), device='cpu')
    # the reverse: a shape with the stage, a state dict without one of the weights
    sd2 = dict(sd)
    del sd2['model.layers.1.self_attn.k_norm.weight']
    with pytest.raises(ValueError, match=r'no model\.layers\.1\.self_attn\.k_norm\.weight'):
        LlamaVerifyEngine(shape, sd2)
    qshape = LlamaShape(2, 256, 4, 2, 512, 512, 1e-6, head_dim=128, norm_cast_first=True, qk_norm=True)
    with pytest.raises(ValueError, match='shape.qk_norm is set'):
        LlamaVerifyEngine(qshape, random_weights(LlamaShape(2, 256, 4, 2, 512, 512, 1e-6, head_dim=128)))
    # combinations the stage does not serve are refused, never served without the norm
    with pytest.raises(ValueError, match='head_dim'):
        LlamaVerifyEngine(LlamaShape(2, 256, 4, 2, 512, 512, 1e-6, head_dim=64, qk_norm=True), {})
    with pytest.raises(ValueError, match='fuse'):
        LlamaVerifyEngine(shape, dict(sd), fuse=2)
    # random_weights draws the norms away from 1 for a qk_norm shape, and only then
    rw = random_weights(qshape, seed=1)
    qn = rw['model.layers.0.self_attn.q_norm.weight'].float()
    assert qn.shape == (128,) and float(qn.min()) >= 0.19 and float(qn.max()) <= 2.21 and float((qn - 1).abs().mean()) > 0.3
    assert not any('_norm.weight' in k and 'self_attn' in k for k in random_weights(LlamaShape(1, 256, 2, 2, 512, 512)))


def test_abi_declares_exports_and_binds_the_stage():
    assert _lib.lib.la_abi_version() == _lib.ABI_VERSION
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), 'include', 'lookahead_hip.h')).read()
    for name, nargs in (('la_qk_norm_rope', 12), ('la_llama_create_qk_norm', 5)):
        assert re.search(r'\b' + name + r'\s*\(', hdr), name
        assert name in _lib.PROTOTYPES and len(getattr(_lib.lib, name).argtypes) == nargs, name
    body = re.search(r'typedef struct la_qk_norm_weights \{(.*?)\} la_qk_norm_weights;', hdr, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    assert re.findall(r'(\w+);', body) == [f[0] for f in _lib.QkNormWeightsC._fields_] == ['q_norm', 'k_norm', 'rope_cos_id', 'rope_sin_id']
    # the stage came WITHOUT a change to the structs every caller of la_llama_create fills: their last fields are the earlier ones
    assert _lib.LlamaConfigC._fields_[-1][0] == 'weight_format' and _lib.LlamaLayerWeightsC._fields_[-1][0] == 'wdown_scale'
    assert _lib.LlamaWeightsC._fields_[-1][0] == 'layers'
    for struct, last in (('la_llama_config', 'weight_format'), ('la_llama_layer_weights', 'wdown_scale'), ('la_llama_weights', 'layers')):
        text = re.search(r'typedef struct ' + struct + r' \{(.*?)\} ' + struct + ';', hdr, re.S).group(1)
        assert re.findall(r'(\w+);', re.sub(r'/\*.*?\*/', '', text, flags=re.S))[-1] == last, struct
    # without a device both create entry points fail loudly; argument checks of the stage's own entry point need no device either
    assert _lib.lib.la_qk_norm_rope(None, None, None, 1, 2, 2, None, None, 1e-6, None, None, None) == -1
    import ctypes as C
    cfg = _lib.LlamaConfigC()
    assert not _lib.lib.la_llama_create_qk_norm(C.byref(cfg), None, None, None, 0)
