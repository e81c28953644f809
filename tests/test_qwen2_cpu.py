# -*- coding: utf-8 -*-
"""CPU (not gpu): the Qwen2 family on the host side — config mapping, the Qwen2 oracle (tests/qwen2_oracle.py) against the
transformers eager forward in fp32, its relation to the Llama oracle, its lookahead loop, and the refusal of biases the engine
cannot apply."""
import numpy as np
import pytest
import torch

from oracle import llama_oracle as lo
from painlessinferenceacceleration_amd.llama_engine import LlamaShape, LlamaVerifyEngine, legacy_state_dict
from tests.qwen2_oracle import OracleQwen2


def _qwen2(n_kv=1, head_dim=None, tied=False, seed=11):
    import transformers
    torch.manual_seed(seed)
    kw = dict(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
              num_key_value_heads=n_kv, rms_norm_eps=1e-6, max_position_embeddings=1024, rope_theta=1e6, pad_token_id=0,
              bos_token_id=1, eos_token_id=2, tie_word_embeddings=tied, attn_implementation='eager')
    if head_dim:
        kw['head_dim'] = head_dim
    cfg = transformers.Qwen2Config(**kw)
    m = transformers.Qwen2ForCausalLM(cfg).eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.dim() >= 2:
                p.mul_(4.0)
            elif n.endswith('.bias'):          # trained-Qwen2-like biases: small, with a few large K entries
                p.copy_(torch.randn_like(p) * 0.1)
                if 'k_proj' in n:
                    p[::7] = torch.randn_like(p[::7]) * 4.0
    return m


def _fp32_sd(m, shape):
    return {k: v.float() for k, v in legacy_state_dict(m.state_dict(), shape).items()}


def test_config_mapping():
    import transformers
    cfg = transformers.Qwen2Config(vocab_size=152064, hidden_size=3584, intermediate_size=18944, num_hidden_layers=28,
                                   num_attention_heads=28, num_key_value_heads=4, rms_norm_eps=1e-6, rope_theta=1e6,
                                   tie_word_embeddings=False)
    s = LlamaShape.from_hf(cfg)
    assert s.qkv_bias and s.norm_cast_first and s.rms_eps == 1e-6 and s.rope_theta == 1e6
    assert (s.n_layers, s.hidden, s.n_heads, s.n_kv_heads, s.head_dim, s.ffn, s.vocab) == (28, 3584, 28, 4, 128, 18944, 152064)
    ref = LlamaShape.qwen2_7b()
    assert vars(s) == vars(ref)
    # 0.5B: head_dim 64, tied head -> legacy_state_dict takes lm_head from the embedding
    small = LlamaShape.qwen2_0_5b()
    assert (small.hidden, small.n_heads, small.n_kv_heads, small.head_dim, small.vocab) == (896, 14, 2, 64, 151936)
    m = _qwen2(tied=True)
    sd = legacy_state_dict(m.state_dict(), LlamaShape.from_hf(m.config))
    assert torch.equal(sd['lm_head.weight'], sd['model.embed_tokens.weight'])
    # the bias enters the parameter count: q/k/v bias = (nh + 2 nkv) * hd per layer
    plain = LlamaShape.qwen2_7b()
    plain.qkv_bias = False
    assert ref.n_params_no_embed() - plain.n_params_no_embed() == 28 * (28 + 8) * 128
    # other families are unchanged
    assert not LlamaShape.from_hf(transformers.LlamaConfig()).qkv_bias
    assert not LlamaShape.from_hf(transformers.MistralConfig()).qkv_bias


def test_family_check_of_the_wrappers():
    import transformers
    from painlessinferenceacceleration_amd import BatchQwen2ForCausalLM, Qwen2ForCausalLM
    for cls in (Qwen2ForCausalLM, BatchQwen2ForCausalLM):
        assert cls._shape_of(_qwen2().config, {}).qkv_bias
        with pytest.raises(ValueError, match='qwen2'):
            cls._shape_of(transformers.LlamaConfig(), {})
        with pytest.raises(ValueError, match='qwen2_moe'):
            cls._shape_of(transformers.Qwen2MoeConfig(), {})


@pytest.mark.parametrize('n_kv,head_dim', [(1, None), (2, 64)])
def test_oracle_matches_transformers_fp32(n_kv, head_dim):
    m = _qwen2(n_kv=n_kv, head_dim=head_dim, tied=head_dim is not None)
    shape = LlamaShape.from_hf(m.config)
    orc = OracleQwen2(shape, _fp32_sd(m, shape.__class__.from_hf(m.config)))
    ids = torch.from_numpy(np.random.RandomState(3).randint(3, 512, size=40)).long()
    m32 = m.float()
    with torch.no_grad():
        ref = m32(ids[None]).logits[0]
    got, _ = orc.forward(ids, torch.tril(torch.ones((40, 40), dtype=torch.long)), None)
    err = float((got - ref).abs().max() / ref.abs().max())
    assert err <= 1e-5, err
    # the bias is visible: without it the logits move far beyond that
    sd0 = {k: (torch.zeros_like(v) if k.endswith('.bias') else v) for k, v in orc.w.items()}
    lg0, _ = OracleQwen2(shape, sd0).forward(ids, torch.tril(torch.ones((40, 40), dtype=torch.long)), None)
    assert float((lg0 - ref).abs().max() / ref.abs().max()) > 1e-2


def test_zero_bias_oracle_is_the_cast_first_llama_oracle_bitwise():
    m = _qwen2()
    shape = LlamaShape.from_hf(m.config)
    sd = {k: (torch.zeros_like(v) if k.endswith('.bias') else v) for k, v in legacy_state_dict(m.state_dict(), shape).items()}
    sd = {k: v.to(torch.bfloat16) for k, v in sd.items()}
    lshape = LlamaShape.from_hf(m.config)
    lshape.qkv_bias = False
    assert lshape.norm_cast_first
    ids = torch.from_numpy(np.random.RandomState(5).randint(3, 512, size=24)).long()
    mask = torch.tril(torch.ones((24, 24), dtype=torch.long))
    a, pa = OracleQwen2(shape, sd).forward(ids, mask, None)
    b, pb = lo.OracleLlama(lshape, {k: v for k, v in sd.items() if not k.endswith('.bias')}).forward(ids, mask, None)
    assert torch.equal(a, b)
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(pa, pb))


def test_oracle_lookahead_loop_gives_hf_greedy_tokens():
    from painlessinferenceacceleration_amd.lookahead_cache import LookaheadCache
    m = _qwen2(n_kv=1).float()
    shape = LlamaShape.from_hf(m.config)
    orc = OracleQwen2(shape, _fp32_sd(m, shape))
    rs = np.random.RandomState(9)
    prompt = rs.randint(3, 512, size=20).tolist()
    n_new = 24
    seq = list(prompt)
    with torch.no_grad():
        for _ in range(n_new):
            seq.append(int(m(torch.tensor([seq])).logits[0, -1].argmax()))
    # warm the trie with the greedy continuation so that the verify steps carry multi-token drafts
    cache = LookaheadCache(eos_ids=[None])
    cache.put(seq[len(prompt) - 1:], branch_length=13, mode='output', idx=-1)
    out = lo.lookahead_generate(orc, cache, prompt, max_length=len(prompt) + n_new, eos_token_id=None)
    assert out['sequences'][:len(seq)] == seq
    assert sum(out['edls']) == len(out['sequences']) - len(prompt)
    assert max(out['edls']) > 1, 'the drafts were never accepted: the loop did not exercise tree verification'


def test_unsupported_biases_are_refused():
    import transformers
    from painlessinferenceacceleration_amd.modeling_llama import LlamaForCausalLM
    # Llama with attention_bias=True: o_proj carries a bias the engine has no kernel for
    cfg = transformers.LlamaConfig(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=1, num_attention_heads=2,
                                   num_key_value_heads=2, attention_bias=True)
    hf = transformers.LlamaForCausalLM(cfg)
    with pytest.raises(ValueError, match=r'_proj\.bias.*refusing to drop it'):
        LlamaForCausalLM.from_hf(hf, device='cpu')
    # a Qwen2 state dict with an extra o_proj bias
    m = _qwen2()
    shape = LlamaShape.from_hf(m.config)
    sd = legacy_state_dict(m.state_dict(), shape)
    sd['model.layers.0.self_attn.o_proj.bias'] = torch.zeros(256)
    with pytest.raises(ValueError, match='o_proj.bias'):
        LlamaVerifyEngine(shape, sd)
    # an MLP bias
    sd = legacy_state_dict(m.state_dict(), shape)
    sd['model.layers.1.mlp.down_proj.bias'] = torch.zeros(256)
    with pytest.raises(ValueError, match='down_proj.bias'):
        LlamaVerifyEngine(shape, sd)
    # q/k/v biases under a shape without qkv_bias
    sd = legacy_state_dict(m.state_dict(), shape)
    plain = LlamaShape.from_hf(m.config)
    plain.qkv_bias = False
    with pytest.raises(ValueError, match='qkv_bias'):
        LlamaVerifyEngine(plain, sd)
