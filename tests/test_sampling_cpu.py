# -*- coding: utf-8 -*-
"""CPU: the model of the device sampler (tests/sampling_model.py) — Philox known answers, the filter against transformers' warpers,
the distribution of the Gumbel-max draw — and the recognition rule of the stage (lookahead_generation_utils.device_sampling)."""
import numpy as np
import pytest
import torch

from painlessinferenceacceleration_amd.lookahead_generation_utils import device_sampling
from tests import sampling_model as sm


def _u32(words):
    return np.array([int(w, 16) for w in words.split()], dtype=np.uint32)


@pytest.mark.parametrize('ctr,key,want', [
    ('00000000 00000000 00000000 00000000', '00000000 00000000', '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ('ffffffff ffffffff ffffffff ffffffff', 'ffffffff ffffffff', '408f276d 41c83b0e a20bc7c6 6d5451fd'),
    ('243f6a88 85a308d3 13198a2e 03707344', 'a4093822 299f31d0', 'd16cfe09 94fdcceb 5001e420 24126ea1'),
])
def test_philox_known_answers(ctr, key, want):
    k = _u32(key)
    got = sm.philox4x32(_u32(ctr)[None], (k[0], k[1]))[0]
    assert [f'{int(w):08x}' for w in got] == want.split()


def test_sample_bits_layout():
    """token v reads word v & 3 of the block with counter (v >> 2, position, stream, 0) and key (seed lo, seed hi)"""
    seed, stream, position = 0x299f31d0a4093822, 0x13198a2e, 0x85a308d3
    bits = sm.sample_bits(seed, stream, position, 4 * 7 + 2)
    assert len(bits) == 30
    for v in (0, 5, 29):
        blk = sm.philox4x32(np.array([[v >> 2, position, stream, 0]], dtype=np.uint32), (seed & 0xFFFFFFFF, seed >> 32))[0]
        assert bits[v] == blk[v & 3]
    u = sm.uniform_of(np.array([0, 0xFFFFFFFF], dtype=np.uint32))
    assert u[0] == 2.0 ** -24 and u[1] == 1 - 2.0 ** -24
    assert (np.float32(u) == u).all()                        # exact in fp32, never 0 or 1


def test_keys_are_monotone_and_fold_zero():
    for dtype, inf in (('bf16', 0x7F80), ('fp16', 0x7C00)):
        bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
        keys = sm.keys_of(bits, dtype)
        vals = sm.bits_to_f64(bits, dtype)
        ok = ~np.isnan(vals)
        assert (keys[~ok] == 0).all() and (keys[ok] > 0).all()
        order = np.argsort(keys[ok], kind='stable')
        v = vals[ok][order]
        assert (np.diff(v) >= 0).all()
        k = keys[ok][order]
        assert ((np.diff(k) == 0) == (np.diff(v) == 0)).all()          # equal keys <=> equal values (-0 == +0)
        assert (sm.key_to_f64(k, dtype) == v).all()


def _tie_free_rows(n_rows, vocab, seed):
    """bf16 rows without two equal values: distinct bf16 bit patterns in random order"""
    rs = np.random.RandomState(seed)
    rows = []
    for _ in range(n_rows):
        mags = rs.choice(np.arange(0x3C00, 0x4180), size=vocab, replace=False).astype(np.uint16)      # 2^-7 .. ~16, distinct
        sign = (rs.rand(vocab) < 0.5).astype(np.uint16) << 15
        rows.append(mags | sign)
    return np.stack(rows)


@pytest.mark.parametrize('temperature', [0.7, 1.0])
@pytest.mark.parametrize('top_k', [0, 1, 50])
@pytest.mark.parametrize('top_p', [1.0, 0.9, 0.3])
def test_filter_equals_hf_warpers(temperature, top_k, top_p):
    """the model's kept set == TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper run in fp32 on tie-free rows"""
    from transformers import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    bits = _tie_free_rows(6, 640, 3)
    for row in bits:
        x = torch.from_numpy(sm.bits_to_f64(row, 'bf16')).float()[None]
        sc = x
        if temperature != 1.0:
            sc = TemperatureLogitsWarper(temperature)(None, sc)
        if top_k:
            sc = TopKLogitsWarper(top_k)(None, sc)
        if top_p < 1.0:
            sc = TopPLogitsWarper(top_p)(None, sc)
        want = torch.isfinite(sc[0]).numpy()
        kk, kp, kept = sm.filter_row(row, 'bf16', temperature, top_k, top_p)
        assert (kept == want).all(), (kk, kp, int(kept.sum()), int(want.sum()))
        assert (kk == 0) == (top_k == 0) and (kp == 0) == (top_p >= 1.0)


def test_topk_keeps_ties_and_topp_keeps_ties_at_the_edge():
    bits = sm.f32_to_bits(np.array([3.0, 1.0, 2.0, 2.0, 0.5, -1.0, 2.0, 0.25], dtype=np.float32), 'bf16')
    kk, kp, kept = sm.filter_row(bits, 'bf16', 1.0, 2, 1.0)
    assert kept.tolist() == [True, False, True, True, False, False, True, False]          # the three 2.0 tie at the threshold
    # top-p: 3.0 alone has mass 0.42 < 0.5, so the 2.0 level is reached: all three tokens of the level stay
    kk, kp, kept = sm.filter_row(bits, 'bf16', 1.0, 0, 0.5)
    assert kept.tolist() == [True, False, True, True, False, False, True, False]
    kk, kp, kept = sm.filter_row(bits, 'bf16', 1.0, 0, 0.3)
    assert kept.tolist() == [True] + [False] * 7
    nan = bits.copy()
    nan[0] = 0x7FC0
    assert not sm.filter_row(nan, 'bf16', 1.0, 0, 1.0)[2][0]                              # NaN is never kept


@pytest.mark.parametrize('top_k,top_p', [(0, 1.0), (12, 1.0), (0, 0.8), (20, 0.9)])
def test_distribution_of_the_draw(top_k, top_p):
    """vocab 64, one fixed row, 200 000 draws over seeds and positions: every token's count within 5 sigma of N p, tokens outside
    the kept set never drawn.  Seeds are fixed: the test is deterministic."""
    vocab, temperature = 64, 0.8
    n_seeds, n_pos = 200, 1000
    N = n_seeds * n_pos
    rs = np.random.RandomState(11)
    bits = sm.f32_to_bits((rs.randn(vocab) * 2).astype(np.float32), 'bf16')
    kk, kp, kept = sm.filter_row(bits, 'bf16', temperature, top_k, top_p)
    z = sm.bits_to_f64(bits, 'bf16') / float(np.float32(temperature))
    p = np.where(kept, np.exp(z - z[kept].max()), 0.0)
    p /= p.sum()
    ctr = np.zeros((n_seeds, n_pos, vocab // 4, 4), dtype=np.uint32)
    ctr[..., 0] = np.arange(vocab // 4, dtype=np.uint32)
    ctr[..., 1] = (np.arange(n_pos, dtype=np.uint32) + 1)[None, :, None]
    ctr[..., 2] = 3
    seeds = (np.arange(n_seeds, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(12345))
    k0 = (seeds & np.uint64(0xFFFFFFFF))[:, None, None]
    k1 = (seeds >> np.uint64(32))[:, None, None]
    words = sm.philox4x32(ctr, (k0, k1)).reshape(n_seeds, n_pos, vocab)
    # spot check: the vectorised words are sample_bits'
    assert (words[5, 7] == sm.sample_bits(int(seeds[5]), 3, 8, vocab)).all()
    score = np.where(kept, z + sm.gumbel_of(words), -np.inf)
    toks = score.argmax(-1).reshape(-1)
    counts = np.bincount(toks, minlength=vocab)
    assert counts.sum() == N and (counts[~kept] == 0).all()
    sigma = np.sqrt(N * p * (1 - p))
    assert (np.abs(counts - N * p) <= 5 * sigma + 1e-9).all(), np.abs(counts - N * p).max()
    assert kept.sum() >= 2 and (counts[kept] > 0).sum() >= 2


def test_sample_row_is_a_function_of_seed_stream_position():
    rs = np.random.RandomState(2)
    bits = sm.f32_to_bits((rs.randn(512) * 2).astype(np.float32), 'bf16')
    a = [sm.sample_row(bits, 'bf16', pos, 0, 7, 0.8, 20, 0.9) for pos in range(1, 30)]
    assert a == [sm.sample_row(bits, 'bf16', pos, 0, 7, 0.8, 20, 0.9) for pos in range(1, 30)]
    assert a != [sm.sample_row(bits, 'bf16', pos, 1, 7, 0.8, 20, 0.9) for pos in range(1, 30)]
    assert a != [sm.sample_row(bits, 'bf16', pos, 0, 8, 0.8, 20, 0.9) for pos in range(1, 30)]
    assert len(set(a)) >= 2
    # top_k = 1 is the plain argmax whatever the seed
    assert sm.sample_row(bits, 'bf16', 5, 0, 99, 0.8, 1, 1.0) == int(np.argmax(sm.bits_to_f64(bits, 'bf16')))
    # the penalty moves a member: penalise the argmax hard and it is no longer the top_k = 1 pick
    top = int(np.argmax(sm.bits_to_f64(bits, 'bf16')))
    members = np.zeros(512, dtype=bool)
    members[top] = True
    assert sm.sample_row(bits, 'bf16', 5, 0, 99, 0.8, 1, 1.0, members=members, penalty=50.0) != top


# ---- recognition ---------------------------------------------------------------------------------------------------------------------
class _Eng(object):
    def set_sampling(self, *a, **k):
        pass

    def set_repetition_penalty(self, p):
        pass


def _warpers():
    from transformers import (LogitsProcessorList, RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper, TopKLogitsWarper,
                              TopPLogitsWarper)
    return LogitsProcessorList, RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper


def test_device_sampling_accepts_every_list_shape():
    L, RP, T, K, P = _warpers()
    eng = _Eng()
    base = {'seed': 7, 'temperature': 1.0, 'top_k': 0, 'top_p': 1.0, 'penalty': None}
    cases = [
        ([], {}),
        ([T(0.8)], {'temperature': 0.8}),
        ([K(50)], {'top_k': 50}),
        ([P(0.95)], {'top_p': 0.95}),
        ([T(0.8), K(50)], {'temperature': 0.8, 'top_k': 50}),
        ([T(0.8), P(0.95)], {'temperature': 0.8, 'top_p': 0.95}),
        ([K(50), P(0.95)], {'top_k': 50, 'top_p': 0.95}),
        ([T(0.8), K(50), P(0.95)], {'temperature': 0.8, 'top_k': 50, 'top_p': 0.95}),
        ([RP(1.3)], {'penalty': 1.3}),
        ([RP(1.3), T(0.8), K(50), P(0.95)], {'penalty': 1.3, 'temperature': 0.8, 'top_k': 50, 'top_p': 0.95}),
        ([RP(1.3), P(0.5)], {'penalty': 1.3, 'top_p': 0.5}),
    ]
    for procs, want in cases:
        got = device_sampling(L(procs), eng, do_sample=True, seed=7)
        assert got == dict(base, **want), (procs, got)
    assert device_sampling(None, eng, do_sample=True, seed=7) == base
    assert device_sampling(L([T(0.8)]), eng, do_sample=True, seed=-1)['seed'] == 0xFFFFFFFFFFFFFFFF


def test_device_sampling_rejections():
    L, RP, T, K, P = _warpers()
    from transformers import NoRepeatNGramLogitsProcessor
    eng = _Eng()
    full = [T(0.8), K(50), P(0.95)]
    ok = dict(do_sample=True, seed=7)
    assert device_sampling(L(full), eng, **ok) is not None
    assert device_sampling(L(full), eng, do_sample=False, seed=7) is None                 # greedy
    assert device_sampling(L(full), eng, do_sample=True, seed=None) is None               # no seed: the stage is opt-in
    assert device_sampling(L(full), eng, do_sample=True, seed=7.0) is None
    assert device_sampling(L(full), eng, do_sample=True, seed=True) is None
    assert device_sampling(L(full), eng, do_sample=True, seed=7, enabled=False) is None   # device_processors=False
    assert device_sampling(L(full), object(), **ok) is None                               # an engine without the stage
    assert device_sampling(L([K(50), T(0.8)]), eng, **ok) is None                         # wrong order
    assert device_sampling(L([P(0.9), K(50)]), eng, **ok) is None
    assert device_sampling(L([T(0.8), RP(1.3)]), eng, **ok) is None                       # the penalty goes first
    assert device_sampling(L([T(0.8), T(0.9)]), eng, **ok) is None                        # one type twice
    assert device_sampling(L([K(50, min_tokens_to_keep=2)]), eng, **ok) is None
    assert device_sampling(L([P(0.9, min_tokens_to_keep=2)]), eng, **ok) is None
    assert device_sampling(L([P(0.9, filter_value=-1e4)]), eng, **ok) is None
    assert device_sampling(L([K(50, filter_value=-1e4)]), eng, **ok) is None
    assert device_sampling(L(full + [NoRepeatNGramLogitsProcessor(2)]), eng, **ok) is None      # an extra processor
    assert device_sampling(L([NoRepeatNGramLogitsProcessor(2)] + full), eng, **ok) is None
    assert device_sampling(L([RP(1.3), RP(1.2)] + full), eng, **ok) is None

    class MyTopK(K):
        pass
    assert device_sampling(L([MyTopK(50)]), eng, **ok) is None                            # a subclass may override __call__
    t = T(0.8)
    t.temperature = 0.0
    assert device_sampling(L([t]), eng, **ok) is None
