# -*- coding: utf-8 -*-
"""The device images LlamaVerifyEngine builds from a state dict, pinned byte for byte: plans (balanced_wg, qkv_mb_wg), the byte
accounting (weight_bytes), a sha256 over every torch tensor the engine keeps alive (packed projections, scales, biases, norms,
embedding, MoE expert buffers) and over the RoPE tables.  tests/golden/weight_image_digests.json was recorded on an MI355X from the
commit BEFORE the weight-image builder moved into weight_images.py (record() below, run twice in separate processes, the second
over poisoned allocator memory: every digest agreed, so no image has bytes the pack kernels leave unwritten).  The plans depend
on the CU count, which the fixture stores: on another device the test fails rather than skips."""
import hashlib
import json
import os

import pytest
import torch

from painlessinferenceacceleration_amd.llama_engine import LlamaShape, LlamaVerifyEngine, random_weights
from tests.tiny_model import TINY, TINY_MOE, moe_shape

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'weight_image_digests.json')


def _tiny(**kw):
    return LlamaShape(1, TINY['hidden'], TINY['n_heads'], TINY['n_kv_heads'], TINY['ffn'], TINY['vocab'], TINY['rms_eps'], **kw)


def _hd64():
    return LlamaShape(1, TINY['hidden'], 4, 2, TINY['ffn'], TINY['vocab'], TINY['rms_eps'], head_dim=64, qkv_bias=True)


def _llama7b():
    return LlamaShape(1, 4096, 32, 32, 11008, 32000)


def _gqa():
    return LlamaShape(1, 4096, 32, 8, 512, 512)


# name -> (shape factory, random_weights seed, weights dtype, engine keyword arguments)
CONFIGS = {
    'tiny': (_tiny, 1, torch.bfloat16, {}),
    'tiny_f16': (_tiny, 1, torch.float16, {}),
    'tiny_unfused_qkv': (_tiny, 1, torch.bfloat16, dict(gemm_cfg=[0, -1])),
    'hd64_gqa_bias': (_hd64, 2, torch.bfloat16, {}),
    'hd64_gqa_bias_fp8': (_hd64, 2, torch.bfloat16, dict(weight_format='fp8')),
    'hd64_unbalanced': (_hd64, 2, torch.bfloat16, dict(balanced=False)),          # lanes, then la_qkv_row_perm, then the plain image
    'hd64_unbalanced_fp8': (_hd64, 2, torch.bfloat16, dict(balanced=False, weight_format='fp8')),
    'moe': (lambda: moe_shape(dict(TINY_MOE, n_layers=1)), 3, torch.bfloat16, dict(n_slots=2, max_blocks=2)),
    'llama7b_layer_mb4': (_llama7b, 5, torch.bfloat16, dict(n_slots=4, max_blocks=4)),
    'llama7b_layer_fp8': (_llama7b, 5, torch.bfloat16, dict(weight_format='fp8', max_blocks=0)),
    'gqa_mb2': (_gqa, 4, torch.bfloat16, dict(n_slots=2, max_blocks=2)),
    'gqa_unbalanced': (_gqa, 4, torch.bfloat16, dict(balanced=False)),
}
_weights = {}


def _state_dict(name):
    """random_weights on the CPU, once per (shape, seed, dtype): the engine leaves the dict as it is (consume_state_dict=False)"""
    make, seed, dtype, _ = CONFIGS[name]
    key = (make, seed, dtype)
    if key not in _weights:
        _weights.clear()                 # one set at a time: the 7B layer is 0.9 GB
        _weights[key] = random_weights(make(), seed, device='cpu', dtype=dtype)
    return _weights[key]


def digest(t):
    return hashlib.sha256(memoryview(t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy())).hexdigest()


def record(name):
    make, _, _, kw = CONFIGS[name]
    eng = LlamaVerifyEngine(make(), _state_dict(name), max_length=128, **kw)
    torch.cuda.synchronize()
    kept = [t for t in eng._keep if torch.is_tensor(t)]
    return {'balanced_wg': [int(x) for x in eng.balanced_wg], 'qkv_mb_wg': int(eng.qkv_mb_wg),
            'weight_bytes': {k: int(v) for k, v in eng.weight_bytes.items()},
            'keep': sorted(digest(t) for t in kept),
            'rope_cos': digest(eng.rope_cos), 'rope_sin': digest(eng.rope_sin)}


def record_all():
    """the fixture's content, from whatever tree this runs in"""
    return {'cu_count': int(torch.cuda.get_device_properties(0).multi_processor_count),
            'configs': {name: record(name) for name in CONFIGS}}


@pytest.fixture(scope='module')
def golden():
    with open(FIXTURE) as f:
        g = json.load(f)
    assert sorted(g['configs']) == sorted(CONFIGS)
    return g


def test_device_is_the_one_the_fixture_was_recorded_on(golden):
    assert torch.cuda.get_device_properties(0).multi_processor_count == golden['cu_count'], \
        'the balanced plans deal rows out per CU: the digests hold for the recorded CU count only'


@pytest.mark.parametrize('name', list(CONFIGS))
def test_weight_images_match_the_recorded_digests(golden, name):
    assert torch.cuda.get_device_properties(0).multi_processor_count == golden['cu_count']
    got, want = record(name), golden['configs'][name]
    print(name, got['balanced_wg'], got['qkv_mb_wg'], got['weight_bytes'], len(got['keep']))
    assert got['balanced_wg'] == want['balanced_wg'] and got['qkv_mb_wg'] == want['qkv_mb_wg']
    assert got['weight_bytes'] == want['weight_bytes']
    assert len(got['keep']) == len(want['keep'])
    assert got['keep'] == want['keep'], [i for i, (a, b) in enumerate(zip(got['keep'], want['keep'])) if a != b]
    assert got['rope_cos'] == want['rope_cos'] and got['rope_sin'] == want['rope_sin']


def test_plans_of_the_recorded_shapes(golden):
    """what the shapes were chosen for: no plan at the tiny shape, all three at the 7B layer, the second QKV image at the GQA shape"""
    c = golden['configs']
    assert c['tiny']['balanced_wg'] == [0, 0, 0]
    assert all(c['llama7b_layer_mb4']['balanced_wg']) and c['llama7b_layer_mb4']['qkv_mb_wg'] == 0
    assert c['gqa_mb2']['qkv_mb_wg'] == 96
    assert c['gqa_unbalanced']['balanced_wg'] == [0, 0, 0]
