# -*- coding: utf-8 -*-
"""The host arithmetic of the weight-image builder without a GPU: the rule that turns the second QKV image of the multi-block step
on (qkv_mb_workgroups) and the lane spreader of models with head_dim < 128 (to_lanes / fp8_lanes)."""
import numpy as np
import pytest
import torch

from painlessinferenceacceleration_amd import _lib
from painlessinferenceacceleration_amd.llama_engine import fp8_lanes
from painlessinferenceacceleration_amd.weight_images import qkv_mb_workgroups, to_lanes


@pytest.fixture(autouse=True)
def _no_override(monkeypatch):
    monkeypatch.delenv('LA_QKV_MB_WG', raising=False)


@pytest.mark.parametrize('args,want', [
    ((32, 32, 256, 8, 128), 0),          # Llama-2-7B: 24 pairs per workgroup, 75 % of a 32-row MFMA block, a multiple of 4
    ((40, 40, 256, 4, 128), 240),        # Llama-2-13B: 30 pairs per workgroup is no multiple of 4
    ((32, 8, 256, 8, 128), 96),          # Mistral / Mixtral: 12 pairs per workgroup, 37.5 % of a block
])
def test_qkv_mb_workgroups_of_the_model_shapes(args, want):
    assert qkv_mb_workgroups(*args) == want


@pytest.mark.parametrize('nh,nkv', [(32, 32), (40, 40), (32, 8)])
def test_qkv_mb_workgroups_off(nh, nkv, monkeypatch):
    for max_blocks in (0, 1):
        assert qkv_mb_workgroups(nh, nkv, 256, max_blocks, 128) == 0
    assert qkv_mb_workgroups(nh, nkv, 0, 8, 128) == 0
    for head_dim in (64, 96):
        assert qkv_mb_workgroups(nh, nkv, 256, 8, head_dim) == 0
    monkeypatch.setenv('LA_QKV_MB_WG', '128')          # the override does not lift these conditions
    assert qkv_mb_workgroups(nh, nkv, 256, 1, 128) == 0 and qkv_mb_workgroups(nh, nkv, 0, 8, 128) == 0


def test_qkv_mb_workgroups_override(monkeypatch):
    monkeypatch.setenv('LA_QKV_MB_WG', '0')
    assert qkv_mb_workgroups(32, 8, 256, 8, 128) == 0 and qkv_mb_workgroups(40, 40, 256, 4, 128) == 0
    monkeypatch.setenv('LA_QKV_MB_WG', '128')
    assert qkv_mb_workgroups(32, 8, 256, 8, 128) == 128
    monkeypatch.setenv('LA_QKV_MB_WG', '100')          # no multiple of 16
    assert qkv_mb_workgroups(32, 8, 256, 8, 128) == 0
    monkeypatch.setenv('LA_QKV_MB_WG', '256')          # not fewer workgroups than the CU-wide plan
    assert qkv_mb_workgroups(32, 8, 256, 8, 128) == 0
    monkeypatch.setenv('LA_QKV_MB_WG', '64')           # 48 pairs per workgroup: more than a 32-row block
    assert qkv_mb_workgroups(32, 8, 256, 8, 128) == 0


def lane_map(head_dim):
    src = np.zeros(128, dtype=np.int32)
    _lib.check(_lib.lib.la_head_lane_map(head_dim, src.ctypes.data_as(_lib.pi32)), 'head_lane_map')
    return src


@pytest.mark.parametrize('head_dim', [64, 96])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.uint8])
def test_to_lanes_rows_and_columns(head_dim, dtype):
    src = lane_map(head_dim)
    assert sorted(src[src >= 0].tolist()) == list(range(head_dim))
    n_h, K = 3, 5
    w = (torch.arange(n_h * head_dim * K, dtype=torch.float32).reshape(n_h * head_dim, K) % 251 + 1).to(dtype)      # no zero entry
    rows = to_lanes(w, n_h, 0, src)
    cols = to_lanes(w.t().contiguous(), n_h, 1, src)
    assert rows.shape == (n_h * 128, K) and cols.shape == (K, n_h * 128) and rows.dtype == dtype
    assert torch.equal(cols, rows.t())
    for h in range(n_h):
        for lane in range(128):
            got = rows[h * 128 + lane]
            if src[lane] >= 0:
                assert torch.equal(got, w[h * head_dim + src[lane]]), (h, lane)
            else:
                assert not got.any(), (h, lane)          # padding lanes: exact zeros


def test_to_lanes_of_a_bias_column_and_of_full_heads():
    src = lane_map(64)
    b = torch.arange(1, 2 * 64 + 1, dtype=torch.bfloat16)
    out = to_lanes(b.reshape(-1, 1), 2, 0, src).reshape(-1)
    assert out.shape == (256,) and out[:128][src >= 0].tolist() == b[:64][src[src >= 0]].tolist() and not out[:128][src < 0].any()
    w = torch.ones(256, 4)
    assert to_lanes(w, 2, 0, lane_map(128)) is w


@pytest.mark.parametrize('head_dim', [64, 96])
@pytest.mark.parametrize('dim', [0, 1])
def test_fp8_lanes_is_to_lanes_of_the_bytes(head_dim, dim):
    src = lane_map(head_dim)
    n_h = 2
    rs = np.random.RandomState(head_dim + dim)
    shape = (n_h * head_dim, 7) if dim == 0 else (7, n_h * head_dim)
    q = torch.from_numpy(rs.randint(1, 256, size=shape).astype(np.uint8))
    s = torch.from_numpy(rs.rand(shape[0]).astype(np.float32) + 0.5)
    q2, s2 = fp8_lanes(q, s, n_h, dim, src)
    assert torch.equal(q2, to_lanes(q, n_h, dim, src))
    if dim == 0:                         # the scales follow the rows; padding rows get 1
        keep = torch.from_numpy(np.tile(src >= 0, n_h))
        assert torch.equal(s2[keep], to_lanes(s.reshape(-1, 1), n_h, 0, src).reshape(-1)[keep]) and bool((s2[~keep] == 1).all())
    else:
        assert s2 is s
