# -*- coding: utf-8 -*-
"""The census (tests/census.py) against the CPU oracle: expected_visible + the readout recover every class count from the oracle's
residual stream, and a planted wrong bit in the expected mask is reported as that (row, key) pair.  No GPU."""
import numpy as np
import pytest
import torch

from oracle import llama_oracle as lo
from oracle.tiny import random_tree
from tests.census import BAR, CensusModel, CensusStats, census_check, expected_visible, wide_rowmasks


def _mask(rows, T):
    return np.array([[(int(rows[i]) >> j) & 1 for j in range(T)] for i in range(T)], dtype=np.int64)


def _oracle_step(cm, dtype, P, T, seed, oracle_cls=lo.OracleLlama):
    """prompt of P tokens + one T-row random tree through the oracle -> (hidden of the tree rows, ids, rows, key tokens)"""
    shape, sd = cm.shape(), cm.weights(dtype)
    oracle = oracle_cls(shape, sd)
    oracle.trace_hidden = True
    rs = np.random.RandomState(seed)
    prompt = rs.randint(0, cm.vocab, size=P)
    _, past = oracle.forward(torch.from_numpy(prompt), torch.tril(torch.ones((P, P), dtype=torch.long)), None)
    h_prompt = oracle.hidden_trace[-1]
    _, rows = random_tree(rs, T)
    ids = rs.randint(0, cm.vocab, size=T)
    full = torch.cat([torch.ones((T, P), dtype=torch.long), torch.from_numpy(_mask(rows, T))], 1)
    oracle.forward(torch.from_numpy(ids), full, past)
    return oracle.hidden_trace[-1], ids, rows, prompt, h_prompt


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('nh,nkv,hd,window,P', [(2, 2, 128, 0, 37), (2, 2, 128, 0, 700), (4, 2, 128, 40, 150), (4, 2, 128, 100, 333),
                                               (2, 2, 128, 37, 37), (6, 3, 128, 0, 226), (2, 2, 64, 33, 90), (2, 2, 96, 0, 65)])
def test_oracle_reproduces_every_expected_histogram(dtype, nh, nkv, hd, window, P):
    cm = CensusModel(nh, nkv, head_dim=hd, window=window)
    assert cm.layout == 'disjoint'
    st = CensusStats(f'oracle {nh}/{nkv} hd {hd} window {window} P {P} {dtype}')
    for T in (1, 17, 64):
        h, ids, rows, prompt, h_prompt = _oracle_step(cm, dtype, P, T, seed=P + T)
        vis = expected_visible(P, [int(r) for r in rows], window)
        census_check(cm, h, ids, vis, np.concatenate([prompt, ids]), f'tree T={T}', st)
    # the prompt rows themselves: one causal chain from an empty cache
    visp = expected_visible(0, [(2 << i) - 1 for i in range(P)], window)
    census_check(cm, h_prompt, prompt, visp, prompt, 'prompt chain', st)
    print(st)
    assert st.checks == (1 + 17 + 64 + P) * nh and st.worst < BAR


def test_overlap_layout_when_the_lanes_fill_the_hidden_limit():
    """40 / 40 heads at head_dim 128: hidden = 5120 holds no separate class dims; the row's own embedding is dropped"""
    cm = CensusModel(40, 40, vocab=512)
    assert cm.layout == 'overlap' and cm.hidden == 5120
    st = CensusStats('oracle 40/40 overlap')
    h, ids, rows, prompt, _ = _oracle_step(cm, torch.bfloat16, 50, 20, seed=3)
    vis = expected_visible(50, [int(r) for r in rows], 0)
    census_check(cm, h, ids, vis, np.concatenate([prompt, ids]), 'overlap tree', st)
    print(st)


def test_k_proj_does_not_matter():
    """q = 0: another k_proj (another seed) gives the same residual stream, bit for bit"""
    a, b = CensusModel(2, 2, seed=0), CensusModel(2, 2, seed=0)
    sa, sb = a.weights(), b.weights()
    kp = 'model.layers.0.self_attn.k_proj.weight'
    assert float(sa[kp].float().abs().max()) > 0
    sb[kp] = torch.flip(sb[kp], dims=[0, 1]).contiguous()
    assert not torch.equal(sa[kp], sb[kp])
    outs = []
    for sd in (sa, sb):
        o = lo.OracleLlama(a.shape(), sd)
        o.trace_hidden = True
        ids = torch.arange(40) * 7 % a.vocab
        o.forward(ids, torch.tril(torch.ones((40, 40), dtype=torch.long)), None)
        outs.append(o.hidden_trace[-1])
    assert torch.equal(outs[0], outs[1])


def test_batch_oracle_slots_are_invisible_to_each_other(monkeypatch):
    """OracleLlamaBatch (the cursor-batch twin: softmax in the storage dtype, in-place KV buffers): two samples, one left-padded,
    one tree step at their cursors; each sample's rows see its own unpadded keys and its own tree rows only"""
    cm = CensusModel(2, 2)
    shape, sd = cm.shape(), cm.weights(torch.bfloat16)
    oracle = lo.OracleLlamaBatch(shape, sd, max_pos=256)
    seen = []
    real_rms = lo._rms
    monkeypatch.setattr(lo, '_rms', lambda x, w, eps, cast_first=False: (seen.append(x), real_rms(x, w, eps, cast_first))[1])
    rs = np.random.RandomState(11)
    B, P, W, L, pad = 2, 40, 9, 128, 7
    ids0 = rs.randint(0, cm.vocab, size=(B, P))
    am = np.ones((B, P), dtype=np.int64)
    am[1, :pad] = 0
    col = np.concatenate([am, np.ones((B, L - P), dtype=np.int64)], axis=1)
    full = torch.tril(torch.from_numpy(col)[:, None, None].expand(-1, -1, L, -1), 0).contiguous()
    _, past = oracle.forward_batch(torch.from_numpy(ids0), full[:, :, :P, :P], None, decoding_max_length=L)
    trees = [random_tree(rs, W)[1] for _ in range(B)]
    d_ids = rs.randint(0, cm.vocab, size=(B, W))
    d_masks = np.stack([_mask(t, W) for t in trees])
    step_mask = torch.cat([full[:, :, P:P + W, :P], torch.from_numpy(d_masks[:, None])], dim=-1)
    seen.clear()
    oracle.forward_batch(torch.from_numpy(d_ids), step_mask, past, cursors=[P, P])
    h = seen[-1]                                                     # the input of the final norm: the residual stream [B, W, hidden]
    st = CensusStats('batch oracle')
    for b in range(B):
        vis = expected_visible(P, [int(r) for r in trees[b]], 0)
        vis[:, :P] &= am[b].astype(bool)[None, :]                    # padding keys are masked for every row
        census_check(cm, h[b], d_ids[b], vis, np.concatenate([ids0[b], d_ids[b]]), f'batch sample {b}', st)
    print(st)
    assert st.checks == B * W * cm.nh


@pytest.mark.parametrize('flip', ['lost', 'gained'])
def test_planted_bit_is_reported_at_its_row_and_key(flip):
    """Control on the detector (not on a kernel): one wrong bit in the expected mask is reported as that (row, key) pair"""
    cm = CensusModel(4, 2, window=40)
    P, T = 150, 33
    h, ids, rows, prompt, _ = _oracle_step(cm, torch.bfloat16, P, T, seed=5)
    keys = np.concatenate([prompt, ids])
    vis = expected_visible(P, [int(r) for r in rows], 40)
    census_check(cm, h, ids, vis, keys, 'unplanted')
    row = 21
    if flip == 'lost':          # the expectation loses a key the row does see
        key = int(np.nonzero(vis[row])[0][5])
    else:                       # the expectation gains a key below the row's window horizon
        key = int(np.nonzero(~vis[row, :P])[0][-1])
    bad = vis.copy()
    bad[row, key] = not bad[row, key]
    with pytest.raises(AssertionError) as e:
        census_check(cm, h, ids, bad, keys, 'planted')
    msg = str(e.value)
    c = int(cm.cls[keys[key]])
    assert f'row {row} ' in msg and f'class {c}:' in msg, msg
    listed = msg.split('should see: ')[1].split(';')[0] if flip == 'gained' else msg.split('should NOT see: ')[1].split(' (key')[0]
    assert str(key) in [s.strip() for s in listed.strip('[]').split(',')], (key, msg)


def test_expected_visible_is_the_documented_rule():
    # no window: all committed keys, ancestors + self
    v = expected_visible(5, [0b1, 0b11, 0b101])
    assert v.shape == (3, 8) and v[:, :5].all()
    assert v[:, 5:].tolist() == [[True, False, False], [True, True, False], [True, False, True]]
    # window 3, nkeys 10: root at position 10 sees keys 7.., a depth-2 row at position 11 sees 8..
    v = expected_visible(10, [0b1, 0b11], window=3)
    assert np.nonzero(v[0, :10])[0].tolist() == [7, 8, 9] and np.nonzero(v[1, :10])[0].tolist() == [8, 9]
    # a wide tree: row 70 names an ancestor in an earlier block
    rm = np.zeros((71, 2), dtype=np.uint64)
    rm[70] = (1 | (1 << 5), 1 << 6)
    masks = wide_rowmasks(rm)
    assert masks[70] == 1 | (1 << 5) | (1 << 70)
    v = expected_visible(2, masks)
    assert np.nonzero(v[70])[0].tolist() == [0, 1, 2, 7, 72]
