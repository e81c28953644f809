# -*- coding: utf-8 -*-
"""CPU: top-N log-probabilities — the numpy model of the device stage (tests/top_logprob_model.py) against a brute-force sort on
every planted row, the ABI surface, and how the generation loops plan the stage: decoding_kwargs['top_logprobs'] implies
output_logprobs, is refused where that is refused, switches the stage on after the scalar stage and off before it (also when a step
raises), leaves a request without the key with exactly the calls of today, and returns per generated token a list of n
(token_id, logprob) pairs aligned with kwargs['logprobs'] (every batch list cut at its own stop)."""
import os
import re

import numpy as np
import pytest
import torch

from painlessinferenceacceleration_amd import _lib
from painlessinferenceacceleration_amd.lookahead_generation_utils import device_stages, plan_top_logprobs
from tests import logprob_model as lm
from tests import test_logprobs_cpu as base
from tests import top_logprob_model as tm
from tests.oracle_engine import OracleEngine
from tests.tiny_model import tiny_shape, tiny_weights

N_NEW, PROMPT, B_IDS, B_AM, B_LEN, DK = base.N_NEW, base.PROMPT, base.B_IDS, base.B_AM, base.B_LEN, base.DK
NEW_SYMBOLS = ('la_llama_set_top_logprobs', 'la_llama_top_logprobs_read', 'la_top_logprob_rows')
TOP = 5


# ---------------------------------------------------------------------------------------------------------------- the model
def _brute(row, n):
    """ids of the n largest values, value descending then id ascending; -0.0 == 0.0 in Python, so signed zeros tie"""
    return sorted(range(len(row)), key=lambda i: (-float(row[i]), i))[:n]


@pytest.mark.parametrize('dtype', ['bfloat16', 'float16'])
@pytest.mark.parametrize('vocab,n', [(8, 1), (8, 5), (512, 5), (512, 20), (32000, 1), (32000, 20), (152064, 5)])
def test_model_agrees_with_a_brute_force_sort_on_every_planted_row(vocab, n, dtype):
    rows = tm.planted_rows(vocab, dtype, n, n_rows=12)
    ids, f64, im = tm.top_model(rows, dtype, n)
    assert np.array_equal(f64[:, 0], lm.logprob_f64(rows, ids[:, 0])) and np.array_equal(f64[:, -1], lm.logprob_f64(rows, ids[:, -1]))
    for r in range(rows.shape[0]):
        assert ids[r].tolist() == _brute(rows[r], n), r
    assert np.all(np.diff(f64, axis=1) <= 0)                                  # most likely first
    assert np.all(np.abs(im.astype(np.float64) - f64) <= lm.bound_device(f64))           # the documented bound of the scalar stage
    # the planted rows are what their names say
    assert ids[4].tolist() == list(range(n)) and np.allclose(f64[4], -np.log(vocab), atol=1e-12)      # all values equal
    g = n // 2
    cut = rows[8][ids[8][-1]]
    assert (rows[8] > cut).sum() == g and (rows[8] == cut).sum() > n - g      # the plateau: more ties than places
    assert ids[8][g:].tolist() == np.flatnonzero(rows[8] == cut)[:n - g].tolist() and ids[8][g] == 0
    assert set(np.flatnonzero(rows[8] == cut)) >= {i for i in tm.PLATEAU_IDS if i < vocab} | {vocab - 1}
    assert ids[9].tolist() == sorted(ids[9].tolist(), reverse=True)           # ascending values at ascending ids: listed backwards
    z = ids[10][g:]
    assert (rows[10][z] == 0).all() and z.tolist() == np.flatnonzero(rows[10] == 0)[:n - g].tolist()
    if vocab >= 32:
        assert {bool(np.signbit(v)) for v in rows[10][rows[10] == 0]} == {True, False}      # both zeros are in the row
    assert ids[11][0] == vocab - 1
    if dtype == 'float16':
        assert rows[6].max() > 59000 and rows[6].min() < -59000


def test_keys_fold_the_zeros_and_drop_nan():
    x = np.array([[0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 2.0]], dtype=np.float32)
    for dtype in ('bfloat16', 'float16'):
        k = tm.keys(x, dtype)[0]
        assert k[0] == k[1] and k[6] == 0 and k[5] >= 1
        assert k[5] < k[3] < k[0] < k[2] < k[7] < k[4]
        assert tm.top_ids(x, dtype, 8)[0].tolist() == [4, 7, 2, 0, 1, 3, 5, -1]      # NaN is never listed


# ------------------------------------------------------------------------------------------------------------------- the ABI
def test_abi_still_reports_17_and_binds_the_new_entry_points():
    assert _lib.ABI_VERSION == 17 and _lib.lib.la_abi_version() == 17
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), 'include', 'lookahead_hip.h')).read()
    assert int(re.search(r'#define LA_TOPLP_MAX\s+(\d+)', hdr).group(1)) == tm.TOP_MAX == 20
    for name in NEW_SYMBOLS:
        assert re.search(r'\b' + name + r'\s*\(', hdr), name
        assert name in _lib.PROTOTYPES and getattr(_lib.lib, name).argtypes is not None, name
    assert _lib.PROTOTYPES['la_llama_set_logprobs'] == (_lib.i32, _lib.vp, _lib.vp, _lib.i32)      # the scalar switch keeps its signature
    from painlessinferenceacceleration_amd.llama_engine import LlamaVerifyEngine
    for name in ('set_top_logprobs', 'top_logprobs'):
        assert callable(getattr(LlamaVerifyEngine, name))


# -------------------------------------------------------------------------------------------------------------- the planning
class Model(base.Model):
    def __init__(self, engine=None):
        super().__init__(engine or tm.RecordingEngine(tiny_shape(), tiny_weights(0), max_length=256))


class BModel(base.BModel):
    def __init__(self, engine=None, max_blocks=0):
        super().__init__(engine or tm.RecordingBatchEngine(tiny_shape(), tiny_weights(0), max_length=256, n_slots=4, max_blocks=max_blocks))


def _call(model, batch, entry, which, top=TOP, dk_extra=None, **kw):
    """one request with top_logprobs = top (0: without the key) and WITHOUT output_logprobs -> what the front door returned"""
    if entry == 'lookahead':
        dk_extra = dict(dk_extra or {}, **({'top_logprobs': top} if top else {}))
        return base._call(model, batch, entry, which, logprobs=False, dk_extra=dk_extra, **kw)
    procs = base._lists()[which]
    sampling = which == 'sampling'
    ids = torch.tensor(B_IDS if batch else PROMPT)
    extra = {'attention_mask': torch.tensor(B_AM), 'pad_token_id': kw.get('pad', 0)} if batch else {}
    max_length = ids.shape[1] + N_NEW
    seed = kw.get('sample_seed', 7)
    return model.greedy_search(ids, max_length, eos_token_id=kw.get('eos'), logits_processor=procs, do_sample=sampling,
                               stopping_criteria=base._criteria(max_length), device_processors=kw.get('device_processors', True),
                               sample_seed=seed if sampling else None, **({'top_logprobs': top} if top else {}), **extra)


@pytest.mark.parametrize('which', ['plain', 'penalty', 'sampling'])
@pytest.mark.parametrize('entry', ['lookahead', 'plain'])
@pytest.mark.parametrize('batch,max_blocks', base.FORMS)
def test_the_key_implies_logprobs_and_brackets_the_request(batch, max_blocks, entry, which):
    """on: scalar stage, then top-N, both before the prefill; off: top-N, then the scalar stage, last — also when a step raises"""
    for boom in (None, 'step'):
        model = BModel(max_blocks=max_blocks) if batch else Model()
        model.engine.boom_at = boom
        if boom:
            with pytest.raises(RuntimeError, match='boom'):
                _call(model, batch, entry, which)
        else:
            _call(model, batch, entry, which)
        log = model.engine.log
        on = log.index(('lp', True))
        assert log[on + 1] == ('top', TOP) and on + 1 < log.index(('prefill',)), log
        assert log[-2:] == [('top', 0), ('lp', False)], log
        assert [c for c in log if c[0] == 'top'] == [('top', TOP), ('top', 0)] and log.count(('lp', True)) == 1, log
        assert [c for c in log if c[0] not in ('lp', 'top')] == base._today(batch, which), log
        assert (len(model.engine.top_reads) == 0) == bool(boom) and (len(model.engine.reads) == 0) == bool(boom)


@pytest.mark.parametrize('which', ['plain', 'penalty', 'sampling'])
@pytest.mark.parametrize('entry', ['lookahead', 'plain'])
@pytest.mark.parametrize('batch,max_blocks', base.FORMS)
@pytest.mark.parametrize('logprobs', [False, True])
def test_a_request_without_the_key_makes_the_calls_of_today(logprobs, batch, max_blocks, entry, which):
    """byte for byte the logs of today, with and without output_logprobs: set_top_logprobs is never called, and the recording
    engines of tests/logprob_model.py (which have no such method) serve the request"""
    for model in (BModel(max_blocks=max_blocks) if batch else Model(),
                  base.BModel(max_blocks=max_blocks) if batch else base.Model()):
        out = base._call(model, batch, entry, which, logprobs=logprobs)
        log = model.engine.log
        assert not any(c[0] == 'top' for c in log)
        if logprobs:
            assert log[-1] == ('lp', False) and [c for c in log if c[0] != 'lp'] == base._today(batch, which)
        else:
            assert log == base._today(batch, which) and model.engine.reads == []
        if entry == 'lookahead':
            assert 'top_logprobs' not in out.kwargs
        else:
            assert torch.is_tensor(out) or len(out) == 2


def test_device_stages_switches_top_n_off_before_the_scalar_stage_when_the_body_raises():
    eng = tm.RecordingEngine(tiny_shape(), tiny_weights(0), max_length=256)
    with pytest.raises(KeyError):
        with device_stages(eng, None, [(0, 0, None)], logprobs=True, top_logprobs=3):
            assert eng.log == [('lp', True), ('top', 3)]
            raise KeyError('x')
    assert eng.log == [('lp', True), ('top', 3), ('top', 0), ('lp', False)]
    del eng.log[:]
    with device_stages(eng, None, [(0, 0, None)], logprobs=True):             # the default: one argument, no top-N call
        pass
    assert eng.log == [('lp', True), ('lp', False)]


@pytest.mark.parametrize('which,dk_extra,kw,word', base.REFUSED)
@pytest.mark.parametrize('batch', [False, True], ids=['bs1', 'batch'])
def test_requests_that_would_take_the_host_walk_are_refused_before_any_engine_call(batch, which, dk_extra, kw, word):
    model = BModel(max_blocks=4) if batch else Model()
    dk_extra = {k: (base._gather(batch) if v == 'GATHER' else v) for k, v in dk_extra.items()}
    with pytest.raises(ValueError, match=word):
        _call(model, batch, 'lookahead', which, dk_extra=dk_extra, **kw)
    assert model.engine.log == [] and model.engine.top_reads == []


@pytest.mark.parametrize('which,kw,word', [('other', {}, 'processor'), ('sampling', {'sample_seed': None}, 'sample_seed'),
                                           ('penalty', {'device_processors': False}, 'device_processors')])
@pytest.mark.parametrize('batch', [False, True], ids=['bs1', 'batch'])
def test_the_plain_front_doors_refuse_the_host_pick(batch, which, kw, word):
    model = BModel() if batch else Model()
    with pytest.raises(ValueError, match=word):
        _call(model, batch, 'plain', which, **kw)
    assert model.engine.log == []


@pytest.mark.parametrize('bad', [-1, 21, 2.5, True, 'five'])
def test_n_outside_1_to_20_is_refused(bad):
    eng = tm.RecordingEngine(tiny_shape(), tiny_weights(0), max_length=256)
    with pytest.raises(ValueError, match='top_logprobs'):
        plan_top_logprobs(bad, eng)
    assert plan_top_logprobs(0, eng) == 0 and plan_top_logprobs(None, eng) == 0 and plan_top_logprobs(False, eng) == 0
    assert plan_top_logprobs(1, eng) == 1 and plan_top_logprobs(20, eng) == 20
    for entry in ('lookahead', 'plain'):
        model = Model()
        with pytest.raises(ValueError, match='top_logprobs'):
            _call(model, False, entry, 'plain', top=bad)
        assert model.engine.log == []


@pytest.mark.parametrize('entry', ['lookahead', 'plain'])
def test_an_engine_without_the_stage_is_refused(entry):
    for eng in (OracleEngine(tiny_shape(), tiny_weights(0), max_length=256),
                lm.RecordingEngine(tiny_shape(), tiny_weights(0), max_length=256)):      # no stage at all; the scalar stage only
        with pytest.raises(ValueError, match='top_logprobs.*engine'):
            _call(base.Model(engine=eng), False, entry, 'plain')


# ---------------------------------------------------------------------------------------------------------- the output shape
def _ramp(slot, first, n_pos, n=TOP):
    return [[(100 * j + p, 1000.0 * slot + p - j) for j in range(n)] for p in range(first, first + n_pos)]


@pytest.mark.parametrize('entry', ['lookahead', 'plain'])
def test_bs1_returns_n_pairs_per_new_token_aligned_with_the_scalar_list(entry):
    model = Model()
    out = _call(model, False, entry, 'plain')
    seqs, lps, tops = (out.sequences, out.kwargs['logprobs'], out.kwargs['top_logprobs']) if entry == 'lookahead' else out
    n_new = seqs.shape[1] - len(PROMPT[0])
    assert n_new == N_NEW and model.engine.top_reads == [(0, len(PROMPT[0]), n_new)] == model.engine.reads
    assert len(lps) == len(tops) == n_new and tops == _ramp(0, len(PROMPT[0]), n_new)
    assert all(type(t) is int and type(v) is float for row in tops for t, v in row)


@pytest.mark.parametrize('entry', ['lookahead', 'plain'])
@pytest.mark.parametrize('max_blocks', [0, 2], ids=['cursor-batch', 'multi-block'])
def test_batch_lists_are_cut_at_the_stop(max_blocks, entry):
    P = len(B_IDS[0])
    ref = base._call(BModel(max_blocks=max_blocks), True, entry, 'plain', logprobs=False)
    ref = (ref.sequences if entry == 'lookahead' else ref).tolist()
    PAD = next(t for t in range(1, 64) if all(t not in r[P:] for r in ref))
    eos = next((t for t in ref[0][P:P + 5] if t not in ref[1][P:]), None)
    assert eos is not None
    model = BModel(max_blocks=max_blocks)
    out = _call(model, True, entry, 'plain', eos=eos, pad=PAD)
    seqs, lps, tops = (out.sequences, out.kwargs['logprobs'], out.kwargs['top_logprobs']) if entry == 'lookahead' else out
    n_new = [len([t for t in r[P:] if t != PAD]) for r in seqs.tolist()]
    assert n_new[0] < n_new[1] == N_NEW, n_new
    assert sorted(model.engine.top_reads) == [(b, B_LEN[b], n_new[b]) for b in range(2)]
    assert tops == [_ramp(b, B_LEN[b], n_new[b]) for b in range(2)] and [len(x) for x in lps] == n_new


def test_generate_carries_the_key_on_both_legs():
    for batch in (False, True):
        ids = torch.tensor(B_IDS if batch else PROMPT)
        extra = {'attention_mask': torch.tensor(B_AM)} if batch else {}
        for use_lookahead in (True, False):
            model = BModel() if batch else Model()
            out = model.generate(ids, max_new_tokens=N_NEW, pad_token_id=0, return_dict_in_generate=True,
                                 decoding_kwargs=dict(DK, use_lookahead=use_lookahead, top_logprobs=3), **extra)
            tops, lps = out.kwargs['top_logprobs'], out.kwargs['logprobs']
            one = tops if not batch else tops[0]
            assert len(one) == N_NEW == len(lps if not batch else lps[0]) and all(len(row) == 3 for row in one)
            assert model.engine.log[-2:] == [('top', 0), ('lp', False)]
