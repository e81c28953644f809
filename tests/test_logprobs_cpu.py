# -*- coding: utf-8 -*-
"""CPU: per-token log-probabilities — the numpy models of the device stage (tests/logprob_model.py) against each other, the ABI
surface, and how the four generation loops plan the stage: which requests switch it on (and off again, also when a step raises),
which are refused before any engine call, that a request without the key makes exactly the calls it made before, and the shape of
kwargs['logprobs'] (unpadded positions, every list cut at its own stop)."""
import re
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from painlessinferenceacceleration_amd import _lib
from painlessinferenceacceleration_amd.lookahead_cache import LookaheadCache
from painlessinferenceacceleration_amd.pretrained_model import LookaheadPreTrainedModel
from painlessinferenceacceleration_amd.pretrained_model_batch import LookaheadPreTrainedModel as BatchMixin
from tests import logprob_model as lm
from tests.oracle_engine import OracleBatchEngine, OracleEngine
from tests.tiny_model import tiny_shape, tiny_weights

N_NEW = 8
PROMPT = [[5 + 3 * i for i in range(17)]]
B_IDS = [[0, 0, 5, 6, 7], [3, 4, 5, 6, 8]]
B_AM = [[0, 0, 1, 1, 1], [1, 1, 1, 1, 1]]
B_LEN = [3, 5]                       # unpadded prompt lengths
DK = {'use_lookahead': True, 'decoding_mode': 'hier', 'decoding_length': 64, 'branch_length': 12, 'stop_words': {}}
NEW_SYMBOLS = ('la_llama_set_logprobs', 'la_llama_logprob_launches', 'la_llama_logprobs_read', 'la_logprob_rows')


# ---------------------------------------------------------------------------------------------------------------- the models
@pytest.mark.parametrize('dtype', ['bfloat16', 'float16'])
@pytest.mark.parametrize('vocab', [512, 32000, 152064])
def test_integer_mass_model_agrees_with_the_definition(vocab, dtype):
    rows, toks = lm.planted_rows(vocab, dtype, n_rows=12)
    want = lm.logprob_f64(rows, toks)
    got = lm.logprob_intmass(rows, toks).astype(np.float64)
    err = np.abs(got - want)
    print('vocab', vocab, dtype, 'worst err / bound', float((err / lm.bound_intmass(vocab, want)).max()))
    assert np.all(np.isfinite(want)) and np.all(want <= 0)
    assert np.all(err <= lm.bound_intmass(vocab, want)), (err, lm.bound_intmass(vocab, want))
    # the planted rows are what their names say
    assert abs(want[4] + np.log(vocab)) < 1e-12                               # all values equal
    assert -1e-6 < want[2] <= 0 and want[3] < -30                             # one logit 30 above the rest: its own lp, a far-down target
    assert rows[5].max() < -190
    if dtype == 'float16':
        assert rows[6].max() > 59000 and rows[6].min() < -59000 and want[7] < -100000


def test_integer_mass_is_order_independent():
    rows, toks = lm.planted_rows(32000, 'bfloat16', n_rows=8)
    perm = np.random.default_rng(3).permutation(32000)
    inv = np.argsort(perm)
    a = lm.logprob_intmass(rows, toks)
    b = lm.logprob_intmass(rows[:, perm], inv[toks])
    assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------------------------- the ABI
def test_abi_declares_exports_and_binds_the_new_entry_points():
    assert _lib.ABI_VERSION == 17 and _lib.lib.la_abi_version() == 17
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), 'include', 'lookahead_hip.h')).read()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b' + name + r'\s*\(', hdr), name
        assert name in _lib.PROTOTYPES and getattr(_lib.lib, name).argtypes is not None, name
    from painlessinferenceacceleration_amd.llama_engine import LlamaVerifyEngine
    for name in ('set_logprobs', 'logprobs', 'logprob_launches'):
        assert callable(getattr(LlamaVerifyEngine, name))


# -------------------------------------------------------------------------------------------------------------- the planning
class Model(LookaheadPreTrainedModel):
    def __init__(self, engine=None):
        self.engine = engine or lm.RecordingEngine(tiny_shape(), tiny_weights(0), max_length=256)
        self.generation_config = SimpleNamespace(eos_token_id=None, pad_token_id=0, return_dict_in_generate=False)
        self.lookahead_cache = LookaheadCache()


class BModel(BatchMixin):
    def __init__(self, engine=None, max_blocks=0):
        self.engine = engine or lm.RecordingBatchEngine(tiny_shape(), tiny_weights(0), max_length=256, n_slots=4, max_blocks=max_blocks)
        self.generation_config = SimpleNamespace(eos_token_id=None, pad_token_id=0, return_dict_in_generate=False)
        self.lookahead_cache = LookaheadCache()


def _lists():
    from transformers import (LogitsProcessorList, NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor,
                              TemperatureLogitsWarper, TopKLogitsWarper)
    return {'plain': None,
            'penalty': LogitsProcessorList([RepetitionPenaltyLogitsProcessor(1.3)]),
            'sampling': LogitsProcessorList([RepetitionPenaltyLogitsProcessor(1.3), TemperatureLogitsWarper(0.8), TopKLogitsWarper(20)]),
            'other': LogitsProcessorList([NoRepeatNGramLogitsProcessor(3)])}


def _criteria(max_length):
    from transformers import MaxLengthCriteria, StoppingCriteriaList
    return StoppingCriteriaList([MaxLengthCriteria(max_length)])


def _call(model, batch, entry, which, logprobs=True, dk_extra=None, sample_seed=7, device_processors=True, eos=None, pad=0, **kw):
    """one request -> what the front door returned"""
    procs = _lists()[which]
    sampling = which == 'sampling'
    ids = torch.tensor(B_IDS if batch else PROMPT)
    extra = {'attention_mask': torch.tensor(B_AM)} if batch else {}
    max_length = ids.shape[1] + N_NEW
    if entry == 'lookahead':
        dk = dict(DK, do_sample=sampling, device_processors=device_processors, **(dk_extra or {}))
        if logprobs:
            dk['output_logprobs'] = True
        if sampling and sample_seed is not None:
            dk['sample_seed'] = sample_seed
        return model.lookahead_generation(ids, logits_processor=procs, stopping_criteria=_criteria(max_length), eos_token_id=[eos],
                                          pad_token_id=pad, decoding_kwargs=dk, return_dict_in_generate=True, **extra, **kw)
    if batch:
        extra['pad_token_id'] = pad
    return model.greedy_search(ids, max_length, eos_token_id=eos, logits_processor=procs, do_sample=sampling,
                               stopping_criteria=_criteria(max_length), device_processors=device_processors,
                               sample_seed=sample_seed if sampling else None, output_logprobs=logprobs, **extra)


def _today(batch, which):
    """the stage calls of a request before this stage existed (pinned by tests/test_device_stages_cpu.py)"""
    log = [('reset_slot', -1)] if batch else [('reset',)]
    if which != 'plain':
        log.append(('pen', 1.3))
        if batch:
            log += [('seed', 0, B_IDS[0]), ('seed', 1, B_IDS[1])]
    if which == 'sampling':
        log += [('stream', 0, 0), ('stream', 1, 1)] if batch else [('stream', 0, 0)]
        log.append(('samp', True, 7, 0.8, 20, 1.0))
    log.append(('prefill',))
    if which != 'plain':
        log.append(('pen', 1.0))
    if which == 'sampling':
        log.append(('samp', False))
    return log


FORMS = [pytest.param(False, 0, id='bs1'), pytest.param(True, 0, id='cursor-batch'), pytest.param(True, 2, id='multi-block')]


@pytest.mark.parametrize('which', ['plain', 'penalty', 'sampling'])
@pytest.mark.parametrize('entry', ['lookahead', 'plain'])
@pytest.mark.parametrize('batch,max_blocks', FORMS)
def test_honoured_requests_switch_the_stage_on_before_the_prefill_and_off_at_the_end(batch, max_blocks, entry, which):
    for boom in (None, 'step'):
        model = BModel(max_blocks=max_blocks) if batch else Model()
        model.engine.boom_at = boom
        if boom:
            with pytest.raises(RuntimeError, match='boom'):
                _call(model, batch, entry, which)
        else:
            _call(model, batch, entry, which)
        log = model.engine.log
        assert log.index(('lp', True)) < log.index(('prefill',)), log
        assert log[-1] == ('lp', False) and log.count(('lp', True)) == 1 and log.count(('lp', False)) == 1, log
        assert [c for c in log if c[0] != 'lp'] == _today(batch, which), log
        assert (len(model.engine.reads) == 0) == bool(boom)          # read once per sequence, at the end of the request


@pytest.mark.parametrize('which', ['plain', 'penalty', 'sampling'])
@pytest.mark.parametrize('entry', ['lookahead', 'plain'])
@pytest.mark.parametrize('batch,max_blocks', FORMS)
def test_a_request_without_the_key_makes_the_calls_of_today(batch, max_blocks, entry, which):
    model = BModel(max_blocks=max_blocks) if batch else Model()
    out = _call(model, batch, entry, which, logprobs=False)
    assert model.engine.log == _today(batch, which) and model.engine.reads == []
    if entry == 'lookahead':
        assert 'logprobs' not in out.kwargs
    else:
        assert torch.is_tensor(out)


def _gather(batch):
    return SimpleNamespace(b_loc=2 if batch else 1)


REFUSED = [
    ('other', {}, {}, 'processor'),                                                           # any other processor list
    ('sampling', {}, {'sample_seed': None}, 'sample_seed'),                                   # do_sample without sample_seed
    ('penalty', {}, {'device_processors': False}, 'device_processors'),                       # ... =False together with processors
    ('plain', {}, {'output_scores': True}, 'scores'),
    ('plain', {'fresh_scores': True}, {'output_scores': True}, 'scores'),
    ('plain', {'decoding_length': 128}, {}, 'wider'),                                         # wide trees
    ('plain', {'device_trie': True}, {}, 'device trie'),
    ('plain', {'gather': 'GATHER'}, {}, 'gather'),                                            # sharded jobs
]


@pytest.mark.parametrize('which,dk_extra,kw,word', REFUSED)
@pytest.mark.parametrize('batch', [False, True], ids=['bs1', 'batch'])
def test_requests_that_would_take_the_host_walk_are_refused_before_any_engine_call(batch, which, dk_extra, kw, word):
    model = BModel(max_blocks=4) if batch else Model()
    dk_extra = {k: (_gather(batch) if v == 'GATHER' else v) for k, v in dk_extra.items()}
    with pytest.raises(ValueError, match='output_logprobs.*' + word):
        _call(model, batch, 'lookahead', which, dk_extra=dk_extra, **kw)
    assert model.engine.log == [] and model.engine.reads == []


@pytest.mark.parametrize('which,kw,word', [('other', {}, 'processor'), ('sampling', {'sample_seed': None}, 'sample_seed'),
                                           ('penalty', {'device_processors': False}, 'device_processors')])
@pytest.mark.parametrize('batch', [False, True], ids=['bs1', 'batch'])
def test_the_plain_front_doors_refuse_the_host_pick(batch, which, kw, word):
    model = BModel() if batch else Model()
    with pytest.raises(ValueError, match='output_logprobs.*' + word):
        _call(model, batch, 'plain', which, **kw)
    assert model.engine.log == []


@pytest.mark.parametrize('entry', ['lookahead', 'plain'])
@pytest.mark.parametrize('batch', [False, True], ids=['bs1', 'batch'])
def test_an_engine_without_the_stage_is_refused(batch, entry):
    eng = OracleBatchEngine(tiny_shape(), tiny_weights(0), max_length=256, n_slots=4) if batch else \
        OracleEngine(tiny_shape(), tiny_weights(0), max_length=256)
    model = BModel(engine=eng) if batch else Model(engine=eng)
    with pytest.raises(ValueError, match='output_logprobs.*engine'):
        _call(model, batch, entry, 'plain')


# ---------------------------------------------------------------------------------------------------------- the output shape
@pytest.mark.parametrize('entry', ['lookahead', 'plain'])
def test_bs1_returns_one_value_per_new_token(entry):
    model = Model()
    out = _call(model, False, entry, 'plain')
    seqs, lps = (out.sequences, out.kwargs['logprobs']) if entry == 'lookahead' else out
    n_new = seqs.shape[1] - len(PROMPT[0])
    assert n_new == N_NEW and model.engine.reads == [(0, len(PROMPT[0]), n_new)]
    assert lps == [float(len(PROMPT[0]) + i) for i in range(n_new)] and all(type(x) is float for x in lps)


@pytest.mark.parametrize('entry', ['lookahead', 'plain'])
@pytest.mark.parametrize('max_blocks', [0, 2], ids=['cursor-batch', 'multi-block'])
def test_batch_positions_are_unpadded_and_every_list_is_cut_at_its_own_stop(max_blocks, entry):
    P = len(B_IDS[0])
    ref = _call(BModel(max_blocks=max_blocks), True, entry, 'plain', logprobs=False)
    ref = (ref.sequences if entry == 'lookahead' else ref).tolist()
    PAD = next(t for t in range(1, 64) if all(t not in r[P:] for r in ref))      # a pad id greedy decoding never emits here
    # an eos that stops the two sequences at different lengths: a token sequence 0 emits early and sequence 1 does not emit at all
    eos = next((t for t in ref[0][P:P + 5] if t not in ref[1][P:]), None)
    assert eos is not None, 'the tiny model leaves no token to tell the two stops apart'
    model = BModel(max_blocks=max_blocks)
    out = _call(model, True, entry, 'plain', eos=eos, pad=PAD)
    seqs, lps = (out.sequences, out.kwargs['logprobs']) if entry == 'lookahead' else out
    seqs = seqs.tolist()
    n_new = [len([t for t in r[P:] if t != PAD]) for r in seqs]
    assert n_new[0] < n_new[1] == N_NEW, n_new
    assert sorted(model.engine.reads) == [(b, B_LEN[b], n_new[b]) for b in range(2)]
    assert lps == [[1000.0 * b + B_LEN[b] + i for i in range(n_new[b])] for b in range(2)]


def test_generate_carries_the_key_on_both_legs():
    for batch in (False, True):
        ids = torch.tensor(B_IDS if batch else PROMPT)
        extra = {'attention_mask': torch.tensor(B_AM)} if batch else {}
        for use_lookahead in (True, False):
            model = BModel() if batch else Model()
            out = model.generate(ids, max_new_tokens=N_NEW, pad_token_id=0, return_dict_in_generate=True,
                                 decoding_kwargs=dict(DK, use_lookahead=use_lookahead, output_logprobs=True), **extra)
            lps = out.kwargs['logprobs']
            assert len(lps if not batch else lps[0]) == N_NEW and model.engine.log[-1] == ('lp', False)
