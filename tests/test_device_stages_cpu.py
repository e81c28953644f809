# -*- coding: utf-8 -*-
"""CPU: the engine calls with which the four generation loops (bs=1 / batch x lookahead / plain) switch the device stages
(repetition penalty, sampling) on for one request and off again — which calls, with which arguments, in which order, and that an
exception mid-request leaves the same trail, teardown included.

The oracle engines get recording stubs for the four stage methods, so the loops take their "device" branch and run a plain greedy
accept.  Tokens are not asserted here (the stubs change nothing); only the call log is."""
from types import SimpleNamespace

import pytest
import torch

from painlessinferenceacceleration_amd.lookahead_cache import LookaheadCache
from painlessinferenceacceleration_amd.pretrained_model import LookaheadPreTrainedModel
from painlessinferenceacceleration_amd.pretrained_model_batch import LookaheadPreTrainedModel as BatchMixin
from tests.oracle_engine import OracleBatchEngine, OracleEngine
from tests.tiny_model import tiny_shape, tiny_weights

N_NEW = 8
PROMPT = [[5 + 3 * i for i in range(17)]]
B_IDS = [[0, 0, 5, 6, 7], [3, 4, 5, 6, 8]]
B_AM = [[0, 0, 1, 1, 1], [1, 1, 1, 1, 1]]
DK = {'use_lookahead': True, 'decoding_mode': 'hier', 'decoding_length': 64, 'branch_length': 12, 'stop_words': {}}


class _Stages(object):
    """recording stubs of the device-stage surface of LlamaVerifyEngine"""

    def set_repetition_penalty(self, penalty):
        self.log.append(('pen', penalty))

    def seed_penalty_context(self, slot, tokens):
        self.log.append(('seed', slot, list(tokens)))

    def sampling_stream(self, slot, stream_id):
        self.log.append(('stream', slot, stream_id))

    def set_sampling(self, enabled, *params):
        self.log.append(('samp', enabled) + params)


class RecordingEngine(_Stages, OracleEngine):
    def __init__(self, *a, **k):
        self.log = []
        super().__init__(*a, **k)
        del self.log[:]                     # the constructor's own reset

    def reset(self):
        self.log.append(('reset',))
        super().reset()

    def prefill(self, *a, **k):
        self.log.append(('prefill',))
        return super().prefill(*a, **k)


class RecordingBatchEngine(_Stages, OracleBatchEngine):
    def __init__(self, *a, **k):
        self.log = []
        super().__init__(*a, **k)
        del self.log[:]

    def reset_slot(self, slot):
        self.log.append(('reset_slot', slot))
        super().reset_slot(slot)

    def bprefill_many(self, *a, **k):
        self.log.append(('prefill',))
        return super().bprefill_many(*a, **k)


class Model(LookaheadPreTrainedModel):
    def __init__(self):
        self.engine = RecordingEngine(tiny_shape(), tiny_weights(0), max_length=256)
        self.generation_config = SimpleNamespace(eos_token_id=None, pad_token_id=0, return_dict_in_generate=False)
        self.lookahead_cache = LookaheadCache()


class BModel(BatchMixin):
    def __init__(self):
        self.engine = RecordingBatchEngine(tiny_shape(), tiny_weights(0), max_length=256, n_slots=4, max_blocks=0)
        self.generation_config = SimpleNamespace(eos_token_id=None, pad_token_id=0, return_dict_in_generate=False)
        self.lookahead_cache = LookaheadCache()


def _lists():
    from transformers import (LogitsProcessorList, RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper, TopKLogitsWarper)
    return {'sampling': LogitsProcessorList([RepetitionPenaltyLogitsProcessor(1.3), TemperatureLogitsWarper(0.8), TopKLogitsWarper(20)]),
            'greedy': LogitsProcessorList([RepetitionPenaltyLogitsProcessor(1.3)])}


def _criteria(max_length, raising):
    from transformers import MaxLengthCriteria, StoppingCriteria, StoppingCriteriaList

    class Boom(StoppingCriteria):
        def __call__(self, input_ids, scores, **kw):
            raise RuntimeError('boom')

    return StoppingCriteriaList([MaxLengthCriteria(max_length)] + ([Boom()] if raising else []))


def _run(batch, entry, which, raising, device_processors=True):
    """one request on a fresh model -> the engine's call log"""
    model = BModel() if batch else Model()
    procs = _lists()[which]
    sampling = which == 'sampling'
    ids = torch.tensor(B_IDS if batch else PROMPT)
    extra = {'attention_mask': torch.tensor(B_AM)} if batch else {}
    max_length = ids.shape[1] + N_NEW
    crit = _criteria(max_length, raising)

    def call():
        if entry == 'lookahead':
            dk = dict(DK, do_sample=sampling, device_processors=device_processors)
            if sampling:
                dk['sample_seed'] = 7
            model.lookahead_generation(ids, logits_processor=procs, stopping_criteria=crit, eos_token_id=[None], pad_token_id=0,
                                       decoding_kwargs=dk, **extra)
        else:
            model.greedy_search(ids, max_length, eos_token_id=None, logits_processor=procs, do_sample=sampling,
                                stopping_criteria=crit, device_processors=device_processors,
                                sample_seed=7 if sampling else None, **extra)

    if raising:
        with pytest.raises(RuntimeError, match='boom'):
            call()
    else:
        call()
    return model.engine.log


def _expected(batch, which):
    log = [('reset_slot', -1)] if batch else [('reset',)]
    log.append(('pen', 1.3))
    if batch:
        log += [('seed', 0, B_IDS[0]), ('seed', 1, B_IDS[1])]             # the PADDED rows; bs=1: prefill seeds the context itself
    if which == 'sampling':
        log += [('stream', 0, 0), ('stream', 1, 1)] if batch else [('stream', 0, 0)]
        log.append(('samp', True, 7, 0.8, 20, 1.0))
    log += [('prefill',), ('pen', 1.0)]
    if which == 'sampling':
        log.append(('samp', False))
    return log


@pytest.mark.parametrize('which', ['sampling', 'greedy'])
@pytest.mark.parametrize('entry', ['lookahead', 'plain'])
@pytest.mark.parametrize('batch', [False, True], ids=['bs1', 'batch'])
def test_stage_calls_of_a_request_and_of_one_that_raises(batch, entry, which):
    want = _expected(batch, which)
    assert _run(batch, entry, which, raising=False) == want
    assert _run(batch, entry, which, raising=True) == want


@pytest.mark.parametrize('entry', ['lookahead', 'plain'])
@pytest.mark.parametrize('batch', [False, True], ids=['bs1', 'batch'])
def test_device_processors_off_calls_no_stage_method(batch, entry):
    for which in ('sampling', 'greedy'):
        log = _run(batch, entry, which, raising=False, device_processors=False)
        assert not [c for c in log if c[0] in ('pen', 'seed', 'stream', 'samp')], log


@pytest.mark.parametrize('batch', [False, True], ids=['bs1', 'batch'])
def test_generate_reaches_the_same_stage_calls(batch):
    """through generate(): the configuration-derived processor and warpers (repetition_penalty, temperature, top_k) with
    decoding_kwargs['sample_seed'] give the log of the hand-built sampling list, on the lookahead and on the plain leg"""
    ids = torch.tensor(B_IDS if batch else PROMPT)
    extra = {'attention_mask': torch.tensor(B_AM)} if batch else {}
    for use_lookahead in (True, False):
        model = BModel() if batch else Model()
        dk = dict(DK, use_lookahead=use_lookahead, sample_seed=7)
        model.generate(ids, max_new_tokens=N_NEW, do_sample=True, repetition_penalty=1.3, temperature=0.8, top_k=20, pad_token_id=0,
                       decoding_kwargs=dk, **extra)
        assert model.engine.log == _expected(batch, 'sampling'), use_lookahead
