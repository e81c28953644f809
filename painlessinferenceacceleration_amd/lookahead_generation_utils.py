# -*- coding: utf-8 -*-
"""API types of the lookahead path (mirror of lookahead/lookahead/common/lookahead_generation_utils.py:19-76) and the front end the
single-sequence and the batch loop share (pretrained_model.py, pretrained_model_batch.py): the device-stage scope, the host token
pick, the request prologue and the body of generate()."""
import gc
import warnings
from contextlib import contextmanager
from dataclasses import dataclass, field
from enum import Enum
from typing import Any, Dict, Optional, Tuple

import numpy as np
import torch


class GenerationMode(str, Enum):
    GREEDY_SEARCH = "greedy_search"
    LOOKAHEAD_GENERATION = "lookahead_generation"


class LookaheadGenerationConfig(object):
    """Mirror of LookaheadGenerationConfig(GenerationConfig) (lookahead_generation_utils.py:19-29): the lookahead fields with
    the reference's defaults, plus whatever generation fields the caller passes (max_new_tokens, eos_token_id, ...), which
    generate(generation_config=...) reads."""

    def __init__(self, **kwargs):
        self.use_lookahead = kwargs.pop('use_lookahead', False)
        self.debug_lookahead = kwargs.pop('debug_lookahead', False)
        self.decoding_length = kwargs.pop('decoding_length', 63)
        self.branch_length = kwargs.pop('branch_length', 12)
        self.decoding_mode = kwargs.pop('decoding_mode', 'hier')
        self.decoding_kwargs = kwargs.pop('decoding_kwargs', {})
        self.inputs_embeds_position = kwargs.pop('inputs_embeds_position', False)
        self.max_query_length = kwargs.pop('max_query_length', 2)
        self.stop_words = kwargs.pop('stop_words', None)
        self.tokenizer = kwargs.pop('tokenizer', None)
        for k, v in kwargs.items():            # max_new_tokens, max_length, eos_token_id, pad_token_id, do_sample, ...
            setattr(self, k, v)

    def to_decoding_kwargs(self) -> Dict[str, Any]:
        out = dict(self.decoding_kwargs or {})
        out.update({'use_lookahead': self.use_lookahead, 'debug_lookahead': self.debug_lookahead,
                    'decoding_mode': self.decoding_mode, 'decoding_length': self.decoding_length,
                    'branch_length': self.branch_length, 'max_query_length': self.max_query_length,
                    'stop_words': self.stop_words if self.stop_words is not None else {}, 'tokenizer': self.tokenizer})
        return out


@dataclass
class LookaheadDecoderOnlyOutput(object):
    """sequences + kwargs{dls, edls, fts, qts} (pretrained_model.py:1256-1266)."""
    sequences: Any = None
    scores: Optional[Tuple] = None
    attentions: Optional[Tuple] = None
    hidden_states: Optional[Tuple] = None
    kwargs: Dict[str, Any] = field(default_factory=dict)


def device_repetition_penalty(logits_processor, engine, do_sample=False, enabled=True):
    """The penalty value when the processor list can run as the engine's device stage (LlamaVerifyEngine.set_repetition_penalty), else
    None (-> the host walk).  The list must be exactly ONE transformers RepetitionPenaltyLogitsProcessor — the exact type, not a
    subclass (a subclass may override __call__) — whose optional attributes are at their defaults, so that `penalty` is its whole
    state; greedy decoding; an engine that has the stage (the oracle-backed CPU engines of the tests do not); and `enabled`
    (decoding_kwargs['device_processors'], default True: False is the A/B switch and escape hatch)."""
    if not enabled or do_sample or logits_processor is None or len(logits_processor) != 1:
        return None
    if not hasattr(engine, 'set_repetition_penalty'):
        return None
    from transformers import RepetitionPenaltyLogitsProcessor
    proc = logits_processor[0]
    if type(proc) is not RepetitionPenaltyLogitsProcessor:
        return None
    if any(getattr(proc, name, None) is not None for name in ('prompt_ignore_length', 'logits_indices', 'cu_seq_lens_q')):
        return None
    penalty = getattr(proc, 'penalty', None)
    if not isinstance(penalty, float) or not penalty > 0:
        return None
    return penalty


def device_sampling(logits_processor, engine, do_sample=False, seed=None, enabled=True):
    """The parameter set {'seed', 'temperature', 'top_k', 'top_p', 'penalty'} when a do_sample request can run as the engine's device
    stage (LlamaVerifyEngine.set_sampling: csrc/la_sample.hip), else None (-> the host walk, exactly as without this stage).  All of:
    `do_sample`; `seed` (decoding_kwargs['sample_seed']) an int — the stage is opt-in through that key; `enabled`
    (decoding_kwargs['device_processors'], default True); an engine that has the stage; and a list that is exactly
        [RepetitionPenaltyLogitsProcessor?] + [TemperatureLogitsWarper?, TopKLogitsWarper?, TopPLogitsWarper?]
    in that order, each the exact transformers type (a subclass may override __call__) with filter_value == -inf,
    min_tokens_to_keep == 1 and temperature > 0.  'penalty' is None without the processor; top_k 0 / top_p 1.0 mean off."""
    if not enabled or not do_sample or isinstance(seed, bool) or not isinstance(seed, int):
        return None
    if not hasattr(engine, 'set_sampling'):
        return None
    from transformers import RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    items = list(logits_processor) if logits_processor is not None else []
    out = {'seed': int(seed) & 0xFFFFFFFFFFFFFFFF, 'temperature': 1.0, 'top_k': 0, 'top_p': 1.0, 'penalty': None}
    if items and type(items[0]) is RepetitionPenaltyLogitsProcessor:
        penalty = device_repetition_penalty(items[:1], engine, do_sample=False, enabled=True)
        if penalty is None:
            return None
        out['penalty'] = penalty
        items = items[1:]
    order = (TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper)
    at = 0
    for proc in items:
        while at < 3 and type(proc) is not order[at]:
            at += 1
        if at == 3:                                  # not a warper of the three, out of order, or one type twice
            return None
        if at == 0:
            t = getattr(proc, 'temperature', None)
            if isinstance(t, bool) or not isinstance(t, (int, float)) or not t > 0:
                return None
            out['temperature'] = float(t)
        else:
            if getattr(proc, 'filter_value', None) != -float('inf') or getattr(proc, 'min_tokens_to_keep', 1) != 1:
                return None
            if at == 1:
                k = getattr(proc, 'top_k', None)
                if isinstance(k, bool) or not isinstance(k, int) or k < 1:
                    return None
                out['top_k'] = int(k)
            else:
                p = getattr(proc, 'top_p', None)
                if not isinstance(p, float) or not 0.0 <= p <= 1.0:
                    return None
                out['top_p'] = float(p)
        at += 1
    return out


def plan_device_stages(logits_processor, engine, eligible, do_sample=False, seed=None, enabled=True):
    """Which device stages serve this request: None (-> the host pick) or {'penalty': float | None, 'sampling': dict | None}, the
    answers of device_repetition_penalty / device_sampling with the sampling list's own penalty folded in.  `eligible`: the loop's
    own conditions (no scores, no wide tree, no sharded job, no device trie, ...), which differ between the loops."""
    if not eligible:
        return None
    penalty = device_repetition_penalty(logits_processor, engine, do_sample=do_sample, enabled=enabled)
    sampling = device_sampling(logits_processor, engine, do_sample=do_sample, seed=seed, enabled=enabled)
    if sampling is not None:
        penalty = sampling['penalty']
    if penalty is None and sampling is None:
        return None
    return {'penalty': penalty, 'sampling': sampling}


def plan_logprobs(requested, engine, host_walk, do_sample=False, seed=None, enabled=True, scores=False, wide=False,
                  device_trie=False, gather=False):
    """Whether this request returns per-token log-probabilities (decoding_kwargs['output_logprobs'] / output_logprobs=True): they are
    taken by a stage of the device step (LlamaVerifyEngine.set_logprobs: csrc/la_logprob.hip), so the request must run the device
    accept.  -> False when not requested; True when honoured; ValueError naming the condition when the request would take the host
    walk (`host_walk`: a processor list or sampling that plan_device_stages did not place on the device) or a step form without
    the stage.  Called before the loop's first engine call."""
    if not requested:
        return False
    why = None
    if not hasattr(engine, 'set_logprobs'):
        why = 'this engine has no log-probability stage'
    elif scores:
        why = 'output_scores / fresh_scores take the host walk'
    elif wide:
        why = 'trees wider than one 64-row block (decoding_length > 64) have no log-probability stage'
    elif device_trie:
        why = 'the device trie (device_trie=True) is not served'
    elif gather:
        why = "sharded jobs (decoding_kwargs['gather']) are not served"
    elif host_walk:
        if do_sample and (isinstance(seed, bool) or not isinstance(seed, int)):
            why = "do_sample without decoding_kwargs['sample_seed'] takes the host walk"
        elif not enabled:
            why = 'device_processors=False together with processors / sampling takes the host walk'
        else:
            why = 'this logits-processor list has no device stage and takes the host walk'
    if why is not None:
        raise ValueError(f'output_logprobs: {why}')
    return True


TOP_LOGPROBS_MAX = 20        # LA_TOPLP_MAX (include/lookahead_hip.h)


def plan_top_logprobs(requested, engine):
    """decoding_kwargs['top_logprobs'] / top_logprobs=n: how many alternatives per generated token the device step lists
    (LlamaVerifyEngine.set_top_logprobs: csrc/la_logprob.hip).  -> 0 when not requested, else n (1 .. 20); ValueError otherwise.  A
    request with n > 0 implies output_logprobs: hand `requested or n > 0` to plan_logprobs, which refuses the host-walk paths."""
    if requested is None or requested is False or (not isinstance(requested, bool) and requested == 0):
        return 0
    if isinstance(requested, bool) or not isinstance(requested, int) or not 1 <= requested <= TOP_LOGPROBS_MAX:
        raise ValueError(f'top_logprobs: an int 1 .. {TOP_LOGPROBS_MAX} (got {requested!r})')
    if not hasattr(engine, 'set_top_logprobs'):
        raise ValueError('top_logprobs: this engine has no top-N log-probability stage')
    return int(requested)


def read_top_logprobs(engine, slot, first_pos, n_pos):
    """the top-N log of one slot as the front doors return it: per position a list of n (token_id, logprob) pairs, most likely first"""
    ids, vals = engine.top_logprobs(slot, first_pos, n_pos)
    return [[(int(t), float(v)) for t, v in zip(ids[p], vals[p])] for p in range(n_pos)]


@contextmanager
def device_stages(engine, plan, slots, logprobs=False, top_logprobs=0):
    """The stages of `plan` (plan_device_stages; None: nothing) switched on for one request and off again, also after an exception:
    the next request starts without them.  slots: (slot, sampling stream word, token row the slot's penalty context is seeded
    with) per sequence — the batch loops seed with the padded row (what the reference's walk hands the processor); row None: the
    prefill seeds the context with the prompt itself.  logprobs (plan_logprobs): the log-probability stage, likewise; top_logprobs
    (plan_top_logprobs, only with logprobs): its top-N list, switched off before the scalar stage."""
    penalty, sampling = (None, None) if plan is None else (plan['penalty'], plan['sampling'])
    try:
        if logprobs:
            engine.set_logprobs(True)
            if top_logprobs:
                engine.set_top_logprobs(top_logprobs)
        if penalty is not None:
            engine.set_repetition_penalty(penalty)
            for slot, _, row in slots:
                if row is not None:
                    engine.seed_penalty_context(slot, row)
        if sampling is not None:
            for slot, stream, _ in slots:
                engine.sampling_stream(slot, stream)
            engine.set_sampling(True, sampling['seed'], sampling['temperature'], sampling['top_k'], sampling['top_p'])
        yield
    finally:
        if penalty is not None:
            engine.set_repetition_penalty(1.0)
        if sampling is not None:
            engine.set_sampling(False)
        if logprobs:
            try:
                if top_logprobs:
                    engine.set_top_logprobs(0)
            finally:
                engine.set_logprobs(False)


def pick_token(logits_processor, do_sample, ctx_ids, logits_row, device):
    """Next token from one logits row through the processor list (pretrained_model.py:833-839, pretrained_model_batch.py:840-846):
    -> (token, processed scores [1, vocab]).  The scores may alias the engine's logits buffer: a caller that keeps them clones."""
    sc = logits_row[None]
    if logits_processor is not None and len(logits_processor) > 0:
        sc = logits_processor(torch.tensor([ctx_ids], dtype=torch.long, device=device), sc.clone())
    if do_sample:
        return int(torch.multinomial(torch.softmax(sc.float(), dim=-1), num_samples=1)[0, 0]), sc
    return int(torch.argmax(sc, dim=-1)[0]), sc


def _parents_of(rowmask, T):
    """parent row of every tree row = highest set bit below the row over the concatenated ancestor words (DFS order)"""
    rm = np.asarray(rowmask, dtype=np.uint64)
    if rm.ndim == 1:
        rm = rm[:, None]
    parent = [-1] * T
    for j in range(1, T):
        below = 0
        for w in range(rm.shape[1]):
            below |= int(rm[j, w]) << (64 * w)
        below &= (1 << j) - 1
        parent[j] = below.bit_length() - 1
    return parent


def _max_length_of(stopping_criteria, max_length):
    if max_length is not None:
        warnings.warn("`max_length` is deprecated in this function, use "
                      "`stopping_criteria=StoppingCriteriaList([MaxLengthCriteria(max_length=max_length)])` instead.",
                      UserWarning)
        return int(max_length)
    if stopping_criteria is None:
        return None
    ml = getattr(stopping_criteria, 'max_length', None)
    if ml is None and isinstance(stopping_criteria, int):
        ml = stopping_criteria
    return None if ml is None else int(ml)


def _custom_stop(stopping_criteria):
    """The user's criteria besides MaxLengthCriteria as one predicate stop(token_row) -> bool, or None when there are none.
    The reference evaluates `stopping_criteria(input_ids, scores)` after every verify step (pretrained_model.py:1225-1226;
    batch: once per sample on input_ids[i:i+1, :cur+1], pretrained_model_batch.py:1284); scores = the tuple collected so far under
    output_scores, else None.  The length criterion itself is the `len(seq) >= max_length` test of the loops."""
    if stopping_criteria is None or isinstance(stopping_criteria, int) or not callable(stopping_criteria):
        return None
    try:
        crit = list(stopping_criteria)
    except TypeError:
        crit = [stopping_criteria]
    crit = [c for c in crit if type(c).__name__ != 'MaxLengthCriteria']
    if not crit:
        return None

    def stop(token_row, device='cpu', scores=None):
        ids = torch.tensor([list(token_row)], dtype=torch.long, device=device)
        for c in crit:
            r = c(ids, scores)
            if bool(r.any()) if torch.is_tensor(r) else bool(r):
                return True
        return False
    return stop


@contextmanager
def gc_paused():
    """The step loops run with the cyclic garbage collector paused: a generation-2 pass over torch's object graph stalls the host
    thread for tens of ms (measured 37 ms = 9 verify steps) and the loops create no reference cycles."""
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was_enabled:
            gc.enable()


def begin_request(model, logits_processor, stopping_criteria, max_length, pad_token_id, eos_token_id, output_attentions,
                  output_hidden_states, output_scores, return_dict_in_generate, model_kwargs):
    """What both lookahead_generation loops settle before they touch the engine: the processor list wrapped, whether it (or sampling)
    asks for the sequential accept path, pad / eos / return_dict_in_generate / output_scores resolved against the
    model's generation_config, the trie cache created and given its eos ids and stop words, the per-request lists of
    decoding_kwargs emptied and the length bound read.
    -> (logits_processor, sequential, pad_token_id, eos_token_id, return_dict_in_generate, scores, decoding_kwargs, stop_max_length);
    `scores` is () when the request returns scores (return_dict_in_generate and output_scores), else None."""
    if isinstance(logits_processor, (list, tuple)) and not callable(logits_processor):
        from transformers import LogitsProcessorList      # a plain list of processors: the reference's generate() wraps it the same way
        logits_processor = LogitsProcessorList(list(logits_processor))
    sequential = (logits_processor is not None and len(logits_processor) > 0) or \
        bool(model_kwargs.get('decoding_kwargs', {}).get('do_sample', False))
    if output_attentions or output_hidden_states:
        raise NotImplementedError('attentions / hidden_states are intermediates the device path never materialises '
                                  '(fused attention, activations in MFMA fragment order); scores are returned (output_scores)')
    cfg = model.generation_config
    pad_token_id = pad_token_id if pad_token_id is not None else getattr(cfg, 'pad_token_id', None)
    eos_token_id = eos_token_id if eos_token_id is not None else getattr(cfg, 'eos_token_id', None)
    if isinstance(eos_token_id, int):
        eos_token_id = [eos_token_id]
    return_dict_in_generate = bool(return_dict_in_generate) if return_dict_in_generate is not None \
        else bool(getattr(cfg, 'return_dict_in_generate', False))
    output_scores = bool(output_scores) if output_scores is not None else bool(getattr(cfg, 'output_scores', False))
    scores = () if (return_dict_in_generate and output_scores) else None
    if not hasattr(model, 'lookahead_cache') or model.lookahead_cache is None:
        from .lookahead_cache import LookaheadCache
        model.lookahead_cache = LookaheadCache()
    decoding_kwargs = model_kwargs['decoding_kwargs']
    model.lookahead_cache.eos_ids = eos_token_id
    model.lookahead_cache.stop_words = decoding_kwargs.get('stop_words', {})
    decoding_kwargs.update({'edls': [], 'dls': [], 'fts': [], 'qts': []})
    stop_max_length = _max_length_of(stopping_criteria, max_length)
    if stop_max_length is None:
        raise ValueError('lookahead_generation needs a MaxLengthCriteria (stopping_criteria.max_length)')
    return logits_processor, sequential, pad_token_id, eos_token_id, return_dict_in_generate, scores, decoding_kwargs, stop_max_length


# ---------------------------------------------------------------------------------------------------- generate() front door
_GEN_FIELDS = ('max_length', 'max_new_tokens', 'min_length', 'min_new_tokens', 'eos_token_id', 'pad_token_id', 'do_sample',
               'repetition_penalty', 'no_repeat_ngram_size', 'bad_words_ids', 'temperature', 'top_k', 'top_p', 'max_time',
               'return_dict_in_generate', 'output_scores')


@dataclass
class GenerateArgs(object):
    """What the reference's generate() derives before it dispatches to a decoding loop (pretrained_model.py:213-372)."""
    max_length: int = 0
    eos_token_id: Any = None
    pad_token_id: Any = None
    do_sample: bool = False
    return_dict_in_generate: bool = False
    output_scores: bool = False
    logits_processor: Any = None            # LogitsProcessorList: config-derived processors, then the caller's
    logits_warper: Any = None               # LogitsProcessorList of warpers (do_sample only)
    stopping_criteria: Any = None           # StoppingCriteriaList: MaxLengthCriteria (+ MaxTimeCriteria), then the caller's
    decoding_kwargs: Dict[str, Any] = field(default_factory=dict)


def _merge_lists(default_list, custom_list, what):
    """transformers' _merge_criteria_processor_list: the caller's objects go BEHIND the config-derived ones; passing an object of a
    type generate() already built from the configuration is an error there, and here."""
    if not custom_list:
        return default_list
    for d in default_list:
        for c in custom_list:
            if type(c) is type(d):
                raise ValueError(f'A custom {what} of type {type(c)} with values {c} has been passed to `generate`, but it has '
                                 f'already been created with the values {d}. {d} has been created by passing the corresponding '
                                 f'arguments to generate or by the model\'s config default values.')
    default_list.extend(custom_list)
    return default_list


def _on_device(cls, *args, device=None):
    """transformers >= 4.4x: the eos-aware processors keep their eos ids as a tensor created on `device` (default 'cpu') and compare
    it with the scores' vocabulary index — HF's _get_logits_processor passes device=input_ids.device; older releases take no such
    argument."""
    if device is not None:
        try:
            return cls(*args, device=device)
        except TypeError:
            pass
    return cls(*args)


def resolve_generate_args(model_generation_config, input_length, generation_config=None, logits_processor=None,
                          stopping_criteria=None, device=None, **kwargs):
    """The front half of the reference's generate() (common/pretrained_model.py:213-372) for the two modes this package serves.

    Precedence of every generation field: explicit keyword > `generation_config=` argument > the model's own generation_config
    (`generation_config.update(**kwargs)`, :229).  Then, in the reference's order:
      * pad_token_id defaults to the first eos id (:239-249);
      * max_length = max_new_tokens + prompt length when max_new_tokens is given (:325-336);
      * `_get_logits_processor` (:350-356): repetition_penalty, no_repeat_ngram_size, bad_words_ids, min_length, min_new_tokens —
        the transformers classes themselves, in transformers' order — then the caller's `logits_processor` list merged behind them;
      * `_get_stopping_criteria` (:359-361): MaxLengthCriteria, MaxTimeCriteria, then the caller's `stopping_criteria`;
      * warpers (temperature, top_k, top_p) are built for do_sample — the reference hands them to `sample()` only (:465-479); its
        LOOKAHEAD branch passes processors and criteria and NO warper (:428-441), and so does generate() here.
    `device`: where the logits rows handed to the processors live (the engine's device) — the eos-aware processors build their
    eos tensor there.
    Returns (GenerateArgs, leftover kwargs = model kwargs such as attention_mask)."""
    from transformers import (LogitsProcessorList, MaxLengthCriteria, MaxTimeCriteria, MinLengthLogitsProcessor,
                              MinNewTokensLengthLogitsProcessor, NoBadWordsLogitsProcessor, NoRepeatNGramLogitsProcessor,
                              RepetitionPenaltyLogitsProcessor, StoppingCriteriaList, TemperatureLogitsWarper, TopKLogitsWarper,
                              TopPLogitsWarper)
    val = {}
    for k in _GEN_FIELDS:
        if k in kwargs and kwargs[k] is not None:
            val[k] = kwargs.pop(k)
            continue
        kwargs.pop(k, None)
        v = getattr(generation_config, k, None) if generation_config is not None else None
        if v is None and k not in ('max_length', 'max_new_tokens'):          # the model's defaults never shorten an explicit budget
            v = getattr(model_generation_config, k, None) if model_generation_config is not None else None
        val[k] = v
    # decoding_kwargs: the keyword, else the config's (LookaheadGenerationConfig.to_decoding_kwargs / attributes, :232-233)
    dk = kwargs.pop('decoding_kwargs', None)
    if dk is None and generation_config is not None:
        if hasattr(generation_config, 'to_decoding_kwargs'):
            dk = generation_config.to_decoding_kwargs()
        else:
            dk = dict(getattr(generation_config, 'decoding_kwargs', {}) or {})
            for k in ('use_lookahead', 'debug_lookahead', 'decoding_length', 'branch_length', 'decoding_mode'):
                if hasattr(generation_config, k):
                    dk.setdefault(k, getattr(generation_config, k))
    dk = dict(dk or {})
    eos = val['eos_token_id']
    pad = val['pad_token_id']
    if pad is None and eos is not None:
        pad = eos[0] if isinstance(eos, (list, tuple)) else eos
    if val['max_new_tokens'] is not None:
        max_length = int(val['max_new_tokens']) + int(input_length)
    elif val['max_length'] is not None:
        max_length = int(val['max_length'])
    else:
        max_length = int(input_length) + 20
    eos_list = [eos] if isinstance(eos, int) else (list(eos) if eos is not None else None)
    procs = LogitsProcessorList()
    rp = val['repetition_penalty']
    if rp is not None and float(rp) != 1.0:
        procs.append(RepetitionPenaltyLogitsProcessor(penalty=float(rp)))
    if val['no_repeat_ngram_size'] is not None and int(val['no_repeat_ngram_size']) > 0:
        procs.append(NoRepeatNGramLogitsProcessor(int(val['no_repeat_ngram_size'])))
    if val['bad_words_ids'] is not None:
        procs.append(NoBadWordsLogitsProcessor(val['bad_words_ids'], eos_list))
    if val['min_length'] is not None and eos_list is not None and int(val['min_length']) > 0:
        procs.append(_on_device(MinLengthLogitsProcessor, int(val['min_length']), eos_list, device=device))
    if val['min_new_tokens'] is not None and eos_list is not None and int(val['min_new_tokens']) > 0:
        procs.append(_on_device(MinNewTokensLengthLogitsProcessor, int(input_length), int(val['min_new_tokens']), eos_list, device=device))
    procs = _merge_lists(procs, list(logits_processor) if logits_processor is not None else None, 'logits processor')
    warpers = LogitsProcessorList()
    if bool(val['do_sample']):
        if val['temperature'] is not None and float(val['temperature']) != 1.0:
            warpers.append(TemperatureLogitsWarper(float(val['temperature'])))
        if val['top_k'] is not None and int(val['top_k']) != 0:
            warpers.append(TopKLogitsWarper(top_k=int(val['top_k'])))
        if val['top_p'] is not None and float(val['top_p']) < 1.0:
            warpers.append(TopPLogitsWarper(top_p=float(val['top_p'])))
    crit = StoppingCriteriaList([MaxLengthCriteria(max_length=max_length)])
    if val['max_time'] is not None:
        crit.append(MaxTimeCriteria(max_time=float(val['max_time'])))
    crit = _merge_lists(crit, list(stopping_criteria) if stopping_criteria is not None else None, 'stopping criteria')
    ga = GenerateArgs(max_length=max_length, eos_token_id=eos, pad_token_id=pad, do_sample=bool(val['do_sample']),
                      return_dict_in_generate=bool(val['return_dict_in_generate']), output_scores=bool(val['output_scores']),
                      logits_processor=procs, logits_warper=warpers, stopping_criteria=crit, decoding_kwargs=dk)
    return ga, kwargs


def _get_generation_mode(decoding_kwargs):
    """pretrained_model.py:55-106 reduced to the two modes this path serves."""
    dk = decoding_kwargs or {}
    if dk.get('use_lookahead', False) and dk.get('decoding_length', 64) > 1 and dk.get('branch_length', 12) > 0:
        return GenerationMode.LOOKAHEAD_GENERATION
    return GenerationMode.GREEDY_SEARCH


def run_generate(model, batch, inputs, generation_config, logits_processor, stopping_criteria, prefix_allowed_tokens_fn,
                 assistant_model, streamer, kwargs):
    """The body of both generate() methods: resolve the arguments, then dispatch to model.lookahead_generation or
    model.greedy_search.  `batch`: the plain leg takes attention_mask / pad_token_id; the single-sequence model records
    dk['generation_mode'] and forwards output_scores to its lookahead loop, the batch model does neither."""
    from transformers import LogitsProcessorList
    if prefix_allowed_tokens_fn is not None or assistant_model is not None:
        raise NotImplementedError('prefix_allowed_tokens_fn / assistant_model: outside the lookahead path (SURVEY section 2, out of scope)')
    input_ids = inputs if inputs is not None else kwargs.pop('input_ids', None)
    kwargs.pop('input_ids', None)
    if input_ids is None:
        raise ValueError('generate() needs input_ids')
    ga, model_kwargs = resolve_generate_args(model.generation_config, input_ids.size(1), generation_config=generation_config,
                                             logits_processor=logits_processor, stopping_criteria=stopping_criteria,
                                             device=getattr(getattr(model, 'engine', None), 'device', None), **kwargs)
    attention_mask = model_kwargs.pop('attention_mask', None)
    dk = ga.decoding_kwargs
    if _get_generation_mode(dk) == GenerationMode.LOOKAHEAD_GENERATION:      # the loops feed the streamer themselves (prompt first, :318-319)
        dk['do_sample'] = ga.do_sample
        extra = {}
        if not batch:
            dk['generation_mode'] = GenerationMode.LOOKAHEAD_GENERATION
            extra['output_scores'] = ga.output_scores or None
        la_procs = ga.logits_processor
        if ga.do_sample and 'sample_seed' in dk:         # opt-in: the config-derived warpers reach the lookahead branch too
            la_procs = LogitsProcessorList(list(ga.logits_processor) + list(ga.logits_warper))
        return model.lookahead_generation(input_ids, logits_processor=la_procs if len(la_procs) else None,
                                          stopping_criteria=ga.stopping_criteria, pad_token_id=ga.pad_token_id,
                                          eos_token_id=ga.eos_token_id, return_dict_in_generate=ga.return_dict_in_generate,
                                          streamer=streamer, attention_mask=attention_mask, decoding_kwargs=dk, **extra)
    procs = LogitsProcessorList(list(ga.logits_processor) + list(ga.logits_warper))
    extra = {'attention_mask': attention_mask, 'pad_token_id': ga.pad_token_id if ga.pad_token_id is not None else 0} if batch else {}
    out = model.greedy_search(input_ids, ga.max_length, eos_token_id=ga.eos_token_id if ga.eos_token_id is not None
                              else getattr(model.generation_config, 'eos_token_id', None),
                              logits_processor=procs if len(procs) else None, do_sample=ga.do_sample,
                              stopping_criteria=ga.stopping_criteria, device_processors=dk.get('device_processors', True),
                              sample_seed=dk.get('sample_seed', None), output_logprobs=bool(dk.get('output_logprobs', False)), **extra,
                              **({'top_logprobs': dk['top_logprobs']} if dk.get('top_logprobs', 0) else {}))
    out_kwargs = {}
    if dk.get('top_logprobs', 0):                 # the plain leg's (sequences, logprobs, top_logprobs)
        out, out_kwargs['logprobs'], out_kwargs['top_logprobs'] = out
    elif dk.get('output_logprobs', False):        # the plain leg's (sequences, logprobs)
        out, out_kwargs['logprobs'] = out
    return LookaheadDecoderOnlyOutput(sequences=out, kwargs=out_kwargs) if ga.return_dict_in_generate else out
