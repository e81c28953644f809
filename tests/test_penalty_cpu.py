# -*- coding: utf-8 -*-
"""CPU: the host side of the device repetition penalty (csrc/la_penalty.hip).

1. The set argument the device stage rests on: on every tree row the host walk reaches, the context it hands the processor
   (seq + next_tokens) is, AS A SET, set(seq) + the tokens at the set bits of that row's ancestor mask — for the hier, par and
   one layouts of the native trie.  So the penalised argmax of a row can be taken before the walk.
2. A numpy model of the row stage (context set from the bitmap + rowmask, penalty, lowest-index argmax) followed by the unchanged
   accept walk emits what the sequential host walk with transformers' RepetitionPenaltyLogitsProcessor emits.
3. Which processor lists take the device stage (device_repetition_penalty): exactly one RepetitionPenaltyLogitsProcessor of the
   exact type, defaults everywhere, greedy, an engine that has the stage, and the device_processors switch.
4. The new C entry points validate their arguments without a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import llama_oracle as lo
from painlessinferenceacceleration_amd import _lib
from painlessinferenceacceleration_amd.lookahead_cache import LookaheadCache
from painlessinferenceacceleration_amd.lookahead_generation_utils import device_repetition_penalty
from painlessinferenceacceleration_amd.pretrained_model import _pack_rows, _parents_of

VOCAB = 40          # small: repeats are frequent, so contexts and path sets overlap in every way


def _warm_trie(rs, n_seq=30, length=40):
    cache = LookaheadCache(eos_ids=[None])
    seqs = []
    for _ in range(n_seq):
        s = rs.randint(3, VOCAB, size=length).tolist()
        seqs.append(s)
        cache.put(s, branch_length=13, mode='output', idx=-1)
    return cache, seqs


def _draft(cache, fmt, qids, decoding_length=64, branch_length=12):
    """(ids, rowmask uint64[T]) of one layout, as pretrained_model.lookahead_prepare_inputs_for_generation builds them"""
    if fmt == 'hier':
        ids, rowmask, _, _ = cache.hier_get_packed(qids, decoding_length=decoding_length, branch_length=branch_length,
                                                   min_input_size=0, min_output_size=max(decoding_length // 2, 1), mode='mix', idx=0)
        return np.asarray(ids, dtype=np.int32), np.asarray(rowmask, dtype=np.uint64)
    lst, mask, _ = getattr(cache, fmt + '_get')(qids, decoding_length=decoding_length, branch_length=branch_length,
                                                min_input_size=0, min_output_size=max(decoding_length // 2, 1), mode='mix', idx=0)
    if len(lst) == 0:
        return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.uint64)
    return np.asarray(lst, dtype=np.int32), np.atleast_1d(_pack_rows(mask, None))


def _host_walk(seq, ids, rowmask, pick):
    """the sequential walk of pretrained_model._lookahead_generation; pick(context, row) -> token.  -> (tokens, rows)"""
    T = len(ids)
    parent = _parents_of(rowmask, T)
    cur, live, rows, next_tokens = 0, {0}, [0], []
    while True:
        t = pick(seq + next_tokens, cur)
        next_tokens.append(t)
        nxt = [j for j in range(1, T) if parent[j] in live and int(ids[j]) == t]
        if not nxt:
            break
        cur, live = nxt[0], set(nxt)
        rows.append(cur)
    return next_tokens, rows


def _path_tokens(ids, rowmask, r):
    return {int(ids[a]) for a in range(len(ids)) if (int(rowmask[r]) >> a) & 1}


@pytest.mark.parametrize('fmt', ['hier', 'par', 'one'])
def test_context_of_a_reached_row_is_the_seeded_set_plus_its_ancestor_tokens(fmt):
    rs = np.random.RandomState(7)
    cache, seqs = _warm_trie(rs)
    reached, deep = 0, 0
    for case in range(200):
        s = seqs[rs.randint(len(seqs))]
        cut = rs.randint(2, len(s) - 14)
        seq = rs.randint(3, VOCAB, size=rs.randint(1, 6)).tolist() + s[:cut]        # the context so far; its tail is in the trie
        ids, rowmask = _draft(cache, fmt, seq[-2:])
        if len(ids) == 0:
            continue
        assert int(ids[0]) == seq[-1]
        truth = s[cut:]

        def pick(ctx, row, _state={'k': 0}):
            assert set(ctx) == set(seq) | _path_tokens(ids, rowmask, row), (fmt, case, row)
            k = len(ctx) - len(seq)
            # mostly follow the stored continuation (long walks), sometimes leave the tree
            return int(truth[k]) if k < len(truth) and rs.rand() < 0.9 else int(rs.randint(3, VOCAB))

        toks, rows = _host_walk(seq, ids, rowmask, pick)
        reached += len(rows)
        deep = max(deep, len(rows))
    assert reached > 300 and deep >= 5, (reached, deep)          # the walks did go down the trees


def _row_stage(logits, ctx_bits, ids, rowmask, p):
    """numpy model of k_pen_argmax: per row, members = seeded set + path tokens; penalise in the storage type; lowest-index argmax"""
    out = []
    for r in range(len(ids)):
        member = ctx_bits.copy()
        for a in range(len(ids)):
            if (int(rowmask[r]) >> a) & 1:
                member[int(ids[a])] = True
        x = logits[r]
        pen = torch.where(x < 0, x * p, x / p)
        sc = torch.where(torch.from_numpy(member), pen, x)
        out.append(int(torch.argmax(sc)))
    return out


@pytest.mark.parametrize('fmt', ['hier', 'par', 'one'])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_row_stage_then_plain_accept_walk_equals_the_sequential_host_walk(fmt, dtype):
    """penalised argmax of every row, then the UNCHANGED accept walk (oracle accept_scan = accept_walk of csrc/la_kernels.hip)
    == the host walk that calls transformers' processor token by token"""
    from transformers import LogitsProcessorList, RepetitionPenaltyLogitsProcessor
    rs = np.random.RandomState(11)
    cache, seqs = _warm_trie(rs)
    multi = 0
    for case in range(60):
        p = float(rs.choice([1.05, 1.3, 2.0, 0.8]))
        procs = LogitsProcessorList([RepetitionPenaltyLogitsProcessor(p)])
        s = seqs[rs.randint(len(seqs))]
        cut = rs.randint(2, len(s) - 14)
        seq = s[:cut]
        ids, rowmask = _draft(cache, fmt, seq[-2:])
        if len(ids) == 0:
            continue
        T = len(ids)
        # coarse logits: ties after the rounding are the rule, and the stored continuation is usually among the maxima
        logits = torch.from_numpy(rs.randint(-3, 4, size=(T, VOCAB)).astype(np.float32)).to(dtype)
        parent = _parents_of(rowmask, T)
        for r in range(T):
            kids = [j for j in range(1, T) if parent[j] == r]
            if kids and rs.rand() < 0.8:
                logits[r, int(ids[kids[rs.randint(len(kids))]])] = 6.0

        def pick(ctx, row):
            sc = procs(torch.tensor([ctx], dtype=torch.long), logits[row][None].clone())
            return int(torch.argmax(sc, dim=-1)[0])

        want_toks, want_rows = _host_walk(seq, ids, rowmask, pick)
        bits = np.zeros(VOCAB, dtype=bool)
        bits[seq] = True
        am = _row_stage(logits, bits, ids, rowmask, p)
        mask = np.array([[(int(rowmask[i]) >> j) & 1 for j in range(T)] for i in range(T)], dtype=np.int64)
        toks, rows = lo.accept_scan(ids.tolist(), mask, am)
        assert list(toks) == want_toks and list(rows) == want_rows, (fmt, case)
        multi += len(rows) > 1
    assert multi >= 10, multi


class _Eng(object):
    def set_repetition_penalty(self, p):
        pass


def test_which_processor_lists_take_the_device_stage():
    from transformers import LogitsProcessorList, NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor

    class Sub(RepetitionPenaltyLogitsProcessor):
        pass

    eng = _Eng()
    one = LogitsProcessorList([RepetitionPenaltyLogitsProcessor(1.05)])
    assert device_repetition_penalty(one, eng) == 1.05
    assert device_repetition_penalty([RepetitionPenaltyLogitsProcessor(0.8)], eng) == 0.8          # p < 1 is legal
    assert device_repetition_penalty(one, eng, enabled=False) is None                               # device_processors=False
    assert device_repetition_penalty(one, eng, do_sample=True) is None
    assert device_repetition_penalty(one, object()) is None                                        # an engine without the stage
    assert device_repetition_penalty(None, eng) is None and device_repetition_penalty(LogitsProcessorList(), eng) is None
    assert device_repetition_penalty(LogitsProcessorList([Sub(1.05)]), eng) is None                # exact type only
    two = LogitsProcessorList([RepetitionPenaltyLogitsProcessor(1.05), NoRepeatNGramLogitsProcessor(3)])
    assert device_repetition_penalty(two, eng) is None
    assert device_repetition_penalty(LogitsProcessorList([NoRepeatNGramLogitsProcessor(3)]), eng) is None
    import inspect
    if 'prompt_ignore_length' in inspect.signature(RepetitionPenaltyLogitsProcessor.__init__).parameters:
        ign = LogitsProcessorList([RepetitionPenaltyLogitsProcessor(1.05, prompt_ignore_length=4)])
        assert device_repetition_penalty(ign, eng) is None                                         # more state than `penalty`


def test_host_loop_keeps_the_host_walk_on_an_engine_without_the_stage():
    """the oracle-backed CPU engine of the host-loop tests has no set_repetition_penalty: the loops test with hasattr"""
    from tests.oracle_engine import OracleEngine
    assert not hasattr(OracleEngine, 'set_repetition_penalty')


def test_penalty_entry_points_validate_arguments_without_a_gpu():
    lib = _lib.lib
    buf = C.create_string_buffer(64)
    p = C.cast(buf, C.c_void_p)
    assert lib.la_llama_set_repetition_penalty(None, None, 1.05) == -1
    assert lib.la_llama_penalty_seed(None, None, 0, None, 0) == -1
    assert lib.la_llama_penalty_launches(None) == -1
    assert lib.la_penalty_argmax(None, None, 512, 1, p, p, p, p, p) == -1                  # null logits
    assert lib.la_penalty_argmax(None, p, 500, 1, p, p, p, p, p) == -1                     # vocab % 32
    assert lib.la_penalty_argmax(None, p, 512, 65, p, p, p, p, p) == -1                    # rows > 64
    assert lib.la_penalty_argmax(None, p, 32 * 20000, 1, p, p, p, p, p) == -1              # bitmap larger than the LDS
    assert lib.la_penalty_transform(None, None, 4, p, p) == -1
