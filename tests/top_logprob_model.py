# -*- coding: utf-8 -*-
"""numpy model of the top-N log-probability stage (csrc/la_logprob.hip: k_top_logprob_rows; include/lookahead_hip.h "top-N
log-probabilities on the device"), the rows the unit tests run it on, and the recording engines of the planning tests.

Selection: the n largest stored logits of a row, compared through the monotone 16-bit key of the sampling stage (-0 == +0, NaN = key
0 = never listed), value descending, then token id ascending; ties at the cut go to the lowest ids.  Values: those of
tests/logprob_model.py (logprob_f64: the definition; logprob_intmass: the kernel's arithmetic) for every listed token."""
import numpy as np

from tests import logprob_model as lm

TOP_MAX = 20


def keys(rows, dtype):
    """uint32 keys of float32 values representable in `dtype` ('bfloat16' | 'float16'): unsigned order == value order"""
    x = np.ascontiguousarray(rows, dtype=np.float32)
    if dtype == 'float16':
        u = x.astype(np.float16).view(np.uint16).astype(np.uint32)
        inf = 0x7c00
    else:
        u = x.view(np.uint32) >> 16
        inf = 0x7f80
    mag = u & 0x7fff
    u = np.where(mag == 0, 0, u)
    key = np.where(u & 0x8000, ~u & 0xffff, u | 0x8000).astype(np.uint32)
    key[mag > inf] = 0
    return key


def top_ids(rows, dtype, n):
    """-> int32 [n_rows][n]: the listed tokens of every row in contract order (-1 past the row's last non-NaN logit)"""
    k = keys(rows, dtype).astype(np.int64)
    out = np.full((k.shape[0], n), -1, dtype=np.int32)
    ids = np.arange(k.shape[1])
    for r in range(k.shape[0]):
        order = np.lexsort((ids, -k[r]))[:n]            # primary: key descending; then id ascending
        order = order[k[r][order] > 0]
        out[r, :len(order)] = order
    return out


def top_model(rows, dtype, n, intmass=True):
    """-> (ids int32 [n_rows][n], fp64 values [n_rows][n], values of the kernel's arithmetic float32 [n_rows][n] or None).  The fp64
    values are logprob_model.logprob_f64's, column by column, with the row's log-sum-exp taken once."""
    ids = top_ids(rows, dtype, n)
    assert (ids >= 0).all()
    x = np.asarray(rows, dtype=np.float64)
    m = x.max(axis=1, keepdims=True)
    lse = np.log(np.exp(x - m).sum(axis=1, keepdims=True))
    f64 = (np.take_along_axis(x, ids.astype(np.int64), axis=1) - m) - lse
    im = np.stack([lm.logprob_intmass(rows, ids[:, j]) for j in range(n)], axis=1) if intmass else None
    return ids, f64, im


PLATEAU_IDS = (0, 7, 8, 8 * 1024 - 1, 8 * 1024, 8 * 4096 - 1, 8 * 4096)      # chunk, thread and round boundaries of the row scan


def planted_rows(vocab, dtype, n, n_rows=64, seed=0):
    """logprob_model.planted_rows (16 of them at least; rows 0 .. 7 as there: row 4 = all values equal, float16 rows 6 / 7 near
    +-60 000) with rows 8 .. 11 replaced by
       8   a plateau: g = n // 2 strictly larger values, then MORE than n - g logits tied at the cut, among them PLATEAU_IDS (those
           below vocab) and vocab - 1
       9   exactly n distinct large values at ascending ids in ASCENDING value (the list is sorted by value, not by id)
       10  +0 and -0 mixed at the cut, everything else negative
       11  the winner at vocab - 1
    -> float32 [n_rows][vocab] of values representable in `dtype`.  n_rows < 12 keeps the first rows."""
    rows, _ = lm.planted_rows(vocab, dtype, n_rows=max(n_rows, 16), seed=seed)
    rows = rows.copy()
    rng = np.random.default_rng(seed + 7 * vocab + n)
    g = n // 2
    special = sorted({i for i in PLATEAU_IDS if i < vocab} | {vocab - 1})
    # ---- 8: the plateau
    free = np.array([i for i in rng.permutation(vocab)[:64] if i not in special], dtype=np.int64)
    n_tied = max(n - g + 5, len(special))
    n_tied = min(n_tied, vocab - g)
    tied = special + free[:max(0, n_tied - len(special))].tolist()
    larger = [i for i in free[::-1] if i not in tied][:g]
    if len(larger) < g:                                  # a tiny vocabulary: take them from the plateau's own ids
        larger = larger + [i for i in tied if i not in (0, vocab - 1)][:g - len(larger)]
        tied = [i for i in tied if i not in larger]
    assert len(larger) == g and len(tied) > n - g
    rows[8, tied] = 20.0
    rows[8, larger] = 21.0 + np.arange(g)
    # ---- 9: n distinct values, ascending with the id
    at = np.sort(rng.permutation(vocab)[:n])
    rows[9, at] = 30.0 + np.arange(n)
    # ---- 10: signed zeros at the cut
    rows[10] = -np.abs(rows[10]) - 1.0
    zeros = rng.permutation(vocab)[:min(vocab, n + 6)]
    top = zeros[:g]
    rest = zeros[g:]
    rows[10, rest[0::2]] = 0.0
    rows[10, rest[1::2]] = -0.0
    rows[10, top] = 1.0 + np.arange(g)
    # ---- 11: the winner is the row's last token
    rows[11, vocab - 1] = rows[11].max() + 10.0
    return lm.round16(rows, dtype)[:n_rows]


# ---- recording engines of the planning tests (tests/test_top_logprobs_cpu.py)
class _TopStage(object):
    def set_top_logprobs(self, n):
        self.top_n = n
        self.log.append(('top', n))

    def top_logprobs(self, slot, first_pos, n_pos):
        """a ramp: entry j at position p of slot s is (token 100 j + p, value 1000 s + p - j)"""
        assert self.top_n > 0
        self.top_reads.append((slot, first_pos, n_pos))
        p = np.arange(first_pos, first_pos + n_pos)[:, None]
        j = np.arange(self.top_n)[None, :]
        return (100 * j + p).astype(np.int32), (1000.0 * slot + p - j).astype(np.float32)


class RecordingEngine(_TopStage, lm.RecordingEngine):
    def __init__(self, *a, **k):
        self.top_reads, self.top_n = [], 0
        super().__init__(*a, **k)


class RecordingBatchEngine(_TopStage, lm.RecordingBatchEngine):
    def __init__(self, *a, **k):
        self.top_reads, self.top_n = [], 0
        super().__init__(*a, **k)
