# -*- coding: utf-8 -*-
"""numpy models of the device log-probability stage (csrc/la_logprob.hip, include/lookahead_hip.h "log-probabilities on the
device"), the rows the unit tests run it on, and the recording engines of the planning tests.

    lp = (x_t - m) - log(sum_v exp(x_v - m))        x = the stored 16-bit logits widened, m = the row maximum

logprob_f64: the definition in float64 — the reference every bound is stated against.
logprob_intmass: the arithmetic of the kernel — fp32 differences, fp32 exp, q_v = floor(exp * 2^32) summed as INTEGERS (order-
independent), lp = fp32(x_t - m) - fp32(log(fp32(Z * 2^-32))).  Against the definition: <= V * 2^-32 (V floors against Z >= 2^32,
the maximum's own term) + 2^-22 |lp| (the fp32 roundings of the two subtractions)."""
import numpy as np

from tests.oracle_engine import OracleBatchEngine, OracleEngine


def round16(x, dtype):
    """float array rounded (nearest even) to the 16-bit storage type, as float32"""
    x = np.asarray(x, dtype=np.float32)
    if dtype == 'float16':
        return x.astype(np.float16).astype(np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32)


def logprob_f64(rows, toks):
    x = np.asarray(rows, dtype=np.float64)
    m = x.max(axis=1, keepdims=True)
    lse = np.log(np.exp(x - m).sum(axis=1))
    r = np.arange(x.shape[0])
    return (x[r, toks] - m[:, 0]) - lse


def logprob_intmass(rows, toks):
    x = np.asarray(rows, dtype=np.float32)
    m = x.max(axis=1, keepdims=True)
    e = np.exp(x - m)                                                   # fp32
    q = np.floor(e.astype(np.float64) * 4294967296.0).astype(np.uint64)
    z = q.sum(axis=1, dtype=np.uint64)
    lse = np.log((z.astype(np.float64) / 4294967296.0).astype(np.float32))      # fp32 log of an fp32 argument
    r = np.arange(x.shape[0])
    return ((x[r, toks] - m[:, 0]).astype(np.float32) - lse.astype(np.float32)).astype(np.float32)


def bound_intmass(vocab, lp):
    """the integer-mass form against the definition (module docstring)"""
    return vocab * 2.0 ** -32 + 2.0 ** -22 * np.abs(lp)


def bound_device(lp):
    """the kernel against the definition: bound_intmass at the largest vocabulary served (152 064 * 2^-32 = 3.5e-5) plus a margin for
    the ulps of expf / logf"""
    return 1e-4 + 2.0 ** -22 * np.abs(lp)


def planted_rows(vocab, dtype, n_rows=64, seed=0):
    """-> (rows float32 [n_rows][vocab] of values representable in `dtype`, tokens int32 [n_rows]).  N(0, 2) rows (variance 2) with a
    random target each, except the planted ones, in this order: target at index 0; target at vocab - 1; one logit 30 above the rest,
    that logit the target (lp ~ 0); the same with the row's LOWEST logit the target (far down); all values equal (lp = -log V); a
    row shifted to ~ -200; float16 only: values near +-60 000, a high and a low target.  n_rows < the planted count keeps the
    first rows."""
    rng = np.random.default_rng(seed + vocab)
    n_all = max(n_rows, 8)
    rows = rng.normal(0.0, np.sqrt(2.0), size=(n_all, vocab)).astype(np.float32)
    toks = rng.integers(0, vocab, size=n_all).astype(np.int32)
    toks[0], toks[1] = 0, vocab - 1
    peak = int(rng.integers(1, vocab - 1))
    rows[2, peak] = rows[2].max() + 30.0
    toks[2] = peak
    rows[3] = rows[2]
    toks[3] = int(np.argmin(rows[3]))
    rows[4] = 1.5
    rows[5] -= 200.0
    if dtype == 'float16':
        sign = np.where(rng.random(vocab) < 0.5, -1.0, 1.0).astype(np.float32)
        rows[6] = sign * 60000.0 + 32.0 * rows[6]
        rows[7] = rows[6]
        toks[6] = int(np.argmax(rows[6]))
        toks[7] = int(np.argmin(rows[7]))
    return round16(rows, dtype)[:n_rows], toks[:n_rows]


# ---- recording engines of the planning tests (tests/test_logprobs_cpu.py): the oracle engines + stubs of the device-stage surface
class _Stages(object):
    def set_repetition_penalty(self, penalty):
        self.log.append(('pen', penalty))

    def seed_penalty_context(self, slot, tokens):
        self.log.append(('seed', slot, list(tokens)))

    def sampling_stream(self, slot, stream_id):
        self.log.append(('stream', slot, stream_id))

    def set_sampling(self, enabled, *params):
        self.log.append(('samp', enabled) + params)

    def set_logprobs(self, enabled):
        self.log.append(('lp', enabled))

    def logprobs(self, slot, first_pos, n):
        """a ramp: the value at position p of slot s is 1000 s + p"""
        self.reads.append((slot, first_pos, n))
        return (1000.0 * slot + np.arange(first_pos, first_pos + n)).astype(np.float32)


class RecordingEngine(_Stages, OracleEngine):
    def __init__(self, *a, **k):
        self.log, self.reads, self.boom_at = [], [], None
        super().__init__(*a, **k)
        del self.log[:]                     # the constructor's own reset

    def reset(self):
        self.log.append(('reset',))
        super().reset()

    def prefill(self, *a, **k):
        self.log.append(('prefill',))
        return super().prefill(*a, **k)

    def step(self, *a, **k):
        if self.boom_at == 'step':
            raise RuntimeError('boom')
        return super().step(*a, **k)


class RecordingBatchEngine(_Stages, OracleBatchEngine):
    def __init__(self, *a, **k):
        self.log, self.reads, self.boom_at, self._prefilling = [], [], None, False
        super().__init__(*a, **k)
        del self.log[:]

    def reset_slot(self, slot):
        self.log.append(('reset_slot', slot))
        super().reset_slot(slot)

    def bprefill_many(self, *a, **k):
        self.log.append(('prefill',))
        self._prefilling = True
        try:
            return super().bprefill_many(*a, **k)
        finally:
            self._prefilling = False

    def mprefill_many(self, *a, **k):
        self.log.append(('prefill',))
        self._prefilling = True
        try:
            return super().mprefill_many(*a, **k)
        finally:
            self._prefilling = False

    def bstep(self, *a, **k):
        if self.boom_at == 'step' and not self._prefilling:
            raise RuntimeError('boom')
        return super().bstep(*a, **k)

    def mstep(self, *a, **k):
        if self.boom_at == 'step' and not self._prefilling:
            raise RuntimeError('boom')
        return super().mstep(*a, **k)
