# -*- coding: utf-8 -*-
"""The host protocol of the multi-block step (mstep / tstep / mstep_trees / mstep_trie / the three commits) without a GPU: an engine
shell (LlamaVerifyEngine.__new__, unpinned host blocks, a fake stream and a fake library that records what it is handed and answers
with a canned LA_MOUT_* header).  The expected input words are built HERE from the layout documented in include/lookahead_hip.h
(LA_MIN_* / LA_MOUT_*), not from engine code."""
import ctypes as C

import numpy as np
import pytest
import torch

from painlessinferenceacceleration_amd import _lib
from painlessinferenceacceleration_amd.llama_engine import LlamaVerifyEngine

# include/lookahead_hip.h, "Multi-block step"
MB_MAX = 8
MIN_NBLK, MIN_BLK, MIN_IDS, MIN_ROWMASK, MIN_XMASK, MIN_WORDS = 0, 4, 36, 548, 1572, 4644
TREE_PIECE, TOKS = 3, 40
MOUT_NOUT, MOUT_NKEYS, MOUT_OUTTOK, MOUT_T, MOUT_DST = 0, 8, 24, 344, 352
CAPACITY = 512
FULL = 0xFFFFFFFFFFFFFFFF


def test_layout_constants_are_the_headers():
    assert (_lib.LA_MB_MAX, _lib.LA_MIN_NBLK, _lib.LA_MIN_BLK, _lib.LA_MIN_IDS, _lib.LA_MIN_ROWMASK, _lib.LA_MIN_XMASK,
            _lib.LA_MIN_WORDS) == (MB_MAX, MIN_NBLK, MIN_BLK, MIN_IDS, MIN_ROWMASK, MIN_XMASK, MIN_WORDS)
    assert (_lib.LA_MODE_TREE_PIECE, _lib.LA_MOUT_TOKS, _lib.LA_MOUT_NOUT, _lib.LA_MOUT_NKEYS, _lib.LA_MOUT_OUTTOK, _lib.LA_MOUT_T,
            _lib.LA_MOUT_DST) == (TREE_PIECE, TOKS, MOUT_NOUT, MOUT_NKEYS, MOUT_OUTTOK, MOUT_T, MOUT_DST)


def canned_header(seed):
    """a result header: 1..40 tokens per block, keys per slot, draft lengths"""
    rs = np.random.RandomState(seed)
    o = np.zeros(MOUT_DST, dtype=np.int32)
    o[MOUT_NOUT:MOUT_NOUT + 8] = rs.randint(1, TOKS + 1, size=8)
    o[MOUT_NKEYS:MOUT_NKEYS + 16] = rs.randint(1, CAPACITY, size=16)
    o[MOUT_OUTTOK:MOUT_OUTTOK + 8 * TOKS] = rs.randint(3, 32000, size=8 * TOKS)
    o[MOUT_T:MOUT_T + 8] = rs.randint(1, 65, size=8)
    return o


def header_tokens(o, b):
    return o[MOUT_OUTTOK + TOKS * b:MOUT_OUTTOK + TOKS * b + int(o[MOUT_NOUT + b])].tolist()


class FakeStream(object):
    cuda_stream = 0

    def __init__(self):
        self.syncs = 0

    def synchronize(self):
        self.syncs += 1


class FakeLib(object):
    """la_llama_mstep / _eager / _trie / mcommit: record the arguments, snapshot the input block, answer with the next canned header"""

    def __init__(self, eng):
        self.eng, self.calls, self.answers = eng, [], []

    def _answer(self, out_ptr):
        assert out_ptr == self.eng.host_mout.data_ptr()
        self.eng._mout_np[:] = self.answers.pop(0)
        return 0

    def _step(self, name, h, sp, in_ptr, out_ptr):
        assert h == self.eng._h and isinstance(sp, C.c_void_p) and in_ptr == self.eng.host_min.data_ptr()
        self.calls.append((name, self.eng._min_np.copy()))
        return self._answer(out_ptr)

    def la_llama_mstep(self, h, sp, in_ptr, out_ptr):
        return self._step('mstep', h, sp, in_ptr, out_ptr)

    def la_llama_mstep_eager(self, h, sp, in_ptr, out_ptr):
        return self._step('mstep_eager', h, sp, in_ptr, out_ptr)

    def la_llama_mstep_trie(self, h, sp, nb, slots, limits, last, ids_ptr, rm_ptr, n_ptr, out_ptr):
        assert h == self.eng._h
        self.calls.append(('mstep_trie', nb, list(slots), list(limits), list(last), ids_ptr.value, rm_ptr.value, n_ptr.value))
        return self._answer(out_ptr)

    def la_llama_mcommit(self, h, sp, nb, keep, out_ptr):
        assert h == self.eng._h
        self.calls.append(('mcommit', nb, np.ctypeslib.as_array(keep, shape=(64 * nb,)).copy()))
        return self._answer(out_ptr)

    def la_llama_destroy(self, h):
        pass


def make_engine(slot_keys=(100, 200, 300, 350), n_keys=17):
    eng = LlamaVerifyEngine.__new__(LlamaVerifyEngine)
    eng.host_min = torch.zeros(MIN_WORDS, dtype=torch.int32)
    eng.host_mout = torch.zeros(MOUT_DST, dtype=torch.int32)
    eng._min_np = eng.host_min.numpy()
    eng._mout_np = eng.host_mout.numpy()
    eng._min_np[:] = 0x5A5A5A5A                      # stale words of an earlier pass: zeros must be WRITTEN
    eng._min_rm = eng._min_np[MIN_ROWMASK:MIN_ROWMASK + 2 * 64 * MB_MAX].view(np.uint64)
    eng._min_xm = eng._min_np[MIN_XMASK:MIN_XMASK + 2 * 3 * 64 * MB_MAX].view(np.uint64).reshape(MB_MAX * 64, 3)
    eng.n_slots, eng.max_blocks = 4, 8
    eng.slot_keys, eng.n_keys = list(slot_keys), n_keys
    eng.kv_ring, eng.max_keys, eng.max_pos = False, CAPACITY, CAPACITY + 64
    eng.stream = FakeStream()
    eng._h = 7
    eng._lib = FakeLib(eng)
    return eng


def random_tree(rs, T, W):
    """ids int32[T], masks uint64[T][W] with arbitrary bits (the codec copies words; it does not interpret them)"""
    ids = rs.randint(3, 32000, size=T).astype(np.int32)
    rm = (rs.randint(0, 1 << 32, size=(T, W)).astype(np.uint64) << np.uint64(32)) | rs.randint(0, 1 << 32, size=(T, W)).astype(np.uint64)
    return ids, rm


def expected_blocks(trees):
    """trees: (slot, ids[T], masks [T][W], mode, limit word) -> per block (table entry, ids, own-block words, ancestor words [n][p]):
    rows 64 p .. 64 p + 63 of a tree are its block p; block 0 runs in `mode`, the others as LA_MODE_TREE_PIECE; word w of a row's mask
    covers tree columns 64 w ...: word p is the block's own LA_MIN_ROWMASK word, words q < p its LA_MIN_XMASK words; a mask with
    fewer words than the tree has blocks stands for zeros"""
    out = []
    for slot, ids, rm, mode, lim in trees:
        T, W = len(ids), rm.shape[1]
        for p in range((T + 63) // 64):
            rows = slice(64 * p, min(T, 64 * p + 64))
            n = rows.stop - rows.start
            own = rm[rows, p] if p < W else np.zeros(n, dtype=np.uint64)
            anc = np.zeros((n, p), dtype=np.uint64)
            for q in range(min(p, W)):
                anc[:, q] = rm[rows, q]
            out.append(((slot, n, mode if p == 0 else TREE_PIECE, lim), ids[rows], own, anc))
    return out


def check_input_block(words, blocks):
    assert words[MIN_NBLK] == len(blocks)
    for b, (entry, ids, own, anc) in enumerate(blocks):
        n = entry[1]
        assert tuple(words[MIN_BLK + 4 * b:MIN_BLK + 4 * b + 4]) == entry, b
        assert words[MIN_IDS + 64 * b:MIN_IDS + 64 * b + n].tolist() == ids.tolist(), b
        rm = words[MIN_ROWMASK + 2 * 64 * b:MIN_ROWMASK + 2 * 64 * (b + 1)].view(np.uint64)
        assert rm[:n].tolist() == own.tolist(), b
        xm = words[MIN_XMASK + 2 * 3 * 64 * b:MIN_XMASK + 2 * 3 * 64 * (b + 1)].view(np.uint64).reshape(64, 3)
        assert xm[:n, :anc.shape[1]].tolist() == anc.tolist(), b


def check_keys(eng, header, slots, before_keys, before_n_keys):
    """slot_keys of the slots that took part come from the header; the others, and n_keys unless slot 0 took part, stay"""
    for s in range(eng.n_slots):
        assert eng.slot_keys[s] == (int(header[MOUT_NKEYS + s]) if s in slots else before_keys[s]), s
    assert eng.n_keys == (int(header[MOUT_NKEYS]) if 0 in slots else before_n_keys)


# ---- mstep ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('slots,eager', [((2,), False), ((0,), True), ((1, 3, 2), False), ((3, 0, 1), True)])
def test_mstep_blocks(slots, eager):
    eng, rs = make_engine(), np.random.RandomState(len(slots))
    hdr = canned_header(1)
    eng._lib.answers.append(hdr)
    blocks = []
    for i, s in enumerate(slots):
        ids, rm = random_tree(rs, (64, 1, 37)[i], 1)
        blocks.append((s, ids, rm[:, 0], 0 if i != 1 else 2, (16, 0, 99)[i]))
    keys, nk = list(eng.slot_keys), eng.n_keys
    out = eng.mstep(blocks, eager=eager)
    (name, words), = eng._lib.calls
    assert name == ('mstep_eager' if eager else 'mstep')
    check_input_block(words, expected_blocks([(s, ids, rm[:, None], mode, max(1, min(TOKS, lim))) for s, ids, rm, mode, lim in blocks]))
    assert out == [header_tokens(hdr, b) for b in range(len(slots))]
    check_keys(eng, hdr, slots, keys, nk)
    assert eng._mstep_slots == list(slots) and eng.stream.syncs == 1


def test_mstep_prefill_chain_of_one_slot():
    eng, rs = make_engine(), np.random.RandomState(7)
    hdr = canned_header(2)
    eng._lib.answers.append(hdr)
    ids = rs.randint(3, 32000, size=69).astype(np.int32)
    chain = LlamaVerifyEngine._CHAIN
    assert chain[0] == 1 and chain[5] == 63 and chain[63] == FULL
    blocks = [(1, ids[:64], chain[:64], 1, 1), (1, ids[64:], chain[:5], 1, 1)]
    keys, nk = list(eng.slot_keys), eng.n_keys
    out = eng.mstep(blocks)
    want = [((1, 64, 1, 1), ids[:64], chain[:64], np.zeros((64, 0), dtype=np.uint64)),
            ((1, 5, 1, 1), ids[64:], chain[:5], np.zeros((5, 0), dtype=np.uint64))]
    check_input_block(eng._lib.calls[0][1], want)
    assert out == [header_tokens(hdr, 0), header_tokens(hdr, 1)]
    check_keys(eng, hdr, (1,), keys, nk)
    assert eng._mstep_slots == [1, 1]


def test_mstep_refuses_a_chain_whose_first_block_is_short():
    eng = make_engine()
    ids = np.arange(3, 72, dtype=np.int32)
    chain = LlamaVerifyEngine._CHAIN
    with pytest.raises(AssertionError, match='prefill chain of full blocks'):
        eng.mstep_async([(1, ids[:5], chain[:5], 1, 1), (1, ids[5:], chain[:64], 1, 1)])
    with pytest.raises(AssertionError, match='prefill chain of full blocks'):          # two trees of one slot are no chain either
        eng.mstep_async([(1, ids[:64], chain[:64], 0, 16), (1, ids[:64], chain[:64], 0, 16)])
    assert eng._lib.calls == []


def test_mstep_capacity_is_the_sum_over_a_slots_blocks():
    ids = np.arange(3, 72, dtype=np.int32)
    chain = LlamaVerifyEngine._CHAIN
    blocks = [(1, ids[:64], chain[:64], 1, 1), (1, ids[64:], chain[:5], 1, 1)]
    eng = make_engine(slot_keys=(0, CAPACITY - 69, 0, 0))
    eng._lib.answers.append(canned_header(3))
    eng.mstep(blocks)
    eng = make_engine(slot_keys=(0, CAPACITY - 68, 0, 0))
    with pytest.raises(AssertionError, match='capacity'):
        eng.mstep_async(blocks)
    assert eng._lib.calls == []
    with pytest.raises(AssertionError, match='max_blocks'):
        eng.mstep_async([(0, ids[:1], chain[:1], 0, 1)] * 9)


# ---- tstep ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T,one_d,slot,mode,limit,eager', [(1, False, 0, 0, None, False), (1, True, 2, 2, 7, False),
                                                           (64, False, 3, 0, 100, True), (64, True, 0, 2, 0, False),
                                                           (65, False, 1, 0, None, False), (130, False, 0, 2, 12, True)])
def test_tstep(T, one_d, slot, mode, limit, eager):
    eng, rs = make_engine(), np.random.RandomState(T)
    hdr = canned_header(10 + T)
    eng._lib.answers.append(hdr)
    nb = (T + 63) // 64
    ids, rm = random_tree(rs, T, nb)
    keys, nk = list(eng.slot_keys), eng.n_keys
    toks, kept = eng.tstep(ids, rm[:, 0] if one_d else rm, slot=slot, mode=mode, limit=limit, eager=eager)
    (name, words), = eng._lib.calls
    assert name == ('mstep_eager' if eager else 'mstep')
    lim = TOKS if limit is None else max(1, min(TOKS, limit))
    check_input_block(words, expected_blocks([(slot, ids, rm, mode, lim)]))
    assert toks == header_tokens(hdr, 0) and kept == int(hdr[MOUT_NKEYS + slot]) - keys[slot]
    check_keys(eng, hdr, (slot,), keys, nk)
    assert eng._mstep_slots == [slot] * nb and eng.stream.syncs == 1


def test_tstep_refuses_a_mask_without_an_ancestor_word():
    eng, rs = make_engine(), np.random.RandomState(0)
    ids, rm = random_tree(rs, 130, 3)
    with pytest.raises(AssertionError, match='needs 3 mask words'):          # (an IndexError before the codec was shared)
        eng.tstep(ids, rm[:, 0])
    assert eng._lib.calls == []


def test_tstep_refuses_a_one_word_mask_at_65_rows():
    """(before the codec was shared only a missing ANCESTOR word raised; this mask went through with a zero own-block word in block 1)"""
    eng, rs = make_engine(), np.random.RandomState(0)
    ids, rm = random_tree(rs, 65, 2)
    with pytest.raises(AssertionError, match='mask word'):
        eng.tstep(ids, rm[:, 0])
    assert eng._lib.calls == []


def test_tstep_capacity_and_block_limit():
    rs = np.random.RandomState(1)
    ids, rm = random_tree(rs, 130, 3)
    eng = make_engine(slot_keys=(0, 0, CAPACITY - 130, 0))
    eng._lib.answers.append(canned_header(4))
    eng.tstep(ids, rm, slot=2)
    eng = make_engine(slot_keys=(0, 0, CAPACITY - 129, 0))
    with pytest.raises(AssertionError, match='capacity'):
        eng.tstep(ids, rm, slot=2)
    eng = make_engine()
    eng.max_blocks = 2
    with pytest.raises(AssertionError, match='max_blocks >= 3'):
        eng.tstep(ids, rm)
    assert eng._lib.calls == []


# ---- mstep_trees ---------------------------------------------------------------------------------------------------------------
def _three_trees(rs):
    """70 rows (2 blocks, 2 words), 3 rows (a 1-D mask), 129 rows with ONE word: 3 blocks whose later ancestor words are zeros"""
    (i0, m0), (i1, m1), (i2, m2) = random_tree(rs, 70, 2), random_tree(rs, 3, 1), random_tree(rs, 129, 1)
    return [(2, i0, m0, 0, 16), (0, i1, m1[:, 0], 2, 100), (3, i2, m2, 0, 0)]


@pytest.mark.parametrize('eager', [False, True])
def test_mstep_trees(eager):
    eng, rs = make_engine(), np.random.RandomState(5)
    hdr = canned_header(20)
    eng._lib.answers.append(hdr)
    trees = _three_trees(rs)
    keys, nk = list(eng.slot_keys), eng.n_keys
    out = eng.mstep_trees(trees, eager=eager)
    (name, words), = eng._lib.calls
    assert name == ('mstep_eager' if eager else 'mstep')
    want = expected_blocks([(s, ids, rm if rm.ndim == 2 else rm[:, None], mode, max(1, min(TOKS, lim))) for s, ids, rm, mode, lim in trees])
    assert len(want) == 6 and not want[5][3][:, 1].any() and want[5][3][:, 0].any() and not want[4][2].any()
    check_input_block(words, want)
    assert out == [header_tokens(hdr, 0), header_tokens(hdr, 2), header_tokens(hdr, 3)]
    check_keys(eng, hdr, (2, 0, 3), keys, nk)
    assert eng._mstep_slots == [2, 2, 0, 3, 3, 3] and eng.stream.syncs == 1


def test_mstep_trees_leaves_n_keys_alone_without_slot_0():
    eng, rs = make_engine(), np.random.RandomState(6)
    hdr = canned_header(21)
    eng._lib.answers.append(hdr)
    ids, rm = random_tree(rs, 70, 2)
    keys, nk = list(eng.slot_keys), eng.n_keys
    assert eng.mstep_trees([(1, ids, rm, 0, 16)]) == [header_tokens(hdr, 0)]
    check_keys(eng, hdr, (1,), keys, nk)


def test_mstep_trees_refusals():
    rs = np.random.RandomState(8)
    ids, rm = random_tree(rs, 70, 2)
    eng = make_engine()
    with pytest.raises(AssertionError, match='one tree per slot'):
        eng.mstep_trees([(1, ids, rm, 0, 16), (1, ids, rm, 0, 16)])
    eng = make_engine(slot_keys=(0, CAPACITY - 70, 0, 0))
    eng._lib.answers.append(canned_header(5))
    eng.mstep_trees([(1, ids, rm, 0, 16)])
    eng = make_engine(slot_keys=(0, CAPACITY - 69, 0, 0))
    with pytest.raises(AssertionError, match='capacity'):
        eng.mstep_trees([(1, ids, rm, 0, 16)])
    eng = make_engine()
    eng.max_blocks = 3
    with pytest.raises(AssertionError, match='max_blocks >= 4'):
        eng.mstep_trees([(1, ids, rm, 0, 16), (2, ids, rm, 0, 16)])
    assert eng._lib.calls == []


# ---- chained device trie -------------------------------------------------------------------------------------------------------
class FakeTensor(object):
    def __init__(self, ptr):
        self.ptr = ptr

    def data_ptr(self):
        return self.ptr


class FakeTrie(object):
    out_ids, out_rm, out_n = FakeTensor(1 << 20), FakeTensor(2 << 20), FakeTensor(3 << 20)


@pytest.mark.parametrize('q0,slots', [(0, (1, 2)), (5, (3, 0, 1))])
def test_mstep_trie_without_device_put(q0, slots):
    eng = make_engine()
    hdr = canned_header(30 + q0)
    eng._lib.answers.append(hdr)
    limits, last = (0, 16, 99)[:len(slots)], (11, 12, 13)[:len(slots)]
    keys, nk = list(eng.slot_keys), eng.n_keys
    eng.mstep_trie_async(FakeTrie(), q0, list(slots), limits, last)
    assert eng.stream.syncs == 0
    toks, dls = eng.mstep_trie_finish()
    assert eng._lib.calls == [('mstep_trie', len(slots), list(slots), [max(1, min(TOKS, x)) for x in limits], list(last),
                               (1 << 20) + 4 * 64 * q0, (2 << 20) + 8 * 64 * q0, (3 << 20) + 4 * q0)]
    assert toks == [header_tokens(hdr, b) for b in range(len(slots))]
    assert dls == hdr[MOUT_T:MOUT_T + len(slots)].tolist()
    check_keys(eng, hdr, slots, keys, nk)
    assert eng._mstep_slots == list(slots) and eng.stream.syncs == 1      # no device put queued: the stream is what is waited for


# ---- commits -------------------------------------------------------------------------------------------------------------------
def _keep_array(n_blocks, kept_at):
    """kept_at: (first block of the tree, rows to keep): keep[64 * block + row] = position on the kept path, -1 elsewhere"""
    keep = np.full(64 * n_blocks, -1, dtype=np.int32)
    for b0, rows in kept_at:
        for k, r in enumerate(rows):
            keep[64 * b0 + r] = k
    return keep


def test_mcommit():
    eng, rs = make_engine(), np.random.RandomState(9)
    eng._lib.answers += [canned_header(40), canned_header(41)]
    blocks = [(s, *[x if x.ndim == 1 else x[:, 0] for x in random_tree(rs, n, 1)], 2, 16) for s, n in ((3, 64), (0, 9), (1, 30))]
    eng.mstep(blocks)
    keys, nk = list(eng.slot_keys), eng.n_keys
    kept = [[0, 5, 63], [0], [0, 1, 2, 29]]
    eng.mcommit(kept)
    name, nb, keep = eng._lib.calls[1]
    assert (name, nb) == ('mcommit', 3) and keep.tolist() == _keep_array(3, [(0, kept[0]), (1, kept[1]), (2, kept[2])]).tolist()
    check_keys(eng, canned_header(41), (3, 0, 1), keys, nk)
    with pytest.raises(AssertionError):
        eng.mcommit(kept[:2])


def test_mcommit_trees():
    eng, rs = make_engine(), np.random.RandomState(10)
    eng._lib.answers += [canned_header(42), canned_header(43)]
    (i0, m0), (i1, m1) = random_tree(rs, 70, 2), random_tree(rs, 3, 1)
    eng.mstep_trees([(2, i0, m0, 2, 16), (1, i1, m1, 2, 16)])
    keys, nk = list(eng.slot_keys), eng.n_keys
    kept = [[0, 3, 64, 69], [0, 2]]
    eng.mcommit_trees(kept, (70, 3))
    name, nb, keep = eng._lib.calls[1]
    assert (name, nb) == ('mcommit', 3) and keep.tolist() == _keep_array(3, [(0, kept[0]), (2, kept[1])]).tolist()
    check_keys(eng, canned_header(43), (2, 1), keys, nk)


@pytest.mark.parametrize('slot', [0, 2])
def test_tcommit(slot):
    eng, rs = make_engine(), np.random.RandomState(11)
    eng._lib.answers += [canned_header(44), canned_header(45)]
    ids, rm = random_tree(rs, 130, 3)
    eng.tstep(ids, rm, slot=slot, mode=2)
    keys, nk = list(eng.slot_keys), eng.n_keys
    rows = [0, 1, 64, 100, 129]
    eng.tcommit(rows, 130)
    name, nb, keep = eng._lib.calls[1]
    assert (name, nb) == ('mcommit', 3) and keep.tolist() == _keep_array(3, [(0, rows)]).tolist()
    check_keys(eng, canned_header(45), (slot,), keys, nk)
