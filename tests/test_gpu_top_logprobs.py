# -*- coding: utf-8 -*-
"""GPU: top-N log-probabilities on the device (csrc/la_logprob.hip: k_top_logprob_rows) against the numpy model of
tests/top_logprob_model.py.

Ids: EQUAL to the model — both select on the same stored 16-bit values (key descending, then id ascending).  Values: within
logprob_model.bound_device (1e-4 + 2^-22 |lp|: the documented bound of the scalar stage) of the fp64 model on the SAME stored logits,
and the entry of a token has the bits the scalar stage gives for that token (the same maximum, the same integer mass)."""
import numpy as np
import pytest
import torch

from oracle import llama_oracle as lo
from painlessinferenceacceleration_amd import _lib
from painlessinferenceacceleration_amd._lib import check
from painlessinferenceacceleration_amd.llama_engine import LlamaVerifyEngine
from painlessinferenceacceleration_amd.lookahead_cache import LookaheadCache
from painlessinferenceacceleration_amd.modeling_llama_batch import LlamaForCausalLM as BatchLlama
from tests import logprob_model as lm
from tests import test_gpu_logprobs as tgl
from tests import top_logprob_model as tm
from tests.gpu_utils import DEV, ptr, sp
from tests.tiny_model import tiny_shape

pytestmark = pytest.mark.gpu

DTYPES, IDS, ONE, DK = tgl.DTYPES, tgl.IDS, tgl.ONE, tgl.DK
_name = tgl._name
WORST = {'rows': 0.0, 'steps': 0.0}      # worst measured error / bound of the session: printed


# ------------------------------------------------------------------------------------------------ 1. the row stage alone
_ROWS = {}


def _rows(V, dtype, n):
    """the planted rows of one (vocab, dtype, n) and their model lists, computed once"""
    key = (V, dtype, n)
    if key not in _ROWS:
        rows = tm.planted_rows(V, _name(dtype), n, n_rows=64)
        ids, f64, _ = tm.top_model(rows, _name(dtype), n, intmass=False)
        _ROWS[key] = (rows, ids, f64)
    return _ROWS[key]


def _run_top(lib, lg_dev, n):
    R = lg_dev.shape[0]
    ids = torch.full((64, n), 7, dtype=torch.int32, device=DEV)
    vals = torch.full((64, n), 7.0, dtype=torch.float32, device=DEV)
    check(lib.la_top_logprob_rows(sp(), ptr(lg_dev), lg_dev.shape[1], R, n, ptr(ids), ptr(vals)), 'top_logprob_rows')
    torch.cuda.synchronize()
    ids, vals = ids.cpu().numpy(), vals.cpu().numpy()
    assert (ids[R:] == 7).all() and (vals[R:] == 7.0).all()                    # rows past n_rows are untouched
    return ids[:R], vals[:R]


def _scalar(lib, lg_dev, toks):
    d_tok = torch.from_numpy(np.ascontiguousarray(toks, dtype=np.int32)).to(DEV)
    out = torch.zeros((64,), dtype=torch.float32, device=DEV)
    check(lib.la_logprob_rows(sp(), ptr(lg_dev), lg_dev.shape[1], lg_dev.shape[0], ptr(d_tok), ptr(out)), 'logprob_rows')
    torch.cuda.synchronize()
    return out.cpu().numpy()[:lg_dev.shape[0]]


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('n_rows', [1, 64])
@pytest.mark.parametrize('V,n', [(V, n) for V in (8, 512, 32000, 152064) for n in (1, 5, 20) if n <= V])
def test_row_stage_equals_the_model(V, n, n_rows, dtype):
    lib = _lib.lib_for(dtype)
    rows, want_ids, want = _rows(V, dtype, n)
    rows, want_ids, want = rows[:n_rows], want_ids[:n_rows], want[:n_rows]
    lg = torch.from_numpy(rows).to(dtype)
    assert (lg.float().numpy() == rows).all()                                  # the rows are values of the storage type
    lg_dev = lg.to(DEV).contiguous()
    ids, vals = _run_top(lib, lg_dev, n)
    assert np.array_equal(ids, want_ids), np.argwhere(ids != want_ids)[:8]     # no tolerance
    err, bound = np.abs(vals.astype(np.float64) - want), lm.bound_device(want)
    WORST['rows'] = max(WORST['rows'], float((err / bound).max()))
    print(f'V={V} n={n} n_rows={n_rows} {_name(dtype)}: worst err {err.max():.3e}, worst err / bound {(err / bound).max():.3e} '
          f'(session {WORST["rows"]:.3e})')
    assert np.all(np.isfinite(vals)) and np.all(err <= bound), (err.max(), bound)
    for j in range(n):                                                         # the bits of the scalar stage, token by token
        assert _scalar(lib, lg_dev, ids[:, j]).tobytes() == np.ascontiguousarray(vals[:, j]).tobytes(), j
    again = _run_top(lib, lg_dev, n)
    assert again[0].tobytes() == ids.tobytes() and again[1].tobytes() == vals.tobytes()      # the same bytes on every run
    if n_rows == 64:                                                           # ... and at every row index
        perm = np.random.RandomState(1).permutation(64)
        moved = _run_top(lib, lg_dev[torch.from_numpy(perm).to(DEV)].contiguous(), n)
        assert moved[0].tobytes() == ids[perm].tobytes() and moved[1].tobytes() == vals[perm].tobytes()


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_row_stage_refuses_n_outside_its_range(dtype):
    lib = _lib.lib_for(dtype)
    lg = torch.zeros((2, 16), dtype=dtype, device=DEV)
    ids = torch.full((64, 32), 7, dtype=torch.int32, device=DEV)
    vals = torch.full((64, 32), 7.0, dtype=torch.float32, device=DEV)
    for n in (0, 21, 17, -1):                                                  # off the range; 17 > vocab = 16
        assert lib.la_top_logprob_rows(sp(), ptr(lg), 16, 2, n, ptr(ids), ptr(vals)) == -2, n      # LA_E_RANGE
    assert lib.la_top_logprob_rows(sp(), ptr(lg), 12, 2, 4, ptr(ids), ptr(vals)) == -2      # vocab % 8
    torch.cuda.synchronize()
    assert (ids.cpu().numpy() == 7).all() and (vals.cpu().numpy() == 7.0).all()
    eng = LlamaVerifyEngine(tiny_shape(), tgl._sd(dtype), max_length=256)
    for n in (-1, 21):
        with pytest.raises(_lib.LookaheadHipError):                            # LA_E_RANGE
            eng.set_top_logprobs(n)
    eng.set_top_logprobs(20)
    eng.set_top_logprobs(0)


# ------------------------------------------------------------------------------------------------ 2. the stage inside the steps
def _check_log(eng, slot, expected, first, n, dtype, greedy, npos=150):
    """the slot's logs from position `first` on.  expected: {position: (the engine's own logits row, float32; the emitted token)}.
    At an emitted position: ids equal the model on that row, values within the bound, entry 0 = the token under plain greedy, the
    token's entry has the bits of the scalar log; everywhere else (-1, NaN)."""
    ids, vals = eng.top_logprobs(slot, first, npos)
    lps = eng.logprobs(slot, first, npos)
    assert ids.shape == vals.shape == (npos, n)
    at = sorted(p for p in expected if first <= p < first + npos)
    assert len(at) == len([p for p in expected if p >= first])
    if at:
        want_ids, want, _ = tm.top_model(np.stack([expected[p][0] for p in at]), _name(dtype), n, intmass=False)
    for i, p in enumerate(at):
        tok, got_ids, got = int(expected[p][1]), ids[p - first], vals[p - first]
        assert got_ids.tolist() == want_ids[i].tolist(), (slot, p, got_ids, want_ids[i])
        err, bound = np.abs(got.astype(np.float64) - want[i]), lm.bound_device(want[i])
        WORST['steps'] = max(WORST['steps'], float((err / bound).max()))
        assert np.all(np.isfinite(got)) and np.all(err <= bound), (slot, p, got, want[i])
        if greedy:
            assert got_ids[0] == tok, (slot, p, got_ids, tok)
        where = np.flatnonzero(got_ids == tok)
        if len(where):
            assert got[where[0]:where[0] + 1].tobytes() == lps[p - first:p - first + 1].tobytes(), (slot, p)
        assert np.isfinite(lps[p - first])
    empty = np.ones(npos, dtype=bool)
    empty[[p - first for p in at]] = False
    assert (ids[empty] == -1).all() and np.isnan(vals[empty]).all() and np.isnan(lps[empty]).all(), slot


def _stages_on(eng, which, slots):
    if which == 'penalty':
        eng.set_repetition_penalty(1.3)
    if which == 'sampling':
        for s in slots:
            eng.sampling_stream(s, s)
        eng.set_sampling(True, 7, 0.8, 20, 0.9)


def _stages_off(eng, which):
    if which == 'penalty':
        eng.set_repetition_penalty(1.0)
    if which == 'sampling':
        eng.set_sampling(False)


def _np_row(lg, r):
    return lg[r].float().cpu().numpy()


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('n', [5, 20])
@pytest.mark.parametrize('which', ['greedy', 'penalty', 'sampling'])
def test_stage_inside_the_single_step(which, n, dtype):
    """prefill chain (two blocks), graph and eager tree steps with a dropped sibling at every depth, a forward-only step; then the
    off path: the same request with top-N off (before and after it was on) gives the same tokens, launch counts and scalar log bytes"""
    shape = tiny_shape()
    eng = LlamaVerifyEngine(shape, tgl._sd(dtype), max_length=512)
    prompt = np.random.RandomState(4).randint(3, shape.vocab, size=70).tolist()
    tok = eng.prefill(prompt, fast=False)
    cont = [tok]                                                               # the plain greedy continuation: the drafts of the trees
    for _ in range(16):
        cont.append(eng.step(np.asarray(cont[-1:], dtype=np.int32), ONE)[0][0])

    def run(top):
        rs = np.random.RandomState(11)
        eng.reset()
        _stages_on(eng, which, [0])
        eng.set_logprobs(True)
        if top:
            eng.set_top_logprobs(n)
        n0 = eng.logprob_launches()
        first = eng.prefill(prompt, fast=False)
        expected = {70: (_np_row(eng.logits(), 5), first)}                     # row (70 - 1) % 64 chooses the token at index 70
        if top:
            _check_log(eng, 0, expected, 70, n, dtype, which == 'greedy')
        out, last = [first], first
        for step, (k, eager) in enumerate([(3, False), (2, True), (1, False)]):
            ids, rm = tgl._planted_tree(last, cont[len(out):], k, 6, rs, shape.vocab)
            nk = eng.n_keys
            toks, kept_n = eng.step(ids.copy(), rm.copy(), eager=eager)
            words = eng.state().cpu().numpy()[_lib.LA_ST_ARGMAX:_lib.LA_ST_ARGMAX + len(ids)]
            want, rows = lo.accept_scan_limited(ids.tolist(), tgl._mask_matrix(rm), [int(w) for w in words], 64)
            assert list(toks) == want and kept_n == len(rows)
            if which == 'greedy':
                assert len(rows) >= k + 1                                      # the planted chain was accepted
            lg = eng.logits()
            for i, r in enumerate(rows):
                expected[nk + i + 1] = (_np_row(lg, r), words[r])
            if top:
                _check_log(eng, 0, expected, 70, n, dtype, which == 'greedy')
            out += list(toks)
            last = toks[-1]
        before = [a.tobytes() for a in eng.top_logprobs(0, 0, 300)] if top else None
        ids, rm = tgl._planted_tree(last, cont[len(out):], 2, 6, rs, shape.vocab)
        eng.verify_only(ids, rm)                                               # a forward-only step (mode 2) stores nothing
        if top:
            assert [a.tobytes() for a in eng.top_logprobs(0, 0, 300)] == before
        scalar = eng.logprobs(0, 0, 300).tobytes()
        launches = eng.logprob_launches() - n0
        if top:
            eng.set_top_logprobs(0)
        eng.set_logprobs(False)
        _stages_off(eng, which)
        return out, scalar, launches

    off = run(False)
    on = run(True)
    assert on == off                                                           # tokens, scalar log bytes, launch count
    assert run(False) == off                                                   # set_top_logprobs(0) after use restores the off path
    print(f'single step {which} n={n} {_name(dtype)}: worst err / bound so far {WORST["steps"]:.3e}')


# which stages x n: every pick stage at n = 5, and n = 20 (the widest list) under plain greedy; the list never reads the pick
BATCH_CASES = [('greedy', 5), ('penalty', 5), ('sampling', 5), ('greedy', 20)]


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('which,n', BATCH_CASES)
@pytest.mark.parametrize('blocks', [0, 2, 3], ids=['bstep', 'mstep2', 'mstep3'])
def test_stage_inside_the_batch_steps(blocks, which, n, dtype):
    """bstep: two slots at their own cursors + one slot as a prefill chain in ONE block; mstep: one tree per block, 2 and 3 blocks;
    bprefill / mprefill (mode 1) before them; a forward-only pass (mode 2) after them"""
    shape = tiny_shape()
    eng = LlamaVerifyEngine(shape, tgl._sd(dtype), max_length=256, n_slots=3, max_blocks=blocks)
    rs = np.random.RandomState(20 + blocks)
    S = 3 if blocks == 3 else 2                                                # slots that carry a tree
    lens = [40, 20, 9][:S]                                                     # one chain of one pass each: every last row stays readable
    prompts = {b: rs.randint(3, shape.vocab, size=lens[b]).tolist() for b in range(S)}
    late = rs.randint(3, shape.vocab, size=20).tolist()                        # bstep: slot 2's prompt, prefilled inside the tree step
    prefill = eng.mprefill_many if blocks else eng.bprefill_many
    greedy = which == 'greedy'

    def step(segs):
        if blocks:
            return dict(zip([s[0] for s in segs], eng.mstep(segs)))
        return eng.bstep(segs)

    # stages off: the plain greedy continuations (the drafts)
    first = prefill(prompts)
    cont = {b: [first[b]] for b in range(S)}
    for _ in range(8):
        out = step([(b, np.asarray(cont[b][-1:], dtype=np.int32), ONE, 0, 1) for b in range(S)])
        for b in range(S):
            cont[b].append(out[b][0])
    eng.reset_slot(-1)
    _stages_on(eng, which, range(3))
    eng.set_logprobs(True)
    eng.set_top_logprobs(n)
    first = prefill(prompts)
    if blocks:
        lg, base, am = eng.mlogits(), {b: 64 * b for b in range(S)}, eng.mout().cpu().numpy()[_lib.LA_MOUT_ARGMAX:]
    else:
        lg, base, am = eng.logits(), eng.bstep_rows(), eng.bstate().cpu().numpy()[_lib.LA_BST_ARGMAX:]
    expected = {b: {} for b in range(3)}
    for b in range(S):
        r = base[b] + lens[b] - 1
        assert first[b] == int(am[r])
        expected[b][lens[b]] = (_np_row(lg, r), first[b])
    for b in range(3):
        _check_log(eng, b, expected[b], 0, n, dtype, greedy)
    # one tree step
    segs = []
    for b in range(S):
        ids, rm = tgl._planted_tree(first[b], cont[b][1:], [3, 1, 2][b], 6, rs, shape.vocab)
        segs.append((b, ids, rm, 0, 16))
    nk = list(eng.slot_keys)
    if not blocks:
        segs.append((2, np.asarray(late, dtype=np.int32), eng._CHAIN[:len(late)], 1, 1))
    out = step(segs)
    if blocks:
        lg, base, am = eng.mlogits(), {b: 64 * b for b in range(S)}, eng.mout().cpu().numpy()[_lib.LA_MOUT_ARGMAX:]
    else:
        lg, base, am = eng.logits(), eng.bstep_rows(), eng.bstate().cpu().numpy()[_lib.LA_BST_ARGMAX:]
    for b, ids, rm, mode, limit in segs[:S]:
        T = len(ids)
        words = [int(w) for w in am[base[b]:base[b] + T]]
        want, rows = lo.accept_scan_limited(ids.tolist(), tgl._mask_matrix(rm), words, limit)
        assert list(out[b]) == want, (b, out[b], want)
        if greedy:
            assert len(rows) >= 2
        for i, r in enumerate(rows):
            expected[b][nk[b] + i + 1] = (_np_row(lg, base[b] + r), words[r])
    if not blocks:
        r = base[2] + len(late) - 1
        assert out[2] == [int(am[r])]
        expected[2][len(late)] = (_np_row(lg, r), int(am[r]))
    for b in range(3):
        _check_log(eng, b, expected[b], 0, n, dtype, greedy)
    # forward only (mode 2): nothing stored
    before = [[a.tobytes() for a in eng.top_logprobs(b, 0, 200)] for b in range(3)]
    step([(b, np.asarray(cont[b][:1], dtype=np.int32), ONE, 2, 1) for b in range(S)])
    assert [[a.tobytes() for a in eng.top_logprobs(b, 0, 200)] for b in range(3)] == before
    # a slot reset clears that slot's list only
    eng.reset_slot(1)
    assert (eng.top_logprobs(1, 0, 200)[0] == -1).all() and np.isnan(eng.top_logprobs(1, 0, 200)[1]).all()
    assert [a.tobytes() for a in eng.top_logprobs(0, 0, 200)] == before[0]
    eng.set_top_logprobs(0)
    eng.set_logprobs(False)
    _stages_off(eng, which)
    print(f'{"mstep" if blocks else "bstep"} {blocks} {which} n={n} {_name(dtype)}: worst err / bound so far {WORST["steps"]:.3e}')


# ------------------------------------------------------------------------------------------------ 3. the front doors
def _check_lists(tops, lps, new_tokens, n):
    """shape, alignment, order; entry 0 = the generated token (greedy) with the bits of the scalar value"""
    assert len(tops) == len(lps) == len(new_tokens)
    for row, lp, tok in zip(tops, lps, new_tokens):
        assert len(row) == n and len({t for t, _ in row}) == n
        vals = [v for _, v in row]
        assert all(np.isfinite(v) and v <= 0 for v in vals) and all(a >= b for a, b in zip(vals, vals[1:])), row
        assert row[0][0] == tok
        assert np.float32(row[0][1]).tobytes() == np.float32(lp).tobytes()


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('n', [5, 20])
def test_front_doors_bs1(n, dtype):
    model = tgl._model(dtype)
    eng = model.engine
    rs = np.random.RandomState(8)
    P, n_new = 45, 40
    prompt = torch.tensor([rs.randint(3, eng.shape.vocab, size=P).tolist()])
    launches = eng.logprob_launches()
    plain, plain_lps = model.greedy_search(prompt, P + n_new, eos_token_id=None, output_logprobs=True)
    launches = eng.logprob_launches() - launches
    n0 = eng.logprob_launches()
    seq_g, lps_g, tops_g = model.greedy_search(prompt, P + n_new, eos_token_id=None, top_logprobs=n)
    assert eng.logprob_launches() - n0 == launches and eng.top_logprobs_n == 0 and not eng.logprobs_on
    assert seq_g.tolist() == plain.tolist()                                    # tokens and scalar values do not change with the list on
    assert np.asarray(lps_g, dtype=np.float32).tobytes() == np.asarray(plain_lps, dtype=np.float32).tobytes()
    new = seq_g[0].tolist()[P:]
    _check_lists(tops_g, lps_g, new, n)
    runs = {}
    for door in ('native', 'interpreter', 'generate'):
        model.lookahead_cache = tgl._warm_trie([seq_g[0].tolist()[P - 1:]])
        if door == 'generate':
            out = model.generate(prompt, max_new_tokens=n_new, return_dict_in_generate=True, decoding_kwargs=dict(DK, top_logprobs=n))
        else:
            out = model.lookahead_generation(prompt, stopping_criteria=P + n_new, eos_token_id=[None], return_dict_in_generate=True,
                                             decoding_kwargs=dict(DK, native_loop=door == 'native', top_logprobs=n))
        seq, lps, tops = out.sequences[0].tolist(), out.kwargs['logprobs'], out.kwargs['top_logprobs']
        assert np.mean(out.kwargs['edls'][1:]) > 2 and eng.top_logprobs_n == 0 and not eng.logprobs_on
        _check_lists(tops, lps, seq[P:], n)
        w = min(len(seq), P + n_new)
        assert seq[:w] == seq_g[0].tolist()[:w]                                # lookahead == no-draft: sequences and top-1 ids
        assert [row[0][0] for row in tops[:w - P]] == [row[0][0] for row in tops_g[:w - P]]
        runs[door] = (seq, tops)
    assert runs['native'] == runs['interpreter'] == runs['generate']           # the same ids and the same bits through every loop


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('max_blocks', [0, 2], ids=['cursor', 'multiblock'])
def test_front_doors_batch_of_two_left_padded_prompts(max_blocks, dtype):
    n = 5
    model = BatchLlama(tiny_shape(), tgl._sd_decisive(dtype), max_length=512, max_batch=4, eos_token_id=None, max_blocks=max_blocks)
    eng = model.engine
    rs = np.random.RandomState(15)
    lens, n_new = [40, 20], 24
    P = max(lens)
    ids = np.zeros((2, P), dtype=np.int64)
    am = np.zeros((2, P), dtype=np.int64)
    for b, ln in enumerate(lens):
        ids[b, P - ln:] = rs.randint(3, eng.shape.vocab, size=ln)
        am[b, P - ln:] = 1
    t_ids, t_am = torch.from_numpy(ids), torch.from_numpy(am)
    plain, plain_lps = model.greedy_search(t_ids, P + n_new, attention_mask=t_am, eos_token_id=None, output_logprobs=True)
    seq_g, lps_g, tops_g = model.greedy_search(t_ids, P + n_new, attention_mask=t_am, eos_token_id=None, top_logprobs=n)
    seq_g = seq_g.cpu().numpy()
    assert seq_g.tolist() == plain.cpu().numpy().tolist() and eng.top_logprobs_n == 0 and not eng.logprobs_on
    for b in range(2):
        assert np.asarray(lps_g[b], dtype=np.float32).tobytes() == np.asarray(plain_lps[b], dtype=np.float32).tobytes()
        _check_lists(tops_g[b], lps_g[b], seq_g[b, P:].tolist(), n)
    warm = [seq_g[b, P - 1:] for b in range(2)]
    extra = {'per_sample_budget': True} if max_blocks else {}
    for door in ('lookahead_generation', 'generate'):
        model.lookahead_cache = tgl._warm_trie(warm)
        dk = dict(DK, top_logprobs=n, **extra)
        if door == 'generate':
            out = model.generate(input_ids=t_ids, attention_mask=t_am, max_new_tokens=n_new, eos_token_id=[None], pad_token_id=0,
                                 return_dict_in_generate=True, decoding_kwargs=dk)
        else:
            out = model.lookahead_generation(t_ids, stopping_criteria=P + n_new, eos_token_id=[None], pad_token_id=0,
                                             return_dict_in_generate=True, attention_mask=t_am, decoding_kwargs=dk)
        got = out.sequences.cpu().numpy()
        w = min(got.shape[1], P + n_new)
        assert got[:, :w].tolist() == seq_g[:, :w].tolist() and np.mean(out.kwargs['edls'][2:]) > 2
        assert eng.top_logprobs_n == 0 and not eng.logprobs_on
        for b in range(2):
            tops, lps = out.kwargs['top_logprobs'][b], out.kwargs['logprobs'][b]
            _check_lists(tops, lps, got[b, P:].tolist(), n)
            assert [row[0][0] for row in tops[:w - P]] == [row[0][0] for row in tops_g[b][:w - P]]


# ------------------------------------------------------------------------------------------------ 4. the off path
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_a_request_without_the_option_is_the_request_of_before(dtype):
    """tokens, logprob_launches and the scalar log bytes of an output_logprobs request: before the list was ever on (an engine that
    has allocated nothing), and again after a request with the list"""
    model = tgl._model(dtype)
    eng = model.engine
    prompt = torch.tensor([np.random.RandomState(9).randint(3, eng.shape.vocab, size=33).tolist()])

    def request(extra):
        model.lookahead_cache = LookaheadCache()
        n0 = eng.logprob_launches()
        out = model.lookahead_generation(prompt, stopping_criteria=33 + 24, eos_token_id=[None], return_dict_in_generate=True,
                                         decoding_kwargs=dict(DK, output_logprobs=True, **extra))
        return (out.sequences[0].tolist(), np.asarray(out.kwargs['logprobs'], dtype=np.float32).tobytes(),
                eng.logprob_launches() - n0), out.kwargs

    before, kw = request({})
    assert 'top_logprobs' not in kw
    with_list, kw = request({'top_logprobs': 20})
    assert with_list == before and len(kw['top_logprobs']) == len(kw['logprobs'])
    after, kw = request({})
    assert after == before and 'top_logprobs' not in kw and eng.top_logprobs_n == 0
