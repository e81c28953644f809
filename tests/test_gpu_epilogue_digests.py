# -*- coding: utf-8 -*-
"""The GEMM epilogues (RoPE + fragment stores, SwiGLU, rounded logits + argmax candidates, split-K slabs) pinned bit for bit where
tests/golden/prologue_digests.json and tests/golden/step_form_digests.json leave them open: tests/golden/epilogue_digests.json holds a
sha256 of every output buffer a launch writes, recorded (record_all() below) on an MI355X from the libraries of the commit BEFORE the
epilogue arithmetic moved into csrc/la_epilogue.h.  The fixture was recorded twice in separate processes, the second with the
allocator's memory pre-filled non-zero (LA_RECORD_DIRTY=1, record_all()); both runs gave the same digests.

  forms      every row of tests/mb_form_cases.py FORM_CASES (one small la_mb_gemm launch per GEMM form of the product build), in bf16
             and in fp16: the fresh fragments, act, slab, logits and the candidate words of the blocks that carry data
  odd_r      (bf16 and fp16) R = 5 RoPE pairs per workgroup (tests/mb_form_cases.py ODD_R_CASES; tests/test_mb_forms_cpu.py asserts the forms): the
             one-row-per-store QKV paths, which no product shape reaches — la_gemm64r_qkv(_bias), the general-R form of the 64-row
             kernel, and la_mb_gemm(_bias) on k_gemm_mb, k_gemm_wide unpaired and paired.  Each case is also checked against the fp32
             torch reference at the tolerance tests/test_gpu_mblock.py uses for QKV (1e-2): a digest alone would pin a wrong parent
  classic    (bf16 and fp16) la_gemm64_swiglu, la_gemm64_logits and la_gemm64_qkv at hidden 256 in the instantiations prologue_digests.json does not
             hold: the 4 waves x 6 tile-sets form of SwiGLU and QKV (variant 2; a two-row-block epilogue has no 8-wave form), the
             bias-free QKV entry point, and the one-row-block logits launches with 4 and with 8 waves; plus, for the fp16 build's sake, the
             planned kernel's one-pass QKV form and the fp8 QKV kernels (prologue_digests.json holds them in bf16)

Inputs come from numpy.random.RandomState.  The module uses only API of the commit the fixture was recorded from.  Forms depend on the
CU count, which the fixture stores."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from painlessinferenceacceleration_amd import _lib
from painlessinferenceacceleration_amd._lib import check
from painlessinferenceacceleration_amd.llama_engine import rope_tables
from tests import gpu_utils as gu
from tests.gpu_utils import DEV, ptr, sp
from tests.mb_form_cases import FORM_CASES, ODD_R_CASES

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'epilogue_digests.json')
DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}
HIDDEN = 256


def _sha(*ts):
    h = hashlib.sha256()
    for t in ts:
        h.update(np.ascontiguousarray(t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy()).tobytes())
    return h.hexdigest()


def _randn(rs, dt, *shape, scale=1.0):
    return torch.from_numpy((rs.standard_normal(shape) * scale).astype(np.float32)).to(DEV).to(dt)


def _bits(t):
    """the packers move 16-bit elements whatever they mean"""
    return t.contiguous().view(torch.bfloat16)


def _pack_blocks(x):
    return torch.cat([gu.pack_x(_bits(x[b * 64:(b + 1) * 64])) for b in range(x.shape[0] // 64)])


def _qkv_image(w, nh, nkv, nwg):
    if nwg:
        return gu.pack_planned(2, [_bits(w)], nwg)
    perm = np.zeros(w.shape[0], dtype=np.int32)
    check(_lib.lib.la_qkv_row_perm(nh, nkv, perm.ctypes.data_as(_lib.pi32)), 'perm')
    return gu.pack_weight(_bits(w[torch.from_numpy(perm.astype(np.int64)).to(DEV)]))


def _mb(L, kind, wp, xp, N, K, nblk, n_wg, bias=None, slabs=None, slab_rows=0, act=None, logits=None, cv=None, ci=None, pos=None, rc=None,
        rs_=None, qf=None, kf=None, vf=None, nh=0, nkv=0):
    args = (sp(), kind, ptr(wp), ptr(xp), N, K, nblk, n_wg, 1, ptr(slabs), slab_rows, ptr(act), ptr(logits), ptr(cv), ptr(ci), ptr(pos),
            ptr(rc), ptr(rs_), ptr(qf), ptr(kf), ptr(vf), nh, nkv)
    check(L.la_mb_gemm_bias(*args, ptr(bias)) if bias is not None else L.la_mb_gemm(*args), 'mb_gemm')
    torch.cuda.synchronize()


def _qkv_inputs(rs, dt, nblk, K, nh, nkv):
    N = (nh + 2 * nkv) * 128
    x, w = _randn(rs, dt, nblk * 64, K), _randn(rs, dt, N, K, scale=0.05)
    bias = _randn(rs, dt, N, scale=0.5)
    pos = torch.from_numpy(rs.randint(0, 900, size=nblk * 64).astype(np.int32)).to(DEV)
    rc, rs_ = rope_tables(128, 1024, 10000.0, DEV, dt)
    return N, x, w, bias, pos, rc, rs_


def _fragments(dt, nblk, nh, nkv):
    return [torch.zeros(nblk * n * 8192, dtype=dt, device=DEV) for n in (nh, nkv, nkv)]


def mb_launch(L, dt, seed, kind, nblk, K, shp):
    """one la_mb_gemm launch of tests/mb_form_cases.py -> the buffers it writes, cut to the blocks that carry data"""
    rs = np.random.RandomState(seed)
    if kind == 2:
        nh, nkv, nwg = shp
        N, x, w, _, pos, rc, rs_ = _qkv_inputs(rs, dt, nblk, K, nh, nkv)
        qf, kf, vf = _fragments(dt, nblk, nh, nkv)
        _mb(L, 2, _qkv_image(w, nh, nkv, nwg), _pack_blocks(x), N, K, nblk, nwg, pos=pos, rc=rc, rs_=rs_, qf=qf, kf=kf, vf=vf, nh=nh, nkv=nkv)
        return [qf, kf, vf]
    x = _randn(rs, dt, nblk * 64, K)
    xp = _pack_blocks(x)
    if kind == 0:
        N = shp
        w = _randn(rs, dt, N, K, scale=0.05)
        rows = (nblk if nblk <= 2 else (nblk + 3) // 4 * 4) * 64
        slabs = torch.full((1, rows, N), float('nan'), dtype=torch.float32, device=DEV)
        _mb(L, 0, gu.pack_weight(_bits(w)), xp, N, K, nblk, 0, slabs=slabs, slab_rows=rows)
        assert not torch.isnan(slabs[0, :nblk * 64]).any()
        return [slabs[0, :nblk * 64]]
    if kind == 1:
        F, nwg = shp
        wg, wu = _randn(rs, dt, F, K, scale=0.05), _randn(rs, dt, F, K, scale=0.05)
        act = torch.zeros(8 * 64 * F, dtype=dt, device=DEV)
        _mb(L, 1, gu.pack_planned(1, [_bits(wg), _bits(wu)], nwg) if nwg else gu.pack_weight(_bits(wg), _bits(wu)), xp, F, K, nblk, nwg, act=act)
        return [act[:nblk * 64 * F]]
    V, nwg = shp
    w = _randn(rs, dt, V, K, scale=0.05)
    n_tiles = 4 * (nwg if nwg else V // 128)
    logits = torch.zeros(8 * 64, V, dtype=dt, device=DEV)
    cv = torch.zeros(8 * n_tiles * 64, dtype=torch.float32, device=DEV)
    ci = torch.zeros(8 * n_tiles * 64, dtype=torch.int32, device=DEV)
    _mb(L, 3, gu.pack_planned(0, [_bits(w)], nwg) if nwg else gu.pack_weight(_bits(w)), xp, V, K, nblk, nwg, logits=logits, cv=cv, ci=ci)
    return [logits[:nblk * 64], cv[:nblk * n_tiles * 64], ci[:nblk * n_tiles * 64]]


def form_digests(name):
    dt = DTYPES[name]
    L = _lib.lib_for(dt)
    return {f'{form}/nblk{nblk}/K{K}/{shp}': _sha(*mb_launch(L, dt, 31 * i + 5, kind, nblk, K, shp))
            for i, (form, kind, nblk, K, shp) in enumerate(FORM_CASES)}


def _check_qkv_against_torch(what, nblk, nh, nkv, x, w, bias, pos, qf, kf, vf):
    from tests.test_gpu_kernels import _rope_ref
    qkv = x.float() @ w.float().t()
    if bias is not None:
        qkv = qkv + bias.float()
    q = _rope_ref(qkv[:, :nh * 128].reshape(-1, nh, 128), pos.long())
    k = _rope_ref(qkv[:, nh * 128:(nh + nkv) * 128].reshape(-1, nkv, 128), pos.long())
    v = qkv[:, (nh + nkv) * 128:].reshape(-1, nkv, 128)
    for b in range(nblk):
        rows = slice(b * 64, (b + 1) * 64)
        got_q = gu.from_packed(qf[b * nh * 8192:(b + 1) * nh * 8192].view(nh, 8192), gu.rf_index(64)).transpose(0, 1)
        got_k = gu.from_packed(kf[b * nkv * 8192:(b + 1) * nkv * 8192].view(nkv, 8192), gu.rf_index(64)).transpose(0, 1)
        got_v = gu.from_packed(vf[b * nkv * 8192:(b + 1) * nkv * 8192].view(nkv, 8192), gu.vf_index(64)).transpose(0, 1)
        for got, ref, name in ((got_q, q[rows], 'q'), (got_k, k[rows], 'k'), (got_v, v[rows], 'v')):
            err = gu.rel_err(got.float(), ref)
            assert err < 1e-2, (what, b, name, err)


def odd_r_digests(name):
    """R = 5: the multi-block launches of ODD_R_CASES and the 64-row planned kernel at both shapes, each with and without a bias"""
    dt, out = DTYPES[name], {}
    L = _lib.lib_for(dt)
    launches = [('mb', form, nblk, K, shp) for form, _, nblk, K, shp in ODD_R_CASES]
    launches += [('gemm64r', 'k_gemm64r', 1, K, shp) for K, shp in sorted({(c[3], c[4]) for c in ODD_R_CASES})]
    for i, (entry, form, nblk, K, (nh, nkv, nwg)) in enumerate(launches):
        rs = np.random.RandomState(400 + i)
        N, x, w, bias, pos, rc, rs_ = _qkv_inputs(rs, dt, nblk, K, nh, nkv)
        assert (nh + 2 * nkv) * 64 // nwg == 5
        wp, xp = _qkv_image(w, nh, nkv, nwg), _pack_blocks(x)
        for tag, b in (('nobias', None), ('bias', bias)):
            qf, kf, vf = _fragments(dt, nblk, nh, nkv)
            if entry == 'mb':
                _mb(L, 2, wp, xp, N, K, nblk, nwg, bias=b, pos=pos, rc=rc, rs_=rs_, qf=qf, kf=kf, vf=vf, nh=nh, nkv=nkv)
            elif b is None:
                check(L.la_gemm64r_qkv(sp(), ptr(wp), ptr(xp), nh, nkv, K, nwg, ptr(pos), ptr(rc), ptr(rs_), ptr(qf), ptr(kf), ptr(vf)), 'qkv_r')
            else:
                check(L.la_gemm64r_qkv_bias(sp(), ptr(wp), ptr(xp), nh, nkv, K, nwg, ptr(pos), ptr(rc), ptr(rs_), ptr(qf), ptr(kf), ptr(vf), ptr(b)), 'qkv_r')
            torch.cuda.synchronize()
            key = f'{entry}/{form}/nblk{nblk}/{(nh, nkv, nwg)}/{tag}'
            _check_qkv_against_torch(key, nblk, nh, nkv, x, w, b, pos, qf, kf, vf)
            out[key] = _sha(qf, kf, vf)
    return out


def classic_digests(name):
    dt, out = DTYPES[name], {}
    L = _lib.lib_for(dt)
    nh, nkv = 4, 2
    rs = np.random.RandomState(70)
    N, x, w, _, pos, rc, rs_ = _qkv_inputs(rs, dt, 1, HIDDEN, nh, nkv)
    wp, xp = _qkv_image(w, nh, nkv, 0), gu.pack_x(_bits(x))
    for variant in (0, 2):
        o = _fragments(dt, 1, nh, nkv)
        check(L.la_gemm64_qkv(sp(), ptr(wp), ptr(xp), nh, nkv, HIDDEN, ptr(pos), ptr(rc), ptr(rs_), *[ptr(t) for t in o], variant), 'qkv')
        torch.cuda.synchronize()
        out[f'qkv/variant{variant}'] = _sha(*o)
    # the planned 64-row kernel's one-pass form (R = 24: a multiple of 4) and both kernels on fp8 weights: prologue_digests.json holds them
    # in bf16 only, and the fp16 build's RoPE rounding is the compiler's choice per kernel (csrc/la_epilogue.h, rope_half)
    from painlessinferenceacceleration_amd.llama_engine import quantize_fp8
    from tests.test_gpu_fp8 import pack8, pack_planned8
    nwg = 16
    bias = _randn(rs, dt, N, scale=0.5)
    q8, s8 = quantize_fp8(w.to(torch.bfloat16))
    perm = np.zeros(N, dtype=np.int32)
    check(L.la_qkv_row_perm(nh, nkv, perm.ctypes.data_as(_lib.pi32)), 'perm')
    images = {'planned': gu.pack_planned(2, [_bits(w)], nwg), 'planned_fp8': pack_planned8(L, 2, [q8], nwg),
              'classic_fp8': pack8(L, q8.view(torch.uint8)[torch.from_numpy(perm.astype(np.int64)).to(DEV)].contiguous().view(torch.float8_e4m3fn))}
    for form, wq in images.items():
        for tag, b in (('nobias', None), ('bias', bias)):
            o = _fragments(dt, 1, nh, nkv)
            tail = (ptr(pos), ptr(rc), ptr(rs_), *[ptr(t) for t in o], ptr(b))
            if form == 'planned':
                check(L.la_gemm64r_qkv_bias(sp(), ptr(wq), ptr(xp), nh, nkv, HIDDEN, nwg, *tail), 'qkv_r')
            elif form == 'planned_fp8':
                check(L.la_gemm64r_qkv_fp8(sp(), ptr(wq), ptr(xp), nh, nkv, HIDDEN, nwg, *tail, ptr(s8)), 'qkv8_r')
            else:
                check(L.la_gemm64_qkv_fp8(sp(), ptr(wq), ptr(xp), nh, nkv, HIDDEN, *tail, ptr(s8)), 'qkv8')
            torch.cuda.synchronize()
            out[f'qkv/{form}/{tag}'] = _sha(*o)
    F = 352
    rs = np.random.RandomState(71)
    x, wg, wu = _randn(rs, dt, 64, HIDDEN), _randn(rs, dt, F, HIDDEN, scale=0.05), _randn(rs, dt, F, HIDDEN, scale=0.05)
    act = torch.zeros(64 * F, dtype=dt, device=DEV)
    check(L.la_gemm64_swiglu(sp(), ptr(gu.pack_weight(_bits(wg), _bits(wu))), ptr(gu.pack_x(_bits(x))), F, HIDDEN, ptr(act), 2), 'swiglu')
    torch.cuda.synchronize()
    out['swiglu/variant2'] = _sha(act)
    V = 960
    rs = np.random.RandomState(72)
    x, w = _randn(rs, dt, 64, HIDDEN), _randn(rs, dt, V, HIDDEN, scale=0.05)
    wp, xp = gu.pack_weight(_bits(w)), gu.pack_x(_bits(x))
    for waves, rbv in ((4, 1), (8, 1 | 1 << 8)):
        n_tiles = V // 32 * (waves // 2)                   # one candidate per (workgroup, register-group owner)
        logits = torch.zeros(64, V, dtype=dt, device=DEV)
        cv = torch.zeros(n_tiles * 64, dtype=torch.float32, device=DEV)
        ci = torch.zeros(n_tiles * 64, dtype=torch.int32, device=DEV)
        state = torch.zeros(_lib.LA_ST_WORDS, dtype=torch.int32, device=DEV)
        check(L.la_gemm64_logits(sp(), ptr(wp), ptr(xp), V, HIDDEN, rbv, ptr(logits), ptr(cv), ptr(ci)), 'logits')
        check(L.la_argmax_finalize(sp(), ptr(cv), ptr(ci), n_tiles, ptr(state)), 'argmax')
        torch.cuda.synchronize()
        am = state[_lib.LA_ST_ARGMAX:_lib.LA_ST_ARGMAX + 64]
        assert np.array_equal(am.cpu().numpy(), np.argmax(logits.float().cpu().numpy(), axis=-1)), 'the first maximum of the stored row'
        out[f'logits/rb1/w{waves}'] = _sha(logits, cv, ci, am)
    return out


GROUPS = {f'{group}_{name}': (lambda fn=fn, name=name: fn(name))
          for group, fn in (('forms', form_digests), ('odd_r', odd_r_digests), ('classic', classic_digests)) for name in DTYPES}


def record_all():
    """the fixture's content, from whatever libraries lie beside the package; LA_RECORD_DIRTY=1 first fills the allocator's memory with
    non-zero bytes, so that a launch that leaves part of a buffer unwritten (or reads a padding it should not) shows as another digest"""
    if os.environ.get('LA_RECORD_DIRTY', '') not in ('', '0'):
        junk = [torch.full((1 << 28,), 0xA5, dtype=torch.uint8, device=DEV) for _ in range(4)]
        torch.cuda.synchronize()
        del junk
    d = {name: fn() for name, fn in GROUPS.items()}
    d['cu_count'] = int(torch.cuda.get_device_properties(0).multi_processor_count)
    return d


@pytest.fixture(scope='module')
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_holds_the_cases_it_was_chosen_for(golden):
    assert len(golden['forms_bf16']) == len(golden['forms_fp16']) == len(FORM_CASES) == 38
    for name in DTYPES:
        assert len(golden[f'odd_r_{name}']) == 2 * (len(ODD_R_CASES) + 2)
        assert sorted(golden[f'classic_{name}']) == ['logits/rb1/w4', 'logits/rb1/w8'] + [f'qkv/{f}/{t}' for f in ('classic_fp8', 'planned', \
            'planned_fp8') for t in ('bias', 'nobias')] + ['qkv/variant0', 'qkv/variant2', 'swiglu/variant2']
        for k, v in golden[f'odd_r_{name}'].items():          # what must differ does: a bias ...
            if k.endswith('/bias'):
                assert v != golden[f'odd_r_{name}'][k[:-len('bias')] + 'nobias']
    for group in ('forms', 'odd_r', 'classic'):              # ... and the two storage types
        assert not set(golden[f'{group}_bf16'].values()) & set(golden[f'{group}_fp16'].values())


@pytest.mark.parametrize('group', list(GROUPS))
def test_epilogue_digests_match_the_recorded_ones(golden, group):
    assert torch.cuda.get_device_properties(0).multi_processor_count == golden['cu_count'], \
        'launch forms follow the CU count: the digests hold for the recorded one only'
    got = json.loads(json.dumps(GROUPS[group]()))
    want = golden[group]
    assert sorted(got) == sorted(want)
    diff = [k for k in sorted(want) if got[k] != want[k]]
    assert not diff, (group, len(diff), diff[:8])
