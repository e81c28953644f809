# -*- coding: utf-8 -*-
"""Which kernel instantiation a multi-block GEMM launch runs (la_mb_select / kMbForms, csrc/la_mb_forms.h), pinned on the CPU: a
stand-alone host program, compiled from the header la_mblock.hip includes — once as the product build and once as the lab build —
(1) answers every input tuple of tests/golden/mb_launch_forms.json, recorded from the launches of the commit before the selector
existed (scripts/mb_launch_trace.py), and (2) sweeps a whole domain of tuples and knob values and checks what must hold for every
answer.  The launch forms are mostly bit-identical to one another, so no result test notices a slipped condition: this one does."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'painlessinferenceacceleration_amd', 'csrc')
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'mb_launch_forms.json')
FIELDS = ('kind', 'nblk', 'n_wg', 'ksplit', 'K16', 'N', 'R', 'planned', 'gu_interleaved', 'ex_n', 'nblk_dev', 'bias')

PROGRAM = r'''
#include "la_mb_forms.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "la_knobs.h"
#define LA_KNOB_DEFAULT(name, dflt, key, lo, hi) static constexpr int dflt_##name = dflt;
LA_KNOB_TABLE(LA_KNOB_DEFAULT)
static MbFormKnobs defaults() { return MbFormKnobs{dflt_g_la_mb_pair, dflt_g_la_mb_narrow, dflt_g_la_mb_dbg, dflt_g_la_mb_sch, dflt_g_la_mb_ks2, dflt_g_la_ex_d4, dflt_g_la_fatd, dflt_g_la_fatx}; }
static bool reached[MBF_COUNT];
static long answers = 0, refusals = 0;
static int fail(const char* what, const MbFormIn& s, const MbFormKnobs& k, const MbForm& f) {
    printf("%s: kind=%d nblk=%d n_wg=%d ksplit=%d K16=%d N=%d R=%d planned=%d gu=%d ex_n=%d nblk_dev=%d bias=%d | pair=%d narrow=%d dbg=%d sch=%d ks2=%d ex_d4=%d fatd=%d fatx=%d -> id=%d grid=%u,%u,%u\n",
           what, s.kind, s.nblk, s.n_wg, s.ksplit, s.K16, s.N, s.R, s.planned, s.gu_interleaved, s.ex_n, s.nblk_dev, s.bias,
           k.pair, k.narrow, k.dbg, k.sch, k.ks2, k.ex_d4, k.fatd, k.fatx, f.id, f.gx, f.gy, f.gz);
    return 1;
}
// `complete`: every form the selector can want is a row of this build's table (the lab build always; the product build at its defaults)
static int check(const MbFormIn& s, const MbFormKnobs& k, bool complete) {
    const MbForm f = la_mb_select(s, k);
    ++answers;
    const bool must_refuse = (s.ksplit > 1 && s.K16 < 2 * s.ksplit) || (s.bias && k.dbg == 4);
    if (f.id < -1 || f.id >= MBF_COUNT) return fail("not a table row", s, k, f);
    if (must_refuse && f.id != -1) return fail("launched what must be refused", s, k, f);
    if (f.id == -1) { ++refusals; return (complete && !must_refuse) ? fail("refused a launch this build has every form for", s, k, f) : 0; }
    reached[f.id] = true;
    const MbFormRow& r = kMbForms[f.id];
    if (f.gx == 0 || f.gy == 0 || f.gz == 0) return fail("empty grid", s, k, f);
    if (r.lds > 160 * 1024 || r.lds <= 0 || (r.block != 256 && r.block != 512)) return fail("LDS / block", s, k, f);
    const int fam = (int)(r.key & 15);
    if ((fam == MBK_FAT || fam == MBK_FATD) && ((s.K16 & 1) || s.K16 < 2 * s.ksplit)) return fail("fat form with an odd K16 or an empty split", s, k, f);
    if (f.regions != 1 && f.regions != 2 && f.regions != 4) return fail("regions", s, k, f);
    if ((long)f.gx * f.regions != s.n_wg) return fail("grid.x x regions != workgroup regions", s, k, f);
    return 0;
}
static int sweep_tuples(const MbFormKnobs& k, bool complete) {
    static const int n_wgs[] = {15, 16, 32, 96, 128, 160, 256};
    for (int kind = 0; kind <= 3; ++kind)
    for (int nblk = 1; nblk <= 8; ++nblk)
    for (int n_wg : n_wgs)
    for (int ksplit = 1; ksplit <= 8; ++ksplit) {
        const int k16s[] = {2 * ksplit - 1, 2 * ksplit, 2 * ksplit + 1, 64, 65, 256};
        for (int K16 : k16s)
        for (int r4 = 0; r4 < 3; ++r4)                    // R = 2 mod 4, 0 mod 4, and a small one (few weight bytes per workgroup: the quad QKV form)
        for (int planned = 0; planned < 2; ++planned)
        for (int ex = 0; ex < 3; ++ex)                    // host block count; device block count of one expert; of 8 merged experts
        for (int bias = 0; bias < (kind == MB_QKV ? 2 : 1); ++bias) {
            if (ex == 2 && kind > 1) continue;           // lk_mb_gemm: merged experts are slab / gate-up launches
            MbFormIn s{};
            s.kind = kind; s.nblk = nblk; s.n_wg = n_wg; s.ksplit = ksplit; s.K16 = K16; s.planned = planned && kind != MB_SLAB;
            const int Rp[4][3] = {{2, 0, 0}, {42, 64, 36}, {30, 32, 8}, {98, 128, 100}}, Rc[4] = {0, 64, 32, 128};
            s.R = s.planned ? Rp[kind][r4] : Rc[kind];
            s.gu_interleaved = kind == MB_SWIGLU && !s.planned;
            s.N = kind == MB_SLAB ? n_wg * 64 : kind == MB_QKV ? n_wg * s.R * 2 : n_wg * s.R;
            s.ex_n = ex == 2 ? 8 : 1; s.nblk_dev = ex > 0; s.bias = bias;
            if (check(s, k, complete)) return 1;
        }
    }
    return 0;
}
int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "answer")) {       // one tuple per line of the file -> "name gx gy gz lds" (or "refuse")
        FILE* fp = fopen(argv[2], "r");
        if (!fp) return 2;
        MbFormIn s{};
        while (fscanf(fp, "%d %d %d %d %d %d %d %d %d %d %d %d", &s.kind, &s.nblk, &s.n_wg, &s.ksplit, &s.K16, &s.N, &s.R, &s.planned,
                      &s.gu_interleaved, &s.ex_n, &s.nblk_dev, &s.bias) == 12) {
            const MbForm f = la_mb_select(s, defaults());
            if (f.id < 0) printf("refuse\n");
            else printf("%s %u %u %u %d\n", kMbForms[f.id].name, f.gx, f.gy, f.gz, kMbForms[f.id].lds);
        }
        fclose(fp);
        return 0;
    }
    // keys at their defaults, then every bit of key 6 flipped and every other value of keys 3, 4, 12, 24, 25, 35, 36
    if (sweep_tuples(defaults(), true)) return 1;
    printf("default-forms");
    for (int i = 0; i < MBF_COUNT; ++i) if (reached[i]) printf(" %s", kMbForms[i].name);
    printf("\n");
    for (int bit = 0; bit < 15; ++bit) { MbFormKnobs k = defaults(); k.pair ^= 1 << bit; if (sweep_tuples(k, LA_LAB)) return 1; }
    for (int v = 0; v <= 1; ++v) {
        MbFormKnobs k = defaults(); k.narrow = v; if (sweep_tuples(k, LA_LAB)) return 1;
        k = defaults(); k.sch = v; if (sweep_tuples(k, LA_LAB)) return 1;
        k = defaults(); k.ks2 = v; if (sweep_tuples(k, LA_LAB)) return 1;
        k = defaults(); k.fatd = v; if (sweep_tuples(k, LA_LAB)) return 1;
        k = defaults(); k.fatx = v; if (sweep_tuples(k, LA_LAB)) return 1;
        // the forms behind two knobs at once: the paired gate/up fat launch needs bit 6 of key 6 off below 5 blocks, schedule 0 reaches every wide form
        k = defaults(); k.fatd = v; k.pair &= ~64; if (sweep_tuples(k, LA_LAB)) return 1;
        k = defaults(); k.sch = 0; k.pair = v ? (k.pair | 4) & ~(32 | 64 | 256) : k.pair & ~(16 | 32 | 64 | 256); if (sweep_tuples(k, LA_LAB)) return 1;
        k = defaults(); k.pair = v ? (k.pair | 2048) & ~64 : (k.pair | 512); if (sweep_tuples(k, LA_LAB)) return 1;
    }
    for (int v = 0; v <= 6; ++v) { MbFormKnobs k = defaults(); k.dbg = v; if (sweep_tuples(k, LA_LAB)) return 1; }
    for (int v = 0; v <= 15; ++v) { MbFormKnobs k = defaults(); k.ex_d4 = v; if (sweep_tuples(k, LA_LAB)) return 1; }
    printf("all-forms");
    for (int i = 0; i < MBF_COUNT; ++i) if (reached[i]) printf(" %s", kMbForms[i].name);
    printf("\ntable");
    for (int i = 0; i < MBF_COUNT; ++i) printf(" %s", kMbForms[i].name);
    printf("\nok %ld %ld\n", answers, refusals);
    return 0;
}
'''


@pytest.fixture(scope='module')
def programs(tmp_path_factory):
    """{0: product build, 1: lab build} of the host program."""
    cxx = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not os.path.exists(cxx):
        cxx = shutil.which('hipcc')
    assert cxx, 'hipcc builds the library; the same compiler builds this host program'
    d = tmp_path_factory.mktemp('mb_forms')
    (d / 'mb_forms.cpp').write_text(PROGRAM)
    exes = {}
    for lab in (0, 1):
        exes[lab] = d / f'mb_forms_{lab}'
        # plain host C++: the header includes nothing of HIP
        subprocess.run([cxx, '-x', 'c++', '-O1', '-std=c++17', f'-DLA_LAB={lab}', '-I', CSRC, str(d / 'mb_forms.cpp'), '-o', str(exes[lab])], check=True, capture_output=True, text=True)
    return exes


def _lines(exe, *args):
    r = subprocess.run([str(exe)] + list(args), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.splitlines()


@pytest.mark.parametrize('lab', [0, 1])
def test_selector_answers_the_recorded_launches(programs, tmp_path, lab):
    """Every launch recorded from the parent commit (product and lab libraries at default knobs): same form, same grid, same LDS."""
    with open(GOLDEN) as f:
        cases = json.load(f)['product' if lab == 0 else 'lab']
    assert len(cases) >= 40
    p = tmp_path / 'tuples.txt'
    p.write_text(''.join(' '.join(str(c['in'][k]) for k in FIELDS) + '\n' for c in cases))
    got = _lines(programs[lab], 'answer', str(p))
    want = ['%s %d %d %d %d' % ((c['form'],) + tuple(c['grid']) + (c['lds'],)) for c in cases]
    assert got == want


@pytest.mark.parametrize('lab', [0, 1])
def test_sweep_of_the_whole_domain(programs, lab):
    """kinds 0-3 x 1-8 blocks x n_wg {15, 16, 32, 96, 128, 160, 256} x 1-8 K splits x K16 odd and even down to 2 ksplit - 1 x R (2 | 0 mod 4, small)
    x planned / classic x host / device block count x 1 / 8 experts x bias, at the default knobs and with every bit of key 6 and every value
    of keys 3, 4, 12, 24, 25, 35, 36 changed.  The program asserts per answer: a row of this build's table or a refusal; no empty grid
    dimension; LDS <= 160 KiB; ksplit > 1 with K16 < 2 ksplit refuses; no fat form with an odd K16 or an empty split; grid.x x merged
    regions = the workgroup regions of the image; and nothing is refused for want of a table row where the build must have them all (the
    lab build everywhere, the product build at its defaults).  Here: the table holds nothing the selector cannot return in that build."""
    out = {l.split(' ', 1)[0]: l.split()[1:] for l in _lines(programs[lab])}
    assert int(out['ok'][0]) > 1000000 and 0 < int(out['ok'][1]) < int(out['ok'][0])
    table = out['table']
    assert len(set(table)) == len(table)
    if lab:
        assert set(out['all-forms']) == set(table)
        assert set(out['default-forms']) < set(table)
    else:
        assert set(out['default-forms']) == set(table) == set(out['all-forms'])


def test_gpu_form_cases_select_the_forms_they_name(programs, tmp_path):
    """tests/mb_form_cases.py (launched by tests/test_gpu_mblock.py): each case selects the form it names in the product build, and together
    they cover every row of the product table that a la_mb_gemm call can reach (all but the merged-expert rows, MB<..,1,..>)."""
    from tests.mb_form_cases import FORM_CASES, selector_input
    p = tmp_path / 'cases.txt'
    p.write_text(''.join(' '.join(str(v) for v in selector_input(*c[1:])) + '\n' for c in FORM_CASES))
    got = [l.split()[0] for l in _lines(programs[0], 'answer', str(p))]
    assert got == [c[0] for c in FORM_CASES]
    table = [l.split()[1:] for l in _lines(programs[0]) if l.startswith('table ')][0]
    assert set(got) == {n for n in table if not (n.startswith('MB<') and n.split(',')[3] == '1')}


@pytest.mark.parametrize('bias', [0, 1])
def test_odd_r_qkv_cases_select_the_one_row_per_store_forms(programs, tmp_path, bias):
    """tests/mb_form_cases.py ODD_R_CASES (launched by tests/test_gpu_epilogue_digests.py): R = 5 pairs per workgroup, with and without a
    bias, selects the three kernels that hold a one-row-per-store QKV epilogue — k_gemm_mb, and k_gemm_wide unpaired and paired."""
    from tests.mb_form_cases import ODD_R_CASES, selector_input
    p = tmp_path / 'odd_r.txt'
    p.write_text(''.join(' '.join(str(v) for v in selector_input(*c[1:], bias=bias)) + '\n' for c in ODD_R_CASES))
    for c in ODD_R_CASES:
        assert selector_input(*c[1:])[FIELDS.index('R')] == 5
    assert [l.split()[0] for l in _lines(programs[0], 'answer', str(p))] == [c[0] for c in ODD_R_CASES]
