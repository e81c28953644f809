# -*- coding: utf-8 -*-
"""The K range of a slab launch's split without a division (la_krange_magic / la_krange_bound, csrc/la_common.h): a stand-alone host
program, compiled from the header the kernels include, compares the multiply-high form with (long)K16 * ks / ksplit over the whole
domain the launchers may promise — every 1 <= K16 <= 4096, 1 <= ksplit <= 8, 0 <= ks <= ksplit — and checks that the launcher's
guarantee (magic != 0) covers that domain, that a magic of 0 takes the division, and that the guarantee is never given where the
proof in the header does not hold.  Any other partition of K would change the summation order of every split-K GEMM."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'painlessinferenceacceleration_amd', 'csrc')

PROGRAM = r'''
#include "la_common.h"
#include <cstdio>
int main() {
    long checked = 0;
    for (int K16 = 1; K16 <= 4096; ++K16)
        for (int ksplit = 1; ksplit <= 8; ++ksplit) {
            const unsigned magic = la_krange_magic(K16, ksplit);
            if (magic == 0u) { printf("no magic at K16=%d ksplit=%d\n", K16, ksplit); return 1; }
            for (int ks = 0; ks <= ksplit; ++ks, ++checked) {
                const int want = (int)(((long)K16 * ks) / ksplit);
                const int got = la_krange_bound(K16, ks, ksplit, magic);
                if (got != want) { printf("K16=%d ks=%d ksplit=%d: %d != %d\n", K16, ks, ksplit, got, want); return 1; }
                if (la_krange_bound(K16, ks, ksplit, 0u) != want) { printf("division form differs\n"); return 1; }
            }
        }
    // past the domain: wherever a magic is given it is exact (spot rows up to the limits of a launch), and none is given past the proof
    const int big_k[] = {4097, 65536, 1000003, 16777216, 2147483647 / 16};
    const int big_s[] = {1, 2, 3, 7, 8, 16, 100, 1023, 65535};
    for (int K16 : big_k)
        for (int ksplit : big_s) {
            const unsigned magic = la_krange_magic(K16, ksplit);
            const bool provable = (long long)K16 * ksplit * ksplit < (1ll << 31);
            if ((magic != 0u) != provable) { printf("guarantee at K16=%d ksplit=%d: %u\n", K16, ksplit, magic); return 1; }
            for (int ks = 0; ks <= ksplit; ks += (ksplit > 64 ? 61 : 1), ++checked)
                if (la_krange_bound(K16, ks, ksplit, magic) != (int)(((long)K16 * ks) / ksplit)) { printf("big K16=%d ks=%d ksplit=%d\n", K16, ks, ksplit); return 1; }
        }
    if (la_krange_magic(0, 4) != 0u || la_krange_magic(64, 0) != 0u) { printf("degenerate launch got a magic\n"); return 1; }
    printf("ok %ld\n", checked);
    return 0;
}
'''


def test_krange_magic_equals_the_division_over_the_whole_domain(tmp_path):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not os.path.exists(hipcc):
        hipcc = shutil.which('hipcc')
    assert hipcc, 'hipcc builds the library; the same compiler builds this host program'
    src = tmp_path / 'krange.cpp'
    src.write_text(PROGRAM)
    exe = tmp_path / 'krange'
    # host pass only: the header's __device__ helpers are parsed, nothing is compiled for or run on a GPU
    subprocess.run([hipcc, '-x', 'hip', '--cuda-host-only', '-nogpulib', '-O1', '-std=c++17', '-I', CSRC, str(src), '-o', str(exe)],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith('ok '), r.stdout + r.stderr
    assert int(r.stdout.split()[1]) >= 4096 * 44
