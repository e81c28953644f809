# -*- coding: utf-8 -*-
"""One small la_mb_gemm launch per GEMM form of the product build (csrc/la_mb_forms.h), shared by tests/test_mb_forms_cpu.py — which
asserts on the CPU that each case selects the form it names and that the cases cover the product table — and
tests/test_gpu_mblock.py, which launches them.  K = 256 (16 k-tiles) or 272 (17: an odd k-tile count keeps the two-k-tile-stage fat
kernels out), N of a few workgroups, n_wg as the form requires.  The four merged-expert rows (MB<..,1,..>) need a device block count,
which la_mb_gemm does not take: the Mixtral step tests launch those.

(form, kind, nblk, K, shape): shape = N (kind 0) | (F, n_wg) (kind 1) | (nh, nkv, n_wg) (kind 2) | (V, n_wg) (kind 3); n_wg 0 = classic image."""

FORM_CASES = [
    ('MB<2,2,SLAB,0,8,0,0>', 0, 1, 256, 128), ('MB<2,4,SLAB,0,8,0,0>', 0, 2, 256, 128),
    ('WIDE<2,1,SLAB,0,2,0,0>', 0, 3, 256, 128), ('WIDE<2,2,SLAB,0,2,0,0>', 0, 5, 256, 128),
    ('WIDE<4,1,SLAB,0,2,0,0>', 0, 3, 272, 1024), ('WIDE<4,2,SLAB,0,2,0,0>', 0, 5, 272, 1024),
    ('FAT<4,1,SLAB,4,0,4,0>', 0, 3, 256, 1024), ('FAT<4,2,SLAB,4,0,4,2>', 0, 5, 256, 1024),
    ('MB<4,2,SWIGLU,0,8,0,0>', 1, 1, 256, (128, 0)), ('MB<4,4,SWIGLU,0,8,0,0>', 1, 2, 256, (128, 0)),
    ('WIDE<4,2,SWIGLU,0,2,0,0>', 1, 3, 256, (128, 0)), ('WIDE<4,3,SWIGLU,0,3,0,0>', 1, 5, 256, (128, 0)),
    ('WIDE<4,4,SWIGLU,0,3,0,0>', 1, 7, 256, (128, 0)),
    ('WIDE<8,2,SWIGLU,0,2,0,0>', 1, 3, 272, (688, 16)), ('WIDE<8,3,SWIGLU,0,3,0,0>', 1, 5, 272, (688, 16)),
    ('WIDE<8,4,SWIGLU,0,3,0,0>', 1, 7, 272, (688, 16)),
    ('FAT<4,2,SWIGLU,4,2,4,0>', 1, 3, 256, (688, 16)), ('FATD<3,0,SWIGLU,0,0,0,0>', 1, 5, 256, (688, 16)),
    ('FATD<4,0,SWIGLU,0,0,0,0>', 1, 7, 256, (688, 16)),
    ('MB<2,2,QKV,0,8,0,0>', 2, 1, 256, (2, 2, 0)), ('MB<2,4,QKV,0,8,0,0>', 2, 2, 256, (2, 2, 0)),
    ('WIDE<2,1,QKV,0,2,0,0>', 2, 3, 272, (2, 2, 0)), ('WIDE<2,2,QKV,0,2,0,0>', 2, 5, 272, (2, 2, 0)),
    ('WIDE<4,1,QKV,0,2,0,0>', 2, 3, 272, (8, 2, 32)), ('WIDE<4,2,QKV,0,2,0,0>', 2, 5, 272, (32, 8, 256)),
    ('FAT<2,1,QKV,4,0,2,0>', 2, 3, 256, (2, 2, 0)), ('FAT<2,1,QKV,2,0,2,0>', 2, 3, 256, (5, 1, 32)),
    ('FAT<2,2,QKV,4,2,2,0>', 2, 3, 256, (32, 8, 256)), ('FAT<2,2,QKV,2,2,2,0>', 2, 3, 256, (40, 40, 256)),
    ('FAT<4,1,QKV,4,0,4,0>', 2, 5, 256, (8, 2, 32)), ('FAT<4,1,QKV,2,0,4,0>', 2, 5, 256, (5, 1, 32)),
    ('FAT<4,2,QKV,4,0,4,0>', 2, 5, 256, (32, 8, 256)), ('FAT<4,2,QKV,2,0,4,0>', 2, 5, 256, (40, 40, 256)),
    ('MB<4,2,LOGITS,0,8,0,0>', 3, 1, 256, (256, 0)), ('MB<4,4,LOGITS,0,8,0,0>', 3, 2, 256, (256, 0)),
    ('WIDE<4,2,LOGITS,0,2,0,0>', 3, 3, 256, (256, 0)), ('WIDE<4,3,LOGITS,0,3,0,0>', 3, 5, 256, (256, 0)),
    ('WIDE<4,4,LOGITS,0,3,0,0>', 3, 7, 256, (256, 0)),
]

# QKV launches whose plan gives a workgroup an ODD number of RoPE pairs (R = 5): the one-row-per-store paths of the multi-block QKV
# epilogues, which no product shape reaches (R is a multiple of 4 at every model shape).  tests/test_gpu_epilogue_digests.py pins them.
ODD_R_CASES = [
    ('MB<2,2,QKV,0,8,0,0>', 2, 1, 272, (3, 1, 64)),
    ('WIDE<4,1,QKV,0,2,0,0>', 2, 3, 272, (3, 1, 64)),
    ('WIDE<4,2,QKV,0,2,0,0>', 2, 5, 272, (11, 2, 192)),
]


def selector_input(kind, nblk, K, shape, bias=0):
    """The MbFormIn tuple lk_mb_gemm derives from a la_mb_gemm call (field order of tests/test_mb_forms_cpu.py FIELDS)."""
    if kind == 0:
        N, n_wg, R, planned = shape, shape // 64, 0, 0
    elif kind == 2:
        nh, nkv, n_wg = shape
        N, planned = (nh + 2 * nkv) * 128, int(n_wg > 0)
        n_wg, R = (n_wg, (nh + 2 * nkv) * 64 // n_wg) if planned else ((nh + 2 * nkv) * 2, 32)
    else:
        N, n_wg = shape
        per = 64 if kind == 1 else 128
        planned = int(n_wg > 0)
        n_wg, R = (n_wg, N // n_wg) if planned else (N // per, per)
    return (kind, nblk, n_wg, 1, K // 16, N, R, planned, int(kind == 1 and not planned), 0, 0, bias)
