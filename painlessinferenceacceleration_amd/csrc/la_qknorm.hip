// la_qknorm.hip — per-head q / k RMSNorm + RoPE (Qwen3: Qwen3Attention.forward applies q_norm / k_norm, an RMSNorm over the head's 128
// features, to the q_proj / k_proj output BEFORE apply_rotary_pos_emb), as ONE stage between the QKV launch and the attention launch.
//
// Why a stage and not a QKV epilogue: a QKV workgroup owns at most 32 RoPE pairs of a head (la_mb_forms.h; pr = R * bx + f0 in
// gemm64r_body), so a head's 128 features are finished by two or more workgroups and none of them ever holds the head's sum of
// squares.  The QKV launch of a qk_norm model therefore runs with IDENTITY RoPE tables (cos = 1, sin = 0: rope_half(x, xr, 1, 0) = x
// exactly, in both builds) and leaves round(x W^T) in the QF / fresh KF fragments; this kernel finishes them in place:
//   f      the 128 stored values of one (block, q or k head, token row)
//   n      = storage(f * rsqrt(mean(f^2) + eps))          fp32 mean of squares, one rounding        (Qwen3RMSNorm.forward: the
//   y      = storage(w * n)                               the cast-first flavour                      normalised value is cast first)
//   out    = rope_half(y, rot(y), cos, sin)               the real [position][64] tables: two rounded products, one rounded sum
// V is not touched.  One workgroup per (head slot, 64-row block), 256 threads, four lanes per token: lane j owns the 16-byte chunks
// {2j, 2j + 1, 2j + 8, 2j + 9} of its token row, i.e. features [16j, 16j + 16) and their rotary partners [64 + 16j, 64 + 16j + 16),
// so every (d, d + 64) pair and its cos / sin run sit in one lane and the sum of squares closes with two cross-lane steps.  No LDS;
// four 16-byte fragment loads and stores per lane.  The dependent pos -> cos / sin loads are issued first (as k_qkv_post does).
#include "la_common.h"
#include "la_kernels.h"
#include "la_epilogue.h"

__global__ __launch_bounds__(256) void k_qk_norm_rope(bf16_t* __restrict__ qf, bf16_t* __restrict__ kfresh, int nh, int nkv,
                                                       const bf16_t* __restrict__ qw, const bf16_t* __restrict__ kw, float eps,
                                                       const int* __restrict__ pos, const bf16_t* __restrict__ rcos,
                                                       const bf16_t* __restrict__ rsin) {
    const int slot = blockIdx.x, blk = blockIdx.y;                 // slot: [q heads | k heads]
    const int tok = threadIdx.x >> 2, j = threadIdx.x & 3;
    const int ps = pos[blk * LA_TB + tok];
    bf16x8 cs[2], sn[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        cs[i] = *(const bf16x8*)(rcos + (size_t)ps * 64 + 16 * j + 8 * i);
        sn[i] = *(const bf16x8*)(rsin + (size_t)ps * 64 + 16 * j + 8 * i);
    }
    const bool is_q = slot < nh;
    bf16_t* base = is_q ? qf + ((size_t)blk * nh + slot) * 8192 : kfresh + ((size_t)blk * nkv + (slot - nh)) * 8192;
    const bf16_t* w = is_q ? qw : kw;
    bf16x8 x[2][2], wv[2][2];                                      // [half: d, d + 64][chunk of the lane's 16 features]
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int d = 64 * h + 16 * j + 8 * i;
            x[h][i] = *(const bf16x8*)(base + rf_offset(tok, d));
            wv[h][i] = *(const bf16x8*)(w + d);
        }
    float ss = 0.f;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float f = bf2f((bf16_t)x[h][i][e]); ss += f * f; }
    ss += __shfl_xor(ss, 1, 64);
    ss += __shfl_xor(ss, 2, 64);
    const float rs = rsqrtf(ss * (1.0f / 128.0f) + eps);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        bf16x8 olo, ohi;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float yl = bfr(bf2f((bf16_t)wv[0][i][e]) * bfr(bf2f((bf16_t)x[0][i][e]) * rs));
            const float yh = bfr(bf2f((bf16_t)wv[1][i][e]) * bfr(bf2f((bf16_t)x[1][i][e]) * rs));
            const float c = bf2f((bf16_t)cs[i][e]), s = bf2f((bf16_t)sn[i][e]);
            olo[e] = (short)rope_half(yl, -yh, c, s);
            ohi[e] = (short)rope_half(yh, yl, c, s);
        }
        *(bf16x8*)(base + rf_offset(tok, 16 * j + 8 * i)) = olo;
        *(bf16x8*)(base + rf_offset(tok, 64 + 16 * j + 8 * i)) = ohi;
    }
}

int lk_qk_norm_rope(hipStream_t st, void* qf, void* kfresh, int nblk, int nh, int nkv, const void* qw, const void* kw, float eps,
                    const int* pos, const void* rcos, const void* rsin) {
    if (nblk < 1 || nblk > LA_MB_MAX || nh < 1 || nkv < 1) return -1;
    k_qk_norm_rope<<<dim3(nh + nkv, nblk), 256, 0, st>>>((bf16_t*)qf, (bf16_t*)kfresh, nh, nkv, (const bf16_t*)qw, (const bf16_t*)kw, eps,
                                                         pos, (const bf16_t*)rcos, (const bf16_t*)rsin);
    return (int)hipGetLastError();
}
