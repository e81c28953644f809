// la_select.h — the exact radix select the row stages share (la_sample.hip: the top-k / top-p thresholds; la_logprob.hip: the top-N
// list): the monotone 16-bit key of a stored logit, and the suffix-sum search over one 256-bin histogram level kept in LDS in 8
// interleaved copies (lane & 7), so that the few bins a row of logits really populates do not serialise a whole wave on one address.
#pragma once
#include "la_common.h"

#define SAMP_COPIES 8

// storage bits -> monotone key (0 = NaN: never kept); key -> value
__device__ __forceinline__ unsigned samp_key(bf16_t b) {
    unsigned u = b;
    const unsigned mag = u & 0x7fffu;
    if (mag > (LA_DTYPE == 1 ? 0x7c00u : 0x7f80u)) return 0u;
    if (mag == 0u) u = 0u;
    return (u & 0x8000u) ? (~u & 0xffffu) : (u | 0x8000u);
}
__device__ __forceinline__ float samp_val(unsigned key) {
    return bf2f((bf16_t)((key & 0x8000u) ? (key & 0x7fffu) : (~key & 0xffffu)));
}

__device__ __forceinline__ unsigned long long shfl_up64(unsigned long long v, int o) {
    const unsigned lo = __shfl_up((unsigned)v, o, 64), hi = __shfl_up((unsigned)(v >> 32), o, 64);
    return ((unsigned long long)hi << 32) | lo;
}

// Wave 0, after the 8 copies of a 256-bin histogram are complete: the HIGHEST bin b whose suffix sum S(b) = sum_{j >= b} h[j] reaches the
// target, and the sum above it.  frac < 0: the target is `target`; else target = max(1, floor(frac * total)) and *s_target receives it.
// sel[0] = bin or -1 (the target is never reached), sel64[0] = S(b + 1), sel64[1] = the target used.
__device__ __forceinline__ void samp_select(const unsigned long long* hist, bool as_u32, unsigned long long target, double frac, int* sel,
                                            unsigned long long* sel64) {
    typedef unsigned long long u64;
    const int lane = (int)threadIdx.x;                 // < 64
    u64 h[4], loc = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int b = 255 - 4 * lane - j;
        u64 s = 0;
        if (as_u32) { for (int c = 0; c < SAMP_COPIES; ++c) s += ((const unsigned*)hist)[b * SAMP_COPIES + c]; }
        else { for (int c = 0; c < SAMP_COPIES; ++c) s += hist[b * SAMP_COPIES + c]; }
        h[j] = s; loc += s;
    }
    u64 inc = loc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 t = shfl_up64(inc, o);
        if (lane >= o) inc += t;
    }
    if (frac >= 0.0) {
        const unsigned tlo = __shfl((unsigned)inc, 63, 64), thi = __shfl((unsigned)(inc >> 32), 63, 64);
        const u64 total = ((u64)thi << 32) | tlo;
        target = (u64)(frac * (double)total);
        if (target < 1) target = 1;
    }
    u64 run = inc - loc, above = 0;
    int hit = -1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (hit < 0 && run + h[j] >= target) { hit = 255 - 4 * lane - j; above = run; }
        run += h[j];
    }
    const unsigned long long bal = __ballot(hit >= 0);
    if (bal == 0ull) { if (lane == 0) { sel[0] = -1; sel64[0] = 0; sel64[1] = target; } }
    else if (lane == __builtin_ctzll(bal)) { sel[0] = hit; sel64[0] = above; sel64[1] = target; }
}
