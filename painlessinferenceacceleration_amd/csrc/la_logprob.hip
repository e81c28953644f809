// la_logprob.hip — per-token log-probabilities on the device: the model's own log-softmax value of every token a step emits, taken
// over the raw logits lm_head wrote, AFTER the accept scan of the step (the scan decides which rows emit).
//
//   lp = (x_t - m) - log(sum_v exp(x_v - m))       x = the row of stored 16-bit logits widened to fp32, raw (before any penalty,
//                                                  temperature or filter), m = the row maximum, t = the row's ARGMAX word (the
//                                                  argmax, the penalised argmax or the sampled token: whatever the walk compared)
// The sum is the 64-bit INTEGER mass la_sample.hip uses for top-p: q_v = floor(expf(x_v - m) * 2^32) (the maximum: exactly 2^32),
// added as integers — order-independent, so the value has the same bits for the same row of logits on every run and every step form.
// lp = (x_t - m) - logf(float(Z * 2^-32)).  Error against the exact value: V * 2^-32 (the floors, against Z >= 1) + the fp32
// roundings of the two subtractions (2^-22 |lp|) + a few ulps of expf / logf.
//
// One workgroup of 1024 threads per (row, block); row addressing and liveness: pen_row (la_rows.h).  A workgroup works only when its
// row is live AND the scan kept it — the root and the accepted rows (their picks are the path tokens and the bonus: exactly the
// emitted tokens), or the emitting row of a prefill chain.  Sibling rows share a position, so a dropped row must never store.  The
// value goes to log[slot][pos[row] + 1]: the index, in the unpadded sequence, of the token being chosen (the sampler's Philox
// counter) — no counter, no ordering between workgroups.  The row is read twice (maximum, mass) with 16-byte loads, four in flight.
#include "la_common.h"
#include "la_kernels.h"
#include "la_mblock.h"
#include "la_rows.h"

#define LP_THREADS 1024
typedef unsigned long long u64;

// every 16-byte chunk of the row: f(values[8]); four chunks per thread and round in flight
template <typename F>
__device__ __forceinline__ void lp_scan(const bf16_t* __restrict__ lg, int nchunk, F&& f) {
    const int tid = (int)threadIdx.x;
    for (int base = tid; base < nchunk; base += 4 * LP_THREADS) {
        bf16x8 x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = base + k * LP_THREADS;
            x[k] = *(const bf16x8*)(lg + (size_t)(c < nchunk ? c : base) * 8);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (base + k * LP_THREADS >= nchunk) break;
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = bf2f((bf16_t)x[k][e]);
            f(v);
        }
    }
}

// did the accept scan of this step keep the row?  (block-uniform)
__device__ __forceinline__ bool lp_kept(const PenArgs& a, const PenRow& r) {
    if (a.kind == LA_PEN_SINGLE) {
        const int j = (int)blockIdx.x;
        if (j == 0) return true;                                               // the root always emits
        int n = a.state[LA_ST_NCOMMIT];
        n = n < LA_TREE_MAX ? n : LA_TREE_MAX;
        bool kept = false;
        for (int i = 0; i < n; ++i) kept = kept || a.state[LA_ST_SRCIDX + i] == j;
        return kept;
    }
    if (a.kind == LA_PEN_BATCH) return a.state[LA_BST_DST + r.row] >= 0;
    if (a.kind == LA_PEN_MBLOCK) return a.state[LA_MOUT_DST + r.row] >= 0;
    return true;                                                               // LA_PEN_ROWS: every row (unit entry)
}

__global__ __launch_bounds__(LP_THREADS) void k_logprob_rows(const LpArgs a) {
    __shared__ float red_m[LP_THREADS / 64];
    __shared__ u64 red_z[LP_THREADS / 64];
    const PenRow r = pen_row(a.p);
    if (!r.live || !lp_kept(a.p, r)) return;                                   // block-uniform
    const int tid = (int)threadIdx.x, vocab = a.p.vocab, nchunk = vocab >> 3;
    const bf16_t* lg = (const bf16_t*)a.p.logits + (size_t)r.row * vocab;

    // ---- the row maximum
    float m = -INFINITY;
    lp_scan(lg, nchunk, [&](const float* v) {
#pragma unroll
        for (int e = 0; e < 8; ++e) m = v[e] > m ? v[e] : m;
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const float t = __shfl_xor(m, o, 64); m = t > m ? t : m; }
    if ((tid & 63) == 0) red_m[tid >> 6] = m;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < LP_THREADS / 64; ++w) m = red_m[w] > m ? red_m[w] : m;

    // ---- the integer mass
    u64 z = 0;
    lp_scan(lg, nchunk, [&](const float* v) {
#pragma unroll
        for (int e = 0; e < 8; ++e) z += (u64)(expf(v[e] - m) * 4294967296.f);
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)z, o, 64), hi = __shfl_xor((unsigned)(z >> 32), o, 64);
        z += ((u64)hi << 32) | lo;
    }
    if ((tid & 63) == 0) red_z[tid >> 6] = z;
    __syncthreads();
    if (tid != 0) return;
    z = 0;
#pragma unroll
    for (int w = 0; w < LP_THREADS / 64; ++w) z += red_z[w];
    const int tok = a.p.out[r.row];
    float lp = __builtin_nanf("");
    if (tok >= 0 && tok < vocab) lp = (bf2f(lg[tok]) - m) - logf((float)((double)z * (1.0 / 4294967296.0)));
    if (a.log) {
        const int at = a.pos[r.row] + 1;                   // outside the log: nothing stored (the limit stated in lookahead_hip.h)
        if (at >= 0 && at < a.stride && r.slot >= 0 && r.slot < a.p.n_slots) a.log[(size_t)r.slot * a.stride + at] = lp;
    } else {
        a.out[r.row] = lp;
    }
}

int lk_logprob_rows(hipStream_t st, const LpArgs& a) {
    if (a.p.vocab <= 0 || (a.p.vocab & 7) || (!a.log && !a.out) || (a.log && (!a.pos || a.stride <= 0))) return -1;
    const int blocks = a.p.kind == LA_PEN_MBLOCK ? a.p.nblk : 1;
    if (blocks < 1 || blocks > LA_MB_MAX) return -1;
    k_logprob_rows<<<dim3(LA_TB, blocks), LP_THREADS, 0, st>>>(a);
    return (int)hipGetLastError();
}
