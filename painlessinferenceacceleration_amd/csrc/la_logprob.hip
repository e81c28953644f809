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
//
// Top-N (k_top_logprob_rows, launched after k_logprob_rows while la_llama_set_top_logprobs(n > 0)): for the same rows, the n tokens
// with the largest RAW logits — value descending, then token id ascending — each with (x_v - m) - logf(float(Z * 2^-32)), the same m
// and Z (the same code) as above, so the entry of the chosen token carries the bits of the scalar value.  Values compare through the
// monotone 16-bit key of la_select.h (-0 == +0, NaN never listed).  The list is a pure function of the row:
//   pass 1  the maximum + a 256-bin histogram of the keys' high bytes   -> the high byte of the threshold key T
//   pass 2  the mass + a histogram of the low bytes inside that bin     -> T, g = #(key > T) < n, c = #(key == T) >= n - g
//   c > n - g only: the (n - g) LOWEST ids among key == T by the same select over the id's bytes above the lowest (one pass per
//           byte: one up to 65 536 tokens, two up to 2^24), then one wave ballots the 256 ids that share the cut's upper bytes
//   pass 3  collect exactly the n items (key > T, or key == T and id <= the cut) into LDS — the SET is decided, so the slot an
//           item lands in is irrelevant: one wave ranks the n <= 20 items by (key descending, id ascending) and stores them
// A row with fewer than n non-NaN logits lists those and pads with (-1, NaN).
#include "la_common.h"
#include "la_kernels.h"
#include "la_mblock.h"
#include "la_rows.h"
#include "la_select.h"

#define LP_THREADS 1024
typedef unsigned long long u64;

// every 16-byte chunk of the row: f(chunk index, the 8 stored values, widened values[8]); four chunks per thread and round in flight
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
            f(base + k * LP_THREADS, x[k], v);
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

// The row maximum, in every thread (ends with a barrier).  `also` sees every chunk of the pass: (chunk index, stored values).
template <typename F>
__device__ __forceinline__ float lp_row_max(const bf16_t* __restrict__ lg, int nchunk, float* red_m, F&& also) {
    const int tid = (int)threadIdx.x;
    float m = -INFINITY;
    lp_scan(lg, nchunk, [&](int c, const bf16x8& x, const float* v) {
#pragma unroll
        for (int e = 0; e < 8; ++e) m = v[e] > m ? v[e] : m;
        also(c, x);
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const float t = __shfl_xor(m, o, 64); m = t > m ? t : m; }
    if ((tid & 63) == 0) red_m[tid >> 6] = m;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < LP_THREADS / 64; ++w) m = red_m[w] > m ? red_m[w] : m;
    return m;
}

// The integer mass of the row against its maximum, in every thread (ends with a barrier).  `also` as in lp_row_max.
template <typename F>
__device__ __forceinline__ u64 lp_row_mass(const bf16_t* __restrict__ lg, int nchunk, float m, u64* red_z, F&& also) {
    const int tid = (int)threadIdx.x;
    u64 z = 0;
    lp_scan(lg, nchunk, [&](int c, const bf16x8& x, const float* v) {
#pragma unroll
        for (int e = 0; e < 8; ++e) z += (u64)(expf(v[e] - m) * 4294967296.f);
        also(c, x);
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)z, o, 64), hi = __shfl_xor((unsigned)(z >> 32), o, 64);
        z += ((u64)hi << 32) | lo;
    }
    if ((tid & 63) == 0) red_z[tid >> 6] = z;
    __syncthreads();
    z = 0;
#pragma unroll
    for (int w = 0; w < LP_THREADS / 64; ++w) z += red_z[w];
    return z;
}

// the value of one stored logit of the row
__device__ __forceinline__ float lp_value(bf16_t x, float m, u64 z) {
    return (bf2f(x) - m) - logf((float)((double)z * (1.0 / 4294967296.0)));
}

__global__ __launch_bounds__(LP_THREADS) void k_logprob_rows(const LpArgs a) {
    __shared__ float red_m[LP_THREADS / 64];
    __shared__ u64 red_z[LP_THREADS / 64];
    const PenRow r = pen_row(a.p);
    if (!r.live || !lp_kept(a.p, r)) return;                                   // block-uniform
    const int tid = (int)threadIdx.x, vocab = a.p.vocab, nchunk = vocab >> 3;
    const bf16_t* lg = (const bf16_t*)a.p.logits + (size_t)r.row * vocab;
    auto none = [](int, const bf16x8&) {};
    const float m = lp_row_max(lg, nchunk, red_m, none);
    const u64 z = lp_row_mass(lg, nchunk, m, red_z, none);
    if (tid != 0) return;
    const int tok = a.p.out[r.row];
    float lp = __builtin_nanf("");
    if (tok >= 0 && tok < vocab) lp = lp_value(lg[tok], m, z);
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

// ---- top-N ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LP_THREADS) void k_top_logprob_rows(const TopLpArgs a) {
    __shared__ unsigned hist[256 * SAMP_COPIES];
    __shared__ float red_m[LP_THREADS / 64];
    __shared__ u64 red_z[LP_THREADS / 64];
    __shared__ u64 sel64[2];
    __shared__ int sel[2];
    __shared__ unsigned it_key[LA_TOPLP_MAX];
    __shared__ int it_id[LA_TOPLP_MAX];
    __shared__ int it_cnt, id_cut;
    const PenRow r = pen_row(a.p);
    if (!r.live || !lp_kept(a.p, r)) return;                                   // block-uniform
    const int tid = (int)threadIdx.x, vocab = a.p.vocab, nchunk = vocab >> 3, n = a.n;
    size_t dst = (size_t)r.row * n;
    if (a.log_ids) {
        const int at = a.pos[r.row] + 1;                   // outside the log: nothing stored, as the scalar stage
        if (at < 0 || at >= a.stride || r.slot < 0 || r.slot >= a.p.n_slots) return;
        dst = ((size_t)r.slot * a.stride + at) * n;
    }
    int* o_ids = (a.log_ids ? a.log_ids : a.out_ids) + dst;
    float* o_vals = (a.log_ids ? a.log_vals : a.out_vals) + dst;
    const bf16_t* lg = (const bf16_t*)a.p.logits + (size_t)r.row * vocab;
    const int cp = tid & (SAMP_COPIES - 1);
    auto zero_hist = [&]() { for (int i = tid; i < 256 * SAMP_COPIES; i += LP_THREADS) hist[i] = 0u; };
    if (tid == 0) { it_cnt = 0; id_cut = 0x7fffffff; }

    // ---- pass 1: the maximum + the high byte of the threshold key
    zero_hist();
    __syncthreads();
    const float m = lp_row_max(lg, nchunk, red_m, [&](int, const bf16x8& x) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const unsigned key = samp_key((bf16_t)x[e]);
            if (key) atomicAdd(&hist[(key >> 8) * SAMP_COPIES + cp], 1u);
        }
    });
    if (tid < 64) samp_select((const u64*)hist, true, (u64)n, -1.0, sel, sel64);
    __syncthreads();
    const int hb = sel[0];                                 // -1: fewer than n logits that are not NaN — all of them are listed
    int g = (int)sel64[0];
    __syncthreads();

    // ---- pass 2: the mass + the low byte
    zero_hist();
    __syncthreads();
    const u64 z = lp_row_mass(lg, nchunk, m, red_z, [&](int, const bf16x8& x) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const unsigned key = samp_key((bf16_t)x[e]);
            if (key && (int)(key >> 8) == hb) atomicAdd(&hist[(key & 0xffu) * SAMP_COPIES + cp], 1u);
        }
    });
    unsigned T = 1u;
    if (hb >= 0) {
        if (tid < 64) samp_select((const u64*)hist, true, (u64)(n - g), -1.0, sel, sel64);
        __syncthreads();
        const int lb = sel[0] < 0 ? 0 : sel[0];
        g += (int)sel64[0];
        T = ((unsigned)hb << 8) | (unsigned)lb;
        int ties = 0;
#pragma unroll
        for (int c = 0; c < SAMP_COPIES; ++c) ties += (int)hist[lb * SAMP_COPIES + c];
        int need = n - g;                                  // >= 1 of the `ties` tokens at T
        __syncthreads();

        // ---- more ties than places: the `need` lowest ids among key == T
        if (ties > need) {
            const int levels = vocab <= (1 << 16) ? 1 : vocab <= (1 << 24) ? 2 : 3;
            unsigned pfx = 0u;                             // the cut's id bytes above the current one
            for (int l = 0; l < levels; ++l) {
                const int sh = 8 * (levels - l);
                zero_hist();
                __syncthreads();
                lp_scan(lg, nchunk, [&](int c, const bf16x8& x, const float*) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const unsigned id = (unsigned)(c * 8 + e);
                        if (samp_key((bf16_t)x[e]) == T && (unsigned)((u64)id >> (sh + 8)) == pfx)
                            atomicAdd(&hist[(255u - ((id >> sh) & 0xffu)) * SAMP_COPIES + cp], 1u);      // bin 255 = the lowest ids
                    }
                });
                __syncthreads();
                if (tid < 64) samp_select((const u64*)hist, true, (u64)need, -1.0, sel, sel64);
                __syncthreads();
                pfx = (pfx << 8) | (255u - (unsigned)(sel[0] < 0 ? 0 : sel[0]));
                need -= (int)sel64[0];
                __syncthreads();
            }
            if (tid < 64) {                                // the 256 ids under the cut's upper bytes, in ascending order
                for (int q = 0; q < 4; ++q) {
                    const int id = (int)(pfx << 8) + q * 64 + tid;
                    const bool tie = id < vocab && samp_key(lg[id < vocab ? id : 0]) == T;
                    const u64 bal = __ballot(tie);
                    const int cnt = __popcll(bal);
                    if (need <= cnt) {
                        if (tie && __popcll(bal & ((1ull << tid) - 1ull)) == need - 1) id_cut = id;
                        break;
                    }
                    need -= cnt;
                }
            }
        }
    }
    __syncthreads();
    const int cut = id_cut;

    // ---- pass 3: the n items
    lp_scan(lg, nchunk, [&](int c, const bf16x8& x, const float*) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const unsigned key = samp_key((bf16_t)x[e]);
            const int id = c * 8 + e;
            if (key > T || (key == T && id <= cut)) {
                const int at = atomicAdd(&it_cnt, 1);
                if (at < LA_TOPLP_MAX) { it_key[at] = key; it_id[at] = id; }
            }
        }
    });
    __syncthreads();
    if (tid >= n) return;
    const int cnt = it_cnt < n ? it_cnt : n;
    if (tid >= cnt) { o_ids[tid] = -1; o_vals[tid] = __builtin_nanf(""); return; }
    const unsigned key = it_key[tid];
    const int id = it_id[tid];
    int rank = 0;
    for (int j = 0; j < cnt; ++j) rank += (it_key[j] > key || (it_key[j] == key && it_id[j] < id)) ? 1 : 0;
    o_ids[rank] = id;
    o_vals[rank] = lp_value(lg[id], m, z);
}

int lk_top_logprob_rows(hipStream_t st, const TopLpArgs& a) {
    if (a.p.vocab <= 0 || (a.p.vocab & 7) || a.n < 1 || a.n > LA_TOPLP_MAX || a.n > a.p.vocab) return -1;
    if (a.log_ids ? (!a.log_vals || !a.pos || a.stride <= 0) : (!a.out_ids || !a.out_vals)) return -1;
    const int blocks = a.p.kind == LA_PEN_MBLOCK ? a.p.nblk : 1;
    if (blocks < 1 || blocks > LA_MB_MAX) return -1;
    k_top_logprob_rows<<<dim3(LA_TB, blocks), LP_THREADS, 0, st>>>(a);
    return (int)hipGetLastError();
}
