// la_sample.hip — sampling on the device: the seeded temperature / top-k / top-p token of every live tree row, between the lm_head
// launch and the (unchanged) accept walk.
//
// The random draw of a row is a pure function of (seed, stream, position, token) — never of call order — so the "sampled token of
// every tree row" can be taken in parallel BEFORE the walk, exactly as k_pen_argmax takes the penalised argmax: a draft child is
// accepted iff it equals the token sampled at its parent, which is ancestral sampling, and the same seed gives the same sequence
// whatever trees the steps carried (lookahead == no-draft, token for token).
//
// The sampler of one row r (x = the 16-bit logits lm_head wrote; every threshold is a 16-bit KEY: the storage bits mapped so that
// unsigned order == value order, -0 folded into +0, NaN -> key 0 = never kept):
//   1. repetition penalty (only with the penalty stage on): members of the slot's context set + the row's path tokens are rewritten
//      by pen_value (la_rows.h) and rounded to the storage type, as k_pen_argmax does
//   2. temperature   z_v = x_v / T in fp32 (IEEE division)
//   3. top-k         keep v iff key_v >= the k-th largest key of the row (ties at the threshold stay, TopKLogitsWarper);
//                    top_k <= 0 or >= vocab: off.  An exact two-level radix select: 256 bins over the high byte, then the low byte.
//   4. top-p         over the survivors, q_v = floor(expf(z_v - z_max) * 2^32) (the row maximum: exactly 2^32), summed as 64-bit
//                    INTEGERS (order-independent: the same bits on every run and every step path); keep v iff the mass of the
//                    survivors with a key strictly greater than key_v is < top_p * Z.  TopPLogitsWarper with min_tokens_to_keep = 1,
//                    except that every token tied with the lowest kept value stays.  top_p >= 1: off.  Again two 256-bin levels.
//   5. draw          Gumbel-max over the kept set: tok = argmax_v (z_v + g_v), lowest index among equals; g_v = -logf(-logf(u_v));
//                    u_v = (k_v + 0.5) * 2^-23 with k_v the top 23 bits of the token's Philox word (exact in fp32, never 0 or 1);
//                    Philox4x32-10, key (seed_lo, seed_hi), counter (v >> 2, pos[r] + 1, stream, 0), output word v & 3 is token v's.
//                    pos[r] + 1 = the index, in the unpadded sequence, of the token being chosen.
// One workgroup of 1024 threads per live row (row addressing and liveness: pen_row, la_rows.h).  The row is read with 16-byte loads
// once per histogram level that is switched on and once for the draw (it is cache-resident just after lm_head); histograms sit in
// LDS in 8 interleaved copies (lane & 7) so that the few bins a row of logits really populates do not serialise a whole wave on one
// LDS address; the penalty bitmap sits in LDS too.
#include "la_common.h"
#include "la_kernels.h"
#include "la_mblock.h"
#include "la_rows.h"
#include "la_select.h"

#define SAMP_THREADS 1024
typedef unsigned long long u64;

// Philox4x32-10 (Salmon et al., SC'11)
__host__ __device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const u64 p0 = (u64)0xD2511F53u * c0, p1 = (u64)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1; c3 = (unsigned)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the keys of every 16-byte chunk of the row, penalty applied: f(chunk index, keys[8]); four chunks per thread and round in flight
template <typename F>
__device__ __forceinline__ void samp_scan(const bf16_t* __restrict__ lg, int nchunk, const unsigned* bm, float pen, F&& f) {
    const int tid = (int)threadIdx.x;
    for (int base = tid; base < nchunk; base += 4 * SAMP_THREADS) {
        bf16x8 x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = base + k * SAMP_THREADS;
            x[k] = *(const bf16x8*)(lg + (size_t)(c < nchunk ? c : base) * 8);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = base + k * SAMP_THREADS;
            if (c >= nchunk) break;
            const unsigned member = bm ? (bm[c >> 2] >> ((c & 3) * 8)) & 0xffu : 0u;
            unsigned keys[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                bf16_t s = (bf16_t)x[k][e];
                if ((member >> e) & 1u) s = f2bf(pen_value(s, pen));
                keys[e] = samp_key(s);
            }
            f(c, keys);
        }
    }
}

__global__ __launch_bounds__(SAMP_THREADS) void k_sample_rows(const SampArgs a) {
    // [256 x 8] 64-bit histogram copies | 32 x 8 bytes of scratch | the context bitmap (penalty on)
    extern __shared__ __attribute__((aligned(16))) unsigned long long samp_lds[];
    const PenRow r = pen_row(a.p);
    if (!r.live) return;                                                       // block-uniform
    const int tid = (int)threadIdx.x, vocab = a.p.vocab, words = vocab >> 5, nchunk = vocab >> 3;
    u64* hist = samp_lds;
    unsigned* hist32 = (unsigned*)hist;
    u64* sel64 = hist + 256 * SAMP_COPIES;                                     // [0..1] select result, [2..17] per-wave scratch
    int* sel = (int*)(sel64 + 18);                                             // [0] select result, [1] max key, [2] kept count, [3..] per-wave
    float* redv = (float*)(sel64 + 2);
    int* redi = sel + 4;
    unsigned* bm = nullptr;
    float pen = 1.f;
    if (a.pen) {
        bm = (unsigned*)(sel64 + 32);
        const unsigned* src = a.p.bitmaps + (size_t)r.slot * words;
        for (int w = tid; w < words; w += SAMP_THREADS) bm[w] = src[w];
        pen = *a.p.penalty;
    }
    if (tid < 4) sel[tid] = 0;
    __syncthreads();
    if (a.pen && tid < 64 && ((r.path >> tid) & 1ull)) {
        const int tok = a.p.ids[r.row0 + tid];
        if (tok >= 0 && tok < vocab) atomicOr(&bm[tok >> 5], 1u << (tok & 31));
    }
    unsigned seed_lo = a.seed_lo, seed_hi = a.seed_hi, stream = a.stream_id;
    float T = a.temperature, top_p = a.top_p;
    int top_k = a.top_k;
    if (a.params) {
        seed_lo = a.params[LA_SAMP_SEED_LO]; seed_hi = a.params[LA_SAMP_SEED_HI]; T = __uint_as_float(a.params[LA_SAMP_TEMP]);
        top_k = (int)a.params[LA_SAMP_TOPK]; top_p = __uint_as_float(a.params[LA_SAMP_TOPP]); stream = a.params[LA_SAMP_STREAM + r.slot];
    }
    const bool k_on = top_k > 0 && top_k < vocab, p_on = top_p < 1.f;
    const bf16_t* lg = (const bf16_t*)a.p.logits + (size_t)r.row * vocab;
    const int cp = tid & (SAMP_COPIES - 1);
    auto zero_hist = [&]() { for (int i = tid; i < 256 * SAMP_COPIES; i += SAMP_THREADS) hist[i] = 0ull; };

    // ---- level 1 of the top-k select + the row maximum
    zero_hist();
    __syncthreads();
    unsigned kmax = 0;
    samp_scan(lg, nchunk, bm, pen, [&](int, const unsigned* keys) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            kmax = keys[e] > kmax ? keys[e] : kmax;
            if (k_on && keys[e]) atomicAdd(&hist32[(keys[e] >> 8) * SAMP_COPIES + cp], 1u);
        }
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned t = __shfl_xor(kmax, o, 64); kmax = t > kmax ? t : kmax; }
    if ((tid & 63) == 0) atomicMax((unsigned*)&sel[1], kmax);
    __syncthreads();
    kmax = (unsigned)sel[1];
    unsigned kk = 0;                                                           // top-k threshold key (0: off)
    if (k_on) {
        if (tid < 64) samp_select(hist, true, (u64)top_k, -1.0, sel, sel64);
        __syncthreads();
        const int hb = sel[0];
        const u64 above = sel64[0];
        __syncthreads();
        if (hb >= 0) {
            zero_hist();
            __syncthreads();
            samp_scan(lg, nchunk, bm, pen, [&](int, const unsigned* keys) {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if ((int)(keys[e] >> 8) == hb && keys[e]) atomicAdd(&hist32[(keys[e] & 0xffu) * SAMP_COPIES + cp], 1u);
            });
            __syncthreads();
            if (tid < 64) samp_select(hist, true, (u64)top_k - above, -1.0, sel, sel64);
            __syncthreads();
            kk = ((unsigned)hb << 8) | (unsigned)(sel[0] < 0 ? 0 : sel[0]);
            __syncthreads();
        }
    }
    const unsigned kfloor = kk > 1u ? kk : 1u;                                 // NaN (key 0) never survives
    const float zmax = samp_val(kmax) / T;
    auto mass = [&](unsigned key) -> u64 {
        if (key == kmax) return 1ull << 32;
        return (u64)(expf(samp_val(key) / T - zmax) * 4294967296.f);
    };
    unsigned kp = 0;                                                           // top-p threshold key (0: off)
    if (p_on && kmax) {
        zero_hist();
        __syncthreads();
        samp_scan(lg, nchunk, bm, pen, [&](int, const unsigned* keys) {
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (keys[e] >= kfloor) atomicAdd(&hist[(keys[e] >> 8) * SAMP_COPIES + cp], mass(keys[e]));
        });
        __syncthreads();
        if (tid < 64) samp_select(hist, false, 0ull, (double)(top_p > 0.f ? top_p : 0.f), sel, sel64);
        __syncthreads();
        const int pb = sel[0];
        const u64 above = sel64[0], target = sel64[1];
        __syncthreads();
        if (pb >= 0) {
            zero_hist();
            __syncthreads();
            samp_scan(lg, nchunk, bm, pen, [&](int, const unsigned* keys) {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if ((int)(keys[e] >> 8) == pb && keys[e] >= kfloor) atomicAdd(&hist[(keys[e] & 0xffu) * SAMP_COPIES + cp], mass(keys[e]));
            });
            __syncthreads();
            if (tid < 64) samp_select(hist, false, target - above, -1.0, sel, sel64);
            __syncthreads();
            kp = ((unsigned)pb << 8) | (unsigned)(sel[0] < 0 ? 0 : sel[0]);
            __syncthreads();
        }
    }
    const unsigned kmin = kp > kfloor ? kp : kfloor;

    // ---- the draw: Gumbel-max over the kept set
    const unsigned position = (unsigned)(a.pos[r.row] + 1);
    float best = -INFINITY;
    int bidx = 0x7fffffff, kept = 0;
    samp_scan(lg, nchunk, bm, pen, [&](int c, const unsigned* keys) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            bool any = false;
#pragma unroll
            for (int e = 0; e < 4; ++e) any = any || keys[half * 4 + e] >= kmin;
            if (!any) continue;
            unsigned w[4];
            philox4x32_10((unsigned)(c * 2 + half), position, stream, 0u, seed_lo, seed_hi, w);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned key = keys[half * 4 + e];
                if (key < kmin) continue;
                ++kept;
                const float u = ((float)(w[e] >> 9) + 0.5f) * 1.1920928955078125e-07f;
                const float g = -logf(-logf(u));
                argmax_better(samp_val(key) / T + g, c * 8 + half * 4 + e, best, bidx);
            }
        }
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bidx, o, 64);
        argmax_better(ob, oi, best, bidx);
        kept += __shfl_xor(kept, o, 64);
    }
    if ((tid & 63) == 0) { redv[tid >> 6] = best; redi[tid >> 6] = bidx; atomicAdd(&sel[2], kept); }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < SAMP_THREADS / 64; ++w) argmax_better(redv[w], redi[w], best, bidx);
        a.p.out[r.row] = bidx < vocab ? bidx : 0;
        if (a.info) {
            int* inf = a.info + (size_t)r.row * 4;
            inf[0] = (int)kk; inf[1] = (int)kp; inf[2] = sel[2]; inf[3] = 0;
        }
    }
}

// the raw Philox word of every token at one (seed, stream, position): the known-answer entry of the unit tests
__global__ void k_sample_bits(unsigned seed_lo, unsigned seed_hi, unsigned stream, unsigned position, int vocab, unsigned* __restrict__ out) {
    const int q = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (q * 4 >= vocab) return;
    unsigned w[4];
    philox4x32_10((unsigned)q, position, stream, 0u, seed_lo, seed_hi, w);
#pragma unroll
    for (int e = 0; e < 4; ++e) if (q * 4 + e < vocab) out[q * 4 + e] = w[e];
}

size_t lk_sample_lds_bytes(int vocab, int pen) {
    return (size_t)256 * SAMP_COPIES * 8 + 32 * 8 + 64 * 4 + (pen ? (size_t)(vocab >> 5) * 4 : 0);
}

int lk_sample_rows(hipStream_t st, const SampArgs& a) {
    if (a.p.vocab <= 0 || (a.p.vocab & 31) || lk_sample_lds_bytes(a.p.vocab, a.pen) > 64 * 1024) return -1;
    const int blocks = a.p.kind == LA_PEN_MBLOCK ? a.p.nblk : 1;
    if (blocks < 1 || blocks > LA_MB_MAX) return -1;
    k_sample_rows<<<dim3(LA_TB, blocks), SAMP_THREADS, lk_sample_lds_bytes(a.p.vocab, a.pen), st>>>(a);
    return (int)hipGetLastError();
}

int lk_sample_bits(hipStream_t st, unsigned seed_lo, unsigned seed_hi, unsigned stream_id, unsigned position, int vocab, unsigned* out) {
    if (vocab <= 0) return 0;
    const int quads = (vocab + 3) / 4;
    k_sample_bits<<<(quads + 255) / 256, 256, 0, st>>>(seed_lo, seed_hi, stream_id, position, vocab, out);
    return (int)hipGetLastError();
}
