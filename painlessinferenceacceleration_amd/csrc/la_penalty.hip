// la_penalty.hip — repetition penalty on the device: the penalised argmax of every live tree row, between the lm_head launch and
// the (unchanged) accept walk, and the update of the per-slot context sets by the step that emits tokens.
//
// transformers' RepetitionPenaltyLogitsProcessor.__call__(input_ids, scores) rewrites scores[t] for every t in set(input_ids):
//     s < 0 ? s * penalty : s / penalty
// and the host walk of the loops (pretrained_model.py: pick(seq + next_tokens, cur)) hands it, at tree row `cur`, the context
// seq + the tokens accepted so far.  Every row the walk moves to carries the token just picked, so the context of row r — IF the
// walk ever reaches it — is set(seq) + { ids[a] : a an ancestor of r, or r itself } = set(seq) + the set bits of rowmask[r]
// (ids[0] == seq[-1] is in seq already).  The penalty needs set membership only, so the penalised argmax of ALL rows can be taken
// before the walk, in parallel, and the walk kernels (accept_walk, k_accept_scan_b, k_accept_scan_mb) run as they are.
//
//   context set of a slot   a bitmap of vocab bits in HBM ([n_slots][vocab / 32] words), seeded by the host with the tokens the
//                           host walk would hand the processor at the first pick (la_llama_penalty_seed: a bitmap built on the host), then kept current by
//                           the steps themselves: k_pen_update ORs in the tokens a step emits (vector atomics), so neither the
//                           native loop nor a graph replay needs the host between steps
//   k_pen_argmax            one workgroup per live row: slot bitmap -> LDS, OR in the <= 64 path tokens, scan the row of logits
//                           lm_head has just written ([rows][vocab], 16-byte loads, one LDS bitmap word per 32 tokens: the four
//                           lanes of a word read one address = a broadcast, 32 lanes cover 8 consecutive banks), penalise the
//                           members, reduce to one (value, index); writes the ARGMAX words the candidate reduction writes otherwise
//
// Arithmetic (pinned to what the host path computes on the engine's 16-bit logits, bit for bit): widen to fp32; members: multiply
// (s < 0) or DIVIDE (IEEE, correctly rounded: no reciprocal) by float32(penalty); round to nearest-even back to the storage type;
// compare the rounded values; the lowest index wins among equal maxima (torch.argmax).  Any penalty > 0 is legal.
#include "la_common.h"
#include "la_kernels.h"
#include "la_mblock.h"
#include "la_rows.h"

__global__ __launch_bounds__(1024) void k_pen_argmax(const PenArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned pen_lds[];        // [words] context bitmap, then the reduction scratch
    const PenRow r = pen_row(a);
    if (!r.live) return;                                                       // block-uniform
    const int tid = (int)threadIdx.x, words = a.vocab >> 5;
    float* sv = (float*)(pen_lds + words);
    int* si = (int*)(sv + 16);
    const unsigned* bm = a.bitmaps + (size_t)r.slot * words;
    for (int w = tid; w < words; w += 1024) pen_lds[w] = bm[w];
    __syncthreads();
    if (tid < 64 && ((r.path >> tid) & 1ull)) {
        const int tok = a.ids[r.row0 + tid];
        if (tok >= 0 && tok < a.vocab) atomicOr(&pen_lds[tok >> 5], 1u << (tok & 31));
    }
    __syncthreads();
    const float p = *a.penalty;
    const bf16_t* lg = (const bf16_t*)a.logits + (size_t)r.row * a.vocab;
    const int nchunk = a.vocab >> 3;                                           // 16-byte chunks of 8 logits (vocab % 32 == 0)
    float best = -INFINITY;
    int bidx = 0x7fffffff;
    // four chunks per thread and round, all requested before the first compare
    for (int base = tid; base < nchunk; base += 4 * 1024) {
        bf16x8 x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = base + k * 1024;
            x[k] = *(const bf16x8*)(lg + (size_t)(c < nchunk ? c : base) * 8);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = base + k * 1024;
            if (c >= nchunk) break;
            const unsigned member = (pen_lds[c >> 2] >> ((c & 3) * 8)) & 0xffu;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const bf16_t s = (bf16_t)x[k][e];
                const float v = ((member >> e) & 1u) ? pen_value(s, p) : bf2f(s);
                argmax_better(v, c * 8 + e, best, bidx);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bidx, o, 64);
        argmax_better(ob, oi, best, bidx);
    }
    if ((tid & 63) == 0) { sv[tid >> 6] = best; si[tid >> 6] = bidx; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < 16; ++w) argmax_better(sv[w], si[w], best, bidx);
        a.out[r.row] = bidx;
    }
}

// The tokens the step has just emitted join the context set of their slot (after the accept walk, before the next step's
// k_pen_argmax on the same stream).  A mode-2 (forward only) step emits nothing.  A prefill chain emits the token of its last row:
// only the LAST block of a slot in a pass counts (the earlier blocks of a multi-block chain emit a token nobody reads), and the host
// seeds a slot after every pass of its prompt but the last (la_llama_penalty_seed clears the set first).
__global__ void k_pen_update(const PenArgs a) {
    const int words = a.vocab >> 5, t = (int)threadIdx.x;
    int tok = -1, slot = 0;
    if (a.kind == LA_PEN_SINGLE) {                       // 64 threads
        if (t < a.state[LA_ST_NOUT]) tok = a.state[LA_ST_OUTTOK + t];
    } else if (a.kind == LA_PEN_BATCH) {                 // 256 threads = 16 slots x 16 tokens
        slot = t >> 4;
        if (slot < a.n_slots && (t & 15) < a.state[LA_BST_NOUT + slot]) tok = a.state[LA_BST_OUTTOK + t];
    } else {                                             // LA_PEN_MBLOCK: 512 threads = 8 blocks x 64 (LA_MOUT_TOKS used)
        const int b = t >> 6, j = t & 63;
        if (b < a.nblk) {
            slot = a.meta[b * LA_MB_META + LA_MBM_SLOT];
            bool last_of_slot = true;
            for (int q = b + 1; q < a.nblk; ++q) last_of_slot = last_of_slot && a.meta[q * LA_MB_META + LA_MBM_SLOT] != slot;
            const bool counts = a.meta[b * LA_MB_META + LA_MBM_MODE] != 1 || last_of_slot;
            if (counts && j < LA_MOUT_TOKS && j < a.state[LA_MOUT_NOUT + b]) tok = a.state[LA_MOUT_OUTTOK + b * LA_MOUT_TOKS + j];
        }
    }
    if (tok >= 0 && tok < a.vocab && slot >= 0 && slot < a.n_slots)
        atomicOr(a.bitmaps + (size_t)slot * words + (tok >> 5), 1u << (tok & 31));
}

// the row transform alone (unit entry of the exhaustive arithmetic check): out[i] = member ? penalised x[i] : x[i]
__global__ void k_pen_transform(const bf16_t* __restrict__ x, int n, const float* __restrict__ penalty, bf16_t* __restrict__ out) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n) out[i] = f2bf(pen_value(x[i], *penalty));
}

size_t lk_pen_lds_bytes(int vocab) { return (size_t)(vocab >> 5) * 4 + 16 * 8; }

int lk_pen_argmax(hipStream_t st, const PenArgs& a) {
    if (a.vocab <= 0 || (a.vocab & 31) || lk_pen_lds_bytes(a.vocab) > 64 * 1024) return -1;
    const int blocks = a.kind == LA_PEN_MBLOCK ? a.nblk : 1;
    if (blocks < 1 || blocks > LA_MB_MAX) return -1;
    k_pen_argmax<<<dim3(LA_TB, blocks), 1024, lk_pen_lds_bytes(a.vocab), st>>>(a);
    return (int)hipGetLastError();
}

int lk_pen_update(hipStream_t st, const PenArgs& a) {
    const int threads = a.kind == LA_PEN_SINGLE ? 64 : a.kind == LA_PEN_BATCH ? 256 : 512;
    if (a.kind != LA_PEN_SINGLE && a.kind != LA_PEN_BATCH && a.kind != LA_PEN_MBLOCK) return -1;
    k_pen_update<<<1, threads, 0, st>>>(a);
    return (int)hipGetLastError();
}

int lk_pen_transform(hipStream_t st, const void* x, int n, const float* d_penalty, void* out) {
    if (n <= 0) return 0;
    k_pen_transform<<<(n + 255) / 256, 256, 0, st>>>((const bf16_t*)x, n, d_penalty, (bf16_t*)out);
    return (int)hipGetLastError();
}
