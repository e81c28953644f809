// la_epilogue.h — what a GEMM kernel does with a FINISHED fp32 accumulator value, written once (device only; la_kernels.hip and
// la_mblock.hip include it).  The kernels keep what differs between them: the reduction layout, the wave -> slice mapping, the nv[]
// masks and everything before the sums are final (fp8 row scales included: the caller multiplies them in first).  Here live
//   rope_half / rope_pair   rotate-half RoPE of one (d, d + 64) pair in storage-type arithmetic
//   RopeTab / rope_tab_load the cos / sin entries of RV consecutive pairs of one position, as one 8 / 4 / 2-byte load each
//   qkv_store<RV>           q/k/v bias, RoPE and the QF / KF / VF fragment stores of RV consecutive pairs of one lane
//   swiglu_act<FAST>        act = silu(g) * u with its three roundings; the exact and the fast SiLU
//   argmax_better / argmax_merge_halves (la_common.h)   the first-maximum candidate rule of every argmax
// Rounding points fixed here (the reference's eager graph rounds at each of them, la_common.h): the nn.Linear output (after the bias, which
// is added in fp32), each RoPE product, their sum; gate, up, silu(gate), silu(gate) * up.
#pragma once
#include "la_common.h"
#include <type_traits>

// x * cos + rot(x) * sin for one element, x and xr (the rotate-half partner: -x[d + 64] for the low half, x[d - 64] for the high half)
// already in the storage type (apply_rotary_pos_emb, modeling_llama.py:154-169: two rounded products, one rounded sum).
// fp16 build: the compiler narrows this to half arithmetic and contracts it into v_fma_f16(one product, the rounded other one); which
// product is rounded is its choice per kernel — tests/test_gpu_epilogue_digests.py pins the outcome; the inline QKV sites of k_gemm_wide
// and gemm64_body are its consequence.
__device__ __forceinline__ bf16_t rope_half(float x, float xr, float c, float s) { return f2bf(bfr(x * c) + bfr(xr * s)); }
// ... for the pair (xl, xh) = features (d, d + 64) of one head as fp32 sums: rounded to the storage type first
__device__ __forceinline__ void rope_pair(float xl, float xh, float c, float s, bf16_t* olo, bf16_t* ohi) {
    const float bl = bfr(xl), bh = bfr(xh);
    *olo = rope_half(bl, -bh, c, s);
    *ohi = rope_half(bh, bl, c, s);
}

// Where a QKV epilogue writes: filled from GemmArgs (64-row kernels) or MbArgs (multi-block kernels).
struct QkvDst {
    bf16_t* qf; bf16_t* kfresh; bf16_t* vfresh;      // QF / fresh KF / fresh VF fragments, 8192 elements per head and 64-row block
    const bf16_t* rcos; const bf16_t* rsin;          // [position][64]
    const bf16_t* bias;                              // null, or the lane-ordered q/k/v bias (qkv_bias_add, la_common.h)
    int nh, nkv;
    int q_blk, kv_blk;                               // heads per 64-row block of qf / kfresh, vfresh: nh, nkv; 0 in the single-block kernels
};
template <typename A> __device__ __forceinline__ QkvDst qkv_dst(const A& a, bool multi_block) {
    return QkvDst{a.qf, a.kfresh, a.vfresh, a.rcos, a.rsin, a.qkv_bias, a.nh, a.nkv, multi_block ? a.nh : 0, multi_block ? a.nkv : 0};
}

// RV consecutive 16-bit elements as one value: an 8 / 4 / 2-byte load or store
template <int RV> struct Run16 {
    typedef __attribute__((ext_vector_type(RV))) short type;
    static __device__ __forceinline__ bf16_t get(const type& v, int e) { return (bf16_t)v[e]; }
    static __device__ __forceinline__ void set(type& v, int e, bf16_t x) { v[e] = (short)x; }
};
template <> struct Run16<1> {
    typedef bf16_t type;
    static __device__ __forceinline__ bf16_t get(const type& v, int) { return v; }
    static __device__ __forceinline__ void set(type& v, int, bf16_t x) { v = x; }
};
// cos / sin of pairs dlo .. dlo + RV - 1 at position ps.  A kernel that wants the dependent pos -> cos / sin loads in flight across a
// barrier calls rope_tab_load before it and hands the table to qkv_store.
template <int RV> struct RopeTab { typename Run16<RV>::type c, s; };
template <int RV> __device__ __forceinline__ RopeTab<RV> rope_tab_load(const QkvDst& d, int ps, int dlo) {
    static_assert(RV == 4 || RV == 2 || RV == 1, "4, 2 or 1 pairs per load");
    typedef typename Run16<RV>::type run_t;
    return RopeTab<RV>{*(const run_t*)(d.rcos + (size_t)ps * 64 + dlo), *(const run_t*)(d.rsin + (size_t)ps * 64 + dlo)};
}

// RV consecutive RoPE pairs pr .. pr + RV - 1 of token row `tok` of 64-row block `blk` (pair index = head slot * 64 + d; the caller
// guarantees they lie in one head slot and one 16-byte fragment chunk): lo[o + e] / hi[o + e] are the finished sums of features d + e and
// d + e + 64.  bias (fp32) -> q/k slots: RoPE, one 8 / 4 / 2-byte store per half into the QF / KF fragment; v slots: rounded, scalar
// stores into the transposed VF fragment.  `tab` is the RopeTab<RV> of the token's position loaded earlier, or the position itself: the
// table is then read here, and only by lanes of a q/k slot.
template <int RV, typename V, typename T>
__device__ __forceinline__ void qkv_store(const QkvDst& d, int blk, int tok, int pr, V& lo, V& hi, int o, const T& tab) {
    const int slot = pr >> 6, dlo = pr & 63, dhi = dlo + 64;
    qkv_bias_add<RV>(d.bias, slot * 128 + dlo, lo, o);
    qkv_bias_add<RV>(d.bias, slot * 128 + dhi, hi, o);
    if (slot < d.nh + d.nkv) {
        bf16_t* dst = slot < d.nh ? d.qf + ((size_t)blk * d.q_blk + slot) * 8192 : d.kfresh + ((size_t)blk * d.kv_blk + (slot - d.nh)) * 8192;
        RopeTab<RV> t;
        if constexpr (std::is_integral<T>::value) t = rope_tab_load<RV>(d, tab, dlo);
        else t = tab;
        typename Run16<RV>::type olo, ohi;
#pragma unroll
        for (int e = 0; e < RV; ++e) {
            bf16_t l16, h16;
            rope_pair(lo[o + e], hi[o + e], bf2f(Run16<RV>::get(t.c, e)), bf2f(Run16<RV>::get(t.s, e)), &l16, &h16);
            Run16<RV>::set(olo, e, l16); Run16<RV>::set(ohi, e, h16);
        }
        *(typename Run16<RV>::type*)(dst + rf_offset(tok, dlo)) = olo;
        *(typename Run16<RV>::type*)(dst + rf_offset(tok, dhi)) = ohi;
    } else {
        bf16_t* dst = d.vfresh + ((size_t)blk * d.kv_blk + (slot - d.nh - d.nkv)) * 8192;
#pragma unroll
        for (int e = 0; e < RV; ++e) {
            dst[vf_offset(tok, dlo + e)] = f2bf(lo[o + e]);
            dst[vf_offset(tok, dhi + e)] = f2bf(hi[o + e]);
        }
    }
}

// act = storage(silu(storage(g)) * storage(u)), silu rounded too (LlamaMLP.forward, modeling_llama.py:185-186), as the storage-type value.
// FAST = false: libm expf and an IEEE division (the 64-row kernels and k_gemm_mb).  FAST = true: v_exp_f32 + v_rcp_f32, ~1 ulp each
// before the rounding (k_gemm_wide, k_gemm_fat, k_gemm_fatd: the exact form costs ~60 VALU instructions per element, and a lane of those
// kernels has up to 64 elements).  The two forms differ on a few elements per thousand: a site keeps the form it has.
template <bool FAST>
__device__ __forceinline__ bf16_t swiglu_act(float g, float u) {
    const float gv = bfr(g), uv = bfr(u);
    const float sv = FAST ? bfr(gv * __builtin_amdgcn_rcpf(1.0f + __expf(-gv))) : bfr(gv / (1.0f + expf(-gv)));
    return f2bf(sv * uv);
}
