// la_mb_forms.h — which kernel instantiation a multi-block GEMM launch runs, with which grid: ONE table of forms and ONE pure selector.
// Host-only C++17, no HIP include: la_mblock.hip expands the table into kernel pointers (lk_mb_init's attribute loop, launch_mb's launch),
// and tests/test_mb_forms_cpu.py compiles the same header into a host program that sweeps the selector.
//
// A row names a kernel family and its template arguments; block size, dynamic LDS bytes and the name string follow from them, so a row
// cannot carry the LDS size of another kernel.  The selector computes the family and arguments a launch wants and looks the row up: a form
// that is not in the table of this build is refused (-1), never launched.  Rows of LA_MB_FORMS_LAB are reachable only through a knob value
// that the product build (constexpr defaults, la_knobs.h) cannot take: the product build leaves them out, and their kernels uninstantiated.
#pragma once
#include <stdint.h>

enum { MB_SLAB = 0, MB_SWIGLU = 1, MB_QKV = 2, MB_LOGITS = 3 };          // epilogue of a launch = `kind` of lk_mb_gemm
enum { MBK_MB = 0, MBK_WIDE = 1, MBK_FAT = 2, MBK_FATD = 3 };            // kernel family

// X(family, template arguments...) — unused trailing arguments are 0:
//   MB   (RBV, NT, EPI, EX, DW)               k_gemm_mb<RBV, NT, EPI, EX, DW>                 512 threads
//   WIDE (RBV, TW, EPI, DBG, SCH)             k_gemm_wide<RBV, TW, EPI, DBG, SCH>             512 threads
//   FAT  (RBV, TW, EPI, RV, WPOL, RPW, STG)   k_gemm_fat<RBV, TW, EPI, RV, WPOL, RPW, STG>    256 threads
//   FATD (TW, WPOL)                           k_gemm_fatd<TW, WPOL>                           256 threads
#define LA_MB_FORMS_PRODUCT(X) \
    X(MB, 2, 2, SLAB, 0, 8, 0, 0)   X(MB, 4, 2, SWIGLU, 0, 8, 0, 0)   X(MB, 2, 2, QKV, 0, 8, 0, 0)   X(MB, 4, 2, LOGITS, 0, 8, 0, 0) \
    X(MB, 2, 4, SLAB, 0, 8, 0, 0)   X(MB, 4, 4, SWIGLU, 0, 8, 0, 0)   X(MB, 2, 4, QKV, 0, 8, 0, 0)   X(MB, 4, 4, LOGITS, 0, 8, 0, 0) \
    X(MB, 2, 4, SLAB, 1, 8, 0, 0)   X(MB, 4, 4, SWIGLU, 1, 4, 0, 0)   X(MB, 4, 4, SLAB, 1, 8, 0, 0)  X(MB, 8, 4, SWIGLU, 1, 8, 0, 0) \
    X(WIDE, 2, 1, SLAB, 0, 2, 0, 0) X(WIDE, 2, 2, SLAB, 0, 2, 0, 0)   X(WIDE, 2, 1, QKV, 0, 2, 0, 0) X(WIDE, 2, 2, QKV, 0, 2, 0, 0) \
    X(WIDE, 4, 1, SLAB, 0, 2, 0, 0) X(WIDE, 4, 2, SLAB, 0, 2, 0, 0)   X(WIDE, 4, 1, QKV, 0, 2, 0, 0) X(WIDE, 4, 2, QKV, 0, 2, 0, 0) \
    X(WIDE, 4, 2, SWIGLU, 0, 2, 0, 0) X(WIDE, 4, 3, SWIGLU, 0, 3, 0, 0) X(WIDE, 4, 4, SWIGLU, 0, 3, 0, 0) \
    X(WIDE, 8, 2, SWIGLU, 0, 2, 0, 0) X(WIDE, 8, 3, SWIGLU, 0, 3, 0, 0) X(WIDE, 8, 4, SWIGLU, 0, 3, 0, 0) \
    X(WIDE, 4, 2, LOGITS, 0, 2, 0, 0) X(WIDE, 4, 3, LOGITS, 0, 3, 0, 0) X(WIDE, 4, 4, LOGITS, 0, 3, 0, 0) \
    X(FAT, 2, 1, QKV, 4, 0, 2, 0)   X(FAT, 2, 1, QKV, 2, 0, 2, 0)     X(FAT, 2, 2, QKV, 4, 2, 2, 0)  X(FAT, 2, 2, QKV, 2, 2, 2, 0) \
    X(FAT, 4, 1, QKV, 4, 0, 4, 0)   X(FAT, 4, 1, QKV, 2, 0, 4, 0)     X(FAT, 4, 2, QKV, 4, 0, 4, 0)  X(FAT, 4, 2, QKV, 2, 0, 4, 0) \
    X(FAT, 4, 1, SLAB, 4, 0, 4, 0)  X(FAT, 4, 2, SLAB, 4, 0, 4, 2)    X(FAT, 4, 2, SWIGLU, 4, 2, 4, 0) \
    X(FATD, 3, 0, SWIGLU, 0, 0, 0, 0) X(FATD, 4, 0, SWIGLU, 0, 0, 0, 0)
// what only a knob reaches: key 3 (NT = 8), key 25 (the other DW), key 24 = 0 (SCH = 0), key 4 (DBG), and bits 2 / 7 / 9 / 10 / 11 of key 6,
// key 35 = 0 or bit 6 of key 6 off (the paired k_gemm_fat gate/up), key 36 = 0 (slabs with x through LDS)
#define LA_MB_FORMS_LAB(X) \
    X(MB, 2, 8, SLAB, 0, 8, 0, 0)   X(MB, 4, 8, SWIGLU, 0, 8, 0, 0)   X(MB, 2, 8, QKV, 0, 8, 0, 0)   X(MB, 4, 8, LOGITS, 0, 8, 0, 0) \
    X(MB, 2, 4, SLAB, 1, 4, 0, 0)   X(MB, 4, 4, SWIGLU, 1, 8, 0, 0) \
    X(WIDE, 2, 1, SLAB, 0, 0, 0, 0) X(WIDE, 2, 2, SLAB, 0, 0, 0, 0)   X(WIDE, 2, 1, QKV, 0, 0, 0, 0) X(WIDE, 2, 2, QKV, 0, 0, 0, 0) \
    X(WIDE, 4, 1, SLAB, 0, 0, 0, 0) X(WIDE, 4, 2, SLAB, 0, 0, 0, 0)   X(WIDE, 4, 1, QKV, 0, 0, 0, 0) X(WIDE, 4, 2, QKV, 0, 0, 0, 0) \
    X(WIDE, 4, 2, SWIGLU, 0, 0, 0, 0) X(WIDE, 4, 3, SWIGLU, 0, 0, 0, 0) X(WIDE, 4, 4, SWIGLU, 0, 0, 0, 0) \
    X(WIDE, 8, 2, SWIGLU, 0, 0, 0, 0) X(WIDE, 8, 3, SWIGLU, 0, 0, 0, 0) X(WIDE, 8, 4, SWIGLU, 0, 0, 0, 0) \
    X(WIDE, 4, 2, LOGITS, 0, 0, 0, 0) X(WIDE, 4, 3, LOGITS, 0, 0, 0, 0) X(WIDE, 4, 4, LOGITS, 0, 0, 0, 0) \
    X(WIDE, 8, 2, QKV, 0, 0, 0, 0)  X(WIDE, 8, 2, QKV, 0, 2, 0, 0)    X(WIDE, 4, 2, SLAB, 4, 0, 0, 0) X(WIDE, 4, 2, QKV, 4, 0, 0, 0) \
    X(WIDE, 4, 4, SWIGLU, 1, 0, 0, 0) X(WIDE, 4, 4, SWIGLU, 2, 0, 0, 0) X(WIDE, 4, 4, SWIGLU, 3, 0, 0, 0) \
    X(WIDE, 4, 4, SWIGLU, 4, 0, 0, 0) X(WIDE, 4, 4, SWIGLU, 5, 0, 0, 0) X(WIDE, 4, 4, SWIGLU, 6, 3, 0, 0) \
    X(FAT, 2, 2, QKV, 4, 0, 2, 0)   X(FAT, 2, 2, QKV, 2, 0, 2, 0)     X(FAT, 2, 2, SLAB, 4, 2, 2, 0) X(FAT, 4, 2, SLAB, 4, 0, 4, 0) \
    X(FAT, 4, 3, SWIGLU, 4, 2, 4, 0) X(FAT, 4, 4, SWIGLU, 4, 2, 4, 0) \
    X(FAT, 8, 2, SWIGLU, 4, 0, 4, 0) X(FAT, 8, 3, SWIGLU, 4, 0, 4, 0) X(FAT, 8, 4, SWIGLU, 4, 0, 4, 0) \
    X(FAT, 8, 2, SWIGLU, 4, 0, 4, 1) X(FAT, 8, 3, SWIGLU, 4, 0, 4, 1) X(FAT, 8, 4, SWIGLU, 4, 0, 4, 1)
#if LA_LAB
#define LA_MB_FORMS(X) LA_MB_FORMS_PRODUCT(X) LA_MB_FORMS_LAB(X)
#else
#define LA_MB_FORMS(X) LA_MB_FORMS_PRODUCT(X)
#endif

// dynamic LDS of a family's instantiation (la_mblock.hip static_asserts them against the kernels' own geometry)
constexpr int la_mb_lds_mb(int nt) { return (2 * 4 * nt * 1024) > 65536 ? (2 * 4 * nt * 1024) : 65536; }   // x double buffer vs reduction (64 KiB)
constexpr int la_mb_lds_wide(int rbv, int tw) { return 4 * (2 * rbv + 2 * (8 / (rbv / 2)) * tw) * 1024; }    // WideGeom<RBV, TW>::LDS: 4 ring slots
constexpr int la_mb_lds_fat(int rbv, int tw, int rpw) {                                                        // FatGeom<RBV, TW, RPW>::LDS
    const int stage = 2 * rbv + 2 * (4 / (rbv / rpw)) * tw;
    return (4 * stage * 1024 <= 144 * 1024 ? 4 : 3) * stage * 1024;
}
constexpr int LA_MB_LDS_FATD = 96 * 1024;

struct MbFormRow { uint64_t key; int block, lds; const char* name; };
constexpr uint64_t la_mb_form_key(int fam, int a, int b, int c, int d, int e, int f, int g) {
    return (uint64_t)fam | (uint64_t)a << 4 | (uint64_t)b << 8 | (uint64_t)c << 12 | (uint64_t)d << 16 | (uint64_t)e << 20 | (uint64_t)f << 24 | (uint64_t)g << 28;
}
constexpr int la_mb_form_block(int fam) { return fam == MBK_MB || fam == MBK_WIDE ? 512 : 256; }
constexpr int la_mb_form_lds(int fam, int a, int b, int f) {
    return fam == MBK_MB ? la_mb_lds_mb(b) : fam == MBK_WIDE ? la_mb_lds_wide(a, b) : fam == MBK_FAT ? la_mb_lds_fat(a, b, f) : LA_MB_LDS_FATD;
}
// form ids = row indices, e.g. MBF_WIDE_4_2_SLAB_0_2_0_0
#define LA_MBF_ID(FAM, a, b, c, d, e, f, g) MBF_##FAM##_##a##_##b##_##c##_##d##_##e##_##f##_##g,
enum MbFormId { LA_MB_FORMS(LA_MBF_ID) MBF_COUNT };
#undef LA_MBF_ID
#define LA_MBF_ROW(FAM, a, b, c, d, e, f, g) \
    {la_mb_form_key(MBK_##FAM, a, b, MB_##c, d, e, f, g), la_mb_form_block(MBK_##FAM), la_mb_form_lds(MBK_##FAM, a, b, f), \
     #FAM "<" #a "," #b "," #c "," #d "," #e "," #f "," #g ">"},
static constexpr MbFormRow kMbForms[MBF_COUNT] = { LA_MB_FORMS(LA_MBF_ROW) };
#undef LA_MBF_ROW
inline int la_mb_form_find(int fam, int a, int b, int c, int d = 0, int e = 0, int f = 0, int g = 0) {
    const uint64_t key = la_mb_form_key(fam, a, b, c, d, e, f, g);
    for (int i = 0; i < MBF_COUNT; ++i) if (kMbForms[i].key == key) return i;
    return -1;
}

// what the choice depends on (lk_mb_gemm fills it from MbArgs), and the knobs it reads (la_knobs.h: globals in the lab build, constexprs in
// the product build — the caller fills the struct, so the product build folds them)
struct MbFormIn {
    int kind;                // = EPI; RBV = 2 row-blocks per workgroup for MB_SLAB / MB_QKV, 4 for MB_SWIGLU / MB_LOGITS
    int nblk, n_wg, ksplit, K16, N, R, planned, gu_interleaved, ex_n;
    int nblk_dev;            // 1 = the block count is a device value (gathered expert)
    int bias;                // 1 = MB_QKV with a q/k/v bias
};
struct MbFormKnobs { int pair, narrow, dbg, sch, ks2, ex_d4, fatd, fatx; };   // g_la_mb_pair, _mb_narrow, _mb_dbg, _mb_sch, _mb_ks2, _ex_d4, _fatd, _fatx
struct MbForm {
    int id;                  // row of kMbForms, or -1 = refuse
    unsigned gx, gy, gz;
    int regions;             // adjacent weight regions per workgroup (1, 2 or 4): merge_regions rewrites MbArgs for them
    int w_keep, xcd_map;     // MbArgs fields of the same names
};

inline MbForm la_mb_select(const MbFormIn& s, const MbFormKnobs& k) {
    const int EPI = s.kind, RBV = (EPI == MB_SLAB || EPI == MB_QKV) ? 2 : 4;
    const int nblk = s.nblk, n_wg = s.n_wg, ksplit = s.ksplit, K16 = s.K16, R = s.R;
    const unsigned un_wg = (unsigned)n_wg, uks = (unsigned)ksplit;
    auto form = [](int id, unsigned gx, unsigned gy, unsigned gz, int regions = 1, int w_keep = 0, int xcd_map = 0) {
        return MbForm{id, gx, gy, gz, regions, w_keep, xcd_map};
    };
    // schedule (k_gemm_wide SCH): buffer-addressed pieces everywhere; a fragment read after every MFMA where a wave has >= 3 token tiles
    // (6+ MFMAs per half stage to cover a read; with 1-2 tiles the reads-together form covers them better).  Mistral bs=8 9.88-9.97 ->
    // 9.70-9.72 ms, 13B bs=4 10.68-10.73 -> 10.59-10.63 ms per step (profiles/r04_wide_gemm_schedule.txt); la_lab_set(24, 0) = schedule 0
    auto wide = [&](int rbv, int tw) { return la_mb_form_find(MBK_WIDE, rbv, tw, EPI, 0, k.sch ? (tw >= 3 ? 3 : 2) : 0); };
    const MbForm refuse = form(-1, 0, 0, 0);
    if (EPI < MB_SLAB || EPI > MB_LOGITS || nblk < 1 || nblk > 8 || n_wg < 1) return refuse;
    if (s.bias && k.dbg == 4) return refuse;      // the no-epilogue measurement build would drop the bias
    // mb_k_range cuts an even K16 on even k-tiles: with fewer than two k-tiles per split a split would be EMPTY (t0 == t1), which only the
    // fat launches guard against — k_gemm_wide's DMA clamp (t1 - 1) would read below its range.  No engine shape gets here (resolve_cfg keeps
    // >= 4 k-tiles per split); refuse instead of computing garbage.
    if (ksplit < 1 || (ksplit > 1 && K16 < 2 * ksplit)) return refuse;
    if (s.nblk_dev) {
        // gathered expert: the block count is a device value (typically 1-2 of the step's nblk): passes of two blocks, a pass
        // past the expert's count returns before it touches the weights
        const unsigned passes = (unsigned)(nblk + 1) / 2;
        if (EPI == MB_SLAB || EPI == MB_SWIGLU) {
            if (s.ex_n > 1 && (k.ex_d4 & (RBV == 4 ? 4 : 8)) && n_wg % 2 == 0 && (EPI == MB_SLAB || (s.planned && !s.gu_interleaved))) {
                // round 5 (la_lab_set key 25, bit 2 = gate/up, bit 3 = down): TWO adjacent weight regions per workgroup.  Every workgroup of an
                // expert stages the expert's whole x through LDS: 0.5-1.8 MB from L2 per 0.9 MB of weights from HBM, and the per-CU times of
                // the two ADD (T = W / 25 GB/s + x / 130 GB/s) — the gap between these launches (4.6-5.2 TB/s of weights) and the
                // dense 64-row kernels (5.9).  With two regions per workgroup the x traffic and the LDS reads per weight byte halve: the 8 waves
                // are 2 RBV row-blocks x 4 / RBV K parts (gate/up: one row-block per wave over the whole K range; down: 2 K parts instead of 4).
                // FEWER K parts = ANOTHER fp32 summation order than the one-region launch: results agree to tolerance, not bitwise
                // (include/lookahead_hip_lab.h key 25; tests/test_gpu_mblock.py::test_merged_expert_launch_forms_agree asserts 1e-2) —
                // so Mixtral's default numerics moved by that much when this form became the default in round 5.
                return form(la_mb_form_find(MBK_MB, 2 * RBV, 4, EPI, 1, 8), un_wg / 2, uks, passes * s.ex_n, 2);
            }
            if (s.ex_n > 1) {
                // two workgroups per CU (D = 4, <= 128 VGPRs): la_lab_set key 25 bit 0 = the gate/up launch (default on: Mixtral bs=4
                // 21.0-21.5 -> 20.1-20.2 ms per step), bit 1 = the down launch (RBV = 2: 44 B per lane of scratch at that bound)
                return form(la_mb_form_find(MBK_MB, RBV, 4, EPI, 1, (k.ex_d4 & (RBV == 4 ? 1 : 2)) ? 4 : 8), un_wg, uks, passes * s.ex_n);
            }
        }
        return form(la_mb_form_find(MBK_MB, RBV, 4, EPI, 0, 8), un_wg, uks, passes);
    }
    if (nblk < 3 || k.narrow) {
        // token blocks per pass: the smallest template that covers the step in <= 2 passes
        const int nt = nblk <= 1 ? 2 : nblk == 2 ? 4 : 8;
        return form(la_mb_form_find(MBK_MB, RBV, nt, EPI, 0, 8), un_wg, uks, nt == 8 ? (unsigned)(nblk + 3) / 4 : 1);
    }
    // nblk >= 3: every token block in ONE weight pass (k_gemm_wide): RBV = 4 -> 4 TW token blocks per workgroup, RBV = 2 -> 8 TW
    const int tw4 = (nblk + 1) / 2 < 4 ? (nblk + 1) / 2 : 4;        // 64-row blocks per workgroup = TW of the RBV = 4 / 8 forms (2..4)
    const unsigned halves = (unsigned)(nblk + 1) / 2, quarters_z = (unsigned)(nblk + 3) / 4;
    if (RBV == 4 && EPI == MB_SWIGLU && k.dbg && nblk >= 7)         // measurement builds of the 512-row gate/up launch (la_lab_set key 4); 6 stamps
        return form(la_mb_form_find(MBK_WIDE, 4, 4, MB_SWIGLU, k.dbg, k.dbg == 6 ? 3 : 0), un_wg, uks, 1);
    if (RBV == 2) {
        // Paired form (MB_SLAB, MB_QKV): TWO adjacent weight regions per workgroup and HALF the token blocks — the RBV = 4 wave
        // grid (2 row groups x 4 token groups) over regions {2 x, 2 x + 1}, grid.z = 2 token halves.  Every workgroup re-reads the
        // whole x operand of its token blocks from L2 (1 GB per launch at 512 rows and 256 workgroups: the dominant term of these
        // launches); pairing halves that, and the second reader of a weight region (z = 1, 128 workgroup ids later: same XCD)
        // finds it in L2.  Same MFMAs on the same operands in the same order per output: bit-identical results.
        // Quad form (MB_QKV of a GQA model at >= 7 blocks: small N, many rows — the x re-reads dominate): FOUR adjacent regions and
        // a QUARTER of the token blocks per workgroup.  L2 -> LDS traffic of the launch = x bytes x (workgroup columns) + W bytes x
        // (token groups): Mistral QKV at 512 rows 512 + 100 MB paired -> 256 + 200 MB quad; not taken where W dominates
        // (MHA / 13B shapes, <= 4 blocks).  Same MFMA chain per output element: bit-identical to the paired and unpaired forms.
        if (EPI == MB_QKV) {
            const double xb = (double)nblk * 64 * K16 * 32, wb = (double)s.N * K16 * 32;       // bytes of x and of W
            const double paired = xb * (n_wg / 2) + wb * ((nblk + 3) / 4), quad = xb * (n_wg / 4) + wb * ((nblk + 1) / 2);
            if ((k.pair & 4) && s.planned && nblk >= 7 && n_wg % 4 == 0 && (n_wg / 4 * ksplit) % 8 == 0 && quad < 0.85 * paired)
                return form(wide(8, 2), un_wg / 4, uks, halves, 4, 1);
            // round 5 (bit 8 of key 6): ONE {lo, hi} region x 256 rows per workgroup as four fat waves of 2 row-blocks x 2 token blocks.
            // The paired quarters give a CU TWO regions' weights for 128 rows, and the token groups run in lockstep, so every CU waits for
            // its weights at the HBM-class rate: 1.05 MB per CU at the Mistral shape (512 rows) = the 42 of the launch's 45 us.  One
            // region x 256 rows: half the weight bytes per CU, twice the x (which comes from L2).  Taken at <= 4 blocks, and at 5-8
            // blocks when the two token halves still fit one wave of workgroups (the fuller QKV image of a GQA model: 96 x 2).
            // bit 12 of key 6: the same one-region form with ONE token tile per wave (128 rows per workgroup, grid.z = pairs of blocks) where 256
            // rows per workgroup leave most of the chip idle — the fuller GQA image (Mistral / Mixtral: 96 regions) at 3-4 blocks is 96
            // workgroups on 256 CUs, each waiting for 0.5 MB of weights at the HBM-class per-CU rate; two token groups = 192 workgroups
            // (the second reader of a region finds it in L2).  <= 2 blocks: the 2 x 2 form would run MFMAs on absent blocks.
            const bool one_region = (k.pair & 256) && ksplit == 1 && (K16 & 1) == 0 && (R & 1) == 0 && k.dbg == 0;
            const int rv = (R & 3) == 0 ? 4 : 2;     // RoPE pairs per workgroup: groups of 4 (7B, Mistral, Mixtral) or 2 (13B) rows per store
            if (one_region && (k.pair & 4096) && nblk <= 4 && (nblk <= 2 || n_wg <= 128))
                return form(la_mb_form_find(MBK_FAT, 2, 1, MB_QKV, rv, 0, 2), un_wg, 1, halves);
            // Measured (profiles/r05_fat_waves.txt, call 7): 13B bs=4 10.64 -> 10.59 ms, Mixtral bs=4 19.65 -> 19.41 at 4 blocks; Mistral bs=8
            // (8 blocks, two token halves) 9.465 -> 9.489: taken at <= 4 blocks only (bit 9 forces the 5-8 block form: measurement).
            if (one_region && (quarters_z == 1 || ((k.pair & 512) && un_wg * quarters_z <= 256)))
                return form(la_mb_form_find(MBK_FAT, 2, 2, MB_QKV, rv, quarters_z == 1 ? 2 : 0, 2), un_wg, 1, quarters_z);
        }
        // round 5 (bit 10 of key 6): the slab launches (o_proj / down) at <= 4 blocks as ONE 64-row weight region x 256 rows per workgroup
        // (four fat waves of 2 row-blocks x 2 token blocks) instead of two regions x 128 rows: half the weight bytes per CU at the
        // HBM-class rate, twice the x from L2 — the trade that paid for gate/up and QKV at 256 rows.  Measured SLOWER here (13B bs=4 10.50 ->
        // 10.63 ms, Mixtral bs=4 19.15 -> 19.45, profiles/r05_fat_waves.txt call 8): opt-in, bit-identical.
        if (EPI == MB_SLAB && (k.pair & 1024) && nblk <= 4 && (K16 & 1) == 0 && K16 >= 2 * ksplit && k.dbg == 0 && !s.planned)
            return form(la_mb_form_find(MBK_FAT, 2, 2, MB_SLAB, 4, 2, 2), un_wg, uks, 1);
        if ((k.pair & 1) && n_wg % 2 == 0 && (n_wg / 2 * ksplit) % 8 == 0) {
            // la_lab_set key 12 (slab launches with <= 2 K splits): more token groups instead — 2 blocks per workgroup at every block count
            // QKV over at most 128 (fuller) workgroups — the multi-block image of a GQA model, cfg.qkv_mb_wg — takes token QUARTERS at
            // every block count: n_wg / 2 x 4 <= 256 workgroups of 4 row-blocks x 4 token tiles (la_lab_set(6, 9) forces the form)
            // round 5 (bit 5 of key 6): the paired slab / QKV launches as four fat waves of 4 row-blocks x TW token blocks (k_gemm_fat);
            // every K split must hold an even number of k-tiles
            const bool fat = (k.pair & 32) && (K16 & 1) == 0 && K16 >= 2 * ksplit && k.dbg == 0;
            const bool quarters = nblk <= 4 || (EPI == MB_SLAB && k.ks2 && ksplit <= 2) || (EPI == MB_QKV && (n_wg <= 128 || (k.pair & 8)));
            const unsigned gz = quarters ? halves : quarters_z;
            if (EPI == MB_SLAB && fat) {
                // bit 13 of key 6: one K split per XCD (k_gemm_fat, MbArgs.xcd_map) — 2 / 4 / 8 splits over a grid of a multiple of 8 workgroups
                // (bit 14: also on grids that are not whole multiples of 256 workgroups — the forced-4-split 13B launch over 160 workgroups that measured
                //  30 % slower with the mapping, profiles/r05_fat_waves.txt call 14: measurement only)
                const unsigned total = un_wg / 2 * uks * gz;
                const int xcd_map = ((k.pair & 8192) && (ksplit == 2 || ksplit == 4 || ksplit == 8) && total % 8 == 0 && (total % 256 == 0 || (k.pair & 16384))) ? 1 : 0;
                // round 6 (late; knob 36, default on): the two-token-tile form with x DIRECT (k_gemm_fat, STG = 2): 43.1 -> 41.2 us per launch at the
                // Mistral shape, 512 rows.  The other one-row-group forms (quarters, QKV, one-region gate/up) measured level or slower with it.
                return form(la_mb_form_find(MBK_FAT, 4, quarters ? 1 : 2, MB_SLAB, 4, 0, 4, (k.fatx && !quarters) ? 2 : 0), un_wg / 2, uks, gz, 2, 1, xcd_map);
            }
            if (EPI == MB_QKV && fat && (R & 1) == 0)
                return form(la_mb_form_find(MBK_FAT, 4, quarters ? 1 : 2, MB_QKV, (R & 3) == 0 ? 4 : 2, 0, 4), un_wg / 2, uks, gz, 2, 1);
            if (!quarters && k.dbg == 4) return form(la_mb_form_find(MBK_WIDE, 4, 2, EPI, 4, 0), un_wg / 2, uks, gz, 2, 1);   // measurement: no epilogue
            return form(wide(4, quarters ? 1 : 2), un_wg / 2, uks, gz, 2, 1);
        }
        if (nblk <= 4) return form(wide(2, 1), un_wg, uks, quarters_z);
        return form(wide(2, 2), un_wg, uks, 1);
    }
    if (EPI == MB_SWIGLU) {
        // round 5 (bit 6 of key 6): ONE planned region x ALL token blocks per workgroup as four fat waves (4 row-blocks x TW token blocks each,
        // 1 x 4 wave grid).  The paired fat form makes every CU pull TWO regions' weights, and since the two token halves run in lockstep
        // both wait for the same HBM miss: 1.83 MB per CU at the HBM-class per-CU rate (~25 GB/s) = 73 us of the 103-113 us launch at the
        // Mistral shape, 512 rows.  One region per workgroup: 0.92 MB of weights (nt) + 4 MB of x from L2 (~130 GB/s) per CU.
        // Measured (profiles/r05_fat_waves.txt, call 6): it wins at <= 4 blocks (13B 256 rows 90.3 -> 84.6 us, 13B bs=4 10.77 -> 10.63 ms per
        // step) and LOSES at 512 rows (Mistral 115.8 -> 121.2 us: 4 MB of x per CU instead of 2) — so it is taken at <= 4 blocks only;
        // bit 7 forces it at every block count (measurement).
        if ((k.pair & 64) && s.planned && !s.gu_interleaved && ksplit == 1 && (K16 & 1) == 0 && (nblk <= 4 || ((k.pair & 128) && nblk <= 8)))
            return form(la_mb_form_find(MBK_FAT, 4, tw4, MB_SWIGLU, 4, 2, 4), un_wg, 1, 1);
        // paired gate/up launch (planned images): regions {2 x, 2 x + 1} = row-blocks 0..7, half the token blocks per workgroup.
        // Bit-identical, but NOT faster (this launch is bound by its MFMA / ds_read side, not by the x traffic: 512 rows 116.5 vs
        // 116.4 us, 256 rows 68.4 vs 76.6 us at the 7B shape, profiles/r02b_mblock_paired_ab.txt): opt-in (la_lab_set(6, 3)).
        if ((k.pair & (2 | 16)) && s.planned && !s.gu_interleaved && n_wg % 16 == 0 && ksplit == 1) {
            int id;
            // round 5 (bit 4 of key 6): the same pair of regions as FOUR fat waves (4 x TW accumulator tiles each, one wave per SIMD): k_gemm_fat
            if (!((k.pair & 16) && (K16 & 1) == 0)) id = wide(8, tw4);
            else if (k.pair & 2048) id = la_mb_form_find(MBK_FAT, 8, tw4, MB_SWIGLU, 4, 0, 4, 1);      // bit 11: the register-staged form (k_gemm_fat, STG = 1)
            // round 6 (late; knob 35, default on): weights straight into MFMA operand registers (k_gemm_fatd) at 5-8 blocks (an even number of
            // k-tiles).  Measured (profiles/r06_gateup_direct_weights.txt): 512 rows 115.4 -> 109.1 us per launch at the Mistral
            // shape, Mistral bs=8 9.55 -> 9.36 ms per step, Llama-2-7B bs=8 9.94 -> 9.76; bit-identical.
            else if (k.fatd && tw4 >= 3 && R <= 64) id = la_mb_form_find(MBK_FATD, tw4, 0, MB_SWIGLU);
            else id = la_mb_form_find(MBK_FAT, 8, tw4, MB_SWIGLU, 4, 0, 4, 0);
            return form(id, un_wg / 2, 1, 2, 2, 1);
        }
    }
    return form(wide(4, tw4), un_wg, uks, 1);
}
