// la_rows.h — which tree row a workgroup of a row stage serves (la_penalty.hip: k_pen_argmax; la_sample.hip: k_sample_rows), and
// the repetition-penalty arithmetic both stages apply to the members of a row's context.  One workgroup per (row, block): the row
// addressing and the liveness rules of the four step forms (LA_PEN_SINGLE / BATCH / MBLOCK / ROWS) live here only.
#pragma once
#include "la_common.h"
#include "la_kernels.h"
#include "la_mblock.h"

// the processor's arithmetic on one stored value
__device__ __forceinline__ float pen_value(bf16_t x, float p) {
    const float v = bf2f(x);
    return bfr(v < 0.f ? v * p : v / p);
}

// Which row of which slot this workgroup serves, and whether the step reads its argmax at all.
struct PenRow {
    bool live;
    int slot;            // context bitmap
    int row0;            // first row of the block the ancestor bits of rowmask[row] count from (ids / rowmask index base)
    int row;             // row of logits / ids / rowmask / out
    unsigned long long path;
};

__device__ __forceinline__ PenRow pen_row(const PenArgs& a) {
    PenRow r{false, 0, 0, 0, 0ull};
    const int j = (int)blockIdx.x;
    if (a.kind == LA_PEN_SINGLE) {
        const int T = a.state[LA_ST_T], mode = a.state[LA_ST_MODE];
        r.live = j < T && (mode == 0 || (mode == 1 && j == T - 1));          // a prefill chain emits from its last row only
        r.row = j;
    } else if (a.kind == LA_PEN_BATCH) {
        const int slot = a.state[LA_BST_SEQ + j];
        r.row = j;
        if (slot >= 0 && slot < a.n_slots) {
            const int mode = a.in[LA_BIN_MODE + slot];
            bool last = true;                                                  // the slot's last block row
            for (int q = j + 1; q < LA_TREE_MAX; ++q) last = last && a.state[LA_BST_SEQ + q] != slot;
            r.live = mode == 0 || (mode == 1 && last);
            r.slot = slot;
        }
    } else if (a.kind == LA_PEN_MBLOCK) {
        const int b = (int)blockIdx.y;
        const int* mt = a.meta + b * LA_MB_META;
        const int slot = mt[LA_MBM_SLOT], T = mt[LA_MBM_T], mode = mt[LA_MBM_MODE];
        bool last_of_slot = true;                                              // a prompt's last block of this pass
        for (int q = b + 1; q < a.nblk; ++q) last_of_slot = last_of_slot && a.meta[q * LA_MB_META + LA_MBM_SLOT] != slot;
        r.live = slot >= 0 && slot < a.n_slots && j < T && (mode == 0 || (mode == 1 && j == T - 1 && last_of_slot));
        r.slot = slot;
        r.row0 = b * 64;
        r.row = b * 64 + j;
    } else {                                                                   // LA_PEN_ROWS: every row of slot 0 (unit entry)
        r.live = j < a.n_rows;
        r.row = j;
    }
    if (r.live && a.rowmask) r.path = a.rowmask[r.row];
    return r;
}
