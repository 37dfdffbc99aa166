// What the row-wise metric kernels share: the valid corner of a pair (planted.hip, qap.hip, qap_weighted.hip: corner_of; eval.hip,
// rank.hip: clamp_nv), the arg-max of a score row (eval.hip, train_ops.hip) and the launch geometry of the kernels that give every
// row a group of lanes (eval.hip, rank.hip).
#pragma once
#include "fgnn_common.h"

// The vertex count of pair b clamped to [0, N]: nothing outside the n x n corner is ever trusted.  One value, written in the two
// forms its callers were compiled from: the compiler keeps a wave-uniform clamp_nv on the scalar unit and moves a corner_of there
// to the vector unit (the fold kernels of eval.hip and rank.hip), and gives planted.hip and the qap files other selects for a
// clamp_nv, so each file keeps the form that keeps its instructions.
DEVI int corner_of(const int *nvalid, int b, int N) { return min(max(nvalid_of(nvalid, b, N), 0), N); }
DEVI int clamp_nv(const int *nvalid, int b, int N) {
    const int n = nvalid ? nvalid[b] : N;
    return n < 0 ? 0 : (n > N ? N : n);
}

struct RowMax {
    float best;
    int bj;
};

// The arg-max of row[0 .. n) by the W lanes of a row's group (64: a wave; 16: a quarter of one), np.argmax's order: the first
// maximum on ties, NaN above every number (the first NaN wins), column 0 for a row of -inf.  Lane `sub` takes the columns sub,
// sub + W, ... in ascending order; a lane without columns holds (-inf, INT_MAX), which loses every comparison with a real entry.
// The group meets by xor butterflies below W, so every lane of it returns the same (best, bj); n must be uniform in the group.
// Called by eval_pairs_kernel and accuracy_max_kernel; accuracy_max_labels_kernel (planted.hip) has the same text written out, and
// eval_ranks_kernel (rank.hip) does not call it but counts by its order: rank == 1 exactly when bj is the target.
template <int W>
DEVI RowMax row_argmax(const float *row, int n, int sub) {
    float best = -INFINITY;
    int bj = 0x7fffffff;
    for (int j = sub; j < n; j += W) {                   // ascending j: an equal later value never replaces
        const float v = row[j];
        if (bj == 0x7fffffff || (best == best && (v > best || v != v))) {
            best = v;
            bj = j;
        }
    }
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) {                // ties towards the smaller index
        const float ob = __shfl_xor(best, o);
        const int oj = __shfl_xor(bj, o);
        const bool onan = ob != ob, bnan = best != best;
        if (onan ? (!bnan || oj < bj) : (!bnan && (ob > best || (ob == best && oj < bj)))) {
            best = ob;
            bj = oj;
        }
    }
    return {best, bj};
}

// Row groups: W = row_group_width(N) lanes per row (64: one wave per row; 16: four rows per wave, for rows of at most 16 columns),
// threads / W rows per workgroup.  row_group_wgs: the workgroups of a launch over the B N rows, 0 when they are more than one
// launch takes (B, N > 0, so a launch that fits has at least one).
inline int row_group_width(int N) { return N <= 16 ? 16 : WAVE; }
inline unsigned row_group_wgs(int B, int N, int threads) {
    const long long per = threads / row_group_width(N), wgs = ((long long)B * N + per - 1) / per;
    return wgs <= 0x7fffffffll ? (unsigned)wgs : 0u;
}
