// What the kernels on bit-packed adjacency pairs share (qap.hip, qap_2opt.hip): the corner masks, the staging of bit rows into LDS,
// the ballot bit transpose and the gather of a row's bits through a matching.  One workgroup of QAP_THREADS threads per call.
#pragma once
#include "fgnn_rows.h"

namespace {

constexpr int QAP_THREADS = 256;           // 4 waves: wave w transposes rows 64 w .. 64 w + 63 (N <= 256)

// the bits of word w of a row that lie inside the n x n corner
DEVI unsigned corner_mask(int w, int n) {
    const int lo = 32 * w;
    return n >= lo + 32 ? 0xffffffffu : (n > lo ? (1u << (n - lo)) - 1u : 0u);
}
// rows r0 .. r0 + rows - 1 of a bit matrix -> dst (row pitch P words, NW words per row written), zero outside the corner
template <int NW>
DEVI void stage_rows(unsigned *dst, int P, const unsigned *g, int r0, int rows, int n, int W, int tid) {
    for (int idx = tid; idx < rows * NW; idx += QAP_THREADS) {
        const int r = idx / NW, w = idx - r * NW, gi = r0 + r;
        dst[r * P + w] = (gi < n && w < W) ? g[(long long)gi * W + w] & corner_mask(w, n) : 0u;
    }
}
// the bit transpose of the n x n corner: dst[j * P + w] bit t = M[32 w + t][j], rows j < 32 ceil(n / 32) written (NW words each).
// Thread tid holds row tid in registers; bit j of the 64 rows of a wave is one ballot, which lane j % 32 keeps.
template <int NW>
DEVI void stage_transposed(unsigned *dst, int P, const unsigned *g, int n, int W, int tid) {
    const int wv = tid >> 6, lane = tid & 63;
    unsigned row[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) row[w] = (tid < n && w < W) ? g[(long long)tid * W + w] & corner_mask(w, n) : 0u;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        if (32 * w >= n) break;                 // uniform
        unsigned lo = 0, hi = 0;
#pragma unroll 8
        for (int t = 0; t < 32; ++t) {
            const unsigned long long m = __ballot((row[w] >> t) & 1u);
            if ((lane & 31) == t) {
                lo = (unsigned)m;
                hi = (unsigned)(m >> 32);
            }
        }
        if (lane < 32) {
            const int j = 32 * w + lane;
            if (2 * wv < NW) dst[j * P + 2 * wv] = lo;
            if (2 * wv + 1 < NW) dst[j * P + 2 * wv + 1] = hi;
        }
    }
}
// word w of A'[r]: bit m = A[r][inv[m]] (a: rows of A with pitch PA)
DEVI unsigned permuted_word(const unsigned *arow, const int *inv, int w) {
    unsigned v = 0;
#pragma unroll 8
    for (int t = 0; t < 32; ++t) {
        const int k = inv[32 * w + t];
        const unsigned bit = k >= 0 ? (arow[k >> 5] >> (k & 31)) & 1u : 0u;
        v |= bit << t;
    }
    return v;
}

}  // namespace
