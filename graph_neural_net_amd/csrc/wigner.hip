// Correlated Gaussian (Wigner) pairs on the device (include/fgnn_hip.h; graph_neural_net_amd/wigner.py): A symmetric with
// independent N(0, c^2) entries above the diagonal, B = rho A + sig Z with an independent Z of the same law, both written in ONE
// launch as the reference's tensor representation (channel 0 = W, channel 1 = diag(row sums), loaders/data_generator.py:118-125).
// tests/wigner_ref.py restates every step in numpy.
//
// Addressing.  The normal of the unordered entry {i, j}, i < j, of stream s (10 parent, 11 noise) of pair k has the linear index
// t = i N + j with N the PADDED size, so an entry does not move when the vertex count changes: Philox block t >> 3 of the stream
// (counter (t >> 3, k, s, 0), key (seed, 0), fgnn_philox.h), 64-bit word (t & 7) >> 1 of it, w0 its low and w1 its high half.
// Box-Muller on 24-bit uniforms that are exact in fp32: u = ((w0 >> 8) + 1) 2^-24 in (0, 1], v = (w1 >> 8) 2^-24 in [0, 1),
// r = sqrtf(-2 logf(u)), z = r cospif(2 v) for even t and r sinpif(2 v) for odd t (t and t ^ 1 share their word pair).  The
// accurate logf / sinpif / cospif and IEEE sqrt and division: the Makefile builds this file without fast-math.  A value depends on
// (seed, k, i, j) only -- not on the launch, the vertex count, rho / sig (so a level changes no draw) or the support.
//
// Values.  A_ij = c z10(t), B_ij = fmaf(rho, A_ij, sig (c z11(t))), c = 1 / sqrtf(n) or 1; every product is rounded on its own
// (__fmul_rn: no contraction into a neighbouring addition).  With sig = 0 and rho = 1 side 2 equals side 1.
//
// Launch.  Grid (ceil(N / 16), B), 4 waves: a workgroup owns 16 output rows of both sides of one pair, a wave 4 consecutive rows,
// one at a time, its lanes striding the columns (lane l: columns l, l + 64, l + 128, l + 192).  Each lane computes the normal of
// (min, max) of its entry: the lower triangle costs its Philox blocks a second time, which is cheaper than a transpose through
// LDS at these sizes.  Every wave draws the vertex count itself (fgnn_pairgen_dev.h: the draws of fgnn_pairgen).  No LDS, no atomics.
// With labels the wave first inverts the permutation for its own rows and columns by one pass over the n labels (wave-uniform
// loads, compares only: a label is never an address), then writes side 2 at its OUTPUT position: out[r][c] = B[inv r][inv c].
//
// Row sums.  The sum of output row r is a function of the stored row alone: lane l adds its columns in ascending order,
// s_l = (((0 + w[l]) + w[l + 64]) + w[l + 128]) + w[l + 192] over the columns < N, then six butterfly steps s_l += s_(l ^ o),
// o = 32, 16, 8, 4, 2, 1 (both partners add the same two numbers: all lanes end with the same bits); fp32, round to nearest.  So
// the relabelled side sums its own row in its own column order, and the sum does not depend on B or on how a range is cut.
#include "fgnn_common.h"
#include "fgnn_pairgen_dev.h"
#include "fgnn_philox.h"

namespace {

constexpr int WG_WAVES = 4, WG_THREADS = WG_WAVES * 64;
constexpr int WG_RPW = 4;                          // rows per wave
constexpr int WG_ROWS = WG_WAVES * WG_RPW;         // rows per workgroup
constexpr int WG_COLS = FGNN_PAIRGEN_MAX_N / 64;   // columns per lane

// z_stream(t) of the file header
DEVI float wigner_normal(const Pair &pr, int stream, unsigned t) {
    const P4 r = pr.block(stream, (unsigned long long)(t >> 3));
    const int p = (t & 7) >> 1;
    const unsigned long long x = p == 0 ? r.v0 : p == 1 ? r.v1 : p == 2 ? r.v2 : r.v3;
    const unsigned w0 = (unsigned)x, w1 = (unsigned)(x >> 32);
    const float u = (float)((w0 >> 8) + 1u) * 0x1p-24f;       // exact: an integer <= 2^24 times a power of two
    const float v2 = (float)(w1 >> 8) * 0x1p-23f;             // 2 v, exact
    const float rad = sqrtf(-2.0f * logf(u));
    return __fmul_rn(rad, (t & 1) ? sinpif(v2) : cospif(v2));
}

DEVI bool support_bit(const unsigned *bits, long long off, int W, int i, int j) {      // bit (min, max) of the pair's words
    const int a = min(i, j), b = max(i, j);
    return (bits[off + a * W + (b >> 5)] >> (b & 31)) & 1u;
}

DEVI float row_sum(float s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s = __fadd_rn(s, __shfl_xor(s, o));
    return s;
}

// PERM: side 2 is written relabelled by a.labels
template <bool PERM>
__global__ __launch_bounds__(WG_THREADS) void wigner_kernel(fgnn_wigner_args a) {
    const int N = a.N, W = (N + 31) >> 5, b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long k = a.index ? a.index[b] : a.first + b;
    float rho = a.rho, sig = a.sig;
    if (a.level) {
        const int lv = a.level[b];
        if (lv < 0 || lv >= a.K) {
            k = -1;              // a level outside the table is a caller error like a negative index
        } else {
            rho = a.level_coef[2 * lv];
            sig = a.level_coef[2 * lv + 1];
        }
    }
    const Pair pr{a.seed, (unsigned long long)k};
    const int n = k < 0 ? 0 : uni(vertex_count(pr, N, a.thr_vertex, lane));      // 0: the empty graph, every entry below is zero
    if (a.nvalid && blockIdx.x == 0 && threadIdx.x == 0) a.nvalid[b] = n;
    if (!a.x1) return;           // the vertex counts only
    const float c = a.scale ? 1.0f / sqrtf((float)max(n, 1)) : 1.0f;
    const int r0 = blockIdx.x * WG_ROWS + wave * WG_RPW;

    // the source row / column of side 2's output rows r0 + q and columns lane + 64 m (-1: none, zeros)
    int sr[WG_RPW], sc[WG_COLS];
#pragma unroll
    for (int q = 0; q < WG_RPW; ++q) sr[q] = (!PERM && r0 + q < n) ? r0 + q : -1;
#pragma unroll
    for (int m = 0; m < WG_COLS; ++m) sc[m] = (!PERM && lane + 64 * m < n) ? lane + 64 * m : -1;
    if (PERM) {
        const int *lab = a.labels + (long long)b * N;
        for (int i = 0; i < n; ++i) {
            const int l = lab[i];                          // wave-uniform
            const int p = (l >= 0 && l < n) ? l : -1;      // (a row that is no permutation of [0, n) leaves zeros, nothing else)
#pragma unroll
            for (int q = 0; q < WG_RPW; ++q)
                if (p == r0 + q) sr[q] = i;
#pragma unroll
            for (int m = 0; m < WG_COLS; ++m)
                if (p == lane + 64 * m) sc[m] = i;
        }
    }

    const long long woff = (long long)b * N * W;
    for (int q = 0; q < WG_RPW && r0 + q < N; ++q) {       // (a run-time loop: one copy of the row body; wave-uniform bounds)
        const int row = r0 + q;
        int si = -1;
#pragma unroll
        for (int qq = 0; qq < WG_RPW; ++qq) si = qq == q ? sr[qq] : si;      // sr[q] without a run-time register index
        float v1[WG_COLS], v2[WG_COLS], s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int m = 0; m < WG_COLS; ++m) {
            const int col = lane + 64 * m;
            float x1 = 0.f, x2 = 0.f;
            if (col < N) {
                const bool in1 = row < n && col < n && col != row;
                const bool on1 = in1 && (!a.bits1 || support_bit(a.bits1, woff, W, row, col));
                const int sj = sc[m];
                const bool in2 = PERM ? (si >= 0 && sj >= 0 && si != sj) : in1;
                const bool on2 = in2 && (!a.bits2 || support_bit(a.bits2, woff, W, PERM ? si : row, PERM ? sj : col));
                if (PERM) {
                    if (on1) x1 = __fmul_rn(c, wigner_normal(pr, FGNN_WIGNER_PARENT_STREAM, (unsigned)(min(row, col) * N + max(row, col))));
                    if (on2) {
                        const unsigned t = (unsigned)(min(si, sj) * N + max(si, sj));
                        const float av = __fmul_rn(c, wigner_normal(pr, FGNN_WIGNER_PARENT_STREAM, t));
                        const float zv = __fmul_rn(c, wigner_normal(pr, FGNN_WIGNER_NOISE_STREAM, t));
                        x2 = fmaf(rho, av, __fmul_rn(sig, zv));
                    }
                } else if (on1 || on2) {
                    const unsigned t = (unsigned)(min(row, col) * N + max(row, col));
                    const float av = __fmul_rn(c, wigner_normal(pr, FGNN_WIGNER_PARENT_STREAM, t));
                    if (on1) x1 = av;
                    if (on2) x2 = fmaf(rho, av, __fmul_rn(sig, __fmul_rn(c, wigner_normal(pr, FGNN_WIGNER_NOISE_STREAM, t))));
                }
                s1 = __fadd_rn(s1, x1);
                s2 = __fadd_rn(s2, x2);
            }
            v1[m] = x1;
            v2[m] = x2;
        }
        s1 = row_sum(s1);
        s2 = row_sum(s2);
        float *o1 = a.x1 + ((long long)b * 2 * N + row) * N, *o2 = a.x2 + ((long long)b * 2 * N + row) * N;
        const long long plane = (long long)N * N;
#pragma unroll
        for (int m = 0; m < WG_COLS; ++m) {
            const int col = lane + 64 * m;
            if (col < N) {
                o1[col] = v1[m];
                o2[col] = v2[m];
                o1[plane + col] = col == row ? s1 : 0.f;
                o2[plane + col] = col == row ? s2 : 0.f;
            }
        }
    }
}

}  // namespace

extern "C" int fgnn_wigner_pairs(const fgnn_wigner_args *args, void *stream) {
    FGNN_CHECK(args, "fgnn_wigner_pairs: NULL arguments");
    const fgnn_wigner_args &a = *args;
    FGNN_CHECK(a.N >= 1 && a.N <= FGNN_PAIRGEN_MAX_N, "fgnn_wigner_pairs: N=%d outside [1, %d]", a.N, FGNN_PAIRGEN_MAX_N);
    FGNN_CHECK(a.B >= 0 && a.B <= 65535 && (a.index || a.first >= 0), "fgnn_wigner_pairs: bad arguments (B=%d in [0, 65535], first=%lld)",
               a.B, a.first);
    FGNN_CHECK(a.thr_vertex <= THR_ONE && a.thr_vertex > 0, "fgnn_wigner_pairs: vertex threshold outside (0, 2^32]");
    FGNN_CHECK(a.thr_vertex == THR_ONE || a.N >= 2, "fgnn_wigner_pairs: a binomial vertex count needs N >= 2");
    FGNN_CHECK(!a.x1 == !a.x2, "fgnn_wigner_pairs: x1 and x2 go together");
    FGNN_CHECK(a.x1 || a.nvalid, "fgnn_wigner_pairs: no output");
    FGNN_CHECK(!a.bits1 == !a.bits2, "fgnn_wigner_pairs: the support words of both sides go together");
    FGNN_CHECK(!a.level == !a.level_coef, "fgnn_wigner_pairs: level and level_coef go together");
    FGNN_CHECK(!a.level || (a.K >= 1 && a.K <= FGNN_MAX_LEVELS), "fgnn_wigner_pairs: K=%d levels outside [1, %d]", a.K, FGNN_MAX_LEVELS);
    if (a.B == 0) return 0;
    if (!a.x1) {                 // the vertex counts only: one wave per pair
        hipLaunchKernelGGL(wigner_kernel<false>, dim3(1, (unsigned)a.B), dim3(64), 0, (hipStream_t)stream, a);
    } else {
        const dim3 grid((unsigned)((a.N + WG_ROWS - 1) / WG_ROWS), (unsigned)a.B), block(WG_THREADS);
        if (a.labels)
            hipLaunchKernelGGL(wigner_kernel<true>, grid, block, 0, (hipStream_t)stream, a);
        else
            hipLaunchKernelGGL(wigner_kernel<false>, grid, block, 0, (hipStream_t)stream, a);
    }
    FGNN_LAUNCH_CHECK();
    return 0;
}
