// Decoding a matching on the device: the QAP objective of all_acc_qap (toolbox/metrics.py:168-193) and the greedy refinement
// greedy_qap (toolbox/utils.py:225-256: perm_matrix, score, improve) on the bit-packed 0/1 adjacency pairs.
//
// With P[i, pi(i)] = 1 the reference's matrices are
//     (A P B)[i][j]       = sum_k A[i,k] B[pi(k), j]                 improve(): the cost of the next assignment problem is its negative
//     trace(A P B P^T)    = sum_{i,k} A[i,k] B[pi(k), pi(i)]         score(): twice its first value
//     sum(g1 * g2[pi][:, pi]) = sum_{i,k} A[i,k] B[pi(i), pi(k)]     all_acc_qap's qap (the same number when A or B is symmetric)
// and on 0/1 matrices each is a popcount: with A'[i] = row i of A with bit k moved to bit pi(k) (built ONCE per row, by a gather
// through the inverse matching), (A P B)[i][j] = popc(A'[i] & Bt[j]) with Bt the bit transpose of B (built once per workgroup with
// wave ballots: nothing assumes B symmetric), qap = sum_i popc(A'[i] & B[pi(i)]) and the trace = sum_i popc(A'[i] & Bt[pi(i)]).
// One pair's matrices are at most 2 x 8 KB: they live in LDS.  Rows are NW in {1, 2, 4, 8} words (N <= 32 NW), zero-filled past the
// valid corner, so nothing outside the corner is trusted.  Rows that lanes gather from at lane-dependent words have an odd pitch.
#include "fgnn_qap_bits.h"

namespace {

constexpr int QAP_SLAB = 64;               // rows of the cost matrix per workgroup of the improve-cost kernel

// inv[m] = the row matched to column m (-1: none) for the columns of the corner; returns 1 if an entry of the corner is not a column of it
template <int NW>
DEVI int stage_inverse(int *inv, const int *pi, int n, int tid) {
    for (int m = tid; m < 32 * NW; m += QAP_THREADS) inv[m] = -1;
    __syncthreads();
    int bad = 0;
    for (int k = tid; k < n; k += QAP_THREADS) {
        const int p = pi[k];
        if (p >= 0 && p < n) inv[p] = k;
        else bad = 1;
    }
    return bad;
}

// cost[b][i][j] = -(A P B)[i][j] on the corner.  grid (ceil(N / 64), B): a workgroup stages Bt (all of it), its 64 rows of A, their
// permuted form, then thread (j, row group) walks its rows with Bt[j] in registers and A'[i] as an LDS broadcast; stores run along j.
template <int NW>
__global__ __launch_bounds__(QAP_THREADS) void qap_improve_cost_kernel(const unsigned *bits1, const unsigned *bits2, const int *assign,
                                                                       const int *nvalid, int N, float *cost, long long bstride, int ld) {
    constexpr int PA = NW | 1, NJ = 32 * NW, RG = QAP_THREADS / NJ;
    __shared__ __attribute__((aligned(16))) unsigned bt[32 * NW * NW];
    __shared__ __attribute__((aligned(16))) unsigned a_perm[QAP_SLAB * NW];
    __shared__ unsigned a_raw[QAP_SLAB * PA];
    __shared__ int inv[32 * NW];
    const int b = blockIdx.y, i0 = blockIdx.x * QAP_SLAB, tid = threadIdx.x;
    const int n = corner_of(nvalid, b, N), W = (N + 31) >> 5;
    if (i0 >= n) return;                        // uniform
    const int rows = min(QAP_SLAB, n - i0);
    const unsigned *A = bits1 + (long long)b * N * W, *Bm = bits2 + (long long)b * N * W;
    stage_inverse<NW>(inv, assign + (long long)b * N, n, tid);
    stage_rows<NW>(a_raw, PA, A, i0, QAP_SLAB, n, W, tid);
    stage_transposed<NW>(bt, NW, Bm, n, W, tid);
    __syncthreads();
    for (int idx = tid; idx < rows * NW; idx += QAP_THREADS) {
        const int r = idx / NW, w = idx - r * NW;
        a_perm[idx] = permuted_word(a_raw + r * PA, inv, w);
    }
    __syncthreads();
    const int j = tid % NJ, rg = tid / NJ;
    if (j >= n) return;
    unsigned btj[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) btj[w] = bt[j * NW + w];
    float *out = cost + (long long)b * bstride + (long long)i0 * ld + j;
    for (int r = rg; r < rows; r += RG) {
        int acc = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) acc += __popc(a_perm[r * NW + w] & btj[w]);
        out[(long long)r * ld] = (float)(-acc);
    }
}

// One workgroup per pair, thread i owns row i: A'[i] word by word against B[pi(i)] (TRACE: against Bt[pi(i)], the trace form of
// score(); planted is then not defined and must be NULL), plus the three plain sums.
template <int NW, bool TRACE>
__global__ __launch_bounds__(QAP_THREADS) void qap_objective_kernel(const unsigned *bits1, const unsigned *bits2, const int *assign,
                                                                    const int *nvalid, int N, int *qap, int *planted, int *na, int *nb) {
    constexpr int PA = NW | 1;
    __shared__ unsigned a_l[32 * NW * PA], b_l[32 * NW * PA];
    __shared__ int inv[32 * NW];
    __shared__ int red[QAP_THREADS / 64][5];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = corner_of(nvalid, b, N), W = (N + 31) >> 5;
    const unsigned *A = bits1 + (long long)b * N * W, *Bm = bits2 + (long long)b * N * W;
    const int *pi = assign + (long long)b * N;
    int v[5] = {0, 0, 0, 0, 0};                 // qap, planted, na, nb, bad
    v[4] = stage_inverse<NW>(inv, pi, n, tid);
    stage_rows<NW>(a_l, PA, A, 0, 32 * NW, n, W, tid);
    if (TRACE) stage_transposed<NW>(b_l, PA, Bm, n, W, tid);
    else stage_rows<NW>(b_l, PA, Bm, 0, 32 * NW, n, W, tid);
    __syncthreads();
    if (tid < n) {
        const int p = pi[tid];
        const bool matched = p >= 0 && p < n;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            if (32 * w < n) {
                const unsigned ap = permuted_word(a_l + tid * PA, inv, w);
                const unsigned bp = matched ? b_l[p * PA + w] : 0u;
                const unsigned aw = a_l[tid * PA + w], bw = b_l[tid * PA + w];
                v[0] += __popc(ap & bp);
                v[1] += __popc(aw & bw);
                v[2] += __popc(aw);
                v[3] += __popc(bw);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        for (int o = 32; o > 0; o >>= 1) v[q] += __shfl_xor(v[q], o);
        if ((tid & 63) == 0) red[tid >> 6][q] = v[q];
    }
    __syncthreads();
    if (tid == 0) {
        int s[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) s[q] = red[0][q] + red[1][q] + red[2][q] + red[3][q];
        if (qap) qap[b] = s[4] ? -1 : s[0];
        if (planted) planted[b] = s[1];
        if (na) na[b] = s[2];
        if (nb) nb[b] = s[3];
    }
}

// The bookkeeping of greedy_qap, one wave per pair.  round < 0: after the first improve() -- perm_best = the initial matching,
// acc_best = that improve()'s fixed points, t_best = 0 (s_best2 already holds the initial score).  round >= 0: keep the round's
// matching if its score is strictly better.
__global__ __launch_bounds__(64) void qap_keep_kernel(int round, const int *cur_q, const int *cur_correct, const int *cur_assign,
                                                      const int *nvalid, int N, int *s_best2, int *acc_best, int *t_best, int *perm_best) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = corner_of(nvalid, b, N);
    const bool take = round < 0 || cur_q[b] > s_best2[b];
    __syncthreads();
    if (!take) return;
    if (perm_best)
        for (int k = lane; k < N; k += 64) perm_best[(long long)b * N + k] = k < n ? cur_assign[(long long)b * N + k] : -1;
    if (lane == 0) {
        if (round >= 0) s_best2[b] = cur_q[b];
        acc_best[b] = cur_correct[b];
        t_best[b] = round < 0 ? 0 : round;
    }
}

template <int NW>
int launch_cost(const unsigned *bits1, const unsigned *bits2, const int *assign, const int *nvalid, int B, int N, float *cost,
                long long bstride, int ld, hipStream_t st) {
    hipLaunchKernelGGL((qap_improve_cost_kernel<NW>), dim3((N + QAP_SLAB - 1) / QAP_SLAB, B), dim3(QAP_THREADS), 0, st, bits1, bits2, assign,
                       nvalid, N, cost, bstride, ld);
    FGNN_LAUNCH_CHECK();
    return 0;
}
template <int NW, bool TRACE>
int launch_objective(const unsigned *bits1, const unsigned *bits2, const int *assign, const int *nvalid, int B, int N, int *qap,
                     int *planted, int *na, int *nb, hipStream_t st) {
    hipLaunchKernelGGL((qap_objective_kernel<NW, TRACE>), dim3(B), dim3(QAP_THREADS), 0, st, bits1, bits2, assign, nvalid, N, qap, planted,
                       na, nb);
    FGNN_LAUNCH_CHECK();
    return 0;
}
int improve_cost(const unsigned *bits1, const unsigned *bits2, const int *assign, const int *nvalid, int B, int N, float *cost,
                 long long bstride, int ld, hipStream_t st) {
    if (N <= 32) return launch_cost<1>(bits1, bits2, assign, nvalid, B, N, cost, bstride, ld, st);
    if (N <= 64) return launch_cost<2>(bits1, bits2, assign, nvalid, B, N, cost, bstride, ld, st);
    if (N <= 128) return launch_cost<4>(bits1, bits2, assign, nvalid, B, N, cost, bstride, ld, st);
    return launch_cost<8>(bits1, bits2, assign, nvalid, B, N, cost, bstride, ld, st);
}
template <bool TRACE>
int objective(const unsigned *bits1, const unsigned *bits2, const int *assign, const int *nvalid, int B, int N, int *qap, int *planted,
              int *na, int *nb, hipStream_t st) {
    if (N <= 32) return launch_objective<1, TRACE>(bits1, bits2, assign, nvalid, B, N, qap, planted, na, nb, st);
    if (N <= 64) return launch_objective<2, TRACE>(bits1, bits2, assign, nvalid, B, N, qap, planted, na, nb, st);
    if (N <= 128) return launch_objective<4, TRACE>(bits1, bits2, assign, nvalid, B, N, qap, planted, na, nb, st);
    return launch_objective<8, TRACE>(bits1, bits2, assign, nvalid, B, N, qap, planted, na, nb, st);
}

constexpr long long WS_ALIGN = 256;
long long ws_round(long long x) { return (x + WS_ALIGN - 1) / WS_ALIGN * WS_ALIGN; }

}  // namespace

extern "C" int fgnn_qap_objective(const unsigned *bits1, const unsigned *bits2, const int *assign, const int *nvalid, int B, int N, int *qap,
                                  int *planted, int *na, int *nb, void *stream) {
    FGNN_CHECK(bits1 && bits2 && assign && B > 0 && N > 0, "fgnn_qap_objective: bad arguments");
    FGNN_CHECK(N <= FGNN_QAP_MAX_N, "fgnn_qap_objective: at most %d vertices per graph (got %d)", FGNN_QAP_MAX_N, N);
    return objective<false>(bits1, bits2, assign, nvalid, B, N, qap, planted, na, nb, (hipStream_t)stream);
}

extern "C" int fgnn_qap_improve_cost(const unsigned *bits1, const unsigned *bits2, const int *assign, const int *nvalid, int B, int N,
                                     float *cost, long long bstride, int ld, void *stream) {
    FGNN_CHECK(bits1 && bits2 && assign && cost && B > 0 && N > 0, "fgnn_qap_improve_cost: bad arguments");
    FGNN_CHECK(N <= FGNN_QAP_MAX_N, "fgnn_qap_improve_cost: at most %d vertices per graph (got %d)", FGNN_QAP_MAX_N, N);
    FGNN_CHECK(ld >= N && bstride >= (long long)N * ld, "fgnn_qap_improve_cost: strides smaller than the matrices");
    return improve_cost(bits1, bits2, assign, nvalid, B, N, cost, bstride, ld, (hipStream_t)stream);
}

extern "C" long long fgnn_greedy_qap_ws_bytes(int B, int N) {
    if (B <= 0 || N <= 0) return 0;
    return ws_round((long long)B * N * N * 4) + ws_round((long long)B * N * 4) + 2 * ws_round((long long)B * 4);
}

// fgnn_greedy_qap (labels = NULL) and fgnn_greedy_qap_labels: one launch sequence; with labels a fgnn_count_matches launch overwrites
// `correct` after every solver call, so acc_best counts the matches with the labels instead of the fixed points
static int greedy(const unsigned *bits1, const unsigned *bits2, const int *assign0, const int *labels, const int *nvalid, int B, int N, int T,
                  void *ws, long long ws_bytes, int *s_best2, int *acc_best, int *t_best, int *perm_best, void *stream) {
    FGNN_CHECK(bits1 && bits2 && assign0 && ws && s_best2 && acc_best && t_best && B > 0 && N > 0 && T >= 0, "fgnn_greedy_qap: bad arguments");
    FGNN_CHECK(N <= FGNN_QAP_MAX_N, "fgnn_greedy_qap: at most %d vertices per graph (got %d)", FGNN_QAP_MAX_N, N);
    FGNN_CHECK(ws_bytes >= fgnn_greedy_qap_ws_bytes(B, N) && ((uintptr_t)ws & 15) == 0,
               "fgnn_greedy_qap: the workspace needs %lld bytes, 16-byte aligned (got %lld)", fgnn_greedy_qap_ws_bytes(B, N), ws_bytes);
    hipStream_t st = (hipStream_t)stream;
    char *p = (char *)ws;
    float *cost = (float *)p;
    p += ws_round((long long)B * N * N * 4);
    int *cur = (int *)p;
    p += ws_round((long long)B * N * 4);
    int *correct = (int *)p;
    p += ws_round((long long)B * 4);
    int *cur_q = (int *)p;
    const long long bs = (long long)N * N;
    int rc;
    // s_best = score(pi0); pi = improve(pi0) -- never scored -- sets acc_best, T_best = 0
    if ((rc = objective<true>(bits1, bits2, assign0, nvalid, B, N, s_best2, nullptr, nullptr, nullptr, st))) return rc;
    if ((rc = improve_cost(bits1, bits2, assign0, nvalid, B, N, cost, bs, N, st))) return rc;
    if ((rc = fgnn_lsap_accuracy(cost, bs, N, nvalid, B, N, correct, cur, stream))) return rc;
    if (labels && (rc = fgnn_count_matches(cur, labels, nvalid, B, N, correct, stream))) return rc;
    hipLaunchKernelGGL(qap_keep_kernel, dim3(B), dim3(64), 0, st, -1, cur_q, correct, assign0, nvalid, N, s_best2, acc_best, t_best, perm_best);
    FGNN_LAUNCH_CHECK();
    for (int i = 0; i < T; ++i) {
        if ((rc = improve_cost(bits1, bits2, cur, nvalid, B, N, cost, bs, N, st))) return rc;
        if ((rc = fgnn_lsap_accuracy(cost, bs, N, nvalid, B, N, correct, cur, stream))) return rc;
        if (labels && (rc = fgnn_count_matches(cur, labels, nvalid, B, N, correct, stream))) return rc;
        if ((rc = objective<true>(bits1, bits2, cur, nvalid, B, N, cur_q, nullptr, nullptr, nullptr, st))) return rc;
        hipLaunchKernelGGL(qap_keep_kernel, dim3(B), dim3(64), 0, st, i, cur_q, correct, cur, nvalid, N, s_best2, acc_best, t_best, perm_best);
        FGNN_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int fgnn_greedy_qap(const unsigned *bits1, const unsigned *bits2, const int *assign0, const int *nvalid, int B, int N, int T,
                               void *ws, long long ws_bytes, int *s_best2, int *acc_best, int *t_best, int *perm_best, void *stream) {
    return greedy(bits1, bits2, assign0, nullptr, nvalid, B, N, T, ws, ws_bytes, s_best2, acc_best, t_best, perm_best, stream);
}

extern "C" int fgnn_greedy_qap_labels(const unsigned *bits1, const unsigned *bits2, const int *assign0, const int *labels, const int *nvalid,
                                      int B, int N, int T, void *ws, long long ws_bytes, int *s_best2, int *acc_best, int *t_best,
                                      int *perm_best, void *stream) {
    FGNN_CHECK(labels, "fgnn_greedy_qap_labels: NULL labels");
    return greedy(bits1, bits2, assign0, labels, nvalid, B, N, T, ws, ws_bytes, s_best2, acc_best, t_best, perm_best, stream);
}
