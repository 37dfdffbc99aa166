// Decoding a matching on REAL-weighted pairs: the twin of qap.hip for fp32 matrices (a spectral L = D^-1/2 W D^-1/2, any weighted
// graph), where (A P B)[i][j] is no popcount but a product on the fp32 matrix cores.
//
//     (A P B)[i][j]    = sum_k A[i,k] B[pi(k), j]                  improve(): a GEMM whose right operand is ROW-GATHERED through pi
//     trace(A P B P^T) = sum_{i,k} A[i,k] B[pi(k), pi(i)]          score(): twice its first value
//     qap              = sum_{i,k} A[i,k] B[pi(i), pi(k)]          all_acc_qap's qap (differs from the trace when neither is symmetric)
//
// Matrices: fp32, row pitch ld, pairs gstride floats apart (channel 0 of a (B, C, N, N) batch in place: gstride = C N N).  Only the
// n_b x n_b corner is ever READ (it may be surrounded by NaN), rows pi(k) outside [0, n_b) count as zero rows.
// Every reduction has a fixed order (no float atomics): results are bit-identical from run to run.
#include "fgnn_rows.h"

namespace {

constexpr int QW_THREADS = 256;            // 4 waves
constexpr int QW_ROWS = 32;                // rows of the cost matrix per workgroup (one MFMA tile)
constexpr int QW_COLS = 128;               // columns per workgroup: wave w owns columns 32 w .. 32 w + 31 of them
constexpr int QW_KC = 32;                  // k per staged chunk
constexpr int QW_PA = QW_KC + 1;           // pitch of the A tile: lanes read it down a column (odd pitch: conflict-free)

// pi_l[k] = pi(k) if it is a column of the corner, else -1, for k < n; returns 1 if this thread saw an entry that is not
DEVI int stage_assign(int *pi_l, const int *pi, int n, int tid) {
    int bad = 0;
    for (int k = tid; k < n; k += QW_THREADS) {
        const int p = pi[k];
        const bool ok = p >= 0 && p < n;
        pi_l[k] = ok ? p : -1;
        bad |= !ok;
    }
    return bad;
}

// cost[b][i][j] = -sum_k A[i,k] B[pi(k),j] on the corner.  grid (ceil(N / 32), ceil(N / 128), B): a workgroup owns a 32 x 128 block of
// the cost matrix, wave w its 32 x 32 tile w.  Per chunk of 32 k: the A tile (32 x 32) and the GATHERED rows B[pi(k0 + k)][c0 .. c0 +
// 127] go to LDS (zero outside the corner / for an unmatched k), then 16 v_mfma_f32_32x32x2_f32 per wave walk k upwards: lane l feeds
// a = A[i0 + (l & 31)][k + (l >> 5)] (a column of the odd-pitch tile) and b = Bg[k + (l >> 5)][32 w + (l & 31)] (a row: contiguous).
__global__ __launch_bounds__(QW_THREADS) void qapw_improve_cost_kernel(const float *a1, const float *a2, long long gstride, int ld,
                                                                       const int *assign, const int *nvalid, int N, float *cost,
                                                                       long long bstride, int cld) {
    __shared__ float a_l[QW_ROWS * QW_PA];
    __shared__ float b_l[QW_KC * QW_COLS];
    __shared__ int pi_l[FGNN_QAPW_MAX_N];
    const int b = blockIdx.z, i0 = blockIdx.x * QW_ROWS, c0 = blockIdx.y * QW_COLS, tid = threadIdx.x;
    const int n = corner_of(nvalid, b, N);
    if (i0 >= n || c0 >= n) return;             // uniform
    const float *A = a1 + (long long)b * gstride, *Bm = a2 + (long long)b * gstride;
    stage_assign(pi_l, assign + (long long)b * N, n, tid);
    __syncthreads();
    const int wv = tid >> 6, lane = tid & 63, h = lane >> 5, c = lane & 31;
    const bool live = c0 + 32 * wv < n;         // wave-uniform: a wave whose tile lies outside the corner only helps staging
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int k0 = 0; k0 < n; k0 += QW_KC) {
        for (int idx = tid; idx < QW_ROWS * QW_KC; idx += QW_THREADS) {
            const int r = idx >> 5, k = idx & 31, gi = i0 + r, gk = k0 + k;
            a_l[r * QW_PA + k] = (gi < n && gk < n) ? A[(long long)gi * ld + gk] : 0.f;
        }
        for (int idx = tid; idx < QW_KC * QW_COLS; idx += QW_THREADS) {
            const int k = idx >> 7, j = idx & (QW_COLS - 1), gk = k0 + k, gj = c0 + j;
            const int p = gk < n ? pi_l[gk] : -1;
            b_l[idx] = (p >= 0 && gj < n) ? Bm[(long long)p * ld + gj] : 0.f;
        }
        __syncthreads();
        if (live) {
#pragma unroll
            for (int kk = 0; kk < QW_KC; kk += 2) acc = mfma32(a_l[c * QW_PA + kk + h], b_l[(kk + h) * QW_COLS + 32 * wv + c], acc);
        }
        __syncthreads();
    }
    const int gj = c0 + 32 * wv + c;
    if (!live || gj >= n) return;
    float *out = cost + (long long)b * bstride + gj;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int gi = i0 + ch_of(r, h);
        if (gi < n) out[(long long)gi * cld] = -acc[r];
    }
}

// One workgroup per pair.  Thread t takes the corner's elements t, t + 256, ... (row-major), one fmaf chain per output; the 64 chains of
// a wave are folded by a butterfly, the 4 waves by thread 0, always in the same order.
__global__ __launch_bounds__(QW_THREADS) void qapw_objective_kernel(const float *a1, const float *a2, long long gstride, int ld,
                                                                    const int *assign, const int *nvalid, int N, float *qap, float *trace,
                                                                    float *planted, float *na, float *nb) {
    __shared__ int pi_l[FGNN_QAPW_MAX_N];
    __shared__ float red[QW_THREADS / 64][5];
    __shared__ int bad_l[QW_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = corner_of(nvalid, b, N);
    const float *A = a1 + (long long)b * gstride, *Bm = a2 + (long long)b * gstride;
    const int bad = stage_assign(pi_l, assign + (long long)b * N, n, tid);
    const unsigned long long anybad = __ballot(bad);
    if ((tid & 63) == 0) bad_l[tid >> 6] = anybad != 0ull;
    __syncthreads();
    const bool want_q = qap != nullptr, want_t = trace != nullptr, want_sums = planted || na || nb;      // uniform
    float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};     // qap, trace, planted, na, nb
    for (int idx = tid; idx < n * n; idx += QW_THREADS) {
        const int i = idx / n, k = idx - i * n;
        const float a = A[(long long)i * ld + k];
        const int pi = pi_l[i], pk = pi_l[k];
        if (pi >= 0 && pk >= 0) {
            if (want_q) v[0] = fmaf(a, Bm[(long long)pi * ld + pk], v[0]);
            if (want_t) v[1] = fmaf(a, Bm[(long long)pk * ld + pi], v[1]);
        }
        if (want_sums) {
            const float bb = Bm[(long long)i * ld + k];
            v[2] = fmaf(a, bb, v[2]);
            v[3] += a;
            v[4] += bb;
        }
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        for (int o = 32; o > 0; o >>= 1) v[q] += __shfl_xor(v[q], o);
        if ((tid & 63) == 0) red[tid >> 6][q] = v[q];
    }
    __syncthreads();
    if (tid == 0) {
        float s[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) s[q] = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
        const bool holed = (bad_l[0] | bad_l[1] | bad_l[2] | bad_l[3]) != 0;
        if (qap) qap[b] = holed ? -1.f : s[0];
        if (trace) trace[b] = holed ? -1.f : s[1];
        if (planted) planted[b] = s[2];
        if (na) na[b] = s[3];
        if (nb) nb[b] = s[4];
    }
}

// The bookkeeping of greedy_qap, one wave per pair (the float twin of qap_keep_kernel).  round < 0: after the first improve() -- s_best
// = half the initial trace (it arrives in s_best as the trace), perm_best = the initial matching, acc_best = that improve()'s fixed
// points, t_best = 0.  round >= 0: keep the round's matching if its score is strictly better.  Halving is exact in fp32.
__global__ __launch_bounds__(64) void qapw_keep_kernel(int round, const float *cur_trace, const int *cur_correct, const int *cur_assign,
                                                       const int *nvalid, int N, float *s_best, int *acc_best, int *t_best, int *perm_best) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = corner_of(nvalid, b, N);
    const float s = round < 0 ? 0.5f * s_best[b] : 0.5f * cur_trace[b];
    const bool take = round < 0 || s > s_best[b];
    __syncthreads();
    if (!take) return;
    if (perm_best)
        for (int k = lane; k < N; k += 64) perm_best[(long long)b * N + k] = k < n ? cur_assign[(long long)b * N + k] : -1;
    if (lane == 0) {
        s_best[b] = s;
        acc_best[b] = cur_correct[b];
        t_best[b] = round < 0 ? 0 : round;
    }
}

int improve_cost(const float *a1, const float *a2, long long gstride, int ld, const int *assign, const int *nvalid, int B, int N,
                 float *cost, long long bstride, int cld, hipStream_t st) {
    hipLaunchKernelGGL(qapw_improve_cost_kernel, dim3((N + QW_ROWS - 1) / QW_ROWS, (N + QW_COLS - 1) / QW_COLS, B), dim3(QW_THREADS), 0, st,
                       a1, a2, gstride, ld, assign, nvalid, N, cost, bstride, cld);
    FGNN_LAUNCH_CHECK();
    return 0;
}
int objective(const float *a1, const float *a2, long long gstride, int ld, const int *assign, const int *nvalid, int B, int N, float *qap,
              float *trace, float *planted, float *na, float *nb, hipStream_t st) {
    hipLaunchKernelGGL(qapw_objective_kernel, dim3(B), dim3(QW_THREADS), 0, st, a1, a2, gstride, ld, assign, nvalid, N, qap, trace, planted,
                       na, nb);
    FGNN_LAUNCH_CHECK();
    return 0;
}

constexpr long long WS_ALIGN = 256;
constexpr int QW_MAX_B = 65535;            // pairs ride on a grid dimension
long long ws_round(long long x) { return (x + WS_ALIGN - 1) / WS_ALIGN * WS_ALIGN; }

}  // namespace

#define QAPW_CHECK_SHAPE(name)                                                                                                       \
    FGNN_CHECK(N <= FGNN_QAPW_MAX_N, name ": at most %d vertices per graph (got %d)", FGNN_QAPW_MAX_N, N);                            \
    FGNN_CHECK(B <= QW_MAX_B, name ": at most %d pairs per call (got %d)", QW_MAX_B, B);                                              \
    FGNN_CHECK(ld >= N && gstride >= (long long)N * ld, name ": ld / gstride smaller than the matrices")

extern "C" int fgnn_qapw_objective(const float *a1, const float *a2, long long gstride, int ld, const int *assign, const int *nvalid, int B,
                                   int N, float *qap, float *trace, float *planted, float *na, float *nb, void *stream) {
    FGNN_CHECK(a1 && a2 && assign && B > 0 && N > 0, "fgnn_qapw_objective: bad arguments");
    QAPW_CHECK_SHAPE("fgnn_qapw_objective");
    return objective(a1, a2, gstride, ld, assign, nvalid, B, N, qap, trace, planted, na, nb, (hipStream_t)stream);
}

extern "C" int fgnn_qapw_improve_cost(const float *a1, const float *a2, long long gstride, int ld, const int *assign, const int *nvalid,
                                      int B, int N, float *cost, long long bstride, int cost_ld, void *stream) {
    FGNN_CHECK(a1 && a2 && assign && cost && B > 0 && N > 0, "fgnn_qapw_improve_cost: bad arguments");
    QAPW_CHECK_SHAPE("fgnn_qapw_improve_cost");
    FGNN_CHECK(cost_ld >= N && bstride >= (long long)N * cost_ld, "fgnn_qapw_improve_cost: cost strides smaller than the matrices");
    return improve_cost(a1, a2, gstride, ld, assign, nvalid, B, N, cost, bstride, cost_ld, (hipStream_t)stream);
}

extern "C" long long fgnn_greedy_qapw_ws_bytes(int B, int N) {
    if (B <= 0 || N <= 0) return 0;
    return ws_round((long long)B * N * N * 4) + ws_round((long long)B * N * 4) + 2 * ws_round((long long)B * 4);
}

// fgnn_greedy_qapw (labels = NULL) and fgnn_greedy_qapw_labels: one launch sequence; with labels a fgnn_count_matches launch overwrites
// `correct` after every solver call (qap.hip)
static int greedy(const float *a1, const float *a2, long long gstride, int ld, const int *assign0, const int *labels, const int *nvalid,
                  int B, int N, int T, void *ws, long long ws_bytes, float *s_best, int *acc_best, int *t_best, int *perm_best,
                  void *stream) {
    FGNN_CHECK(a1 && a2 && assign0 && ws && s_best && acc_best && t_best && B > 0 && N > 0 && T >= 0, "fgnn_greedy_qapw: bad arguments");
    QAPW_CHECK_SHAPE("fgnn_greedy_qapw");
    FGNN_CHECK(ws_bytes >= fgnn_greedy_qapw_ws_bytes(B, N) && ((uintptr_t)ws & 15) == 0,
               "fgnn_greedy_qapw: the workspace needs %lld bytes, 16-byte aligned (got %lld)", fgnn_greedy_qapw_ws_bytes(B, N), ws_bytes);
    hipStream_t st = (hipStream_t)stream;
    char *p = (char *)ws;
    float *cost = (float *)p;
    p += ws_round((long long)B * N * N * 4);
    int *cur = (int *)p;
    p += ws_round((long long)B * N * 4);
    int *correct = (int *)p;
    p += ws_round((long long)B * 4);
    float *cur_trace = (float *)p;
    const long long bs = (long long)N * N;
    int rc;
    // s_best = score(pi0); pi = improve(pi0) -- never scored -- sets acc_best, T_best = 0
    if ((rc = objective(a1, a2, gstride, ld, assign0, nvalid, B, N, nullptr, s_best, nullptr, nullptr, nullptr, st))) return rc;
    if ((rc = improve_cost(a1, a2, gstride, ld, assign0, nvalid, B, N, cost, bs, N, st))) return rc;
    if ((rc = fgnn_lsap_accuracy(cost, bs, N, nvalid, B, N, correct, cur, stream))) return rc;
    if (labels && (rc = fgnn_count_matches(cur, labels, nvalid, B, N, correct, stream))) return rc;
    hipLaunchKernelGGL(qapw_keep_kernel, dim3(B), dim3(64), 0, st, -1, cur_trace, correct, assign0, nvalid, N, s_best, acc_best, t_best, perm_best);
    FGNN_LAUNCH_CHECK();
    for (int i = 0; i < T; ++i) {
        if ((rc = improve_cost(a1, a2, gstride, ld, cur, nvalid, B, N, cost, bs, N, st))) return rc;
        if ((rc = fgnn_lsap_accuracy(cost, bs, N, nvalid, B, N, correct, cur, stream))) return rc;
        if (labels && (rc = fgnn_count_matches(cur, labels, nvalid, B, N, correct, stream))) return rc;
        if ((rc = objective(a1, a2, gstride, ld, cur, nvalid, B, N, nullptr, cur_trace, nullptr, nullptr, nullptr, st))) return rc;
        hipLaunchKernelGGL(qapw_keep_kernel, dim3(B), dim3(64), 0, st, i, cur_trace, correct, cur, nvalid, N, s_best, acc_best, t_best, perm_best);
        FGNN_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int fgnn_greedy_qapw(const float *a1, const float *a2, long long gstride, int ld, const int *assign0, const int *nvalid, int B,
                                int N, int T, void *ws, long long ws_bytes, float *s_best, int *acc_best, int *t_best, int *perm_best,
                                void *stream) {
    return greedy(a1, a2, gstride, ld, assign0, nullptr, nvalid, B, N, T, ws, ws_bytes, s_best, acc_best, t_best, perm_best, stream);
}

extern "C" int fgnn_greedy_qapw_labels(const float *a1, const float *a2, long long gstride, int ld, const int *assign0, const int *labels,
                                       const int *nvalid, int B, int N, int T, void *ws, long long ws_bytes, float *s_best,
                                       int *acc_best, int *t_best, int *perm_best, void *stream) {
    FGNN_CHECK(labels, "fgnn_greedy_qapw_labels: NULL labels");
    return greedy(a1, a2, gstride, ld, assign0, labels, nvalid, B, N, T, ws, ws_bytes, s_best, acc_best, t_best, perm_best, stream);
}
