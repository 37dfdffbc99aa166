// Random restarts for the Frank-Wolfe chain (qap_faq.hip): R starts per pair from one launch, and the choice of the best of R
// results from another.
//
// fgnn_faq_restart_starts: one workgroup per (pair b, restart k) writes start b R + k of a (B R, N, N) fp32 buffer.  With n = n_b
// the side of the live corner, p = pair_index[b] (b without) and `base` the pair's own start (null: the barycenter J = 1 / n):
//
//     k = 0      the start is base's corner, copied bit for bit, or (float)(1.0 / n)
//     k >= 1     the start is (base + K_k) / 2, K_k = SciPy's _doubly_stochastic(U_k) -- its randomized P0 = (J + K) / 2 when base is J
//     U_k[i][j]  = ((u32 >> 8) + 1) 2^-24 in (0, 1], exact in fp32; u32 = raw draw t = (k << 32) | (i << 16) | j of pair stream
//                  FGNN_RESTART_STREAM of pair p (fgnn_philox.h): one Philox block gives the eight columns 8 g .. 8 g + 7 of a row
//
// _doubly_stochastic is linear-domain Sinkhorn-Knopp: c = 1 / colsum(U), r = 1 / (U c); if every row and column sum OF U ITSELF lies
// within 1e-3 of 1, K = U (SciPy's first test runs on the unscaled matrix; kept); else up to 1000 times c = 1 / (r U), r = 1 / (U c),
// stopping as soon as every row and column sum of r_i U_ij c_j lies within 1e-3 of 1; K_ij = (r_i U_ij) c_j.  Here the row sum of
// row i after an update is r_i (U c)_i and the column sum of column j is c_j (r U)_j, and that (r U) is the next update's input, so
// an update is one column pass and one row pass.  n = 1 is K = [[1]], the only doubly stochastic 1 x 1 matrix (SciPy's first test
// would let a u within 1e-3 of 1 through as it is).
//
// U lives in the output buffer (fp32, exact), r and c in LDS as fp64; every sum is fp64 in an order fixed by n alone: a column is
// summed by RS_T / roundup(n, 64) threads over ascending row slices folded in slice order, a row by one wave, lane l taking the
// columns l, l + 64, .. ascending, then an xor butterfly.  The start is rounded to fp32 once, from ((double)base + K) / 2.  So a
// start is a function of (seed, p, k, n, base's corner) only -- not of B, R or the padded N -- and bit-identical from run to run.
// Everything outside the corner is an exact zero; n = 0 writes zeros.  Nothing outside base's corner is read.
//
// fgnn_qap_best_of_i64 / _f32: one wave per pair picks, among the restarts whose status is not 2 (and whose veto, when given, is not
// 2), the largest objective -- a NaN never wins, ties go to the smallest k -- and copies that restart's perm row, objective, nit and
// status, plus its k; without a candidate restart 0 is copied as it is.
#include "fgnn_philox.h"
#include "fgnn_rows.h"

namespace {

constexpr int RS_T = 1024;                 // threads of a start's workgroup: 16 waves
constexpr int RS_MAX_N = FGNN_QAP_MAX_N;
constexpr int RS_ROUNDS = 1000;            // SciPy's max_iter
constexpr double RS_TOL = 1e-3;            // SciPy's tol

DEVI double wave_sum_f64(double v) {       // a + b == b + a bit for bit: every lane returns the same sum
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// s[j] = sum_i w[i] U[i][j] (w null: 1) for the columns j < n; thread tid is column c of row slice p.  Ends behind a barrier.
DEVI void column_sums(const float *U, int N, int n, const double *w, double *part, double *s, int tid) {
    const int cw = (n + 63) & ~63, parts = RS_T / cw, chunk = (n + parts - 1) / parts;
    const int c = tid % cw, p = tid / cw;
    if (p < parts) {
        double a = 0.0;
        if (c < n) {
            const int i0 = p * chunk, i1 = min(n, i0 + chunk);
            for (int i = i0; i < i1; ++i) a += (w ? w[i] : 1.0) * (double)U[(long long)i * N + c];
        }
        part[tid] = a;
    }
    __syncthreads();
    if (tid < n) {
        double a = 0.0;
        for (int q = 0; q < parts; ++q) a += part[q * cw + tid];
        s[tid] = a;
    }
    __syncthreads();
}

// t[i] = sum_j U[i][j] w[j] (w null: 1) for the rows i < n, a wave per row.  Ends behind a barrier.
DEVI void row_sums(const float *U, int N, int n, const double *w, double *t, int tid) {
    const int wv = tid >> 6, lane = tid & 63;
    for (int i = wv; i < n; i += RS_T / 64) {
        double a = 0.0;
        for (int j = lane; j < n; j += 64) a += (double)U[(long long)i * N + j] * (w ? w[j] : 1.0);
        a = wave_sum_f64(a);
        if (lane == 0) t[i] = a;
    }
    __syncthreads();
}

__global__ __launch_bounds__(RS_T) void restart_starts_kernel(const float *base, const int *nside, const long long *pair_index,
                                                              unsigned long long seed, int N, int R, float *out) {
    __shared__ double r_l[RS_MAX_N], c_l[RS_MAX_N], s_l[RS_MAX_N], t_l[RS_MAX_N];
    __shared__ double part[RS_T];
    const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int n = corner_of(nside, b, N);
    const float *Bb = base ? base + (long long)b * N * N : nullptr;
    float *U = out + ((long long)b * R + k) * N * N;
    const float bary = n > 0 ? (float)(1.0 / (double)n) : 0.f;

    if (k == 0 || n <= 1) {                 // the pair's own start; n = 1: K = [[1]]
        for (int idx = tid; idx < N * N; idx += RS_T) {
            const int i = idx / N, j = idx - i * N;
            float v = 0.f;
            if (i < n && j < n) {
                v = Bb ? Bb[idx] : bary;
                if (k > 0) v = (float)(((Bb ? (double)v : 1.0) + 1.0) / 2);
            }
            U[idx] = v;
        }
        return;
    }

    // U into the corner of the output: one Philox block per eight columns of a row
    const Pair pr{seed, (unsigned long long)(pair_index ? pair_index[b] : (long long)b)};
    const int g8 = (n + 7) >> 3;
    for (int idx = tid; idx < n * g8; idx += RS_T) {
        const int i = idx / g8, g = idx - i * g8;
        const P4 blk = pr.block(FGNN_RESTART_STREAM, ((unsigned long long)k << 29) | ((unsigned long long)i << 13) | (unsigned long long)g);
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            const int j = 8 * g + w;
            if (j < n) U[(long long)i * N + j] = (float)((word_of(blk, w) >> 8) + 1) * 0x1p-24f;
        }
    }
    __syncthreads();                        // (the corner is read back by other threads of this workgroup from here on)

    column_sums(U, N, n, nullptr, part, s_l, tid);          // s = colsum(U)
    row_sums(U, N, n, nullptr, t_l, tid);                   // t = rowsum(U)
    int ok = 1;
    if (tid < n) ok = fabs(s_l[tid] - 1.0) < RS_TOL && fabs(t_l[tid] - 1.0) < RS_TOL;
    const bool plain = __syncthreads_and(ok);               // SciPy's first test: on U itself
    if (!plain) {
        if (tid < n) c_l[tid] = 1.0 / s_l[tid];
        __syncthreads();
        row_sums(U, N, n, c_l, t_l, tid);
        if (tid < n) r_l[tid] = 1.0 / t_l[tid];
        __syncthreads();
        column_sums(U, N, n, r_l, part, s_l, tid);          // s = r U
        for (int round = 0; round < RS_ROUNDS; ++round) {
            if (tid < n) c_l[tid] = 1.0 / s_l[tid];
            __syncthreads();
            row_sums(U, N, n, c_l, t_l, tid);
            if (tid < n) r_l[tid] = 1.0 / t_l[tid];
            __syncthreads();
            column_sums(U, N, n, r_l, part, s_l, tid);
            ok = 1;
            if (tid < n) ok = fabs(r_l[tid] * t_l[tid] - 1.0) < RS_TOL && fabs(c_l[tid] * s_l[tid] - 1.0) < RS_TOL;
            if (__syncthreads_and(ok)) break;
        }
    }

    const double bary64 = 1.0 / (double)n;
    for (int idx = tid; idx < N * N; idx += RS_T) {
        const int i = idx / N, j = idx - i * N;
        float v = 0.f;
        if (i < n && j < n) {
            const double u = (double)U[idx];
            const double K = plain ? u : (r_l[i] * u) * c_l[j];
            v = (float)(((Bb ? (double)Bb[idx] : bary64) + K) / 2);
        }
        U[idx] = v;
    }
}

template <typename Q>
__global__ __launch_bounds__(64) void best_of_kernel(const Q *qap, const int *status, const int *veto, const int *nit, const int *perm,
                                                     int N, int R, int *perm_out, Q *qap_out, int *nit_out, int *status_out,
                                                     int *restart_out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const long long r0 = (long long)b * R;
    int win = -1;
    Q best = 0;
    for (int k = 0; k < R; ++k) {           // every lane walks the same R values: the choice is wave-uniform
        const Q q = qap[r0 + k];
        if (status[r0 + k] == 2 || (veto && veto[r0 + k] == 2) || !(q == q)) continue;
        if (win < 0 || q > best) {
            win = k;
            best = q;
        }
    }
    const int pick = win < 0 ? 0 : win;
    for (int i = lane; i < N; i += 64) perm_out[(long long)b * N + i] = perm[(r0 + pick) * N + i];
    if (lane == 0) {
        qap_out[b] = qap[r0 + pick];
        nit_out[b] = nit[r0 + pick];
        status_out[b] = status[r0 + pick];
        restart_out[b] = pick;
    }
}

template <typename Q>
int best_of(const char *who, const Q *qap, const int *status, const int *veto, const int *nit, const int *perm, int B, int N, int R,
            int *perm_out, Q *qap_out, int *nit_out, int *status_out, int *restart_out, void *stream) {
    FGNN_CHECK(qap && status && nit && perm && perm_out && qap_out && nit_out && status_out && restart_out && B > 0 && N > 0,
               "%s: bad arguments", who);
    FGNN_CHECK(R >= 1 && R <= FGNN_RESTART_MAX_R, "%s: 1 to %d restarts (got %d)", who, FGNN_RESTART_MAX_R, R);
    hipLaunchKernelGGL((best_of_kernel<Q>), dim3(B), dim3(64), 0, (hipStream_t)stream, qap, status, veto, nit, perm, N, R, perm_out,
                       qap_out, nit_out, status_out, restart_out);
    FGNN_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int fgnn_faq_restart_starts(const float *base, const int *n, const long long *pair_index, unsigned long long seed, int B,
                                       int N, int R, float *starts, void *stream) {
    FGNN_CHECK(starts && B > 0 && N > 0, "fgnn_faq_restart_starts: bad arguments");
    FGNN_CHECK(N <= RS_MAX_N, "fgnn_faq_restart_starts: at most %d vertices per graph (got %d)", RS_MAX_N, N);
    FGNN_CHECK(R >= 1 && R <= FGNN_RESTART_MAX_R, "fgnn_faq_restart_starts: 1 to %d restarts (got %d)", FGNN_RESTART_MAX_R, R);
    FGNN_CHECK((long long)B * R <= FGNN_RESTART_MAX_STARTS, "fgnn_faq_restart_starts: at most %d starts per call (got %lld)",
               FGNN_RESTART_MAX_STARTS, (long long)B * R);
    hipLaunchKernelGGL(restart_starts_kernel, dim3(R, B), dim3(RS_T), 0, (hipStream_t)stream, base, n, pair_index, seed, N, R, starts);
    FGNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int fgnn_qap_best_of_i64(const long long *qap, const int *status, const int *veto, const int *nit, const int *perm, int B,
                                    int N, int R, int *perm_out, long long *qap_out, int *nit_out, int *status_out, int *restart_out,
                                    void *stream) {
    return best_of<long long>("fgnn_qap_best_of_i64", qap, status, veto, nit, perm, B, N, R, perm_out, qap_out, nit_out, status_out,
                              restart_out, stream);
}

extern "C" int fgnn_qap_best_of_f32(const float *qap, const int *status, const int *veto, const int *nit, const int *perm, int B, int N,
                                    int R, int *perm_out, float *qap_out, int *nit_out, int *status_out, int *restart_out,
                                    void *stream) {
    return best_of<float>("fgnn_qap_best_of_f32", qap, status, veto, nit, perm, B, N, R, perm_out, qap_out, nit_out, status_out,
                          restart_out, stream);
}
