// GRAMPA (Fan, Mao, Wu, Xu, "Spectral graph matching and regularized quadratic relaxations"): the spectral similarity
//
//     X = sum_ij u_i u_i^T H v_j v_j^T / ((lambda_i - mu_j)^2 + eta^2),   A = U Lambda U^T,  B = V M V^T,  H = all ones (or rhs)
//
// without an eigendecomposition.  With T(X) = A X - X B and T^T(S) = A^T S - S B^T, X is the solution of the symmetric positive
// definite system (T^T T + eta^2 I) X = H -- the minimiser of 1/2 |AX - XB|^2 + eta^2 / 2 |X|^2 - <H, X> -- and conjugate gradient
// on it is, per round and pair, on the n_b x n_b corner,
//
//     S  = A P - P B                                grampa_t_kernel: two fmaf chains over ascending k, subtracted once
//     Q  = A^T S - S B^T + eta^2 P                  grampa_q_kernel: two chains, one subtraction, one fmaf with eta^2;
//                                                   its epilogue leaves the block's part of <P, Q> as an fp64 value in its slot
//     pq = the slots in slot order;  alpha = (float)(rr / pq);  R -= alpha Q;  rn = <R, R>;  res = sqrt(rn / r0)
//     res < tol: X += alpha P, the pair stops (status 0);  else X += alpha P, P = R + (float)(rn / rr) P, rr = rn     grampa_step_kernel
//
// from X = 0, R = P = H, r0 = rr = <H, H>.  No problem of this family needs the right-hand side again, so H is read once.
// Matrices: fp32, row pitch ld, pairs gstride floats apart; only the corner is ever READ (it may be surrounded by NaN), in a1, a2
// and rhs alike.  The products run on v_mfma_f32_32x32x2_f32 (every entry one fp32 fmaf chain, k ascending); every sum is fp64 in a
// fixed order that depends on n_b alone (no float atomics); every division and root is fp64 (IEEE), rounded once to fp32 where the
// result is an fp32 coefficient: results are bit-identical from run to run under any flags, and a pair's bits do not depend on B or
// on the pairs around it.  The state (X, R, P, S, Q; rr, r0) lives in the workspace with row pitch N.
#include "fgnn_rows.h"

namespace {

constexpr int GR_THREADS = 256;            // 4 waves
constexpr int GR_ROWS = 32;                // rows of the output per workgroup (one MFMA tile)
constexpr int GR_COLS = 128;               // columns per workgroup: wave w owns columns 32 w .. 32 w + 31 of them
constexpr int GR_KC = 32;                  // k per staged chunk
constexpr int GR_PA = GR_KC + 1;           // pitch of the left tile: lanes read it down a column, a transposed operand is written
constexpr int GR_PB = GR_COLS + 1;         // down one -- and of the right tile, which a transposed operand fills down a column
constexpr int GR_MAX_N = FGNN_QAPW_MAX_N;  // as the FAQ chain
constexpr int GR_MAX_B = 65535;            // pairs ride on a grid dimension
constexpr int GR_MAX_ITER = 1024;

// acc += X Y over k < n for the 32 x 128 block at (i0, c0), wave w its 32 x 32 tile w: the tile loop of qap_faq.hip, restated.
// X(i, k) = XT ? X[k ldx + i] : X[i ldx + k], Y(k, j) = YT ? Y[j ldy + k] : Y[k ldy + j].  Staging walks the contiguous index of the
// source fastest, so global reads coalesce both ways; the odd pitches keep the strided LDS writes of a transposed operand off a
// common bank.  Zero outside the corner: nothing beyond it is read.  k ascends: every output is one fmaf chain over k = 0 .. n - 1.
template <bool XT, bool YT>
DEVI void tile_product(f32x16 &acc, float *a_l, float *b_l, const float *X, int ldx, const float *Y, int ldy, int n, int i0, int c0,
                       int tid, bool live) {
    const int wv = tid >> 6, lane = tid & 63, h = lane >> 5, c = lane & 31;
    for (int k0 = 0; k0 < n; k0 += GR_KC) {
        for (int idx = tid; idx < GR_ROWS * GR_KC; idx += GR_THREADS) {
            const int hi = idx >> 5, lo = idx & 31;
            const int r = XT ? lo : hi, k = XT ? hi : lo, gi = i0 + r, gk = k0 + k;
            float x = 0.f;
            if (gi < n && gk < n) x = XT ? X[(long long)gk * ldx + gi] : X[(long long)gi * ldx + gk];
            a_l[r * GR_PA + k] = x;
        }
        for (int idx = tid; idx < GR_KC * GR_COLS; idx += GR_THREADS) {
            const int k = YT ? (idx & 31) : (idx >> 7), j = YT ? (idx >> 5) : (idx & (GR_COLS - 1)), gk = k0 + k, gj = c0 + j;
            float y = 0.f;
            if (gk < n && gj < n) y = YT ? Y[(long long)gj * ldy + gk] : Y[(long long)gk * ldy + gj];
            b_l[k * GR_PB + j] = y;
        }
        __syncthreads();
        if (live) {
#pragma unroll
            for (int kk = 0; kk < GR_KC; kk += 2) acc = mfma32(a_l[c * GR_PA + kk + h], b_l[(kk + h) * GR_PB + 32 * wv + c], acc);
        }
        __syncthreads();
    }
}

// the sum of v over the workgroup in every thread: butterfly inside a wave, the 4 waves folded in one order
DEVI double block_sum(double v, double *red, int tid) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    const double s = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return s;
}

DEVI bool finite64(double v) { return v - v == 0.0; }

// The optional prologue, a workgroup per (pair, side): W[b] = the standardised corner of side `blockIdx.y`, (w - m) / (sqrt(n_b) sd)
// off the diagonal and 0 on it, with m and sd the mean and the (population) standard deviation of the n_b (n_b - 1) off-diagonal
// corner entries -- the paper's (A - p) / sqrt(n p (1 - p)) for a 0/1 graph with the empirical p.  Thread t takes the corner's
// elements t, t + 256, ... (row-major) in every pass; the sums are fp64, the quotient is fp64 and rounded once.  flat[2 b + side] = 1
// where sd is not a finite number greater than 0 (an empty or complete graph, n_b < 2): the start freezes such a pair, status 2.
__global__ __launch_bounds__(GR_THREADS) void grampa_standardize_kernel(const float *a1, const float *a2, long long gstride, int ld,
                                                                        const int *nvalid, int N, float *W, int *flat) {
    __shared__ double red[GR_THREADS / 64];
    const int b = blockIdx.x, side = blockIdx.y, tid = threadIdx.x, B = gridDim.x;
    const int n = corner_of(nvalid, b, N);
    const float *A = (side ? a2 : a1) + (long long)b * gstride;
    float *Wb = W + ((long long)side * B + b) * N * N;
    const double cnt = (double)n * (double)(n - 1);
    double s = 0.0;
    for (int idx = tid; idx < n * n; idx += GR_THREADS) {
        const int i = idx / n, j = idx - i * n;
        if (i != j) s += (double)A[(long long)i * ld + j];
    }
    const double m = block_sum(s, red, tid) / cnt;
    double ss = 0.0;
    for (int idx = tid; idx < n * n; idx += GR_THREADS) {
        const int i = idx / n, j = idx - i * n;
        if (i != j) {
            const double d = (double)A[(long long)i * ld + j] - m;
            ss += d * d;
        }
    }
    const double sd = sqrt(block_sum(ss, red, tid) / cnt);
    const bool ok = n > 1 && finite64(sd) && sd > 0.0;
    const double den = sqrt((double)n) * sd;
    for (int idx = tid; idx < n * n; idx += GR_THREADS) {
        const int i = idx / n, j = idx - i * n;
        Wb[(long long)i * N + j] = (ok && i != j) ? (float)(((double)A[(long long)i * ld + j] - m) / den) : 0.f;
    }
    if (tid == 0) flat[2 * b + side] = !ok;
}

// One workgroup per pair: the start.  X = 0 on the whole matrix, R = P = H on the corner (rhs's corner, or all ones), r0 = rr =
// <H, H>; status 1 (it becomes 0 when the pair meets tol), or 2 with the done flag set where n_b = 0, r0 = 0 or a side is flat.
__global__ __launch_bounds__(GR_THREADS) void grampa_init_kernel(const float *rhs, const int *nvalid, const int *flat, int N, float *X,
                                                                 float *R, float *P, double *rr, double *r0, int *nvc, int *done,
                                                                 int *nit, float *res, int *status) {
    __shared__ double red[GR_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = corner_of(nvalid, b, N);
    const long long o = (long long)b * N * N;
    for (int idx = tid; idx < N * N; idx += GR_THREADS) X[o + idx] = 0.f;
    double s = 0.0;
    for (int idx = tid; idx < n * n; idx += GR_THREADS) {
        const int i = idx / n, j = idx - i * n;
        const float h = rhs ? rhs[o + (long long)i * N + j] : 1.f;
        R[o + (long long)i * N + j] = h;
        P[o + (long long)i * N + j] = h;
        s += (double)h * (double)h;
    }
    s = block_sum(s, red, tid);
    if (tid == 0) {
        const int frozen = n == 0 || s == 0.0 || (flat && (flat[2 * b] || flat[2 * b + 1]));
        rr[b] = s;
        r0[b] = s;
        nvc[b] = n;
        done[b] = frozen;
        nit[b] = 0;
        res[b] = frozen ? 0.f : 1.f;
        status[b] = frozen ? 2 : 1;
    }
}

// S[b] = A P - P B on the corner.  grid (ceil(N / 32), ceil(N / 128), B).  A pair whose done flag is set is left at once.
__global__ __launch_bounds__(GR_THREADS) void grampa_t_kernel(const float *a1, const float *a2, long long gstride, int ld, const float *P,
                                                              const int *nvc, const int *done, int N, float *S) {
    __shared__ float a_l[GR_ROWS * GR_PA];
    __shared__ float b_l[GR_KC * GR_PB];
    const int b = blockIdx.z, i0 = blockIdx.x * GR_ROWS, c0 = blockIdx.y * GR_COLS, tid = threadIdx.x;
    if (done[b]) return;                        // uniform
    const int n = nvc[b];
    if (i0 >= n || c0 >= n) return;             // uniform
    const float *A = a1 + (long long)b * gstride, *Bm = a2 + (long long)b * gstride, *Pb = P + (long long)b * N * N;
    const int wv = tid >> 6, lane = tid & 63, h = lane >> 5, c = lane & 31;
    const bool live = c0 + 32 * wv < n;         // wave-uniform: a wave whose tile lies outside the corner only helps staging
    f32x16 ap, pb;
#pragma unroll
    for (int r = 0; r < 16; ++r) ap[r] = 0.f, pb[r] = 0.f;
    tile_product<false, false>(ap, a_l, b_l, A, ld, Pb, N, n, i0, c0, tid, live);
    tile_product<false, false>(pb, a_l, b_l, Pb, N, Bm, ld, n, i0, c0, tid, live);
    const int gj = c0 + 32 * wv + c;
    if (!live || gj >= n) return;
    float *out = S + (long long)b * N * N + gj;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int gi = i0 + ch_of(r, h);
        if (gi < n) out[(long long)gi * N] = ap[r] - pb[r];
    }
}

// Q[b] = A^T S - S B^T + eta^2 P on the corner, same grid; part[b][blockIdx.y gridDim.x + blockIdx.x] = the block's sum of P Q in
// fp64: a lane adds its 16 entries in register order, a butterfly folds the wave, the 4 waves fold in one order.
__global__ __launch_bounds__(GR_THREADS) void grampa_q_kernel(const float *a1, const float *a2, long long gstride, int ld, const float *S,
                                                              const float *P, float eta2, const int *nvc, const int *done, int N,
                                                              float *Q, double *part) {
    __shared__ float a_l[GR_ROWS * GR_PA];
    __shared__ float b_l[GR_KC * GR_PB];
    __shared__ double red[GR_THREADS / 64];
    const int b = blockIdx.z, i0 = blockIdx.x * GR_ROWS, c0 = blockIdx.y * GR_COLS, tid = threadIdx.x;
    if (done[b]) return;                        // uniform
    const int n = nvc[b];
    if (i0 >= n || c0 >= n) return;             // uniform
    const float *A = a1 + (long long)b * gstride, *Bm = a2 + (long long)b * gstride, *Sb = S + (long long)b * N * N;
    const int wv = tid >> 6, lane = tid & 63, h = lane >> 5, c = lane & 31;
    const bool live = c0 + 32 * wv < n;
    f32x16 as, sb;
#pragma unroll
    for (int r = 0; r < 16; ++r) as[r] = 0.f, sb[r] = 0.f;
    tile_product<true, false>(as, a_l, b_l, A, ld, Sb, N, n, i0, c0, tid, live);
    tile_product<false, true>(sb, a_l, b_l, Sb, N, Bm, ld, n, i0, c0, tid, live);
    const int gj = c0 + 32 * wv + c;
    double pq = 0.0;
    if (live && gj < n) {
        const long long o = (long long)b * N * N + gj;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int gi = i0 + ch_of(r, h);
            if (gi < n) {
                const float p = P[o + (long long)gi * N];
                const float q = fmaf(eta2, p, as[r] - sb[r]);
                Q[o + (long long)gi * N] = q;
                pq += (double)p * (double)q;
            }
        }
    }
    pq = block_sum(pq, red, tid);
    if (tid == 0) part[((long long)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = pq;
}

// One workgroup per pair: the update and the stop test of one round.  Thread t takes the corner's elements t, t + 256, ...
// (row-major) in both passes.  Pass 1: R -= alpha Q and rn = <R, R>;  pass 2, only once rn is known to be a finite number: X += alpha P
// and, unless the pair stops, P = R + beta P.  Breakdown -- pq not a finite number greater than 0, or rn not finite (an inf or a
// NaN in a corner) -- freezes the pair with status 3 before X is touched: X stays the last iterate.
__global__ __launch_bounds__(GR_THREADS) void grampa_step_kernel(const float *Q, const double *part, int slots_x, int slots_y,
                                                                 const int *nvc, int N, float tol, float *X, float *R, float *P,
                                                                 double *rr, const double *r0, int *done, int *nit, float *res,
                                                                 int *status) {
    __shared__ double red[GR_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (done[b]) return;                        // uniform: a frozen pair keeps its X, nit, res and status
    const int n = nvc[b];
    const long long o = (long long)b * N * N;
    double pq = 0.0;                            // the slots of the blocks that meet the corner, in slot order
    for (int y = 0; y < slots_y && y * GR_COLS < n; ++y)
        for (int x = 0; x < slots_x && x * GR_ROWS < n; ++x) pq += part[((long long)b * slots_y + y) * slots_x + x];
    const double rr_b = rr[b];
    if (!(finite64(pq) && pq > 0.0)) {          // uniform
        if (tid == 0) {
            done[b] = 1;
            status[b] = 3;
        }
        return;
    }
    const float alpha = (float)(rr_b / pq);
    double rn = 0.0;
    for (int idx = tid; idx < n * n; idx += GR_THREADS) {
        const int i = idx / n, j = idx - i * n;
        const long long at = o + (long long)i * N + j;
        const float r = fmaf(-alpha, Q[at], R[at]);
        R[at] = r;
        rn += (double)r * (double)r;
    }
    rn = block_sum(rn, red, tid);
    if (!finite64(rn)) {                        // uniform
        if (tid == 0) {
            done[b] = 1;
            status[b] = 3;
        }
        return;
    }
    const double rs = sqrt(rn / r0[b]);
    const bool stop = rs < (double)tol;
    const float beta = (float)(rn / rr_b);
    for (int idx = tid; idx < n * n; idx += GR_THREADS) {
        const int i = idx / n, j = idx - i * n;
        const long long at = o + (long long)i * N + j;
        const float p = P[at];
        X[at] = fmaf(alpha, p, X[at]);
        if (!stop) P[at] = fmaf(beta, p, R[at]);
    }
    if (tid == 0) {
        nit[b] += 1;
        res[b] = (float)rs;
        rr[b] = rn;
        if (stop) {
            done[b] = 1;
            status[b] = 0;
        }
    }
}

// cost[b] = -X on the corner, for the assignment.  grid (N, B): a workgroup per row.
__global__ __launch_bounds__(64) void grampa_neg_x_kernel(const float *X, const int *nvc, int N, float *cost) {
    const int i = blockIdx.x, b = blockIdx.y, n = nvc[b];
    if (i >= n) return;
    const long long row = ((long long)b * N + i) * N;
    for (int j = threadIdx.x; j < n; j += 64) cost[row + j] = -X[row + j];
}

// One workgroup per pair: the outputs.  perm arrives from the solver (-1 everywhere if it found no assignment: status 2 then);
// a status-2 pair gets perm = -1 and nit = 0; -1 past the corner; x_out = X on the corner, exact zeros around it.
__global__ __launch_bounds__(GR_THREADS) void grampa_finish_kernel(const float *X, const int *nvc, int N, int *perm, int *nit, int *status,
                                                                   float *x_out) {
    const int b = blockIdx.x, tid = threadIdx.x, n = nvc[b];
    int bad = 0;
    for (int k = tid; k < n; k += GR_THREADS) {
        const int p = perm[(long long)b * N + k];
        bad |= p < 0 || p >= n;
    }
    bad = __syncthreads_or(bad);
    const bool failed = status[b] == 2 || bad || n == 0;
    for (int k = tid; k < N; k += GR_THREADS)
        if (k >= n || failed) perm[(long long)b * N + k] = -1;
    for (int idx = tid; idx < N * N; idx += GR_THREADS) {
        const int i = idx / N, j = idx - i * N;
        x_out[(long long)b * N * N + idx] = (i < n && j < n) ? X[(long long)b * N * N + idx] : 0.f;
    }
    __syncthreads();                             // every thread has read status[b]
    if (tid == 0 && failed) {
        status[b] = 2;
        nit[b] = 0;
    }
}

constexpr long long WS_ALIGN = 256;
long long ws_round(long long x) { return (x + WS_ALIGN - 1) / WS_ALIGN * WS_ALIGN; }

struct GrampaWs {
    float *X, *R, *P, *S, *Q, *cost, *W;        // the state, the two products, -X, the standardised copies (2 B matrices)
    double *part, *rr, *r0;                     // a slot per block, <R, R>, <H, H>
    int *nvc, *done, *correct, *flat;
    long long bytes;
};

// (ws may be NULL: only `bytes` is then of use)
GrampaWs grampa_carve(void *ws, int B, int N) {
    const long long mat = ws_round((long long)B * N * N * 4), vec = ws_round((long long)B * 8);
    const long long slots = (long long)((N + GR_ROWS - 1) / GR_ROWS) * ((N + GR_COLS - 1) / GR_COLS);
    uintptr_t p = (uintptr_t)ws;
    const auto take = [&p](long long bytes) {
        const uintptr_t at = p;
        p += bytes;
        return at;
    };
    GrampaWs w = {};
    w.X = (float *)take(mat), w.R = (float *)take(mat), w.P = (float *)take(mat), w.S = (float *)take(mat), w.Q = (float *)take(mat);
    w.cost = (float *)take(mat), w.W = (float *)take(2 * mat);
    w.part = (double *)take(ws_round((long long)B * slots * 8)), w.rr = (double *)take(vec), w.r0 = (double *)take(vec);
    w.nvc = (int *)take(vec), w.done = (int *)take(vec), w.correct = (int *)take(vec), w.flat = (int *)take(vec);
    w.bytes = (long long)(p - (uintptr_t)ws);
    return w;
}

}  // namespace

extern "C" long long fgnn_grampa_ws_bytes(int B, int N) { return B <= 0 || N <= 0 ? 0 : grampa_carve(nullptr, B, N).bytes; }

extern "C" int fgnn_grampa(const float *a1, const float *a2, long long gstride, int ld, const float *rhs, const int *nvalid, int B, int N,
                           float eta, int maxiter, float tol, int standardize, void *ws, float *X, int *perm, int *nit, float *res,
                           int *status, void *stream) {
    FGNN_CHECK(a1 && a2 && ws && X && perm && nit && res && status && B > 0 && N > 0, "fgnn_grampa: bad arguments");
    FGNN_CHECK(N <= GR_MAX_N, "fgnn_grampa: at most %d vertices per graph (got %d)", GR_MAX_N, N);
    FGNN_CHECK(B <= GR_MAX_B, "fgnn_grampa: at most %d pairs per call (got %d)", GR_MAX_B, B);
    FGNN_CHECK(maxiter >= 1 && maxiter <= GR_MAX_ITER, "fgnn_grampa: maxiter must be in [1, %d] (got %d)", GR_MAX_ITER, maxiter);
    FGNN_CHECK(eta > 0.f && eta - eta == 0.f && tol > 0.f && tol - tol == 0.f, "fgnn_grampa: eta and tol must be positive and finite (got %g, %g)",
               (double)eta, (double)tol);
    FGNN_CHECK(ld >= N && gstride >= (long long)N * ld, "fgnn_grampa: ld / gstride smaller than the matrices");
    FGNN_CHECK(((uintptr_t)ws & 15) == 0, "fgnn_grampa: the workspace (fgnn_grampa_ws_bytes bytes) must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const GrampaWs w = grampa_carve(ws, B, N);
    const long long bs = (long long)N * N;
    const dim3 tiles((N + GR_ROWS - 1) / GR_ROWS, (N + GR_COLS - 1) / GR_COLS, B);
    const float eta2 = (float)((double)eta * (double)eta);
    const float *A = a1, *Bm = a2;
    long long gs = gstride;
    int pitch = ld, rc;
    if (standardize) {
        hipLaunchKernelGGL(grampa_standardize_kernel, dim3(B, 2), dim3(GR_THREADS), 0, st, a1, a2, gstride, ld, nvalid, N, w.W, w.flat);
        FGNN_LAUNCH_CHECK();
        A = w.W, Bm = w.W + (long long)B * bs, gs = bs, pitch = N;
    }
    hipLaunchKernelGGL(grampa_init_kernel, dim3(B), dim3(GR_THREADS), 0, st, rhs, nvalid, standardize ? w.flat : nullptr, N, w.X, w.R, w.P,
                       w.rr, w.r0, w.nvc, w.done, nit, res, status);
    FGNN_LAUNCH_CHECK();
    for (int it = 0; it < maxiter; ++it) {
        hipLaunchKernelGGL(grampa_t_kernel, tiles, dim3(GR_THREADS), 0, st, A, Bm, gs, pitch, w.P, w.nvc, w.done, N, w.S);
        FGNN_LAUNCH_CHECK();
        hipLaunchKernelGGL(grampa_q_kernel, tiles, dim3(GR_THREADS), 0, st, A, Bm, gs, pitch, w.S, w.P, eta2, w.nvc, w.done, N, w.Q, w.part);
        FGNN_LAUNCH_CHECK();
        hipLaunchKernelGGL(grampa_step_kernel, dim3(B), dim3(GR_THREADS), 0, st, w.Q, w.part, (int)tiles.x, (int)tiles.y, w.nvc, N, tol, w.X,
                           w.R, w.P, w.rr, w.r0, w.done, nit, res, status);
        FGNN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(grampa_neg_x_kernel, dim3(N, B), dim3(64), 0, st, w.X, w.nvc, N, w.cost);
    FGNN_LAUNCH_CHECK();
    if ((rc = fgnn_lsap_accuracy(w.cost, bs, N, w.nvc, B, N, w.correct, perm, stream))) return rc;
    hipLaunchKernelGGL(grampa_finish_kernel, dim3(B), dim3(GR_THREADS), 0, st, w.X, w.nvc, N, perm, nit, status, X);
    FGNN_LAUNCH_CHECK();
    return 0;
}
