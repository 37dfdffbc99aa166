// Fast Approximate QAP (FAQ; Vogelstein et al., PLOS ONE 10(4), 2015) on real-weighted pairs: Frank-Wolfe on the relaxed objective
// f(P) = tr(A^T P B P^T) over the doubly stochastic matrices, the algorithm of scipy.optimize.quadratic_assignment(method='faq',
// options={'maximize': True}) without seeds and without shuffling.  Per pair, on the n_b x n_b corner, one round is
//
//     G  = A P B^T + A^T P B                      two chained fp32 products on the matrix cores, fresh from P in every round
//     q  = argmax_Q <G, Q>                        the solver of fgnn_lsap_accuracy on cost = -G
//     R  = P - Q;  f(Q + x R) = f(Q) + b x + a x^2, from <G, P> = 2 f(P), <G, R> = b + 2 a, f(P) - f(Q) = a + b:
//          a = <G, P> / 2 - <G, Q> + f(Q),  b = <G, Q> - 2 f(Q)          fp64 sums in a fixed order over the fp32 G
//     x  = -b / (2 a) if a < 0 and 0 <= -b / (2 a) <= 1, else 1 if -(a + b) < 0, else 0
//     P' = x P + (1 - x) Q;  the pair stops when ||P - P'||_F / sqrt(n_b) < tol
//
// and the matching is the assignment that maximises the last P.  Matrices: fp32, row pitch ld, pairs gstride floats apart; only
// the corner is ever READ (it may be surrounded by NaN), in a1, a2 and p0 alike.  Every reduction has a fixed order (no float
// atomics): results are bit-identical from run to run, and a pair's bits do not depend on the batch it sits in.
//
// Seeds (fgnn_qapw_faq_seeded, further down) are the same chain on the free block: one faq_chain() issues the launches of both
// entry points on one workspace layout (FaqWs), and the two kernels that know the seeds' constant term C, faq_grad_kernel and
// faq_step_kernel, are templates on SEEDED -- one body each, the reads of C and the sums over it under `if constexpr`, so the
// unseeded instantiations do exactly the work written above.
#include "fgnn_rows.h"

namespace {

constexpr int FQ_THREADS = 256;            // 4 waves
constexpr int FQ_ROWS = 32;                // rows of the output per workgroup (one MFMA tile)
constexpr int FQ_COLS = 128;               // columns per workgroup: wave w owns columns 32 w .. 32 w + 31 of them
constexpr int FQ_KC = 32;                  // k per staged chunk
constexpr int FQ_PA = FQ_KC + 1;           // pitch of the left tile: lanes read it down a column, a transposed operand is written
constexpr int FQ_PB = FQ_COLS + 1;         // down one -- and of the right tile, which a transposed operand fills down a column
constexpr int FQ_MAX_B = 65535;            // pairs ride on a grid dimension

// acc += X Y over k < n for the 32 x 128 block at (i0, c0), wave w its 32 x 32 tile w: the tile loop of qapw_improve_cost_kernel
// (qap_weighted.hip) without the gather and with either operand read transposed.  X(i, k) = XT ? X[k ldx + i] : X[i ldx + k],
// Y(k, j) = YT ? Y[j ldy + k] : Y[k ldy + j].  Staging walks the contiguous index of the source fastest, so global reads
// coalesce both ways; the odd pitches keep the strided LDS writes of a transposed operand off a common bank.  Zero outside the
// corner: nothing beyond it is read.  k ascends: every output is one fmaf chain over k = 0 .. n - 1.
template <bool XT, bool YT>
DEVI void tile_product(f32x16 &acc, float *a_l, float *b_l, const float *X, int ldx, const float *Y, int ldy, int n, int i0, int c0,
                       int tid, bool live) {
    const int wv = tid >> 6, lane = tid & 63, h = lane >> 5, c = lane & 31;
    for (int k0 = 0; k0 < n; k0 += FQ_KC) {
        for (int idx = tid; idx < FQ_ROWS * FQ_KC; idx += FQ_THREADS) {
            const int hi = idx >> 5, lo = idx & 31;
            const int r = XT ? lo : hi, k = XT ? hi : lo, gi = i0 + r, gk = k0 + k;
            float x = 0.f;
            if (gi < n && gk < n) x = XT ? X[(long long)gk * ldx + gi] : X[(long long)gi * ldx + gk];
            a_l[r * FQ_PA + k] = x;
        }
        for (int idx = tid; idx < FQ_KC * FQ_COLS; idx += FQ_THREADS) {
            const int k = YT ? (idx & 31) : (idx >> 7), j = YT ? (idx >> 5) : (idx & (FQ_COLS - 1)), gk = k0 + k, gj = c0 + j;
            float y = 0.f;
            if (gk < n && gj < n) y = YT ? Y[(long long)gj * ldy + gk] : Y[(long long)gk * ldy + gj];
            b_l[k * FQ_PB + j] = y;
        }
        __syncthreads();
        if (live) {
#pragma unroll
            for (int kk = 0; kk < FQ_KC; kk += 2) acc = mfma32(a_l[c * FQ_PA + kk + h], b_l[(kk + h) * FQ_PB + 32 * wv + c], acc);
        }
        __syncthreads();
    }
}

// T[b][0] = P B^T, T[b][1] = P B on the corner.  grid (ceil(N / 32), 2 ceil(N / 128), B): the upper half of blockIdx.y is T[.][1].
// P and T live in the workspace with row pitch N.  A pair whose done flag is set is left at once.
__global__ __launch_bounds__(FQ_THREADS) void faq_pb_kernel(const float *a2, long long gstride, int ld, const float *P, const int *nvc,
                                                            const int *done, int N, float *T) {
    __shared__ float a_l[FQ_ROWS * FQ_PA];
    __shared__ float b_l[FQ_KC * FQ_PB];
    const int b = blockIdx.z, ny = gridDim.y >> 1, which = blockIdx.y >= ny ? 1 : 0, tid = threadIdx.x;
    const int i0 = blockIdx.x * FQ_ROWS, c0 = (blockIdx.y - which * ny) * FQ_COLS;
    if (done[b]) return;                        // uniform
    const int n = nvc[b];
    if (i0 >= n || c0 >= n) return;             // uniform
    const float *Bm = a2 + (long long)b * gstride, *Pb = P + (long long)b * N * N;
    const int wv = tid >> 6, lane = tid & 63, h = lane >> 5, c = lane & 31;
    const bool live = c0 + 32 * wv < n;         // wave-uniform: a wave whose tile lies outside the corner only helps staging
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    if (which) tile_product<false, false>(acc, a_l, b_l, Pb, N, Bm, ld, n, i0, c0, tid, live);
    else tile_product<false, true>(acc, a_l, b_l, Pb, N, Bm, ld, n, i0, c0, tid, live);
    const int gj = c0 + 32 * wv + c;
    if (!live || gj >= n) return;
    float *out = T + ((long long)b * 2 + which) * N * N + gj;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int gi = i0 + ch_of(r, h);
        if (gi < n) out[(long long)gi * N] = acc[r];
    }
}

// cost[b] = -G = -([A | A^T] [T0; T1]) on the corner, in the layout the solver reads (row pitch N, pairs N N apart): one fmaf chain
// per entry, the n terms of A T0 (k ascending) and then the n terms of A^T T1.  grid (ceil(N / 32), ceil(N / 128), B).
// SEEDED: cost = -(chain + C), the seeds' constant term added once, in the epilogue, to the finished chain; else C is not read.
template <bool SEEDED>
__global__ __launch_bounds__(FQ_THREADS) void faq_grad_kernel(const float *a1, long long gstride, int ld, const float *T, const float *C,
                                                              const int *nvc, const int *done, int N, float *cost) {
    __shared__ float a_l[FQ_ROWS * FQ_PA];
    __shared__ float b_l[FQ_KC * FQ_PB];
    const int b = blockIdx.z, i0 = blockIdx.x * FQ_ROWS, c0 = blockIdx.y * FQ_COLS, tid = threadIdx.x;
    if (done[b]) return;                        // uniform
    const int n = nvc[b];
    if (i0 >= n || c0 >= n) return;             // uniform
    const float *A = a1 + (long long)b * gstride, *T0 = T + (long long)b * 2 * N * N, *T1 = T0 + (long long)N * N;
    const int wv = tid >> 6, lane = tid & 63, h = lane >> 5, c = lane & 31;
    const bool live = c0 + 32 * wv < n;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    tile_product<false, false>(acc, a_l, b_l, A, ld, T0, N, n, i0, c0, tid, live);
    tile_product<true, false>(acc, a_l, b_l, A, ld, T1, N, n, i0, c0, tid, live);
    const int gj = c0 + 32 * wv + c;
    if (!live || gj >= n) return;
    float *out = cost + (long long)b * N * N + gj;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int gi = i0 + ch_of(r, h);
        if (gi >= n) continue;
        if constexpr (SEEDED) out[(long long)gi * N] = -(acc[r] + C[(long long)b * N * N + gj + (long long)gi * N]);
        else out[(long long)gi * N] = -acc[r];
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

// One workgroup per pair: the start.  P = p0's corner, the permutation matrix of assign0, or the barycenter (every entry 1 / n_b);
// status 1 (it becomes 0 when the pair meets tol), or 2 with the done flag set where n_b = 0 or assign0 is no permutation of
// [0, n_b) (P is then zero).  nvc = the clamped n_b, nvw = the solver's working copy: 0 for a frozen pair.
__global__ __launch_bounds__(FQ_THREADS) void faq_init_kernel(const float *p0, const int *assign0, const int *nvalid, int N, float *P,
                                                              int *nvc, int *nvw, int *done, int *nit, int *status) {
    __shared__ int seen[FGNN_QAPW_MAX_N];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = corner_of(nvalid, b, N);
    int bad = 0;
    if (assign0) {
        for (int k = tid; k < n; k += FQ_THREADS) seen[k] = 0;
        __syncthreads();
        for (int k = tid; k < n; k += FQ_THREADS) {
            const int p = assign0[(long long)b * N + k];
            if (p >= 0 && p < n) atomicAdd(&seen[p], 1);
            else bad = 1;
        }
        __syncthreads();
        for (int k = tid; k < n; k += FQ_THREADS) bad |= seen[k] != 1;
    }
    bad = __syncthreads_or(bad);
    float *Pb = P + (long long)b * N * N;
    const float bary = n > 0 ? (float)(1.0 / (double)n) : 0.f;
    for (int idx = tid; idx < n * n; idx += FQ_THREADS) {
        const int i = idx / n, j = idx - i * n;
        float v = bary;
        if (bad) v = 0.f;
        else if (p0) v = p0[((long long)b * N + i) * N + j];
        else if (assign0) v = assign0[(long long)b * N + i] == j ? 1.f : 0.f;
        Pb[(long long)i * N + j] = v;
    }
    if (tid == 0) {
        const int frozen = n == 0 || bad;
        nvc[b] = n;
        nvw[b] = frozen ? 0 : n;
        done[b] = frozen;
        nit[b] = 0;
        status[b] = frozen ? 2 : 1;
    }
}

// One workgroup per pair: the line search, the update and the stop test of one round.  cost holds -G, q the solver's assignment.
// Thread t takes the corner's elements t, t + 256, ... (row-major) in both passes; the sums are fp64, folded in a fixed order.
// SEEDED: the linear term.  f(P) = q(P) + <C, P> with q(P) = tr(A22^T P B22 P^T), whose gradient is G - C, so <G - C, P> = 2 q(P),
// and with R = P - Q: f(Q + x R) = f(Q) + b x + a x^2,
//     a = (<G,P> - <C,P>) / 2 - (<G,Q> - <C,Q>) + q(Q),   b = (<G,Q> - <C,Q>) - 2 q(Q) + <C,P> - <C,Q>
// (SciPy's a and b21 + b12 + b22a + b22b): two more sums.  Without seeds C is not read and the three sums are all there is.
template <bool SEEDED>
__global__ __launch_bounds__(FQ_THREADS) void faq_step_kernel(const float *a1, const float *a2, long long gstride, int ld,
                                                              const float *cost, const float *C, const int *q, const int *nvc, int N,
                                                              float tol, float *P, int *nvw, int *done, int *nit, int *status) {
    __shared__ int q_l[FGNN_QAPW_MAX_N];
    __shared__ double red[FQ_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (done[b]) return;                        // uniform: a frozen pair keeps its P, nit and status
    const int n = nvc[b];
    int bad = 0;
    for (int k = tid; k < n; k += FQ_THREADS) {
        const int p = q[(long long)b * N + k];
        const bool ok = p >= 0 && p < n;
        q_l[k] = ok ? p : 0;
        bad |= !ok;
    }
    if (__syncthreads_or(bad)) {                // the solver found no finite assignment (a NaN in the corner): the pair ends here
        if (tid == 0) {
            done[b] = 1;
            nvw[b] = 0;
            nit[b] = 0;
            status[b] = 2;
        }
        return;
    }
    const float *A = a1 + (long long)b * gstride, *Bm = a2 + (long long)b * gstride, *Gb = cost + (long long)b * N * N;
    float *Pb = P + (long long)b * N * N;
    double gp = 0.0, gq = 0.0, fq = 0.0, cp = 0.0, cq = 0.0;       // <G, P>, <G, Q>, f(Q) (seeded: q(Q)); seeded: <C, P>, <C, Q>
    for (int idx = tid; idx < n * n; idx += FQ_THREADS) {
        const int i = idx / n, k = idx - i * n, qi = q_l[i];
        const double g = -(double)Gb[(long long)i * N + k], p = (double)Pb[(long long)i * N + k];
        gp += g * p;
        if (k == qi) gq += g;
        if constexpr (SEEDED) {
            const double cc = (double)C[(long long)b * N * N + (long long)i * N + k];
            cp += cc * p;
            if (k == qi) cq += cc;
        }
        fq += (double)A[(long long)i * ld + k] * (double)Bm[(long long)qi * ld + q_l[k]];
    }
    gp = block_sum(gp, red, tid);
    gq = block_sum(gq, red, tid);
    fq = block_sum(fq, red, tid);
    double a = 0.5 * gp - gq + fq, bb = gq - 2.0 * fq;
    if constexpr (SEEDED) {
        cp = block_sum(cp, red, tid);
        cq = block_sum(cq, red, tid);
        a = 0.5 * (gp - cp) - (gq - cq) + fq, bb = (gq - cq) - 2.0 * fq + cp - cq;
    }
    double alpha;
    if (a < 0.0 && 0.0 <= -bb / (2.0 * a) && -bb / (2.0 * a) <= 1.0) alpha = -bb / (2.0 * a);
    else alpha = -(a + bb) < 0.0 ? 1.0 : 0.0;
    double ss = 0.0;
    for (int idx = tid; idx < n * n; idx += FQ_THREADS) {
        const int i = idx / n, k = idx - i * n;
        const double p = (double)Pb[(long long)i * N + k];
        const float p1 = (float)(alpha * p + (1.0 - alpha) * (k == q_l[i] ? 1.0 : 0.0));      // one rounding, to fp32
        const double d = p - (double)p1;
        ss += d * d;
        Pb[(long long)i * N + k] = p1;
    }
    ss = block_sum(ss, red, tid);
    if (tid == 0) {
        nit[b] += 1;
        if (sqrt(ss) / sqrt((double)n) < (double)tol) {
            done[b] = 1;
            nvw[b] = 0;
            status[b] = 0;
        }
    }
}

// cost[b] = -P on the corner, for the last assignment.  grid (N, B): a workgroup per row.
__global__ __launch_bounds__(64) void faq_neg_p_kernel(const float *P, const int *nvc, int N, float *cost) {
    const int i = blockIdx.x, b = blockIdx.y, n = nvc[b];
    if (i >= n) return;
    const long long row = ((long long)b * N + i) * N;
    for (int j = threadIdx.x; j < n; j += 64) cost[row + j] = -P[row + j];
}

// One workgroup per pair: the outputs.  perm arrives from the solver (-1 everywhere if it found no assignment: status 2 then);
// a status-2 pair gets assign0 (or -1) and nit = 0; -1 past the corner; p_out = P on the corner, zero around it.
__global__ __launch_bounds__(FQ_THREADS) void faq_finish_kernel(const float *P, const int *assign0, const int *nvc, int N, int *perm,
                                                                int *nit, int *status, float *p_out) {
    const int b = blockIdx.x, tid = threadIdx.x, n = nvc[b];
    int bad = 0;
    for (int k = tid; k < n; k += FQ_THREADS) {
        const int p = perm[(long long)b * N + k];
        bad |= p < 0 || p >= n;
    }
    bad = __syncthreads_or(bad);
    const bool failed = status[b] == 2 || bad || n == 0;
    for (int k = tid; k < N; k += FQ_THREADS) {
        if (k >= n) perm[(long long)b * N + k] = -1;
        else if (failed) perm[(long long)b * N + k] = assign0 ? assign0[(long long)b * N + k] : -1;
    }
    if (p_out) {
        for (int idx = tid; idx < N * N; idx += FQ_THREADS) {
            const int i = idx / N, j = idx - i * N;
            p_out[(long long)b * N * N + idx] = (i < n && j < n) ? P[(long long)b * N * N + idx] : 0.f;
        }
    }
    __syncthreads();                             // every thread has read status[b]
    if (tid == 0 && failed) {
        status[b] = 2;
        nit[b] = 0;
    }
}

constexpr long long WS_ALIGN = 256;
long long ws_round(long long x) { return (x + WS_ALIGN - 1) / WS_ALIGN * WS_ALIGN; }

// ---- seeds (fgnn_qapw_faq_seeded): the chain above on the free block A22, B22 with n_b := u_b, the seeds' constant term C in the
// gradient, G = C + A22 P B22^T + A22^T P B22, and its linear term in the line search.  The kernels above run as they are wherever
// the seeds change nothing (the start, the first product, -P, the outputs of the free block); the second product and the step run
// in their SEEDED instantiation; the two kernels below are the way in and out of free coordinates.

// One workgroup per pair: what the start needs in free coordinates.  ok = the seeds are valid and assign0 (if given) holds them on
// every seeded row; ueff = u_b for such a pair, else 0 (the chain above then freezes it); assign_s[r] = the rank among the free
// columns of assign0[free_a[r]], -1 where that is no free column (the start refuses the pair: status 2).
__global__ __launch_bounds__(FQ_THREADS) void faq_seed_start_kernel(const int *seeds, const int *assign0, const int *nvalid, int N,
                                                                    const int *free_a, const int *free_b, const int *nfree,
                                                                    const int *valid, int *ok, int *ueff, int *assign_s) {
    __shared__ int col_rank[FGNN_QAPW_MAX_N];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = corner_of(nvalid, b, N), good = valid[b], u = good ? min(max(nfree[b], 0), n) : 0;
    const long long o = (long long)b * N;
    int bad = 0;
    if (assign0) {
        for (int k = tid; k < N; k += FQ_THREADS) col_rank[k] = -1;
        __syncthreads();
        for (int c = tid; c < u; c += FQ_THREADS) col_rank[free_b[o + c]] = c;
        __syncthreads();
        for (int k = tid; k < n; k += FQ_THREADS) {
            const int s = seeds[o + k];
            bad |= s >= 0 && assign0[o + k] != s;
        }
        for (int r = tid; r < N; r += FQ_THREADS) {
            int v = -1;
            if (r < u) {
                const int p = assign0[o + free_a[o + r]];
                if (p >= 0 && p < n) v = col_rank[p];
            }
            assign_s[o + r] = v;
        }
    }
    bad = __syncthreads_or(bad);
    if (tid == 0) {
        ok[b] = good && !bad;
        ueff[b] = good && !bad ? u : 0;
    }
}

// One workgroup per pair: out of free coordinates.  perm_s holds the free block's assignment as faq_finish_kernel left it.
//   invalid seeds: perm = -1, nit 0, status 2;   assign0 against the seeds, or refused / no assignment (status 2 above): perm =
//   assign0 (or -1), nit 0, status 2;   u_b = 0 < n_b: perm = seeds, nit 0, status 0;   n_b = 0: status 2, as without seeds;
//   else perm[free_a[r]] = free_b[perm_s[r]] and perm[i] = seeds[i] on the seeded rows.  -1 past the corner.
__global__ __launch_bounds__(FQ_THREADS) void faq_seed_finish_kernel(const int *seeds, const int *assign0, const int *nvalid, int N,
                                                                     const int *free_a, const int *free_b, const int *nfree,
                                                                     const int *nseed, const int *valid, const int *ok,
                                                                     const int *perm_s, int *perm, int *nit, int *status,
                                                                     int *seeded) {
    __shared__ int row_rank[FGNN_QAPW_MAX_N];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = corner_of(nvalid, b, N), good = valid[b], agreed = ok[b], u = agreed ? min(max(nfree[b], 0), n) : 0;
    const long long o = (long long)b * N;
    const int st = status[b];
    const bool trivial = agreed && u == 0 && n > 0, failed = !agreed || (!trivial && st == 2);
    for (int k = tid; k < N; k += FQ_THREADS) row_rank[k] = -1;
    __syncthreads();                             // (every thread has read status[b])
    for (int r = tid; r < u; r += FQ_THREADS) row_rank[free_a[o + r]] = r;
    __syncthreads();
    for (int k = tid; k < N; k += FQ_THREADS) {
        int v = -1;
        if (k < n) {
            const int s = seeds[o + k];
            if (failed) {
                v = (good && assign0) ? assign0[o + k] : -1;
            } else if (s >= 0) {
                v = s;
            } else {
                const int r = row_rank[k], c = r >= 0 ? perm_s[o + r] : -1;
                v = (c >= 0 && c < u) ? free_b[o + c] : -1;
            }
        }
        perm[o + k] = v;
    }
    if (tid == 0) {
        if (failed) {
            status[b] = 2;
            nit[b] = 0;
        } else if (trivial) {
            status[b] = 0;
            nit[b] = 0;
        }
        if (seeded) seeded[b] = nseed[b];
    }
}

// The workspace of a call: the chain's own part, then what only the seeded entry point uses (null without seeds).
struct FaqWs {
    float *P, *T, *cost;                        // the iterate, the two products, -G (then -P)
    int *q, *nvc, *nvw, *done, *correct;
    float *A22, *B22, *C, *P0;                  // the free blocks, the constant term, the gathered p0
    int *free_a, *free_b, *seed_a, *seed_b, *assign_s, *perm_s;
    int *nfree, *nseed, *valid, *ok, *ueff;
    long long bytes;
};

// (ws may be NULL: only `bytes` is then of use)
FaqWs faq_carve(void *ws, int B, int N, bool seeded) {
    const long long mat = ws_round((long long)B * N * N * 4), lst = ws_round((long long)B * N * 4), vec = ws_round((long long)B * 4);
    uintptr_t p = (uintptr_t)ws;
    const auto take = [&p](long long bytes) {
        const uintptr_t at = p;
        p += bytes;
        return at;
    };
    FaqWs w = {};
    w.P = (float *)take(mat), w.T = (float *)take(2 * mat), w.cost = (float *)take(mat);
    w.q = (int *)take(lst);
    w.nvc = (int *)take(vec), w.nvw = (int *)take(vec), w.done = (int *)take(vec), w.correct = (int *)take(vec);
    if (seeded) {
        w.A22 = (float *)take(mat), w.B22 = (float *)take(mat), w.C = (float *)take(mat), w.P0 = (float *)take(mat);
        w.free_a = (int *)take(lst), w.free_b = (int *)take(lst), w.seed_a = (int *)take(lst), w.seed_b = (int *)take(lst);
        w.assign_s = (int *)take(lst), w.perm_s = (int *)take(lst);
        w.nfree = (int *)take(vec), w.nseed = (int *)take(vec), w.valid = (int *)take(vec), w.ok = (int *)take(vec), w.ueff = (int *)take(vec);
    }
    w.bytes = (long long)(p - (uintptr_t)ws);
    return w;
}

// what both entry points check; `who` names the entry point in the messages
int faq_check(const char *who, bool pointers, const float *p0, const int *assign0, long long gstride, int ld, int B, int N, int maxiter,
              float tol, const void *ws, long long ws_bytes, long long need) {
    FGNN_CHECK(pointers && B > 0 && N > 0, "%s: bad arguments", who);
    FGNN_CHECK(!(p0 && assign0), "%s: at most one of p0 and assign0", who);
    FGNN_CHECK(maxiter > 0 && tol > 0.f, "%s: maxiter and tol must be positive (got %d, %g)", who, maxiter, (double)tol);
    FGNN_CHECK(N <= FGNN_QAPW_MAX_N, "%s: at most %d vertices per graph (got %d)", who, FGNN_QAPW_MAX_N, N);
    FGNN_CHECK(B <= FQ_MAX_B, "%s: at most %d pairs per call (got %d)", who, FQ_MAX_B, B);
    FGNN_CHECK(ld >= N && gstride >= (long long)N * ld, "%s: ld / gstride smaller than the matrices", who);
    FGNN_CHECK(ws_bytes >= need && ((uintptr_t)ws & 15) == 0, "%s: the workspace needs %lld bytes, 16-byte aligned (got %lld)", who, need,
               ws_bytes);
    return 0;
}

// The chain on the corners nvalid names: init, maxiter x (the two products, the assignment, the step), -P, the last assignment,
// the outputs.  C (may be NULL: no seeds) is the constant term of the gradient and picks the instantiations of the two kernels
// that know it.
int faq_chain(const float *a1, const float *a2, long long gstride, int ld, const float *C, const float *p0, const int *assign0,
              const int *nvalid, int B, int N, int maxiter, float tol, const FaqWs &w, int *perm, int *nit, int *status, float *p_out,
              void *stream) {
    hipStream_t st = (hipStream_t)stream;
    const long long bs = (long long)N * N;
    const dim3 tiles((N + FQ_ROWS - 1) / FQ_ROWS, (N + FQ_COLS - 1) / FQ_COLS, B);
    int rc;
    hipLaunchKernelGGL(faq_init_kernel, dim3(B), dim3(FQ_THREADS), 0, st, p0, assign0, nvalid, N, w.P, w.nvc, w.nvw, w.done, nit, status);
    FGNN_LAUNCH_CHECK();
    for (int it = 0; it < maxiter; ++it) {
        hipLaunchKernelGGL(faq_pb_kernel, dim3(tiles.x, 2 * tiles.y, B), dim3(FQ_THREADS), 0, st, a2, gstride, ld, w.P, w.nvc, w.done, N, w.T);
        FGNN_LAUNCH_CHECK();
        hipLaunchKernelGGL(C ? faq_grad_kernel<true> : faq_grad_kernel<false>, tiles, dim3(FQ_THREADS), 0, st, a1, gstride, ld, w.T, C, w.nvc,
                           w.done, N, w.cost);
        FGNN_LAUNCH_CHECK();
        if ((rc = fgnn_lsap_accuracy(w.cost, bs, N, w.nvw, B, N, w.correct, w.q, stream))) return rc;      // a frozen pair: n = 0, no work
        hipLaunchKernelGGL(C ? faq_step_kernel<true> : faq_step_kernel<false>, dim3(B), dim3(FQ_THREADS), 0, st, a1, a2, gstride, ld, w.cost, C,
                           w.q, w.nvc, N, tol, w.P, w.nvw, w.done, nit, status);
        FGNN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(faq_neg_p_kernel, dim3(N, B), dim3(64), 0, st, w.P, w.nvc, N, w.cost);
    FGNN_LAUNCH_CHECK();
    if ((rc = fgnn_lsap_accuracy(w.cost, bs, N, w.nvc, B, N, w.correct, perm, stream))) return rc;
    hipLaunchKernelGGL(faq_finish_kernel, dim3(B), dim3(FQ_THREADS), 0, st, w.P, assign0, w.nvc, N, perm, nit, status, p_out);
    FGNN_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" long long fgnn_qapw_faq_ws_bytes(int B, int N) { return B <= 0 || N <= 0 ? 0 : faq_carve(nullptr, B, N, false).bytes; }

extern "C" int fgnn_qapw_faq(const float *a1, const float *a2, long long gstride, int ld, const float *p0, const int *assign0,
                             const int *nvalid, int B, int N, int maxiter, float tol, void *ws, long long ws_bytes, int *perm, int *nit,
                             int *status, float *p_out, void *stream) {
    if (int rc = faq_check("fgnn_qapw_faq", a1 && a2 && ws && perm && nit && status, p0, assign0, gstride, ld, B, N, maxiter, tol, ws,
                           ws_bytes, fgnn_qapw_faq_ws_bytes(B, N)))
        return rc;
    return faq_chain(a1, a2, gstride, ld, nullptr, p0, assign0, nvalid, B, N, maxiter, tol, faq_carve(ws, B, N, false), perm, nit, status,
                     p_out, stream);
}

extern "C" long long fgnn_qapw_faq_seeded_ws_bytes(int B, int N) { return B <= 0 || N <= 0 ? 0 : faq_carve(nullptr, B, N, true).bytes; }

extern "C" int fgnn_qapw_faq_seeded(const float *a1, const float *a2, long long gstride, int ld, const int *seeds, const float *p0,
                                    int p0_free, const int *assign0, const int *nvalid, int B, int N, int maxiter, float tol, void *ws,
                                    long long ws_bytes, int *perm, int *nit, int *status, int *seeded, float *p_out, void *stream) {
    int rc;
    if ((rc = faq_check("fgnn_qapw_faq_seeded", a1 && a2 && seeds && ws && perm && nit && status, p0, assign0, gstride, ld, B, N, maxiter,
                        tol, ws, ws_bytes, fgnn_qapw_faq_seeded_ws_bytes(B, N))))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    const FaqWs w = faq_carve(ws, B, N, true);
    // into free coordinates: the index lists, the free blocks A22, B22 (and p0's), the constant term
    if ((rc = fgnn_seed_index(seeds, nvalid, B, N, w.nfree, w.nseed, w.free_a, w.free_b, w.seed_a, w.seed_b, w.valid, stream))) return rc;
    hipLaunchKernelGGL(faq_seed_start_kernel, dim3(B), dim3(FQ_THREADS), 0, st, seeds, assign0, nvalid, N, w.free_a, w.free_b, w.nfree,
                       w.valid, w.ok, w.ueff, w.assign_s);
    FGNN_LAUNCH_CHECK();
    if ((rc = fgnn_seed_gather(a1, gstride, ld, w.free_a, w.free_a, w.ueff, B, N, w.A22, stream))) return rc;
    if ((rc = fgnn_seed_gather(a2, gstride, ld, w.free_b, w.free_b, w.ueff, B, N, w.B22, stream))) return rc;
    if (p0 && !p0_free && (rc = fgnn_seed_gather(p0, (long long)N * N, N, w.free_a, w.free_b, w.ueff, B, N, w.P0, stream))) return rc;
    if ((rc = fgnn_seed_const(a1, a2, gstride, ld, w.free_a, w.free_b, w.seed_a, w.seed_b, w.ueff, w.nseed, B, N, w.C, stream))) return rc;
    // the chain on the free block, its matching in free coordinates
    if ((rc = faq_chain(w.A22, w.B22, (long long)N * N, N, w.C, p0 ? (p0_free ? p0 : w.P0) : nullptr, assign0 ? w.assign_s : nullptr, w.ueff,
                        B, N, maxiter, tol, w, w.perm_s, nit, status, p_out, stream)))
        return rc;
    hipLaunchKernelGGL(faq_seed_finish_kernel, dim3(B), dim3(FQ_THREADS), 0, st, seeds, assign0, nvalid, N, w.free_a, w.free_b, w.nfree,
                       w.nseed, w.valid, w.ok, w.perm_s, perm, nit, status, seeded);
    FGNN_LAUNCH_CHECK();
    return 0;
}
