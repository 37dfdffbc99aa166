// Seeds (known matches; SciPy's partial_match, the setting of seeded graph matching, Fishkind et al. 2019) for the QAP solvers:
// the index lists of a seed vector, the gather of a free block, and the constant term the seeds add to FAQ's gradient.
// seeds[b][i] = j >= 0 fixes vertex i of graph 1 to vertex j of graph 2, a negative entry leaves row i free (the convention of
// labels); rows at or beyond n_b are ignored.  Pair b has m_b seeds and u_b = n_b - m_b free vertices; free rows and free columns
// are taken in ascending order (SciPy's setdiff1d), seeded rows in ascending order of the row.
//
//   fgnn_seed_index  : seeds -> u_b, m_b, free_a, free_b, seed_a, seed_b, valid.  One workgroup per pair, thread t owns row t and
//                      column t; ranks are ballot + popcount prefix counts, waves folded in order.  No atomics: a column's owner is
//                      written by plain LDS stores, and of two rows that claim one column the one that lost the store sees it.
//   fgnn_seed_gather : out[b][r][c] = in[b][rows[r]][cols[c]] for r, c < u_b, exact zeros elsewhere: A22, B22, a float P0, scores.
//   fgnn_seed_const  : C[r][c] = sum_s A[fa r][sa s] B[fb c][sb s] + A[sa s][fa r] B[sb s][fb c] (SciPy's A21 B21^T + A12^T B12):
//                      one fp32 fmaf chain per entry, s ascending, the row term before the column term.
//
// Everything here runs once per call on at most 256 vertices: latency work, no matrix cores.
#include "fgnn_rows.h"

namespace {

constexpr int SD_THREADS = 256;            // = FGNN_SEED_MAX_N: a thread per row / column
constexpr int SD_WAVES = SD_THREADS / 64;
constexpr int SD_MAX_B = 65535;            // pairs ride on grid.y in the gather and the constant term

// The number of flagged threads below this one, and the workgroup's total: ballot inside a wave, the waves added in order.
DEVI int rank_of(bool flag, int *wave_cnt, int tid, int &total) {
    const unsigned long long m = __ballot(flag);
    const int lane = tid & 63, wv = tid >> 6;
    if (lane == 0) wave_cnt[wv] = __popcll(m);
    __syncthreads();
    int base = 0, all = 0;
#pragma unroll
    for (int w = 0; w < SD_WAVES; ++w) {
        const int c = wave_cnt[w];
        base += w < wv ? c : 0;
        all += c;
    }
    __syncthreads();
    total = all;
    return base + __popcll(m & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(SD_THREADS) void seed_index_kernel(const int *seeds, const int *nvalid, int N, int *nfree, int *nseed,
                                                                int *free_a, int *free_b, int *seed_a, int *seed_b, int *valid) {
    __shared__ int owner[SD_THREADS];          // owner[j]: a row seeded to column j, -1 without
    __shared__ int list[4][SD_THREADS];        // free_a, free_b, seed_a, seed_b; -1 past their ends
    __shared__ int wave_cnt[SD_WAVES];
    const int b = blockIdx.x, t = threadIdx.x;
    const int n = corner_of(nvalid, b, N);
    const int s = t < n ? seeds[(long long)b * N + t] : -1;
    const bool seeded = t < n && s >= 0, inside = seeded && s < n;
    owner[t] = -1;
#pragma unroll
    for (int l = 0; l < 4; ++l) list[l][t] = -1;
    __syncthreads();
    if (inside) owner[s] = t;
    __syncthreads();
    const int bad = __syncthreads_or(seeded && (!inside || owner[s] != t));
    const bool row_free = t < n && !seeded, col_free = t < n && owner[t] < 0;
    int u, m, uc;
    const int rf = rank_of(row_free, wave_cnt, t, u), rs = rank_of(seeded, wave_cnt, t, m), cf = rank_of(col_free, wave_cnt, t, uc);
    if (!bad) {                                 // (valid seeds: uc == u, every rank < 256)
        if (row_free) list[0][rf] = t;
        if (col_free) list[1][cf] = t;
        if (seeded) {
            list[2][rs] = t;
            list[3][rs] = s;
        }
    }
    __syncthreads();
    if (t < N) {
        const long long o = (long long)b * N + t;
        free_a[o] = list[0][t];
        free_b[o] = list[1][t];
        seed_a[o] = list[2][t];
        seed_b[o] = list[3][t];
    }
    if (t == 0) {
        nfree[b] = u;
        nseed[b] = m;
        valid[b] = bad ? 0 : 1;
    }
}

DEVI int count_of(const int *cnt, int b, int N) { return min(max(cnt[b], 0), N); }

// grid (N, B): a workgroup per output row.  An index outside [0, N) (a caller error) reads as an empty source.
__global__ __launch_bounds__(64) void seed_gather_kernel(const float *in, long long gstride, int ld, const int *rows, const int *cols,
                                                         const int *nfree, int N, float *out) {
    const int r = blockIdx.x, b = blockIdx.y, u = count_of(nfree, b, N);
    const int i = r < u ? rows[(long long)b * N + r] : -1;
    const float *src = in + (long long)b * gstride + (long long)(i >= 0 && i < N ? i : 0) * ld;
    float *dst = out + ((long long)b * N + r) * N;
    for (int c = threadIdx.x; c < N; c += 64) {
        const int j = c < u ? cols[(long long)b * N + c] : -1;
        dst[c] = (i >= 0 && i < N && j >= 0 && j < N) ? src[j] : 0.f;
    }
}

// grid (N, B): a workgroup per row r of C, thread c its column.  The row's 2 m_b entries of A wait in LDS.
__global__ __launch_bounds__(SD_THREADS) void seed_const_kernel(const float *a1, const float *a2, long long gstride, int ld,
                                                                const int *free_a, const int *free_b, const int *seed_a,
                                                                const int *seed_b, const int *nfree, const int *nseed, int N, float *out) {
    __shared__ float a_row[SD_THREADS], a_col[SD_THREADS];
    __shared__ int sb_l[SD_THREADS];
    const int r = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const int u = count_of(nfree, b, N), m = count_of(nseed, b, N);
    const float *A = a1 + (long long)b * gstride, *Bm = a2 + (long long)b * gstride;
    const long long o = (long long)b * N;
    const int i = r < u ? free_a[o + r] : -1;
    const bool row_ok = i >= 0 && i < N;        // uniform
    if (row_ok && t < m) {
        const int sa = seed_a[o + t], sb = seed_b[o + t];
        const bool ok = sa >= 0 && sa < N && sb >= 0 && sb < N;
        a_row[t] = ok ? A[(long long)i * ld + sa] : 0.f;
        a_col[t] = ok ? A[(long long)sa * ld + i] : 0.f;
        sb_l[t] = ok ? sb : 0;
    }
    __syncthreads();
    if (t >= N) return;
    float acc = 0.f;
    const int j = (row_ok && t < u) ? free_b[o + t] : -1;
    if (j >= 0 && j < N) {
        for (int s = 0; s < m; ++s) {
            const int sb = sb_l[s];
            acc = fmaf(a_row[s], Bm[(long long)j * ld + sb], acc);
            acc = fmaf(a_col[s], Bm[(long long)sb * ld + j], acc);
        }
    }
    out[(o + r) * N + t] = acc;
}

}  // namespace

extern "C" int fgnn_seed_index(const int *seeds, const int *nvalid, int B, int N, int *nfree, int *nseed, int *free_a, int *free_b,
                               int *seed_a, int *seed_b, int *valid, void *stream) {
    FGNN_CHECK(seeds && nfree && nseed && free_a && free_b && seed_a && seed_b && valid && B > 0 && N > 0, "fgnn_seed_index: bad arguments");
    FGNN_CHECK(N <= FGNN_SEED_MAX_N, "fgnn_seed_index: at most %d vertices per graph (got %d)", FGNN_SEED_MAX_N, N);
    hipLaunchKernelGGL(seed_index_kernel, dim3(B), dim3(SD_THREADS), 0, (hipStream_t)stream, seeds, nvalid, N, nfree, nseed, free_a,
                       free_b, seed_a, seed_b, valid);
    FGNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int fgnn_seed_gather(const float *in, long long gstride, int ld, const int *rows, const int *cols, const int *nfree, int B,
                                int N, float *out, void *stream) {
    FGNN_CHECK(in && rows && cols && nfree && out && B > 0 && N > 0, "fgnn_seed_gather: bad arguments");
    FGNN_CHECK(N <= FGNN_SEED_MAX_N, "fgnn_seed_gather: at most %d vertices per graph (got %d)", FGNN_SEED_MAX_N, N);
    FGNN_CHECK(B <= SD_MAX_B, "fgnn_seed_gather: at most %d pairs per call (got %d)", SD_MAX_B, B);
    FGNN_CHECK(ld >= N && gstride >= (long long)N * ld, "fgnn_seed_gather: ld / gstride smaller than the matrices");
    hipLaunchKernelGGL(seed_gather_kernel, dim3(N, B), dim3(64), 0, (hipStream_t)stream, in, gstride, ld, rows, cols, nfree, N, out);
    FGNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int fgnn_seed_const(const float *a1, const float *a2, long long gstride, int ld, const int *free_a, const int *free_b,
                               const int *seed_a, const int *seed_b, const int *nfree, const int *nseed, int B, int N, float *out,
                               void *stream) {
    FGNN_CHECK(a1 && a2 && free_a && free_b && seed_a && seed_b && nfree && nseed && out && B > 0 && N > 0, "fgnn_seed_const: bad arguments");
    FGNN_CHECK(N <= FGNN_SEED_MAX_N, "fgnn_seed_const: at most %d vertices per graph (got %d)", FGNN_SEED_MAX_N, N);
    FGNN_CHECK(B <= SD_MAX_B, "fgnn_seed_const: at most %d pairs per call (got %d)", SD_MAX_B, B);
    FGNN_CHECK(ld >= N && gstride >= (long long)N * ld, "fgnn_seed_const: ld / gstride smaller than the matrices");
    hipLaunchKernelGGL(seed_const_kernel, dim3(N, B), dim3(SD_THREADS), 0, (hipStream_t)stream, a1, a2, gstride, ld, free_a, free_b,
                       seed_a, seed_b, nfree, nseed, N, out);
    FGNN_LAUNCH_CHECK();
    return 0;
}
