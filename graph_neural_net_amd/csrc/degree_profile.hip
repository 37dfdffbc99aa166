// Degree-profile matching (Ding, Ma, Wu, Xu, "Efficient random graph matching via degree profiles"): every vertex gets a sorted
// multiset of real values, its profile, and the similarity of vertex i of side 1 and vertex j of side 2 is minus the 1-Wasserstein
// distance of their profiles.  No iteration, no tolerance, no start: a SCORE producer of O(n^2 d) work.
//
//     weighted input    profile of i = { A[i, k] : k != i, k < n_b }, the fp32 inputs themselves; m_i = n_b - 1
//     0/1 input         one value per neighbour k of i, m_i = d_i:  (c_ik - r_i q) / sqrt(r_i q (1 - q)),  r_i = n_b - 1 - d_i,
//                       q = (sum of degrees) / (n_b (n_b - 1)),  c_ik = d_k - 1 - |N(i) & N(k)| (a popcount over the bit words);
//                       r_i = 0 gives 0.  Self-loops are ignored; the bit rows are taken as they are (symmetric input is assumed)
//     empty profile     the point mass at 0
//     Z(i, j) = (1 / (m l)) sum_t len_t |a[t / l] - b[t / m]|   over the segments of [0, m l) cut at the multiples of l and of m, in
//                       ascending order -- every tie between break points decided in integer arithmetic --, each term the fp64
//                       product of the integer length and the fp64 difference, added to an fp64 sum in that order (no fused
//                       multiply-add: the sum is the one numpy float64 forms), one fp64 division, one rounding to fp32
//     X = -Z on the n_b x n_b corner, exact +0.0 around it;  perm = the assignment of fgnn_lsap_accuracy on Z
//
// Launches: dp_scan_kernel (degrees and their sum, or the inf / NaN flag of a weighted corner) -> dp_profiles_kernel (a wave per
// vertex row: build, sort in LDS, write) -> dp_distance_kernel (the hot one: a 16 x 16 tile of (i, j) per workgroup, the 32 sorted
// rows in LDS, a thread per entry walks the merge) -> the solver -> dp_finish_kernel.  No atomics, no scratch, nothing outside a
// corner is read; every value depends on its own pair alone, so results are bit-identical from run to run and across batches.
#include "fgnn_qap_bits.h"

namespace {

constexpr int DP_THREADS = 256;            // 4 waves
constexpr int DP_WAVES = DP_THREADS / 64;  // vertex rows per workgroup of the profile launch
constexpr int DP_MAX_N = 256;              // a wave sorts at most 256 keys, 4 per lane; the scan gives every row one thread
constexpr int DP_MAX_B = 65535;            // pairs ride on a grid dimension
constexpr int DP_NW = DP_MAX_N / 32;       // words of a bit row
constexpr int DP_TILE = 16;                // the distance launch: 16 x 16 entries per workgroup
constexpr int DP_PITCH = DP_MAX_N + 1;     // odd: the 16 rows that the lanes of a wave walk at a similar index sit on 16 banks
constexpr int DP_PAD_KEY = 0x7fffffff;     // above every key: padding sorts last

// fp32 <-> an int32 of the same order (-0.0 below +0.0, +inf below DP_PAD_KEY); its own inverse
DEVI int key_of(float v) {
    const unsigned u = __float_as_uint(v);
    return (int)(u ^ ((u >> 31) ? 0x7fffffffu : 0u));
}
DEVI float value_of(int k) {
    const unsigned u = (unsigned)k;
    return __uint_as_float(u ^ ((u >> 31) ? 0x7fffffffu : 0u));
}

// word w of bit row r of M inside the n x n corner, the diagonal bit cleared
DEVI unsigned row_word(const unsigned *M, int W, int r, int w, int n) {
    unsigned v = M[(long long)r * W + w] & corner_mask(w, n);
    if ((r >> 5) == w) v &= ~(1u << (r & 31));
    return v;
}

// A workgroup per (pair, side).  0/1 input: thread k owns row k, deg[b][side][k] = its degree (0 past the corner), degsum = their sum;
// flag = 2 where n_b < 2 or the density is 0 or 1.  Weighted input: flag = 2 where n_b < 2, else 3 where the corner holds an inf or
// a NaN.  nvc[b] = the clamped vertex count.
__global__ __launch_bounds__(DP_THREADS) void dp_scan_kernel(const float *a1, const float *a2, long long gstride, int ld,
                                                             const unsigned *bits1, const unsigned *bits2, const int *nvalid, int N,
                                                             int *deg, int *degsum, int *flag, int *nvc) {
    __shared__ int red[DP_WAVES];
    const int b = blockIdx.x, side = blockIdx.y, tid = threadIdx.x;
    const int n = corner_of(nvalid, b, N);
    int f = 0, total = 0;
    if (bits1) {
        const int W = (N + 31) >> 5;
        const unsigned *M = (side ? bits2 : bits1) + (long long)b * N * W;
        int d = 0;
        if (tid < n)
            for (int w = 0; w < W; ++w) d += __popc(row_word(M, W, tid, w, n));
        if (tid < N) deg[((long long)b * 2 + side) * N + tid] = d;
        int s = d;
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if ((tid & 63) == 0) red[tid >> 6] = s;
        __syncthreads();
        total = (red[0] + red[1]) + (red[2] + red[3]);
        f = (n < 2 || total == 0 || total == n * (n - 1)) ? 2 : 0;
    } else {
        const float *A = (side ? a2 : a1) + (long long)b * gstride;
        int bad = 0;
        for (int idx = tid; idx < n * n; idx += DP_THREADS) {
            const int i = idx / n, j = idx - i * n;
            const float v = A[(long long)i * ld + j];
            bad |= !(v - v == 0.f);
        }
        bad = __syncthreads_or(bad);
        f = n < 2 ? 2 : (bad ? 3 : 0);
    }
    if (tid == 0) {
        flag[2 * b + side] = f;
        degsum[2 * b + side] = total;
        if (side == 0) nvc[b] = n;
    }
}

// grid (ceil(N / 4), 2, B): wave w of a workgroup owns vertex row i = 4 blockIdx.x + w of side blockIdx.y.  It writes the row's m keys
// into its 256 slots of LDS -- the fp32 entries as order-preserving integers, or the integers c_ik of which a row's values are an
// increasing affine map --, the four waves sort their rows side by side with one bitonic network over P = the power of two >= n_b
// slots (padding above every key), and the wave writes prof[side][b][i][0 .. N) = the m values ascending, +inf behind them, and
// counts[b][side][i] = m.  A row past the corner, and every row of a pair whose flag is set, has m = 0.
__global__ __launch_bounds__(DP_THREADS) void dp_profiles_kernel(const float *a1, const float *a2, long long gstride, int ld,
                                                                 const unsigned *bits1, const unsigned *bits2, const int *nvc,
                                                                 const int *deg, const int *degsum, const int *flag, int N, float *prof,
                                                                 int *counts) {
    __shared__ int keys[DP_WAVES][DP_MAX_N];
    __shared__ unsigned rowi[DP_WAVES][DP_NW];
    const int b = blockIdx.z, side = blockIdx.y, B = gridDim.z, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int i = DP_WAVES * blockIdx.x + wv;
    const int n = nvc[b], W = (N + 31) >> 5;
    const bool ok = flag[2 * b] == 0 && flag[2 * b + 1] == 0;      // uniform in the workgroup: then n >= 2
    const bool live = ok && i < n;                                 // uniform in the wave
    const unsigned *M = bits1 ? (side ? bits2 : bits1) + (long long)b * N * W : nullptr;
    const int *dg = deg + ((long long)b * 2 + side) * N;
    int P = 0;
    if (ok)
        for (P = 2; P < n; P <<= 1) {}
    for (int t = lane; t < P; t += 64) keys[wv][t] = DP_PAD_KEY;
    if (M && lane < DP_NW) rowi[wv][lane] = (live && lane < W) ? row_word(M, W, i, lane, n) : 0u;
    __syncthreads();
    int m = 0;
    if (live && M) {
        for (int k0 = 0; k0 < n; k0 += 64) {                       // 64 candidate neighbours per turn, compacted by a ballot
            const int k = k0 + lane;
            const bool nb = k < n && ((rowi[wv][k >> 5] >> (k & 31)) & 1u);
            int c = 0;
            if (nb) {
                int inter = 0;
                for (int w = 0; w < W; ++w) inter += __popc(row_word(M, W, k, w, n) & rowi[wv][w]);
                c = dg[k] - 1 - inter;
            }
            const unsigned long long mask = __ballot(nb);
            if (nb) keys[wv][m + __popcll(mask & ((1ull << lane) - 1ull))] = c;
            m += __popcll(mask);
        }
    } else if (live) {
        const float *row = (side ? a2 : a1) + (long long)b * gstride + (long long)i * ld;
        for (int k = lane; k < n; k += 64)
            if (k != i) keys[wv][k - (k > i)] = key_of(row[k]);
        m = n - 1;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < (P >> 1); t += 64) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const int x = keys[wv][lo], y = keys[wv][hi];
                if ((x > y) == ((lo & k) == 0)) {
                    keys[wv][lo] = y;
                    keys[wv][hi] = x;
                }
            }
            __syncthreads();
        }
    }
    if (i >= N) return;
    float *out = prof + (((long long)side * B + b) * N + i) * N;
    if (M) {
        const int r = live ? n - 1 - dg[i] : 0, S = degsum[2 * b + side], nn1 = n * (n - 1);
        const double q = live ? (double)S / (double)nn1 : 0.5;
        const double sd = sqrt((double)r * q * (1.0 - q));
        for (int k = lane; k < N; k += 64) {
            float v = INFINITY;
            if (k < m) v = r > 0 ? (float)((double)(keys[wv][k] * nn1 - r * S) / (double)nn1 / sd) : 0.f;
            out[k] = v;
        }
    } else {
        for (int k = lane; k < N; k += 64) out[k] = k < m ? value_of(keys[wv][k]) : INFINITY;
    }
    if (lane == 0) counts[((long long)b * 2 + side) * N + i] = m;
}

// grid (ceil(N / 16), ceil(N / 16), B): the tile (i0 .. i0 + 15) x (j0 .. j0 + 15) of pair b.  The 16 + 16 sorted rows go to LDS (an
// empty profile as the one value 0), thread (ti, tj) walks the merge of row i0 + ti of side 1 and row j0 + tj of side 2 and writes
// cost = (float)Z and X = -(float)Z; outside the corner X = +0.0, and a pair whose flag is set gets X = 0 and cost = 0 everywhere.
__global__ __launch_bounds__(DP_THREADS) void dp_distance_kernel(const float *prof, const int *counts, const int *nvc, const int *flag,
                                                                 int N, float *cost, float *X) {
    __shared__ float pa[DP_TILE * DP_PITCH];
    __shared__ float pb[DP_TILE * DP_PITCH];
    __shared__ int ma[DP_TILE], mb[DP_TILE];
    const int b = blockIdx.z, B = gridDim.z, i0 = blockIdx.x * DP_TILE, j0 = blockIdx.y * DP_TILE, tid = threadIdx.x;
    const int ti = tid >> 4, tj = tid & 15, i = i0 + ti, j = j0 + tj;
    const int n = nvc[b];
    const bool ok = flag[2 * b] == 0 && flag[2 * b + 1] == 0;
    const long long at = ((long long)b * N + i) * N + j;
    if (!ok || i0 >= n || j0 >= n) {                               // uniform
        if (i < N && j < N) {
            X[at] = 0.f;
            if (i < n && j < n) cost[at] = 0.f;
        }
        return;
    }
    const int wv = tid >> 6, lane = tid & 63;
    for (int r = wv; r < 2 * DP_TILE; r += DP_WAVES) {             // a wave per staged row
        const int sd = r >= DP_TILE, rr = r - sd * DP_TILE, g = (sd ? j0 : i0) + rr;
        float *dst = (sd ? pb : pa) + rr * DP_PITCH;
        int m = 1;
        if (g < n) {
            m = counts[((long long)b * 2 + sd) * N + g];
            const float *src = prof + (((long long)sd * B + b) * N + g) * N;
            for (int k = lane; k < m; k += 64) dst[k] = src[k];
        }
        if (lane == 0) {
            if (m == 0 || g >= n) dst[0] = 0.f;
            (sd ? mb : ma)[rr] = m > 0 ? m : 1;
        }
    }
    __syncthreads();
    if (i >= N || j >= N) return;
    if (i >= n || j >= n) {
        X[at] = 0.f;
        return;
    }
    const float *a = pa + ti * DP_PITCH, *bq = pb + tj * DP_PITCH;
    const int m = ma[ti], l = mb[tj], ml = m * l;
    int ia = 0, ib = 0, na = l, nb = m, pos = 0;
    double va = (double)a[0], vb = (double)bq[0], sum = 0.0;
    while (pos < ml) {
        const int nxt = min(na, nb);
        sum = __dadd_rn(sum, __dmul_rn((double)(nxt - pos), fabs(va - vb)));
        if (na == nxt) {
            na += l;
            if (++ia < m) va = (double)a[ia];
        }
        if (nb == nxt) {
            nb += m;
            if (++ib < l) vb = (double)bq[ib];
        }
        pos = nxt;
    }
    const float z = (float)(sum / (double)ml);
    cost[at] = z;
    X[at] = -z;
}

// One workgroup per pair: status = the pair's flag (2 as well where the solver found no assignment), perm = -1 past the corner and
// everywhere unless status is 0.
__global__ __launch_bounds__(DP_THREADS) void dp_finish_kernel(const int *nvc, const int *flag, int N, int *perm, int *status) {
    const int b = blockIdx.x, tid = threadIdx.x, n = nvc[b];
    const int st = max(flag[2 * b], flag[2 * b + 1]);
    int bad = 0;
    for (int k = tid; k < n; k += DP_THREADS) {
        const int p = perm[(long long)b * N + k];
        bad |= p < 0 || p >= n;
    }
    bad = __syncthreads_or(bad);
    const bool failed = st != 0 || bad;
    for (int k = tid; k < N; k += DP_THREADS)
        if (k >= n || failed) perm[(long long)b * N + k] = -1;
    if (tid == 0) status[b] = st ? st : (bad ? 2 : 0);
}

constexpr long long DP_WS_ALIGN = 256;
long long dp_round(long long x) { return (x + DP_WS_ALIGN - 1) / DP_WS_ALIGN * DP_WS_ALIGN; }

struct DegreeProfileWs {
    float *cost, *prof;                         // Z; the two profile slabs, (2, B, N, N)
    int *counts, *deg, *degsum, *flag, *nvc, *correct;
    long long bytes;
};

// (ws may be NULL: only `bytes` is then of use)
DegreeProfileWs dp_carve(void *ws, int B, int N) {
    const long long mat = dp_round((long long)B * N * N * 4), rows = dp_round((long long)B * 2 * N * 4), vec = dp_round((long long)B * 8);
    uintptr_t p = (uintptr_t)ws;
    const auto take = [&p](long long bytes) {
        const uintptr_t at = p;
        p += bytes;
        return at;
    };
    DegreeProfileWs w = {};
    w.cost = (float *)take(mat), w.prof = (float *)take(2 * mat);
    w.counts = (int *)take(rows), w.deg = (int *)take(rows);
    w.degsum = (int *)take(vec), w.flag = (int *)take(vec), w.nvc = (int *)take(vec), w.correct = (int *)take(vec);
    w.bytes = (long long)(p - (uintptr_t)ws);
    return w;
}

}  // namespace

extern "C" long long fgnn_degree_profile_ws_bytes(int B, int N) { return B <= 0 || N <= 0 ? 0 : dp_carve(nullptr, B, N).bytes; }

extern "C" int fgnn_degree_profile(const float *a1, const float *a2, long long gstride, int ld, const unsigned *bits1,
                                   const unsigned *bits2, const int *nvalid, int B, int N, void *ws, float *X, int *perm, int *status,
                                   float *profiles, int *counts, void *stream) {
    FGNN_CHECK(ws && X && perm && status && B > 0 && N > 0, "fgnn_degree_profile: bad arguments");
    FGNN_CHECK((a1 && a2 && !bits1 && !bits2) || (bits1 && bits2 && !a1 && !a2),
               "fgnn_degree_profile: give either the two fp32 matrices or the two bit matrices");
    FGNN_CHECK(N <= DP_MAX_N, "fgnn_degree_profile: at most %d vertices per graph (got %d)", DP_MAX_N, N);
    FGNN_CHECK(B <= DP_MAX_B, "fgnn_degree_profile: at most %d pairs per call (got %d)", DP_MAX_B, B);
    FGNN_CHECK(bits1 || (ld >= N && gstride >= (long long)N * ld), "fgnn_degree_profile: ld / gstride smaller than the matrices");
    FGNN_CHECK(((uintptr_t)ws & 15) == 0, "fgnn_degree_profile: the workspace (fgnn_degree_profile_ws_bytes bytes) must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const DegreeProfileWs w = dp_carve(ws, B, N);
    float *prof = profiles ? profiles : w.prof;
    int *cnt = counts ? counts : w.counts;
    const int tiles = (N + DP_TILE - 1) / DP_TILE;
    hipLaunchKernelGGL(dp_scan_kernel, dim3(B, 2), dim3(DP_THREADS), 0, st, a1, a2, gstride, ld, bits1, bits2, nvalid, N, w.deg, w.degsum,
                       w.flag, w.nvc);
    FGNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(dp_profiles_kernel, dim3((N + DP_WAVES - 1) / DP_WAVES, 2, B), dim3(DP_THREADS), 0, st, a1, a2, gstride, ld, bits1,
                       bits2, w.nvc, w.deg, w.degsum, w.flag, N, prof, cnt);
    FGNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(dp_distance_kernel, dim3(tiles, tiles, B), dim3(DP_THREADS), 0, st, prof, cnt, w.nvc, w.flag, N, w.cost, X);
    FGNN_LAUNCH_CHECK();
    const int rc = fgnn_lsap_accuracy(w.cost, (long long)N * N, N, w.nvc, B, N, w.correct, perm, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(dp_finish_kernel, dim3(B), dim3(DP_THREADS), 0, st, w.nvc, w.flag, N, perm, status);
    FGNN_LAUNCH_CHECK();
    return 0;
}
