// Pairwise-exchange local search (2-opt) on REAL-weighted pairs: the fp32 twin of qap_2opt.hip, with the addressing of qap_weighted.hip
// (fp32 matrices, row pitch ld, pairs gstride floats apart, only the n_b x n_b corner is ever read).  The whole search of one pair
// runs inside one workgroup and one launch.  The semantics are SciPy's _quadratic_assignment_2opt with maximize=True and a full
// partial_guess: S(p) = sum_{i,k} A[i,k] B[p(i),p(k)]; the pairs (i, j), i <= j, are scanned in the order (0,0), (0,1), .., (0,n-1),
// (1,1), ..; the first pair with a positive gain is exchanged and the scan starts over; a scan without such a pair ends the search.
// A round is: all gains in parallel, one min-reduction over the scan position, one exchange.
//
// With Bp[a][k] = B[p(a)][p(k)] the gain of exchanging i < j is
//     sum_{k != i,j} (A[i,k] - A[j,k]) (Bp[j,k] - Bp[i,k])                                     rows i, j
//   + sum_{k != i,j} (A[k,i] - A[k,j]) (Bp[k,j] - Bp[k,i])                                     columns i, j
//   + (A[i,i] - A[j,j]) (Bp[j,j] - Bp[i,i]) + (A[i,j] - A[j,i]) (Bp[j,i] - Bp[i,j])            the four crossings
// evaluated by ONE fmaf chain per pair: k ascending, the row term before the column term, then the two crossings.  The order
// depends on (A, Bp, i, j) only and no gain state survives a round: an exchange swaps rows i, j and columns i, j of Bp (and p(i),
// p(j)), nothing else changes, so nothing drifts.  Every term is a difference times a difference, so the gain of undoing an exchange
// is the exact negative of the gain that made it: no two-cycle on rounding noise.  A pair is accepted iff its fp32 gain is > 0.
// On integer or dyadic weights whose partial sums stay below 2^24 units every gain is exact and perm, swaps, nit are SciPy's.
// Nothing assumes A or B symmetric or zero on the diagonal.
//
// Termination is a property of the code: the round loop is counted (max_swaps rounds, n^2 without a limit) and a start that is no
// permutation of the corner is refused before it.  With real weights the n^2 bound can bind: that is status 1.
//
// N <= 128: A and Bp live in LDS with an odd pitch (lanes read rows j at lane-dependent offsets), three sizes (32, 64, 128 rows) so
// that small pairs share a CU.  128 < N <= 256: Bp lives in the caller's workspace (N x N floats per pair), A is read in place.
//
// Seeds (fgnn_qapw_2opt_seeded) are the SEEDED instantiation of the same kernel body, built as qap_2opt.hip builds its own: the
// search over the free rows only, SciPy's scan over combinations_with_replacement(i_free, 2).  fr[r] = the r-th free row
// (ascending) is the rank table, f their number: the scan walks the rank pairs (ri, rj), ri < rj, in the order above with n := f
// and exchanges rows and columns fr[ri], fr[rj]; ascending ranks are ascending rows, so the smallest key (ri << 8) | rj is still
// the first improving pair of SciPy's scan, and nit counts positions among the free rows.  Without seeds f = n and the rank of a
// row is the row, at compile time: no table exists and none is read.  The gain chain (all n terms of it: seeded rows and columns
// are part of the objective), the exchange, the round bound n^2 and the refusal of a start that is no permutation do not know
// about seeds.
#include "fgnn_qap_search.h"

namespace {

constexpr int OPTW_LDS_MAX_N = 128;            // beyond: Bp in the workspace
constexpr long long OPTW_WS_ALIGN = 256;
constexpr int OPTW_MAX_B = 65535;              // pairs ride on a grid dimension

// a, bp: row pitches pa, pb.  One chain, k ascending (see above).
DEVI float exchange_gain(const float *a, int pa, const float *bp, int pb, int n, int i, int j) {
    const float *ai = a + i * pa, *aj = a + j * pa, *bi = bp + i * pb, *bj = bp + j * pb;
    float g = 0.f;
    for (int k = 0; k < n; ++k) {
        float t = fmaf(ai[k] - aj[k], bj[k] - bi[k], g);
        t = fmaf(a[k * pa + i] - a[k * pa + j], bp[k * pb + j] - bp[k * pb + i], t);
        g = (k == i || k == j) ? g : t;
    }
    g = fmaf(ai[i] - aj[j], bj[j] - bi[i], g);
    return fmaf(ai[j] - aj[i], bj[i] - bi[j], g);
}

// One workgroup of T threads per pair.  R: rows the LDS matrices hold (LDS variant), else the largest n (R = 256, Bp in ws).
// T >= R in every variant: thread t owns row t where the rank table is built.  SEEDED adds the rank table fr (R ints) and
// free_s, one count per wave.  The R = 128 variant then holds 2 x 128 x 129 floats (132 096 B) + pl, cnt (1 024 B) + fr (512 B) +
// free_s (64 B) + red (128 B) + bad_s (4 B) = 133 828 B, the compiler's figure (133 252 B without seeds): under the CU's 160 KB
// (163 840 B), one workgroup per CU as before.  seeds is not read when !SEEDED (it comes last: the other
// arguments keep their places).
template <int R, int T, bool IN_LDS, bool SEEDED>
__global__ __launch_bounds__(T) void qapw_2opt_kernel(const float *a1, const float *a2, long long gstride, int ld, const int *assign,
                                                      const int *nvalid, int N, int max_swaps, float *ws, int *perm, int *swaps,
                                                      long long *nit, int *status, const int *seeds) {
    constexpr int P = R | 1, WAVES = T / 64, CELLS = IN_LDS ? R * P : 1;
    static_assert(T >= R, "thread t owns row t of the rank table");
    __shared__ float a_l[CELLS], bp_l[CELLS];
    __shared__ int pl[R], cnt[R], fr[SEEDED ? R : 1];
    __shared__ unsigned red[2][WAVES];
    __shared__ int free_s[SEEDED ? WAVES : 1];
    __shared__ int bad_s;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = corner_of(nvalid, b, N);
    const float *A = a1 + (long long)b * gstride, *Bm = a2 + (long long)b * gstride;
    const int *pi = assign + (long long)b * N;
    int *po = perm + (long long)b * N;

    // pl = assign on the corner (-1 past it), refused unless it is a permutation of [0, n) -- that holds every seed
    load_start<T>(pl, cnt, &bad_s, pi, n, R, tid);
    int nfree = n;                              // the rows the scan walks, and the row of a scan rank
    const auto row_of = [&](int rank) {
        if constexpr (SEEDED) return fr[rank];
        else return rank;
    };
    if constexpr (SEEDED) {
        const int sd = tid < n ? seeds[(long long)b * N + tid] : 0;    // (n <= R <= T: thread t owns row t)
        const bool is_free = tid < n && sd < 0;
        if (tid < n && sd >= 0 && pl[tid] != sd) bad_s = 1;
        // the rank table: ballot and prefix counts, the waves in order
        const unsigned long long fm = __ballot(is_free);
        if ((tid & 63) == 0) free_s[tid >> 6] = __popcll(fm);
        __syncthreads();
        int rank = __popcll(fm & ((1ull << (tid & 63)) - 1ull));
        nfree = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            rank += w < (tid >> 6) ? free_s[w] : 0;
            nfree += free_s[w];
        }
        if (is_free) fr[rank] = tid;
    }
    const int f = nfree;
    __syncthreads();
    if (bad_s) {                                // uniform
        refuse_start<T>(po, pi, n, N, tid);
        if (tid == 0) {
            swaps[b] = 0;
            nit[b] = 0;
            status[b] = 2;
        }
        return;
    }

    // a, bp: the matrices the gains read.  Bp[r][k] = B[p(r)][p(k)]; only the corner is read, only the corner is written.
    const float *a;
    float *bp;
    int pa, pb;
    if constexpr (IN_LDS) {
        a = a_l, bp = bp_l, pa = P, pb = P;
        for (int idx = tid; idx < n * n; idx += T) {
            const int r = idx / n, k = idx - r * n;
            a_l[r * P + k] = A[(long long)r * ld + k];
        }
    } else {
        a = A, bp = ws + (long long)b * N * N, pa = ld, pb = N;
    }
    for (int idx = tid; idx < n * n; idx += T) {
        const int r = idx / n, k = idx - r * n;
        bp[r * pb + k] = Bm[(long long)pl[r] * ld + pl[k]];
    }

    // The rounds: a counted loop.
    const int pairs = f * (f - 1) / 2;
    const int bound = max_swaps < 0 ? n * n : min(max_swaps, n * n);
    int done = 0, st = n == 0 ? 0 : 1, par = 0;
    long long evals = 0;
    for (int round = 0; round < bound; ++round) {
        __syncthreads();                        // Bp of this round
        unsigned best = SEARCH_NONE;
        int i = 0, j = 1 + tid;                 // (rank) pair number tid of the scan without its (i,i)
        for (int base = 0; base < pairs; base += T) {       // uniform: T pairs in scan order between two meetings
            unsigned key = SEARCH_NONE;
            while (j >= f && i < f - 1) {       // past the end of row i: on into the next row
                ++i;
                j += i + 1 - f;
            }
            if (i < f - 1) {
                if (exchange_gain(a, pa, bp, pb, n, row_of(i), row_of(j)) > 0.f) key = (unsigned)((i << 8) | j);
                j += T;
            }
            best = first_key<WAVES>(key, best, red[par], tid);
            par ^= 1;                           // (the next meeting writes the other half: no second barrier)
            if (best != SEARCH_NONE) break;     // uniform
        }
        if (best == SEARCH_NONE) {              // a whole scan without an improving pair
            evals += full_scan(f);
            st = 0;
            break;
        }
        const int ri = (int)(best >> 8), rj = (int)(best & 255u), bi = row_of(ri), bj = row_of(rj);
        evals += scan_position(ri, rj, f);
        ++done;
        // rows bi, bj of Bp change places, then columns bi, bj
        for (int k = tid; k < n; k += T) {
            const float x = bp[bi * pb + k];
            bp[bi * pb + k] = bp[bj * pb + k];
            bp[bj * pb + k] = x;
        }
        if (tid == T - 1) {
            const int x = pl[bi];
            pl[bi] = pl[bj];
            pl[bj] = x;
        }
        __syncthreads();
        for (int r = tid; r < n; r += T) {
            const float x = bp[r * pb + bi];
            bp[r * pb + bi] = bp[r * pb + bj];
            bp[r * pb + bj] = x;
        }
    }
    __syncthreads();

    for (int k = tid; k < N; k += T) po[k] = k < n ? pl[k] : -1;
    if (tid == 0) {
        swaps[b] = done;
        nit[b] = evals;
        status[b] = st;
    }
}

template <int R, int T, bool IN_LDS, bool SEEDED>
int launch_2optw(const float *a1, const float *a2, long long gstride, int ld, const int *assign, const int *seeds, const int *nvalid, int B,
                 int N, int max_swaps, float *ws, int *perm, int *swaps, long long *nit, int *status, hipStream_t st) {
    hipLaunchKernelGGL((qapw_2opt_kernel<R, T, IN_LDS, SEEDED>), dim3(B), dim3(T), 0, st, a1, a2, gstride, ld, assign, nvalid, N, max_swaps,
                       ws, perm, swaps, nit, status, seeds);
    FGNN_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" long long fgnn_qapw_2opt_ws_bytes(int B, int N) {
    if (B <= 0 || N <= OPTW_LDS_MAX_N) return 0;
    return ((long long)B * N * N * 4 + OPTW_WS_ALIGN - 1) / OPTW_WS_ALIGN * OPTW_WS_ALIGN;
}

namespace {

// both entry points: `who` names the one in the messages; seeds (may be NULL: the unseeded search) picks the instantiation
int two_opt_w(const char *who, const float *a1, const float *a2, long long gstride, int ld, const int *assign, const int *seeds,
              const int *nvalid, int B, int N, int max_swaps, void *ws, long long ws_bytes, int *perm, int *swaps, long long *nit,
              int *status, void *stream) {
    FGNN_CHECK(a1 && a2 && assign && perm && swaps && nit && status && B > 0 && N > 0, "%s: bad arguments", who);
    FGNN_CHECK(N <= FGNN_QAPW_MAX_N, "%s: at most %d vertices per graph (got %d)", who, FGNN_QAPW_MAX_N, N);
    FGNN_CHECK(B <= OPTW_MAX_B, "%s: at most %d pairs per call (got %d)", who, OPTW_MAX_B, B);
    FGNN_CHECK(ld >= N && gstride >= (long long)N * ld, "%s: ld / gstride smaller than the matrices", who);
    hipStream_t st = (hipStream_t)stream;
    const auto launch = [&](auto r, auto t, auto in_lds, float *w) {
        constexpr int R = decltype(r)::value, T = decltype(t)::value;
        constexpr bool IN_LDS = decltype(in_lds)::value;
        return seeds ? launch_2optw<R, T, IN_LDS, true>(a1, a2, gstride, ld, assign, seeds, nvalid, B, N, max_swaps, w, perm, swaps, nit,
                                                        status, st)
                     : launch_2optw<R, T, IN_LDS, false>(a1, a2, gstride, ld, assign, seeds, nvalid, B, N, max_swaps, w, perm, swaps, nit,
                                                         status, st);
    };
    using std::integral_constant;
    if (N <= 32) return launch(integral_constant<int, 32>(), integral_constant<int, 256>(), std::true_type(), nullptr);
    if (N <= 64) return launch(integral_constant<int, 64>(), integral_constant<int, 512>(), std::true_type(), nullptr);
    if (N <= OPTW_LDS_MAX_N) return launch(integral_constant<int, 128>(), integral_constant<int, 1024>(), std::true_type(), nullptr);
    FGNN_CHECK(ws && ws_bytes >= fgnn_qapw_2opt_ws_bytes(B, N) && ((uintptr_t)ws & 15) == 0,
               "%s: the workspace needs %lld bytes, 16-byte aligned (got %lld)", who, fgnn_qapw_2opt_ws_bytes(B, N), ws_bytes);
    return launch(integral_constant<int, 256>(), integral_constant<int, 1024>(), std::false_type(), (float *)ws);
}

}  // namespace

extern "C" int fgnn_qapw_2opt_seeded(const float *a1, const float *a2, long long gstride, int ld, const int *assign, const int *seeds,
                                     const int *nvalid, int B, int N, int max_swaps, void *ws, long long ws_bytes, int *perm, int *swaps,
                                     long long *nit, int *status, void *stream) {
    FGNN_CHECK(seeds, "fgnn_qapw_2opt_seeded: bad arguments");
    return two_opt_w("fgnn_qapw_2opt_seeded", a1, a2, gstride, ld, assign, seeds, nvalid, B, N, max_swaps, ws, ws_bytes, perm, swaps, nit,
                     status, stream);
}

extern "C" int fgnn_qapw_2opt(const float *a1, const float *a2, long long gstride, int ld, const int *assign, const int *nvalid, int B,
                              int N, int max_swaps, void *ws, long long ws_bytes, int *perm, int *swaps, long long *nit, int *status,
                              void *stream) {
    return two_opt_w("fgnn_qapw_2opt", a1, a2, gstride, ld, assign, nullptr, nvalid, B, N, max_swaps, ws, ws_bytes, perm, swaps, nit, status,
                     stream);
}
