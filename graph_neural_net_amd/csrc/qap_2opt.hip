// Pairwise-exchange local search (2-opt) on the bit-packed 0/1 adjacency pairs: the whole search of one pair inside one workgroup
// and one launch.  The semantics are SciPy's _quadratic_assignment_2opt (scipy/optimize/_qap.py) with maximize=True and a full
// partial_guess: S(p) = sum_{i,k} A[i,k] B[p(i),p(k)], the pairs (i, j), i <= j, scanned in the order (0,0), (0,1), .., (0,n-1),
// (1,1), ..; the first pair whose exchange p(i) <-> p(j) raises S is applied and the scan starts over; a scan without such a pair
// ends the search.  "The first improving pair in scan order" is the minimum of (i, j) over the pairs with a positive gain, so a
// round is: all gains in parallel, one min-reduction, one exchange.  Everything is integer arithmetic: perm, qap, swaps and the
// evaluation count nit are those of the serial loop.
//
// With Bp[a] bit k = B[p(a)][p(k)] the objective is S = sum_a popc(A[a] & Bp[a]), and the exchange of i and j swaps rows i, j and
// bit columns i, j of Bp.  Four bit matrices live in LDS -- A, At, Bp, Bpt (t: the bit transpose; nothing assumes A or B symmetric
// or zero on the diagonal) -- beside row_s[a] = popc(A[a] & Bp[a]) and col_s[a] = popc(At[a] & Bpt[a]).  The gain of (i, j), i < j:
//     rows i, j:            popc(A[i] & Bp[j]) + popc(A[j] & Bp[i]) - row_s[i] - row_s[j]          (with bits i, j of Bp's rows swapped)
//     columns i, j, other rows: popc(At[i] & Bpt[j]) + popc(At[j] & Bpt[i]) - col_s[i] - col_s[j]  (without rows i, j)
// and the eight terms the two lines get wrong at the four crossings (i,i), (i,j), (j,i), (j,j) add up to
//     (A[i][i] + A[j][j] - A[i][j] - A[j][i]) (Bp[i][i] + Bp[j][j] - Bp[i][j] - Bp[j][i]).
// 4 NW popcounts per pair (NW words per bit row); an accepted exchange touches two words of every row of Bp and Bpt.
// The pairs i < j are taken QAP_THREADS at a time in scan order (a pair (i,i) never improves: it only counts in nit), and the
// workgroup meets every OPT_PER of them per thread: the first meeting that holds an improving pair holds the first one.
// Rows have an odd pitch: lanes read rows j at lane-dependent words.
//
// Seeds (fgnn_qap_2opt_seeded) are the SEEDED instantiation of the same kernel body: the search over the free rows only, SciPy's
// scan over combinations_with_replacement(i_free, 2).  fr[r] = the r-th free row (ascending) is the rank table, f their number:
// the scan walks the rank pairs (ri, rj), ri < rj, in the order above with n := f and exchanges rows fr[ri], fr[rj]; ascending
// ranks are ascending rows, so the smallest key (ri << 8) | rj is still the first improving pair of SciPy's scan, and its 1-based
// position is ri f - ri (ri - 1) / 2 + (rj - ri) + 1.  Without seeds f = n and the rank of a row is the row, at compile time: no
// table exists and none is read.  The gains, the exchange and the round bound n^2 do not know about seeds.
#include "fgnn_qap_bits.h"
#include "fgnn_qap_search.h"

namespace {

constexpr int OPT_PER = 4;                     // pairs per thread between two meetings of the workgroup

template <int NW>
DEVI int exchange_gain(const unsigned *a, const unsigned *at, const unsigned *bp, const unsigned *bpt, const int *row_s, const int *col_s,
                       int i, int j) {
    constexpr int P = NW | 1;
    const unsigned *ai = a + i * P, *aj = a + j * P, *bi = bp + i * P, *bj = bp + j * P;
    const unsigned *ati = at + i * P, *atj = at + j * P, *bti = bpt + i * P, *btj = bpt + j * P;
    int g = -(row_s[i] + row_s[j] + col_s[i] + col_s[j]);
#pragma unroll
    for (int w = 0; w < NW; ++w)
        g += __popc(ai[w] & bj[w]) + __popc(aj[w] & bi[w]) + __popc(ati[w] & btj[w]) + __popc(atj[w] & bti[w]);
    const int wi = i >> 5, si = i & 31, wj = j >> 5, sj = j & 31;
    const int da = (int)((ai[wi] >> si) & 1u) + (int)((aj[wj] >> sj) & 1u) - (int)((ai[wj] >> sj) & 1u) - (int)((aj[wi] >> si) & 1u);
    const int db = (int)((bi[wi] >> si) & 1u) + (int)((bj[wj] >> sj) & 1u) - (int)((bi[wj] >> sj) & 1u) - (int)((bj[wi] >> si) & 1u);
    return g + da * db;
}

// One workgroup per pair.  LDS (NW = 8): five matrices of 256 x 9 words (the fifth stages B and Bt for the gather) + 4 KB = 50 KB;
// SEEDED adds the rank table (1 KB).  seeds is not read when !SEEDED (it comes last: the other arguments keep their places).
template <int NW, bool SEEDED>
__global__ __launch_bounds__(QAP_THREADS) void qap_2opt_kernel(const unsigned *bits1, const unsigned *bits2, const int *assign,
                                                               const int *nvalid, int N, int max_swaps, int *perm, int *qap, int *swaps,
                                                               long long *nit, int *status, const int *seeds) {
    constexpr int P = NW | 1, R = 32 * NW, WAVES = QAP_THREADS / 64;
    __shared__ unsigned a_l[R * P], at_l[R * P], bp_l[R * P], bpt_l[R * P], stage[R * P];
    __shared__ int pl[R], cnt[R], row_s[R], col_s[R], fr[SEEDED ? R : 1];
    __shared__ unsigned red[2][WAVES];
    __shared__ int sum_s[WAVES], free_s[SEEDED ? WAVES : 1];
    __shared__ int bad_s;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = corner_of(nvalid, b, N), W = (N + 31) >> 5;
    const unsigned *A = bits1 + (long long)b * N * W, *Bm = bits2 + (long long)b * N * W;
    const int *pi = assign + (long long)b * N;
    int *po = perm + (long long)b * N;

    // pl = assign on the corner (-1 past it), refused unless it is a permutation of [0, n) -- that holds every seed
    load_start<QAP_THREADS>(pl, cnt, &bad_s, pi, n, R, tid);
    int nfree = n;                              // the rows the scan walks, and the row of a scan rank
    const auto row_of = [&](int rank) {
        if constexpr (SEEDED) return fr[rank];
        else return rank;
    };
    if constexpr (SEEDED) {
        const int sd = tid < n ? seeds[(long long)b * N + tid] : 0;    // (n <= QAP_THREADS: thread t owns row t)
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
        refuse_start<QAP_THREADS>(po, pi, n, N, tid);
        if (tid == 0) {
            qap[b] = -1;
            swaps[b] = 0;
            nit[b] = 0;
            status[b] = 2;
        }
        return;
    }

    // A, At; Bp[a] = the gather of B[p(a)] through p, Bpt[a] = the gather of Bt[p(a)] through p
    stage_rows<NW>(a_l, P, A, 0, R, n, W, tid);
    stage_transposed<NW>(at_l, P, A, n, W, tid);
    stage_rows<NW>(stage, P, Bm, 0, R, n, W, tid);
    __syncthreads();
    for (int idx = tid; idx < n * NW; idx += QAP_THREADS) {
        const int r = idx / NW, w = idx - r * NW;
        bp_l[r * P + w] = permuted_word(stage + pl[r] * P, pl, w);
    }
    __syncthreads();
    stage_transposed<NW>(stage, P, Bm, n, W, tid);
    __syncthreads();
    for (int idx = tid; idx < n * NW; idx += QAP_THREADS) {
        const int r = idx / NW, w = idx - r * NW;
        bpt_l[r * P + w] = permuted_word(stage + pl[r] * P, pl, w);
    }
    __syncthreads();
    for (int r = tid; r < n; r += QAP_THREADS) {
        int rs = 0, cs = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            rs += __popc(a_l[r * P + w] & bp_l[r * P + w]);
            cs += __popc(at_l[r * P + w] & bpt_l[r * P + w]);
        }
        row_s[r] = rs;
        col_s[r] = cs;
    }

    // The rounds: a counted loop.  Every exchange raises S <= n^2 by at least 1, so n^2 rounds end any search on their own.
    const int pairs = f * (f - 1) / 2;
    const int bound = max_swaps < 0 ? n * n : min(max_swaps, n * n);
    int done = 0, st = n == 0 ? 0 : 1, par = 0;
    long long evals = 0;
    for (int round = 0; round < bound; ++round) {
        __syncthreads();                        // Bp, Bpt, row_s, col_s of this round
        unsigned best = SEARCH_NONE;
        int i = 0, j = 1 + tid;                 // (rank) pair number tid of the scan without its (i,i)
        for (int base = 0; base < pairs; base += OPT_PER * QAP_THREADS) {       // uniform
            unsigned key = SEARCH_NONE;
#pragma unroll
            for (int c = 0; c < OPT_PER; ++c) {
                while (j >= f && i < f - 1) {   // past the end of row i: on into the next row
                    ++i;
                    j += i + 1 - f;
                }
                if (i < f - 1) {
                    if (exchange_gain<NW>(a_l, at_l, bp_l, bpt_l, row_s, col_s, row_of(i), row_of(j)) > 0)
                        key = min(key, (unsigned)((i << 8) | j));
                    j += QAP_THREADS;
                }
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
        // rows bi, bj of Bp and Bpt change places, then bits bi, bj of every row
        if (tid < 2 * NW) {
            unsigned *m = tid < NW ? bp_l : bpt_l;
            const int w = tid & (NW - 1);
            const unsigned x = m[bi * P + w];
            m[bi * P + w] = m[bj * P + w];
            m[bj * P + w] = x;
        }
        if (tid == QAP_THREADS - 1) {
            const int x = pl[bi];
            pl[bi] = pl[bj];
            pl[bj] = x;
        }
        __syncthreads();
        const int wi = bi >> 5, si = bi & 31, wj = bj >> 5, sj = bj & 31;
        for (int r = tid; r < n; r += QAP_THREADS) {
            unsigned *rows[2] = {bp_l + r * P, bpt_l + r * P};
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const unsigned d = ((rows[q][wi] >> si) ^ (rows[q][wj] >> sj)) & 1u;
                rows[q][wi] ^= d << si;
                rows[q][wj] ^= d << sj;
            }
            int rs = 0, cs = 0;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                rs += __popc(a_l[r * P + w] & bp_l[r * P + w]);
                cs += __popc(at_l[r * P + w] & bpt_l[r * P + w]);
            }
            row_s[r] = rs;
            col_s[r] = cs;
        }
    }
    __syncthreads();

    for (int k = tid; k < N; k += QAP_THREADS) po[k] = k < n ? pl[k] : -1;
    int s = 0;
    for (int r = tid; r < n; r += QAP_THREADS) s += row_s[r];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((tid & 63) == 0) sum_s[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) total += sum_s[w];
        qap[b] = total;
        swaps[b] = done;
        nit[b] = evals;
        status[b] = st;
    }
}

template <int NW, bool SEEDED>
int launch_2opt(const unsigned *bits1, const unsigned *bits2, const int *assign, const int *seeds, const int *nvalid, int B, int N,
                int max_swaps, int *perm, int *qap, int *swaps, long long *nit, int *status, hipStream_t st) {
    hipLaunchKernelGGL((qap_2opt_kernel<NW, SEEDED>), dim3(B), dim3(QAP_THREADS), 0, st, bits1, bits2, assign, nvalid, N, max_swaps, perm,
                       qap, swaps, nit, status, seeds);
    FGNN_LAUNCH_CHECK();
    return 0;
}

// both entry points: `who` names the one in the messages; seeds (may be NULL: the unseeded search) picks the instantiation
int two_opt(const char *who, const unsigned *bits1, const unsigned *bits2, const int *assign, const int *seeds, const int *nvalid, int B,
            int N, int max_swaps, int *perm, int *qap, int *swaps, long long *nit, int *status, void *stream) {
    FGNN_CHECK(bits1 && bits2 && assign && perm && qap && swaps && nit && status && B > 0 && N > 0, "%s: bad arguments", who);
    FGNN_CHECK(N <= FGNN_QAP_MAX_N, "%s: at most %d vertices per graph (got %d)", who, FGNN_QAP_MAX_N, N);
    hipStream_t st = (hipStream_t)stream;
    const auto launch = [&](auto nw) {
        constexpr int NW = decltype(nw)::value;
        return seeds ? launch_2opt<NW, true>(bits1, bits2, assign, seeds, nvalid, B, N, max_swaps, perm, qap, swaps, nit, status, st)
                     : launch_2opt<NW, false>(bits1, bits2, assign, seeds, nvalid, B, N, max_swaps, perm, qap, swaps, nit, status, st);
    };
    if (N <= 32) return launch(std::integral_constant<int, 1>());
    if (N <= 64) return launch(std::integral_constant<int, 2>());
    if (N <= 128) return launch(std::integral_constant<int, 4>());
    return launch(std::integral_constant<int, 8>());
}

}  // namespace

extern "C" int fgnn_qap_2opt_seeded(const unsigned *bits1, const unsigned *bits2, const int *assign, const int *seeds, const int *nvalid,
                                    int B, int N, int max_swaps, int *perm, int *qap, int *swaps, long long *nit, int *status,
                                    void *stream) {
    FGNN_CHECK(seeds, "fgnn_qap_2opt_seeded: bad arguments");
    return two_opt("fgnn_qap_2opt_seeded", bits1, bits2, assign, seeds, nvalid, B, N, max_swaps, perm, qap, swaps, nit, status, stream);
}

extern "C" int fgnn_qap_2opt(const unsigned *bits1, const unsigned *bits2, const int *assign, const int *nvalid, int B, int N, int max_swaps,
                             int *perm, int *qap, int *swaps, long long *nit, int *status, void *stream) {
    return two_opt("fgnn_qap_2opt", bits1, bits2, assign, nullptr, nvalid, B, N, max_swaps, perm, qap, swaps, nit, status, stream);
}
