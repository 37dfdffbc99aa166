// What the pairwise-exchange searches share (qap_2opt.hip: both instantiations; qap_2opt_weighted.hip): the check of the start
// matching, the write-out of a refused one, the meeting that finds the first improving pair of a scan, and SciPy's evaluation
// count.  One workgroup of T threads per pair; a scan key is (i << 8) | j < 2^16 for the pair of scan ranks i < j.
#pragma once
#include "fgnn_rows.h"

namespace {

constexpr unsigned SEARCH_NONE = 0xffffffffu;  // no improving pair

// pl[0 .. R) = assign on the corner (-1 past it); *bad_s = 1 unless it is a permutation of [0, n).  Ends WITHOUT a barrier: the
// caller meets once more before it reads *bad_s (and may flag more reasons to refuse before that meeting).
template <int T>
DEVI void load_start(int *pl, int *cnt, int *bad_s, const int *pi, int n, int R, int tid) {
    for (int m = tid; m < R; m += T) {
        pl[m] = -1;
        cnt[m] = 0;
    }
    if (tid == 0) *bad_s = 0;
    __syncthreads();
    for (int k = tid; k < n; k += T) {
        const int p = pi[k];
        if (p >= 0 && p < n) {
            pl[k] = p;
            atomicAdd(&cnt[p], 1);
        } else {
            *bad_s = 1;
        }
    }
    __syncthreads();
    for (int m = tid; m < n; m += T)
        if (cnt[m] != 1) *bad_s = 1;
}

// a refused start goes out as it came in: perm = assign on the corner, -1 past it
template <int T>
DEVI void refuse_start(int *po, const int *pi, int n, int N, int tid) {
    for (int k = tid; k < N; k += T) po[k] = k < n ? pi[k] : -1;
}

// One meeting of the workgroup: the minimum of `best` and every thread's key, in every thread.  Wave butterfly, then the waves'
// minima through red[0 .. WAVES); the caller alternates between two such rows, so the next meeting needs no second barrier.
// (The parity stays with the caller, by value: handed in by reference it changed the code of the scan loop around the call.)
template <int WAVES>
DEVI unsigned first_key(unsigned key, unsigned best, unsigned *red, int tid) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) key = min(key, (unsigned)__shfl_xor((int)key, o));
    if ((tid & 63) == 0) red[tid >> 6] = key;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < WAVES; ++w) best = min(best, red[w]);
    return best;
}

// SciPy's evaluation count over a scan of n rows: the 1-based position of the pair (i, j), i < j, and a whole scan
DEVI long long scan_position(int i, int j, int n) { return (long long)i * n - (long long)i * (i - 1) / 2 + (j - i) + 1; }
DEVI long long full_scan(int n) { return (long long)n * (n + 1) / 2; }

}  // namespace
