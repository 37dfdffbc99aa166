// Seeds from a model's scores (include/fgnn_hip.h, "confident seeds"): the rows whose best column picks them back with a clear
// margin become the seed vector of the seeded solvers (csrc/qap_seeds.hip), and a meter says what those seeds were worth.
//   fgnn_confident_seeds : scores -> seeds, nseeds, margin.  One workgroup per pair, ONE pass over the matrix: wave w takes the
//                          rows w, w + 4, ... in ascending order, lane l the columns l, l + 64, l + 128, l + 192 of each, so a row
//                          read is coalesced along j.  The row's arg-max, runner-up and NaN flag meet by a butterfly; the same
//                          loads feed the lane's running column maxima (registers), which the four waves fold in LDS in wave order.
//                          Selection is rank by counting over the candidates' margins in LDS: no sort, no atomics.
//   fgnn_seed_fold(_bins): per pair the seeds that are right and the free rows the matchings got right, added to an all-int64
//                          fgnn_seed_record by one workgroup in pair order -- qap_fold_kernel's build (csrc/qap_fold.hip).
// All are plain launches on the caller's stream: capturable, no allocation, no copy, no synchronisation.
#include "fgnn_rows.h"

namespace {

constexpr int CS_THREADS = 256;            // = FGNN_SEED_MAX_N: a thread per row / column in the tail
constexpr int CS_WAVES = CS_THREADS / WAVE;
constexpr int CS_COLS = FGNN_SEED_MAX_N / WAVE;        // columns a lane owns
constexpr int NO_INDEX = 0x7fffffff;

// a beats b in the arg-max order: the larger value, the smaller index on ties (-0.0 == +0.0).  No NaN reaches this: the passes
// read a NaN as -inf and flag its row and column instead.
DEVI bool beats(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }

__global__ __launch_bounds__(CS_THREADS) void confident_seeds_kernel(const float *scores, long long bstride, int ld, const int *nvalid,
                                                                     int N, int count, float min_margin, int *seeds, int *nseeds,
                                                                     float *margin) {
    __shared__ float col_best[CS_WAVES][CS_THREADS];       // per wave: the maximum of column j over the wave's rows
    __shared__ int col_row[CS_WAVES][CS_THREADS];          //           its first row, NO_INDEX without a row
    __shared__ int col_nan[CS_WAVES][CS_THREADS];
    __shared__ int row_col[CS_THREADS], col_pick[CS_THREADS], cand[CS_THREADS];
    __shared__ float row_margin[CS_THREADS];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & (WAVE - 1), wave = t / WAVE;
    const int n = corner_of(nvalid, b, N);
    const float *S = scores + (long long)b * bstride;

    float cbest[CS_COLS];
    int crow[CS_COLS], cnan[CS_COLS];
#pragma unroll
    for (int c = 0; c < CS_COLS; ++c) {
        cbest[c] = -INFINITY;
        crow[c] = NO_INDEX;
        cnan[c] = 0;
    }
    for (int i = wave; i < n; i += CS_WAVES) {             // (uniform in the wave)
        const float *row = S + (long long)i * ld;
        float best = -INFINITY, second = -INFINITY;
        int bj = NO_INDEX, bad = 0;
#pragma unroll
        for (int c = 0; c < CS_COLS; ++c) {                // ascending j: an equal later value never replaces
            const int j = lane + c * WAVE;
            if (j < n) {
                float v = row[j];
                if (v != v) {
                    bad = 1;
                    cnan[c] = 1;
                    v = -INFINITY;
                }
                if (bj == NO_INDEX || v > best) {
                    second = bj == NO_INDEX ? second : best;
                    best = v;
                    bj = j;
                } else {
                    second = fmaxf(second, v);
                }
                if (crow[c] == NO_INDEX || v > cbest[c]) { // ascending i
                    cbest[c] = v;
                    crow[c] = i;
                }
            }
        }
#pragma unroll
        for (int o = WAVE / 2; o > 0; o >>= 1) {           // the winner keeps its index, the runner-up is the best of the rest
            const float ob = __shfl_xor(best, o), os = __shfl_xor(second, o);
            const int oj = __shfl_xor(bj, o);
            bad |= __shfl_xor(bad, o);
            const bool take = beats(ob, oj, best, bj);
            second = fmaxf(fmaxf(second, os), take ? best : ob);
            best = take ? ob : best;
            bj = take ? oj : bj;
        }
        if (lane == 0) {
            const bool ok = !bad && best > -INFINITY && best < INFINITY;
            row_col[i] = bj;
            row_margin[i] = ok ? best - second : -INFINITY;   // one fp32 subtraction; +inf for n = 1
        }
    }
#pragma unroll
    for (int c = 0; c < CS_COLS; ++c) {
        col_best[wave][lane + c * WAVE] = cbest[c];
        col_row[wave][lane + c * WAVE] = crow[c];
        col_nan[wave][lane + c * WAVE] = cnan[c];
    }
    __syncthreads();
    {                                                       // thread t owns column t: the waves in order
        float best = col_best[0][t];
        int br = col_row[0][t], bad = col_nan[0][t];
#pragma unroll
        for (int w = 1; w < CS_WAVES; ++w) {
            const float ov = col_best[w][t];
            const int orow = col_row[w][t];
            bad |= col_nan[w][t];
            if (beats(ov, orow, best, br)) {
                best = ov;
                br = orow;
            }
        }
        col_pick[t] = (t < n && !bad) ? br : -1;
    }
    __syncthreads();
    const int c = t < n ? row_col[t] : 0;
    const float m = t < n ? row_margin[t] : 0.f;
    const bool is_cand = t < n && col_pick[c] == t && m >= min_margin;
    cand[t] = is_cand ? 1 : 0;
    __syncthreads();
    int before = 0;
    for (int k = 0; k < n; ++k) {                          // rank by counting: broadcast reads, integer adds
        const float mk = row_margin[k];
        before += cand[k] && (mk > m || (mk == m && k < t)) ? 1 : 0;
    }
    const bool kept = is_cand && (count < 0 || before < count);
    const int total = __syncthreads_count(kept);
    if (t < N) {
        const long long at = (long long)b * N + t;
        seeds[at] = kept ? c : -1;
        if (margin) margin[at] = m;
    }
    if (t == 0) nseeds[b] = total;
}

constexpr int SFOLD_THREADS = 256;

// qap_fold_kernel's build: wave w takes the pairs 4 c + w of chunk c and counts over the rows l, l + 64, ... of the pair; the wave
// meets by a butterfly and leaves the pair's integers in LDS; thread k < K owns record k and adds the chunk's pairs below `live`
// of its bin in pair order.  Integer sums only: the bytes of a record do not depend on how an epoch was cut into calls.
template <bool BINS>
__global__ __launch_bounds__(SFOLD_THREADS) void seed_fold_kernel(const int *seeds, const int *assign, const int *perm, const int *labels,
                                                                  const int *nvalid, int B, int N, int live, const int *bin, int K,
                                                                  fgnn_seed_record *records) {
    __shared__ int s_n[SFOLD_THREADS / WAVE], s_m[SFOLD_THREADS / WAVE], s_sc[SFOLD_THREADS / WAVE], s_fc[SFOLD_THREADS / WAVE],
        s_frc[SFOLD_THREADS / WAVE];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const bool owner = BINS ? (int)threadIdx.x < K : threadIdx.x == 0;
    long long n_seeds = 0, seed_correct = 0, free_nodes = 0, free_correct = 0, free_refined = 0, clean = 0, exact_free = 0, nodes = 0,
              pairs = 0;
    for (int b0 = 0; b0 < live; b0 += SFOLD_THREADS / WAVE) {        // (uniform bounds: every thread meets every barrier)
        const int b = b0 + wave;
        if (b < live) {
            const int n = clamp_nv(nvalid, b, N);
            int m = 0, sc = 0, fc = 0, frc = 0;
            for (int i = lane; i < n; i += WAVE) {
                const long long at = (long long)b * N + i;
                const int s = seeds ? seeds[at] : -1;
                const int t = labels ? labels[at] : i;
                const bool has = t >= 0 && t < n, seeded = s >= 0;
                m += seeded ? 1 : 0;
                sc += seeded && has && s == t ? 1 : 0;
                fc += !seeded && has && assign[at] == t ? 1 : 0;
                if (perm) frc += !seeded && has && perm[at] == t ? 1 : 0;
            }
            for (int o = 32; o > 0; o >>= 1) {
                m += __shfl_xor(m, o);
                sc += __shfl_xor(sc, o);
                fc += __shfl_xor(fc, o);
                frc += __shfl_xor(frc, o);
            }
            if (lane == 0) {
                s_n[wave] = n;
                s_m[wave] = m;
                s_sc[wave] = sc;
                s_fc[wave] = fc;
                s_frc[wave] = frc;
            }
        }
        __syncthreads();
        if (owner) {
            for (int w = 0; w < SFOLD_THREADS / WAVE && b0 + w < live; ++w) {
                if (BINS && bin[b0 + w] != (int)threadIdx.x) continue;
                const int n = s_n[w], m = s_m[w];
                nodes += n;
                pairs += 1;
                n_seeds += m;
                seed_correct += s_sc[w];
                free_nodes += n - m;
                free_correct += s_fc[w];
                if (perm) free_refined += s_frc[w];
                clean += s_sc[w] == m ? 1 : 0;
                exact_free += (perm ? s_frc[w] : s_fc[w]) == n - m ? 1 : 0;
            }
        }
        __syncthreads();
    }
    if (owner && (BINS ? pairs > 0 : live > 0)) {          // (a plain fold took a pair exactly when live > 0)
        fgnn_seed_record *meter = records + (BINS ? threadIdx.x : 0);
        meter->seeds += n_seeds;
        meter->seed_correct += seed_correct;
        meter->free_nodes += free_nodes;
        meter->free_correct += free_correct;
        if (perm) meter->free_refined_correct += free_refined;       // without a final matching the field is not touched
        meter->clean_pairs += clean;
        meter->exact_free += exact_free;
        meter->nodes += nodes;
        meter->pairs += pairs;
        meter->steps += 1;
    }
}

}  // namespace

extern "C" int fgnn_confident_seeds(const float *scores, long long bstride, int ld, const int *nvalid, int B, int N, int count,
                                    float min_margin, int *seeds, int *nseeds, float *margin, void *stream) {
    FGNN_CHECK(scores && seeds && nseeds && B > 0 && N > 0, "fgnn_confident_seeds: bad arguments");
    FGNN_CHECK(N <= FGNN_SEED_MAX_N, "fgnn_confident_seeds: at most %d vertices per graph (got %d)", FGNN_SEED_MAX_N, N);
    FGNN_CHECK(ld >= N && bstride >= (long long)N * ld, "fgnn_confident_seeds: score strides smaller than the matrices");
    FGNN_CHECK(min_margin >= 0.f, "fgnn_confident_seeds: min_margin must be >= 0 (and no NaN)");
    hipLaunchKernelGGL(confident_seeds_kernel, dim3(B), dim3(CS_THREADS), 0, (hipStream_t)stream, scores, bstride, ld, nvalid, N, count,
                       min_margin, seeds, nseeds, margin);
    FGNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int fgnn_seed_fold(const int *seeds, const int *assign, const int *perm, const int *labels, const int *nvalid, int B, int N,
                              int live, fgnn_seed_record *meter, void *stream) {
    FGNN_CHECK(assign && meter && B > 0 && N > 0, "fgnn_seed_fold: bad arguments");
    FGNN_CHECK(live >= 0 && live <= B, "fgnn_seed_fold: live = %d outside [0, %d]", live, B);
    hipLaunchKernelGGL(seed_fold_kernel<false>, dim3(1), dim3(SFOLD_THREADS), 0, (hipStream_t)stream, seeds, assign, perm, labels, nvalid,
                       B, N, live, (const int *)NULL, 1, meter);
    FGNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int fgnn_seed_fold_bins(const int *seeds, const int *assign, const int *perm, const int *labels, const int *nvalid, int B,
                                   int N, int live, const int *bin, int K, fgnn_seed_record *records, void *stream) {
    FGNN_CHECK(assign && bin && records && B > 0 && N > 0, "fgnn_seed_fold_bins: bad arguments");
    FGNN_CHECK(live >= 0 && live <= B, "fgnn_seed_fold_bins: live = %d outside [0, %d]", live, B);
    FGNN_CHECK(K >= 1 && K <= FGNN_MAX_LEVELS, "fgnn_seed_fold_bins: K = %d records outside [1, %d]", K, FGNN_MAX_LEVELS);
    hipLaunchKernelGGL(seed_fold_kernel<true>, dim3(1), dim3(SFOLD_THREADS), 0, (hipStream_t)stream, seeds, assign, perm, labels, nvalid,
                       B, N, live, bin, K, records);
    FGNN_LAUNCH_CHECK();
    return 0;
}
