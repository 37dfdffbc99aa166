// Rank metrics on the device (include/fgnn_hip.h, "evaluation"): where the true match of a row stands among the row's scores, and
// the Hits@k / reciprocal-rank sums of an epoch -- what the arg-max hit of csrc/eval.hip cannot say about a row it got wrong.
//   fgnn_eval_ranks : ONE pass over the scores: per valid row the rank of its target column (1 = the arg-max of eval_pairs_kernel).
//   fgnn_rank_fold  : per-pair sums of those rows and the add into the epoch record(s), by one workgroup in a fixed order.
// Both are plain launches on the caller's stream: capturable, no allocation, no copy, no synchronisation.
#include "fgnn_rows.h"

namespace {

constexpr int RANK_THREADS = 256;

// The row grouping of eval_pairs_kernel (fgnn_rows.h); lane `sub` of a row's group counts among the columns sub, sub + W, ...
// those that BEAT the target column t:
//   s_j is NaN and s_t is not;  s_j > s_t;  j < t and (s_j == s_t or both are NaN)
// -- the order of row_argmax (first maximum on ties, NaN above every number, the first NaN wins, -0.0 == +0.0), so
// rank == 1 exactly when that kernel's row_hit is 1.  Column t itself beats nothing (s_t == s_t needs j < t).  The counts are integers: the
// butterfly's order is free and the result exact.
template <int W>
__global__ __launch_bounds__(RANK_THREADS) void eval_ranks_kernel(const float *scores, long long bstride, int ld, const int *nvalid,
                                                                  const int *labels, int B, int N, int *rank) {
    const int sub = threadIdx.x & (W - 1);
    const long long t = (long long)blockIdx.x * (RANK_THREADS / W) + threadIdx.x / W;      // row index over (b, i)
    const bool inside = t < (long long)B * N;
    const long long tc = inside ? t : 0;
    const int b = (int)(tc / N), i = (int)(tc - (long long)b * N);
    const int nb = clamp_nv(nvalid, b, N);
    const bool live = inside && i < nb;                  // (uniform inside a row's group)
    const int tgt = live ? (labels ? labels[tc] : i) : -1;
    const bool has = tgt >= 0 && tgt < nb;               // dead groups and rows without a target run the butterflies on empty rows
    const int n = has ? nb : 0;
    const float *row = scores + (long long)b * bstride + (long long)i * ld;
    const float st = has ? row[tgt] : 0.f;               // one broadcast load
    const bool tnan = st != st;

    int count = 0;
    for (int j = sub; j < n; j += W) {
        const float v = row[j];
        const bool vnan = v != v;
        const bool beats = tnan ? (vnan && j < tgt) : (vnan || v > st || (v == st && j < tgt));
        count += beats ? 1 : 0;
    }
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) count += __shfl_xor(count, o);
    if (live && sub == 0) rank[t] = has ? 1 + count : 0;
}

struct RankKs {
    int k[FGNN_RANK_MAX_K];          // thresholds past nk are 0: no rank >= 1 lies below them
};

// The discipline of eval_fold_kernel.  One workgroup of four waves.  Wave w takes the pairs 4 c + w of
// chunk c: lane l adds the rows l, l + 64, ... of the pair in ascending order (1.0 / rank in fp64), the wave meets by a butterfly;
// thread r < K then owns record r and walks the chunk's pairs below `live` in pair order, one pair at a time, taking those of its
// bin (bin == NULL: every pair is record 0's).  Every addition has its place fixed by (B, N, live) and the record it started from.
// A record that took no pair is not written, so its bytes stay.
__global__ __launch_bounds__(RANK_THREADS) void rank_fold_kernel(const int *rank, const int *nvalid, int B, int N, int live, RankKs ks,
                                                                 int nk, const int *bin, int K, int *pair_hits, double *pair_rr,
                                                                 long long *pair_rank_sum, int *pair_targets, fgnn_rank_record *records) {
    __shared__ double s_rr[RANK_THREADS / WAVE];
    __shared__ long long s_rs[RANK_THREADS / WAVE];
    __shared__ int s_tg[RANK_THREADS / WAVE];
    __shared__ int s_hits[RANK_THREADS / WAVE][FGNN_RANK_MAX_K];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const bool owner = (int)threadIdx.x < K;
    double rr_sum = 0.0;
    long long rank_sum = 0, targets = 0, nodes = 0, pairs = 0;
    long long hits_sum[FGNN_RANK_MAX_K];
#pragma unroll
    for (int q = 0; q < FGNN_RANK_MAX_K; ++q) hits_sum[q] = 0;
    if (owner) rr_sum = records[threadIdx.x].rr_sum;
    for (int b0 = 0; b0 < live; b0 += RANK_THREADS / WAVE) {         // (uniform bounds: every thread meets every barrier)
        const int b = b0 + wave;
        if (b < live) {
            const int n = clamp_nv(nvalid, b, N);
            double rr = 0.0;
            long long rs = 0;
            int tg = 0;
            int hits[FGNN_RANK_MAX_K];
#pragma unroll
            for (int q = 0; q < FGNN_RANK_MAX_K; ++q) hits[q] = 0;
            for (int i = lane; i < n; i += WAVE) {
                const int r = rank[(long long)b * N + i];
                if (r >= 1) {
                    rr += 1.0 / (double)r;
                    rs += r;
                    tg += 1;
#pragma unroll
                    for (int q = 0; q < FGNN_RANK_MAX_K; ++q) hits[q] += r <= ks.k[q] ? 1 : 0;
                }
            }
            for (int o = 32; o > 0; o >>= 1) {
                rr += __shfl_xor(rr, o);
                rs += __shfl_xor(rs, o);
                tg += __shfl_xor(tg, o);
#pragma unroll
                for (int q = 0; q < FGNN_RANK_MAX_K; ++q) hits[q] += __shfl_xor(hits[q], o);
            }
            if (lane == 0) {
                s_rr[wave] = rr;
                s_rs[wave] = rs;
                s_tg[wave] = tg;
                if (pair_rr) pair_rr[b] = rr;
                if (pair_rank_sum) pair_rank_sum[b] = rs;
                if (pair_targets) pair_targets[b] = tg;
#pragma unroll
                for (int q = 0; q < FGNN_RANK_MAX_K; ++q) {
                    s_hits[wave][q] = hits[q];
                    if (pair_hits && q < nk) pair_hits[(long long)b * nk + q] = hits[q];
                }
            }
        }
        __syncthreads();
        if (owner) {
            for (int w = 0; w < RANK_THREADS / WAVE && b0 + w < live; ++w) {
                if ((bin ? bin[b0 + w] : 0) != (int)threadIdx.x) continue;
                rr_sum += s_rr[w];
                rank_sum += s_rs[w];
                targets += s_tg[w];
#pragma unroll
                for (int q = 0; q < FGNN_RANK_MAX_K; ++q) hits_sum[q] += s_hits[w][q];
                nodes += clamp_nv(nvalid, b0 + w, N);
                pairs += 1;
            }
        }
        __syncthreads();
    }
    if (owner && pairs > 0) {
        fgnn_rank_record *rec = records + threadIdx.x;
        rec->rr_sum = rr_sum;
        rec->rank_sum += rank_sum;
        rec->targets += targets;
        rec->nodes += nodes;
        rec->pairs += pairs;
        rec->steps += 1;
#pragma unroll
        for (int q = 0; q < FGNN_RANK_MAX_K; ++q) rec->hits[q] += hits_sum[q];
    }
}

}  // namespace

extern "C" int fgnn_eval_ranks(const float *scores, long long bstride, int ld, const int *nvalid, const int *labels, int B, int N,
                               int *rank, void *stream) {
    FGNN_CHECK(scores && rank && B > 0 && N > 0, "fgnn_eval_ranks: bad arguments");
    FGNN_CHECK(ld >= N && bstride >= (long long)N * ld, "fgnn_eval_ranks: score strides smaller than the matrices");
    const unsigned wgs = row_group_wgs(B, N, RANK_THREADS);
    FGNN_CHECK(wgs, "fgnn_eval_ranks: %lld rows are more than one launch takes", (long long)B * N);
    hipLaunchKernelGGL(row_group_width(N) == 16 ? eval_ranks_kernel<16> : eval_ranks_kernel<WAVE>, dim3(wgs), dim3(RANK_THREADS), 0,
                       (hipStream_t)stream, scores, bstride, ld, nvalid, labels, B, N, rank);
    FGNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int fgnn_rank_fold(const int *rank, const int *nvalid, int B, int N, int live, const int *ks, int nk, const int *bins, int K,
                              int *pair_hits, double *pair_rr, long long *pair_rank_sum, int *pair_targets, fgnn_rank_record *records,
                              void *stream) {
    FGNN_CHECK(rank && ks && records && B > 0 && N > 0, "fgnn_rank_fold: bad arguments");
    FGNN_CHECK(live >= 0 && live <= B, "fgnn_rank_fold: live = %d outside [0, %d]", live, B);
    FGNN_CHECK(nk >= 1 && nk <= FGNN_RANK_MAX_K, "fgnn_rank_fold: nk = %d thresholds outside [1, %d]", nk, FGNN_RANK_MAX_K);
    FGNN_CHECK(bins ? K >= 1 && K <= FGNN_MAX_LEVELS : K == 1, "fgnn_rank_fold: K = %d records outside [1, %d] (1 without bins)", K,
               FGNN_MAX_LEVELS);
    RankKs kv;
    for (int q = 0; q < FGNN_RANK_MAX_K; ++q) {
        kv.k[q] = q < nk ? ks[q] : 0;
        FGNN_CHECK(q >= nk || ks[q] > (q ? ks[q - 1] : 0), "fgnn_rank_fold: thresholds must be positive and strictly increasing");
    }
    hipLaunchKernelGGL(rank_fold_kernel, dim3(1), dim3(RANK_THREADS), 0, (hipStream_t)stream, rank, nvalid, B, N, live, kv, nk, bins, K,
                       pair_hits, pair_rr, pair_rank_sum, pair_targets, records);
    FGNN_LAUNCH_CHECK();
    return 0;
}
