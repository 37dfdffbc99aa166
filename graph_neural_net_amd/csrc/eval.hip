// Validation on the device (include/fgnn_hip.h, "evaluation"): what the reference's all_losses_acc (toolbox/metrics.py:144-166)
// and the val_loss of its ReduceLROnPlateau (models/trainers.py:78-104) need from a batch of raw scores, without the eager
// prologue of the Hungarian accuracy (masked_fill, log_softmax, negation, contiguous: five passes over B N^2 floats) and without
// a read-back per batch.
//   fgnn_eval_pairs : ONE pass over the scores: per valid row the log-sum-exp, the cost row -log_softmax for fgnn_lsap_accuracy,
//                     the cross-entropy against the identity and the arg-max hit (fgnn_eval_pairs_labels: against the labels).
//   fgnn_eval_fold  : per-pair sums of those rows and the add into the epoch record, by one workgroup in a fixed order.
//   fgnn_eval_fold_bins : the same kernel with one record per bin (the noise levels of FgnnTrainer.noise_curve).
// All are plain launches on the caller's stream: capturable, no allocation, no copy, no synchronisation.
#include "fgnn_rows.h"

namespace {

constexpr int EVAL_THREADS = 256;

// W lanes per row (fgnn_rows.h).  Lane `sub` of a row's group takes the columns sub, sub + W, ... in ascending order and the group
// meets by xor butterflies below W (a + b == b + a: every lane of the group ends with the same bits), so the order of every
// addition is a function of (N, lane) alone -- W is chosen from N -- and a row has the same lse in any batch, at any position.
// The arg-max is the rule of fgnn_accuracy_max (row_argmax).  Its value doubles as the row maximum m of the lse: a NaN there makes
// the lse NaN, which exp(NaN - m) would as well.
// LCE (fgnn_eval_pairs_labels): the target of the cross-entropy is the row's label as well: row_ce = lse - s[i, t_i], and 0 for a
// row whose label lies outside [0, n_b) (no target); row_hit and the cost corner are those of the plain kernel.
template <int W, bool LCE>
__global__ __launch_bounds__(EVAL_THREADS) void eval_pairs_kernel(const float *scores, const int *nvalid, const int *labels, int B, int N,
                                                                  float *cost, long long cost_bstride, int cost_ld, float *row_ce,
                                                                  int *row_hit) {
    const int sub = threadIdx.x & (W - 1);
    const long long t = (long long)blockIdx.x * (EVAL_THREADS / W) + threadIdx.x / W;      // row index over (b, i)
    const bool inside = t < (long long)B * N;
    const long long tc = inside ? t : 0;
    const int b = (int)(tc / N), i = (int)(tc - (long long)b * N);
    const int nb = clamp_nv(nvalid, b, N);
    const bool live = inside && i < nb;                  // (uniform inside a row's group)
    const int n = live ? nb : 0;                         // dead groups run the butterflies on empty rows and store nothing
    const float *row = scores + ((long long)b * N + i) * N;

    const RowMax am = row_argmax<W>(row, n, sub);
    const float m = am.best;
    float sum = 0.f;
    for (int j = sub; j < n; j += W) sum += expf(row[j] - m);
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    const float lse = m + logf(sum);
    float *crow = cost + (long long)b * cost_bstride + (long long)i * cost_ld;
    for (int j = sub; j < n; j += W) crow[j] = lse - row[j];
    if (live && sub == 0) {
        if (LCE) {
            const int ti = labels[t];
            row_ce[t] = ti >= 0 && ti < nb ? lse - row[ti] : 0.f;
            row_hit[t] = am.bj == ti ? 1 : 0;
        } else {
            row_ce[t] = lse - row[i];
            row_hit[t] = am.bj == (labels ? labels[t] : i) ? 1 : 0;
        }
    }
}

// One workgroup of four waves.  Wave w takes the pairs 4 c + w of chunk c: lane l adds the rows l, l + 64, ... of the pair in
// ascending order (fp64 for the cross-entropy), the wave meets by a butterfly; thread k < K then owns record k and adds the chunk's
// pairs below `live` to its running record in pair order, one pair at a time, taking those of its bin (BINS = false, fgnn_eval_fold:
// thread 0 owns the one record and takes every pair; `bin` and K are not read).  Every addition has its place fixed by (B, N, live)
// and the record it started from, so an epoch's record has the same bits on every run, however its examples were cut into calls.
// A record that took no pair is not written, so its bytes stay.
// One body, two instantiations: with `bin` tested for NULL at run time instead, both folds measured 0.8 to 1.3 us slower.  The
// `BINS ? ... :` selections below keep the plain instantiation at the instructions of the stand-alone kernel it replaced (thread 0,
// the record through a uniform pointer, the write decided by `live`, clamp_nv): with the record indexed by thread, `pairs` tested and
// corner_of it took two more registers and measured 0.45 us more than that kernel's 7.4.
template <bool BINS>
__global__ __launch_bounds__(EVAL_THREADS) void eval_fold_kernel(const float *row_ce, const int *row_hit, const int *correct_lsap,
                                                                 const int *nvalid, int B, int N, int live, const int *bin, int K,
                                                                 double *pair_ce, int *pair_max, fgnn_eval_record *records) {
    __shared__ double s_ce[EVAL_THREADS / WAVE];
    __shared__ int s_hit[EVAL_THREADS / WAVE];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const bool owner = BINS ? (int)threadIdx.x < K : threadIdx.x == 0;
    double ce_sum = 0.0;
    long long nodes = 0, c_lsap = 0, c_max = 0, pairs = 0;
    fgnn_eval_record *meter = records + (BINS ? threadIdx.x : 0);
    if (owner) ce_sum = meter->ce_sum;
    for (int b0 = 0; b0 < live; b0 += EVAL_THREADS / WAVE) {         // (uniform bounds: every thread meets every barrier)
        const int b = b0 + wave;
        if (b < live) {
            const int n = clamp_nv(nvalid, b, N);
            double ce = 0.0;
            int hit = 0;
            for (int i = lane; i < n; i += WAVE) {
                ce += (double)row_ce[(long long)b * N + i];
                hit += row_hit[(long long)b * N + i];
            }
            for (int o = 32; o > 0; o >>= 1) {
                ce += __shfl_xor(ce, o);
                hit += __shfl_xor(hit, o);
            }
            if (lane == 0) {
                s_ce[wave] = ce;
                s_hit[wave] = hit;
                if (pair_ce) pair_ce[b] = ce;
                if (pair_max) pair_max[b] = hit;
            }
        }
        __syncthreads();
        if (owner) {
            for (int w = 0; w < EVAL_THREADS / WAVE && b0 + w < live; ++w) {
                if (BINS && bin[b0 + w] != (int)threadIdx.x) continue;
                ce_sum += s_ce[w];
                c_max += s_hit[w];
                nodes += clamp_nv(nvalid, b0 + w, N);
                if (correct_lsap) c_lsap += correct_lsap[b0 + w];
                pairs += 1;
            }
        }
        __syncthreads();
    }
    if (owner && (BINS ? pairs > 0 : live > 0)) {          // (a plain fold took a pair exactly when live > 0)
        meter->ce_sum = ce_sum;
        meter->nodes += nodes;
        meter->correct_lsap += c_lsap;
        meter->correct_max += c_max;
        meter->pairs += pairs;
        meter->steps += 1;
    }
}

// the one launcher of fgnn_eval_pairs (LCE = false) and fgnn_eval_pairs_labels (LCE = true, which needs its labels)
template <bool LCE>
int launch_eval_pairs(const char *who, const float *scores, const int *nvalid, const int *labels, int B, int N, float *cost,
                      long long cost_bstride, int cost_ld, float *row_ce, int *row_hit, void *stream) {
    FGNN_CHECK(scores && (!LCE || labels) && cost && row_ce && row_hit && B > 0 && N > 0, "%s: bad arguments", who);
    FGNN_CHECK(N <= FGNN_LSAP_MAX_N, "%s: at most %d vertices per graph (got %d)", who, FGNN_LSAP_MAX_N, N);
    FGNN_CHECK(cost_ld >= N && cost_bstride >= (long long)N * cost_ld, "%s: cost strides smaller than the matrices", who);
    const unsigned wgs = row_group_wgs(B, N, EVAL_THREADS);
    FGNN_CHECK(wgs, "%s: %lld rows are more than one launch takes", who, (long long)B * N);
    const auto kernel = row_group_width(N) == 16 ? eval_pairs_kernel<16, LCE> : eval_pairs_kernel<WAVE, LCE>;
    hipLaunchKernelGGL(kernel, dim3(wgs), dim3(EVAL_THREADS), 0, (hipStream_t)stream, scores, nvalid, labels, B, N, cost, cost_bstride,
                       cost_ld, row_ce, row_hit);
    FGNN_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int fgnn_eval_pairs(const float *scores, const int *nvalid, const int *labels, int B, int N, float *cost,
                               long long cost_bstride, int cost_ld, float *row_ce, int *row_hit, void *stream) {
    return launch_eval_pairs<false>("fgnn_eval_pairs", scores, nvalid, labels, B, N, cost, cost_bstride, cost_ld, row_ce, row_hit, stream);
}

extern "C" int fgnn_eval_pairs_labels(const float *scores, const int *nvalid, const int *labels, int B, int N, float *cost,
                                      long long cost_bstride, int cost_ld, float *row_ce, int *row_hit, void *stream) {
    return launch_eval_pairs<true>("fgnn_eval_pairs_labels", scores, nvalid, labels, B, N, cost, cost_bstride, cost_ld, row_ce, row_hit,
                                   stream);
}

extern "C" int fgnn_eval_fold(const float *row_ce, const int *row_hit, const int *correct_lsap, const int *nvalid, int B, int N,
                              int live, double *pair_ce, int *pair_max, fgnn_eval_record *meter, void *stream) {
    FGNN_CHECK(row_ce && row_hit && meter && B > 0 && N > 0, "fgnn_eval_fold: bad arguments");
    FGNN_CHECK(live >= 0 && live <= B, "fgnn_eval_fold: live = %d outside [0, %d]", live, B);
    hipLaunchKernelGGL(eval_fold_kernel<false>, dim3(1), dim3(EVAL_THREADS), 0, (hipStream_t)stream, row_ce, row_hit, correct_lsap, nvalid,
                       B, N, live, (const int *)NULL, 1, pair_ce, pair_max, meter);
    FGNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int fgnn_eval_fold_bins(const float *row_ce, const int *row_hit, const int *correct_lsap, const int *nvalid, int B, int N,
                                   int live, const int *bin, int K, double *pair_ce, int *pair_max, fgnn_eval_record *records,
                                   void *stream) {
    FGNN_CHECK(row_ce && row_hit && bin && records && B > 0 && N > 0, "fgnn_eval_fold_bins: bad arguments");
    FGNN_CHECK(live >= 0 && live <= B, "fgnn_eval_fold_bins: live = %d outside [0, %d]", live, B);
    FGNN_CHECK(K >= 1 && K <= FGNN_MAX_LEVELS, "fgnn_eval_fold_bins: K = %d records outside [1, %d]", K, FGNN_MAX_LEVELS);
    hipLaunchKernelGGL(eval_fold_kernel<true>, dim3(1), dim3(EVAL_THREADS), 0, (hipStream_t)stream, row_ce, row_hit, correct_lsap, nvalid,
                       B, N, live, bin, K, pair_ce, pair_max, records);
    FGNN_LAUNCH_CHECK();
    return 0;
}
