// Decode epochs on the device (include/fgnn_hip.h, "decode epochs"): what the reference's all_acc_qap(val_loader, ...) and
// all_greedy_losses_acc (toolbox/metrics.py:168-223) keep of a dataset -- the accuracy of the Hungarian matching, its QAP
// objective, the planted objective and the same after greedy_qap -- folded into one record per epoch (or per noise level) from the
// per-pair integers fgnn_lsap_accuracy, fgnn_qap_objective and fgnn_greedy_qap leave on the device.  0/1 graphs only: the
// objectives are the int32 values of csrc/qap.hip (the fp32 objectives of qap_weighted.hip have no epoch form).
//   fgnn_qap_fold      : the matches of assign and perm with the target of every row, per pair, and the add into the record.
//   fgnn_qap_fold_bins : the same kernel with one record per bin (the noise levels of FgnnTrainer.noise_curve).
// Both are plain launches on the caller's stream: capturable, no allocation, no copy, no synchronisation.
#include "fgnn_rows.h"

namespace {

constexpr int QFOLD_THREADS = 256;

// One workgroup of four waves, built like eval_fold_kernel (eval.hip).  Wave w takes the pairs 4 c + w of chunk c: lane l counts
// over the rows l, l + 64, ... of the pair those whose assign entry -- and, with `perm`, whose perm entry -- is the row's target
// (labels[b][i]; i without labels; none outside [0, n_b)), the wave meets by a butterfly, lane 0 forms the pair's ratio and leaves
// it with the pair's integers in LDS.  Thread k < K then owns record k and adds the chunk's pairs below `live` to its running
// record in pair order, one pair at a time, taking those of its bin (BINS = false: thread 0 owns the one record and takes every
// pair; `bin` and K are not read); with the pairs' values in LDS its serial walk waits for no global load.  Every addition,
// the fp64 one included, has its place fixed by (B, N, live), the bins and the record it started from, so an epoch's record has
// the same bits however its examples were cut into calls.  A record that took no pair is not written, so its bytes stay.
// The ratio is the IEEE quotient of two int32 values converted exactly: nothing in the build relaxes fp64 division.
template <bool BINS>
__global__ __launch_bounds__(QFOLD_THREADS) void qap_fold_kernel(const int *assign, const int *perm, const int *labels, const int *qap,
                                                                 const int *planted, const int *refined, const int *nvalid, int B, int N,
                                                                 int live, const int *bin, int K, int *pair_correct,
                                                                 int *pair_refined_correct, double *pair_ratio, fgnn_qap_record *records) {
    __shared__ double s_ratio[QFOLD_THREADS / WAVE];
    __shared__ int s_hit[QFOLD_THREADS / WAVE], s_rhit[QFOLD_THREADS / WAVE], s_n[QFOLD_THREADS / WAVE], s_qap[QFOLD_THREADS / WAVE],
        s_planted[QFOLD_THREADS / WAVE], s_refined[QFOLD_THREADS / WAVE];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const bool owner = BINS ? (int)threadIdx.x < K : threadIdx.x == 0;
    double ratio_sum = 0.0;
    long long ratio_pairs = 0, qap_sum = 0, planted_sum = 0, correct = 0, refined_sum = 0, refined_correct = 0, recovered = 0, exact = 0,
              improved = 0, unmatched = 0, nodes = 0, pairs = 0;
    fgnn_qap_record *meter = records + (BINS ? threadIdx.x : 0);
    if (owner) ratio_sum = meter->ratio_sum;
    for (int b0 = 0; b0 < live; b0 += QFOLD_THREADS / WAVE) {        // (uniform bounds: every thread meets every barrier)
        const int b = b0 + wave;
        if (b < live) {
            const int n = clamp_nv(nvalid, b, N);
            int hit = 0, rhit = 0;
            for (int i = lane; i < n; i += WAVE) {
                const long long at = (long long)b * N + i;
                const int t = labels ? labels[at] : i;
                const bool has = t >= 0 && t < n;
                hit += has && assign[at] == t ? 1 : 0;
                if (perm) rhit += has && perm[at] == t ? 1 : 0;
            }
            for (int o = 32; o > 0; o >>= 1) {
                hit += __shfl_xor(hit, o);
                rhit += __shfl_xor(rhit, o);
            }
            if (lane == 0) {
                const int q = qap[b], p = planted[b];
                const double ratio = q >= 0 && p > 0 ? (double)q / (double)p : 0.0;
                s_ratio[wave] = ratio;
                s_hit[wave] = hit;
                s_rhit[wave] = rhit;
                s_n[wave] = n;                             // (the owner's serial walk then reads LDS only)
                s_qap[wave] = q;
                s_planted[wave] = p;
                s_refined[wave] = perm ? refined[b] : 0;
                if (pair_correct) pair_correct[b] = hit;
                if (pair_refined_correct) pair_refined_correct[b] = rhit;
                if (pair_ratio) pair_ratio[b] = ratio;
            }
        }
        __syncthreads();
        if (owner) {
            for (int w = 0; w < QFOLD_THREADS / WAVE && b0 + w < live; ++w) {
                if (BINS && bin[b0 + w] != (int)threadIdx.x) continue;
                const int n = s_n[w], q = s_qap[w], p = s_planted[w];
                nodes += n;
                pairs += 1;
                correct += s_hit[w];
                exact += s_hit[w] == n ? 1 : 0;
                if (perm) refined_correct += s_rhit[w];
                if (q < 0) {                                         // no finite matching: none of the objective sums
                    unmatched += 1;
                    continue;
                }
                qap_sum += q;
                planted_sum += p;
                recovered += q >= p ? 1 : 0;
                if (p > 0) {
                    ratio_sum += s_ratio[w];
                    ratio_pairs += 1;
                }
                if (perm) {
                    const int r = s_refined[w];
                    refined_sum += r;
                    improved += r > q ? 1 : 0;
                }
            }
        }
        __syncthreads();
    }
    if (owner && (BINS ? pairs > 0 : live > 0)) {          // (a plain fold took a pair exactly when live > 0)
        meter->ratio_sum = ratio_sum;
        meter->ratio_pairs += ratio_pairs;
        meter->qap_sum += qap_sum;
        meter->planted_sum += planted_sum;
        meter->correct += correct;
        if (perm) {                                        // without a refinement its three fields are not touched
            meter->refined_sum += refined_sum;
            meter->refined_correct += refined_correct;
            meter->improved += improved;
        }
        meter->recovered += recovered;
        meter->exact += exact;
        meter->unmatched += unmatched;
        meter->nodes += nodes;
        meter->pairs += pairs;
        meter->steps += 1;
    }
}

}  // namespace

extern "C" int fgnn_qap_fold(const int *assign, const int *perm, const int *labels, const int *qap, const int *planted, const int *refined,
                             const int *nvalid, int B, int N, int live, int *pair_correct, int *pair_refined_correct, double *pair_ratio,
                             fgnn_qap_record *meter, void *stream) {
    FGNN_CHECK(assign && qap && planted && meter && B > 0 && N > 0, "fgnn_qap_fold: bad arguments");
    FGNN_CHECK((perm == NULL) == (refined == NULL), "fgnn_qap_fold: perm and refined go together");
    FGNN_CHECK(live >= 0 && live <= B, "fgnn_qap_fold: live = %d outside [0, %d]", live, B);
    hipLaunchKernelGGL(qap_fold_kernel<false>, dim3(1), dim3(QFOLD_THREADS), 0, (hipStream_t)stream, assign, perm, labels, qap, planted,
                       refined, nvalid, B, N, live, (const int *)NULL, 1, pair_correct, pair_refined_correct, pair_ratio, meter);
    FGNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int fgnn_qap_fold_bins(const int *assign, const int *perm, const int *labels, const int *qap, const int *planted,
                                  const int *refined, const int *nvalid, int B, int N, int live, const int *bin, int K, int *pair_correct,
                                  int *pair_refined_correct, double *pair_ratio, fgnn_qap_record *records, void *stream) {
    FGNN_CHECK(assign && qap && planted && bin && records && B > 0 && N > 0, "fgnn_qap_fold_bins: bad arguments");
    FGNN_CHECK((perm == NULL) == (refined == NULL), "fgnn_qap_fold_bins: perm and refined go together");
    FGNN_CHECK(live >= 0 && live <= B, "fgnn_qap_fold_bins: live = %d outside [0, %d]", live, B);
    FGNN_CHECK(K >= 1 && K <= FGNN_MAX_LEVELS, "fgnn_qap_fold_bins: K = %d records outside [1, %d]", K, FGNN_MAX_LEVELS);
    hipLaunchKernelGGL(qap_fold_kernel<true>, dim3(1), dim3(QFOLD_THREADS), 0, (hipStream_t)stream, assign, perm, labels, qap, planted,
                       refined, nvalid, B, N, live, bin, K, pair_correct, pair_refined_correct, pair_ratio, records);
    FGNN_LAUNCH_CHECK();
    return 0;
}
