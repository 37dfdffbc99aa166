// Decode epochs on REAL-weighted pairs (include/fgnn_hip.h, "decode epochs on real-weighted pairs"): the fp32-objective twins of
// qap_fold.hip, over what fgnn_qapw_objective, fgnn_greedy_qapw and fgnn_qapw_2opt leave on the device.
//   fgnn_qapw_fold      : the matches of assign and perm with the target of every row, per pair, and the add into the record.
//   fgnn_qapw_fold_bins : the same kernel with one record per bin.
// Both are plain launches on the caller's stream: capturable, no allocation, no copy, no synchronisation.  qap_fold.hip is left
// as it is: its int32 sums and its "qap < 0 means no matching" have no meaning here, and its code stays instruction for instruction.
#include "fgnn_rows.h"

namespace {

constexpr int QWFOLD_THREADS = 256;

// One workgroup of four waves, built like qap_fold_kernel.  Wave w takes the pairs 4 c + w of chunk c: lane l counts over the rows
// l, l + 64, ... of the pair the hits of assign (and of perm) and the assign entries outside [0, n_b) -- a weighted objective may be
// negative, so "no matching" is read from assign itself -- the wave meets by a butterfly, lane 0 leaves the pair's values in LDS.
// Thread k < K then owns record k (BINS = false: thread 0 owns the one record) and adds the chunk's pairs below `live` in pair
// order, one pair at a time.  The four fp64 sums start from the record's own values and every addition has its place fixed by
// (B, N, live), the bins and that start, so a record has the same bits however its pairs were cut into calls and equals a
// sequential host loop in IEEE double.  fp32 -> fp64 is exact; the ratio is the IEEE quotient: nothing in the build relaxes fp64
// division.  A NaN objective is not special-cased: it fails the comparisons and propagates into the sums.
template <bool BINS>
__global__ __launch_bounds__(QWFOLD_THREADS) void qapw_fold_kernel(const int *assign, const int *perm, const int *labels, const float *qap,
                                                                   const float *planted, const float *refined, const int *nvalid, int B,
                                                                   int N, int live, const int *bin, int K, int *pair_correct,
                                                                   int *pair_refined_correct, double *pair_ratio,
                                                                   fgnn_qapw_record *records) {
    constexpr int CHUNK = QWFOLD_THREADS / WAVE;
    __shared__ double s_ratio[CHUNK];
    __shared__ float s_qap[CHUNK], s_planted[CHUNK], s_refined[CHUNK];
    __shared__ int s_hit[CHUNK], s_rhit[CHUNK], s_n[CHUNK], s_out[CHUNK];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const bool owner = BINS ? (int)threadIdx.x < K : threadIdx.x == 0;
    double ratio_sum = 0.0, qap_sum = 0.0, planted_sum = 0.0, refined_sum = 0.0;
    long long ratio_pairs = 0, correct = 0, refined_correct = 0, recovered = 0, exact = 0, improved = 0, unmatched = 0, nodes = 0,
              pairs = 0;
    fgnn_qapw_record *meter = records + (BINS ? threadIdx.x : 0);
    if (owner) {
        ratio_sum = meter->ratio_sum;
        qap_sum = meter->qap_sum;
        planted_sum = meter->planted_sum;
        if (perm) refined_sum = meter->refined_sum;
    }
    for (int b0 = 0; b0 < live; b0 += CHUNK) {             // (uniform bounds: every thread meets every barrier)
        const int b = b0 + wave;
        if (b < live) {
            const int n = clamp_nv(nvalid, b, N);
            int hit = 0, rhit = 0, out = 0;
            for (int i = lane; i < n; i += WAVE) {
                const long long at = (long long)b * N + i;
                const int t = labels ? labels[at] : i, a = assign[at];
                const bool has = t >= 0 && t < n;
                hit += has && a == t ? 1 : 0;
                out += a < 0 || a >= n ? 1 : 0;
                if (perm) rhit += has && perm[at] == t ? 1 : 0;
            }
            for (int o = 32; o > 0; o >>= 1) {
                hit += __shfl_xor(hit, o);
                rhit += __shfl_xor(rhit, o);
                out += __shfl_xor(out, o);
            }
            if (lane == 0) {
                const float q = qap[b], p = planted[b];
                const double ratio = out == 0 && p > 0.f ? (double)q / (double)p : 0.0;
                s_ratio[wave] = ratio;
                s_hit[wave] = hit;
                s_rhit[wave] = rhit;
                s_n[wave] = n;                             // (the owner's serial walk then reads LDS only)
                s_out[wave] = out;
                s_qap[wave] = q;
                s_planted[wave] = p;
                s_refined[wave] = perm ? refined[b] : 0.f;
                if (pair_correct) pair_correct[b] = hit;
                if (pair_refined_correct) pair_refined_correct[b] = rhit;
                if (pair_ratio) pair_ratio[b] = ratio;
            }
        }
        __syncthreads();
        if (owner) {
            for (int w = 0; w < CHUNK && b0 + w < live; ++w) {
                if (BINS && bin[b0 + w] != (int)threadIdx.x) continue;
                const int n = s_n[w];
                const float q = s_qap[w], p = s_planted[w];
                nodes += n;
                pairs += 1;
                correct += s_hit[w];
                if (s_out[w] != 0) {                       // an assign entry outside the corner: none of the other sums
                    unmatched += 1;
                    continue;
                }
                exact += s_hit[w] == n ? 1 : 0;
                if (perm) refined_correct += s_rhit[w];
                qap_sum += (double)q;
                planted_sum += (double)p;
                recovered += q >= p ? 1 : 0;
                if (p > 0.f) {
                    ratio_sum += s_ratio[w];
                    ratio_pairs += 1;
                }
                if (perm) {
                    const float r = s_refined[w];
                    refined_sum += (double)r;
                    improved += r > q ? 1 : 0;
                }
            }
        }
        __syncthreads();
    }
    if (owner && (BINS ? pairs > 0 : live > 0)) {          // (a plain fold took a pair exactly when live > 0)
        meter->ratio_sum = ratio_sum;
        meter->qap_sum = qap_sum;
        meter->planted_sum = planted_sum;
        meter->ratio_pairs += ratio_pairs;
        meter->correct += correct;
        if (perm) {                                        // without a refinement its three fields are not touched
            meter->refined_sum = refined_sum;
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

int fold_w(const char *who, bool bins, const int *assign, const int *perm, const int *labels, const float *qap, const float *planted,
           const float *refined, const int *nvalid, int B, int N, int live, const int *bin, int K, int *pair_correct,
           int *pair_refined_correct, double *pair_ratio, fgnn_qapw_record *records, void *stream) {
    FGNN_CHECK(assign && qap && planted && records && (!bins || bin) && B > 0 && N > 0, "%s: bad arguments", who);
    FGNN_CHECK((perm == NULL) == (refined == NULL), "%s: perm and refined go together", who);
    FGNN_CHECK(live >= 0 && live <= B, "%s: live = %d outside [0, %d]", who, live, B);
    FGNN_CHECK(!bins || (K >= 1 && K <= FGNN_MAX_LEVELS), "%s: K = %d records outside [1, %d]", who, K, FGNN_MAX_LEVELS);
    if (bins)
        hipLaunchKernelGGL(qapw_fold_kernel<true>, dim3(1), dim3(QWFOLD_THREADS), 0, (hipStream_t)stream, assign, perm, labels, qap, planted,
                           refined, nvalid, B, N, live, bin, K, pair_correct, pair_refined_correct, pair_ratio, records);
    else
        hipLaunchKernelGGL(qapw_fold_kernel<false>, dim3(1), dim3(QWFOLD_THREADS), 0, (hipStream_t)stream, assign, perm, labels, qap,
                           planted, refined, nvalid, B, N, live, (const int *)NULL, 1, pair_correct, pair_refined_correct, pair_ratio,
                           records);
    FGNN_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int fgnn_qapw_fold(const int *assign, const int *perm, const int *labels, const float *qap, const float *planted,
                              const float *refined, const int *nvalid, int B, int N, int live, int *pair_correct,
                              int *pair_refined_correct, double *pair_ratio, fgnn_qapw_record *meter, void *stream) {
    return fold_w("fgnn_qapw_fold", false, assign, perm, labels, qap, planted, refined, nvalid, B, N, live, NULL, 1, pair_correct,
                  pair_refined_correct, pair_ratio, meter, stream);
}

extern "C" int fgnn_qapw_fold_bins(const int *assign, const int *perm, const int *labels, const float *qap, const float *planted,
                                   const float *refined, const int *nvalid, int B, int N, int live, const int *bin, int K,
                                   int *pair_correct, int *pair_refined_correct, double *pair_ratio, fgnn_qapw_record *records,
                                   void *stream) {
    return fold_w("fgnn_qapw_fold_bins", true, assign, perm, labels, qap, planted, refined, nvalid, B, N, live, bin, K, pair_correct,
                  pair_refined_correct, pair_ratio, records, stream);
}
