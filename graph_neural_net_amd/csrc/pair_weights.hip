// Per-pair loss weights of the fused step (include/fgnn_hip.h): the weights of a reduction with their
// normaliser (fgnn_pair_weights) and the weighted sum of the per-pair loss partials (fgnn_pair_loss_w).  Two one-workgroup kernels
// with fixed summation orders; the weighted score backward is an instantiation of the bodies in pool_score.hip.
#include "fgnn_common.h"

namespace {

// toolbox/losses.py:14-15 ('mean_of_mean': the average over graphs of the per-graph mean) and :27-34 ('mean': the sum over the
// node count), with the positions >= live of a short last step switched off.  D: every thread sums its pairs b = tid, tid + 256, ...
// in fp64, the 256 sums meet in a fixed tree.
__global__ __launch_bounds__(256) void pair_weights_kernel(const int *nvalid, const int *live_dev, int mode, const float *user, int B,
                                                           int N, float *w_out, float *denom_out) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    int live = live_dev ? *live_dev : B;
    live = live < 0 ? 0 : (live > B ? B : live);
    double d = 0.0;
    for (int b = tid; b < B; b += 256) {
        int n = nvalid_of(nvalid, b, N);
        n = n < 0 ? 0 : (n > N ? N : n);
        const float u = user ? user[b] : 1.f;
        float w = 0.f;
        if (b < live && (mode == 0 || n > 0)) {
            // 1 / n rounded once from the fp64 quotient, whatever division the fp32 operator compiles to
            w = mode == 0 ? u : (user ? (float)(1.0 / (double)n) * u : (float)(1.0 / (double)n));
            d += mode == 0 ? (double)n * (double)u : (double)u;
        }
        w_out[b] = w;
    }
    red[tid] = d;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) denom_out[0] = (float)red[0];
}

// The order of reduce_cols (norm.hip) on one column of R = B * row_blocks rows, which fgnn_sum_scale and the loss job of
// fgnn_grad_finalize run on the unweighted partials: lane l of four adds the rows l, l + 4, l + 8, ... in ascending order, then
// (l0 + l1) + (l2 + l3).  A row of a pair with w == 0 is stepped over (its partial is not read into the sum); every product is
// rounded on its own (__fmul_rn: no contraction into the addition), so with w == 1 the sum has the bits of the unweighted one.
// The terms are formed by all 256 threads, PL_CHUNK rows at a time through LDS (independent loads; a stepped-over row leaves +0,
// which adds nothing), and the four lanes then walk the chunk: no chain of dependent memory round trips.
constexpr int PL_CHUNK = 1024;      // a multiple of 4: row r of a chunk belongs to lane r & 3 as in the whole column
__global__ __launch_bounds__(256) void pair_loss_w_kernel(const float *pair_loss, int row_blocks, const float *pair_weight, int B,
                                                          float *out) {
    __shared__ float term[PL_CHUNK];
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const long long R = (long long)B * row_blocks;
    float a = 0.f;
    for (long long base = 0; base < R; base += PL_CHUNK) {
        const int n = (int)(R - base < PL_CHUNK ? R - base : PL_CHUNK);
        for (int k = tid; k < n; k += 256) {
            const long long r = base + k;
            const float w = pair_weight[r / row_blocks];
            const float p = pair_loss[r];
            term[k] = w != 0.f ? __fmul_rn(w, p) : 0.f;
        }
        __syncthreads();
        if (tid < 4)
            for (int k = tid; k < n; k += 4) a += term[k];
        __syncthreads();
    }
    if (tid < 4) red[tid] = a;
    __syncthreads();
    if (tid == 0) out[0] = (red[0] + red[1]) + (red[2] + red[3]);
}

}  // namespace

extern "C" int fgnn_pair_weights(const int *nvalid, const int *live_dev, int mode, const float *user, int B, int N, float *w_out,
                                 float *denom_out, void *stream) {
    FGNN_CHECK(w_out && denom_out && B > 0 && N > 0 && (mode == 0 || mode == 1), "fgnn_pair_weights: bad arguments (mode=%d)", mode);
    hipLaunchKernelGGL(pair_weights_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, nvalid, live_dev, mode, user, B, N, w_out,
                       denom_out);
    FGNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int fgnn_pair_loss_w(const float *pair_loss, int row_blocks, const float *pair_weight, int B, float *out, void *stream) {
    FGNN_CHECK(pair_loss && pair_weight && out && B > 0 && row_blocks > 0, "fgnn_pair_loss_w: bad arguments");
    hipLaunchKernelGGL(pair_loss_w_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, pair_loss, row_blocks, pair_weight, B, out);
    FGNN_LAUNCH_CHECK();
    return 0;
}
