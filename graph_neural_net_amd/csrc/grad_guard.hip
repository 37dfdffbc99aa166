// Guarded optimizer step (include/fgnn_hip.h): the global L2 norm of the scaled gradient, the clip_grad_norm_ coefficient and a
// non-finite flag in one launch, and the Adam update of train_ops.hip that honours them in a second.  The reference has both from
// its trainer: pl.Trainer(precision=16) (commander_explore.py:120-122) steps through an AMP GradScaler, which skips
// optimizer.step() on an inf / NaN gradient, and gradient_clip_val clips by global norm.  Both launches read their decisions from
// device memory, so they sit in the captured step graph.
#include "fgnn_common.h"

namespace {

constexpr int GUARD_THREADS = 256;
constexpr int GUARD_CHUNK = 4096;       // elements per workgroup until all FGNN_GUARD_MAX_PARTS workgroups are in use

// a function of n alone: with the chunk bounds below it fixes the order of every addition
inline int guard_workgroups(int n) {
    const long long w = ((long long)n + GUARD_CHUNK - 1) / GUARD_CHUNK;
    return (int)(w < FGNN_GUARD_MAX_PARTS ? w : FGNN_GUARD_MAX_PARTS);
}

// Workgroup b owns elements [b * chunk, (b + 1) * chunk); thread t adds its elements t, t + 256, ... in that order, the wave sums
// by a butterfly (a + b == b + a: every lane ends with the same bits), thread 0 adds the four wave sums in wave order and the
// last workgroup to sign the arrival counter adds the partials in workgroup order.
// gi^2 is exact in fp64 (24 x 24 bits) and at most 1.2e77, so the fp64 sum cannot overflow and is non-finite exactly when some
// gi is an inf or a NaN (squares are never negative: no inf - inf): the flag is read off the sum.
__global__ __launch_bounds__(GUARD_THREADS) void grad_guard_kernel(const float *g, int n, const double *hp, fgnn_guard_record *gd) {
    __shared__ double red[GUARD_THREADS / WAVE];
    const float scale = (float)hp[4];
    const long long chunk = ((long long)n + gridDim.x - 1) / gridDim.x;
    const long long i0 = blockIdx.x * chunk, i1 = i0 + chunk < n ? i0 + chunk : n;
    double s = 0.0;
#pragma unroll 4
    for (long long i = i0 + threadIdx.x; i < i1; i += GUARD_THREADS) {
        const float gi = g[i] * scale;
        s += (double)gi * (double)gi;
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double part = red[0];
    for (int w = 1; w < GUARD_THREADS / WAVE; ++w) part += red[w];
    // the partial crosses to another compute unit: a write-through store and a release ahead of the counter, an acquire and
    // cache-bypassing loads behind it
    __hip_atomic_store(&gd->partial[blockIdx.x], part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();
    if (atomicAdd(&gd->arrivals, 1) != (int)gridDim.x - 1) return;
    __threadfence();
    double sum = 0.0;
    for (unsigned b = 0; b < gridDim.x; ++b) sum += __hip_atomic_load(&gd->partial[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const double norm = sqrt(sum), max_norm = gd->max_norm;
    const bool nonfinite = !(fabs(sum) <= 1.7976931348623157e308);      // inf or NaN
    double coef = 1.0;
    if (max_norm > 0.0) {
        const double c = max_norm / (norm + 1e-6);
        coef = c > 1.0 ? 1.0 : c;            // torch.clamp(c, max=1): a NaN stays a NaN
    }
    gd->norm = norm;
    gd->coef = coef;
    gd->flags = nonfinite ? FGNN_GUARD_NONFINITE : 0;
    if (nonfinite && (gd->mode & FGNN_GUARD_SKIP_NONFINITE)) gd->skipped += 1;
    gd->arrivals = 0;                        // ready for the next launch / replay
}

// adam_dev_kernel of train_ops.hip with grad_scale = (float)(hp[4] * coef) and the skip: when the guard says so, no workgroup
// stores anything except the reset of the arrival counter.
__global__ __launch_bounds__(256) void adam_guarded_kernel(float *p, const float *g, float *m, float *v, int n, const double *hp,
                                                           int *state, const fgnn_guard_record *gd) {
    __shared__ float sh[7];
    __shared__ int s_step, s_skip;
    if (threadIdx.x == 0) {
        const int step = state[0] + 1;
        const double lr = hp[0], b1 = hp[1], b2 = hp[2];
        const double bc1 = 1.0 - pow(b1, (double)step), bc2 = 1.0 - pow(b2, (double)step);
        sh[0] = (float)(lr / bc1);
        sh[1] = (float)(1.0 - b1);
        sh[2] = (float)b2;
        sh[3] = (float)(1.0 - b2);
        sh[4] = (float)(1.0 / sqrt(bc2));
        sh[5] = (float)hp[3];
        sh[6] = (float)(hp[4] * gd->coef);
        s_step = step;
        s_skip = (gd->mode & FGNN_GUARD_SKIP_NONFINITE) && (gd->flags & FGNN_GUARD_NONFINITE);
    }
    __syncthreads();
    const float step_size = sh[0], w1 = sh[1], beta2 = sh[2], w2 = sh[3], inv_sqrt_bc2 = sh[4], eps = sh[5], grad_scale = sh[6];
    const bool skip = s_skip != 0;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && !skip) {
        const float gi = g[i] * grad_scale;
        const float mi = m[i] + (gi - m[i]) * w1;
        const float vi = v[i] * beta2 + gi * gi * w2;
        m[i] = mi;
        v[i] = vi;
        const float denom = sqrtf(vi) * inv_sqrt_bc2 + eps;
        p[i] = p[i] - step_size * (mi / denom);
    }
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(&state[1], 1) == (int)gridDim.x - 1) {      // every workgroup has read state[0] by now
            state[1] = 0;
            if (!skip) state[0] = s_step;                         // a skipped step does not count
        }
    }
}

}  // namespace

extern "C" int fgnn_grad_guard(const float *grads, int n, const double *hp, fgnn_guard_record *guard, void *stream) {
    FGNN_CHECK(grads && hp && guard && n > 0, "fgnn_grad_guard: bad arguments");
    hipLaunchKernelGGL(grad_guard_kernel, dim3(guard_workgroups(n)), dim3(GUARD_THREADS), 0, (hipStream_t)stream, grads, n, hp, guard);
    FGNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int fgnn_adam_step_guarded(float *params, const float *grads, float *exp_avg, float *exp_avg_sq, int n, const double *hp,
                                      int *state, const fgnn_guard_record *guard, void *stream) {
    FGNN_CHECK(params && grads && exp_avg && exp_avg_sq && hp && state && guard && n > 0, "fgnn_adam_step_guarded: bad arguments");
    hipLaunchKernelGGL(adam_guarded_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, params, grads, exp_avg,
                       exp_avg_sq, n, hp, state, guard);
    FGNN_LAUNCH_CHECK();
    return 0;
}
