// Sinkhorn normalisation of a batch of score matrices, in the log domain, one workgroup per pair and the whole iteration in ONE
// launch: the doubly stochastic start a Frank-Wolfe chain (qap_faq.hip) takes from a model's scores.  Per pair, on the n_b x n_b
// corner, with Z = S / tau (one correctly rounded fp32 division per entry), f = 0, g = 0, `iters` times
//
//     f_i = -LSE_j(Z_ij + g_j)        a wave per row: lane l takes the columns l, l + 64, ..; max and sum meet by xor butterflies
//     g_j = -LSE_i(Z_ij + f_i)        a thread per (column, slice of the rows), the rows of a slice ascending; the slices' (max, sum)
//                                     pairs are folded in slice order
//
// then P_ij = exp((Z_ij + f_i) + g_j) on the corner and an exact 0 around it (every element of the (N, N) output is written), and
// err = max_i |sum_j P_ij - 1| from the row sums of the P just written.  Every LSE subtracts its maximum; every reduction has a
// fixed order that depends on (n_b, the kernel form) only -- no float atomics -- so the output is bit-identical from run to run and
// a pair's bits do not depend on the batch around it.  -inf entries are legal and give P = 0.
//
// A pair whose corner holds a NaN or a +inf (in Z), or a row or a column without a finite entry, or n_b = 0, is degenerate:
// status 1, P = 1 / n_b on the corner (the barycenter), err = 0.  The NaN / +inf test is made while Z is loaded; given it, a row
// (column) has no finite entry exactly when the maximum of its first LSE is -inf, which the first iteration reports.
//
// Z stays resident in LDS for N <= 192 (SK_LDS_MAX_N): 192 x 192 floats are 144 KiB of the CU's 160 KiB, and the column slices
// (8 KiB at 1024 threads) and f, g still fit beside them; from N = 197 on they no longer do (Z alone fits up to 202).  Above,
// every pass re-reads S in place (it stays in L2: 256 KiB per pair at N = 256) and divides again.  N <= 64 has a form of its own
// (16 KiB, 256 threads) so that small pairs share a CU; the 192-row form is one workgroup of 16 waves per CU.
// Nothing outside a pair's corner is read.
#include "fgnn_rows.h"

namespace {

constexpr int SK_LDS_MAX_N = FGNN_SINKHORN_LDS_MAX_N;      // 192; beyond: Z is recomputed from S in every pass

DEVI float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

DEVI float wave_sum(float v) {             // a + b == b + a bit for bit: every lane returns the same sum
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// One workgroup of T threads per pair.  R: the largest corner of this form (the rows Z holds in LDS, IN_LDS).
template <int R, int T, bool IN_LDS>
__global__ __launch_bounds__(T) void sinkhorn_kernel(const float *S, long long pair_stride, int ld, const int *nvalid, int N, float tau,
                                                     int iters, float *P, float *err, int *status) {
    constexpr int WAVES = T / 64, KMAX = (R + 63) / 64, CELLS = IN_LDS ? R * R : 1;
    __shared__ float z_l[CELLS];               // Z, row pitch n
    __shared__ float f_l[R], g_l[R];
    __shared__ float pm[T], ps[T];             // the column slices' maxima and sums; pm[0 .. WAVES) later the waves' row errors
    const int b = blockIdx.x, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int n = corner_of(nvalid, b, N);
    const float *Sb = S + (long long)b * pair_stride;
    float *Pb = P + (long long)b * N * N;
    auto zat = [&](int i, int j) -> float {
        if constexpr (IN_LDS) return z_l[i * n + j];
        else return Sb[(long long)i * ld + j] / tau;
    };

    int bad = 0;
    for (int idx = tid; idx < n * n; idx += T) {
        const int i = idx / n, j = idx - i * n;
        const float z = Sb[(long long)i * ld + j] / tau;
        if constexpr (IN_LDS) z_l[idx] = z;
        bad |= !(z < INFINITY);                 // NaN or +inf
    }
    for (int k = tid; k < n; k += T) g_l[k] = 0.f;
    bad = __syncthreads_or(bad) || n == 0;      // uniform from here on

    // the column pass gives every column cw / 64 whole waves' worth of lanes: thread tid is column c of slice p (tid = p cw + c)
    const int cw = (n + 63) & ~63, parts = cw ? T / cw : 0, chunk = parts ? (n + parts - 1) / parts : 0;
    const int c = cw ? tid % cw : 0, p = cw ? tid / cw : 0;

    for (int it = 0; it < iters && !bad; ++it) {
        int deg = 0;
        for (int i = wv; i < n; i += WAVES) {
            float v[KMAX], m = -INFINITY;
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                const int j = lane + 64 * k;
                v[k] = j < n ? zat(i, j) + g_l[j] : -INFINITY;
                m = fmaxf(m, v[k]);
            }
            m = wave_max(m);
            float s = 0.f;
            if (m > -INFINITY) {
#pragma unroll
                for (int k = 0; k < KMAX; ++k) s += expf(v[k] - m);      // (a lane past the row adds exp(-inf) = 0)
            }
            s = wave_sum(s);
            if (lane == 0) f_l[i] = -(m + logf(s));
            deg |= !(m > -INFINITY);
        }
        if (__syncthreads_or(it == 0 && deg)) {     // a row without a finite entry
            bad = 1;
            break;
        }
        if (p < parts) {
            float m = -INFINITY, s = 0.f;
            if (c < n) {
                const int i0 = p * chunk, i1 = min(n, i0 + chunk);
                for (int i = i0; i < i1; ++i) m = fmaxf(m, zat(i, c) + f_l[i]);
                if (m > -INFINITY)
                    for (int i = i0; i < i1; ++i) s += expf((zat(i, c) + f_l[i]) - m);
            }
            pm[tid] = m;
            ps[tid] = s;
        }
        __syncthreads();
        deg = 0;
        if (tid < n) {
            float m = -INFINITY, s = 0.f;
            for (int q = 0; q < parts; ++q) m = fmaxf(m, pm[q * cw + tid]);
            if (m > -INFINITY)
                for (int q = 0; q < parts; ++q) s += ps[q * cw + tid] * expf(pm[q * cw + tid] - m);     // (an empty slice: 0 * 0)
            g_l[tid] = -(m + logf(s));
            deg = !(m > -INFINITY);
        }
        if (__syncthreads_or(it == 0 && deg)) {     // a column without a finite entry
            bad = 1;
            break;
        }
    }

    const float bary = n > 0 ? (float)(1.0 / (double)n) : 0.f;
    float emax = 0.f;
    for (int i = wv; i < N; i += WAVES) {
        float rs = 0.f;
        for (int j = lane; j < N; j += 64) {
            float v = 0.f;
            if (i < n && j < n) v = bad ? bary : expf((zat(i, j) + f_l[i]) + g_l[j]);
            Pb[(long long)i * N + j] = v;
            rs += v;
        }
        rs = wave_sum(rs);
        if (i < n) emax = fmaxf(emax, fabsf(rs - 1.f));
    }
    if (lane == 0) pm[wv] = emax;
    __syncthreads();
    if (tid == 0) {
        float e = 0.f;
        for (int w = 0; w < WAVES; ++w) e = fmaxf(e, pm[w]);
        err[b] = bad ? 0.f : e;
        status[b] = bad ? 1 : 0;
    }
}

template <int R, int T, bool IN_LDS>
int launch_sinkhorn(const float *S, long long pair_stride, int ld, const int *nvalid, int B, int N, float tau, int iters, float *P,
                    float *err, int *status, hipStream_t st) {
    hipLaunchKernelGGL((sinkhorn_kernel<R, T, IN_LDS>), dim3(B), dim3(T), 0, st, S, pair_stride, ld, nvalid, N, tau, iters, P, err, status);
    FGNN_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int fgnn_sinkhorn(const float *S, long long pair_stride, int ld, const int *nvalid, int B, int N, float tau, int iters,
                             float *P, float *err, int *status, void *stream) {
    FGNN_CHECK(S && P && err && status && B > 0 && N > 0, "fgnn_sinkhorn: bad arguments");
    FGNN_CHECK(N <= FGNN_QAP_MAX_N, "fgnn_sinkhorn: at most %d vertices per graph (got %d)", FGNN_QAP_MAX_N, N);
    FGNN_CHECK(tau > 0.f && tau < INFINITY, "fgnn_sinkhorn: tau must be a positive finite number (got %g)", (double)tau);
    FGNN_CHECK(iters >= 1, "fgnn_sinkhorn: iters must be at least 1 (got %d)", iters);
    FGNN_CHECK(ld >= N && (B == 1 || pair_stride >= (long long)N * ld), "fgnn_sinkhorn: ld / pair_stride smaller than the matrices");
    hipStream_t st = (hipStream_t)stream;
    if (N <= 64) return launch_sinkhorn<64, 256, true>(S, pair_stride, ld, nvalid, B, N, tau, iters, P, err, status, st);
    if (N <= SK_LDS_MAX_N) return launch_sinkhorn<SK_LDS_MAX_N, 1024, true>(S, pair_stride, ld, nvalid, B, N, tau, iters, P, err, status, st);
    return launch_sinkhorn<FGNN_QAP_MAX_N, 1024, false>(S, pair_stride, ld, nvalid, B, N, tau, iters, P, err, status, st);
}
