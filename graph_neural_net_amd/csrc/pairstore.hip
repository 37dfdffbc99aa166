// Pairs from stored graphs (loaders/data_generator.py:133-155, Base_Generator.load_dataset: a dataset that is loaded, not
// generated): a store is M graphs in the engine's wire format, resident in device memory, and one launch gathers a batch from it
// in the form fgnn_pairgen_indexed writes (include/fgnn_hip.h; graph_neural_net_amd/pairstore.py).
//
// The execution shape is the generator's (pairgen.hip): one single-wave workgroup per pair, parent and copy as bit rows in LDS,
// and the noisy copy is made by the generator's own device code (fgnn_pairgen_dev.h) on the same Philox streams, positions and
// thresholds for pair (seed, k) -- a draw depends on (seed, pair, stream, position) only, so the copy of a stored parent is the
// copy the generator makes of the same parent, bit for bit (tests/pairgen_ref.py restates both noise functions on any parent).
// A store with a second side of its own is a plain copy of two slabs, without LDS.
#include "fgnn_common.h"
#include "fgnn_pairgen_dev.h"
#include "fgnn_philox.h"

namespace {

// the number of entries edge_list writes: the bits (u, j > u) of rows u < n (wave-uniform)
DEVI int edge_count(const unsigned *rows, int W, int n) {
    const int lane = threadIdx.x;
    int c = 0;
    for (int u = lane; u < n; u += PG_THREADS)
        for (int w = 0; w < W; ++w) c += __popc(rows[u * W + w] & (32 * w > u ? ~0u : 32 * w + 31 <= u ? 0u : ~0u << (u - 32 * w + 1)));
#pragma unroll
    for (int off = 1; off < PG_THREADS; off <<= 1) c += __shfl_xor(c, off);
    return uni(c);
}

__global__ __launch_bounds__(PG_THREADS) void pairstore_kernel(fgnn_pairstore_args a) {
    extern __shared__ unsigned smem[];
    const int N = a.N, W = (N + 31) >> 5, lane = threadIdx.x;
    const long long off = (long long)blockIdx.x * N * W;
    long long k = a.index ? a.index[blockIdx.x] : a.first + blockIdx.x;
    unsigned long long thr_noise1 = a.thr_noise1, thr_noise2 = a.thr_noise2;
    if (a.level) {
        const int lv = a.level[blockIdx.x];
        if (lv < 0 || lv >= a.K) {
            k = -1;              // a level outside the table is a caller error like an index outside the store
        } else {
            thr_noise1 = a.level_thr[2 * lv];
            thr_noise2 = a.level_thr[2 * lv + 1];
        }
    }
    // a caller error (an index outside the store, or a level outside the table): the empty graph, wave-uniform exit before any barrier
    if (k < 0 || k >= a.M) {
        for (int i = lane; i < N * W; i += PG_THREADS) a.bits1[off + i] = a.bits2[off + i] = 0;
        if (a.nvalid && lane == 0) a.nvalid[blockIdx.x] = 0;
        return;
    }
    const unsigned *src = a.parents + k * N * W;
    const int n = a.sizes ? min(max(a.sizes[k], 0), N) : N;
    if (a.seconds) {             // a stored second side: both sides as they are
        const unsigned *src2 = a.seconds + k * N * W;
        for (int i = lane; i < N * W; i += PG_THREADS) {
            a.bits1[off + i] = src[i];
            a.bits2[off + i] = src2[i];
        }
        if (a.nvalid && lane == 0) a.nvalid[blockIdx.x] = n;
        return;
    }
    const Pair pr{a.seed, (unsigned long long)k};
    unsigned *rp = smem, *rq = smem + N * W;
    unsigned short *edges = (unsigned short *)(rq + N * W);
    const bool swap = a.noise_model == FGNN_PAIRGEN_EDGE_SWAP;
    for (int i = lane; i < N * W; i += PG_THREADS) {
        const unsigned w = src[i];
        rp[i] = w;
        rq[i] = swap ? w : 0;
    }
    __syncthreads();

    if (swap) {
        if (edge_count(rp, W, n) > a.emax) {      // more edges than the list holds (a caller error): the empty graph
            for (int i = lane; i < N * W; i += PG_THREADS) a.bits1[off + i] = a.bits2[off + i] = 0;
            if (a.nvalid && lane == 0) a.nvalid[blockIdx.x] = 0;
            return;
        }
        const int me = edge_list(rp, W, n, edges);
        __syncthreads();
        noise_edge_swap(rq, W, edges, me, pr, thr_noise1);
    } else {
        noise_erdos_renyi(rp, rq, W, n, N, pr, thr_noise1, thr_noise2);
    }
    __syncthreads();

    for (int i = lane; i < N * W; i += PG_THREADS) {
        a.bits1[off + i] = rp[i];
        a.bits2[off + i] = rq[i];
    }
    if (a.nvalid && lane == 0) a.nvalid[blockIdx.x] = n;
}

LdsAttrCache g_pairstore_lds;

}  // namespace

extern "C" int fgnn_pairstore_supported(int N, int noise_model) {
    return N >= 1 && N <= FGNN_PAIRGEN_MAX_N && noise_model >= 0 && noise_model <= 1;
}

extern "C" int fgnn_pairstore_gather(const fgnn_pairstore_args *args, void *stream) {
    FGNN_CHECK(args, "fgnn_pairstore_gather: NULL arguments");
    const fgnn_pairstore_args &a = *args;
    const bool levels = a.level_thr || a.level || a.K;
    const bool noisy = !a.seconds;
    FGNN_CHECK(fgnn_pairstore_supported(a.N, noisy ? a.noise_model : 0), "fgnn_pairstore_gather: unsupported N=%d noise_model=%d", a.N,
               a.noise_model);
    FGNN_CHECK(a.B >= 0 && a.M >= 1 && (a.index || a.first >= 0) && a.parents && a.bits1 && a.bits2,
               "fgnn_pairstore_gather: bad arguments (B=%d, M=%lld, first=%lld)", a.B, a.M, a.first);
    FGNN_CHECK(!levels || noisy, "fgnn_pairstore_gather: noise levels with a stored second side");
    FGNN_CHECK(!levels || (a.K >= 1 && a.K <= FGNN_MAX_LEVELS), "fgnn_pairstore_gather: K=%d levels outside [1, %d]", a.K, FGNN_MAX_LEVELS);
    FGNN_CHECK(!levels || (a.level_thr && (a.level || a.B == 0)), "fgnn_pairstore_gather: NULL threshold table or level list");
    FGNN_CHECK(!noisy || levels || (a.thr_noise1 <= THR_ONE && a.thr_noise2 <= THR_ONE), "fgnn_pairstore_gather: thresholds outside [0, 2^32]");
    const int N = a.N, W = (N + 31) / 32;
    const bool swap = noisy && a.noise_model == FGNN_PAIRGEN_EDGE_SWAP;
    FGNN_CHECK(!swap || (a.emax >= 0 && a.emax <= N * (N - 1) / 2), "fgnn_pairstore_gather: emax=%d outside [0, N (N - 1) / 2]", a.emax);
    if (a.B == 0) return 0;
    const size_t lds = noisy ? (size_t)2 * N * W * 4 + (swap ? (size_t)((a.emax + 1) & ~1) * 2 : 0) : 0;
    FGNN_CHECK(lds <= 160 * 1024, "fgnn_pairstore_gather: %zu bytes of LDS needed", lds);
    FGNN_CHECK(fgnn_raise_lds(g_pairstore_lds, (const void *)pairstore_kernel, lds), "fgnn_pairstore_gather: cannot raise LDS to %zu bytes", lds);
    hipLaunchKernelGGL(pairstore_kernel, dim3((unsigned)a.B), dim3(PG_THREADS), lds, (hipStream_t)stream, a);
    FGNN_LAUNCH_CHECK();
    return 0;
}
