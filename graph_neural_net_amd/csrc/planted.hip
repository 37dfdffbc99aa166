// Planted permutations (include/fgnn_hip.h; graph_neural_net_amd/planted.py): a uniform permutation per pair from the pair's own
// Philox stream, the relabelling out[pi(i)][pi(j)] = in[i][j] of bit rows and of dense fp32 planes, and the two counts that score a
// matching against labels[i] = pi(i) instead of against the identity.  tests/planted_ref.py restates all of it in numpy, bit for bit.
//
// Everything here is latency work on at most 256 vertices: one wave or one small workgroup per pair, the permutation and its inverse
// in LDS.  An inverse is built by scatter (inv[labels[i]] = i for i < n, -1 elsewhere), so a labels row that is no permutation of
// [0, n) never indexes out of bounds: a column nobody maps to reads as an empty source (zeros).
#include "fgnn_rows.h"
#include "fgnn_philox.h"

namespace {

constexpr int PL_MAX_N = FGNN_PLANTED_MAX_N;
constexpr int PL_THREADS = 256;
constexpr int PL_SLAB = 16;                // output rows per workgroup of the dense relabelling

// inv[m] = i with labels[i] = m (i < n), -1 for every other m < PL_MAX_N; ends with a barrier
DEVI void stage_inverse(int *inv, const int *labels, int n, int tid, int nthreads) {
    for (int m = tid; m < PL_MAX_N; m += nthreads) inv[m] = -1;
    __syncthreads();
    for (int i = tid; i < n; i += nthreads) {
        const int l = labels[i];
        if (l >= 0 && l < n) inv[l] = i;
    }
    __syncthreads();
}

// One wave per pair.  Fisher-Yates from the top: for k = n-1 .. 1, j = (u32_k (k + 1)) >> 32 with u32_k draw k of stream
// FGNN_PLANTED_STREAM, swap p[k], p[j].  The draws of 64 steps are made one per lane and read back by readlane; the swaps are
// wave-uniform code on LDS (lane 0 stores; a wave's LDS accesses complete in issue order, so the next step's reads see them).
__global__ __launch_bounds__(64) void planted_perm_kernel(unsigned long long seed, long long first, const long long *index,
                                                          const int *nvalid, int N, int *labels) {
    __shared__ int p[PL_MAX_N];
    const int b = blockIdx.x, lane = threadIdx.x;
    const long long k = index ? index[b] : first + b;
    int *out = labels + (long long)b * N;
    if (k < 0) {                 // a caller error, as in fgnn_pairgen_indexed: the empty permutation (wave-uniform exit)
        for (int i = lane; i < N; i += 64) out[i] = -1;
        return;
    }
    const int n = corner_of(nvalid, b, N);
    const Pair pr{seed, (unsigned long long)k};
    for (int i = lane; i < n; i += 64) p[i] = i;
    __syncthreads();
    for (int top = n - 1; top >= 1; top -= 64) {
        const int i = top - lane;
        const int rj = i >= 1 ? below(pr.draw(FGNN_PLANTED_STREAM, (unsigned long long)i), i + 1) : 0;
        const int cnt = min(64, top);
        for (int l = 0; l < cnt; ++l) {
            const int ii = top - l, j = __builtin_amdgcn_readlane(rj, l);
            const int pi = uni(p[ii]), pj = uni(p[j]);
            if (lane == 0) {
                p[ii] = pj;
                p[j] = pi;
            }
        }
    }
    __syncthreads();
    for (int i = lane; i < N; i += 64) out[i] = p[i < n ? i : 0] | (i < n ? 0 : -1);
}

// One workgroup per pair: the bit matrix and the inverse permutation in LDS, one wave per output row r; lane l tests bit
// in[inv r][inv c] for c = l, l + 64, ...; the ballot is the output word pair.  Output words are written for every row and word of
// the pair, zero outside the n x n corner whatever the input holds there.  out may be in: the input is staged before any store.
__global__ __launch_bounds__(PL_THREADS) void relabel_bits_kernel(const unsigned *in, const int *labels, const int *nvalid, int N,
                                                                  unsigned *out) {
    __shared__ unsigned rows[PL_MAX_N * (PL_MAX_N / 32)];
    __shared__ int inv[PL_MAX_N];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = (N + 31) >> 5, n = corner_of(nvalid, b, N);
    const long long off = (long long)b * N * W;
    for (int i = tid; i < N * W; i += PL_THREADS) rows[i] = in[off + i];
    stage_inverse(inv, labels + (long long)b * N, n, tid, PL_THREADS);
    for (int r = wave; r < N; r += PL_THREADS / 64) {
        const int ir = r < n ? inv[r] : -1;                        // wave-uniform
        for (int w0 = 0; w0 < W; w0 += 2) {
            const int c = 32 * w0 + lane;                          // < 256: inside inv
            const int ic = c < n ? inv[c] : -1;
            const bool live = ir >= 0 && ic >= 0;
            const unsigned word = rows[live ? ir * W + (ic >> 5) : 0];
            const unsigned long long m = __ballot(live && ((word >> (ic & 31)) & 1u));
            if (lane == 0) {
                out[off + (long long)r * W + w0] = (unsigned)m;
                if (w0 + 1 < W) out[off + (long long)r * W + w0 + 1] = (unsigned)(m >> 32);
            }
        }
    }
}

// grid (ceil(ld / PL_SLAB), B), 4 waves: a workgroup owns PL_SLAB output rows of every channel of one pair, a wave one row at a time.
// The source row inv[r] is loaded along j (coalesced; lanes past the corner, and every lane of a row without a source, use the
// out-of-range buffer offset and receive 0) into the wave's own LDS row, read back at inv[j], and stored along j: all ld columns of
// all ld rows are written, exact zeros outside the corner.  The LDS row is private to the wave, whose LDS accesses complete in issue
// order: no barrier inside the loop.
__global__ __launch_bounds__(PL_THREADS) void relabel_dense_kernel(const float *in, const int *labels, const int *nvalid, int B, int C,
                                                                   int ld, int NL, float *out) {
    __shared__ int inv[PL_MAX_N];
    __shared__ float row[PL_THREADS / 64][PL_MAX_N];
    const int b = blockIdx.y, r0 = blockIdx.x * PL_SLAB, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = corner_of(nvalid, b, min(ld, NL));
    stage_inverse(inv, labels + (long long)b * NL, n, tid, PL_THREADS);
    const View v = make_view(in, (long long)C * ld * ld, (long long)ld * ld, B);
    float *mine = row[wave];
    for (int c = 0; c < C; ++c) {
        for (int r = r0 + wave; r < min(r0 + PL_SLAB, ld); r += PL_THREADS / 64) {
            const int ir = r < n ? inv[r] : -1;                    // wave-uniform
            const int soff = b * v.gs4 + c * v.ld4 + max(ir, 0) * ld * 4;
            for (int j = lane; j < ld; j += 64) mine[j] = buf_load(v, (ir >= 0 && j < n) ? j * 4 : OOB_OFF, soff);
            __builtin_amdgcn_wave_barrier();
            float *o = out + (((long long)b * C + c) * ld + r) * ld;
            for (int j = lane; j < ld; j += 64) {
                const int ij = j < n ? inv[j] : -1;
                const unsigned keep = ij >= 0 ? 0xffffffffu : 0u;
                o[j] = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, mine[max(ij, 0)]) & keep);
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// one wave per pair: #{i < n : assign[i] == labels[i]}
__global__ __launch_bounds__(64) void count_matches_kernel(const int *assign, const int *labels, const int *nvalid, int N, int *correct) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = corner_of(nvalid, b, N);
    int cnt = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const bool hit = i < n && assign[(long long)b * N + min(i, n - 1)] == labels[(long long)b * N + min(i, n - 1)];
        cnt += __popcll(__ballot(hit));
    }
    if (lane == 0) correct[b] = cnt;
}

// accuracy_max_kernel (train_ops.hip) with a label row: the same arg-max -- row_argmax (fgnn_rows.h), written out here because the
// call moves one instruction of this kernel -- compared with labels[i] instead of i.
__global__ __launch_bounds__(256) void accuracy_max_labels_kernel(const float *scores, const int *labels, const int *nvalid, int N,
                                                                  int *correct) {
    __shared__ int red[4];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nv = corner_of(nvalid, b, N);
    const float *S = scores + (long long)b * N * N;
    int cnt = 0;
    for (int i = wave; i < nv; i += 4) {
        float best = -INFINITY;
        int bj = 0x7fffffff;
        for (int j = lane; j < nv; j += WAVE) {          // ascending j: an equal later value never replaces
            const float v = S[(long long)i * N + j];
            if (bj == 0x7fffffff || (best == best && (v > best || v != v))) {
                best = v;
                bj = j;
            }
        }
        for (int o = 32; o > 0; o >>= 1) {               // ties towards the smaller index
            const float ob = __shfl_xor(best, o);
            const int oj = __shfl_xor(bj, o);
            const bool onan = ob != ob, bnan = best != best;
            if (onan ? (!bnan || oj < bj) : (!bnan && (ob > best || (ob == best && oj < bj)))) {
                best = ob;
                bj = oj;
            }
        }
        if (bj == labels[(long long)b * N + i]) ++cnt;
    }
    if (lane == 0) red[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) correct[b] = red[0] + red[1] + red[2] + red[3];
}

// One wave per pair: min(count, n) rows of labels, uniform without replacement -- the top `cnt` steps of planted_perm_kernel's
// Fisher-Yates on the identity, on stream FGNN_SEEDS_STREAM: for k = n-1 .. n-cnt, j = (u32_k (k + 1)) >> 32, swap p[k], p[j]; the
// rows revealed are p[n-cnt .. n-1].  seeds[i] = labels[i] on them, -1 on every other entry.
__global__ __launch_bounds__(64) void reveal_seeds_kernel(unsigned long long seed, long long first, const long long *index,
                                                          const int *labels, const int *nvalid, int N, int count, int *seeds) {
    __shared__ int p[PL_MAX_N], chosen[PL_MAX_N];
    const int b = blockIdx.x, lane = threadIdx.x;
    const long long k = index ? index[b] : first + b;
    int *out = seeds + (long long)b * N;
    if (k < 0) {                 // a caller error, as in planted_perm_kernel: nothing revealed (wave-uniform exit)
        for (int i = lane; i < N; i += 64) out[i] = -1;
        return;
    }
    const int n = corner_of(nvalid, b, N), low = n - min(max(count, 0), n), last = max(low, 1);
    const Pair pr{seed, (unsigned long long)k};
    for (int i = lane; i < n; i += 64) {
        p[i] = i;
        chosen[i] = 0;
    }
    __syncthreads();
    for (int top = n - 1; top >= last; top -= 64) {
        const int i = top - lane;
        const int rj = i >= last ? below(pr.draw(FGNN_SEEDS_STREAM, (unsigned long long)i), i + 1) : 0;
        const int cnt = min(64, top - last + 1);
        for (int l = 0; l < cnt; ++l) {
            const int ii = top - l, j = __builtin_amdgcn_readlane(rj, l);
            const int pi = uni(p[ii]), pj = uni(p[j]);
            if (lane == 0) {
                p[ii] = pj;
                p[j] = pi;
            }
        }
    }
    __syncthreads();
    for (int i = low + lane; i < n; i += 64) chosen[p[i]] = 1;
    __syncthreads();
    for (int i = lane; i < N; i += 64) out[i] = (i < n && chosen[i]) ? labels[(long long)b * N + i] : -1;
}

}  // namespace

extern "C" int fgnn_reveal_seeds(unsigned long long seed, long long first, const long long *index, const int *labels, const int *nvalid,
                                 int B, int N, int count, int *seeds, void *stream) {
    FGNN_CHECK(B >= 0 && N >= 1 && N <= FGNN_PLANTED_MAX_N, "fgnn_reveal_seeds: B=%d, N=%d (1 <= N <= %d)", B, N, FGNN_PLANTED_MAX_N);
    FGNN_CHECK(index || first >= 0, "fgnn_reveal_seeds: first=%lld < 0", first);
    FGNN_CHECK(count >= 0, "fgnn_reveal_seeds: count=%d < 0", count);
    if (B == 0) return 0;
    FGNN_CHECK(labels && seeds, "fgnn_reveal_seeds: NULL labels or output");
    hipLaunchKernelGGL(reveal_seeds_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, seed, first, index, labels, nvalid, N, count,
                       seeds);
    FGNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int fgnn_planted_perm(unsigned long long seed, long long first, const long long *index, const int *nvalid, int B, int N,
                                 int *labels, void *stream) {
    FGNN_CHECK(B >= 0 && N >= 1 && N <= FGNN_PLANTED_MAX_N, "fgnn_planted_perm: B=%d, N=%d (1 <= N <= %d)", B, N, FGNN_PLANTED_MAX_N);
    FGNN_CHECK(index || first >= 0, "fgnn_planted_perm: first=%lld < 0", first);
    if (B == 0) return 0;
    FGNN_CHECK(labels, "fgnn_planted_perm: NULL output");
    hipLaunchKernelGGL(planted_perm_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, seed, first, index, nvalid, N, labels);
    FGNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int fgnn_relabel_bits(const unsigned *in, const int *labels, const int *nvalid, int B, int N, unsigned *out, void *stream) {
    FGNN_CHECK(in && labels && out && B > 0, "fgnn_relabel_bits: bad arguments");
    FGNN_CHECK(N >= 1 && N <= FGNN_PLANTED_MAX_N, "fgnn_relabel_bits: 1 to %d vertices per graph (got %d)", FGNN_PLANTED_MAX_N, N);
    hipLaunchKernelGGL(relabel_bits_kernel, dim3((unsigned)B), dim3(PL_THREADS), 0, (hipStream_t)stream, in, labels, nvalid, N, out);
    FGNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int fgnn_relabel_dense(const float *in, const int *labels, const int *nvalid, int B, int C, int ld, int NL, float *out,
                                  void *stream) {
    FGNN_CHECK(in && labels && out && in != out && B > 0 && C > 0, "fgnn_relabel_dense: bad arguments");
    FGNN_CHECK(B <= 65535, "fgnn_relabel_dense: at most 65535 pairs per call (got %d)", B);
    FGNN_CHECK(ld >= 1 && ld <= FGNN_PLANTED_MAX_N && NL >= 1, "fgnn_relabel_dense: planes of 1 to %d rows (got %d), labels pitch %d",
               FGNN_PLANTED_MAX_N, ld, NL);
    FGNN_CHECK((long long)B * C * ld * ld * 4 <= 0x7fffffffll, "fgnn_relabel_dense: the batch must be smaller than 2 GiB");
    hipLaunchKernelGGL(relabel_dense_kernel, dim3((ld + PL_SLAB - 1) / PL_SLAB, B), dim3(PL_THREADS), 0, (hipStream_t)stream, in, labels,
                       nvalid, B, C, ld, NL, out);
    FGNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int fgnn_count_matches(const int *assign, const int *labels, const int *nvalid, int B, int N, int *correct, void *stream) {
    FGNN_CHECK(assign && labels && correct && B > 0 && N > 0, "fgnn_count_matches: bad arguments");
    hipLaunchKernelGGL(count_matches_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, assign, labels, nvalid, N, correct);
    FGNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int fgnn_accuracy_max_labels(const float *scores, const int *labels, const int *nvalid, int B, int N, int *correct,
                                        void *stream) {
    FGNN_CHECK(scores && labels && correct && B > 0 && N > 0, "fgnn_accuracy_max_labels: bad arguments");
    hipLaunchKernelGGL(accuracy_max_labels_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, scores, labels, nvalid, N, correct);
    FGNN_LAUNCH_CHECK();
    return 0;
}
