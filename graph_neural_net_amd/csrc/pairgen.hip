// QAP pair generation on the device (loaders/data_generator.py:38-125,175-219, QAP_Generator): one single-wave workgroup per
// pair builds the parent graph and its noisy copy as bit rows in LDS and stores both in the engine's wire format.
//
// Randomness is counter-based (fgnn_philox.h): raw 32-bit draw t of stream s of pair k is word t & 7 (low half first) of Philox4x64-10
// at counter (t >> 3, k, s, 0) under key (seed, 0), so a pair never depends on the launch that made it.  Events are u32 < thr,
// integers in [0, k) are (u32 * k) >> 32 (tests/pairgen_ref.py restates every step in numpy, bit for bit).
//
// The parallel parts (vertex count, Erdos-Renyi draws, noise, relabelling, stores) run across the 64 lanes; the serial chains
// (Regular's double-edge swaps, Barabasi-Albert attachment, EdgeSwap noise) are wave-uniform code on LDS, with their draws
// precomputed one per lane and read back by readlane.  Inside a chain LDS is written by single instructions of a few lanes
// (atomics without return: nothing waits for them); a wave's LDS accesses complete in issue order, so the next step's reads see
// those writes without a barrier.
//
// Which pair a workgroup builds is first + b (fgnn_pairgen) or index[b] (fgnn_pairgen_indexed); fgnn_epoch_index, at the end of the
// file, writes such an index list: a window of the shuffled order of an epoch.  fgnn_pairgen_levels
// takes the two noise thresholds of workgroup b from a table row level[b] instead of the launch arguments: the draws of a pair
// do not depend on the thresholds they are compared with, so one launch holds pairs of several noise levels (section 10.3).
#include <type_traits>

#include "fgnn_common.h"
#include "fgnn_pairgen_dev.h"
#include "fgnn_philox.h"

namespace {

DEVI void set_edge_one(unsigned *rows, int W, int i, int j) {      // one lane, both directions (LDS atomics without return)
    atomicOr(&rows[i * W + (j >> 5)], 1u << (j & 31));
    atomicOr(&rows[j * W + (i >> 5)], 1u << (i & 31));
}

DEVI int regular_degree(int n, double p) {
    int d = (int)(p * n);
    if ((n * d) & 1) d++;
    return d;
}
DEVI int ba_attachments(int n, double p) { return (int)(p * (n - 1) / 2.0); }

// Independent Bernoulli draws (event u32 < thr) of one stream at positions i N + j, i < j < n, as symmetric bits
DEVI void erdos_renyi(unsigned *rows, int W, int n, int N, const Pair &pr, int stream, unsigned long long thr) {
    const int lane = threadIdx.x;
    const int nq = (n * N + 7) >> 3;
    for (int q = lane; q < nq; q += PG_THREADS) {
        const P4 r = pr.block(stream, q);
        int i = (8 * q) / N, j = 8 * q - i * N;
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            if (j > i && j < n && word_of(r, w) < thr) set_edge(rows, W, i, j);
            if (++j == N) {
                j = 0;
                ++i;
            }
        }
    }
}

// Random d-regular graph (synthetic.random_regular's scheme): circulant seed, `steps` double-edge swaps, random relabelling
DEVI void random_regular(unsigned *rp, int W, int n, int d, int swaps_per_edge, const Pair &pr, unsigned short *edges,
                         unsigned char *perm, unsigned char *inv) {
    const int lane = threadIdx.x;
    const int m = n * d / 2, half = (d / 2) * n;
    for (int e = lane; e < m; e += PG_THREADS) {       // edge (s-1) n + i = {i, i+s}, then {i, i + n/2} for odd d
        int i, v;
        if (e < half) {
            i = e % n;
            v = (i + e / n + 1) % n;
        } else {
            i = e - half;
            v = i + n / 2;
        }
        const int a = min(i, v), b = max(i, v);
        edges[e] = (unsigned short)(a | (b << 8));
        set_edge(rp, W, a, b);
    }
    __syncthreads();
    const int steps = swaps_per_edge * m;
    for (int base = 0; base < steps; base += PG_THREADS) {
        const int s = base + lane;                       // swap s: draws 4 s .. 4 s + 2 = block s >> 1, words 4 (s & 1) ..
        const P4 r = pr.block(ST_CHAIN, (unsigned long long)(s >> 1));
        const unsigned long long x = (s & 1) ? r.v2 : r.v0, y = (s & 1) ? r.v3 : r.v1;
        const int ra = below((unsigned)x, m), rb = below((unsigned)(x >> 32), m), rf = (int)((unsigned)y >> 31);
        const int cnt = min(PG_THREADS, steps - base);
        // the edges of swap l + 1 are read while swap l is decided (one LDS round trip per swap); if swap l rewrites one of
        // them, the register copy is patched with the new value
        int A = __builtin_amdgcn_readlane(ra, 0), Bi = __builtin_amdgcn_readlane(rb, 0);
        int pe1 = edges[A], pe2 = edges[Bi];
        for (int l = 0; l < cnt; ++l) {
            const int e1 = uni(pe1), e2 = uni(pe2);
            const int nA = l + 1 < cnt ? __builtin_amdgcn_readlane(ra, min(l + 1, PG_THREADS - 1)) : 0;
            const int nB = l + 1 < cnt ? __builtin_amdgcn_readlane(rb, min(l + 1, PG_THREADS - 1)) : 0;
            pe1 = edges[nA];
            pe2 = edges[nB];
            const int u = e1 & 255, v = e1 >> 8;
            int s0 = e2 & 255, t0 = e2 >> 8;
            if (__builtin_amdgcn_readlane(rf, l)) {
                const int tmp = s0;
                s0 = t0;
                t0 = tmp;
            }
            const unsigned w1 = rp[u * W + (t0 >> 5)], w2 = rp[s0 * W + (v >> 5)];      // both reads in one round trip
            const int hit = uni(((w1 >> (t0 & 31)) | (w2 >> (v & 31))) & 1);
            if (A != Bi && u != t0 && s0 != v && u != s0 && v != t0 && !hit) {
                const int ea = min(u, t0) | (max(u, t0) << 8), eb = min(s0, v) | (max(s0, v) << 8);
                swap_edges(rp, W, u, v, s0, t0, edges, A, ea, Bi, eb);
                pe1 = nA == A ? ea : nA == Bi ? eb : pe1;
                pe2 = nB == A ? ea : nB == Bi ? eb : pe2;
            }
            A = nA;
            Bi = nB;
        }
    }
    // relabel: Fisher-Yates from the top (draw i of the relabel stream picks j in [0, i]), W'[a][b] = W[perm a][perm b]
    for (int i = lane; i < n; i += PG_THREADS) perm[i] = (unsigned char)i;
    __syncthreads();
    for (int top = n - 1; top >= 1; top -= PG_THREADS) {
        const int i = top - lane;
        const int rj = i >= 1 ? below(pr.draw(ST_RELABEL, (unsigned long long)i), i + 1) : 0;
        const int cnt = min(PG_THREADS, top);
        for (int l = 0; l < cnt; ++l) {
            const int ii = top - l, j = __builtin_amdgcn_readlane(rj, l);
            const int pi = uni(perm[ii]), pj = uni(perm[j]);
            if (lane == 0) {
                perm[ii] = (unsigned char)pj;
                perm[j] = (unsigned char)pi;
            }
        }
    }
    __syncthreads();
    for (int a = lane; a < n; a += PG_THREADS) inv[perm[a]] = (unsigned char)a;
    for (int i = lane; i < n * W; i += PG_THREADS) rp[i] = 0;
    __syncthreads();
    for (int e = lane; e < m; e += PG_THREADS) set_edge(rp, W, inv[edges[e] & 255], inv[edges[e] >> 8]);
    __syncthreads();
}

// networkx 3.x barabasi_albert_graph: star on m + 1 nodes, then each new node takes m distinct targets drawn from the
// repeated-nodes list (duplicates rejected); the list grows by the targets (in draw order) and m copies of the new node
DEVI void barabasi_albert(unsigned *rp, int W, int n, int m, const Pair &pr, unsigned char *rep, unsigned char *mark) {
    const int lane = threadIdx.x;
    for (int i = lane; i < m; i += PG_THREADS) {
        rep[i] = 0;
        rep[m + i] = (unsigned char)(i + 1);
        set_edge(rp, W, 0, i + 1);
    }
    for (int i = lane; i < n; i += PG_THREADS) mark[i] = 0;      // sources are >= 2
    __syncthreads();
    int len = 2 * m;
    long long t = 0, t0 = -PG_THREADS;
    unsigned rr = 0;
    for (int source = m + 1; source < n; ++source) {
        int cnt = 0;
        while (cnt < m) {
            if (t - t0 >= PG_THREADS) {
                t0 = t;
                rr = pr.draw(ST_CHAIN, (unsigned long long)(t0 + lane));
            }
            const unsigned u = __builtin_amdgcn_readlane(rr, (int)(t - t0));
            ++t;
            const int x = uni(rep[below(u, len)]);
            if (uni(mark[x]) != source) {
                if (lane == 0) {
                    mark[x] = (unsigned char)source;
                    rep[len + cnt] = (unsigned char)x;
                    set_edge_one(rp, W, source, x);
                }
                ++cnt;
            }
        }
        for (int i = lane; i < m; i += PG_THREADS) rep[len + m + i] = (unsigned char)source;
        len += 2 * m;
        __syncthreads();
    }
}

struct KArgs {
    fgnn_pairgen_args a;
    int emax;                    // edge-list entries in LDS
    const long long *index;      // INDEXED: the pair of workgroup b is index[b]
};
struct KArgsLevels : KArgs {     // LEVELS (index may be NULL: first + b)
    const unsigned long long *level_thr;      // (K, 2): thr_noise1, thr_noise2 of each level
    const int *level;                         // (B): the level of workgroup b
    int K;
};

// INDEXED: the pair of workgroup b is index[b] (fgnn_pairgen_indexed), else first + b (fgnn_pairgen: the kernel as it always was)
// LEVELS (fgnn_pairgen_levels; a kernel of its own, so that the other two keep their code and its placement): index[b] when there
// is an index, and the noise thresholds are row level[b] of the table, read once per workgroup (wave-uniform values)
template <bool INDEXED, bool LEVELS = false>
__global__ __launch_bounds__(PG_THREADS) void pairgen_kernel(std::conditional_t<LEVELS, KArgsLevels, KArgs> ka) {
    extern __shared__ unsigned smem[];
    const fgnn_pairgen_args &a = ka.a;
    const int N = a.N, W = (N + 31) >> 5, lane = threadIdx.x;
    long long k;
    unsigned long long thr_noise1 = a.thr_noise1, thr_noise2 = a.thr_noise2;
    if constexpr (LEVELS) {
        k = ka.index ? ka.index[blockIdx.x] : a.first + blockIdx.x;
        const int lv = ka.level[blockIdx.x];
        if (lv < 0 || lv >= ka.K) {
            k = -1;              // a level outside the table is a caller error like a negative index
        } else {
            thr_noise1 = ka.level_thr[2 * lv];
            thr_noise2 = ka.level_thr[2 * lv + 1];
        }
    } else {
        k = INDEXED ? ka.index[blockIdx.x] : a.first + blockIdx.x;
    }
    // a caller error (a negative index, or a level outside the table): the empty graph, wave-uniform exit before any barrier
    if ((INDEXED || LEVELS) && k < 0) {
        const long long off = (long long)blockIdx.x * N * W;
        for (int i = lane; i < N * W; i += PG_THREADS) a.bits1[off + i] = a.bits2[off + i] = 0;
        if (a.nvalid && lane == 0) a.nvalid[blockIdx.x] = 0;
        return;
    }
    const Pair pr{a.seed, (unsigned long long)k};
    unsigned *rp = smem, *rq = smem + N * W;
    unsigned char *perm = (unsigned char *)(rq + N * W), *inv = perm + 256;    // BA: mark = perm
    unsigned short *edges = (unsigned short *)(inv + 256);
    unsigned char *rep = (unsigned char *)(edges + ((ka.emax + 1) & ~1));
    for (int i = lane; i < 2 * N * W; i += PG_THREADS) smem[i] = 0;

    // vertex count: n ~ Binomial(N, vertex_proba) as N Bernoulli draws; n < 2 redrawn from the next N positions
    const int n = vertex_count(pr, N, a.thr_vertex, lane);      // (fgnn_pairgen_dev.h: wigner.hip draws the same count)
    __syncthreads();

    if (a.family == FGNN_PAIRGEN_REGULAR)
        random_regular(rp, W, n, regular_degree(n, a.edge_density), a.swaps_per_edge, pr, edges, perm, inv);
    else if (a.family == FGNN_PAIRGEN_BARABASI_ALBERT)
        barabasi_albert(rp, W, n, ba_attachments(n, a.edge_density), pr, rep, perm);
    else
        erdos_renyi(rp, W, n, N, pr, ST_PARENT, a.thr_edge);
    __syncthreads();

    if (a.noise_model == FGNN_PAIRGEN_EDGE_SWAP) {
        for (int i = lane; i < N * W; i += PG_THREADS) rq[i] = rp[i];
        const int me = edge_list(rp, W, n, edges);
        __syncthreads();
        noise_edge_swap(rq, W, edges, me, pr, thr_noise1);
    } else {
        noise_erdos_renyi(rp, rq, W, n, N, pr, thr_noise1, thr_noise2);
    }
    __syncthreads();

    const long long off = (long long)blockIdx.x * N * W;
    for (int i = lane; i < N * W; i += PG_THREADS) {
        a.bits1[off + i] = rp[i];
        a.bits2[off + i] = rq[i];
    }
    if (a.nvalid && lane == 0) a.nvalid[blockIdx.x] = n;
}

int host_regular_degree(int n, double p) {
    int d = (int)(p * n);
    if ((n * d) & 1) d++;
    return d;
}

LdsAttrCache g_pairgen_lds, g_pairgen_indexed_lds, g_pairgen_levels_lds;

}  // namespace

extern "C" int fgnn_pairgen_supported(int N, int family, int noise_model) {
    return N >= 1 && N <= FGNN_PAIRGEN_MAX_N && family >= 0 && family <= 2 && noise_model >= 0 && noise_model <= 1;
}

// which entry point a launch serves: it selects the kernel instance and what the launch reads beside the arguments
enum class PairgenForm {
    CONTIGUOUS,      // fgnn_pairgen: pair first + b
    INDEXED,         // fgnn_pairgen_indexed: pair index[b]
    LEVELS           // fgnn_pairgen_levels: pair index[b], or first + b without an index; noise thresholds from the level table
};
struct LevelTable {
    const unsigned long long *thr;      // (K, 2)
    int K;
    const int *level;                   // (B)
};

// the checks and the launch shared by the three entry points (levels: the table of PairgenForm::LEVELS, else NULL)
static int launch_pairgen(PairgenForm form, const fgnn_pairgen_args *args, const long long *index, const LevelTable *levels,
                          void *stream) {
    FGNN_CHECK(args, "fgnn_pairgen: NULL arguments");
    const fgnn_pairgen_args &a = *args;
    const bool by_index = form == PairgenForm::INDEXED || (form == PairgenForm::LEVELS && index);
    const bool own_noise = form != PairgenForm::LEVELS;      // the noise thresholds of the arguments are used
    FGNN_CHECK(fgnn_pairgen_supported(a.N, a.family, a.noise_model), "fgnn_pairgen: unsupported N=%d family=%d noise_model=%d",
               a.N, a.family, a.noise_model);
    FGNN_CHECK(a.B >= 0 && (by_index || a.first >= 0) && a.bits1 && a.bits2, "fgnn_pairgen: bad arguments (B=%d, first=%lld)", a.B,
               a.first);
    FGNN_CHECK(form != PairgenForm::INDEXED || index || a.B == 0, "fgnn_pairgen_indexed: NULL index for B=%d pairs", a.B);
    FGNN_CHECK(a.edge_density >= 0.0 && a.edge_density < 1.0, "fgnn_pairgen: edge_density %g outside [0, 1)", a.edge_density);
    FGNN_CHECK(a.swaps_per_edge >= 0 && a.swaps_per_edge <= 10000, "fgnn_pairgen: swaps_per_edge %d outside [0, 10000]",
               a.swaps_per_edge);
    FGNN_CHECK(a.thr_edge <= THR_ONE && (!own_noise || (a.thr_noise1 <= THR_ONE && a.thr_noise2 <= THR_ONE)) && a.thr_vertex <= THR_ONE &&
                   a.thr_vertex > 0, "fgnn_pairgen: thresholds outside [0, 2^32] (vertex threshold > 0)");
    FGNN_CHECK(a.thr_vertex == THR_ONE || a.N >= 2, "fgnn_pairgen: a binomial vertex count needs N >= 2");
    const int N = a.N;
    long long emax = 0, rep = 0;
    if (a.family == FGNN_PAIRGEN_REGULAR) {
        for (int n = (a.thr_vertex == THR_ONE ? N : 2); n <= N; ++n) emax = std::max(emax, (long long)n * host_regular_degree(n, a.edge_density) / 2);
    } else if (a.family == FGNN_PAIRGEN_BARABASI_ALBERT) {
        const int m = (int)(a.edge_density * (N - 1) / 2.0);
        FGNN_CHECK(a.thr_vertex == THR_ONE, "fgnn_pairgen: BarabasiAlbert needs a constant vertex count");
        FGNN_CHECK(m >= 1 && m < N, "fgnn_pairgen: BarabasiAlbert with m=%d attachments on N=%d vertices", m, N);
        emax = (long long)m * (N - m);
        rep = 2 * emax;
    }
    if (a.noise_model == FGNN_PAIRGEN_EDGE_SWAP && a.family == FGNN_PAIRGEN_ERDOS_RENYI) emax = (long long)N * (N - 1) / 2;
    if (a.B == 0) return 0;
    const int W = (N + 31) / 32;
    const size_t lds = (size_t)2 * N * W * 4 + 512 + (size_t)((emax + 1) & ~1ll) * 2 + (size_t)rep;
    FGNN_CHECK(lds <= 160 * 1024, "fgnn_pairgen: %zu bytes of LDS needed", lds);
    const dim3 grid((unsigned)a.B), block(PG_THREADS);
    KArgsLevels ka;      // (the first two forms pass its KArgs part)
    ka.a = a;
    ka.emax = (int)emax;
    ka.index = by_index ? index : nullptr;
    switch (form) {
    case PairgenForm::CONTIGUOUS:
        FGNN_CHECK(fgnn_raise_lds(g_pairgen_lds, (const void *)pairgen_kernel<false>, lds), "fgnn_pairgen: cannot raise LDS to %zu bytes", lds);
        hipLaunchKernelGGL(pairgen_kernel<false>, grid, block, lds, (hipStream_t)stream, (KArgs)ka);
        break;
    case PairgenForm::INDEXED:
        FGNN_CHECK(fgnn_raise_lds(g_pairgen_indexed_lds, (const void *)pairgen_kernel<true>, lds), "fgnn_pairgen: cannot raise LDS to %zu bytes",
                   lds);
        hipLaunchKernelGGL(pairgen_kernel<true>, grid, block, lds, (hipStream_t)stream, (KArgs)ka);
        break;
    case PairgenForm::LEVELS:
        FGNN_CHECK(fgnn_raise_lds(g_pairgen_levels_lds, (const void *)pairgen_kernel<true, true>, lds),
                   "fgnn_pairgen_levels: cannot raise LDS to %zu bytes", lds);
        ka.level_thr = levels->thr;
        ka.level = levels->level;
        ka.K = levels->K;
        hipLaunchKernelGGL((pairgen_kernel<true, true>), grid, block, lds, (hipStream_t)stream, ka);
        break;
    }
    FGNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int fgnn_pairgen(const fgnn_pairgen_args *args, void *stream) {
    return launch_pairgen(PairgenForm::CONTIGUOUS, args, nullptr, nullptr, stream);
}

extern "C" int fgnn_pairgen_indexed(const fgnn_pairgen_args *args, const long long *index, void *stream) {
    return launch_pairgen(PairgenForm::INDEXED, args, index, nullptr, stream);
}

extern "C" int fgnn_pairgen_levels(const fgnn_pairgen_args *args, const long long *index, const unsigned long long *level_thr, int K,
                                   const int *level, void *stream) {
    FGNN_CHECK(K >= 1 && K <= FGNN_MAX_LEVELS, "fgnn_pairgen_levels: K=%d levels outside [1, %d]", K, FGNN_MAX_LEVELS);
    FGNN_CHECK(level_thr && (level || !args || args->B == 0), "fgnn_pairgen_levels: NULL threshold table or level list");
    const LevelTable levels{level_thr, K, level};
    return launch_pairgen(PairgenForm::LEVELS, args, index, &levels, stream);
}

// ---- the order of a shuffled epoch (include/fgnn_hip.h; tests/epoch_ref.py restates it in numpy, bit for bit) -----------------
namespace {

constexpr int EP_THREADS = 256;

// one pass of the balanced Feistel network on 2 h bits: a bijection of [0, 4^h) whatever the round function returns
DEVI unsigned long long feistel(unsigned long long x, int h, unsigned long long seed, unsigned long long epoch) {
    const unsigned long long mask = (1ull << h) - 1;
    unsigned long long L = x >> h, R = x & mask;
#pragma unroll
    for (int r = 0; r < FGNN_EPOCH_ROUNDS; ++r) {
        const unsigned long long f = philox(epoch, (unsigned long long)r, R, seed, FGNN_EPOCH_STREAM).v0 & mask;
        const unsigned long long t = L ^ f;
        L = R;
        R = t;
    }
    return (L << h) | R;
}

__global__ __launch_bounds__(EP_THREADS) void epoch_index_kernel(unsigned long long seed, unsigned long long epoch,
                                                                unsigned long long M, unsigned long long first_pos, int count, int h,
                                                                long long *out) {
    const int i = blockIdx.x * EP_THREADS + threadIdx.x;
    if (i >= count) return;
    unsigned long long x = (first_pos + (unsigned long long)i) % M;
    do x = feistel(x, h, seed, epoch);      // x < M lies on a cycle of the bijection that comes back below M: the walk ends
    while (x >= M);
    out[i] = (long long)x;
}

}  // namespace

extern "C" int fgnn_epoch_index(unsigned long long seed, unsigned long long epoch, long long M, long long first_pos, long long count,
                                long long *out, void *stream) {
    FGNN_CHECK(M >= 1 && M <= (1ll << FGNN_EPOCH_MAX_LOG2_M), "fgnn_epoch_index: M=%lld outside [1, 2^%d]", M, FGNN_EPOCH_MAX_LOG2_M);
    FGNN_CHECK(count >= 0 && count < (1ll << 31), "fgnn_epoch_index: count=%lld outside [0, 2^31)", count);
    FGNN_CHECK(first_pos >= 0 && first_pos <= (1ll << 62), "fgnn_epoch_index: first_pos=%lld outside [0, 2^62]", first_pos);
    if (count == 0) return 0;
    FGNN_CHECK(out, "fgnn_epoch_index: NULL output");
    int bits = 0;
    while ((1ll << bits) < M) ++bits;
    const int h = std::max(1, (bits + 1) / 2);
    hipLaunchKernelGGL(epoch_index_kernel, dim3((unsigned)((count + EP_THREADS - 1) / EP_THREADS)), dim3(EP_THREADS), 0,
                       (hipStream_t)stream, seed, epoch, (unsigned long long)M, (unsigned long long)first_pos, (int)count, h, out);
    FGNN_LAUNCH_CHECK();
    return 0;
}
