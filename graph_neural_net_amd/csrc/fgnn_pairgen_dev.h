// Device code shared by the pair kernels (pairgen.hip: generated parents; pairstore.hip: stored parents): bit rows in LDS, and the
// two noise functions of loaders/data_generator.py:79-116 on a parent graph that is already there.  Written for ONE wave per
// workgroup: the loops stride by the 64 lanes, and inside the serial chains LDS is written by single instructions of a few lanes
// (atomics without return: nothing waits for them); a wave's LDS accesses complete in issue order, so the next step's reads see
// those writes without a barrier.  The streams, positions and thresholds are documented in graph_neural_net_amd/pairgen.py and
// restated in numpy by tests/pairgen_ref.py.
#pragma once
#include "fgnn_common.h"
#include "fgnn_philox.h"

namespace {

constexpr int PG_THREADS = 64;
enum { ST_SIZE = 0, ST_PARENT, ST_NOISE1, ST_NOISE2, ST_RELABEL, ST_CHAIN };
constexpr unsigned long long THR_ONE = 1ull << 32;

constexpr int MAX_SIZE_DRAWS = 64;       // n < 2 is redrawn at most this often, then n = 2 (tests/pairgen_ref.py)

// The vertex count of pair `pr` (pairgen.hip, wigner.hip): N, or n ~ Binomial(N, vertex_proba) as N Bernoulli draws of stream
// ST_SIZE; n < 2 is redrawn from the next N positions.  Called by every lane of one wave (lane: its number); wave-uniform result
DEVI int vertex_count(const Pair &pr, int N, unsigned long long thr_vertex, int lane) {
    int n = N;
    if (thr_vertex < THR_ONE) {
        n = 2;
        for (int r = 0; r < MAX_SIZE_DRAWS; ++r) {
            int c = 0;
            for (int b = 0; b < N; b += PG_THREADS) {
                const int i = b + lane;
                c += __popcll(__ballot(i < N && pr.draw(ST_SIZE, (unsigned long long)(r * N + i)) < thr_vertex));
            }
            if (c >= 2) {
                n = c;
                break;
            }
        }
    }
    return n;
}

DEVI int bit(const unsigned *rows, int W, int i, int j) { return uni((rows[i * W + (j >> 5)] >> (j & 31)) & 1); }
DEVI void set_edge(unsigned *rows, int W, int i, int j) {           // any lane, both directions
    atomicOr(&rows[i * W + (j >> 5)], 1u << (j & 31));
    atomicOr(&rows[j * W + (i >> 5)], 1u << (i & 31));
}
// The double-edge swap (u, v), (s, t) -> (u, t), (s, v) on four distinct vertices: the 8 bits it changes toggled by lanes 0-7 in
// ONE atomic xor (some may share a word), plus lanes 8 / 9 storing the two edge-list entries (wave-uniform call)
DEVI void swap_edges(unsigned *rows, int W, int u, int v, int s, int t, unsigned short *edges, int A, int ea, int Bi, int eb) {
    const int lane = threadIdx.x;
    if (lane < 8) {
        const int p = lane >> 1;                                 // (u, v), (s, t) go; (u, t), (s, v) come
        const int a = (p & 1) ? s : u, b = (p == 0 || p == 3) ? v : t;
        const int r = (lane & 1) ? b : a, c = (lane & 1) ? a : b;
        atomicXor(&rows[r * W + (c >> 5)], 1u << (c & 31));
    } else if (edges && lane < 10) {
        edges[lane == 8 ? A : Bi] = (unsigned short)(lane == 8 ? ea : eb);
    }
}

// W' = (W & ~Z1) | (~W & Z2) on the upper triangle, mirrored (data_generator.py:79-87)
DEVI void noise_erdos_renyi(const unsigned *rp, unsigned *rq, int W, int n, int N, const Pair &pr, unsigned long long thr1,
                            unsigned long long thr2) {
    const int lane = threadIdx.x;
    const int nq = (n * N + 7) >> 3;
    for (int q = lane; q < nq; q += PG_THREADS) {
        const P4 r1 = pr.block(ST_NOISE1, q), r2 = pr.block(ST_NOISE2, q);
        int i = (8 * q) / N, j = 8 * q - i * N;
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            if (j > i && j < n) {
                const bool par = (rp[i * W + (j >> 5)] >> (j & 31)) & 1;
                if (par ? word_of(r1, w) >= thr1 : word_of(r2, w) < thr2) set_edge(rq, W, i, j);
            }
            if (++j == N) {
                j = 0;
                ++i;
            }
        }
    }
}

// The (u < v) edges of `rows` in row-major order -> edges[] (u | v << 8); returns their count (wave-uniform)
DEVI int edge_list(const unsigned *rows, int W, int n, unsigned short *edges) {
    const int lane = threadIdx.x;
    int carry = 0;
    for (int rb = 0; rb < n; rb += PG_THREADS) {
        const int u = rb + lane;
        int c = 0;
        if (u < n)
            for (int w = 0; w < W; ++w) c += __popc(rows[u * W + w] & (32 * w > u ? ~0u : 32 * w + 31 <= u ? 0u : ~0u << (u - 32 * w + 1)));
        int x = c;
#pragma unroll
        for (int off = 1; off < PG_THREADS; off <<= 1) {
            const int y = __shfl_up(x, off);
            if (lane >= off) x += y;
        }
        int o = carry + x - c;
        if (u < n)
            for (int w = 0; w < W; ++w) {
                unsigned b = rows[u * W + w] & (32 * w > u ? ~0u : 32 * w + 31 <= u ? 0u : ~0u << (u - 32 * w + 1));
                while (b) {
                    const int j = 32 * w + __ffs(b) - 1;
                    b &= b - 1;
                    edges[o++] = (unsigned short)(u | (j << 8));
                }
            }
        carry += __shfl(x, PG_THREADS - 1);
    }
    return uni(carry);
}

DEVI void directed(const unsigned short *edges, int me, int i, int &s, int &t) {
    const int e = uni(edges[i < me ? i : i - me]);
    s = i < me ? (e & 255) : (e >> 8);
    t = i < me ? (e >> 8) : (e & 255);
}

// data_generator.py:89-116 on rq (a copy of the parent), edge list of the parent (row-major u < v, then the reversals):
// outer edge o fires on draw o of noise-1; inner edge i on draw o * 2m + i of noise-2; the first inner edge that fires and is
// swappable on the current graph is swapped; (u, v) is gone after it, so no later inner edge of the same o can be
DEVI void noise_edge_swap(unsigned *rq, int W, const unsigned short *edges, int me, const Pair &pr, unsigned long long thr) {
    const int lane = threadIdx.x;
    const int L = 2 * me;
    for (int ob = 0; ob < L; ob += PG_THREADS) {
        const int o = ob + lane;
        unsigned long long fire = __ballot(o < L && pr.draw(ST_NOISE1, (unsigned long long)o) < thr);
        while (fire) {
            const int oo = ob + __ffsll((long long)fire) - 1;
            fire &= fire - 1;
            int u, v;
            directed(edges, me, oo, u, v);
            if (!bit(rq, W, u, v)) continue;
            const long long pos0 = (long long)oo * L;
            const long long q0 = pos0 >> 3, q1 = (pos0 + L + 7) >> 3;
            for (long long qb = q0; qb < q1; qb += PG_THREADS) {
                const long long q = qb + lane;
                int best = -1;
                if (q < q1) {
                    const P4 r = pr.block(ST_NOISE2, (unsigned long long)q);
#pragma unroll
                    for (int w = 0; w < 8; ++w) {
                        const long long i = 8 * q + w - pos0;
                        if (best < 0 && i >= 0 && i < L && word_of(r, w) < thr) {
                            const int ii = (int)i;
                            const int e = edges[ii < me ? ii : ii - me];
                            const int s = ii < me ? (e & 255) : (e >> 8), t = ii < me ? (e >> 8) : (e & 255);
                            const bool has_st = (rq[s * W + (t >> 5)] >> (t & 31)) & 1;
                            const bool has_ut = (rq[u * W + (t >> 5)] >> (t & 31)) & 1;
                            const bool has_sv = (rq[s * W + (v >> 5)] >> (v & 31)) & 1;
                            if (has_st && u != t && s != v && !has_ut && !has_sv) best = ii;
                        }
                    }
                }
                const unsigned long long found = __ballot(best >= 0);
                if (found) {
                    const int i = __builtin_amdgcn_readlane(best, __ffsll((long long)found) - 1);
                    int s, t;
                    directed(edges, me, i, s, t);
                    swap_edges(rq, W, u, v, s, t, nullptr, 0, 0, 0, 0);
                    break;
                }
            }
        }
    }
}

}  // namespace
