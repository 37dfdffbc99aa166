// bf16 variant of the fused MlpBlock_Real backward for gfx950, one MLP per launch.  The per-tile algorithm and its rounding
// points are described in fgnn_bwd16.h, which also holds what this kernel shares with its mlp1 + mlp2 pair twin
// (mlp_bwd16_pair.hip): the LDS layout, the parked accumulator tiles, the per-graph record fetch, the phases of a tile (functions
// and FGNN_BWD16_* macros) and the host side.  This kernel's own: a second input slab (CB), ragged batches (SKIP), the slab-b
// gradient and the two forms of per-tile sums it emits with the slab-a gradient.
#include "fgnn_bwd16.h"

using namespace bwd16;

namespace {

// dx of slab s still to be added to (read-modify-write), requested with the tile's other loads.  Writes old##s; reads rmw_##s, lo4, c,
// vdx##s, roff.
#define LOAD_OLD_DX(s, S)                                                                                   \
    if constexpr (C##S >= 32) {                                                                             \
        if (rmw_##s) {                                                                                      \
            const int vo = lo4 + c.g * vdx##s.gs2;                                                          \
            _Pragma("unroll") for (int r = 0; r < 16; ++r) old##s[r] = buf_load_u32(vdx##s, vo, roff(r));   \
        }                                                                                                   \
    }
// v = R(d in_0 (+ old dx)) of slab s.  Writes v; reads d, wl, PK, lane, rmw_##s, old##s, GRP.
#define DX_VALUE(v, s)                                                                              \
    {                                                                                               \
        f32x16 acc = input_grad(wl, PK.off_wt0##s, d, lane);                                        \
        if (rmw_##s) {                                                                              \
            _Pragma("unroll") for (int r = 0; r < 16; ++r) acc[r] += half_of<GRP>(old##s[r]);       \
        }                                                                                           \
        pack_acc(v, acc);                                                                           \
    }

// SKIP (ragged batches with A.ranges): work-balanced tile range from fgnn_ragged_tile_ranges16; the waves step over tiles
// without a valid element (no contribution to the parameter gradients, dx not written there); such a tile only gets an empty
// S1/S2 (or trace-term) record.
template <int CA, int CB, int DEPTH, bool SKIP = false>
__global__ __launch_bounds__(64 * NWB, NWB / 4) void mlp_bwd16_kernel(const fgnn_mlp_bwd16_args A, const int tpg,
                                                                 const int total_tiles) {
    static_assert(DEPTH == 3, "built for depth_of_mlp = 3");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    using L = Bwd16Layout<CA, CB, DEPTH>;
    constexpr Pk16 PK = L::PK;
    constexpr int CIN = CA + CB;
    constexpr int XA = CA >= 32 ? 16 : 2, XB = CB >= 32 ? 16 : 2;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int PP = A.N * A.ldr;
    const View16 va = make_view16(A.a.ptr, A.a.gstride, A.a.ldp, A.G);
    const View16 vb = make_view16(A.b.ptr, A.b.gstride, A.b.ldp, A.G);
    const View16 vdy = make_view16(A.dy, A.dgstride, A.ldd, A.G);
    const View16 vz = make_view16(A.z, A.zgstride, A.ldz, A.G);
    const View16 vdxa = make_view16(A.dxa, A.dxa_gstride, A.dxa_ld, A.G);
    const View16 vdxb = make_view16(A.dxb, A.dxb_gstride, A.dxb_ld, A.G);

    float *wl = smem;
    const float *tail = wl + PK.bias_f;
    float *rec = smem + L::WEIGHT_F + wv * L::REC_F;
    float *recA = rec, *recB = rec + 64, *recK = rec + 128;
    const F16 ident = make_identity(lane);

    FGNN_BWD16_ACCUMULATORS
    FGNN_BWD16_TILE_RANGE
    const bool normA = (CA >= 32) && A.a.nrm != nullptr, normB = (CB >= 32) && A.b.nrm != nullptr;
    // per-tile sums of the slab-a gradient: for a normalised single slab {sum dx, sum dx (z_a - mean_a)} (the GraphNorm backward
    // sums of its producer); for the raw first slab of a two-slab MLP (mlp3: slab a = mult) {sum dx, sum dx * x_a} =
    // the trace term T = <dM, M> from which fgnn_chan_matmul_bwd16 derives the S2 sums of both its operands
    const bool emit = (CA == 32) && (CB == 0 ? normA : !normA) && A.dxa != nullptr && A.s12part != nullptr;

    {
        const float4 *src = reinterpret_cast<const float4 *>(A.packed);
        float4 *dst = reinterpret_cast<float4 *>(wl);
        for (int e = threadIdx.x; e < L::WEIGHT_F / 4; e += 64 * NWB) dst[e] = src[e];
    }
    unsigned xa[XA], xb[CB > 0 ? XB : 1];
    int cached_g = -1, cur_nv = A.N;
    float la_a = 1.f, la_b = 0.f, lb_a = 1.f, lb_b = 0.f, la_mean = 0.f;      // lane-channel constants (transposed layout)
    auto graph_change = [&](int g) {
        fetch_rec2<true>(recA, A.a, g, lane);
        if constexpr (CB > 0) fetch_rec2<true>(recB, A.b, g, lane);
        if (lane < 32) reinterpret_cast<float4 *>(recK)[lane] = reinterpret_cast<const float4 *>(opaque_ptr(A.coef))[(long long)g * FGNN_H + lane];
        cached_g = g;
        cur_nv = __builtin_amdgcn_readfirstlane(nvalid_of(A.nvalid, g, A.N));
        const float2 ra = reinterpret_cast<const float2 *>(recA)[j];
        la_a = ra.x;
        la_b = ra.y;
        if constexpr (CB > 0) {
            const float2 rb = reinterpret_cast<const float2 *>(recB)[j];
            lb_a = rb.x;
            lb_b = rb.y;
        }
        if (normA) la_mean = opaque_ptr(A.a.nrm)[((long long)g * A.a.C + j) * 4];
    };
    int first = T0 + wv;
    if constexpr (SKIP) first = __builtin_amdgcn_readfirstlane(next_live_tile_p(first, T1, NWB, tpg, 64, A.ldr, A.nvalid));
    {
        const int t = first;
        const Tile16 c = decode16(t, t < T1, tpg, A.ldr, PP, j);
        load_slab16<CA>(xa, va, c, h);
        if constexpr (CB > 0) load_slab16<CB>(xb, vb, c, h);
        if (t < T1) graph_change(c.g);
    }
    __syncthreads();

    // row offsets of the 16 channel rows a lane touches (all 32-channel tensors of a launch share one channel stride)
    const int ld2 = va.ld2;
    auto roff = [&](int r) { return ((r & 3) + 8 * (r >> 2)) * ld2; };

    int tnext = 0;
    for (int tile = first; tile < T1; tile = tnext) {
        tnext = tile + NWB;
        if constexpr (SKIP) tnext = __builtin_amdgcn_readfirstlane(next_live_tile_p(tnext, T1, NWB, tpg, 64, A.ldr, A.nvalid));
        const Tile16 c = decode16(tile, true, tpg, A.ldr, PP, j);
        if (c.g != cached_g) graph_change(c.g);
        const bool v0 = c.inb && c.i < cur_nv && c.jj < cur_nv;
        const bool v1 = c.inb && c.i < cur_nv && c.jj + 1 < cur_nv;
        const int lo4 = c.inb ? 4 * h * ld2 + 4 * c.pp : OOB_OFF;      // lane part of every 32-channel access

        // ---- all loads of the tile are requested up front ----
        FGNN_BWD16_LOAD_DY_Z
        unsigned olda[CA >= 32 ? 16 : 1], oldb[CB >= 32 ? 16 : 1];
        const bool rmw_a = (CA >= 32) && A.dxa != nullptr && A.accumulate_a;
        const bool rmw_b = (CB >= 32) && A.dxb != nullptr && A.accumulate_b;
        LOAD_OLD_DX(a, A)
        LOAD_OLD_DX(b, B)
        F16 keepA, keepB;           // rounded dx of the even pixels, waiting for the odd ones
        float es1 = 0.f, es2 = 0.f; // S1 / S2 of the tile (emit)

        // One pixel group (GRP 0 = even, 1 = odd pixels of the pairs) end to end.  The two groups are separated by a
        // scheduling barrier: interleaving them doubles the live fragments and spills.
        auto group = [&](auto tag) {
            constexpr int GRP = decltype(tag)::value;
            const float fv = GRP ? (v1 ? 1.f : 0.f) : (v0 ? 1.f : 0.f);
            // ---- input operands: normal (recompute) and transposed (layer-0 weight gradient) ----
            F16 ya, yb, raw_a, raw_b, yTa, yTb;
            FGNN_BWD16_INPUT(a, A)
            FGNN_BWD16_INPUT(b, B)

            F16 hs[DEPTH - 1];
            recompute_hidden<CA, CB, DEPTH>(hs, ya, yb, wl, tail, lane, h);

            F16 d;       // dz, zero in the padding
            dz_of<GRP>(d, dyr, zr, recK, fv, h);

            FGNN_BWD16_HIDDEN_LAYERS
            FGNN_BWD16_LAYER0

            // ---- dx of slab a ----
            if constexpr (CA >= 32) {
                if (A.dxa) {
                    F16 v;
                    DX_VALUE(v, a)
                    if constexpr (CB == 0) {
                        if (emit) FGNN_BWD16_EMIT_NORMALISED(v)
                    }
                    if constexpr (CB > 0) {
                        if (emit) {          // un-normalised slab: yTa is the transposed raw input itself
                            const f32x16 tv = transpose16(v, ident);
#pragma unroll
                            for (int q = 0; q < 8; ++q) {
                                es1 += tv[2 * q] + tv[2 * q + 1];
                                es2 = fmaf(tv[2 * q], bf_lo(yTa.d[q]), es2);
                                es2 = fmaf(tv[2 * q + 1], bf_hi(yTa.d[q]), es2);
                            }
                        }
                    }
                    FGNN_BWD16_KEEP_OR_STORE(v, a, A)
                }
            }
            // ---- dx of slab b ----
            if constexpr (CB >= 32) {
                if (A.dxb) {
                    F16 v;
                    DX_VALUE(v, b)
                    FGNN_BWD16_KEEP_OR_STORE(v, b, B)
                }
            }
        };
        group(std::integral_constant<int, 0>{});
        __builtin_amdgcn_sched_barrier(0);
        group(std::integral_constant<int, 1>{});
        __builtin_amdgcn_sched_barrier(0);
        if (emit) {
            es1 += __shfl_xor(es1, 32);
            es2 += __shfl_xor(es2, 32);
            if constexpr (CB == 0) {
                if (h == 0) reinterpret_cast<float2 *>(A.s12part)[((long long)c.g * FGNN_H + j) * tpg + c.tt] = make_float2(es1, es2);
            } else {
                // the trace term only, (G, 32, tpg): its one reader (the matmul workgroup of (g, c)) walks the tiles of one channel
                if (h == 0) A.s12part[((long long)c.g * FGNN_H + j) * tpg + c.tt] = es2;
            }
        }
        // the wave's next tile
        {
            const int tn = tnext;
            const Tile16 cn = decode16(tn, tn < T1, tpg, A.ldr, PP, j);
            load_slab16<CA>(xa, va, cn, h);
            if constexpr (CB > 0) load_slab16<CB>(xb, vb, cn, h);
        }
    }

    if constexpr (SKIP) {       // padding-only tiles of this wave's share: empty S1/S2 / trace-term records
        if (emit) {
            for (int t = T0 + wv; t < T1; t += NWB) {
                const int g = __builtin_amdgcn_readfirstlane(t / tpg), tt = t - g * tpg;
                if (tile_live_p(tt, 64, A.ldr, A.nvalid[g])) continue;
                if (h == 0) {
                    if constexpr (CB == 0) reinterpret_cast<float2 *>(A.s12part)[((long long)g * FGNN_H + j) * tpg + tt] = make_float2(0.f, 0.f);
                    else A.s12part[((long long)g * FGNN_H + j) * tpg + tt] = 0.f;
                }
            }
        }
    }

    // ---- workgroup reduction of the parameter gradients (fixed order over the waves) ----
    FGNN_BWD16_SCATTER_PARTIALS
    float4 *out = reinterpret_cast<float4 *>(A.wpart + (long long)blockIdx.x * PCOUNT);
    const float4 *part4 = reinterpret_cast<const float4 *>(smem);
    for (int e = threadIdx.x; e < PCOUNT / 4; e += 64 * NWB) {
        float4 a = part4[e];
#pragma unroll
        for (int w = 1; w < NWB; ++w) {                                  // fixed order
            const float4 b = part4[w * (PCOUNT / 4) + e];
            a.x += b.x;
            a.y += b.y;
            a.z += b.z;
            a.w += b.w;
        }
        out[e] = a;
    }
}
#undef LOAD_OLD_DX
#undef DX_VALUE

template <int CA, int CB, int DEPTH>
int launch_bwd16(const fgnn_mlp_bwd16_args *a, int tpg, int total, void *stream) {
    static_assert(BWD16_WG == FGNN_RANGE_WG, "fgnn_ragged_tile_ranges16 splits for the backward grid");
    constexpr int LDS = Bwd16Layout<CA, CB, DEPTH>::LDS_F * 4;
    if (a->ranges) return launch_bwd16_grid<mlp_bwd16_kernel<CA, CB, DEPTH, true>, LDS>(*a, tpg, total, stream);
    return launch_bwd16_grid<mlp_bwd16_kernel<CA, CB, DEPTH, false>, LDS>(*a, tpg, total, stream);
}

}  // namespace

extern "C" int fgnn_mlp_bwd16(const fgnn_mlp_bwd16_args *a, void *stream) {
    FGNN_CHECK(a != nullptr, "fgnn_mlp_bwd16: null args");
    FGNN_CHECK(shape_ok16(a), "fgnn_mlp_bwd16: bad G=%d N=%d ldr=%d", a->G, a->N, a->ldr);
    FGNN_CHECK(a->depth == 3, "fgnn_mlp_bwd16: built for depth_of_mlp = 3 (got %d)", a->depth);
    FGNN_CHECK(a->a.ptr && a->a.C > 0 && a->packed, "fgnn_mlp_bwd16: slab a / operand image missing");
    FGNN_CHECK(a->b.C == 0 || a->b.ptr, "fgnn_mlp_bwd16: slab b has channels but no pointer");
    if (check_mlp_args(a, "fgnn_mlp_bwd16", true)) return 1;
    FGNN_CHECK(!a->s12part || (a->a.C == 32 && a->dxa && ((a->b.C == 0 && a->a.nrm) || (a->b.C > 0 && !a->a.nrm))),
               "fgnn_mlp_bwd16: s12part needs dxa and either a single normalised 32-channel slab or a raw first slab of a two-slab MLP");
    int tpg, total;
    if (count_tiles16(a, "fgnn_mlp_bwd16", tpg, total)) return 1;
    const int ca = a->a.C, cb = a->b.C;
    if (ca == 2 && cb == 0) return launch_bwd16<2, 0, 3>(a, tpg, total, stream);
    if (ca == 32 && cb == 0) return launch_bwd16<32, 0, 3>(a, tpg, total, stream);
    if (ca == 32 && cb == 2) return launch_bwd16<32, 2, 3>(a, tpg, total, stream);
    if (ca == 32 && cb == 32) return launch_bwd16<32, 32, 3>(a, tpg, total, stream);
    fgnn_set_error("fgnn_mlp_bwd16: unsupported input channels (%d + %d); built for 2, 32, 32+2, 32+32", ca, cb);
    return 1;
}
