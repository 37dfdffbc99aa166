// What the two fp32 MLP forward files share (mlp_fwd.hip, mlp_fwd_x3.hip), i.e. what surrounds the conv chain: the views and the
// LDS pieces of a wave, the per-graph record fetch, the statistics epilogue, the test-only export of the ReLU decisions, the entry
// points' common argument checks and the launch.  Tile geometry and slab loads come from fgnn_tile.h, the workgroup's tile range
// (wg_tile_range) from fgnn_common.h.
#pragma once
#include "fgnn_tile.h"

namespace {

// The pieces of the tile loop are macros pasted into both bodies where the same text as a function -- arguments by value or by
// reference, whole or in halves -- changed the kernels' instructions; they use the bodies' own names: A, PK, NMLP,
// c, c_valid, vmask, inv, tl, tpg, lane, j, h.

// the buffer views of a launch: the two input slabs (or the bit-packed adjacency in place of a 2-channel one) and the outputs
#define FGNN_FWD32_VIEWS                                                                       \
    const View va = make_view(A.a.ptr, A.a.gstride, A.a.ldp, A.G);                             \
    const View vb = make_view(A.b.ptr, A.b.gstride, A.b.ldp, A.G);                             \
    PackedSrc ps = {};                                                                         \
    if constexpr (PK) ps = make_packed_src(A.xbits, A.xdeg, A.G, A.N);                         \
    View vz[NMLP];                                                                             \
    _Pragma("unroll") for (int m = 0; m < NMLP; ++m) vz[m] = make_view(A.z[m], FGNN_H * A.ldz, A.ldz, A.G);

// LDS of a workgroup (layout L): WEIGHT_F floats of operand images, then a transpose tile per wave, then per wave the records of
// slab a (128 floats) and slab b
template <class L>
DEVI float *fwd_lds_tile(float *smem, int wv) { return smem + L::WEIGHT_F + wv * TILE_F; }
template <class L>
DEVI float *fwd_lds_records(float *smem, int wv) { return smem + L::WEIGHT_F + L::NW * TILE_F + wv * L::REC_F; }

// n = GraphNorm record {mean, a, beta, -} of channel `lane` of graph g of an input slab (nrm: (G, C) records {mean, a, -, -})
DEVI void fetch_record(float4 &n, const float *nrm, const float *beta, int C, int g, int lane) {
    n = reinterpret_cast<const float4 *>(nrm)[(long long)g * C + lane];
    n.z = beta ? beta[lane] : 0.f;
}

// Epilogue of one MLP's tile: mask, store z (view vz), transpose through the wave's LDS tile tl, per-tile {mean, M2} with
// lane = channel -> part
#define FGNN_FWD32_STATS(acc, vz, part)                                                        \
    {                                                                                          \
        const int zoff = lane_off<4>(vz, c, h);                                                \
        const int zs0 = c.g * vz.gs4;                                                          \
        _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                       \
            const int chl = (r & 3) + 8 * (r >> 2); /* channel minus 4*h */                    \
            const float v = c_valid ? acc[r] : 0.f;                                            \
            buf_store(v, vz, zoff, zs0 + chl * vz.ld4);                                        \
            tl[(chl + 4 * h) * TLD + j] = v;                                                   \
        }                                                                                      \
        /* lane (ch = j, h) owns pixels 16h .. 16h+15 of channel ch */                         \
        const float4 *rp = reinterpret_cast<const float4 *>(tl + j * TLD + 16 * h);            \
        float4 qv[4];                                                                          \
        _Pragma("unroll") for (int k = 0; k < 4; ++k) qv[k] = rp[k];                           \
        float s = 0.f;                                                                         \
        _Pragma("unroll") for (int k = 0; k < 4; ++k) s += (qv[k].x + qv[k].y) + (qv[k].z + qv[k].w); \
        s += __shfl_xor(s, 32);                                                                \
        const float mean = s * inv;                                                            \
        const unsigned mh = vmask >> (16 * h);                                                 \
        float m2 = 0.f;                                                                        \
        _Pragma("unroll") for (int k = 0; k < 4; ++k) {                                        \
            const float d0 = ((mh >> (4 * k + 0)) & 1u) ? qv[k].x - mean : 0.f;                \
            const float d1 = ((mh >> (4 * k + 1)) & 1u) ? qv[k].y - mean : 0.f;                \
            const float d2 = ((mh >> (4 * k + 2)) & 1u) ? qv[k].z - mean : 0.f;                \
            const float d3 = ((mh >> (4 * k + 3)) & 1u) ? qv[k].w - mean : 0.f;                \
            m2 += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);                                   \
        }                                                                                      \
        m2 += __shfl_xor(m2, 32);                                                              \
        if (h == 0) {                                                                          \
            float2 o;                                                                          \
            o.x = mean;                                                                        \
            o.y = m2;                                                                          \
            reinterpret_cast<float2 *>(part)[((long long)c.g * tpg + c.tt) * FGNN_H + j] = o;  \
        }                                                                                      \
    }

// Test-only (the DBG twins): the decisions relu1 takes on hidden layer `hid` (of nhid) -- bit pattern > 0 as a signed integer -- one
// bit per pixel: dbg[((g * nhid + hid) * 32 + channel) * tpg + tile], bit j = pixel 32 * tile + j
#define FGNN_FWD32_EXPORT_RELU(acc, dbg, nhid, hid)                                            \
    _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                           \
        const unsigned long long mk = __ballot(__float_as_int(acc[r]) > 0);                    \
        if (lane == 0) {                                                                       \
            unsigned *o = (dbg) + (((long long)c.g * (nhid) + (hid)) * 32 + ch_of(r, 0)) * tpg + c.tt; \
            o[0] = (unsigned)mk;                                                               \
            o[4ll * tpg] = (unsigned)(mk >> 32); /* channel ch_of(r, 1) = ch_of(r, 0) + 4 */   \
        }                                                                                      \
    }

// ---- host side ----------------------------------------------------------------------------------------------------------------
// what both entry points check (`fn` = the entry's name), ahead of the checks only one of them has
inline int check_mlp_fwd_common(const fgnn_mlp_fwd_args *a, const char *fn) {
    FGNN_CHECK(a != nullptr, "%s: null args", fn);
    FGNN_CHECK(a->G > 0 && a->N > 0, "%s: bad G=%d N=%d", fn, a->G, a->N);
    FGNN_CHECK(a->nmlp == 1 || a->nmlp == 2, "%s: nmlp must be 1 or 2 (got %d)", fn, a->nmlp);
    FGNN_CHECK(!a->xbits || a->xdeg, "%s: xbits without xdeg (fgnn_adjacency_degree)", fn);
    const bool pk_a = a->xbits && a->a.C == 2;          // that slab's memory is never touched
    FGNN_CHECK((long long)a->N * a->N <= a->ldz && (pk_a || (long long)a->N * a->N <= a->a.ldp), "%s: channel stride < N*N", fn);
    for (int m = 0; m < a->nmlp; ++m) FGNN_CHECK(a->z[m] && a->part[m], "%s: missing output %d", fn, m);
    FGNN_CHECK(a->cnt, "%s: missing cnt", fn);
    const long long lim = 0x7fffffffll / 4, G = a->G;
    FGNN_CHECK(G * a->a.gstride < lim && G * a->b.gstride < lim && G * FGNN_H * a->ldz < lim,
               "%s: a tensor exceeds 2 GiB (32-bit buffer addressing); split the batch", fn);
    FGNN_CHECK(G * fgnn_tiles_per_graph(a->N) < (1ll << 30), "%s: too many tiles", fn);
    return 0;
}

// The launch of a forward kernel or of its decision-exporting twin.  KP names the pair: KP::product() and KP::dbg() return the two
// kernels (only the one launched is instantiated).  One workgroup per NW tiles, at most one per CU (cu_share 2: per CU of one half
// of the device, two launches on two streams side by side); `ragged_grid` (> 0) fixes the grid of a launch with tile ranges.
template <class KP, bool DBG, int NW, int LDS>
int launch_fwd32(const fgnn_mlp_fwd_args *a, int tpg, int total, int ragged_grid, hipStream_t st, unsigned *d0, unsigned *d1) {
    static_assert(LDS <= 160 * 1024, "LDS budget");
    static LdsAttrCache attr_cache;
    int grid = (total + NW - 1) / NW;
    const int cap = a->cu_share == 2 ? 128 : 256;
    if (grid > cap) grid = cap;
    if (ragged_grid > 0) grid = ragged_grid;
    if constexpr (DBG) {
        (void)fgnn_raise_lds(attr_cache, (const void *)KP::dbg(), LDS);
        hipLaunchKernelGGL(KP::dbg(), dim3(grid), dim3(64 * NW), LDS, st, *a, tpg, total, d0, d1);
    } else {
        (void)fgnn_raise_lds(attr_cache, (const void *)KP::product(), LDS);
        hipLaunchKernelGGL(KP::product(), dim3(grid), dim3(64 * NW), LDS, st, *a, tpg, total);
    }
    FGNN_LAUNCH_CHECK();
    return 0;
}

}  // namespace
