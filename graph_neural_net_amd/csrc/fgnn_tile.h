// Tile geometry, slab loads and operand reads shared by the 32-pixel MLP kernels (mlp_fwd.hip, the backward kernels and the x3
// kernels):
// a tile = 32 consecutive pixels of one graph; lane (j, h) = pixel j of the tile, half-wave h; a 32-channel slab gives
// the lane its 16 channels ch_of(r, h), a 2-channel slab gives half-wave h channel h.
#pragma once
#include "fgnn_common.h"

namespace {

constexpr int TLD = 36;              // LDS tile row stride (floats): 144 B rows, 16-B aligned
constexpr int TILE_F = 32 * TLD;     // floats per 32-row tile

struct TileCtx {
    int g, tt, p, i, jj;
    bool inb;
};

// The valid-vertex count of the graph is NOT read here: a global load at the top of every tile makes
// the compiler drain the whole memory pipeline (s_waitcnt vmcnt(0): next-tile prefetch AND the previous
// tile's stores).  It is fetched once per graph change, next to the per-graph records.
DEVI TileCtx decode_tile(int tile, bool active, int tpg, int N, int P, int j) {
    TileCtx c;
    c.g = __builtin_amdgcn_readfirstlane(active ? tile / tpg : 0);
    c.tt = active ? tile - c.g * tpg : 0;
    c.p = c.tt * FGNN_TILE + j;
    c.inb = active && c.p < P;
    c.i = c.p / N;
    c.jj = c.p - c.i * N;
    return c;
}
DEVI bool tile_valid(const TileCtx &c, int nv) { return c.inb && c.i < nv && c.jj < nv; }

// channel contracted by k-step k in half-wave h; its h-independent part and the row multiplier of the h part
template <int S>
DEVI constexpr int slab_ch(int k, int h) { return S == 16 ? ch_of(k, h) : 2 * k + h; }
template <int S>
DEVI constexpr int slab_kbase(int k) { return S == 16 ? (k & 3) + 8 * (k >> 2) : 2 * k; }
template <int S>
DEVI constexpr int slab_hmul() { return S == 16 ? 4 : 1; }

// per-lane byte offset of pixel c.p in the half-wave's first row (OOB_OFF when out of range)
template <int HMUL>
DEVI int lane_off(const View &v, const TileCtx &c, int h) {
    return c.inb ? HMUL * h * v.ld4 + 4 * c.p : OOB_OFF;
}

template <int S>
DEVI void load_raw(float (&x)[S > 0 ? S : 1], const View &v, const TileCtx &c, int h) {
    if constexpr (S > 0) {
        const int voff = lane_off<slab_hmul<S>()>(v, c, h);
        const int s0 = c.g * v.gs4;
#pragma unroll
        for (int k = 0; k < S; ++k) x[k] = buf_load(v, voff, s0 + slab_kbase<S>(k) * v.ld4);
    }
}

// slab load: from memory, or (PK, 2-channel slabs only) from the packed adjacency
template <int S, bool PK>
DEVI void load_slab(float (&x)[S > 0 ? S : 1], const View &v, const PackedSrc &ps, const TileCtx &c, int h) {
    if constexpr (PK && S == 1) load_packed(x, ps, c, h);
    else load_raw<S>(x, v, c, h);
}

// rows ch_of(r,h) of a (G,32,ld) tensor
DEVI void load_rows16(float (&x)[16], const View &v, const TileCtx &c, int h) {
    const int voff = lane_off<4>(v, c, h);
    const int s0 = c.g * v.gs4;
#pragma unroll
    for (int r = 0; r < 16; ++r) x[r] = buf_load(v, voff, s0 + ((r & 3) + 8 * (r >> 2)) * v.ld4);
}

// y = (x - mean) * a + beta with the per-graph records {mean, a, beta, -} read from wave-private LDS; 0 on invalid pixels
// (a 0/1 mask multiply: `valid ? .. : 0` becomes divergent control flow around the LDS reads, with a full-array phi copy per element)
template <int S>
DEVI void norm_slab(float (&y)[S > 0 ? S : 1], const float (&x)[S > 0 ? S : 1], const float *rec, bool on, bool valid, int h) {
    if constexpr (S > 0) {
        const float4 *r4 = reinterpret_cast<const float4 *>(rec);
        if (on) {                       // wave-uniform
            const float vf = valid ? 1.f : 0.f;
#pragma unroll
            for (int k = 0; k < S; ++k) {
                const float4 n = r4[slab_ch<S>(k, h)];
                y[k] = ((x[k] - n.x) * n.y + n.z) * vf;
            }
        } else {
#pragma unroll
            for (int k = 0; k < S; ++k) y[k] = x[k];
        }
    }
}

// ---- operand reads of the fp32 32-pixel backward kernels (mlp_bwd.hip, mlp_bwd_pair.hip) -------------------------------------

// dW += Dt (rows = out channel) x In (rows = in channel), contraction over the 32 pixels.
// The Dt fragments of lane (o, h) are 16 pixels of channel o, so the bias gradient
// db[o] = sum_px Dt[o][px] falls out of the same LDS reads (WITH_DB).
template <bool WITH_DB>
DEVI f32x16 wgrad_tile(const float *Dt, const float *In, f32x16 acc, float &db, int lane) {
    const int i = lane & 31, h = lane >> 5;
    const float4 *dp = reinterpret_cast<const float4 *>(Dt + i * TLD + 4 * h);
    const float4 *ip = reinterpret_cast<const float4 *>(In + i * TLD + 4 * h);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 a = dp[2 * q];
        const float4 b = ip[2 * q];
        if (WITH_DB) db += (a.x + a.y) + (a.z + a.w);
        acc = mfma32(a.x, b.x, acc);
        acc = mfma32(a.y, b.y, acc);
        acc = mfma32(a.z, b.z, acc);
        acc = mfma32(a.w, b.w, acc);
    }
    return acc;
}

DEVI void zero16(f32x16 &a) {
#pragma unroll
    for (int r = 0; r < 16; ++r) a[r] = 0.f;
}

// CNT k-steps of an operand set from the workgroup-shared LDS image (one float per lane per k-step, stored as
// [step/4][lane][4] so a ds_read_b128 returns four consecutive k-steps of a lane)
template <int OFF, int CNT>
DEVI void load_ops(float (&dst)[CNT > 0 ? CNT : 1], const float *wl, int lane) {
    static_assert(OFF % 4 == 0, "operand sets are float4 aligned");
    const float4 *p = reinterpret_cast<const float4 *>(wl) + (OFF / 4) * 64 + lane;
#pragma unroll
    for (int q = 0; q < (CNT + 3) / 4; ++q) {
        const float4 v = p[q * 64];
        if (4 * q + 0 < CNT) dst[4 * q + 0] = v.x;
        if (4 * q + 1 < CNT) dst[4 * q + 1] = v.y;
        if (4 * q + 2 < CNT) dst[4 * q + 2] = v.z;
        if (4 * q + 3 < CNT) dst[4 * q + 3] = v.w;
    }
}

// bias[ch_of(r, h)], r = 0..15, of one layer from the compact tail (broadcast reads)
DEVI void load_bias(float (&dst)[16], const float *tail, int layer, int h) {
    const float4 *p = reinterpret_cast<const float4 *>(tail + layer * 32 + h * 16);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 v = p[q];
        dst[4 * q + 0] = v.x;
        dst[4 * q + 1] = v.y;
        dst[4 * q + 2] = v.z;
        dst[4 * q + 3] = v.w;
    }
}

}  // namespace
