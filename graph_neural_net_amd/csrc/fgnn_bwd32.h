// What the six fp32 MLP backward files share (mlp_bwd.hip, mlp_bwd_pair.hip, mlp_bwd_x3.hip, mlp_bwd_pair_x3.hip, mlp_bwd_t16.hip,
// mlp_bwd_pair_t16.hip): the launch geometry, the dz coefficient records, the
// fixed-order sum of the waves' partials and the entry points' argument checks.  Tile geometry is NOT here: the 32-pixel kernels
// take theirs from fgnn_tile.h, the 16-pixel ones from fgnn_t16.h.
#pragma once
#include "fgnn_common.h"

namespace {

constexpr int BWD_WG = 256;          // persistent workgroups (one per CU) = rows of each wpart
constexpr int NW = 8;                // waves per workgroup (2 per SIMD); the pair kernels run them as NP pairs
constexpr int NP = 4;
static_assert(BWD_WG == FGNN_RANGE_WG, "fgnn_ragged_tile_ranges splits for the backward grid");

// dz coefficients {mean, ca, cb, cc} of channel `ch` of graph g: precomputed (A.coef) or derived here
// from the GraphNorm-backward sums S1,S2 and the output's GraphNorm record:
//   dz = a*dy - a*S2*r2/m * (z - mean) - a*S1/m
DEVI float4 coef_from_sums(const float4 n, const float2 sv, float nv) {
    const float m = nv * nv;
    float4 k;
    k.x = n.x;
    k.y = n.y;
    k.z = m > 0.f ? -n.y * sv.y * n.w / m : 0.f;
    k.w = m > 0.f ? -n.y * sv.x / m : 0.f;
    return k;
}
// (the 16-pixel kernels hold the graph's vertex count already -- graph_nv -- and pass it in)
DEVI float4 coef_record(const fgnn_mlp_bwd_args &A, int g, int ch, int nv) {
    if (A.coef) return reinterpret_cast<const float4 *>(A.coef)[(long long)g * FGNN_H + ch];
    const float4 n = reinterpret_cast<const float4 *>(A.znrm)[(long long)g * FGNN_H + ch];
    const float2 sv = reinterpret_cast<const float2 *>(A.s12)[(long long)g * FGNN_H + ch];
    return coef_from_sums(n, sv, (float)nv);
}
// (written out, not forwarded to the overload above: forwarding reads nvalid[g] before the A.coef branch, not inside it, which costs
// every 32-pixel kernel two more s_waitcnt)
DEVI float4 coef_record(const fgnn_mlp_bwd_args &A, int g, int ch) {
    if (A.coef) return reinterpret_cast<const float4 *>(A.coef)[(long long)g * FGNN_H + ch];
    const float4 n = reinterpret_cast<const float4 *>(A.znrm)[(long long)g * FGNN_H + ch];
    const float2 sv = reinterpret_cast<const float2 *>(A.s12)[(long long)g * FGNN_H + ch];
    return coef_from_sums(n, sv, (float)nvalid_of(A.nvalid, g, A.N));
}

// (a workgroup's tile range, wg_tile_range<SKIP>, is in fgnn_common.h: the forward kernels use it too)

// the two argument blocks of a fused mlp1 + mlp2 launch
struct PairArgs {
    fgnn_mlp_bwd_args m[2];
};

// ---- workgroup reduction of the parameter gradients ------------------------------------------------------------------------
// Every wave has put its partial (PCOUNT floats) at smem + wave * PCOUNT; one row per workgroup goes to wpart, to be reduced in
// fixed order by fgnn_grad_finalize.  The waves are summed in a fixed order too: results are bit-reproducible run to run.
template <int PCOUNT, int NWV>
DEVI void sum_wave_partials(const float *smem, float *wpart) {
    static_assert(PCOUNT % 4 == 0, "partials are summed four at a time");
    float4 *out = reinterpret_cast<float4 *>(wpart + (long long)blockIdx.x * PCOUNT);
    const float4 *part4 = reinterpret_cast<const float4 *>(smem);
    for (int e = threadIdx.x; e < PCOUNT / 4; e += 64 * NWV) {
        float4 a = part4[e];
#pragma unroll
        for (int w = 1; w < NWV; ++w) {                                 // fixed order
            const float4 b = part4[w * (PCOUNT / 4) + e];
            a.x += b.x;
            a.y += b.y;
            a.z += b.z;
            a.w += b.w;
        }
        out[e] = a;
    }
}
// pair kernels: waves 0..NP-1 hold mlp1's partials, waves NP..NW-1 mlp2's; each MLP's row = the sum of its four waves
template <int PCOUNT>
DEVI void sum_pair_partials(const float *smem, const PairArgs &P) {
    static_assert(PCOUNT % 4 == 0, "partials are summed four at a time");
    const float4 *part4 = reinterpret_cast<const float4 *>(smem);
    for (int e = threadIdx.x; e < 2 * (PCOUNT / 4); e += 64 * NW) {
        const int m = e >= PCOUNT / 4 ? 1 : 0, ee = e - m * (PCOUNT / 4);
        float4 a = part4[(4 * m) * (PCOUNT / 4) + ee];
#pragma unroll
        for (int w = 1; w < NP; ++w) {                                  // fixed order over the MLP's four waves
            const float4 b = part4[(4 * m + w) * (PCOUNT / 4) + ee];
            a.x += b.x;
            a.y += b.y;
            a.z += b.z;
            a.w += b.w;
        }
        reinterpret_cast<float4 *>(P.m[m].wpart + (long long)blockIdx.x * PCOUNT)[ee] = a;
    }
}

// ---- what every entry point checks (`fn` = its name; `tile_bits`: the tile count must stay below 2^tile_bits) ---------------
// one MLP: fgnn_mlp_bwd, fgnn_mlp_bwd_x3, fgnn_mlp_bwd_t16
inline int check_mlp_bwd_common(const fgnn_mlp_bwd_args *a, const char *fn, int tile_bits) {
    FGNN_CHECK(a->dy && a->z && a->wpart, "%s: missing dy/z/wpart", fn);
    FGNN_CHECK(a->coef || (a->s12 && a->znrm) || (a->s12tiles && a->znrm), "%s: need coef, or s12 + znrm, or s12tiles + znrm", fn);
    const long long lim = 0x7fffffffll / 4, G = a->G;
    FGNN_CHECK(G * a->a.gstride < lim && G * a->b.gstride < lim && G * a->dgstride < lim && G * a->zgstride < lim &&
               G * a->dxa_gstride < lim && G * a->dxb_gstride < lim,
               "%s: a tensor exceeds 2 GiB (32-bit buffer addressing); split the batch", fn);
    FGNN_CHECK(G * fgnn_tiles_per_graph(a->N) < (1ll << tile_bits), "%s: too many tiles", fn);
    // (trivially true in fgnn_mlp_bwd itself, whose file defines that function)
    FGNN_CHECK(BWD_WG == fgnn_mlp_bwd_num_workgroups(), "%s: workgroup count differs from fgnn_mlp_bwd", fn);
    return 0;
}
// a pair: fgnn_mlp_bwd_pair, fgnn_mlp_bwd_pair_x3, fgnn_mlp_bwd_pair_t16 (`dense_only`: no bit-packed input, slab a must exist)
inline int check_pair_common(const fgnn_mlp_bwd_args *a1, const fgnn_mlp_bwd_args *a2, const char *fn, int tile_bits, bool dense_only) {
    FGNN_CHECK(a1 && a2, "%s: null args", fn);
    FGNN_CHECK(BWD_WG == fgnn_mlp_bwd_num_workgroups(), "%s: workgroup count differs from fgnn_mlp_bwd", fn);
    FGNN_CHECK(a1->G > 0 && a1->N > 0 && a1->G == a2->G && a1->N == a2->N && a1->depth == a2->depth,
               "%s: the two MLPs must share G, N and depth", fn);
    FGNN_CHECK((!dense_only || a1->a.ptr) && a1->a.ptr == a2->a.ptr && a1->a.C == a2->a.C && a1->a.gstride == a2->a.gstride &&
               a1->a.ldp == a2->a.ldp && a1->a.nrm == a2->a.nrm && a1->a.beta == a2->a.beta &&
               (dense_only || (a1->xbits == a2->xbits && a1->xdeg == a2->xdeg)) && a1->nvalid == a2->nvalid,
               "%s: the two MLPs must read the same input slab", fn);
    FGNN_CHECK(!a1->dxa && !a1->s12part, "%s: the input gradient and its tile sums belong to the SECOND argument block", fn);
    FGNN_CHECK(!a1->s12tiles && !a2->s12tiles, "%s: s12tiles is an mlp3 feature", fn);
    for (const fgnn_mlp_bwd_args *a : {a1, a2}) {
        FGNN_CHECK(a->dy && a->z && a->wpart, "%s: missing dy/z/wpart", fn);
        FGNN_CHECK(a->coef || (a->s12 && a->znrm), "%s: need coef, or s12 + znrm", fn);
        const long long lim = 0x7fffffffll / 4, G = a->G;
        FGNN_CHECK(G * a->a.gstride < lim && G * a->dgstride < lim && G * a->zgstride < lim && G * a->dxa_gstride < lim,
                   "%s: a tensor exceeds 2 GiB (32-bit buffer addressing); split the batch", fn);
    }
    FGNN_CHECK((long long)a1->G * fgnn_tiles_per_graph(a1->N) < (1ll << tile_bits), "%s: too many tiles", fn);
    return 0;
}

}  // namespace
