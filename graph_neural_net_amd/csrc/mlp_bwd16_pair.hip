// mlp1 + mlp2 of one FGNN block (models/blocks_emb.py:16-27: two MlpBlock_Real on the SAME input), bf16 backward in ONE
// launch -- the bf16 twin of mlp_bwd_pair.hip.  Per MLP and per tile the algorithm, rounding points and fragment conventions
// are those of fgnn_bwd16.h, which holds what this kernel shares with mlp_bwd16.hip; what changes is who does it and what
// travels through HBM:
//   * the two waves that share a SIMD form a PAIR on the same tile: wave p (p = 0..3) runs mlp1, wave p + 4 runs mlp2, each with
//     only its own weight-gradient accumulators (registers + the same parked LDS tiles as the single-MLP kernel);
//   * the gradient of the shared input is summed in the pair: the mlp1 wave leaves its fp32 dx fragments (even / odd pixel
//     group) in a double-buffered LDS slot, the mlp2 wave forms R(R(d_in3 + dx1) + dx2) -- the two roundings of the two
//     read-modify-write launches it replaces, so the stored d_in is bit-identical to theirs -- and stores once.  Two LDS words
//     per pair (release / acquire at workgroup scope) order the hand-over; with two buffers neither wave waits in steady state.
//   Per block: x is read once, d_in is read and written once (7 slab passes instead of 10: 287 MB instead of 422 MB at the
//   cfg4 size), one prologue / tail instead of two.
// Depth 3, one input slab of 32 channels (blocks > 1) or 2 channels (block 1: no input gradient, the pair only shares the
// launch), constant-size batches.
#include "fgnn_bwd16.h"

using namespace bwd16;

namespace {

// the single kernel's layout with two operand images, then the hand-over of the mlp1 wave's fp32 dx fragments: per pair
// 2 buffers x 2 pixel groups x [4][64 lanes][4 floats], and 4 flag words per pair
template <int CA>
struct Pair16Layout : Bwd16Layout<CA, 0, 3, 2> {
    using B = Bwd16Layout<CA, 0, 3, 2>;
    static constexpr int XCH_OFF = B::PARK_OFF + B::PARK_F;
    static constexpr int XCH_F = (CA >= 32) ? NP * 2 * 2 * 1024 : 0;
    static constexpr int FLAG_OFF = XCH_OFF + XCH_F;
    static constexpr int LDS_F = FLAG_OFF + 4 * NP > B::RED_F ? FLAG_OFF + 4 * NP : B::RED_F;
};

struct Pair16Args {
    fgnn_mlp_bwd16_args m[2];
};

template <int CA>
__global__ __launch_bounds__(64 * NWB, NWB / 4) void mlp_bwd16_pair_kernel(const Pair16Args P, const int tpg, const int total_tiles) {
    constexpr int CB = 0, DEPTH = 3;      // what the shared phases of fgnn_bwd16.h call the second slab's channels (none here: dW0b, yb
    constexpr bool SKIP = false;          // and yTb below are never touched) and the ragged tile ranges (constant-size batches only)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    using L = Pair16Layout<CA>;
    constexpr Pk16 PK = L::PK;
    constexpr int CIN = CA + CB;
    constexpr int XA = CA >= 32 ? 16 : 2;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int role = wv >> 2, pair = wv & 3;        // role 0: mlp1 (hands its dx over), role 1: mlp2 (sums, stores, emits)
    const fgnn_mlp_bwd16_args &A = P.m[role];
    const int j = lane & 31, h = lane >> 5;
    const int PP = A.N * A.ldr;
    const View16 va = make_view16(A.a.ptr, A.a.gstride, A.a.ldp, A.G);
    const View16 vdy = make_view16(A.dy, A.dgstride, A.ldd, A.G);
    const View16 vz = make_view16(A.z, A.zgstride, A.ldz, A.G);
    const View16 vdxa = make_view16(P.m[1].dxa, P.m[1].dxa_gstride, P.m[1].dxa_ld, P.m[1].G);

    float *wl = smem + role * L::WEIGHT_F;
    const float *tail = wl + PK.bias_f;
    float *rec = smem + 2 * L::WEIGHT_F + wv * L::REC_F;
    float *xch = smem + L::XCH_OFF + pair * (2 * 2 * 1024);
    int *flags = reinterpret_cast<int *>(smem + L::FLAG_OFF) + 4 * pair;     // [0] = last tile handed over, [1] = last tile consumed
    float *recA = rec, *recK = rec + 128;
    const F16 ident = make_identity(lane);

    FGNN_BWD16_ACCUMULATORS
    FGNN_BWD16_TILE_RANGE
    const bool normA = (CA >= 32) && A.a.nrm != nullptr;
    // per-tile sums of the input gradient {sum dx, sum dx (z_a - mean_a)}: the GraphNorm backward sums of the slab's producer
    const bool has_dx = (CA == 32) && P.m[1].dxa != nullptr;
    const bool emit = (CA == 32) && role == 1 && normA && has_dx && P.m[1].s12part != nullptr;

    {
        float4 *dst = reinterpret_cast<float4 *>(smem);
        for (int e = threadIdx.x; e < 2 * (L::WEIGHT_F / 4); e += 64 * NWB) {
            const int m = e >= L::WEIGHT_F / 4 ? 1 : 0;
            dst[e] = reinterpret_cast<const float4 *>(P.m[m].packed)[e - m * (L::WEIGHT_F / 4)];
        }
        if (threadIdx.x < 4 * NP) reinterpret_cast<int *>(smem + L::FLAG_OFF)[threadIdx.x] = -1;
    }
    unsigned xa[XA];
    int cached_g = -1, cur_nv = A.N;
    float la_a = 1.f, la_b = 0.f, la_mean = 0.f;      // lane-channel constants (transposed layout)
    auto graph_change = [&](int g) {
        fetch_rec2<false>(recA, A.a, g, lane);
        if (lane < 32) reinterpret_cast<float4 *>(recK)[lane] = reinterpret_cast<const float4 *>(A.coef)[(long long)g * FGNN_H + lane];
        cached_g = g;
        cur_nv = __builtin_amdgcn_readfirstlane(nvalid_of(A.nvalid, g, A.N));
        const float2 ra = reinterpret_cast<const float2 *>(recA)[j];
        la_a = ra.x;
        la_b = ra.y;
        if (normA) la_mean = A.a.nrm[((long long)g * A.a.C + j) * 4];
    };
    int first = T0 + pair;
    {
        const int t = first;
        const Tile16 c = decode16(t, t < T1, tpg, A.ldr, PP, j);
        load_slab16<CA>(xa, va, c, h);
        if (t < T1) graph_change(c.g);
    }
    __syncthreads();

    // row offsets of the 16 channel rows a lane touches (all 32-channel tensors of a launch share one channel stride)
    const int ld2 = va.ld2;
    auto roff = [&](int r) { return ((r & 3) + 8 * (r >> 2)) * ld2; };

    // static priority for the mlp2 waves (the younger half of the workgroup AND the longer half of the pair): see mlp_bwd_pair_t16.hip
    if (role == 1) __builtin_amdgcn_s_setprio(1);
    int tnext = 0;
    for (int tile = first; tile < T1; tile = tnext) {
        tnext = tile + NP;
        const Tile16 c = decode16(tile, true, tpg, A.ldr, PP, j);
        if (c.g != cached_g) graph_change(c.g);
        const bool v0 = c.inb && c.i < cur_nv && c.jj < cur_nv;
        const bool v1 = c.inb && c.i < cur_nv && c.jj + 1 < cur_nv;
        const int lo4 = c.inb ? 4 * h * ld2 + 4 * c.pp : OOB_OFF;      // lane part of every 32-channel access

        // ---- all loads of the tile are requested up front ----
        FGNN_BWD16_LOAD_DY_Z
        unsigned olda[CA >= 32 ? 16 : 1];
        const bool rmw_a = has_dx && role == 1 && P.m[1].accumulate_a;
        float *xbuf = xch + (((tile - first) / NP) & 1) * (2 * 1024);          // this tile's hand-over buffer
        if constexpr (CA >= 32) {
            if (has_dx) {     // (issued on every path -- out of range when nothing is accumulated: no traffic -- so that the compiler can count
                              // what is in flight behind the x prefetch below and its s_waitcnt for x does not drain these)
                const int vo = (rmw_a ? lo4 : OOB_OFF) + c.g * vdxa.gs2;
#pragma unroll
                for (int r = 0; r < 16; ++r) olda[r] = buf_load_u32(vdxa, vo, roff(r));
            }
        }
        const Tile16 cn = decode16(tnext, tnext < T1, tpg, A.ldr, PP, j);       // the wave's next tile
        F16 keepA;                  // rounded dx of the even pixels, waiting for the odd ones
        float es1 = 0.f, es2 = 0.f; // S1 / S2 of the tile (emit)

        // One pixel group (GRP 0 = even, 1 = odd pixels of the pairs) end to end.  The two groups are separated by a
        // scheduling barrier: interleaving them doubles the live fragments and spills.
        auto group = [&](auto tag) {
            constexpr int GRP = decltype(tag)::value;
            const float fv = GRP ? (v1 ? 1.f : 0.f) : (v0 ? 1.f : 0.f);
            // ---- input operands: normal (recompute) and transposed (layer-0 weight gradient) ----
            F16 ya, yb, raw_a, yTa, yTb;
            FGNN_BWD16_INPUT(a, A)

            F16 hs[DEPTH - 1];
            recompute_hidden<CA, CB, DEPTH>(hs, ya, yb, wl, tail, lane, h);
            F16 d;       // dz, zero in the padding
            dz_of<GRP>(d, dyr, zr, recK, fv, h);

            FGNN_BWD16_HIDDEN_LAYERS
            FGNN_BWD16_LAYER0

            // ---- dx of the shared input slab ----
            if constexpr (CA >= 32) {
                if (has_dx) {
                    f32x16 acc = input_grad(wl, PK.off_wt0a, d, lane);
                    if (role == 0) {
                        // hand the fp32 fragment over ([4][lane][4] like a parked tile).  The buffer was last used two tiles ago:
                        // wait until that tile has been consumed
                        if constexpr (GRP == 0) {
                            if (tile - first >= 2 * NP) {
                                while (__hip_atomic_load(&flags[1], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < tile - 2 * NP) __builtin_amdgcn_s_sleep(1);
                            }
                        }
                        park_put(xbuf + GRP * 1024, lane, acc);
                        if constexpr (GRP == 1) __hip_atomic_store(&flags[0], tile, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                    } else {
                        if constexpr (GRP == 0) {
                            while (__hip_atomic_load(&flags[0], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < tile) __builtin_amdgcn_s_sleep(1);
                        }
                        // R(d_in3 + dx1) first -- what the mlp1 launch used to store -- then this MLP's share on top of it
                        f32x16 t = park_get(xbuf + GRP * 1024, lane);
                        if constexpr (GRP == 1) __hip_atomic_store(&flags[1], tile, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                        if (rmw_a) {
#pragma unroll
                            for (int r = 0; r < 16; ++r) t[r] += half_of<GRP>(olda[r]);
                        }
                        F16 v1;
                        pack_acc(v1, t);
#pragma unroll
                        for (int q = 0; q < 8; ++q) {
                            acc[2 * q] += bf_lo(v1.d[q]);
                            acc[2 * q + 1] += bf_hi(v1.d[q]);
                        }
                        F16 v;
                        pack_acc(v, acc);
                        if (emit) FGNN_BWD16_EMIT_NORMALISED(v)
                        FGNN_BWD16_KEEP_OR_STORE(v, a, A)
                    }
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
            if (h == 0) reinterpret_cast<float2 *>(P.m[1].s12part)[((long long)c.g * FGNN_H + j) * tpg + c.tt] = make_float2(es1, es2);
        }
        load_slab16<CA>(xa, va, cn, h);     // the wave's next tile
    }

    // ---- workgroup reduction of the parameter gradients (fixed order over the waves) ----
    FGNN_BWD16_SCATTER_PARTIALS
    const float4 *part4 = reinterpret_cast<const float4 *>(smem);
    for (int e = threadIdx.x; e < 2 * (PCOUNT / 4); e += 64 * NWB) {
        const int m = e >= PCOUNT / 4 ? 1 : 0, ee = e - m * (PCOUNT / 4);
        float4 a = part4[(4 * m) * (PCOUNT / 4) + ee];
#pragma unroll
        for (int w = 1; w < NP; ++w) {                                   // fixed order over the MLP's four waves
            const float4 b = part4[(4 * m + w) * (PCOUNT / 4) + ee];
            a.x += b.x;
            a.y += b.y;
            a.z += b.z;
            a.w += b.w;
        }
        reinterpret_cast<float4 *>(P.m[m].wpart + (long long)blockIdx.x * PCOUNT)[ee] = a;
    }
}

template <int CA>
int launch_pair16(const fgnn_mlp_bwd16_args *a1, const fgnn_mlp_bwd16_args *a2, int tpg, int total, void *stream) {
    Pair16Args P;
    P.m[0] = *a1;
    P.m[1] = *a2;
    return launch_bwd16_grid<mlp_bwd16_pair_kernel<CA>, Pair16Layout<CA>::LDS_F * 4>(P, tpg, total, stream);
}

}  // namespace

extern "C" int fgnn_mlp_bwd16_pair(const fgnn_mlp_bwd16_args *a1, const fgnn_mlp_bwd16_args *a2, void *stream) {
    FGNN_CHECK(a1 && a2, "fgnn_mlp_bwd16_pair: null args");
    FGNN_CHECK(BWD16_WG == fgnn_mlp_bwd_num_workgroups(), "fgnn_mlp_bwd16_pair: workgroup count differs from fgnn_mlp_bwd");
    FGNN_CHECK(shape_ok16(a1) && a1->G == a2->G && a1->N == a2->N && a1->ldr == a2->ldr,
               "fgnn_mlp_bwd16_pair: the two MLPs must share G, N and ldr (G=%d N=%d ldr=%d)", a1->G, a1->N, a1->ldr);
    FGNN_CHECK(a1->depth == 3 && a2->depth == 3, "fgnn_mlp_bwd16_pair: built for depth_of_mlp = 3");
    FGNN_CHECK((a1->a.C == 2 || a1->a.C == 32) && a1->b.C == 0 && a2->b.C == 0,
               "fgnn_mlp_bwd16_pair: ONE input slab of 2 or 32 channels (got %d + %d); use fgnn_mlp_bwd16", a1->a.C, a1->b.C);
    FGNN_CHECK(a1->a.ptr && a1->a.ptr == a2->a.ptr && a1->a.C == a2->a.C && a1->a.gstride == a2->a.gstride && a1->a.ldp == a2->a.ldp &&
               a1->a.nrm == a2->a.nrm && a1->a.beta == a2->a.beta && a1->nvalid == a2->nvalid,
               "fgnn_mlp_bwd16_pair: the two MLPs must read the same input slab");
    FGNN_CHECK(!a1->ranges && !a2->ranges && !a1->nvalid, "fgnn_mlp_bwd16_pair: constant-size batches only; use fgnn_mlp_bwd16");
    FGNN_CHECK(a1->packed && a2->packed, "fgnn_mlp_bwd16_pair: needs both operand images (fgnn_pack16_operands, kind 1)");
    FGNN_CHECK(!a1->dxa && !a1->s12part, "fgnn_mlp_bwd16_pair: the input gradient and its tile sums belong to the SECOND argument block");
    FGNN_CHECK(!(a2->dxa && a2->a.C != 32), "fgnn_mlp_bwd16_pair: the input gradient exists for the 32-channel slab only");
    FGNN_CHECK(!a2->s12part || (a2->a.C == 32 && a2->dxa && a2->a.nrm), "fgnn_mlp_bwd16_pair: s12part needs dxa and a normalised 32-channel slab");
    for (const fgnn_mlp_bwd16_args *a : {a1, a2})
        if (check_mlp_args(a, "fgnn_mlp_bwd16_pair", false)) return 1;
    int tpg, total;
    if (count_tiles16(a1, "fgnn_mlp_bwd16_pair", tpg, total)) return 1;
    if (a1->a.C == 2) return launch_pair16<2>(a1, a2, tpg, total, stream);
    return launch_pair16<32>(a1, a2, tpg, total, stream);
}
