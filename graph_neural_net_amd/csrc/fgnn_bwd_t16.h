// What the two 16-pixel fp32 MLP backward kernels share beyond fgnn_bwd32.h: mlp_bwd_t16.hip (mlp3 of a block: two input slabs) and
// mlp_bwd_pair_t16.hip (mlp1 + mlp2 of a block in one launch, one MLP per wave of a SIMD's pair).  Autograd of models/layers.py:126-131
// with the GraphNorm backward of :68-80 folded into dz, depth 3, on v_mfma_f32_16x16x4_f32 (fgnn_t16.h).
//
// Per 16-pixel half tile (one wave; lane (px, q) holds 8 channels of pixel px in registers):
//   1. the input slab(s), normalised with the graph's record {mean, a, beta}, are staged as x tile(s) and run through layer 0;
//      h1 = relu(.) -> tile S0, layer 1, h2 = relu(.) -> tile S1 (FGNN_T16_RECOMPUTE_HIDDEN).  The fma sequence is the forward's, so h1, h2 and
//      every ReLU decision are bit-identical to it; both stay in registers for the masks;
//   2. dz = cb*(z - mean) + (ca*dy + cc) from the graph's dz record {mean, ca, cb, cc}, zero on padding pixels -- the ONLY place the
//      padding mask is applied: every weight-gradient operand and every dx of a padding pixel is then 0 (FGNN_T16_DZ) -> tile S2;
//   3. layer 2: d h2 = W_2^T dz, dW_2 += dz (x) h2 (wgrad16 reads both operands transposed from their tiles, db_2 from the same
//      reads), dpre_1 = d h2 * [h2 > 0] -> tile S1; layer 1 the same with (W_1^T, dpre_1, h1) -> dpre_0 -> tile S2 (FGNN_T16_HIDDEN_BWD);
//   4. layer 0: dx = W_0^T dpre_0 per slab, dW_0 += dpre_0 (x) x tile.  This part differs: the mlp3 kernel has two slabs and stores
//      two dx, the pair kernel runs one dx chain through both waves of the pair.
// Per-graph records live in registers for all halves of a graph; at a graph change one channel per lane (lanes 0..31) fetches or
// derives them (the derivation -- two divisions per channel -- is then one instance per lane instead of eight) and a wave-private
// LDS copy hands every lane its 8 channels (FGNN_T16_READ_RECORDS).
// dW / db accumulate in registers over the wave's halves; at the end each wave scatters them into the reduction buffer in the
// partial's layout [W0 (32 * CIN) | b0 (32) | W1 (1024) | b1 (32) | W2 (1024) | b2 (32)] and fgnn_bwd32.h sums the waves.
// NOT here: which half a wave takes next, the hand-over between the waves of a pair, the order in which the loads of the next half
// are issued and every sched_barrier.  They are what differs between the two kernels; the comments there say why each line is
// where it is.
#pragma once
#include "fgnn_t16.h"
#include "fgnn_pack.h"
#include "fgnn_bwd32.h"

namespace {

using namespace t16;

// IMAGES operand images of kind 5 (fgnn_pack.h: 32 + CB input channels), then NSLOTS 32 x 16 tiles per wave; the kernel's own
// buffers follow from TILE_END, the reduction buffer aliases everything
template <int CB, int IMAGES, int NSLOTS>
struct BwdT16Layout {
    static constexpr int DEPTH = 3;
    static constexpr PkBwd PK = pk_bwd(32, CB, DEPTH);
    static constexpr int OFF_W1 = PK.off_wh, OFF_WT1 = PK.off_wt, OFF_WT2 = PK.off_wt + 16;
    static constexpr int BIAS_F = PK.bias_f;
    static constexpr int WEIGHT_F = pk_pad_floats(PK.floats);             // floats per image (whole KiB: global_load_lds)
    static constexpr int NSLOT = NSLOTS;
    static constexpr int CIN = 32 + CB;
    static constexpr int PCOUNT = 32 * CIN + 32 + (DEPTH - 1) * (32 * 32 + 32);
    static constexpr int TILE_OFF = IMAGES * WEIGHT_F;
    static constexpr int TILE_END = TILE_OFF + NW * NSLOT * TILE_F;
    static constexpr int RED_F = NW * PCOUNT;
};

// ---- phases of one half ----------------------------------------------------------------------------------------------------------
// These are MACROS, pasted into the two tile loops, and not functions: both loops sit at the register limit of two waves per SIMD
// (232 - 255 VGPRs) and each of these phases, tried as a function with reference parameters, changed the register allocation or the
// s_waitcnt count of several kernels (DESIGN.md section 4 has the figures).  They use the kernels' common names: wl, lane, q,
// lane_base, rec (the wave's 64 float4 of records), kx / ky / kz / kw / mean / av, dyr / zr, the tiles S0 / S1 / S2, L = the layout.

// the records of this lane's 8 channels from the wave's LDS copy: dz coefficients, and (norm) the input slab's {mean, a}
#define FGNN_T16_READ_RECORDS(norm)                                 \
    _Pragma("unroll") for (int s = 0; s < 8; ++s) {                 \
        const float4 k4 = rec[chan_s(s) + chan_q(q)];               \
        kx[s] = k4.x;                                               \
        ky[s] = k4.y;                                               \
        kz[s] = k4.z;                                               \
        kw[s] = k4.w;                                               \
        if (norm) {                                                 \
            const float4 n = rec[32 + chan_s(s) + chan_q(q)];       \
            mean[s] = n.x;                                          \
            av[s] = n.y;                                            \
        }                                                           \
    }

// acc = layer 0's pre-activation: h1 -> S0, layer 1, h2 -> S1 (h1, h2 stay in registers for the ReLU masks)
#define FGNN_T16_RECOMPUTE_HIDDEN(acc, h1, h2)                                              \
    _Pragma("unroll") for (int s = 0; s < 8; ++s) h1[s] = relu1(acc[s >> 2][s & 3]);        \
    stage8(S0, lane_base, h1);                                                              \
    load_bias(acc, wl + L::BIAS_F, 1, q);                                                   \
    gemm32<L::OFF_W1>(acc, wl, h1, lane);                                                   \
    _Pragma("unroll") for (int s = 0; s < 8; ++s) h2[s] = relu1(acc[s >> 2][s & 3]);        \
    stage8(S1, lane_base, h2);

// dz from (dy, z, coef); the ONLY place the padding mask is applied (`full`, wave-uniform: no padding pixel in this half)
#define FGNN_T16_DZ(dpre)                                                                                                   \
    _Pragma("unroll") for (int s = 0; s < 8; ++s) dpre[s] = fmaf(kz[s], zr[s] - kx[s], fmaf(ky[s], dyr[s], kw[s]));         \
    if (!full) {                                                                                                            \
        _Pragma("unroll") for (int s = 0; s < 8; ++s) dpre[s] = valid ? dpre[s] : 0.f;                                      \
    }

// one hidden layer backward: d in = W^T dpre (operand set OFF_WT), dW += Dt (x) In with db from the same reads, dpre <- d in * [h > 0]
#define FGNN_T16_HIDDEN_BWD(OFF_WT, dpre, dW, db, Dt, In, h)                                                \
    {                                                                                                       \
        f32x4 a2[2];                                                                                        \
        a2[0] = a2[1] = zero4();                                                                            \
        gemm32<OFF_WT>(a2, wl, dpre, lane);                                                                 \
        wgrad16(dW, db, Dt, In, lane);                                                                      \
        _Pragma("unroll") for (int s = 0; s < 8; ++s) dpre[s] = h[s] > 0.f ? a2[s >> 2][s & 3] : 0.f;       \
    }

// bias gradients: lane (i, q) holds the sum over pixels 4 q .. 4 q + 3 of its row; sum the four q
#define FGNN_T16_DB_BUTTERFLY(db0, db1, db2)            \
    _Pragma("unroll") for (int b = 0; b < 2; ++b) {     \
        db0[b] += __shfl_xor(db0[b], 16);               \
        db0[b] += __shfl_xor(db0[b], 32);               \
        db1[b] += __shfl_xor(db1[b], 16);               \
        db1[b] += __shfl_xor(db1[b], 32);               \
        db2[b] += __shfl_xor(db2[b], 16);               \
        db2[b] += __shfl_xor(db2[b], 32);               \
    }

}  // namespace
