// What the bf16 MLP backward (mlp_bwd16.hip) and its mlp1 + mlp2 pair twin (mlp_bwd16_pair.hip) share: the LDS layout, the
// parked accumulator tiles, the per-graph record fetch, the phases of a tile, the launch checks and the launch.  Fused MlpBlock_Real
// backward (autograd of models/layers.py:126-131 with the GraphNorm backward of :68-80 folded into the load of dz) for gfx950:
// storage bf16, matrix work on v_mfma_f32_32x32x16_bf16, fp32 accumulation of every parameter gradient.  See mlp_fwd16.hip
// for the tile / fragment conventions (64-element tiles = 32 pixel pairs, two 32-column problems E / O per tile).
//
// Per tile and per pixel group:
//   1. recompute the hidden activations h_0 .. h_{d-2} with the forward's in-register chain (bf16 operands);
//   2. dz = R(ca*dy + cb*(z - mean) + cc)                                  (coef from fgnn_gn_bwd_coef*)
//   3. for l = d-1 .. 0:  dW_l += dpre_l (x) in_l,  db_l += dpre_l,  d in_l = R(W_l)^T dpre_l,
//                         dpre_{l-1} = R(d in_l * [h_{l-1} > 0])
//   4. dx = R(d in_0 (+ old dx)), optionally the per-tile sums {sum dx, sum dx (z_in - mean_in)} of the rounded values.
// Here, as functions: steps 1 and 2, the raw / 2-channel input fragments and the MFMA pair of every d in_l (input_grad).  As
// macros pasted into both kernels (FGNN_BWD16_*, "the tile body" below): the weight-gradient accumulators, the workgroup's tile
// range, the loads of dy and z, a slab's input operands, the step-3 loops, the S1/S2 sums of a normalised slab, the keep / store
// of a rounded dx and the scatter of a wave's partial into the reduction buffer.  NOT here, because it differs between the
// kernels: the views and the operand image(s), the per-graph record fetch, which tile a wave takes next, the old-dx loads, how
// d in_0 becomes dx (one MLP's own, or handed from the mlp1 wave to the mlp2 wave), what is emitted per tile, the sum over waves.
// The weight-gradient products contract over pixels and need lane = channel operands.  They are NOT staged through LDS:
// a fragment is transposed by multiplying it with an identity matrix on the (otherwise idle) matrix pipe
// (fgnn_bf16.h: transpose16, exact), which also yields the bias gradients as register sums.
// dW/db accumulate in registers over the wave's statically assigned tiles; the waves of a workgroup are summed through
// LDS in a fixed order and one partial per workgroup is written for fgnn_grad_finalize: bit-reproducible run to run.
#pragma once
#include <type_traits>
#include "fgnn_bf16.h"

namespace bwd16 {

constexpr int NWB = 8;           // waves per workgroup (2 per SIMD); the pair kernel runs them as NP pairs
constexpr int NP = 4;
constexpr int BWD16_WG = 256;   // persistent workgroups (partials layout shared with the fp32 path)

// IMAGES operand images (the pair kernel holds one per MLP), then the per-wave records and the parked accumulators
template <int CA, int CB, int DEPTH, int IMAGES = 1>
struct Bwd16Layout {
    static constexpr Pk16 PK = pk16_layout(1, CA, CB, DEPTH);
    static constexpr int WEIGHT_F = PK.floats;
    static constexpr int REC_F = 64 + 64 + 128;                     // per wave: {a, b'} slab a, slab b, {mean, ca, cb, cc}
    static constexpr int PCOUNT = 32 * (CA + CB) + 32 + (DEPTH - 1) * (32 * 32 + 32);
    static constexpr int MAIN_F = IMAGES * WEIGHT_F + NWB * REC_F;
    // Weight-gradient accumulator tiles kept in LDS between the tiles of the loop ("parked") instead of in registers: the
    // variants that would otherwise spill them to scratch (the 64-input-channel kernel needs four 32x32 fp32 accumulators on
    // top of everything else).  A scratch reload retires in order with the prefetch loads in flight and stalls behind them;
    // LDS does not, and ~130 KB of it are idle here.  Slots in order of use: dW_2, dW_1, dW_0 (slab a), dW_0 (slab b).
    static constexpr int NPARK = (CA >= 32 && CB >= 32) ? 4 : (CA >= 32 && CB > 0) ? 2 : (CA >= 32 ? 1 : 0);
    static constexpr int PARK_OFF = (MAIN_F + 3) & ~3;
    static constexpr int PARK_F = NWB * NPARK * 1024;
    static constexpr int RED_F = NWB * PCOUNT;                      // the reduction buffer aliases everything before it
    static constexpr int LDS_F = PARK_OFF + PARK_F > RED_F ? PARK_OFF + PARK_F : RED_F;
};

// a parked accumulator tile: [4][64 lanes][4 floats] -> conflict-free 16-byte accesses
DEVI f32x16 park_get(const float *slot, int lane) {
    f32x16 v;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 t = reinterpret_cast<const float4 *>(slot)[q * 64 + lane];
        v[4 * q] = t.x;
        v[4 * q + 1] = t.y;
        v[4 * q + 2] = t.z;
        v[4 * q + 3] = t.w;
    }
    return v;
}
DEVI void park_put(float *slot, int lane, const f32x16 &v) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
        reinterpret_cast<float4 *>(slot)[q * 64 + lane] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
}

// A base pointer passed through an empty asm: the per-lane 64-bit addresses of a once-per-graph load are then formed at the
// load, in the rarely taken branch, instead of being hoisted out of the tile loop -- where they were the single kernel's only
// spilled registers.  The pair kernel reads the same records through the plain pointers (OPAQUE = false).
template <typename T>
DEVI const T *opaque_ptr(const T *p) {
    asm volatile("" : "+s"(p));
    return p;
}
template <bool OPAQUE, typename T>
DEVI const T *graph_ptr(const T *p) {
    if constexpr (OPAQUE) return opaque_ptr(p);
    else return p;
}
// per-channel {a, b'} of a slab's GraphNorm: y = a x + b'
template <bool OPAQUE>
DEVI void fetch_rec2(float *rec, const fgnn_slab16 &s, int g, int lane) {
    if (lane < 32) {
        float2 o = make_float2(1.f, 0.f);
        if (s.nrm && lane < s.C) {
            const float4 n = reinterpret_cast<const float4 *>(graph_ptr<OPAQUE>(s.nrm))[(long long)g * s.C + lane];
            const float be = s.beta ? graph_ptr<OPAQUE>(s.beta)[lane] : 0.f;
            o.x = n.y;
            o.y = be - n.x * n.y;
        }
        reinterpret_cast<float2 *>(rec)[lane] = o;
    }
}

// transposed, normalised operand of one pixel group: lane = channel, y^T = R(x^T * a_lane + b_lane)
DEVI F16 transposed_input(const F16 &raw, const F16 &ident, bool norm, float la, float lb) {
    const f32x16 t = transpose16(raw, ident);
    F16 f;
    if (norm) {
#pragma unroll
        for (int q = 0; q < 8; ++q) f.d[q] = cvt_pk(fmaf(t[2 * q], la, lb), fmaf(t[2 * q + 1], la, lb));
    } else {
        pack_acc(f, t);
    }
    return f;
}

DEVI float sum16(const f32x16 &t) {
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) s += t[r];
    return s;
}

// the pixel group's half of a loaded dword (GRP 0 = even, 1 = odd pixels of the pairs)
template <int GRP>
DEVI float half_of(unsigned d) { return GRP ? bf_hi(d) : bf_lo(d); }
template <int GRP>
DEVI unsigned pack_of(unsigned a, unsigned b) { return GRP ? pack_hi(a, b) : pack_lo(a, b); }

// ---- the phases of one pixel group -----------------------------------------------------------------------------------------

template <int GRP>
DEVI void raw_fragment(F16 &raw, const unsigned (&x)[16]) {
#pragma unroll
    for (int q = 0; q < 8; ++q) raw.d[q] = pack_of<GRP>(x[2 * q], x[2 * q + 1]);
}
template <int GRP>
DEVI void narrow_fragment(F16 &y, const unsigned (&x)[2]) {
#pragma unroll
    for (int q = 0; q < 8; ++q) y.d[q] = 0u;
    y.d[0] = pack_of<GRP>(x[0], x[1]);
}

// forward recompute: h_0 .. h_{d-2} from the operand image `wl` (biases in its `tail`)
template <int CA, int CB, int DEPTH>
DEVI void recompute_hidden(F16 (&hs)[DEPTH - 1], const F16 &ya, const F16 &yb, const float *wl, const float *tail, int lane, int h) {
    constexpr Pk16 PK = Bwd16Layout<CA, CB, DEPTH>::PK;
    constexpr int SA = pk16_steps(CA), SB = pk16_steps(CB);
    f32x16 acc;
    load_bias16(acc, tail, 0, h);
#pragma unroll
    for (int t = 0; t < SA; ++t) acc = mfma16(lds_step(wl, PK.off_w0a + t, lane), step_of(ya, t), acc);
#pragma unroll
    for (int t = 0; t < SB; ++t) acc = mfma16(lds_step(wl, PK.off_w0b + t, lane), step_of(yb, t), acc);
    pack_acc_relu(hs[0], acc);
#pragma unroll
    for (int l = 1; l + 1 < DEPTH; ++l) {
        load_bias16(acc, tail, l, h);
#pragma unroll
        for (int t = 0; t < 2; ++t) acc = mfma16(lds_step(wl, PK.off_wh + 2 * (l - 1) + t, lane), step_of(hs[l - 1], t), acc);
        pack_acc_relu(hs[l], acc);
    }
}

// dz from (dy, z, coef), rounded to bf16; fv = 0 in the padding, 1 elsewhere
template <int GRP>
DEVI void dz_of(F16 &d, const unsigned (&dyr)[16], const unsigned (&zr)[16], const float *recK, float fv, int h) {
    const float4 *kp = reinterpret_cast<const float4 *>(recK);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const float4 k0 = kp[ch_of(2 * q, h)], k1 = kp[ch_of(2 * q + 1, h)];
        const float e0 = fmaf(k0.y, half_of<GRP>(dyr[2 * q]), fmaf(k0.z, half_of<GRP>(zr[2 * q]) - k0.x, k0.w));
        const float e1 = fmaf(k1.y, half_of<GRP>(dyr[2 * q + 1]), fmaf(k1.z, half_of<GRP>(zr[2 * q + 1]) - k1.x, k1.w));
        d.d[q] = cvt_pk(e0 * fv, e1 * fv);
    }
}

// d in = R(W)^T d: the two MFMAs against the transposed weights at image step `step`
DEVI f32x16 input_grad(const float *wl, int step, const F16 &d, int lane) {
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f32x16 acc = mfma16(lds_step(wl, step, lane), step_of(d, 0), zero);
    return mfma16(lds_step(wl, step + 1, lane), step_of(d, 1), acc);
}

// ---- the tile body -----------------------------------------------------------------------------------------------------------
// These are MACROS, pasted into the two kernels, and not functions: as functions, as a struct or behind reference parameters each
// of them changed the register allocation of several instantiations; a macro hands the compiler the text it
// had before.  The comment above each names what it reads and writes of the enclosing scope.  `s` / `S` select a slab: (a, A) or (b, B).

// The weight-gradient accumulators of a wave.  DEFINES, for the rest of the kernel: dW0a, dW0b, dWh[], db[] (zeroed), NPARK,
// park (this wave's NPARK parked tiles, zeroed) and accum(slot, reg, f), which applies f to parked tile `slot` if slot < NPARK
// and to the register tile `reg` otherwise.  Reads smem, wv, lane, L, DEPTH.
#define FGNN_BWD16_ACCUMULATORS                                                                         \
    f32x16 dW0a, dW0b, dWh[DEPTH - 1];                                                                  \
    float db[DEPTH];                                                                                    \
    zero16f(dW0a);                                                                                      \
    zero16f(dW0b);                                                                                      \
    _Pragma("unroll") for (int l = 0; l + 1 < DEPTH; ++l) zero16f(dWh[l]);                              \
    constexpr int NPARK = L::NPARK;                                                                     \
    float *park = smem + L::PARK_OFF + wv * (NPARK * 1024);                                             \
    _Pragma("unroll") for (int s = 0; s < NPARK; ++s) park_put(park + s * 1024, lane, dW0a);            \
    auto accum = [&](auto slot, f32x16 &reg, auto &&f) {                                                \
        constexpr int S = decltype(slot)::value;                                                        \
        if constexpr (S < NPARK) {                                                                      \
            f32x16 a = park_get(park + S * 1024, lane);                                                 \
            f(a);                                                                                       \
            park_put(park + S * 1024, lane, a);                                                         \
        } else {                                                                                        \
            f(reg);                                                                                     \
        }                                                                                               \
    };                                                                                                  \
    _Pragma("unroll") for (int l = 0; l < DEPTH; ++l) db[l] = 0.f;

// The workgroup's tile range.  DEFINES nwg, q_, rem, T0, T1: an even split of total_tiles, or (SKIP) the work-balanced range of
// fgnn_ragged_tile_ranges16.  Reads total_tiles, SKIP, A.ranges.
#define FGNN_BWD16_TILE_RANGE                                                           \
    const int nwg = gridDim.x;                                                          \
    const int q_ = total_tiles / nwg, rem = total_tiles % nwg;                          \
    int T0 = blockIdx.x * q_ + ((int)blockIdx.x < rem ? (int)blockIdx.x : rem);         \
    int T1 = T0 + q_ + ((int)blockIdx.x < rem ? 1 : 0);                                 \
    if constexpr (SKIP) {                                                               \
        T0 = A.ranges[blockIdx.x];                                                      \
        T1 = A.ranges[blockIdx.x + 1];                                                  \
    }

// dy and z of a tile, requested up front.  DEFINES dyr[16], zr[16].  Reads lo4, c, vdy, vz, roff.
#define FGNN_BWD16_LOAD_DY_Z                                                                            \
    unsigned dyr[16], zr[16];                                                                           \
    {                                                                                                   \
        const int vo_dy = lo4 + c.g * vdy.gs2, vo_z = lo4 + c.g * vz.gs2;                               \
        _Pragma("unroll") for (int r = 0; r < 16; ++r) dyr[r] = buf_load_u32(vdy, vo_dy, roff(r));      \
        _Pragma("unroll") for (int r = 0; r < 16; ++r) zr[r] = buf_load_u32(vz, vo_z, roff(r));         \
    }

// Input operands of slab s for pixel group GRP: y##s (normal: the recompute's) and yT##s (transposed: the layer-0 weight
// gradient's), for a 32-channel slab also raw_##s; nothing for an absent slab.  Writes these three; reads x##s, C##S, norm##S,
// rec##S, l##s##_a, l##s##_b, ident, h.
#define FGNN_BWD16_INPUT(s, S)                                                                                                  \
    if constexpr (C##S >= 32) {                                                                                                 \
        raw_fragment<GRP>(raw_##s, x##s);                                                                                       \
        if (norm##S) {                                                                                                          \
            const float2 *r2 = reinterpret_cast<const float2 *>(rec##S);                                                        \
            _Pragma("unroll") for (int q = 0; q < 8; ++q) {                                                                     \
                const float2 n0 = r2[ch_of(2 * q, h)], n1 = r2[ch_of(2 * q + 1, h)];                                            \
                y##s.d[q] = cvt_pk(fmaf(half_of<GRP>(x##s[2 * q]), n0.x, n0.y), fmaf(half_of<GRP>(x##s[2 * q + 1]), n1.x, n1.y)); \
            }                                                                                                                   \
        } else {                                                                                                                \
            y##s = raw_##s;                                                                                                     \
        }                                                                                                                       \
        yT##s = transposed_input(raw_##s, ident, norm##S, l##s##_a, l##s##_b);                                                  \
    } else if constexpr (C##S > 0) {                                                                                            \
        narrow_fragment<GRP>(y##s, x##s);                                                                                       \
        yT##s = transposed_input(y##s, ident, false, 1.f, 0.f);                                                                 \
    }

// Hidden layers l = DEPTH-1 .. 1: dW_l += dpre_l (x) h_{l-1} (slot 0 for l = 2, slot 1 for l = 1), db_l, and d <- dpre_{l-1}.
// Reads hs, ident, wl, PK, lane, accum; writes d, db, dWh.
#define FGNN_BWD16_HIDDEN_LAYERS                                                                                        \
    _Pragma("unroll") for (int l = DEPTH - 1; l >= 1; --l) {                                                            \
        const F16 &in = hs[l - 1];                                                                                      \
        {                                                                                                               \
            f32x16 t = transpose16(d, ident);                                                                           \
            db[l] += sum16(t);                                                                                          \
            F16 dT, hT;                                                                                                 \
            pack_acc(dT, t);                                                                                            \
            t = transpose16(in, ident);                                                                                 \
            pack_acc(hT, t);                                                                                            \
            auto upd = [&](f32x16 &a) {                                                                                 \
                a = mfma16(step_of(dT, 0), step_of(hT, 0), a);                                                          \
                a = mfma16(step_of(dT, 1), step_of(hT, 1), a);                                                          \
            };                                                                                                          \
            if (l == 2) accum(std::integral_constant<int, 0>(), dWh[l - 1], upd);                                       \
            else accum(std::integral_constant<int, 1>(), dWh[l - 1], upd);                                              \
        }                                                                                                               \
        {                                                                                                               \
            const f32x16 acc = input_grad(wl, PK.off_wt + 2 * (DEPTH - 1 - l), d, lane);                                \
            _Pragma("unroll") for (int q = 0; q < 8; ++q) d.d[q] = cvt_pk(acc[2 * q], acc[2 * q + 1]) & pos_mask_pk(in.d[q]); \
        }                                                                                                               \
    }

// Layer 0: dW_0 += dpre_0 (x) the transposed inputs (slot 2: slab a, slot 3: slab b), db_0.  Reads d, ident, yTa, yTb, CB, accum;
// writes db, dW0a, dW0b.
#define FGNN_BWD16_LAYER0                                                           \
    {                                                                               \
        f32x16 t = transpose16(d, ident);                                           \
        db[0] += sum16(t);                                                          \
        F16 dT;                                                                     \
        pack_acc(dT, t);                                                            \
        accum(std::integral_constant<int, 2>(), dW0a, [&](f32x16 &a) {              \
            a = mfma16(step_of(dT, 0), step_of(yTa, 0), a);                         \
            a = mfma16(step_of(dT, 1), step_of(yTa, 1), a);                         \
        });                                                                         \
        if constexpr (CB > 0) {                                                     \
            accum(std::integral_constant<int, 3>(), dW0b, [&](f32x16 &a) {          \
                a = mfma16(step_of(dT, 0), step_of(yTb, 0), a);                     \
                a = mfma16(step_of(dT, 1), step_of(yTb, 1), a);                     \
            });                                                                     \
        }                                                                           \
    }

// Sums of the producer of a normalised slab a: S1 = sum v, S2 = sum v (z_a - mean_a), v = R(dx) (exactly 0 on invalid pixels: dz
// is masked and the stored padding of the old dx is 0).  Reads v, raw_a, ident, la_mean; adds to es1, es2.
#define FGNN_BWD16_EMIT_NORMALISED(v)                                               \
    {                                                                               \
        const f32x16 tv = transpose16(v, ident), tx = transpose16(raw_a, ident);    \
        _Pragma("unroll") for (int r = 0; r < 16; ++r) {                            \
            es1 += tv[r];                                                           \
            es2 = fmaf(tv[r], tx[r] - la_mean, es2);                                \
        }                                                                           \
    }

// The rounded dx `v` of slab s: kept (keep##S) on the even pixel group, stored interleaved with the kept half on the odd one.
// Reads GRP, lo4, c, vdx##s, roff.
#define FGNN_BWD16_KEEP_OR_STORE(v, s, S)                                                       \
    if constexpr (GRP == 0) {                                                                   \
        keep##S = v;                                                                            \
    } else {                                                                                    \
        const int vo = lo4 + c.g * vdx##s.gs2;                                                  \
        _Pragma("unroll") for (int q = 0; q < 8; ++q) {                                         \
            buf_store_u32(pack_lo(keep##S.d[q], v.d[q]), vdx##s, vo, roff(2 * q));              \
            buf_store_u32(pack_hi(keep##S.d[q], v.d[q]), vdx##s, vo, roff(2 * q + 1));          \
        }                                                                                       \
    }

// After the tile loop: the two halves of db summed, the parked accumulators back in registers (the reduction buffer aliases
// them), and, behind a barrier, this wave's partial scattered into the reduction buffer in the partial's layout
// [W0 (32*CIN) | b0 (32) | W1 (1024) | b1 (32) | ...].  DEFINES PCOUNT.  Reads smem, wv, lane, j, h, park, NPARK, CA, CB, CIN, L.
#define FGNN_BWD16_SCATTER_PARTIALS                                                                             \
    constexpr int PCOUNT = L::PCOUNT;                                                                           \
    _Pragma("unroll") for (int l = 0; l < DEPTH; ++l) db[l] += __shfl_xor(db[l], 32);                           \
    if constexpr (NPARK > 0) dWh[1] = park_get(park, lane);                                                     \
    if constexpr (NPARK > 1) dWh[0] = park_get(park + 1024, lane);                                              \
    if constexpr (NPARK > 2) dW0a = park_get(park + 2 * 1024, lane);                                            \
    if constexpr (NPARK > 3) dW0b = park_get(park + 3 * 1024, lane);                                            \
    __syncthreads(); /* everyone done with the operand image and the parked tiles */                            \
    {                                                                                                           \
        float *red = smem + wv * PCOUNT;                                                                        \
        _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                                        \
            const int o = ch_of(r, h);                                                                          \
            if (j < CA) red[o * CIN + j] = dW0a[r];                                                             \
            if (CB > 0 && j < CB) red[o * CIN + CA + j] = dW0b[r];                                              \
        }                                                                                                       \
        int off = 32 * CIN;                                                                                     \
        _Pragma("unroll") for (int l = 0; l < DEPTH; ++l) {                                                     \
            if (l > 0) {                                                                                        \
                _Pragma("unroll") for (int r = 0; r < 16; ++r) red[off + ch_of(r, h) * 32 + j] = dWh[l - 1][r]; \
                off += 1024;                                                                                    \
            }                                                                                                   \
            if (h == 0) red[off + j] = db[l];                                                                   \
            off += 32;                                                                                          \
        }                                                                                                       \
    }                                                                                                           \
    __syncthreads();                                                                                            \
    static_assert(PCOUNT % 4 == 0, "partials are summed four at a time");

// ---- host side: what the two entry points check and how they launch (`fn` = the entry point's name) ---------------------------
inline bool shape_ok16(const fgnn_mlp_bwd16_args *a) { return a->G > 0 && a->N > 0 && a->ldr >= a->N && a->ldr % 8 == 0; }

// per MLP (`two_slabs`: slab b and dxb count too)
inline int check_mlp_args(const fgnn_mlp_bwd16_args *a, const char *fn, bool two_slabs) {
    FGNN_CHECK(a->dy && a->z && a->wpart && a->coef, "%s: missing dy/z/wpart/coef", fn);
    const long long lim = 0x7fffffffll / 2, G = a->G;
    FGNN_CHECK(G * a->a.gstride < lim && G * a->dgstride < lim && G * a->zgstride < lim && G * a->dxa_gstride < lim &&
               (!two_slabs || (G * a->b.gstride < lim && G * a->dxb_gstride < lim)),
               "%s: a tensor exceeds 2 GiB (32-bit buffer addressing); split the batch", fn);
    return 0;
}

// tiles per graph and of the batch
inline int count_tiles16(const fgnn_mlp_bwd16_args *a, const char *fn, int &tpg, int &total) {
    tpg = fgnn_tiles_per_graph16(a->N, a->ldr);
    const long long t = (long long)a->G * tpg;
    FGNN_CHECK(t < (1ll << 30), "%s: too many tiles", fn);
    total = (int)t;
    return 0;
}

// KERNEL(args, tpg, total) on the persistent grid with LDS bytes of dynamic shared memory
template <auto KERNEL, int LDS, class Args>
int launch_bwd16_grid(const Args &args, int tpg, int total, void *stream) {
    static_assert(LDS <= 160 * 1024, "LDS budget");
    static LdsAttrCache attr_cache;
    (void)fgnn_raise_lds(attr_cache, (const void *)KERNEL, LDS);
    hipLaunchKernelGGL(KERNEL, dim3(BWD16_WG), dim3(64 * NWB), LDS, (hipStream_t)stream, args, tpg, total);
    FGNN_LAUNCH_CHECK();
    return 0;
}

}  // namespace bwd16
