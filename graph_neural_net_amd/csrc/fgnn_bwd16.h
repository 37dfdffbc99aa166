// What the bf16 MLP backward (mlp_bwd16.hip) and its mlp1 + mlp2 pair twin (mlp_bwd16_pair.hip) share: the LDS layout, the
// parked accumulator tiles, the per-graph record fetch, phases of one pixel group and the launch checks.  Fused MlpBlock_Real
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
// Here: steps 1 and 2, the raw / 2-channel input fragments and the MFMA pair of every d in_l (input_grad).  The normalised
// input fragment, the weight-gradient accumulators with the step-3 loop around them and the workgroup reduction are still
// written out in both kernels: moved into functions of this header they compile to different code.
// The weight-gradient products contract over pixels and need lane = channel operands.  They are NOT staged through LDS:
// a fragment is transposed by multiplying it with an identity matrix on the (otherwise idle) matrix pipe
// (fgnn_bf16.h: transpose16, exact), which also yields the bias gradients as register sums.
// dW/db accumulate in registers over the wave's statically assigned tiles; the waves of a workgroup are summed through
// LDS in a fixed order and one partial per workgroup is written for fgnn_grad_finalize: bit-reproducible run to run.
#pragma once
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

// ---- what a launch checks per MLP (`fn` = the entry point's name; `two_slabs`: slab b and dxb count too) ---------------------
inline int check_mlp_args(const fgnn_mlp_bwd16_args *a, const char *fn, bool two_slabs) {
    FGNN_CHECK(a->dy && a->z && a->wpart && a->coef, "%s: missing dy/z/wpart/coef", fn);
    const long long lim = 0x7fffffffll / 2, G = a->G;
    FGNN_CHECK(G * a->a.gstride < lim && G * a->dgstride < lim && G * a->zgstride < lim && G * a->dxa_gstride < lim &&
               (!two_slabs || (G * a->b.gstride < lim && G * a->dxb_gstride < lim)),
               "%s: a tensor exceeds 2 GiB (32-bit buffer addressing); split the batch", fn);
    return 0;
}

}  // namespace bwd16
