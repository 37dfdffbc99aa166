// The panel code of the spectral-feature kernels (gfx950), shared by spectral.hip (fp32 planes) and spectral_slab.hip (the bf16
// input slab): the staging of W and s, the power chain on v_mfma_f32_32x32x2_f32 and the panel hand-over between two powers.  The
// two kernels differ in where a power goes, nothing else: the chain below hands every power of every column block to the caller's
// `emit` as the fp32 D fragment, so both write the same values by construction.  See spectral.hip for the scheme.
#pragma once
#include "fgnn_common.h"

constexpr int SP_THREADS = 256;            // 4 waves; thread t stages row t of W (N <= 256)
constexpr int SP_ROWS = 32;                // rows of a panel

// the bits of word w of a row that lie inside the n x n corner
DEVI unsigned corner_mask(int w, int n) {
    const int lo = 32 * w;
    return n >= lo + 32 ? 0xffffffffu : (n > lo ? (1u << (n - lo)) - 1u : 0u);
}
DEVI rsrc_t make_rsrc(const void *p, long long bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, (int)bytes, 0x00020000);
}
// the vertex count of graph g, clamped to [0, N] (N without nvalid)
DEVI int sp_nvalid(const int *nvalid, int G, int g, int N) {
    const rsrc_t nv_r = make_rsrc(nvalid, nvalid ? (long long)G * 4 : 0);
    const int nv = __builtin_amdgcn_raw_buffer_load_b32(nv_r, 0, g * 4, 0);
    return nvalid ? min(max(nv, 0), N) : N;
}

// NW = words per staged row (N <= 32 NW).  42 KB at NW = 8.
template <int NW>
struct SpLds {
    static constexpr int NP = 32 * NW, P = NP + 1;     // P odd: the 32 rows a half-wave reads at one k are 32 banks
    unsigned wl[NP * NW];                  // rows of W, zero outside the corner
    float sl[NP];                          // s_k, zero for k >= n and for isolated vertices
    float panel[SP_ROWS * P];              // F_p[i0 + i][k] s_k
};

// one power of one column block: acc += panel (32 x K, scaled by s_k) @ W[0 .. K)[32 jb .. 32 jb + 31]
template <int NW, int P>
DEVI void panel_times_w(f32x16 &acc, const float *panel, const unsigned *wl, int K, int jb, int lane) {
    const int j = lane & 31, h = lane >> 5;
    const float *a = panel + j * P + h;
    const unsigned *w = wl + h * NW + jb;
    for (int k0 = 0; k0 < K; k0 += 32) {        // K is a multiple of 32
#pragma unroll
        for (int k = k0; k < k0 + 32; k += 2) acc = mfma32(a[k], (float)((w[k * NW] >> j) & 1u), acc);
    }
}
// the same for two column blocks sharing the A operand
template <int NW, int P>
DEVI void panel_times_w2(f32x16 &acc0, f32x16 &acc1, const float *panel, const unsigned *wl, int K, int jb0, int jb1, int lane) {
    const int j = lane & 31, h = lane >> 5;
    const float *a = panel + j * P + h;
    const unsigned *w = wl + h * NW;
    for (int k0 = 0; k0 < K; k0 += 32) {
#pragma unroll
        for (int k = k0; k < k0 + 32; k += 2) {
            const float av = a[k];
            acc0 = mfma32(av, (float)((w[k * NW + jb0] >> j) & 1u), acc0);
            acc1 = mfma32(av, (float)((w[k * NW + jb1] >> j) & 1u), acc1);
        }
    }
}

// stage W of graph g (masked to the n x n corner) and s; ends with the barrier that publishes them
template <int NW>
DEVI void sp_stage(SpLds<NW> &L, const unsigned *bits, int g, int N, int n, int tid) {
    constexpr int NP = SpLds<NW>::NP;
    const int W = (N + 31) >> 5;
    const rsrc_t bits_r = make_rsrc(bits + (long long)g * N * W, (long long)N * W * 4);
    int deg = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const unsigned v = (unsigned)__builtin_amdgcn_raw_buffer_load_b32(bits_r, (tid < N && w < W) ? (tid * W + w) * 4 : OOB_OFF, 0, 0)
                           & (tid < n ? corner_mask(w, n) : 0u);
        if (tid < NP) L.wl[tid * NW + w] = v;
        deg += __popc(v);
    }
    if (tid < NP) L.sl[tid] = deg > 0 ? 1.0f / __builtin_sqrtf((float)deg) : 0.0f;
    __syncthreads();
}

// The power chain of the panel of rows i0 .. i0 + 31 (i0 < n) after sp_stage.  emit(p, jb, f): f = rows ch_of(r, h) of column
// 32 jb + (lane & 31) of F_{p+1}, for every column block jb the wave owns (wave w: blocks w and, at NW = 8, w + 4) -- zeros where
// the block lies past the corner.  Every wave calls emit the same number of times, with all lanes active.
template <int NW, class Emit>
DEVI void sp_powers(SpLds<NW> &L, int n, int i0, int n_powers, int tid, Emit &&emit) {
    constexpr int P = SpLds<NW>::P, NACC = NW > 4 ? 2 : 1;
    const int wv = tid >> 6, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const unsigned *wl = L.wl;
    const float *sl = L.sl;
    float *panel = L.panel;
    const int nb = (n + 31) >> 5, K = 32 * nb;  // live column blocks; the contraction runs over whole words (zeros past n)
    int jb[NACC];
    bool live[NACC];
    float sj[NACC];
    f32x16 acc[NACC];
#pragma unroll
    for (int a = 0; a < NACC; ++a) {
        jb[a] = wv + 4 * a;
        live[a] = jb[a] < nb;                   // uniform per wave
        const int jc = live[a] ? jb[a] : 0;
        sj[a] = live[a] ? sl[32 * jc + j] : 0.0f;
        // power 1 before its column scale: s_i w_ij, in the D layout (register r of half h = row (r & 3) + 8 (r >> 2) + 4 h)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = i0 + ch_of(r, h);
            const unsigned bit = (wl[i * NW + jc] >> j) & 1u;
            acc[a][r] = (live[a] && bit) ? sl[i] : 0.0f;
        }
    }

    for (int p = 0; p < n_powers; ++p) {
        if (p > 0) {
            if (NACC == 2 && live[NACC - 1]) {
                panel_times_w2<NW, P>(acc[0], acc[NACC - 1], panel, wl, K, jb[0], jb[NACC - 1], lane);
            } else if (live[0]) {
                panel_times_w<NW, P>(acc[0], panel, wl, K, jb[0], lane);
            }
        }
        // F_p = acc s_j -> the caller; acc <- F_p s_j, the next A operand
#pragma unroll
        for (int a = 0; a < NACC; ++a) {
            f32x16 f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                f[r] = acc[a][r] * sj[a];
                acc[a][r] = f[r] * sj[a];
            }
            emit(p, jb[a], f);
        }
        if (p + 1 == n_powers) break;
        __syncthreads();                        // every wave has read the panel of this power
#pragma unroll
        for (int a = 0; a < NACC; ++a) {
            if (live[a]) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    panel[ch_of(r, h) * P + 32 * jb[a] + j] = acc[a][r];
                    acc[a][r] = 0.0f;
                }
            }
        }
        __syncthreads();
    }
}
