// The spectral input straight into the bf16 input slab of block 1 (gfx950): what fgnn_spectral_features followed by
// fgnn_to_bf16_pad leave in the (G, CP, ldp) slab, byte for byte, in ONE launch and without the fp32 planes in HBM.
//
// The power chain is the one of spectral.hip (fgnn_spectral.h: same staging, same MFMA order, fp32 throughout); a power is rounded
// to bf16 (nearest even, v_cvt_pk_bf16_f32) only on its way out.  Every element of the slab has exactly one writer:
//   * the VALUE part -- channels p < n_powers, rows i < N of a live panel (i0 < n_g), columns j < N8 = N rounded up to 8 -- is written
//     by the workgroup that owns the panel, from the D fragments.  Inside it everything outside the n_g x n_g corner is +0 by
//     arithmetic (s_j = 0 there, the masked bit rows are zero), as in the fp32 planes.
//   * everything else -- channels >= n_powers (28 of 32 at P = 4: the bulk of the bytes), the panels of the ragged padding, the pitch
//     columns N8 <= j < ldr and the tail of every channel up to ldp -- is +0 written as 16-byte pieces, dealt round-robin over the
//     `panels` workgroups of the graph BEFORE they stage W (the stores drain under the chain).  ldr is a multiple of 8 and ldp of 64,
//     so a piece lies inside one row of one channel and is either wholly value or wholly zero.
// The D fragment has the column on the lane: neighbouring lanes exchange the registers of each register pair (DPP quad_perm
// [1,0,3,2]), so that the even lane holds columns (j, j + 1) of row ch_of(2q, h) and the odd lane those of row ch_of(2q + 1, h):
// eight dword stores per column block and power instead of sixteen 2-byte ones, every lane storing, no LDS (the panel is still
// being read by the other waves at that point).  ldr is even, so a pair never straddles rows.
// No scratch; LDS = the one SpLds of spectral.hip (42 KB at N = 256); figures in DESIGN.md section 10.1.
#include "fgnn_bf16.h"
#include "fgnn_spectral.h"

namespace {

// grid: G * panels workgroups, panels = ceil(N / 32); workgroup b = (graph b / panels, panel b % panels).  pieces = ldp / 8.
template <int NW>
__global__ __launch_bounds__(SP_THREADS) void spectral_slab_kernel(const unsigned *bits, const int *nvalid, int G, int N, int n_powers,
                                                                   int CP, int ldr, uint4 *y, int pieces, int panels) {
    __shared__ SpLds<NW> L;
    const int g = blockIdx.x / panels, pn = blockIdx.x - g * panels, i0 = pn * SP_ROWS, tid = threadIdx.x;
    const int lane = tid & 63, j = lane & 31, h = lane >> 5;
    const int n = sp_nvalid(nvalid, G, g, N);
    const int N8 = (N + 7) & ~7;
    uint4 *yg = y + (long long)g * CP * pieces;          // (CP * pieces < 2^27: checked by the launcher)

    // ---- the zero part, this workgroup's share
    {
        const uint4 z = {0u, 0u, 0u, 0u};
        const int stride = panels * SP_THREADS, low = n_powers * pieces, all = CP * pieces;
        for (int t = pn * SP_THREADS + tid; t < low; t += stride) {      // channels that hold a power: all but the value part
            const int q = t % pieces, pos = 8 * q, i = pos / ldr, j0 = pos - i * ldr;
            const bool value = i < N && (i & ~(SP_ROWS - 1)) < n && j0 < N8;
            if (!value) yg[t] = z;
        }
        for (int t = low + pn * SP_THREADS + tid; t < all; t += stride) yg[t] = z;      // channels >= n_powers
    }
    if (i0 >= n) return;                        // uniform: a panel of the padding

    sp_stage<NW>(L, bits, g, N, n, tid);
    const rsrc_t y_r = make_rsrc(yg, (long long)CP * pieces * 16);
    const int ldp2 = pieces * 16;               // bytes per channel
    const bool odd = j & 1;
    sp_powers<NW>(L, n, i0, n_powers, tid, [&](int p, int jb, const f32x16 &f) {
        const int c0 = (32 * jb + j) & ~1;      // the even column of the lane pair
        const int coff = c0 < N8 ? c0 * 2 : OOB_OFF;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            // both registers of the pair cross over (a select between f[2q] and f[2q + 1] on the lane's parity becomes a dynamic
            // index into the fragment: a 16-deep select chain per access)
            const float n0 = dpp_mov<0xB1>(f[2 * q]), n1 = dpp_mov<0xB1>(f[2 * q + 1]);     // the neighbour's rows 2q, 2q + 1
            const unsigned even_row = cvt_pk(f[2 * q], n0);          // even lane: columns (j, j + 1) of row ch_of(2q, h)
            const unsigned odd_row = cvt_pk(n1, f[2 * q + 1]);       // odd lane: columns (j - 1, j) of row ch_of(2q + 1, h)
            const int i = i0 + ch_of(2 * q, h) + (odd ? 1 : 0);
            __builtin_amdgcn_raw_buffer_store_b32(odd ? odd_row : even_row, y_r, (i < N && c0 < N8) ? coff + i * ldr * 2 : OOB_OFF,
                                                  p * ldp2, 0);
        }
    });
}

template <int NW>
int launch(const unsigned *bits, const int *nvalid, int G, int N, int n_powers, int CP, int ldr, void *y, long long ldp, hipStream_t st) {
    const int panels = (N + SP_ROWS - 1) / SP_ROWS;
    hipLaunchKernelGGL((spectral_slab_kernel<NW>), dim3(G * panels), dim3(SP_THREADS), 0, st, bits, nvalid, G, N, n_powers, CP, ldr,
                       (uint4 *)y, (int)(ldp / 8), panels);
    FGNN_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int fgnn_spectral_slab16(const unsigned *bits, const int *nvalid, int G, int N, int n_powers, int CP, int ldr, void *y,
                                    long long ldp, void *stream) {
    FGNN_CHECK(bits && y && G > 0, "fgnn_spectral_slab16: bad arguments");
    FGNN_CHECK(N >= 1 && N <= FGNN_SPECTRAL_MAX_N, "fgnn_spectral_slab16: 1 to %d vertices per graph (got %d)", FGNN_SPECTRAL_MAX_N, N);
    FGNN_CHECK(CP == 2 || CP == 32, "fgnn_spectral_slab16: the slab has 2 or 32 channels (got %d)", CP);
    FGNN_CHECK(n_powers >= 1 && n_powers <= FGNN_SPECTRAL_MAX_POWERS && n_powers <= CP,
               "fgnn_spectral_slab16: 1 to %d powers for a %d-channel slab (got %d)",
               CP < FGNN_SPECTRAL_MAX_POWERS ? CP : FGNN_SPECTRAL_MAX_POWERS, CP, n_powers);
    FGNN_CHECK(ldr >= N && ldr % 8 == 0 && ldp >= (long long)N * ldr && ldp % 64 == 0,
               "fgnn_spectral_slab16: ldr must be a multiple of 8 and >= N, ldp a multiple of 64 and >= N * ldr (N=%d ldr=%d ldp=%lld)",
               N, ldr, ldp);
    FGNN_CHECK(((unsigned long long)y & 15) == 0, "fgnn_spectral_slab16: y must be 16-byte aligned");
    FGNN_CHECK((long long)CP * ldp * 2 <= 0x7fffffffll, "fgnn_spectral_slab16: a graph's slab must stay below 2 GiB (CP=%d ldp=%lld)", CP, ldp);
    FGNN_CHECK((long long)G * ((N + SP_ROWS - 1) / SP_ROWS) <= 0x7fffffffll, "fgnn_spectral_slab16: too many graphs (%d)", G);
    hipStream_t st = (hipStream_t)stream;
    if (N <= 32) return launch<1>(bits, nvalid, G, N, n_powers, CP, ldr, y, ldp, st);
    if (N <= 64) return launch<2>(bits, nvalid, G, N, n_powers, CP, ldr, y, ldp, st);
    if (N <= 128) return launch<4>(bits, nvalid, G, N, n_powers, CP, ldr, y, ldp, st);
    return launch<8>(bits, nvalid, G, N, n_powers, CP, ldr, y, ldp, st);
}
