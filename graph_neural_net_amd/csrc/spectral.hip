// The spectral input of the reference's second dataset class (loaders/data_generator.py:221-232, QAP_spectralGenerator): per graph
// the powers L, L^2, ..., L^P of L = D^-1/2 W D^-1/2 as P fp32 channels, straight from the bit rows of the engine's wire format.
//
//     d_i = sum_j w_ij  (row sum of the valid n x n corner; bits outside it are masked, not trusted)
//     s_i = 1 / sqrt(d_i)  in fp32 (IEEE sqrt and division), and s_i = 0 where d_i = 0  -- the ONE deviation: the reference computes
//           inf * 0 = NaN for an isolated vertex and every later power is NaN in every entry; here its row and column are zeros
//     F_1[i][j] = (s_i w_ij) s_j                      one correctly rounded product: bit-exact against the reference
//     F_{p+1}[i][j] = s_j sum_k (F_p[i][k] s_k) w_kj   = (F_p @ L)[i][j], the reference's left-to-right chain, in fp32
//
// Row i of F_{p+1} depends on row i of F_p only, so a workgroup owns a 32-row panel of one graph through all powers and nothing but
// the results goes to HBM.  L is never materialised: the panel is kept in LDS already scaled by s_k (the A operand of
// v_mfma_f32_32x32x2_f32), the B operand of k-step (k, k + 1) is the 0/1 bit w_kj that lane (j = l & 31, h = l >> 5) extracts from
// word j / 32 of ROW k + h of W -- the operand layout wants W by rows, so no transpose is built and nothing assumes W symmetric --
// and the result column is scaled by s_j.  The four waves split the 32-column blocks (wave w: blocks w and w + 4).  The next power's
// panel is written from the accumulators after a barrier, so ONE panel in LDS is enough (the accumulators are the second buffer):
// 42 KB at N = 256.  The D fragment has the column on the lane, so each store instruction writes two 128-byte row segments.
// Loads and stores go through per-graph buffer descriptors: lanes outside the tensors take an out-of-range offset.
#include "fgnn_spectral.h"      // the panel code, shared with spectral_slab.hip

namespace {

// grid: G * ceil(Nout / 32) workgroups, workgroup b = (graph b / panels, panel b % panels).  NW = words per staged row (N <= 32 NW).
template <int NW>
__global__ __launch_bounds__(SP_THREADS) void spectral_kernel(const unsigned *bits, const int *nvalid, int G, int N, int n_powers,
                                                              float *out, int Nout, int panels) {
    __shared__ SpLds<NW> L;
    const int g = blockIdx.x / panels, i0 = (blockIdx.x - g * panels) * SP_ROWS, tid = threadIdx.x;
    const int lane = tid & 63, j = lane & 31, h = lane >> 5;
    const int n = sp_nvalid(nvalid, G, g, N);
    const long long plane = (long long)Nout * Nout;
    const rsrc_t out_r = make_rsrc(out + (long long)g * n_powers * plane, (long long)n_powers * plane * 4);
    const int plane4 = (int)plane * 4;

    if (i0 >= n) {                              // uniform: a panel of the padding is zeros in every power
        const int off = (tid < Nout) ? tid * 4 : OOB_OFF;
        for (int p = 0; p < n_powers; ++p)
            for (int r = 0; r < SP_ROWS; ++r)
                __builtin_amdgcn_raw_buffer_store_b32(0u, out_r, (i0 + r < Nout) ? off + (i0 + r) * Nout * 4 : OOB_OFF, p * plane4, 0);
        return;
    }
    sp_stage<NW>(L, bits, g, N, n, tid);
    // F_p -> HBM (column blocks up to Nout; zeros where the block is past the corner)
    sp_powers<NW>(L, n, i0, n_powers, tid, [&](int p, int jb, const f32x16 &f) {
        const int col = 32 * jb + j;
        const int off = col < Nout ? col * 4 : OOB_OFF;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = i0 + ch_of(r, h);
            const float v = f[r];               // (a copy: __builtin_bit_cast applied to the vector element itself reads element 0)
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), out_r, i < Nout ? off + i * Nout * 4 : OOB_OFF,
                                                  p * plane4, 0);
        }
    });
}

template <int NW>
int launch(const unsigned *bits, const int *nvalid, int G, int N, int n_powers, float *out, int Nout, hipStream_t st) {
    const int panels = (Nout + SP_ROWS - 1) / SP_ROWS;
    hipLaunchKernelGGL((spectral_kernel<NW>), dim3(G * panels), dim3(SP_THREADS), 0, st, bits, nvalid, G, N, n_powers, out, Nout, panels);
    FGNN_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int fgnn_spectral_features(const unsigned *bits, const int *nvalid, int G, int N, int n_powers, float *out, int Nout,
                                      void *stream) {
    FGNN_CHECK(bits && out && G > 0, "fgnn_spectral_features: bad arguments");
    FGNN_CHECK(N >= 1 && N <= FGNN_SPECTRAL_MAX_N, "fgnn_spectral_features: 1 to %d vertices per graph (got %d)", FGNN_SPECTRAL_MAX_N, N);
    FGNN_CHECK(n_powers >= 1 && n_powers <= FGNN_SPECTRAL_MAX_POWERS, "fgnn_spectral_features: 1 to %d powers (got %d)",
               FGNN_SPECTRAL_MAX_POWERS, n_powers);
    FGNN_CHECK(Nout >= 1 && Nout <= N, "fgnn_spectral_features: the output size must be in [1, N = %d] (got %d)", N, Nout);
    FGNN_CHECK((long long)G * ((Nout + SP_ROWS - 1) / SP_ROWS) <= 0x7fffffffll, "fgnn_spectral_features: too many graphs (%d)", G);
    hipStream_t st = (hipStream_t)stream;
    if (N <= 32) return launch<1>(bits, nvalid, G, N, n_powers, out, Nout, st);
    if (N <= 64) return launch<2>(bits, nvalid, G, N, n_powers, out, Nout, st);
    if (N <= 128) return launch<4>(bits, nvalid, G, N, n_powers, out, Nout, st);
    return launch<8>(bits, nvalid, G, N, n_powers, out, Nout, st);
}
