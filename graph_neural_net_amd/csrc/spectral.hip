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
#include "fgnn_common.h"

namespace {

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

// grid: G * ceil(Nout / 32) workgroups, workgroup b = (graph b / panels, panel b % panels).  NW = words per staged row (N <= 32 NW).
template <int NW>
__global__ __launch_bounds__(SP_THREADS) void spectral_kernel(const unsigned *bits, const int *nvalid, int G, int N, int n_powers,
                                                              float *out, int Nout, int panels) {
    constexpr int NP = 32 * NW, P = NP + 1, NACC = NW > 4 ? 2 : 1;       // P odd: the 32 rows a half-wave reads at one k are 32 banks
    __shared__ unsigned wl[NP * NW];           // rows of W, zero outside the corner
    __shared__ float sl[NP];                   // s_k, zero for k >= n and for isolated vertices
    __shared__ float panel[SP_ROWS * P];       // F_p[i0 + i][k] s_k
    const int g = blockIdx.x / panels, i0 = (blockIdx.x - g * panels) * SP_ROWS, tid = threadIdx.x;
    const int wv = tid >> 6, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const int W = (N + 31) >> 5;
    const rsrc_t nv_r = make_rsrc(nvalid, nvalid ? (long long)G * 4 : 0);
    const int nv = __builtin_amdgcn_raw_buffer_load_b32(nv_r, 0, g * 4, 0);
    const int n = nvalid ? min(max(nv, 0), N) : N;
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

    // ---- stage W (masked to the corner) and s
    {
        const rsrc_t bits_r = make_rsrc(bits + (long long)g * N * W, (long long)N * W * 4);
        int deg = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const unsigned v = (unsigned)__builtin_amdgcn_raw_buffer_load_b32(bits_r, (tid < N && w < W) ? (tid * W + w) * 4 : OOB_OFF, 0, 0)
                               & (tid < n ? corner_mask(w, n) : 0u);
            if (tid < NP) wl[tid * NW + w] = v;
            deg += __popc(v);
        }
        if (tid < NP) sl[tid] = deg > 0 ? 1.0f / __builtin_sqrtf((float)deg) : 0.0f;
    }
    __syncthreads();

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
        // F_p = acc s_j -> HBM (column blocks up to Nout; zeros where the block is past the corner); acc <- F_p s_j, the next A operand
#pragma unroll
        for (int a = 0; a < NACC; ++a) {
            const int col = 32 * jb[a] + j;
            const int off = col < Nout ? col * 4 : OOB_OFF;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = i0 + ch_of(r, h);
                const float v = acc[a][r] * sj[a];
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), out_r, i < Nout ? off + i * Nout * 4 : OOB_OFF,
                                                      p * plane4, 0);
                acc[a][r] = v * sj[a];
            }
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
