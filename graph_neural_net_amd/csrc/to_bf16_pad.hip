// fp32 (G, c, N, N) input, 1 <= c <= CP  ->  the bf16 slab block 1 of the bf16 engine reads, in ONE pass (gfx950): CP = 2 or 32
// channels (the caller's slab width, the engine's layout.c0) with the engine's pitches (gstride = CP * ldp, ldp, ldr).  Channels < c: round-to-nearest-even of the
// input inside the graph's n_g x n_g corner; everything else of the slab -- channels >= c, the ragged padding, the pitch columns
// N <= j < ldr and the tail of every channel up to ldp -- exact +0.  Replaces "zero-padded fp32 staging buffer + fgnn_to_bf16":
// 4c + 2 CP bytes per pixel instead of 4c + 4*32 (staging write) + 4*32 (its read) + 2*32.
//
// One thread per 16-byte piece (eight elements) of the output: ldr is a multiple of 8 and ldp of 64, so a piece lies inside one
// row of one channel and every store is one aligned 16-byte vector store; every output element has exactly one writer (no
// atomics, no LDS, nothing to order: capturable).  The eight inputs of a piece come as two 16-byte loads where the row pitch
// keeps them aligned (`vec`: N % 4 == 0 and a 16-byte aligned x) and the piece half lies inside the corner, as scalar loads of
// the valid columns otherwise: nothing outside the corner is read (it may hold anything, NaN included).
#include "fgnn_bf16.h"

namespace {

__global__ __launch_bounds__(256) void to_bf16_pad_kernel(const float *__restrict__ x, const int *__restrict__ nvalid, int c, int CP,
                                                          int N, int ldr, uint4 *__restrict__ y, int pieces, long long total, int vec) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const long long gc = t / pieces;                     // (g, ch) of the OUTPUT slab; consecutive channels are ldp apart
    const int q = (int)(t - gc * pieces);
    const int g = (int)(gc / CP), ch = (int)(gc - (long long)g * CP);
    const int p = 8 * q, i = p / ldr, j0 = p - i * ldr;         // (8 * pieces = ldp < 2^31: checked by the launcher)
    const int nv = min(max(nvalid_of(nvalid, g, N), 0), N);
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0.f;
    if (ch < c && i < nv && j0 < nv) {                   // (i < nv <= N also keeps the channel tail p >= N * ldr out)
        const float *src = x + ((long long)g * c + ch) * N * N + (long long)i * N + j0;
#pragma unroll
        for (int hlf = 0; hlf < 2; ++hlf) {
            const int j = j0 + 4 * hlf;
            if (vec && j + 4 <= nv) {
                const float4 f = *reinterpret_cast<const float4 *>(src + 4 * hlf);
                v[4 * hlf] = f.x;
                v[4 * hlf + 1] = f.y;
                v[4 * hlf + 2] = f.z;
                v[4 * hlf + 3] = f.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (j + e < nv) v[4 * hlf + e] = src[4 * hlf + e];
            }
        }
    }
    uint4 o;
    o.x = cvt_pk(v[0], v[1]);
    o.y = cvt_pk(v[2], v[3]);
    o.z = cvt_pk(v[4], v[5]);
    o.w = cvt_pk(v[6], v[7]);
    y[t] = o;                                            // piece t of the slab: (gc * ldp + 8 q) elements from its base
}

}  // namespace

extern "C" int fgnn_to_bf16_pad(const float *x, const int *nvalid, int G, int c, int CP, int N, int ldr, void *y, long long ldp,
                                void *stream) {
    FGNN_CHECK(x && y && G > 0 && N > 0, "fgnn_to_bf16_pad: bad arguments");
    FGNN_CHECK(CP == 2 || CP == 32, "fgnn_to_bf16_pad: the slab has 2 or 32 channels (got %d)", CP);
    FGNN_CHECK(c >= 1 && c <= CP, "fgnn_to_bf16_pad: 1 <= c <= %d input channels for a %d-channel slab (got %d)", CP, CP, c);
    FGNN_CHECK(ldr >= N && ldr % 8 == 0 && ldp >= (long long)N * ldr && ldp % 64 == 0,
               "fgnn_to_bf16_pad: ldr must be a multiple of 8 and >= N, ldp a multiple of 64 and >= N * ldr (N=%d ldr=%d ldp=%lld)", N, ldr, ldp);
    FGNN_CHECK(((unsigned long long)y & 15) == 0, "fgnn_to_bf16_pad: y must be 16-byte aligned");
    const int vec = (N % 4 == 0 && ((unsigned long long)x & 15) == 0) ? 1 : 0;      // then every (i * N + j0) * 4 bytes is a multiple of 16
    FGNN_CHECK(ldp < (1ll << 31), "fgnn_to_bf16_pad: channel stride too large (ldp < 2^31)");
    const int pieces = (int)(ldp / 8);
    const long long total = (long long)G * CP * pieces;
    const long long blocks = (total + 255) / 256;
    FGNN_CHECK(blocks < (1ll << 31), "fgnn_to_bf16_pad: too many pieces; split the batch");
    hipLaunchKernelGGL(to_bf16_pad_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, nvalid, c, CP, N, ldr,
                       (uint4 *)y, pieces, total, vec);
    FGNN_LAUNCH_CHECK();
    return 0;
}
