/*
 * fgnn_hip.h -- C ABI of libfgnn_hip.so, the MI355X (gfx950) implementation of the
 * 2-FGNN hot path of mlelarge/graph_neural_net.
 *
 * The reference has no FFI: its boundary is the Python nn.Module surface
 * (models/layers.py, models/blocks_emb.py, maskedtensors/maskedtensor.py).  Each entry
 * point below names the reference code (file:line under /root/reference) whose
 * arithmetic it replaces; graph_neural_net_amd/ (Python) binds them with ctypes and
 * re-exposes the reference's module names on top.
 *
 * Conventions
 *   - all pointers are DEVICE pointers (HBM), fp32 unless stated, owned by the caller;
 *   - activations are channel-first: element (g, c, i, j) of a (G, C, N, N) tensor lives at
 *     ptr[g*gstride + c*ldp + i*N + j]; ldp >= N*N is the channel stride (the Python host
 *     uses ldp = N*N for user-visible tensors and a 32-float-aligned ldp internally);
 *   - `nvalid` (optional, int32[G]) is the per-graph vertex count of a ragged batch
 *     (MaskedTensor masks, maskedtensor.py:8-48); NULL means every graph has N vertices.
 *     Entries with i >= nvalid[g] or j >= nvalid[g] are padding: read as 0, written as 0,
 *     excluded from every statistic (maskedtensor.py:87-112, 310-335);
 *   - `stream` is a hipStream_t passed as void*; every call only enqueues work on it;
 *   - return value 0 = success; non-zero = error, message via fgnn_last_error().
 *     Unsupported shapes are errors, never a silent fallback.
 *   - hidden/output width of the MLP kernels is FGNN_H = 32 channels (the reference's
 *     in_features = out_features = 32, default_config.yaml:47-57).
 */
#ifndef FGNN_HIP_H
#define FGNN_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define FGNN_H 32            /* hidden / output channels of every MLP kernel          */
#define FGNN_TILE 32         /* pixels per statistics tile                             */
#define FGNN_MAX_DEPTH 3     /* convs per MlpBlock_Real handled by the fused kernels  */

/* One input slab of an MLP: C channels, optionally the *pre-norm* output `z` of an
 * earlier MLP kernel together with that MLP's GraphNorm record, in which case the
 * consumer applies y = (z - mean) * a + beta on load (models/layers.py:68-80). */
typedef struct {
    const float *ptr;        /* (G, C, ldp)                                            */
    long long gstride;       /* floats between graphs                                  */
    long long ldp;           /* floats between channels                                */
    int C;                   /* channels (even; 0 = slab unused)                       */
    const float *nrm;        /* optional (G*C*4): {mean, a, q, r2} per (g,c)           */
    const float *beta;       /* optional (C): GraphNorm bias                           */
} fgnn_slab;

/* ---- library ---------------------------------------------------------------------- */
const char *fgnn_last_error(void);
int fgnn_version(void);
/* number of statistics tiles per graph for N vertices: ceil(N*N / FGNN_TILE) */
int fgnn_tiles_per_graph(int N);
/* workgroups the persistent MLP kernels launch (partials buffers are sized by it) */
int fgnn_mlp_bwd_num_workgroups(void);

/* ---- LDS operand images ------------------------------------------------------------------
 * The MLP kernels keep their MFMA A-operands (weights, biases, transposed weights) in LDS.
 * Weights are constant within a step, so the images of all MLP launches can be packed ONCE
 * per step by one small launch and are then copied straight into LDS by every workgroup.
 * kind 0 = forward image (nmlp MLPs), kind 1 = backward image (one MLP; uses W[0], bias[0]);
 * kind 5 = the backward image in the layout of the 16-pixel-tile kernels (fgnn_mlp_bwd_*t16; padded to whole KiB). */
#define FGNN_MAX_PACK_JOBS 24
typedef struct {
    int kind, ca, cb, depth, nmlp;
    const float *W[2][FGNN_MAX_DEPTH];
    const float *bias[2][FGNN_MAX_DEPTH];
    float *out;                              /* fgnn_pack_floats(kind, ca, cb, depth, nmlp) floats */
} fgnn_pack_job;
int fgnn_pack_floats(int kind, int ca, int cb, int depth, int nmlp);
int fgnn_pack_operands(const fgnn_pack_job *jobs, int njobs, void *stream);

/* ---- MlpBlock_Real.forward minus the final normalisation ---------------------------
 * replaces models/layers.py:126-131 (conv1x1+ReLU chain, last conv without ReLU) and the
 * reductions of normalize (:72-73).  Computes, for nmlp (1 or 2) MLPs sharing one input
 *   z_m = W_m[d-1] relu(... relu(W_m[0] x + b_m[0]) ...) + b_m[d-1]      (G, 32, ldz)
 * with x = [slab a ; slab b] on channels (Concat, layers.py:145-146, never materialised),
 * and per (graph, tile, channel) partial statistics {mean, M2} of z over valid pixels.  */
typedef struct {
    int G, N, depth, nmlp;
    const int *nvalid;
    fgnn_slab a, b;
    const float *W[2][FGNN_MAX_DEPTH];      /* conv weights (32, Cin_l) row-major       */
    const float *bias[2][FGNN_MAX_DEPTH];   /* conv biases (32)                          */
    float *z[2];                            /* out (G, 32, ldz)                          */
    long long ldz;
    float *part[2];                         /* out (G, tpg, 32, 2) {mean, M2}            */
    float *cnt;                             /* out (G, tpg) valid pixels per tile        */
    const float *packed;                    /* optional: operand image from fgnn_pack_operands
                                               (kind 0) for exactly these weights; NULL = the kernel
                                               builds it itself (slower prologue)              */
    const unsigned *xbits;                  /* optional: the 2-channel slab (a when a.C == 2, else b when b.C == 2) is not read
                                               from its ptr but expanded on the fly from the bit-packed adjacency
                                               (G, N, ceil(N/32)) words, bit j of row i = W[i][j]: channel 0 = W, channel 1 =
                                               diag(xdeg) (loaders/data_generator.py:118-125); the slab need not exist */
    const float *xdeg;                      /* (G, N) row sums over the valid columns, from fgnn_adjacency_degree */
    const int *ranges;                      /* optional, ragged batches (nvalid != NULL): FGNN_RANGE_WG + 1 tile bounds from
                                               fgnn_ragged_tile_ranges.  Workgroup w then owns tiles [ranges[w], ranges[w+1])
                                               (equal WORK instead of equal tile counts) and tiles that lie entirely in the
                                               padding are stepped over: their statistics records are written as empty, their
                                               z pixels are left untouched (consumers must do the same, or read the valid
                                               n x n corner only -- all kernels of this library do) */
    int cu_share;                           /* 0 / 1: the whole GPU (up to 256 persistent workgroups).  2: HALF of the CUs (at most 128
                                               workgroups): two launches on different streams -- independent half-batches, see
                                               engine_dual.py -- run side by side on disjoint CUs, one chain's ramps under the
                                               other's streaming.  Results do not depend on it.  IGNORED when `ranges` is given:
                                               the range table has one entry per workgroup of the full grid, so a ragged launch
                                               always runs FGNN_RANGE_WG workgroups */
} fgnn_mlp_fwd_args;
int fgnn_mlp_fwd(const fgnn_mlp_fwd_args *args, void *stream);

/* ---- the same two MLP entry points on the bf16 matrix cores ("x3": csrc/fgnn_x3.h) ------------------------------
 * replaces the same reference lines as fgnn_mlp_fwd / fgnn_mlp_bwd (models/layers.py:126-131 and its autograd).  Tensors,
 * argument structs, tile statistics and results are those of the fp32-MFMA kernels (same parity gates); inside, every fp32
 * operand of a channel contraction is split exactly into three bf16 numbers and the product is accumulated in fp32 from
 * the six partial products >= 2^-16 (error < 3 * 2^-24 |a b| per product, the size of an fp32 rounding).  Built for
 * depth 3, slabs of 2 / 32 / 32+2 / 32+32 channels and constant-size batches (no `ranges`); `packed` is mandatory and
 * comes from fgnn_pack_x3_operands (same job struct as fgnn_pack_operands, fgnn_pack_x3_floats floats per image; jobs of
 * kind 2 / 3 produce the fp32 images of fgnn_pack_operands kind 0 / 1 in the same launch, for steps that mix both kernel sets). */
int fgnn_pack_x3_floats(int kind, int ca, int cb, int depth, int nmlp);
int fgnn_pack_x3_operands(const fgnn_pack_job *jobs, int njobs, void *stream);
int fgnn_mlp_fwd_x3(const fgnn_mlp_fwd_args *args, void *stream);

/* ---- GraphNorm statistics ------------------------------------------------------------
 * replaces torch.mean / torch.var(unbiased=False) over (N,N) and the scale of normalize
 * (models/layers.py:71-80) incl. the ragged n = sum(mask) (:79).  Combines the tile
 * partials (two fixed-order wave sums: grand mean, then M2 + m (mean_t - mean)^2) into nrm[g,c] = {mean, a, q, r2} with
 *   var = M2/m, r2 = 1/(var+eps), q = 1/(2 sqrt(n (var+eps))), a = gn_weight[c] * q.     */
int fgnn_gn_finalize(const float *part, const float *cnt, const float *gn_weight /* (C) or NULL=1 */,
                     const int *nvalid, int G, int C, int N, float eps, float *nrm, void *stream);
/* two MLPs (sharing cnt, e.g. mlp1 / mlp2 of one fgnn_mlp_fwd call) in one launch */
int fgnn_gn_finalize2(const float *part0, const float *part1, const float *cnt, const float *gn_weight0,
                      const float *gn_weight1, const int *nvalid, int G, int C, int N, float eps,
                      float *nrm0, float *nrm1, void *stream);
/* same record computed directly from a dense (G, C, ldp) tensor (two-pass), any C */
int fgnn_gn_stats(const float *x, long long gstride, long long ldp, const float *gn_weight,
                  const int *nvalid, int G, int C, int N, float eps, float *nrm, void *stream);
/* y = (z - mean) * a + beta on valid entries, 0 on padding (GraphNorm.forward, :68-69) */
int fgnn_gn_apply(const float *z, long long zgstride, long long ldz, const float *nrm, const float *beta /* (C) or NULL=0 */,
                  const int *nvalid, int G, int C, int N, float *y, long long ygstride, long long ldy, void *stream);

/* GraphNorm.forward (models/layers.py:47-80) of a dense tensor in ONE pass and ONE launch when a plane fits a workgroup's
 * registers (N*N <= 4096): statistics record (nrm, as fgnn_gn_stats) + y = (x - mean) a + beta (as fgnn_gn_apply).
 * fgnn_gn_plane_bwd: its autograd -- S1 / S2 of the plane (written to s12), dz = ca dy + cb (z - mean) + cc, and the affine
 * gradients d gn_weight / d gn_bias (fixed order over the graphs) -- replacing fgnn_gn_bwd_stats + _coef + _apply.        */
int fgnn_gn_plane_supported(int N);
int fgnn_gn_plane_fwd(const float *x, long long gstride, long long ldp, const float *gn_weight, const float *beta /* NULL = 0 */,
                      const int *nvalid, int G, int C, int N, float eps, float *y, long long ygstride, long long ldy,
                      float *nrm /* (G*C*4) */, void *stream);
int fgnn_gn_plane_bwd(const float *dy, long long dgstride, long long ldd, const float *z, long long zgstride, long long ldz,
                      const float *nrm, const int *nvalid, int G, int C, int N, float *dz, long long ogstride, long long ldo,
                      float *s12 /* (G*C*2) */, float *dgn_w /* (C) or NULL */, float *dgn_b /* (C) or NULL */, void *stream);

/* ---- generic-width 1x1 convolution (conv.hip) ------------------------------------------
 * One layer of MlpBlock_Real.forward, `out = activation(conv_layer(out))` (models/layers.py:125-131: nn.Conv2d(k=1, bias=True)
 * + F.relu), for channel widths the fused 32-wide fgnn_mlp_fwd / fgnn_mlp_bwd are not built for (any Cin = K and Cout = M up
 * to FGNN_CONV_MAX_CH).  fp32, exact fma chain over the input channels.
 *   y[g][o][p] = act( bias[o] + sum_k W[o*w_ostride + k*w_kstride] * xm[g][k][p] ),  act = ReLU when `relu`, else identity;
 *   xm = x where relu_mask > 0 (same strides as x) or x itself when relu_mask == NULL.  Pixels outside the valid n x n corner of
 *   a ragged graph (nvalid) are written as 0.
 * The same entry point gives the input gradient of a layer: x := dy, relu_mask := the layer's saved (post-ReLU) output,
 * W strides swapped (W^T), bias NULL, relu 0.                                                                            */
#define FGNN_CONV_MAX_CH 256
int fgnn_conv1x1(const float *x, long long x_gstride, long long x_ld, const float *relu_mask, const float *W,
                 long long w_ostride, long long w_kstride, const float *bias, int relu, const int *nvalid, int G, int N,
                 int M, int K, float *y, long long y_gstride, long long y_ld, void *stream);
/* Parameter gradients of one layer: with dz = dy where relu_mask > 0 (all of dy when NULL), restricted to valid pixels,
 *   dW[o][c] = sum_{g,p} dz[g][o][p] * x[g][c][p],  db[o] = sum_{g,p} dz[g][o][p]
 * as fgnn_conv1x1_dw_chunks(G, N) partial records of M*K + M floats ([dW (M,K) | db (M)]) in `wpart`; finish with
 * fgnn_reduce_partials(wpart, chunks, M*K + M, out) (fixed order: bit-reproducible).                                    */
int fgnn_conv1x1_dw_chunks(int G, int N);
int fgnn_conv1x1_dw(const float *dy, long long d_gstride, long long d_ld, const float *relu_mask, const float *x,
                    long long x_gstride, long long x_ld, const int *nvalid, int G, int N, int M, int K, float *wpart,
                    void *stream);

/* the same for up to FGNN_DW_MAX_JOBS layers in one launch (the convs of one MlpBlock_Real): a chunk's partial record is the
 * concatenation of the jobs' records [dW_0 | db_0 | dW_1 | db_1 | ...], so one fgnn_reduce_partials(wpart, chunks, sum of the
 * counts, out) finishes all of them */
#define FGNN_DW_MAX_JOBS 4
typedef struct {
    const float *dy; long long d_gstride, d_ld;
    const float *relu_mask;                 /* optional */
    const float *x; long long x_gstride, x_ld;
    int M, K;
} fgnn_dw_job;
int fgnn_conv1x1_dw_multi(const fgnn_dw_job *jobs, int njobs, const int *nvalid, int G, int N, float *wpart, void *stream);

/* A chain of up to three 1x1 convolutions in ONE launch, the intermediate activations never leaving the register file
 * (channel widths the fused 32-wide kernels are not built for; conv.hip).  Layer l maps K_l -> M_l channels (K_{l+1} = M_l):
 *     t_l = W_l in_l + bias_l;   t_l = relu(t_l) if relu;   t_l = t_l where mask_l > 0 else 0 if mask_l;   out_l = t_l
 * in_0 = x, in_{l+1} = t_l; padding pixels of ragged graphs are exact zeros in every out_l.  Two uses:
 *   forward of MlpBlock_Real's conv stack (models/layers.py:125-131): relu on all but the last layer, every out_l kept for
 *     the backward;
 *   its input-gradient chain: layers in reverse with W^T given by strides, no bias, mask_l = the saved post-ReLU activation
 *     the gradient flows into, out_l = d(pre-activation) of that layer (what fgnn_conv1x1_dw then takes with relu_mask = NULL).
 * Limits (fgnn_conv_chain_supported): depth <= 3, K_0 <= 128, every M_l <= 128, hidden widths (M_l, l < depth-1) <= 64.   */
typedef struct {
    const float *W;                         /* element (o, k) at W[o * w_ostride + k * w_kstride]                        */
    long long w_ostride, w_kstride;
    const float *bias;                      /* (M) or NULL                                                               */
    int M, K;
    int relu;
    const float *mask;                      /* optional (G, M, N*N) with the strides of `out`                            */
    float *out;                             /* optional (G, M, N*N)                                                      */
    long long o_gstride;                    /* graph stride of mask / out (their channel stride is fgnn_chain_args.o_ld)   */
} fgnn_chain_layer;
typedef struct {
    const float *x;
    long long x_gstride, x_ld;
    int depth;
    fgnn_chain_layer layer[3];
    long long o_ld;                         /* channel stride of every layer's mask / out                                */
    const int *nvalid;
    int G, N;
} fgnn_chain_args;
int fgnn_conv_chain_supported(int depth, int K0, const int *M /* depth widths */);
int fgnn_conv_chain(const fgnn_chain_args *args, void *stream);

/* ---- the conv stack of a 64-wide MlpBlock_Real, fused (csrc/mlp64.hip; models/layers.py:113-131 with out_features = 64, depth_of_mlp = 3:
 * the three MLPs of a 64-feature block, models/blocks_emb.py:16-36) -------------------------------------------------------------------
 *   forward   out = W2 relu(W1 relu(W0 x + b0) + b1) + b2  (zeros outside the valid corner); nothing else is written;
 *   backward  recomputes the hidden activations from x, then dx (optional) and one row of parameter-gradient partials per workgroup:
 *             wpart[wg][fgnn_mlp64_param_count(cin)] = [dW0 (64 x K0P, K0P = cin rounded up to 32: columns >= cin are zero) | db0 (64) |
 *             dW1 (64 x 64) | db1 | dW2 | db2]; fgnn_reduce_partials(wpart, fgnn_mlp64_num_workgroups(), count, ...) sums the rows.
 * fgnn_mlp64_pack turns the nn.Conv2d parameters (W0 (64, cin), W1, W2 (64, 64) row-major; biases (64) or NULL) into the operand record
 * both directions read (MFMA operand order, forward and transposed images; one small launch per forward call).  16-pixel tiles on
 * v_mfma_f32_16x16x4_f32; the backward keeps a wave's whole parameter-gradient set in its (AGPR) registers, one wave per SIMD.
 * fgnn_mlp64_supported: depth 3, width 64, cin in 1..128; N <= 256. */
typedef struct {
    const float *x;                          /* (G, cin, N*N) */
    long long x_gstride, x_ld;
    int cin;
    const float *xb;                         /* optional second slab (G, cb, N*N) stacked after x along the channels (mlp3 of a block reads  */
    long long xb_gstride, xb_ld;             /* [mult ; in] without the concatenated copy): cin == 64 then, cb <= 64, W0 is                   */
    int cb;                                  /* (64, cin + cb); NULL: one slab                                                               */
    const float *packed;                     /* fgnn_mlp64_packed_floats(cin) floats written by fgnn_mlp64_pack */
    const int *nvalid;                       /* (G) or NULL */
    int G, N;
    float *out;                              /* forward: (G, 64, N*N) */
    long long o_gstride, o_ld;
    const float *dz;                         /* backward: gradient of out */
    long long dz_gstride, dz_ld;
    float *dx;                               /* backward: (G, cin, N*N) or NULL */
    long long dx_gstride, dx_ld;
    float *dxb;                              /* backward, two slabs: (G, cb, N*N), required when dx is given */
    long long dxb_gstride, dxb_ld;
    int accumulate_dx, accumulate_dxb;       /* != 0: dx (dxb) += instead of a store (the input also feeds other MLPs: their launches add to one buffer) */
    float *wpart;                            /* backward: (fgnn_mlp64_num_workgroups(), fgnn_mlp64_param_count(cin)) */
} fgnn_mlp64_args;
int fgnn_mlp64_supported(int cin, int depth, int width);
int fgnn_mlp64_num_workgroups(void);
int fgnn_mlp64_param_count(int cin);
int fgnn_mlp64_packed_floats(int cin);
int fgnn_mlp64_pack(const float *W0, const float *W1, const float *W2, const float *b0, const float *b1, const float *b2, int cin,
                    float *packed, void *stream);
typedef struct {
    const float *W[3];                       /* W0 (64, cin), W1, W2 (64, 64) */
    const float *bias[3];                    /* (64) or NULL */
    int cin;
    float *packed;                           /* fgnn_mlp64_packed_floats(cin) floats */
} fgnn_mlp64_pack_job;
/* ... for up to 16 MLPs in one launch (every MLP of a model at the top of its forward pass) */
int fgnn_mlp64_pack_multi(const fgnn_mlp64_pack_job *jobs, int njobs, void *stream);
int fgnn_mlp64_fwd(const fgnn_mlp64_args *args, void *stream);
int fgnn_mlp64_bwd(const fgnn_mlp64_args *args, void *stream);

/* ---- Matmul.forward: per (g,c) N x N product (models/layers.py:161-162) --------------
 * out[g,c] = Ya[g,c] @ Yb[g,c], Y = normalised slab (or the raw slab when nrm == NULL). */
int fgnn_chan_matmul_fwd(const fgnn_slab *ya, const fgnn_slab *yb, const int *nvalid, int G, int N,
                         float *out, long long ogstride, long long ldo, void *stream);
/* Ragged batches (64 < N <= 256, one workgroup per matrix): the same product with the workgroups issued in the order of
 * `order` (G graph indices from fgnn_ragged_tile_ranges_order: largest graph first), so that the hardware's in-order
 * dispatch is a longest-job-first schedule -- the matrices of a batch differ by up to (Nmax / nmin)^3 in work.  Results
 * do not depend on the order (every matrix is computed by one workgroup on its own).  order == NULL: as above.          */
/* fill: what the kernel zeroes of the output outside the valid corner (64 < N <= 256).  0: all of it.  1: only what a consumer
 * that steps over padding-only tiles (fgnn_ragged_tile_ranges) can read -- the row tails of the valid rows up to the next multiple
 * of 32 columns and the head of the row after the last one; the rest of the frame is left as it was.                              */
int fgnn_chan_matmul_fwd_ord(const fgnn_slab *ya, const fgnn_slab *yb, const int *nvalid, int G, int N,
                             float *out, long long ogstride, long long ldo, const int *order, int fill, void *stream);
/* The same product with the work of fgnn_gn_finalize2 folded into its prologue (one workgroup or wave per matrix: N <= 256):
 * each (g,c) workgroup finalizes the two GraphNorm records it needs from the tile statistics (part_a / part_b /
 * cnt of the preceding two-MLP fgnn_mlp_fwd call) while its tile loads are in flight, normalises with them and
 * writes them to ya->nrm / yb->nrm for the later consumers -- one launch less per block.                     */
int fgnn_chan_matmul_fwd_fin_supported(int N);
int fgnn_chan_matmul_fwd_fin(const fgnn_slab *ya, const fgnn_slab *yb, const float *part_a, const float *part_b,
                             const float *cnt, const float *gn_weight_a, const float *gn_weight_b, float eps,
                             const int *nvalid, int G, int N, float *out, long long ogstride, long long ldo, void *stream);
int fgnn_chan_matmul_fwd_fin_ord(const fgnn_slab *ya, const fgnn_slab *yb, const float *part_a, const float *part_b,
                                 const float *cnt, const float *gn_weight_a, const float *gn_weight_b, float eps,
                                 const int *nvalid, int G, int N, float *out, long long ogstride, long long ldo,
                                 const int *order /* as fgnn_chan_matmul_fwd_ord; used for 64 < N <= 256 */, int fill, void *stream);

/* ---- ColumnMaxPooling.forward (models/layers.py:202-203; masked: maskedtensor.py:213-228)
 * e[g,c,i] = max_j y[g,c,i,j] (first index on ties), idx int32; rows i >= nvalid -> 0.   */
int fgnn_colmax_fwd(const fgnn_slab *y, const int *nvalid, int G, int N, float *e /* (G,C,N) */,
                    int *idx /* (G,C,N) */, void *stream);
/* the same with the GraphNorm finalize of its input folded in (N <= 64): every (g,c) wave combines the tile
 * statistics (part, cnt of the fgnn_mlp_fwd call that produced y) itself and writes the record to y->nrm */
int fgnn_colmax_fwd_fin_supported(int N);
int fgnn_colmax_fwd_fin(const fgnn_slab *y, const float *part, const float *cnt, const float *gn_weight, float eps,
                        const int *nvalid, int G, int N, float *e, int *idx, void *stream);

/* ---- Siamese scoring + triplet_loss (models/trainers.py:67, toolbox/losses.py:20-34) ---
 * e1,e2: (B, C, N).  scores[b] = e1[b]^T e2[b] (B,N,N); lse (B,N) row log-sum-exp;
 * pair_loss (B * FGNN_SCORE_SPLIT): partial sums of (lse_i - scores[b,i,i]) over the valid rows of
 * FGNN_SCORE_SPLIT row blocks per pair (the loss of pair b is the sum of its FGNN_SCORE_SPLIT entries). */
#define FGNN_SCORE_SPLIT 4
int fgnn_score_ce_fwd(const float *e1, const float *e2, const int *nvalid, int B, int C, int N,
                      float *scores, float *lse, float *pair_loss, void *stream);
/* the same with `row_blocks` row blocks per pair instead of FGNN_SCORE_SPLIT (pair_loss: B * row_blocks partial sums);
 * fgnn_score_row_blocks(B, N) is the count that fills the chip for a batch of B pairs of N vertices */
int fgnn_score_row_blocks(int B, int N);
int fgnn_score_ce_fwd_blocks(const float *e1, const float *e2, const int *nvalid, int B, int C, int N, int row_blocks,
                             float *scores, float *lse, float *pair_loss, void *stream);
/* d e1, d e2 of loss = sum_b pair_loss[b] * (*gscale)   (gscale: device scalar = grad / sum n) */
int fgnn_score_ce_bwd(const float *e1, const float *e2, const float *scores, const float *lse,
                      const int *nvalid, const float *gscale, int B, int C, int N,
                      float *de1, float *de2, void *stream);

/* ---- cross-entropy against labels: the four launches above with the target of row i of pair b taken from
 * labels[b][i] (int32 (B, N), read in place; -1 in the padding, as planted.py / metrics.labels_tensor write it) instead of i:
 *   loss_b = sum over i < n_b with 0 <= t_i < n_b of (lse_i - S[i][t_i]),    dS[i][j] = (exp(S_ij - lse_i) - [j == t_i]) * gscale.
 * A live row whose label lies outside [0, n_b) has NO target (torch's ignore_index): it adds nothing to the loss, its row of dS is
 * zero and nothing is indexed with it; lse is written for every live row as before.  The normaliser of the loss stays sum n_b (the
 * reference divides by the node count, toolbox/losses.py:27-34), rows without a target included.  With labels[b][i] = i every
 * output is bit-identical to the label-less entry point: the additions keep their order, the only differences are the index of
 * the target score and the comparison j == t_i.  Geometry, form selection and LDS are those of the label-less launches (the
 * backward stages the pair's labels in N more ints of LDS).  No scratch, no atomics; single capturable launches. */
int fgnn_score_ce_fwd_blocks_labels(const float *e1, const float *e2, const int *nvalid, const int *labels, int B, int C, int N,
                                    int row_blocks, float *scores, float *lse, float *pair_loss, void *stream);
int fgnn_score_ce_bwd_labels(const float *e1, const float *e2, const float *scores, const float *lse, const int *nvalid,
                             const int *labels, const float *gscale, int B, int C, int N, float *de1, float *de2, void *stream);
int fgnn_ce_fwd_labels(const float *scores, const int *nvalid, const int *labels, int B, int N, float *lse, float *pair_loss,
                       void *stream);
int fgnn_ce_bwd_labels(const float *scores, const float *lse, const int *nvalid, const int *labels, const float *gscale, int B, int N,
                       float *dscores, void *stream);

/* ---- per-pair loss weights in the fused step: triplet_loss('mean_of_mean'), an exact short last batch, or any
 * weighting of the caller's.  pair_weight: (B,) fp32 on the device, w_b >= 0, read in place like nvalid and labels.
 *     loss_sum = sum over b with w_b != 0 of w_b * CE_b           (CE_b: the sum of the pair's row-block partials, which stay unweighted)
 *     dS_b     = w_b * gscale * (softmax_row(S_b) - target)       for w_b != 0;  exactly +0 for w_b == 0
 * w_b == 0 is a SELECT, not a multiply: the backward treats the pair as nvalid = 0 and the loss sum steps over it, so NaN or inf in
 * the scores / lse / partials of a filler pair reach neither the loss nor the gradient.  With w == 1 everywhere every output has the
 * bits of the unweighted entry point: the one new operation is gs = *gscale * w_b per workgroup, and fgnn_pair_loss_w adds in the
 * order of fgnn_sum_scale / the loss job of fgnn_grad_finalize.  No scratch, no atomics, plain vector stores; single capturable
 * launches without a host read, allocation or synchronisation.
 *
 * fgnn_score_ce_bwd_w: fgnn_score_ce_bwd (labels == NULL) or fgnn_score_ce_bwd_labels with the weights; geometry, form selection
 * and LDS are theirs (WGT instantiations of the same bodies). */
int fgnn_score_ce_bwd_w(const float *e1, const float *e2, const float *scores, const float *lse, const int *nvalid,
                        const int *labels /* may be NULL */, const float *pair_weight, const float *gscale, int B, int C, int N,
                        float *de1, float *de2, void *stream);
/* The weights of a reduction and their normaliser D, in one workgroup and a fixed order.  With n_b = nvalid[b] (NULL: N) and
 * live = *live_dev (an int32 DEVICE scalar, clamped to [0, B]; NULL: B), u_b = user[b] (NULL: 1):
 *     mode 0 ('mean'):          w_b = [b < live] * u_b,                  D = sum_{b < live} n_b * u_b
 *     mode 1 ('mean_of_mean'):  w_b = [b < live and n_b > 0] / n_b * u_b, D = sum_{b < live, n_b > 0} u_b
 * (user == NULL: D is the node count resp. the number of non-empty live pairs.)  D is summed in fp64 and written as fp32; the
 * division is IEEE.  w_out (B,), denom_out (1,). */
int fgnn_pair_weights(const int *nvalid, const int *live_dev, int mode, const float *user, int B, int N, float *w_out,
                      float *denom_out, void *stream);
/* out[0] = sum over b with w_b != 0, over the pair's row_blocks partials, of w_b * pair_loss[b * row_blocks + k]: the four-lane
 * order of fgnn_sum_scale on the same (B * row_blocks) partials (rows r = 0, 4, 8, ... / 1, 5, ... / 2, ... / 3, ..., then
 * (l0 + l1) + (l2 + l3)), each product rounded before it is added. */
int fgnn_pair_loss_w(const float *pair_loss, int row_blocks, const float *pair_weight, int B, float *out, void *stream);

/* triplet_loss on a given score tensor: lse (B,N), pair_loss (B) (toolbox/losses.py:27-34) */
int fgnn_ce_fwd(const float *scores, const int *nvalid, int B, int N, float *lse, float *pair_loss, void *stream);
/* dscores = (softmax_row(scores) - I) * (*gscale) on valid entries, 0 on padding */
int fgnn_ce_bwd(const float *scores, const float *lse, const int *nvalid, const float *gscale, int B, int N,
                float *dscores, void *stream);
/* d scores given (B,N,N) -> d e1, d e2 (plain bmm backward, for the module-level API) */
int fgnn_score_bwd(const float *e1, const float *e2, const float *dscores, const int *nvalid,
                   int B, int C, int N, float *de1, float *de2, void *stream);

/* ---- backward ---------------------------------------------------------------------- */
/* ColumnMaxPooling backward: dy[g,c,i,idx] = de[g,c,i], 0 elsewhere (dense write).
 * Optional: y (the normalised-on-load input slab of the pooling) and s12 (G*C*2) -> also emits
 * the GraphNorm-backward sums {sum dy, sum dy*(z-mean)} of the MLP that produced y.         */
int fgnn_colmax_bwd(const float *de, const int *idx, const int *nvalid, int G, int C, int N,
                    float *dy, long long gstride, long long ldp, const fgnn_slab *y, float *s12, void *stream);

/* GraphNorm backward reductions per (g,c): S1 = sum dy, S2 = sum dy * (z - mean).         */
int fgnn_gn_bwd_stats(const float *dy, long long dgstride, long long ldd,
                      const float *z, long long zgstride, long long ldz, const float *nrm,
                      const int *nvalid, int G, int C, int N, float *s12 /* (G*C*2) */, void *stream);
/* coefficients of dz = ca*dy + cb*(z-mean) + cc : coef[g,c] = {mean, ca, cb, cc};
 * plus d gn_weight[c] = sum_g q*S2, d gn_bias[c] = sum_g S1 (fixed order over g).         */
int fgnn_gn_bwd_coef(const float *s12, const float *nrm, const int *nvalid, int G, int C, int N,
                     float *coef /* (G*C*4) */, float *dgn_w /* (C) or NULL */, float *dgn_b /* (C) or NULL */,
                     void *stream);
/* same coefficients from per-tile partial sums (G, tpg, C, 2) as emitted by fgnn_mlp_bwd
 * (s12part); also writes the summed s12 (G*C*2) for the affine gradients.                  */
int fgnn_gn_bwd_coef_tiles(const float *s12part, const float *nrm, const int *nvalid, int G, int C, int N,
                           float *s12, float *coef, void *stream);
/* dense dz = ca*dy + cb*(z-mean) + cc on valid entries (module-level GraphNorm backward) */
int fgnn_gn_bwd_apply(const float *dy, long long dgstride, long long ldd,
                      const float *z, long long zgstride, long long ldz, const float *coef,
                      const int *nvalid, int G, int C, int N, float *dz, long long ogstride, long long ldo, void *stream);

/* MlpBlock_Real backward (autograd of models/layers.py:126-131): recomputes the hidden
 * activations from the input slabs, forms dz from (dy, z, coef), back-propagates through
 * the convs and accumulates per-workgroup partial weight/bias gradients.                 */
typedef struct {
    int G, N, depth;
    const int *nvalid;
    fgnn_slab a, b;                          /* forward inputs (recompute)                */
    const float *W[FGNN_MAX_DEPTH];
    const float *bias[FGNN_MAX_DEPTH];
    const float *dy;  long long dgstride, ldd;   /* grad of the normalised output (G,32,ldd) */
    const float *z;   long long zgstride, ldz;   /* saved pre-norm output                    */
    const float *coef;                       /* (G*32*4) from fgnn_gn_bwd_coef*, or NULL: then the kernel */
    const float *s12;                        /*   derives it from s12 (G*32*2) = {sum dy, sum dy*(z-mean)}  */
    const float *znrm;                       /*   and znrm (G*32*4), the GraphNorm record of z              */
    float *dxa; long long dxa_gstride, dxa_ld;   /* out: grad wrt slab a (NULL = not needed) */
    float *dxb; long long dxb_gstride, dxb_ld;   /* out: grad wrt slab b (NULL = not needed) */
    int accumulate_a, accumulate_b;          /* 1: dx += (read-modify-write)             */
    float *wpart;                            /* out (num_wg, fgnn_mlp_param_count) partial dW/db */
    float *s12part;                          /* optional out (G, tpg, 32, 2): per-tile {sum dxa, sum dxa*(z_a-mean_a)} of
                                                the FINAL dxa values (needs a.C == 32, a.nrm and dxa) -- the GraphNorm
                                                backward sums of the MLP that produced slab a */
    const float *packed;                     /* optional: operand image from fgnn_pack_operands (kind 1) */
    const float *s12tiles;                   /* optional (G, tpg, 32, 2): per-tile sums for THIS MLP's output as emitted by its
                                                consumer's s12part; with znrm they replace coef / s12 -- every workgroup sums
                                                the tiles of the graphs it touches in its prologue (the work of
                                                fgnn_gn_bwd_coef_tiles without its launch; see ..._coef_tiles_supported).
                                                Two-slab MLPs (b.C > 0, i.e. mlp3) only                                 */
    float *s12_out;                          /* optional (G*32*2): the summed s12 is also written here (affine gradients) */
    const unsigned *xbits;                   /* optional: 2-channel slab expanded from the bit-packed adjacency, as in  */
    const float *xdeg;                       /*   fgnn_mlp_fwd_args                                                      */
    const int *ranges;                       /* optional work-balanced tile bounds + padding-tile skipping, as in the forward
                                                arguments; cannot be combined with s12tiles                                  */
    int cu_share;                            /* as in fgnn_mlp_fwd_args; 2 = fgnn_mlp_bwd_num_workgroups() / 2 workgroups and rows of
                                                wpart.  IGNORED when `ranges` is given: a ragged launch always runs the full grid
                                                and writes fgnn_mlp_bwd_num_workgroups() rows of wpart -- size wpart for that */
} fgnn_mlp_bwd_args;
int fgnn_mlp_bwd(const fgnn_mlp_bwd_args *args, void *stream);
int fgnn_mlp_bwd_x3(const fgnn_mlp_bwd_args *args, void *stream);   /* the x3 form (see fgnn_mlp_fwd_x3): image of kind 1 from
                                                                         fgnn_pack_x3_operands; input gradients for 32-channel slabs */
/* mlp1 + mlp2 of one block (models/blocks_emb.py:16-27: two MlpBlock_Real on the same input; their autograd) in ONE launch:
 * `m1` / `m2` are the argument blocks of the two fgnn_mlp_bwd calls it replaces, describing the same input slab; the input
 * gradient (dxa, accumulate_a) and its tile sums (s12part) are given in m2 only and receive (old + dx1) + dx2, bit-identical to
 * the two accumulating launches.  Depth 3, one slab of 2 or 32 channels, constant-size batches, both operand images. */
int fgnn_mlp_bwd_pair(const fgnn_mlp_bwd_args *m1, const fgnn_mlp_bwd_args *m2, void *stream);
/* The same launch with every contraction on the bf16 matrix cores through the exact three-way operand split (the arithmetic of
 * fgnn_mlp_bwd_x3 / fgnn_mlp_fwd_x3: the recompute reproduces the x3 forward bit for bit): both images are of kind 1 from
 * fgnn_pack_x3_operands; the weight-gradient operands are transposed on the matrix pipe instead of through LDS tiles
 * (csrc/mlp_bwd_pair_x3.hip).  d_in is bit-identical to two accumulating fgnn_mlp_bwd_x3 launches.  No `ranges`. */
int fgnn_mlp_bwd_pair_x3(const fgnn_mlp_bwd_args *m1, const fgnn_mlp_bwd_args *m2, void *stream);
/* Round 6: the same launch on 16-pixel tiles / v_mfma_f32_16x16x4_f32 (csrc/mlp_bwd_pair_t16.hip, csrc/fgnn_t16.h) -- same arguments,
 * work unit (a 32-pixel tile, processed as two halves), S1/S2 records and partial rows as fgnn_mlp_bwd_pair, so it is a drop-in; the
 * operand images are of kind 5 (fgnn_pack_operands).  The recomputed hidden
 * activations follow the SAME fma sequence as the 32-pixel kernels (bit-identical ReLU masks); d_in is one fma chain over (the
 * gradient mlp3 left, mlp1's terms, mlp2's terms) instead of three separately rounded sums, the weight-gradient sums run in another
 * pixel order: equal to the 32-pixel kernel to fp32 rounding, not bit for bit.  Depth 3, one dense 32-channel slab, N <= 256,
 * constant-size and ragged batches (nvalid, ranges). */
/* ... and fgnn_mlp_bwd for a two-slab MLP (mlp3 of a block: [mult ; in]) on 16-pixel tiles (csrc/mlp_bwd_t16.hip): work is assigned in
 * 16-pixel halves (4.94 per wave instead of 2.47 32-pixel tiles at the benchmarked shape).  Same argument block, partial rows and
 * results (to fp32 rounding) as fgnn_mlp_bwd; image of kind 5.  fgnn_mlp_bwd_t16_supported(args) says whether an argument block is one
 * of the built shapes: depth 3, slab a = 32 raw channels with dxa stored, slab b = 32 normalised channels with dxb stored, or 2 raw
 * channels (dense or bit-packed) without dxb; no accumulation; N <= 256. */
int fgnn_mlp_bwd_t16_supported(const fgnn_mlp_bwd_args *args);
int fgnn_mlp_bwd_t16(const fgnn_mlp_bwd_args *args, void *stream);
int fgnn_mlp_bwd_pair_t16(const fgnn_mlp_bwd_args *m1, const fgnn_mlp_bwd_args *m2, void *stream);
#define FGNN_BWD_COEF_GRAPHS 4
int fgnn_mlp_bwd_coef_tiles_supported(int G, int N);   /* s12tiles usable: a workgroup spans <= FGNN_BWD_COEF_GRAPHS graphs */
/* floats per workgroup in `wpart` for an MLP with Cin input channels and `depth` convs:
 * layout [W0 (32*Cin) | b0 (32) | W1 (32*32) | b1 (32) | ...]                           */
int fgnn_mlp_param_count(int Cin, int depth);
/* deterministic reduction of the per-workgroup partials: out[i] = sum_w wpart[w][i]      */
int fgnn_reduce_partials(const float *wpart, int num_wg, int count, float *out, void *stream);

/* One launch that finishes the parameter gradients of up to FGNN_MAX_GRAD_JOBS MLPs:
 * out[i] = sum_w wpart[w][i] (fixed order) and, when s12 is given, the GraphNorm affine
 * gradients dgn_w[c] = sum_g q[g,c]*S2[g,c], dgn_b[c] = sum_g S1[g,c].                      */
#define FGNN_MAX_GRAD_JOBS 16
typedef struct {
    const float *wpart; int count; float *out;
    const float *s12; const float *nrm; float *dgn_w; float *dgn_b;
    int rows;      /* rows of wpart to sum; 0 = num_wg (the MLP backward partials) */
    float scale;   /* factor applied to the sums; 0 = 1 (lets the loss = sum pair_loss / nodes ride along) */
    const float *scale_dev;   /* optional device scalar multiplied in as well (1 / sum(n) of a ragged batch computed on the device:
                                 fgnn_inv_node_count) */
} fgnn_grad_job;
int fgnn_grad_finalize(const fgnn_grad_job *jobs, int njobs, int num_wg, int G, int C, void *stream);
/* out[0] = 1 / sum_{b < B} nvalid[b] (0 if the sum is 0): the normaliser of triplet_loss('mean') on a ragged batch
 * (toolbox/losses.py:27-34) as a device scalar -- fgnn_score_ce_bwd's gscale and fgnn_grad_job.scale_dev read it, so a captured step
 * serves batches of any node count without a host round trip. */
int fgnn_inv_node_count(const int *nvalid, int B, float *out, void *stream);

/* Matmul backward: da = dm @ Yb^T, db = Ya^T @ dm per (g,c) (autograd of layers.py:161-162) */
int fgnn_chan_matmul_bwd(const fgnn_slab *ya, const fgnn_slab *yb, const float *dm, long long dmgstride, long long ldm,
                         const int *nvalid, int G, int N,
                         float *da, float *db, long long ogstride, long long ldo,
                         float *s12a /* optional (G*C*2): {sum da, sum da*(z_a-mean_a)} */,
                         float *s12b /* optional (G*C*2) */, void *stream);
/* longest-job-first order as in fgnn_chan_matmul_fwd_ord; with an order the two products of a matrix are separate work
 * items (dm is then read by both) */
int fgnn_chan_matmul_bwd_ord(const fgnn_slab *ya, const fgnn_slab *yb, const float *dm, long long dmgstride, long long ldm,
                             const int *nvalid, int G, int N, float *da, float *db, long long ogstride, long long ldo,
                             float *s12a, float *s12b, const int *order, int fill /* as fgnn_chan_matmul_fwd_ord */, void *stream);

/* ---- next to the hot path -------------------------------------------
 * Fused Adam over a flat fp32 buffer: torch.optim.Adam(amsgrad=False, weight_decay=0) single-tensor
 * semantics (models/trainers.py:92-104); grads are multiplied by grad_scale first; step >= 1.      */
int fgnn_adam_step(float *params, const float *grads, float *exp_avg, float *exp_avg_sq, int n, double lr,
                   double beta1, double beta2, double eps, int step, double grad_scale, void *stream);
/* the same update for a captured / replayed launch: hp (device, 5 doubles) = {lr, beta1, beta2, eps, grad_scale};
 * state (device, 2 ints, zero-initialised) = {steps taken, internal arrival counter}; the kernel advances state[0] */
int fgnn_adam_step_dev(float *params, const float *grads, float *exp_avg, float *exp_avg_sq, int n,
                       const double *hp, int *state, void *stream);
/* ---- guarded optimizer step (csrc/grad_guard.hip): what the reference gets from pl.Trainer(precision=16) -- the AMP GradScaler
 * skips optimizer.step() on a non-finite gradient -- and from Lightning's gradient_clip_val, on the device and capturable.
 * The record lives in device memory, zero-initialised by its owner, who then writes max_norm and mode; the kernels write the rest. */
#define FGNN_GUARD_MAX_PARTS 64
#define FGNN_GUARD_SKIP_NONFINITE 1 /* mode bit 0: a non-finite gradient skips the whole update */
#define FGNN_GUARD_NONFINITE 1      /* flags bit 0: the last guarded gradient held an inf or a NaN */
typedef struct {
    double max_norm; /* in: clip the global L2 norm to this; <= 0: no clipping */
    double norm;     /* out: L2 norm of the scaled gradient, before clipping (what clip_grad_norm_ returns) */
    double coef;     /* out: min(1, max_norm / (norm + 1e-6)); 1 without clipping; NaN when the norm is NaN (torch.clamp) */
    int flags;       /* out: FGNN_GUARD_NONFINITE or 0, rewritten by every launch */
    int skipped;     /* out: updates skipped so far (counts only in skip mode) */
    int arrivals;    /* internal arrival counter, 0 between launches */
    int mode;        /* in: FGNN_GUARD_SKIP_NONFINITE or 0 */
    double partial[FGNN_GUARD_MAX_PARTS]; /* internal: the workgroups' sums of squares */
} fgnn_guard_record;
/* norm, coef and flags of gi = grads[i] * (float)hp[4], i < n (the fp32 product the Adam kernels form); sum of gi^2 in fp64.
 * The order of every addition is a function of n alone (a fixed number of workgroups with one contiguous chunk each, fixed-order
 * wave / LDS / partial sums, no floating-point atomics): the same buffer gives the same bits on every launch and every rank.
 * In skip mode a non-finite gradient also advances guard->skipped.                                                           */
int fgnn_grad_guard(const float *grads, int n, const double *hp, fgnn_guard_record *guard, void *stream);
/* fgnn_adam_step_dev with grad_scale = (float)(hp[4] * guard->coef), after fgnn_grad_guard on the same grads / hp / guard.  In
 * skip mode with the non-finite flag set nothing is written: parameters, both moments and state[0] keep their values (a skipped
 * step does not count towards the bias correction, as under GradScaler).  Without skip mode a non-finite gradient propagates
 * as in torch (clip_grad_norm_(error_if_nonfinite=False) + Adam).                                                            */
int fgnn_adam_step_guarded(float *params, const float *grads, float *exp_avg, float *exp_avg_sq, int n, const double *hp,
                           int *state, const fgnn_guard_record *guard, void *stream);
/* accuracy_max (toolbox/metrics.py:119-141): correct[b] = #{i < n_b : argmax_j scores[b,i,j] == i},
 * with np.argmax's order: first maximum on ties, NaN above every number (the first NaN wins), a row of -inf
 * has column 0 as arg-max; int32, bit-exact.                                                         */
int fgnn_accuracy_max(const float *scores, const int *nvalid, int B, int N, int *correct, void *stream);
/* accuracy_linear_assignment (toolbox/metrics.py:92-116): per graph b the minimum-cost perfect matching of the n_b x n_b corner
 * of cost[b] (= -log_softmax(scores[b]); row pitch ld, graphs bstride apart), correct[b] = #{i : matched column of row i == i};
 * assign (optional, (B, N) int32) receives the matched column of every row (-1 in the padding).  The algorithm, arithmetic
 * (fp64) and tie rules are those of scipy.optimize.linear_sum_assignment (Crouse's shortest augmenting paths), so the
 * ASSIGNMENT equals SciPy's, ties included (tests/test_gpu_lsap.py).  A cost matrix without a finite matching (SciPy raises)
 * yields correct[b] = 0 and assign = -1.  No device->host copy, no host loop over the graphs.                          */
#define FGNN_LSAP_MAX_N 2048
int fgnn_lsap_accuracy(const float *cost, long long bstride, int ld, const int *nvalid, int B, int N, int *correct,
                       int *assign /* optional */, void *stream);

/* ---- block 1 on its structured input (csrc/block1_struct.hip) -----------------------------------------------------------
 * The reference always feeds block 1 the tensor representation of a graph (loaders/data_generator.py:118-125: channel 0 = the
 * 0/1 adjacency, channel 1 = diag(row sums)), so mlp1 / mlp2 of block 1 (models/blocks_emb.py:16-27, models/layers.py:126-131)
 * take one value per input class -- off-diagonal w = 0 / 1, diagonal (w_ii, deg_i) -- and their per-channel product
 * (models/layers.py:161-162) has a closed form in W, W^2, the degrees and the class values.  For bit-packed inputs of
 * batches (constant-size or ragged) with N <= 256, depth 3, these entry points replace fgnn_mlp_fwd (mlp1 + mlp2) + fgnn_chan_matmul_fwd
 * and fgnn_chan_matmul_bwd + fgnn_mlp_bwd_pair of block 1: same function, another evaluation order (equal to fp32 rounding).
 *   tables : (2 models, 2 + 2 (N + 1) classes, {h1, h2, z, z as stored}, 32) floats, graph independent: built by the first launch
 *            of fwd from tW1 / tb1 / tW2 / tb2
 *   fwd    : GraphNorm records nrm1 / nrm2 (G, 32, 4) of mlp1 / mlp2 and the raw slab mult (G, 32, ldp)
 *   bwd    : from d(mult): the first fgnn_block1_struct_rows(G, N) rows of wpart1 / wpart2 (the partial layout of fgnn_mlp_bwd; the
 *            other rows are not written: reduce exactly these, fgnn_grad_job.rows) and s12_1 / s12_2 (G, 32, 2), ready for
 *            fgnn_grad_finalize
 * The ...16 forms take the bf16 slabs of the 16-bit engine (row pitch ldr elements, channel stride ldp, tables built with the
 * arithmetic of the 16-bit engine: matrix-core operands R(W), R(relu(.)), stored R(z)): mult is rounded to nearest even on store, the statistics stay fp32 and the class sums of the backward pass
 * are formed in fp32 from the bf16 d(mult) (the generic 16-bit kernels round every pixel of dY1 / dY2 / dz instead).          */
int fgnn_block1_struct_supported(int N, int depth, int original_features_num);      /* N <= 256, depth 3, 2 input channels */
int fgnn_block1_struct_table_floats(int N);
long long fgnn_block1_struct_ws_floats(int G, int N);       /* workspace shared by fwd and bwd of one step (16-byte aligned) */
int fgnn_block1_struct_rows(int G, int N);                  /* bwd writes rows 0 .. rows-1 of wpart1 / wpart2 (<= fgnn_mlp_bwd_num_workgroups()) and no others; G > that many rows: row b sums the graphs b, b + rows, ... */
/* nvalid: optional per-graph vertex counts (ragged batches: the N x N planes are padded; mult is written as 0 outside the valid
 * corner, class counts and the GraphNorm n use nvalid[g]).  fwd fills ws (16-bit code plane (W^2)_ij | w_ij << 15, per-vertex
 * {row sum, column sum, w_ii, class}); bwd of the same step reads it. */
int fgnn_block1_struct_fwd(const unsigned *bits, const int *nvalid, int G, int N, const float *tables, const float *gnw1, const float *gnb1,
                           const float *gnw2, const float *gnb2, float eps, float *nrm1, float *nrm2, float *mult, long long gstride,
                           long long ldp, float *xdeg /* optional: (G, N) row sums, as fgnn_adjacency_degree writes them */, float *ws,
                           const float *const *tW1, const float *const *tb1, const float *const *tW2, const float *const *tb2
                           /* required: the three weights / biases of mlp1 and mlp2 of block 1 -- `tables` is (re)built from them
                              inside the first launch of this call */,
                           void *stream);
int fgnn_block1_struct_bwd(const unsigned *bits, const int *nvalid, int G, int N, const float *tables, const float *const *W1,
                           const float *const *W2, const float *nrm1, const float *nrm2, const float *gnb1, const float *gnb2,
                           const float *dmult, long long gstride, long long ldp, float *ws, float *wpart1, float *wpart2, float *s12_1,
                           float *s12_2, void *stream);
/* fgnn_block1_struct_fwd with the step's operand packing folded in: `jobs` (njobs <= FGNN_MAX_PACK_JOBS) are what fgnn_pack_operands would be
 * launched with; they run as extra workgroups of the first launch (which, like them, depends on the weights and the input only), one launch
 * less per step.  Results identical to the two entry points called one after the other. */
int fgnn_block1_struct_fwd_pack(const unsigned *bits, const int *nvalid, int G, int N, const float *tables, const float *gnw1, const float *gnb1,
                                const float *gnw2, const float *gnb2, float eps, float *nrm1, float *nrm2, float *mult, long long gstride,
                                long long ldp, float *xdeg, float *ws, const float *const *tW1, const float *const *tb1,
                                const float *const *tW2, const float *const *tb2, const fgnn_pack_job *jobs, int njobs, void *stream);
/* x16 (optional): the (G, 2, ldp) bf16 input slab (channel 0 = W, channel 1 = diag(row sums)) the later kernels of block 1 read */
int fgnn_block1_struct_fwd16(const unsigned *bits, const int *nvalid, int G, int N, int ldr, const float *tables, const float *gnw1,
                             const float *gnb1, const float *gnw2, const float *gnb2, float eps, float *nrm1, float *nrm2,
                             void *mult /* bf16 */, long long gstride, long long ldp, void *x16 /* bf16, optional */, float *ws,
                             const float *const *tW1, const float *const *tb1, const float *const *tW2, const float *const *tb2, void *stream);
/* ... and fgnn_block1_struct_fwd16 with the jobs of fgnn_pack16_operands riding in its first launch */
int fgnn_block1_struct_fwd16_pack(const unsigned *bits, const int *nvalid, int G, int N, int ldr, const float *tables, const float *gnw1,
                                  const float *gnb1, const float *gnw2, const float *gnb2, float eps, float *nrm1, float *nrm2, void *mult,
                                  long long gstride, long long ldp, void *x16, float *ws, const float *const *tW1, const float *const *tb1,
                                  const float *const *tW2, const float *const *tb2, const fgnn_pack_job *jobs, int njobs, void *stream);
int fgnn_block1_struct_bwd16(const unsigned *bits, const int *nvalid, int G, int N, int ldr, const float *tables, const float *const *W1,
                             const float *const *W2, const float *nrm1, const float *nrm2, const float *gnb1, const float *gnb2,
                             const void *dmult /* bf16 */, long long gstride, long long ldp, float *ws, float *wpart1, float *wpart2,
                             float *s12_1, float *s12_2, void *stream);

/* Input expansion (loaders/data_generator.py:118-125): bits (G, N, ceil(N/32)) uint32, bit j of row i =
 * W[i][j]  ->  x (G, 2, N, N) fp32 with x[g,0] = W, x[g,1] = diag(row sums); exact 0/1/integer values. */
int fgnn_expand_adjacency(const unsigned *bits, const int *nvalid, int G, int N, float *x, void *stream);
/* ... and back: the (G, 2, N, N) tensor representation a dense loader produced -> bit-packed adjacency (rows / columns >= nvalid[g]
 * read as empty).  bad (optional device int, zeroed by the caller): set to 1 if x is NOT a tensor representation on the valid corners
 * (an entry of channel 0 outside {0, 1}, channel 1 != diag(row sums of channel 0)) -- the structured block 1 must not see such bits. */
int fgnn_pack_adjacency(const float *x, const int *nvalid, int G, int N, unsigned *bits, int *bad, void *stream);
/* The same with the loader's padded size Nin (x is (G, 2, Nin, Nin)) smaller than the engine's N (bits are (G, N, ceil(N/32)): rows
 * and columns >= Nin are empty): what Siamese_Node_Exp.fused_step(input_form='tensor_representation') runs on each side of a dense or
 * MaskedTensor loader batch (loaders/loaders.py:5-15) in front of the structured block 1.  `bad` is OR-ed (sticky until the caller
 * zeroes it); an nvalid[g] outside [0, Nin] also sets it. */
int fgnn_pack_adjacency_ld(const float *x, const int *nvalid, int G, int Nin, int N, unsigned *bits, int *bad, void *stream);
/* Both sides of a siamese batch in ONE launch (loaders/loaders.py:12-15 yields the two sides as two tensors): bits (2 B, N, words) = the B graphs
 * of x1 followed by the B graphs of x2, each side with its own vertex counts (both NULL: constant-size).  Optionally the counts are copied to
 * nv_out (2 B entries: the engine's nvalid) and 1 / sum(nvalid1) -- the normaliser of triplet_loss 'mean', toolbox/losses.py:27-34 -- is left
 * in inv_out (what fgnn_inv_node_count computes).  Same verdict flag as fgnn_pack_adjacency_ld. */
int fgnn_pack_adjacency_pair(const float *x1, const float *x2, const int *nvalid1, const int *nvalid2, int B, int Nin, int N, unsigned *bits,
                             int *nv_out, float *inv_out, int *bad, void *stream);
/* deg[g][i] = number of set bits j < nvalid[g] in row i (0 for rows >= nvalid[g]): the diagonal of channel 1, for the
 * kernels that expand the adjacency themselves (fgnn_mlp_fwd_args.xbits / xdeg) */
int fgnn_adjacency_degree(const unsigned *bits, const int *nvalid, int G, int N, float *deg, void *stream);

/* Ragged batches: work-balanced tile ranges for the persistent MLP kernels.  A tile (32 consecutive pixels of one graph's
 * N x N plane) that holds no pixel of the valid n x n corner costs a zero-fill, any other tile a full pass; ranges[w] ..
 * ranges[w+1] (w < FGNN_RANGE_WG) split the G * tiles_per_graph tiles into pieces of equal cost.  One small launch per
 * batch; the result depends on nvalid only (deterministic).  No reference counterpart: the reference computes the padded
 * (Nmax x Nmax) tensors in full (maskedtensors/maskedtensor.py:98-112).                                                  */
#define FGNN_RANGE_WG 256
int fgnn_ragged_tile_ranges(const int *nvalid, int G, int N, int *ranges /* FGNN_RANGE_WG + 1 */, void *stream);
/* the same launch also writes order[0 .. G): the graph indices sorted by nvalid, largest first (ties: lower index first),
 * the schedule of fgnn_chan_matmul_fwd_ord / fgnn_chan_matmul_bwd_ord */
int fgnn_ragged_tile_ranges_order(const int *nvalid, int G, int N, int *ranges /* FGNN_RANGE_WG + 1 */, int *order /* G */,
                                  void *stream);
/* the same for the bf16 slabs (tiles of 64 elements of the ldr-pitched planes) */
int fgnn_ragged_tile_ranges16(const int *nvalid, int G, int N, int ldr, int *ranges /* FGNN_RANGE_WG + 1 */, void *stream);

/* out[i] = sum_k in[k][i] * scale  (tiny fixed-order reduction used for the loss) */
int fgnn_sum_scale(const float *in, int rows, int cols, float scale, float *out, void *stream);

/* =====================================================================================================
 * bf16 variant of the same path (BASELINE config 4: N = 200 dense pairs, 16-bit).  The reference trains under
 * 16-bit AMP (commander_explore.py:120-122, Network.half models/utils.py:71-74); here activations and gradient
 * slabs are STORED as bf16, every channel contraction / per-channel N x N product runs on
 * v_mfma_f32_32x32x16_bf16 with fp32 accumulation, and biases, GraphNorm statistics, embeddings, scores, loss
 * and all parameter gradients stay fp32.  Rounding points: oracle/fgnn_oracle_bf16.py.
 *
 * Layout of a bf16 activation tensor (G, C, ldp): a channel holds N rows of `ldr` elements, ldr = N rounded up
 * to a multiple of 8 (rows 16-byte aligned), element (i, j) at i*ldr + j; ldp >= N*ldr is a multiple of 64
 * (channels 128-byte aligned).  Columns j >= N, like all padding of a ragged graph, are stored as exact zeros.
 * A "tile" of the bf16 MLP kernels is 64 consecutive elements of a channel; tile statistics / per-tile sums
 * (part, cnt, s12part) have fgnn_tiles_per_graph16(N, ldr) = ceil(N*ldr / 64) entries per graph. */
typedef struct {
    const void *ptr;         /* bf16 (G, C, ldp)                                        */
    long long gstride;       /* elements between graphs                                 */
    long long ldp;           /* elements between channels                               */
    int C;                   /* channels: 2 or 32 (0 = slab unused)                     */
    const float *nrm;        /* optional (G*C*4) fp32 {mean, a, q, r2}                  */
    const float *beta;       /* optional (C) fp32                                       */
} fgnn_slab16;
int fgnn_tiles_per_graph16(int N, int ldr);

/* fp32 (G, C, N, N) contiguous  ->  bf16 (G, C, ldp) with row pitch ldr (padding zero-filled), and back */
int fgnn_to_bf16(const float *x, const int *nvalid, int G, int C, int N, int ldr, void *y, long long gstride, long long ldp,
                 void *stream);
int fgnn_from_bf16(const void *y, long long gstride, long long ldp, int G, int C, int N, int ldr, float *x, void *stream);
/* fp32 (G, c, N, N) contiguous  ->  the bf16 input slab of block 1 in one pass: CP = 2 or 32 channels (the slab's width, stated
 * by the caller), 1 <= c <= CP, (G, CP, ldp) with gstride = CP * ldp.  Channels < c: round-to-nearest-even inside the graph's n_g x n_g corner (nvalid, or N);
 * channels >= c, the ragged padding, the pitch columns and the tail of every channel up to ldp: exact +0.  Nothing outside the
 * corner of x is read.  ldr: multiple of 8, ldp: multiple of 64 (the engine's pitches); y 16-byte aligned. */
int fgnn_to_bf16_pad(const float *x, const int *nvalid, int G, int c, int CP, int N, int ldr, void *y, long long ldp, void *stream);

/* operand images of the bf16 MLP kernels (weights rounded to bf16, biases fp32), packed once per step.
 * kind 0 = forward image (nmlp MLPs back to back), kind 1 = backward image (one MLP, W[0] / bias[0]). */
int fgnn_pack16_floats(int kind, int ca, int cb, int depth, int nmlp);   /* size in 4-byte units */
int fgnn_pack16_operands(const fgnn_pack_job *jobs, int njobs, void *stream);

/* MlpBlock_Real.forward minus the normalisation (models/layers.py:126-131), bf16 storage: see fgnn_mlp_fwd */
typedef struct {
    int G, N, ldr, depth, nmlp;
    const int *nvalid;
    fgnn_slab16 a, b;
    void *z[2];                             /* out bf16 (G, 32, ldz)                      */
    long long ldz;
    float *part[2];                         /* out (G, 32, tpg16, 2) {mean, M2} of the fp32 z (tile index fastest: the
                                               *_tpg helpers and fgnn_chan_matmul_fwd16_fin walk one (g, c) column) */
    float *cnt;                             /* out (G, tpg16)                             */
    const void *packed;                     /* operand image (kind 0) -- required          */
    const int *ranges;                      /* optional (ragged): tile bounds from fgnn_ragged_tile_ranges16, see fgnn_mlp_fwd_args.ranges */
} fgnn_mlp_fwd16_args;
int fgnn_mlp_fwd16(const fgnn_mlp_fwd16_args *args, void *stream);
/* Test-only: the same launch that also writes its ReLU decisions (the bf16 twin of fgnn_debug_mlp_fwd_masks): masks[m] is
 * (G, 2, 32, fgnn_tiles_per_graph16(N, ldr), 2) words, bit j of word (g, layer, channel, t, parity) = [hidden pre-activation of element
 * 64 t + 2 j + parity of the ldr-pitched plane > 0].  Constant-size batches, the fused engine's shapes. */
int fgnn_debug_mlp_fwd16_masks(const fgnn_mlp_fwd16_args *args, unsigned *masks0, unsigned *masks1, void *stream);

/* GraphNorm finalize / backward-coefficient helpers of the bf16 kernels: explicit tile count per graph (the fp32 entry
 * points derive it from FGNN_TILE) and partials in the bf16 kernels' layout (G, C, tpg, 2) -- tile index fastest -- instead
 * of the fp32 kernels' (G, tpg, C, 2) */
int fgnn_gn_finalize_tpg(const float *part, const float *cnt, const float *gn_weight, const int *nvalid, int G, int C, int N,
                         int tpg, float eps, float *nrm, void *stream);
int fgnn_gn_finalize2_tpg(const float *part0, const float *part1, const float *cnt, const float *gn_weight0,
                          const float *gn_weight1, const int *nvalid, int G, int C, int N, int tpg, float eps, float *nrm0,
                          float *nrm1, void *stream);
int fgnn_gn_bwd_coef_tiles_tpg(const float *s12part, const float *nrm, const int *nvalid, int G, int C, int N, int tpg,
                               float *s12, float *coef, void *stream);

/* Matmul.forward / backward on bf16 slabs (models/layers.py:161-162), N <= 256: operands normalised on load and
 * rounded to bf16, fp32 accumulation, outputs rounded to bf16; s12a / s12b as in fgnn_chan_matmul_bwd (sums of the
 * ROUNDED outputs). */
int fgnn_chan_matmul_fwd16(const fgnn_slab16 *ya, const fgnn_slab16 *yb, const int *nvalid, int G, int N, int ldr,
                           void *out, long long ogstride, long long ldo, void *stream);
/* the forward product with the GraphNorm finalize of its two operands folded into the prologue (replaces a
 * fgnn_gn_finalize2_tpg launch): part_a / part_b / cnt are the tile statistics of the fgnn_mlp_fwd16 call that produced the
 * operands; the records are written to ya->nrm / yb->nrm (G*C*4 floats each, for the backward pass) and used at once */
int fgnn_chan_matmul_fwd16_fin(const fgnn_slab16 *ya, const fgnn_slab16 *yb, const float *part_a, const float *part_b,
                               const float *cnt, const float *gn_weight_a, const float *gn_weight_b, float eps, int tpg,
                               const int *nvalid, int G, int N, int ldr, void *out, long long ogstride, long long ldo,
                               void *stream);
int fgnn_chan_matmul_bwd16(const fgnn_slab16 *ya, const fgnn_slab16 *yb, const void *dm, long long dmgstride, long long ldm,
                           const int *nvalid, int G, int N, int ldr, void *da, void *db, long long ogstride, long long ldo,
                           float *s12a, float *s12b, void *stream);

/* the same with S2 derived from the trace term T = <dM, M> instead of re-reading the two raw operand slabs:
 * tpart (G, C, tpg): per-tile sum dM * M as emitted (into s12part) by the fgnn_mlp_bwd16 call that produced dM
 * from the MLP whose first input slab is M = the forward product (mlp3);
 *   sum dA (z_a - mean_a) = (T - beta_a S1_a) / a_a,   sum dB (z_b - mean_b) = (T - beta_b S1_b) / a_b */
int fgnn_chan_matmul_bwd16_t(const fgnn_slab16 *ya, const fgnn_slab16 *yb, const void *dm, long long dmgstride, long long ldm,
                             const float *tpart, int tpg, const int *nvalid, int G, int N, int ldr, void *da, void *db,
                             long long ogstride, long long ldo, float *s12a, float *s12b, void *stream);

/* fgnn_chan_matmul_bwd16_t that also writes the dz-coefficient records (G*C*4, the output of fgnn_gn_bwd_coef) of the two
 * operand MLPs from the s12 sums it has just formed -- one tiny launch per block less */
int fgnn_chan_matmul_bwd16_tc(const fgnn_slab16 *ya, const fgnn_slab16 *yb, const void *dm, long long dmgstride, long long ldm,
                              const float *tpart, int tpg, const int *nvalid, int G, int N, int ldr, void *da, void *db,
                              long long ogstride, long long ldo, float *s12a, float *s12b, float *coefa, float *coefb,
                              void *stream);
/* ColumnMaxPooling on a bf16 slab: e (G,C,N) fp32 = max_j of the fp32-normalised values, idx int32 */
int fgnn_colmax_fwd16(const fgnn_slab16 *y, const int *nvalid, int G, int N, int ldr, float *e, int *idx, void *stream);
/* its backward: dy (bf16) [g,c,i,idx] = R(de[g,c,i]); s12 = {sum dy, sum dy*(z-mean)} of the rounded values */
int fgnn_colmax_bwd16(const float *de, const int *idx, const int *nvalid, int G, int C, int N, int ldr, void *dy,
                      long long gstride, long long ldp, const fgnn_slab16 *y, float *s12, void *stream);
/* the same, also writing the dz-coefficient record (G*C*4) of the pooled MLP from its s12 sums */
int fgnn_colmax_bwd16_coef(const float *de, const int *idx, const int *nvalid, int G, int C, int N, int ldr, void *dy,
                           long long gstride, long long ldp, const fgnn_slab16 *y, float *s12, float *coef, void *stream);

/* MlpBlock_Real backward on bf16 slabs: see fgnn_mlp_bwd.  coef (G*32*4) is required (fgnn_gn_bwd_coef*).
 * dx outputs are rounded to bf16; with accumulate the old bf16 value is added in fp32 before rounding. */
typedef struct {
    int G, N, ldr, depth;
    const int *nvalid;
    fgnn_slab16 a, b;
    const void *dy;  long long dgstride, ldd;
    const void *z;   long long zgstride, ldz;
    const float *coef;
    void *dxa; long long dxa_gstride, dxa_ld;
    void *dxb; long long dxb_gstride, dxb_ld;
    int accumulate_a, accumulate_b;
    float *wpart;                            /* out (num_wg, fgnn_mlp_param_count) partial dW/db (fp32) */
    float *s12part;                          /* optional out, needs a.C == 32 and dxa.  Single normalised slab (no slab b):
                                                (G, 32, tpg16, 2) per-tile {sum dxa, sum dxa*(z_a-mean_a)} of the FINAL (rounded)
                                                dxa values.  Raw first slab of a two-slab MLP (mlp3: a = mult): (G, 32, tpg16)
                                                per-tile sum dxa * x_a, the trace term read by fgnn_chan_matmul_bwd16_t */
    const void *packed;                      /* operand image (kind 1) -- required */
    const int *ranges;                       /* optional (ragged): tile bounds from fgnn_ragged_tile_ranges16 */
} fgnn_mlp_bwd16_args;
int fgnn_mlp_bwd16(const fgnn_mlp_bwd16_args *args, void *stream);
/* mlp1 + mlp2 of one block in ONE launch, bf16 (the twin of fgnn_mlp_bwd_pair): m1 / m2 are the argument blocks of the two
 * fgnn_mlp_bwd16 calls it replaces; the input gradient (dxa, accumulate_a, s12part) is given in m2 only and receives
 * R(R(old + dx1) + dx2), bit-identical to the two read-modify-write launches.  One slab of 2 or 32 channels, constant-size batches. */
int fgnn_mlp_bwd16_pair(const fgnn_mlp_bwd16_args *m1, const fgnn_mlp_bwd16_args *m2, void *stream);

/* ---- QAP pair generation (loaders/data_generator.py:38-125,175-219: QAP_Generator) ------------------------------------------
 * B pairs (graph, noisy graph) written straight into the engine's wire format: bits1 / bits2 (B, N, ceil(N/32)) words, bit j of
 * word row i = W[i][j] (the layout of fgnn_expand_adjacency), rows / columns >= n_k and padding bits zero; nvalid (optional,
 * int32[B]) = n_k.  Pair k (= first + b) of dataset `seed` depends on (seed, k) only: every draw is addressed by (pair, stream,
 * position) on Philox4x64-10, never by thread or launch.  Probabilities arrive as integer thresholds thr = min(2^32,
 * floor(prob * 2^32)); an event is u32 < thr.  graph_neural_net_amd/pairgen.py documents the streams and algorithms. */
#define FGNN_PAIRGEN_ERDOS_RENYI 0      /* family / noise model */
#define FGNN_PAIRGEN_REGULAR 1          /* family */
#define FGNN_PAIRGEN_BARABASI_ALBERT 2  /* family */
#define FGNN_PAIRGEN_EDGE_SWAP 1        /* noise model */
#define FGNN_PAIRGEN_MAX_N 256
typedef struct {
    unsigned long long seed;            /* Philox key */
    long long first;                    /* index of the first pair of the launch */
    int B, N;                           /* pairs, padded size (1 <= N <= FGNN_PAIRGEN_MAX_N) */
    int family, noise_model;
    double edge_density;                /* p: Regular degree int(p n) (+1 if n d is odd), BA attachments int(p (n-1) / 2) */
    unsigned long long thr_edge;        /* ErdosRenyi parent: p */
    unsigned long long thr_noise1;      /* ErdosRenyi noise: edge removal (noise); EdgeSwap: both loops (noise) */
    unsigned long long thr_noise2;      /* ErdosRenyi noise: edge insertion (p noise / (1 - p)) */
    unsigned long long thr_vertex;      /* vertex_proba; 2^32 = constant N, else n ~ Binomial(N, vertex_proba) */
    int swaps_per_edge;                 /* Regular: double-edge swaps per edge of the circulant seed */
    unsigned *bits1, *bits2;            /* out (B, N, ceil(N/32)) */
    int *nvalid;                        /* optional out (B) */
} fgnn_pairgen_args;
/* 1 if (N, family, noise_model) is a shape fgnn_pairgen runs */
int fgnn_pairgen_supported(int N, int family, int noise_model);
int fgnn_pairgen(const fgnn_pairgen_args *args, void *stream);
/* The same launch with pair b = dataset pair index[b] (int64[B] on the device; any order, duplicates allowed): args->first is
 * ignored, every stream, draw and output is that of the contiguous launch for the same pair.  A negative index is a caller error:
 * its pair is written as the empty graph (all words zero, nvalid = 0) and nothing outside index[0..B) is read. */
int fgnn_pairgen_indexed(const fgnn_pairgen_args *args, const long long *index, void *stream);
/* Pairs of several noise levels in one launch: pair b takes its two noise thresholds from row level[b] (int32[B] on the device) of
 * level_thr ((K, 2) 64-bit words on the device: thr_noise1, thr_noise2 of each level; 1 <= K <= FGNN_MAX_LEVELS; 2^32 is noise 1);
 * args->thr_noise1 / thr_noise2 are ignored.  Pair b is index[b], or args->first + b when index is NULL, and is what
 * fgnn_pairgen_indexed writes for that dataset index with the thresholds of its level -- the same streams, draws and words: a draw
 * does not depend on the threshold it is compared with.  EdgeSwap reads the first threshold only.  A level outside [0, K) is a
 * caller error treated like a negative index: the empty graph, nvalid = 0. */
#define FGNN_MAX_LEVELS 64
int fgnn_pairgen_levels(const fgnn_pairgen_args *args, const long long *index /* NULL: args->first + b */,
                        const unsigned long long *level_thr /* (K, 2) */, int K, const int *level /* (B) */, void *stream);

/* ---- stored graphs (csrc/pairstore.hip; graph_neural_net_amd/pairstore.py) -----------------------------------------------------
 * A store is M graphs in the wire format above, resident in device memory: parents (M, N, ceil(N/32)) words, symmetric, zero
 * diagonal, rows / columns >= n_k and padding bits zero; sizes (optional, int32[M]) = n_k in [0, N], NULL when every graph has N
 * vertices; seconds (optional, the shape of parents): a stored second side.  One launch writes the batch (bits1, bits2, nvalid) of
 * fgnn_pairgen_indexed: workgroup b takes example k = index[b] (int64[B] on the device), or first + b when index is NULL.  bits1 is
 * parents[k], nvalid n_k, and bits2
 *   with seconds: seconds[k] as it is (seed, noise_model, emax, the thresholds and the levels are not used; levels are refused);
 *   without: the noisy copy that pairgen_kernel's noise stage makes of that parent for pair (seed, k) at this N and n_k -- streams
 *     2 / 3, positions i N + j (ErdosRenyi), o and o 2m + i (EdgeSwap), the thresholds below -- so a store filled with a generator's
 *     parents returns that generator's pairs bit for bit.  EdgeSwap keeps the parent's edge list in LDS: emax >= the largest edge
 *     count of a stored parent (at most N (N - 1) / 2).
 * level_thr, K, level: as in fgnn_pairgen_levels (all NULL / 0: thr_noise1 / thr_noise2 of the arguments hold for every pair).
 * Caller errors that the host cannot see are handled as fgnn_pairgen_indexed handles a negative index -- the empty graph, nvalid = 0,
 * nothing outside the arguments' extents read: k outside [0, M), a level outside [0, K), a parent with more than emax edges. */
typedef struct {
    unsigned long long seed;            /* Philox key of the noise */
    long long first;                    /* example of workgroup 0 when index is NULL */
    long long M;                        /* stored graphs */
    int B, N;                           /* pairs of the launch, padded size (1 <= N <= FGNN_PAIRGEN_MAX_N) */
    int noise_model;                    /* FGNN_PAIRGEN_ERDOS_RENYI / FGNN_PAIRGEN_EDGE_SWAP */
    int emax;                           /* EdgeSwap: largest edge count of a stored parent */
    unsigned long long thr_noise1;      /* as in fgnn_pairgen_args */
    unsigned long long thr_noise2;
    const unsigned *parents;            /* (M, N, ceil(N/32)) */
    const int *sizes;                   /* optional (M) */
    const unsigned *seconds;            /* optional (M, N, ceil(N/32)) */
    const long long *index;             /* optional (B) */
    const unsigned long long *level_thr; /* optional (K, 2) */
    const int *level;                   /* optional (B) */
    int K;
    unsigned *bits1, *bits2;            /* out (B, N, ceil(N/32)) */
    int *nvalid;                        /* optional out (B) */
} fgnn_pairstore_args;
/* 1 if (N, noise_model) is a shape fgnn_pairstore_gather runs */
int fgnn_pairstore_supported(int N, int noise_model);
int fgnn_pairstore_gather(const fgnn_pairstore_args *args, void *stream);

/* ---- correlated Gaussian (Wigner) pairs (csrc/wigner.hip; graph_neural_net_amd/wigner.py) ---------------------------------------
 * B real-weighted pairs, both sides in one launch, as tensor representations (loaders/data_generator.py:118-125 on a real W):
 * x1 / x2 (B, 2, N, N) fp32, channel 0 = W (symmetric, zero diagonal), channel 1 = diag(row sums of W); everything outside the
 * n_b x n_b corner and every off-diagonal entry of channel 1 is +0.0f.  Pair b is index[b], or first + b when index is NULL.
 *   vertex count: n_b of fgnn_pairgen for the same (seed, pair, N, thr_vertex) -- stream 0, the same redraw rule;
 *   normals: z_s(t) for the unordered entry {i, j}, i < j, t = i N + j (N the padded size), from stream s = FGNN_WIGNER_PARENT_STREAM
 *     / FGNN_WIGNER_NOISE_STREAM of the pair: Philox block t >> 3, 64-bit word (t & 7) >> 1 = (w0 low half, w1 high half),
 *     u = ((w0 >> 8) + 1) 2^-24, v = (w1 >> 8) 2^-24, r = sqrtf(-2 logf(u)), z = r cospif(2 v) for even t, r sinpif(2 v) for odd t;
 *   values: A_ij = c_b z_parent(t), B_ij = fmaf(rho, A_ij, sig (c_b z_noise(t))), c_b = 1 / sqrtf(n_b) with scale != 0, else 1;
 *     every product is rounded on its own.  rho, sig: the arguments', or row level[b] of level_coef ((K, 2) fp32 on the device,
 *     1 <= K <= FGNN_MAX_LEVELS) when level is given: a draw does not depend on them;
 *   support (bits1, bits2: both or neither; (B, N, ceil(N/32)) words of the same pairs, unpermuted): A_ij is written where bit
 *     (min, max) of bits1 is set, B_ij where that of bits2 is, +0.0f elsewhere;
 *   labels ((B, N) int32, labels[b, i] = pi_b(i) for i < n_b): side 2 is written relabelled, x2[pi(i)][pi(j)] = B_ij; a column or
 *     row no label < n_b maps to is written as zeros, and no label is used as an address;
 *   row sums: fp32, of the output row as it is stored, in the order fixed in csrc/wigner.hip (per-lane column sums, xor butterfly).
 * nvalid (optional, int32[B]) = n_b.  x1 = x2 = NULL: only nvalid is written (the vertex counts the planted permutation needs
 * before the pairs are made).  Caller errors the host cannot see -- a negative index, a level outside [0, K) -- give the empty
 * graph (all zeros) and nvalid = 0, as in fgnn_pairgen_indexed.  1 <= N <= FGNN_PAIRGEN_MAX_N, B <= 65535. */
#define FGNN_WIGNER_PARENT_STREAM 10
#define FGNN_WIGNER_NOISE_STREAM 11
typedef struct {
    unsigned long long seed;            /* Philox key */
    long long first;                    /* pair of b = 0 when index is NULL */
    int B, N;
    unsigned long long thr_vertex;      /* as in fgnn_pairgen_args */
    float rho, sig;                     /* (float)sqrt(1 - s^2), (float)s: used when level is NULL */
    int scale;                          /* 1: c_b = 1 / sqrtf(n_b); 0: c_b = 1 */
    int K;                              /* rows of level_coef */
    const long long *index;             /* optional (B) */
    const float *level_coef;            /* optional (K, 2): rho, sig of each level */
    const int *level;                   /* optional (B) */
    const unsigned *bits1, *bits2;      /* optional support (B, N, ceil(N/32)) */
    const int *labels;                  /* optional (B, N) */
    float *x1, *x2;                     /* out (B, 2, N, N); both NULL: nvalid only */
    int *nvalid;                        /* optional out (B) */
} fgnn_wigner_args;
int fgnn_wigner_pairs(const fgnn_wigner_args *args, void *stream);

/* ---- the order of a shuffled epoch (csrc/pairgen.hip; graph_neural_net_amd/sampler.py) ---------------------------------------
 * out[i] = pi((first_pos + i) mod M) for i < count, with pi the permutation of [0, M) that (seed, epoch) select: a balanced Feistel
 * network on 2 h bits (h = max(1, ceil(ceil(log2 M) / 2))), FGNN_EPOCH_ROUNDS rounds, walked along its cycle until the value is
 * < M.  The round function of round r on right half R is the low h bits of word 0 of Philox4x64-10 at counter
 * (epoch, r, R, FGNN_EPOCH_STREAM) under key (seed, 0) -- the fourth counter word of every pair stream is 0, so the two never
 * meet.  O(1) per position, no M-sized temporary: position p of epoch e is the same however the epoch is cut into launches or
 * ranks.  1 <= M <= 2^40, first_pos >= 0, 0 <= count < 2^31; out is int64[count] on the device. */
#define FGNN_EPOCH_ROUNDS 8
#define FGNN_EPOCH_STREAM 6
#define FGNN_EPOCH_MAX_LOG2_M 40
int fgnn_epoch_index(unsigned long long seed, unsigned long long epoch, long long M, long long first_pos, long long count,
                     long long *out, void *stream);

/* ---- planted permutations (csrc/planted.hip; graph_neural_net_amd/planted.py) -------------------------------------------------
 * labels: (B, N) int32, labels[b][i] = pi_b(i): vertex i of the first graph of pair b is vertex pi_b(i) of the second; entries
 * i >= n_b are -1, like assign.  nvalid (optional, int32[B]) = n_b, clamped to [0, N]; N <= FGNN_PLANTED_MAX_N.  No entry point copies
 * to the host, allocates or synchronises: all are capturable.
 *
 * fgnn_planted_perm: a uniform permutation of [0, n_b) per pair, a function of (seed, pair index) only: pair b is first + b, or
 *   index[b] when index (int64[B] on the device) is given (first is then ignored; a negative index, a caller error, gives the empty
 *   permutation: all -1).  Fisher-Yates from the top on the identity: for k = n_b - 1 .. 1, j = (u32_k (k + 1)) >> 32, swap p[k], p[j],
 *   with u32_k raw draw k of pair stream FGNN_PLANTED_STREAM (third counter word, fourth word 0, as every pair stream).
 * fgnn_relabel_bits: out[pi(i)][pi(j)] = in[i][j] on (B, N, ceil(N/32)) bit words; no symmetry assumed; rows, columns and padding bits
 *   >= n_b of out are zero whatever in holds there.  out may be in.
 * fgnn_relabel_dense: the same movement on (B, C, ld, ld) fp32 planes (out != in), any C >= 1, ld <= FGNN_PLANTED_MAX_N; labels has
 *   row pitch NL and n_b is clamped to [0, min(ld, NL)].  Pure data movement: bit-exact; everything outside the n_b x n_b corner of
 *   out is an exact zero, and nothing outside the corner of in is read.  The batch must be smaller than 2 GiB, B <= 65535.
 * A labels row that is no permutation of [0, n_b) is a caller error; rows and columns no entry maps to come out zero.
 * fgnn_count_matches: correct[b] = #{i < n_b : assign[b][i] == labels[b][i]} (both (B, N) int32).
 * fgnn_accuracy_max_labels: fgnn_accuracy_max against labels: correct[b] = #{i < n_b : argmax_j scores[b,i,j] == labels[b][i]}, the
 *   same arg-max (first maximum on ties, NaN above every number). */
#define FGNN_PLANTED_STREAM 7
#define FGNN_PLANTED_MAX_N 256
int fgnn_planted_perm(unsigned long long seed, long long first, const long long *index /* optional */, const int *nvalid /* optional */,
                      int B, int N, int *labels, void *stream);
/* fgnn_reveal_seeds: a seed vector (see the seeds section below) from labels: min(count, n_b) rows of pair b keep their label, every
 * other entry is -1.  The rows are uniform without replacement and a function of (seed, pair index) only (first / index as above):
 * the first min(count, n_b) steps of fgnn_planted_perm's Fisher-Yates from the top on the identity, with the draws of pair stream
 * FGNN_SEEDS_STREAM; the rows revealed are p[n_b - count .. n_b - 1]. */
#define FGNN_SEEDS_STREAM 8
int fgnn_reveal_seeds(unsigned long long seed, long long first, const long long *index /* optional */, const int *labels,
                      const int *nvalid /* optional */, int B, int N, int count, int *seeds, void *stream);
int fgnn_relabel_bits(const unsigned *in, const int *labels, const int *nvalid, int B, int N, unsigned *out, void *stream);
int fgnn_relabel_dense(const float *in, const int *labels, const int *nvalid, int B, int C, int ld, int NL, float *out, void *stream);
int fgnn_count_matches(const int *assign, const int *labels, const int *nvalid, int B, int N, int *correct, void *stream);
int fgnn_accuracy_max_labels(const float *scores, const int *labels, const int *nvalid, int B, int N, int *correct, void *stream);

/* ---- decoding a matching: QAP objective and greedy refinement (csrc/qap.hip; toolbox/metrics.py:168-193 all_acc_qap,
 * toolbox/utils.py:225-256 perm_matrix / score / improve / greedy_qap) --------------------------------------------------------
 * bits1 / bits2: (B, N, ceil(N/32)) words, bit j of word row i = A[i][j] resp. B[i][j] (the layout of fgnn_expand_adjacency).
 * nvalid (optional, int32[B]): pair b is the n_b x n_b corner (n_b clamped to [0, N]); bits outside it are ignored, they need not
 * be zero.  assign: (B, N) int32, the matched column pi(i) of row i, as fgnn_lsap_accuracy writes it; entries outside [0, n_b) (the
 * -1 of an infeasible pair) contribute nothing; the entries inside the corner must be distinct.  On 0/1 matrices everything here is
 * integer arithmetic, so every output is exact.  N <= FGNN_QAP_MAX_N; no entry point copies to the host or synchronises.
 *
 * fgnn_qap_objective, per pair, int32, every output optional:
 *   qap[b]     = sum_{i,k} A[i,k] B[pi(i),pi(k)]  (all_acc_qap's qap; = trace(A P B P^T) = 2 x the first value of score() whenever
 *                A or B is symmetric); -1 if an assign entry of the corner is outside [0, n_b)
 *   planted[b] = sum_{i,k} A[i,k] B[i,k],  na[b] = sum A,  nb[b] = sum B  (score() returns na / 2 and nb / 2)
 * fgnn_qap_improve_cost: cost[b][i][j] = -(sum_k A[i,k] B[pi(k),j]) = (-A P B)[i][j] of improve() with P[i,pi(i)] = 1, fp32 (exact:
 *   |value| <= 256), for ANY 0/1 matrices (no symmetry assumed), written to the n_b x n_b corner of the layout fgnn_lsap_accuracy
 *   reads: row pitch ld >= N, pairs bstride >= N ld apart; nothing outside the corner is written.
 * fgnn_greedy_qap: greedy_qap(A, B, P(assign0), T) for every pair as a chain of launches on `stream` (per round: improve cost ->
 *   the solver of fgnn_lsap_accuracy -> objective -> keep if strictly better), scratch from ws (fgnn_greedy_qap_ws_bytes bytes,
 *   16-byte aligned): no allocation, capturable.  The reference's order of events is kept, its quirk included: s_best starts as the
 *   score of the INITIAL matching, acc_best / T_best = 0 start from the first improve() whose matching is never scored, rounds
 *   i = 0 .. T-1 score improve()'s next matching (as trace(A P B P^T)) and keep it when strictly better.  Outputs, int32: s_best2 =
 *   2 s_best, acc_best, t_best, and perm_best (B, N; optional; not in the reference) = the matching whose score is s_best: assign0
 *   where no round improved -- acc_best then does NOT describe perm_best -- else the matching of round t_best; -1 in the padding.
 *   A pair with n_b = 0 yields zeros. */
#define FGNN_QAP_MAX_N 256
int fgnn_qap_objective(const unsigned *bits1, const unsigned *bits2, const int *assign, const int *nvalid, int B, int N, int *qap,
                       int *planted, int *na, int *nb, void *stream);
int fgnn_qap_improve_cost(const unsigned *bits1, const unsigned *bits2, const int *assign, const int *nvalid, int B, int N, float *cost,
                          long long bstride, int ld, void *stream);
long long fgnn_greedy_qap_ws_bytes(int B, int N);
int fgnn_greedy_qap(const unsigned *bits1, const unsigned *bits2, const int *assign0, const int *nvalid, int B, int N, int T, void *ws,
                    long long ws_bytes, int *s_best2, int *acc_best, int *t_best, int *perm_best /* optional */, void *stream);
/* fgnn_greedy_qap scored against labels (B, N; the section on planted permutations): the same launch sequence and workspace, with a
 * fgnn_count_matches launch after every solver call, so that acc_best counts assign[i] == labels[i] instead of fixed points.  An
 * extension: the reference's greedy_qap has no such parameter (its label is arange).  Every other output is that of fgnn_greedy_qap. */
int fgnn_greedy_qap_labels(const unsigned *bits1, const unsigned *bits2, const int *assign0, const int *labels, const int *nvalid, int B,
                           int N, int T, void *ws, long long ws_bytes, int *s_best2, int *acc_best, int *t_best,
                           int *perm_best /* optional */, void *stream);
/* fgnn_qap_2opt (csrc/qap_2opt.hip): pairwise-exchange local search from `assign`, one workgroup per pair, the whole search in ONE
 * launch.  The semantics are those of scipy.optimize.quadratic_assignment(A, B, method='2opt', options={'maximize': True,
 * 'partial_guess': [[i, assign[i]]]}) (scipy/optimize/_qap.py, _quadratic_assignment_2opt): the objective is
 * S(p) = sum_{i,k} A[i,k] B[p(i),p(k)] on the corner (the qap of fgnn_qap_objective); the pairs (i, j), i <= j, are scanned in the
 * order (0,0), (0,1), .., (0,n-1), (1,1), ..; the first pair whose exchange p(i) <-> p(j) gives a strictly larger S is applied and
 * the scan restarts at (0,0); the search ends after a scan without an improving pair.  "First improving pair in scan order" is the
 * minimum scan position among the pairs with a positive gain, so a round is all gains in parallel and one min-reduction; perm,
 * qap, swaps and nit equal the serial algorithm's.  No symmetry and no zero diagonal is assumed of A or B.  The round loop is a
 * counted loop of min(max_swaps, n_b n_b) rounds (max_swaps < 0: no limit of the caller's): every exchange raises an integer
 * S <= n_b^2 by at least 1, so on valid input the bound does not bind by itself, and no input can make the kernel spin.
 * Outputs per pair (all required):
 *   perm (B, N) int32: the matching, -1 past the corner;  qap int32: S(perm);  swaps int32: the exchanges applied;
 *   nit int64: the evaluations SciPy counts -- an applied pair (i, j) adds its 1-based scan position i n - i (i - 1) / 2 + (j - i) + 1,
 *   the last, fruitless scan n (n + 1) / 2;
 *   status int32: 0 a local optimum; 1 stopped after max_swaps exchanges (perm / qap the state reached, nit without a last scan);
 *   2 `assign` is no permutation of [0, n_b) (an entry outside, or a duplicate): perm = assign (-1 past the corner), qap = -1,
 *   swaps = nit = 0.  A pair with n_b = 0: status 0, qap = 0, nit = 0. */
int fgnn_qap_2opt(const unsigned *bits1, const unsigned *bits2, const int *assign, const int *nvalid, int B, int N, int max_swaps,
                  int *perm, int *qap, int *swaps, long long *nit, int *status, void *stream);
/* fgnn_qap_2opt_seeded: fgnn_qap_2opt over the free rows only -- SciPy's scan over combinations_with_replacement(i_free, 2) with
 * partial_match.  seeds: (B, N) int32 as the seeds section below describes (a negative entry: the row is free).  With f the number
 * of free rows and r(i) the rank of row i among them, an applied pair (i, j) adds r(i) f - r(i) (r(i) - 1) / 2 + (r(j) - r(i)) + 1 to
 * nit and the last, fruitless scan f (f + 1) / 2; the round bound stays min(max_swaps, n_b n_b).  `assign` must be a permutation of
 * [0, n_b) that holds every seed, else status 2 (perm = assign, qap = -1, swaps = nit = 0).  Everything else as fgnn_qap_2opt; the
 * rank table lives in LDS beside the bit matrices. */
int fgnn_qap_2opt_seeded(const unsigned *bits1, const unsigned *bits2, const int *assign, const int *seeds, const int *nvalid, int B, int N,
                         int max_swaps, int *perm, int *qap, int *swaps, long long *nit, int *status, void *stream);

/* ---- decoding a matching on real-weighted pairs (csrc/qap_weighted.hip): the fp32 twin of the section above, for what the
 * reference's all_acc_qap / greedy_qap take besides 0/1 adjacency -- a spectral L = D^-1/2 W D^-1/2, any weighted graph ---------
 * a1 / a2: B pairs of fp32 matrices A resp. B, row pitch ld >= N, pairs gstride >= N ld floats apart (both sides share ld and
 * gstride; a (B, C, N, N) batch passes its channel 0 in place with gstride = C N N).  nvalid, assign and the -1 conventions are
 * those of the bit-word entry points: pair b is the n_b x n_b corner (n_b clamped to [0, N]); NOTHING outside it is read (it may
 * hold NaN); assign entries outside [0, n_b) contribute nothing; the entries inside the corner must be distinct.  No symmetry is
 * assumed.  N <= FGNN_QAPW_MAX_N, B <= 65535; no entry point copies to the host, allocates or synchronises.  Every reduction has a
 * fixed order (no float atomics): a result is bit-identical from run to run.  Where every product and partial sum is exactly
 * representable (integer or dyadic weights with all sums below 2^24 units) every output is exact; otherwise each sum of m terms
 * lies within gamma_m sum |terms| of its exact value, gamma_m = m u / (1 - m u), u = 2^-24 (m = n_b^2; a cost entry: m = n_b).
 *
 * fgnn_qapw_objective, per pair, fp32, every output optional:
 *   qap[b]     = sum_{i,k} A[i,k] B[pi(i),pi(k)]  (all_acc_qap's qap)
 *   trace[b]   = sum_{i,k} A[i,k] B[pi(k),pi(i)] = trace(A P B P^T) = 2 x the first value of score(); != qap when neither matrix is
 *                symmetric
 *   qap / trace are the sentinel -1 if an assign entry of the corner is outside [0, n_b): -1 is then NOT a value (weights may be
 *                negative, so a caller that cannot rule such entries out must look at assign itself)
 *   planted[b] = sum A o B,  na[b] = sum A,  nb[b] = sum B  (score() returns na / 2 and nb / 2)
 * fgnn_qapw_improve_cost: cost[b][i][j] = -(sum_k A[i,k] B[pi(k),j]) = (-A P B)[i][j] of improve(), written to the n_b x n_b corner of
 *   the layout fgnn_lsap_accuracy reads (row pitch cost_ld >= N, pairs bstride >= N cost_ld apart); nothing outside the corner is
 *   written.  A GEMM with a row-gathered right operand on v_mfma_f32_32x32x2_f32 (fp32 in, fp32 accumulate: an fmaf chain over k
 *   upwards), gathered rows staged through LDS; grid (ceil(N/32), ceil(N/128), B).
 * fgnn_greedy_qapw: greedy_qap(A, B, P(assign0), T) for every pair as a chain of launches on `stream` (per round: improve cost ->
 *   the solver of fgnn_lsap_accuracy -> trace -> keep if strictly better), scratch from ws (fgnn_greedy_qapw_ws_bytes bytes, 16-byte
 *   aligned): capturable.  Order of events and quirk as fgnn_greedy_qap.  Outputs: s_best fp32 = trace / 2 (the halving is exact),
 *   acc_best, t_best int32, perm_best (B, N; optional) with the semantics of fgnn_greedy_qap.  A pair with n_b = 0 yields zeros. */
#define FGNN_QAPW_MAX_N 256
int fgnn_qapw_objective(const float *a1, const float *a2, long long gstride, int ld, const int *assign, const int *nvalid, int B, int N,
                        float *qap, float *trace, float *planted, float *na, float *nb, void *stream);
int fgnn_qapw_improve_cost(const float *a1, const float *a2, long long gstride, int ld, const int *assign, const int *nvalid, int B, int N,
                           float *cost, long long bstride, int cost_ld, void *stream);
long long fgnn_greedy_qapw_ws_bytes(int B, int N);
int fgnn_greedy_qapw(const float *a1, const float *a2, long long gstride, int ld, const int *assign0, const int *nvalid, int B, int N, int T,
                     void *ws, long long ws_bytes, float *s_best, int *acc_best, int *t_best, int *perm_best /* optional */,
                     void *stream);
/* the weighted twin of fgnn_greedy_qap_labels: fgnn_greedy_qapw with acc_best counted against labels */
int fgnn_greedy_qapw_labels(const float *a1, const float *a2, long long gstride, int ld, const int *assign0, const int *labels,
                            const int *nvalid, int B, int N, int T, void *ws, long long ws_bytes, float *s_best, int *acc_best,
                            int *t_best, int *perm_best /* optional */, void *stream);
/* fgnn_qapw_2opt (csrc/qap_2opt_weighted.hip): the pairwise-exchange local search of fgnn_qap_2opt on real-weighted pairs, one
 * workgroup per pair, the whole search in ONE launch.  Addressing and input contract are those of the fgnn_qapw_* entry points
 * above; scan order, acceptance of the first improving pair, perm (-1 past the corner), swaps, nit (the same closed formulas) and
 * status (0 a local optimum, 1 stopped at the exchange bound, 2 `assign` is no permutation of the corner: perm = assign, swaps =
 * nit = 0) are those of fgnn_qap_2opt.  There is no qap output: fgnn_qapw_objective on perm is the objective, a fresh sum.
 * With Bp[a][k] = B[p(a)][p(k)] the gain of exchanging i < j is
 *     sum_{k != i,j} (A[i,k] - A[j,k]) (Bp[j,k] - Bp[i,k]) + sum_{k != i,j} (A[k,i] - A[k,j]) (Bp[k,j] - Bp[k,i])
 *     + (A[i,i] - A[j,j]) (Bp[j,j] - Bp[i,i]) + (A[i,j] - A[j,i]) (Bp[j,i] - Bp[i,j]),
 * one fp32 fmaf chain per pair (k ascending, row term before column term, then the two crossings) that depends on (A, Bp, i, j)
 * only; no gain state is carried between rounds; the gain of undoing an exchange is the exact negative of the gain that made it.
 * A pair is accepted iff its fp32 gain is > 0.  On integer or dyadic weights whose partial sums stay below 2^24 units every gain is
 * exact and perm, swaps, nit are SciPy's; on general real weights the trajectory is the kernel's own, the same from run to run.
 * The round loop is a counted loop of max_swaps rounds (max_swaps < 0: n_b n_b); with real weights that default bound can bind
 * (status 1).  N <= 128: A and Bp live in LDS and ws may be NULL / 0 bytes; 128 < N <= 256: Bp lives in ws
 * (fgnn_qapw_2opt_ws_bytes(B, N) bytes, 16-byte aligned), A is read in place. */
long long fgnn_qapw_2opt_ws_bytes(int B, int N);
int fgnn_qapw_2opt(const float *a1, const float *a2, long long gstride, int ld, const int *assign, const int *nvalid, int B, int N,
                   int max_swaps, void *ws, long long ws_bytes, int *perm, int *swaps, long long *nit, int *status, void *stream);
/* fgnn_qapw_2opt_seeded: fgnn_qapw_2opt over the free rows only -- SciPy's scan over combinations_with_replacement(i_free, 2) with
 * partial_match; the SEEDED instantiation of the same kernel body, as fgnn_qap_2opt_seeded is of the bit kernel's.  seeds: (B, N)
 * int32 as the seeds section below describes (a negative entry: the row is free; rows at or beyond n_b are not read).  With f the
 * number of free rows and r(i) the rank of row i among them, an applied pair (i, j) adds r(i) f - r(i) (r(i) - 1) / 2 + (r(j) - r(i))
 * + 1 to nit and the last, fruitless scan f (f + 1) / 2; the round bound stays min(max_swaps, n_b n_b).  The gain of a pair is the
 * chain above over ALL k < n_b: seeded rows and columns are part of the objective, they only never move.  `assign` must be a
 * permutation of [0, n_b) that holds every seed -- so a seed outside [0, n_b), one target for two rows and a start against a seed
 * all give status 2 (perm = assign, swaps = nit = 0).  f <= 1: status 0, perm = assign, swaps = 0, nit = f (f + 1) / 2.  Everything
 * else, the workspace included, as fgnn_qapw_2opt; the rank table (n_b ints) lives in LDS in all four variants. */
int fgnn_qapw_2opt_seeded(const float *a1, const float *a2, long long gstride, int ld, const int *assign, const int *seeds,
                          const int *nvalid, int B, int N, int max_swaps, void *ws, long long ws_bytes, int *perm, int *swaps,
                          long long *nit, int *status, void *stream);
/* fgnn_qapw_faq (csrc/qap_faq.hip): the Fast Approximate QAP algorithm -- Frank-Wolfe on f(P) = tr(A^T P B P^T) over the doubly
 * stochastic matrices, scipy.optimize.quadratic_assignment(method='faq', options={'maximize': True}) without seeds or shuffling --
 * for every pair, as a chain of launches on `stream` with scratch from ws (fgnn_qapw_faq_ws_bytes bytes, 16-byte aligned): no
 * allocation, no host copy, no synchronisation, capturable.  Addressing and input contract are those of the fgnn_qapw_* entry
 * points above; nothing outside a pair's corner is read, in a1, a2 and p0 alike.  The start is p0 ((B, N, N) fp32, optional; that
 * it is doubly stochastic is NOT checked), the permutation matrix of assign0 ((B, N) int32, optional), or with neither the
 * barycenter, every entry 1 / n_b; at most one of the two may be given.  A round:
 *     G = A P B^T + A^T P B          two launches on v_mfma_f32_32x32x2_f32, operands staged through LDS: T = P [B^T | B], then
 *                                    -G = -([A | A^T] [T0; T1]) into the layout fgnn_lsap_accuracy reads; every entry of T is an fmaf
 *                                    chain of n_b terms, every entry of G one of 2 n_b terms; G is fresh from P in every round
 *     q = argmax_Q <G, Q>            the solver of fgnn_lsap_accuracy on -G
 *     a = <G, P> / 2 - <G, Q> + f(Q), b = <G, Q> - 2 f(Q)      (R = P - Q: f(Q + x R) = f(Q) + b x + a x^2), fp64 sums in a fixed order
 *     x = -b / (2 a) if a < 0 and 0 <= -b / (2 a) <= 1, else 1 if -(a + b) < 0, else 0;  P' = x P + (1 - x) Q, formed in fp64 and
 *                                    rounded once to fp32;  the pair stops when ||P - P'||_F / sqrt(n_b) < tol, keeping P'
 * Always maxiter rounds of 4 launches are issued; a pair that has met tol is frozen by a done flag in the workspace: the round's
 * kernels leave it at once and the solver sees n_b = 0 for it.  Then perm = argmax_Q <P, Q> by the same solver on -P.
 * Outputs: perm (B, N) int32, -1 past the corner; nit int32 = the rounds performed (>= 1, as SciPy counts them); status int32: 0
 * stopped on tol, 1 maxiter reached, 2 n_b = 0, assign0 no permutation of [0, n_b), or the solver found no assignment (a NaN inside
 * the corner) -- perm is then assign0 (or -1 without) and nit 0; p_out (optional, (B, N, N) fp32) = the last P, zero around the
 * corner.  There is no objective output: fgnn_qapw_objective on perm is the objective, a fresh sum.  Results are bit-identical
 * from run to run, and a pair's do not depend on the batch around it.  maxiter > 0, tol > 0. */
long long fgnn_qapw_faq_ws_bytes(int B, int N);
int fgnn_qapw_faq(const float *a1, const float *a2, long long gstride, int ld, const float *p0 /* optional, (B,N,N) */,
                  const int *assign0 /* optional, (B,N) */, const int *nvalid, int B, int N, int maxiter, float tol, void *ws,
                  long long ws_bytes, int *perm, int *nit, int *status, float *p_out /* optional, (B,N,N) */, void *stream);

/* ---- seeds: known matches for the QAP solvers (csrc/qap_seeds.hip; SciPy's partial_match, seeded graph matching) ----------------
 * seeds: (B, N) int32; seeds[b][i] = j >= 0 fixes vertex i of graph 1 to vertex j of graph 2, a negative entry leaves row i free
 * (the convention of labels); rows i >= n_b are ignored.  Pair b has m_b seeds and u_b = n_b - m_b free vertices; free rows and
 * free columns are taken in ascending order (SciPy's setdiff1d), seeded rows in ascending order of the row.  A pair is INVALID if a
 * seed lies outside [0, n_b) or two rows share one.  N <= FGNN_SEED_MAX_N; B <= 65535 for the gather and the constant term.  No
 * entry point allocates, copies to the host or synchronises; none uses an atomic: all are capturable and bit-identical from run to run.
 *
 * fgnn_seed_index: one workgroup per pair -> nfree[b] = u_b and nseed[b] = m_b (rows counted, whether the pair is valid or not),
 *   valid[b] (1 / 0), and four (B, N) int32 lists, -1 past their ends and all -1 for an invalid pair: free_a, free_b (the free rows
 *   and columns, ascending), seed_a (the seeded rows, ascending) and seed_b[s] = seeds[seed_a[s]].
 * fgnn_seed_gather: out[b][r][c] = in[b][rows[b][r]][cols[b][c]] for r, c < nfree[b] (clamped to [0, N]) and an exact 0.0f in every
 *   other entry of the contiguous (B, N, N) out; in has the gstride / ld addressing of the fgnn_qapw_* entry points.  Pure data
 *   movement, bit-exact: A22 (free_a, free_a), B22 (free_b, free_b), a float P0 or scores (free_a, free_b).  An index outside
 *   [0, N) reads as zero.
 * fgnn_seed_const: SciPy's const_sum = A21 B21^T + A12^T B12 on the free block, into the contiguous (B, N, N) out (zero around it):
 *   C[r][c] = sum_s A[fa r][sa s] B[fb c][sb s] + A[sa s][fa r] B[sb s][fb c], one fp32 fmaf chain per entry from 0, s ascending, the
 *   row term before the column term.  No symmetry and no zero diagonal is assumed. */
#define FGNN_SEED_MAX_N 256
int fgnn_seed_index(const int *seeds, const int *nvalid /* optional */, int B, int N, int *nfree, int *nseed, int *free_a, int *free_b,
                    int *seed_a, int *seed_b, int *valid, void *stream);
int fgnn_seed_gather(const float *in, long long gstride, int ld, const int *rows, const int *cols, const int *nfree, int B, int N,
                     float *out, void *stream);
int fgnn_seed_const(const float *a1, const float *a2, long long gstride, int ld, const int *free_a, const int *free_b, const int *seed_a,
                    const int *seed_b, const int *nfree, const int *nseed, int B, int N, float *out, void *stream);
/* fgnn_qapw_faq_seeded (csrc/qap_faq.hip): fgnn_qapw_faq with seeds -- SciPy's method='faq' with partial_match -- as one chain of
 * launches: fgnn_seed_index, the gathers of A22 and B22 (and of p0's free block), fgnn_seed_const, then the rounds of fgnn_qapw_faq
 * on A22 / B22 with n_b := u_b, the gradient G = C + A22 P B22^T + A22^T P B22 and the line search
 *     a = (<G,P> - <C,P>) / 2 - (<G,Q> - <C,Q>) + q(Q),  b = (<G,Q> - <C,Q>) - 2 q(Q) + <C,P> - <C,Q>,   q(Q) = tr(A22^T Q B22 Q^T)
 * (fp64 sums in a fixed order; the stop test is over sqrt(u_b)).  C enters the second gradient launch in its EPILOGUE: every entry
 * of G is the finished fmaf chain of 2 u_b terms plus C, one more rounding.  With no seeds C = 0 and every bit is fgnn_qapw_faq's.
 * The start: the barycenter 1 / u_b; assign0, which must hold every seed; or p0 ((B, N, N) fp32, contiguous): its (free_a, free_b) block, or with p0_free != 0 its u_b x u_b corner as it is
 * (a start already in free coordinates: Sinkhorn on the gathered scores).  The assignment of
 * the last P is scattered back: perm[free_a[r]] = free_b[q[r]], perm[i] = seeds[i] on seeded rows, -1 past the corner.
 * status as fgnn_qapw_faq, and: invalid seeds -> status 2, perm = -1, nit 0; assign0 against a seed -> status 2, perm = assign0,
 * nit 0; u_b = 0 < n_b with valid seeds -> perm = seeds, nit 0, status 0.  seeded (optional, int32[B]) = m_b.  p_out (optional) = the
 * last P IN FREE COORDINATES: the u_b x u_b corner of (B, N, N), zero around it.  ws: fgnn_qapw_faq_seeded_ws_bytes bytes. */
long long fgnn_qapw_faq_seeded_ws_bytes(int B, int N);
int fgnn_qapw_faq_seeded(const float *a1, const float *a2, long long gstride, int ld, const int *seeds, const float *p0 /* optional */,
                         int p0_free, const int *assign0 /* optional */, const int *nvalid, int B, int N, int maxiter, float tol, void *ws,
                         long long ws_bytes, int *perm, int *nit, int *status, int *seeded /* optional */,
                         float *p_out /* optional, (B,N,N) */, void *stream);

/* ---- GRAMPA (csrc/grampa.hip): the spectral similarity of Fan, Mao, Wu, Xu, "Spectral graph matching and regularized quadratic
 * relaxations" -- a SCORE producer, X = sum_ij u_i u_i^T H v_j v_j^T / ((lambda_i - mu_j)^2 + eta^2) with A = U Lambda U^T,
 * B = V M V^T -- computed without an eigendecomposition as the solution of the symmetric positive definite system
 *     (T^T T + eta^2 I) X = H,   T(X) = A X - X B,  T^T(S) = A^T S - S B^T       (no symmetry of A, B is assumed)
 * by conjugate gradient, for every pair, as a chain of launches on `stream` with scratch from ws (fgnn_grampa_ws_bytes bytes,
 * 16-byte aligned): no allocation, no host copy, no synchronisation, capturable.  Addressing and input contract are those of the
 * fgnn_qapw_* entry points; nothing outside a pair's corner is read, in a1, a2 and rhs alike.  H = the corner of rhs ((B, N, N) fp32,
 * contiguous) or, with rhs NULL, all ones.  From X = 0, R = P = H, r0 = rr = <H, H>, a round is three launches:
 *     S = A P - P B                      v_mfma_f32_32x32x2_f32, operands staged through LDS: two fmaf chains of n_b terms, k
 *                                        ascending, subtracted once
 *     Q = A^T S - S B^T + eta^2 P        two chains, one subtraction, one fmaf with eta^2 = (float)((double)eta * eta); the block's
 *                                        part of <P, Q> goes to its slot of a partials buffer as an fp64 value (no atomics)
 *     pq = the slots in slot order;  alpha = (float)(rr / pq);  R = fmaf(-alpha, Q, R);  rn = <R, R> (fp64, fixed order);
 *     res = sqrt(rn / r0);  X = fmaf(alpha, P, X);  res < tol: the pair stops, status 0;  else P = fmaf((float)(rn / rr), P, R), rr = rn
 * Breakdown -- pq not a finite number greater than 0, or rn not finite (an inf or NaN inside a corner) -- freezes the pair with
 * status 3 BEFORE X is updated: X stays its last iterate.  Always maxiter rounds are issued; a pair that has stopped is frozen by a
 * done flag in the workspace and left at once by all three kernels.  Then perm = argmax_Q <X, Q> by the solver of fgnn_lsap_accuracy
 * on -X.  standardize != 0: a prologue writes fp32 work copies of both corners, (w - m) / (sqrt(n_b) sd) off the diagonal and 0 on
 * it, m and sd the mean and population standard deviation of the n_b (n_b - 1) off-diagonal corner entries (fp64 sums in a fixed
 * order, the quotient fp64 and rounded once) -- the paper's (A - p) / sqrt(n p (1 - p)) with the empirical p -- and the rounds read
 * those; a side whose sd is not a finite number > 0 (an empty or complete graph, n_b < 2) gives status 2.
 * Outputs (all required): X (B, N, N) fp32 contiguous, exact zeros around the corner (all zeros for status 2); perm (B, N) int32, -1
 * past the corner and everywhere for status 2; nit int32 = the rounds whose update was made; res fp32 = sqrt(<R, R> / <H, H>) of the
 * recurrence's residual after the last update (1 before any, 0 for status 2); status int32: 0 stopped on tol, 1 maxiter reached,
 * 2 n_b = 0, <H, H> = 0, a flat side under standardize, or no assignment found; 3 breakdown.  Every reduction has a fixed order that
 * depends on n_b alone: results are bit-identical from run to run, and a pair's do not depend on B or on the pairs around it.
 * 1 <= N <= FGNN_QAPW_MAX_N, B <= 65535, 1 <= maxiter <= 1024, eta > 0, tol > 0 (finite). */
long long fgnn_grampa_ws_bytes(int B, int N);
int fgnn_grampa(const float *a1, const float *a2, long long gstride, int ld, const float *rhs /* NULL: all ones */, const int *nvalid,
                int B, int N, float eta, int maxiter, float tol, int standardize, void *ws, float *X, int *perm, int *nit, float *res,
                int *status, void *stream);

/* ---- Degree-profile matching (csrc/degree_profile.hip): the baseline of Ding, Ma, Wu, Xu, "Efficient random graph matching via
 * degree profiles" for correlated Erdos-Renyi and Wigner pairs -- a SCORE producer without iteration, tolerance or start, O(n^2 d)
 * work per pair -- as a chain of launches on `stream` with scratch from ws (fgnn_degree_profile_ws_bytes bytes, 16-byte aligned): no
 * allocation, no host copy, no synchronisation, capturable.  Give EITHER a1, a2 (fp32, addressing and input contract of the
 * fgnn_qapw_* entry points; bits1 = bits2 = NULL) OR bits1, bits2 ((B, N, ceil(N/32)) words, the layout of fgnn_qap_objective; a1 =
 * a2 = NULL, gstride and ld unused).  Nothing outside a pair's n_b x n_b corner is read.  Every vertex gets a profile, m values
 * sorted ascending:
 *     fp32 input   { A[i, k] : k != i, k < n_b }, the inputs themselves; m = n_b - 1
 *     bit input    one value per neighbour k of i (m = d_i): ((c_ik n_b (n_b - 1) - r_i S) / (n_b (n_b - 1))) / sqrt(r_i q (1 - q)) =
 *                  (c_ik - r_i q) / sqrt(r_i q (1 - q)) with d the degrees, S their sum, q = S / (n_b (n_b - 1)), r_i = n_b - 1 - d_i,
 *                  c_ik = d_k - 1 - |N(i) & N(k)| (popcounts of the bit rows); the numerator is formed in integers, the rest in fp64,
 *                  rounded once to fp32; r_i = 0 gives 0.  Diagonal bits are ignored; the rows are taken as they are: the formula
 *                  is the paper's for SYMMETRIC input only.
 *     m = 0        the point mass at 0
 * Z(i, j) = the 1-Wasserstein distance of profile i of side 1 (a, length m) and profile j of side 2 (b, length l) over the integer
 * quantile grid: (1 / (m l)) sum_t len_t |a[t / l] - b[t / m]|, t over the segments of [0, m l) cut at the multiples of l and of m
 * in ascending order (ties of break points are integer comparisons), every term an fp64 product of the length and the fp64
 * difference, added to an fp64 sum in that order without fused multiply-add, one fp64 division: the fp64 value is the one a
 * sequential float64 loop forms, its relative error at most (m + l) 2^-53.  X = -(float)Z on the corner, +0.0 around it.
 * perm = argmax_Q <X, Q> by the solver of fgnn_lsap_accuracy on (float)Z.
 * Outputs: X (B, N, N) fp32 contiguous; perm (B, N) int32, -1 past the corner; status int32: 0 computed; 2 n_b < 2, or on bit input
 * a side whose density q is 0 or 1 (or no assignment found); 3 an inf or NaN inside an fp32 corner (the diagonal included) -- for 2
 * and 3 X is all zeros and perm all -1, and the other pairs keep their bits.  profiles (optional, (2, B, N, N) fp32: side, pair,
 * vertex): the sorted values, +inf behind the m-th; counts (optional, (B, 2, N) int32): m; both all +inf / 0 for a row past the
 * corner and for a pair whose status is not 0.  Every value depends on its own pair's corner alone and no launch has atomics:
 * results are bit-identical from run to run, and a pair's do not depend on B, on N or on the pairs around it.
 * 1 <= N <= 256, B <= 65535. */
long long fgnn_degree_profile_ws_bytes(int B, int N);
int fgnn_degree_profile(const float *a1, const float *a2, long long gstride, int ld, const unsigned *bits1, const unsigned *bits2,
                        const int *nvalid, int B, int N, void *ws, float *X, int *perm, int *status, float *profiles /* optional */,
                        int *counts /* optional */, void *stream);

/* ---- Sinkhorn normalisation of scores (csrc/sinkhorn.hip): the doubly stochastic start fgnn_qapw_faq takes from a model's scores,
 * one workgroup per pair, the whole iteration in ONE launch, in the log domain --------------------------------------------------
 * S: B pairs of (N, N) fp32 scores, row pitch ld >= N, pairs pair_stride >= N ld floats apart.  nvalid (optional, int32[B]): pair b
 * is the n_b x n_b corner (n_b clamped to [0, N]); nothing outside it is read (it may hold NaN).  tau > 0 (finite), iters >= 1.
 * With Z = S / tau (a correctly rounded fp32 division), f = 0, g = 0, `iters` times:
 *     f_i = -LSE_j(Z_ij + g_j) over j < n_b,  then  g_j = -LSE_i(Z_ij + f_i) over i < n_b          (every LSE max-subtracted)
 * Outputs (all required): P (B, N, N) fp32, contiguous: P_ij = exp((Z_ij + f_i) + g_j) on the corner and exactly 0.0f around it --
 * every element is written; the columns of the corner sum to 1 up to rounding (g came last);  err[b] fp32 = max_i |sum_j P_ij - 1|,
 * the row sums of the P written, added in a fixed order;  status[b] int32.  -inf entries are legal and give P = 0 there.
 * A pair is degenerate -- status 1, P = 1 / n_b on the corner (the barycenter of fgnn_qapw_faq; nothing for n_b = 0), err = 0 -- if
 * its corner of Z holds a NaN or a +inf, or it has a row or a column without a finite entry, or n_b = 0; every other pair has
 * status 0.  So a following fgnn_qapw_faq always has a valid p0.
 * Every reduction has a fixed order that depends on n_b and N only (no float atomics): the output is bit-identical from run to
 * run, and a pair's does not depend on B or on its place in the batch.  N <= FGNN_QAP_MAX_N.  Z is resident in LDS for
 * N <= FGNN_SINKHORN_LDS_MAX_N (192 x 192 floats = 144 KiB of the CU's 160 KiB, plus 9.5 KiB of vectors); above, S is re-read in
 * place in every pass.  No workspace, no allocation, no host copy, no synchronisation: capturable. */
#define FGNN_SINKHORN_LDS_MAX_N 192
int fgnn_sinkhorn(const float *S, long long pair_stride, int ld, const int *nvalid /* optional */, int B, int N, float tau, int iters,
                  float *P, float *err, int *status, void *stream);

/* ---- spectral input features (csrc/spectral.hip; loaders/data_generator.py:221-232 make_laplacian / make_spectral_feature, the
 * input of QAP_spectralGenerator) ---------------------------------------------------------------------------------------------
 * bits: (G, N, ceil(N/32)) words, bit j of word row i = W[i][j] (the layout of fgnn_expand_adjacency); nvalid (optional, int32[G]):
 * graph g is the n_g x n_g corner (n_g clamped to [0, N]); bits outside it are ignored, they need not be zero.  W need not be
 * symmetric.  out: (G, n_powers, Nout, Nout) fp32, channel p - 1 = L^p with L = D^-1/2 W D^-1/2:
 *   d_i = sum_j W[i][j] over the corner, s_i = 1 / sqrt(d_i) in fp32 (IEEE), s_i = 0 where d_i = 0;
 *   F_1[i][j] = (s_i W[i][j]) s_j (bit-exact against the reference), F_{p+1} = F_p @ L as s_j sum_k (F_p[i][k] s_k) W[k][j] in fp32.
 * Deviation: for a vertex of degree 0 the reference computes inf * 0 = NaN, and every later power is NaN in every entry; here the
 * row and column of an isolated vertex are zeros.  Nout <= N is the row pitch and plane size of out: the top-left Nout x Nout corner
 * of every N x N plane is written (a ragged batch goes out at its largest n_g), with exact zeros outside the n_g x n_g corner.
 * One launch on `stream`, no workspace, no copy to the host, no synchronisation: capturable. */
#define FGNN_SPECTRAL_MAX_N 256
#define FGNN_SPECTRAL_MAX_POWERS 8
int fgnn_spectral_features(const unsigned *bits, const int *nvalid, int G, int N, int n_powers, float *out, int Nout, void *stream);
/* The same features straight into the bf16 input slab of block 1 (csrc/spectral_slab.hip): y is the (G, CP, ldp) slab of
 * fgnn_to_bf16_pad (CP = 2 or 32, row pitch ldr a multiple of 8, channel stride ldp a multiple of 64, y 16-byte aligned),
 * 1 <= n_powers <= min(CP, FGNN_SPECTRAL_MAX_POWERS).  ONE launch writes every byte of the slab: channel p < n_powers = the
 * round-to-nearest-even bf16 of the fp32 value fgnn_spectral_features computes for L^(p+1) (the chain stays in fp32; rounding happens
 * on the way out only); channels >= n_powers, the ragged padding, the pitch columns j >= N and the tail of every channel up to ldp:
 * exact +0.  The slab is byte-identical to fgnn_to_bf16_pad(fgnn_spectral_features(bits, nvalid, ..., Nout = N), ...).
 * No workspace, no copy to the host, no synchronisation: capturable. */
int fgnn_spectral_slab16(const unsigned *bits, const int *nvalid, int G, int N, int n_powers, int CP, int ldr, void *y, long long ldp,
                         void *stream);

/* ---- evaluation (csrc/eval.hip): what the reference's all_losses_acc (toolbox/metrics.py:144-166) and the val_loss behind its
 * ReduceLROnPlateau (models/trainers.py:78-104) take from a batch of raw scores, kept on the device ---------------------------
 * scores: (B, N, N) fp32 raw scores.  nvalid (optional, int32[B]): pair b is the n_b x n_b corner (n_b clamped to [0, N]; NULL:
 * n_b = N); NOTHING outside the corner of scores is read (it may hold NaN).  1 <= N <= FGNN_LSAP_MAX_N.
 *
 * fgnn_eval_pairs, one pass, for every row i < n_b of pair b over the columns j < n_b:
 *   lse           = m + log(sum_j exp(s_ij - m)), m = max_j s_ij, in fp32; the order of the additions is fixed by (N, lane) alone: a
 *                   row has the same bits in any batch, at any position
 *   cost[b][i][j] = lse - s_ij (= -log_softmax), written to the n_b x n_b corner of the layout fgnn_lsap_accuracy reads (row pitch
 *                   cost_ld >= N, pairs cost_bstride >= N cost_ld apart); nothing outside the corner is written
 *   row_ce[b][i]  = lse - s_ii: the reference loss (toolbox/losses.py:20-34), whose target is the identity; labels never enter it
 *   row_hit[b][i] = [argmax_j s_ij == (labels ? labels[b][i] : i)] with the arg-max of fgnn_accuracy_max / fgnn_accuracy_max_labels:
 *                   first maximum on ties, NaN above every number, column 0 for a row of -inf
 *   row_ce (fp32) and row_hit (int32) are (B, N); entries of rows >= n_b are not written.  Non-finite scores propagate by IEEE
 *   rules (a NaN or +inf in a row, or a row of -inf, gives a NaN lse); nothing is special-cased beyond the arg-max rule.
 * fgnn_eval_fold, for the pairs b < live (0 <= live <= B; pairs >= live are ignored entirely -- the surplus of a short last step):
 *   pair_ce[b] (optional, fp64) = sum_i row_ce[b][i] in fp64, pair_max[b] (optional, int32) = sum_i row_hit[b][i]; then ONE
 *   workgroup adds the pairs to the epoch record in pair order, one pair at a time: ce_sum += pair_ce[b], nodes += n_b,
 *   correct_max += pair_max[b], correct_lsap += correct_lsap[b] (optional: the correct[] of fgnn_lsap_accuracy / fgnn_count_matches),
 *   pairs += 1; steps += 1 per call with live > 0.  No floating-point atomics, a fixed order: the record of an epoch is
 *   bit-identical from run to run and does not depend on how its examples were cut into calls.  The record lives in device
 *   memory, zero-initialised (and reset) by its owner.
 * Both are single launches on `stream`: capturable, no allocation, no host copy, no synchronisation. */
typedef struct {
    double ce_sum;          /* sum of the row cross-entropies of every live pair */
    long long nodes;        /* sum of n_b */
    long long correct_lsap; /* matches of the Hungarian matching */
    long long correct_max;  /* arg-max hits */
    long long pairs;        /* live pairs folded */
    long long steps;        /* fgnn_eval_fold calls with live > 0 */
} fgnn_eval_record;
int fgnn_eval_pairs(const float *scores, const int *nvalid /* optional */, const int *labels /* optional */, int B, int N, float *cost,
                    long long cost_bstride, int cost_ld, float *row_ce, int *row_hit, void *stream);
/* fgnn_eval_pairs with the cross-entropy against the labels as well (labels required): row_ce[b][i] = lse - s[i][t_i], t_i =
 * labels[b][i], and 0 for a row whose label lies outside [0, n_b) (no target, see "cross-entropy against labels"); lse, the cost
 * corner and row_hit are those of fgnn_eval_pairs with the same labels, bit for bit. */
int fgnn_eval_pairs_labels(const float *scores, const int *nvalid /* optional */, const int *labels, int B, int N, float *cost,
                           long long cost_bstride, int cost_ld, float *row_ce, int *row_hit, void *stream);
int fgnn_eval_fold(const float *row_ce, const int *row_hit, const int *correct_lsap /* optional */, const int *nvalid /* optional */,
                   int B, int N, int live, double *pair_ce /* optional */, int *pair_max /* optional */, fgnn_eval_record *meter,
                   void *stream);
/* fgnn_eval_fold with one record per bin (1 <= K <= FGNN_MAX_LEVELS records, contiguous): pair_ce / pair_max are those of
 * fgnn_eval_fold, bit for bit; record k then receives the pairs b < live with bin[b] == k (int32[B] on the device) in ascending
 * b, one pair at a time, and its `steps` advances only in a call that added a pair to it.  A pair whose bin lies outside [0, K) is
 * ignored like a pair >= live.  Record k ends with the bytes fgnn_eval_fold leaves after folding just those pairs, in that order,
 * into the same starting record; a record that received no pair is not written.  One workgroup, no floating-point atomics. */
int fgnn_eval_fold_bins(const float *row_ce, const int *row_hit, const int *correct_lsap /* optional */, const int *nvalid /* optional */,
                        int B, int N, int live, const int *bin /* (B) */, int K, double *pair_ce /* optional */,
                        int *pair_max /* optional */, fgnn_eval_record *records /* K records */, void *stream);

/* Rank metrics (csrc/rank.hip): Hits@k and the mean reciprocal rank of the true match, per epoch and per bin.
 * fgnn_eval_ranks, one pass over scores (fp32; row pitch ld >= N, pairs bstride >= N ld apart; nvalid as above, NOTHING outside
 * the n_b x n_b corner is read): for a row i < n_b of pair b with target t = labels ? labels[b][i] : i (labels: optional int32 (B, N))
 *   rank[b][i] = 1 + #{ j < n_b, j != t : column j beats column t }   when 0 <= t < n_b, and 0 otherwise (no target)
 *   column j BEATS column t iff  s_j is NaN and s_t is not,  or  s_j > s_t,  or  j < t and (s_j == s_t or both are NaN)
 * -- the order of the arg-max of fgnn_accuracy_max / fgnn_eval_pairs (first maximum on ties, NaN above every number, the first NaN
 * wins, -0.0 == +0.0): rank == 1 exactly when row_hit of fgnn_eval_pairs is 1.  rank is int32 (B, N); rows >= n_b are not written.
 * Integer counts: exact, whatever the order.  No limit on N beyond the launch grid.
 * fgnn_rank_fold, for the pairs b < live (0 <= live <= B; the others are ignored entirely), with the nk thresholds ks (host memory,
 * 1 <= nk <= FGNN_RANK_MAX_K, positive and strictly increasing; they reach the kernel by value):
 *   pair_hits[b][q] (int32 (B, nk)) = #{i : 1 <= rank <= ks[q]}, pair_rr[b] (fp64) = sum_i 1.0 / rank, pair_rank_sum[b] (int64)
 *   = sum_i rank, pair_targets[b] (int32) = #{i : rank >= 1}, all over the rows i < n_b with a target and each optional; lane l of
 *   a wave adds the rows l, l + 64, ... in ascending order, the wave meets by a butterfly.  Then ONE workgroup adds the pairs to
 *   the records in pair order, one pair at a time: pair b goes to records[bins[b]] (bins: optional int32[B] on the device, with K
 *   contiguous records, 1 <= K <= FGNN_MAX_LEVELS; NULL: record 0, K must be 1); a pair whose bin lies outside [0, K) is added
 *   nowhere.  rr_sum += pair_rr[b], rank_sum, targets, hits[q] likewise, nodes += n_b, pairs += 1; steps += 1 per call that added
 *   a pair to the record.  A record that took no pair is not written.  No floating-point atomics, a fixed order: a record is
 *   bit-identical however its examples were cut into calls, and a binned record has the bytes the plain fold gives for its pairs
 *   alone.  hits[q] for q >= nk stay as they are.
 * Both are single launches on `stream`: capturable, no allocation, no host copy, no synchronisation. */
#define FGNN_RANK_MAX_K 8
typedef struct {
    double rr_sum;          /* sum of 1 / rank over the rows with a target of every live pair */
    long long rank_sum;     /* sum of their ranks */
    long long targets;      /* rows with a target */
    long long nodes;        /* sum of n_b */
    long long pairs;        /* live pairs folded */
    long long steps;        /* fgnn_rank_fold calls that added a pair */
    long long hits[FGNN_RANK_MAX_K];        /* rows with 1 <= rank <= ks[q] */
} fgnn_rank_record;
int fgnn_eval_ranks(const float *scores, long long bstride, int ld, const int *nvalid /* optional */, const int *labels /* optional */,
                    int B, int N, int *rank, void *stream);
int fgnn_rank_fold(const int *rank, const int *nvalid /* optional */, int B, int N, int live, const int *ks, int nk,
                   const int *bins /* optional */, int K, int *pair_hits /* optional */, double *pair_rr /* optional */,
                   long long *pair_rank_sum /* optional */, int *pair_targets /* optional */, fgnn_rank_record *records, void *stream);

/* Decode epochs (csrc/qap_fold.hip): the reference's all_acc_qap(val_loader, ...) and all_greedy_losses_acc over a whole loader
 * (toolbox/metrics.py:168-223), per epoch and per bin, from what the decode launches leave on the device.  0/1 graphs only: qap,
 * planted and refined are the int32 values of the bit-word entry points above (the fp32 objectives of fgnn_qapw_* have a fold of their own, fgnn_qapw_fold below).
 * fgnn_qap_fold, for the pairs b < live (0 <= live <= B; the others are ignored entirely); all inputs int32 on the device:
 *   assign  (B, N): the matching, as fgnn_lsap_accuracy writes it;  qap, planted (B): as fgnn_qap_objective writes them (planted may
 *   be the qap of the labels' matching instead);  perm (B, N) and refined (B): perm_best and s_best2 of fgnn_greedy_qap -- s_best2 =
 *   trace(A P B P^T) = 2 s_best IS the qap of perm whenever A or B is symmetric, so it is stored as it comes and refined_sum /
 *   planted_sum reads like qap_sum / planted_sum; the two are optional and go together;  labels (B, N) optional;  nvalid (B)
 *   optional (n_b clamped to [0, N]).  target(b, i) = labels ? labels[b][i] : i, and none when that lies outside [0, n_b).
 *   Per pair: pair_correct[b] = #{i < n_b : assign[b][i] == target(b, i)}, pair_refined_correct[b] the same of perm (0 without),
 *   pair_ratio[b] (fp64) = (double)qap / (double)planted, the IEEE quotient, when qap >= 0 and planted > 0, else 0; each optional.
 *   Lane l of a wave counts the rows l, l + 64, ...; the wave meets by a butterfly.  Then ONE workgroup adds the pairs to the
 *   record in pair order, one pair at a time:
 *     nodes += n_b, pairs += 1, correct += pair_correct, exact += [pair_correct == n_b], refined_correct += pair_refined_correct;
 *     a pair with qap < 0 (the solver found no finite matching) then adds unmatched += 1 and nothing else; every other pair
 *     qap_sum += qap, planted_sum += planted, recovered += [qap >= planted], with planted > 0: ratio_sum += pair_ratio,
 *     ratio_pairs += 1, and with perm: refined_sum += refined, improved += [refined > qap];
 *   steps += 1 per call that added a pair.  Without perm the three refinement fields are not touched.  A record that took no pair
 *   is not written.  No floating-point atomics, a fixed order: a record is bit-identical from run to run and does not depend on
 *   how its examples were cut into calls.  The record lives in device memory, zero-initialised (and reset) by its owner.
 * fgnn_qap_fold_bins: the same kernel with K contiguous records (1 <= K <= FGNN_MAX_LEVELS): record k receives the pairs b < live
 *   with bin[b] == k (int32[B] on the device) in ascending b and ends with the bytes fgnn_qap_fold leaves after folding just those
 *   pairs into the same starting record; a pair whose bin lies outside [0, K) is added nowhere; the per-pair outputs are those of
 *   fgnn_qap_fold.
 * Both are single launches on `stream`: capturable, no allocation, no host copy, no synchronisation. */
typedef struct {
    double ratio_sum;           /* sum of qap / planted over the matched pairs with planted > 0 */
    long long ratio_pairs;      /* how many pairs entered ratio_sum */
    long long qap_sum;          /* sum of qap over the matched pairs */
    long long planted_sum;      /* sum of planted over the matched pairs */
    long long correct;          /* rows with assign == target */
    long long refined_sum;      /* sum of refined (s_best2: the unit of qap) over the matched pairs */
    long long refined_correct;  /* rows with perm == target */
    long long recovered;        /* matched pairs with qap >= planted */
    long long exact;            /* pairs with every row correct */
    long long improved;         /* matched pairs with refined > qap */
    long long unmatched;        /* pairs with qap < 0 */
    long long nodes;            /* sum of n_b */
    long long pairs;            /* live pairs folded */
    long long steps;            /* fold calls that added a pair */
} fgnn_qap_record;
int fgnn_qap_fold(const int *assign, const int *perm /* optional */, const int *labels /* optional */, const int *qap, const int *planted,
                  const int *refined /* with perm */, const int *nvalid /* optional */, int B, int N, int live,
                  int *pair_correct /* optional */, int *pair_refined_correct /* optional */, double *pair_ratio /* optional */,
                  fgnn_qap_record *meter, void *stream);
int fgnn_qap_fold_bins(const int *assign, const int *perm /* optional */, const int *labels /* optional */, const int *qap,
                       const int *planted, const int *refined /* with perm */, const int *nvalid /* optional */, int B, int N, int live,
                       const int *bin /* (B) */, int K, int *pair_correct /* optional */, int *pair_refined_correct /* optional */,
                       double *pair_ratio /* optional */, fgnn_qap_record *records /* K records */, void *stream);

/* Decode epochs on real-weighted pairs (csrc/qap_fold_weighted.hip): the fp32-objective twins of fgnn_qap_fold(_bins), over what
 * fgnn_qapw_objective, fgnn_greedy_qapw and fgnn_qapw_2opt leave on the device.  assign, perm, labels, nvalid, live, bin, K, the
 * targets, the per-pair counts, the kernel's structure and the rule "a record that took no pair is not written" are those of
 * fgnn_qap_fold; qap, planted, refined (B) are fp32 (refined: the objective of perm in the unit of qap -- 2 s_best of
 * fgnn_greedy_qapw, an exact doubling, or fgnn_qapw_objective on perm).  What differs:
 *   a weighted objective may be negative, so qap < 0 marks nothing: a pair is UNMATCHED iff some assign[b][i], i < n_b, lies outside
 *   [0, n_b) (the wave counts that in its pass over the rows); it adds nodes, pairs, correct and unmatched += 1, nothing else
 *   (not refined_correct either; it cannot be exact);
 *   pair_ratio[b] (fp64) = (double)qap / (double)planted, the IEEE quotient of the two fp32 values converted exactly, when the pair
 *   is matched and planted > 0, else 0; only then the pair enters ratio_sum and ratio_pairs;
 *   recovered += [qap >= planted], improved += [refined > qap]: fp32 comparisons on the stored values;
 *   qap_sum += (double)qap, planted_sum += (double)planted, refined_sum += (double)refined, ratio_sum += pair_ratio: fp64 additions
 *   in pair order, each starting from the record's own value -- so a record has the same bits however its pairs were cut into calls,
 *   and equals a sequential loop over the pairs in IEEE double bit for bit.
 * A NaN objective is not special-cased: it fails every comparison (not recovered, not improved; a NaN planted: no ratio) and
 * propagates into the sums it is added to.  Without perm refined_sum, refined_correct and improved are not touched. */
typedef struct {
    double ratio_sum;           /* sum of qap / planted over the matched pairs with planted > 0 */
    double qap_sum;             /* sum of qap over the matched pairs */
    double planted_sum;         /* sum of planted over the matched pairs */
    double refined_sum;         /* sum of refined over the matched pairs */
    long long ratio_pairs;      /* how many pairs entered ratio_sum */
    long long correct;          /* rows with assign == target */
    long long refined_correct;  /* rows with perm == target */
    long long recovered;        /* matched pairs with qap >= planted */
    long long exact;            /* pairs with every row correct */
    long long improved;         /* matched pairs with refined > qap */
    long long unmatched;        /* pairs with an assign entry outside [0, n_b) */
    long long nodes;            /* sum of n_b */
    long long pairs;            /* live pairs folded */
    long long steps;            /* fold calls that added a pair */
} fgnn_qapw_record;
int fgnn_qapw_fold(const int *assign, const int *perm /* optional */, const int *labels /* optional */, const float *qap,
                   const float *planted, const float *refined /* with perm */, const int *nvalid /* optional */, int B, int N, int live,
                   int *pair_correct /* optional */, int *pair_refined_correct /* optional */, double *pair_ratio /* optional */,
                   fgnn_qapw_record *meter, void *stream);
int fgnn_qapw_fold_bins(const int *assign, const int *perm /* optional */, const int *labels /* optional */, const float *qap,
                        const float *planted, const float *refined /* with perm */, const int *nvalid /* optional */, int B, int N,
                        int live, const int *bin /* (B) */, int K, int *pair_correct /* optional */,
                        int *pair_refined_correct /* optional */, double *pair_ratio /* optional */,
                        fgnn_qapw_record *records /* K records */, void *stream);

/* ---- confident seeds (csrc/seed_select.hip): a seed vector for the seeded solvers from a model's own scores, and its meter ------
 * fgnn_confident_seeds.  scores: B pairs of (N, N) fp32, row pitch ld >= N, pairs bstride >= N ld floats apart; nvalid (optional,
 * int32[B]): pair b is the n x n corner, n = n_b clamped to [0, N]; NOTHING outside the corner is read (it may hold NaN).
 * N <= FGNN_SEED_MAX_N.  Per pair:
 *   rows     c_i = the arg-max column of row i over [0, n), top2_i = the largest value among the OTHER columns, m_i = s[i][c_i] -
 *            top2_i, one fp32 subtraction (+inf for n = 1, and wherever top2_i is -inf).  A row that holds a NaN anywhere in its
 *            corner, or whose maximum is not finite, is never a candidate: m_i = -inf.
 *   columns  r_j = the arg-max row of column j over [0, n); a column that holds a NaN has none.
 *   ties     the smaller index, in both passes; -0.0 == +0.0 (the order of fgnn_accuracy_max and fgnn_eval_ranks).
 *   row i is a CANDIDATE iff r_{c_i} == i and m_i >= min_margin (min_margin >= 0, no NaN).  Mutual best makes the targets distinct
 *   and puts them inside [0, n): the output is always a valid seed vector for fgnn_seed_index.
 *   candidate i is KEPT iff fewer than `count` candidates come before it (count < 0: no cap); k comes before i when m_k > m_i, or
 *   m_k == m_i and k < i.  The rank is a count over the candidates, so nothing depends on a sort's or an atomic's order.
 * Outputs: seeds (B, N) int32 = c_i on kept rows and -1 in every other entry of the N, the padding rows included; nseeds int32[B] =
 * the kept rows; margin (optional, (B, N) fp32) = m_i for i < n and 0 in the padding.  n = 0: all -1, nseeds 0.
 * One launch with one workgroup per pair; the matrix is read once (row reads coalesced along j feed the row and the column pass),
 * every reduction has a fixed order: bit-identical from run to run, a pair's result independent of the batch around it.  No
 * workspace, no allocation, no host copy, no synchronisation: capturable.
 *
 * fgnn_seed_fold, for the pairs b < live (0 <= live <= B; the others are ignored entirely); all inputs int32 on the device: seeds
 * (B, N) optional (NULL: every row is free); assign (B, N): the first matching; perm (B, N) optional: the final matching of the
 * decode chain; labels (B, N) optional; nvalid (B) optional.  target(b, i) = labels ? labels[b][i] : i, none outside [0, n_b).
 * A row i < n_b is SEEDED when seeds[b][i] >= 0, else FREE.  Per pair, m = the seeded rows, then ONE workgroup adds the pairs to the
 * record in pair order:
 *   seeds += m, seed_correct += #{seeded i : seeds[b][i] == target}, free_nodes += n_b - m,
 *   free_correct += #{free i : assign[b][i] == target}, free_refined_correct += #{free i : perm[b][i] == target} (with perm; without
 *   it the field is not touched), clean_pairs += [every seed is right], exact_free += [every free row of perm -- of assign without
 *   perm -- is right], nodes += n_b, pairs += 1; steps += 1 per call that added a pair.  A record that took no pair is not written.
 *   Integer sums: a record does not depend on how its examples were cut into calls.
 * fgnn_seed_fold_bins: the same kernel with K contiguous records (1 <= K <= FGNN_MAX_LEVELS): record k receives the pairs b < live
 *   with bin[b] == k and ends with the bytes fgnn_seed_fold leaves after folding just those pairs into the same starting record; a
 *   pair whose bin lies outside [0, K) is added nowhere.
 * Both are single launches on `stream`: capturable, no allocation, no host copy, no synchronisation. */
typedef struct {
    long long seeds;                /* seeded rows */
    long long seed_correct;         /* seeded rows whose seed is the row's target */
    long long free_nodes;           /* rows without a seed */
    long long free_correct;         /* free rows with assign == target */
    long long free_refined_correct; /* free rows with perm == target */
    long long clean_pairs;          /* pairs whose every seed is right */
    long long exact_free;           /* pairs whose every free row of the final matching is right */
    long long nodes;                /* sum of n_b */
    long long pairs;                /* live pairs folded */
    long long steps;                /* fold calls that added a pair */
} fgnn_seed_record;
int fgnn_confident_seeds(const float *scores, long long bstride, int ld, const int *nvalid /* optional */, int B, int N,
                         int count /* < 0: no cap */, float min_margin, int *seeds, int *nseeds, float *margin /* optional, (B,N) */,
                         void *stream);
int fgnn_seed_fold(const int *seeds /* optional */, const int *assign, const int *perm /* optional */, const int *labels /* optional */,
                   const int *nvalid /* optional */, int B, int N, int live, fgnn_seed_record *meter, void *stream);
int fgnn_seed_fold_bins(const int *seeds /* optional */, const int *assign, const int *perm /* optional */,
                        const int *labels /* optional */, const int *nvalid /* optional */, int B, int N, int live,
                        const int *bin /* (B) */, int K, fgnn_seed_record *records /* K records */, void *stream);

/* ---- random restarts for the FAQ chain (csrc/qap_restarts.hip): R starts per pair, and the best of R results ---------------------
 * fgnn_faq_restart_starts writes starts (B R, N, N) fp32, pair-major (start b R + k is restart k of pair b), in ONE launch with one
 * workgroup per start.  base: (B, N, N) fp32 contiguous, or NULL for the barycenter 1 / n_b; n (optional, int32[B]): the side of
 * pair b's live corner, clamped to [0, N] -- nvalid, or with seeds nfree of fgnn_seed_index and base in free coordinates (what
 * fgnn_qapw_faq_seeded takes with p0_free); pair_index (optional, int64[B]): the pair's index p, b without.  Per (b, k):
 *   k = 0   base's corner bit for bit, or (float)(1.0 / n_b);
 *   k >= 1  (base + K_k) / 2, K_k = SciPy's _doubly_stochastic(U_k) (scipy/optimize/_qap.py; its randomized start when base is
 *           the barycenter): c = 1 / colsum(U), r = 1 / (U c), then c = 1 / (r U), r = 1 / (U c) until every row and column sum of
 *           r_i U_ij c_j lies within 1e-3 of 1, at most 1000 times; SciPy's first test runs on the unscaled U (then K = U): kept.
 *           U_k[i][j] = ((u32 >> 8) + 1) 2^-24, in (0, 1] and exact in fp32, u32 = raw draw t = (k << 32) | (i << 16) | j of pair
 *           stream FGNN_RESTART_STREAM of pair p under `seed` (the pair streams of fgnn_pairgen).  n_b = 1: K = [[1]].
 * Sums, r and c are fp64 in an order fixed by n_b alone; the start is rounded to fp32 once.  A start is a function of (seed, p, k,
 * n_b, base's corner) only -- not of B, R or N -- and bit-identical from run to run.  Outside the corner: exact zeros; n_b = 0: all
 * zeros.  Nothing outside base's corner is read.  U stays in the output buffer and two fp64 N-vectors (with two sums' worth more)
 * in LDS: there is no LDS-resident form and hence no size threshold.  N <= FGNN_QAP_MAX_N, 1 <= R <= FGNN_RESTART_MAX_R, B R <=
 * FGNN_RESTART_MAX_STARTS (the pairs of one fgnn_qapw_faq call).
 *
 * fgnn_qap_best_of_i64 / fgnn_qap_best_of_f32 (int64 objectives of 0/1 graphs, fp32 of weighted ones): qap, status, nit (B R) and
 * perm (B R, N) int32, pair-major as above; veto (optional, int32[B R]): a second status.  Per pair, the CANDIDATES are the
 * restarts k with status != 2, veto != 2 and an objective that is no NaN; the largest objective wins, ties go to the smallest k;
 * without a candidate restart 0 stands in.  perm_out (B, N), qap_out, nit_out, status_out (B) are the winner's entries copied as
 * they are, restart_out (B) int32 its k.  One wave per pair.
 * All three are single launches on `stream`: capturable, no workspace, no allocation, no host copy, no synchronisation. */
#define FGNN_RESTART_STREAM 9
#define FGNN_RESTART_MAX_R 64
#define FGNN_RESTART_MAX_STARTS 65535
int fgnn_faq_restart_starts(const float *base /* optional */, const int *n /* optional */, const long long *pair_index /* optional */,
                            unsigned long long seed, int B, int N, int R, float *starts, void *stream);
int fgnn_qap_best_of_i64(const long long *qap, const int *status, const int *veto /* optional */, const int *nit, const int *perm, int B,
                         int N, int R, int *perm_out, long long *qap_out, int *nit_out, int *status_out, int *restart_out, void *stream);
int fgnn_qap_best_of_f32(const float *qap, const int *status, const int *veto /* optional */, const int *nit, const int *perm, int B, int N,
                         int R, int *perm_out, float *qap_out, int *nit_out, int *status_out, int *restart_out, void *stream);

/* ---- test-only entry points (never on the product path; tests/ and tools/ call them) ---------------------------------------
 * fgnn_debug_mlp_fwd_masks / fgnn_debug_mlp_fwd_x3_masks: fgnn_mlp_fwd / fgnn_mlp_fwd_x3 once more -- the same tile code, the same
 * outputs, bit for bit -- that ALSO exports the ReLU decisions of the conv chain (models/layers.py:129-130), the input of the
 * decision-pinned gradient test (tests/test_gpu_grad_pinned.py): masks[m] is (G, depth - 1, 32, fgnn_tiles_per_graph(N)) words, bit j
 * of word (g, layer, channel, t) = [hidden pre-activation of pixel 32 t + j > 0] as `relu` sees it (bit pattern > 0).  Every
 * depth (depth 1 writes no mask, its buffers may be NULL); words of tiles a ragged launch steps over are not written.  The x3 twin exists for the two-MLP launches (masks1 required).
 * fgnn_debug_matmul_variant: 0 selects the workgroup-per-matrix forward product (N <= 64) that fgnn_chan_matmul_fwd_w replaced, 1
 * (default) the wave-per-matrix kernel, 9 its four-byte-access form; process-global; for the bit-identity tests of the three
 * (tests/test_gpu_kernels.py). */
int fgnn_debug_mlp_fwd_masks(const fgnn_mlp_fwd_args *args, unsigned *masks0, unsigned *masks1 /* nmlp == 2 */, void *stream);
int fgnn_debug_mlp_fwd_x3_masks(const fgnn_mlp_fwd_args *args, unsigned *masks0, unsigned *masks1, void *stream);
int fgnn_debug_matmul_variant(int wave_per_matrix);

#ifdef __cplusplus
}
#endif
#endif /* FGNN_HIP_H */
