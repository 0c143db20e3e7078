/* fsraft.h -- C ABI of libfsraft.so, the MI355X (gfx950) implementation of the RAFT
 * hot path of iwbn/flow-supervisor.
 *
 * Everything here takes plain device pointers, sizes and a hipStream_t; no torch types
 * cross this boundary.  All tensors are fp32.  Every function only enqueues work on
 * `stream` (no allocation, no synchronisation -> safe under hipGraph capture) and
 * returns 0 (FSRAFT_OK), 1 (bad argument) or 2 (launch failed).
 *
 * Threads and devices (the reference's multi-GPU caller is nn.DataParallel, pytorch/train.py:192: one host thread per device in
 * one process).  A call launches on the CALLER's current device -- bind the device of the pointers first (hipSetDevice) -- and
 * on the stream it is given.  Entry points may be called concurrently from several host threads: no per-call state is shared
 * (scratch travels in the call, fsraft_conv_desc.ws; fsraft_conv_workspace and the statistics request of
 * fsraft_conv_forward_stats are per calling thread).  What IS process-wide is configuration -- fsraft_set_arithmetic and the
 * switches of fsraft_tuning.h -- to be set once, before worker threads start.
 *
 * Each entry point names the reference interface it replaces, as file:line under
 * /root/reference.  The Python binding a maintainer would add is shown in
 * INTEGRATION.md; ours lives in flow_supervisor_amd/_lib.py.
 */
#ifndef FSRAFT_H
#define FSRAFT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP_PLATFORM_AMD__
typedef struct ihipStream_t* hipStream_t;
#endif

#define FSRAFT_OK 0
#define FSRAFT_ERR_ARG 1
#define FSRAFT_ERR_LAUNCH 2

/* ---- all-pairs correlation volume + pyramid ---------------------------------------
 * Replaces CorrBlock.__init__ / CorrBlock.corr, pytorch/core/corr.py:13-27, 52-60
 * (torch.matmul + 3x avg_pool2d) and TF calc_all_field, raft/allfield.py:61-92.
 * fmap1, fmap2: [B,C,H,W].  levels[l]: [B*H*W, H>>l, W>>l] (floor), l < num_levels <= 4. */
int fsraft_corr_build(const float* fmap1, const float* fmap2, float* const* levels, int num_levels,
                      int B, int C, int H, int W, hipStream_t stream);

/* Backward of the pooling chain: dlevels[0] += unpool(dlevels[1..]) in place.
 * (autograd of F.avg_pool2d, pytorch/core/corr.py:25-27) */
/* Pyramid of an existing level-0 volume (raft/allfield.py:94-106 build_pyramid; the backward-flow pyramid of the transposed
 * volume at raft/semi.py:250-251): levels[0] = [rows][H2][W2] given, levels[l] = 2x2 averages of levels[l-1], floor sizes. */
int fsraft_corr_pool_pyramid(float* const* levels, int num_levels, int64_t rows, int H2, int W2, hipStream_t stream);
/* TensorFlow semantics of the same pyramid (raft/allfield.py:99-104, tf.nn.avg_pool2d(level 0, s, s, 'SAME'), s = 2, 4, ...):
 * levels[l] = [rows][ceil(H2/2^l)][ceil(W2/2^l)], partial edge windows averaged over their in-range elements, and the
 * forward lookup over a pyramid of those sizes (raft/allfield.py:109-135). */
int fsraft_corr_pool_pyramid_same(float* const* levels, int num_levels, int64_t rows, int H2, int W2, hipStream_t stream);
int fsraft_corr_lookup_fwd_same(float* const* levels, int num_levels, const float* coords, int64_t coords_bs,
                                int64_t coords_cs, int64_t coords_ps, float* out, int nhwc_out, int B, int H, int W,
                                int radius, hipStream_t stream);
int fsraft_corr_unpool_bwd(float* const* dlevels, int num_levels, int B, int H, int W, hipStream_t stream);
/* The backward of the 'SAME' pyramid and of the lookup over it, so that both are differentiable:
 *   fsraft_corr_unpool_same_bwd      dlevels[0] += sum over l >= 1 of (the 'SAME' pooling of level l)^T dlevels[l], in place; sizes
 *                                    and padding as fsraft_corr_pool_pyramid_same, num_levels 1..8, any rows >= 1; a level-0 cell
 *                                    lies in one window per level and receives that window's gradient over its in-range count.
 *                                    Levels >= 1 are only read; a gather without atomics (two calls give the same bits).
 *   fsraft_corr_lookup_bwd_same      fsraft_corr_lookup_bwd onto level gradients of the ceil sizes (4 levels)
 *   fsraft_corr_lookup_dcoords_same  fsraft_corr_lookup_dcoords on levels of the ceil sizes (num_levels 1..4)
 * Bad arguments: FSRAFT_ERR_ARG and nothing is written. */
int fsraft_corr_unpool_same_bwd(float* const* dlevels, int num_levels, int64_t rows, int H2, int W2, hipStream_t stream);
int fsraft_corr_lookup_bwd_same(float* const* dlevels, int num_levels, const float* coords, int64_t coords_bs,
                                int64_t coords_cs, int64_t coords_ps, const float* dout, int nhwc_in, int B, int H, int W,
                                int radius, hipStream_t stream);
int fsraft_corr_lookup_dcoords_same(float* const* levels, int num_levels, const float* coords, int64_t coords_bs, int64_t coords_cs,
                                    int64_t coords_ps, const float* dout, int nhwc_in, float* dcoords, int64_t dbs, int64_t dcs,
                                    int64_t dps, int B, int H, int W, int radius, hipStream_t stream);

/* ---- the same volume in the tiled-row layout (what CorrBlock runs on) ------------------------------------------------
 * Every query i = (b, y, x) owns ONE row of P floats: its pyramid levels back to back, each level cut into 4x4-cell
 * tiles of 64 contiguous bytes (tiles x-fastest; ceil(h_l/4) x ceil(w_l/4) tiles, pad cells beyond the reference's
 * floor-halved h_l x w_l):
 *     cell (y, x) of level l  at  row[off[l] + ((y>>2) * tw[l] + (x>>2)) * 16 + (y&3) * 4 + (x&3)]
 * fsraft_vol_layout fills out[24] = {nlev, H, W, P, h[4], w[4], th[4], tw[4], off[4]}; P % 32 == 0.
 * A (2r+2)^2 lookup window touches ~0.8 KB of 128-byte lines here against ~1.7 KB in the reference's row-major
 * [B*N,1,h_l,w_l] tensors (pytorch/core/corr.py:19-27), which fsraft_corr_build above still produces for API twins. */
int fsraft_vol_layout(int H, int W, int num_levels, int* out);
/* vol [B*H*W][P] <- all-pairs volume + pyramid (pad cells of V: unspecified, never read by the lookup) */
int fsraft_corr_build_tiled(const float* fmap1, const float* fmap2, float* vol, int num_levels, int B, int C, int H, int W,
                            hipStream_t stream);
/* the same from pre-split feature maps f1r, f2r = [B][H*W][C/32] records (fsraft_to_records of the channels-last maps,
 * C % 32 == 0): both operands staged by LDS-DMA on the record GEMM core, 256 queries x an 8x16 target patch per workgroup */
int fsraft_corr_build_rec(const void* f1r, const void* f2r, float* vol, int num_levels, int B, int C, int H, int W,
                          hipStream_t stream);
/* CorrBlock.__call__ (pytorch/core/corr.py:29-50) on that layout; out [B,H,W,L*(2r+1)^2] channels-last; one wave per query.
 * add_grid != 0: `coords` holds the FLOW and the query position is pixel grid + flow (the caller's coords0 + flow,
 * pytorch/core/raft.py:121-131, never materialised) */
int fsraft_corr_lookup_tiled_fwd(const float* vol, int num_levels, const float* coords, int64_t coords_bs, int64_t coords_cs,
                                 int64_t coords_ps, float* out, int B, int H, int W, int radius, int add_grid, hipStream_t stream);
/* d (lookup) / d coords (grid_sampler_2d_backward w.r.t. the grid): dcoords element (b,c,pix) written at
 * dcoords[b*dbs + c*dcs + pix*dps] -- every element, never accumulated; dout [B,H,W,CH] channels-last.  At integer positions
 * the slope is that of the cell to the right / below; taps outside a level are zero and the jump to zero is part of the slope;
 * positions whose window misses a level contribute 0.  With add_grid this is also the gradient w.r.t. the flow.  Enqueues
 * only; radius 3 or 4, num_levels 1..4, B*H*W < 2^31, else FSRAFT_ERR_ARG and nothing is written. */
int fsraft_corr_lookup_tiled_dcoords(const float* vol, int num_levels, const float* coords, int64_t coords_bs, int64_t coords_cs,
                                     int64_t coords_ps, const float* dout, float* dcoords, int64_t dbs, int64_t dcs, int64_t dps,
                                     int B, int H, int W, int radius, int add_grid, hipStream_t stream);
/* Gradient volume of n lookups at once (grid_sampler_2d_backward w.r.t. the volume, pytorch/core/utils/utils.py:57-71, for
 * all iterations of a step): dvol [B*H*W][P] = (or +=, accumulate != 0) sum_t (d out_t / d V)^T dout_t, pad cells zero;
 * dout[t] is [B,H,W,CH] channels-last, coords[t] element (b, c, pix) at coords[t][b*s0 + c*s1 + pix*s2] with
 * (s0, s1, s2) = coords_str[3t .. 3t+2].  n <= 16 per call.  Each row is accumulated in LDS and written once; records != 0:
 * as [32 bf16 hi | 32 bf16 lo] records, the operand format of fsraft_gemm_rec_nt / _tn below.  Only queries [q0, q0 + nq)
 * (nq == 0: all from q0) are built, into dvol rows 0 .. nq-1 -- AlternateCorrBlock's backward walks the queries in chunks so
 * that no O(N^2) buffer exists.  qlist (nullable): caller-owned scratch of 1 + rows unsigned.  With it, one wave per query
 * builds the row from the bounding boxes of its lookups' windows (a few KB of LDS instead of the whole row) and queries whose
 * lookups spread beyond the box are listed there for the row-at-a-time kernel; without it every query takes that kernel.
 * wmask (nullable; needs qlist, records, no accumulate, all queries or a chunk inside one image): the record bitmap of
 * fsraft_corr_bwd_ktiles for the same queries -- only the
 * records either list GEMM reads are written, the rest of dvol stays untouched (it would be zero records nobody reads). */
int fsraft_corr_dvol_build(const float* const* dout, const float* const* coords, const int64_t* coords_str, int n, float* dvol,
                           int num_levels, int B, int H, int W, int radius, int accumulate, int records, int add_grid,
                           int64_t q0, int64_t nq, unsigned* qlist, const unsigned* wmask,
                           hipStream_t stream);
/* Backward of matmul + avg_pool2d chain (pytorch/core/corr.py:21-27, 52-60) without un-pooling the volume gradient:
 *   f2cat [B][C][P]: level-l cell = mean of fmap2 over its 2^l x 2^l pixels (0 in pad cells), so that
 *   dF1[b][c][i] = s * sum_p f2cat[b][c][p] * dvol[b][i][p]   (one NT GEMM, K = P)  and
 *   d2cat[b][p][c] = s * sum_i dvol[b][i][p] * f1[b][i][c]    (one TN GEMM, M = P);
 *   fsraft_corr_dfmap2: d2 [B][H*W][C] = sum_l 4^-l * d2cat[b][cell_l(y>>l, x>>l)][c] over the levels whose cell exists. */
int fsraft_corr_f2cat(const float* fmap2, float* f2cat, int num_levels, int B, int C, int H, int W, hipStream_t stream);
int fsraft_corr_dfmap2(const float* d2cat, float* d2, int num_levels, int B, int C, int H, int W, hipStream_t stream);
/* f2cat directly as records [B][C][P / 32] x ([32 hi | 32 lo] bf16) -- fsraft_corr_f2cat followed by fsraft_to_records in one
 * pass (the plane pooled in LDS by the reference's recursion, corr.py:24-26).  Planes of at most 12288 pixels (H * W);
 * FS_ERR_ARG above that, the caller then takes the two calls. */
int fsraft_corr_f2cat_rec(const float* fmap2, void* f2r, int num_levels, int B, int C, int H, int W, hipStream_t stream);

/* ---- radius-r pyramid lookup --------------------------------------------------------
 * Replaces CorrBlock.__call__, pytorch/core/corr.py:29-50 (+ bilinear_sampler,
 * core/utils/utils.py:57-71) and TF smurf_corr_block, raft/allfield.py:109-135.
 * coords element (b,c,pix) is read at coords[b*bs + c*cs + pix*ps] (c=0: x, c=1: y).
 * out: [B, 4*(2r+1)^2, H, W] (nhwc == 0) or [B, H, W, 4*(2r+1)^2] (nhwc != 0). radius in {3,4}. */
int fsraft_corr_lookup_fwd(float* const* levels, int num_levels, const float* coords, int64_t coords_bs,
                           int64_t coords_cs, int64_t coords_ps, float* out, int nhwc_out, int B, int H, int W,
                           int radius, hipStream_t stream);
/* dlevels[l] += (d out / d V_l)^T dout.  (grid_sampler_2d_backward w.r.t. the volume) */
int fsraft_corr_lookup_bwd(float* const* dlevels, int num_levels, const float* coords, int64_t coords_bs,
                           int64_t coords_cs, int64_t coords_ps, const float* dout, int nhwc_in, int B, int H, int W,
                           int radius, hipStream_t stream);
/* fsraft_corr_lookup_tiled_dcoords on row-major levels[l] [B*H*W, 1, H >> l, W >> l]; dout [B,CH,H,W], or [B,H,W,CH] when
 * nhwc_in != 0.  num_levels 1..4. */
int fsraft_corr_lookup_dcoords(float* const* levels, int num_levels, const float* coords, int64_t coords_bs, int64_t coords_cs,
                               int64_t coords_ps, const float* dout, int nhwc_in, float* dcoords, int64_t dbs, int64_t dcs,
                               int64_t dps, int B, int H, int W, int radius, hipStream_t stream);

/* ---- memory-efficient correlation (no N x N volume) ----------------------------------
 * Replaces alt_cuda_corr.forward / .backward, pytorch/alt_cuda_corr/correlation.cpp:23-54
 * (kernels correlation_kernel.cu:18-119, 122-256).  Same argument meaning:
 * fmap1 [B,H1,W1,C], fmap2 [B,H2,W2,C] channels-last, coords [B,N,H1,W1,2] (x,y; N coordinate sets per query
 * pixel, correlation_kernel.cu:34,59 -- the reference's caller passes N = 1, corr.py:84),
 * corr [B,N,(2r+1)^2,H1,W1], UNSCALED (caller divides by sqrt(C), corr.py:91). */
int fsraft_altcorr_fwd(const float* fmap1, const float* fmap2, const float* coords, float* corr, int B, int N, int H1,
                       int W1, int H2, int W2, int C, int radius, hipStream_t stream);
/* fmap1_grad [B,H1,W1,C] is overwritten; fmap2_grad [B,H2,W2,C] must be zeroed by the caller
 * (it is accumulated with atomics); coords get no gradient (the reference returns zeros).
 * Both entries: radius 3 or 4, B, N, H1, W1, H2, W2 >= 1, 1 <= C <= 256, no null pointer, else FSRAFT_ERR_ARG and nothing
 * is written. */
int fsraft_altcorr_bwd(const float* fmap1, const float* fmap2, const float* coords, const float* corr_grad,
                       float* fmap1_grad, float* fmap2_grad, int B, int N, int H1, int W1, int H2, int W2, int C,
                       int radius, hipStream_t stream);

/* AlternateCorrBlock.__call__ (pytorch/core/corr.py:74-91: four alt_cuda_corr.forward calls, stack, reshape, / sqrt(C)) as ONE
 * launch that writes the channels-last [B,H,W,L*(2r+1)^2] lookup: fmap1 [B,H,W,C], fmap2_levels[l] [B,H>>l,W>>l,C] (the
 * average-pooled maps), coords as in fsraft_corr_lookup_tiled_fwd.  The tile kernel (C a multiple of 64) reads the maps 16
 * bytes at a time: a call whose fmap1 or any level is not 16-byte aligned is served by the wave-per-query kernel. */
int fsraft_altcorr_fused_fwd(const float* fmap1, const float* const* fmap2_levels, int num_levels, const float* coords,
                             int64_t coords_bs, int64_t coords_cs, int64_t coords_ps, int add_grid, float* out, int B, int H, int W,
                             int C, int radius, hipStream_t stream);
/* d (that lookup) / d coords, on the volume that is never formed, V_l[q,y,x] = fmap1[q] . fmap2_l[y,x] / sqrt(C) (the reference's
 * extension returns zeros, alt_cuda_corr/correlation_kernel.cu:307).  fmap1, fmap2_levels, coords and add_grid as
 * fsraft_altcorr_fused_fwd; dout [B,H,W,L*(2r+1)^2] channels-last; dcoords element (b,c,pix) written at
 * dcoords[b*dbs + c*dcs + pix*dps] -- every element, never accumulated: the contract of fsraft_corr_lookup_tiled_dcoords (the
 * cell to the right / below at integer positions, the jump to zero at a level's edge is part of the slope, a level at which
 * |coords 2^-l| >= 30000 contributes 0).  With num_levels = 1 and a pre-pooled map: the per-level coords_grad the extension
 * never computed.  fp32 arithmetic, no atomics: two launches give the same bits.  Enqueues only; radius 3 or 4, num_levels
 * 1..4 (every level at least 1x1), 1 <= C <= 256, B*H*W < 2^31, no null pointer, else FSRAFT_ERR_ARG and nothing is written. */
int fsraft_altcorr_fused_dcoords(const float* fmap1, const float* const* fmap2_levels, int num_levels, const float* coords,
                                 int64_t coords_bs, int64_t coords_cs, int64_t coords_ps, int add_grid, const float* dout,
                                 float* dcoords, int64_t dbs, int64_t dcs, int64_t dps, int B, int H, int W, int C, int radius,
                                 hipStream_t stream);

/* The same lookup with the dot products of a tile of queries against a region of target rows as one small GEMM on the matrix
 * pipe (bf16x3 on pre-split operands, the arithmetic of the volume build): f1r [B][H*W][C/32 records] and f2r_levels[l]
 * [B][(H>>l)*(W>>l)][C/32 records] = fsraft_to_records of the channels-last maps, which are passed as well (window positions
 * outside a tile's region -- flow discontinuities -- are taken from them in fp32).  C % 32 == 0, C <= 256. */
int fsraft_altcorr_mfma_fwd(const void* f1r, const void* const* f2r_levels, const float* fmap1, const float* const* fmap2_levels,
                            int num_levels, const float* coords, int64_t coords_bs, int64_t coords_cs, int64_t coords_ps,
                            int add_grid, float* out, int B, int H, int W, int C, int radius, hipStream_t stream);

/* ---- convex 8x upsampler -------------------------------------------------------------
 * Replaces RAFT.upsample_flow, pytorch/core/raft.py:72-83 and UpsampleConvexWithMask,
 * raft/upsample.py:11-41.  flow element (n,c,pix) at flow[n*bs + c*cs + pix*ps];
 * mask channels-last [N,H,W,576]; up [N,2,8H,8W]. */
int fsraft_upsample_fwd(const float* flow, int64_t flow_bs, int64_t flow_cs, int64_t flow_ps,
                        const float* mask_nhwc, float* up, int N, int H, int W, hipStream_t stream);
/* dmask_nhwc [N,H,W,576], dflow [N,2,H,W]; scratch: N*H*W*18 floats. */
int fsraft_upsample_bwd(const float* flow, int64_t flow_bs, int64_t flow_cs, int64_t flow_ps,
                        const float* mask_nhwc, const float* dup, float* dmask_nhwc, float* dflow, float* scratch,
                        int N, int H, int W, hipStream_t stream);
/* upflow8, pytorch/core/utils/utils.py:80-82 (raft-small). flow [N,C,H,W] -> up [N,C,8H,8W]. */
int fsraft_upflow8_fwd(const float* flow, float* up, int N, int C, int H, int W, hipStream_t stream);
int fsraft_upflow8_bwd(const float* dup, float* dflow, int N, int C, int H, int W, hipStream_t stream);

/* ---- update-block convolutions (implicit GEMM, fp32 MFMA) ----------------------------
 * Replace every nn.Conv2d of pytorch/core/update.py:6-136 together with the cat / ReLU /
 * sigmoid / tanh / GRU-gate elementwise ops around them.  Activations are channels-last
 * with pitch ld (ld % 4 == 0, padding channels zero). */
typedef struct fsraft_conv_desc {
  const float* src[3]; int srcC[3]; int srcld[3]; int nsrc;   /* concatenated inputs            */
  const float* wpk; const float* bias;                        /* packed weights, bias[N] or NULL */
  const float* wpk_split;                                     /* same, packed split-bf16 (modes 10/11), or NULL */
  int B, H, W, KH, KW, N;                                     /* N = output channels             */
  float* dst[3]; int64_t dst_bs[3]; int64_t dst_ps[3]; int64_t dst_cs[3];
  int dst_n0[3]; int dst_acc[3]; int ndst;                    /* output channel ranges           */
  int relu; float alpha;                                      /* y = relu?(alpha*(acc+bias))     */
  int epi;                                                    /* 0 plain, 2 GRU z|r, 3 GRU q     */
  const float* h; int ldh; const float* z; int ldz;
  float* aux1; int ld1; float* aux2; int ld2; int hid;
  const float* pre; int ldpre;                                /* epi 2/3: [M][ldpre] addend to the pre-activation, or NULL */
  const float* rmask[3]; int ldmask[3]; int maskc[3];         /* epi 0, per destination: ReLU-backward mask (zero column
                                                                 j < maskc of the range where rmask[m*ldmask+j] <= 0), or NULL */
  const float* wpk_frag;                                      /* optional: wpk_split re-ordered for direct fragment loads --
                                                                 [k-tile][32-row block][hi k0-15, hi k16-31, lo k0-15, lo k16-31]
                                                                 [lane = 32 * (k half) + row][16 B], rows zero-padded to 32;
                                                                 enables the resident-patch 3x3 kernel (one source, 33..64
                                                                 channels in, N <= 64, large B*H*W).  NULL: never used */
  int pad_h1, pad_w1;                                         /* 0: taps centred (KH/2, KW/2 rows / columns above / left of
                                                                 the output pixel); else 1 + that count -- even kernel sizes:
                                                                 a 2x2 kernel has pad 1 forward and pad 0 in its data gradient */
  float* ws; int64_t ws_floats;                               /* scratch of THIS call for the split-K route at small pixel
                                                                 counts (16-byte aligned, on the device the call runs on, not
                                                                 shared with a call on another stream); NULL: the buffer the
                                                                 calling thread registered with fsraft_conv_workspace, if any */
} fsraft_conv_desc;

int fsraft_conv_ktot(const int* srcC, int nsrc, int KH, int KW);
int fsraft_conv_forward(const fsraft_conv_desc* d, hipStream_t stream);
/* The same convolution; where the chosen kernel's tiles lie inside one image (the resident-patch kernels) and the epilogue is
 * the raw result (one destination, no bias / ReLU / scale / mask / accumulation) it also adds the per-image column sums of the
 * result and of its squares to sum / sq [B * slots][N] (fp32, ZERO on entry; workgroups spread over the `slots` rows of their
 * image) -- the statistics of the InstanceNorm2d that follows the convolution in pytorch/core/extractor.py:13-57, 118-170 --
 * and sets *done = 1; *done = 0: not carried, the caller computes them.  Pass the buffers to fsraft_inorm_relu_cl_fwd
 * (slots = 8, have_sums = *done). */
int fsraft_conv_forward_stats(const fsraft_conv_desc* d, float* sum, float* sq, int slots, int* done, hipStream_t stream);
/* dwpk[Cout][Ktot] += dY^T im2col(src);  dbias (nullable): dbias[co] += sum over pixels of dY[:, co] */
int fsraft_conv_wgrad(const float* dy, int ldy, int Cout, const float* const* src, const int* srcC,
                      const int* srcld, int nsrc, float* dwpk, float* dbias, int B, int H, int W, int KH, int KW,
                      hipStream_t stream);
/* The same reduction over nseg (dY, X) pairs of identical shape -- the iterations of one training step -- in one launch:
 * dwpk += sum_t dY_t^T im2col(X_t).  src[t * nsrc + s] is source s of pair t. */
int fsraft_conv_wgrad_multi(const float* const* dy, int nseg, int ldy, int Cout, const float* const* src,
                            const int* srcC, const int* srcld, int nsrc, float* dwpk, float* dbias, int B, int H, int W,
                            int KH, int KW, hipStream_t stream);
/* mode 0: OIHW -> packed forward; 1: OIHW -> packed data-gradient; 2: packed -> OIHW (+=);
 * modes 10 / 11: as 0 / 1 but every 32-k run stored as [32 hi | 32 lo] bf16 (split-bf16 GEMM core) */
int fsraft_pack_conv_weight(float* w_oihw, float* wpk, int Cout, int Cin, int KH, int KW, const int* srcC,
                            int nsrc, int mode, int accumulate, hipStream_t stream);

/* Batched form: every packed matrix of a module (or, mode 2, every weight gradient) in one launch per 16 jobs, read in place
 * from / written in place to the parameter-shaped tensors -- no torch.cat of fused layers, no channel gather.
 *   w[p], rows[p]   up to three OIHW tensors stacked along the output channels (z|r gates, flow-head|mask-head), all with
 *                   cin_full input channels and kh x kw taps
 *   srcC, srcOff    GEMM source s = input channels [srcOff[s], srcOff[s] + srcC[s]) of those tensors
 *   mode            0 / 1 / 10 / 11 as above; 2: wpk -> w (w = scale * wpk, or += when accumulate); 3: wpk = the rows[p]-long
 *                   vectors w[p] concatenated (fused biases)
 *   flags           bit 0: split pack in fragment order (resident-patch 3x3 kernel, rows zero-padded to a multiple of 32);
 *                   bit 1: w is the [N][C][3][3] weight of a stride-2, pad-1 convolution and the packed matrix is its
 *                   stride-1 2x2 equivalent over the space-to-depth input ([N][4C][2][2], fsraft_space_to_depth2):
 *                   cin_full = C, kh = kw = 2, one source of 4C channels */
typedef struct {
  float* w[3]; int rows[3]; int npiece;
  float* wpk;
  int cin_full, kh, kw;
  int srcC[3], srcOff[3], nsrc;
  int mode, flags;
  float scale; int accumulate;
} fsraft_pack_job;
int fsraft_pack_conv_weights(const fsraft_pack_job* jobs, int njobs, hipStream_t stream);

/* Convolutions with 2 output channels (FlowHead.conv2, pytorch/core/update.py:10: 3x3, hidden -> 2) as per-pixel dot
 * products instead of a padded GEMM tile.  x channels-last [M][ld]; w_oihw [2][C][3][3]; out element (b,o,pix) at
 * out[b*obs + o*ocs + pix*ops].  C % 4 == 0, C <= 512. */
int fsraft_conv_small_fwd(const float* x, int ld, int C, const float* w_oihw, const float* bias, float* out, int64_t obs,
                          int64_t ocs, int64_t ops, int N, int B, int H, int W, int KH, int KW, hipStream_t stream);
/* dwpk[o][tap*ceil32(C) + c] += sum over nseg (dy_t, x_t) pairs and pixels of dy_t[pix][o] * x_t[pix+shift][c];
 * dbias[o] += sum dy (nullable) */
int fsraft_conv_small_wgrad(const float* const* dy, const float* const* x, int nseg, int ldy, int ldx, int C, float* dwpk,
                            float* dbias, int N, int B, int H, int W, int KH, int KW, hipStream_t stream);
/* Data gradient of fsraft_conv_small_fwd (the flow head's 256 -> 2 convolution, pytorch/core/update.py:6-14, as autograd's
 * conv2d backward w.r.t. its input): dx[pix][c] = sum_{o < 2, tap} w_oihw[o][c][tap] * dy[pix - shift(tap)][o], zero where
 * relu_src <= 0 (nullable: the ReLU in front of the convolution, pitch ldm).  dy channels-last with pitch ldy >= 2; dx
 * channels-last with pitch lddx, 16-byte aligned.  C % 4 == 0, C <= 256, N == 2, 3x3. */
int fsraft_conv_small_dgrad(const float* dy, int ldy, const float* w_oihw, float* dx, int lddx, const float* relu_src, int ldm,
                            int C, int N, int B, int H, int W, int KH, int KW, hipStream_t stream);

/* Scratch buffer for the split-K route of the convolutions at small pixel counts (one or two pairs per GPU: the layer's
 * k-tiles are dealt to several workgroups per tile, which park partial tiles here; a second kernel adds them and applies the
 * layer's epilogue).  The library allocates nothing: the caller owns `ws` (16-byte aligned, `floats` fp32) and keeps it alive.
 * Preferred: hand it over per call in fsraft_conv_desc.ws.  This entry point registers a buffer for the CALLING THREAD only
 * (thread-local; NULL clears it) and serves descriptors whose ws is NULL -- a worker thread per device, as in the reference's
 * nn.DataParallel caller (pytorch/train.py:192), registers its own device's buffer and never sees another thread's. */
int fsraft_conv_workspace(float* ws, int64_t floats);

/* ---- arithmetic of the dense contractions -------------------------------------------------------------------------
 * Storage and accumulation are fp32 everywhere.  mode 1 (default): every fp32 product of the GEMM-shaped kernels (volume
 * build and its backward, the update block's / encoders' convolutions, their weight gradients, the GMA GEMMs) is evaluated
 * as three bf16 MFMA products with fp32 accumulation (hi*hi + hi*lo + lo*hi, ~2^-17 relative error per product);
 * mode 0: exact fp32 MFMA (v_mfma_f32_32x32x2_f32, a pure fmaf chain) -- the test / reference mode.  Process-wide; not
 * to be flipped while kernels of another thread are being enqueued.  Replaces nothing in the reference (its
 * torch.backends.cuda.matmul.allow_tf32 default plays the same role on the reference's hardware). */
int fsraft_set_arithmetic(int mode);
int fsraft_get_arithmetic(void);   /* 1 / 0 as above */

/* ---- batched fp32 GEMM (volume backward: autograd of torch.matmul, corr.py:57) ------- */
int fsraft_gemm_f32(const float* A, int64_t lda, int64_t sA, const float* Bm, int64_t ldb, int64_t sB, float* C,
                    int64_t ldc, int64_t sC, int batch, int M, int N, int K, int trans_b, float alpha,
                    int accumulate, hipStream_t stream);

/* C[b][m][n] = alpha * sum_k A[b][k][m] * Bm[b][k][n] (both k-major) on the split-bf16 core. */
int fsraft_gemm_tn_split(const float* A, int64_t lda, int64_t sA, const float* Bm, int64_t ldb, int64_t sB, float* C,
                         int64_t ldc, int64_t sC, int batch, int M, int N, int K, float alpha, int accumulate,
                         hipStream_t stream);

/* ---- GEMM on pre-split ("record") operands -------------------------------------------------------------------------
 * A record is 32 consecutive k of one row as [32 x bf16 hi | 32 x bf16 lo] (hi = bf16(x), lo = bf16(x - hi)): 128 bytes, the
 * bytes the 32 floats took.  Producers split once; the GEMM stages by LDS-DMA (no conversion, no VGPR round trip) and
 * evaluates a_hi b_hi + a_hi b_lo + a_lo b_hi on bf16 MFMA with fp32 accumulation (csrc/gemm_rec.hpp).
 * fsraft_to_records: src [rows][K] fp32 (pitch ld floats) -> dst [rows][ceil(K/32)] records (tail of the last record zero),
 * row pitch dst_ld floats (0 = dense; activation tensors use an ODD number of 128-byte lines per row so that the rows of a
 * k-tile spread over all L2 channels instead of every 4th / 8th line).
 * fsraft_gemm_rec_nt: C[b][m][n] = alpha * sum_k A[b][m][k] B[b][n][k]; A [batch][M] rows of K/32 records (row pitch lda
 * floats), B [batch][N] rows (pitch ldb; 0 = K), K % 32 == 0, sA / sB batch strides in BYTES.  ksplit > 1: K split over workgroups, partial tiles added with fp32
 * atomics (C zeroed first unless accumulate != 0). */
int fsraft_to_records(const float* src, int64_t ld, void* dst, int64_t dst_ld, int64_t rows, int K, hipStream_t stream);
int fsraft_gemm_rec_nt(const void* A, int64_t lda, int64_t sA, const void* Bm, int64_t ldb, int64_t sB, float* C, int64_t ldc,
                       int64_t sC, int batch, int M, int N, int K, float alpha, int ksplit, int accumulate, hipStream_t stream);
/* C[b][m][n] = alpha * sum_k A[b][k][m] B[b][k][n]: both operands k-major, A [batch][K][lda floats] with the records along m,
 * B [batch][K][ldb floats] with the records along n (lda, ldb multiples of 32; K arbitrary).  Fragments are gathered with the
 * transposed LDS read (ds_read_b64_tr_b16). */
int fsraft_gemm_rec_tn(const void* A, int64_t lda, int64_t sA, const void* Bm, int64_t ldb, int64_t sB, float* C, int64_t ldc,
                       int64_t sC, int batch, int M, int N, int K, float alpha, int ksplit, int accumulate, hipStream_t stream);

/* The two contractions above over LISTED k-tiles only (32 k each, ascending): klist[(b * tiles + tile) * kl_stride + i],
 * i < kcount[b * tiles + tile], one list per tile of the sparse operand -- the 128-row tiles of B resp. 128-column tiles of B
 * (kl_by_n != 0) or the 256-row / 256-column tiles of A.  Everything the lists leave out must be zero records: the skipped
 * products would have added +-0.  Replaces nothing in the reference (its autograd contracts the dense gradient volume,
 * pytorch/core/corr.py:52-60); the lists come from fsraft_corr_bwd_ktiles. */
int fsraft_gemm_rec_nt_list(const void* A, int64_t lda, int64_t sA, const void* Bm, int64_t ldb, int64_t sB, float* C, int64_t ldc,
                            int64_t sC, int batch, int M, int N, int K, float alpha, int ksplit, int accumulate, const int* klist,
                            const int* kcount, int kl_stride, int kl_by_n, hipStream_t stream);
int fsraft_gemm_rec_tn_list(const void* A, int64_t lda, int64_t sA, const void* Bm, int64_t ldb, int64_t sB, float* C, int64_t ldc,
                            int64_t sC, int batch, int M, int N, int K, float alpha, int ksplit, int accumulate, const int* klist,
                            const int* kcount, int kl_stride, int kl_by_n, hipStream_t stream);
/* Which k-tiles of the volume-backward GEMMs the step's lookups can reach, from their coordinates alone (arguments as
 * fsraft_corr_dvol_build; n <= 16): nt_list [B][ceil(H*W / 128)][nt_stride >= P / 32] + nt_count = records per 128-query tile
 * (dF1 = s * F2cat . dV^T with dV as the B operand, kl_by_n = 1); tn_list [B][ceil(P / 256)][tn_stride >= ceil(H*W / 32)] +
 * tn_count = 32-query blocks per 256-cell tile (d2cat = s * dV^T . f1 with dV as the A operand); tn_bits: scratch of
 * B * ceil(H*W / 32) * ceil(ceil(P / 256) / 32) unsigned.  wmask (nullable): [B][ceil(H*W / 32)][ceil(P / 1024)] unsigned, bit r of
 * a 32-query block = record r of its rows is read by one of the two list GEMMs; handed to fsraft_corr_dvol_build, the gradient
 * volume is then written there and nowhere else.  P = the row length of fsraft_vol_layout.  nq > 0: one list set for the chunk
 * of queries [q0, q0 + nq) of one image (the chunked backward of AlternateCorrBlock): read B = 1 and H*W = nq above. */
int fsraft_corr_bwd_ktiles(const float* const* coords, const int64_t* coords_str, int n, int num_levels, int B, int H, int W,
                           int radius, int add_grid, int64_t q0, int64_t nq, int* nt_list, int* nt_count, int nt_stride, unsigned* tn_bits,
                           int* tn_list, int* tn_count, int tn_stride, unsigned* wmask, hipStream_t stream);

/* ---- GMA variant (config 5) --------------------------------------------------------------
 * Attention.forward, pytorch/core/gma.py:54-76: sim = scale * q k^T runs on fsraft_gemm_f32 (trans_b), then this
 * in-place row softmax over the last dimension (rows = B*heads*N, n = N; rows up to 16384 floats are staged in LDS). */
int fsraft_softmax_rows(float* S, int64_t rows, int n, hipStream_t stream);
/* dA <- A * (dA - rowsum(dA * A))  (softmax backward, in place over dA) */
int fsraft_softmax_rows_bwd(const float* A, float* dA, int64_t rows, int n, hipStream_t stream);
/* The same softmax (gma.py:71-74) with the probabilities written over the logits as RECORDS ([32 bf16 hi | 32 bf16 lo] per 32
 * columns: the operand form of fsraft_gemm_rec_nt / _tn): for n % 32 == 0 (n <= 16352) the record row is as long as the fp32
 * row, so the map exists once.  The backward reads those records (a = hi + lo) and turns the fp32 gradient dA into the records
 * of dS = A * (dA - rowsum(dA * A)) in place (n <= 8160). */
int fsraft_softmax_rows_rec(float* S, int64_t rows, int n, hipStream_t stream);
int fsraft_softmax_rows_bwd_rec(const void* A_records, float* dA, int64_t rows, int n, hipStream_t stream);
/* RelPosEmb.forward + Attention.forward with --position_only / --position_and_content, pytorch/core/gma.py:6-31, 62-74: the
 * row softmax above with the relative-position logits added while the row is in LDS.  n = h * w; row r of S [rows][n] is query
 * (x, y) = ((r % n) / w, (r % n) % w), so rows is a multiple of n; G [rows][ldg] (ldg >= 2h + 2w - 2) holds the query's scores
 * against the stacked table slices, G = scale * q . [rel_height.weight[P-h : P+h-1] ; rel_width.weight[P-w : P+w-1]]^T, and
 *   logit[r][u*w + v] = (content ? S[r][u*w + v] : 0) + G[r][u - x + h - 1] + G[r][(2h - 1) + v - y + w - 1].
 * content == 0 (position_only): S is written without being read.  records != 0: the probabilities leave as records, as
 * fsraft_softmax_rows_rec (n % 32 == 0, S 16-byte aligned), bit for bit the records of the dense result.
 * Limits (FS_ERR_ARG beyond them; one row plus its h + w bias values in the 64 KB of LDS a launch gets without an opt-in, less
 * 16 bytes of static reduction words): 4 * ceil4(n) + 4 * (h + w) <= 65520. */
int fsraft_softmax_rows_pos(float* S, const float* G, int64_t ldg, int64_t rows, int n, int h, int w, int content, int records,
                            hipStream_t stream);
/* Its backward (autograd of gma.py:6-31, 62-74): dA <- dS = A * (dA - rowsum(dA * A)) in place (records != 0: A is read as
 * records and dS written as records, as fsraft_softmax_rows_bwd_rec; A and dA 16-byte aligned, n % 32 == 0), and the gradient of
 * G, every one of the ldg columns of a row written (no memset needed):
 *   dG[r][u - x + h - 1] = sum_v dS[r][u*w + v],  dG[r][(2h - 1) + v - y + w - 1] = sum_u dS[r][u*w + v],  0 elsewhere,
 * summed in a fixed order without atomics.  Limit: 8 * ceil4(n) + 4 * (h + w) <= 65520 (two rows and the h + w sums in LDS). */
int fsraft_softmax_rows_pos_bwd(const void* A, float* dA, float* dG, int64_t ldg, int64_t rows, int n, int h, int w, int records,
                                hipStream_t stream);
/* Aggregate.forward, gma.py:113: dst = x + gamma[0] * y with gamma a device scalar (the nn.Parameter). */
int fsraft_gma_mix_fwd(const float* x, int ldx, const float* y, int ldy, const float* gamma, float* dst, int ldd,
                       int64_t M, int C, hipStream_t stream);
/* d = dL/d dst:  dx += d;  dy = gamma * d;  dgamma[0] += sum(d * y) */
int fsraft_gma_mix_bwd(const float* d, int ldd, const float* y, int ldy, const float* gamma, float* dx, int ldx,
                       float* dy, int lddy, float* dgamma, int64_t M, int C, hipStream_t stream);

/* ---- normalisation + ReLU around the encoder convolutions (callers of the path) ------------------------------
 * pytorch/core/extractor.py:6-57: relu(norm(conv(x))) with norm = InstanceNorm2d (feature net) or a frozen
 * BatchNorm2d (context net).  The convolutions stay MIOpen; these fuse what surrounds them.  NCHW, one (n,c) plane
 * of HW floats per workgroup; stats[plane] = (mean, rstd). */
int fsraft_inorm_relu_fwd(const float* x, float* y, float* stats, int64_t planes, int HW, float eps, int relu, hipStream_t stream);
int fsraft_inorm_relu_bwd(const float* g, const float* x, const float* stats, float* dx, int64_t planes, int HW, int relu,
                          hipStream_t stream);
/* y = relu?(x * scale[c] + shift[c]);  backward: dx = g' * scale[c], dsum_g[c] += sum g', dsum_gx[c] += sum g' * x */
int fsraft_affine_relu_fwd(const float* x, const float* scale, const float* shift, float* y, int64_t planes, int C, int HW,
                           int relu, hipStream_t stream);
int fsraft_affine_relu_bwd(const float* g, const float* x, const float* scale, const float* shift, float* dx, float* dsum_g,
                           float* dsum_gx, int64_t planes, int C, int HW, int relu, hipStream_t stream);

/* ---- sequence loss (a step next to the path: pytorch/train.py:60-96) -----------------------------------------------
 * loss = sum_i weights[i] * mean(mask * sqrt((pred_i - gt)^2 + eps^2)), mask = valid >= 0.5 && |gt| < max_flow, over n
 * predictions [B,2,H,W] in one pass; dpred[i] (nullable) receives d loss / d pred_i; out[0] = loss, out[1..5] = EPE sum,
 * counts < 1 / 3 / 5 px and valid (> 0.5) count of prediction metric_idx.  gt / valid may be NULL (zero flow / all valid).
 * out[6] must be zero on entry (or hold sums: the launch adds to it, once, the float64 total of its workgroups' partial sums,
 * so a result does not depend on the order the workgroups retire in).  Launches on one device must not overlap: one stream. */
int fsraft_sequence_loss(const float* const* pred, float* const* dpred, const float* weights, int n, int metric_idx,
                         const float* gt, const float* valid, float max_flow, float eps, int B, int H, int W, float* out,
                         hipStream_t stream);

/* ---- flow losses of the TensorFlow trainers (raft/loss.py FlowLossL1 / FlowLossL2 / FlowLossRobust over a sequence of
 * predictions, raft/semi.py:373-405, 447-471; raft/metric.py EPE; csrc/flow_loss.hip) -----------------------------------
 * One launch for n (1..32) predictions against one target.  Per pixel and channel, d = pred_i - target:
 *   m = mask * (sqrt(t0^2 + t1^2) < max_flow)   (the mask is a factor, not thresholded; the comparison is strict)
 *   psi(d) = |d| (L1), d^2 (L2), sqrt(d^2 + eps^2) (ROBUST)
 *   out[0] = scale * sum_i weights[i] * sum m * psi(d)                                   (written, not added to)
 *   dpred[i] = scale * weights[i] * m * psi'(d), every element written (+0 where m == 0); dpred or dpred[i] may be NULL
 *   sample_stats[b] = (sum mask * |pred[metric_idx] - target|_2, sum mask) of sample b (NULL: none; the cut does not enter)
 *   pixel_out[b][y][x] = m * (psi(d_0) + psi(d_1)) / 2, contiguous [B][H][W], only with n == 1 (NULL: none)
 * scale = 1 / (2 B H W): Keras' mean over the channel axis and SUM_OVER_BATCH_SIZE; scale = 1 / 2: the gradient of the SUM of a
 * Reduction.NONE loss.  Strides are in elements: (batch, channel, pixel) shared by all predictions and their gradients, a triple
 * of its own for the target, (batch, pixel) for the mask; pixel y * W + x of sample b, channel c is at b * bs + (y * W + x) * ps
 * + c * cs.  [B,H,W,2]: (2HW, 1, 2); [B,2,H,W]: (2HW, HW, 1); a [B,H,W,3] ground truth in place: target (3HW, 1, 3), mask =
 * base + 2 with (3HW, 3).  target NULL: zero flow, no cut; mask NULL: ones.  Both floats of a pixel are one 8-byte access when
 * cs == 1, bs and ps are even and every base is 8-byte aligned, two 4-byte accesses otherwise.
 * workspace: fsraft_flow_loss_workspace_bytes(B, H, W) bytes (>= 64; 1 = bad sizes), 8-byte aligned, whose first 4 bytes are
 * zero before the first launch that uses it; every launch leaves them zero, so a workspace is reusable by launches that do not
 * overlap.  Overlapping launches (two streams) take two workspaces; no other state is shared.  The sums are the float64 total,
 * in workgroup order, of per-workgroup fp32 partial sums: the same bits for the same inputs.
 * FSRAFT_ERR_ARG before any HIP call for: n outside 1..32, an unknown penalty, NULL pred / pred[i] / weights / out / workspace,
 * a workspace too small or misaligned, pixel_out with n != 1, sample_stats with metric_idx outside [0, n), B > 65535. */
#define FSRAFT_FLOW_L1 0
#define FSRAFT_FLOW_L2 1
#define FSRAFT_FLOW_ROBUST 2
int fsraft_flow_loss_workspace_bytes(int B, int H, int W);
int fsraft_flow_loss(const float* const* pred, float* const* dpred, const float* weights, int n,
                     int64_t pred_bs, int64_t pred_cs, int64_t pred_ps,
                     const float* target, int64_t target_bs, int64_t target_cs, int64_t target_ps,
                     const float* mask, int64_t mask_bs, int64_t mask_ps,
                     int penalty, float max_flow, float eps, float scale, int B, int H, int W,
                     float* out, float* sample_stats, int metric_idx, float* pixel_out,
                     void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* ---- warm start (a step next to the path: pytorch/core/utils/utils.py:26-54 forward_interpolate, called between the
 * frames of a sequence at pytorch/evaluate.py:43) -------------------------------------------------------------------
 * flow [2][H][W] (dx plane, dy plane) at the resolution the flow lives on: every vector is carried to (x + dx, y + dy),
 * landings outside the open rectangle (0, W) x (0, H) are dropped, and every grid node takes the vector of the nearest
 * landed point (float64 distances, as scipy's griddata(method="nearest")); all zero when nothing lands.  out != flow. */
int fsraft_forward_interpolate(const float* flow, float* out, int H, int W, hipStream_t stream);

/* ---- validation metrics (a step next to the path: pytorch/evaluate.py:117-124 validate_sintel / validate_chairs and
 * :150-165 validate_kitti, which reduce on the host after a device -> host copy of every prediction) --------------------
 * One pass over B predictions against ground truth.  pred, gt: [B][2][H][W] views, valid: [B][H][W] (NULL: every pixel is
 * valid); strides in elements, the x stride is 1, nothing else is assumed (pred is typically InputPadder.unpad of a padded
 * prediction: a 4-byte aligned base and a row stride other than W).  Per pixel, in the reference's fp32 with every operation
 * rounded on its own: d = pred - gt, epe = sqrt(d0*d0 + d1*d1), mag = sqrt(g0*g0 + g1*g1); a pixel counts when
 * valid >= 0.5; it is an outlier when epe > 3 && epe / mag > 0.05 (mag == 0 gives inf, as in the reference).  Sums are fp64.
 *   sample_stats[b] (overwritten) = { n valid, sum epe, n(epe < 1), n(epe < 3), n(epe < 5), n outliers, 0, 0 }
 *   acc (nullable, accumulated into in stream order, ascending b): acc[0..5] += sample_stats[b][0..5]; for a sample with a
 *   valid pixel acc[6] += its mean epe (evaluate.py:158) and acc[7] += 1.
 * No atomics: bit-identical from run to run, and sample b of a batch gives the bits it gives alone.  scratch: at least
 * fsraft_flow_metrics_scratch_bytes(B, H, W) bytes, 8-byte aligned like sample_stats and acc; nothing to initialise.
 * fsraft_flow_metrics_scratch_bytes returns the size (a multiple of 64), or FS_ERR_ARG (1) for B, H or W below 1 or
 * H * W beyond 2^31 - 1. */
int fsraft_flow_metrics_scratch_bytes(int B, int H, int W);
int fsraft_flow_metrics(const float* pred, int64_t pred_bs, int64_t pred_cs, int64_t pred_rs,
                        const float* gt, int64_t gt_bs, int64_t gt_cs, int64_t gt_rs,
                        const float* valid, int64_t valid_bs, int64_t valid_rs, int B, int H, int W,
                        double* sample_stats, double* acc, void* scratch, int64_t scratch_bytes, hipStream_t stream);

/* ---- flow visualisation and submission encoding (a step next to the path; csrc/flow_viz.hip) -----------------------------
 * What the reference's inference scripts do on the host after `.cpu().numpy()`: the Middlebury colour wheel of
 * pytorch/core/utils/flow_viz.py, the HSV coding of util/visualize.py:5-27 and the 16-bit KITTI encoding of
 * pytorch/raft_utils/frame_utils.py:121-125.  flow: a [B][2][H][W] fp32 view, strides in elements, x stride 1, nothing else
 * assumed (the un-padded view of a padded prediction is read in place); outputs are contiguous, every element written.  All
 * arithmetic is fp32 with every operation rounded on its own.  No allocation, no synchronisation, no device -> host read;
 * every launch goes on `stream`, so a call can be captured in a graph.  Bit-identical from run to run, and sample b of a batch
 * gives the bits it gives alone.  FSRAFT_ERR_ARG, before any HIP call, for a null flow or output, B, H or W below 1, B beyond
 * 65535, H * W beyond 2^31 - 1, a misaligned pointer and the argument values named below.
 *
 * fsraft_flow_rad_max (flow_viz.py:123-128): rad_max[b] = the maximum over the sample's finite pixels (both components
 * finite) of sqrtf(u*u + v*v); 0 for a sample without one.  clip > 0: u and v are first clamped to [0, clip] -- the LOWER
 * BOUND 0 IS THE REFERENCE'S QUIRK, np.clip(flow_uv, 0, clip_flow), kept here: negative components vanish (by comparison, as np.clip: a component of -0.0 stays
 * -0.0, and keeps its end of the wheel).  clip == 0: no clamp.  A negative, NaN or infinite clip is refused.  rad_max (float[B], device) is zeroed by the call itself and then
 * raised with an atomic maximum on the bit pattern of the non-negative float: a maximum is order-independent.
 *
 * fsraft_flow_wheel (flow_viz.py:70-106, 129-132): out uint8 [B][H][W][3], RGB (bgr 1: BGR).  Per pixel, after the same
 * clamp: den = rad_max[b] + 1e-5f (rad_max non-NULL) or the host scalar `scale` (rad_max NULL; not positive, NaN or infinite
 * is refused); u' = u / den, v' = v / den, rad = sqrtf(u'*u' + v'*v'); a = atan2f(-v', -u') / pi; fk = (a + 1) / 2 * 54;
 * k0 = floor(fk), f = fk - k0, k0 then clamped to [0, 54], k1 = k0 + 1 with 55 wrapping to 0; per channel
 * col = (1 - f) * wheel[k0] / 255 + f * wheel[k1] / 255; rad <= 1: col = 1 - rad * (1 - col), else col = 0.75 * col;
 * out = floor(255 * col).  wheel is the 55-entry table of make_colorwheel (RY 15, YG 6, GC 4, CB 11, BM 13, MR 6).  With
 * scale 1 this is flow_uv_to_colors(u, v), the only way into the 0.75 branch.  A pixel with a non-finite component is painted
 * (0, 0, 0) and takes no part in the maximum; the reference has no rule there (a NaN poisons np.max and the whole picture).
 * The reference evaluates everything from the table lookup on in float64; a value that lands within rounding of an integer
 * may come out one level off (tests/test_flow_viz_gpu.py bounds how many).
 *
 * fsraft_flow_hsv (util/visualize.py:5-27): rho = sqrtf(x*x + y*y); phi = atan2f(y, x), plus 2 pi where negative;
 * max_mag > 0: s = clamp(rho / max_mag, 0, 1); max_mag == 0: s = rho / rad_max[b] (from fsraft_flow_rad_max with clip 0; a
 * maximum of 0 is replaced by 1; rad_max NULL is refused); a negative, NaN or infinite max_mag is refused.  h = phi / (2 pi),
 * v = 1, and RGB as tf.image.hsv_to_rgb has it: d_r = clamp(|6h - 3| - 1), d_g = clamp(2 - |6h - 2|), d_b = clamp(2 - |6h - 4|),
 * each to [0, 1], c = ((d - 1) * s + 1) * v.  out: fp32 [B][H][W][3] in [0, 1] (out_u8 0) or uint8, (uint8)(255 * c)
 * truncated as extract_flow.py:154 does (out_u8 1).  A pixel with a non-finite component is (0, 0, 0).  TensorFlow exists on
 * no machine this runs on: the formula is restated from its source, and parity with TensorFlow is unpinned.
 *
 * fsraft_flow_kitti16 (frame_utils.py:122-124): out uint16 [B][H][W][3] = (64 * u + 32768, 64 * v + 32768, valid) in fp32,
 * truncated toward zero and clamped to [0, 65535] (NaN: 0); the reference's astype(np.uint16) wraps or is undefined from
 * |flow| >= 512 on.  The third channel is 1, or valid >= 0.5 from a [B][H][W] view with unit x stride (NULL: all ones).
 * The order (u, v, valid) is the file's R, G, B. */
int fsraft_flow_rad_max(const float* flow, int64_t flow_bs, int64_t flow_cs, int64_t flow_rs, int B, int H, int W,
                        float clip, float* rad_max, hipStream_t stream);
int fsraft_flow_wheel(const float* flow, int64_t flow_bs, int64_t flow_cs, int64_t flow_rs, int B, int H, int W,
                      float clip, const float* rad_max, float scale, int bgr, uint8_t* out, hipStream_t stream);
int fsraft_flow_hsv(const float* flow, int64_t flow_bs, int64_t flow_cs, int64_t flow_rs, int B, int H, int W,
                    const float* rad_max, float max_mag, int out_u8, void* out, hipStream_t stream);
int fsraft_flow_kitti16(const float* flow, int64_t flow_bs, int64_t flow_cs, int64_t flow_rs,
                        const float* valid, int64_t valid_bs, int64_t valid_rs, int B, int H, int W, uint16_t* out,
                        hipStream_t stream);

/* ---- unsupervised (SMURF) loss (a step next to the path: raft/unsup_loss.py UnsupervisedLoss over
 * raft/smurf_models/smurf_utils.py: compute_range_map, census_loss, first/second_order_smoothness_loss) -------------------
 * PyTorch layout: images [B][3][.][.] in [0,1], flows [B][2][H][W] with channel 0 = x (the reference's tf.reverse to
 * (row, col) is absorbed).  Every view comes with strides in elements and a unit x stride.  An image argument is a frame of
 * Hf x Wf of which sample b uses the H x W window at (crop_yx[2b], crop_yx[2b+1]) = (y, x); crop_yx is a HOST array of
 * 2 * B ints (NULL: all zero), read during the call and passed to the kernels by value, so a captured call keeps its
 * offsets.  Per-pixel arithmetic is fp32, sums are fp64 in workgroup order through `scratch` (8-byte aligned, at least the
 * _scratch_bytes companion's size, nothing to initialise); results are bit-identical from run to run, and the per-pixel
 * outputs of sample b do not depend on the rest of the batch.  No allocation, no synchronisation.  FSRAFT_ERR_ARG, before any
 * HIP call, for a null pointer, B, H or W below 1 (census: H or W below 7; smoothness: H or W <= order), H * W or Hf * Wf beyond
 * 2^31 - 1, a window outside the frame, a misaligned fp64 pointer or too little scratch.
 *
 * fsraft_range_map: out [B][H][W] = R[p] = the bilinear weights of every q + flow(q) that land on p (taps outside the image
 * and zero weights are skipped), summed exactly in 64-bit fixed point (units of 2^-32; integer atomics commute) and rounded
 * to fp32 once; clip != 0 gives min(R, 1), the 'wang' mask of the opposite direction (occlusions_are_zeros).
 *
 * fsraft_census_fwd: img2 is a frame; img1 is one too when img1_frame != 0 (the same offsets), else the H x W image i itself.
 * Iw[p] = bilinear(img2, p + crop + flow(p)) with zero taps outside the frame, valid[p] = that point
 * inside [0, Wf-1] x [0, Hf-1], M = mask * valid (mask [B][H][W], NULL: 1) and zero on a 3-pixel border;
 * gray = 255 * (0.2989 R + 0.5870 G + 0.1140 B), c_k = d / sqrt(0.81 + d^2) over the 7 x 7 patch, ham = sum_k u^2 / (0.1 + u^2)
 * with u = cA_k - cB_k, l = (ham + 0.01)^0.4.  out[0] = sum l * M / out[1], out[1] = sum M + 1e-6 * B * H * W.  Saved for the
 * backward, [B][H][W] each: grayB = gray(Iw), hplane = M * 0.4 * (ham + 0.01)^-0.6.
 * fsraft_census_bwd: dflow [B][2][H][W] (every element written) = up[0] / den[0] * dL/dgray(Iw) * d gray(Iw) / d(x, y), the
 * resampler's coordinate gradient with the zero-tap rule; up (fp32) and den (fp64, out + 1 of the forward) are device scalars.
 * A pixel none of whose 7 x 7 neighbours has M != 0 gets +0.0.
 *
 * fsraft_smoothness: order 1: (mean(w_y * r(D_y f)) + mean(w_x * r(D_x f))) / 2 with forward differences, r(x) =
 * sqrt(x^2 + 1e-6) and w = exp(-mean_c |k * D I|) (gaussian != 0: exp(-mean_c (k * D I)^2)), k = edge_constant; order 2:
 * second differences of the flow and stride-2 differences of the image.  out[0] = the value, dflow [B][2][H][W] = its
 * gradient, both from one pass. */
int fsraft_range_map_scratch_bytes(int B, int H, int W);
int fsraft_range_map(const float* flow, int64_t flow_bs, int64_t flow_cs, int64_t flow_rs, int B, int H, int W, int clip,
                     float* out, void* scratch, int64_t scratch_bytes, hipStream_t stream);
int fsraft_census_scratch_bytes(int B, int H, int W);
int fsraft_census_fwd(const float* img1, int64_t img1_bs, int64_t img1_cs, int64_t img1_rs, int img1_frame,
                      const float* img2, int64_t img2_bs, int64_t img2_cs, int64_t img2_rs, int Hf, int Wf,
                      const int* crop_yx, const float* flow, int64_t flow_bs, int64_t flow_cs, int64_t flow_rs,
                      const float* mask, int64_t mask_bs, int64_t mask_rs, int B, int H, int W,
                      float* grayB, float* hplane, double* out, void* scratch, int64_t scratch_bytes, hipStream_t stream);
int fsraft_census_bwd(const float* img1, int64_t img1_bs, int64_t img1_cs, int64_t img1_rs, int img1_frame,
                      const float* img2, int64_t img2_bs, int64_t img2_cs, int64_t img2_rs, int Hf, int Wf,
                      const int* crop_yx, const float* flow, int64_t flow_bs, int64_t flow_cs, int64_t flow_rs,
                      const float* grayB, const float* hplane, const float* up, const double* den, int B, int H, int W,
                      float* dflow, hipStream_t stream);
int fsraft_smoothness_scratch_bytes(int B, int H, int W);
int fsraft_smoothness(const float* img, int64_t img_bs, int64_t img_cs, int64_t img_rs, int Hf, int Wf, const int* crop_yx,
                      const float* flow, int64_t flow_bs, int64_t flow_cs, int64_t flow_rs, int B, int H, int W, int order,
                      float edge_constant, int gaussian, float* dflow, double* out, void* scratch, int64_t scratch_bytes,
                      hipStream_t stream);

/* ---- forward-backward consistency masks and the self-supervision term of the SMURF loss (smurf_utils.py
 * compute_occlusions_brox :432-453, self_supervision_loss :735-829 with a plain crop as the transform) ---------------------
 * Conventions of the section above: flows [B][2][.][.] with channel 0 = x, strides in elements with a unit x stride, frames
 * of Hf x Wf with the H x W window of sample b at (crop_yx[2b], crop_yx[2b+1]) = (y, x) (HOST array, NULL: all zero; with
 * Hf = H and Wf = W the views are the images themselves), fp32 per pixel with one rounding per operation, fp64 sums in
 * workgroup order through `scratch`; bit-identical from run to run, capturable, no allocation, no synchronisation.
 * For a pair (f, g) over an image of Hi x Wi, at pixel p: r = bilinear(g, p + f(p)) with zero taps outside the image,
 * sq = |f + r|^2, ss = |f|^2 + |r|^2, valid = p + f(p) inside [0, Wi-1] x [0, Hi-1].  The consistency c is
 * exp(-sq / norm) (FSRAFT_FB_GAUSSIAN; norm = sigma^2 * (h^2 + w^2), chosen by the caller) or [sq < 0.01 ss + 0.5]
 * (FSRAFT_FB_DDFLOW).
 * FSRAFT_ERR_ARG, before any HIP call, for a null pointer (teacher_mask excepted), B, H or W below 1, H * W or Hf * Wf beyond
 * 2^31 - 1, a frame smaller than the window, a window outside the frame, an unknown mode (FSRAFT_FB_BROX is one for
 * fsraft_selfsup, FSRAFT_FB_NONE for fsraft_fb_mask), complement other than 0 or 1, norm <= 0 (or NaN) in gaussian mode, a
 * misaligned fp64 pointer or too little scratch.
 *
 * fsraft_fb_mask: flow and flow_back are frames and the image of the pair is the frame; out [B][H][W] (every element
 * written) is evaluated on the window: c * valid (complement 0) or 1 - c * valid (complement 1; the gaussian's as
 * -expm1(-sq / norm), which keeps its relative accuracy next to c = 1, here and in fsraft_selfsup) in the gaussian and ddflow
 * modes; FSRAFT_FB_BROX gives visible = 1 - [sq > 0.01 ss + 0.5], without the valid factor (a warp outside the frame has
 * r = 0) and whatever complement says.
 *
 * fsraft_selfsup: teacher is a frame [B][2][Hf][Wf] of which the window is read; teacher_mask [B][H][W] (NULL: ones) is what
 * fsraft_fb_mask left for the teacher's pair, computed once and reused by every prediction; student and student_back are
 * [B][2][H][W] and their image is the H x W window itself.  m = teacher_mask * (1 - c * valid) of the student's pair, formed
 * in registers (FSRAFT_FB_NONE: m = teacher_mask); d = teacher - student, e = sqrt(d^2 + 1e-6) per channel.
 * out[0] = sum m * (e_x + e_y) / (2 * B * H * W); dflow [B][2][H][W] (every element written) = d out[0] / d student =
 * -m * d / e / (2 * H * W) / B, divided in that order, so that a sample alone gives, divided by B, the bits it gives in the
 * batch; +0.0 where m == 0.  No gradient for the teacher, the mask or student_back. */
#define FSRAFT_FB_GAUSSIAN 0
#define FSRAFT_FB_DDFLOW 1
#define FSRAFT_FB_BROX 2
#define FSRAFT_FB_NONE 3
int fsraft_fb_mask(const float* flow, int64_t flow_bs, int64_t flow_cs, int64_t flow_rs,
                   const float* flow_back, int64_t back_bs, int64_t back_cs, int64_t back_rs, int Hf, int Wf,
                   const int* crop_yx, int B, int H, int W, int mode, int complement, float norm, float* out, hipStream_t stream);
int fsraft_selfsup_scratch_bytes(int B, int H, int W);
int fsraft_selfsup(const float* teacher, int64_t teacher_bs, int64_t teacher_cs, int64_t teacher_rs, int Hf, int Wf,
                   const int* crop_yx, const float* teacher_mask, int64_t tmask_bs, int64_t tmask_rs,
                   const float* student, int64_t student_bs, int64_t student_cs, int64_t student_rs,
                   const float* student_back, int64_t sback_bs, int64_t sback_cs, int64_t sback_rs, int B, int H, int W,
                   int mode, float norm, float* dflow, double* out, void* scratch, int64_t scratch_bytes, hipStream_t stream);

/* ---- UnsupAugmentor applied to a batch (csrc/augment.hip; flow_supervisor_amd/augment.py draws the parameters) ----------
 * pytorch/raft_utils/augmentor.py:496-657 (spatial_transform, color_transform, eraser_transform), ColorJitter :15-37 and the
 * "* 255" of pytorch/train.py:251-258.  The reference's augmentor is TensorFlow on the host and does not run here: the formulas
 * below are the definition (restated in float64 in tests/_augref.py).
 *
 * Sources are interleaved: image1 / image2 [B][Hs][Ws][3], uint8 in [0, 255] (FSRAFT_AUG_U8) or float in [0, 1]
 * (FSRAFT_AUG_F32); flow [B][Hs][Ws][2]; valid [B][Hs][Ws] (NULL: ones).  params is a HOST array of B structs, read and checked
 * during the call and passed to the kernels by value, so a captured call keeps its parameters.  Outputs are planar, contiguous
 * fp32, every element written: frame1 / frame2 [B][3][Hf][Wf] in [0, 255] without photometric change, frame_flow [B][2][Hf][Wf],
 * frame_valid [B][1][Hf][Wf], crop1 / crop2 [B][3][h][w] in [0, 255] after colour and eraser, crop_flow [B][2][h][w],
 * crop_valid [B][1][h][w].
 *
 * Frame pixel (y, x) of sample b is pixel (vflip ? Hf-1-y : y) + win_y, (hflip ? Wf-1-x : x) + win_x of the source resized to
 * th x tw (resize 0: the source itself, th = Hs, tw = Ws).  Images: TF2 tf.image.resize(BILINEAR), half-pixel centres, no
 * antialias: src = (dst + 0.5) * (in / out) - 0.5, lo = max(floor(src), 0), hi = min(ceil(src), in - 1), weight src - floor(src),
 * along x within the two rows, then along y; a float source is multiplied by 255 afterwards.  Flow and valid: NEAREST_NEIGHBOR,
 * index min(floor((dst + 0.5) * (in / out)), in - 1); all of this index arithmetic in float32.  The flow is multiplied by
 * (scale_x, scale_y), by (-1, 1) under hflip and by (1, -1) under vflip.  The crop is the h x w window of the frame at
 * (crop_y, crop_x).
 * Colour, per image i on x = frame / 255: x * brightness[i]; (x - mean) * contrast[i] + mean with the per-channel mean of the
 * brightness-scaled crop (asym 0: over both crops); RGB -> HSV -> RGB with s = clip(s * saturation[i], 0, 1); again with
 * h = frac(h + hue[i]); clip to [0, 1]; * 255.  HSV: v = max, c = max - min, s = c / v (0 when v <= 0), h the hexcone sector in
 * [0, 1) (0 when c = 0); back: ((d - 1) * s + 1) * v with d = clip(|6h - 3| - 1), clip(2 - |6h - 2|), clip(2 - |6h - 4|) in [0, 1].
 * Eraser: rect[r] = (x0, y0, dx, dy), r < nrect, of crop2 is overwritten with crop2's per-channel mean after the colour step
 * and before any rectangle; an empty rectangle writes nothing.
 *
 * Sums are fp64 per workgroup in `scratch` (8-byte aligned, at least fsraft_augment_scratch_bytes, nothing to initialise) and
 * added in workgroup order: no float atomics, bit-identical from run to run.  No allocation, no synchronisation; four launches
 * per 16 samples (three when none of them has a rectangle).
 * FSRAFT_ERR_ARG, before any HIP call, for a null (valid excepted) or misaligned pointer, an unknown dtype, a size below 1,
 * Hs * Ws * 3, Hf * Wf * 3 or th * tw beyond 2^31 - 1, h > Hf or w > Wf, th < Hf or tw < Wf, resize 0 with (th, tw) != (Hs, Ws),
 * a window outside the resized image, a crop outside the frame, a rectangle outside the crop, nrect outside 0..2, a flag
 * other than 0 or 1, a non-finite factor, asym 0 with factors that differ between the two images, or too little scratch. */
#define FSRAFT_AUG_U8 0
#define FSRAFT_AUG_F32 1
typedef struct fsraft_aug_params {
  int resize, th, tw;
  float scale_x, scale_y;
  int win_y, win_x, hflip, vflip, crop_y, crop_x;
  int asym;
  float brightness[2], contrast[2], saturation[2], hue[2];
  int nrect;
  int rect[2][4];
} fsraft_aug_params;
int fsraft_augment_scratch_bytes(int B, int Hf, int Wf, int h, int w);
int fsraft_augment(const void* image1, const void* image2, int dtype, const float* flow, const float* valid, int B, int Hs, int Ws,
                   const fsraft_aug_params* params, int Hf, int Wf, int h, int w, float* frame1, float* frame2, float* frame_flow,
                   float* frame_valid, float* crop1, float* crop2, float* crop_flow, float* crop_valid, void* scratch,
                   int64_t scratch_bytes, hipStream_t stream);

/* ---- FlowAugmentor / SparseFlowAugmentor applied to a batch (csrc/augment.hip; flow_supervisor_amd/augment.py) -------------
 * pytorch/raft_utils/augmentor.py:39-188 (dense ground truth) and :191-330 (sparse), in the order of their __call__: colour,
 * eraser, spatial.  The formulas below are the definition (restated in float64 in tests/_supaugref.py).
 *
 * Sources, dtypes and params as for fsraft_augment, with fsraft_aug_params read this way: win_y = win_x = 0; th x tw is the size
 * of the resized image (resize 0: Hs x Ws); (crop_y, crop_x) is the crop's corner in the flipped resized image, any integer;
 * rect[r] is in SOURCE coordinates.  th and tw may differ between the samples of a batch.  Outputs are planar, contiguous fp32,
 * every element written: crop1 / crop2 [B][3][h][w] in [0, 255], crop_flow [B][2][h][w], crop_valid [B][1][h][w].
 *
 * Per sample, with x = source / 255 (uint8) or the source (float):
 * Photometric source: P_i = clip(hue(sat(contrast(x * brightness[i]))), 0, 1) with the colour formulas of fsraft_augment, the
 * contrast mean being the per-channel mean of the brightness-scaled SOURCE image i (asym 0: over both sources, which the
 * reference stacks into one image).
 * Eraser: m2 = the per-channel mean of P_2 over the whole source, before any rectangle; E_2 = m2 inside any rect[r], else P_2;
 * E_1 = P_1.  An empty rectangle changes nothing.
 * Spatial: crop pixel (y, x) is pixel ry = vflip ? th-1-(crop_y+y) : crop_y+y, rx = hflip ? tw-1-(crop_x+x) : crop_x+x of E_i
 * resized to th x tw with TF2 tf.image.resize(BILINEAR) (half-pixel centres, no antialias; the taps and weights of
 * fsraft_augment, along x within the two rows, then along y; resize 0: the pixel itself), times 255.
 * Flow: FSRAFT_AUG_FLOW_BILINEAR the same bilinear taps on the flow, FSRAFT_AUG_FLOW_NEAREST the nearest-neighbour index of
 * fsraft_augment on flow and valid; then times (scale_x, scale_y) (resize 0: not at all), times (-1, 1) under hflip and
 * (1, -1) under vflip.  crop_valid in mode BILINEAR is all ones and a given `valid` is ignored (flow_dataset.py:126).
 * All index arithmetic in float32.  Nothing of source or resized size is written to memory: the colour step and the rectangle
 * test are evaluated at each tap.
 *
 * Sums are fp64 per workgroup in `scratch` (8-byte aligned, at least fsraft_augment_sup_scratch_bytes, nothing to initialise),
 * added in workgroup order: no float atomics, bit-identical from run to run.  No allocation, no synchronisation; five launches
 * per 16 samples (three when none of them has a non-empty rectangle).
 * FSRAFT_ERR_ARG, before any HIP call, for a null (valid excepted) or misaligned pointer, an unknown dtype or flow_mode, a size
 * below 1, Hs * Ws * 3, h * w * 3 or th * tw beyond 2^31 - 1, resize 0 with (th, tw) != (Hs, Ws), win_y or win_x != 0, th < h or
 * tw < w, a crop outside th x tw, a rectangle outside the source, nrect outside 0..2, a flag other than 0 or 1, a non-finite
 * factor, asym 0 with factors that differ between the two images, or too little scratch. */
#define FSRAFT_AUG_FLOW_BILINEAR 0   /* FlowAugmentor */
#define FSRAFT_AUG_FLOW_NEAREST  1   /* SparseFlowAugmentor */
int fsraft_augment_sup_scratch_bytes(int B, int Hs, int Ws);
int fsraft_augment_sup(const void* image1, const void* image2, int dtype, const float* flow, const float* valid, int flow_mode,
                       int B, int Hs, int Ws, const fsraft_aug_params* params, int h, int w,
                       float* crop1, float* crop2, float* crop_flow, float* crop_valid,
                       void* scratch, int64_t scratch_bytes, hipStream_t stream);

/* Channels-last ([B][HW][C], C % 4 == 0, C <= 256) variants, for the encoder stages whose convolutions run on
 * fsraft_conv_forward.  sums/sumsq/s1/s2 and dsum_g/dsum_gx: [B * 8][C] partial rows (workgroups spread their atomics over
 * eight rows per sample: thousands of adds on the same C addresses serialise in L2 otherwise; dsum_*: the per-channel sums
 * are the column sums of the rows); all must be ZERO on entry.  stats: [B][C][2] = (mean, rstd).
 * Fused residual unit (pytorch/core/extractor.py:43-56, "return self.relu(x+y)"): res != NULL makes the forward write
 * y = relu(res + relu?(norm(x))); the backward then takes out = that y and writes the shortcut's gradient g * (out > 0)
 * to dres before continuing into the norm branch (out and dres both NULL: plain norm + ReLU). */
/* have_sums != 0: sums / sumsq already hold the partial rows -- accumulated by the convolution that produced x
 * (fsraft_conv_forward_stats, 8 slots) -- and the statistics pass over x is skipped. */
/* s2d_w != 0 (= the image width W; W and H = HW / W even): the result y is written in the space-to-depth layout of
 * fsraft_space_to_depth2 ([B][H/2][W/2][2][2][C]) -- what the stride-2 residual unit behind it reads (extractor.py:23-57 with
 * stride 2) -- and the backward reads the gradient g and the saved result `out` from that layout; x, res, dx, dres stay
 * [B][HW][C].  0: everything [B][HW][C].  (fsraft_affine_relu_cl_fwd takes HW for this; ignored when s2d_w == 0.) */
int fsraft_inorm_relu_cl_fwd(const float* x, const float* res, float* y, float* sums, float* sumsq, float* stats, int B, int HW,
                             int C, float eps, int relu, int have_sums, int s2d_w, hipStream_t stream);
int fsraft_inorm_relu_cl_bwd(const float* g, const float* x, const float* stats, const float* out, float* s1, float* s2, float* dx,
                             float* dres, int B, int HW, int C, int relu, int s2d_w, hipStream_t stream);
int fsraft_affine_relu_cl_fwd(const float* x, const float* res, const float* scale, const float* shift, float* y, int64_t M, int C,
                              int relu, int HW, int s2d_w, hipStream_t stream);
int fsraft_affine_relu_cl_bwd(const float* g, const float* x, const float* scale, const float* shift, const float* out, float* dx,
                              float* dres, float* dsum_g, float* dsum_gx, int B, int HW, int C, int relu, int s2d_w, hipStream_t stream);

/* Frozen-BatchNorm parameter folding in one launch per direction (instead of ~11 framework launches on [C] tensors per layer
 * and step): scale = weight * rsqrt(var + eps), shift = bias - (mean - cbias) * scale, rs = rsqrt(var + eps), rmc = mean - cbias
 * (cbias: bias of the preceding convolution, folded in; nullable).  Backward from the partial sums [2][R][C] that
 * fsraft_affine_relu_cl_bwd leaves: dweight = rs * (S1 - rmc * S0), dbias = S0, dcbias = scale * S0 (nullable). */
int fsraft_bn_fold(const float* weight, const float* bias, const float* rm, const float* rv, const float* cbias, float eps, int C,
                   float* scale, float* shift, float* rs, float* rmc, hipStream_t stream);
int fsraft_bn_fold_bwd(const float* part, int R, int C, const float* rs, const float* rmc, const float* scale, float* dweight,
                       float* dbias, float* dcbias, hipStream_t stream);

/* Training-mode BatchNorm2d on the same channels-last layout (csrc/norm_bn.hip): torch.nn.BatchNorm2d in training mode behind
 * pytorch/core/extractor.py:13-57, 118-170 (the context encoder of pytorch/core/raft.py:55 while its trainer has not called
 * freeze_bn).  With n = B * HW: mean = sum x / n, var = max(sum x^2 / n - mean^2, 0) (biased), rstd = rsqrt(var + eps),
 * scale = weight * rstd, shift = bias - mean * scale, t = fma(x, scale, shift), y = relu?(t) or relu(res + relu?(t));
 * stats [4][C] = (mean, rstd, scale, shift) out.  running_mean / running_var (both or neither) are updated in place:
 * rm = (1 - momentum) rm + momentum (mean + cbias), rv = (1 - momentum) rv + momentum var n / (n - 1); cbias (nullable) is the
 * bias of the convolution in front, which ran without it: y does not depend on it, the running mean does.
 * Backward: g' = g [out > 0] (with a shortcut) [t > 0] (with relu), t recomputed by the forward's fma; xhat = (x - mean) rstd,
 * S1 = sum g', S2 = sum g' xhat over all n; dx = scale (g' - S1 / n - xhat S2 / n), dweight = S2, dbias = S1, dres = g [out > 0].
 * acc: [2][FSRAFT_BN_PARTIAL_ROWS][C] partial rows, ZERO on entry.  res / out / dres / s2d_w as for the entries above.
 * FSRAFT_ERR_ARG, nothing written: n < 2, C outside 4..256 or no multiple of 4, s2d_w odd or HW / s2d_w odd, out without dres. */
#define FSRAFT_BN_PARTIAL_ROWS 64
int fsraft_bnorm_cl_fwd(const float* x, const float* res, const float* weight, const float* bias, const float* cbias,
                        float* running_mean, float* running_var, float momentum, float eps, float* acc, float* y, float* stats,
                        int B, int HW, int C, int relu, int s2d_w, hipStream_t stream);
int fsraft_bnorm_cl_bwd(const float* g, const float* x, const float* stats, const float* out, float* acc, float* dx, float* dres,
                        float* dweight, float* dbias, int B, int HW, int C, int relu, int s2d_w, hipStream_t stream);

/* ---- the encoders' stem (next-row f3)---------------------------------------------------
 * Replaces `self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3)` and its backward-weights
 * (pytorch/core/extractor.py:135 BasicEncoder, :212 SmallEncoder with 32 outputs).  x [B][3][H][W] planar fp32, w [N][3][7][7],
 * N = 32 or 64; out / dy channels-last [B][Ho][Wo][N] with Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1.  The image needs no
 * gradient (it is the network input).  fsraft_stem7x7s2_wgrad OVERWRITES dw [N][3][7][7]; scratch: fsraft_stem_slots() * 64 *
 * 192 floats of workspace (per-workgroup partial sums). */
int fsraft_stem_slots(void);
int fsraft_stem7x7s2_fwd(const float* x, const float* w, const float* bias, float* out, int B, int H, int W, int N,
                         hipStream_t stream);
int fsraft_stem7x7s2_wgrad(const float* x, const float* dy, float* dw, float* scratch, int B, int H, int W, int N,
                           hipStream_t stream);

/* ---- optimizer step of the train step (row e: what the DP step does after the all-reduce) ---------
 * `torch.nn.utils.clip_grad_norm_(model.parameters(), args.clip)` + `optimizer.step()` of `optim.AdamW(model.parameters(),
 * lr, weight_decay, eps)` (pytorch/train.py:137, 280-282) on FLAT fp32 buffers: parameters p, gradients g (scaled in place
 * like clip_grad_norm_ does), first / second moments m, v, n elements each.  step: device fp32 step count, incremented here;
 * norm: device scalar holding the gradients' 2-norm (null: no clipping); lr: device scalar; state: 4 floats of scratch;
 * beta1 / beta2: double, unrounded (torch forms the bias corrections 1 - beta^step and 1 - beta in double);
 * skip64 (nullable): ceil(n / 64) bytes, non-zero = the 64-element block belongs to a parameter that received no gradient
 * this step and is left untouched with its moments (torch's AdamW skips `p.grad is None`). */
int fsraft_adamw_flat(float* p, float* g, float* m, float* v, int64_t n, float* step, const float* norm, float max_norm,
                      const float* lr, double beta1, double beta2, float eps, float weight_decay, float* state,
                      const unsigned char* skip64, hipStream_t stream);
/* Host helper (no device work): *id = 0 when `stream` is not being captured into a hipGraph, else the capture's id.  The
 * binding keys per-capture scratch (zero-filled accumulation targets) on it. */
int fsraft_stream_capture_id(hipStream_t stream, unsigned long long* id);

/* ---- layout / elementwise helpers around the GEMMs -----------------------------------
 * FSRAFT_ERR_ARG before any launch for a NULL required pointer and for what a kernel makes no provision for: a channel window
 * outside its row (coff < 0, coff + C > ld; C > ld for relu_bwd and col_sum; ldzr < 2 hid), sizes below 1 where the grid is formed
 * from them, pitches that are no multiple of 4 floats and bases off 16 bytes where 16-byte chunks are moved (relu_bwd: g, y, ldg,
 * ldy; space_to_depth2: src, dst, C; im2col7: ld; sum_n: everything), col2im7's ld < 98.  relu_bwd: g[m][c] = y[m][c] > 0 ?
 * g[m][c] : 0 for c < C and nothing else -- columns C .. ld - 1 of g keep their bits. */
int fsraft_nchw_to_nhwc(const float* src, float* dst, int B, int C, int HW, int ld, int coff, int accumulate, hipStream_t s);
/* Space-to-depth by 2 of a channels-last tensor: dst[b][y/2][x/2][(y%2)*2 + x%2][c] = src[b][y][x][c] (inverse != 0: back).
 * A stride-2 3x3 / 1x1 convolution over src (pytorch/core/extractor.py:13, 39: the first convolution and the shortcut of a
 * stride-2 ResidualBlock) is a stride-1 2x2 / 1x1 convolution of fsraft_conv_forward over dst viewed as [B][H/2][W/2][4C]. */
int fsraft_space_to_depth2(const float* src, float* dst, int B, int H, int W, int C, int inverse, hipStream_t s);
int fsraft_nhwc_to_nchw(const float* src, float* dst, int B, int C, int HW, int ld, int coff, int accumulate, hipStream_t s);
int fsraft_im2col7(const float* flow, int64_t bs, int64_t cs, int64_t ps, float* cols, int ld, int B, int H, int W, hipStream_t s);
int fsraft_col2im7(const float* dcols, int ld, float* dflow, int B, int H, int W, int accumulate, hipStream_t s);
int fsraft_flow_to_nhwc(const float* flow, int64_t bs, int64_t cs, int64_t ps, float* dst, int ld, int coff, int B, int HW, hipStream_t s);
int fsraft_nhwc_to_flow(const float* src, int ld, int coff, float* dflow, int B, int HW, int accumulate, hipStream_t s);
int fsraft_relu_bwd(float* g, int ldg, const float* y, int ldy, int64_t M, int C, hipStream_t s);
/* dzr_sum / dq_sum (nullable, same layouts as dzr / dq): running sums over the iterations of a step; dhn2 (nullable): a second
 * summand of the incoming gradient (dh' = dhn + dhn2: the heads' part and the part arriving from the next iteration) */
int fsraft_gru_bwd1(const float* dhn, const float* dhn2, const float* z, const float* q, const float* h, float* dzr, int ldzr, float* dq, float* dh, float* dzr_sum, float* dq_sum, int64_t M, int hid, hipStream_t s);
int fsraft_gru_bwd2(const float* drh, const float* r, const float* h, float* dzr, int ldzr, float* dh, float* dzr_sum, int64_t M, int hid, hipStream_t s);
int fsraft_col_sum(const float* x, int ld, int64_t M, int C, float* out, float scale, hipStream_t s);
int fsraft_axpby(const float* x, float* y, float a, float b, int64_t n, hipStream_t s);
/* out[0..count) = (accumulate ? out : 0) + src[0] + ... + src[n - 1], added in list order (count % 4 == 0, 16-byte aligned): the sum
 * of the GRU gate gradients over the iterations of a step (the context part's backward, update.py:16-60 with x = cat(inp, motion)
 * split into a per-step context convolution), formed once from the kept per-iteration gradients. */
int fsraft_sum_n(const float* const* src, int n, float* out, int64_t count, int accumulate, hipStream_t s);

/* ---- image plumbing of the TensorFlow tree (util/image.py:6-49 crop_bboxes / pad_bboxes, raft/__init__.py:199-222 resize /
 * resize_flow, util/pad.py + util/validate.py:301-325 pad_edge / pad_inputs; csrc/image_ops.hip) ---------------------------
 * List form: src[i] -> dst[i] for n (1..32) tensors of ONE geometry in one launch.  fp32.  A tensor is [B][H][W][C] read through
 * four strides in elements (batch, channel, row, x): element (b, c, y, x) is at b * bs + c * cs + y * rs + x * xs.  NHWC is
 * (HWC, 1, WC, C), planar [B][C][H][W] is (CHW, HW, W, 1); the two sides of a call have strides of their own.  Enqueue only: no
 * allocation, no synchronisation, no read back.  FSRAFT_ERR_ARG before any HIP call for a NULL table or entry, n outside
 * 1..32, B, C or a size below 1, C * H * W of either side beyond 2^31 - 1, and what each entry names below.
 *
 * fsraft_box_copy: sample b's H x W window sits at (yx[2b], yx[2b+1]) = (y, x) of its Hf x Wf frame; yx is a HOST array of 2 * B
 * ints, read during the call and passed to the kernel by value (64 samples per launch).  place == 0 (gather): src are frames,
 * dst windows (crop_bboxes; the backward of pad_bboxes).  place != 0: src are windows, dst frames, every frame element outside
 * the window written +0.0 by the same launch (pad_bboxes; the backward of crop_bboxes).  Bit-exact.  Where both sides are laid
 * out alike with unit inner strides (cs == 1 and xs == C, or xs == 1), 16-byte aligned bases, outer strides and row lengths
 * (W * E, Wf * E floats, E = C or 1) that are multiples of 4, a sample whose row start x * E is one too moves 16-byte units;
 * every other sample moves 4-byte units.  Also an error: yx NULL, a window outside the frame.
 *
 * fsraft_resize_bilinear_fwd: tf.image.resize(method 'bilinear', antialias False) from Hi x Wi to Ho x Wo.  Per axis, in float32
 * as TensorFlow forms them: scale = (float)n_in / (float)n_out, in = (o + 0.5f) * scale - 0.5f (two roundings), lo =
 * max(floor(in), 0), hi = min(ceil(in), n_in - 1), lerp = in - floor(in); the value is top + (bottom - top) * lerp_y with top =
 * tl + (tr - tl) * lerp_x.  factors (a HOST array of C floats, C <= 8, or NULL) multiply channel c behind the interpolation:
 * (Wo / Wi, Ho / Hi) makes resize_flow one launch.  The s_ strides describe the Hi x Wi side, the d_ strides the Ho x Wo side.
 * fsraft_resize_bilinear_bwd: its exact transpose.  ddst are the upstream gradients (Ho x Wo, d_ strides), dsrc (Hi x Wi, s_
 * strides) receive them: every element written, each a sum over the destination pixels whose taps reach it, rows ascending,
 * columns ascending inside, no atomics: the same bits twice; +0.0 where no tap reaches.  Also an error: B > 65535, factors with
 * C > 8.
 *
 * fsraft_pad_edge: np.pad(x, ((0,0), (top, bottom), (left, right), (0,0)), 'edge'): dst is (H + top + bottom) x (W + left + right).
 * Bit-exact.  Also an error: a negative pad, B > 65535. */
int fsraft_box_copy(const float* const* src, float* const* dst, int n, int place, int B, int C, int Hf, int Wf, int H, int W,
                    const int* yx, int64_t f_bs, int64_t f_cs, int64_t f_rs, int64_t f_xs,
                    int64_t w_bs, int64_t w_cs, int64_t w_rs, int64_t w_xs, hipStream_t stream);
int fsraft_resize_bilinear_fwd(const float* const* src, float* const* dst, int n, int B, int C, int Hi, int Wi, int Ho, int Wo,
                               int64_t s_bs, int64_t s_cs, int64_t s_rs, int64_t s_xs,
                               int64_t d_bs, int64_t d_cs, int64_t d_rs, int64_t d_xs, const float* factors, hipStream_t stream);
int fsraft_resize_bilinear_bwd(const float* const* ddst, float* const* dsrc, int n, int B, int C, int Hi, int Wi, int Ho, int Wo,
                               int64_t s_bs, int64_t s_cs, int64_t s_rs, int64_t s_xs,
                               int64_t d_bs, int64_t d_cs, int64_t d_rs, int64_t d_xs, const float* factors, hipStream_t stream);
int fsraft_pad_edge(const float* const* src, float* const* dst, int n, int B, int C, int H, int W,
                    int top, int bottom, int left, int right, int64_t s_bs, int64_t s_cs, int64_t s_rs, int64_t s_xs,
                    int64_t d_bs, int64_t d_cs, int64_t d_rs, int64_t d_xs, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FSRAFT_H */
