/* fsraft_tuning.h -- measurement and test knobs of libfsraft.so.
 *
 * NOT part of the drop-in boundary (include/fsraft.h): nothing here corresponds to an interface of the reference, and a
 * maintainer integrating the library never calls these.  They exist so that tests can reach a kernel at sizes its
 * selection heuristic would not pick (e.g. the resident-patch 3x3 kernel at a 16x16 test grid), so that scripts/ can A/B
 * kernel variants inside one process, and so that the parity suite can run the GEMM families in either arithmetic mode
 * one by one (fsraft_set_arithmetic of fsraft.h switches them together).
 *
 * Kernels that lost their A/B twice (LDS-direct weight tiles, record-activation convolution, resident-weight 64 -> 64 kernel,
 * the transposed-role / persistent volume builds; keys 24 / 25 / 30 of earlier rounds) were removed from the tree in round 5: their
 * measurements are in docs/history/ and profiles/; the keys return FSRAFT_ERR_ARG.
 */
#ifndef FSRAFT_TUNING_H
#define FSRAFT_TUNING_H

#ifdef __cplusplus
extern "C" {
#endif

/* Keys of fsraft_set_tuning / fsraft_get_tuning: the knobs of the convolution family; any other number is no key. */
enum fsraft_tuning_key {
  FSRAFT_KEY_CONV_TILE = 0,            /* conv tile (0 auto, 1 128x128, 2 64x128, 3 64x64) */
  FSRAFT_KEY_WGRAD_TILE = 1,           /* wgrad tile (0 128x128, 3 64x64) */
  FSRAFT_KEY_WGRAD_BLOCKS = 2,         /* target workgroup count of the weight-gradient pixel split (11: of the multi-segment
                                          launch, 17: of the few-channel kernel) */
  FSRAFT_KEY_CONV_ARITH = 3,           /* arithmetic of the forward / data-gradient convolutions (0 exact fp32, 1 bf16x3;
                                          3 / 4 / 5 force a tile shape) */
  FSRAFT_KEY_WGRAD_ARITH = 4,          /* arithmetic of the weight gradients (0 exact, 2 bf16x3) */
  FSRAFT_KEY_CONV_BUF = 5,             /* buffer-addressed loaders: forward / data gradient (8: weight gradient) */
  FSRAFT_KEY_XCD_SWIZZLE = 7,          /* XCD swizzle */
  FSRAFT_KEY_WGRAD_BUF = 8,
  FSRAFT_KEY_CONV_N256 = 9,            /* tile-shape thresholds (9 / 13 / 14 / 15 / 18 / 19): 64x256 tiles */
  FSRAFT_KEY_WGRAD_MULTI = 10,         /* one weight-gradient launch per layer over all iterations of a step */
  FSRAFT_KEY_WGRAD_BLOCKS_MULTI = 11,
  FSRAFT_KEY_CONV_UNIFORM = 12,        /* uniform k-tile table */
  FSRAFT_KEY_CONV_W8 = 13,             /* eight- / sixteen-wave tiles for wide layers (14: minimum workgroup count) */
  FSRAFT_KEY_CONV_W8_MIN = 14,
  FSRAFT_KEY_WGRAD_W8 = 15,            /* eight-wave workgroups in the multi-segment weight gradient */
  FSRAFT_KEY_WGRAD_PACK = 16,          /* few-channel weight-gradient kernel */
  FSRAFT_KEY_WGRAD_BLOCKS_PACK = 17,
  FSRAFT_KEY_CONV_N64 = 18,            /* 256x64 tiles for N <= 64 (19: minimum pixel count) */
  FSRAFT_KEY_CONV_N64_MIN_M = 19,
  FSRAFT_KEY_CONV_HALO = 20,           /* 20 / 21: resident-patch 3x3 encoder kernel and its minimum pixel count */
  FSRAFT_KEY_CONV_HALO_MIN_M = 21,
  FSRAFT_KEY_WGRAD_XCD = 22,           /* XCD-aware weight-gradient order */
  FSRAFT_KEY_CONV_PATCH = 26,          /* resident-patch forward / data-gradient kernel */
  FSRAFT_KEY_WGRAD_PATCH = 27,         /* resident-block weight gradient (0 off, 1 the 3x3 layers, 2 the five-tap layers too) */
  FSRAFT_KEY_CONV_PATCH64 = 28,        /* 64-column patch tiles */
  FSRAFT_KEY_WGRAD_PATCH1 = 29,        /* single-segment resident-block weight gradient, minimum pixel count */
  FSRAFT_KEY_CONV_PATCH_MIN_M = 31,    /* minimum pixel count of the resident-patch forward / data-gradient kernel */
  FSRAFT_KEY_CONV_KSPLIT = 32          /* split-K slices of the small-M convolutions (-1 auto, 0 off, >= 2 forced) */
};
/* set: FSRAFT_OK, or FSRAFT_ERR_ARG for a key that is not in the enum.  get: the knob's value, INT_MIN for such a key. */
int fsraft_set_tuning(int key, int value);
int fsraft_get_tuning(int key);
/* Route attestation: the kernel the CALLING THREAD's last convolution ran (0 none / rejected call, -1 bad `which`).
 * which 0, fsraft_conv_forward (forward and data-gradient calls):
 *   exact-fp32 implicit GEMM tiles  1 Cfg32 (N <= 32, either mode), 2 Cfg64, 3 64x128, 4 128x128, 5 64x64 (key 0 = 3),
 *                                   6 64x64 k16 (key 0 = 4), 7 64x128 k16 (key 0 = 5);
 *   resident-patch kernel           10 128-pixel x 128-column tiles, 11 256 x 128, 12 128 x 64, 13 256 x 64 (conv_patch.inc);
 *   conv3x3_halo_kernel             20 <2,1> (N <= 64), 21 <2,2>;
 *   bf16x3 implicit GEMM tiles      30 64x256 (key 9 / key 3 = 5), 31 256x64, 32 256x128 sixteen waves, 33 128x128 eight
 *                                   waves, 34 64x128, 35 128x128;
 *   + 100: the same tile as split-K slices followed by conv_finish_kernel.
 * which 1, fsraft_conv_wgrad / fsraft_conv_wgrad_multi (weight gradients):
 *   1 exact 32x128 (Cout <= 32, either mode), 2 exact 64x64 (key 1 = 3), 3 exact 128x128, 4 bf16x3 128x128 (key 4 = 1),
 *   5 bf16x3 128x128 single LDS image, 6 few-channel pack kernel, 7 resident-block kernel (wgrad_patch.inc), 8 multi-segment
 *   launch, 9 multi-segment launch with eight-wave workgroups (key 15). */
int fsraft_conv_last_route(int which);
/* Wide tiles of the per-tap weight-gradient kernel (routes 5 and 8 keep their codes): 256x256 (Cout >= 256) and 128x256, whose
 * 256-column x tile is two 128-column groups of the packed-K layout; an odd last group and Cout beyond the last full 256 stay on
 * the 128x128 tile.  0 off, 1 by shape (default: the layer classes that won their A/B), 2 wherever the shape allows. */
int fsraft_set_wgrad_wide(int mode);
/* The tile of the calling thread's last weight-gradient launch as BM << 16 | BN (dY columns x packed-K columns; the wide tile when a
 * layer ran as wide tiles plus a 128x128 remainder); 0: none / rejected call / the resident-block kernel (no fixed tile). */
int fsraft_conv_wgrad_last_tile(void);
int fsraft_set_build_split(int on);   /* volume build: 1 bf16x3 (default), 0 exact fp32 MFMA */
int fsraft_set_build_kernel(int which); /* record build: bits 8..15 start-up stagger of odd workgroups (x 64 x 127 cycles), bits 16..18 store policy (0 auto, 1 plain, 2 sc1, 3 nt) */
/* cache policy of the tiled lookup's window loads: -1 auto (nt for volumes beyond the Infinity Cache; default), 0 plain, 2 nt,
 * 16 sc1, 18 nt + sc1 (A/B switch); 100 = measurement only: the nt window loads alone, no blends and no output (the gather floor of
 * the tiled layout, scripts/lookup_gather_floor.py) */
int fsraft_set_lookup_policy(int aux);
/* fsraft_corr_bwd_ktiles: 0 = per query and level the bounding rectangle of its lookups' windows is marked; 1 / 2 = on the
 * first one / two levels every lookup's window is marked on its own (tighter lists, a longer pre-pass). */
int fsraft_set_ktile_exact(int levels);
int fsraft_set_upsample_kernel(int v4);  /* convex upsampler: 1 (default) the 16-byte kernels for 16-byte aligned tensors, 0 the 4-byte ones */
int fsraft_set_dvol_box(int on);        /* gradient volume: 1 (default) one wave per query on its lookups' bounding boxes (corr_dvol_sep_kernel) + work list, 0 row-segment kernel only */
int fsraft_set_dvol_policy(int policy); /* cache policy of the gradient-volume stores: 0 plain, 1 sc1, 2 nt */
int fsraft_set_gemm_split(int on);    /* fsraft_gemm_f32 with trans_b: 1 bf16x3 when operands are 16-byte aligned */
int fsraft_set_lookup_qb(int qb);     /* queries per workgroup of the row-major lookup kernels: 0 auto, 8, 16 or 32 */
int fsraft_set_norm_blocks(int target_workgroups);   /* workgroups per launch of the channels-last norm kernels (default 4096) */
int fsraft_set_rec_mfma16(int on);    /* record GEMM (NT): 1 = v_mfma_f32_16x16x32_bf16, 0 = 32x32x16 */
int fsraft_set_alt_tile(int on);      /* alt-corr forward: 1 (default) 4x4-query tile kernel, 0 wave per query */

#ifdef __cplusplus
}
#endif
#endif
