// Flow validation metrics on the device (pytorch/evaluate.py:117-124 Sintel / Chairs, :150-165 KITTI): one pass over a batch
// of predictions against ground truth gives, per sample, the valid-pixel count, the end-point-error sum, the counts under
// 1 / 3 / 5 px and the KITTI outlier count (epe > 3 && epe / |gt| > 0.05), and folds them into a running accumulator.  The
// reference copies every full-resolution prediction to the host and reduces there.
//
// Per pixel the arithmetic is the reference's fp32 expressions with every operation correctly rounded on its own: torch on the
// CPU does not contract, so contraction is switched off for the whole file (a fused d0*d0 + d1*d1 differs in the last bit and
// flips `epe < 3`-style decisions).  Square root and division are the correctly rounded expansions the compiler emits by default
// (v_sqrt_f32 / v_rcp_f32 with their fix-up sequences; the __fsqrt_rn / __fmul_rn intrinsics of this toolchain are the native
// square root and a plain, contractable `*`, so they are not used).  (torch's own fp32 CPU sqrt is one ulp low for a share of
// arguments that depends on the build, tests/_evalref.py: IEEE is the one definition every host agrees on.)  Sums are fp64 from
// the first addition: an fp32 sum stops being exact for the counts at 2^24 pixels, a dataset pass has ~5e8.
//
// Deterministic and batch-independent: no atomics; a sample's pixels are split over a number of blocks that depends on H * W
// only, every block leaves its six partial sums in `scratch`, and one finalising block adds them in a fixed tree order, sample
// after sample, and updates the accumulator in ascending sample order.
#include "common.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int FM_THREADS = 256;
constexpr int FM_MAX_BLOCKS = 256;     // per sample: frames beyond 65536 pixels take more than one trip of the grid-stride loop
constexpr int FM_STATS = 8;            // doubles per partial / per sample (6 used)

struct Plane2 {                         // a [B,2,H,W] view with unit x stride (strides in elements)
  const float* p;
  int64_t bs, cs, rs;
};

static inline int fm_blocks(int64_t hw) {
  const int64_t n = (hw + FM_THREADS - 1) / FM_THREADS;
  return (int)(n < FM_MAX_BLOCKS ? n : FM_MAX_BLOCKS);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The sum of one value per thread of a 256-thread block, in a fixed order; the result is valid in thread 0.
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
  v = wave_sum_f64(v);
  __syncthreads();                      // red may still be read from the previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(FM_THREADS) void flow_metrics_partial_kernel(Plane2 pred, Plane2 gt, const float* __restrict__ valid,
                                                                         int64_t valid_bs, int64_t valid_rs, int HW, int W,
                                                                         double* __restrict__ partial) {
  __shared__ double red[FM_THREADS / 64];
  const int b = blockIdx.y;
  const float* p0 = pred.p + b * pred.bs;
  const float* g0p = gt.p + b * gt.bs;
  const float* vp = valid ? valid + b * valid_bs : nullptr;
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t e = (int64_t)blockIdx.x * FM_THREADS + threadIdx.x; e < HW; e += (int64_t)gridDim.x * FM_THREADS) {
    const int y = (int)e / W, x = (int)e - y * W;
    if (vp && !(vp[y * valid_rs + x] >= 0.5f)) continue;
    const int64_t ip = y * pred.rs + x, ig = y * gt.rs + x;
    const float g0 = g0p[ig], g1 = g0p[ig + gt.cs];
    const float d0 = p0[ip] - g0, d1 = p0[ip + pred.cs] - g1;
    const float epe = sqrtf(d0 * d0 + d1 * d1);
    const float mag = sqrtf(g0 * g0 + g1 * g1);
    s[0] += 1.0;
    s[1] += (double)epe;
    s[2] += epe < 1.0f ? 1.0 : 0.0;
    s[3] += epe < 3.0f ? 1.0 : 0.0;
    s[4] += epe < 5.0f ? 1.0 : 0.0;
    s[5] += (epe > 3.0f && epe / mag > 0.05f) ? 1.0 : 0.0;     // mag == 0: inf > 0.05, as evaluate.py:157
  }
  double* out = partial + ((int64_t)b * gridDim.x + blockIdx.x) * FM_STATS;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const double t = block_sum_f64(s[k], red);
    if (threadIdx.x == 0) out[k] = t;
  }
}

__global__ __launch_bounds__(FM_THREADS) void flow_metrics_finalise_kernel(const double* __restrict__ partial, int nblk, int B,
                                                                          double* __restrict__ sample_stats, double* __restrict__ acc) {
  __shared__ double red[FM_THREADS / 64];
  double a[FM_STATS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (threadIdx.x == 0 && acc) {
#pragma unroll
    for (int k = 0; k < FM_STATS; ++k) a[k] = acc[k];
  }
  for (int b = 0; b < B; ++b) {
    double st[6];
#pragma unroll
    for (int k = 0; k < 6; ++k)       // nblk <= FM_MAX_BLOCKS == FM_THREADS: one partial per thread
      st[k] = block_sum_f64((int)threadIdx.x < nblk ? partial[((int64_t)b * nblk + threadIdx.x) * FM_STATS + k] : 0.0, red);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < 6; ++k) sample_stats[(int64_t)b * FM_STATS + k] = st[k];
      sample_stats[(int64_t)b * FM_STATS + 6] = 0.0;
      sample_stats[(int64_t)b * FM_STATS + 7] = 0.0;
      if (acc) {
#pragma unroll
        for (int k = 0; k < 6; ++k) a[k] += st[k];
        if (st[0] > 0.0) { a[6] += st[1] / st[0]; a[7] += 1.0; }     // KITTI's per-image mean (evaluate.py:158)
      }
    }
  }
  if (threadIdx.x == 0 && acc) {
#pragma unroll
    for (int k = 0; k < FM_STATS; ++k) acc[k] = a[k];
  }
}

static_assert(FM_MAX_BLOCKS <= FM_THREADS, "the finalising block reads one partial per thread");

}  // namespace

// Bytes of scratch fsraft_flow_metrics needs for a batch of B frames of H x W (a multiple of 64, so never FS_ERR_ARG's value);
// FS_ERR_ARG for B, H or W below 1, H * W beyond 2^31 - 1 or a size beyond INT_MAX.
extern "C" int fsraft_flow_metrics_scratch_bytes(int B, int H, int W) {
  if (B < 1 || H < 1 || W < 1 || (int64_t)H * W > INT32_MAX) return FS_ERR_ARG;
  const int64_t bytes = (int64_t)B * fm_blocks((int64_t)H * W) * FM_STATS * (int64_t)sizeof(double);
  return bytes > INT32_MAX ? FS_ERR_ARG : (int)bytes;
}

extern "C" int fsraft_flow_metrics(const float* pred, int64_t pred_bs, int64_t pred_cs, int64_t pred_rs,
                                   const float* gt, int64_t gt_bs, int64_t gt_cs, int64_t gt_rs,
                                   const float* valid, int64_t valid_bs, int64_t valid_rs,
                                   int B, int H, int W, double* sample_stats, double* acc,
                                   void* scratch, int64_t scratch_bytes, hipStream_t s) {
  if (!pred || !gt || !sample_stats || !scratch) return FS_ERR_ARG;
  const int need = fsraft_flow_metrics_scratch_bytes(B, H, W);
  if (need == FS_ERR_ARG || scratch_bytes < need) return FS_ERR_ARG;
  if (B > 65535 || ((uintptr_t)sample_stats | (uintptr_t)acc | (uintptr_t)scratch) % sizeof(double)) return FS_ERR_ARG;
  const int nblk = fm_blocks((int64_t)H * W);
  const Plane2 p{pred, pred_bs, pred_cs, pred_rs}, g{gt, gt_bs, gt_cs, gt_rs};
  hipLaunchKernelGGL(flow_metrics_partial_kernel, dim3(nblk, B), dim3(FM_THREADS), 0, s, p, g, valid, valid_bs, valid_rs, H * W, W,
                     (double*)scratch);
  if (fs_launch_status() != FS_OK) return FS_ERR_LAUNCH;
  hipLaunchKernelGGL(flow_metrics_finalise_kernel, dim3(1), dim3(FM_THREADS), 0, s, (const double*)scratch, nblk, B, sample_stats, acc);
  return fs_launch_status();
}
