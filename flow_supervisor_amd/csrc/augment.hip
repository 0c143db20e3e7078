// UnsupAugmentor applied on the device (pytorch/raft_utils/augmentor.py:496-657 with ColorJitter :15-37 and the "* 255" of
// pytorch/train.py:251-258): the parameters are drawn on the host (flow_supervisor_amd/augment.py) and arrive by value, one
// fsraft_aug_params per sample; four kernels apply them to a batch.
//
//   spatial   one thread per frame pixel: undo the vertical flip, the horizontal flip and the window offset, then sample the
//             source -- images with TF2's tf.image.resize(BILINEAR) (half-pixel centres, no antialias), flow and valid with
//             NEAREST_NEIGHBOR, the flow times the scales and the flips' signs.  Writes the frame outputs, the crop's flow and
//             valid, and per-block sums of the crop's raw pixel values (what the contrast step's mean is made of).
//   means     per sample, image and channel, the partial sums in block order -> the mean over the crop
//   colour    one thread per crop pixel, both images: x / 255, brightness, contrast, saturation, hue, clip, * 255; per-block
//             sums of the second image's result (the eraser's mean colour)
//   eraser    for the samples that drew rectangles: the partial sums in block order -> the mean colour -> the rectangles
//
// Interleaved sources ([B][Hs][Ws][3] uint8 in [0, 255] or float in [0, 1]; flow [B][Hs][Ws][2]; valid [B][Hs][Ws]), planar
// fp32 outputs.  Every sum is fp64, per block in a fixed order and the blocks in ascending order: no float atomics, a second
// launch gives the same bits.  No allocation, no synchronisation, no host read: every entry can be captured.
//
// One rounding per operation (no contraction into fused multiply-adds), in the order of the restatement in tests/_augref.py:
// the index arithmetic is TF's float32 arithmetic and a fused multiply-add would move a nearest-neighbour index.
//
// The supervised augmentors (FlowAugmentor, SparseFlowAugmentor: colour -> eraser -> spatial) are a second kernel family on the
// same helpers, further down (fsraft_augment_sup; restated in tests/_supaugref.py).
#include "common.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int AUG_THREADS = 256;
constexpr int AUG_MAX_BLOCKS = 2048;     // per sample and kernel (grid-stride beyond 524288 pixels; the recipe's frame has 442368)
constexpr int AUG_CHUNK = 16;            // samples per launch: their parameters travel in the kernel arguments (1856 bytes)
constexpr int AUG_ERASE_BLOCKS = 8;      // per rectangle (at most 100 x 100 pixels)

struct Chunk { fsraft_aug_params p[AUG_CHUNK]; };
struct EraseList { int n; int sample[AUG_CHUNK]; };     // chunk-local indices of the samples with a rectangle to fill

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The sum of one value per thread of a 256-thread block, in a fixed order; every thread gets the result.
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
  v = wave_sum_f64(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// N sums at once: dst[q] = the sum of v[q] over the block, in the order of block_sum_f64, with one pair of barriers.
template <int N> __device__ __forceinline__ void block_sums_f64(double (&v)[N], double* red, double* __restrict__ dst) {
#pragma unroll
  for (int q = 0; q < N; ++q) v[q] = wave_sum_f64(v[q]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int q = 0; q < N; ++q) red[(threadIdx.x >> 6) * N + q] = v[q];
  }
  __syncthreads();
  if (threadIdx.x < N) dst[threadIdx.x] = (red[threadIdx.x] + red[N + threadIdx.x]) + (red[2 * N + threadIdx.x] + red[3 * N + threadIdx.x]);
}

// n partials with a stride, every thread taking tid, tid + 256, ... in ascending order.
__device__ __forceinline__ double finish_sum(const double* __restrict__ partial, int n, int stride, double* red) {
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += AUG_THREADS) a += partial[(int64_t)i * stride];
  return block_sum_f64(a, red);
}

template <bool U8> __device__ __forceinline__ float px(const void* img, int64_t i) {
  if (U8) return (float)((const uint8_t*)img)[i];
  return ((const float*)img)[i];
}

// tf.image.resize(BILINEAR), half_pixel_centers: src = (dst + 0.5) * (in / out) - 0.5, lo = max(floor(src), 0),
// hi = min(ceil(src), in - 1), weight = src - floor(src).
__device__ __forceinline__ void lerp_taps(int dst, float scale, int in, int& lo, int& hi, float& w) {
  const float src = ((float)dst + 0.5f) * scale - 0.5f;
  const float fl = floorf(src);
  lo = min(max((int)fl, 0), in - 1);      // (the upper bound is never met by a dst inside the resized image; it guards the read)
  hi = min((int)ceilf(src), in - 1);
  w = src - fl;
}

// NEAREST_NEIGHBOR, half_pixel_centers: min(floor((dst + 0.5) * (in / out)), in - 1).
__device__ __forceinline__ int nearest_tap(int dst, float scale, int in) {
  return min((int)floorf(((float)dst + 0.5f) * scale), in - 1);
}

struct Outputs {
  float* frame[2];       // [B][3][Hf][Wf]
  float* frame_flow;     // [B][2][Hf][Wf]
  float* frame_valid;    // [B][1][Hf][Wf]
  float* crop_flow;      // [B][2][h][w]
  float* crop_valid;     // [B][1][h][w]
};

// scratch, in doubles: spatial partials [B][nblk_f][6] | means [B][8] | colour partials [B][nblk_c][3]
struct Scratch {
  double* spatial;
  double* means;
  double* colour;
};

template <bool U8>
__global__ __launch_bounds__(AUG_THREADS) void aug_spatial_kernel(const void* __restrict__ img1, const void* __restrict__ img2,
                                                                  const float* __restrict__ flow, const float* __restrict__ valid,
                                                                  int Hs, int Ws, Chunk chunk, int b0, int Hf, int Wf, int h, int w,
                                                                  Outputs out, double* __restrict__ partial) {
  __shared__ double red[AUG_THREADS / 64 * 6];
  const int bl = blockIdx.y, b = b0 + bl;
  const fsraft_aug_params& P = chunk.p[bl];
  const int64_t src_px = (int64_t)Hs * Ws, frame_px = (int64_t)Hf * Wf, crop_px = (int64_t)h * w;
  const void* src[2] = {U8 ? (const void*)((const uint8_t*)img1 + b * src_px * 3) : (const void*)((const float*)img1 + b * src_px * 3),
                        U8 ? (const void*)((const uint8_t*)img2 + b * src_px * 3) : (const void*)((const float*)img2 + b * src_px * 3)};
  const float* fl = flow + b * src_px * 2;
  const float* va = valid ? valid + b * src_px : nullptr;
  // in / out, the division in float32 as TF's CalculateResizeScale does it
  const float rs_y = (float)Hs / (float)P.th, rs_x = (float)Ws / (float)P.tw;
  const float sign_x = P.hflip ? -1.0f : 1.0f, sign_y = P.vflip ? -1.0f : 1.0f;
  double sum[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t e = (int64_t)blockIdx.x * AUG_THREADS + threadIdx.x; e < frame_px; e += (int64_t)gridDim.x * AUG_THREADS) {
    const int fy = (int)(e / Wf), fx = (int)(e - (int64_t)fy * Wf);
    // frame pixel -> pixel of the resized image: the flips act on the window
    const int ry = (P.vflip ? Hf - 1 - fy : fy) + P.win_y, rx = (P.hflip ? Wf - 1 - fx : fx) + P.win_x;
    float c[2][3], u, v, m;
    if (P.resize) {
      int y0, y1, x0, x1;
      float wy, wx;
      lerp_taps(ry, rs_y, Hs, y0, y1, wy);
      lerp_taps(rx, rs_x, Ws, x0, x1, wx);
      const int64_t tl = ((int64_t)y0 * Ws + x0) * 3, tr = ((int64_t)y0 * Ws + x1) * 3, bl_ = ((int64_t)y1 * Ws + x0) * 3,
                    br = ((int64_t)y1 * Ws + x1) * 3;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float a = px<U8>(src[i], tl + k), bq = px<U8>(src[i], tr + k), cq = px<U8>(src[i], bl_ + k), d = px<U8>(src[i], br + k);
          const float top = a + (bq - a) * wx, bot = cq + (d - cq) * wx;
          c[i][k] = top + (bot - top) * wy;
        }
      }
      const int64_t n = (int64_t)nearest_tap(ry, rs_y, Hs) * Ws + nearest_tap(rx, rs_x, Ws);
      u = fl[2 * n] * P.scale_x;
      v = fl[2 * n + 1] * P.scale_y;
      m = va ? va[n] : 1.0f;
    } else {
      const int64_t n = (int64_t)ry * Ws + rx;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int k = 0; k < 3; ++k) c[i][k] = px<U8>(src[i], n * 3 + k);
      }
      u = fl[2 * n];
      v = fl[2 * n + 1];
      m = va ? va[n] : 1.0f;
    }
    u *= sign_x;
    v *= sign_y;
    if (!U8) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int k = 0; k < 3; ++k) c[i][k] *= 255.0f;
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int k = 0; k < 3; ++k) out.frame[i][(b * 3 + k) * frame_px + e] = c[i][k];
    }
    out.frame_flow[(b * 2 + 0) * frame_px + e] = u;
    out.frame_flow[(b * 2 + 1) * frame_px + e] = v;
    out.frame_valid[b * frame_px + e] = m;
    const int cy = fy - P.crop_y, cx = fx - P.crop_x;
    if (cy >= 0 && cy < h && cx >= 0 && cx < w) {
      const int64_t o = (int64_t)cy * w + cx;
      out.crop_flow[(b * 2 + 0) * crop_px + o] = u;
      out.crop_flow[(b * 2 + 1) * crop_px + o] = v;
      out.crop_valid[b * crop_px + o] = m;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int k = 0; k < 3; ++k) sum[i * 3 + k] += (double)c[i][k];
      }
    }
  }
  block_sums_f64<6>(sum, red, partial + ((int64_t)b * gridDim.x + blockIdx.x) * 6);
}

// means[b][i * 3 + k]: the mean over the crop of image i, channel k, of x / 255.  One block per sample and quantity.
__global__ __launch_bounds__(AUG_THREADS) void aug_means_kernel(const double* __restrict__ partial, int nblk, int b0, double crop_px,
                                                                double* __restrict__ means) {
  __shared__ double red[AUG_THREADS / 64];
  const int q = blockIdx.x, b = b0 + blockIdx.y;
  const double t = finish_sum(partial + (int64_t)b * nblk * 6 + q, nblk, 6, red);
  if (threadIdx.x == 0) means[b * 8 + q] = t / crop_px / 255.0;
}

__device__ __forceinline__ float clip01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }

// The RGB -> HSV -> RGB trip of TF's fused adjust_saturation / adjust_hue: v = max, c = max - min, s = c / v (0 when v <= 0),
// h the hexcone sector formula in [0, 1) (0 when c = 0); SAT: s <- clip(s * f, 0, 1), else h <- frac(h + f);
// rgb = ((d - 1) * s + 1) * v with d = clip(|6h - 3| - 1), clip(2 - |6h - 2|), clip(2 - |6h - 4|).
template <bool SAT> __device__ __forceinline__ void hsv_trip(float& r, float& g, float& b, float f) {
  const float v = fmaxf(r, fmaxf(g, b)), c = v - fminf(r, fminf(g, b));
  float s = v > 0.0f ? c / v : 0.0f;
  float h = 0.0f;
  if (c > 0.0f) {
    if (r == v) {
      h = ((g - b) / c) / 6.0f;
      if (h < 0.0f) h += 1.0f;
    } else if (g == v) {
      h = (2.0f + (b - r) / c) / 6.0f;
    } else {
      h = (4.0f + (r - g) / c) / 6.0f;
    }
  }
  if (SAT) {
    s = clip01(s * f);
  } else {
    h = h + f;
    h = h - floorf(h);
  }
  const float h6 = 6.0f * h;
  const float dr = clip01(fabsf(h6 - 3.0f) - 1.0f), dg = clip01(2.0f - fabsf(h6 - 2.0f)), db = clip01(2.0f - fabsf(h6 - 4.0f));
  r = ((dr - 1.0f) * s + 1.0f) * v;
  g = ((dg - 1.0f) * s + 1.0f) * v;
  b = ((db - 1.0f) * s + 1.0f) * v;
}

__global__ __launch_bounds__(AUG_THREADS) void aug_colour_kernel(const float* __restrict__ frame1, const float* __restrict__ frame2, int Hf,
                                                                 int Wf, Chunk chunk, int b0, int h, int w, const double* __restrict__ means,
                                                                 float* __restrict__ crop1, float* __restrict__ crop2,
                                                                 double* __restrict__ partial) {
  __shared__ double red[AUG_THREADS / 64 * 3];
  const int bl = blockIdx.y, b = b0 + bl;
  const fsraft_aug_params& P = chunk.p[bl];
  const int64_t frame_px = (int64_t)Hf * Wf, crop_px = (int64_t)h * w;
  const float* frame[2] = {frame1, frame2};
  float* crop[2] = {crop1, crop2};
  float mean[2][3];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      // symmetric: one mean over both crops, which the reference concatenates into one 2h x w image before random_contrast
      const double m = P.asym ? means[b * 8 + i * 3 + k] : (means[b * 8 + k] + means[b * 8 + 3 + k]) * 0.5;
      mean[i][k] = P.brightness[i] * (float)m;                                                   // of the brightness-scaled crop
    }
  }
  double sum[3] = {0.0, 0.0, 0.0};
  for (int64_t e = (int64_t)blockIdx.x * AUG_THREADS + threadIdx.x; e < crop_px; e += (int64_t)gridDim.x * AUG_THREADS) {
    const int y = (int)(e / w), x = (int)(e - (int64_t)y * w);
    const int64_t o = (int64_t)(y + P.crop_y) * Wf + (x + P.crop_x);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      float c[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float t = frame[i][(b * 3 + k) * frame_px + o] / 255.0f * P.brightness[i];
        c[k] = (t - mean[i][k]) * P.contrast[i] + mean[i][k];
      }
      hsv_trip<true>(c[0], c[1], c[2], P.saturation[i]);
      hsv_trip<false>(c[0], c[1], c[2], P.hue[i]);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        c[k] = clip01(c[k]) * 255.0f;
        crop[i][(b * 3 + k) * crop_px + e] = c[k];
        if (i == 1) sum[k] += (double)c[k];
      }
    }
  }
  block_sums_f64<3>(sum, red, partial + ((int64_t)b * gridDim.x + blockIdx.x) * 3);
}

// grid (AUG_ERASE_BLOCKS, 2 rectangles, samples of the list).  Every block adds its sample's partials itself (the same order,
// so the same mean in every block); the mean is that of the crop before any rectangle, which both rectangles are filled with.
__global__ __launch_bounds__(AUG_THREADS) void aug_eraser_kernel(Chunk chunk, EraseList list, int b0, int h, int w,
                                                                 const double* __restrict__ partial, int nblk, float* __restrict__ crop2) {
  __shared__ double red[AUG_THREADS / 64];
  const int bl = list.sample[blockIdx.z], b = b0 + bl, r = blockIdx.y;
  const fsraft_aug_params& P = chunk.p[bl];
  if (r >= P.nrect) return;
  const int x0 = P.rect[r][0], y0 = P.rect[r][1], dx = P.rect[r][2], dy = P.rect[r][3];
  const int n = dx * dy;
  if (n <= 0) return;
  const int64_t crop_px = (int64_t)h * w;
  float mean[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) mean[k] = (float)(finish_sum(partial + (int64_t)b * nblk * 3 + k, nblk, 3, red) / (double)crop_px);
  for (int e = blockIdx.x * AUG_THREADS + threadIdx.x; e < n; e += gridDim.x * AUG_THREADS) {
    const int y = e / dx, x = e - y * dx;
    const int64_t o = (int64_t)(y0 + y) * w + (x0 + x);
#pragma unroll
    for (int k = 0; k < 3; ++k) crop2[(b * 3 + k) * crop_px + o] = mean[k];
  }
}

static inline int aug_blocks(int64_t px) {
  const int64_t n = (px + AUG_THREADS - 1) / AUG_THREADS;
  return (int)(n < AUG_MAX_BLOCKS ? n : AUG_MAX_BLOCKS);
}

static inline bool aligned(const void* p, int a) { return (uintptr_t)p % a == 0; }
static inline bool bit(int v) { return v == 0 || v == 1; }
static inline bool finite_f(float v) { return v - v == 0.0f; }

static bool sizes_ok(int B, int Hf, int Wf, int h, int w) {
  return B >= 1 && Hf >= 1 && Wf >= 1 && h >= 1 && w >= 1 && h <= Hf && w <= Wf && (int64_t)Hf * Wf * 3 <= INT32_MAX;
}

// What both entries ask of a parameter set: flags, the resized size, finite factors, and rectangles inside an h x w image (the
// crop for fsraft_augment, the source for fsraft_augment_sup).
static bool factors_ok(const fsraft_aug_params& P, int Hs, int Ws, int h, int w) {
  if (!bit(P.resize) || !bit(P.hflip) || !bit(P.vflip) || !bit(P.asym)) return false;
  if (P.th < 1 || P.tw < 1 || (int64_t)P.th * P.tw > INT32_MAX) return false;
  if (!P.resize && (P.th != Hs || P.tw != Ws)) return false;
  if (!finite_f(P.scale_x) || !finite_f(P.scale_y)) return false;
  for (int i = 0; i < 2; ++i)
    if (!finite_f(P.brightness[i]) || !finite_f(P.contrast[i]) || !finite_f(P.saturation[i]) || !finite_f(P.hue[i])) return false;
  // symmetric colour is one quadruple for the stacked pair: the contrast mean over both images is that of one brightness
  if (!P.asym && (P.brightness[0] != P.brightness[1] || P.contrast[0] != P.contrast[1] || P.saturation[0] != P.saturation[1] ||
                  P.hue[0] != P.hue[1]))
    return false;
  if (P.nrect < 0 || P.nrect > 2) return false;
  for (int r = 0; r < P.nrect; ++r) {
    const int x0 = P.rect[r][0], y0 = P.rect[r][1], dx = P.rect[r][2], dy = P.rect[r][3];
    if (x0 < 0 || y0 < 0 || dx < 0 || dy < 0 || dx > w - x0 || dy > h - y0) return false;
  }
  return true;
}

static bool params_ok(const fsraft_aug_params& P, int Hs, int Ws, int Hf, int Wf, int h, int w) {
  if (!factors_ok(P, Hs, Ws, h, w)) return false;
  if (P.th < Hf || P.tw < Wf) return false;                                    // a resized image smaller than the frame
  if (P.win_y < 0 || P.win_x < 0 || P.win_y > P.th - Hf || P.win_x > P.tw - Wf) return false;
  return P.crop_y >= 0 && P.crop_x >= 0 && P.crop_y <= Hf - h && P.crop_x <= Wf - w;
}

// ------------------------------------------------------------------------------------------------------------------------
// FlowAugmentor / SparseFlowAugmentor (augmentor.py:39-188, :191-330): colour -> eraser -> spatial, so the colour step and the
// eraser live in SOURCE coordinates and the resize interpolates pixels that were already jittered, clipped and erased.  Nothing
// of source or resized size is written: the output kernel evaluates the colour step and the rectangle test at each of its taps.
//
//   sums      one thread per source pixel, both images: per-block sums of the raw values (the contrast step's mean)
//   means     the partial sums in block order -> the six means of x (source / 255, or the float source)
//   photo     for the samples with a rectangle: per-block sums of the second image after the colour step (the eraser's colour)
//   erase     those partial sums in block order -> the mean colour
//   output    one thread per crop pixel: at most four taps per image, each through the colour step and the rectangle test, then
//             the bilinear weights; flow with the same taps (FlowAugmentor) or the nearest neighbour (SparseFlowAugmentor)
//
// scratch, in doubles: sums partials [B][nblk][6] | means [B][SUP_MEANS] | photo partials [B][nblk][3], nblk of the source

constexpr int SUP_MEANS = 12;            // per sample: 6 contrast means, 3 eraser colours, 3 unused

template <bool U8>
__global__ __launch_bounds__(AUG_THREADS) void sup_sums_kernel(const void* __restrict__ img1, const void* __restrict__ img2, int64_t src_px,
                                                               int b0, double* __restrict__ partial) {
  __shared__ double red[AUG_THREADS / 64 * 6];
  const int b = b0 + blockIdx.y;
  const void* src[2] = {U8 ? (const void*)((const uint8_t*)img1 + b * src_px * 3) : (const void*)((const float*)img1 + b * src_px * 3),
                        U8 ? (const void*)((const uint8_t*)img2 + b * src_px * 3) : (const void*)((const float*)img2 + b * src_px * 3)};
  double sum[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t e = (int64_t)blockIdx.x * AUG_THREADS + threadIdx.x; e < src_px; e += (int64_t)gridDim.x * AUG_THREADS) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int k = 0; k < 3; ++k) sum[i * 3 + k] += (double)px<U8>(src[i], e * 3 + k);
    }
  }
  block_sums_f64<6>(sum, red, partial + ((int64_t)b * gridDim.x + blockIdx.x) * 6);
}

// means[b][i * 3 + k]: the mean over the source of image i, channel k, of x (unit 255 for a uint8 source, 1 for a float one).
__global__ __launch_bounds__(AUG_THREADS) void sup_means_kernel(const double* __restrict__ partial, int nblk, int b0, double src_px,
                                                                double unit, double* __restrict__ means) {
  __shared__ double red[AUG_THREADS / 64];
  const int q = blockIdx.x, b = b0 + blockIdx.y;
  const double t = finish_sum(partial + (int64_t)b * nblk * 6 + q, nblk, 6, red);
  if (threadIdx.x == 0) means[b * SUP_MEANS + q] = t / src_px / unit;
}

// The contrast step's means of image i: of the brightness-scaled source, symmetric over both sources (stacked into one image).
__device__ __forceinline__ void sup_contrast_mean(const fsraft_aug_params& P, const double* __restrict__ means, int i, float (&mean)[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double m = P.asym ? means[i * 3 + k] : (means[k] + means[3 + k]) * 0.5;
    mean[k] = P.brightness[i] * (float)m;
  }
}

// P_i at one source pixel: clip01(hue(sat(contrast(x * brightness)))), in [0, 1].
template <bool U8>
__device__ __forceinline__ void sup_photo(const void* src, int64_t pixel, const fsraft_aug_params& P, int i, const float (&mean)[3],
                                          float (&c)[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float t = px<U8>(src, pixel * 3 + k);
    if (U8) t = t / 255.0f;
    t = t * P.brightness[i];
    c[k] = (t - mean[k]) * P.contrast[i] + mean[k];
  }
  hsv_trip<true>(c[0], c[1], c[2], P.saturation[i]);
  hsv_trip<false>(c[0], c[1], c[2], P.hue[i]);
#pragma unroll
  for (int k = 0; k < 3; ++k) c[k] = clip01(c[k]);
}

// grid (blocks of the source, samples of the list): per-block sums of P_2 over the whole source.
template <bool U8>
__global__ __launch_bounds__(AUG_THREADS) void sup_photo_sums_kernel(const void* __restrict__ img2, int64_t src_px, Chunk chunk, EraseList list,
                                                                     int b0, const double* __restrict__ means, double* __restrict__ partial) {
  __shared__ double red[AUG_THREADS / 64 * 3];
  const int bl = list.sample[blockIdx.y], b = b0 + bl;
  const fsraft_aug_params& P = chunk.p[bl];
  const void* src = U8 ? (const void*)((const uint8_t*)img2 + b * src_px * 3) : (const void*)((const float*)img2 + b * src_px * 3);
  float mean[3];
  sup_contrast_mean(P, means + b * SUP_MEANS, 1, mean);
  double sum[3] = {0.0, 0.0, 0.0};
  for (int64_t e = (int64_t)blockIdx.x * AUG_THREADS + threadIdx.x; e < src_px; e += (int64_t)gridDim.x * AUG_THREADS) {
    float c[3];
    sup_photo<U8>(src, e, P, 1, mean, c);
#pragma unroll
    for (int k = 0; k < 3; ++k) sum[k] += (double)c[k];
  }
  block_sums_f64<3>(sum, red, partial + ((int64_t)b * gridDim.x + blockIdx.x) * 3);
}

// means[b][6 + k]: the mean of P_2 over the whole source, before any rectangle.  grid (3, samples of the list).
__global__ __launch_bounds__(AUG_THREADS) void sup_erase_mean_kernel(const double* __restrict__ partial, int nblk, EraseList list, int b0,
                                                                     double src_px, double* __restrict__ means) {
  __shared__ double red[AUG_THREADS / 64];
  const int k = blockIdx.x, b = b0 + list.sample[blockIdx.y];
  const double t = finish_sum(partial + (int64_t)b * nblk * 3 + k, nblk, 3, red);
  if (threadIdx.x == 0) means[b * SUP_MEANS + 6 + k] = t / src_px;
}

__device__ __forceinline__ bool sup_erased(const fsraft_aug_params& P, int y, int x) {
  bool in = false;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int dx = x - P.rect[r][0], dy = y - P.rect[r][1];
    in = in || (r < P.nrect && dx >= 0 && dx < P.rect[r][2] && dy >= 0 && dy < P.rect[r][3]);
  }
  return in;
}

// E_i at one source pixel: the eraser's colour inside a rectangle of image 2, else P_i.
template <bool U8>
__device__ __forceinline__ void sup_tap(const void* src, int y, int x, int Ws, const fsraft_aug_params& P, int i, const float (&mean)[3],
                                        const float (&fill)[3], float (&c)[3]) {
  if (i == 1 && sup_erased(P, y, x)) {
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = fill[k];
  } else {
    sup_photo<U8>(src, (int64_t)y * Ws + x, P, i, mean, c);
  }
}

template <bool U8>
__global__ __launch_bounds__(AUG_THREADS) void sup_output_kernel(const void* __restrict__ img1, const void* __restrict__ img2,
                                                                 const float* __restrict__ flow, const float* __restrict__ valid, int Hs, int Ws,
                                                                 Chunk chunk, int b0, int h, int w, int flow_mode,
                                                                 const double* __restrict__ means, float* __restrict__ crop1,
                                                                 float* __restrict__ crop2, float* __restrict__ crop_flow,
                                                                 float* __restrict__ crop_valid) {
  const int bl = blockIdx.y, b = b0 + bl;
  const fsraft_aug_params& P = chunk.p[bl];
  const int64_t src_px = (int64_t)Hs * Ws, crop_px = (int64_t)h * w;
  const void* src[2] = {U8 ? (const void*)((const uint8_t*)img1 + b * src_px * 3) : (const void*)((const float*)img1 + b * src_px * 3),
                        U8 ? (const void*)((const uint8_t*)img2 + b * src_px * 3) : (const void*)((const float*)img2 + b * src_px * 3)};
  float* crop[2] = {crop1, crop2};
  const float* fl = flow + b * src_px * 2;
  const float* va = (valid && flow_mode == FSRAFT_AUG_FLOW_NEAREST) ? valid + b * src_px : nullptr;
  float mean[2][3], fill[3] = {0.0f, 0.0f, 0.0f};
  sup_contrast_mean(P, means + b * SUP_MEANS, 0, mean[0]);
  sup_contrast_mean(P, means + b * SUP_MEANS, 1, mean[1]);
  bool any = false;
  for (int r = 0; r < P.nrect; ++r) any = any || (P.rect[r][2] > 0 && P.rect[r][3] > 0);
  if (any) {      // (the eraser's colour exists for these samples only)
#pragma unroll
    for (int k = 0; k < 3; ++k) fill[k] = (float)means[b * SUP_MEANS + 6 + k];
  }
  // in / out, the division in float32 as TF's CalculateResizeScale does it
  const float rs_y = (float)Hs / (float)P.th, rs_x = (float)Ws / (float)P.tw;
  const float sign_x = P.hflip ? -1.0f : 1.0f, sign_y = P.vflip ? -1.0f : 1.0f;
  for (int64_t e = (int64_t)blockIdx.x * AUG_THREADS + threadIdx.x; e < crop_px; e += (int64_t)gridDim.x * AUG_THREADS) {
    const int y = (int)(e / w), x = (int)(e - (int64_t)y * w);
    // crop pixel -> pixel of the resized image: the flips act on the whole resized image
    const int ry = P.vflip ? P.th - 1 - (P.crop_y + y) : P.crop_y + y, rx = P.hflip ? P.tw - 1 - (P.crop_x + x) : P.crop_x + x;
    float u, v, m = 1.0f;
    if (P.resize) {
      int y0, y1, x0, x1;
      float wy, wx;
      lerp_taps(ry, rs_y, Hs, y0, y1, wy);
      lerp_taps(rx, rs_x, Ws, x0, x1, wx);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        float tl[3], tr[3], bl_[3], br[3];
        sup_tap<U8>(src[i], y0, x0, Ws, P, i, mean[i], fill, tl);
        sup_tap<U8>(src[i], y0, x1, Ws, P, i, mean[i], fill, tr);
        sup_tap<U8>(src[i], y1, x0, Ws, P, i, mean[i], fill, bl_);
        sup_tap<U8>(src[i], y1, x1, Ws, P, i, mean[i], fill, br);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float top = tl[k] + (tr[k] - tl[k]) * wx, bot = bl_[k] + (br[k] - bl_[k]) * wx;
          crop[i][(b * 3 + k) * crop_px + e] = (top + (bot - top) * wy) * 255.0f;
        }
      }
      if (flow_mode == FSRAFT_AUG_FLOW_BILINEAR) {
        const int64_t tl = ((int64_t)y0 * Ws + x0) * 2, tr = ((int64_t)y0 * Ws + x1) * 2, bl_ = ((int64_t)y1 * Ws + x0) * 2,
                      br = ((int64_t)y1 * Ws + x1) * 2;
        const float utop = fl[tl] + (fl[tr] - fl[tl]) * wx, ubot = fl[bl_] + (fl[br] - fl[bl_]) * wx;
        const float vtop = fl[tl + 1] + (fl[tr + 1] - fl[tl + 1]) * wx, vbot = fl[bl_ + 1] + (fl[br + 1] - fl[bl_ + 1]) * wx;
        u = (utop + (ubot - utop) * wy) * P.scale_x;
        v = (vtop + (vbot - vtop) * wy) * P.scale_y;
      } else {
        const int64_t n = (int64_t)nearest_tap(ry, rs_y, Hs) * Ws + nearest_tap(rx, rs_x, Ws);
        u = fl[2 * n] * P.scale_x;
        v = fl[2 * n + 1] * P.scale_y;
        if (va) m = va[n];
      }
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        float c[3];
        sup_tap<U8>(src[i], ry, rx, Ws, P, i, mean[i], fill, c);
#pragma unroll
        for (int k = 0; k < 3; ++k) crop[i][(b * 3 + k) * crop_px + e] = c[k] * 255.0f;
      }
      const int64_t n = (int64_t)ry * Ws + rx;
      u = fl[2 * n];
      v = fl[2 * n + 1];
      if (va) m = va[n];
    }
    crop_flow[(b * 2 + 0) * crop_px + e] = u * sign_x;
    crop_flow[(b * 2 + 1) * crop_px + e] = v * sign_y;
    crop_valid[b * crop_px + e] = m;
  }
}

static bool sup_params_ok(const fsraft_aug_params& P, int Hs, int Ws, int h, int w) {
  if (!factors_ok(P, Hs, Ws, Hs, Ws)) return false;                            // rectangles are in source coordinates
  if (P.win_y != 0 || P.win_x != 0) return false;                              // the frame is the whole resized image
  if (P.th < h || P.tw < w) return false;                                      // a resized image smaller than the crop
  return P.crop_y >= 0 && P.crop_x >= 0 && P.crop_y <= P.th - h && P.crop_x <= P.tw - w;
}

}  // namespace

extern "C" int fsraft_augment_scratch_bytes(int B, int Hf, int Wf, int h, int w) {
  if (!sizes_ok(B, Hf, Wf, h, w)) return FS_ERR_ARG;
  const int64_t doubles = (int64_t)B * ((int64_t)aug_blocks((int64_t)Hf * Wf) * 6 + 8 + (int64_t)aug_blocks((int64_t)h * w) * 3);
  const int64_t bytes = (doubles * 8 + 63) / 64 * 64;
  return bytes > INT32_MAX ? FS_ERR_ARG : (int)bytes;
}

extern "C" int fsraft_augment(const void* image1, const void* image2, int dtype, const float* flow, const float* valid, int B, int Hs,
                              int Ws, const fsraft_aug_params* params, int Hf, int Wf, int h, int w, float* frame1, float* frame2,
                              float* frame_flow, float* frame_valid, float* crop1, float* crop2, float* crop_flow, float* crop_valid,
                              void* scratch, int64_t scratch_bytes, hipStream_t s) {
  if (!image1 || !image2 || !flow || !params || !frame1 || !frame2 || !frame_flow || !frame_valid || !crop1 || !crop2 || !crop_flow ||
      !crop_valid || !scratch)
    return FS_ERR_ARG;
  if (dtype != FSRAFT_AUG_U8 && dtype != FSRAFT_AUG_F32) return FS_ERR_ARG;
  const int ia = dtype == FSRAFT_AUG_F32 ? 4 : 1;
  if (!aligned(image1, ia) || !aligned(image2, ia) || !aligned(flow, 4) || !aligned(valid, 4) || !aligned(frame1, 4) || !aligned(frame2, 4) ||
      !aligned(frame_flow, 4) || !aligned(frame_valid, 4) || !aligned(crop1, 4) || !aligned(crop2, 4) || !aligned(crop_flow, 4) ||
      !aligned(crop_valid, 4) || !aligned(scratch, 8))
    return FS_ERR_ARG;
  if (Hs < 1 || Ws < 1 || (int64_t)Hs * Ws * 3 > INT32_MAX) return FS_ERR_ARG;
  const int need = fsraft_augment_scratch_bytes(B, Hf, Wf, h, w);
  if (need == FS_ERR_ARG || scratch_bytes < need) return FS_ERR_ARG;
  for (int b = 0; b < B; ++b)
    if (!params_ok(params[b], Hs, Ws, Hf, Wf, h, w)) return FS_ERR_ARG;

  const int nblk_f = aug_blocks((int64_t)Hf * Wf), nblk_c = aug_blocks((int64_t)h * w);
  Scratch sc;
  sc.spatial = (double*)scratch;
  sc.means = sc.spatial + (int64_t)B * nblk_f * 6;
  sc.colour = sc.means + (int64_t)B * 8;
  const Outputs out{{frame1, frame2}, frame_flow, frame_valid, crop_flow, crop_valid};
  for (int b0 = 0; b0 < B; b0 += AUG_CHUNK) {
    const int nb = B - b0 < AUG_CHUNK ? B - b0 : AUG_CHUNK;
    Chunk chunk;
    EraseList list;
    list.n = 0;
    for (int i = 0; i < AUG_CHUNK; ++i) {
      chunk.p[i] = params[b0 + (i < nb ? i : 0)];
      list.sample[i] = 0;
    }
    for (int i = 0; i < nb; ++i) {
      bool any = false;
      for (int r = 0; r < chunk.p[i].nrect; ++r) any = any || (chunk.p[i].rect[r][2] > 0 && chunk.p[i].rect[r][3] > 0);
      if (any) list.sample[list.n++] = i;
    }
    if (dtype == FSRAFT_AUG_U8)
      hipLaunchKernelGGL(aug_spatial_kernel<true>, dim3(nblk_f, nb), dim3(AUG_THREADS), 0, s, image1, image2, flow, valid, Hs, Ws, chunk, b0,
                         Hf, Wf, h, w, out, sc.spatial);
    else
      hipLaunchKernelGGL(aug_spatial_kernel<false>, dim3(nblk_f, nb), dim3(AUG_THREADS), 0, s, image1, image2, flow, valid, Hs, Ws, chunk, b0,
                         Hf, Wf, h, w, out, sc.spatial);
    if (fs_launch_status() != FS_OK) return FS_ERR_LAUNCH;
    hipLaunchKernelGGL(aug_means_kernel, dim3(6, nb), dim3(AUG_THREADS), 0, s, (const double*)sc.spatial, nblk_f, b0, (double)h * w, sc.means);
    if (fs_launch_status() != FS_OK) return FS_ERR_LAUNCH;
    hipLaunchKernelGGL(aug_colour_kernel, dim3(nblk_c, nb), dim3(AUG_THREADS), 0, s, (const float*)frame1, (const float*)frame2, Hf, Wf, chunk,
                       b0, h, w, (const double*)sc.means, crop1, crop2, sc.colour);
    if (fs_launch_status() != FS_OK) return FS_ERR_LAUNCH;
    if (list.n > 0) {
      hipLaunchKernelGGL(aug_eraser_kernel, dim3(AUG_ERASE_BLOCKS, 2, list.n), dim3(AUG_THREADS), 0, s, chunk, list, b0, h, w,
                         (const double*)sc.colour, nblk_c, crop2);
      if (fs_launch_status() != FS_OK) return FS_ERR_LAUNCH;
    }
  }
  return FS_OK;
}

extern "C" int fsraft_augment_sup_scratch_bytes(int B, int Hs, int Ws) {
  if (B < 1 || Hs < 1 || Ws < 1 || (int64_t)Hs * Ws * 3 > INT32_MAX) return FS_ERR_ARG;
  const int64_t doubles = (int64_t)B * ((int64_t)aug_blocks((int64_t)Hs * Ws) * (6 + 3) + SUP_MEANS);
  const int64_t bytes = (doubles * 8 + 63) / 64 * 64;
  return bytes > INT32_MAX ? FS_ERR_ARG : (int)bytes;
}

extern "C" int fsraft_augment_sup(const void* image1, const void* image2, int dtype, const float* flow, const float* valid, int flow_mode,
                                  int B, int Hs, int Ws, const fsraft_aug_params* params, int h, int w, float* crop1, float* crop2,
                                  float* crop_flow, float* crop_valid, void* scratch, int64_t scratch_bytes, hipStream_t s) {
  if (!image1 || !image2 || !flow || !params || !crop1 || !crop2 || !crop_flow || !crop_valid || !scratch) return FS_ERR_ARG;
  if (dtype != FSRAFT_AUG_U8 && dtype != FSRAFT_AUG_F32) return FS_ERR_ARG;
  if (flow_mode != FSRAFT_AUG_FLOW_BILINEAR && flow_mode != FSRAFT_AUG_FLOW_NEAREST) return FS_ERR_ARG;
  const int ia = dtype == FSRAFT_AUG_F32 ? 4 : 1;
  if (!aligned(image1, ia) || !aligned(image2, ia) || !aligned(flow, 4) || !aligned(valid, 4) || !aligned(crop1, 4) || !aligned(crop2, 4) ||
      !aligned(crop_flow, 4) || !aligned(crop_valid, 4) || !aligned(scratch, 8))
    return FS_ERR_ARG;
  if (h < 1 || w < 1 || (int64_t)h * w * 3 > INT32_MAX) return FS_ERR_ARG;
  const int need = fsraft_augment_sup_scratch_bytes(B, Hs, Ws);
  if (need == FS_ERR_ARG || scratch_bytes < need) return FS_ERR_ARG;
  for (int b = 0; b < B; ++b)
    if (!sup_params_ok(params[b], Hs, Ws, h, w)) return FS_ERR_ARG;

  const int64_t src_px = (int64_t)Hs * Ws;
  const int nblk_s = aug_blocks(src_px), nblk_c = aug_blocks((int64_t)h * w);
  double* sums = (double*)scratch;
  double* means = sums + (int64_t)B * nblk_s * 6;
  double* photo = means + (int64_t)B * SUP_MEANS;
  const bool u8 = dtype == FSRAFT_AUG_U8;
  for (int b0 = 0; b0 < B; b0 += AUG_CHUNK) {
    const int nb = B - b0 < AUG_CHUNK ? B - b0 : AUG_CHUNK;
    Chunk chunk;
    EraseList list;
    list.n = 0;
    for (int i = 0; i < AUG_CHUNK; ++i) {
      chunk.p[i] = params[b0 + (i < nb ? i : 0)];
      list.sample[i] = 0;
    }
    for (int i = 0; i < nb; ++i) {
      bool any = false;
      for (int r = 0; r < chunk.p[i].nrect; ++r) any = any || (chunk.p[i].rect[r][2] > 0 && chunk.p[i].rect[r][3] > 0);
      if (any) list.sample[list.n++] = i;
    }
    if (u8)
      hipLaunchKernelGGL(sup_sums_kernel<true>, dim3(nblk_s, nb), dim3(AUG_THREADS), 0, s, image1, image2, src_px, b0, sums);
    else
      hipLaunchKernelGGL(sup_sums_kernel<false>, dim3(nblk_s, nb), dim3(AUG_THREADS), 0, s, image1, image2, src_px, b0, sums);
    if (fs_launch_status() != FS_OK) return FS_ERR_LAUNCH;
    hipLaunchKernelGGL(sup_means_kernel, dim3(6, nb), dim3(AUG_THREADS), 0, s, (const double*)sums, nblk_s, b0, (double)src_px,
                       u8 ? 255.0 : 1.0, means);
    if (fs_launch_status() != FS_OK) return FS_ERR_LAUNCH;
    if (list.n > 0) {
      if (u8)
        hipLaunchKernelGGL(sup_photo_sums_kernel<true>, dim3(nblk_s, list.n), dim3(AUG_THREADS), 0, s, image2, src_px, chunk, list, b0,
                           (const double*)means, photo);
      else
        hipLaunchKernelGGL(sup_photo_sums_kernel<false>, dim3(nblk_s, list.n), dim3(AUG_THREADS), 0, s, image2, src_px, chunk, list, b0,
                           (const double*)means, photo);
      if (fs_launch_status() != FS_OK) return FS_ERR_LAUNCH;
      hipLaunchKernelGGL(sup_erase_mean_kernel, dim3(3, list.n), dim3(AUG_THREADS), 0, s, (const double*)photo, nblk_s, list, b0,
                         (double)src_px, means);
      if (fs_launch_status() != FS_OK) return FS_ERR_LAUNCH;
    }
    if (u8)
      hipLaunchKernelGGL(sup_output_kernel<true>, dim3(nblk_c, nb), dim3(AUG_THREADS), 0, s, image1, image2, flow, valid, Hs, Ws, chunk, b0, h,
                         w, flow_mode, (const double*)means, crop1, crop2, crop_flow, crop_valid);
    else
      hipLaunchKernelGGL(sup_output_kernel<false>, dim3(nblk_c, nb), dim3(AUG_THREADS), 0, s, image1, image2, flow, valid, Hs, Ws, chunk, b0, h,
                         w, flow_mode, (const double*)means, crop1, crop2, crop_flow, crop_valid);
    if (fs_launch_status() != FS_OK) return FS_ERR_LAUNCH;
  }
  return FS_OK;
}
