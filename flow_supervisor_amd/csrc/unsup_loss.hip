// The SMURF photometric loss of the unsupervised trainer (raft/unsup_loss.py UnsupervisedLoss over
// raft/smurf_models/smurf_utils.py): the 'wang' range map, the census loss on the warped second image with its flow gradient,
// and the edge-aware smoothness terms with theirs.  PyTorch layout: images [B,3,H,W] in [0,1], flows [B,2,H,W] with channel
// 0 = x; every view is read through element strides with a unit x stride, and the images may be full frames of which sample b
// uses the window at (crop_y[b], crop_x[b]) (smurf_utils.py:614-647), so neither a crop nor an un-padded prediction is copied.
//
// Range map (compute_range_map, downsampling 1): every source pixel adds its four bilinear weights to the pixels it lands
// between.  The sum is taken in 64-bit fixed point (units of 2^-32) with integer atomics, which commute: the result does not
// depend on the order of arrival, and a second pass converts to fp32.
//
// Census (census_loss, patch 7): a 32 x 16 tile of pixels per workgroup; the gray value of image i and of the warped image j
// are staged in LDS with a 3-pixel halo and the 49 soft-hamming terms are formed out of that, so the 49-channel census tensors
// of the reference never exist.  The forward saves two planes, the warped gray value gB and h = M * 0.4 * (ham + 0.01)^-0.6;
// the backward is a gather over the same tile shape:
//   dL/dgB[q] = sum_d (h[q] + h[q + d]) * phi'(u) * psi'(gB[q + d] - gB[q]),  u = psi(gA[q + d] - gA[q]) - psi(gB[q + d] - gB[q]),
// psi(d) = d / sqrt(0.81 + d^2), phi(u) = u^2 / (0.1 + u^2): the h[q] part is q's own patch (it is the centre of every one of
// its 49 terms), the h[q + d] part the patches of the neighbours q belongs to; psi is odd and phi' is odd, so both meet in one
// expression.  A pixel outside the mask still receives a gradient from the patches of its unmasked neighbours.
//
// Sums: every workgroup leaves its partial sums (fp64) in caller-provided scratch and one finalising block adds them in
// workgroup order.  No allocation, no synchronisation and no host read of device memory, so every entry can be captured.
#include "common.hpp"

namespace {

constexpr int UL_THREADS = 256;
constexpr int UL_MAX_BLOCKS = 256;       // smoothness, per sample (grid-stride beyond 65536 pixels)
constexpr int UL_CHUNK = 32;             // samples per launch of a kernel that takes crop offsets by value
constexpr int CT_W = 32, CT_H = 16, CT_R = 3;
constexpr int CT_LW = CT_W + 2 * CT_R, CT_LH = CT_H + 2 * CT_R, CT_N = CT_LW * CT_LH;

struct View {                             // [B,C,H,W] with unit x stride (strides in elements)
  const float* p;
  int64_t bs, cs, rs;
};
struct Crops { int y[UL_CHUNK], x[UL_CHUNK]; };

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The sum of one value per thread of a 256-thread block, in a fixed order; the result is valid in thread 0.
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
  v = wave_sum_f64(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// Sum of n partial pairs, every thread taking partials tid, tid + 256, ... in ascending order.
__device__ __forceinline__ void sum_pairs(const double* __restrict__ partial, int64_t n, double* red, double& s0, double& s1) {
  double a = 0.0, b = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += UL_THREADS) { a += partial[2 * i]; b += partial[2 * i + 1]; }
  s0 = block_sum_f64(a, red);
  s1 = block_sum_f64(b, red);
}

__device__ __forceinline__ float gray255(float r, float g, float b) {
  return 255.0f * (0.2989f * r + 0.5870f * g + 0.1140f * b);
}

// Bilinear sampling with zero taps outside the frame (tfa.image.resampler, grid_sample(align_corners=True, 'zeros') in pixel
// units): the gray value at (sx, sy) and, when asked for, its derivative along x and y.
template <bool GRAD>
__device__ __forceinline__ float warp_gray(const float* __restrict__ img, int64_t cs, int64_t rs, int Hf, int Wf, float sx, float sy,
                                           float& gx, float& gy) {
  gx = 0.0f; gy = 0.0f;
  if (!(sx > -1.0f && sx < (float)Wf && sy > -1.0f && sy < (float)Hf)) return 0.0f;   // no tap inside (NaN included)
  const float x0 = floorf(sx), y0 = floorf(sy);
  const float ox = sx - x0, oy = sy - y0;
  const int ix = (int)x0, iy = (int)y0;                                               // [-1, Wf - 1], [-1, Hf - 1]
  const bool l = ix >= 0, r = ix + 1 < Wf, t = iy >= 0, b = iy + 1 < Hf;
  const float w00 = (1.0f - ox) * (1.0f - oy), w10 = ox * (1.0f - oy), w01 = (1.0f - ox) * oy, w11 = ox * oy;
  const float cw[3] = {0.2989f, 0.5870f, 0.1140f};
  float v = 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* p = img + c * cs + (int64_t)iy * rs + ix;
    const float v00 = (l && t) ? p[0] : 0.0f, v10 = (r && t) ? p[1] : 0.0f;
    const float v01 = (l && b) ? p[rs] : 0.0f, v11 = (r && b) ? p[rs + 1] : 0.0f;
    v += cw[c] * (((w00 * v00 + w10 * v10) + w01 * v01) + w11 * v11);
    if (GRAD) {
      gx += cw[c] * ((1.0f - oy) * (v10 - v00) + oy * (v11 - v01));
      gy += cw[c] * ((1.0f - ox) * (v01 - v00) + ox * (v11 - v10));
    }
  }
  if (GRAD) { gx *= 255.0f; gy *= 255.0f; }
  return 255.0f * v;
}

// ---------------------------------------------------------------------------------------------------------------- range map
__global__ __launch_bounds__(UL_THREADS) void range_map_scatter_kernel(View flow, int H, int W, unsigned long long* __restrict__ acc) {
  const int b = blockIdx.y, HW = H * W;
  const float* f = flow.p + b * flow.bs;
  unsigned long long* a = acc + (int64_t)b * HW;
  for (int64_t e = (int64_t)blockIdx.x * UL_THREADS + threadIdx.x; e < HW; e += (int64_t)gridDim.x * UL_THREADS) {
    const int y = (int)e / W, x = (int)e - y * W;
    const float cx = (float)x + f[y * flow.rs + x], cy = (float)y + f[flow.cs + y * flow.rs + x];
    if (!(cx > -1.0f && cx < (float)W && cy > -1.0f && cy < (float)H)) continue;      // no tap inside (NaN included)
    const float x0 = floorf(cx), y0 = floorf(cy);
    const float ox = cx - x0, oy = cy - y0;
    const int ix = (int)x0, iy = (int)y0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int xx = ix + (k & 1), yy = iy + (k >> 1);
      const float w = ((k & 1) ? ox : 1.0f - ox) * ((k >> 1) ? oy : 1.0f - oy);
      if (xx < 0 || xx >= W || yy < 0 || yy >= H || !(w > 0.0f)) continue;
      atomicAdd(a + (int64_t)yy * W + xx, __float2ull_rn(w * 4294967296.0f));
    }
  }
}

// (a kernel, not hipMemsetAsync: a memset node on the captured stream has been seen to drop out of a graph's replays)
__global__ __launch_bounds__(UL_THREADS) void range_map_zero_kernel(unsigned long long* __restrict__ acc, int64_t n) {
  for (int64_t e = (int64_t)blockIdx.x * UL_THREADS + threadIdx.x; e < n; e += (int64_t)gridDim.x * UL_THREADS) acc[e] = 0ull;
}

__global__ __launch_bounds__(UL_THREADS) void range_map_convert_kernel(const unsigned long long* __restrict__ acc, int64_t n, int clip,
                                                                      float* __restrict__ out) {
  for (int64_t e = (int64_t)blockIdx.x * UL_THREADS + threadIdx.x; e < n; e += (int64_t)gridDim.x * UL_THREADS) {
    float v = (float)((double)acc[e] * (1.0 / 4294967296.0));
    if (clip) v = fminf(v, 1.0f);
    out[e] = v;
  }
}

// ------------------------------------------------------------------------------------------------------------------- census
__device__ __forceinline__ float psi(float d) { return d / sqrtf(0.81f + d * d); }

// Stages gA (gray of image i) and, when `gBsrc` is null, the gray of the warped image j over the tile and its halo; with
// `gBsrc` the saved plane is read instead.  Positions outside the image hold zero.
__device__ __forceinline__ void stage_tile(const float* __restrict__ i1, View img1, int c1y, int c1x, const float* __restrict__ i2, View img2, int Hf, int Wf,
                                           int cy, int cx, const float* __restrict__ f, View flow, const float* __restrict__ gBsrc,
                                           const float* __restrict__ hsrc, int H, int W, int tx0, int ty0, float* gA, float* gB, float* hh) {
  for (int i = threadIdx.x; i < CT_N; i += UL_THREADS) {
    const int ly = i / CT_LW, lx = i - ly * CT_LW;
    const int y = ty0 + ly - CT_R, x = tx0 + lx - CT_R;
    float a = 0.0f, bb = 0.0f, h = 0.0f;
    if (x >= 0 && x < W && y >= 0 && y < H) {
      const float* p = i1 + (int64_t)(c1y + y) * img1.rs + (c1x + x);
      a = gray255(p[0], p[img1.cs], p[2 * img1.cs]);
      if (gBsrc) {
        bb = gBsrc[(int64_t)y * W + x];
        h = hsrc[(int64_t)y * W + x];
      } else {
        float gx, gy;
        const float sx = (float)(x + cx) + f[y * flow.rs + x], sy = (float)(y + cy) + f[flow.cs + y * flow.rs + x];
        bb = warp_gray<false>(i2, img2.cs, img2.rs, Hf, Wf, sx, sy, gx, gy);
      }
    }
    gA[i] = a;
    gB[i] = bb;
    if (hh) hh[i] = h;
  }
}

__global__ __launch_bounds__(UL_THREADS) void census_fwd_kernel(View img1, int img1_frame, View img2, int Hf, int Wf, Crops crops, int b0, View flow,
                                                                const float* __restrict__ mask, int64_t mask_bs, int64_t mask_rs, int H, int W,
                                                                float* __restrict__ grayB, float* __restrict__ hplane,
                                                                double* __restrict__ partial) {
  __shared__ float gA[CT_N], gB[CT_N];
  __shared__ double red[UL_THREADS / 64];
  const int bl = blockIdx.z, b = b0 + bl;
  const int cy = crops.y[bl], cx = crops.x[bl];
  const int tx0 = blockIdx.x * CT_W, ty0 = blockIdx.y * CT_H;
  const float* i1 = img1.p + b * img1.bs;
  const float* i2 = img2.p + b * img2.bs;
  const float* f = flow.p + b * flow.bs;
  stage_tile(i1, img1, img1_frame ? cy : 0, img1_frame ? cx : 0, i2, img2, Hf, Wf, cy, cx, f, flow, nullptr, nullptr, H, W, tx0, ty0, gA, gB, nullptr);
  __syncthreads();
  const int tx = threadIdx.x & (CT_W - 1), ty = threadIdx.x / CT_W;
  double sl = 0.0, sm = 0.0;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int ly = ty + r * (CT_H / 2), x = tx0 + tx, y = ty0 + ly;
    if (x >= W || y >= H) continue;
    const int c = (ly + CT_R) * CT_LW + tx + CT_R;
    float M = 0.0f;
    if (x >= CT_R && x < W - CT_R && y >= CT_R && y < H - CT_R) {
      const float sx = (float)(x + cx) + f[y * flow.rs + x], sy = (float)(y + cy) + f[flow.cs + y * flow.rs + x];
      const bool valid = sx >= 0.0f && sx <= (float)(Wf - 1) && sy >= 0.0f && sy <= (float)(Hf - 1);
      M = valid ? (mask ? mask[b * mask_bs + y * mask_rs + x] : 1.0f) : 0.0f;
    }
    float h = 0.0f;
    if (M != 0.0f) {
      const float a0 = gA[c], b0v = gB[c];
      float ham = 0.0f;
      for (int dy = -CT_R; dy <= CT_R; ++dy) {
#pragma unroll
        for (int dx = -CT_R; dx <= CT_R; ++dx) {
          const int n = c + dy * CT_LW + dx;
          const float u = psi(gA[n] - a0) - psi(gB[n] - b0v);
          const float u2 = u * u;
          ham += u2 / (0.1f + u2);
        }
      }
      const float l = powf(ham + 0.01f, 0.4f);
      h = M * (0.4f * (l / (ham + 0.01f)));
      sl += (double)(l * M);
      sm += (double)M;
    }
    grayB[((int64_t)b * H + y) * W + x] = gB[c];
    hplane[((int64_t)b * H + y) * W + x] = h;
  }
  const int64_t blk = ((int64_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  const double tl = block_sum_f64(sl, red), tm = block_sum_f64(sm, red);
  if (threadIdx.x == 0) { partial[2 * blk] = tl; partial[2 * blk + 1] = tm; }
}

// out[0] = sum l * M / (sum M + 1e-6 * B * H * W), out[1] = that denominator.
__global__ __launch_bounds__(UL_THREADS) void census_finalise_kernel(const double* __restrict__ partial, int64_t n, double npix,
                                                                    double* __restrict__ out) {
  __shared__ double red[UL_THREADS / 64];
  double s0, s1;
  sum_pairs(partial, n, red, s0, s1);
  if (threadIdx.x == 0) {
    const double den = s1 + 1e-6 * npix;
    out[0] = s0 / den;
    out[1] = den;
  }
}

__global__ __launch_bounds__(UL_THREADS) void census_bwd_kernel(View img1, int img1_frame, View img2, int Hf, int Wf, Crops crops, int b0, View flow,
                                                                const float* __restrict__ grayB, const float* __restrict__ hplane,
                                                                const float* __restrict__ up, const double* __restrict__ den, int H, int W,
                                                                float* __restrict__ dflow) {
  __shared__ float gA[CT_N], gB[CT_N], hh[CT_N];
  const int bl = blockIdx.z, b = b0 + bl;
  const int cy = crops.y[bl], cx = crops.x[bl];
  const int tx0 = blockIdx.x * CT_W, ty0 = blockIdx.y * CT_H;
  const float* i1 = img1.p + b * img1.bs;
  const float* i2 = img2.p + b * img2.bs;
  const float* f = flow.p + b * flow.bs;
  const int64_t plane = (int64_t)b * H * W;
  stage_tile(i1, img1, img1_frame ? cy : 0, img1_frame ? cx : 0, i2, img2, Hf, Wf, cy, cx, f, flow, grayB + plane, hplane + plane, H, W, tx0, ty0, gA, gB, hh);
  __syncthreads();
  const float scale = (float)((double)up[0] / den[0]);
  const int tx = threadIdx.x & (CT_W - 1), ty = threadIdx.x / CT_W;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int ly = ty + r * (CT_H / 2), x = tx0 + tx, y = ty0 + ly;
    if (x >= W || y >= H) continue;
    const int c = (ly + CT_R) * CT_LW + tx + CT_R;
    const float a0 = gA[c], b0v = gB[c], hq = hh[c];
    float G = 0.0f;
    for (int dy = -CT_R; dy <= CT_R; ++dy) {
#pragma unroll
      for (int dx = -CT_R; dx <= CT_R; ++dx) {
        const int n = c + dy * CT_LW + dx;
        const float hs = hq + hh[n];
        if (hs == 0.0f) continue;
        const float dB = gB[n] - b0v;
        const float rB = 1.0f / sqrtf(0.81f + dB * dB);
        const float u = psi(gA[n] - a0) - dB * rB;
        const float q = 0.1f + u * u;
        G += hs * ((0.2f * u) / (q * q)) * (0.81f * (rB * rB * rB));
      }
    }
    float dfx = 0.0f, dfy = 0.0f;
    if (G != 0.0f) {                  // (an untouched pixel gets +0.0, not the -0.0 of 0 * a negative slope)
      float gx, gy;
      const float sx = (float)(x + cx) + f[y * flow.rs + x], sy = (float)(y + cy) + f[flow.cs + y * flow.rs + x];
      warp_gray<true>(i2, img2.cs, img2.rs, Hf, Wf, sx, sy, gx, gy);
      dfx = gx == 0.0f ? 0.0f : scale * G * gx;
      dfy = gy == 0.0f ? 0.0f : scale * G * gy;
    }
    dflow[((int64_t)b * 2 * H + y) * W + x] = dfx;
    dflow[((int64_t)(b * 2 + 1) * H + y) * W + x] = dfy;
  }
}

// --------------------------------------------------------------------------------------------------------------- smoothness
// exp(-mean_c |k * dI|) ('exponential') or exp(-mean_c (k * dI)^2) ('gaussian') between two pixels of one sample.
__device__ __forceinline__ float edge_weight(const float* __restrict__ img, int64_t cs, int64_t o0, int64_t o1, float k, int gaussian) {
  float s = 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float d = k * (img[c * cs + o1] - img[c * cs + o0]);
    s += gaussian ? d * d : fabsf(d);
  }
  return expf(-(s / 3.0f));
}

// One direction (step `st` elements in the image, `fst` in the flow) at position `pos` of `len` along it: adds this pixel's own
// terms to `sum` and its share of the neighbouring terms' derivatives to g[0..1].
__device__ __forceinline__ void smooth_dir(const float* __restrict__ img, int64_t ics, int64_t ioff, int64_t ist,
                                           const float* __restrict__ f, int64_t fcs, int64_t foff, int64_t fst, int pos, int len, int order,
                                           float k, int gaussian, double& sum, float* g) {
  const int n = len - order;                      // terms along this direction
  for (int j = 0; j <= order; ++j) {
    const int q = pos - j;
    if (q < 0 || q >= n) continue;
    const float w = edge_weight(img, ics, ioff - j * ist, ioff + (order - j) * ist, k, gaussian);
    const float coef = order == 1 ? (j == 0 ? -1.0f : 1.0f) : (j == 1 ? -2.0f : 1.0f);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const float* p = f + c * fcs + foff - j * fst;
      const float d = order == 1 ? p[fst] - p[0] : (p[2 * fst] - p[fst]) - (p[fst] - p[0]);
      const float r = sqrtf(d * d + 1e-6f);
      if (j == 0) sum += (double)(w * r);
      g[c] += coef * (w * (d / r));
    }
  }
}

__global__ __launch_bounds__(UL_THREADS) void smoothness_kernel(View img, Crops crops, int b0, View flow, int H, int W, int order, float k,
                                                                int gaussian, float scale_x, float scale_y, float* __restrict__ dflow,
                                                                double* __restrict__ partial) {
  __shared__ double red[UL_THREADS / 64];
  const int bl = blockIdx.y, b = b0 + bl, HW = H * W;
  const float* im = img.p + b * img.bs + (int64_t)crops.y[bl] * img.rs + crops.x[bl];
  const float* f = flow.p + b * flow.bs;
  double sx = 0.0, sy = 0.0;
  for (int64_t e = (int64_t)blockIdx.x * UL_THREADS + threadIdx.x; e < HW; e += (int64_t)gridDim.x * UL_THREADS) {
    const int y = (int)e / W, x = (int)e - y * W;
    float gx[2] = {0.0f, 0.0f}, gy[2] = {0.0f, 0.0f};
    smooth_dir(im, img.cs, y * img.rs + x, 1, f, flow.cs, y * flow.rs + x, 1, x, W, order, k, gaussian, sx, gx);
    smooth_dir(im, img.cs, y * img.rs + x, img.rs, f, flow.cs, y * flow.rs + x, flow.rs, y, H, order, k, gaussian, sy, gy);
    dflow[((int64_t)b * 2 * H + y) * W + x] = scale_x * gx[0] + scale_y * gy[0];
    dflow[((int64_t)(b * 2 + 1) * H + y) * W + x] = scale_x * gx[1] + scale_y * gy[1];
  }
  const int64_t blk = (int64_t)b * gridDim.x + blockIdx.x;
  const double tx = block_sum_f64(sx, red), ty = block_sum_f64(sy, red);
  if (threadIdx.x == 0) { partial[2 * blk] = tx; partial[2 * blk + 1] = ty; }
}

__global__ __launch_bounds__(UL_THREADS) void smoothness_finalise_kernel(const double* __restrict__ partial, int64_t n, double nx, double ny,
                                                                        double* __restrict__ out) {
  __shared__ double red[UL_THREADS / 64];
  double s0, s1;
  sum_pairs(partial, n, red, s0, s1);
  if (threadIdx.x == 0) out[0] = (s0 / nx + s1 / ny) / 2.0;
}

static inline int sm_blocks(int64_t hw) {
  const int64_t n = (hw + UL_THREADS - 1) / UL_THREADS;
  return (int)(n < UL_MAX_BLOCKS ? n : UL_MAX_BLOCKS);
}

static inline bool aligned8(const void* p) { return (uintptr_t)p % 8 == 0; }

// The window of every sample inside the frame (crop_yx NULL: offsets 0, so the window is the frame's top-left H x W).
static bool crops_ok(const int* crop_yx, int B, int H, int W, int Hf, int Wf) {
  if (Hf < H || Wf < W || (int64_t)Hf * Wf > INT32_MAX) return false;
  for (int b = 0; crop_yx && b < B; ++b) {
    const int cy = crop_yx[2 * b], cx = crop_yx[2 * b + 1];
    if (cy < 0 || cx < 0 || cy > Hf - H || cx > Wf - W) return false;
  }
  return true;
}

static Crops crops_of(const int* crop_yx, int b0, int nb) {
  Crops c;
  for (int i = 0; i < UL_CHUNK; ++i) {
    c.y[i] = crop_yx && i < nb ? crop_yx[2 * (b0 + i)] : 0;
    c.x[i] = crop_yx && i < nb ? crop_yx[2 * (b0 + i) + 1] : 0;
  }
  return c;
}

static inline bool sizes_ok(int B, int H, int W, int minhw) {
  return B >= 1 && H >= minhw && W >= minhw && (int64_t)H * W <= INT32_MAX;
}

static inline int64_t census_blocks(int B, int H, int W) {
  return (int64_t)B * ceil_div(H, CT_H) * ceil_div(W, CT_W);
}

}  // namespace

extern "C" int fsraft_range_map_scratch_bytes(int B, int H, int W) {
  if (!sizes_ok(B, H, W, 1)) return FS_ERR_ARG;
  const int64_t bytes = (int64_t)B * H * W * 8;
  return bytes > INT32_MAX ? FS_ERR_ARG : (int)bytes;
}

extern "C" int fsraft_range_map(const float* flow, int64_t flow_bs, int64_t flow_cs, int64_t flow_rs, int B, int H, int W, int clip,
                                float* out, void* scratch, int64_t scratch_bytes, hipStream_t s) {
  if (!flow || !out || !scratch || !aligned8(scratch)) return FS_ERR_ARG;
  const int need = fsraft_range_map_scratch_bytes(B, H, W);
  if (need == FS_ERR_ARG || scratch_bytes < need || B > 65535) return FS_ERR_ARG;
  const View f{flow, flow_bs, flow_cs, flow_rs};
  const int64_t n = (int64_t)B * H * W;
  const int64_t nb = (n + UL_THREADS - 1) / UL_THREADS;
  const dim3 flat((unsigned)(nb < 4096 ? nb : 4096));
  hipLaunchKernelGGL(range_map_zero_kernel, flat, dim3(UL_THREADS), 0, s, (unsigned long long*)scratch, n);
  if (fs_launch_status() != FS_OK) return FS_ERR_LAUNCH;
  hipLaunchKernelGGL(range_map_scatter_kernel, dim3(sm_blocks((int64_t)H * W), B), dim3(UL_THREADS), 0, s, f, H, W,
                     (unsigned long long*)scratch);
  if (fs_launch_status() != FS_OK) return FS_ERR_LAUNCH;
  hipLaunchKernelGGL(range_map_convert_kernel, flat, dim3(UL_THREADS), 0, s,
                     (const unsigned long long*)scratch, n, clip, out);
  return fs_launch_status();
}

extern "C" int fsraft_census_scratch_bytes(int B, int H, int W) {
  if (!sizes_ok(B, H, W, 2 * CT_R + 1)) return FS_ERR_ARG;
  const int64_t bytes = (census_blocks(B, H, W) * 16 + 63) / 64 * 64;
  return bytes > INT32_MAX ? FS_ERR_ARG : (int)bytes;
}

extern "C" int fsraft_census_fwd(const float* img1, int64_t img1_bs, int64_t img1_cs, int64_t img1_rs, int img1_frame,
                                 const float* img2, int64_t img2_bs, int64_t img2_cs, int64_t img2_rs, int Hf, int Wf,
                                 const int* crop_yx, const float* flow, int64_t flow_bs, int64_t flow_cs, int64_t flow_rs,
                                 const float* mask, int64_t mask_bs, int64_t mask_rs, int B, int H, int W,
                                 float* grayB, float* hplane, double* out, void* scratch, int64_t scratch_bytes, hipStream_t s) {
  if (!img1 || !img2 || !flow || !grayB || !hplane || !out || !scratch || !aligned8(out) || !aligned8(scratch)) return FS_ERR_ARG;
  const int need = fsraft_census_scratch_bytes(B, H, W);
  if (need == FS_ERR_ARG || scratch_bytes < need || !crops_ok(crop_yx, B, H, W, Hf, Wf)) return FS_ERR_ARG;
  const View i1{img1, img1_bs, img1_cs, img1_rs}, i2{img2, img2_bs, img2_cs, img2_rs}, f{flow, flow_bs, flow_cs, flow_rs};
  for (int b0 = 0; b0 < B; b0 += UL_CHUNK) {
    const int nb = B - b0 < UL_CHUNK ? B - b0 : UL_CHUNK;
    hipLaunchKernelGGL(census_fwd_kernel, dim3(ceil_div(W, CT_W), ceil_div(H, CT_H), nb), dim3(UL_THREADS), 0, s, i1, img1_frame, i2, Hf, Wf,
                       crops_of(crop_yx, b0, nb), b0, f, mask, mask_bs, mask_rs, H, W, grayB, hplane, (double*)scratch);
    if (fs_launch_status() != FS_OK) return FS_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(census_finalise_kernel, dim3(1), dim3(UL_THREADS), 0, s, (const double*)scratch, census_blocks(B, H, W),
                     (double)B * H * W, out);
  return fs_launch_status();
}

extern "C" int fsraft_census_bwd(const float* img1, int64_t img1_bs, int64_t img1_cs, int64_t img1_rs, int img1_frame,
                                 const float* img2, int64_t img2_bs, int64_t img2_cs, int64_t img2_rs, int Hf, int Wf,
                                 const int* crop_yx, const float* flow, int64_t flow_bs, int64_t flow_cs, int64_t flow_rs,
                                 const float* grayB, const float* hplane, const float* up, const double* den, int B, int H, int W,
                                 float* dflow, hipStream_t s) {
  if (!img1 || !img2 || !flow || !grayB || !hplane || !up || !den || !dflow || !aligned8(den)) return FS_ERR_ARG;
  if (!sizes_ok(B, H, W, 2 * CT_R + 1) || !crops_ok(crop_yx, B, H, W, Hf, Wf)) return FS_ERR_ARG;
  const View i1{img1, img1_bs, img1_cs, img1_rs}, i2{img2, img2_bs, img2_cs, img2_rs}, f{flow, flow_bs, flow_cs, flow_rs};
  for (int b0 = 0; b0 < B; b0 += UL_CHUNK) {
    const int nb = B - b0 < UL_CHUNK ? B - b0 : UL_CHUNK;
    hipLaunchKernelGGL(census_bwd_kernel, dim3(ceil_div(W, CT_W), ceil_div(H, CT_H), nb), dim3(UL_THREADS), 0, s, i1, img1_frame, i2, Hf, Wf,
                       crops_of(crop_yx, b0, nb), b0, f, grayB, hplane, up, den, H, W, dflow);
    if (fs_launch_status() != FS_OK) return FS_ERR_LAUNCH;
  }
  return FS_OK;
}

extern "C" int fsraft_smoothness_scratch_bytes(int B, int H, int W) {
  if (!sizes_ok(B, H, W, 1)) return FS_ERR_ARG;
  const int64_t bytes = ((int64_t)B * sm_blocks((int64_t)H * W) * 16 + 63) / 64 * 64;
  return bytes > INT32_MAX ? FS_ERR_ARG : (int)bytes;
}

extern "C" int fsraft_smoothness(const float* img, int64_t img_bs, int64_t img_cs, int64_t img_rs, int Hf, int Wf, const int* crop_yx,
                                 const float* flow, int64_t flow_bs, int64_t flow_cs, int64_t flow_rs, int B, int H, int W, int order,
                                 float edge_constant, int gaussian, float* dflow, double* out, void* scratch, int64_t scratch_bytes,
                                 hipStream_t s) {
  if (!img || !flow || !dflow || !out || !scratch || !aligned8(out) || !aligned8(scratch)) return FS_ERR_ARG;
  if ((order != 1 && order != 2) || (gaussian != 0 && gaussian != 1)) return FS_ERR_ARG;
  const int need = fsraft_smoothness_scratch_bytes(B, H, W);
  if (need == FS_ERR_ARG || scratch_bytes < need || H <= order || W <= order || !crops_ok(crop_yx, B, H, W, Hf, Wf)) return FS_ERR_ARG;
  const View im{img, img_bs, img_cs, img_rs}, f{flow, flow_bs, flow_cs, flow_rs};
  const int nblk = sm_blocks((int64_t)H * W);
  const double nx = 2.0 * B * H * (W - order), ny = 2.0 * B * (H - order) * W;     // elements of the two means
  for (int b0 = 0; b0 < B; b0 += UL_CHUNK) {
    const int nb = B - b0 < UL_CHUNK ? B - b0 : UL_CHUNK;
    hipLaunchKernelGGL(smoothness_kernel, dim3(nblk, nb), dim3(UL_THREADS), 0, s, im, crops_of(crop_yx, b0, nb), b0, f, H, W, order,
                       edge_constant, gaussian, (float)(0.5 / nx), (float)(0.5 / ny), dflow, (double*)scratch);
    if (fs_launch_status() != FS_OK) return FS_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(smoothness_finalise_kernel, dim3(1), dim3(UL_THREADS), 0, s, (const double*)scratch, (int64_t)B * nblk, nx, ny, out);
  return fs_launch_status();
}
