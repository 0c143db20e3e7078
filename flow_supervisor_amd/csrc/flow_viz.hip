// Flow visualisation and submission encoding on the device: the Middlebury colour wheel of pytorch/core/utils/flow_viz.py,
// the HSV coding of util/visualize.py and the 16-bit KITTI encoding of pytorch/raft_utils/frame_utils.py:121-125.  The
// reference copies every full-resolution prediction to the host (8 bytes a pixel) and colours it in NumPy / TensorFlow; here
// the un-padded view of the padded prediction is read in place and 3 (picture) or 6 (KITTI) bytes a pixel go back.
//
// Formulas: include/fsraft.h.  Everything is fp32 with every operation rounded on its own (the floor(255 * col) decisions sit
// on the rounding, so contraction is off for the whole file, as in flow_metrics.hip); division and square root are the
// correctly rounded expansions the compiler emits by default.
//
// The maximum is an atomicMax on the bit pattern of a non-negative float (the order of unsigned integers is the order of
// non-negative floats): a maximum does not depend on the order of its operands, so the result is the same bits from run to run
// and for a sample alone or in a batch.  The result is zeroed by the call itself, on the caller's stream.
#include "common.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int FV_THREADS = 256;
constexpr int FV_MAX_BLOCKS = 256;      // per sample, for the maximum: larger frames take more trips of the grid-stride loop
constexpr int FV_GROUP = 4;             // pixels per thread of the uint8 kernels: 12 bytes, three dwords

struct Plane2 {                          // a [B,2,H,W] view with unit x stride (strides in elements)
  const float* p;
  int64_t bs, cs, rs;
};

// RY 15, YG 6, GC 4, CB 11, BM 13, MR 6 (flow_viz.py:33-67): floor(255 * i / n) along each ramp
__constant__ unsigned char WHEEL[55][3] = {
    {255, 0, 0},   {255, 17, 0},  {255, 34, 0},  {255, 51, 0},  {255, 68, 0},  {255, 85, 0},  {255, 102, 0}, {255, 119, 0},
    {255, 136, 0}, {255, 153, 0}, {255, 170, 0}, {255, 187, 0}, {255, 204, 0}, {255, 221, 0}, {255, 238, 0},
    {255, 255, 0}, {213, 255, 0}, {170, 255, 0}, {128, 255, 0}, {85, 255, 0},  {43, 255, 0},
    {0, 255, 0},   {0, 255, 63},  {0, 255, 127}, {0, 255, 191},
    {0, 255, 255}, {0, 232, 255}, {0, 209, 255}, {0, 186, 255}, {0, 163, 255}, {0, 140, 255}, {0, 116, 255}, {0, 93, 255},
    {0, 70, 255},  {0, 47, 255},  {0, 24, 255},
    {0, 0, 255},   {19, 0, 255},  {39, 0, 255},  {58, 0, 255},  {78, 0, 255},  {98, 0, 255},  {117, 0, 255}, {137, 0, 255},
    {156, 0, 255}, {176, 0, 255}, {196, 0, 255}, {215, 0, 255}, {235, 0, 255},
    {255, 0, 255}, {255, 0, 213}, {255, 0, 170}, {255, 0, 128}, {255, 0, 85},  {255, 0, 43}};

constexpr float FV_PI = 3.14159265358979323846f;
constexpr float FV_2PI = 6.28318530717958647692f;

__device__ __forceinline__ bool finite2(float u, float v) { return isfinite(u) && isfinite(v); }

// np.clip(flow_uv, 0, clip_flow) (flow_viz.py:123-124): the lower bound is 0, not -clip -- the reference's quirk, kept.  As
// np.clip does, by comparison: -0.0 is not below 0 and stays -0.0 (fmaxf would make it +0.0, and the sign of a zero v decides
// between the two ends of the wheel, atan2f(+-0, -u) = +-pi).
__device__ __forceinline__ float clip0(float x, float clip) {
  return clip > 0.0f ? (x < 0.0f ? 0.0f : (x > clip ? clip : x)) : x;
}

__device__ __forceinline__ void load_uv(const Plane2& f, int b, int e, int W, float& u, float& v) {
  const int y = e / W, x = e - y * W;
  const float* p = f.p + b * f.bs + y * f.rs + x;
  u = p[0];
  v = p[f.cs];
}

__global__ __launch_bounds__(FV_THREADS) void flow_rad_max_kernel(Plane2 flow, int HW, int W, float clip,
                                                                 unsigned* __restrict__ rad_max_bits) {
  __shared__ float red[FV_THREADS / 64];
  const int b = blockIdx.y;
  float m = 0.0f;
  for (int64_t e = (int64_t)blockIdx.x * FV_THREADS + threadIdx.x; e < HW; e += (int64_t)gridDim.x * FV_THREADS) {
    float u, v;
    load_uv(flow, b, (int)e, W, u, v);
    if (!finite2(u, v)) continue;
    u = clip0(u, clip);
    v = clip0(v, clip);
    m = fmaxf(m, sqrtf(u * u + v * v));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    if (m > 0.0f) atomicMax(rad_max_bits + b, __float_as_uint(m));      // m >= 0 and never NaN: fmaxf drops a NaN operand
  }
}

struct Rgb { unsigned char c[3]; };

__device__ __forceinline__ unsigned char level(float col) {             // floor(255 * col) as uint8
  const float t = floorf(255.0f * col);
  return (unsigned char)(t >= 255.0f ? 255 : (t > 0.0f ? (int)t : 0));
}

__device__ __forceinline__ Rgb wheel_pixel(float u, float v, float clip, float den, int bgr) {
  Rgb o = {{0, 0, 0}};
  if (!finite2(u, v)) return o;
  u = clip0(u, clip) / den;
  v = clip0(v, clip) / den;
  const float rad = sqrtf(u * u + v * v);
  const float a = atan2f(-v, -u) / FV_PI;
  const float fk = (a + 1.0f) / 2.0f * 54.0f;
  const float k0f = floorf(fk);
  const float f = fk - k0f;
  int k0 = (int)k0f;
  k0 = k0 < 0 ? 0 : (k0 > 54 ? 54 : k0);      // an atan2f one ulp above pi must give a colour, not a read outside the table
  const int k1 = k0 == 54 ? 0 : k0 + 1;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    float col = (1.0f - f) * ((float)WHEEL[k0][i] / 255.0f) + f * ((float)WHEEL[k1][i] / 255.0f);
    if (rad <= 1.0f) col = 1.0f - rad * (1.0f - col);
    else col = col * 0.75f;                   // out of range
    o.c[bgr ? 2 - i : i] = level(col);
  }
  return o;
}

__device__ __forceinline__ void hsv_pixel(float x, float y, float max_mag, float mx, float c[3]) {
  const float rho = sqrtf(x * x + y * y);
  float phi = atan2f(y, x);
  if (phi < 0.0f) phi = phi + FV_2PI;
  const float s = max_mag > 0.0f ? fminf(fmaxf(rho / max_mag, 0.0f), 1.0f) : rho / mx;
  const float h6 = phi / FV_2PI * 6.0f;
  const float d[3] = {fminf(fmaxf(fabsf(h6 - 3.0f) - 1.0f, 0.0f), 1.0f), fminf(fmaxf(2.0f - fabsf(h6 - 2.0f), 0.0f), 1.0f),
                      fminf(fmaxf(2.0f - fabsf(h6 - 4.0f), 0.0f), 1.0f)};
#pragma unroll
  for (int i = 0; i < 3; ++i) c[i] = ((d[i] - 1.0f) * s + 1.0f) * 1.0f;
}

enum { MODE_WHEEL = 0, MODE_HSV = 1 };

// uint8 [B][H][W][3], taken as one flat run of B * H * W pixels: thread t colours pixels 4t .. 4t+3, which are bytes
// 12t .. 12t+11 -- three whole dwords when the output base is dword-aligned, wherever rows and samples begin.  The last,
// partial group and a base that is not dword-aligned take byte stores.
template <int MODE>
__global__ __launch_bounds__(FV_THREADS) void flow_colour_u8_kernel(Plane2 flow, int B, int HW, int W, float clip,
                                                                   const float* __restrict__ rad_max, float scale, int bgr,
                                                                   unsigned char* __restrict__ out, int out_aligned) {
  const int64_t total = (int64_t)B * HW;
  const int64_t p0 = ((int64_t)blockIdx.x * FV_THREADS + threadIdx.x) * FV_GROUP;
  if (p0 >= total) return;
  unsigned char bytes[3 * FV_GROUP] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const int n = total - p0 < FV_GROUP ? (int)(total - p0) : FV_GROUP;
#pragma unroll
  for (int j = 0; j < FV_GROUP; ++j) {
    if (j >= n) break;
    const int64_t p = p0 + j;
    const int b = (int)(p / HW), e = (int)(p - (int64_t)b * HW);
    float u, v;
    load_uv(flow, b, e, W, u, v);
    if (MODE == MODE_WHEEL) {
      const float den = rad_max ? rad_max[b] + 1e-5f : scale;
      const Rgb o = wheel_pixel(u, v, clip, den, bgr);
      bytes[3 * j] = o.c[0]; bytes[3 * j + 1] = o.c[1]; bytes[3 * j + 2] = o.c[2];
    } else {
      float c[3] = {0.0f, 0.0f, 0.0f};
      if (finite2(u, v)) {
        float mx = rad_max ? rad_max[b] : 1.0f;
        if (mx == 0.0f) mx = 1.0f;
        hsv_pixel(u, v, scale, mx, c);
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) {                // np.uint8(vis * 255): truncation; c is in [0, 1]
        const float t = 255.0f * c[i];
        bytes[3 * j + i] = (unsigned char)(t >= 255.0f ? 255 : (t > 0.0f ? (int)t : 0));
      }
    }
  }
  unsigned char* dst = out + 3 * p0;
  if (n == FV_GROUP && out_aligned) {
    unsigned* d32 = (unsigned*)dst;
#pragma unroll
    for (int k = 0; k < 3; ++k)
      d32[k] = (unsigned)bytes[4 * k] | (unsigned)bytes[4 * k + 1] << 8 | (unsigned)bytes[4 * k + 2] << 16 | (unsigned)bytes[4 * k + 3] << 24;
  } else {
#pragma unroll
    for (int k = 0; k < 3 * FV_GROUP; ++k)
      if (k < 3 * n) dst[k] = bytes[k];
  }
}

__global__ __launch_bounds__(FV_THREADS) void flow_hsv_f32_kernel(Plane2 flow, int B, int HW, int W, const float* __restrict__ rad_max,
                                                                 float max_mag, float* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * FV_THREADS + threadIdx.x;
  if (p >= (int64_t)B * HW) return;
  const int b = (int)(p / HW), e = (int)(p - (int64_t)b * HW);
  float u, v;
  load_uv(flow, b, e, W, u, v);
  float c[3] = {0.0f, 0.0f, 0.0f};
  if (finite2(u, v)) {
    float mx = rad_max ? rad_max[b] : 1.0f;
    if (mx == 0.0f) mx = 1.0f;
    hsv_pixel(u, v, max_mag, mx, c);
  }
  float* dst = out + 3 * p;
  dst[0] = c[0]; dst[1] = c[1]; dst[2] = c[2];
}

__device__ __forceinline__ unsigned short kitti_level(float x) {         // (uint16)(64 * x + 2^15), truncated, saturating
  const float t = 64.0f * x + 32768.0f;
  return (unsigned short)(t >= 65535.0f ? 65535 : (t > 0.0f ? (int)t : 0));      // NaN: 0
}

__global__ __launch_bounds__(FV_THREADS) void flow_kitti16_kernel(Plane2 flow, const float* __restrict__ valid, int64_t valid_bs,
                                                                 int64_t valid_rs, int B, int HW, int W,
                                                                 unsigned short* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * FV_THREADS + threadIdx.x;
  if (p >= (int64_t)B * HW) return;
  const int b = (int)(p / HW), e = (int)(p - (int64_t)b * HW);
  float u, v;
  load_uv(flow, b, e, W, u, v);
  const int y = e / W, x = e - y * W;
  unsigned short* dst = out + 3 * p;
  dst[0] = kitti_level(u);
  dst[1] = kitti_level(v);
  dst[2] = valid ? (valid[b * valid_bs + y * valid_rs + x] >= 0.5f ? 1 : 0) : 1;
}

static inline bool bad_view(const float* flow, int B, int H, int W) {
  return !flow || B < 1 || H < 1 || W < 1 || (int64_t)H * W > INT32_MAX || B > 65535;
}

static inline unsigned blocks_for(int64_t items) { return (unsigned)((items + FV_THREADS - 1) / FV_THREADS); }

// one block index per 256 items (1024 pixels of the uint8 kernels): the grid's x dimension holds 2^31 - 1 of them
static inline bool too_many(int64_t items) { return (items + FV_THREADS - 1) / FV_THREADS > INT32_MAX; }

}  // namespace

extern "C" int fsraft_flow_rad_max(const float* flow, int64_t flow_bs, int64_t flow_cs, int64_t flow_rs, int B, int H, int W,
                                   float clip, float* rad_max, hipStream_t s) {
  if (bad_view(flow, B, H, W) || !rad_max || (uintptr_t)rad_max % sizeof(float) || !(clip >= 0.0f) || !(clip < INFINITY))
    return FS_ERR_ARG;
  if (hipMemsetAsync(rad_max, 0, (size_t)B * sizeof(float), s) != hipSuccess) return FS_ERR_LAUNCH;
  const int64_t hw = (int64_t)H * W;
  const int64_t nb = (hw + FV_THREADS - 1) / FV_THREADS;
  const Plane2 f{flow, flow_bs, flow_cs, flow_rs};
  hipLaunchKernelGGL(flow_rad_max_kernel, dim3((unsigned)(nb < FV_MAX_BLOCKS ? nb : FV_MAX_BLOCKS), B), dim3(FV_THREADS), 0, s, f,
                     (int)hw, W, clip, (unsigned*)rad_max);
  return fs_launch_status();
}

extern "C" int fsraft_flow_wheel(const float* flow, int64_t flow_bs, int64_t flow_cs, int64_t flow_rs, int B, int H, int W,
                                 float clip, const float* rad_max, float scale, int bgr, uint8_t* out, hipStream_t s) {
  if (bad_view(flow, B, H, W) || !out || !(clip >= 0.0f) || !(clip < INFINITY) || (bgr != 0 && bgr != 1)) return FS_ERR_ARG;
  if (rad_max ? (uintptr_t)rad_max % sizeof(float) != 0 : !(scale > 0.0f && scale < INFINITY)) return FS_ERR_ARG;
  const int64_t groups = ((int64_t)B * H * W + FV_GROUP - 1) / FV_GROUP;
  if (too_many(groups)) return FS_ERR_ARG;
  const Plane2 f{flow, flow_bs, flow_cs, flow_rs};
  hipLaunchKernelGGL(flow_colour_u8_kernel<MODE_WHEEL>, dim3(blocks_for(groups)), dim3(FV_THREADS), 0, s, f, B, H * W, W, clip, rad_max,
                     scale, bgr, out, (int)((uintptr_t)out % 4 == 0));
  return fs_launch_status();
}

extern "C" int fsraft_flow_hsv(const float* flow, int64_t flow_bs, int64_t flow_cs, int64_t flow_rs, int B, int H, int W,
                               const float* rad_max, float max_mag, int out_u8, void* out, hipStream_t s) {
  if (bad_view(flow, B, H, W) || !out || (out_u8 != 0 && out_u8 != 1)) return FS_ERR_ARG;
  if (!(max_mag >= 0.0f) || !(max_mag < INFINITY) || (max_mag == 0.0f && !rad_max)) return FS_ERR_ARG;
  if ((uintptr_t)rad_max % sizeof(float) || (!out_u8 && (uintptr_t)out % sizeof(float))) return FS_ERR_ARG;
  const int64_t pixels = (int64_t)B * H * W;
  const Plane2 f{flow, flow_bs, flow_cs, flow_rs};
  if (out_u8) {
    const int64_t groups = (pixels + FV_GROUP - 1) / FV_GROUP;
    if (too_many(groups)) return FS_ERR_ARG;
    hipLaunchKernelGGL(flow_colour_u8_kernel<MODE_HSV>, dim3(blocks_for(groups)), dim3(FV_THREADS), 0, s, f, B, H * W, W, 0.0f, rad_max,
                       max_mag, 0, (unsigned char*)out, (int)((uintptr_t)out % 4 == 0));
  } else {
    if (too_many(pixels)) return FS_ERR_ARG;
    hipLaunchKernelGGL(flow_hsv_f32_kernel, dim3(blocks_for(pixels)), dim3(FV_THREADS), 0, s, f, B, H * W, W, rad_max, max_mag,
                       (float*)out);
  }
  return fs_launch_status();
}

extern "C" int fsraft_flow_kitti16(const float* flow, int64_t flow_bs, int64_t flow_cs, int64_t flow_rs,
                                   const float* valid, int64_t valid_bs, int64_t valid_rs, int B, int H, int W, uint16_t* out,
                                   hipStream_t s) {
  if (bad_view(flow, B, H, W) || !out || (uintptr_t)out % sizeof(uint16_t)) return FS_ERR_ARG;
  const int64_t pixels = (int64_t)B * H * W;
  if (too_many(pixels)) return FS_ERR_ARG;
  const Plane2 f{flow, flow_bs, flow_cs, flow_rs};
  hipLaunchKernelGGL(flow_kitti16_kernel, dim3(blocks_for(pixels)), dim3(FV_THREADS), 0, s, f, valid, valid_bs, valid_rs, B, H * W, W,
                     out);
  return fs_launch_status();
}
