// The forward-backward consistency masks and the self-supervision term of the SMURF loss (raft/smurf_models/smurf_utils.py
// compute_occlusions_brox :432-453 and self_supervision_loss :735-829, called from raft/unsup_loss.py with selfsup_mask
// 'gaussian' and a plain crop as the transform).  Conventions of unsup_loss.hip: flows [B,2,.,.] with channel 0 = x, every view
// read through element strides with a unit x stride, a frame argument of which sample b uses the window at (crop_y[b], crop_x[b]),
// offsets passed by value in chunks, fp64 partial sums in caller-provided scratch added in workgroup order by a finalising block.
// No allocation, no synchronisation, no host read and no float atomics, so every entry can be captured and a second launch
// gives the same bits.
//
// Forward-backward quantities of a pair (f, g) over an image of Hi x Wi, at pixel p: r = resample(g, p + f(p)) (bilinear, zero
// taps outside), sq = |f + r|^2, ss = |f|^2 + |r|^2, valid = p + f(p) inside [0, Wi-1] x [0, Hi-1].  The consistency c is
// exp(-sq / norm) ('gaussian'), [sq < 0.01 ss + 0.5] ('ddflow'); 'brox' is visible = 1 - [sq > 0.01 ss + 0.5], without valid.
//
// f + r is a difference of nearly equal numbers wherever the pair is consistent, so the order of the roundings shows in sq.
// The operations are kept one rounding each (no contraction into fused multiply-adds) in the order of the restatement in
// tests/_selfsupref.py; a call lasts under 20 us at the recipe size and the unfused multiplies are not what it waits for.
#include "common.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int SS_THREADS = 256;
// per sample (grid-stride beyond 262144 pixels).  A pixel is two dependent trips to memory (the flow, then the taps it points at)
// and little else, so the waves in flight hide them: at the recipe size (4 x 368 x 768) 256 workgroups a sample are 4 waves a SIMD
constexpr int SS_MAX_BLOCKS = 1024;
constexpr int SS_CHUNK = 32;             // samples per launch of a kernel that takes crop offsets by value

struct View {                             // [B,2,H,W] with unit x stride (strides in elements)
  const float* p;
  int64_t bs, cs, rs;
};
struct Crops { int y[SS_CHUNK], x[SS_CHUNK]; };

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

// Bilinear sampling of a two-channel field with zero taps outside the Hi x Wi image (tfa.image.resampler).
__device__ __forceinline__ void resample_flow(const float* __restrict__ g, int64_t cs, int64_t rs, int Hi, int Wi, float sx, float sy,
                                              float& rx, float& ry) {
  rx = 0.0f; ry = 0.0f;
  if (!(sx > -1.0f && sx < (float)Wi && sy > -1.0f && sy < (float)Hi)) return;        // no tap inside (NaN included)
  const float x0 = floorf(sx), y0 = floorf(sy);
  const float ox = sx - x0, oy = sy - y0;
  const int ix = (int)x0, iy = (int)y0;                                               // [-1, Wi - 1], [-1, Hi - 1]
  const bool l = ix >= 0, r = ix + 1 < Wi, t = iy >= 0, b = iy + 1 < Hi;
  const float w00 = (1.0f - ox) * (1.0f - oy), w10 = ox * (1.0f - oy), w01 = (1.0f - ox) * oy, w11 = ox * oy;
  float v[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const float* p = g + c * cs + (int64_t)iy * rs + ix;
    const float v00 = (l && t) ? p[0] : 0.0f, v10 = (r && t) ? p[1] : 0.0f;
    const float v01 = (l && b) ? p[rs] : 0.0f, v11 = (r && b) ? p[rs + 1] : 0.0f;
    v[c] = ((w00 * v00 + w10 * v10) + w01 * v01) + w11 * v11;
  }
  rx = v[0]; ry = v[1];
}

struct FB { float sq, ss; bool valid; };

// The pair (f, g) of one sample over its Hi x Wi image, at the pixel (px, py) of that image.
__device__ __forceinline__ FB fb_at(const float* __restrict__ f, int64_t fcs, int64_t frs, const float* __restrict__ g, int64_t gcs, int64_t grs,
                                    int Hi, int Wi, int px, int py) {
  const int64_t o = (int64_t)py * frs + px;
  const float fx = f[o], fy = f[fcs + o];
  const float sx = (float)px + fx, sy = (float)py + fy;
  float rx, ry;
  resample_flow(g, gcs, grs, Hi, Wi, sx, sy, rx, ry);
  const float ax = fx + rx, ay = fy + ry;
  FB q;
  q.sq = ax * ax + ay * ay;
  q.ss = (fx * fx + rx * rx) + (fy * fy + ry * ry);
  q.valid = sx >= 0.0f && sx <= (float)(Wi - 1) && sy >= 0.0f && sy <= (float)(Hi - 1);
  return q;
}

// c * valid of 'gaussian' or 'ddflow'.
__device__ __forceinline__ float consistency(const FB& q, int mode, float norm) {
  if (!q.valid) return 0.0f;
  if (mode == FSRAFT_FB_GAUSSIAN) return expf(-q.sq / norm);
  return q.sq < 0.01f * q.ss + 0.5f ? 1.0f : 0.0f;
}

// 1 - c * valid.  The gaussian's goes through expm1f: next to c = 1 (a consistent pair under a wide normaliser, the student's
// usual state) 1 - expf() keeps only the last bits of c, and the error of expf in those bits does not average out over an image.
__device__ __forceinline__ float inconsistency(const FB& q, int mode, float norm) {
  if (!q.valid) return 1.0f;
  if (mode == FSRAFT_FB_GAUSSIAN) return -expm1f(-q.sq / norm);
  return q.sq < 0.01f * q.ss + 0.5f ? 0.0f : 1.0f;
}

__global__ __launch_bounds__(SS_THREADS) void fb_mask_kernel(View flow, View back, int Hf, int Wf, Crops crops, int b0, int H, int W, int mode,
                                                             int complement, float norm, float* __restrict__ out) {
  const int bl = blockIdx.y, b = b0 + bl, HW = H * W;
  const int cy = crops.y[bl], cx = crops.x[bl];
  const float* f = flow.p + b * flow.bs;
  const float* g = back.p + b * back.bs;
  float* o = out + (int64_t)b * HW;
  for (int64_t e = (int64_t)blockIdx.x * SS_THREADS + threadIdx.x; e < HW; e += (int64_t)gridDim.x * SS_THREADS) {
    const int y = (int)e / W, x = (int)e - y * W;
    const FB q = fb_at(f, flow.cs, flow.rs, g, back.cs, back.rs, Hf, Wf, x + cx, y + cy);
    float v;
    if (mode == FSRAFT_FB_BROX) {
      v = q.sq > 0.01f * q.ss + 0.5f ? 0.0f : 1.0f;
    } else {
      v = complement ? inconsistency(q, mode, norm) : consistency(q, mode, norm);
    }
    o[e] = v;
  }
}

__global__ __launch_bounds__(SS_THREADS) void selfsup_kernel(View teacher, Crops crops, int b0, const float* __restrict__ tmask, int64_t tm_bs,
                                                             int64_t tm_rs, View student, View sback, int H, int W, int mode, float norm,
                                                             float den_hw, float den_b, float* __restrict__ dflow,
                                                             double* __restrict__ partial) {
  __shared__ double red[SS_THREADS / 64];
  const int bl = blockIdx.y, b = b0 + bl, HW = H * W;
  const float* T = teacher.p + b * teacher.bs + (int64_t)crops.y[bl] * teacher.rs + crops.x[bl];
  const float* S = student.p + b * student.bs;
  const float* Sb = sback.p + b * sback.bs;
  const float* tm = tmask ? tmask + b * tm_bs : nullptr;
  double sum = 0.0;
  for (int64_t e = (int64_t)blockIdx.x * SS_THREADS + threadIdx.x; e < HW; e += (int64_t)gridDim.x * SS_THREADS) {
    const int y = (int)e / W, x = (int)e - y * W;
    float m = tm ? tm[y * tm_rs + x] : 1.0f;
    if (mode != FSRAFT_FB_NONE) {
      const FB q = fb_at(S, student.cs, student.rs, Sb, sback.cs, sback.rs, H, W, x, y);
      m = m * inconsistency(q, mode, norm);
    }
    float gx = 0.0f, gy = 0.0f;
    if (m != 0.0f) {                  // (a masked pixel gets +0.0, not the -0.0 of 0 * a negative slope)
      const int64_t so = (int64_t)y * student.rs + x, to = (int64_t)y * teacher.rs + x;
      const float dx = T[to] - S[so], dy = T[teacher.cs + to] - S[student.cs + so];
      const float ex = sqrtf(dx * dx + 1e-6f), ey = sqrtf(dy * dy + 1e-6f);
      sum += (double)(m * ex) + (double)(m * ey);
      // first by the pixels, then by the batch: a sample alone, divided by the batch's B, gives the bits it gives in the batch
      gx = -(m * (dx / ex)) / den_hw / den_b;
      gy = -(m * (dy / ey)) / den_hw / den_b;
    }
    dflow[((int64_t)b * 2 * H + y) * W + x] = gx;
    dflow[((int64_t)(b * 2 + 1) * H + y) * W + x] = gy;
  }
  const double total = block_sum_f64(sum, red);
  if (threadIdx.x == 0) partial[(int64_t)b * gridDim.x + blockIdx.x] = total;
}

// out[0] = sum of n partials / count, every thread taking partials tid, tid + 256, ... in ascending order.
__global__ __launch_bounds__(SS_THREADS) void selfsup_finalise_kernel(const double* __restrict__ partial, int64_t n, double count,
                                                                     double* __restrict__ out) {
  __shared__ double red[SS_THREADS / 64];
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += SS_THREADS) a += partial[i];
  const double s = block_sum_f64(a, red);
  if (threadIdx.x == 0) out[0] = s / count;
}

static inline int ss_blocks(int64_t hw) {
  const int64_t n = (hw + SS_THREADS - 1) / SS_THREADS;
  return (int)(n < SS_MAX_BLOCKS ? n : SS_MAX_BLOCKS);
}

static inline bool aligned8(const void* p) { return (uintptr_t)p % 8 == 0; }

static inline bool sizes_ok(int B, int H, int W) {
  return B >= 1 && H >= 1 && W >= 1 && (int64_t)H * W <= INT32_MAX;
}

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
  for (int i = 0; i < SS_CHUNK; ++i) {
    c.y[i] = crop_yx && i < nb ? crop_yx[2 * (b0 + i)] : 0;
    c.x[i] = crop_yx && i < nb ? crop_yx[2 * (b0 + i) + 1] : 0;
  }
  return c;
}

}  // namespace

extern "C" int fsraft_fb_mask(const float* flow, int64_t flow_bs, int64_t flow_cs, int64_t flow_rs,
                              const float* flow_back, int64_t back_bs, int64_t back_cs, int64_t back_rs, int Hf, int Wf,
                              const int* crop_yx, int B, int H, int W, int mode, int complement, float norm, float* out, hipStream_t s) {
  if (!flow || !flow_back || !out) return FS_ERR_ARG;
  if (mode != FSRAFT_FB_GAUSSIAN && mode != FSRAFT_FB_DDFLOW && mode != FSRAFT_FB_BROX) return FS_ERR_ARG;
  if ((complement != 0 && complement != 1) || (mode == FSRAFT_FB_GAUSSIAN && !(norm > 0.0f))) return FS_ERR_ARG;
  if (!sizes_ok(B, H, W) || !crops_ok(crop_yx, B, H, W, Hf, Wf)) return FS_ERR_ARG;
  const View f{flow, flow_bs, flow_cs, flow_rs}, g{flow_back, back_bs, back_cs, back_rs};
  const int nblk = ss_blocks((int64_t)H * W);
  for (int b0 = 0; b0 < B; b0 += SS_CHUNK) {
    const int nb = B - b0 < SS_CHUNK ? B - b0 : SS_CHUNK;
    hipLaunchKernelGGL(fb_mask_kernel, dim3(nblk, nb), dim3(SS_THREADS), 0, s, f, g, Hf, Wf, crops_of(crop_yx, b0, nb), b0, H, W, mode,
                       complement, norm, out);
    if (fs_launch_status() != FS_OK) return FS_ERR_LAUNCH;
  }
  return FS_OK;
}

extern "C" int fsraft_selfsup_scratch_bytes(int B, int H, int W) {
  if (!sizes_ok(B, H, W)) return FS_ERR_ARG;
  const int64_t bytes = ((int64_t)B * ss_blocks((int64_t)H * W) * 8 + 63) / 64 * 64;
  return bytes > INT32_MAX ? FS_ERR_ARG : (int)bytes;
}

extern "C" int fsraft_selfsup(const float* teacher, int64_t teacher_bs, int64_t teacher_cs, int64_t teacher_rs, int Hf, int Wf,
                              const int* crop_yx, const float* teacher_mask, int64_t tmask_bs, int64_t tmask_rs,
                              const float* student, int64_t student_bs, int64_t student_cs, int64_t student_rs,
                              const float* student_back, int64_t sback_bs, int64_t sback_cs, int64_t sback_rs, int B, int H, int W,
                              int mode, float norm, float* dflow, double* out, void* scratch, int64_t scratch_bytes, hipStream_t s) {
  if (!teacher || !student || !student_back || !dflow || !out || !scratch || !aligned8(out) || !aligned8(scratch)) return FS_ERR_ARG;
  if (mode != FSRAFT_FB_GAUSSIAN && mode != FSRAFT_FB_DDFLOW && mode != FSRAFT_FB_NONE) return FS_ERR_ARG;
  if (mode == FSRAFT_FB_GAUSSIAN && !(norm > 0.0f)) return FS_ERR_ARG;
  const int need = fsraft_selfsup_scratch_bytes(B, H, W);
  if (need == FS_ERR_ARG || scratch_bytes < need || !crops_ok(crop_yx, B, H, W, Hf, Wf)) return FS_ERR_ARG;
  const View t{teacher, teacher_bs, teacher_cs, teacher_rs}, st{student, student_bs, student_cs, student_rs},
      sb{student_back, sback_bs, sback_cs, sback_rs};
  const int nblk = ss_blocks((int64_t)H * W);
  for (int b0 = 0; b0 < B; b0 += SS_CHUNK) {
    const int nb = B - b0 < SS_CHUNK ? B - b0 : SS_CHUNK;
    hipLaunchKernelGGL(selfsup_kernel, dim3(nblk, nb), dim3(SS_THREADS), 0, s, t, crops_of(crop_yx, b0, nb), b0, teacher_mask, tmask_bs,
                       tmask_rs, st, sb, H, W, mode, norm, (float)(2.0 * H * W), (float)B, dflow, (double*)scratch);
    if (fs_launch_status() != FS_OK) return FS_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(selfsup_finalise_kernel, dim3(1), dim3(SS_THREADS), 0, s, (const double*)scratch, (int64_t)B * nblk,
                     2.0 * B * H * W, out);
  return fs_launch_status();
}
