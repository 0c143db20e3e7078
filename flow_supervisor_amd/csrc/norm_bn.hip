// Training-mode BatchNorm2d (+ ReLU, + the residual unit's add and outer ReLU) for channels-last tensors ([B][HW][C] fp32,
// C % 4 == 0, 4 <= C <= 256): torch.nn.BatchNorm2d in training mode behind pytorch/core/extractor.py:13-57, 118-170.  The
// statistics are per channel over all n = B * HW pixels.  As in norm_cl.hip every workgroup walks a strip of one sample's pixels
// with one float4 of channels per lane, reduces across its pixel lanes in LDS (pairwise) and adds its partial sums to one of
// BN_ROWS partial rows with atomics; a one-block finalise kernel adds the rows up and leaves the per-channel constants the apply
// pass reads.  Three launches per direction:
//   forward   sums (read x)            finalise (stats, running statistics)   apply (read x (+res), write y)
//   backward  sums (read g, x (+out);  finalise (dweight, dbias)              apply (read g -- dres with a shortcut --, x; write dx)
//             write dres)
#include "common.hpp"

namespace {

constexpr int BN_ROWS = FSRAFT_BN_PARTIAL_ROWS;
constexpr int BN_TARGET_WGS = 2048;   // workgroups aimed at per launch: eight per CU; each ends in 2 C atomics on BN_ROWS rows
inline int bn_strip(int B, int HW) {  // pixels of one sample per workgroup
  int64_t p = ((int64_t)B * HW + BN_TARGET_WGS - 1) / BN_TARGET_WGS;
  p = (p + 63) / 64 * 64;
  return p < 128 ? 128 : p > 2048 ? 2048 : (int)p;
}

// float offset of channel 0 of pixel p of sample b; s2w = W: in the space-to-depth layout [B][H/2][W/2][2][2][C] (fsraft_space_to_depth2)
__device__ __forceinline__ int64_t bn_pix_off(int b, int p, int HW, int C, int s2w) {
  if (s2w == 0) return ((int64_t)b * HW + p) * C;
  const int y = p / s2w, x = p - y * s2w;
  return (((int64_t)b * (HW >> 2) + (y >> 1) * (s2w >> 1) + (x >> 1)) * 4 + ((y & 1) * 2 + (x & 1))) * C;
}

// Pairwise sum of the lanes_p pixel lanes' partial sums (thread pl * c4n + cl holds lane pl of channel quad cl), left in lane 0:
// the reduction norm_cl.hip documents at cl_reduce_lanes (a chain of adds missed its limit on flat planes).
__device__ __forceinline__ void bn_reduce_lanes(f32x4 (*red)[256], int pl, int lanes_p, int c4n) {
  __syncthreads();
  for (int n = lanes_p; n > 1;) {
    const int half = (n + 1) >> 1;
    if (pl + half < n) {                                   // (the idle tail threads have pl == lanes_p: never)
      red[0][threadIdx.x] += red[0][threadIdx.x + half * c4n];
      red[1][threadIdx.x] += red[1][threadIdx.x + half * c4n];
    }
    __syncthreads();
    n = half;
  }
}

// the workgroup's two column sums -> its partial row of acc [2][BN_ROWS][C]
__device__ __forceinline__ void bn_add_row(const f32x4 (*red)[256], float* __restrict__ acc, int C) {
  if ((int)threadIdx.x < (C >> 2)) {
    const int row = (int)((blockIdx.y * gridDim.x + blockIdx.x) % BN_ROWS);
    float* a0 = acc + row * C + threadIdx.x * 4;
    float* a1 = a0 + BN_ROWS * C;
    const f32x4 t0 = red[0][threadIdx.x], t1 = red[1][threadIdx.x];
#pragma unroll
    for (int i = 0; i < 4; ++i) { atomicAdd(a0 + i, t0[i]); atomicAdd(a1 + i, t1[i]); }
  }
}

// acc[0][row][c] += sum x, acc[1][row][c] += sum x^2 over the workgroup's strip
__global__ __launch_bounds__(256) void bn_fwd_sums_kernel(const float* __restrict__ x, float* __restrict__ acc, int HW, int C, int strip) {
  __shared__ f32x4 red[2][256];
  const int c4n = C >> 2, lanes_p = 256 / c4n;
  const int cl = threadIdx.x % c4n, pl = threadIdx.x / c4n;
  const int b = blockIdx.y;
  const int p0 = blockIdx.x * strip, p1 = min(p0 + strip, HW);
  f32x4 s = {0.f, 0.f, 0.f, 0.f}, q = {0.f, 0.f, 0.f, 0.f};
  if (pl < lanes_p)
#pragma unroll 4
    for (int p = p0 + pl; p < p1; p += lanes_p) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(x + ((int64_t)b * HW + p) * C + cl * 4);
      s += v; q += v * v;
    }
  red[0][threadIdx.x] = s; red[1][threadIdx.x] = q;
  bn_reduce_lanes(red, pl, lanes_p, c4n);
  bn_add_row(red, acc, C);
}

// Column c of the BN_ROWS rows of both sums.  Sixteen rows of each are requested before their first add (rolled, the loop is a
// chain of dependent round trips to L2: bn_fold_bwd_kernel's note in norm_cl.hip), and the four groups are added pairwise.
// (Sixteen rows in all held a chain of 87 atomic adds each at 1387 workgroups: 12 u on the mean of a same-signed channel.)
__device__ __forceinline__ void bn_sum_rows(const float* __restrict__ acc, int C, int c, float& s0, float& s1) {
  static_assert(BN_ROWS == 64, "four groups of sixteen rows");
  float g0[4], g1[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float a[16], q[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { a[r] = acc[(k * 16 + r) * C + c]; q[r] = acc[(BN_ROWS + k * 16 + r) * C + c]; }
    float ta = 0.f, tq = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) { ta += a[r]; tq += q[r]; }
    g0[k] = ta; g1[k] = tq;
  }
  s0 = (g0[0] + g0[1]) + (g0[2] + g0[3]);
  s1 = (g1[0] + g1[1]) + (g1[2] + g1[3]);
}

// one thread per channel: the rows of acc -> stats [4][C] = (mean, rstd, scale, shift), and the running statistics
__global__ void bn_fwd_finalise_kernel(const float* __restrict__ acc, const float* __restrict__ weight, const float* __restrict__ bias,
                                       const float* __restrict__ cbias, float* __restrict__ rm, float* __restrict__ rv, float momentum,
                                       float eps, float n, int C, float* __restrict__ stats) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float su, sq;
  bn_sum_rows(acc, C, c, su, sq);
  const float mean = su / n;
  const float var = fmaxf(sq / n - mean * mean, 0.f);      // biased; the single-pass formula of the instance route
  const float rstd = rsqrtf(var + eps);
  const float scale = weight[c] * rstd;
  stats[c] = mean; stats[C + c] = rstd; stats[2 * C + c] = scale; stats[3 * C + c] = bias[c] - mean * scale;
  if (rm) {
    rm[c] = (1.f - momentum) * rm[c] + momentum * (mean + (cbias ? cbias[c] : 0.f));
    rv[c] = (1.f - momentum) * rv[c] + momentum * (var * (n / (n - 1.f)));
  }
}

// y = relu?(fma(x, scale, shift)), or relu(res + that)
__global__ __launch_bounds__(256) void bn_fwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ res,
                                                           const float* __restrict__ stats, float* __restrict__ y, int HW, int C,
                                                           int relu, int strip, int s2w) {
  const int c4n = C >> 2, lanes_p = 256 / c4n;
  const int cl = threadIdx.x % c4n, pl = threadIdx.x / c4n;
  if (pl >= lanes_p) return;
  const int b = blockIdx.y;
  const f32x4 scale = *reinterpret_cast<const f32x4*>(stats + 2 * C + cl * 4), shift = *reinterpret_cast<const f32x4*>(stats + 3 * C + cl * 4);
  const int p0 = blockIdx.x * strip, p1 = min(p0 + strip, HW);
#pragma unroll 4
  for (int p = p0 + pl; p < p1; p += lanes_p) {
    const int64_t o = ((int64_t)b * HW + p) * C + cl * 4;
    const f32x4 xv = *reinterpret_cast<const f32x4*>(x + o);
    f32x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[i] = fmaf(xv[i], scale[i], shift[i]); if (relu) v[i] = fmaxf(v[i], 0.f); }
    if (res) {
      const f32x4 rv = *reinterpret_cast<const f32x4*>(res + o);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = fmaxf(v[i] + rv[i], 0.f);
    }
    *reinterpret_cast<f32x4*>(y + (s2w ? bn_pix_off(b, p, HW, C, s2w) + cl * 4 : o)) = v;
  }
}

// g' = g [out > 0] [t > 0], t = fma(x, scale, shift) as the forward computed it; xhat = (x - mean) rstd
__device__ __forceinline__ float bn_gate(float g, float x, float scale, float shift, int relu) {
  return (relu && fmaf(x, scale, shift) <= 0.f) ? 0.f : g;
}

// acc[0] += sum g', acc[1] += sum g' xhat; with a shortcut dres = g [out > 0]
__global__ __launch_bounds__(256) void bn_bwd_sums_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                          const float* __restrict__ stats, const float* __restrict__ out,
                                                          float* __restrict__ acc, float* __restrict__ dres, int HW, int C, int relu,
                                                          int strip, int s2w) {
  __shared__ f32x4 red[2][256];
  const int c4n = C >> 2, lanes_p = 256 / c4n;
  const int cl = threadIdx.x % c4n, pl = threadIdx.x / c4n;
  const int b = blockIdx.y;
  const int p0 = blockIdx.x * strip, p1 = min(p0 + strip, HW);
  f32x4 a1 = {0.f, 0.f, 0.f, 0.f}, a2 = {0.f, 0.f, 0.f, 0.f};
  if (pl < lanes_p) {
    const f32x4 mean = *reinterpret_cast<const f32x4*>(stats + cl * 4), rstd = *reinterpret_cast<const f32x4*>(stats + C + cl * 4);
    const f32x4 scale = *reinterpret_cast<const f32x4*>(stats + 2 * C + cl * 4), shift = *reinterpret_cast<const f32x4*>(stats + 3 * C + cl * 4);
#pragma unroll 4
    for (int p = p0 + pl; p < p1; p += lanes_p) {
      const int64_t o = ((int64_t)b * HW + p) * C + cl * 4;
      const int64_t og = s2w ? bn_pix_off(b, p, HW, C, s2w) + cl * 4 : o;       // (the gradient and the saved result)
      f32x4 gv = *reinterpret_cast<const f32x4*>(g + og);
      const f32x4 xv = *reinterpret_cast<const f32x4*>(x + o);
      if (out) {
        const f32x4 ov = *reinterpret_cast<const f32x4*>(out + og);
#pragma unroll
        for (int i = 0; i < 4; ++i) gv[i] = ov[i] > 0.f ? gv[i] : 0.f;
        *reinterpret_cast<f32x4*>(dres + o) = gv;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float gg = bn_gate(gv[i], xv[i], scale[i], shift[i], relu);
        a1[i] += gg;
        a2[i] += gg * ((xv[i] - mean[i]) * rstd[i]);
      }
    }
  }
  red[0][threadIdx.x] = a1; red[1][threadIdx.x] = a2;
  bn_reduce_lanes(red, pl, lanes_p, c4n);
  bn_add_row(red, acc, C);
}

// one thread per channel: dbias = S1, dweight = S2 (the column sums of the rows)
__global__ void bn_bwd_finalise_kernel(const float* __restrict__ acc, int C, float* __restrict__ dweight, float* __restrict__ dbias) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float s1, s2;
  bn_sum_rows(acc, C, c, s1, s2);
  dbias[c] = s1; dweight[c] = s2;
}

// dx = scale (g' - S1 / n - xhat S2 / n).  g: in the layout s2w names; with a shortcut the caller passes dres (plain layout, s2w 0,
// out NULL): exactly g [out > 0], written by the sums pass
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                           const float* __restrict__ stats, const float* __restrict__ dweight,
                                                           const float* __restrict__ dbias, float* __restrict__ dx, float n, int HW,
                                                           int C, int relu, int strip, int s2w) {
  const int c4n = C >> 2, lanes_p = 256 / c4n;
  const int cl = threadIdx.x % c4n, pl = threadIdx.x / c4n;
  if (pl >= lanes_p) return;
  const int b = blockIdx.y;
  const f32x4 mean = *reinterpret_cast<const f32x4*>(stats + cl * 4), rstd = *reinterpret_cast<const f32x4*>(stats + C + cl * 4);
  const f32x4 scale = *reinterpret_cast<const f32x4*>(stats + 2 * C + cl * 4), shift = *reinterpret_cast<const f32x4*>(stats + 3 * C + cl * 4);
  const f32x4 m1 = *reinterpret_cast<const f32x4*>(dbias + cl * 4) / n, m2 = *reinterpret_cast<const f32x4*>(dweight + cl * 4) / n;
  const int p0 = blockIdx.x * strip, p1 = min(p0 + strip, HW);
#pragma unroll 4
  for (int p = p0 + pl; p < p1; p += lanes_p) {
    const int64_t o = ((int64_t)b * HW + p) * C + cl * 4;
    const f32x4 gv = *reinterpret_cast<const f32x4*>(g + (s2w ? bn_pix_off(b, p, HW, C, s2w) + cl * 4 : o));
    const f32x4 xv = *reinterpret_cast<const f32x4*>(x + o);
    f32x4 dv;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float gg = bn_gate(gv[i], xv[i], scale[i], shift[i], relu);
      const float xh = (xv[i] - mean[i]) * rstd[i];
      dv[i] = scale[i] * (gg - m1[i] - xh * m2[i]);
    }
    *reinterpret_cast<f32x4*>(dx + o) = dv;
  }
}

inline bool bn_shape_ok(int B, int HW, int C, int s2d_w) {
  return B >= 1 && HW >= 1 && (int64_t)B * HW >= 2 && C >= 4 && C <= 256 && C % 4 == 0 &&      // (n = 1 has no unbiased variance)
         (s2d_w == 0 || (s2d_w > 0 && (s2d_w & 1) == 0 && HW % s2d_w == 0 && ((HW / s2d_w) & 1) == 0));
}

}  // namespace

extern "C" int fsraft_bnorm_cl_fwd(const float* x, const float* res, const float* weight, const float* bias, const float* cbias,
                                   float* running_mean, float* running_var, float momentum, float eps, float* acc, float* y,
                                   float* stats, int B, int HW, int C, int relu, int s2d_w, hipStream_t s) {
  if (!x || !weight || !bias || !acc || !y || !stats || (running_mean != nullptr) != (running_var != nullptr) ||
      !bn_shape_ok(B, HW, C, s2d_w)) return FS_ERR_ARG;
  const int strip = bn_strip(B, HW);
  dim3 grid(ceil_div(HW, strip), B);
  hipLaunchKernelGGL(bn_fwd_sums_kernel, grid, dim3(256), 0, s, x, acc, HW, C, strip);
  hipLaunchKernelGGL(bn_fwd_finalise_kernel, dim3(1), dim3(256), 0, s, acc, weight, bias, cbias, running_mean, running_var, momentum, eps,
                     (float)((int64_t)B * HW), C, stats);
  hipLaunchKernelGGL(bn_fwd_apply_kernel, grid, dim3(256), 0, s, x, res, stats, y, HW, C, relu, strip, s2d_w);
  return fs_launch_status();
}

extern "C" int fsraft_bnorm_cl_bwd(const float* g, const float* x, const float* stats, const float* out, float* acc, float* dx,
                                   float* dres, float* dweight, float* dbias, int B, int HW, int C, int relu, int s2d_w, hipStream_t s) {
  if (!g || !x || !stats || !acc || !dx || !dweight || !dbias || (out != nullptr) != (dres != nullptr) || !bn_shape_ok(B, HW, C, s2d_w))
    return FS_ERR_ARG;
  const int strip = bn_strip(B, HW);
  const float n = (float)((int64_t)B * HW);
  dim3 grid(ceil_div(HW, strip), B);
  hipLaunchKernelGGL(bn_bwd_sums_kernel, grid, dim3(256), 0, s, g, x, stats, out, acc, dres, HW, C, relu, strip, s2d_w);
  hipLaunchKernelGGL(bn_bwd_finalise_kernel, dim3(1), dim3(256), 0, s, acc, C, dweight, dbias);
  if (dres) hipLaunchKernelGGL(bn_bwd_apply_kernel, grid, dim3(256), 0, s, dres, x, stats, dweight, dbias, dx, n, HW, C, relu, strip, 0);
  else hipLaunchKernelGGL(bn_bwd_apply_kernel, grid, dim3(256), 0, s, g, x, stats, dweight, dbias, dx, n, HW, C, relu, strip, s2d_w);
  return fs_launch_status();
}
