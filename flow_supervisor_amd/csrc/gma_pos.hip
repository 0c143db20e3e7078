// Row softmax of the GMA attention map with the relative-position terms (RelPosEmb.forward and Attention.forward with
// --position_only / --position_and_content, pytorch/core/gma.py:6-31, 62-74) and its backward.
//
// For query i = (x, y) and key j = (u, v) of an h x w grid the positional logit is hs[i][u] + ws[i][v]: h + w numbers per row of
// n = h * w logits.  They come from one small GEMM, G = scale * q . T^T with T the stacked slices of the two embedding tables
// (2h - 1 rows for the height offsets u - x = -(h-1) .. h-1, then 2w - 1 rows for the width offsets), and are added while the
// row is in LDS for the softmax -- the [n][n] positional tensor of the reference never exists.  The backward reduces dS of the
// row to the same h + w numbers (dG) before the row leaves LDS.
#include "common.hpp"
#include "gemm_rec.hpp"      // rec_split4: the [32 hi | 32 lo] bf16 records the GEMMs on the attention map read

namespace {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// 256 threads = 4 waves; reduce across the workgroup through 4 LDS slots
template <bool MAX>
__device__ __forceinline__ float block_reduce(float v, float* red) {
  v = MAX ? wave_max(v) : wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return MAX ? fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) : (red[0] + red[1]) + (red[2] + red[3]);
}

// One workgroup per row, in place over S [rows][n].  CONTENT: S holds scale * q k^T and the bias is added to it; otherwise S
// is written without being read (position_only).  REC: the probabilities leave as records (n % 32 == 0), bit for bit the
// records of what the dense variant stores.
template <bool CONTENT, bool REC>
__global__ __launch_bounds__(256) void softmax_rows_pos_kernel(float* __restrict__ S, const float* __restrict__ G, int64_t ldg,
                                                               int n, int h, int w) {
  extern __shared__ float row[];            // [ceil4(n)] logits, [h + w] bias of this row
  __shared__ float red[4];
  float* bias = row + ((n + 3) & ~3);
  const int64_t r = blockIdx.x;
  const int q = (int)(r % n), x = q / w, y = q - x * w;
  const float* g = G + r * ldg;
  for (int t = threadIdx.x; t < h + w; t += 256) bias[t] = t < h ? g[t - x + h - 1] : g[(2 * h - 1) + (t - h) - y + w - 1];
  __syncthreads();
  float* p = S + r * n;
  const int n4 = (n & 3) ? 0 : (n >> 2);      // rows are 16-byte aligned only when n % 4 == 0
  float m = -INFINITY;
  for (int i = threadIdx.x; i < n4; i += 256) {
    f32x4 c = {0.f, 0.f, 0.f, 0.f};
    if (CONTENT) c = reinterpret_cast<const f32x4*>(p)[i];
    int u = (i * 4) / w, v = i * 4 - u * w;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      c[k] += bias[u] + bias[h + v];
      if (++v == w) { v = 0; ++u; }
    }
    reinterpret_cast<f32x4*>(row)[i] = c;
    m = fmaxf(fmaxf(m, fmaxf(c[0], c[1])), fmaxf(c[2], c[3]));
  }
  for (int i = (n4 << 2) + threadIdx.x; i < n; i += 256) {
    const int u = i / w, v = i - u * w;
    const float c = (CONTENT ? p[i] : 0.f) + (bias[u] + bias[h + v]);
    row[i] = c;
    m = fmaxf(m, c);
  }
  m = block_reduce<true>(m, red);
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) { const float e = __expf(row[i] - m); row[i] = e; s += e; }
  s = block_reduce<false>(s, red);
  const float inv = 1.0f / s;
  if (REC) {
    char* out = reinterpret_cast<char*>(p);
    for (int u = threadIdx.x; u < (n >> 3); u += 256) {          // 8-float units: 16 bytes of hi and 16 of lo
      float v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {      // (the product rounded as the dense variant stores it: the empty asm keeps hipcc from
        v[i] = row[u * 8 + i] * inv;       //  contracting it into the split's x - hi as an fma on the unrounded product)
        asm volatile("" : "+v"(v[i]));
      }
      uint2 h0, l0, h1, l1;
      rec_split4(v, h0, l0);
      rec_split4(v + 4, h1, l1);
      char* d = out + (u >> 2) * 128 + (u & 3) * 16;
      *reinterpret_cast<u32x4*>(d) = u32x4{h0.x, h0.y, h1.x, h1.y};
      *reinterpret_cast<u32x4*>(d + 64) = u32x4{l0.x, l0.y, l1.x, l1.y};
    }
  } else {
    for (int i = threadIdx.x; i < n4; i += 256) {
      f32x4 v = reinterpret_cast<f32x4*>(row)[i];
      v *= inv;
      reinterpret_cast<f32x4*>(p)[i] = v;
    }
    for (int i = (n4 << 2) + threadIdx.x; i < n; i += 256) p[i] = row[i] * inv;
  }
}

// dS = A * (dA - sum_j dA_j A_j) written over dA (REC: A read as records, dS written as records), and the row's positional
// gradient dG[r][0 .. ldg): dG[u - x + h - 1] = sum_v dS[u][v], dG[(2h-1) + v - y + w - 1] = sum_u dS[u][v], zero elsewhere.
// The sums run in a fixed order (a wave per u over the lanes' v, then the butterfly; a thread per v over u): no atomics.
template <bool REC>
__global__ __launch_bounds__(256) void softmax_rows_pos_bwd_kernel(const void* __restrict__ A, float* __restrict__ dA,
                                                                   float* __restrict__ dG, int64_t ldg, int n, int h, int w) {
  extern __shared__ float row[];          // [2][ceil4(n)]: A row, dA row (then dS); [h + w] sums
  __shared__ float red[4];
  const int npad = (n + 3) & ~3;
  float* ra = row;
  float* rd = row + npad;
  float* acc = rd + npad;
  const int64_t r = blockIdx.x;
  float* d = dA + r * n;
  float dot = 0.f;
  if (REC) {
    const char* a = reinterpret_cast<const char*>(A) + r * n * 4;
    for (int u = threadIdx.x; u < (n >> 3); u += 256) {
      const char* s = a + (u >> 2) * 128 + (u & 3) * 16;
      const u32x4 hh = *reinterpret_cast<const u32x4*>(s), ll = *reinterpret_cast<const u32x4*>(s + 64);
      const f32x4 d0 = reinterpret_cast<const f32x4*>(d)[u * 2], d1 = reinterpret_cast<const f32x4*>(d)[u * 2 + 1];
      float av[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        av[2 * i] = __builtin_bit_cast(float, hh[i] << 16) + __builtin_bit_cast(float, ll[i] << 16);
        av[2 * i + 1] = __builtin_bit_cast(float, hh[i] & 0xffff0000u) + __builtin_bit_cast(float, ll[i] & 0xffff0000u);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) ra[u * 8 + i] = av[i];
      reinterpret_cast<f32x4*>(rd)[u * 2] = d0;
      reinterpret_cast<f32x4*>(rd)[u * 2 + 1] = d1;
#pragma unroll
      for (int i = 0; i < 4; ++i) dot += av[i] * d0[i] + av[4 + i] * d1[i];
    }
  } else {
    const float* a = reinterpret_cast<const float*>(A) + r * n;
    const int n4 = (n & 3) ? 0 : (n >> 2);
    for (int i = threadIdx.x; i < n4; i += 256) {
      const f32x4 av = reinterpret_cast<const f32x4*>(a)[i];
      const f32x4 dv = reinterpret_cast<const f32x4*>(d)[i];
      reinterpret_cast<f32x4*>(ra)[i] = av;
      reinterpret_cast<f32x4*>(rd)[i] = dv;
      dot += av[0] * dv[0] + av[1] * dv[1] + av[2] * dv[2] + av[3] * dv[3];
    }
    for (int i = (n4 << 2) + threadIdx.x; i < n; i += 256) { ra[i] = a[i]; rd[i] = d[i]; dot += a[i] * d[i]; }
  }
  dot = block_reduce<false>(dot, red);
  for (int i = threadIdx.x; i < n; i += 256) rd[i] = ra[i] * (rd[i] - dot);      // dS stays in LDS for the two reductions
  __syncthreads();
  if (REC) {
    char* out = reinterpret_cast<char*>(d);
    for (int u = threadIdx.x; u < (n >> 3); u += 256) {
      uint2 h0, l0, h1, l1;
      rec_split4(rd + u * 8, h0, l0);
      rec_split4(rd + u * 8 + 4, h1, l1);
      char* o = out + (u >> 2) * 128 + (u & 3) * 16;
      *reinterpret_cast<u32x4*>(o) = u32x4{h0.x, h0.y, h1.x, h1.y};
      *reinterpret_cast<u32x4*>(o + 64) = u32x4{l0.x, l0.y, l1.x, l1.y};
    }
  } else {
    const int n4 = (n & 3) ? 0 : (n >> 2);
    for (int i = threadIdx.x; i < n4; i += 256) reinterpret_cast<f32x4*>(d)[i] = reinterpret_cast<const f32x4*>(rd)[i];
    for (int i = (n4 << 2) + threadIdx.x; i < n; i += 256) d[i] = rd[i];
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int u = wave; u < h; u += 4) {                 // consecutive lanes on consecutive LDS words
    float s = 0.f;
    for (int v = lane; v < w; v += 64) s += rd[u * w + v];
    s = wave_sum(s);
    if (lane == 0) acc[u] = s;
  }
  for (int v = threadIdx.x; v < w; v += 256) {
    float s = 0.f;
    for (int u = 0; u < h; ++u) s += rd[u * w + v];
    acc[h + v] = s;
  }
  __syncthreads();
  const int q = (int)(r % n), x = q / w, y = q - x * w;
  float* g = dG + r * ldg;
  for (int c = threadIdx.x; c < ldg; c += 256) {
    float val = 0.f;
    if (c < 2 * h - 1) {
      const int u = c - (h - 1) + x;
      if (u >= 0 && u < h) val = acc[u];
    } else if (c < 2 * h + 2 * w - 2) {
      const int v = c - (2 * h - 1) - (w - 1) + y;
      if (v >= 0 && v < w) val = acc[h + v];
    }
    g[c] = val;
  }
}

// the 64 KB a launch gets without an opt-in, less the kernels' static reduction words
constexpr int64_t kLdsLimit = 65536 - 16;

inline bool bad_grid(int64_t rows, int n, int h, int w, int64_t ldg) {
  return rows < 1 || rows > 0x7fffffff || n < 1 || h < 1 || w < 1 || (int64_t)h * w != n || (rows % n) ||
         ldg < 2 * ((int64_t)h + w) - 2;
}

}  // namespace

// S [rows][n] in place, n = h * w, rows a multiple of n (row r is query r % n); G [rows][ldg], ldg >= 2h + 2w - 2.
// LDS: 4 * ceil4(n) + 4 * (h + w) <= 65520 bytes.  records: n % 32 == 0, S 16-byte aligned.
extern "C" int fsraft_softmax_rows_pos(float* S, const float* G, int64_t ldg, int64_t rows, int n, int h, int w, int content,
                                       int records, hipStream_t s) {
  if (!S || !G || bad_grid(rows, n, h, w, ldg)) return FS_ERR_ARG;
  const int64_t lds = (((int64_t)n + 3) & ~3) * 4 + ((int64_t)h + w) * 4;
  if (lds > kLdsLimit) return FS_ERR_ARG;
  if (records && ((n % 32) || ((uintptr_t)S % 16))) return FS_ERR_ARG;
  const dim3 grid((unsigned)rows), block(256);
  if (records) {
    if (content) hipLaunchKernelGGL((softmax_rows_pos_kernel<true, true>), grid, block, (size_t)lds, s, S, G, ldg, n, h, w);
    else hipLaunchKernelGGL((softmax_rows_pos_kernel<false, true>), grid, block, (size_t)lds, s, S, G, ldg, n, h, w);
  } else {
    if (content) hipLaunchKernelGGL((softmax_rows_pos_kernel<true, false>), grid, block, (size_t)lds, s, S, G, ldg, n, h, w);
    else hipLaunchKernelGGL((softmax_rows_pos_kernel<false, false>), grid, block, (size_t)lds, s, S, G, ldg, n, h, w);
  }
  return fs_launch_status();
}

// A [rows][n] (records != 0: the records of fsraft_softmax_rows_pos), dA [rows][n] fp32 in, dS out in place (as records when
// records != 0), dG [rows][ldg] written whole.  LDS: 8 * ceil4(n) + 4 * (h + w) <= 65520 bytes.  records: n % 32 == 0, A and
// dA 16-byte aligned.
extern "C" int fsraft_softmax_rows_pos_bwd(const void* A, float* dA, float* dG, int64_t ldg, int64_t rows, int n, int h, int w,
                                           int records, hipStream_t s) {
  if (!A || !dA || !dG || bad_grid(rows, n, h, w, ldg)) return FS_ERR_ARG;
  const int64_t lds = (((int64_t)n + 3) & ~3) * 8 + ((int64_t)h + w) * 4;
  if (lds > kLdsLimit) return FS_ERR_ARG;
  if (records && ((n % 32) || ((uintptr_t)A % 16) || ((uintptr_t)dA % 16))) return FS_ERR_ARG;
  const dim3 grid((unsigned)rows), block(256);
  if (records) hipLaunchKernelGGL(softmax_rows_pos_bwd_kernel<true>, grid, block, (size_t)lds, s, A, dA, dG, ldg, n, h, w);
  else hipLaunchKernelGGL(softmax_rows_pos_bwd_kernel<false>, grid, block, (size_t)lds, s, A, dA, dG, ldg, n, h, w);
  return fs_launch_status();
}
