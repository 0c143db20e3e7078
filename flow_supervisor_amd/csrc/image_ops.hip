// Image plumbing of the reference's TensorFlow tree between the model blocks, in list form (up to 32 tensors of one geometry per
// launch):
//   fsraft_box_copy             util/image.py:6-49 crop_bboxes (gather: frame -> window) and pad_bboxes (place: window -> frame,
//                               every other frame element written +0.0 by the same launch); each is the other's backward
//   fsraft_resize_bilinear_fwd  tf.image.resize's default (raft/__init__.py:206-222 resize / resize_flow): half-pixel centres, no
//   fsraft_resize_bilinear_bwd  antialias, optional per-channel factors behind the interpolation; the backward is the exact
//                               transpose as a gather over the destination range of each source pixel: no atomics, one order
//   fsraft_pad_edge             util/pad.py np.pad(..., 'edge') on H and W (util/validate.py:301-315 pad_inputs)
// fp32.  A tensor is [B][H][W][C] read through four element strides (batch, channel, row, x): NHWC is (HWC, 1, WC, C), planar
// [B][C][H][W] is (CHW, HW, W, 1).  One thread per destination unit, blockIdx.y the sample, blockIdx.z the list entry; the
// pointer tables are read from the kernel arguments with scalar loads.  A thread walks the destination in its memory order:
// channel fastest where the destination's channel stride is 1, x fastest otherwise.
//
// Box copy, 16-byte route: a window's row starts x_b * E floats into the frame's (E = C interleaved, 1 planar).  Where both
// tensors are laid out alike with unit inner strides, every base is 16-byte aligned, every outer stride and both row lengths are
// multiples of 4 floats, a sample whose start x_b * E is one too moves float4 units; any other sample of the same launch moves
// single floats (the choice is uniform in a workgroup).  Copies are bit-exact on either route.
#include "common.hpp"
#include <cstddef>

namespace {

constexpr int IM_MAX_LIST = 32;
constexpr int IM_THREADS = 256;
constexpr int IM_CHUNK = 64;             // samples per box-copy launch: their offsets travel by value
constexpr int IM_MAX_B = 65535;          // gridDim.y
constexpr int IM_MAX_FAC = 8;            // channels that can carry a factor

struct Strides { int64_t bs, cs, rs, xs; };

struct Ptrs {
  const float* src[IM_MAX_LIST];
  float* dst[IM_MAX_LIST];
};

typedef const float* cfptr;
typedef float* fptr;

// entry blockIdx.z of the pointer tables, which open the kernel's (single) argument
__device__ __forceinline__ void list_entry(const float*& src, float*& dst) {
  const auto* karg = (const char __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr();
  src = ((const cfptr __attribute__((address_space(4)))*)(karg + offsetof(Ptrs, src)))[blockIdx.z];
  dst = ((const fptr __attribute__((address_space(4)))*)(karg + offsetof(Ptrs, dst)))[blockIdx.z];
}

// unit `idx` of a sample's Hd x Wd x C destination in its memory order
__device__ __forceinline__ void split(int idx, int inter, int C, int Hd, int Wd, int& c, int& y, int& x) {
  if (inter) {
    c = idx % C; idx /= C;
    x = idx % Wd; y = idx / Wd;
  } else {
    x = idx % Wd; idx /= Wd;
    y = idx % Hd; c = idx / Hd;
  }
}

__device__ __forceinline__ int64_t at(const Strides& s, int b, int c, int y, int x) {
  return (int64_t)b * s.bs + (int64_t)c * s.cs + (int64_t)y * s.rs + (int64_t)x * s.xs;
}

// ------------------------------------------------------------------------------------------------------------------ box copy
struct BoxArgs {
  Ptrs p;                                // first: list_entry reads it at offset 0
  int y0[IM_CHUNK], x0[IM_CHUNK];
  Strides f, w;                          // frame, window
  int C, Hf, Wf, H, W;
  int inter;                             // the destination's channel stride is 1
  int vec;                               // bases, strides and row lengths allow float4 units
  int b0;
};

template <bool PLACE>
__global__ __launch_bounds__(IM_THREADS) void box_copy_kernel(BoxArgs a) {
  const float* src; float* dst;
  list_entry(src, dst);
  const int b = a.b0 + blockIdx.y;
  const int y0 = a.y0[blockIdx.y], x0 = a.x0[blockIdx.y];
  const int Hd = PLACE ? a.Hf : a.H, Wd = PLACE ? a.Wf : a.W;
  const int total = a.C * Hd * Wd;
  const int idx = blockIdx.x * IM_THREADS + threadIdx.x;
  const int E = a.inter ? a.C : 1;
  if (a.vec && ((x0 * E) & 3) == 0) {
    if (idx >= total / 4) return;
    const int upr = Wd * E / 4;                          // units per destination row
    const int r = idx / upr, j = (idx - r * upr) * 4;    // row (plane-major), float within it
    const int c = a.inter ? 0 : r / Hd, y = a.inter ? r : r - c * Hd;
    const int64_t pb = (int64_t)b, pc = (int64_t)c;
    if (PLACE) {
      const int jw = j - x0 * E;
      const bool in = y >= y0 && y < y0 + a.H && jw >= 0 && jw < a.W * E;
      f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
      if (in) v = gload4(src + pb * a.w.bs + pc * a.w.cs + (int64_t)(y - y0) * a.w.rs + jw);
      gstore4(dst + pb * a.f.bs + pc * a.f.cs + (int64_t)y * a.f.rs + j, v);
    } else {
      gstore4(dst + pb * a.w.bs + pc * a.w.cs + (int64_t)y * a.w.rs + j,
              gload4(src + pb * a.f.bs + pc * a.f.cs + (int64_t)(y + y0) * a.f.rs + x0 * E + j));
    }
    return;
  }
  if (idx >= total) return;
  int c, y, x;
  split(idx, a.inter, a.C, Hd, Wd, c, y, x);
  if (PLACE) {
    const int yw = y - y0, xw = x - x0;
    const bool in = yw >= 0 && yw < a.H && xw >= 0 && xw < a.W;
    gstore1(dst + at(a.f, b, c, y, x), in ? gload1(src + at(a.w, b, c, yw, xw)) : 0.0f);
  } else {
    gstore1(dst + at(a.w, b, c, y, x), gload1(src + at(a.f, b, c, y + y0, x + x0)));
  }
}

// ------------------------------------------------------------------------------------------------------------ bilinear resize
struct ResizeArgs {
  Ptrs p;
  Strides s, d;                          // the Hi x Wi side, the Ho x Wo side
  int C, Hi, Wi, Ho, Wo;
  float sy, sx;                          // (float)n_in / (float)n_out
  float iy, ix;                          // (float)n_out / (float)n_in: first guesses of the backward's ranges only
  float fac[IM_MAX_FAC];
  int has_fac;
  int inter;
};

// factor c of the kernel's argument, read from the argument segment (a by-value array indexed per lane would go through scratch)
__device__ __forceinline__ float factor_of(int c) {
  const auto* karg = (const char __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr();
  return ((const float __attribute__((address_space(4)))*)(karg + offsetof(ResizeArgs, fac)))[c];
}

// TF's HalfPixelScaler and compute_interpolation_weights in float32: a product rounded, then a difference rounded.  Contraction is
// switched off for this function: the compiler's default would fuse the two into one fma (__fmul_rn / __fsub_rn are plain
// operators here and fuse as well), which moves the coordinate by an ulp where the scale is not a dyadic fraction.
__device__ __forceinline__ void taps(int o, float scale, int n_in, int& lo, int& hi, float& lerp) {
#pragma clang fp contract(off)
  const float prod = ((float)o + 0.5f) * scale;
  const float in = prod - 0.5f;
  const float fl = floorf(in);
  lo = max((int)fl, 0);
  hi = min((int)ceilf(in), n_in - 1);
  lerp = in - fl;
}

__global__ __launch_bounds__(IM_THREADS) void resize_fwd_kernel(ResizeArgs a) {
  const float* src; float* dst;
  list_entry(src, dst);
  const int idx = blockIdx.x * IM_THREADS + threadIdx.x;
  if (idx >= a.C * a.Ho * a.Wo) return;
  const int b = blockIdx.y;
  int c, y, x;
  split(idx, a.inter, a.C, a.Ho, a.Wo, c, y, x);
  int yl, yh, xl, xh;
  float ly, lx;
  taps(y, a.sy, a.Hi, yl, yh, ly);
  taps(x, a.sx, a.Wi, xl, xh, lx);
  const float tl = gload1(src + at(a.s, b, c, yl, xl)), tr = gload1(src + at(a.s, b, c, yl, xh));
  const float bl = gload1(src + at(a.s, b, c, yh, xl)), br = gload1(src + at(a.s, b, c, yh, xh));
  const float top = tl + (tr - tl) * lx, bot = bl + (br - bl) * lx;
  float v = top + (bot - top) * ly;
  if (a.has_fac) v *= factor_of(c);
  gstore1(dst + at(a.d, b, c, y, x), v);
}

// [o0, o1): the destination indices one of whose two taps is source i.  lo(o) and hi(o) do not decrease with o (every float32
// step of taps() is monotone) and hi - lo <= 1, so the set is the run from the first o with hi(o) >= i to the last with
// lo(o) <= i.  An analytic first guess is walked to the exact ends with taps() itself.
__device__ __forceinline__ void reach(int i, float scale, float inv, int n_in, int n_out, int& o0, int& o1) {
  int lo, hi;
  float lerp;
  int g = (int)floorf(((float)i - 0.5f) * inv - 0.5f);                  // in(o) = i - 1 there
  g = min(max(g, 0), n_out);
  while (g > 0) { taps(g - 1, scale, n_in, lo, hi, lerp); if (hi < i) break; --g; }
  while (g < n_out) { taps(g, scale, n_in, lo, hi, lerp); if (hi >= i) break; ++g; }
  o0 = g;
  int e = (int)ceilf(((float)i + 1.5f) * inv - 0.5f);                   // in(o) = i + 1 there
  e = min(max(e, o0), n_out);
  while (e < n_out) { taps(e, scale, n_in, lo, hi, lerp); if (lo > i) break; ++e; }
  while (e > o0) { taps(e - 1, scale, n_in, lo, hi, lerp); if (lo <= i) break; --e; }
  o1 = e;
}

// the weight of source i in destination o, given lo(o) <= i <= hi(o): the derivative of tl + (tr - tl) * lerp
__device__ __forceinline__ float tap_weight(int i, int lo, int hi, float lerp) {
  return lo == hi ? 1.0f : (i == lo ? 1.0f - lerp : lerp);
}

// src = the upstream gradient [Ho x Wo], dst = the source's gradient [Hi x Wi]: rows ascending, columns ascending inside
__global__ __launch_bounds__(IM_THREADS) void resize_bwd_kernel(ResizeArgs a) {
  const float* src; float* dst;
  list_entry(src, dst);
  const int idx = blockIdx.x * IM_THREADS + threadIdx.x;
  if (idx >= a.C * a.Hi * a.Wi) return;
  const int b = blockIdx.y;
  int c, y, x;
  split(idx, a.inter, a.C, a.Hi, a.Wi, c, y, x);
  int ya, yb, xa, xb;
  reach(y, a.sy, a.iy, a.Hi, a.Ho, ya, yb);
  reach(x, a.sx, a.ix, a.Wi, a.Wo, xa, xb);
  float acc = 0.0f;
  for (int yo = ya; yo < yb; ++yo) {
    int lo, hi;
    float lerp;
    taps(yo, a.sy, a.Hi, lo, hi, lerp);
    const float wy = tap_weight(y, lo, hi, lerp);
    for (int xo = xa; xo < xb; ++xo) {
      taps(xo, a.sx, a.Wi, lo, hi, lerp);
      acc += (wy * tap_weight(x, lo, hi, lerp)) * gload1(src + at(a.d, b, c, yo, xo));
    }
  }
  if (a.has_fac) acc *= factor_of(c);
  gstore1(dst + at(a.s, b, c, y, x), acc);
}

// ---------------------------------------------------------------------------------------------------------------- edge padding
struct PadArgs {
  Ptrs p;
  Strides s, d;
  int C, H, W, Hd, Wd, top, left;
  int inter;
};

__global__ __launch_bounds__(IM_THREADS) void pad_edge_kernel(PadArgs a) {
  const float* src; float* dst;
  list_entry(src, dst);
  const int idx = blockIdx.x * IM_THREADS + threadIdx.x;
  if (idx >= a.C * a.Hd * a.Wd) return;
  const int b = blockIdx.y;
  int c, y, x;
  split(idx, a.inter, a.C, a.Hd, a.Wd, c, y, x);
  const int ys = min(max(y - a.top, 0), a.H - 1), xs = min(max(x - a.left, 0), a.W - 1);
  gstore1(dst + at(a.d, b, c, y, x), gload1(src + at(a.s, b, c, ys, xs)));
}

// --------------------------------------------------------------------------------------------------------------------- host
static inline bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

static inline bool fits(int C, int H, int W) {
  return C >= 1 && H >= 1 && W >= 1 && (int64_t)C * H * W <= INT32_MAX;
}

static bool fill_list(Ptrs& p, const float* const* src, float* const* dst, int n) {
  if (!src || !dst || n < 1 || n > IM_MAX_LIST) return false;
  for (int i = 0; i < n; ++i) {
    if (!src[i] || !dst[i]) return false;
    p.src[i] = src[i]; p.dst[i] = dst[i];
  }
  return true;
}

static inline int blocks_of(int64_t units) { return (int)((units + IM_THREADS - 1) / IM_THREADS); }

}  // namespace

extern "C" int fsraft_box_copy(const float* const* src, float* const* dst, int n, int place, int B, int C, int Hf, int Wf, int H, int W,
                               const int* yx, int64_t f_bs, int64_t f_cs, int64_t f_rs, int64_t f_xs,
                               int64_t w_bs, int64_t w_cs, int64_t w_rs, int64_t w_xs, hipStream_t s) {
  BoxArgs a{};
  if (!fill_list(a.p, src, dst, n) || !yx || B < 1 || !fits(C, Hf, Wf) || !fits(C, H, W) || H > Hf || W > Wf) return FS_ERR_ARG;
  for (int b = 0; b < B; ++b) {
    const int y = yx[2 * b], x = yx[2 * b + 1];
    if (y < 0 || x < 0 || y > Hf - H || x > Wf - W) return FS_ERR_ARG;
  }
  a.f = {f_bs, f_cs, f_rs, f_xs}; a.w = {w_bs, w_cs, w_rs, w_xs};
  a.C = C; a.Hf = Hf; a.Wf = Wf; a.H = H; a.W = W;
  a.inter = (place ? f_cs : w_cs) == 1;
  const bool inter_both = f_cs == 1 && w_cs == 1 && f_xs == C && w_xs == C;
  const bool planar_both = !a.inter && f_xs == 1 && w_xs == 1 && f_cs % 4 == 0 && w_cs % 4 == 0;
  const int E = a.inter ? C : 1;
  bool vec = (a.inter ? inter_both : planar_both) && f_bs % 4 == 0 && w_bs % 4 == 0 && f_rs % 4 == 0 && w_rs % 4 == 0 &&
             ((int64_t)W * E) % 4 == 0 && ((int64_t)Wf * E) % 4 == 0;
  for (int i = 0; i < n; ++i) vec = vec && aligned16(src[i]) && aligned16(dst[i]);
  a.vec = vec;
  const int64_t total = (int64_t)C * (place ? Hf : H) * (place ? Wf : W);
  for (int b0 = 0; b0 < B; b0 += IM_CHUNK) {
    const int nb = B - b0 < IM_CHUNK ? B - b0 : IM_CHUNK;
    bool all_vec = vec;
    for (int i = 0; i < IM_CHUNK; ++i) {
      a.y0[i] = i < nb ? yx[2 * (b0 + i)] : 0;
      a.x0[i] = i < nb ? yx[2 * (b0 + i) + 1] : 0;
      all_vec = all_vec && (((int64_t)a.x0[i] * E) % 4 == 0);
    }
    a.b0 = b0;
    const dim3 grid(blocks_of(all_vec ? total / 4 : total), nb, n);
    if (place) hipLaunchKernelGGL(box_copy_kernel<true>, grid, dim3(IM_THREADS), 0, s, a);
    else hipLaunchKernelGGL(box_copy_kernel<false>, grid, dim3(IM_THREADS), 0, s, a);
  }
  return fs_launch_status();
}

static int resize_launch(bool bwd, const float* const* src, float* const* dst, int n, int B, int C, int Hi, int Wi, int Ho, int Wo,
                         const Strides& in, const Strides& out, const float* factors, hipStream_t s) {
  ResizeArgs a{};
  if (!fill_list(a.p, src, dst, n) || B < 1 || B > IM_MAX_B || !fits(C, Hi, Wi) || !fits(C, Ho, Wo)) return FS_ERR_ARG;
  if (factors && C > IM_MAX_FAC) return FS_ERR_ARG;
  a.s = in; a.d = out;
  a.C = C; a.Hi = Hi; a.Wi = Wi; a.Ho = Ho; a.Wo = Wo;
  a.sy = (float)Hi / (float)Ho; a.sx = (float)Wi / (float)Wo;
  a.iy = (float)Ho / (float)Hi; a.ix = (float)Wo / (float)Wi;
  a.has_fac = factors != nullptr;
  for (int c = 0; factors && c < C; ++c) a.fac[c] = factors[c];
  a.inter = (bwd ? in.cs : out.cs) == 1;
  const int64_t total = (int64_t)C * (bwd ? Hi : Ho) * (bwd ? Wi : Wo);
  const dim3 grid(blocks_of(total), B, n);
  if (bwd) hipLaunchKernelGGL(resize_bwd_kernel, grid, dim3(IM_THREADS), 0, s, a);
  else hipLaunchKernelGGL(resize_fwd_kernel, grid, dim3(IM_THREADS), 0, s, a);
  return fs_launch_status();
}

extern "C" int fsraft_resize_bilinear_fwd(const float* const* src, float* const* dst, int n, int B, int C, int Hi, int Wi, int Ho, int Wo,
                                          int64_t s_bs, int64_t s_cs, int64_t s_rs, int64_t s_xs,
                                          int64_t d_bs, int64_t d_cs, int64_t d_rs, int64_t d_xs, const float* factors, hipStream_t s) {
  return resize_launch(false, src, dst, n, B, C, Hi, Wi, Ho, Wo, {s_bs, s_cs, s_rs, s_xs}, {d_bs, d_cs, d_rs, d_xs}, factors, s);
}

extern "C" int fsraft_resize_bilinear_bwd(const float* const* ddst, float* const* dsrc, int n, int B, int C, int Hi, int Wi, int Ho, int Wo,
                                          int64_t s_bs, int64_t s_cs, int64_t s_rs, int64_t s_xs,
                                          int64_t d_bs, int64_t d_cs, int64_t d_rs, int64_t d_xs, const float* factors, hipStream_t s) {
  return resize_launch(true, ddst, dsrc, n, B, C, Hi, Wi, Ho, Wo, {s_bs, s_cs, s_rs, s_xs}, {d_bs, d_cs, d_rs, d_xs}, factors, s);
}

extern "C" int fsraft_pad_edge(const float* const* src, float* const* dst, int n, int B, int C, int H, int W,
                               int top, int bottom, int left, int right, int64_t s_bs, int64_t s_cs, int64_t s_rs, int64_t s_xs,
                               int64_t d_bs, int64_t d_cs, int64_t d_rs, int64_t d_xs, hipStream_t s) {
  PadArgs a{};
  if (!fill_list(a.p, src, dst, n) || B < 1 || B > IM_MAX_B || !fits(C, H, W)) return FS_ERR_ARG;
  if (top < 0 || bottom < 0 || left < 0 || right < 0) return FS_ERR_ARG;
  const int64_t Hd = (int64_t)H + top + bottom, Wd = (int64_t)W + left + right;
  if (Hd > INT32_MAX || Wd > INT32_MAX || !fits(C, (int)Hd, (int)Wd)) return FS_ERR_ARG;
  a.s = {s_bs, s_cs, s_rs, s_xs}; a.d = {d_bs, d_cs, d_rs, d_xs};
  a.C = C; a.H = H; a.W = W; a.Hd = (int)Hd; a.Wd = (int)Wd; a.top = top; a.left = left;
  a.inter = d_cs == 1;
  hipLaunchKernelGGL(pad_edge_kernel, dim3(blocks_of((int64_t)C * Hd * Wd), B, n), dim3(IM_THREADS), 0, s, a);
  return fs_launch_status();
}
