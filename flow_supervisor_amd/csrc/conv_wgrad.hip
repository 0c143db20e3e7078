// Weight gradient of the convolutions of conv_igemm.hip (see there for the GEMM view and the packed-K layout): the transposed
// product  dWpk[co][k] += sum_m dY[m,co] * Xg[m,k]  with the pixel dimension split across workgroups and fp32 atomics into the
// packed layout.  Entry points: fsraft_conv_wgrad, fsraft_conv_wgrad_multi.
#include "conv_common.hpp"

namespace {

// ---------------------------------------------------------------- weight gradient
struct WgradArgs {
  const float* dy; int ldy; int Cout;     // dY (already multiplied by act'), [M][ldy]
  Src src[3]; int nsrc;
  float* dwpk; int Ktot;
  int B, H, W, KH, KW;
  int kchunk;                              // pixels per split (multiple of 32)
  float* dbias;                            // optional: dbias[co] += sum_pixels dY[pixel][co] (fused in the split kernel)
  // XCD-aware launch (xcd_xt > 0): 1-D grid; the xcd_xt packed-K tiles that read the SAME dY tile -- one (Cout tile, pixel
  // split) group -- get linear ids 8 apart, i.e. the same XCD and its L2, instead of being dealt round-robin over all 8.
  int xcd_xt, xcd_yt, xcd_groups;
};

// Several (dY, X) pairs of identical shape in one launch -- the 12 iterations of a step: dW = sum_t dY_t^T X_t is one
// reduction over 12 x M pixels, so the per-launch prologue / atomic epilogue is paid once per step instead of once
// per iteration.  blockIdx.z = segment * zs + pixel split.  The pointer tables are read from the kernarg segment.
constexpr int WGRAD_MAX_SEG = 16;
struct WgradArgsM {
  WgradArgs a;
  int nseg, zs;
  const float* dys[WGRAD_MAX_SEG];
  const float* srcs[3][WGRAD_MAX_SEG];
};

template <class Cfg>
struct ShiftedXLoader {                    // Bs[k = pixel][n = ci] <- X[pixel + off][ci0 + n]
  static constexpr int BN = Cfg::BN, BK = Cfg::BK, LD = Cfg::LDB;
  static constexpr int F4 = BN / 4;
  static constexpr int NF4 = BK * F4 / 256;
  static constexpr int NREG = NF4 * 4;
  static constexpr int NCH = NF4;
  const float* p; int ld, cvalid;          // p already offset by ci0; cvalid = channels left from ci0
  int dy, dx, H, W, HW; int64_t M; int64_t m_begin, m_end;
  __device__ __forceinline__ bool fetch_chunk(int kt, float (&r)[NREG], int j) const {
    const int e = threadIdx.x + 256 * j;
    const int k = e / F4, c4 = e % F4;
    const int64_t m = m_begin + (int64_t)kt * BK + k;
    const int64_t mm = m < m_end ? m : m_begin;
    const int64_t b = mm / HW; const int pix = (int)(mm % HW);
    const int yy = pix / W + dy, xx = pix % W + dx;
    const bool ok = m < m_end && c4 * 4 < cvalid && yy >= 0 && yy < H && xx >= 0 && xx < W;
    const f32x4 v = gload4(p + (ok ? (b * HW + (int64_t)yy * W + xx) * ld + c4 * 4 : 0));
    r[4 * j + 0] = v[0]; r[4 * j + 1] = v[1]; r[4 * j + 2] = v[2]; r[4 * j + 3] = v[3];
    return ok;
  }
  __device__ __forceinline__ void store_chunk(float* t, const float (&r)[NREG], int j, bool ok) const {
    const int e = threadIdx.x + 256 * j;
    const int k = e / F4, c4 = e % F4;
    f32x4 v = {r[4 * j + 0], r[4 * j + 1], r[4 * j + 2], r[4 * j + 3]};
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    *reinterpret_cast<f32x4*>(t + k * LD + c4 * 4) = ok ? v : z;
  }
};

template <class Cfg>
struct DyLoader {                          // As[k = pixel][m = co] <- dY[pixel][co0 + m]
  static constexpr int BM = Cfg::BM, BK = Cfg::BK, LD = Cfg::LDA;
  static constexpr int F4 = BM / 4;
  static constexpr int NF4 = BK * F4 / 256;
  static constexpr int NREG = NF4 * 4;
  static_assert((BK * F4) % 256 == 0, "dy tile must divide over 256 threads");
  static constexpr int NCH = NF4;
  const float* p; int ld, cvalid; int64_t m_begin, m_end;
  __device__ __forceinline__ bool fetch_chunk(int kt, float (&r)[NREG], int j) const {
    const int e = threadIdx.x + 256 * j;
    const int k = e / F4, c4 = e % F4;
    const int64_t m = m_begin + (int64_t)kt * BK + k;
    const bool ok = m < m_end && c4 * 4 < cvalid;
    const f32x4 v = gload4(p + (ok ? m * ld + c4 * 4 : 0));
    r[4 * j + 0] = v[0]; r[4 * j + 1] = v[1]; r[4 * j + 2] = v[2]; r[4 * j + 3] = v[3];
    return ok;
  }
  __device__ __forceinline__ void store_chunk(float* t, const float (&r)[NREG], int j, bool ok) const {
    const int e = threadIdx.x + 256 * j;
    const int k = e / F4, c4 = e % F4;
    f32x4 v = {r[4 * j + 0], r[4 * j + 1], r[4 * j + 2], r[4 * j + 3]};
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    *reinterpret_cast<f32x4*>(t + k * LD + c4 * 4) = ok ? v : z;
  }
};

// ---- split-bf16 weight gradient (k-major operands, transposed LDS reads) ---------------------
template <class Cfg>
struct SplitDyLoader {                    // chunk e: pixel k = e / 32, channels 4*(e % 32) .. +3 of the 128-wide co tile
  static constexpr int NCH = Cfg::NCH_A, NREG = NCH * 4;
  const float* p; int ld, cvalid; int64_t m_begin, m_end;
  __device__ __forceinline__ void fetch_chunk(int kt, float (&r)[NREG], int j) const {
    const int e = threadIdx.x + 256 * j;
    const int k = e / (Cfg::BM / 4), c4 = e % (Cfg::BM / 4);
    const int64_t m = m_begin + (int64_t)kt * 32 + k;
    const bool ok = m < m_end && c4 * 4 < cvalid;
    const f32x4 v = gload4(ok ? p + m * ld + c4 * 4 : g_fsraft_zero16);
    r[4 * j + 0] = v[0]; r[4 * j + 1] = v[1]; r[4 * j + 2] = v[2]; r[4 * j + 3] = v[3];
  }
};
template <class Cfg>
struct SplitShiftedXLoader {
  static constexpr int NCH = Cfg::NCH_B, NREG = NCH * 4;
  const float* p; int ld, cvalid;
  int dy, dx, H, W, HW; int64_t m_begin, m_end;
  __device__ __forceinline__ void fetch_chunk(int kt, float (&r)[NREG], int j) const {
    const int e = threadIdx.x + 256 * j;
    const int k = e / (Cfg::BN / 4), c4 = e % (Cfg::BN / 4);
    const int64_t m = m_begin + (int64_t)kt * 32 + k;
    const int64_t mm = m < m_end ? m : m_begin;
    const int pix = (int)(mm % HW);
    const int yy = pix / W + dy, xx = pix % W + dx;
    const bool ok = m < m_end && c4 * 4 < cvalid && (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
    const f32x4 v = gload4(ok ? p + (mm + dy * W + dx) * ld + c4 * 4 : g_fsraft_zero16);
    r[4 * j + 0] = v[0]; r[4 * j + 1] = v[1]; r[4 * j + 2] = v[2]; r[4 * j + 3] = v[3];
  }
};

// buffer-addressed variants of the two loaders above (see BufConvALoader): per-lane offsets are fixed for the whole
// k-loop, the k-tile advance is one SGPR offset, and the "shifted pixel inside the image" test -- three integer
// divisions per 16-byte chunk in the loaders above, ~300 VALU instructions per k-tile -- is a bit test against a
// per-workgroup pixel mask that is computed once (one word per k-tile, in LDS).
constexpr int WGRAD_MASK_WORDS = 2048;     // pixels per workgroup / 32 (host caps the pixel split at 65536)
template <class Cfg>
struct BufDyLoader {
  static constexpr int NCH = Cfg::NCH_A, NREG = NCH * 4;
  const float* base; unsigned ld4; int npix;
  unsigned voff[NCH]; int krow[NCH];
  __device__ __forceinline__ void fetch_tile(int kt, float (&r)[NREG]) const {
    const int ku = __builtin_amdgcn_readfirstlane(kt);
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(base, 0x7fffffffu);
    const unsigned soff = (unsigned)ku * 32u * ld4;
    const int left = npix - ku * 32;                              // rows of this tile that exist
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      const unsigned voffj = voff[j] | (krow[j] < left ? 0u : FS_OOB);
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, voffj, soff, 0);
      const f32x4 f = __builtin_bit_cast(f32x4, v);
      r[4 * j + 0] = f[0]; r[4 * j + 1] = f[1]; r[4 * j + 2] = f[2]; r[4 * j + 3] = f[3];
    }
  }
};
template <class Cfg>
struct BufShiftedXLoader {
  static constexpr int NCH = Cfg::NCH_B, NREG = NCH * 4;
  const float* base; unsigned ld4; const unsigned* mask;       // mask: LDS, bit k of word kt = pixel mb + 32 kt + k usable
  unsigned voff[NCH]; int krow[NCH];
  __device__ __forceinline__ void fetch_tile(int kt, float (&r)[NREG]) const {
    const int ku = __builtin_amdgcn_readfirstlane(kt);
    const unsigned w = __builtin_amdgcn_readfirstlane(mask[ku]);
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(base, 0x7fffffffu);
    const unsigned soff = (unsigned)ku * 32u * ld4;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      const unsigned voffj = voff[j] | ((__builtin_amdgcn_ubfe(w, (unsigned)krow[j], 1u) ^ 1u) << 31);
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, voffj, soff, 0);
      const f32x4 f = __builtin_bit_cast(f32x4, v);
      r[4 * j + 0] = f[0]; r[4 * j + 1] = f[1]; r[4 * j + 2] = f[2]; r[4 * j + 3] = f[3];
    }
  }
};


template <class Cfg, bool BUF = false, bool MULTI = false>
__global__ __launch_bounds__(Cfg::NT) void conv_wgrad_split_kernel(const std::conditional_t<MULTI, WgradArgsM, WgradArgs> args) {
  static_assert(Cfg::NT == 256 || BUF, "512-thread workgroups use the buffer-addressed loaders");
  __shared__ __attribute__((aligned(16))) char lds[Cfg::LDS_BYTES];
  __shared__ unsigned pixmask[BUF ? WGRAD_MASK_WORDS : 1];
  const WgradArgs& a = [&]() -> const WgradArgs& { if constexpr (MULTI) return args.a; else return args; }();
  int bx = blockIdx.x, by = blockIdx.y, zblock = blockIdx.z, seg = 0;
  if (a.xcd_xt > 0) {
    const int span = 8 * a.xcd_xt, r = blockIdx.x / span, rem = blockIdx.x - r * span;
    const int g = r * 8 + (rem & 7);
    if (g >= a.xcd_groups) return;
    if (a.xcd_yt > 0) { bx = rem >> 3; by = g % a.xcd_yt; zblock = g / a.xcd_yt; }        // group = (Cout tile, pixel split)
    else { const int tile = rem >> 3, x0 = -a.xcd_yt; bx = tile % x0; by = tile / x0; zblock = g; }   // group = pixel split
  }
  if constexpr (MULTI) { seg = zblock / args.zs; zblock -= seg * args.zs; seg = __builtin_amdgcn_readfirstlane(seg); }
  const int HW = a.H * a.W;
  const int64_t M = (int64_t)a.B * HW;
  const int taps = a.KH * a.KW;
  int t = bx, s = 0, kofs = 0;
  for (;; ++s) {
    const int ct = (a.src[s].C + Cfg::BN - 1) / Cfg::BN;
    if (t < taps * ct) break;
    t -= taps * ct;
    kofs += taps * ((a.src[s].C + 31) / 32) * 32;
  }
  Src sc = s == 0 ? a.src[0] : s == 1 ? a.src[1] : a.src[2];
  const float* dyp = a.dy;
  if constexpr (MULTI) {       // this segment's tensors, read from the kernarg tables with a uniform index
    typedef const float* fptr;
    const auto* karg = (const char __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr();
    dyp = ((const fptr __attribute__((address_space(4)))*)(karg + offsetof(WgradArgsM, dys)))[seg];
    sc.p = ((const fptr __attribute__((address_space(4)))*)(karg + offsetof(WgradArgsM, srcs)))[s * WGRAD_MAX_SEG + seg];
  }
  const int ct = (sc.C + Cfg::BN - 1) / Cfg::BN;
  const int tap = t / ct, ci0 = (t % ct) * Cfg::BN;
  const int cpad = ((sc.C + 31) / 32) * 32;
  kofs += tap * cpad + ci0;
  const int co0 = by * Cfg::BM;
  const int64_t mb = (int64_t)zblock * a.kchunk;
  const int64_t me = mb + a.kchunk < M ? mb + a.kchunk : M;
  if (mb >= M) return;
  const int coleft = ((a.Cout + 3) / 4) * 4 - co0;     // dy may be a channel slice of a wider buffer: never read past it
  const int cleft = ((sc.C + 3) / 4) * 4 - ci0;
  const int dyy = tap / a.KW - a.KH / 2, dxx = tap % a.KW - a.KW / 2;
  const int KT = (int)((me - mb + 31) / 32);
  f32x16 acc[Cfg::TM][Cfg::TN];
#pragma unroll
  for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
    for (int j = 0; j < Cfg::TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  float colsum[4] = {0.f, 0.f, 0.f, 0.f};
  const bool want_bias = a.dbias != nullptr && bx == 0;        // one x-tile per (co tile, pixel split) owns the bias
  if constexpr (BUF) {
    // pixel mask: bit k of word w <=> pixel mb + 32 w + k exists and its (dy, dx)-shifted neighbour is inside the image
    for (int i = threadIdx.x; i < KT * 32; i += Cfg::NT) {
      const int64_t m = mb + i;
      bool ok = m < me;
      if (ok) {
        const int pix = (int)(m % HW), yy = pix / a.W + dyy, xx = pix % a.W + dxx;
        ok = (unsigned)yy < (unsigned)a.H && (unsigned)xx < (unsigned)a.W;
      }
      const unsigned long long bal = __ballot(ok);
      if ((threadIdx.x & 63) == 0) { pixmask[i >> 5] = (unsigned)bal; pixmask[(i >> 5) + 1] = (unsigned)(bal >> 32); }
    }
    __syncthreads();
    BufDyLoader<Cfg> la;
    la.base = uni_ptr(dyp + co0 + mb * a.ldy); la.ld4 = uni((unsigned)a.ldy * 4u); la.npix = (int)(me - mb);
    const int cva = coleft < Cfg::BM ? coleft : Cfg::BM;
#pragma unroll
    for (int j = 0; j < BufDyLoader<Cfg>::NCH; ++j) {
      const int e = threadIdx.x + Cfg::NT * j, k = e / (Cfg::BM / 4), c4 = e % (Cfg::BM / 4);
      la.krow[j] = k; la.voff[j] = c4 * 4 < cva ? (unsigned)(k * a.ldy + c4 * 4) * 4u : FS_OOB;
    }
    BufShiftedXLoader<Cfg> lb;
    lb.base = uni_ptr(sc.p + ci0 + (mb + dyy * a.W + dxx) * sc.ld); lb.ld4 = uni((unsigned)sc.ld * 4u); lb.mask = pixmask;
    const int cvb = cleft < Cfg::BN ? cleft : Cfg::BN;
#pragma unroll
    for (int j = 0; j < BufShiftedXLoader<Cfg>::NCH; ++j) {
      const int e = threadIdx.x + Cfg::NT * j, k = e / (Cfg::BN / 4), c4 = e % (Cfg::BN / 4);
      lb.krow[j] = k; lb.voff[j] = c4 * 4 < cvb ? (unsigned)(k * sc.ld + c4 * 4) * 4u : FS_OOB;
    }
    if (want_bias) split_mainloop_tn<Cfg, BufDyLoader<Cfg>, BufShiftedXLoader<Cfg>, true>(lds, KT, la, lb, acc, colsum);
    else split_mainloop_tn<Cfg>(lds, KT, la, lb, acc);
  } else {
  SplitDyLoader<Cfg> la{dyp + co0, a.ldy, coleft < Cfg::BM ? coleft : Cfg::BM, mb, me};
  SplitShiftedXLoader<Cfg> lb{sc.p + ci0, sc.ld, cleft < Cfg::BN ? cleft : Cfg::BN, dyy, dxx, a.H, a.W, HW, mb, me};
  if (want_bias) split_mainloop_tn<Cfg, SplitDyLoader<Cfg>, SplitShiftedXLoader<Cfg>, true>(lds, KT, la, lb, acc, colsum);
  else split_mainloop_tn<Cfg>(lds, KT, la, lb, acc);
  }
  if (want_bias) {
    // this thread's columns are co0 + 4*(tid % 32) .. +3; NT/32 threads (tid / 32) share them
    float* part = reinterpret_cast<float*>(lds);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) part[(threadIdx.x >> 5) * Cfg::BM + 4 * (threadIdx.x & 31) + q] = colsum[q];
    __syncthreads();
    if (threadIdx.x < Cfg::BM) {
      float s = 0.f;
#pragma unroll
      for (int g = 0; g < Cfg::NT / 32; ++g) s += part[g * Cfg::BM + threadIdx.x];
      if (co0 + threadIdx.x < a.Cout) atomicAdd(a.dbias + co0 + threadIdx.x, s);
    }
  }
#pragma unroll
  for (int nt = 0; nt < Cfg::TN; ++nt) {
    const int n = acc_col<Cfg>(nt);
    if (ci0 + n >= cpad) continue;
#pragma unroll
    for (int mt = 0; mt < Cfg::TM; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = co0 + acc_row<Cfg>(mt, r);
        if (co < a.Cout) atomicAdd(a.dwpk + (int64_t)co * a.Ktot + kofs + n, acc[mt][nt][r]);
      }
  }
}

// ---- few-channel layers (encoder residual stages, C = 32 / 64 / 96) -----------------------------------------------
// A 128-column x tile holding one tap of a 64-channel source is half empty, and so is a 128-row dY tile of a 64-channel
// output: the kernel above then spends 4x the useful MFMA work.  Here the x tile packs TP = BN / cpad CONSECUTIVE taps
// side by side (the packed-K layout is tap-major, so the tile's columns are one contiguous run of dW columns) and the
// dY tile is 64 wide.  A lane's chunk belongs to one tap for the whole k-loop: the tap's pixel shift is folded into its
// fixed buffer offset and its "neighbour inside the image" bit comes from that tap's own pixel mask.
constexpr int WGRAD_PACK_WORDS = 256;      // pixel-mask words per tap slot (pixel split <= 32 * 254)
constexpr int WGRAD_PACK_SLOTS = 8;

template <class Cfg>
struct BufPackedXLoader {
  static constexpr int NCH = Cfg::NCH_B, NREG = NCH * 4;
  const float* base; unsigned ld4; const unsigned* mask;       // mask[word * SLOTS + slot]
  unsigned voff[NCH]; int krow[NCH]; int slot[NCH];
  __device__ __forceinline__ void fetch_tile(int kt, float (&r)[NREG]) const {
    const int ku = __builtin_amdgcn_readfirstlane(kt);
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(base, 0x7fffffffu);
    const unsigned soff = (unsigned)ku * 32u * ld4;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      const unsigned w = mask[ku * WGRAD_PACK_SLOTS + slot[j]];
      const unsigned voffj = voff[j] | ((__builtin_amdgcn_ubfe(w, (unsigned)krow[j], 1u) ^ 1u) << 31);
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, voffj, soff, 0);
      const f32x4 f = __builtin_bit_cast(f32x4, v);
      r[4 * j + 0] = f[0]; r[4 * j + 1] = f[1]; r[4 * j + 2] = f[2]; r[4 * j + 3] = f[3];
    }
  }
};

// grid: x = tap group, y = 64-row Cout tile, z = pixel split.  Single source, split-bf16 arithmetic.
template <class Cfg>
__global__ __launch_bounds__(Cfg::NT) void conv_wgrad_pack_kernel(const WgradArgs a) {
  __shared__ __attribute__((aligned(16))) char lds[Cfg::LDS_BYTES];
  __shared__ unsigned pixmask[WGRAD_PACK_WORDS * WGRAD_PACK_SLOTS];
  const int HW = a.H * a.W;
  const int64_t M = (int64_t)a.B * HW;
  const int taps = a.KH * a.KW;
  const Src sc = a.src[0];
  const int cpad = ((sc.C + 31) / 32) * 32;
  int TP = Cfg::BN / cpad;
  if (TP > WGRAD_PACK_SLOTS) TP = WGRAD_PACK_SLOTS;
  int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  if (a.xcd_xt > 0) {          // tap groups of one (Cout tile, pixel split) on one XCD: they read the same dY and x rows
    const int span = 8 * a.xcd_xt, r = blockIdx.x / span, rem = blockIdx.x - r * span;
    const int g = r * 8 + (rem & 7);
    if (g >= a.xcd_groups) return;
    bx = rem >> 3; by = g % a.xcd_yt; bz = g / a.xcd_yt;
  }
  const int tap0 = bx * TP;
  const int ntap = taps - tap0 < TP ? taps - tap0 : TP;
  const int kofs = tap0 * cpad;
  const int co0 = by * Cfg::BM;
  const int64_t mb = (int64_t)bz * a.kchunk;
  const int64_t me = mb + a.kchunk < M ? mb + a.kchunk : M;
  if (mb >= M) return;
  const int coleft = ((a.Cout + 3) / 4) * 4 - co0;
  const int cva = coleft < Cfg::BM ? coleft : Cfg::BM;
  const int cvb = ((sc.C + 3) / 4) * 4;
  const int KT = (int)((me - mb + 31) / 32);
  f32x16 acc[Cfg::TM][Cfg::TN];
#pragma unroll
  for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
    for (int j = 0; j < Cfg::TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  float colsum[4] = {0.f, 0.f, 0.f, 0.f};
  const bool want_bias = a.dbias != nullptr && bx == 0;
  // pixel masks, one per tap slot: bit k of word w <=> pixel mb + 32 w + k exists and its shifted neighbour is inside the image
  for (int i = threadIdx.x; i < KT * 32; i += Cfg::NT) {
    const int64_t m = mb + i;
    const int pix = (int)(m % HW), py = pix / a.W, px = pix % a.W;
    for (int tp = 0; tp < ntap; ++tp) {
      const int tap = tap0 + tp;
      const int yy = py + tap / a.KW - a.KH / 2, xx = px + tap % a.KW - a.KW / 2;
      const bool ok = m < me && (unsigned)yy < (unsigned)a.H && (unsigned)xx < (unsigned)a.W;
      const unsigned long long bal = __ballot(ok);
      if ((threadIdx.x & 63) == 0) {
        pixmask[(i >> 5) * WGRAD_PACK_SLOTS + tp] = (unsigned)bal;
        pixmask[((i >> 5) + 1) * WGRAD_PACK_SLOTS + tp] = (unsigned)(bal >> 32);
      }
    }
  }
  __syncthreads();
  BufDyLoader<Cfg> la;
  la.base = uni_ptr(a.dy + co0 + mb * a.ldy); la.ld4 = uni((unsigned)a.ldy * 4u); la.npix = (int)(me - mb);
#pragma unroll
  for (int j = 0; j < BufDyLoader<Cfg>::NCH; ++j) {
    const int e = threadIdx.x + Cfg::NT * j, k = e / (Cfg::BM / 4), c4 = e % (Cfg::BM / 4);
    la.krow[j] = k; la.voff[j] = c4 * 4 < cva ? (unsigned)(k * a.ldy + c4 * 4) * 4u : FS_OOB;
  }
  // taps ascend in (dy, dx), so the group's first tap has the smallest pixel shift: every lane offset is >= 0
  const int shift0 = (tap0 / a.KW - a.KH / 2) * a.W + (tap0 % a.KW - a.KW / 2);
  BufPackedXLoader<Cfg> lb;
  lb.base = uni_ptr(sc.p + (mb + shift0) * sc.ld); lb.ld4 = uni((unsigned)sc.ld * 4u); lb.mask = pixmask;
#pragma unroll
  for (int j = 0; j < BufPackedXLoader<Cfg>::NCH; ++j) {
    const int e = threadIdx.x + Cfg::NT * j, k = e / (Cfg::BN / 4), col = (e % (Cfg::BN / 4)) * 4;
    const int tp = col / cpad, cc = col - tp * cpad, tap = tap0 + tp;
    const int shift = (tap / a.KW - a.KH / 2) * a.W + (tap % a.KW - a.KW / 2) - shift0;
    const bool valid = tp < ntap && cc < cvb;
    lb.krow[j] = k; lb.slot[j] = valid ? tp : 0;
    lb.voff[j] = valid ? (unsigned)((k + shift) * sc.ld + cc) * 4u : FS_OOB;
  }
  if (want_bias) split_mainloop_tn<Cfg, BufDyLoader<Cfg>, BufPackedXLoader<Cfg>, true>(lds, KT, la, lb, acc, colsum);
  else split_mainloop_tn<Cfg>(lds, KT, la, lb, acc);
  if (want_bias) {
    // this thread's dY columns are co0 + 4*(tid % (BM/4)) .. +3; NT / (BM/4) threads share them
    constexpr int Q = Cfg::BM / 4, G = Cfg::NT / Q;
    float* part = reinterpret_cast<float*>(lds);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) part[(threadIdx.x / Q) * Cfg::BM + 4 * (threadIdx.x % Q) + q] = colsum[q];
    __syncthreads();
    if (threadIdx.x < Cfg::BM) {
      float s = 0.f;
#pragma unroll
      for (int g = 0; g < G; ++g) s += part[g * Cfg::BM + threadIdx.x];
      if (co0 + threadIdx.x < a.Cout) atomicAdd(a.dbias + co0 + threadIdx.x, s);
    }
  }
#pragma unroll
  for (int nt = 0; nt < Cfg::TN; ++nt) {
    const int n = acc_col<Cfg>(nt);
    if (n >= ntap * cpad) continue;
#pragma unroll
    for (int mt = 0; mt < Cfg::TM; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = co0 + acc_row<Cfg>(mt, r);
        if (co < a.Cout) atomicAdd(a.dwpk + (int64_t)co * a.Ktot + kofs + n, acc[mt][nt][r]);
      }
  }
}

// grid: x = packed-K tile (source, tap, 128-channel tile), y = Cout tile, z = pixel split
template <class Cfg>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(WgradArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[Cfg::LDS_FLOATS];
  const int HW = a.H * a.W;
  const int64_t M = (int64_t)a.B * HW;
  const int taps = a.KH * a.KW;
  // decode blockIdx.x -> (source, tap, channel tile)
  int t = blockIdx.x, s = 0, kofs = 0;
  for (;; ++s) {
    const int ct = (a.src[s].C + Cfg::BN - 1) / Cfg::BN;
    if (t < taps * ct) break;
    t -= taps * ct;
    kofs += taps * ((a.src[s].C + 31) / 32) * 32;
  }
  const Src sc = s == 0 ? a.src[0] : s == 1 ? a.src[1] : a.src[2];
  const int ct = (sc.C + Cfg::BN - 1) / Cfg::BN;
  const int tap = t / ct, ci0 = (t % ct) * Cfg::BN;
  const int cpad = ((sc.C + 31) / 32) * 32;
  kofs += tap * cpad + ci0;
  const int co0 = blockIdx.y * Cfg::BM;
  const int64_t mb = (int64_t)blockIdx.z * a.kchunk;
  const int64_t me = mb + a.kchunk < M ? mb + a.kchunk : M;
  if (mb >= M) return;

  const int coleft = ((a.Cout + 3) / 4) * 4 - co0;     // dy may be a channel slice of a wider buffer: never read past it
  DyLoader<Cfg> la{a.dy + co0, a.ldy, coleft < Cfg::BM ? coleft : Cfg::BM, mb, me};
  const int cleft = ((sc.C + 3) / 4) * 4 - ci0;
  ShiftedXLoader<Cfg> lb{sc.p + ci0, sc.ld, cleft < Cfg::BN ? cleft : Cfg::BN,
                         tap / a.KW - a.KH / 2, tap % a.KW - a.KW / 2, a.H, a.W, HW, M, mb, me};

  f32x16 acc[Cfg::TM][Cfg::TN];
#pragma unroll
  for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
    for (int j = 0; j < Cfg::TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  gemm_mainloop<Cfg>(lds, (int)((me - mb + Cfg::BK - 1) / Cfg::BK), la, lb, acc);

#pragma unroll
  for (int nt = 0; nt < Cfg::TN; ++nt) {
    const int n = acc_col<Cfg>(nt);
    if (ci0 + n >= cpad) continue;
#pragma unroll
    for (int mt = 0; mt < Cfg::TM; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = co0 + acc_row<Cfg>(mt, r);
        if (co < a.Cout) atomicAdd(a.dwpk + (int64_t)co * a.Ktot + kofs + n, acc[mt][nt][r]);
      }
  }
}

}  // namespace

#include "wgrad_patch.inc"

// dwpk[Cout][Ktot] += dY^T * im2col(X)   (same packed layout as the forward weights)
extern "C" int fsraft_conv_wgrad(const float* dy, int ldy, int Cout, const float* const* src, const int* srcC,
                                 const int* srcld, int nsrc, float* dwpk, float* dbias, int B, int H, int W, int KH,
                                 int KW, hipStream_t stream) {
  if (!dy || !src || !dwpk || nsrc < 1 || nsrc > 3 || ldy % 4 != 0) return FS_ERR_ARG;
  t_route[1] = 0;
  WgradArgs a{};
  a.dy = dy; a.ldy = ldy; a.Cout = Cout;
  const bool small_m = Cout <= 32;
  const bool t64 = !small_m && knob.wgrad_tile == 3;
  const int bn = t64 ? 64 : 128, bm = small_m ? 32 : (t64 ? 64 : 128);
  if (!fill_srcs(a.src, src, srcC, srcld, nsrc)) return FS_ERR_ARG;
  int xt128 = 0;
  for (int s = 0; s < nsrc; ++s) xt128 += KH * KW * ceil_div(srcC[s], bn);
  a.nsrc = nsrc; a.dwpk = dwpk; a.Ktot = conv_ktot(srcC, nsrc, KH * KW);
  a.B = B; a.H = H; a.W = W; a.KH = KH; a.KW = KW;
  const int64_t M = (int64_t)B * H * W;
  // one segment of a 3x3 layer at encoder size: the resident-block kernel (wgrad_patch.inc) reads dY and X once instead of once
  // per tap group
  if (knob.wgrad_patch && knob.wgrad_patch1 && knob.wgrad_split != 0 && KH == 3 && KW == 3 && Cout > 32 && M >= knob.wgrad_patch1) {
    WgradArgsM m{};
    m.a = a; m.a.dbias = dbias;
    m.nseg = 1;
    m.dys[0] = dy;
    for (int s = 0; s < nsrc; ++s) m.srcs[s][0] = src[s];
    const int rc = launch_wgrad_patch(m, stream);
    if (rc >= 0) return rc;
  }
  if (knob.wgrad_pack && knob.wgrad_split != 0 && knob.wgrad_buf && nsrc == 1 && srcC[0] <= 96 && KH * KW > 1 &&
      (int64_t)(32 * (WGRAD_PACK_WORDS - 2) + 2 * W + 2) * srcld[0] * 4 < 0x7fffffff) {
    // few input channels: several taps per x tile, 64-row dY tiles (conv_wgrad_pack_kernel)
    const int cpad = ceil_div(srcC[0], 32) * 32;
    int tp = SWCfgPack::BN / cpad;
    if (tp > WGRAD_PACK_SLOTS) tp = WGRAD_PACK_SLOTS;
    const int xt = ceil_div(KH * KW, tp), yt = ceil_div(Cout, SWCfgPack::BM);
    const int64_t chunk = wgrad_chunk(knob.wgrad_blocks_pack, (int64_t)xt * yt, M, WGRAD_PACK_WORDS);
    a.kchunk = (int)chunk;
    a.dbias = dbias;
    dim3 grid(xt, yt, (unsigned)((M + chunk - 1) / chunk));
    if (knob.wgrad_xcd == 2) {      // measured slower here (64 -> 64 at 8x220x512: 406 vs 377 us): three tap groups per dY tile only
      a.xcd_xt = xt; a.xcd_yt = yt; a.xcd_groups = yt * (int)grid.z;
      grid = dim3((unsigned)(ceil_div(a.xcd_groups, 8) * 8 * xt), 1, 1);
    }
    t_route[1] = 6;
    hipLaunchKernelGGL((conv_wgrad_pack_kernel<SWCfgPack>), grid, dim3(SWCfgPack::NT), 0, stream, a);
    return fs_launch_status();
  }
  const int ytiles = ceil_div(Cout, bm);
  // aim for ~4 workgroups per CU; each split handles a multiple of 32 pixels, at least 256
  const int64_t chunk = wgrad_chunk(knob.wgrad_blocks, (int64_t)xt128 * ytiles, M, WGRAD_MASK_WORDS);   // (pixel-mask capacity of the buffer-addressed kernel)
  a.kchunk = (int)chunk;
  const int zs = (int)((M + chunk - 1) / chunk);
  dim3 grid(xt128, ytiles, zs);
  a.dbias = dbias;
  const bool wbuf = knob.wgrad_buf && chunk <= 32 * (WGRAD_MASK_WORDS - 2) && (int64_t)chunk * 4 * 2048 < 0x7fffffff;
  if (!small_m && !t64 && knob.wgrad_split == 1) {
    t_route[1] = 4;
    if (wbuf) hipLaunchKernelGGL((conv_wgrad_split_kernel<SWCfg128, true>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((conv_wgrad_split_kernel<SWCfg128>), grid, dim3(256), 0, stream, a);
    return fs_launch_status();
  }
  if (!small_m && !t64 && knob.wgrad_split == 2) {
    t_route[1] = 5;
    if (wbuf) hipLaunchKernelGGL((conv_wgrad_split_kernel<SWCfg128S, true>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((conv_wgrad_split_kernel<SWCfg128S>), grid, dim3(256), 0, stream, a);
    return fs_launch_status();
  }
  // the exact-fp32 kernels do not fuse the bias gradient: separate column-sum pass
  if (dbias) { const int rc = fsraft_col_sum(dy, ldy, M, Cout, dbias, 1.0f, stream); if (rc) return rc; }
  t_route[1] = small_m ? 1 : t64 ? 2 : 3;
  if (small_m) hipLaunchKernelGGL((conv_wgrad_kernel<WCfg32>), grid, dim3(256), 0, stream, a);
  else if (t64) hipLaunchKernelGGL((conv_wgrad_kernel<WCfg6464>), grid, dim3(256), 0, stream, a);
  else hipLaunchKernelGGL((conv_wgrad_kernel<WCfg128>), grid, dim3(256), 0, stream, a);
  return fs_launch_status();
}

// nseg (dY, X) pairs of identical shape in one launch; src[seg * nsrc + s].  Falls back to one launch per segment when
// the buffer-addressed split kernel cannot take the shape.
extern "C" int fsraft_conv_wgrad_multi(const float* const* dy, int nseg, int ldy, int Cout, const float* const* src,
                                       const int* srcC, const int* srcld, int nsrc, float* dwpk, float* dbias, int B,
                                       int H, int W, int KH, int KW, hipStream_t stream) {
  if (!dy || !src || !dwpk || nseg < 1 || nsrc < 1 || nsrc > 3 || ldy % 4 != 0) return FS_ERR_ARG;
  t_route[1] = 0;
  const int64_t M = (int64_t)B * H * W;
  const bool fast = knob.wgrad_multi && nseg > 1 && Cout > 32 && knob.wgrad_tile != 3 && knob.wgrad_split == 2 && knob.wgrad_buf;
  for (int base = 0; base < nseg; base += WGRAD_MAX_SEG) {
    const int n = nseg - base < WGRAD_MAX_SEG ? nseg - base : WGRAD_MAX_SEG;
    if (!fast || n == 1) {
      for (int i = 0; i < n; ++i) {
        const int rc = fsraft_conv_wgrad(dy[base + i], ldy, Cout, src + (size_t)(base + i) * nsrc, srcC, srcld, nsrc, dwpk,
                                         dbias, B, H, W, KH, KW, stream);
        if (rc) return rc;
      }
      continue;
    }
    WgradArgsM m{};
    WgradArgs& a = m.a;
    a.dy = dy[base]; a.ldy = ldy; a.Cout = Cout;
    if (!fill_srcs(a.src, src + (size_t)base * nsrc, srcC, srcld, nsrc)) return FS_ERR_ARG;
    int xt128 = 0;
    for (int s = 0; s < nsrc; ++s) xt128 += KH * KW * ceil_div(srcC[s], 128);
    for (int i = 0; i < n; ++i) {
      if (!dy[base + i]) return FS_ERR_ARG;
      m.dys[i] = dy[base + i];
      for (int s = 0; s < nsrc; ++s) {
        if (!src[(size_t)(base + i) * nsrc + s]) return FS_ERR_ARG;
        m.srcs[s][i] = src[(size_t)(base + i) * nsrc + s];
      }
    }
    a.nsrc = nsrc; a.dwpk = dwpk; a.Ktot = conv_ktot(srcC, nsrc, KH * KW);
    a.B = B; a.H = H; a.W = W; a.KH = KH; a.KW = KW; a.dbias = dbias;
    if (knob.wgrad_patch && KH * KW > 1) {
      m.nseg = n;
      const int rc = launch_wgrad_patch(m, stream);
      if (rc == 0) continue;
      if (rc > 0) return rc;
    }
    const int ytiles = ceil_div(Cout, 128);
    // ~knob.wgrad_blocks workgroups in total, a whole number of pixel splits per segment
    const int64_t chunk = wgrad_chunk(knob.wgrad_blocks_multi, (int64_t)xt128 * ytiles * n, M, WGRAD_MASK_WORDS);
    if ((int64_t)chunk * 4 * 2048 >= 0x7fffffff) return FS_ERR_ARG;
    a.kchunk = (int)chunk;
    m.zs = (int)((M + chunk - 1) / chunk);
    m.nseg = n;
    dim3 grid(xt128, ytiles, m.zs * n);
    if (knob.wgrad_xcd == 3) {        // all tiles of one pixel split on one XCD (xcd_yt < 0 carries -x tiles)
      m.a.xcd_xt = xt128 * ytiles; m.a.xcd_yt = -xt128; m.a.xcd_groups = m.zs * n;
      grid = dim3((unsigned)(ceil_div(m.a.xcd_groups, 8) * 8 * xt128 * ytiles), 1, 1);
    } else if (knob.wgrad_xcd) {
      m.a.xcd_xt = xt128; m.a.xcd_yt = ytiles; m.a.xcd_groups = ytiles * m.zs * n;
      grid = dim3((unsigned)(ceil_div(m.a.xcd_groups, 8) * 8 * xt128), 1, 1);
    }
    t_route[1] = knob.wgrad_w8 ? 9 : 8;
    if (knob.wgrad_w8) hipLaunchKernelGGL((conv_wgrad_split_kernel<SWCfg128W8, true, true>), grid, dim3(512), 0, stream, m);
    else hipLaunchKernelGGL((conv_wgrad_split_kernel<SWCfg128S, true, true>), grid, dim3(256), 0, stream, m);
    const int rc = fs_launch_status();
    if (rc) return rc;
  }
  return FS_OK;
}
