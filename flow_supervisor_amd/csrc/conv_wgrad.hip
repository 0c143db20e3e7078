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
  // A layer split over several launches (wide tiles + the 128 tile for what is left, disjoint regions of dwpk): this launch's
  // first x tile and first Cout tile, in units of its own tile.
  int bx0, by0;
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


// 256-column x tile (Cfg::BN == 256, 512 threads): waves 0..3 load columns 0..127, waves 4..7 columns 128..255.  The halves are
// two consecutive 128-column groups of the packed-K layout -- two taps of one source, or the last tap of one source and the first
// of the next -- so each half has its own base pointer, pitch, pixel shift and pixel mask, all wave-uniform, and a lane's chunks
// stay in one half for the whole k-loop.  Chunk j of a lane: pixel (t / 32) + 8 j, channels 4 (t % 32) .. +3, t = tid % 256.
constexpr int WGRAD_WIDE_WORDS = 512;      // pixel-mask words per half (pixel split <= 32 * 510)
template <class Cfg>
struct BufWideXLoader : BufShiftedXLoader<Cfg> {
  int e0;                                  // tile element of chunk 0: [pixel][256 columns] in float4 units
  __device__ __forceinline__ int elem(int c) const { return e0 + 8 * (Cfg::BN / 4) * c; }
};

// One 128-column group of the packed-K layout: (source, tap, 128-channel tile); t counts them in layout order.
struct XGroup { int s, tap, ci0, kofs, cpad; };
template <int GW>
__device__ __forceinline__ XGroup wgrad_xgroup(const WgradArgs& a, int t, int taps) {
  int s = 0, kofs = 0;
  for (;; ++s) {
    const int ct = (a.src[s].C + GW - 1) / GW;
    if (t < taps * ct) break;
    t -= taps * ct;
    kofs += taps * ((a.src[s].C + 31) / 32) * 32;
  }
  const int C = s == 0 ? a.src[0].C : s == 1 ? a.src[1].C : a.src[2].C;
  const int ct = (C + GW - 1) / GW, cpad = ((C + 31) / 32) * 32;
  const int tap = t / ct, ci0 = (t % ct) * GW;
  return XGroup{s, tap, ci0, kofs + tap * cpad + ci0, cpad};
}

template <class Cfg, bool BUF = false, bool MULTI = false>
__global__ __launch_bounds__(Cfg::NT) void conv_wgrad_split_kernel(const std::conditional_t<MULTI, WgradArgsM, WgradArgs> args) {
  static_assert(Cfg::NT == 256 || BUF, "512-thread workgroups use the buffer-addressed loaders");
  constexpr bool WIDE = Cfg::BN == 256;
  static_assert(!WIDE || (BUF && Cfg::NT == 512), "the 256-column x tile is loaded by two halves of 256 threads");
  constexpr int GW = WIDE ? 128 : Cfg::BN;
  __shared__ __attribute__((aligned(16))) char lds[Cfg::LDS_BYTES];
  __shared__ unsigned pixmask[BUF ? (WIDE ? 2 * WGRAD_WIDE_WORDS : WGRAD_MASK_WORDS) : 1];
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
  bx += a.bx0; by += a.by0;
  const int HW = a.H * a.W;
  const int64_t M = (int64_t)a.B * HW;
  const int taps = a.KH * a.KW;
  // the group this wave LOADS (xh: its half of a 256-column tile) and the group its accumulator columns belong to (oh)
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int xh = WIDE ? wave >> 2 : 0, oh = WIDE ? ((wave % Cfg::WN) * (Cfg::TN * 32)) >> 7 : 0;
  const XGroup gl = wgrad_xgroup<GW>(a, WIDE ? 2 * bx + xh : bx, taps);
  const XGroup go = WIDE ? wgrad_xgroup<GW>(a, 2 * bx + oh, taps) : gl;
  const int s = gl.s;
  Src sc = s == 0 ? a.src[0] : s == 1 ? a.src[1] : a.src[2];
  const float* dyp = a.dy;
  if constexpr (MULTI) {       // this segment's tensors, read from the kernarg tables with a uniform index
    typedef const float* fptr;
    const auto* karg = (const char __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr();
    dyp = ((const fptr __attribute__((address_space(4)))*)(karg + offsetof(WgradArgsM, dys)))[seg];
    sc.p = ((const fptr __attribute__((address_space(4)))*)(karg + offsetof(WgradArgsM, srcs)))[s * WGRAD_MAX_SEG + seg];
  }
  const int tap = gl.tap, ci0 = gl.ci0;
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
    // (256-column tile: each half of the workgroup builds the mask of its own tap)
    constexpr int MT = WIDE ? 256 : Cfg::NT;
    unsigned* pm = pixmask + xh * WGRAD_WIDE_WORDS;
    for (int i = threadIdx.x % MT; i < KT * 32; i += MT) {
      const int64_t m = mb + i;
      bool ok = m < me;
      if (ok) {
        const int pix = (int)(m % HW), yy = pix / a.W + dyy, xx = pix % a.W + dxx;
        ok = (unsigned)yy < (unsigned)a.H && (unsigned)xx < (unsigned)a.W;
      }
      const unsigned long long bal = __ballot(ok);
      if ((threadIdx.x & 63) == 0) { pm[i >> 5] = (unsigned)bal; pm[(i >> 5) + 1] = (unsigned)(bal >> 32); }
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
    std::conditional_t<WIDE, BufWideXLoader<Cfg>, BufShiftedXLoader<Cfg>> lb;
    lb.base = uni_ptr(sc.p + ci0 + (mb + dyy * a.W + dxx) * sc.ld); lb.ld4 = uni((unsigned)sc.ld * 4u); lb.mask = pm;
    const int cvb = cleft < GW ? cleft : GW;
    if constexpr (WIDE) {
      const int t8 = threadIdx.x & 255, c4 = t8 & 31;
#pragma unroll
      for (int j = 0; j < BufShiftedXLoader<Cfg>::NCH; ++j) {
        const int k = (t8 >> 5) + 8 * j;
        lb.krow[j] = k; lb.voff[j] = c4 * 4 < cvb ? (unsigned)(k * sc.ld + c4 * 4) * 4u : FS_OOB;
      }
      lb.e0 = (t8 >> 5) * (Cfg::BN / 4) + xh * 32 + c4;
    } else {
#pragma unroll
      for (int j = 0; j < BufShiftedXLoader<Cfg>::NCH; ++j) {
        const int e = threadIdx.x + Cfg::NT * j, k = e / (Cfg::BN / 4), c4 = e % (Cfg::BN / 4);
        lb.krow[j] = k; lb.voff[j] = c4 * 4 < cvb ? (unsigned)(k * sc.ld + c4 * 4) * 4u : FS_OOB;
      }
    }
    if (want_bias) split_mainloop_tn<Cfg, BufDyLoader<Cfg>, decltype(lb), true, WIDE>(lds, KT, la, lb, acc, colsum);
    else split_mainloop_tn<Cfg, BufDyLoader<Cfg>, decltype(lb), false, WIDE>(lds, KT, la, lb, acc);
  } else {
  SplitDyLoader<Cfg> la{dyp + co0, a.ldy, coleft < Cfg::BM ? coleft : Cfg::BM, mb, me};
  SplitShiftedXLoader<Cfg> lb{sc.p + ci0, sc.ld, cleft < Cfg::BN ? cleft : Cfg::BN, dyy, dxx, a.H, a.W, HW, mb, me};
  if (want_bias) split_mainloop_tn<Cfg, SplitDyLoader<Cfg>, SplitShiftedXLoader<Cfg>, true>(lds, KT, la, lb, acc, colsum);
  else split_mainloop_tn<Cfg>(lds, KT, la, lb, acc);
  }
  if (want_bias) {
    // this thread's columns are co0 + 4*(tid % (BM/4)) .. +3; NT / (BM/4) threads share them
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
  // (256-column tile: a wave's accumulator columns lie in one half, whose packed-K run starts at go.kofs)
#pragma unroll
  for (int nt = 0; nt < Cfg::TN; ++nt) {
    const int n = acc_col<Cfg>(nt) & (GW - 1);
    if (go.ci0 + n >= go.cpad) continue;
#pragma unroll
    for (int mt = 0; mt < Cfg::TM; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = co0 + acc_row<Cfg>(mt, r);
        if (co < a.Cout) atomicAdd(a.dwpk + (int64_t)co * a.Ktot + go.kofs + n, acc[mt][nt][r]);
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

namespace {
int g_wgrad_wide = 1;                      // fsraft_set_wgrad_wide: 0 off, 1 by shape, 2 wherever the shape allows
__thread int t_wgrad_tile = 0;             // fsraft_conv_wgrad_last_tile

// ---- wide per-tap tiles ------------------------------------------------------------------------------------------------
// The packed-K axis is a run of 128-column groups (source, tap, 128-channel tile).  The wide launch takes them in pairs, and
// Cout in blocks of 256 (Cout >= 256) or 128; what is left -- an odd last group, Cout beyond the last full 256 -- goes to the
// 128x128 tile in one or two more launches into disjoint regions of dwpk.  No wide tile is ever partly empty in a whole half.
struct WidePlan {
  int bm;              // 256 or 128 rows of dY per wide tile; 0: no wide launch
  int pairs, groups;   // pairs of column groups on the wide tile; all column groups
  int yw;              // Cout tiles of the wide launch
  int64_t chunk;       // pixels per split of the wide launch
};

// chunk128: the pixel split the 128 tile would use (it bounds the wide tile's number of splits from above, so the bytes added
// to dwpk by atomics never grow); nseg: segments of the launch.
WidePlan wide_plan(int Cout, const int* srcC, int nsrc, int taps, int64_t M, int nseg, int64_t chunk128) {
  WidePlan p{};
  if (g_wgrad_wide == 0 || Cout <= 32) return p;
  for (int s = 0; s < nsrc; ++s) p.groups += taps * ceil_div(srcC[s], 128);
  p.pairs = p.groups / 2;
  if (p.pairs == 0) return p;
  const int bm = Cout >= 256 ? 256 : 128;
  const int yw = bm == 256 ? Cout / 256 : ceil_div(Cout, 128);
  // One workgroup per CU: at most 512 workgroups, never more splits than the 128 tile has, and whole rounds of 256 -- a grid
  // of 258 workgroups takes as long as one of 512 (2x2 384->128 at 8x55x128: 139 us on 43 splits of 6 tiles).
  const int64_t tiles = (int64_t)p.pairs * yw * nseg, s128 = (M + chunk128 - 1) / chunk128;
  int64_t want = 512 / tiles;
  if (want > s128) want = s128;
  if (tiles * want > 256) want = 256 * (tiles * want / 256) / tiles;
  if (want < 1) want = 1;
  int64_t chunk = (M + want - 1) / want;
  if (chunk < 256) chunk = 256;
  chunk = (chunk + 31) / 32 * 32;
  if (chunk > 32 * (WGRAD_WIDE_WORDS - 2) || chunk * 4 * 2048 >= 0x7fffffff) return p;
  if (g_wgrad_wide == 1) {
    // By shape: a grid that leaves a quarter of the CUs idle loses to the 128 tile's 512+ workgroups.  These classes stay on the
    // 128 tile (us per launch, 128 tile vs wide): 1x1 256->576 at 48x55x128 491 vs 748 (104 workgroups), 1x1 324->256 323 vs 491
    // (52), single-segment 1x5 128->256 / 5x1 128->128 at 4x55x128 67 vs 93 / 48 vs 66 (104).  More splits would fill the grid but
    // add more bytes to dwpk by atomics than the 128 tile does.  Nor does a workgroup with fewer than 16 k-tiles pay for its
    // prologue and the atomics of a 128 - 256 KB tile: single-segment 1x5 / 5x1 128->128 at 4x55x128 (196 workgroups of 9
    // k-tiles) 47 vs 66; 2x2 384->128 at 4x55x128 (21 k-tiles) still wins, 66 vs 63.
    if (tiles * ((M + chunk - 1) / chunk) < 192 || chunk < 512) return p;
  }
  p.bm = bm; p.yw = yw; p.chunk = chunk;
  return p;
}

// One launch of the per-tap kernel on tile `Cfg`: x tiles [bx0, bx0 + xt), Cout tiles [by0, by0 + yt), zs splits of `chunk` pixels
// per segment.  xcd: the XCD-aware 1-D order of the multi-segment launches.
template <class Cfg, bool MULTI, class A>
int launch_split(A m, int xt, int yt, int zs, int nseg, int bx0, int by0, int64_t chunk, int xcd, hipStream_t stream) {
  WgradArgs& a = [&]() -> WgradArgs& { if constexpr (MULTI) return m.a; else return m; }();
  a.kchunk = (int)chunk; a.bx0 = bx0; a.by0 = by0;
  a.xcd_xt = a.xcd_yt = a.xcd_groups = 0;
  if constexpr (MULTI) { m.zs = zs; m.nseg = nseg; }
  dim3 grid(xt, yt, zs * nseg);
  if (xcd == 3) {        // all tiles of one pixel split on one XCD (xcd_yt < 0 carries -x tiles)
    a.xcd_xt = xt * yt; a.xcd_yt = -xt; a.xcd_groups = zs * nseg;
    grid = dim3((unsigned)(ceil_div(a.xcd_groups, 8) * 8 * xt * yt), 1, 1);
  } else if (xcd) {
    a.xcd_xt = xt; a.xcd_yt = yt; a.xcd_groups = yt * zs * nseg;
    grid = dim3((unsigned)(ceil_div(a.xcd_groups, 8) * 8 * xt), 1, 1);
  }
  hipLaunchKernelGGL((conv_wgrad_split_kernel<Cfg, true, MULTI>), grid, dim3(Cfg::NT), 0, stream, m);
  return fs_launch_status();
}

// The wide launch and the 128-tile launches for what it leaves.  chunk128: the 128 tile's pixel split.
template <bool MULTI, class A>
int launch_wide(const A& m, const WidePlan& p, int Cout, int64_t M, int nseg, int64_t chunk128, int xcd, hipStream_t stream) {
  const int zsw = (int)((M + p.chunk - 1) / p.chunk), zs = (int)((M + chunk128 - 1) / chunk128);
  int rc = p.bm == 256 ? launch_split<SWCfgW256, MULTI>(m, p.pairs, p.yw, zsw, nseg, 0, 0, p.chunk, xcd, stream)
                       : launch_split<SWCfgW128, MULTI>(m, p.pairs, p.yw, zsw, nseg, 0, 0, p.chunk, xcd, stream);
  if (rc) return rc;
  const int y128 = ceil_div(Cout, 128), ydone = p.bm == 256 ? 2 * p.yw : p.yw;
  // Cout beyond the wide rows: every column group (its x tile 0 owns the bias gradient of these rows)
  if (ydone < y128) rc = launch_split<SWCfg128S, MULTI>(m, p.groups, y128 - ydone, zs, nseg, 0, ydone, chunk128, xcd, stream);
  if (rc) return rc;
  // an odd last column group under the wide rows
  if (p.groups & 1) rc = launch_split<SWCfg128S, MULTI>(m, 1, ydone, zs, nseg, p.groups - 1, 0, chunk128, xcd, stream);
  t_wgrad_tile = p.bm << 16 | 256;
  return rc;
}
}  // namespace

extern "C" int fsraft_set_wgrad_wide(int mode) {
  if (mode < 0 || mode > 2) return FS_ERR_ARG;
  g_wgrad_wide = mode;
  return FS_OK;
}
extern "C" int fsraft_conv_wgrad_last_tile(void) { return t_wgrad_tile; }

// dwpk[Cout][Ktot] += dY^T * im2col(X)   (same packed layout as the forward weights)
extern "C" int fsraft_conv_wgrad(const float* dy, int ldy, int Cout, const float* const* src, const int* srcC,
                                 const int* srcld, int nsrc, float* dwpk, float* dbias, int B, int H, int W, int KH,
                                 int KW, hipStream_t stream) {
  if (!dy || !src || !dwpk || nsrc < 1 || nsrc > 3 || ldy % 4 != 0) return FS_ERR_ARG;
  t_route[1] = 0; t_wgrad_tile = 0;
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
    t_route[1] = 6; t_wgrad_tile = SWCfgPack::BM << 16 | SWCfgPack::BN;
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
    t_route[1] = 4; t_wgrad_tile = 128 << 16 | 128;
    if (wbuf) hipLaunchKernelGGL((conv_wgrad_split_kernel<SWCfg128, true>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((conv_wgrad_split_kernel<SWCfg128>), grid, dim3(256), 0, stream, a);
    return fs_launch_status();
  }
  if (!small_m && !t64 && knob.wgrad_split == 2) {
    t_route[1] = 5;
    t_wgrad_tile = 128 << 16 | 128;
    if (wbuf) {
      const WidePlan p = wide_plan(Cout, srcC, nsrc, KH * KW, M, 1, chunk);
      if (p.bm) return launch_wide<false>(a, p, Cout, M, 1, chunk, 0, stream);
    }
    if (wbuf)hipLaunchKernelGGL((conv_wgrad_split_kernel<SWCfg128S, true>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((conv_wgrad_split_kernel<SWCfg128S>), grid, dim3(256), 0, stream, a);
    return fs_launch_status();
  }
  // the exact-fp32 kernels do not fuse the bias gradient: separate column-sum pass
  if (dbias) { const int rc = fsraft_col_sum(dy, ldy, M, Cout, dbias, 1.0f, stream); if (rc) return rc; }
  t_route[1] = small_m ? 1 : t64 ? 2 : 3;
  t_wgrad_tile = bm << 16 | bn;
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
  t_route[1] = 0; t_wgrad_tile = 0;
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
    if (!knob.wgrad_w8) {
      const WidePlan p = wide_plan(Cout, srcC, nsrc, KH * KW, M, n, chunk);
      if (p.bm) {
        t_route[1] = 8;
        const int rc = launch_wide<true>(m, p, Cout, M, n, chunk, knob.wgrad_xcd, stream);
        if (rc) return rc;
        continue;
      }
    }
    t_wgrad_tile = 128 << 16 | 128;
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
