// Update-block convolutions as implicit GEMMs on the fp32 MFMA core (rows a6-a8 of
// SURVEY.md section 8; reference: pytorch/core/update.py:6-136, every nn.Conv2d there).
//
// Activations are channels-last: tensor element (pixel m, channel c) at p[m*ld + c], with
// ld % 4 == 0 and any padding channels holding zeros.  A convolution with "same" padding
//   Y[m, co] = act( bias[co] + sum_{src s} sum_{tap t} sum_{ci} X_s[m + off(t), ci] * W[co, coff_s + ci, t] )
// is the GEMM  [M = B*H*W pixels] x [N = Cout] x [K = sum_s taps * ceil32(C_s)]  whose A operand is
// gathered on the fly (zero outside the image) and whose B operand is a pre-packed weight
// matrix Wpk[n][k] (k ordered source-major, then tap, then channel, each channel run zero
// padded to a multiple of 32) produced by fsraft_pack_conv_weight.  Up to three sources
// replace torch.cat on the input side; up to three destination channel ranges replace the
// split on the output side (used by the data-gradient pass, which is this same kernel run
// on flipped/transposed packed weights).
//
// Fused epilogues: bias, ReLU, scale (mask head 0.25), and the two ConvGRU gate stages
//   ZR: z = sigmoid(.), r = sigmoid(.), stores z, r and r*h          (update.py:27-29 / 46-48)
//   Q : q = tanh(.), stores q and h' = (1-z)*h + z*q                 (update.py:29-31 / 48-50)
//
// This file: the forward / data-gradient kernels and their dispatcher.  The weight gradient (the transposed product
// dWpk[co][k] += sum_m dY[m,co] * Xg[m,k]) is conv_wgrad.hip, the weight packers conv_pack.hip, the knobs conv_tuning.hip;
// conv_common.hpp holds what they share.
#include "conv_common.hpp"

namespace {

// Workgroups are dealt to the 8 XCDs round-robin by linear id, and each XCD has its own L2.  With the plain
// (x = N tile, y = M tile) mapping the N tiles of one M tile -- which read the same activation rows -- land on
// different XCDs.  This maps linear id i to logical tile t so that every XCD owns one contiguous run of tiles:
// XCD x holds ids {x, x+8, ...}; its run starts at x*(T/8) + min(x, T%8).
__device__ __forceinline__ void tile_of_block(int swz, int& bx, int& by) {
  if (!swz) return;
  const int nx = gridDim.x, T = nx * gridDim.y, i = by * nx + bx;
  const int x = i & 7, q = T >> 3, r = T & 7;
  const int t = x * q + (x < r ? x : r) + (i >> 3);
  bx = t % nx; by = t / nx;
}

template <class Cfg>
struct ConvALoader {
  static constexpr int BM = Cfg::BM, BK = Cfg::BK, LD = Cfg::LDA;
  static constexpr int F4 = BK / 4;
  static constexpr int NF4 = BM * F4 / 256;
  static constexpr int NREG = NF4 * 4;
  static constexpr int NCH = NF4;
  const float* p0; const float* p1; const float* p2;
  int C0, C1, C2, ld0, ld1, ld2;
  int cpt0, cpt1, cpt2;          // 32-channel chunks per tap for each source
  int taps, KW, PH, PW, H, W;
  int py[NF4], px[NF4];          // pixel coordinates of this thread's rows (py < 0: row outside M)
  int64_t pb[NF4];               // image base pixel index b*H*W
  __device__ __forceinline__ bool fetch_chunk(int kt, float (&r)[NREG], int j) const {
    // source select written as sums of two-way selects: a three-way select chain over kernel
    // arguments is turned by hipcc into a private (scratch) lookup table that is then re-read,
    // with s_waitcnt vmcnt(0), in front of every load of the k-loop
    const int n0 = taps * cpt0, n1 = taps * cpt1;
    const bool is1 = kt >= n0, is2 = kt >= n0 + n1;
    const int k = kt - (is1 ? n0 : 0) - (is2 ? n1 : 0);
    const int C = C0 + (is1 ? C1 - C0 : 0) + (is2 ? C2 - C1 : 0);
    const int ld = ld0 + (is1 ? ld1 - ld0 : 0) + (is2 ? ld2 - ld1 : 0);
    const int cpt = cpt0 + (is1 ? cpt1 - cpt0 : 0) + (is2 ? cpt2 - cpt1 : 0);
    const float* p = p0 + (is1 ? p1 - p0 : 0) + (is2 ? p2 - p1 : 0);
    const int tap = k / cpt, c0 = (k % cpt) * BK;
    const int dy = tap / KW - PH, dx = tap % KW - PW;
    const int kq = (threadIdx.x + 256 * j) % F4;
    const int yy = py[j] + dy, xx = px[j] + dx, c = c0 + kq * 4;
    // unconditional load from a clamped address; the zero-select happens in store_chunk so that
    // nothing consumes the load result here (a use would force s_waitcnt right behind the load)
    const bool ok = py[j] >= 0 && yy >= 0 && yy < H && xx >= 0 && xx < W && c < C;
    const f32x4 v = gload4(p + (ok ? (pb[j] + (int64_t)yy * W + xx) * ld + c : 0));
    r[4 * j + 0] = v[0]; r[4 * j + 1] = v[1]; r[4 * j + 2] = v[2]; r[4 * j + 3] = v[3];
    return ok;
  }
  __device__ __forceinline__ void store_chunk(float* t, const float (&r)[NREG], int j, bool ok) const {
    const int e = threadIdx.x + 256 * j;
    const int row = e / F4, kq = e % F4;
#pragma unroll
    for (int c = 0; c < 4; ++c) t[(kq * 4 + c) * LD + row] = ok ? r[4 * j + c] : 0.f;
  }
};

// ---- loaders of the split-bf16 core ---------------------------------------------------------
template <class Cfg>
struct SplitConvALoader {                 // implicit-GEMM gather of fp32 activations, converted at staging time
  static constexpr int NCH = Cfg::NCH_A, NREG = NCH * 4;
  const float* p0; const float* p1; const float* p2;
  int C0, C1, C2, ld0, ld1, ld2, cpt0, cpt1, cpt2;
  int taps, KW, PH, PW, H, W;
  int py[NCH], px[NCH];                   // pixel coordinates of this thread's rows (py < 0: row outside M)
  int pofs[NCH];                          // pixel index b*H*W + y*W + x of the row
  __device__ __forceinline__ void fetch_chunk(int kt, float (&r)[NREG], int j) const {
    const int n0 = taps * cpt0, n1 = taps * cpt1;
    const bool is1 = kt >= n0, is2 = kt >= n0 + n1;
    const int k = kt - (is1 ? n0 : 0) - (is2 ? n1 : 0);
    const int C = C0 + (is1 ? C1 - C0 : 0) + (is2 ? C2 - C1 : 0);
    const int ld = ld0 + (is1 ? ld1 - ld0 : 0) + (is2 ? ld2 - ld1 : 0);
    const int cpt = cpt0 + (is1 ? cpt1 - cpt0 : 0) + (is2 ? cpt2 - cpt1 : 0);
    const float* p = p0 + (is1 ? p1 - p0 : 0) + (is2 ? p2 - p1 : 0);
    const int tap = k / cpt, c0 = (k % cpt) * 32;
    const int dy = tap / KW - PH, dx = tap % KW - PW;
    const int kq = (threadIdx.x + 256 * j) & 7;
    const int c = c0 + kq * 4;
    const bool ok = ((unsigned)(py[j] + dy) < (unsigned)H) && ((unsigned)(px[j] + dx) < (unsigned)W) && c < C;
    const float* src = ok ? p + (int64_t)(pofs[j] + dy * W + dx) * ld + c : g_fsraft_zero16;
    const f32x4 v = gload4(src);
    r[4 * j + 0] = v[0]; r[4 * j + 1] = v[1]; r[4 * j + 2] = v[2]; r[4 * j + 3] = v[3];
  }
  __device__ __forceinline__ void stage_chunk(char* tile, const float* r4, int j) const {
    stage_convert<Cfg::PITCH>(tile, threadIdx.x + 256 * j, r4);
  }
};

// ---- buffer-addressed variants -----------------------------------------------------------------
// Same tiles, but fetched with buffer_load_dwordx4: the per-lane part of the address is a 32-bit byte offset that
// is constant over the whole k-loop (this thread's pixel row and 16-byte column), the per-k-tile part (tap shift,
// channel chunk, source) is wave-uniform and travels in the SGPR offset, and "outside the image / outside the
// matrix" is expressed by pointing the lane offset past num_records, which makes the hardware return zeros.
// That removes the 64-bit per-lane address arithmetic and the bounds compares (about 15 VALU per 16-byte chunk)
// from the k-loop; what is left per chunk is one mask test and one select.  (FS_OOB, make_rsrc: conv_common.hpp)
template <class Cfg>
struct BufConvALoader {
  static constexpr int NCH = Cfg::NCH_A, NREG = NCH * 4;
  // descriptor bases, biased down by (PH*W + PW) pixels so that tap shifts stay non-negative, and sizes in bytes.
  // (Descriptors are rebuilt from these scalars at each use: a struct holding __amdgpu_buffer_rsrc_t members is not
  // scalarised by the compiler and ends up in scratch, which turns every uniform value read back from it divergent.)
  const float* b0; const float* b1; const float* b2; unsigned nb0, nb1, nb2;
  unsigned ld0x4, ld1x4, ld2x4;           // row pitches in bytes
  const unsigned __attribute__((address_space(4)))* ktab;   // table in the kernarg segment (constant address space -> s_load), see ConvArgsT
  unsigned tapmask[NCH];                  // bit t: tap t of this thread's pixel row lies inside the image (0: row outside M)
  unsigned pofs[NCH];                     // pixel index of the row
  unsigned kq16;                          // byte offset of this thread's 16-byte column inside a 128-byte chunk row
  __device__ __forceinline__ void fetch_tile(int kt, float (&r)[NREG]) const {
    // kt is wave-uniform; saying so explicitly lets the table entry come in with s_load_dword and keeps everything
    // derived from it (descriptor, SGPR offset) in scalar registers -- once per tile, not once per chunk
    const unsigned e = ktab[__builtin_amdgcn_readfirstlane(kt)];
    const unsigned soff = (e & 0xffffu) << 4, tap = (e >> 16) & 15u, src = (e >> 20) & 3u, crem = (e >> 22) & 63u;
    const bool s1 = src >= 1, s2 = src >= 2;
    // (sums of two-way selects: a three-way select chain over kernel arguments becomes a scratch lookup table)
    const unsigned ldb = ld0x4 + (s1 ? ld1x4 - ld0x4 : 0u) + (s2 ? ld2x4 - ld1x4 : 0u);
    const float* bp = b0 + (s1 ? b1 - b0 : 0) + (s2 ? b2 - b1 : 0);
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(bp, 0x7fffffffu);
    const unsigned cok = kq16 < crem * 4u ? 1u : 0u;              // this lane's 16-byte column holds channels of the source
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      // branch-free: lanes whose tap falls outside the image (or whose column is padding) get bit 31 set in their
      // offset, which fails the descriptor's range check and reads as zeros
      const unsigned bad = (__builtin_amdgcn_ubfe(tapmask[j], tap, 1u) & cok) ^ 1u;
      const unsigned voff = (bad << 31) | (__umul24(pofs[j], ldb) + kq16);
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 0);
      const f32x4 f = __builtin_bit_cast(f32x4, v);
      r[4 * j + 0] = f[0]; r[4 * j + 1] = f[1]; r[4 * j + 2] = f[2]; r[4 * j + 3] = f[3];
    }
  }
  __device__ __forceinline__ void stage_chunk(char* tile, const float* r4, int j) const {
    stage_convert<Cfg::PITCH>(tile, threadIdx.x + Cfg::NT * j, r4);
  }
};

template <class Cfg>
struct BufConvALoaderU {                  // uniform form: one base, one pitch, two table dwords per k-tile
  static constexpr int NCH = Cfg::NCH_A, NREG = NCH * 4;
  const float* base;
  const unsigned __attribute__((address_space(4)))* ktab;
  unsigned tapmask[NCH];                  // bit t: tap t of this thread's pixel row lies inside the image (0: row outside M)
  unsigned voff0[NCH];                    // pixel * pitch + 16-byte column, in bytes (constant over the k-loop)
  unsigned kq16;
  __device__ __forceinline__ void fetch_tile(int kt, float (&r)[NREG]) const {
    const int ku = __builtin_amdgcn_readfirstlane(kt);
    const unsigned soff = ktab[2 * ku], e = ktab[2 * ku + 1];
    const unsigned tap = e & 15u, crem4 = (e >> 4) * 4u;
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(base, 0x7fffffffu);
    const unsigned cok = kq16 < crem4 ? 1u : 0u;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      const unsigned bad = (__builtin_amdgcn_ubfe(tapmask[j], tap, 1u) & cok) ^ 1u;
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, (bad << 31) | voff0[j], soff, 0);
      const f32x4 f = __builtin_bit_cast(f32x4, v);
      r[4 * j + 0] = f[0]; r[4 * j + 1] = f[1]; r[4 * j + 2] = f[2]; r[4 * j + 3] = f[3];
    }
  }
  __device__ __forceinline__ void stage_chunk(char* tile, const float* r4, int j) const {
    stage_convert<Cfg::PITCH>(tile, threadIdx.x + Cfg::NT * j, r4);
  }
};

template <class Cfg>
struct BufWeightLoader {                  // pre-split packed weights through one buffer descriptor
  static constexpr int NCH = Cfg::NCH_B, NREG = NCH * 4;
  const char* base; unsigned nbytes;
  unsigned voff[NCH];                     // row * row_bytes + 16 * part, or FS_OOB for rows outside the matrix
  __device__ __forceinline__ void fetch_tile(int kt, float (&r)[NREG]) const {
    const int ku = __builtin_amdgcn_readfirstlane(kt);            // kt < 0: zero tile = a descriptor with no records
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(base, ku < 0 ? 0u : nbytes);
    const unsigned soff = ku < 0 ? 0u : (unsigned)ku * 128u;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, voff[j], soff, 0);
      const f32x4 f = __builtin_bit_cast(f32x4, v);
      r[4 * j + 0] = f[0]; r[4 * j + 1] = f[1]; r[4 * j + 2] = f[2]; r[4 * j + 3] = f[3];
    }
  }
  __device__ __forceinline__ void stage_chunk(char* tile, const float* r4, int j) const {
    stage_copy<Cfg::PITCH>(tile, threadIdx.x + Cfg::NT * j, r4);
  }
};

template <class Cfg>
struct SplitWeightLoader {                // pre-split packed weights: row n = Ktot/32 records of [32 hi | 32 lo] bf16
  static constexpr int NCH = Cfg::NCH_B, NREG = NCH * 4;
  const char* base;                       // row n0 of the packed matrix
  int64_t row_bytes;                      // Ktot * 4
  int rows_valid;
  __device__ __forceinline__ void fetch_chunk(int kt, float (&r)[NREG], int j) const {
    const int e = threadIdx.x + 256 * j;
    const int row = e >> 3, part = e & 7;
    const char* src = (row < rows_valid && kt >= 0) ? base + row * row_bytes + (int64_t)kt * 128 + part * 16
                                                    : reinterpret_cast<const char*>(g_fsraft_zero16);   // kt < 0: zero tile
    const f32x4 v = gload4(src);
    r[4 * j + 0] = v[0]; r[4 * j + 1] = v[1]; r[4 * j + 2] = v[2]; r[4 * j + 3] = v[3];
  }
  __device__ __forceinline__ void stage_chunk(char* tile, const float* r4, int j) const {
    stage_copy<Cfg::PITCH>(tile, threadIdx.x + 256 * j, r4);
  }
};

template <class Cfg, int EPI>
__device__ __forceinline__ void conv_epilogue(const ConvArgs& a, f32x16 (&acc)[Cfg::TM][Cfg::TN], int m0, int n0) {
  const int HW = a.H * a.W;
  const int M = a.B * HW;
  // Epilogue.  Everything is batched per 32x32 MFMA tile: 16 addresses, then (optionally) 16
  // loads in flight, then 16 stores, with no wait between consecutive stores.  Rows of one
  // accumulator tile are m = mbase + (r&3) + 8*(r>>2); a 128-row tile crosses at most one
  // image boundary, so (batch, pixel) is derived from one division per tile.
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int nt = 0; nt < Cfg::TN; ++nt) {
    const int n = n0 + acc_col<Cfg>(nt);
    const bool nok = n < a.N;
    const float bias = (nok && a.bias) ? a.bias[n] : 0.f;
    int di = 0;
    if (a.ndst > 1 && n >= a.dst[1].n0) di = 1;
    if (a.ndst > 2 && n >= a.dst[2].n0) di = 2;
    float* dp = di == 0 ? a.dst[0].p : di == 1 ? a.dst[1].p : a.dst[2].p;
    const int64_t dbs = di == 0 ? a.dst[0].bs : di == 1 ? a.dst[1].bs : a.dst[2].bs;
    const int64_t dps = di == 0 ? a.dst[0].ps : di == 1 ? a.dst[1].ps : a.dst[2].ps;
    const int64_t dcs = di == 0 ? a.dst[0].cs : di == 1 ? a.dst[1].cs : a.dst[2].cs;
    const int dn0 = di == 0 ? a.dst[0].n0 : di == 1 ? a.dst[1].n0 : a.dst[2].n0;
    const bool dacc = (di == 0 ? a.dst[0].accumulate : di == 1 ? a.dst[1].accumulate : a.dst[2].accumulate) != 0;
    const float* mk = di == 0 ? a.rmask[0] : di == 1 ? a.rmask[1] : a.rmask[2];
    const int ldm = di == 0 ? a.ldmask[0] : di == 1 ? a.ldmask[1] : a.ldmask[2];
    const int mkc = di == 0 ? a.maskc[0] : di == 1 ? a.maskc[1] : a.maskc[2];
#pragma unroll
    for (int mt = 0; mt < Cfg::TM; ++mt) {
      const int mbase = m0 + (wave / Cfg::WN) * (Cfg::TM * 32) + mt * 32 + 4 * (lane >> 5);
      const int b0 = mbase / HW, pix0 = mbase - b0 * HW;
      if (EPI == EPI_PLAIN) {
        // two batches of 8 rows: 8 element offsets (32-bit), 8 optional loads in flight, 8 stores
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
          int off[8];
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const int r = hb * 8 + q;
            const int d = (r & 3) + 8 * (r >> 2);
            int pix = pix0 + d, b = b0;
            if (pix >= HW) { pix -= HW; ++b; }
            const bool ok = nok && (mbase + d < M);
            off[q] = ok ? (int)(b * dbs + pix * dps + (n - dn0) * dcs) : -1;
          }
          float old[8];
#pragma unroll
          for (int q = 0; q < 8; ++q) old[q] = (dacc && off[q] >= 0) ? dp[off[q]] : 0.f;
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            float v = (acc[mt][nt][hb * 8 + q] + bias) * a.alpha;
            if (a.relu) v = fmaxf(v, 0.f);
            v += old[q];
            if (off[q] >= 0 && mk && n - dn0 < mkc) {
              const int r = hb * 8 + q;
              const int64_t m = mbase + (r & 3) + 8 * (r >> 2);
              if (mk[m * ldm + (n - dn0)] <= 0.f) v = 0.f;
            }
            if (off[q] >= 0) dp[off[q]] = v;
          }
        }
      } else if (EPI == EPI_ZR) {
        const bool isz = n < a.hid;
        const int c = isz ? n : n - a.hid;
        float hh[16];
        bool ok[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = mbase + (r & 3) + 8 * (r >> 2);
          ok[r] = nok && m < M;
          hh[r] = (ok[r] && !isz) ? a.h[(int64_t)m * a.ldh + c] : 0.f;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int64_t m = mbase + (r & 3) + 8 * (r >> 2);
          const float pre = (a.pre && ok[r]) ? a.pre[m * a.ldpre + n] : 0.f;
          const float sg = 1.0f / (1.0f + expf(-(acc[mt][nt][r] + bias + pre)));
          if (ok[r]) {
            if (isz) {
              a.dst[0].p[m * a.dst[0].ps + c] = sg;                 // z
            } else {
              a.aux2[m * a.ld2 + c] = sg;                           // r
              a.aux1[m * a.ld1 + c] = sg * hh[r];                   // r*h
            }
          }
        }
      } else {   // EPI_Q
        float hh[16], zz[16];
        bool ok[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int64_t m = mbase + (r & 3) + 8 * (r >> 2);
          ok[r] = nok && m < M;
          hh[r] = ok[r] ? a.h[m * a.ldh + n] : 0.f;
          zz[r] = ok[r] ? a.z[m * a.ldz + n] : 0.f;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int64_t m = mbase + (r & 3) + 8 * (r >> 2);
          const float pre = (a.pre && ok[r]) ? a.pre[m * a.ldpre + n] : 0.f;
          const float q = tanhf(acc[mt][nt][r] + bias + pre);
          if (ok[r]) {
            a.aux1[m * a.ld1 + n] = q;
            a.dst[0].p[m * a.dst[0].ps + n] = (1.f - zz[r]) * hh[r] + zz[r] * q;
          }
        }
      }
    }
  }
}

// Epilogue through LDS for channels-last destinations: the accumulator tile is parked in LDS (row
// pitch BN+4 floats) and leaves as whole rows, 16 bytes per lane and 512 contiguous bytes per row of a
// 128-wide tile, instead of 64 four-byte stores per lane.  GRU gate math runs on the float4s.
// PATCH: the tile's 256 rows are an 8 x 32 patch of pixels (conv_patch.inc): row r is pixel (py0 + r / 32, px0 + r % 32) of
// image pb, rows outside the image are skipped.  NTW: threads taking part (the workgroup's).
template <class Cfg, int EPI, int NTW = Cfg::NT, bool PATCH = false>
__device__ __forceinline__ void conv_epilogue_lds(const ConvArgs& a, f32x16 (&acc)[Cfg::TM][Cfg::TN], int m0, int n0,
                                                  float* __restrict__ tile, bool owner = true, int pb = 0, int py0 = 0, int px0 = 0,
                                                  int64_t mofs = 0) {
  constexpr int LD = Cfg::BN + 4;
  const int HW = a.H * a.W;
  const int M = a.B * HW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // row of the tile -> row of the [M][*] tensors (-1: nothing there)
  auto row_m = [&](int row) -> int64_t {
    if constexpr (PATCH) {
      const int y = py0 + (row >> 5), x = px0 + (row & 31);
      return (y < a.H && x < a.W) ? (int64_t)(pb * a.H + y) * a.W + x : -1;
    } else {
      return m0 + row < M ? (int64_t)m0 + row : -1;
    }
  };
  __syncthreads();                                   // the k-loop's last LDS reads are done
#pragma unroll
  for (int nt = 0; nt < Cfg::TN; ++nt) {
    const int nl = acc_col<Cfg>(nt);
    const float bias = (n0 + nl < a.N && a.bias) ? a.bias[n0 + nl] : 0.f;
#pragma unroll
    for (int mt = 0; mt < Cfg::TM; ++mt) {
      const int rbase = (wave / Cfg::WN) * (Cfg::TM * 32) + mt * 32 + 4 * (lane >> 5);
#pragma unroll
      for (int r = 0; r < 16; ++r) tile[(rbase + (r & 3) + 8 * (r >> 2)) * LD + nl] = acc[mt][nt][r] + bias;
    }
  }
  __syncthreads();
  constexpr int C4 = Cfg::BN / 4;                    // float4 columns per row
  constexpr int RPP = NTW / C4;                      // rows covered per pass
  (void)owner;
  const int c4 = threadIdx.x % C4, rsub = threadIdx.x / C4;
  const int n = n0 + c4 * 4;
  const bool stats = PATCH && EPI == EPI_PLAIN && a.st_sum != nullptr;      // (workgroup-uniform: the barriers below are safe)
  if (n >= a.N && !stats) return;
  if (EPI == EPI_PLAIN) {
    f32x4 ssum = {0.f, 0.f, 0.f, 0.f}, ssq = {0.f, 0.f, 0.f, 0.f};
    if (n < a.N) {
    int di = 0;
    if (a.ndst > 1 && n >= a.dst[1].n0) di = 1;
    if (a.ndst > 2 && n >= a.dst[2].n0) di = 2;
    float* dp = di == 0 ? a.dst[0].p : di == 1 ? a.dst[1].p : a.dst[2].p;
    const int64_t dps = di == 0 ? a.dst[0].ps : di == 1 ? a.dst[1].ps : a.dst[2].ps;
    const int dn0 = di == 0 ? a.dst[0].n0 : di == 1 ? a.dst[1].n0 : a.dst[2].n0;
    const bool dacc = (di == 0 ? a.dst[0].accumulate : di == 1 ? a.dst[1].accumulate : a.dst[2].accumulate) != 0;
    const float* mk = di == 0 ? a.rmask[0] : di == 1 ? a.rmask[1] : a.rmask[2];
    const int ldm = di == 0 ? a.ldmask[0] : di == 1 ? a.ldmask[1] : a.ldmask[2];
    const int mkc = di == 0 ? a.maskc[0] : di == 1 ? a.maskc[1] : a.maskc[2];
    const int nv = a.N - n < 4 ? a.N - n : 4;        // valid columns of this float4 (N need not be a multiple of 4)
#pragma unroll 4
    for (int row = rsub; row < Cfg::BM; row += RPP) {
      const int64_t m = row_m(row);
      if (m < 0) { if (PATCH) continue; else break; }
      f32x4 v = *reinterpret_cast<const f32x4*>(tile + row * LD + c4 * 4);
      float* o = dp + (int64_t)(m + mofs) * dps + (n - dn0);      // (mofs: the k-slice's slab of the split-K workspace)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[i] *= a.alpha;
        if (a.relu) v[i] = fmaxf(v[i], 0.f);
      }
      if (nv == 4) {
        if (stats) { ssum += v; ssq += v * v; }
        if (dacc) {
          const f32x4 old = gload4(o);
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] += old[i];
        }
        if (mk) {
          const f32x4 y = gload4(mk + (int64_t)m * ldm + (n - dn0));
#pragma unroll
          for (int i = 0; i < 4; ++i) if (n - dn0 + i < mkc && y[i] <= 0.f) v[i] = 0.f;
        }
        gstore4(o, v);
      } else {
        for (int i = 0; i < nv; ++i) {
          float r = dacc ? gload1(o + i) + v[i] : v[i];
          if (mk && n - dn0 + i < mkc && gload1(mk + (int64_t)m * ldm + (n - dn0) + i) <= 0.f) r = 0.f;
          gstore1(o + i, r);
        }
      }
    }
    }
    if constexpr (PATCH) {
      if (stats) {
        // column sums of the tile: every thread summed its rows of its four columns above; the RPP row groups meet in LDS
        // (the parked tile is no longer needed) and one thread per column adds the workgroup's share to the slot row of its image
        __syncthreads();
        float* red = tile;
        *reinterpret_cast<f32x4*>(red + (rsub * Cfg::BN) + c4 * 4) = ssum;
        *reinterpret_cast<f32x4*>(red + ((RPP + rsub) * Cfg::BN) + c4 * 4) = ssq;
        __syncthreads();
        if (threadIdx.x < Cfg::BN && n0 + (int)threadIdx.x < a.N) {
          float t1 = 0.f, t2 = 0.f;
#pragma unroll 4
          for (int g = 0; g < RPP; ++g) { t1 += red[g * Cfg::BN + threadIdx.x]; t2 += red[(RPP + g) * Cfg::BN + threadIdx.x]; }
          const int64_t o = ((int64_t)pb * a.st_slots + (int)(blockIdx.y % (unsigned)a.st_slots)) * a.N + n0 + threadIdx.x;
          atomicAdd(a.st_sum + o, t1);
          atomicAdd(a.st_sq + o, t2);
        }
      }
    }
  } else if (EPI == EPI_ZR) {
    const bool isz = n < a.hid;
    const int c = isz ? n : n - a.hid;
#pragma unroll 4
    for (int row = rsub; row < Cfg::BM; row += RPP) {
      const int64_t mr = row_m(row);
      if (mr < 0 && !PATCH) break;
      // (patch tiles: rows outside the image read row 0 and store nothing -- no branch around the loads, so the unrolled
      //  iterations' loads are issued together; with half as many threads as the 16-wave kernels the loop is latency-bound)
      const int64_t m = mr < 0 ? 0 : mr;
      f32x4 v = *reinterpret_cast<const f32x4*>(tile + row * LD + c4 * 4);
      if (a.pre) v += gload4(a.pre + m * a.ldpre + n);
      f32x4 hh = {0.f, 0.f, 0.f, 0.f};
      if (!isz) hh = gload4(a.h + m * a.ldh + c);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = 1.0f / (1.0f + expf(-v[i]));
      if (mr < 0) continue;
      if (isz) {
        *reinterpret_cast<f32x4*>(a.dst[0].p + m * a.dst[0].ps + c) = v;                 // z
      } else {
        *reinterpret_cast<f32x4*>(a.aux2 + m * a.ld2 + c) = v;                            // r
        f32x4 rh;
#pragma unroll
        for (int i = 0; i < 4; ++i) rh[i] = v[i] * hh[i];
        *reinterpret_cast<f32x4*>(a.aux1 + m * a.ld1 + c) = rh;                           // r*h
      }
    }
  } else {   // EPI_Q
#pragma unroll 4
    for (int row = rsub; row < Cfg::BM; row += RPP) {
      const int64_t m = row_m(row);
      if (m < 0) { if (PATCH) continue; else break; }
      f32x4 v = *reinterpret_cast<const f32x4*>(tile + row * LD + c4 * 4);
      if (a.pre) v += gload4(a.pre + m * a.ldpre + n);
      const f32x4 hh = gload4(a.h + m * a.ldh + n);
      const f32x4 zz = gload4(a.z + m * a.ldz + n);
      f32x4 hn;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[i] = tanhf(v[i]);
        hn[i] = (1.f - zz[i]) * hh[i] + zz[i] * v[i];
      }
      *reinterpret_cast<f32x4*>(a.aux1 + m * a.ld1 + n) = v;                              // q
      *reinterpret_cast<f32x4*>(a.dst[0].p + m * a.dst[0].ps + n) = hn;                   // h'
    }
  }
}

// rows of every destination are 16-byte aligned and channels-last (column stride 1)?
__device__ __forceinline__ bool epilogue_rows_ok(const ConvArgs& a) {
  bool ok = true;
  for (int i = 0; i < a.ndst; ++i)
    ok = ok && a.dst[i].cs == 1 && (a.dst[i].ps & 3) == 0 && (a.dst[i].n0 & 3) == 0 && ((uintptr_t)a.dst[i].p & 15) == 0 &&
         a.dst[i].bs == a.dst[i].ps * (int64_t)(a.H * a.W);
  return ok;
}

bool epilogue_rows_ok_host(const ConvArgs& a) {
  bool ok = true;
  for (int i = 0; i < a.ndst; ++i)
    ok = ok && a.dst[i].cs == 1 && (a.dst[i].ps & 3) == 0 && (a.dst[i].n0 & 3) == 0 && ((uintptr_t)a.dst[i].p & 15) == 0 &&
         a.dst[i].bs == a.dst[i].ps * (int64_t)(a.H * a.W);
  return ok;
}

// exact-fp32 variant: v_mfma_f32_32x32x2_f32
template <class Cfg, int EPI>
__global__ __launch_bounds__(256) void conv_igemm_kernel(ConvArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[Cfg::LDS_FLOATS];
  const int HW = a.H * a.W;
  const int M = a.B * HW;
  const int n0 = blockIdx.x * Cfg::BN, m0 = blockIdx.y * Cfg::BM;
  ConvALoader<Cfg> la;
  // k-tiles per tap: channel runs are packed in multiples of 32 whatever BK is
  la.p0 = a.src[0].p; la.C0 = a.src[0].C; la.ld0 = a.src[0].ld; la.cpt0 = (a.src[0].C + 31) / 32 * (32 / Cfg::BK);
  la.p1 = a.src[1].p; la.C1 = a.src[1].C; la.ld1 = a.src[1].ld; la.cpt1 = a.nsrc > 1 ? (a.src[1].C + 31) / 32 * (32 / Cfg::BK) : 0;
  la.p2 = a.src[2].p; la.C2 = a.src[2].C; la.ld2 = a.src[2].ld; la.cpt2 = a.nsrc > 2 ? (a.src[2].C + 31) / 32 * (32 / Cfg::BK) : 0;
  if (a.nsrc < 2) { la.p1 = a.src[0].p; la.C1 = 0; la.ld1 = 4; la.cpt1 = 1; }
  if (a.nsrc < 3) { la.p2 = a.src[0].p; la.C2 = 0; la.ld2 = 4; la.cpt2 = 1; }
  la.taps = a.KH * a.KW; la.KW = a.KW; la.PH = a.PH; la.PW = a.PW; la.H = a.H; la.W = a.W;
#pragma unroll
  for (int j = 0; j < ConvALoader<Cfg>::NF4; ++j) {
    const int row = (threadIdx.x + 256 * j) / ConvALoader<Cfg>::F4;
    const int m = m0 + row;
    if (m < M) {
      const int b = m / HW, pix = m % HW;
      la.py[j] = pix / a.W; la.px[j] = pix % a.W; la.pb[j] = (int64_t)b * HW;
    } else {
      la.py[j] = -1; la.px[j] = 0; la.pb[j] = 0;
    }
  }
  RowMajorTileLoader<Cfg::BN, Cfg::BK, Cfg::LDB> lb{a.wpk + (int64_t)n0 * a.Ktot, a.Ktot, a.N - n0, a.Ktot};
  f32x16 acc[Cfg::TM][Cfg::TN];
#pragma unroll
  for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
    for (int j = 0; j < Cfg::TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  gemm_mainloop<Cfg>(lds, a.Ktot / Cfg::BK, la, lb, acc);
  conv_epilogue<Cfg, EPI>(a, acc, m0, n0);
}

// split-bf16 variant: 3 x v_mfma_f32_32x32x16_bf16 per product block, weights pre-split at pack time
template <class Cfg, int EPI, int BUF = 0>       // BUF 0: flat 64-bit addressing, 1: buffer loads + k-tile table, 2: uniform-pitch table
__global__ __launch_bounds__(Cfg::NT) void conv_igemm_split_kernel(const std::conditional_t<BUF != 0, ConvArgsT, ConvArgs> args) {
  static_assert(Cfg::NT == 256 || BUF != 0, "wider workgroups use the buffer-addressed loaders");
  __shared__ __attribute__((aligned(16))) char lds[Cfg::LDS_ALLOC];
  const ConvArgs& a = [&]() -> const ConvArgs& { if constexpr (BUF != 0) return args.a; else return args; }();
  const int HW = a.H * a.W;
  const int M = a.B * HW;
  int bx = blockIdx.x, by = blockIdx.y;
  tile_of_block(a.swz, bx, by);
  const int n0 = bx * Cfg::BN, m0 = by * Cfg::BM;
  f32x16 acc[Cfg::TM][Cfg::TN];
#pragma unroll
  for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
    for (int j = 0; j < Cfg::TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  if constexpr (BUF != 0) {
    const int PH = a.PH, PW = a.PW, taps = a.KH * a.KW;
    // Index the table where it lives, in the kernarg segment: going through the by-value struct would make the
    // compiler copy it to scratch (dynamic index), and a scratch load is per-lane, i.e. no longer provably uniform.
    const auto* ktab = (const unsigned __attribute__((address_space(4)))*)(
        (const char __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(ConvArgsT, ktab));
    // split-K (small M): this workgroup's slice of the k-tiles; the table and the weight rows are entered kt0 tiles further on
    int kt0 = 0, KTs = a.Ktot / 32;
    if (a.ksplit > 1) {
      const int per = (KTs + a.ksplit - 1) / a.ksplit;
      kt0 = (int)blockIdx.z * per;
      KTs = min(per, KTs - kt0);
      ktab += kt0 * (BUF >= 2 ? 2 : 1);
    }
    unsigned tapmask[Cfg::NCH_A], pofs[Cfg::NCH_A];
#pragma unroll
    for (int j = 0; j < Cfg::NCH_A; ++j) {
      const int m = m0 + ((threadIdx.x + Cfg::NT * j) >> 3);
      unsigned mask = 0;
      if (m < M) {
        const int pix = m % HW, y = pix / a.W, x = pix % a.W;
        for (int t = 0; t < taps; ++t) {
          const int yy = y + t / a.KW - PH, xx = x + t % a.KW - PW;
          if ((unsigned)yy < (unsigned)a.H && (unsigned)xx < (unsigned)a.W) mask |= 1u << t;
        }
      }
      tapmask[j] = mask; pofs[j] = m < M ? m : 0;
    }
    BufWeightLoader<Cfg> lb;
    lb.base = uni_ptr(reinterpret_cast<const char*>(a.wpk) + (int64_t)n0 * a.Ktot * 4 + (int64_t)kt0 * 128);
    lb.nbytes = 0x7fffffffu;   // validity is carried by the lane offsets alone (FS_OOB), whatever the range check adds to them
#pragma unroll
    for (int j = 0; j < BufWeightLoader<Cfg>::NCH; ++j) {
      const int e = threadIdx.x + Cfg::NT * j;
      lb.voff[j] = (e >> 3) < a.N - n0 ? (unsigned)((e >> 3) * a.Ktot * 4 + (e & 7) * 16) : FS_OOB;
    }
    if constexpr (BUF >= 2) {
      BufConvALoaderU<Cfg> la;
      la.base = uni_ptr(args.ubase); la.ktab = ktab; la.kq16 = (threadIdx.x & 7) * 16;
      const unsigned ldb = uni((unsigned)args.uld * 4u);
#pragma unroll
      for (int j = 0; j < Cfg::NCH_A; ++j) { la.tapmask[j] = tapmask[j]; la.voff0[j] = pofs[j] * ldb + la.kq16; }
      split_mainloop<Cfg, BufConvALoaderU<Cfg>, BufWeightLoader<Cfg>, true>(lds, KTs, la, lb, acc);
    } else {
      BufConvALoader<Cfg> la;
      la.ld0x4 = uni(a.src[0].ld * 4); la.ld1x4 = uni(a.src[1].ld * 4); la.ld2x4 = uni(a.src[2].ld * 4);
      // descriptor base = tensor base - (PH*W + PW) pixels, so the per-tap SGPR offset (dy*W + dx)*ld is >= 0
      la.b0 = uni_ptr(a.src[0].p - (int64_t)(PH * a.W + PW) * a.src[0].ld); la.nb0 = 0x7fffffffu;
      la.b1 = uni_ptr(a.src[1].p - (int64_t)(PH * a.W + PW) * a.src[1].ld); la.nb1 = 0x7fffffffu;
      la.b2 = uni_ptr(a.src[2].p - (int64_t)(PH * a.W + PW) * a.src[2].ld); la.nb2 = 0x7fffffffu;
      la.ktab = ktab;
      la.kq16 = (threadIdx.x & 7) * 16;
#pragma unroll
      for (int j = 0; j < Cfg::NCH_A; ++j) { la.tapmask[j] = tapmask[j]; la.pofs[j] = pofs[j]; }
      split_mainloop<Cfg, BufConvALoader<Cfg>, BufWeightLoader<Cfg>, true>(lds, KTs, la, lb, acc);
    }
    if constexpr (EPI == EPI_PLAIN && Cfg::LDS_ALLOC >= Cfg::BM * (Cfg::BN + 4) * 4) {
      if (a.ksplit > 1) {               // first pass of the split-K route: the raw partial tile -> slab blockIdx.z of the workspace
        conv_epilogue_lds<Cfg, EPI_PLAIN>(a, acc, m0, n0, reinterpret_cast<float*>(lds), true, 0, 0, 0, (int64_t)blockIdx.z * M);
        return;
      }
    }
  } else {
  SplitConvALoader<Cfg> la;
  la.p0 = a.src[0].p; la.C0 = a.src[0].C; la.ld0 = a.src[0].ld; la.cpt0 = (a.src[0].C + 31) / 32;
  la.p1 = a.src[1].p; la.C1 = a.src[1].C; la.ld1 = a.src[1].ld; la.cpt1 = a.nsrc > 1 ? (a.src[1].C + 31) / 32 : 0;
  la.p2 = a.src[2].p; la.C2 = a.src[2].C; la.ld2 = a.src[2].ld; la.cpt2 = a.nsrc > 2 ? (a.src[2].C + 31) / 32 : 0;
  if (a.nsrc < 2) { la.p1 = a.src[0].p; la.C1 = 0; la.ld1 = 4; la.cpt1 = 1; }
  if (a.nsrc < 3) { la.p2 = a.src[0].p; la.C2 = 0; la.ld2 = 4; la.cpt2 = 1; }
  la.taps = a.KH * a.KW; la.KW = a.KW; la.PH = a.PH; la.PW = a.PW; la.H = a.H; la.W = a.W;
#pragma unroll
  for (int j = 0; j < SplitConvALoader<Cfg>::NCH; ++j) {
    const int m = m0 + ((threadIdx.x + 256 * j) >> 3);
    if (m < M) {
      const int pix = m % HW;
      la.py[j] = pix / a.W; la.px[j] = pix % a.W; la.pofs[j] = m;
    } else {
      la.py[j] = -(1 << 20); la.px[j] = 0; la.pofs[j] = 0;      // fails every (unsigned)(py+dy) < H test
    }
  }
  SplitWeightLoader<Cfg> lb{reinterpret_cast<const char*>(a.wpk) + (int64_t)n0 * a.Ktot * 4, (int64_t)a.Ktot * 4, a.N - n0};
  split_mainloop<Cfg>(lds, a.Ktot / 32, la, lb, acc);
  }
  if constexpr (Cfg::LDS_ALLOC >= Cfg::BM * (Cfg::BN + 4) * 4) {     // the parked tile must fit the LDS allocation
    if (EPI != EPI_PLAIN || epilogue_rows_ok(a)) {
      conv_epilogue_lds<Cfg, EPI>(a, acc, m0, n0, reinterpret_cast<float*>(lds));
      return;
    }
  }
  conv_epilogue<Cfg, EPI>(a, acc, m0, n0);
}

// ---------------------------------------------------------------- 3x3 convolution over a resident input patch
// The implicit GEMM above re-reads every input pixel once per tap: a few-channel 3x3 layer at encoder resolution
// (64 -> 64 at 8 x 220 x 512) moves 9 x 231 MB through the load path for 2 x 0.2 GB of unique data and is bound by
// bytes in flight, not by the matrix pipe.  Here a workgroup owns a 4 x 32 patch of output pixels: it loads the
// 6 x 34 input patch (halo included) ONCE, splits it to [hi | lo] bf16 and keeps it in LDS (one 128-byte record per
// pixel and 32-channel group, same swizzle as the A image of split_mainloop); the k-loop then walks (tap, channel
// group), reading the A fragments straight out of the patch at the tap's row shift, and streams only the weight
// tiles.  Global traffic per output pixel drops from 9 to 1.6 input pixels and the per-k-tile staging to the B tile.
constexpr int HALO_TH = 4, HALO_TW = 32, HALO_PW = HALO_TW + 2, HALO_ROWS = (HALO_TH + 2) * HALO_PW;
struct HaloArgs {
  const float* x; int ldx, C;
  const char* wpk;                    // fragment-order split pack (fsraft_conv_desc.wpk_frag)
  const float* bias;
  float* out; int64_t obs, ops;       // batch / pixel strides of the destination (floats), channels contiguous
  int N, B, H, W, relu;
  int acc;                            // out += result (the data gradient of a residual unit's first convolution adds to the shortcut gradient)
  float* st_sum; float* st_sq; int st_slots;   // as in ConvArgs (NULL: none)
};

template <int CG, int TN>
__global__ __launch_bounds__(256) void conv3x3_halo_kernel(const HaloArgs a) {
  constexpr int PLANE = HALO_ROWS * 128;
  constexpr int NCHH = (HALO_ROWS * CG * 8 + 255) / 256, KT = 9 * CG;
  __shared__ __attribute__((aligned(16))) char lds[CG * PLANE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, lh = lane >> 5;
  const int x0 = blockIdx.x * HALO_TW, y0 = blockIdx.y * HALO_TH, b = blockIdx.z;

  // Weight fragments come straight from the packed matrix (L1/L2-resident: 4 * N * Ktot bytes for the whole grid): lane
  // (n, k half) reads its 16 bytes of hi and of lo for both k-steps of a k-tile.  No B image in LDS, hence no barrier in
  // the k-loop: once the patch is staged the waves run independently.
  // (a.wpk is the FRAGMENT-ORDER pack: [k-tile][32-column block][hi s0, hi s1, lo s0, lo s1][lane][16 B], so that one
  // wave-load is 1 KB of consecutive bytes -- read out of the row-major pack the same fragment touches 32 cache lines
  // and the kernel becomes L1-bound: 352 us instead of 270 us with an LDS-staged B on the 64 -> 64 encoder layer.)
  const int NB = (a.N + 31) >> 5;
  const char* wbase = uni_ptr(a.wpk);
  struct BFrag { u32x4 v[TN][4]; };             // [nt][hi s0, hi s1, lo s0, lo s1]
  auto fetch_b = [&](int kt, BFrag& f) {
    const int ku = __builtin_amdgcn_readfirstlane(kt < KT ? kt : KT - 1);
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(wbase, 0x7fffffffu);
#pragma unroll
    for (int nt = 0; nt < TN; ++nt) {
      const int nb = wn * TN + nt;
      const unsigned soff = (unsigned)((ku * NB + (nb < NB ? nb : 0)) * 4096);
      const unsigned voff = nb < NB ? (unsigned)lane * 16u : FS_OOB;
#pragma unroll
      for (int q = 0; q < 4; ++q) f.v[nt][q] = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff + 1024u * q, 0);
    }
  };
  // Four fragment sets, three k-tiles of look-ahead (an L2 hit is several k-tiles of MFMA time away): 238 -> 231 us.
  // PMC on this kernel: 6.9 VALU instructions per MFMA, 40 % of them in the patch conversion prologue and the 4-byte
  // store epilogue, waves waiting 29 % of their lifetime.
  BFrag f[4];
  fetch_b(0, f[0]);
  fetch_b(1, f[1]);
  fetch_b(2, f[2]);

  // the input patch: chunk e = (patch row, channel group, 16-byte part); consecutive lanes read consecutive bytes
  {
    const float* img = uni_ptr(a.x + (int64_t)b * a.H * a.W * a.ldx);
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(img, 0x7fffffffu);
    float rh[NCHH * 4];
#pragma unroll
    for (int j = 0; j < NCHH; ++j) {
      const int e = threadIdx.x + 256 * j;
      const int row = e / (CG * 8), rem = e % (CG * 8), ch = (rem >> 3) * 32 + (rem & 7) * 4;
      const int y = y0 - 1 + row / HALO_PW, x = x0 - 1 + row % HALO_PW;
      const bool ok = row < HALO_ROWS && (unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W && ch < a.C;
      const unsigned voff = ok ? (unsigned)((y * a.W + x) * a.ldx + ch) * 4u : FS_OOB;
      const f32x4 f = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, 0, 0));
      rh[4 * j + 0] = f[0]; rh[4 * j + 1] = f[1]; rh[4 * j + 2] = f[2]; rh[4 * j + 3] = f[3];
    }
#pragma unroll
    for (int j = 0; j < NCHH; ++j) {
      const int e = threadIdx.x + 256 * j;
      const int row = e / (CG * 8), rem = e % (CG * 8);
      if (row < HALO_ROWS) stage_convert<128>(lds + (rem >> 3) * PLANE, row * 8 + (rem & 7), rh + 4 * j);
    }
  }
  __syncthreads();

  f32x16 acc[2][TN];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  auto compute = [&](int kt, const BFrag& f) {
    const int ku = __builtin_amdgcn_readfirstlane(kt);
    const int tap = ku / CG, g = ku - tap * CG, dy = tap / 3, dx = tap - dy * 3;
    const char* Ap = lds + g * PLANE;
    const int rowa = (2 * wm + dy) * HALO_PW + dx + l31;          // patch row of this lane for mt = 0; mt = 1 is one patch line down
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 ah[2], al[2];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        const int row = rowa + mt * HALO_PW;
        ah[mt] = *reinterpret_cast<const bf16x8*>(Ap + slot_offset<128>(row, 2 * s + lh));
        al[mt] = *reinterpret_cast<const bf16x8*>(Ap + slot_offset<128>(row, 4 + 2 * s + lh));
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < TN; ++nt) {
          const bf16x8 bh = __builtin_bit_cast(bf16x8, f.v[nt][s]), bl = __builtin_bit_cast(bf16x8, f.v[nt][2 + s]);
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[mt], bh, acc[mt][nt], 0, 0, 0);
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mt], bl, acc[mt][nt], 0, 0, 0);
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mt], bh, acc[mt][nt], 0, 0, 0);
        }
    }
  };
  for (int kt = 0; kt < KT; kt += 4) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (kt + i < KT) {
        fetch_b(kt + i + 3, f[(i + 3) & 3]);      // (past the end: re-reads the last tile; unused)
        compute(kt + i, f[i]);
      }
  }

  if (a.st_sum) {
    // InstanceNorm statistics of the result: a lane owns column n of 2 x 16 pixels per nt; the two lane halves and the two
    // pixel-row waves (wm) meet through shuffles / LDS (the patch is no longer needed), one atomic pair per column and workgroup
    __syncthreads();
    float* red = reinterpret_cast<float*>(lds);          // [wm][2][64 * TN]
#pragma unroll
    for (int nt = 0; nt < TN; ++nt) {
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        const int py = y0 + 2 * wm + mt;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int px = x0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          const float v = (py < a.H && px < a.W) ? acc[mt][nt][r] : 0.f;
          s1 += v; s2 += v * v;
        }
      }
      s1 += __shfl_xor(s1, 32, 64); s2 += __shfl_xor(s2, 32, 64);
      const int col = wn * (32 * TN) + nt * 32 + l31;
      if (lh == 0) { red[(wm * 2 + 0) * (64 * TN) + col] = s1; red[(wm * 2 + 1) * (64 * TN) + col] = s2; }
    }
    __syncthreads();
    if ((int)threadIdx.x < 64 * TN && (int)threadIdx.x < a.N) {
      const int col = threadIdx.x;
      const int slot = (int)((blockIdx.y * gridDim.x + blockIdx.x) % (unsigned)a.st_slots);
      const int64_t o = ((int64_t)b * a.st_slots + slot) * a.N + col;
      atomicAdd(a.st_sum + o, red[col] + red[2 * (64 * TN) + col]);
      atomicAdd(a.st_sq + o, red[(64 * TN) + col] + red[3 * (64 * TN) + col]);
    }
  }
  float* outb = a.out + (int64_t)b * a.obs;
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    const int py = y0 + 2 * wm + mt;
    if (py >= a.H) continue;
#pragma unroll
    for (int nt = 0; nt < TN; ++nt) {
      const int n = wn * (32 * TN) + nt * 32 + l31;
      if (n >= a.N) continue;
      const float bv = a.bias ? a.bias[n] : 0.f;
      float old[16];                               // accumulating epilogue: the 16 old values are requested together
#pragma unroll                                     // (`*o = acc ? *o + v : v` is a branch and a round trip per element)
      for (int r = 0; r < 16; ++r) {
        const int px = x0 + (r & 3) + 8 * (r >> 2) + 4 * lh, pc = px < a.W ? px : a.W - 1;
        old[r] = a.acc ? outb[(int64_t)(py * a.W + pc) * a.ops + n] : 0.f;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int px = x0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (px >= a.W) continue;
        float v = acc[mt][nt][r] + bv;
        if (a.relu) v = fmaxf(v, 0.f);
        outb[(int64_t)(py * a.W + px) * a.ops + n] = v + old[r];
      }
    }
  }
}

template <int CG, int TN>
int launch_halo(const HaloArgs& h, hipStream_t s) {
  dim3 grid(ceil_div(h.W, HALO_TW), ceil_div(h.H, HALO_TH), h.B);
  hipLaunchKernelGGL((conv3x3_halo_kernel<CG, TN>), grid, dim3(256), 0, s, h);
  return fs_launch_status();
}

// Fills the per-k-tile table of the buffer-addressed kernels; false when the shape does not fit its fields
// (more than KTAB_MAX k-tiles, more than 15 taps, tap/channel offsets beyond 1 MiB, tensors of 2 GiB or more).
bool build_ktab(const ConvArgs& a, ConvArgsT& t) {
  const int taps = a.KH * a.KW, KT = a.Ktot / 32;
  const int64_t M = (int64_t)a.B * a.H * a.W;
  if (KT > KTAB_MAX || taps > 15) return false;
  int kt = 0;
  for (int s = 0; s < a.nsrc; ++s) {
    const int C = a.src[s].C, ld = a.src[s].ld, cpt = (C + 31) / 32;
    if (M * ld * 4 >= (int64_t)FS_OOB) return false;
    for (int i = 0; i < taps * cpt; ++i, ++kt) {
        const int tap = i / cpt, c = i % cpt;
        const int64_t soff = ((int64_t)((tap / a.KW) * a.W + tap % a.KW) * ld + c * 32) * 4;
        if (soff % 16 != 0 || soff / 16 > 0xffff) return false;
        const int crem = C - c * 32 < 32 ? C - c * 32 : 32;
        t.ktab[kt] = (unsigned)(soff / 16) | (unsigned)tap << 16 | (unsigned)s << 20 | (unsigned)crem << 22;
      }
  }
  if (kt != KT) return false;
  t.a = a;
  return true;
}

// Uniform form of the table (see ConvArgsT): possible when every source has the same pitch and all of them, shifted
// taps included, lie inside one 2 GiB window.
bool build_ktab_uniform(const ConvArgs& a, ConvArgsT& t) {
  const int taps = a.KH * a.KW, KT = a.Ktot / 32, PH = a.PH, PW = a.PW;
  const int64_t M = (int64_t)a.B * a.H * a.W;
  if (!knob.conv_uniform || 2 * KT > KTAB_MAX || taps > 15) return false;
  const int ld = a.src[0].ld;
  const float* lo = a.src[0].p;
  for (int s = 0; s < a.nsrc; ++s) {
    if (a.src[s].ld != ld) return false;
    if (a.src[s].p < lo) lo = a.src[s].p;
  }
  const float* base = lo - (int64_t)(PH * a.W + PW) * ld;      // tap shifts become non-negative offsets
  int kt = 0;
  for (int s = 0; s < a.nsrc; ++s) {
    const int C = a.src[s].C, cpt = (C + 31) / 32;
    const int64_t delta = (a.src[s].p - lo) * 4;                  // bytes
    for (int tap = 0; tap < taps; ++tap)
      for (int c = 0; c < cpt; ++c, ++kt) {
        const int64_t soff = delta + ((int64_t)((tap / a.KW) * a.W + tap % a.KW) * ld + c * 32) * 4;
        if (soff + M * ld * 4 + 256 >= (int64_t)FS_OOB) return false;
        const int crem = C - c * 32 < 32 ? C - c * 32 : 32;
        t.ktab[2 * kt] = (unsigned)soff;
        t.ktab[2 * kt + 1] = (unsigned)tap | (unsigned)crem << 4;
      }
  }
  if (kt != KT) return false;
  t.a = a; t.ubase = base; t.uld = ld;
  return true;
}


// ---- split-K for small M ----------------------------------------------------------------------------------------------
// At one or two pairs per GPU (the flow-supervisor recipe, config 4) a layer has 35-140 tiles of 64 pixels for 256 CUs and
// its time is the LENGTH of one workgroup's k-loop: 3x3 256 -> 192 takes 55 us at 4416 pixels, 57 us at 7332, 59 us at 8832
// (scripts/conv_micro.py) -- 72 k-tiles one after the other at ~0.75 us.  Here the k-tiles are dealt to `ksplit` workgroups per
// tile (grid.z), which park raw partial tiles in a workspace (conv_igemm_split_kernel, ksplit > 1), and this kernel adds the
// slabs and applies the layer's real epilogue (the row code of conv_epilogue_lds): bias / scale / ReLU / mask / accumulate
// into up to three destinations, or the GRU gate maths.
template <int EPI>
__global__ __launch_bounds__(256) void conv_finish_kernel(const ConvArgs a, const float* __restrict__ ws, int S, int ldw) {
  const int HW = a.H * a.W;
  const int64_t M = (int64_t)a.B * HW;
  const int C4 = (a.N + 3) / 4;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < M * C4; e += (int64_t)gridDim.x * 256) {
    const int64_t m = e / C4;
    const int n = (int)(e % C4) * 4;
    const int nv = a.N - n < 4 ? a.N - n : 4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (a.bias) {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = i < nv ? a.bias[n + i] : 0.f;
    }
    for (int s = 0; s < S; ++s) {
      const f32x4 p = gload4(ws + ((int64_t)s * M + m) * ldw + n);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] += p[i];
    }
    if (EPI == EPI_PLAIN) {
      int di = 0;
      if (a.ndst > 1 && n >= a.dst[1].n0) di = 1;
      if (a.ndst > 2 && n >= a.dst[2].n0) di = 2;
      float* dp = di == 0 ? a.dst[0].p : di == 1 ? a.dst[1].p : a.dst[2].p;
      const int64_t dbs = di == 0 ? a.dst[0].bs : di == 1 ? a.dst[1].bs : a.dst[2].bs;
      const int64_t dps = di == 0 ? a.dst[0].ps : di == 1 ? a.dst[1].ps : a.dst[2].ps;
      const int64_t dcs = di == 0 ? a.dst[0].cs : di == 1 ? a.dst[1].cs : a.dst[2].cs;
      const int dn0 = di == 0 ? a.dst[0].n0 : di == 1 ? a.dst[1].n0 : a.dst[2].n0;
      const bool dacc = (di == 0 ? a.dst[0].accumulate : di == 1 ? a.dst[1].accumulate : a.dst[2].accumulate) != 0;
      const float* mk = di == 0 ? a.rmask[0] : di == 1 ? a.rmask[1] : a.rmask[2];
      const int ldm = di == 0 ? a.ldmask[0] : di == 1 ? a.ldmask[1] : a.ldmask[2];
      const int mkc = di == 0 ? a.maskc[0] : di == 1 ? a.maskc[1] : a.maskc[2];
      const int64_t b = m / HW, pix = m - b * HW;
      float* o = dp + b * dbs + pix * dps + (int64_t)(n - dn0) * dcs;
      for (int i = 0; i < nv; ++i) {
        float r = v[i] * a.alpha;
        if (a.relu) r = fmaxf(r, 0.f);
        if (dacc) r += o[i * dcs];
        if (mk && n - dn0 + i < mkc && mk[m * ldm + (n - dn0) + i] <= 0.f) r = 0.f;
        o[i * dcs] = r;
      }
    } else if (EPI == EPI_ZR) {
      const bool isz = n < a.hid;
      const int c = isz ? n : n - a.hid;
      if (a.pre) v += gload4(a.pre + m * a.ldpre + n);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = 1.0f / (1.0f + expf(-v[i]));
      if (isz) {
        *reinterpret_cast<f32x4*>(a.dst[0].p + m * a.dst[0].ps + c) = v;                 // z
      } else {
        const f32x4 hh = gload4(a.h + m * a.ldh + c);
        *reinterpret_cast<f32x4*>(a.aux2 + m * a.ld2 + c) = v;                            // r
        f32x4 rh;
#pragma unroll
        for (int i = 0; i < 4; ++i) rh[i] = v[i] * hh[i];
        *reinterpret_cast<f32x4*>(a.aux1 + m * a.ld1 + c) = rh;                           // r*h
      }
    } else {   // EPI_Q
      if (a.pre) v += gload4(a.pre + m * a.ldpre + n);
      const f32x4 hh = gload4(a.h + m * a.ldh + n);
      const f32x4 zz = gload4(a.z + m * a.ldz + n);
      f32x4 hn;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[i] = tanhf(v[i]);
        hn[i] = (1.f - zz[i]) * hh[i] + zz[i] * v[i];
      }
      *reinterpret_cast<f32x4*>(a.aux1 + m * a.ld1 + n) = v;                              // q
      *reinterpret_cast<f32x4*>(a.dst[0].p + m * a.dst[0].ps + n) = hn;                   // h'
    }
  }
}

// Split-K scratch: the ABI allocates nothing, the caller lends it -- per CALL (fsraft_conv_desc.ws, what the Python mirror does) or,
// for bindings written against the round-3 header, per calling THREAD (fsraft_conv_workspace).  Both live in thread_local storage,
// so two host threads enqueueing convolutions for two devices / streams (the reference's nn.DataParallel caller,
// pytorch/train.py:192) never see each other's pointer.
thread_local float* t_reg_ws = nullptr;        // fsraft_conv_workspace of this thread
thread_local int64_t t_reg_ws_floats = 0;
thread_local float* g_conv_ws = nullptr;       // the scratch of the call this thread is inside (set by fsraft_conv_forward)
thread_local int64_t g_conv_ws_floats = 0;

// Slices for a tile grid of `tiles` workgroups, KT k-tiles and N outputs.  Measured (scripts/conv_micro.py, 1 x 47x156, 1 x 46x96,
// 2 x 46x96, 2 x 54x128; round 3, docs/history): the route pays where fewer than ~half of the CUs have a workgroup AND
// the second pass is small -- layers with <= 256 outputs (3x3 256 -> 126: 52 -> 40 us, 1x5 384 -> 128: 42 -> 34, the 3x3
// 512 -> 128 data gradient: 87 -> 52 us; at 4416 pixels 3x3 256 -> 192: 55 -> 44, 1x5 384 -> 256: 46 -> 39); with 512 outputs
// the slabs cost more than the shorter k-loops save (3x3 128 -> 512: 37 -> 55 us), and from ~230 tiles on the CUs are busy
// anyway.  128-row tiles (eight waves): the one-column layers of a two-pair batch leave 69-108 workgroups for 256 CUs and
// gain 15-45 % from two or three slices when the k-loop is long enough to share (3x3 256 -> 126 at 2 x 46x96: 59 -> 38 us,
// 3x3 512 -> 128 data gradient 100 -> 56, 1x5 384 -> 128: 45 -> 32); two-column layers only with >= 48 k-tiles (1x5 384 -> 256
// at 1 x 47x156: 47 -> 41 us, but the 20-tile data gradient 1x5 128 -> 256: 23 -> 29); above ~120 tiles nothing gains.
int pick_ksplit(int64_t tiles, int KT, int N, int64_t M, int ldw, int bm) {
  int S = 1;
  if (knob.conv_ksplit >= 2) S = knob.conv_ksplit;
  else if (knob.conv_ksplit == -1 && bm == 64 && tiles <= 150 && N <= 256 && KT >= 16) S = (int)((400 + tiles - 1) / tiles);
  else if (knob.conv_ksplit == -1 && bm == 128 && tiles <= 120 && N <= 256 && KT >= (N <= 128 ? 36 : 48)) S = tiles <= 115 ? (int)(230 / tiles) : 2;
  if (S > KT / 6) S = KT / 6;
  if (S > 6) S = 6;
  while (S > 1 && (int64_t)S * M * ldw > g_conv_ws_floats) --S;
  if (S > 1) {                                   // no empty slice
    const int per = (KT + S - 1) / S;
    S = (KT + per - 1) / per;
  }
  return S < 2 ? 1 : S;
}

template <class Cfg>
int launch_conv_split(const ConvArgs& a, int epi, hipStream_t s) {
  const int M = a.B * a.H * a.W;
  dim3 grid(ceil_div(a.N, Cfg::BN), ceil_div(M, Cfg::BM));
  ConvArgsT t;
  // XCD-aware tile order (tile_of_block) once several N tiles re-read each A tile and the grid is many rounds deep:
  // 192 -> 256 at M = 225 K (encoder-sized data gradients): 776 -> 714 us; nothing at the update block's 220..880 tiles.
  const int swz = knob.xcd_swizzle || (grid.x >= 2 && (int64_t)grid.x * grid.y >= 2048);
  // buffer-addressed loaders + branch-free k-loop: measured faster on the 64-row tiles, slower on 128x128
  const bool buf = knob.conv_buf == 2 || (knob.conv_buf == 1 && Cfg::BM == 64) || Cfg::BN == 256 || Cfg::NT != 256;
  if constexpr (Cfg::LDS_ALLOC >= Cfg::BM * (Cfg::BN + 4) * 4) {
    // split-K route (small M): partial tiles into the workspace, then conv_finish_kernel with the layer's own epilogue
    const int ldw = (a.N + 3) / 4 * 4;
    const bool gru_ok = epi == EPI_PLAIN || (a.N % 4 == 0 && (!a.pre || a.ldpre % 4 == 0));
    const int S = (buf && g_conv_ws && gru_ok && (Cfg::BM == 64 || (Cfg::BM == 128 && Cfg::NT == 512) || knob.conv_ksplit >= 2)) ? pick_ksplit((int64_t)grid.x * grid.y, a.Ktot / 32, a.N, M, ldw, Cfg::BM) : 1;
    if (S > 1) {
      const bool uni_tab = build_ktab_uniform(a, t);
      if (uni_tab || build_ktab(a, t)) {
        ConvArgs& p = t.a;
        p.swz = 0;
        p.ksplit = S;
        p.dst[0] = Dst{g_conv_ws, (int64_t)a.H * a.W * ldw, ldw, 1, 0, 0};
        p.dst[1] = p.dst[2] = p.dst[0];
        p.ndst = 1; p.bias = nullptr; p.relu = 0; p.alpha = 1.0f;
        for (int i = 0; i < 3; ++i) p.rmask[i] = nullptr;
        dim3 g3(grid.x, grid.y, S);
        t_route[0] = route_split<Cfg>() + 100;
        if (uni_tab) hipLaunchKernelGGL((conv_igemm_split_kernel<Cfg, EPI_PLAIN, 2>), g3, dim3(Cfg::NT), 0, s, t);
        else hipLaunchKernelGGL((conv_igemm_split_kernel<Cfg, EPI_PLAIN, 1>), g3, dim3(Cfg::NT), 0, s, t);
        int rc = fs_launch_status();
        if (rc) return rc;
        const int64_t work = (int64_t)M * (ldw / 4);
        const int fb = (int)((work + 255) / 256 < 4096 ? (work + 255) / 256 : 4096);
        with_epi(epi, [&](auto e) { hipLaunchKernelGGL(conv_finish_kernel<decltype(e)::value>, dim3(fb), dim3(256), 0, s, a, g_conv_ws, S, ldw); });
        return fs_launch_status();
      }
    }
  }
  if (buf && build_ktab_uniform(a, t)) {
    t.a.swz = swz;
    t_route[0] = route_split<Cfg>();
    with_epi(epi, [&](auto e) { hipLaunchKernelGGL((conv_igemm_split_kernel<Cfg, decltype(e)::value, 2>), grid, dim3(Cfg::NT), 0, s, t); });
    return fs_launch_status();
  }
  if (buf && build_ktab(a, t)) {
    t.a.swz = swz;
    t_route[0] = route_split<Cfg>();
    with_epi(epi, [&](auto e) { hipLaunchKernelGGL((conv_igemm_split_kernel<Cfg, decltype(e)::value, 1>), grid, dim3(Cfg::NT), 0, s, t); });
    return fs_launch_status();
  }
  if constexpr (Cfg::NT != 256) {
    return -1;          // the wide configurations exist for the buffer-addressed paths only: caller falls back
  } else {
  t_route[0] = route_split<Cfg>();
  with_epi(epi, [&](auto e) { hipLaunchKernelGGL((conv_igemm_split_kernel<Cfg, decltype(e)::value>), grid, dim3(256), 0, s, a); });
  return fs_launch_status();
  }
}

// plain-epilogue-only launcher of a wide configuration (the narrow-N tiles never carry a GRU epilogue)
template <class Cfg>
int launch_conv_split_plain(const ConvArgs& a, hipStream_t s) {
  const int M = a.B * a.H * a.W;
  dim3 grid(ceil_div(a.N, Cfg::BN), ceil_div(M, Cfg::BM));
  ConvArgsT t;
  if (build_ktab_uniform(a, t)) {
    t_route[0] = route_split<Cfg>();
    hipLaunchKernelGGL((conv_igemm_split_kernel<Cfg, EPI_PLAIN, 2>), grid, dim3(Cfg::NT), 0, s, t);
    return fs_launch_status();
  }
  if (build_ktab(a, t)) {
    t_route[0] = route_split<Cfg>();
    hipLaunchKernelGGL((conv_igemm_split_kernel<Cfg, EPI_PLAIN, 1>), grid, dim3(Cfg::NT), 0, s, t);
    return fs_launch_status();
  }
  return -1;
}

template <class Cfg>
int launch_conv(const ConvArgs& a, int epi, hipStream_t s) {
  const int M = a.B * a.H * a.W;
  dim3 grid(ceil_div(a.N, Cfg::BN), ceil_div(M, Cfg::BM));
  t_route[0] = route_gemm<Cfg>();
  with_epi(epi, [&](auto e) { hipLaunchKernelGGL((conv_igemm_kernel<Cfg, decltype(e)::value>), grid, dim3(256), 0, s, a); });
  return fs_launch_status();
}

#include "conv_patch.inc"

}  // namespace

extern "C" int fsraft_conv_ktot(const int* srcC, int nsrc, int KH, int KW) {
  if (!srcC || nsrc < 1 || nsrc > 3) return -1;
  return conv_ktot(srcC, nsrc, KH * KW);
}

namespace {
// fsraft_conv_forward_stats parks its request here for the call it wraps (same thread); the launch sites whose kernels can
// carry the statistics pick it up and say so
struct StatReq { float* sum; float* sq; int slots; bool done; };
thread_local StatReq t_stat{nullptr, nullptr, 0, false};
template <class Args>                      // ConvArgs or HaloArgs
void attach_stats(Args& p, bool want) {
  if (want) { p.st_sum = t_stat.sum; p.st_sq = t_stat.sq; p.st_slots = t_stat.slots; }
}
}  // namespace

extern "C" int fsraft_conv_forward(const fsraft_conv_desc* d, hipStream_t stream) {
  if (!d || d->nsrc < 1 || d->nsrc > 3 || d->ndst < 1 || d->ndst > 3 || !d->wpk || d->N < 1) return FS_ERR_ARG;
  // (statistics of the raw result only: one destination, no bias / ReLU / scale / mask / accumulation in the epilogue)
  const bool want_stats = t_stat.sum != nullptr && d->epi == EPI_PLAIN && d->ndst == 1 && !d->relu && d->alpha == 1.0f && !d->dst_acc[0] &&
                          !d->rmask[0] && !d->bias && d->dst_n0[0] == 0 && d->N % 4 == 0;
  if (d->ws && (((uintptr_t)d->ws & 15) || d->ws_floats < 0)) return FS_ERR_ARG;
  t_route[0] = 0;
  g_conv_ws = d->ws ? d->ws : t_reg_ws;                     // scratch of THIS call (thread_local: see the declaration)
  g_conv_ws_floats = d->ws ? d->ws_floats : t_reg_ws_floats;
  ConvArgs a{};
  if (!fill_srcs(a.src, d->src, d->srcC, d->srcld, d->nsrc)) return FS_ERR_ARG;
  for (int s = 0; s < d->nsrc; ++s) if (d->srcC[s] < 1) return FS_ERR_ARG;
  a.nsrc = d->nsrc;
  a.wpk = d->wpk; a.Ktot = conv_ktot(d->srcC, d->nsrc, d->KH * d->KW); a.bias = d->bias;
  a.B = d->B; a.H = d->H; a.W = d->W; a.KH = d->KH; a.KW = d->KW; a.N = d->N;
  a.PH = d->pad_h1 ? d->pad_h1 - 1 : d->KH / 2; a.PW = d->pad_w1 ? d->pad_w1 - 1 : d->KW / 2;
  if (a.PH < 0 || a.PH >= d->KH || a.PW < 0 || a.PW >= d->KW) return FS_ERR_ARG;
  for (int i = 0; i < 3; ++i) {
    const int j = i < d->ndst ? i : 0;
    a.dst[i] = Dst{d->dst[j], d->dst_bs[j], d->dst_ps[j], d->dst_cs[j], d->dst_n0[j], d->dst_acc[j]};
    if (i < d->ndst && !d->dst[i]) return FS_ERR_ARG;
  }
  a.ndst = d->ndst; a.relu = d->relu; a.alpha = d->alpha;
  a.h = d->h; a.ldh = d->ldh; a.z = d->z; a.ldz = d->ldz; a.aux1 = d->aux1; a.ld1 = d->ld1; a.aux2 = d->aux2; a.ld2 = d->ld2;
  a.hid = d->hid;
  a.pre = d->epi == EPI_PLAIN ? nullptr : d->pre; a.ldpre = d->ldpre;
  if (a.pre && (d->ldpre % 4 != 0 || ((uintptr_t)d->pre & 15))) return FS_ERR_ARG;
  for (int i = 0; i < 3; ++i) {
    const bool on = d->epi == EPI_PLAIN && i < d->ndst && d->rmask[i] != nullptr;
    a.rmask[i] = on ? d->rmask[i] : nullptr; a.ldmask[i] = d->ldmask[i]; a.maskc[i] = d->maskc[i];
    if (on && (d->ldmask[i] % 4 != 0 || ((uintptr_t)d->rmask[i] & 15))) return FS_ERR_ARG;
  }
  a.swz = knob.xcd_swizzle;
  if (d->epi == EPI_ZR && (!d->h || !d->aux1 || !d->aux2 || d->hid * 2 != d->N)) return FS_ERR_ARG;
  if (d->epi == EPI_Q && (!d->h || !d->z || !d->aux1)) return FS_ERR_ARG;
  if (d->epi != EPI_PLAIN && d->epi != EPI_ZR && d->epi != EPI_Q) return FS_ERR_ARG;
  if (knob.conv_patch && knob.conv_patch64 && knob.conv_split == 1 && d->wpk_split && d->epi == EPI_PLAIN && d->KH == 3 && d->KW == 3 &&
      d->N > 32 && d->N <= 64 && (int64_t)d->B * d->H * d->W >= knob.conv_patch_min_m) {
    ConvArgs p = a;
    p.wpk = d->wpk_split;
    attach_stats(p, want_stats);
    const int rc = launch_conv_patch(p, d->epi, stream);
    if (rc >= 0) { t_stat.done = want_stats; return rc; }
  }
  if (knob.conv_halo && knob.conv_split == 1 && d->wpk_frag && d->epi == EPI_PLAIN && d->nsrc == 1 && d->KH == 3 && d->KW == 3 &&
      a.PH == 1 && a.PW == 1 &&
      d->srcC[0] % 4 == 0 && d->srcC[0] > 32 && d->srcC[0] <= 64 && d->N <= 128 && d->N > 32 && d->ndst == 1 &&
      d->dst_cs[0] == 1 && d->dst_n0[0] == 0 && !(d->dst_acc[0] && d->relu) && !a.rmask[0] && d->alpha == 1.0f &&
      (int64_t)d->B * d->H * d->W >= knob.conv_halo_min_m && (int64_t)d->H * d->W * d->srcld[0] * 4 < 0x7fffffff) {
    HaloArgs h{d->src[0], d->srcld[0], d->srcC[0], reinterpret_cast<const char*>(d->wpk_frag), d->bias,
               d->dst[0], d->dst_bs[0], d->dst_ps[0], d->N, d->B, d->H, d->W, d->relu, d->dst_acc[0], nullptr, nullptr, 0};
    // Measured (scripts/conv_micro.py, halo on / off): 64 -> 64 at 8x220x512 238 vs 442 us.  With three or four channel
    // groups the patch takes 78 / 104 KB of LDS, one or two 4-wave workgroups per CU, and the kernel loses to the implicit
    // GEMM (96 -> 96 at 8x110x256: 249 vs 165 us; 128 -> 128 at 8x55x128: 93 vs 65 us), so only two-group layers come here.
    attach_stats(h, want_stats);
    t_stat.done = want_stats;
    t_route[0] = d->N > 64 ? 21 : 20;
    return d->N > 64 ? launch_halo<2, 2>(h, stream) : launch_halo<2, 1>(h, stream);
  }
  if (d->N <= 32 && d->epi == EPI_PLAIN) return launch_conv<Cfg32>(a, d->epi, stream);
  // 33..64 outputs: half of a 64x128 split tile is padding, still ~2x faster than the exact 64-wide kernel
  if (d->N <= 64 && d->epi == EPI_PLAIN && !(knob.conv_split && d->wpk_split && knob.conv_buf)) return launch_conv<Cfg64>(a, d->epi, stream);
  // one workgroup per CU is not enough to keep the matrix pipe busy: when the 128x128 grid has
  // fewer than ~2 workgroups per CU, halve the tile height
  const int M = d->B * d->H * d->W;
  if (knob.conv_split && d->wpk_split && d->N > 32) {
    a.wpk = d->wpk_split;
    // 64x128 tiles with the buffer-addressed loaders and the branch-free k-loop are the fastest variant on every
    // update-block shape at M = 28160 (scripts/conv_micro.py: zr 129 us, hd 142 us, q 65 us, m2 61 us, c1 41 us;
    // the 128x128 kernel needs 131 / 157 / 87 / 78 / 45 us); 128x128 stays selectable (key 3 = 4) and is the
    // fallback for shapes the k-tile table cannot describe.
    const bool narrow = knob.conv_buf != 0 || (int64_t)ceil_div(d->N, 128) * ceil_div(M, 128) < 400;
    if (knob.conv_patch && knob.conv_split == 1 && d->KH * d->KW > 1 && d->N > 64 && M >= knob.conv_patch_min_m) {
      ConvArgs p = a;
      attach_stats(p, want_stats);
      const int rc = launch_conv_patch(p, d->epi, stream);
      if (rc >= 0) { t_stat.done = want_stats; return rc; }
    }
    if (knob.conv_split == 5 || (knob.conv_split == 1 && knob.conv_n256 && d->N >= 256 &&
                              ceil_div(d->N, 256) * 256 <= ceil_div(d->N, 128) * 128))
      return launch_conv_split<SCfgN256>(a, d->epi, stream);
    if (knob.conv_split == 1 && knob.conv_n64 && d->N <= 64 && d->epi == EPI_PLAIN && M >= knob.conv_n64_min_m) {
      const int rc = launch_conv_split_plain<SCfg256N64>(a, stream);
      if (rc >= 0) return rc;
    }
    // eight-wave 128x128 tiles where they fill the machine in one round (N >= 256 at M ~ 28 K): key 13
    // sixteen-wave 256x128 tiles: a further 3-6 % on the 192..512-output layers (zr 93 -> 87 us), slower on m2 (N = 576)
    if (knob.conv_split == 1 && ((knob.conv_w8 == 1 && d->N >= 192 && d->N <= 512 && M >= 16384) || knob.conv_w8 == 2) && d->N >= 192) {
      const int rc = launch_conv_split<SCfg256W16>(a, d->epi, stream);
      if (rc >= 0) return rc;
    }
    if (knob.conv_w8 && knob.conv_split == 1 && (int64_t)ceil_div(d->N, 128) * ceil_div(M, 128) >= knob.conv_w8_min) {
      const int rc = launch_conv_split<SCfg128W8>(a, d->epi, stream);
      if (rc >= 0) return rc;
    }
    if (knob.conv_split == 3) return launch_conv_split<SCfgM64>(a, d->epi, stream);
    if (knob.conv_split == 4) return launch_conv_split<SCfg128>(a, d->epi, stream);
    return narrow ? launch_conv_split<SCfgM64>(a, d->epi, stream) : launch_conv_split<SCfg128>(a, d->epi, stream);
  }
  if (knob.conv_tile == 3) return launch_conv<Cfg6464>(a, d->epi, stream);
  if (knob.conv_tile == 4) return launch_conv<Cfg6464K16>(a, d->epi, stream);
  if (knob.conv_tile == 5) return launch_conv<CfgM64K16>(a, d->epi, stream);
  if (knob.conv_tile == 2) return launch_conv<CfgM64>(a, d->epi, stream);
  if (knob.conv_tile == 1) return launch_conv<Cfg128>(a, d->epi, stream);
  if ((int64_t)ceil_div(d->N, 128) * ceil_div(M, 128) < 512) return launch_conv<CfgM64>(a, d->epi, stream);
  return launch_conv<Cfg128>(a, d->epi, stream);
}

// fsraft_conv_forward whose kernel, where it can, also accumulates the per-image column sums of its result and of its squares
// (the statistics the InstanceNorm behind the convolution needs: fsraft_inorm_relu_cl_fwd with have_sums = 1 then skips its
// own pass over the tensor).  sum, sq: [B * slots][N] fp32, ZERO on entry (the rows of one image are added up by the consumer);
// *done = 1 if the launch carried them, 0 if the caller has to compute them (kernels whose tiles straddle images, epilogues
// with a bias / ReLU / mask).
extern "C" int fsraft_conv_forward_stats(const fsraft_conv_desc* d, float* sum, float* sq, int slots, int* done, hipStream_t stream) {
  if (!sum || !sq || slots < 1 || !done) return FS_ERR_ARG;
  t_stat = StatReq{sum, sq, slots, false};
  const int rc = fsraft_conv_forward(d, stream);
  *done = (rc == FS_OK && t_stat.done) ? 1 : 0;
  t_stat = StatReq{nullptr, nullptr, 0, false};
  return rc;
}


// The split-K route of the small-M convolutions needs a scratch buffer; the ABI allocates nothing, so the binding hands one
// over (and keeps it alive): per call in fsraft_conv_desc.ws, or -- this entry point -- for every later call of the CALLING THREAD
// whose descriptor carries none.  Calls that enqueue convolutions on DIFFERENT streams concurrently must not share a buffer.
extern "C" int fsraft_conv_workspace(float* ws, int64_t floats) {
  if (ws && (((uintptr_t)ws & 15) || floats < 0)) return FS_ERR_ARG;
  t_reg_ws = ws;
  t_reg_ws_floats = ws ? floats : 0;
  return FS_OK;
}
