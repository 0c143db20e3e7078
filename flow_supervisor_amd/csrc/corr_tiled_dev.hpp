// Device pieces shared by the kernels that read lookup windows out of the tiled-row volume (corr_layout.hpp): the forward
// lookup and the gradient-volume kernels of corr_tiled.hip, and the coordinate gradient of corr_dcoords.hip.  The query
// position, the per-level window origin and the fixed-order wave sum also serve the coordinate gradient of the
// memory-efficient lookup (altcorr_dcoords.hip), which reads feature rows instead of volume windows.
#pragma once
#include "corr_layout.hpp"

namespace {

struct Coords {
  const float* p;
  int64_t bs, cs, ps;
};
// The query position is either given (coords) or coords = pixel grid + flow: grid_w > 0 names the image width and the
// tensor holds the FLOW, so that the RAFT loop never materialises coords1 = coords0 + flow (raft.py:121-131).
__device__ __forceinline__ void query_xy(const Coords& c, int b, int pix, int grid_w, float& cx, float& cy) {
  cx = gload1(c.p + b * c.bs + pix * c.ps);
  cy = gload1(c.p + b * c.bs + c.cs + pix * c.ps);
  if (grid_w > 0) { cx += (float)(pix % grid_w); cy += (float)(pix / grid_w); }
}

template <int R>
struct TL {
  static constexpr int N1 = 2 * R + 1, WIN = 2 * R + 2, N2 = N1 * N1;
  static constexpr int RP = 20;             // region row pitch (floats): 16-byte aligned rows, <= 3-way bank conflicts in the blend
  static constexpr int REGION = 16 * RP;    // one level's 16x16-cell region
  static constexpr int ROUNDS = (N2 + 63) / 64;
};

struct LevelQ {      // one (query, level): integer window origin and bilinear weights
  int wx0, wy0;
  float fx, fy;
};

__device__ __forceinline__ LevelQ level_query(float cx, float cy, int l, int R) {
  const float s = 1.0f / (float)(1 << l);
  cx *= s; cy *= s;
  // anything this far out has an all-zero window; the clamp keeps floor->int defined (also for NaN)
  cx = (cx > -30000.f && cx < 30000.f) ? cx : -30000.f;
  cy = (cy > -30000.f && cy < 30000.f) ? cy : -30000.f;
  const float flx = floorf(cx), fly = floorf(cy);
  return LevelQ{(int)flx - R, (int)fly - R, cx - flx, cy - fly};
}

__device__ __forceinline__ void wave_lds_sync() {
  // LDS operations of one wave execute in order; this only stops the compiler from moving them across
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

struct Grad2 {      // where dcoords element (b, c, pix) goes
  float* p;
  int64_t bs, cs, ps;
};

// sum over the 64 lanes, the same value in every lane, always added in the same order: quads, halves of a row, rows (DPP), then
// the four rows of 16 lanes left to right
template <int CTRL>
__device__ __forceinline__ float dpp_move(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float wave_sum_fixed(float v) {
  v += dpp_move<0xB1>(v);       // quad_perm [1, 0, 3, 2]
  v += dpp_move<0x4E>(v);       // quad_perm [2, 3, 0, 1]
  v += dpp_move<0x141>(v);      // row_half_mirror
  v += dpp_move<0x140>(v);      // row_mirror
  const int iv = __builtin_bit_cast(int, v);
  const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 0)), r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 16));
  const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 32)), r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 48));
  return ((r0 + r1) + r2) + r3;
}

// A wave walks through QW consecutive queries.  The chain of one query is coords -> window origin -> region loads -> LDS ->
// blends -> stores, every link waiting for the one before, and 32 resident waves per CU do not hide it (measured: 2.5 TB/s
// algorithmic with the queries handled one after the other).  So the chain is software-pipelined over the queries of a wave:
// all QW coordinate pairs are fetched first (wave-uniform addresses), and the region loads of query k + 1 are issued before
// the blends of query k, i.e. two queries' regions (up to 8 KB per wave) are in flight while one is being consumed.
// The loads are buffer loads (base = the query's row, wave-uniform): a lane whose 16 bytes the window does not touch gets bit
// 31 in its offset, fails the range check and reads zeros -- no branch around the load, so the loop body is straight-line
// code and the compiler can count the loads in flight (`s_waitcnt vmcnt(N)`, not 0).
struct LevelGeo { int off, tw, h, w; };        // per-level constants of the layout, in SGPRs

// (only the loaded tile rows are carried from the issue to the blends; the window origin, the fractions and the pad mask of a level
//  are recomputed from the query position at the blend -- 36 registers per query in flight held the kernel at four waves per SIMD,
//  i.e. two rounds of waves for the 27 per CU a four-pair lookup needs)
template <int R>
struct LookupLoad {
  f32x4 v[4];
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t row_rsrc(const float* row, unsigned bytes) {
  const uint64_t u = reinterpret_cast<uint64_t>(row);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
  return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>((uint64_t)hi << 32 | lo), 0, bytes, 0x00020000);
}

template <int R, int AUX = 0>      // AUX: cache policy of the window loads (0 plain, 2 nt, 16 sc1, 18 both: fsraft_set_lookup_policy)
__device__ __forceinline__ void lookup_issue(LookupLoad<R>& ld, const float* __restrict__ row, unsigned row_bytes, const LevelGeo (&g)[4],
                                             int nlev, float cx, float cy, int tsx, int tsy, int r) {
  using S = TL<R>;
  const __amdgpu_buffer_rsrc_t rs = row_rsrc(row, row_bytes);
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    const LevelQ lq = level_query(cx, cy, l, R);
    const int tx = (lq.wx0 >> 2) + tsx, ty = (lq.wy0 >> 2) + tsy;     // >> on negatives = floor division
    const int y = 4 * ty + r, x = 4 * tx;
    const bool need = l < nlev && tx >= 0 && tx < g[l].tw && ty >= 0 && y < g[l].h && y >= lq.wy0 && y < lq.wy0 + S::WIN &&
                      x + 3 >= lq.wx0 && x < lq.wx0 + S::WIN;
    const unsigned voff = need ? (unsigned)(g[l].off + (ty * g[l].tw + tx) * 16 + r * 4) * 4u : 0x80000000u;
    ld.v[l] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, 0, AUX));
  }
}

}  // namespace
