// What the convolution translation units share (conv_igemm.hip: forward / data gradient, conv_wgrad.hip: weight gradient,
// conv_pack.hip: weight packers, conv_tuning.hip: configuration): argument structs, tile configurations, the knob struct,
// the route record and the small host helpers of the entry points.
#pragma once
#include "gemm_core.hpp"
#include "gemm_core_split.hpp"
#include "gemm_rec.hpp"
#include <cstddef>
#include <type_traits>

// Process-wide knobs of the convolution family: fsraft_set_tuning / fsraft_get_tuning (include/fsraft_tuning.h) reach every
// member through the one table of conv_tuning.hip.  The member initialisers are the defaults; they are written nowhere else.
struct ConvKnobs {
  int conv_tile = 0;    // 0 auto, 1 force 128x128, 2 force 64x128, 3 force 64x64   (fsraft_set_tuning key 0)
  int wgrad_tile = 0;   // 0 auto (128x128), 3 force 64x64                           (key 1)
  int wgrad_blocks = 512;   // target workgroup count of the pixel split (key 2); measured 256: 12.9, 512: 11.5, 1024: 12.9, 2048: 14.1 ms/step
  int conv_split = 1;   // 0: exact fp32 MFMA; 1: split-bf16 (3-MFMA) core for forward / data-gradient convolutions (key 3)
  int wgrad_split = 2;  // 0: exact fp32; 1/2: split-bf16 weight gradient (double / single LDS image)   (key 4)
  int conv_buf = 1;     // buffer-addressed loaders in the split conv kernels (key 5): 0 never, 1 on 64-row tiles, 2 always
  int xcd_swizzle = 0;  // experiment switch (key 7)
  int wgrad_buf = 1;    // buffer-addressed loaders + pixel mask in the split weight-gradient kernel (key 8)
  int conv_n256 = 0;    // 64x256 tiles for layers whose N fills them (key 9); measured slower than 64x128 (zr 139 vs 119 us, hd 182 vs 125 us)
  int wgrad_multi = 1;  // one weight-gradient launch per layer per step over all stashed iterations (key 10)
  int wgrad_blocks_multi = 2048;   // workgroup target of the multi-segment launch (key 11); measured 512: 9.0, 1024: 8.5, 2048: 8.35 ms/step
  int conv_uniform = 1;   // uniform-pitch k-tile table when the sources allow it (key 12)
  int conv_w8 = 1;        // 512-thread 128x128 tiles for wide layers (key 13); conv_w8_min: minimum workgroup count (key 14)
  int conv_w8_min = 64;      // (measured faster than 64x128 four-wave tiles on every update-block shape, N = 64 .. 576)
  // Keys 2 / 11 size the pixel split of the 128x128 tile.  The wide tiles (256x256, 128x256; fsraft_set_wgrad_wide, no key) take
  // at most that many splits, at most 512 workgroups and whole rounds of 256 (one workgroup per CU), and run by default where that
  // grid has >= 192 workgroups of >= 16 k-tiles.  Measured, same process, hipGraph, us per launch, 128 tile -> wide (profiles/wgrad_wide_tiles.txt):
  //   1x5 / 5x1 128+128->256 x12  719 -> 617 / 747 -> 641     1x5 / 5x1 128+128->128 x12  382 -> 361 / 397 -> 375
  //   2x2 256->96  232 -> 198 (8x110x256), 127 -> 105 (4x110x256)     2x2 384->128  111 -> 95 (8x55x128), 66 -> 63 (4x55x128)
  //   lost, grid of 52-104 workgroups: 1x1 256->576  491 -> 748, 1x1 324->256  323 -> 491, single five-tap 67 -> 93, 48 -> 66
  int wgrad_w8 = 0;       // 512-thread workgroups in the multi-segment weight gradient (key 15); measured slower (7.96 vs 7.32 ms/step): its grid is large already
  int wgrad_pack = 1;          // few-channel single-source layers on conv_wgrad_pack_kernel (key 16)
  int wgrad_blocks_pack = 1024;   // its workgroup target (key 17)
  int conv_n64 = 1;            // 256x64 tiles for N <= 64 (key 18) once M reaches conv_n64_min_m (key 19)
  int conv_n64_min_m = 65536;
  int conv_halo = 1;           // resident-patch 3x3 kernel for few-channel layers at large M (key 20; threshold key 21)
  int conv_halo_min_m = 65536;
  int wgrad_xcd = 1;           // XCD-aware workgroup order in the multi-segment weight gradient (key 22; 2: the few-channel kernel too).
                               // Measured: 10.73 -> 9.72 ms/step of weight-gradient time (15 K-tiles re-read each dY tile)
  int conv_patch = 1;      // resident-patch, channel-streaming kernel for the 3x3 / 1x5 / 5x1 layers (conv_patch.inc, key 26; 2: 128-pixel tiles too)
  int wgrad_patch = 1;         // resident-pixel-block weight gradient for the 3x3 / 1x5 / 5x1 layers (wgrad_patch.inc, key 27)
  int conv_patch64 = 1;    // ... also for the 3x3 layers with 33..64 outputs (64-column tiles; key 28; 2: 128-pixel tiles)
  int wgrad_patch1 = 8192;     // single-segment 3x3 layers with at least this many pixels on the resident-block kernel (key 29; 0: never)
  int conv_patch_min_m = 8192;   // ... from this many pixels on (key 31)
  int conv_ksplit = -1;          // -1 auto (small grids only), 0 / 1 off, >= 2 forced slice count (fsraft_set_tuning key 32)
};
// (both defined in conv_tuning.hip; hidden: the library exports its C ABI only)
__attribute__((visibility("hidden"))) extern ConvKnobs knob;
// Route attestation (fsraft_conv_last_route, include/fsraft_tuning.h): every launch site records which kernel the calling
// thread's last forward / data-gradient call (t_route[0]) and weight-gradient call (t_route[1]) ran.  Codes as in the header.
// (__thread, not thread_local: a thread_local declared extern is reached through an init wrapper that tests a weak symbol,
// which position-independent code cannot test when the symbol is hidden)
__attribute__((visibility("hidden"))) extern __thread int t_route[2];

namespace {
struct Src { const float* p; int C; int ld; };
struct Dst { float* p; int64_t bs, ps, cs; int n0; int accumulate; };   // channels [n0, next n0)

struct ConvArgs {
  Src src[3]; int nsrc;
  const float* wpk; int Ktot;
  const float* bias;
  int B, H, W, KH, KW, N;        // N = output channels of this GEMM
  int PH, PW;                    // tap t reads pixel (y + t / KW - PH, x + t % KW - PW); KH / 2, KW / 2 unless overridden
  Dst dst[3]; int ndst;
  int relu; float alpha;
  // GRU epilogues
  const float* h; int ldh;
  const float* z; int ldz;
  float* aux1; int ld1;          // ZR: r*h     Q: q
  float* aux2; int ld2;          // ZR: r
  int hid;
  const float* pre; int ldpre;   // GRU epilogues: per-pixel addend to the pre-activation, [M][ldpre] (NULL: none)
  // plain epilogue, per destination: ReLU-backward mask.  After scaling / accumulation, column j of the destination
  // range (j < maskc) is zeroed where rmask[m*ldmask + j] <= 0 -- the data gradient of a layer whose input came
  // out of a ReLU leaves the kernel already masked, instead of a separate pass over the tensor.
  const float* rmask[3]; int ldmask[3]; int maskc[3];
  // InstanceNorm statistics of the OUTPUT from the epilogue (kernels whose tiles lie inside one image: conv_patch.inc, the halo
  // kernel): st_sum / st_sq [B * st_slots][N] += column sums of the tile's results and of their squares (fsraft_conv_forward_stats)
  float* st_sum; float* st_sq; int st_slots;
  int swz;                       // 1: XCD-aware workgroup -> tile mapping (see tile_of_block)
  int ksplit;                    // > 1: blockIdx.z owns a slice of the k-tiles and parks its RAW partial tile in a workspace (dst[0],
                                 // rows z * M + m): the first pass of the split-K route for small M (conv_finish_kernel is the second)
};

// Arguments of the buffer-addressed split kernels: ConvArgs plus one dword per k-tile, built on the host, that
// says where the tile comes from -- bits 0..15: SGPR byte offset / 16 of (tap shift, channel chunk) inside the
// source, 16..19: tap, 20..21: source, 22..27: channels left in the source from this chunk (1..32).  The kernel
// reads it with one scalar load; without it the (source, tap, chunk) decode is two integer divisions per k-tile,
// which the compiler can only do on the vector ALU (~50 instructions) even though the values are wave-uniform.
// "Uniform" form (BUF = 2), used when all sources share one row pitch and lie within 2 GiB of each other: two dwords
// per k-tile -- the complete SGPR byte offset from ONE base pointer (source delta + tap shift + channel chunk), and
// tap | channels-left << 4.  One descriptor and one pitch for the whole k-loop: the per-tile scalar work shrinks from
// ~30 instructions (source selects, 64-bit base arithmetic) to a two-dword load and two bit-field extracts.
constexpr int KTAB_MAX = 512;
struct ConvArgsT {
  ConvArgs a;
  const float* ubase; int uld;   // uniform form: biased base pointer and the common pitch (floats)
  unsigned ktab[KTAB_MAX];
};

enum { EPI_PLAIN = 0, EPI_ZR = 2, EPI_Q = 3 };

// ---- helpers of the buffer-addressed loaders (BufConvALoader in conv_igemm.hip, BufDyLoader in conv_wgrad.hip) ----
#define FS_RSRC_FLAGS 0x00020000            // raw buffer, 32-bit data format (gfx9 family word 3)
#define FS_OOB 0x80000000u                  // lane offset that always fails the num_records check

__device__ __forceinline__ unsigned uni(unsigned v) { return __builtin_amdgcn_readfirstlane(v); }
template <class T>
__device__ __forceinline__ const T* uni_ptr(const T* p) {
  const uint64_t u = reinterpret_cast<uint64_t>(p);
  return reinterpret_cast<const T*>((uint64_t)uni((unsigned)(u >> 32)) << 32 | uni((unsigned)u));
}
// p and bytes must be wave-uniform; the readfirstlanes state that (a descriptor the compiler believes to be
// divergent is wrapped in a waterfall loop around every load).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p, unsigned bytes) {
  const uint64_t u = reinterpret_cast<uint64_t>(p);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
  void* q = reinterpret_cast<void*>((uint64_t)hi << 32 | lo);
  return __builtin_amdgcn_make_buffer_rsrc(q, 0, __builtin_amdgcn_readfirstlane(bytes), FS_RSRC_FLAGS);
}

using SWCfg128 = SplitTnCfg<128, 128, 2, 2, 2>;
using SWCfg128S = SplitTnCfg<128, 128, 2, 2, 1>;
using SWCfg128W8 = SplitTnCfg<128, 128, 2, 4, 1, 512>;   // eight waves per workgroup (multi-segment launches)
using SWCfgPack = SplitTnCfg<64, 192, 2, 2, 1>;
// wide per-tap tiles (fsraft_set_wgrad_wide): eight waves, two LDS images, one workgroup per CU.  A 256-column x tile is two
// 128-column groups of the packed-K layout (two taps or two sources), each loaded by one half of the workgroup.
using SWCfgW256 = SplitTnCfg<256, 256, 2, 4, 2, 512>;      // 64 KB staged per k-tile for four times the MFMAs of the 128x128 tile's 32 KB
using SWCfgW128 = SplitTnCfg<128, 256, 2, 4, 2, 512>;      // Cout <= 128 (the q layers): 0.75 of the bytes per MFMA
using Cfg128 = GemmCfg<128, 128, 32, 2, 2, 2, 2>;
using Cfg64 = GemmCfg<128, 64, 32, 4, 1, 2, 2>;
using CfgM64 = GemmCfg<64, 128, 32, 1, 4, 2, 2>;     // half-height tile: doubles the workgroup count for narrow N
using Cfg6464 = GemmCfg<64, 64, 32, 2, 2, 2, 2>;     // small tile: 4 workgroups/CU, fine-grained balance over 256 CUs
using WCfg6464 = GemmCfg<64, 64, 32, 2, 2, 0, 0>;
using Cfg6464K16 = GemmCfg<64, 64, 16, 2, 2, 2, 2>;  // 17 KB of LDS: 8 workgroups/CU
using CfgM64K16 = GemmCfg<64, 128, 16, 1, 4, 2, 2>;  // 25 KB: 6 workgroups/CU

using SCfg128 = SplitCfg<128, 128, 2, 2>;
using SCfgN256 = SplitCfg<64, 256, 1, 4, 2, true>;   // 80 KB of LDS: two workgroups per CU; each wave owns 64x64, A rows are read once for N = 256
using SCfg256W16 = SplitCfg<256, 128, 4, 4, 2, true, 1024>;  // sixteen waves, one workgroup per CU
using SCfg128W8 = SplitCfg<128, 128, 2, 4, 2, true, 512>;   // eight waves per workgroup, 66 KB of LDS: two workgroups per CU
using SCfg256N64 = SplitCfg<256, 64, 4, 2, 2, true, 512>;   // N <= 64 layers at large M (encoder layer1, f2): a 128-wide tile would be half empty
using SCfgM64 = SplitCfg<64, 128, 1, 4, 2, true>;    // swizzled 128-byte rows: 48 KB of LDS -> three workgroups per CU
using Cfg32 = GemmCfg<128, 32, 32, 4, 1, 2, 2>;
// weight-gradient tiles: LDS images are filled with float4 rows, so pitches stay multiples of 4
using WCfg128 = GemmCfg<128, 128, 32, 2, 2, 0, 0>;
using WCfg32 = GemmCfg<32, 128, 32, 1, 4, 0, 0>;

// route codes of the implicit-GEMM tiles (t_route above)
template <class Cfg>
constexpr int route_gemm() {
  return std::is_same_v<Cfg, Cfg32> ? 1 : std::is_same_v<Cfg, Cfg64> ? 2 : std::is_same_v<Cfg, CfgM64> ? 3 :
         std::is_same_v<Cfg, Cfg128> ? 4 : std::is_same_v<Cfg, Cfg6464> ? 5 : std::is_same_v<Cfg, Cfg6464K16> ? 6 :
         std::is_same_v<Cfg, CfgM64K16> ? 7 : 0;
}
template <class Cfg>
constexpr int route_split() {
  return std::is_same_v<Cfg, SCfgN256> ? 30 : std::is_same_v<Cfg, SCfg256N64> ? 31 : std::is_same_v<Cfg, SCfg256W16> ? 32 :
         std::is_same_v<Cfg, SCfg128W8> ? 33 : std::is_same_v<Cfg, SCfgM64> ? 34 : std::is_same_v<Cfg, SCfg128> ? 35 : 0;
}

int conv_ktot(const int* C, int nsrc, int taps) {
  int k = 0;
  for (int s = 0; s < nsrc; ++s) k += taps * (((C[s] + 31) / 32) * 32);
  return k;
}

// ---- host helpers of the entry points ----
// The run-time epilogue kind as a template argument: f(std::integral_constant<int, EPI>) with EPI = epi.
template <class F>
void with_epi(int epi, F&& f) {
  if (epi == EPI_PLAIN) f(std::integral_constant<int, EPI_PLAIN>{});
  else if (epi == EPI_ZR) f(std::integral_constant<int, EPI_ZR>{});
  else f(std::integral_constant<int, EPI_Q>{});
}

// The three source slots of a kernel from the caller's nsrc (slots beyond nsrc: source 0 with no channels); false on a
// null pointer or a pitch that is no multiple of 4.
bool fill_srcs(Src (&dst)[3], const float* const* p, const int* C, const int* ld, int nsrc) {
  for (int s = 0; s < 3; ++s) {
    dst[s] = Src{s < nsrc ? p[s] : p[0], s < nsrc ? C[s] : 0, s < nsrc ? ld[s] : 4};
    if (s < nsrc && (!p[s] || ld[s] % 4 != 0)) return false;
  }
  return true;
}

// Pixels per split of a weight-gradient launch: about `target` workgroups over `tiles` tiles of M pixels; at least 256, at most
// what the kernel's pixel mask of `words` words holds (two words spare), a multiple of 32.
int64_t wgrad_chunk(int target, int64_t tiles, int64_t M, int words) {
  int64_t want = (target + tiles - 1) / tiles;
  if (want < 1) want = 1;
  int64_t chunk = (M + want - 1) / want;
  if (chunk < 256) chunk = 256;
  if (chunk > 32 * (words - 2)) chunk = 32 * (words - 2);
  return (chunk + 31) / 32 * 32;
}

}  // namespace
