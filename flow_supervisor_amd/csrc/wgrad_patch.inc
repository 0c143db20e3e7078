// Weight gradient of the 3x3 / 1x5 / 5x1 layers over RESIDENT PIXEL BLOCKS: included by conv_wgrad.hip (WgradArgsM, loaders'
// helpers, tr_frag, stage_convert_kmajor).
//
//     dW[co][tap][ci] += sum over the stashed iterations t and pixels p of dY_t[p][co] * X_t[p + shift(tap)][ci]
//
// The kernel above it gives every (tap, 128-channel tile) its own workgroup: each fetches, converts and stores its own copy of
// the dY tile and the tap-shifted X tile -- 32 KB per 32-pixel k-tile and 96 MFMAs per wave -- which is 2.6 times what a CU can
// stage while its matrix pipe is busy (~38 GB/s per CU, DESIGN.md 3.1), so the family runs fetch-bound at 0.35 of its roof.
// Here a workgroup owns a (64 output channels, 32 input channels) pair of ALL taps and walks over blocks of 4 x 32 pixels:
// per block it stages dY (128 pixels x 64 channels) and the X patch INCLUDING the halo the taps reach (6 x 34, 4 x 36 or
// 8 x 32 pixels) once, k-major, as bf16 hi / lo planes, and runs every tap out of them: tap (dy, dx) is the same X image
// read (dy, dx) pixels further on (both operands through ds_read_b64_tr_b16).  Bytes staged per MFMA drop by the number of
// taps over the halo factor.  The next block's data is in flight (registers) while this one is multiplied; the sum over all
// blocks of a workgroup stays in registers (TAPS x 64 x 32 over four waves) and leaves as one round of atomics.
//
// Four waves: 2 (co half) x 2 (tap half).  The planes take 60-82 KB, so TWO workgroups share a CU: inside a workgroup the
// phases are serial (fetch addresses and conversion are VALU work, the multiply is MFMA + LDS reads, a barrier in between),
// and a first version with one 8-wave workgroup per CU (64 x 64 pairs) measured exactly the sum of its phases -- 3.2 us of
// MFMA in 7.1 us per block.  Two independent workgroups drift apart and one converts while the other multiplies.
namespace {

constexpr int WP_TH = 4, WP_TW = 32, WP_NT = 256, WP_CO = 64, WP_CI = 32;
constexpr int WP_SLOTS = 64;                                 // workgroups per XCD: 32 CUs x 2
constexpr int WP_DYPITCH = WP_CO * 2 + 64;                   // bytes per k row of the dY planes: 64 bf16 + pad (conflict-free transposed reads)
constexpr int WP_XPITCH = WP_CI * 2;                         // X planes: 32 bf16, no pad (the four rows of a read block cover the 256-byte bank row)
constexpr int WP_DYROWS = WP_TH * WP_TW;                     // 128 pixels per block

struct WgradPatchArgs {
  WgradArgsM m;                       // tensors, segment tables (a.dy / a.src: segment 0), dwpk, dbias, shapes
  int nblk;                           // pixel blocks: nseg * B * ty * tx
  int ty, tx;
  int npair;                          // (co tile, source chunk) pairs
  int cot;                            // co tiles
  unsigned ptab[48];                  // per source chunk: src | chunk32 << 2 | kofs << 8 (first packed-K column of tap 0 of that chunk)
  int cpad[3];
};

template <int KH, int KW>
__global__ __launch_bounds__(WP_NT, 2) void conv_wgrad_patch_kernel(const WgradPatchArgs args) {
  constexpr int TAPS = KH * KW, PHh = KH / 2, PWh = KW / 2;
  constexpr int PH = WP_TH + KH - 1, PW = WP_TW + KW - 1, XROWS = PH * PW;
  constexpr int TA = (TAPS + 1) / 2;                        // taps of tap half 0 (half 1: TAPS - TA)
  constexpr int DY_PLANE = WP_DYROWS * WP_DYPITCH, X_PLANE = XROWS * WP_XPITCH;
  constexpr int NCH_DY = WP_DYROWS * (WP_CO / 4) / WP_NT;   // 16-byte chunks per thread: 8
  constexpr int NCH_X = (XROWS * (WP_CI / 4) + WP_NT - 1) / WP_NT;
  __shared__ __attribute__((aligned(16))) char lds[2 * DY_PLANE + 2 * X_PLANE];
  char* dyh = lds;                    // [128 k][64 co] bf16 hi, lo at + DY_PLANE
  char* xh = lds + 2 * DY_PLANE;      // [XROWS k][32 ci] bf16 hi, lo at + X_PLANE
  const WgradArgs& a = args.m.a;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int mi = wave & 1, th = wave >> 1;                  // co half, tap half
  const int lh = lane >> 5, gb = (lane >> 4) & 1, q = (lane & 15) >> 2, p4 = lane & 3, l31 = lane & 31;

  // ---- work distribution (see launch_wgrad_patch): this workgroup's items [it0, it1) of the item space
  //      item = pair * len + (block - base); a run of items of one pair is a "segment" with its own accumulators
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;   // WP_SLOTS slots per XCD, two per CU
  const int P = args.npair, f = WP_SLOTS / P, nfull = f * P, left = WP_SLOTS - nfull;
  const int span0 = (int)((int64_t)xcd * args.nblk / 8), span1 = (int)((int64_t)(xcd + 1) * args.nblk / 8), span = span1 - span0;
  const int A = f == 0 ? 0 : left ? (int)(((int64_t)span * P + WP_SLOTS - 1) / WP_SLOTS) : (span + f - 1) / f;
  int base, len, it0, it1;
  if (slot < nfull) {                 // lockstep part: sub-range slot / P of the span, pair slot % P
    base = span0 + (slot / P) * A;
    len = span1 - base < A ? span1 - base : A;
    if (len < 0) len = 0;
    it0 = (slot % P) * len; it1 = it0 + len;
  } else {                            // the slots left over share the rest of the span, all pairs, in equal runs of items
    base = span0 + f * A;
    len = span1 - base > 0 ? span1 - base : 0;
    const int total = P * len, n = (total + left - 1) / left;
    it0 = (slot - nfull) * n; it0 = it0 < total ? it0 : total;
    it1 = it0 + n < total ? it0 + n : total;
  }
  const auto* karg = (const char __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr();
  typedef const float* fptr;
  const auto* dytab = (const fptr __attribute__((address_space(4)))*)(karg + offsetof(WgradPatchArgs, m) + offsetof(WgradArgsM, dys));
  const fptr __attribute__((address_space(4)))* xtab = nullptr;
  int co0 = 0, ci0 = 0, kofs0 = 0, cpad = 32;
  bool want_bias = false;
  int xn = 4;                         // channels of this thread's float4 that exist in the source

  // ---- this thread's chunks.  dY chunk c: pixel k = tid / 16 + 16 c of the block (line c / 2, column tid / 16 + 16 (c & 1)),
  //      channels 4 (tid % 16) ..; X chunk c: patch row tid / 8 + 32 c, channels 4 (tid % 8) ..  Everything that does not
  //      depend on the block is worked out once per segment: the fetch is VALU work nothing hides inside a workgroup.
  const int k0 = threadIdx.x >> 4, dyc4 = (threadIdx.x & 15) * 4, xc4 = (threadIdx.x & 7) * 4;
  const unsigned ldy4 = (unsigned)a.ldy * 4u;
  unsigned dyoff = FS_OOB;            // byte offset of (pixel k0 of the block's first line, channel dyc4), or out of bounds: column beyond Cout
  unsigned ldx4 = 0;
  bool xcol = false;                  // this thread's 4 channels exist in the source
  float rdy[NCH_DY * 4], rx[NCH_X * 4];
  float colsum[4];
  auto fetch = [&](int blk) {         // blk is wave-uniform
    const int tx = blk % args.tx, r1 = blk / args.tx, ty = r1 % args.ty, r2 = r1 / args.ty, b = r2 % a.B, seg = r2 / a.B;
    const int y0 = ty * WP_TH, x0 = tx * WP_TW;
    const __amdgpu_buffer_rsrc_t rd = make_rsrc(uni_ptr(dytab[seg]) + co0, 0x7fffffffu);
    const __amdgpu_buffer_rsrc_t rxs = make_rsrc(uni_ptr(xtab[seg]) + ci0, 0x7fffffffu);
    const unsigned pix0 = uni((unsigned)((b * a.H + y0) * a.W + x0));
    const bool okx0 = x0 + k0 < a.W, okx1 = x0 + k0 + 16 < a.W;
#pragma unroll
    for (int c = 0; c < NCH_DY; ++c) {
      const unsigned sb = y0 + (c >> 1) < a.H ? (pix0 + (unsigned)((c >> 1) * a.W + 16 * (c & 1))) * ldy4 : FS_OOB;   // scalar
      const unsigned voff = ((c & 1) ? okx1 : okx0) ? sb + dyoff : FS_OOB;
      const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rd, voff, 0, 0));
      rdy[4 * c] = v[0]; rdy[4 * c + 1] = v[1]; rdy[4 * c + 2] = v[2]; rdy[4 * c + 3] = v[3];
    }
    const int ys = y0 - PHh, xs = x0 - PWh;
    const unsigned xb = pix0 - (unsigned)(PHh * a.W + PWh);       // (24-bit multiplies: launch_wgrad_patch checks the sizes)
#pragma unroll
    for (int c = 0; c < NCH_X; ++c) {
      const unsigned row = (threadIdx.x >> 3) + 32u * c, pyv = __umul24(row, (1u << 20) / PW + 1u) >> 20, pxv = row - pyv * PW;   // row / PW (exact for row < 4096)
      const bool ok = xcol && ((c + 1) * 32 <= XROWS || row < XROWS) && (unsigned)(ys + (int)pyv) < (unsigned)a.H &&
                      (unsigned)(xs + (int)pxv) < (unsigned)a.W;
      const unsigned pix = xb + __umul24(pyv, (unsigned)a.W) + pxv;
      const unsigned voff = ok ? __umul24(pix, ldx4) + (unsigned)xc4 * 4u : FS_OOB;
      const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rxs, voff, 0, 0));
      rx[4 * c] = v[0]; rx[4 * c + 1] = v[1]; rx[4 * c + 2] = v[2]; rx[4 * c + 3] = v[3];
    }
    if (xn < 4) {                     // the source ends inside this thread's 4 channels: what follows belongs to somebody else
#pragma unroll
      for (int c = 0; c < NCH_X; ++c)
#pragma unroll
        for (int i = 1; i < 4; ++i)
          if (i >= xn) rx[4 * c + i] = 0.f;
    }
  };
  // (LDS store addresses: one register per plane pair plus immediates -- written out because the compiler does not see that
  //  (tid + 256 c) / 16 is tid / 16 + 16 c, keeps one address per chunk live across the block loop and spills)
  char* const dyst = dyh + k0 * WP_DYPITCH + (threadIdx.x & 15) * 8;
  char* const xst = xh + (threadIdx.x >> 3) * WP_XPITCH + (threadIdx.x & 7) * 8;
  auto put = [](char* p, const float* r, int plane) {
    uint2 hi, lo;
    split4(r, hi, lo);
    *reinterpret_cast<uint2*>(p) = hi;
    *reinterpret_cast<uint2*>(p + plane) = lo;
  };
  auto stage = [&]() {
#pragma unroll
    for (int c = 0; c < NCH_DY; ++c) {
      put(dyst + c * 16 * WP_DYPITCH, rdy + 4 * c, DY_PLANE);
#pragma unroll
      for (int i = 0; i < 4; ++i) colsum[i] += rdy[4 * c + i];
    }
#pragma unroll
    for (int c = 0; c < NCH_X; ++c)
      if ((c + 1) * 32 <= XROWS || (int)(threadIdx.x >> 3) + 32 * c < XROWS) put(xst + c * 32 * WP_XPITCH, rx + 4 * c, X_PLANE);
  };

  f32x16 acc[TA];

  // fragment bases (split_mainloop_tn): lane (lh, gb, q, p4) reads k rows 8 lh + q (+ 4) of a 16-row k-step, columns 16 gb + 4 p4 ..
  const char* Ab = dyh + (8 * lh + q) * WP_DYPITCH + (mi * 32 + 16 * gb + 4 * p4) * 2;
  const char* Bb = xh + (8 * lh + q) * WP_XPITCH + (16 * gb + 4 * p4) * 2;
  // Software pipeline over "units" u = (k-step, tap): the fragments of unit u + 2 and u + 3 are requested while the six MFMAs
  // of units u, u + 1 run (two accumulators take turns, so consecutive MFMAs never depend on each other).  Left to itself the
  // compiler sinks half of the transposed reads to just before their MFMA and the loop runs at LDS latency, not MFMA rate.
  // (Tap half as a template argument of the loop -- immediates instead of the Bt registers, the centre tap split between the
  //  halves instead of a dropped slot -- doubles the code and made the register allocator spill the fetch registers.)
  const char* Bt[TA];                 // tap t of this wave's half: patch row offset of its shift (th is wave-uniform)
#pragma unroll
  for (int t = 0; t < TA; ++t) {
    const int tap = th * TA + t < TAPS ? th * TA + t : TAPS - 1;   // (a missing last tap re-reads the previous one and is dropped)
    Bt[t] = Bb + ((tap / KW) * PW + tap % KW) * WP_XPITCH;
  }
  constexpr int NU = (WP_DYROWS / 16) * TA;
  static_assert(NU % 2 == 0, "units are processed in pairs");
  auto compute = [&]() {
    bf16x8 ah[2], al[2], bh[4], bl[4];
    auto request = [&](int u) {       // u is a constant after unrolling
      const int ks = u / TA, t = u % TA;
      if (t == 0) {
        ah[ks & 1] = tr_frag(Ab + ks * 16 * WP_DYPITCH, WP_DYPITCH);
        al[ks & 1] = tr_frag(Ab + ks * 16 * WP_DYPITCH + DY_PLANE, WP_DYPITCH);
      }
      const char* bp = Bt[t] + ((ks >> 1) * PW + 16 * (ks & 1)) * WP_XPITCH;   // k-step = half a line of 32 pixels
      bh[u & 3] = tr_frag(bp, WP_XPITCH);
      bl[u & 3] = tr_frag(bp + X_PLANE, WP_XPITCH);
    };
    request(0);
    request(1);
#pragma unroll
    for (int u = 0; u < NU; u += 2) {
      const int k0_ = (u / TA) & 1, k1_ = ((u + 1) / TA) & 1, t0 = u % TA, t1 = (u + 1) % TA, s0 = u & 3, s1 = (u + 1) & 3;
      if (u + 2 < NU) request(u + 2);
      __builtin_amdgcn_sched_barrier(0);
      acc[t0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[k0_], bh[s0], acc[t0], 0, 0, 0);
      acc[t1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[k1_], bh[s1], acc[t1], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (u + 3 < NU) request(u + 3);
      __builtin_amdgcn_sched_barrier(0);
      acc[t0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[k0_], bl[s0], acc[t0], 0, 0, 0);
      acc[t1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[k1_], bl[s1], acc[t1], 0, 0, 0);
      acc[t0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[k0_], bh[s0], acc[t0], 0, 0, 0);
      acc[t1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[k1_], bh[s1], acc[t1], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  for (int it = it0; it < it1;) {
    // ---- next segment: (co tile, source chunk) pair and block run
    const int pair = it / len, bo = it - pair * len, cnt = len - bo < it1 - it ? len - bo : it1 - it;
    it += cnt;
    const int blk0 = base + bo, blk1 = blk0 + cnt;
    const int cot = pair % args.cot, sch = pair / args.cot;
    const unsigned pe = ((const unsigned __attribute__((address_space(4)))*)(karg + offsetof(WgradPatchArgs, ptab)))[sch];
    const int s = pe & 3;
    ci0 = ((pe >> 2) & 63) * WP_CI; kofs0 = (int)(pe >> 8); co0 = cot * WP_CO;
    const Src sc = s == 0 ? a.src[0] : s == 1 ? a.src[1] : a.src[2];
    cpad = s == 0 ? args.cpad[0] : s == 1 ? args.cpad[1] : args.cpad[2];
    xtab = (const fptr __attribute__((address_space(4)))*)(karg + offsetof(WgradPatchArgs, m) + offsetof(WgradArgsM, srcs)) + s * WGRAD_MAX_SEG;
    ldx4 = uni((unsigned)sc.ld * 4u);
    dyoff = dyc4 < ((a.Cout + 3) / 4) * 4 - co0 ? (unsigned)k0 * ldy4 + (unsigned)dyc4 * 4u : FS_OOB;
    xcol = xc4 < sc.C - ci0;
    xn = sc.C - ci0 - xc4 < 4 ? sc.C - ci0 - xc4 : 4;
    want_bias = a.dbias != nullptr && sch == 0;
#pragma unroll
    for (int t = 0; t < TA; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) colsum[i] = 0.f;

    fetch(blk0);
    for (int blk = blk0; blk < blk1; ++blk) {
      stage();                                              // (the planes are free: everybody passed the barrier below)
      if (blk + 1 < blk1) fetch(blk + 1);                   // in flight while this block is multiplied
      __syncthreads();
      compute();
      __syncthreads();
    }

    // ---- out: one round of atomics into the packed layout; the bias gradient from the column sums of the dY loads
    float* dw = a.dwpk;
    asm volatile("" : "+s"(dw));      // (keeps the 80 output addresses from being computed before the block loop and spilled)
#pragma unroll
    for (int t = 0; t < TA; ++t) {
      const int tap = th * TA + t;
      if (tap >= TAPS) continue;
      const int ci = ci0 + l31;
      if (ci >= cpad) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = co0 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (co < a.Cout) atomicAdd(dw + (int64_t)co * a.Ktot + kofs0 + tap * cpad + l31, acc[t][r]);
      }
    }
    if (want_bias) {
      float* part = reinterpret_cast<float*>(lds);
#pragma unroll
      for (int i = 0; i < 4; ++i) part[k0 * WP_CO + dyc4 + i] = colsum[i];
      __syncthreads();
      if (threadIdx.x < WP_CO) {
        float sum = 0.f;
        for (int g = 0; g < WP_NT / 16; ++g) sum += part[g * WP_CO + threadIdx.x];
        if (co0 + threadIdx.x < a.Cout) atomicAdd(a.dbias + co0 + threadIdx.x, sum);
      }
      __syncthreads();
    }
  }
}

// -1: not covered (the caller runs the per-tap kernel)
int launch_wgrad_patch(WgradArgsM m, hipStream_t s) {
  const WgradArgs& a = m.a;
  const bool k33 = a.KH == 3 && a.KW == 3, k15 = a.KH == 1 && a.KW == 5, k51 = a.KH == 5 && a.KW == 1;
  if (!(k33 || k15 || k51) || a.Cout <= 32) return -1;
  if (!k33 && knob.wgrad_patch < 2) return -1;                 // (key 27 = 2: the five-tap layers too)
  WgradPatchArgs p;
  p.m = m;
  p.ty = ceil_div(a.H, WP_TH); p.tx = ceil_div(a.W, WP_TW);
  p.nblk = m.nseg * a.B * p.ty * p.tx;
  p.cot = ceil_div(a.Cout, WP_CO);
  int nsch = 0, kofs = 0;
  const int taps = a.KH * a.KW;
  for (int sidx = 0; sidx < 3; ++sidx) p.cpad[sidx] = 32;
  for (int sidx = 0; sidx < a.nsrc; ++sidx) {
    const int C = a.src[sidx].C, cpad = ceil_div(C, 32) * 32;
    p.cpad[sidx] = cpad;
    if ((int64_t)a.B * a.H * a.W * a.src[sidx].ld * 4 >= (int64_t)0x7fffffff || (int64_t)a.B * a.H * a.W * a.ldy * 4 >= (int64_t)0x7fffffff) return -1;
    if ((int64_t)a.B * a.H * a.W >= (1 << 24) || a.src[sidx].ld * 4 >= (1 << 24)) return -1;
    for (int c = 0; c < ceil_div(C, WP_CI); ++c) {
      if (nsch >= 48 || c >= 64 || kofs + c * WP_CI >= (1 << 24)) return -1;
      p.ptab[nsch++] = (unsigned)sidx | (unsigned)c << 2 | (unsigned)(kofs + c * WP_CI) << 8;
    }
    kofs += taps * cpad;
  }
  if (kofs != a.Ktot || nsch < 1) return -1;
  p.npair = p.cot * nsch;
  // 512 workgroups, two per CU, 64 on each XCD (workgroup id % 8).  An XCD owns one eighth of the blocks ("span") for ALL
  // pairs, so the dY / X blocks its workgroups share come out of its own L2.  With P pairs, floor(64 / P) * P workgroups walk
  // sub-ranges of the span in lockstep, one pair each; the 64 % P workgroups left over share a last, shorter sub-range of all
  // pairs in equal runs of (pair, block) items -- a run that crosses a pair boundary costs one more round of atomics.  Every
  // workgroup gets npair * nblk / 512 block-pairs (dealing whole ranges left the 3x3 256->192 and 1x5 384->256 layers with
  // 36-48 workgroups of 32 on some XCDs: two rounds).
  dim3 grid(8 * WP_SLOTS);
  t_route[1] = 7;
  if (k33) hipLaunchKernelGGL((conv_wgrad_patch_kernel<3, 3>), grid, dim3(WP_NT), 0, s, p);
  else if (k15) hipLaunchKernelGGL((conv_wgrad_patch_kernel<1, 5>), grid, dim3(WP_NT), 0, s, p);
  else hipLaunchKernelGGL((conv_wgrad_patch_kernel<5, 1>), grid, dim3(WP_NT), 0, s, p);
  return fs_launch_status();
}

}  // namespace
