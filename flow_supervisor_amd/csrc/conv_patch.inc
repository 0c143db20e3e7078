// Implicit-GEMM convolution over a RESIDENT INPUT PATCH, channels streamed: included by conv_igemm.hip (ConvArgs, loaders'
// helpers, epilogues).
//
// The kernels above fetch, convert and store to LDS one 256-row A tile per (tap, 32-channel chunk): every activation byte
// crosses L2 -> VGPR -> LDS once per TAP -- nine times for a 3x3 layer -- and that traffic, not the matrix pipe, is what the
// k-loop waits for (1.29 us per k-tile against 0.64 us of MFMA) and what the socket's power budget goes to (DESIGN.md 3.1).
// Here a workgroup owns an 8 x 32 patch of output pixels.  Per 32-channel chunk it stages the input patch INCLUDING the halo
// the taps reach (10 x 34 pixels for 3x3, 8 x 36 for 1x5, 12 x 32 for 5x1) ONCE, as [hi | lo] records, and runs all taps of
// that chunk out of it: the A fragment of tap (dy, dx) is the same LDS image read (dy, dx) pixels further on.  Activation
// traffic and conversions drop by taps / halo factor (6.8x, 4.4x, 3.3x); what is left per k-tile is the 16 KB weight tile
// (register-staged copy of pre-split records) and one barrier.  The k order is (source, chunk) outer, tap inner -- the
// packed weights keep their layout, k-tile (s, tap, c) is just addressed out of sequence.
//
// Two patch planes (the next chunk's patch is fetched during this chunk's taps and stored before its last barrier), two
// weight tiles; eight waves (4 x 2, each 2 patch lines x 64 columns); epilogues of the implicit-GEMM kernels with the tile's
// rows mapped back to pixels.
// TH = 8: 256-pixel tiles, eight waves; TH = 4: 128-pixel tiles, four waves (layers with <= 128 outputs at M ~ 28 K, where
// 256-pixel tiles would leave half of the CUs without a workgroup).
constexpr int PT_TW = 32, PT_BN = 128;
constexpr int PT_GMAX = 32;

struct PatchArgs {
  ConvArgs a;
  int ngroups;
  int tx;                              // tiles per image row
  unsigned gtab[PT_GMAX];              // per (source, chunk): src | chunk << 2 | crem << 10 | (k-tile of tap 0) << 16
  int cpt[3];                          // chunks per source (k-tile of (s, tap, c) = ktile0 + tap * cpt[s])
};

template <int EPI, int KH, int KW, int PT_TH, int BN = PT_BN>
__global__ __launch_bounds__(PT_TH * 64) void conv_patch_kernel(const PatchArgs args) {
  constexpr int PT_NT = PT_TH * 64, TN = BN / 64;                           // BN = 64: layers with <= 64 outputs, one column block per wave
  using PCfg = SplitCfg<PT_TH * 32, BN, PT_TH / 2, 2, 2, true, PT_NT>;      // accumulator ownership / epilogue shape
  constexpr int TAPS = KH * KW, PHh = KH / 2, PWh = KW / 2;
  constexpr int PH = PT_TH + KH - 1, PW = PT_TW + KW - 1, ROWS = PH * PW;
  // patch rows are stored with a 144-byte pitch (9 sixteen-byte slots: the 16 rows of a ds_read_b128 lane group land on 16
  // different slots) instead of the XOR swizzle of the weight tiles: a tap shifts the ROW a lane reads, and with a swizzle that
  // depends on the row every fragment address costs five VALU instructions per tap; with a plain pitch the address is a
  // per-lane constant plus a compile-time immediate.
  constexpr int PPITCH = 144;
  constexpr int PT_PLANE = ROWS * PPITCH;
  constexpr int PT_NCHP = (ROWS * 8 + PT_NT - 1) / PT_NT;          // sixteen-byte chunks of a plane per thread
  constexpr int EPI_BYTES = PT_TH * 32 * (BN + 4) * 4, RING = 2 * PT_PLANE + 2 * BN * 128;
  __shared__ __attribute__((aligned(16))) char lds[RING > EPI_BYTES ? RING : EPI_BYTES];
  const ConvArgs& a = args.a;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, lh = lane >> 5;
  const int n0 = blockIdx.x * BN;
  const int tile = blockIdx.y, tpi = args.tx * ((a.H + PT_TH - 1) / PT_TH);
  const int b = tile / tpi, trem = tile % tpi;
  const int y0 = (trem / args.tx) * PT_TH, x0 = (trem % args.tx) * PT_TW;
  const auto* gtab = (const unsigned __attribute__((address_space(4)))*)(
      (const char __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(PatchArgs, gtab));
  const int NG = args.ngroups;

  // ---- this thread's chunks of a patch plane: (patch row, 16-byte part) -> pixel of the image (or outside)
  unsigned ppix[PT_NCHP];              // pixel index b*HW + y*W + x, or 0x7fffffff: outside the image / beyond the plane
  const unsigned part16 = (threadIdx.x & 7) * 16;
#pragma unroll
  for (int j = 0; j < PT_NCHP; ++j) {
    const int row = (threadIdx.x + PT_NT * j) >> 3;
    const int y = y0 - PHh + row / PW, x = x0 - PWh + row % PW;
    const bool ok = row < ROWS && (unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W;
    ppix[j] = ok ? (unsigned)((b * a.H + y) * a.W + x) : 0x7fffffffu;
  }
  // ---- this thread's chunks of a weight tile (BN rows x 128 bytes)
  constexpr int NCHW = BN * 8 / PT_NT;                             // chunks of a weight tile per thread (1, 2 or 4)
  unsigned vbw[NCHW];
#pragma unroll
  for (int j = 0; j < NCHW; ++j) {
    const int e = threadIdx.x + PT_NT * j;
    vbw[j] = (e >> 3) < a.N - n0 ? (unsigned)((e >> 3) * a.Ktot * 4 + (e & 7) * 16) : FS_OOB;
  }
  const char* wbase = uni_ptr(reinterpret_cast<const char*>(a.wpk) + (int64_t)n0 * a.Ktot * 4);

  struct Group { const float* base; unsigned ld4, soff, crem4; int kt0, step; };
  auto group = [&](int g) {
    const unsigned e = gtab[__builtin_amdgcn_readfirstlane(g < NG ? g : NG - 1)];
    const unsigned src = e & 3u, c = (e >> 2) & 255u, crem = (e >> 10) & 63u;
    const bool s1 = src >= 1, s2 = src >= 2;
    Group r;
    r.base = uni_ptr(a.src[0].p + (s1 ? a.src[1].p - a.src[0].p : 0) + (s2 ? a.src[2].p - a.src[1].p : 0));
    r.ld4 = uni((unsigned)(a.src[0].ld + (s1 ? a.src[1].ld - a.src[0].ld : 0) + (s2 ? a.src[2].ld - a.src[1].ld : 0)) * 4u);
    r.soff = c * 128u; r.crem4 = crem * 4u;
    r.kt0 = (int)(e >> 16);
    r.step = args.cpt[0] + (s1 ? args.cpt[1] - args.cpt[0] : 0) + (s2 ? args.cpt[2] - args.cpt[1] : 0);
    return r;
  };
  float rp[PT_NCHP * 4];               // the next chunk's patch, in flight
  auto fetch_patch = [&](const Group& gr) {
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(gr.base, 0x7fffffffu);
    const unsigned cok = part16 < gr.crem4 ? 0u : 0x80000000u;     // this lane's 16-byte column holds channels of the source
#pragma unroll
    for (int j = 0; j < PT_NCHP; ++j) {
      const unsigned voff = ppix[j] == 0x7fffffffu ? FS_OOB : ((ppix[j] * gr.ld4 + part16) | cok);
      const f32x4 f = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, gr.soff, 0));
      rp[4 * j] = f[0]; rp[4 * j + 1] = f[1]; rp[4 * j + 2] = f[2]; rp[4 * j + 3] = f[3];
    }
  };
  auto stage_patch = [&](char* plane) {
#pragma unroll
    for (int j = 0; j < PT_NCHP; ++j) {
      const int e = threadIdx.x + PT_NT * j;
      if ((e >> 3) < ROWS) stage_convert<PPITCH>(plane, e, rp + 4 * j);
    }
  };
  const __amdgpu_buffer_rsrc_t rsW = make_rsrc(wbase, 0x7fffffffu);
  float rw[NCHW * 4];                  // the next weight tile, in flight
  auto fetch_w = [&](int kt) {         // kt < 0: zeros
    const int ku = __builtin_amdgcn_readfirstlane(kt);
#pragma unroll
    for (int j = 0; j < NCHW; ++j) {
      const f32x4 f = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsW, ku < 0 ? FS_OOB : vbw[j], ku < 0 ? 0u : (unsigned)ku * 128u, 0));
      rw[4 * j] = f[0]; rw[4 * j + 1] = f[1]; rw[4 * j + 2] = f[2]; rw[4 * j + 3] = f[3];
    }
  };
  auto stage_w = [&](char* bt) {
#pragma unroll
    for (int j = 0; j < NCHW; ++j) stage_copy<128>(bt, threadIdx.x + PT_NT * j, rw + 4 * j);
  };

  f32x16 acc[2][TN];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  char* plane0 = lds;
  char* plane1 = lds + PT_PLANE;
  char* bt0 = lds + 2 * PT_PLANE;
  char* bt1 = bt0 + BN * 128;

  // one k-tile = tap (dy, dx) of the chunk in `plane`, weights in `bt`
  const int rb = wn * (BN / 2) + l31;
  const int la_off = (2 * wm * PW + l31) * PPITCH + lh * 16;     // this lane's row (tap (0, 0), mt = 0) and k half inside a plane
  // (reading all sixteen fragments of a k-tile before its MFMAs instead of eight per k-step measured the same)
  auto compute = [&](const char* plane, const char* bt, int dy, int dx) {
    const char* Bs = bt + rb * 128;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 ah[2], al[2], bh[TN], bl[TN];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        ah[mt] = *reinterpret_cast<const bf16x8*>(plane + la_off + ((dy + mt) * PW + dx) * PPITCH + (2 * s) * 16);
        al[mt] = *reinterpret_cast<const bf16x8*>(plane + la_off + ((dy + mt) * PW + dx) * PPITCH + (4 + 2 * s) * 16);
      }
      const int obh = slot_offset<128>(rb, 2 * s + lh) - rb * 128, obl = slot_offset<128>(rb, 4 + 2 * s + lh) - rb * 128;
#pragma unroll
      for (int nt = 0; nt < TN; ++nt) {
        bh[nt] = *reinterpret_cast<const bf16x8*>(Bs + nt * 32 * 128 + obh);
        bl[nt] = *reinterpret_cast<const bf16x8*>(Bs + nt * 32 * 128 + obl);
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < TN; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[mt], bh[nt], acc[mt][nt], 0, 0, 0);
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < TN; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mt], bl[nt], acc[mt][nt], 0, 0, 0);
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < TN; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mt], bh[nt], acc[mt][nt], 0, 0, 0);
    }
  };

  // ---- prologue: patch of chunk 0 and its first weight tile in LDS, chunk 1's patch and the second weight tile in flight
  Group gc = group(0);
  fetch_patch(gc);
  fetch_w(gc.kt0);
  stage_patch(plane0);
  stage_w(bt0);
  Group gn = group(1);
  if (NG > 1) fetch_patch(gn);
  fetch_w(TAPS > 1 ? gc.kt0 + gc.step : (NG > 1 ? gn.kt0 : -1));
  __syncthreads();
  for (int g = 0; g < NG; ++g) {
#pragma unroll
    for (int t = 0; t < TAPS; ++t) {
      const int i = g * TAPS + t;                          // k-tile counter: weight tile i sits in bt[i & 1]
      char* btc = (i & 1) ? bt1 : bt0;
      char* btn = (i & 1) ? bt0 : bt1;
      compute((g & 1) ? plane1 : plane0, btc, t / KW, t % KW);
      // weight tile i + 1 (fetched one k-tile ago) -> the other image; fetch tile i + 2
      stage_w(btn);
      {
        const int t2 = t + 2;
        int kt;
        if (t2 < TAPS) kt = gc.kt0 + t2 * gc.step;
        else kt = g + 1 < NG ? gn.kt0 + (t2 - TAPS) * gn.step : -1;
        if (TAPS == 1) {                                   // (two chunks ahead)
          const Group g2 = group(g + 2);
          kt = g + 2 < NG ? g2.kt0 : -1;
        }
        fetch_w(kt);
      }
      if (t == TAPS - 1 && g + 1 < NG) {                   // the next chunk's patch -> the other plane; fetch the one after
        stage_patch((g & 1) ? plane0 : plane1);
        gc = gn;
        gn = group(g + 2);
        if (g + 2 < NG) fetch_patch(gn);
      }
      __syncthreads();
    }
  }
  conv_epilogue_lds<PCfg, EPI, PT_NT, true>(a, acc, 0, n0, reinterpret_cast<float*>(lds), true, b, y0, x0);
}

template <int KH, int KW, int TH>
int launch_conv_patch_t(const PatchArgs& p, int epi, dim3 grid, hipStream_t s) {
  t_route[0] = (TH == 8 ? 11 : 10) + (KH == 3 && KW == 3 && p.a.N <= 64 ? 2 : 0);
  if constexpr (KH == 3 && KW == 3) {
    if (p.a.N <= 64) {                 // (plain epilogue only: checked by the caller)
      hipLaunchKernelGGL((conv_patch_kernel<EPI_PLAIN, 3, 3, TH, 64>), grid, dim3(TH * 64), 0, s, p);
      return fs_launch_status();
    }
  }
  with_epi(epi, [&](auto e) { hipLaunchKernelGGL((conv_patch_kernel<decltype(e)::value, KH, KW, TH>), grid, dim3(TH * 64), 0, s, p); });
  return fs_launch_status();
}

// -1: not a shape this kernel covers (the caller picks another one)
int launch_conv_patch(const ConvArgs& a, int epi, hipStream_t s) {
  const bool k33 = a.KH == 3 && a.KW == 3, k15 = a.KH == 1 && a.KW == 5, k51 = a.KH == 5 && a.KW == 1;
  if (!(k33 || k15 || k51) || a.PH != a.KH / 2 || a.PW != a.KW / 2 || !epilogue_rows_ok_host(a)) return -1;
  PatchArgs p;
  p.a = a; p.a.swz = 0;
  int ng = 0, kt = 0;
  const int taps = a.KH * a.KW;
  for (int sidx = 0; sidx < 3; ++sidx) p.cpt[sidx] = 1;
  for (int sidx = 0; sidx < a.nsrc; ++sidx) {
    const int C = a.src[sidx].C, cpt = (C + 31) / 32;
    p.cpt[sidx] = cpt;
    if ((int64_t)a.B * a.H * a.W * a.src[sidx].ld * 4 >= (int64_t)0x7fffffff) return -1;
    for (int c = 0; c < cpt; ++c) {
      if (ng >= PT_GMAX || kt + c >= (1 << 16)) return -1;
      const int crem = C - c * 32 < 32 ? C - c * 32 : 32;
      p.gtab[ng++] = (unsigned)sidx | (unsigned)c << 2 | (unsigned)crem << 10 | (unsigned)(kt + c) << 16;
    }
    kt += taps * cpt;
  }
  if (kt * 32 != a.Ktot || ng < 1) return -1;
  for (int g = ng; g < PT_GMAX; ++g) p.gtab[g] = p.gtab[ng - 1];
  p.ngroups = ng;
  p.tx = ceil_div(a.W, PT_TW);
  const int bn = a.N <= 64 ? 64 : PT_BN;
  if (bn == 64 && !(k33 && epi == EPI_PLAIN)) return -1;
  // 256-pixel tiles where they give every CU a workgroup, else 128-pixel tiles
  const int64_t wg8 = (int64_t)ceil_div(a.N, bn) * p.tx * ceil_div(a.H, 8) * a.B;
  // (64-column tiles: 64 -> 64 at 8x220x512 runs 269 us on 256-pixel tiles, 257 us on 128-pixel tiles, 236 us on
  //  conv3x3_halo_kernel -- twelve MFMAs per wave between barriers are too few; 128 -> 64 at M = 28160: 32 us on 128-pixel
  //  tiles against 41 us on the 256x64 implicit GEMM.  So: small grids only, key 28 = 2 / 3 forces 128 / 256-pixel tiles.)
  if (bn == 64 && wg8 >= 200 && knob.conv_patch64 == 1) return -1;
  if (wg8 >= 200 && !(bn == 64 && knob.conv_patch64 == 2)) {
    dim3 grid(ceil_div(a.N, bn), p.tx * ceil_div(a.H, 8) * a.B);
    if (k33) return launch_conv_patch_t<3, 3, 8>(p, epi, grid, s);
    if (k15) return launch_conv_patch_t<1, 5, 8>(p, epi, grid, s);
    return launch_conv_patch_t<5, 1, 8>(p, epi, grid, s);
  }
  // (128-pixel tiles, four waves: measured within +-3 % of the 128x128 implicit-GEMM kernel on the N <= 128 layers at
  //  M = 28160 -- cv 68 / 69 us, q 57 / 59, dg hd 115 / 111 -- so they stay an option: key 26 = 2)
  //  At one or two pairs per GPU (8832 / 13824 pixels) the 3x3 layers with two output tiles run 5-12 % faster here than on the
  //  138 / 216 workgroups of the implicit GEMM (3x3 256 -> 192: 65 -> 57.5 us, its data gradient 47 -> 43): adopted for those.
  const bool small_grid_33 = k33 && a.N > 128 && (int64_t)ceil_div(a.N, 128) * ceil_div(a.B * a.H * a.W, 128) > 120;
  if (knob.conv_patch != 2 && bn != 64 && !small_grid_33) return -1;
  dim3 grid(ceil_div(a.N, bn), p.tx * ceil_div(a.H, 4) * a.B);
  if (k33) return launch_conv_patch_t<3, 3, 4>(p, epi, grid, s);
  if (k15) return launch_conv_patch_t<1, 5, 4>(p, epi, grid, s);
  return launch_conv_patch_t<5, 1, 4>(p, epi, grid, s);
}
