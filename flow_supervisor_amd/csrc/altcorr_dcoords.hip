// Gradient of the memory-efficient lookup (altcorr_fused_fwd_kernel of altcorr.hip) w.r.t. the query COORDINATES: the
// contract of corr_dcoords.hip applied to the volume that is never formed, V_l[q, y, x] = f1[q] . f2_l[y, x] / sqrt(C).
// The reference's extension returns zeros here (alt_cuda_corr/correlation_kernel.cu:307).
//
// Level l, s = 2^-l, p = c s, (x0, y0) = floor(p), (fx, fy) = p - floor(p), window positions (iy, ix) in [0, 2r+1]^2 at
// (y0 - r + iy, x0 - r + ix), g[i][j] = dout[channel l (2r+1)^2 + i (2r+1) + j] (i = x offset, slow).  The bilinear slopes are
// moved from the (2r+1)^2 outputs onto the (2r+2)^2 positions first (weight-first, as altcorr_bwd_kernel forms gpos):
//     Gx[iy][ix] = sum over aa, cc in {0, 1} of g[ix - cc][iy - aa] (aa ? fy : 1 - fy) (cc ? +1 : -1)
//     Gy[iy][ix] = sum over aa, cc in {0, 1} of g[ix - cc][iy - aa] (cc ? fx : 1 - fx) (aa ? +1 : -1)     (indices in [0, 2r] only)
//     dcoords_x  = 1 / sqrt(C) f1[q] . sum over l and the positions inside level l of s Gx[iy][ix] f2_l[y0 - r + iy, x0 - r + ix, :]
// and likewise dcoords_y with Gy.  Positions outside a level read zero and the jump to zero is part of the slope; floor() picks
// the cell to the right / below at an integer position; a level at which |c s| >= 30000 on either axis has its window clamped
// off the map (level_query, the forward's clamp) and contributes nothing.
//
// ONE WAVE PER QUERY, four queries per workgroup, as the forward.  Lane l keeps channels l + 64 k (k < NK = ceil(C / 64)) of the
// query's fmap1 row and of the two running sums in registers.  Per level the wave puts its (2r+1)^2 dOut values in LDS, lane =
// position forms (s Gx, s Gy) -- zero for a position outside the level -- and the wave then walks the window row by row, reading
// every fmap2 row as 256-byte segments: acc_x[k] += Gx row[k], acc_y[k] += Gy row[k].  The x of a position is clamped into the
// level for the ADDRESS only (its G is zero), which keeps the ten positions of a window row straight-line code with all their
// loads in flight; a window row outside the level is skipped (wave-uniform branch).  After the last level each lane multiplies by
// its fmap1 channels and one fixed-order 64-lane sum gives the two floats.  fp32 VALU arithmetic only, no atomics, no cross-wave
// step: two launches give the same bits.
// Compulsory bytes: fmap1 + the fmap2 levels + coords + dOut read, two floats per query written.  FLOPs: 4 C per position.
#include "corr_tiled_dev.hpp"

namespace {

struct AltMaps {
  const float* f2[4];
  int h[4], w[4];
};

template <int R, int NK>
__global__ __launch_bounds__(256) void altcorr_fused_dcoords_kernel(const float* __restrict__ f1, AltMaps lv, Coords co, int grid_w,
                                                                    const float* __restrict__ dout, Grad2 dc, int nlev, unsigned nq,
                                                                    int HW, int C, float scale) {
  constexpr int RD = 2 * R + 1, WIN = RD + 1, NPOS = WIN * WIN, N2 = RD * RD;
  __shared__ float gout[4][N2 + 3];
  __shared__ __attribute__((aligned(8))) float2 gxy[4][NPOS];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const unsigned q = blockIdx.x * 4u + (unsigned)wave;          // wave-uniform; nq < 2^31 (checked by the host)
  if (q >= nq) return;                                          // (no workgroup barrier below)
  const int b = (int)(q / (unsigned)HW), pix = (int)(q % (unsigned)HW);
  float cx0, cy0;
  query_xy(co, b, pix, grid_w, cx0, cy0);
  // channel of this lane in round k; a lane without one re-reads channel 0 and multiplies it by a[k] = 0 at the end
  int ch[NK];
  float a[NK], accx[NK], accy[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const bool has = lane + 64 * k < C;
    ch[k] = has ? lane + 64 * k : 0;
    a[k] = has ? gload1(f1 + (int64_t)q * C + ch[k]) : 0.f;
    accx[k] = accy[k] = 0.f;
  }
  const float* g = dout + (int64_t)q * (nlev * N2);
  for (int l = 0; l < nlev; ++l) {
    const LevelQ lq = level_query(cx0, cy0, l, R);
    const float s = 1.0f / (float)(1 << l);
    const int H2 = lv.h[l], W2 = lv.w[l];
    for (int o = lane; o < N2; o += 64) gout[wave][o] = gload1(g + l * N2 + o);
    wave_lds_sync();
    for (int p = lane; p < NPOS; p += 64) {
      const int iy = p / WIN, ix = p % WIN;
      float gx = 0.f, gy = 0.f;
      // position (iy, ix) is tap (aa, cc) of output (iy - aa, ix - cc); channel = iyo + RD * ixo
#pragma unroll
      for (int aa = 0; aa < 2; ++aa)
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
          const int iyo = iy - aa, ixo = ix - cc;
          if (iyo >= 0 && iyo < RD && ixo >= 0 && ixo < RD) {
            const float v = gout[wave][iyo + RD * ixo];
            gx += v * (aa ? lq.fy : 1.f - lq.fy) * (cc ? 1.f : -1.f);
            gy += v * (cc ? lq.fx : 1.f - lq.fx) * (aa ? 1.f : -1.f);
          }
        }
      const int x = lq.wx0 + ix, y = lq.wy0 + iy;
      const bool in = x >= 0 && x < W2 && y >= 0 && y < H2;
      gxy[wave][p] = in ? make_float2(gx * s, gy * s) : make_float2(0.f, 0.f);
    }
    wave_lds_sync();
    const float* f2b = lv.f2[l] + (int64_t)b * H2 * W2 * C;
#pragma unroll 1
    for (int iy = 0; iy < WIN; ++iy) {
      const int y = lq.wy0 + iy;
      if (y < 0 || y >= H2) continue;                           // (wave-uniform)
      const float* rowy = f2b + (int64_t)y * W2 * C;
#pragma unroll
      for (int ix = 0; ix < WIN; ++ix) {
        const int x = min(max(lq.wx0 + ix, 0), W2 - 1);         // outside the level: an address inside it, G = 0
        const float2 gp = gxy[wave][iy * WIN + ix];
        const float* row = rowy + (int64_t)x * C;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
          const float v = gload1(row + ch[k]);
          accx[k] += gp.x * v;
          accy[k] += gp.y * v;
        }
      }
    }
    wave_lds_sync();
  }
  float ax = 0.f, ay = 0.f;
#pragma unroll
  for (int k = 0; k < NK; ++k) { ax += a[k] * accx[k]; ay += a[k] * accy[k]; }
  ax = wave_sum_fixed(ax) * scale;
  ay = wave_sum_fixed(ay) * scale;
  // every element written, zeros included: lane 0 the x component, lane 1 the y component
  if (lane < 2) gstore1(dc.p + b * dc.bs + lane * dc.cs + pix * dc.ps, lane ? ay : ax);
}

template <int R, int NK>
int launch_alt_dcoords(const float* f1, const AltMaps& lv, const Coords& co, int grid_w, const float* dout, const Grad2& dc, int nlev,
                       int64_t nq, int HW, int C, hipStream_t s) {
  const dim3 grid((unsigned)((nq + 3) / 4));
  hipLaunchKernelGGL((altcorr_fused_dcoords_kernel<R, NK>), grid, dim3(256), 0, s, f1, lv, co, grid_w, dout, dc, nlev, (unsigned)nq, HW, C,
                     1.0f / sqrtf((float)C));
  return fs_launch_status();
}

template <int R>
int launch_alt_dcoords_r(const float* f1, const AltMaps& lv, const Coords& co, int grid_w, const float* dout, const Grad2& dc, int nlev,
                         int64_t nq, int HW, int C, hipStream_t s) {
  switch ((C + 63) / 64) {
    case 1: return launch_alt_dcoords<R, 1>(f1, lv, co, grid_w, dout, dc, nlev, nq, HW, C, s);
    case 2: return launch_alt_dcoords<R, 2>(f1, lv, co, grid_w, dout, dc, nlev, nq, HW, C, s);
    case 3: return launch_alt_dcoords<R, 3>(f1, lv, co, grid_w, dout, dc, nlev, nq, HW, C, s);
    default: return launch_alt_dcoords<R, 4>(f1, lv, co, grid_w, dout, dc, nlev, nq, HW, C, s);
  }
}

}  // namespace

// fmap1, fmap2_levels, coords and add_grid as fsraft_altcorr_fused_fwd; dout [B, H, W, L*(2r+1)^2] channels-last; dcoords element
// (b, c, pix) written at dcoords[b*dbs + c*dcs + pix*dps] (every element, never accumulated).
extern "C" int fsraft_altcorr_fused_dcoords(const float* fmap1, const float* const* fmap2_levels, int num_levels, const float* coords,
                                            int64_t coords_bs, int64_t coords_cs, int64_t coords_ps, int add_grid, const float* dout,
                                            float* dcoords, int64_t dbs, int64_t dcs, int64_t dps, int B, int H, int W, int C, int radius,
                                            hipStream_t stream) {
  if (!fmap1 || !fmap2_levels || !coords || !dout || !dcoords || num_levels < 1 || num_levels > 4 || (radius != 3 && radius != 4) ||
      B < 1 || H < 1 || W < 1 || C < 1 || C > 256)
    return FS_ERR_ARG;
  const int64_t nq = (int64_t)B * H * W;
  if (nq >= (int64_t)1 << 31) return FS_ERR_ARG;
  AltMaps lv;
  for (int l = 0; l < 4; ++l) {
    const bool on = l < num_levels;
    if (on && (!fmap2_levels[l] || (H >> l) < 1 || (W >> l) < 1)) return FS_ERR_ARG;
    lv.f2[l] = on ? fmap2_levels[l] : nullptr;
    lv.h[l] = on ? H >> l : 0;
    lv.w[l] = on ? W >> l : 0;
  }
  const Coords co{coords, coords_bs, coords_cs, coords_ps};
  const Grad2 dc{dcoords, dbs, dcs, dps};
  const int gw = add_grid ? W : 0;
  if (radius == 4) return launch_alt_dcoords_r<4>(fmap1, lv, co, gw, dout, dc, num_levels, nq, H * W, C, stream);
  return launch_alt_dcoords_r<3>(fmap1, lv, co, gw, dout, dc, num_levels, nq, H * W, C, stream);
}
