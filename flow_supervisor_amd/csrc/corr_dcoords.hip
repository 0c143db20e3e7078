// Gradient of the pyramid lookup w.r.t. the query COORDINATES (rows a3 of SURVEY.md section 8; reference:
// grid_sampler_2d_backward w.r.t. the grid, through pytorch/core/corr.py:29-50 + core/utils/utils.py:57-71).
//
// Level l, window entry (i, j) (channel l (2r+1)^2 + i (2r+1) + j, i = x offset), sample position p = c 2^-l + (i - r, j - r),
// (x0, y0) = floor(p), (fx, fy) = p - floor(p), taps v00 = V_l[y0, x0], v01 = V_l[y0, x0 + 1], v10 = V_l[y0 + 1, x0],
// v11 = V_l[y0 + 1, x0 + 1], zero outside the level:
//     d out / d c_x = 2^-l ((1 - fy) (v01 - v00) + fy (v11 - v10))
//     d out / d c_y = 2^-l ((1 - fx) (v10 - v00) + fx (v11 - v01))
//     dcoords[b, 0|1, y, x] = sum over l, i, j of dout[b, y, x, channel] * the above
// floor() fixes the convention at integer positions (the slope of the cell to the right / below), and the jump to zero at an
// edge of a level is part of the slope.  With add_grid the gradient w.r.t. the flow is the gradient w.r.t. the coordinates.
//
// A GATHER with the forward lookup's access pattern: ONE WAVE PER QUERY reads the same (2r+2)^2 windows into the same LDS
// regions (corr_tiled_dev.hpp), plus the L (2r+1)^2 floats of dOut, and writes two floats.  A lane owns channels lane + 64 k of
// every level: both partial derivatives from the four taps in LDS, times its dOut element, times 2^-l, summed over the levels
// in two fp32 partials; the 64 lanes' partials are then added in a fixed order by DPP moves inside the rows of 16 lanes and
// four v_readlane across them.  No atomics, no cross-wave step: two runs give the same bits.  The dOut loads of query k + 1
// are issued with its window loads, before the arithmetic of query k (the forward's software pipeline over QW queries).
// Algorithmic HBM bytes per query: L (2r+2)^2 4 + 8 coords + L (2r+1)^2 4 dOut read, 8 written.
//
// The same arithmetic serves row-major levels ([rows, 1, h_l, w_l], floor sizes: the API twins) behind a second window loader.
#include "corr_tiled_dev.hpp"

namespace {

// window loaders: issue() requests the (2r+2)^2 windows of all levels of one query (16 bytes per lane and level, zeros where the
// window leaves the level), stage() puts one level's into its LDS region and returns where window cell (0, 0) lies in it
template <int R, int AUX>
struct TiledWindows {          // the forward lookup's: the 4x4-tile superset of the window, lane = (tile, row of the tile)
  struct Src { const float* vol; VolLayout L; };
  const float* vol;
  LevelGeo g[4];
  unsigned row_bytes;
  int P, nlev, tsx, tsy, r;
  __device__ __forceinline__ TiledWindows(const Src& s, int lane)
      : vol(s.vol), row_bytes((unsigned)s.L.P * 4u), P(s.L.P), nlev(s.L.nlev), tsx((lane >> 2) & 3), tsy(lane >> 4), r(lane & 3) {
#pragma unroll
    for (int l = 0; l < 4; ++l) g[l] = LevelGeo{s.L.off[l], s.L.tw[l], s.L.h[l], s.L.w[l]};
  }
  __device__ __forceinline__ void issue(LookupLoad<R>& ld, unsigned q, float cx, float cy) const {
    lookup_issue<R, AUX>(ld, vol + (int64_t)q * P, row_bytes, g, nlev, cx, cy, tsx, tsy, r);
  }
  __device__ __forceinline__ int stage(float* reg, f32x4 v, const LevelQ& lq, int l) const {
    const int xr = g[l].w - 4 * ((lq.wx0 >> 2) + tsx);      // true width minus the x of this lane's first cell: cells at or beyond it are pad
#pragma unroll
    for (int c = 1; c < 4; ++c) v[c] = c < xr ? v[c] : 0.f;
    *reinterpret_cast<f32x4*>(reg + (4 * tsy + r) * TL<R>::RP + 4 * tsx) = v;
    return (lq.wy0 & 3) * TL<R>::RP + (lq.wx0 & 3);
  }
};

template <int R>
struct RowWindows {            // row-major levels: lane = (window row, quarter of it), four masked 4-byte buffer loads per level
  struct Src { const float* p[4]; int h[4], w[4], nlev; };
  Src s;
  int wr, c4;
  __device__ __forceinline__ RowWindows(const Src& s_, int lane) : s(s_), wr(lane >> 2), c4(lane & 3) {}
  __device__ __forceinline__ void issue(LookupLoad<R>& ld, unsigned q, float cx, float cy) const {
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const LevelQ lq = level_query(cx, cy, l, R);
      const int h = s.h[l], w = s.w[l], y = lq.wy0 + wr;             // (levels beyond nlev: h = w = 0, nothing in range)
      const __amdgpu_buffer_rsrc_t rs = row_rsrc(s.p[l] + (int64_t)q * h * w, (unsigned)(h * w) * 4u);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int wx = 4 * c4 + c, x = lq.wx0 + wx;
        const bool need = wr < TL<R>::WIN && wx < TL<R>::WIN && y >= 0 && y < h && x >= 0 && x < w;
        const unsigned voff = need ? (unsigned)(y * w + x) * 4u : 0x80000000u;
        ld.v[l][c] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, voff, 0, 0));
      }
    }
  }
  __device__ __forceinline__ int stage(float* reg, f32x4 v, const LevelQ&, int) const {
    *reinterpret_cast<f32x4*>(reg + wr * TL<R>::RP + 4 * c4) = v;
    return 0;
  }
};

template <int R>
struct DoutLoad {
  float g[4][TL<R>::ROUNDS];
};

// this lane's dOut elements of one query (element (b, ch, pix) at p + b bs + ch cs + pix ps): channels lane + 64 k of every
// level.  Unconditional loads (a lane without a channel re-reads channel 0 and drops it later), so they are counted with the
// window loads.
template <int R>
__device__ __forceinline__ void dout_issue(DoutLoad<R>& d, const Coords& go, unsigned q, int HW, int nlev, int lane) {
  using S = TL<R>;
  const float* base = go.p + (int64_t)(q / (unsigned)HW) * go.bs + (int64_t)(q % (unsigned)HW) * go.ps;
#pragma unroll
  for (int l = 0; l < 4; ++l)
#pragma unroll
    for (int k = 0; k < S::ROUNDS; ++k) {
      const int kk = lane + 64 * k;
      const int ch = (l < nlev && kk < S::N2) ? l * S::N2 + kk : 0;
      d.g[l][k] = gload1(base + ch * go.cs);
    }
}

template <int R, int QW, class WINDOWS>
__global__ __launch_bounds__(256) void lookup_dcoords_kernel(typename WINDOWS::Src src, int nlev, Coords co, Coords go, Grad2 dc, int64_t nq,
                                                             int HW, int grid_w) {
  using S = TL<R>;
  __shared__ __attribute__((aligned(16))) float region[4][4][S::REGION];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const WINDOWS win(src, lane);
  float* reg = &region[wave][0][0];
  int choff[S::ROUNDS];            // channel (i, j) of a level handled by this lane in round k -> offset inside the region
#pragma unroll
  for (int k = 0; k < S::ROUNDS; ++k) {
    const int kk = lane + 64 * k;
    choff[k] = kk < S::N2 ? (kk % S::N1) * S::RP + kk / S::N1 : 0;      // i = kk / N1 (x offset, slow), j = kk % N1 (y offset)
  }
  const unsigned q0 = (blockIdx.x * 4u + (unsigned)wave) * QW;          // wave-uniform; nq < 2^31 (checked by the host)
  if (q0 >= (unsigned)nq) return;
  const int nqw = (int)((unsigned)nq - q0 < (unsigned)QW ? (unsigned)nq - q0 : (unsigned)QW);
  float cxs[QW], cys[QW];
#pragma unroll
  for (int qq = 0; qq < QW; ++qq) {
    const unsigned q = q0 + (qq < nqw ? qq : 0);
    query_xy(co, (int)(q / (unsigned)HW), (int)(q % (unsigned)HW), grid_w, cxs[qq], cys[qq]);
  }
  LookupLoad<R> cur, nxt;
  DoutLoad<R> gcur, gnxt;
  win.issue(cur, q0, cxs[0], cys[0]);
  dout_issue<R>(gcur, go, q0, HW, nlev, lane);
#pragma unroll
  for (int qq = 0; qq < QW; ++qq) {
    if (qq >= nqw) break;
    const unsigned q = q0 + qq;
    // the next query's windows and dOut slice are requested before this one's are consumed (the last valid query again at the end)
    const int qn = qq + 1 < nqw ? qq + 1 : qq;
    if (qq + 1 < QW) {
      win.issue(nxt, q0 + qn, cxs[qn], cys[qn]);
      dout_issue<R>(gnxt, go, q0 + qn, HW, nlev, lane);
    }
    LevelQ lqs[4];
    int org[4];
#pragma unroll
    for (int l = 0; l < 4; ++l) lqs[l] = level_query(cxs[qq], cys[qq], l, R);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      org[l] = 0;
      if (l < nlev) org[l] = win.stage(reg + l * S::REGION, cur.v[l], lqs[l], l);
    }
    wave_lds_sync();
    float ax = 0.f, ay = 0.f;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      if (l >= nlev) continue;
      const float* base = reg + l * S::REGION + org[l];
      const float fx = lqs[l].fx, fy = lqs[l].fy, s = 1.0f / (float)(1 << l);
#pragma unroll
      for (int k = 0; k < S::ROUNDS; ++k) {
        const float* p = base + choff[k];
        const float v00 = p[0], v01 = p[1], v10 = p[S::RP], v11 = p[S::RP + 1];
        const float dx = (1.f - fy) * (v01 - v00) + fy * (v11 - v10);
        const float dy = (1.f - fx) * (v10 - v00) + fx * (v11 - v01);
        const float gs = lane + 64 * k < S::N2 ? gcur.g[l][k] * s : 0.f;
        ax += gs * dx;
        ay += gs * dy;
      }
    }
    ax = wave_sum_fixed(ax);
    ay = wave_sum_fixed(ay);
    // every element written, zeros included: lane 0 the x component, lane 1 the y component
    if (lane < 2)
      gstore1(dc.p + (int64_t)(q / (unsigned)HW) * dc.bs + lane * dc.cs + (int64_t)(q % (unsigned)HW) * dc.ps, lane ? ay : ax);
    wave_lds_sync();
    if (qq + 1 < QW) { cur = nxt; gcur = gnxt; }
  }
}

template <int R, class WINDOWS>
int launch_dcoords(const typename WINDOWS::Src& src, int nlev, const Coords& co, const Coords& go, const Grad2& dc, int64_t nq, int HW,
                   int grid_w, hipStream_t s) {
  constexpr int QW = 4;
  const dim3 grid((unsigned)((nq + 4 * QW - 1) / (4 * QW)));
  hipLaunchKernelGGL((lookup_dcoords_kernel<R, QW, WINDOWS>), grid, dim3(256), 0, s, src, nlev, co, go, dc, nq, HW, grid_w);
  return fs_launch_status();
}

// The body of fsraft_corr_lookup_dcoords and its 'SAME' twin: level l is H >> l x W >> l, or the ceil of H / 2^l x W / 2^l.
int row_dcoords_entry(float* const* levels, int num_levels, const float* coords, int64_t coords_bs, int64_t coords_cs, int64_t coords_ps,
                      const float* dout, int nhwc_in, float* dcoords, int64_t dbs, int64_t dcs, int64_t dps, int B, int H, int W,
                      int radius, bool ceil, hipStream_t stream) {
  if (!levels || !coords || !dout || !dcoords || B < 1 || H < 1 || W < 1 || (radius != 3 && radius != 4) || num_levels < 1 || num_levels > 4)
    return FS_ERR_ARG;
  const int64_t nq = (int64_t)B * H * W;
  if (nq >= (int64_t)1 << 31 || (int64_t)H * W * 4 >= (int64_t)1 << 31) return FS_ERR_ARG;
  RowWindows<4>::Src s4;
  for (int l = 0; l < 4; ++l) {
    const bool on = l < num_levels;
    const int h = ceil ? (H + (1 << l) - 1) >> l : H >> l, w = ceil ? (W + (1 << l) - 1) >> l : W >> l;
    if (on && (!levels[l] || h < 1 || w < 1)) return FS_ERR_ARG;
    s4.p[l] = on ? levels[l] : levels[0];
    s4.h[l] = on ? h : 0;
    s4.w[l] = on ? w : 0;
  }
  s4.nlev = num_levels;
  const int CH = num_levels * (2 * radius + 1) * (2 * radius + 1);
  const int64_t HW = (int64_t)H * W;
  const Coords co{coords, coords_bs, coords_cs, coords_ps};
  const Coords go = nhwc_in ? Coords{dout, HW * CH, 1, CH} : Coords{dout, HW * CH, HW, 1};
  const Grad2 dc{dcoords, dbs, dcs, dps};
  if (radius == 4) return launch_dcoords<4, RowWindows<4>>(s4, num_levels, co, go, dc, nq, H * W, 0, stream);
  RowWindows<3>::Src s3;
  for (int l = 0; l < 4; ++l) { s3.p[l] = s4.p[l]; s3.h[l] = s4.h[l]; s3.w[l] = s4.w[l]; }
  s3.nlev = num_levels;
  return launch_dcoords<3, RowWindows<3>>(s3, num_levels, co, go, dc, nq, H * W, 0, stream);
}

}  // namespace

// dcoords element (b, c, pix) written at dcoords[b*dbs + c*dcs + pix*dps] (every element, never accumulated); dout
// [B, H, W, L*(2r+1)^2] channels-last; vol, coords and add_grid as fsraft_corr_lookup_tiled_fwd.
extern "C" int fsraft_corr_lookup_tiled_dcoords(const float* vol, int num_levels, const float* coords, int64_t coords_bs, int64_t coords_cs,
                                                int64_t coords_ps, const float* dout, float* dcoords, int64_t dbs, int64_t dcs, int64_t dps,
                                                int B, int H, int W, int radius, int add_grid, hipStream_t stream) {
  VolLayout L;
  if (!vol || !coords || !dout || !dcoords || B < 1 || (radius != 3 && radius != 4) || !vol_layout_make(H, W, num_levels, L) ||
      ((uintptr_t)vol % 16))
    return FS_ERR_ARG;
  const int64_t nq = (int64_t)B * H * W;
  if (nq >= (int64_t)1 << 31 || (int64_t)L.P * 4 >= (int64_t)1 << 31) return FS_ERR_ARG;
  const int CH = num_levels * (2 * radius + 1) * (2 * radius + 1);
  const Coords co{coords, coords_bs, coords_cs, coords_ps}, go{dout, (int64_t)H * W * CH, 1, CH};
  const Grad2 dc{dcoords, dbs, dcs, dps};
  const int gw = add_grid ? W : 0;
  // window loads non-temporal once the volume is larger than the Infinity Cache, as the forward lookup's (launch_lookup)
  const bool nt = nq * L.P * 4 > ((int64_t)300 << 20);
  if (radius == 4) {
    if (nt) return launch_dcoords<4, TiledWindows<4, 2>>({vol, L}, num_levels, co, go, dc, nq, H * W, gw, stream);
    return launch_dcoords<4, TiledWindows<4, 0>>({vol, L}, num_levels, co, go, dc, nq, H * W, gw, stream);
  }
  if (nt) return launch_dcoords<3, TiledWindows<3, 2>>({vol, L}, num_levels, co, go, dc, nq, H * W, gw, stream);
  return launch_dcoords<3, TiledWindows<3, 0>>({vol, L}, num_levels, co, go, dc, nq, H * W, gw, stream);
}

// The same on row-major levels [B*H*W, 1, H >> l, W >> l] (floor sizes); dout [B, CH, H, W], or [B, H, W, CH] when nhwc_in.
extern "C" int fsraft_corr_lookup_dcoords(float* const* levels, int num_levels, const float* coords, int64_t coords_bs, int64_t coords_cs,
                                          int64_t coords_ps, const float* dout, int nhwc_in, float* dcoords, int64_t dbs, int64_t dcs,
                                          int64_t dps, int B, int H, int W, int radius, hipStream_t stream) {
  return row_dcoords_entry(levels, num_levels, coords, coords_bs, coords_cs, coords_ps, dout, nhwc_in, dcoords, dbs, dcs, dps, B, H, W,
                           radius, false, stream);
}

// The same on the levels of a TensorFlow 'SAME' pyramid: [B*H*W, 1, ceil(H / 2^l), ceil(W / 2^l)].
extern "C" int fsraft_corr_lookup_dcoords_same(float* const* levels, int num_levels, const float* coords, int64_t coords_bs,
                                               int64_t coords_cs, int64_t coords_ps, const float* dout, int nhwc_in, float* dcoords,
                                               int64_t dbs, int64_t dcs, int64_t dps, int B, int H, int W, int radius,
                                               hipStream_t stream) {
  return row_dcoords_entry(levels, num_levels, coords, coords_bs, coords_cs, coords_ps, dout, nhwc_in, dcoords, dbs, dcs, dps, B, H, W,
                           radius, true, stream);
}
