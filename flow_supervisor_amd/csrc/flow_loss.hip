// Flow losses of the reference's TensorFlow trainers (raft/loss.py FlowLossL1 / FlowLossL2 / FlowLossRobust, as train.py:184-186
// compiles them and raft/semi.py:29-34, 373-405, 447-471 sums them over a sequence of predictions), and the per-sample sums
// raft/metric.py:EPE divides.  For n <= 32 predictions p_i against one target t, d = p_i - t per channel:
//   m     = mask[b,y,x] * (sqrt(t0^2 + t1^2) < max_flow)          the mask is a FACTOR (0.25 counts a quarter), the cut is strict
//   psi   = |d| (L1),  d^2 (L2),  sqrt(d^2 + eps^2) (ROBUST)
//   loss  = scale * sum_i w_i sum_{b,y,x,c} m psi(d)
//   dpred_i = scale * w_i * m * psi'(d)     psi' = sign(d) with sign(0) = 0,  2 d,  d / sqrt(d^2 + eps^2); every element written
//   sample_stats[b] = (sum mask * |p_k - t|_2, sum mask) of prediction k = metric_idx: the cut does not enter (metric.py:25-33)
//   pixel_out[b,y,x] = m * (psi(d_0) + psi(d_1)) / 2 of the single prediction (n == 1): the Reduction.NONE forward value
// in ONE launch.  Every operand is read through element strides (batch, channel, pixel), so NHWC [B,H,W,2] (2HW, 1, 2), planar
// [B,2,H,W] (2HW, HW, 1) and a [B,H,W,3] ground truth read in place (3HW, 1, 3; mask at base + 2 with (3HW, 3)) are the same
// kernel.  With a unit channel stride, even batch and pixel strides and 8-byte aligned bases a pixel's two floats travel as one
// 8-byte access (the predictions and their gradients decide together, the target on its own); anything else takes 4-byte accesses.
//
// Sums: fp32 in the thread, one float per workgroup into the caller's workspace, and the workgroup that arrives last adds the
// partials in float64 in workgroup order -- the same bits twice, whatever order the workgroups retire in.  blockIdx.y is the
// sample, so no workgroup straddles two samples and the per-sample sums are formed the same way.  The arrival counter is the first
// word of the workspace: zero before the first launch that uses a workspace, left zero by every launch.  Nothing else is shared
// between launches, so two launches on two streams with two workspaces do not disturb each other.
#include "common.hpp"
#include <cstddef>

namespace {

constexpr int FL_MAX_PRED = 32;
constexpr int FL_THREADS = 256;
constexpr int FL_MAX_WG = 2048;          // workgroups per sample; a sample beyond 2048 x 256 pixels takes strided further trips
constexpr int FL_MAX_B = 65535;          // gridDim.y
constexpr int FL_HEADER = 64;            // bytes in front of the partial sums (the arrival counter, kept on a line of its own)
constexpr int FL_UNROLL = 4;             // predictions loaded before the first of their gradients is stored

typedef float f32x2 __attribute__((ext_vector_type(2)));

struct FlowLossArgs {
  const float* pred[FL_MAX_PRED];
  float* dpred[FL_MAX_PRED];             // nullptr: no gradient for that prediction
  float w[FL_MAX_PRED];
  int n, metric_idx;                     // metric_idx -1: no statistics
  int64_t p_bs, p_cs, p_ps;
  const float* tgt;                      // nullptr: zero flow
  int64_t t_bs, t_cs, t_ps;
  const float* mask;                     // nullptr: ones
  int64_t m_bs, m_ps;
  float max_flow, eps2, scale;
  int B, HW;
  int vec_t;                             // the target's two floats as one 8-byte load
  float* out;                            // [1]
  float* stats;                          // [B][2] or nullptr
  float* pixel_out;                      // [B][HW] or nullptr (n == 1)
  unsigned int* ticket;                  // workspace + 0
  float* part;                           // workspace + FL_HEADER: [3][B * gridDim.x] loss, epe, mask
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sum of part[first], part[first + step], ... below n in that order, in float64, eight loads in flight; the loads are sc1
__device__ __forceinline__ double strided_sum(const float* part, unsigned int n, unsigned int first, unsigned int step) {
  double s = 0.0;
  for (unsigned int j = first; j < n; j += 8 * step) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = j + k * step < n ? __hip_atomic_load(&part[j + k * step], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += (double)v[k];
  }
  return s;
}

template <bool VEC>
__device__ __forceinline__ void load2(const float* p, int64_t cs, float& a, float& b) {
  if (VEC) {
    const f32x2 v = *(const FS_GLOBAL f32x2*)p;
    a = v.x; b = v.y;
  } else {
    a = gload1(p); b = gload1(p + cs);
  }
}

template <bool VEC>
__device__ __forceinline__ void store2(float* p, int64_t cs, float a, float b) {
  if (VEC) {
    f32x2 v; v.x = a; v.y = b;
    *(FS_GLOBAL f32x2*)p = v;
  } else {
    gstore1(p, a); gstore1(p + cs, b);
  }
}

// psi(d) and psi'(d)
template <int PEN>
__device__ __forceinline__ void penalty(float d, float eps2, float& psi, float& dpsi) {
  if (PEN == FSRAFT_FLOW_L1) {
    psi = fabsf(d);
    dpsi = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
  } else if (PEN == FSRAFT_FLOW_L2) {
    psi = d * d;
    dpsi = 2.0f * d;
  } else {
    psi = sqrtf(d * d + eps2);
    dpsi = d / psi;
  }
}

template <int PEN, bool VEC>
__global__ __launch_bounds__(FL_THREADS) void flow_loss_kernel(FlowLossArgs a) {
  __shared__ float red[FL_THREADS / 64][3];
  __shared__ double fin[FL_THREADS / 64];
  __shared__ bool last;
  const auto* karg = (const char __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr();
  typedef const float* cfptr;
  typedef float* fptr;
  const int b = blockIdx.y;
  const int64_t pb = (int64_t)b * a.p_bs;
  const float* tg = a.tgt ? a.tgt + (int64_t)b * a.t_bs : nullptr;
  const float* mk = a.mask ? a.mask + (int64_t)b * a.m_bs : nullptr;
  float acc_loss = 0.0f, acc_epe = 0.0f, acc_mask = 0.0f;
  for (int64_t e = (int64_t)blockIdx.x * FL_THREADS + threadIdx.x; e < a.HW; e += (int64_t)gridDim.x * FL_THREADS) {
    float t0 = 0.0f, t1 = 0.0f;
    if (tg) {
      if (a.vec_t) load2<true>(tg + e * a.t_ps, a.t_cs, t0, t1); else load2<false>(tg + e * a.t_ps, a.t_cs, t0, t1);
    }
    const float mv = mk ? gload1(mk + e * a.m_ps) : 1.0f;
    const bool in = !tg || sqrtf(t0 * t0 + t1 * t1) < a.max_flow;
    const float m = in ? mv : 0.0f;
    const int64_t po = pb + e * a.p_ps;
    for (int i0 = 0; i0 < a.n; i0 += FL_UNROLL) {                       // uniform trip counts, pointer tables via scalar loads
      float p0[FL_UNROLL] = {}, p1[FL_UNROLL] = {};
#pragma unroll
      for (int k = 0; k < FL_UNROLL; ++k) {
        if (i0 + k < a.n) {
          const float* p = ((const cfptr __attribute__((address_space(4)))*)(karg + offsetof(FlowLossArgs, pred)))[i0 + k];
          load2<VEC>(p + po, a.p_cs, p0[k], p1[k]);
        }
      }
#pragma unroll
      for (int k = 0; k < FL_UNROLL; ++k) {
        const int i = i0 + k;
        if (i < a.n) {
          float* dp = ((const fptr __attribute__((address_space(4)))*)(karg + offsetof(FlowLossArgs, dpred)))[i];
          const float wi = ((const float __attribute__((address_space(4)))*)(karg + offsetof(FlowLossArgs, w)))[i];
          const float d0 = p0[k] - t0, d1 = p1[k] - t1;
          float s0, s1, g0, g1;
          penalty<PEN>(d0, a.eps2, s0, g0);
          penalty<PEN>(d1, a.eps2, s1, g1);
          const float s = s0 + s1;
          if (m != 0.0f) acc_loss += wi * (m * s);
          if (dp) {
            const float c = (a.scale * wi) * m;
            store2<VEC>(dp + po, a.p_cs, m != 0.0f ? c * g0 : 0.0f, m != 0.0f ? c * g1 : 0.0f);   // (+0.0 where masked, not 0 * a slope)
          }
          if (i == a.metric_idx && mv != 0.0f) acc_epe += mv * sqrtf(d0 * d0 + d1 * d1);
          if (a.pixel_out) a.pixel_out[(int64_t)b * a.HW + e] = m != 0.0f ? m * (0.5f * s) : 0.0f;
        }
      }
    }
    acc_mask += mv;
  }
  acc_loss = wave_sum(acc_loss); acc_epe = wave_sum(acc_epe); acc_mask = wave_sum(acc_mask);
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6][0] = acc_loss; red[threadIdx.x >> 6][1] = acc_epe; red[threadIdx.x >> 6][2] = acc_mask;
  }
  __syncthreads();
  const unsigned int nwg = gridDim.x * gridDim.y;                       // <= 2048 * 65535 < 2^32
  // The partial sums are written through to memory (relaxed agent-scope atomic stores: sc1), the storing wave waits for them, and one
  // lane then draws a ticket: no release fence.  A release (__threadfence) writes back every dirty line of the XCD's L2, here the
  // gradients of all workgroups in flight, once per workgroup: 59 ns per workgroup serialised, 0.52 ms of a 0.1 ms kernel at
  // 8 x 368 x 768 with 12 predictions (profiles/flow_loss_ab_release_fence.txt).  The last arriver acquires once and reads with sc1 loads.
  if (threadIdx.x < 3) {
    __hip_atomic_store(&a.part[(int64_t)threadIdx.x * nwg + (int64_t)b * gridDim.x + blockIdx.x],
                       (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) last = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nwg - 1;
  __syncthreads();
  if (!last) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  // the loss: every thread takes partials tid, tid + 256, ... of all samples in ascending order
  double s = strided_sum(a.part, nwg, threadIdx.x, FL_THREADS);
  s = wave_sum_f64(s);
  if ((threadIdx.x & 63) == 0) fin[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    a.out[0] = (float)(((fin[0] + fin[1]) + (fin[2] + fin[3])) * (double)a.scale);
    *a.ticket = 0;
  }
  if (!a.stats) return;
  // the per-sample sums: wave v takes samples v, v + 4, ...; its lanes the sample's partials lane, lane + 64, ...
  const int lane = threadIdx.x & 63;
  for (int sb = threadIdx.x >> 6; sb < a.B; sb += FL_THREADS / 64) {
    const float* ps = a.part + (int64_t)nwg + (int64_t)sb * gridDim.x;
    double se = strided_sum(ps, gridDim.x, lane, 64), sm = strided_sum(ps + nwg, gridDim.x, lane, 64);
    se = wave_sum_f64(se); sm = wave_sum_f64(sm);
    if (lane == 0) { a.stats[2 * sb] = (float)se; a.stats[2 * sb + 1] = (float)sm; }
  }
}

static inline int fl_blocks(int64_t hw) {
  const int64_t n = (hw + FL_THREADS - 1) / FL_THREADS;
  return (int)(n < FL_MAX_WG ? n : FL_MAX_WG);
}

static inline bool fl_sizes_ok(int B, int H, int W) {
  return B >= 1 && B <= FL_MAX_B && H >= 1 && W >= 1 && (int64_t)H * W <= INT32_MAX;
}

static inline bool aligned8(const void* p) { return (uintptr_t)p % 8 == 0; }

template <int PEN>
static void fl_launch(bool vec, dim3 grid, hipStream_t s, const FlowLossArgs& a) {
  if (vec) hipLaunchKernelGGL((flow_loss_kernel<PEN, true>), grid, dim3(FL_THREADS), 0, s, a);
  else hipLaunchKernelGGL((flow_loss_kernel<PEN, false>), grid, dim3(FL_THREADS), 0, s, a);
}

}  // namespace

// 64 bytes (the arrival counter) + three floats per workgroup, rounded up to 64.
extern "C" int fsraft_flow_loss_workspace_bytes(int B, int H, int W) {
  if (!fl_sizes_ok(B, H, W)) return FS_ERR_ARG;
  const int64_t bytes = FL_HEADER + ((int64_t)B * fl_blocks((int64_t)H * W) * 3 * 4 + 63) / 64 * 64;
  return bytes > INT32_MAX ? FS_ERR_ARG : (int)bytes;
}

extern "C" int fsraft_flow_loss(const float* const* pred, float* const* dpred, const float* weights, int n,
                                int64_t pred_bs, int64_t pred_cs, int64_t pred_ps,
                                const float* target, int64_t target_bs, int64_t target_cs, int64_t target_ps,
                                const float* mask, int64_t mask_bs, int64_t mask_ps,
                                int penalty, float max_flow, float eps, float scale, int B, int H, int W,
                                float* out, float* sample_stats, int metric_idx, float* pixel_out,
                                void* workspace, int64_t workspace_bytes, hipStream_t s) {
  if (!pred || !weights || !out || !workspace || n < 1 || n > FL_MAX_PRED) return FS_ERR_ARG;
  if (penalty != FSRAFT_FLOW_L1 && penalty != FSRAFT_FLOW_L2 && penalty != FSRAFT_FLOW_ROBUST) return FS_ERR_ARG;
  if (pixel_out && n != 1) return FS_ERR_ARG;
  if (sample_stats && (metric_idx < 0 || metric_idx >= n)) return FS_ERR_ARG;
  const int need = fsraft_flow_loss_workspace_bytes(B, H, W);
  if (need == FS_ERR_ARG || workspace_bytes < need || !aligned8(workspace)) return FS_ERR_ARG;
  FlowLossArgs a{};
  bool vec = pred_cs == 1 && pred_bs % 2 == 0 && pred_ps % 2 == 0;
  for (int i = 0; i < n; ++i) {
    if (!pred[i]) return FS_ERR_ARG;
    a.pred[i] = pred[i]; a.dpred[i] = dpred ? dpred[i] : nullptr; a.w[i] = weights[i];
    vec = vec && aligned8(a.pred[i]) && aligned8(a.dpred[i]);
  }
  a.n = n; a.metric_idx = sample_stats ? metric_idx : -1;
  a.p_bs = pred_bs; a.p_cs = pred_cs; a.p_ps = pred_ps;
  a.tgt = target; a.t_bs = target_bs; a.t_cs = target_cs; a.t_ps = target_ps;
  a.mask = mask; a.m_bs = mask_bs; a.m_ps = mask_ps;
  a.max_flow = max_flow; a.eps2 = eps * eps; a.scale = scale;
  a.B = B; a.HW = H * W;
  a.vec_t = target && target_cs == 1 && target_bs % 2 == 0 && target_ps % 2 == 0 && aligned8(target);
  a.out = out; a.stats = sample_stats; a.pixel_out = pixel_out;
  a.ticket = (unsigned int*)workspace;
  a.part = (float*)((char*)workspace + FL_HEADER);
  const dim3 grid(fl_blocks((int64_t)H * W), B);
  if (penalty == FSRAFT_FLOW_L1) fl_launch<FSRAFT_FLOW_L1>(vec, grid, s, a);
  else if (penalty == FSRAFT_FLOW_L2) fl_launch<FSRAFT_FLOW_L2>(vec, grid, s, a);
  else fl_launch<FSRAFT_FLOW_ROBUST>(vec, grid, s, a);
  return fs_launch_status();
}
