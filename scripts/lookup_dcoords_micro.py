#!/usr/bin/env python3
"""Coordinate gradient of the lookup at the bench shape (4 pairs, 55x128, radius 4, 4 levels, flows of a few cells): the tiled
kernel of csrc/corr_dcoords.hip against the forward lookup kernel (the yardstick: it moves the same windows and writes the stream
this one reads) and against the torch composition a user would otherwise write (the reference's bilinear_sampler over the
row-major pyramid, forward + autograd backward w.r.t. the coordinates), all in one process, the two kernels alternating.
Times are device events around windows of N launches; the median of the rounds is reported with their spread.
usage: python scripts/lookup_dcoords_micro.py [B H W]      (needs the GPU; prints the lines profiles/lookup_dcoords.txt holds)"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from flow_supervisor_amd import ops  # noqa: E402
from flow_supervisor_amd.core.utils.utils import coords_grid  # noqa: E402

B, H, W = (int(v) for v in sys.argv[1:4]) if len(sys.argv) >= 4 else (4, 55, 128)
C, r, L = 256, 4, 4
N, ROUNDS = 200, 7
HBM_PEAK = 8e12
dev = "cuda"
torch.manual_seed(0)
f1 = torch.randn(B, C, H, W, device=dev)
f2 = torch.randn(B, C, H, W, device=dev)
# K flow fields in turn: a launch reads ~90 MB of windows, K of them do not fit the 256 MB Infinity Cache, so no launch finds
# the windows of the one before (the same flow every time would be timed out of the cache, for both kernels)
K = 4
flows = [(torch.rand(B, 2, H, W, device=dev) - 0.5) * 16 for _ in range(K)]
flow = flows[0]
ch = L * (2 * r + 1) ** 2
douts = [torch.randn(B, H, W, ch, device=dev) for _ in range(K)]
dout = douts[0]
turn = [0, 0]
vol, lay = ops.corr_build_tiled(f1, f2, L)
out = torch.empty(B, H, W, ch, device=dev)


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e-3


def fwd():
    turn[0] = (turn[0] + 1) % K
    ops.corr_lookup_tiled_fwd(vol, lay, flows[turn[0]], r, is_flow=True, out=out)


def dco():
    turn[1] = (turn[1] + 1) % K
    return ops.corr_lookup_tiled_dcoords(vol, lay, flows[turn[1]], douts[turn[1]], r, is_flow=True)


# the torch composition on the reference's row-major pyramid (pytorch/core/corr.py:29-50 + utils.py:57-71)
pyr = [lay.level_view(vol, l) for l in range(L)]
d = torch.linspace(-r, r, 2 * r + 1, device=dev)
delta = torch.stack(torch.meshgrid(d, d, indexing="ij"), dim=-1).view(1, 2 * r + 1, 2 * r + 1, 2)
dout_nchw = dout.permute(0, 3, 1, 2).contiguous()


def composition():
    c = (coords_grid(B, H, W, device=dev) + flow).requires_grad_()
    cl = c.permute(0, 2, 3, 1).reshape(B * H * W, 1, 1, 2)
    outs = []
    for i, lv in enumerate(pyr):
        g = cl / 2 ** i + delta
        h, w = lv.shape[-2:]
        grid = torch.cat([2 * g[..., :1] / (w - 1) - 1, 2 * g[..., 1:] / (h - 1) - 1], dim=-1)
        outs.append(F.grid_sample(lv, grid, align_corners=True).view(B, H, W, -1))
    o = torch.cat(outs, dim=-1).permute(0, 3, 1, 2).contiguous()
    o.backward(dout_nchw)
    return c.grad


# same numbers first (random flows: no sample sits on an integer, where the composition's own rounding picks the side)
got, ref = ops.corr_lookup_tiled_dcoords(vol, lay, flow, dout, r, is_flow=True), composition()
scale = ref.abs().max().item()
err = (got - ref).abs().max().item()
assert err <= 1e-4 * scale, (err, scale)
again = ops.corr_lookup_tiled_dcoords(vol, lay, flow, dout, r, is_flow=True)
assert torch.equal(got.view(torch.int32), again.view(torch.int32)), "two launches differ"

for fn in (fwd, dco):                       # warm-up of both kernels
    window(fn, 20)
t_f, t_d = [], []
for _ in range(ROUNDS):                     # alternating windows
    t_f.append(window(fwd, N))
    t_d.append(window(dco, N))
composition()
t_c = [window(composition, 3) for _ in range(3)]
nq = B * H * W
fb = 4.0 * nq * (L * (2 * r + 2) ** 2 + 2 + ch)
db = 4.0 * nq * (L * (2 * r + 2) ** 2 + 2 + ch + 2)
mf, md, mc = statistics.median(t_f), statistics.median(t_d), statistics.median(t_c)
print(f"shape {B}x{H}x{W}, radius {r}, {L} levels, {K} flow fields uniform in +-8 cells in turn; {ROUNDS} alternating windows of {N} launches, medians (min .. max)")
print(f"max |dcoords - torch composition| {err:.3e} (max |ref| {scale:.3e}); two launches bit-identical")
print(f"forward lookup (fsraft_corr_lookup_tiled_fwd)      {mf*1e6:8.1f} us  ({min(t_f)*1e6:.1f} .. {max(t_f)*1e6:.1f})   "
      f"{fb/mf/1e9:6.0f} GB/s algorithmic, {fb/mf/HBM_PEAK*100:4.1f} % of {HBM_PEAK/1e12:.0f} TB/s")
print(f"coordinate gradient (fsraft_corr_lookup_tiled_dcoords) {md*1e6:8.1f} us  ({min(t_d)*1e6:.1f} .. {max(t_d)*1e6:.1f})   "
      f"{db/md/1e9:6.0f} GB/s algorithmic, {db/md/HBM_PEAK*100:4.1f} % of {HBM_PEAK/1e12:.0f} TB/s")
print(f"torch composition, forward + backward to coords.grad  {mc*1e6:8.1f} us  ({min(t_c)*1e6:.1f} .. {max(t_c)*1e6:.1f})")
print(f"coordinate gradient / forward lookup = {md/mf:.2f} (expected within 1.5);  composition / coordinate gradient = {mc/md:.0f}")
