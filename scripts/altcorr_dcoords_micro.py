#!/usr/bin/env python3
"""Coordinate gradient of the memory-efficient lookup at the alt path's bench shape (1 pair, 47x156, C = 256, radius 4, 4 levels,
flows of a few cells): the kernel of csrc/altcorr_dcoords.hip against the wave-per-query fp32 forward (fsraft_altcorr_fused_fwd
without records and with the tile kernel switched off -- the yardstick: it reads the same fmap2 rows, with half the FMAs and a
butterfly) and against what a user has today for coords.grad: CorrBlock on the same maps, forward plus backward to coords.grad, with
and without the volume build it needs first.  One process, the two kernels alternating.  Times are device events around windows
of N launches; the median of the rounds is reported with their spread.
usage: python scripts/altcorr_dcoords_micro.py [B H W]      (needs the GPU; prints the lines profiles/altcorr_dcoords.txt holds)"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from flow_supervisor_amd import _lib, ops  # noqa: E402
from flow_supervisor_amd.core.corr import AlternateCorrBlock, CorrBlock  # noqa: E402
from flow_supervisor_amd.core.utils.utils import coords_grid  # noqa: E402

B, H, W = (int(v) for v in sys.argv[1:4]) if len(sys.argv) >= 4 else (1, 47, 156)
C, r, L = 256, 4, 4
N, ROUNDS = 100, 7
dev = "cuda"
torch.manual_seed(0)
f1 = torch.randn(B, C, H, W, device=dev)
f2 = torch.randn(B, C, H, W, device=dev)
blk = AlternateCorrBlock(f1, f2, num_levels=L, radius=r, coords_grad=True)
f1_cl, f2_cl = blk._f1, blk._f2
# K flow fields and output gradients in turn, so that no launch is served from the cache of the one before
K = 4
flows = [(torch.rand(B, 2, H, W, device=dev) - 0.5) * 16 for _ in range(K)]
ch = L * (2 * r + 1) ** 2
douts = [torch.randn(B, H, W, ch, device=dev) for _ in range(K)]
flow, dout = flows[0], douts[0]
turn = [0, 0]
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
    ops.altcorr_fused_fwd(f1_cl, f2_cl, flows[turn[0]], r, is_flow=True, out=out)


def dco():
    turn[1] = (turn[1] + 1) % K
    return ops.altcorr_fused_dcoords(f1_cl, f2_cl, flows[turn[1]], douts[turn[1]], r, is_flow=True)


built = []


def composition(build=True):
    if build or not built:
        built[:] = [CorrBlock(f1, f2, num_levels=L, radius=r)]
    c = (coords_grid(B, H, W, device=dev) + flow).requires_grad_()
    built[0](c, channels_last=True).backward(dout)
    return c.grad


# same numbers first: CorrBlock's coordinate gradient on the same maps (its volume is built in bf16x3: not bit for bit)
got, ref = ops.altcorr_fused_dcoords(f1_cl, f2_cl, flow, dout, r, is_flow=True), composition()
scale = ref.abs().max().item()
err = (got - ref).abs().max().item()
assert err <= 1e-3 * scale, (err, scale)
again = ops.altcorr_fused_dcoords(f1_cl, f2_cl, flow, dout, r, is_flow=True)
assert torch.equal(got.view(torch.int32), again.view(torch.int32)), "two launches differ"
c = (coords_grid(B, H, W, device=dev) + flow).requires_grad_()
blk(c, channels_last=True).backward(dout)
assert torch.equal(c.grad.view(torch.int32), got.view(torch.int32)), "AlternateCorrBlock(coords_grad=True) is not the kernel"

lib = _lib.load()
t_f, t_d, t_t = [], [], []
try:
    lib.fsraft_set_alt_tile(0)                  # the wave-per-query forward
    for fn in (fwd, dco):                       # warm-up of both kernels
        window(fn, 20)
    for _ in range(ROUNDS):                     # alternating windows
        t_f.append(window(fwd, N))
        t_d.append(window(dco, N))
finally:
    lib.fsraft_set_alt_tile(1)
window(fwd, 20)
t_t = [window(fwd, N) for _ in range(3)]        # for orientation: the fp32 tile forward (the default without records)
composition()
t_c = [window(composition, 3) for _ in range(3)]
t_l = [window(lambda: composition(build=False), 3) for _ in range(3)]
nq = B * H * W
maps = 4.0 * B * (H * W * C + sum(f.shape[1] * f.shape[2] for f in f2_cl) * C)
fb, db = maps + 4.0 * nq * (2 + ch), maps + 4.0 * nq * (2 + ch + 2)          # compulsory bytes (ops.TIMER's model)
rows = 4.0 * nq * L * (2 * r + 2) ** 2 * C                                    # what either kernel asks of the caches: every window row
flops = 2.0 * nq * L * (2 * r + 2) ** 2 * C
mf, md, mt, mc, ml = (statistics.median(t) for t in (t_f, t_d, t_t, t_c, t_l))
print(f"shape {B}x{H}x{W}, C {C}, radius {r}, {L} levels, {K} flow fields uniform in +-8 cells in turn; {ROUNDS} alternating windows of {N} launches, medians (min .. max)")
print(f"max |dcoords - CorrBlock coords.grad| {err:.3e} (max |ref| {scale:.3e}); two launches bit-identical")
print(f"forward, wave per query, fp32 (fsraft_altcorr_fused_fwd, tile off) {mf*1e6:8.1f} us  ({min(t_f)*1e6:.1f} .. {max(t_f)*1e6:.1f})   "
      f"{flops/mf/1e12:5.2f} TFLOP/s, {rows/mf/1e12:5.2f} TB/s of window rows, {fb/1e6:.1f} MB compulsory")
print(f"coordinate gradient (fsraft_altcorr_fused_dcoords)                 {md*1e6:8.1f} us  ({min(t_d)*1e6:.1f} .. {max(t_d)*1e6:.1f})   "
      f"{2*flops/md/1e12:5.2f} TFLOP/s, {rows/md/1e12:5.2f} TB/s of window rows, {db/1e6:.1f} MB compulsory")
print(f"forward, fp32 tile kernel (the default without records)            {mt*1e6:8.1f} us  ({min(t_t)*1e6:.1f} .. {max(t_t)*1e6:.1f})")
print(f"CorrBlock: volume build + lookup + backward to coords.grad         {mc*1e6:8.1f} us  ({min(t_c)*1e6:.1f} .. {max(t_c)*1e6:.1f})")
print(f"CorrBlock: lookup + backward to coords.grad, volume already built  {ml*1e6:8.1f} us  ({min(t_l)*1e6:.1f} .. {max(t_l)*1e6:.1f})")
print(f"coordinate gradient / wave-per-query forward = {md/mf:.2f} (expected within 1.5);  CorrBlock with its build / coordinate gradient = {mc/md:.1f}")
