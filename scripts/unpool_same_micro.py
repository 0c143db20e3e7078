"""A/B of the two un-pooling kernels on identical bytes: fsraft_corr_unpool_same_bwd against fsraft_corr_unpool_bwd at rows = 4608
(one sample of 48x96), 48x96, 4 levels, where the floor and the 'SAME' pyramid have the same sizes and both kernels are valid.  Device
events around windows of 100 launches, the two kernels alternating, 8 windows each; once on one volume launched again and again (85 MB
of level 0: it stays in the Infinity Cache) and once on four volumes in turn (450 MB: every launch reads HBM).  Bytes: level 0 read
and written, the other levels read.  Output kept in profiles/unpool_same_bwd.txt.  Needs an MI355X."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flow_supervisor_amd import _lib as L  # noqa: E402

lib = L.load()
H, W, nlev = 48, 96, 4
rows = H * W
sizes = [(H >> l, W >> l) for l in range(nlev)]
NSETS = 1 + 4                 # set 0: launched again and again (85 MB of level 0: it stays in the 256 MB Infinity Cache); sets 1..4 in turn (450 MB)
sets = [[torch.randn(rows, 1, h, w, device="cuda") for h, w in sizes] for _ in range(NSETS)]
pps = [L.ptr_array(lv) for lv in sets]
lv = sets[0]
pp = pps[0][0]
bytes_moved = 4 * (2 * lv[0].numel() + sum(t.numel() for t in lv[1:]))


def floor():
    assert lib.fsraft_corr_unpool_bwd(pp, nlev, 1, H, W, None) == 0


def same():
    assert lib.fsraft_corr_unpool_same_bwd(pp, nlev, rows, H, W, None) == 0


def window(fn, n=100):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3        # us per launch


def rotating(entry, args):
    def fn(state=[0]):
        state[0] = state[0] % 4 + 1
        assert entry(pps[state[0]][0], nlev, *args, None) == 0
    return fn


floor_rot, same_rot = rotating(lib.fsraft_corr_unpool_bwd, (1, H, W)), rotating(lib.fsraft_corr_unpool_same_bwd, (rows, H, W))
for fn in (floor, same, floor_rot, same_rot):
    window(fn, 20)
res = {"floor": [], "same": [], "floor, 4 volumes in turn": [], "same, 4 volumes in turn": []}
for _ in range(8):
    res["floor"].append(window(floor))
    res["same"].append(window(same))
    res["floor, 4 volumes in turn"].append(window(floor_rot))
    res["same, 4 volumes in turn"].append(window(same_rot))
    for st in sets:
        st[0].normal_()
out = []
for k, v in res.items():
    v = sorted(v)
    med = v[len(v) // 2]
    out.append(f"{k}: median {med:.1f} us  min {v[0]:.1f}  max {v[-1]:.1f}  -> {bytes_moved / med / 1e3:.0f} GB/s over {bytes_moved / 1e6:.1f} MB")
print("\n".join(out))
