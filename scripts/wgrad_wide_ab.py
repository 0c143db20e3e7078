#!/usr/bin/env python3
"""Same-process A/B of the wide per-tap weight-gradient tiles (fsraft_set_wgrad_wide 0 vs 2) per layer class of the benchmarked
step, at the step's shapes: `reps` launches captured in one hipGraph, REPEATS timed replays of each setting, alternating.
Prints one line per layer: median and spread (min .. max) of both settings, the tile that ran, and the ratio of the medians.
    python scripts/wgrad_wide_ab.py [reps] [name prefix]"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from flow_supervisor_amd import _lib, ops  # noqa: E402
from flow_supervisor_amd.ops import V  # noqa: E402

REPEATS = 5
dev = "cuda"
LAYERS = [  # class, B, H, W, kh, kw, source channels, Cout, segments
    ("five-tap x12 Cout=256  1x5 128+128->256", 4, 55, 128, 1, 5, [128, 128], 256, 12),
    ("five-tap x12 Cout=256  5x1 128+128->256", 4, 55, 128, 5, 1, [128, 128], 256, 12),
    ("five-tap x12 Cout=128  1x5 128+128->128", 4, 55, 128, 1, 5, [128, 128], 128, 12),
    ("five-tap x12 Cout=128  5x1 128+128->128", 4, 55, 128, 5, 1, [128, 128], 128, 12),
    ("1x1 256->576", 48, 55, 128, 1, 1, [256], 576, 1),
    ("1x1 324->256", 48, 55, 128, 1, 1, [324], 256, 1),
    ("2x2 256->96 (8x110x256)", 8, 110, 256, 2, 2, [256], 96, 1),
    ("2x2 256->96 (4x110x256)", 4, 110, 256, 2, 2, [256], 96, 1),
    ("2x2 384->128 (8x55x128)", 8, 55, 128, 2, 2, [384], 128, 1),
    ("2x2 384->128 (4x55x128)", 4, 55, 128, 2, 2, [384], 128, 1),
    ("single five-tap 1x5 128->256", 4, 55, 128, 1, 5, [128], 256, 1),
    ("single five-tap 5x1 128->128", 4, 55, 128, 5, 1, [128], 128, 1),
    ("small 1x1 98->128 (one column group: no wide tile)", 48, 55, 128, 1, 1, [98], 128, 1),
    ("small 1x1 128->256 (one column group: no wide tile)", 8, 55, 128, 1, 1, [128], 256, 1),
]
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
only = sys.argv[2] if len(sys.argv) > 2 else None
lib = _lib.load()
print(f"# fsraft_set_wgrad_wide 0 vs 2, hipGraph of {reps} launches, {REPEATS} alternating repeats; us per launch: median (min .. max)", flush=True)
try:
    for name, B, H, W, kh, kw, cs, cout, nseg in LAYERS:
        if only and not name.startswith(only):
            continue
        M = B * H * W
        dys = [V(torch.randn(B, H, W, (cout + 3) // 4 * 4, device=dev) * 0.1, cout) for _ in range(nseg)]
        xss = [[V(torch.randn(B, H, W, (c + 3) // 4 * 4, device=dev), c) for c in cs] for _ in range(nseg)]
        dwpk = torch.zeros(cout, ops.conv_ktot(cs, kh, kw), device=dev)
        dbias = torch.zeros(cout, device=dev)

        def run():
            if nseg > 1:
                ops.conv_wgrad_multi(dys, xss, dwpk, B, H, W, kh, kw, dbias=dbias)
            else:
                ops.conv_wgrad(dys[0], xss[0], dwpk, B, H, W, kh, kw, dbias=dbias)

        graphs, tiles = {}, {}
        for mode in (0, 2):
            lib.fsraft_set_wgrad_wide(mode)
            run()
            tiles[mode] = lib.fsraft_conv_wgrad_last_tile()
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                for _ in range(reps):
                    run()
            gr.replay()
            torch.cuda.synchronize()
            graphs[mode] = gr
        times = {0: [], 2: []}
        for _ in range(REPEATS):
            for mode in (0, 2):
                t0 = time.perf_counter()
                graphs[mode].replay()
                torch.cuda.synchronize()
                times[mode].append((time.perf_counter() - t0) / reps * 1e6)
        fl = 2.0 * M * cout * sum(cs) * kh * kw * nseg
        med = {m: statistics.median(t) for m, t in times.items()}
        line = f"{name:52s}"
        for mode in (0, 2):
            t = times[mode]
            line += f" | wide={mode} {tiles[mode] >> 16:3d}x{tiles[mode] & 0xffff:3d} {med[mode]:7.1f} ({min(t):7.1f} .. {max(t):7.1f}) us {fl / med[mode] / 1e6:6.1f} TF"
        win = max(times[2]) < min(times[0])
        print(line + f" | wide/128 {med[2] / med[0]:.3f} {'WIN' if win else 'no win'}", flush=True)
        del graphs, dys, xss
finally:
    lib.fsraft_set_wgrad_wide(1)
