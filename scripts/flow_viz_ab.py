#!/usr/bin/env python3
"""A/B of turning one prediction into a picture or a KITTI file's pixels: the device path (core/utils/flow_viz.flow_to_image
or ops.flow_kitti16 on the un-padded view of the padded prediction, plus the copy of the uint8 / uint16 result to the host)
against the host path it replaces (`padder.unpad(...).permute(1, 2, 0).cpu().numpy()` plus the NumPy colouring or encoding, as
restated in tests/_vizref.py; the reference itself is not needed).  At Sintel size, 436 x 1024 inside 440 x 1024, and at KITTI
size, 375 x 1242 inside 376 x 1248.

    python scripts/flow_viz_ab.py [--out profiles/flow_viz_ab.txt] [--runs 30]

One process.  The device path is timed between device events (kernels + device -> host copy into pinned memory; "kernels
alone" is the same without the copy), the host path by the host clock (it ends on the host).  Every path is warmed up at the
shape it is timed at; device and host runs alternate, so that both see the same neighbours on the machine; reported are the
median and the range of --runs repetitions.  No threshold beyond: the device path must not be slower than the host path.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"sintel": (436, 1024, "sintel"), "kitti": (375, 1242, "kitti")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_viz_ab.txt"))
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import _vizref as R
    from flow_supervisor_amd import ops
    from flow_supervisor_amd.core.utils import flow_viz
    from flow_supervisor_amd.core.utils.utils import InputPadder
    if not torch.cuda.is_available():
        sys.exit("flow_viz_ab: no GPU visible; nothing is measured without one")
    torch.manual_seed(0)

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    rows, notes = [], []
    for name, (H, W, mode) in SHAPES.items():
        padder = InputPadder((1, 3, H, W), mode=mode)
        Hp, Wp = H + -H % 8, W + -W % 8
        pred = torch.randn(1, 2, Hp, Wp, device="cuda") * 8.0
        view = padder.unpad(pred)
        assert view.shape == (1, 2, H, W)
        img_host = torch.empty(H, W, 3, dtype=torch.uint8).pin_memory()
        k16_host = torch.empty(H, W, 3, dtype=torch.int16).pin_memory()

        def dev_picture():
            img_host.copy_(flow_viz.flow_to_image(view[0]), non_blocking=True)

        def dev_picture_kernels():
            flow_viz.flow_to_image(view[0])

        def host_picture():
            return R.to_image(padder.unpad(pred[0]).permute(1, 2, 0).cpu().numpy())

        def dev_kitti():
            k16_host.copy_(ops.flow_kitti16(view)[0], non_blocking=True)

        def dev_kitti_kernels():
            ops.flow_kitti16(view)

        def host_kitti():
            return R.kitti16(padder.unpad(pred[0]).permute(1, 2, 0).cpu().numpy())

        # the two paths give the same result on what is timed
        dev_picture()
        dev_kitti()
        torch.cuda.synchronize()
        worst, differing, cap = R.two_part(img_host.numpy(), host_picture())
        assert worst <= 1 and differing <= cap, (worst, differing, cap)
        assert np.array_equal(k16_host.numpy().view(np.uint16), host_kitti())
        notes.append(f"{name}: device and host pictures differ on {differing} of {img_host.numel()} values (by at most {worst} level), "
                     "the KITTI arrays on none")

        paths = [("picture device (kernels + copy)", events, dev_picture), ("picture host (copy + NumPy)", clock, host_picture),
                 ("picture device, kernels alone", events, dev_picture_kernels),
                 ("kitti16 device (kernel + copy)", events, dev_kitti), ("kitti16 host (copy + NumPy)", clock, host_kitti),
                 ("kitti16 device, kernel alone", events, dev_kitti_kernels)]
        for _, _, fn in paths:
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {what: [] for what, _, _ in paths}
        for _ in range(a.runs):                       # alternating: one run of every path per round
            for what, timer, fn in paths:
                ms[what].append(timer(fn))
        for what, _, _ in paths:
            rows.append((name, f"{H} x {W} in {Hp} x {Wp}", what, statistics.median(ms[what]), min(ms[what]), max(ms[what])))

    by = {(r[0], r[2]): r[3] for r in rows}
    lines = ["Flow -> picture / KITTI pixels of one prediction, MI355X, one process; device paths between device events, host paths by the",
             f"host clock; {a.warmup} warm-up calls of every path at its shape, then {a.runs} rounds that run every path once (alternating);",
             "ms median (min .. max).  A device call is two or three launches over a few megabytes: its event interval is mostly the host's",
             "enqueue of them, so 'kernels alone' and 'kernels + copy' differ by less than that varies.", "",
             f"{'shape':<30}{'path':<36}{'ms median':>11}{'min':>9}{'max':>9}"]
    lines += [f"{r[1]:<30}{r[2]:<36}{r[3]:>11.3f}{r[4]:>9.3f}{r[5]:>9.3f}" for r in rows]
    lines.append("")
    for name in SHAPES:
        for kind in ("picture", "kitti16"):
            dev = by[(name, f"{kind} device ({'kernels' if kind == 'picture' else 'kernel'} + copy)")]
            host = by[(name, f"{kind} host (copy + NumPy)")]
            alone = by[(name, f"{kind} device, {'kernels' if kind == 'picture' else 'kernel'} alone")]
            verdict = "not slower" if dev <= host else "SLOWER"
            lines.append(f"{name} {kind}: device {dev:.3f} ms, host {host:.3f} ms: the device path is {verdict} ({host / dev:.1f}x); "
                         f"kernels alone {alone:.3f} ms")
    lines += [""] + notes
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
