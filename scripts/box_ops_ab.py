#!/usr/bin/env python3
"""A/B of the list box copies and the bilinear resize of csrc/image_ops.hip at the flow-supervisor recipe's size: 12 predictions of
2 x 2 x 368 x 768 (planar) in 432 x 1024 frames, the two samples at different offsets.

    (a) per op, forward + backward
        crop    l2l._crop_back of the 12 full-frame predictions with l2l.BOX_OPS on (one fsraft_box_copy node) against off (the
                per-sample composition: B strided copies per prediction forward, a zero fill + B copies backward)
        pad     raft_tf.pad_bboxes of the 12 windows (one node) against the per-sample composition l2l._pad_state uses (B F.pad
                and a cat per tensor, autograd for the backward)
        resize  raft_tf.resize_flow of the 12 windows to the frame's size (one node) against F.interpolate(bilinear,
                align_corners=False) times the scale per prediction
    (b) step    train.SemiTrainStep on L2L, eager, the labelled and the unlabelled sample batched (their offsets differ), crop
                368 x 768 in 432 x 1024, 12 + 12 iterations, l2l.BOX_OPS on against off
    (c) kernel  the kernels' own times from `rocprofv3 --kernel-trace --stats`, in a run of its own, over the bytes each moves, as a
                share of the 6.3 TB/s a float4 copy reaches on an MI355X

    python scripts/box_ops_ab.py [--out profiles/box_ops_ab.txt] [--runs 9] [--no-profile]

Events around INNER calls on the current stream, ended by a device synchronise; warm-up first; the two sides of a pair alternate
inside one process, run by run; median and min .. max of the runs.  The parent process never touches the GPU: every part is a child
of its own under `timeout -k 10`, and the first child that fails ends the run.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, C, H, W, FH, FW, N = 2, 2, 368, 768, 432, 1024, 12
OX, OY = [136, 200], [40, 16]                  # the offsets bench.py gives the labelled and the unlabelled sample
INNER, STEP_INNER = 10, 2
HBM_MEASURED = 6.3e12                          # bytes / s a float4 copy reaches (MI355X)
WIN_BYTES, FRAME_BYTES = N * B * C * H * W * 4, N * B * C * FH * FW * 4
# bytes each kernel moves: what it reads plus what it writes (the resize's four taps come out of the caches)
KERNEL_BYTES = {"box_copy_kernel<false>": 2 * WIN_BYTES, "box_copy_kernel<true>": WIN_BYTES + FRAME_BYTES,
                "resize_fwd_kernel": WIN_BYTES + FRAME_BYTES, "resize_bwd_kernel": WIN_BYTES + FRAME_BYTES}
KERNEL_NAMES = {"box_copy_kernel<false>": "box copy, gather (crop forward, pad backward)",
                "box_copy_kernel<true>": "box copy, place (pad forward, crop backward)",
                "resize_fwd_kernel": "resize_flow forward", "resize_bwd_kernel": "resize_flow backward"}


def alternate(steps, runs, warmup, inner):
    """{name: [ms per call of every run]}, the sides taking turns run by run."""
    import torch
    for _ in range(warmup):
        for step in steps.values():
            step()
    torch.cuda.synchronize()
    ms = {k: [] for k in steps}
    for _ in range(runs):
        for k, step in steps.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                step()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / inner)
    return ms


def summary(v):
    return dict(ms_median=statistics.median(v), ms_min=min(v), ms_max=max(v))


def op_inputs():
    import torch
    g = torch.Generator().manual_seed(3)
    frames = [torch.randn(B, C, FH, FW, generator=g).cuda().requires_grad_(True) for _ in range(N)]
    wins = [torch.randn(B, C, H, W, generator=g).cuda().requires_grad_(True) for _ in range(N)]
    up_win = [torch.randn(B, C, H, W, generator=g).cuda() for _ in range(N)]
    up_frame = [torch.randn(B, C, FH, FW, generator=g).cuda() for _ in range(N)]
    return frames, wins, up_win, up_frame


def op_steps():
    """{op: {side: callable}} and the leaves whose gradients each op fills."""
    import torch
    import torch.nn.functional as F
    from flow_supervisor_amd import raft_tf
    from flow_supervisor_amd.core import l2l
    frames, wins, up_win, up_frame = op_inputs()
    yx = list(zip(OY, OX))
    last = {}

    def clear(ts):
        for t in ts:
            t.grad = None

    def crop(on):
        def fn():
            clear(frames)
            l2l.BOX_OPS = on
            out = l2l._crop_back(frames, OX, OY, (H, W))
            torch.autograd.backward(out, up_win)
            last["crop"] = out
        return fn

    def pad_hip():
        clear(wins)
        out = raft_tf.pad_bboxes(wins, yx, (FH, FW), "nchw")
        torch.autograd.backward(out, up_frame)
        last["pad"] = out

    def pad_torch():
        clear(wins)
        out = [torch.cat([F.pad(t[i:i + 1], (OX[i], FW - OX[i] - W, OY[i], FH - OY[i] - H)) for i in range(B)], 0) for t in wins]
        torch.autograd.backward(out, up_frame)
        last["pad"] = out

    def resize_hip():
        clear(wins)
        out = raft_tf.resize_flow(wins, (FH, FW), True, "nchw")
        torch.autograd.backward(out, up_frame)
        last["resize"] = out

    scale = torch.tensor([FW / W, FH / H], device="cuda").view(1, 2, 1, 1)

    def resize_torch():
        clear(wins)
        out = [F.interpolate(t, size=(FH, FW), mode="bilinear", align_corners=False) * scale for t in wins]
        torch.autograd.backward(out, up_frame)
        last["resize"] = out

    return ({"crop": {"hip": crop(True), "framework": crop(False)}, "pad": {"hip": pad_hip, "framework": pad_torch},
             "resize": {"hip": resize_hip, "framework": resize_torch}}, {"crop": frames, "pad": wins, "resize": wins}, last)


def child_ops(runs, warmup):
    sys.path.insert(0, ROOT)
    import torch
    steps, leaves, last = op_steps()
    rows = {}
    for op, sides in steps.items():
        ms = alternate(sides, runs, warmup, INNER)
        row = {k: summary(v) for k, v in ms.items()}
        for k, fn in sides.items():
            fn()
            row[k]["out_norm"] = float(torch.stack([o.detach().double().norm() for o in last[op]]).norm())
            row[k]["grad_norm"] = float(torch.stack([t.grad.double().norm() for t in leaves[op]]).norm())
        rows[op] = row
    print(json.dumps(rows))


def child_step(runs, warmup):
    sys.path.insert(0, ROOT)
    import torch
    from flow_supervisor_amd.core import l2l
    from flow_supervisor_amd.train import SemiTrainStep
    torch.manual_seed(0)
    model = l2l.L2L(argparse.Namespace(small=False, mixed_precision=False, alternate_corr=False)).cuda().train()
    model.freeze_bn()
    g = torch.Generator(device="cuda").manual_seed(1234)

    def pair():
        i1 = torch.rand(1, 3, FH, FW, device="cuda", generator=g) * 255.0
        i2 = (torch.roll(i1, shifts=(3, -5), dims=(2, 3)) + 2.0 * torch.randn(1, 3, FH, FW, device="cuda", generator=g)).clamp(0, 255)
        return i1, i2

    def sample(frame, oy, ox):
        f1, f2 = frame
        c1, c2 = (f[:, :, oy:oy + H, ox:ox + W].contiguous() for f in (f1, f2))
        return (c1, c2, f1, f2, ox, oy, torch.randn(1, 2, H, W, device="cuda", generator=g) * 4.0,
                (torch.rand(1, H, W, device="cuda", generator=g) > 0.1).float())

    sup, unsup = sample(pair(), OY[0], OX[0]), sample(pair(), OY[1], OX[1])
    # train_semi.sh:3-11, but lr 0: the weights stay, so the two sides' losses can be read against each other (the step's work does not
    # depend on the rate)
    step = SemiTrainStep(model, lr=0.0, wdecay=0.0, iters=12, gamma=0.8, unsup_lambda=1.0)
    last = {}

    def side(on):
        def fn():
            l2l.BOX_OPS = on
            last[on] = step(sup, unsup)
        return fn

    ms = alternate({"on": side(True), "off": side(False)}, runs, warmup, STEP_INNER)
    row = {k: summary(v) for k, v in ms.items()}
    for k, on in (("on", True), ("off", False)):
        row[k]["loss"] = [float(x) for x in last[on]]
    print(json.dumps(row))


def child_kernel(calls):
    """What the profiler watches: `calls` forward + backward passes of the three list ops, nothing else of size."""
    sys.path.insert(0, ROOT)
    import torch
    steps, _, _ = op_steps()
    for _ in range(calls):
        for op in steps.values():
            op["hip"]()
    torch.cuda.synchronize()


def run_child(cmd, limit):
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        sys.exit(f"{' '.join(cmd[-4:])}: exit status {r.returncode}; stopping, nothing more is started")
    return r.stdout


def kernel_stats(calls, limit, workdir):
    d = os.path.join(workdir, "box_ops_prof")
    shutil.rmtree(d, ignore_errors=True)
    run_child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--part", "kernel", "--calls", str(calls)], limit)
    found = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            for key in KERNEL_BYTES:
                if key in row["Name"]:
                    found[key] = dict(calls=int(row["Calls"]), avg_ns=float(row["AverageNs"]), min_ns=float(row["MinNs"]), max_ns=float(row["MaxNs"]))
    if len(found) != len(KERNEL_BYTES):
        sys.exit(f"the profiler's kernel statistics hold {sorted(found)} of {sorted(KERNEL_BYTES)}")
    return found


def last_json(out):
    return json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_ops_ab.txt"))
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--workdir", default=os.path.join(tempfile.gettempdir(), "box_ops_ab"), help="where the profiler's traces go")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--part")
    a = ap.parse_args()
    if a.part == "ops":
        return child_ops(a.runs, a.warmup)
    if a.part == "step":
        return child_step(a.runs, a.warmup)
    if a.part == "kernel":
        return child_kernel(a.calls)
    me = [sys.executable, os.path.abspath(__file__), "--runs", str(a.runs), "--warmup", str(a.warmup)]
    ops = last_json(run_child(me + ["--part", "ops"], a.step_timeout))
    step = last_json(run_child(me + ["--part", "step"], a.step_timeout))
    prof = None if a.no_profile else kernel_stats(a.calls, a.step_timeout, a.workdir)

    def line(name, r, tail=""):
        spread = (r["ms_max"] - r["ms_min"]) / r["ms_median"]
        return f"{name:<22}{r['ms_median']:>12.4f}{r['ms_min']:>10.4f}{r['ms_max']:>10.4f}{spread:>9.1%}{tail}"

    head = f"{'':<22}{'ms median':>12}{'min':>10}{'max':>10}{'spread':>9}"
    lines = [f"List box copies and bilinear resize, {N} predictions of {B} x {C} x {H} x {W} (planar) in {FH} x {FW} frames, offsets (y, x) "
             f"{list(zip(OY, OX))}, MI355X;", f"events around {INNER} calls ({STEP_INNER} steps in (b)) ended by a device synchronise, {a.warmup} warm-up "
             f"rounds, the two sides alternating in one process, median of {a.runs} runs", "(min .. max; spread = (max - min) / median).", "",
             "(a) per op, forward + backward: one list node on csrc/image_ops.hip (hip) against the framework composition",
             head + f"{'|out|':>14}{'|grad|':>14}"]
    what = {"crop": "l2l._crop_back, BOX_OPS on / off", "pad": "pad_bboxes / per-sample F.pad + cat", "resize": "resize_flow / F.interpolate * scale"}
    for op in ("crop", "pad", "resize"):
        r = ops[op]
        lines.append(f"  {op}: {what[op]}")
        for k in ("hip", "framework"):
            lines.append(line("    " + k, r[k], f"{r[k]['out_norm']:>14.6e}{r[k]['grad_norm']:>14.6e}"))
        lines.append(f"    hip takes {r['hip']['ms_median'] / r['framework']['ms_median']:.3f}x the composition's time "
                     f"({r['framework']['ms_median'] / r['hip']['ms_median']:.2f}x {'faster' if r['hip']['ms_median'] < r['framework']['ms_median'] else 'SLOWER'})")
    on, off = step["on"], step["off"]
    keep = on["ms_median"] <= off["ms_max"]
    lines += ["", f"(b) train.SemiTrainStep on L2L, eager, both samples in one batch, crop {H} x {W} in {FH} x {FW}, 12 + 12 iterations", head + "   losses (lr 0: equal up to the atomics of other kernels)",
              line("    BOX_OPS on", on, "   " + " ".join(f"{x:.6f}" for x in on["loss"])),
              line("    BOX_OPS off", off, "   " + " ".join(f"{x:.6f}" for x in off["loss"])),
              f"    on / off - 1 = {on['ms_median'] / off['ms_median'] - 1.0:+.2%} of the step; the median with the switch on "
              f"{'does not lie' if keep else 'LIES'} above the max of the runs with it off ({off['ms_max']:.4f} ms) -> BOX_OPS "
              f"{'stays on' if keep else 'ships off'}",
              "", f"(c) the kernels alone (rocprofv3 --kernel-trace --stats, a run of its own, {a.calls} passes), over the bytes each reads and writes;",
              f"    {HBM_MEASURED / 1e12:.1f} TB/s is what a float4 copy reaches.  The {N}-tensor working sets ({WIN_BYTES / 2 ** 20:.0f} MiB of windows, "
              f"{FRAME_BYTES / 2 ** 20:.0f} MiB of frames) fit", "    the 256 MiB Infinity Cache, so a share above 100% is not an error of measurement."]
    if prof:
        lines.append(f"    {'kernel':<48}{'calls':>6}{'us avg':>10}{'min':>9}{'max':>9}{'MiB':>8}{'TB/s':>8}{'of 6.3':>8}")
        for key, p in prof.items():
            rate = KERNEL_BYTES[key] / (p["avg_ns"] * 1e-9)
            lines.append(f"    {KERNEL_NAMES[key]:<48}{p['calls']:>6}{p['avg_ns'] / 1e3:>10.1f}{p['min_ns'] / 1e3:>9.1f}{p['max_ns'] / 1e3:>9.1f}"
                         f"{KERNEL_BYTES[key] / 2 ** 20:>8.0f}{rate / 1e12:>8.2f}{rate / HBM_MEASURED:>8.1%}")
    else:
        lines.append("    not measured (--no-profile)")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
