#!/usr/bin/env python3
"""A/B of the TF tree's sequence loss at the recipe's size: 368 x 768 crops, 12 predictions, B = 1 and 8, forward plus backward.

    (a) hip        raft_tf.flow_sequence_loss, l2 / NHWC, [B,H,W,3] ground truth read in place (csrc/flow_loss.hip: one launch,
                   one _foreach_mul_ in backward)
        torch_ops  the same objective composed of PyTorch-ROCm ops in fp32 on the same device (the op sequence of raft/loss.py
                   FlowLossL2 under Keras' mean, summed with the decay weights, autograd for the gradients).  One favour the
                   reference does not take: mask * (|gt| < 400) is formed once, not once per prediction.
    (b) kernel     the kernel's own time from `rocprofv3 --kernel-trace --stats`, in a run of its own per batch size, over the model
                   bytes n * (8 + 8 [gradient]) + 8 + 4 [mask] per pixel, as a share of the HBM rate of an MI355X
    (c) planar     the new entry in robust / planar / mean mode against fsraft_sequence_loss (train.weighted_sequence_loss) on
                   identical inputs with a 0 / 1 mask: the same bytes

    python scripts/flow_loss_ab.py [--out profiles/flow_loss_ab.txt] [--runs 9] [--no-profile]

Events around INNER steps on the current stream, ended by a device synchronise; warm-up first; the two sides of a pair alternate
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
H, W, N = 368, 768, 12
BATCHES = (1, 8)
GAMMA = 0.8
INNER = 10
HBM_SPEC, HBM_MEASURED = 8.0e12, 6.3e12       # bytes / s: the specification, and what a float4 copy reaches (MI355X)
MODEL_BYTES = N * (8 + 8) + 8 + 4             # per pixel: every prediction read, every gradient written, the target, the mask


def inputs(B, planar=False):
    import torch
    g = torch.Generator().manual_seed(B)
    gt = 4.0 * torch.randn(B, H, W, 2, generator=g)
    gt[:, :2] = 500.0                                         # rows beyond the cut
    mask = (torch.rand(B, H, W, 1, generator=g) > 0.2).float()
    preds = [gt + 3.0 * torch.randn(B, H, W, 2, generator=g) for _ in range(N)]
    if planar:
        return [p.permute(0, 3, 1, 2).contiguous().cuda().requires_grad_(True) for p in preds], \
            gt.permute(0, 3, 1, 2).contiguous().cuda(), mask[..., 0].contiguous().cuda()
    return [p.cuda().requires_grad_(True) for p in preds], torch.cat((gt, mask), 3).cuda(), None


def torch_l2_loss(preds, y, w):
    import torch
    flow, mask = y[..., 0:2], y[..., 2:3]
    m = mask * (torch.sqrt(torch.sum(flow ** 2, dim=-1, keepdim=True)) < 400).to(mask.dtype)
    loss = 0.0
    for wi, p in zip(w, preds):
        a = torch.square(p - flow) * m
        per_pixel = torch.mean(a, dim=3)
        loss = loss + wi * (per_pixel.sum() / per_pixel.numel())
    return loss


def alternate(steps, runs, warmup):
    """{name: [ms per step of every run]}, the sides taking turns run by run."""
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
            for _ in range(INNER):
                step()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / INNER)
    return ms


def summary(v):
    return dict(ms_median=statistics.median(v), ms_min=min(v), ms_max=max(v))


def child_ab(runs, warmup):
    sys.path.insert(0, ROOT)
    import torch
    from flow_supervisor_amd import raft_tf, train
    w = [GAMMA ** (N - i - 1) for i in range(N)]
    rows = {}
    for B in BATCHES:
        preds, y, _ = inputs(B)
        last = {}

        def clear(ps):
            for p in ps:
                p.grad = None

        def hip():
            clear(preds)
            last["hip"] = raft_tf.flow_sequence_loss(preds, y, w, "l2", "mean", "nhwc")
            last["hip"].backward()

        def torch_ops():
            clear(preds)
            last["torch_ops"] = torch_l2_loss(preds, y, w)
            last["torch_ops"].backward()

        ms = alternate({"hip": hip, "torch_ops": torch_ops}, runs, warmup)
        row = {k: summary(v) for k, v in ms.items()}
        for k, step in (("hip", hip), ("torch_ops", torch_ops)):
            step()
            row[k]["loss"] = float(last[k])
            row[k]["grad_norm"] = float(torch.stack([p.grad.double().norm() for p in preds]).norm())
        rows[f"a{B}"] = row
        del preds, y
        pp, gt, valid = inputs(B, planar=True)

        def new():
            clear(pp)
            last["new"] = raft_tf.flow_sequence_loss(pp, (gt, valid), w, "robust", "mean", "nchw")
            last["new"].backward()

        def old():
            clear(pp)
            last["old"] = train.weighted_sequence_loss(pp, w, gt, valid)[0]
            last["old"].backward()

        ms = alternate({"new": new, "old": old}, runs, warmup)
        row = {k: summary(v) for k, v in ms.items()}
        for k, step in (("new", new), ("old", old)):
            step()
            row[k]["loss"] = float(last[k])
            row[k]["grad_norm"] = float(torch.stack([p.grad.double().norm() for p in pp]).norm())
        rows[f"c{B}"] = row
        del pp, gt, valid
    print(json.dumps(rows))


def child_kernel(B, calls):
    """What the profiler watches: `calls` forward launches (gradients written) of the l2 / NHWC case, nothing else of size."""
    sys.path.insert(0, ROOT)
    import torch
    from flow_supervisor_amd import raft_tf
    preds, y, _ = inputs(B)
    w = [GAMMA ** (N - i - 1) for i in range(N)]
    for _ in range(calls):
        raft_tf.flow_sequence_loss(preds, y, w, "l2", "mean", "nhwc")
    torch.cuda.synchronize()


def run_child(cmd, limit):
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        sys.exit(f"{' '.join(cmd[-4:])}: exit status {r.returncode}; stopping, nothing more is started")
    return r.stdout


def kernel_stats(B, calls, limit, workdir):
    d = os.path.join(workdir, f"flow_loss_prof_b{B}")
    shutil.rmtree(d, ignore_errors=True)
    run_child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--part", "kernel", "--batch", str(B), "--calls", str(calls)], limit)
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if "flow_loss_kernel" in row["Name"]:
                return dict(calls=int(row["Calls"]), avg_ns=float(row["AverageNs"]), min_ns=float(row["MinNs"]), max_ns=float(row["MaxNs"]))
    sys.exit("no flow_loss_kernel row in the profiler's kernel statistics")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_loss_ab.txt"))
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--workdir", default=os.path.join(tempfile.gettempdir(), "flow_loss_ab"), help="where the profiler's traces go")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--part")
    ap.add_argument("--batch", type=int, default=1)
    a = ap.parse_args()
    if a.part == "ab":
        return child_ab(a.runs, a.warmup)
    if a.part == "kernel":
        return child_kernel(a.batch, a.calls)
    out = run_child([sys.executable, os.path.abspath(__file__), "--part", "ab", "--runs", str(a.runs), "--warmup", str(a.warmup)], a.step_timeout)
    rows = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
    prof = {} if a.no_profile else {B: kernel_stats(B, a.calls, a.step_timeout, a.workdir) for B in BATCHES}

    def spread(r):
        return (r["ms_max"] - r["ms_min"]) / r["ms_median"]

    head = f"{'B':>3} {'variant':<12}{'ms median':>12}{'min':>10}{'max':>10}{'spread':>9}{'loss':>14}{'|grad|':>14}"
    lines = [f"Sequence loss of the TF tree, forward + backward, {N} predictions of {H} x {W}, MI355X; events around {INNER} steps ended by a",
             f"device synchronise, {a.warmup} warm-up rounds, the two sides alternating in one process, median of {a.runs} runs (min .. max;",
             "spread = (max - min) / median).", "",
             "(a) l2 / NHWC / [B,H,W,3] ground truth: raft_tf.flow_sequence_loss (hip) against the same objective composed of PyTorch-ROCm ops",
             head]
    slower = False
    for B in BATCHES:
        r = rows[f"a{B}"]
        for k in ("hip", "torch_ops"):
            lines.append(f"{B:>3} {k:<12}{r[k]['ms_median']:>12.4f}{r[k]['ms_min']:>10.4f}{r[k]['ms_max']:>10.4f}{spread(r[k]):>9.1%}"
                         f"{r[k]['loss']:>14.6f}{r[k]['grad_norm']:>14.6e}")
        lines.append(f"    B = {B}: hip takes {r['hip']['ms_median'] / r['torch_ops']['ms_median']:.4f}x the composition's time "
                     f"({r['torch_ops']['ms_median'] / r['hip']['ms_median']:.1f}x faster)")
        slower = slower or r["hip"]["ms_median"] >= r["torch_ops"]["ms_median"]
    lines += ["", f"(b) the kernel alone (rocprofv3 --kernel-trace --stats, a run of its own per batch size, {a.calls} launches), model bytes",
              f"    {MODEL_BYTES} per pixel = {N} x (8 read + 8 gradient written) + 8 target + 4 mask; HBM: {HBM_SPEC / 1e12:.1f} TB/s specified,",
              f"    {HBM_MEASURED / 1e12:.1f} TB/s reached by a float4 copy"]
    if prof:
        lines.append(f"{'B':>3}{'us avg':>10}{'min':>9}{'max':>9}{'TB/s':>8}{'of 8.0':>8}{'of 6.3':>8}")
        for B in BATCHES:
            p = prof[B]
            rate = MODEL_BYTES * B * H * W / (p["avg_ns"] * 1e-9)
            lines.append(f"{B:>3}{p['avg_ns'] / 1e3:>10.1f}{p['min_ns'] / 1e3:>9.1f}{p['max_ns'] / 1e3:>9.1f}{rate / 1e12:>8.2f}"
                         f"{rate / HBM_SPEC:>8.1%}{rate / HBM_MEASURED:>8.1%}")
        lines.append("    (a share of the HBM rate only where the working set exceeds the 256 MiB Infinity Cache: B = 1 moves "
                     f"{MODEL_BYTES * H * W / 2 ** 20:.0f} MiB, B = 8 {MODEL_BYTES * 8 * H * W / 2 ** 20:.0f} MiB)")
    else:
        lines.append("    not measured (--no-profile)")
    lines += ["", "(c) robust / planar / mean, 0 / 1 mask: the new entry (flow_sequence_loss, layout 'nchw') against fsraft_sequence_loss",
              "    (train.weighted_sequence_loss) on identical inputs; both move the same bytes", head]
    for B in BATCHES:
        r = rows[f"c{B}"]
        for k in ("new", "old"):
            lines.append(f"{B:>3} {k:<12}{r[k]['ms_median']:>12.4f}{r[k]['ms_min']:>10.4f}{r[k]['ms_max']:>10.4f}{spread(r[k]):>9.1%}"
                         f"{r[k]['loss']:>14.6f}{r[k]['grad_norm']:>14.6e}")
        diff = r["new"]["ms_median"] / r["old"]["ms_median"] - 1.0
        lines.append(f"    B = {B}: new / old - 1 = {diff:+.1%}; the old entry's run-to-run spread is {spread(r['old']):.1%} -> "
                     f"{'within' if abs(diff) <= spread(r['old']) else 'OUTSIDE'} it")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    if slower:
        sys.exit("the fused path is not faster than the composition")


if __name__ == "__main__":
    main()
