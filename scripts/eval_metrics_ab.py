#!/usr/bin/env python3
"""A/B of one frame's validation metrics at Sintel size, 436 x 1024 read as the un-padded view of a 440 x 1024 prediction:
FlowMetrics.update (fsraft_flow_metrics, the statistics stay on the device) against the reference's composed route
(pytorch/evaluate.py:148-159: `.cpu()` of the prediction, then the torch formulas and the masked mean on the host).  Both do
the KITTI set of statistics (epe, |gt|, valid mask, outliers), the superset of what Sintel and Chairs need.  Reported, not
gated: median ms of >= 20 synchronised calls after warm-up.

    python scripts/eval_metrics_ab.py [--out profiles/eval_metrics_ab.txt] [--runs 20]

The parent process never touches the GPU: every variant is a child of its own under `timeout -k 10`, and the first child that
fails ends the run (nothing more is started on a device that has just faulted or hung).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ["hip_update", "hip_update_enqueue_only", "reference_host"]
H, W, HP, WP, TOP = 436, 1024, 440, 1024, 2


def child(name, runs, warmup):
    sys.path.insert(0, ROOT)
    import torch
    from flow_supervisor_amd.evaluate import FlowMetrics
    torch.manual_seed(0)
    gt = torch.randn(2, H, W) * 8.0
    valid = (torch.rand(H, W) < 0.7).float()
    frame = torch.randn(1, 2, HP, WP, device="cuda") * 8.0
    pred = frame[:, :, TOP:TOP + H]                      # what InputPadder.unpad returns
    gt_dev, valid_dev = gt.cuda(), valid.cuda()
    metrics = FlowMetrics()

    def hip():
        metrics.update(pred, gt_dev, valid_dev)

    def host():
        flow = pred[0].cpu()
        epe = torch.sum((flow - gt) ** 2, dim=0).sqrt().view(-1)
        mag = torch.sum(gt ** 2, dim=0).sqrt().view(-1)
        val = valid.view(-1) >= 0.5
        out = ((epe > 3.0) & ((epe / mag) > 0.05)).float()
        return epe[val].mean().item(), out[val].cpu().numpy()

    call = host if name == "reference_host" else hip
    sync = name != "hip_update_enqueue_only"
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        if sync:
            torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    print(json.dumps(dict(variant=name, ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms), runs=runs)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_metrics_ab.txt"))
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=120)
    ap.add_argument("--variant")
    a = ap.parse_args()
    if a.variant:
        return child(a.variant, max(a.runs, 20), a.warmup)
    rows = []
    for name in VARIANTS:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--variant", name,
               "--runs", str(a.runs), "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"{name}: exit status {r.returncode}; stopping, nothing more is started")
        rows.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))
        print(rows[-1], flush=True)
    by = {r["variant"]: r for r in rows}
    lines = [f"Validation metrics of one frame, {H} x {W} read from a {HP} x {WP} padded prediction, KITTI statistics, MI355X; host clock",
             f"around each call, {a.warmup} warm-up calls, median of {max(a.runs, 20)} (min .. max).  hip_update: FlowMetrics.update + a",
             "synchronise; hip_update_enqueue_only: the same without one (what a validation loop pays per frame); reference_host: the",
             "reference's .cpu() copy of the prediction and its torch formulas on the host.", "",
             f"{'variant':<28}{'ms median':>12}{'min':>10}{'max':>10}"]
    lines += [f"{r['variant']:<28}{r['ms_median']:>12.3f}{r['ms_min']:>10.3f}{r['ms_max']:>10.3f}" for r in rows]
    lines += ["", f"hip_update takes {by['hip_update']['ms_median'] / by['reference_host']['ms_median']:.3f}x the reference route's time"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
