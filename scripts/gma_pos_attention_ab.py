#!/usr/bin/env python3
"""A/B of the GMA attention call (forward_cl + backward) at the benchmark grid, 55 x 128 (N = 7040), B = 4:
the torch-composed positional route (gma.POS_HIP = False), the HIP positional route with each flag, and the content-only HIP
route.  Reported, not gated: median ms of >= 20 synchronised runs after warm-up and the peak allocated bytes of one call.

    python scripts/gma_pos_attention_ab.py [--out profiles/gma_pos_attention_ab.txt] [--runs 20] [--batch 4]

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
VARIANTS = [("content_only_hip", "none", True), ("pos_only_hip", "only", True), ("pos_both_hip", "both", True),
            ("pos_only_torch", "only", False), ("pos_both_torch", "both", False)]


def child(name, batch, runs, warmup):
    sys.path.insert(0, ROOT)
    import torch
    from flow_supervisor_amd.core import gma
    flag, hip = next((f, h) for n, f, h in VARIANTS if n == name)
    gma.POS_HIP = hip
    H, W, dev = 55, 128, "cuda"
    N = H * W
    args = argparse.Namespace(position_only=flag == "only", position_and_content=flag == "both")
    torch.manual_seed(0)
    att = gma.Attention(args=args, dim=128, heads=1, max_pos_size=160, dim_head=128).to(dev)
    x = torch.relu(torch.randn(batch, H, W, 128, device=dev) * 1.5)
    dA = torch.randn(batch, 1, N, N, device=dev)

    def call():
        xa = x.clone().requires_grad_(True)
        A = att.forward_cl(xa, records=True)
        g = dA.clone()
        g._fs_owned = True
        A.backward(g)

    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    call()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    ms = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(variant=name, ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms), runs=runs,
                          peak_mb=peak / 2 ** 20)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gma_pos_attention_ab.txt"))
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--variant")
    a = ap.parse_args()
    if a.variant:
        return child(a.variant, a.batch, max(a.runs, 20), a.warmup)
    rows = []
    for name, _, _ in VARIANTS:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--variant", name,
               "--batch", str(a.batch), "--runs", str(a.runs), "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"{name}: exit status {r.returncode}; stopping, nothing more is started")
        rows.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))
        print(rows[-1], flush=True)
    by = {r["variant"]: r for r in rows}
    lines = [f"GMA attention forward_cl(records=True) + backward, 55 x 128 (N = 7040), B = {a.batch}, MI355X; host clock around",
             f"synchronised calls, {a.warmup} warm-up calls, median of {max(a.runs, 20)} (min .. max); peak = allocated bytes of one call above its inputs",
             "", f"{'variant':<20}{'ms median':>12}{'min':>10}{'max':>10}{'peak MB':>12}"]
    lines += [f"{r['variant']:<20}{r['ms_median']:>12.2f}{r['ms_min']:>10.2f}{r['ms_max']:>10.2f}{r['peak_mb']:>12.1f}" for r in rows]
    lines.append("")
    for flag in ("only", "both"):
        hip, tor, base = by[f"pos_{flag}_hip"], by[f"pos_{flag}_torch"], by["content_only_hip"]
        verdict = "faster than" if hip["ms_median"] < tor["ms_median"] else "NOT faster than"
        lines.append(f"pos_{flag}: HIP route {hip['ms_median'] / tor['ms_median']:.2f}x the torch route's time ({verdict} it), "
                     f"{hip['ms_median'] - base['ms_median']:+.2f} ms against content-only; peak {hip['peak_mb']:.0f} MB vs "
                     f"{tor['peak_mb']:.0f} MB (torch) and {base['peak_mb']:.0f} MB (content-only)")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
