#!/usr/bin/env python3
"""A/B of the self-supervision term of the SMURF loss at the reference's recipe size: 4 windows of 368 x 768 in 432 x 1024 frames,
12 predictions per direction, 'gaussian' masks with the reference's sigmas, teacher masks included, forward plus backward:

    hip         flow_supervisor_amd.selfsup_loss (csrc/selfsup_loss.hip): one fsraft_fb_mask per direction for the teacher, one
                fsraft_selfsup per prediction and direction
    torch_ops   the same term composed of PyTorch-ROCm ops in fp32 on the same device: a four-tap gather for the resampler,
                elementwise ops for the masks, autograd for the gradient (the op sequence of tests/_selfsupref.py, copied here).
                Like the hip variant it forms the teacher's mask once per direction, not once per prediction.
    kernels     each entry point alone, with the achieved bytes / time against the HBM roof from the model bytes of DESIGN.md

    python scripts/selfsup_loss_ab.py [--out profiles/selfsup_loss_ab.txt] [--runs 7]

Events around each step on the current stream, warm-up steps first, median of the runs.  The parent process never touches the
GPU: every variant is a child of its own under `timeout -k 10`, and the first child that fails ends the run.  The run fails
unless hip is faster than torch_ops by more than the run-to-run spread (max / min over the runs) of either.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ["hip", "torch_ops", "kernels"]
B, H, W, HF, WF, N = 4, 368, 768, 432, 1024, 12
GAMMA, W_SELFSUP, SIGMA_T, SIGMA_S = 0.8, 0.3, 0.003, 0.03
CROPS = ((0, 0), (64, 256), (31, 77), (17, 200))
HBM_ROOF = 6.3e12                       # achievable bytes / s on an MI355X (8.0e12 is the specification)
# model bytes per window pixel (DESIGN.md "Self-supervision"): compulsory traffic, every plane once
MODEL_BYTES = {"fb_mask": 8 + 8 + 4, "selfsup": 8 + 8 + 8 + 4 + 8}


def inputs():
    import torch
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(0)

    def field(h, w, cells, amp):
        low = torch.rand(B, 2, h // cells + 1, w // cells + 1, generator=g)
        return amp * (F.interpolate(low, size=(h, w), mode="bilinear", align_corners=True) - 0.5)

    def pair(h, w, shift):
        f = field(h, w, 32, 12.0) + shift
        return f.cuda(), (-f + field(h, w, 16, 1.6)).cuda()

    teacher = pair(HF, WF, 0.0)
    fw, bw = zip(*[pair(H, W, 0.3 * t) for t in range(N)])
    return teacher, list(fw), list(bw)


# ---------------------------------------------------------------------------------------------- the composition of torch ops
def torch_loss_and_backward(teacher, fw, bw):
    import torch

    def coords(flow):
        h, w = flow.shape[-2:]
        ys, xs = torch.meshgrid(torch.arange(h, device=flow.device, dtype=flow.dtype),
                                torch.arange(w, device=flow.device, dtype=flow.dtype), indexing="ij")
        return xs + flow[:, 0], ys + flow[:, 1]

    def resample(frame, sx, sy):
        Bn, C, h, w = frame.shape
        x0, y0 = torch.floor(sx), torch.floor(sy)
        ox, oy = (sx - x0).unsqueeze(1), (sy - y0).unsqueeze(1)
        x0, y0 = x0.long(), y0.long()
        flat = frame.reshape(Bn, C, h * w)

        def tap(ix, iy):
            ok = ((ix >= 0) & (ix < w) & (iy >= 0) & (iy < h)).unsqueeze(1)
            idx = (iy.clamp(0, h - 1) * w + ix.clamp(0, w - 1)).view(Bn, 1, -1).expand(Bn, C, -1)
            return torch.gather(flat, 2, idx).view(Bn, C, *ix.shape[1:]) * ok.to(frame.dtype)

        return (((1.0 - ox) * (1.0 - oy) * tap(x0, y0) + ox * (1.0 - oy) * tap(x0 + 1, y0)) + (1.0 - ox) * oy * tap(x0, y0 + 1)) \
            + ox * oy * tap(x0 + 1, y0 + 1)

    def fb_mask(f, g, norm):
        h, w = f.shape[-2:]
        sx, sy = coords(f)
        r = resample(g, sx, sy)
        sq = ((f + r) ** 2).sum(1)
        valid = ((sx >= 0) & (sx <= w - 1) & (sy >= 0) & (sy <= h - 1)).to(f.dtype)
        return torch.exp(-sq / norm) * valid

    def crop(frame):
        return torch.stack([frame[b, :, cy:cy + H, cx:cx + W] for b, (cy, cx) in enumerate(CROPS)])

    size = float(HF) ** 2 + float(WF) ** 2
    with torch.no_grad():
        teacher_mask = [crop(fb_mask(teacher[i], teacher[j], SIGMA_T ** 2 * size).unsqueeze(1)) for i, j in ((0, 1), (1, 0))]
        teacher_flow = [crop(t) for t in teacher]
    total = 0.0
    for t in range(N):
        decay = GAMMA ** (N - 1 - t)
        for i, f, g in ((0, fw[t], bw[t]), (1, bw[t], fw[t])):
            with torch.no_grad():
                m = teacher_mask[i] * (1.0 - fb_mask(f, g, SIGMA_S ** 2 * size)).unsqueeze(1)
            term = decay * W_SELFSUP * (m * ((teacher_flow[i] - f) ** 2 + 0.001 ** 2) ** 0.5).mean() / 2.0
            term.backward()
            total = total + term.detach()
    return total


def timed(step, runs, warmup):
    import torch
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms), runs=runs)


def child(name, runs, warmup):
    sys.path.insert(0, ROOT)
    import torch
    from flow_supervisor_amd import ops
    from flow_supervisor_amd.selfsup_loss import SmurfLoss
    teacher, fw, bw = inputs()
    for f in fw + bw:
        f.requires_grad_(True)
    last = {}

    def clear():
        for f in fw + bw:
            f.grad = None

    if name == "hip":
        fn = SmurfLoss(census=0, smooth1=0, smooth2=0, selfsup=W_SELFSUP, gamma=GAMMA)
        frames = (teacher[0], teacher[0])           # only their presence is used when the census and smoothness weights are 0

        def step():
            clear()
            loss, _ = fn(None, fw, bw, *teacher, full_images=frames, crop_yx=CROPS)
            loss.backward()
            last["loss"] = loss.detach()

        row = timed(step, runs, warmup)
    elif name == "torch_ops":
        def step():
            clear()
            last["loss"] = torch_loss_and_backward(teacher, fw, bw)

        row = timed(step, runs, warmup)
    else:
        size = float(HF) ** 2 + float(WF) ** 2
        crop = ops.crop_offsets(CROPS, B)
        student, back = fw[0].detach(), bw[0].detach()
        mask = ops.fb_mask(*teacher, "gaussian", SIGMA_T ** 2 * size, False, (H, W), crop)
        calls = {"fb_mask": lambda: ops.fb_mask(*teacher, "gaussian", SIGMA_T ** 2 * size, False, (H, W), crop),
                 "selfsup": lambda: ops.selfsup(teacher[0], mask, student, back, "gaussian", SIGMA_S ** 2 * size, crop)}
        row = {"kernels": {k: timed(c, max(runs, 20), warmup) for k, c in calls.items()}}
    if "loss" in last:
        row["loss"] = float(last["loss"])
        row["grad_norm"] = float(torch.stack([f.grad.double().norm() for f in fw + bw]).norm())
        row["peak_GiB"] = torch.cuda.max_memory_allocated() / 2 ** 30
    print(json.dumps(dict(variant=name, **row)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "selfsup_loss_ab.txt"))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--variant")
    a = ap.parse_args()
    if a.variant:
        return child(a.variant, a.runs, a.warmup)
    rows = {}
    for name in VARIANTS:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--variant", name,
               "--runs", str(a.runs), "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"{name}: exit status {r.returncode}; stopping, nothing more is started")
        rows[name] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        print(rows[name], flush=True)
    hip, ref = rows["hip"], rows["torch_ops"]
    px = B * H * W
    spread = {k: r["ms_max"] / r["ms_min"] for k, r in (("hip", hip), ("torch_ops", ref))}
    ratio = ref["ms_median"] / hip["ms_median"]
    lines = [f"Self-supervision term of the SMURF loss, forward + backward, {B} windows of {H} x {W} in {HF} x {WF} frames, {N} predictions",
             f"per direction, 'gaussian' masks (sigma {SIGMA_T:g} / {SIGMA_S:g}), teacher masks included, MI355X; events around each step,",
             f"{a.warmup} warm-up steps, median of {a.runs} (min .. max).  hip: SmurfLoss with only the selfsup weight on",
             "csrc/selfsup_loss.hip; torch_ops: the same term composed of PyTorch-ROCm ops in fp32 (teacher mask once per direction).", "",
             f"{'variant':<12}{'ms median':>12}{'min':>10}{'max':>10}{'max/min':>9}{'loss':>14}{'|grad|':>14}{'peak GiB':>10}"]
    lines += [f"{k:<12}{r['ms_median']:>12.3f}{r['ms_min']:>10.3f}{r['ms_max']:>10.3f}{spread[k]:>9.3f}{r['loss']:>14.6e}{r['grad_norm']:>14.6e}"
              f"{r['peak_GiB']:>10.2f}" for k, r in (("hip", hip), ("torch_ops", ref))]
    lines += ["", f"hip takes {1.0 / ratio:.4f}x the composition's time ({ratio:.1f}x faster); run-to-run spread {max(spread.values()):.3f}", "",
              f"Per entry point, one call at {B} x {H} x {W}; model bytes per pixel from DESIGN.md; roof {HBM_ROOF / 1e12:.1f} TB/s achievable",
              f"{'entry':<12}{'ms median':>12}{'B/pixel':>9}{'TB/s':>8}{'of roof':>9}{'us at roof':>12}"]
    worst = 1.0
    for k, r in rows["kernels"]["kernels"].items():
        rate = MODEL_BYTES[k] * px / (r["ms_median"] * 1e-3)
        worst = min(worst, rate / HBM_ROOF)
        lines.append(f"{k:<12}{r['ms_median']:>12.4f}{MODEL_BYTES[k]:>9d}{rate / 1e12:>8.2f}{rate / HBM_ROOF:>9.1%}"
                     f"{MODEL_BYTES[k] * px / HBM_ROOF * 1e6:>12.1f}")
    lines += ["(one call through the Python wrapper: its allocations and the launches are inside the events; a call moves a few tens",
              " of MB, a handful of microseconds at the roof" + (", so launch latency, not bandwidth, sets these times)" if worst < 0.5 else ")")]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    if ratio <= max(spread.values()):
        sys.exit("hip is not faster than the composition by more than the run-to-run spread")


if __name__ == "__main__":
    main()
