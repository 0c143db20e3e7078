#!/usr/bin/env python3
"""A/B of the unsupervised (SMURF) loss at the training size: 4 pairs of 440 x 1024, 12 predictions per direction, the default
weights (census 1, smooth1 2.5, 'wang' occlusion), forward plus backward:

    hip         flow_supervisor_amd.unsup_loss.UnsupervisedLoss (csrc/unsup_loss.hip)
    torch_ops   the same loss composed of PyTorch-ROCm ops in fp32 on the same device: unfold for the census transform, a four-tap
                gather for the warp, index_add_ for the range map, autograd for the gradients (the op sequence of
                tests/_unsupref.py, copied here).  It is given two favours the reference does not take: the census transform of the
                un-warped image is computed once per direction, not once per prediction, and every term is backpropagated as soon
                as it is formed, so that only one term's 49-channel tensors are alive at a time.
    kernels     every entry point alone, with the achieved bytes / time against the HBM roof from the model bytes of DESIGN.md

    python scripts/unsup_loss_ab.py [--out profiles/unsup_loss_ab.txt] [--runs 7]

Events around each step on the current stream, warm-up steps first, median of the runs.  The parent process never touches the
GPU: every variant is a child of its own under `timeout -k 10`, and the first child that fails ends the run.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ["hip", "torch_ops", "kernels"]
B, H, W, N = 4, 440, 1024, 12
GAMMA, W_CENSUS, W_SMOOTH1 = 0.8, 1.0, 2.5
HBM_ROOF = 6.3e12                       # achievable bytes / s on an MI355X (8.0e12 is the specification)
# model bytes per pixel (DESIGN.md "Unsupervised loss"): compulsory traffic, every plane once
MODEL_BYTES = {"range_map": 8 + 8 + 8 + 4, "census_fwd": 12 + 12 + 8 + 4 + 4 + 4, "census_bwd": 12 + 12 + 8 + 4 + 4 + 8,
               "smoothness": 12 + 8 + 8}


def inputs():
    import torch
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(0)

    def field(c, cells, amp):
        low = torch.rand(B, c, H // cells + 1, W // cells + 1, generator=g)
        return amp * F.interpolate(low, size=(H, W), mode="bilinear", align_corners=True)

    images = [(0.3 + field(3, 8, 0.1) + 0.05 * torch.rand(B, 3, H, W, generator=g)).clamp(0, 1).cuda() for _ in range(2)]
    flows = [[(field(2, 32, 12.0) - 6.0 + 0.3 * t).cuda() for t in range(N)] for _ in range(2)]
    return images, flows


# ---------------------------------------------------------------------------------------------- the composition of torch ops
def torch_loss_and_backward(images, fw, bw):
    import torch
    import torch.nn.functional as F

    def coords(flow):
        ys, xs = torch.meshgrid(torch.arange(H, device=flow.device, dtype=flow.dtype),
                                torch.arange(W, device=flow.device, dtype=flow.dtype), indexing="ij")
        return xs + flow[:, 0], ys + flow[:, 1]

    def range_map(flow):
        cx, cy = coords(flow)
        x0, y0 = torch.floor(cx), torch.floor(cy)
        ox, oy = (cx - x0).reshape(-1), (cy - y0).reshape(-1)
        x0, y0 = x0.long().reshape(-1), y0.long().reshape(-1)
        base = (torch.arange(B, device=flow.device).view(B, 1, 1) * H * W).expand(B, H, W).reshape(-1)
        idxs, weights = [], []
        for di in range(2):
            for dj in range(2):
                i, j = y0 + di, x0 + dj
                m = (i >= 0) & (i < H) & (j >= 0) & (j < W)
                idxs.append((base + i * W + j)[m])
                weights.append(((1.0 - di) - (-1) ** di * oy[m]) * ((1.0 - dj) - (-1) ** dj * ox[m]))
        out = torch.zeros(B * H * W, device=flow.device, dtype=flow.dtype)
        out.index_add_(0, torch.cat(idxs), torch.cat(weights))
        return out.view(B, H, W)

    def resample(frame, sx, sy):
        x0, y0 = torch.floor(sx), torch.floor(sy)
        ox, oy = (sx - x0).unsqueeze(1), (sy - y0).unsqueeze(1)
        x0, y0 = x0.detach().long(), y0.detach().long()
        flat = frame.reshape(B, 3, H * W)

        def tap(ix, iy):
            ok = ((ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)).unsqueeze(1)
            idx = (iy.clamp(0, H - 1) * W + ix.clamp(0, W - 1)).view(B, 1, -1).expand(B, 3, -1)
            return torch.gather(flat, 2, idx).view(B, 3, H, W) * ok.to(frame.dtype)

        return (((1.0 - ox) * (1.0 - oy) * tap(x0, y0) + ox * (1.0 - oy) * tap(x0 + 1, y0)) + (1.0 - ox) * oy * tap(x0, y0 + 1)) \
            + ox * oy * tap(x0 + 1, y0 + 1)

    def census_transform(img):
        gray = 255.0 * (0.2989 * img[:, 0:1] + 0.5870 * img[:, 1:2] + 0.1140 * img[:, 2:3])
        diff = F.unfold(gray, 7, padding=3).view(B, 49, H, W) - gray
        return diff / torch.sqrt(0.81 + diff ** 2)

    def census(census_a, frame2, flow, mask):
        sx, sy = coords(flow)
        valid = ((sx >= 0) & (sx <= W - 1) & (sy >= 0) & (sy <= H - 1)).to(flow.dtype)
        M = (mask * valid).detach()
        border = torch.zeros_like(M)
        border[:, 3:-3, 3:-3] = 1.0
        M = M * border
        u = census_a - census_transform(resample(frame2, sx, sy))
        ham = (u ** 2 / (0.1 + u ** 2)).sum(1)
        return (((ham.abs() + 0.01) ** 0.4) * M).sum() / (M + 1e-6).sum()

    def smooth1(image, flow):
        def grads(t):
            return t[:, :, 1:] - t[:, :, :-1], t[:, :, :, 1:] - t[:, :, :, :-1]

        def weight(d):
            return torch.exp(-(150.0 * d).abs().mean(1, keepdim=True))

        ih, iw = grads(image)
        fh, fw_ = grads(flow)
        return ((weight(ih) * (fh ** 2 + 0.001 ** 2) ** 0.5).mean() + (weight(iw) * (fw_ ** 2 + 0.001 ** 2) ** 0.5).mean()) / 2.0

    total = 0.0
    with torch.no_grad():
        census_of = [census_transform(im) for im in images]
    for t in range(N):
        decay = GAMMA ** (N - 1 - t)
        for i, j, f, g in ((0, 1, fw[t], bw[t]), (1, 0, bw[t], fw[t])):
            with torch.no_grad():
                mask = range_map(g).clamp(0.0, 1.0)
            term = decay * (W_CENSUS * census(census_of[i], images[j], f, mask) + W_SMOOTH1 * smooth1(images[i], f)) / 2.0
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
    from flow_supervisor_amd.unsup_loss import UnsupervisedLoss
    images, (fw, bw) = inputs()
    for f in fw + bw:
        f.requires_grad_(True)
    last = {}

    def clear():
        for f in fw + bw:
            f.grad = None

    if name == "hip":
        fn = UnsupervisedLoss()

        def step():
            clear()
            loss, _ = fn(images, fw, bw)
            loss.backward()
            last["loss"] = loss.detach()

        row = timed(step, runs, warmup)
    elif name == "torch_ops":
        def step():
            clear()
            last["loss"] = torch_loss_and_backward(images, fw, bw)

        row = timed(step, runs, warmup)
    else:
        flow = fw[0].detach()
        mask = ops.range_map(bw[0].detach(), clip=True)
        out, gB, hp = ops.census_fwd(images[0], images[1], flow, mask)
        up = torch.ones((), device="cuda")
        calls = {"range_map": lambda: ops.range_map(flow, clip=True),
                 "census_fwd": lambda: ops.census_fwd(images[0], images[1], flow, mask),
                 "census_bwd": lambda: ops.census_bwd(images[0], images[1], flow, gB, hp, up, out[1:]),
                 "smoothness": lambda: ops.smoothness(images[0], flow, 1)}
        row = {"kernels": {k: timed(c, max(runs, 20), warmup) for k, c in calls.items()}}
    if "loss" in last:
        row["loss"] = float(last["loss"])
        row["grad_norm"] = float(torch.stack([f.grad.double().norm() for f in fw + bw]).norm())
        row["peak_GiB"] = torch.cuda.max_memory_allocated() / 2 ** 30
    print(json.dumps(dict(variant=name, **row)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unsup_loss_ab.txt"))
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
    lines = [f"Unsupervised loss, forward + backward, {B} pairs of {H} x {W}, {N} predictions per direction, census {W_CENSUS:g} /",
             f"smooth1 {W_SMOOTH1:g} / 'wang' occlusion, MI355X; events around each step, {a.warmup} warm-up steps, median of {a.runs}",
             "(min .. max).  hip: UnsupervisedLoss on csrc/unsup_loss.hip; torch_ops: the same loss composed of PyTorch-ROCm ops in",
             "fp32 (census transform of the un-warped image shared by the 12 predictions, every term backpropagated at once).", "",
             f"{'variant':<12}{'ms median':>12}{'min':>10}{'max':>10}{'loss':>14}{'|grad|':>14}{'peak GiB':>10}"]
    lines += [f"{k:<12}{r['ms_median']:>12.3f}{r['ms_min']:>10.3f}{r['ms_max']:>10.3f}{r['loss']:>14.6f}{r['grad_norm']:>14.6e}"
              f"{r['peak_GiB']:>10.2f}" for k, r in (("hip", hip), ("torch_ops", ref))]
    lines += ["", f"hip takes {hip['ms_median'] / ref['ms_median']:.4f}x the composition's time ({ref['ms_median'] / hip['ms_median']:.1f}x faster)", "",
              f"Per entry point, one call at {B} x {H} x {W}; model bytes per pixel from DESIGN.md; roof {HBM_ROOF / 1e12:.1f} TB/s achievable",
              f"{'entry':<12}{'ms median':>12}{'B/pixel':>9}{'TB/s':>8}{'of roof':>9}"]
    for k, r in rows["kernels"]["kernels"].items():
        rate = MODEL_BYTES[k] * px / (r["ms_median"] * 1e-3)
        lines.append(f"{k:<12}{r['ms_median']:>12.4f}{MODEL_BYTES[k]:>9d}{rate / 1e12:>8.2f}{rate / HBM_ROOF:>9.1%}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    if hip["ms_median"] > ref["ms_median"]:
        sys.exit("the fused path is slower than the composition")


if __name__ == "__main__":
    main()
