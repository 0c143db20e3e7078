#!/usr/bin/env python3
"""A/B of the augmentation at the recipe's size: 2 samples, source 436 x 1024, frames 432 x 1024, crops 368 x 768, uint8 and
fp32 sources, on parameters the sampler drew (both samples resized, both with eraser rectangles, one with asymmetric colour):

    hip         flow_supervisor_amd.augment.apply (csrc/augment.hip): four launches per batch
    torch_ops   the same function composed of PyTorch-ROCm tensor ops in fp32 on the same device and the same parameters
                (the op sequence of tests/_augref.py, copied here: index_select gathers for the resizes, elementwise ops for
                the colour, a mean and a slice assignment for the eraser)

    python scripts/augment_ab.py [--out profiles/augment_ab.txt] [--runs 7] [--calls 50]

A timed window is `--calls` calls between two events on the current stream; the two variants alternate window by window in
one process per dtype, after warm-up windows of both; the figure is the median window over its calls.  The parent process never
touches the GPU: every dtype is a child of its own under `timeout -k 10`, and the first child that fails ends the run.  No
ratio is promised: the file says what was measured, the composition is the yardstick.
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, SRC, CROP = 2, (436, 1024), (368, 768)
HBM_ROOF = 6.3e12                       # achievable bytes / s on an MI355X (8.0e12 is the specification)


def draw_params():
    """Two samples from the sampler under a fixed seed: the first two draws that resize and erase, one of them asymmetric."""
    import torch
    from flow_supervisor_amd.augment import UnsupAugmentor
    aug, g = UnsupAugmentor(CROP, do_flip=True), torch.Generator().manual_seed(2024)
    sym, asym = [], []
    while not (sym and asym):
        p = aug.sample(SRC, g)
        if p.resize and p.rects and all(dx * dy > 0 for _, _, dx, dy in p.rects):
            (asym if p.asymmetric else sym).append(p)
    return [sym[0], asym[0]]


def model_bytes(params, elt):
    """Compulsory traffic of a batch: the part of the source the frame's window maps to (a resized sample reads the window
    divided by its scales, plus the taps' border), every output once, and the crop window of the frames a second time (the
    contrast mean has to be complete before the first crop pixel can be written)."""
    total = 0
    for p in params:
        (Hs, Ws), (Hf, Wf), (h, w) = p.src_hw, p.full_hw, p.crop_hw
        src = min(Hs, math.ceil(Hf / p.scale_y) + 2) * min(Ws, math.ceil(Wf / p.scale_x) + 2)
        total += src * (6 * elt + 8 + 4) + Hf * Wf * 36 + h * w * (24 + 36)
    return total


# ---------------------------------------------------------------------------------------------- the composition of torch ops
def torch_apply(img1, img2, flow, valid, params):
    import torch
    dev = flow.device

    def taps(dst, n_in, n_out):
        src = (dst.float() + 0.5) * (torch.tensor(float(n_in)) / torch.tensor(float(n_out))).item() - 0.5
        fl = torch.floor(src)
        return fl.long().clamp(min=0), torch.ceil(src).long().clamp(max=n_in - 1), src - fl

    def nearest(dst, n_in, n_out):
        c = (dst.float() + 0.5) * (torch.tensor(float(n_in)) / torch.tensor(float(n_out))).item()
        return torch.floor(c).long().clamp(max=n_in - 1)

    def hsv(rgb):
        r, g, b = rgb[0], rgb[1], rgb[2]
        v = torch.maximum(r, torch.maximum(g, b))
        c = v - torch.minimum(r, torch.minimum(g, b))
        s = torch.where(v > 0, c / torch.where(v > 0, v, torch.ones_like(v)), torch.zeros_like(v))
        cc = torch.where(c > 0, c, torch.ones_like(c))
        hr = ((g - b) / cc) / 6.0
        hr = torch.where(hr < 0, hr + 1.0, hr)
        h = torch.where(r == v, hr, torch.where(g == v, (2.0 + (b - r) / cc) / 6.0, (4.0 + (r - g) / cc) / 6.0))
        return torch.where(c > 0, h, torch.zeros_like(h)), s, v

    def rgb(h, s, v):
        h6 = 6.0 * h
        d = torch.stack([(h6 - 3.0).abs() - 1.0, 2.0 - (h6 - 2.0).abs(), 2.0 - (h6 - 4.0).abs()]).clamp(0.0, 1.0)
        return ((d - 1.0) * s + 1.0) * v

    out = {k: [] for k in ("frame1", "frame2", "frame_flow", "frame_valid", "crop1", "crop2", "crop_flow", "crop_valid")}
    unit = 1.0 if img1.dtype == torch.uint8 else 255.0
    for b, p in enumerate(params):
        (Hs, Ws), (Hf, Wf), (h, w) = p.src_hw, p.full_hw, p.crop_hw
        rows, cols = torch.arange(Hf, device=dev), torch.arange(Wf, device=dev)
        rows = (Hf - 1 - rows if p.vflip else rows) + p.win_y
        cols = (Wf - 1 - cols if p.hflip else cols) + p.win_x
        imgs, f, v = [img1[b].float(), img2[b].float()], flow[b], valid[b]
        if p.resize:
            y0, y1, wy = taps(rows, Hs, p.t_h)
            x0, x1, wx = taps(cols, Ws, p.t_w)
            wy, wx = wy[:, None, None], wx[None, :, None]
            frames = []
            for t in imgs:
                top, bot = t[y0], t[y1]
                top = top[:, x0] + (top[:, x1] - top[:, x0]) * wx
                bot = bot[:, x0] + (bot[:, x1] - bot[:, x0]) * wx
                frames.append(top + (bot - top) * wy)
            ny, nx = nearest(rows, Hs, p.t_h), nearest(cols, Ws, p.t_w)
            f = f[ny][:, nx] * torch.tensor([p.scale_x, p.scale_y], device=dev)
            v = v[ny][:, nx]
        else:
            frames = [t[rows][:, cols] for t in imgs]
            f, v = f[rows][:, cols], v[rows][:, cols]
        f = f * torch.tensor([-1.0 if p.hflip else 1.0, -1.0 if p.vflip else 1.0], device=dev)
        frames = [(t * unit if unit != 1.0 else t).permute(2, 0, 1).contiguous() for t in frames]
        f, v = f.permute(2, 0, 1).contiguous(), v[None].contiguous()
        win = (slice(None), slice(p.crop_y, p.crop_y + h), slice(p.crop_x, p.crop_x + w))
        xs = [t[win] / 255.0 * q[0] for t, q in zip(frames, p.colour)]
        means = [x.mean((1, 2), keepdim=True) for x in xs] if p.asymmetric else [torch.cat(xs, 1).mean((1, 2), keepdim=True)] * 2
        crops = []
        for x, m, q in zip(xs, means, p.colour):
            x = (x - m) * q[1] + m
            hh, s, vv = hsv(x)
            x = rgb(hh, (s * q[2]).clamp(0.0, 1.0), vv)
            hh, s, vv = hsv(x)
            hh = hh + q[3]
            crops.append(rgb(hh - torch.floor(hh), s, vv).clamp(0.0, 1.0) * 255.0)
        mean = crops[1].mean((1, 2), keepdim=True)
        for x0, y0, dx, dy in p.rects:
            if dx > 0 and dy > 0:
                crops[1][:, y0:y0 + dy, x0:x0 + dx] = mean
        for k, t in zip(out, (*frames, f, v, *crops, f[win], v[win])):
            out[k].append(t)
    return {k: torch.stack(v) for k, v in out.items()}


def window(step, calls):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def child(kind, runs, warmup, calls):
    sys.path.insert(0, ROOT)
    import torch
    from flow_supervisor_amd import augment as A
    params = draw_params()
    g = torch.Generator().manual_seed(1)
    if kind == "u8":
        imgs = [torch.randint(0, 256, (B, *SRC, 3), generator=g, dtype=torch.uint8).cuda() for _ in range(2)]
    else:
        imgs = [torch.rand(B, *SRC, 3, generator=g).cuda() for _ in range(2)]
    flow = (20.0 * (torch.rand(B, *SRC, 2, generator=g) - 0.5)).cuda()
    valid = (torch.rand(B, *SRC, generator=g) > 0.3).float().cuda()
    steps = {"hip": lambda: A.apply(*imgs, flow, valid, params), "torch_ops": lambda: torch_apply(*imgs, flow, valid, params)}
    got, want = steps["hip"](), steps["torch_ops"]()
    pairs = (("frame1", got["original_img"][0]), ("frame2", got["original_img"][1]), ("frame_flow", got["original_flows"]),
             ("frame_valid", got["original_valids"]), ("crop1", got["augmented_img"][0]), ("crop2", got["augmented_img"][1]),
             ("crop_flow", got["flows"]), ("crop_valid", got["valids"]))
    diff = {k: float((t - want[k]).abs().max()) for k, t in pairs}
    for _ in range(warmup):
        for step in steps.values():
            window(step, calls)
    ms = {k: [] for k in steps}
    for _ in range(runs):
        for k, step in steps.items():
            ms[k].append(window(step, calls))
    rows = {k: dict(ms_median=statistics.median(v), ms_min=min(v), ms_max=max(v)) for k, v in ms.items()}
    print(json.dumps(dict(kind=kind, rows=rows, diff=diff, bytes=model_bytes(params, 1 if kind == "u8" else 4),
                          params=[repr(p) for p in params])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_ab.txt"))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--kind")
    a = ap.parse_args()
    if a.kind:
        return child(a.kind, a.runs, a.warmup, a.calls)
    res = {}
    for kind in ("u8", "f32"):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--kind", kind, "--runs", str(a.runs),
               "--warmup", str(a.warmup), "--calls", str(a.calls)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"{kind}: exit status {r.returncode}; stopping, nothing more is started")
        res[kind] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    lines = [f"UnsupAugmentor applied to {B} samples, source {SRC[0]} x {SRC[1]}, frames 432 x 1024, crops {CROP[0]} x {CROP[1]}, MI355X.",
             "hip: flow_supervisor_amd.augment.apply on csrc/augment.hip (four launches); torch_ops: the same function composed of",
             f"PyTorch-ROCm tensor ops in fp32 on the same parameters.  A window is {a.calls} calls between two events (allocations of the",
             f"outputs and the launches inside); the variants alternate, {a.warmup} warm-up windows each, median of {a.runs} windows (min .. max), per call.",
             f"Model bytes: the part of the source under the frame's window, every output once, the frames' crop window twice; roof {HBM_ROOF / 1e12:.1f} TB/s",
             "achievable.", "",
             f"{'source':<8}{'variant':<12}{'ms median':>11}{'min':>9}{'max':>9}{'max/min':>9}{'model MB':>10}{'TB/s':>7}{'of roof':>9}"]
    for kind, r in res.items():
        for k, row in r["rows"].items():
            rate = r["bytes"] / (row["ms_median"] * 1e-3)
            lines.append(f"{kind:<8}{k:<12}{row['ms_median']:>11.4f}{row['ms_min']:>9.4f}{row['ms_max']:>9.4f}{row['ms_max'] / row['ms_min']:>9.3f}"
                         f"{r['bytes'] / 1e6:>10.1f}{rate / 1e12:>7.2f}{rate / HBM_ROOF:>9.1%}")
    lines.append("")
    for kind, r in res.items():
        hip, ref = r["rows"]["hip"]["ms_median"], r["rows"]["torch_ops"]["ms_median"]
        lines.append(f"{kind}: hip takes {hip / ref:.4f}x the composition's time ({ref / hip:.1f}x); largest difference of any output between "
                     f"the two: {max(r['diff'].values()):.3g} (images in [0, 255])")
    lines += ["", "parameters:"] + ["  " + p for p in res["u8"]["params"]]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
