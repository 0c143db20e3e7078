#!/usr/bin/env python3
"""A/B of the supervised augmentors at the sizes of the reference's training stages, uint8 and fp32 sources, on parameters the
samplers drew (every sample resized, every sample with a non-empty eraser rectangle):

    chairs   FlowAugmentor        8 x 384 x 512   -> 368 x 496
    sintel   FlowAugmentor        4 x 436 x 1024  -> 368 x 768
    kitti    SparseFlowAugmentor  4 x 375 x 1242  -> 288 x 960

    hip         flow_supervisor_amd.augment.apply_supervised (fsraft_augment_sup in csrc/augment.hip): five launches per batch
    torch_ops   the same function composed of PyTorch-ROCm tensor ops in fp32 on the same device and the same parameters
                (the op sequence of tests/_supaugref.py, copied here: elementwise ops and means for the colour step, a slice
                assignment for the eraser, index_select gathers for the resizes)

    python scripts/supaug_ab.py [--out profiles/supaug_ab.txt] [--runs 7] [--calls 50]

A timed window is `--calls` calls between two events on the current stream; the two variants alternate window by window in
one process per size and dtype, after warm-up windows of both; the figure is the median window over its calls.  The parent
process never touches the GPU: every child runs under `timeout -k 10`, and the first child that fails ends the run.  No ratio
is promised: the file says what was measured, the composition is the yardstick.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_ROOF = 6.3e12                       # achievable bytes / s on an MI355X (8.0e12 is the specification)
SIZES = {                               # name -> (class, B, source, crop)
    "chairs": ("FlowAugmentor", 8, (384, 512), (368, 496)),
    "sintel": ("FlowAugmentor", 4, (436, 1024), (368, 768)),
    "kitti": ("SparseFlowAugmentor", 4, (375, 1242), (288, 960)),
}


def draw_params(size):
    """B samples from the size's sampler under a fixed seed: the first draws that resize and erase.  (A draw whose resized image
    is not larger than the crop raises, as TensorFlow would die there, and is passed over.)"""
    import torch
    from flow_supervisor_amd import augment as A
    cls, B, src, crop = SIZES[size]
    aug, g, out = getattr(A, cls)(crop), torch.Generator().manual_seed(2024), []
    while len(out) < B:
        try:
            p = aug.sample(src, g)
        except ValueError:
            continue
        if p.resize and any(dx * dy > 0 for _, _, dx, dy in p.rects):
            out.append(p)
    return out


def model_bytes(size, elt):
    """Compulsory traffic of a batch whose samples are all erased: both images once for the contrast means, image 2 once for
    the eraser's colour, both images, the flow and (sparse) the valid map once for the output, every output once."""
    cls, B, (Hs, Ws), (h, w) = SIZES[size]
    src = Hs * Ws
    return B * (src * 3 * elt * (2 + 1 + 2) + src * (8 + (4 if cls == "SparseFlowAugmentor" else 0)) + h * w * 9 * 4)


# ---------------------------------------------------------------------------------------------- the composition of torch ops
def torch_apply(img1, img2, flow, valid, params, dense):
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

    def bilinear(t, y0, y1, wy, x0, x1, wx):
        top, bot = t[y0], t[y1]
        top = top[:, x0] + (top[:, x1] - top[:, x0]) * wx
        bot = bot[:, x0] + (bot[:, x1] - bot[:, x0]) * wx
        return top + (bot - top) * wy

    out = {k: [] for k in ("crop1", "crop2", "crop_flow", "crop_valid")}
    for b, p in enumerate(params):
        (Hs, Ws), (h, w) = p.src_hw, p.crop_hw
        xs = [(t[b].float() / 255.0 if t.dtype == torch.uint8 else t[b]).permute(2, 0, 1) * q[0] for t, q in zip((img1, img2), p.colour)]
        means = [x.mean((1, 2), keepdim=True) for x in xs] if p.asymmetric else [torch.cat(xs, 1).mean((1, 2), keepdim=True)] * 2
        E = []
        for x, m, q in zip(xs, means, p.colour):
            x = (x - m) * q[1] + m
            hh, s, vv = hsv(x)
            x = rgb(hh, (s * q[2]).clamp(0.0, 1.0), vv)
            hh, s, vv = hsv(x)
            hh = hh + q[3]
            E.append(rgb(hh - torch.floor(hh), s, vv).clamp(0.0, 1.0))
        mean = E[1].mean((1, 2), keepdim=True)
        for x0, y0, dx, dy in p.rects:
            if dx > 0 and dy > 0:
                E[1][:, y0:y0 + dy, x0:x0 + dx] = mean
        rows, cols = torch.arange(h, device=dev) + p.crop_y, torch.arange(w, device=dev) + p.crop_x
        rows = p.t_h - 1 - rows if p.vflip else rows
        cols = p.t_w - 1 - cols if p.hflip else cols
        f, v = flow[b], (torch.ones(Hs, Ws, device=dev) if dense or valid is None else valid[b])
        if p.resize:
            y0, y1, wy = taps(rows, Hs, p.t_h)
            x0, x1, wx = taps(cols, Ws, p.t_w)
            wy, wx = wy[:, None, None], wx[None, :, None]
            crops = [bilinear(e.permute(1, 2, 0), y0, y1, wy, x0, x1, wx) * 255.0 for e in E]
            ny, nx = nearest(rows, Hs, p.t_h), nearest(cols, Ws, p.t_w)
            f = bilinear(f, y0, y1, wy, x0, x1, wx) if dense else f[ny][:, nx]
            f = f * torch.tensor([p.scale_x, p.scale_y], device=dev)
            v = v[ny][:, nx]
        else:
            crops = [e.permute(1, 2, 0)[rows][:, cols] * 255.0 for e in E]
            f, v = f[rows][:, cols], v[rows][:, cols]
        f = f * torch.tensor([-1.0 if p.hflip else 1.0, -1.0 if p.vflip else 1.0], device=dev)
        for k, t in zip(out, (crops[0].permute(2, 0, 1), crops[1].permute(2, 0, 1), f.permute(2, 0, 1), v[None])):
            out[k].append(t.contiguous())
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


def child(size, kind, runs, warmup, calls):
    sys.path.insert(0, ROOT)
    import torch
    from flow_supervisor_amd import augment as A
    cls, B, src, _ = SIZES[size]
    dense = cls == "FlowAugmentor"
    params = draw_params(size)
    g = torch.Generator().manual_seed(1)
    if kind == "u8":
        imgs = [torch.randint(0, 256, (B, *src, 3), generator=g, dtype=torch.uint8).cuda() for _ in range(2)]
    else:
        imgs = [torch.rand(B, *src, 3, generator=g).cuda() for _ in range(2)]
    flow = (20.0 * (torch.rand(B, *src, 2, generator=g) - 0.5)).cuda()
    valid = (torch.rand(B, *src, generator=g) > 0.3).float().cuda()
    steps = {"hip": lambda: A.apply_supervised(*imgs, flow, valid, params, dense), "torch_ops": lambda: torch_apply(*imgs, flow, valid, params, dense)}
    got, want = steps["hip"](), steps["torch_ops"]()
    pairs = (("crop1", got["image1"]), ("crop2", got["image2"]), ("crop_flow", got["flow"]), ("crop_valid", got["valid"]))
    diff = {k: float((t - want[k]).abs().max()) for k, t in pairs}
    for _ in range(warmup):
        for step in steps.values():
            window(step, calls)
    ms = {k: [] for k in steps}
    for _ in range(runs):
        for k, step in steps.items():
            ms[k].append(window(step, calls))
    rows = {k: dict(ms_median=statistics.median(v), ms_min=min(v), ms_max=max(v)) for k, v in ms.items()}
    print(json.dumps(dict(size=size, kind=kind, rows=rows, diff=diff, bytes=model_bytes(size, 1 if kind == "u8" else 4),
                          params=[repr(p) for p in params])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "supaug_ab.txt"))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--size", choices=sorted(SIZES))
    ap.add_argument("--kind")
    a = ap.parse_args()
    if a.kind:
        return child(a.size, a.kind, a.runs, a.warmup, a.calls)
    res = {}
    for size in SIZES:
        for kind in ("u8", "f32"):
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--size", size, "--kind", kind,
                   "--runs", str(a.runs), "--warmup", str(a.warmup), "--calls", str(a.calls)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                sys.exit(f"{size} {kind}: exit status {r.returncode}; stopping, nothing more is started")
            res[size, kind] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    lines = ["FlowAugmentor / SparseFlowAugmentor applied to a batch, MI355X.  Sizes (samples x source -> crop): "
             + "; ".join(f"{k} {v[1]} x {v[2][0]} x {v[2][1]} -> {v[3][0]} x {v[3][1]} ({v[0]})" for k, v in SIZES.items()) + ".",
             "hip: flow_supervisor_amd.augment.apply_supervised on fsraft_augment_sup (five launches); torch_ops: the same function",
             f"composed of PyTorch-ROCm tensor ops in fp32 on the same parameters.  A window is {a.calls} calls between two events (allocations",
             f"of the outputs and the launches inside); the variants alternate, {a.warmup} warm-up windows each, median of {a.runs} windows (min .. max),",
             "per call.  Model bytes: both images once for the contrast means, image 2 once for the eraser's colour, both images, flow and",
             f"(kitti) valid once for the output kernel, every output once; roof {HBM_ROOF / 1e12:.1f} TB/s achievable.  Every sample is resized and erased.",
             "A two-pass form (the photometric source written out, then resampled) was not built: there is no figure for it.", "",
             f"{'size':<8}{'source':<8}{'variant':<12}{'ms median':>11}{'min':>9}{'max':>9}{'max/min':>9}{'model MB':>10}{'TB/s':>7}{'of roof':>9}"]
    for (size, kind), r in res.items():
        for k, row in r["rows"].items():
            rate = r["bytes"] / (row["ms_median"] * 1e-3)
            lines.append(f"{size:<8}{kind:<8}{k:<12}{row['ms_median']:>11.4f}{row['ms_min']:>9.4f}{row['ms_max']:>9.4f}"
                         f"{row['ms_max'] / row['ms_min']:>9.3f}{r['bytes'] / 1e6:>10.1f}{rate / 1e12:>7.2f}{rate / HBM_ROOF:>9.1%}")
    lines.append("")
    for (size, kind), r in res.items():
        hip, ref = r["rows"]["hip"]["ms_median"], r["rows"]["torch_ops"]["ms_median"]
        lines.append(f"{size} {kind}: hip takes {hip / ref:.4f}x the composition's time ({ref / hip:.1f}x); largest difference of any output "
                     f"between the two: {max(r['diff'].values()):.3g} (images in [0, 255])")
    for size in SIZES:
        lines += ["", f"parameters, {size}:"] + ["  " + p for p in res[size, "u8"]["params"]]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
