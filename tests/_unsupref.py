"""A restatement of the reference's unsupervised (SMURF) loss in plain torch: raft/unsup_loss.py UnsupervisedLoss over
raft/smurf_models/smurf_utils.py, in the PyTorch layout (images [B,3,H,W], flows [B,2,H,W] with channel 0 = x).  The
reference's TensorFlow does not run here, so this file is the oracle of csrc/unsup_loss.hip.  It keeps the reference's op
sequence -- unfold (the 7x7 identity convolution with zero padding) for the census transform, a four-tap gather for the
resampler, index_add_ (unsorted_segment_sum) for the range map, autograd for the gradients -- and computes in the dtype of its
inputs: float64 is the reference, float32 the twin that rounds every operation and gives the limits (LIMITS below).

The warp is written out in pixel units (floor, four taps, zero outside) as tfa.image.resampler defines it, not through
grid_sample: grid_sample normalises and un-normalises the coordinate, and that round trip moves an integer coordinate across
its floor, which changes the one-sided slope there.  test_unsupref.py pins the two to each other off the integers.
"""
import functools

import torch
import torch.nn.functional as F

GRAY = (0.2989, 0.5870, 0.1140)


# ------------------------------------------------------------------------------------------------------------- the loss
def coords(flow, crop_yx=None):
    """flow_to_warp in (x, y): the sampling point of every pixel, in the frame's coordinates."""
    B, _, H, W = flow.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=flow.dtype), torch.arange(W, dtype=flow.dtype), indexing="ij")
    xs, ys = xs.expand(B, H, W), ys.expand(B, H, W)
    if crop_yx is not None:
        c = torch.as_tensor(crop_yx, dtype=flow.dtype)
        xs, ys = xs + c[:, 1].view(B, 1, 1), ys + c[:, 0].view(B, 1, 1)
    return xs + flow[:, 0], ys + flow[:, 1]


def range_map(flow):
    """compute_range_map(flow, downsampling_factor=1): [B,H,W]."""
    B, _, H, W = flow.shape
    cx, cy = coords(flow)
    x0, y0 = torch.floor(cx), torch.floor(cy)
    ox, oy = (cx - x0).reshape(-1), (cy - y0).reshape(-1)
    x0, y0 = x0.long().reshape(-1), y0.long().reshape(-1)
    base = (torch.arange(B).view(B, 1, 1) * H * W).expand(B, H, W).reshape(-1)
    idxs, weights = [], []
    for di in range(2):
        for dj in range(2):
            i, j = y0 + di, x0 + dj
            m = (i >= 0) & (i < H) & (j >= 0) & (j < W)
            wi = (1.0 - di) - (-1) ** di * oy[m]
            wj = (1.0 - dj) - (-1) ** dj * ox[m]
            idxs.append((base + i * W + j)[m])
            weights.append(wi * wj)
    out = torch.zeros(B * H * W, dtype=flow.dtype)
    out.index_add_(0, torch.cat(idxs), torch.cat(weights))
    return out.view(B, H, W)


def occlusion_mask(flow_bw, method="wang"):
    if method == "none":
        return torch.ones_like(flow_bw[:, 0])
    return 1.0 - (1.0 - range_map(flow_bw).clamp(0.0, 1.0))


def resample(frame, sx, sy):
    """tfa.image.resampler: bilinear, taps outside the frame are zero.  frame [B,C,Hf,Wf], sx / sy [B,H,W] -> [B,C,H,W]."""
    B, C, Hf, Wf = frame.shape
    x0, y0 = torch.floor(sx), torch.floor(sy)
    ox, oy = (sx - x0).unsqueeze(1), (sy - y0).unsqueeze(1)
    x0, y0 = x0.detach().long(), y0.detach().long()
    flat = frame.reshape(B, C, Hf * Wf)

    def tap(ix, iy):
        ok = ((ix >= 0) & (ix < Wf) & (iy >= 0) & (iy < Hf)).unsqueeze(1)
        idx = (iy.clamp(0, Hf - 1) * Wf + ix.clamp(0, Wf - 1)).view(B, 1, -1).expand(B, C, -1)
        return torch.gather(flat, 2, idx).view(B, C, *ix.shape[1:]) * ok.to(frame.dtype)

    return (((1.0 - ox) * (1.0 - oy) * tap(x0, y0) + ox * (1.0 - oy) * tap(x0 + 1, y0)) + (1.0 - ox) * oy * tap(x0, y0 + 1)) \
        + ox * oy * tap(x0 + 1, y0 + 1)


def crop(frame, crop_yx, H, W):
    if crop_yx is None:
        return frame
    return torch.stack([frame[b, :, cy:cy + H, cx:cx + W] for b, (cy, cx) in enumerate(crop_yx)])


def census_transform(img):
    g = 255.0 * (GRAY[0] * img[:, 0:1] + GRAY[1] * img[:, 1:2] + GRAY[2] * img[:, 2:3])
    B, _, H, W = g.shape
    neighbours = F.unfold(g, 7, padding=3).view(B, 49, H, W)
    diff = neighbours - g
    return diff / torch.sqrt(0.81 + diff ** 2)


def census_parts(frame1, frame2, flow, mask, crop_yx=None):
    """-> (loss, M [B,H,W] with the border zeroed, warped image)."""
    B, _, H, W = flow.shape
    Hf, Wf = frame2.shape[-2:]
    sx, sy = coords(flow, crop_yx)
    warped = resample(frame2, sx, sy)
    valid = ((sx >= 0) & (sx <= Wf - 1) & (sy >= 0) & (sy <= Hf - 1)).to(flow.dtype)
    M = ((torch.ones_like(valid) if mask is None else mask) * valid).detach()
    border = torch.zeros_like(M)
    border[:, 3:-3, 3:-3] = 1.0
    M = M * border
    u = census_transform(crop(frame1, crop_yx, H, W)) - census_transform(warped)
    ham = (u ** 2 / (0.1 + u ** 2)).sum(1)
    diff = (ham.abs() + 0.01) ** 0.4 * M
    return diff.sum() / (M + 1e-6).sum(), M, warped


def census_loss(frame1, frame2, flow, mask, crop_yx=None):
    return census_parts(frame1, frame2, flow, mask, crop_yx)[0]


def smoothness_loss(image, flow, order=1, edge_constant=150.0, weighting="exponential"):
    def grads(t, stride=1):
        return t[:, :, stride:] - t[:, :, :-stride], t[:, :, :, stride:] - t[:, :, :, :-stride]

    def weight(d):
        d = edge_constant * d
        return torch.exp(-(d ** 2 if weighting == "gaussian" else d.abs()).mean(1, keepdim=True))

    def robust_l1(x):
        return (x ** 2 + 0.001 ** 2) ** 0.5

    ih, iw = grads(image, order)
    fh, fw = grads(flow)
    if order == 2:
        fh, fw = grads(fh)[0], grads(fw)[1]
    return ((weight(ih) * robust_l1(fh)).mean() + (weight(iw) * robust_l1(fw)).mean()) / 2.0


def unsup_loss(frames, flows_fw, flows_bw, crop_yx=None, census=1.0, smooth1=2.5, smooth2=0.0, occlusion="wang", gamma=0.8):
    """UnsupervisedLoss.call, mode 'unsup_per_update' -> (loss, dict of the weighted terms)."""
    w = {k: v for k, v in (("census", census), ("smooth1", smooth1), ("smooth2", smooth2)) if v > 0}
    H, W = flows_fw[0].shape[-2:]
    imgs = [crop(f, crop_yx, H, W) for f in frames]
    total = {}
    for ffw, fbw in zip(flows_fw, flows_bw):
        one = {k: 0.0 for k in w}
        for i, j, f, g in ((0, 1, ffw, fbw), (1, 0, fbw, ffw)):
            if "census" in w:
                one["census"] = one["census"] + w["census"] * census_loss(frames[i], frames[j], f, occlusion_mask(g.detach(), occlusion),
                                                                          crop_yx) / 2.0
            for k, order in (("smooth1", 1), ("smooth2", 2)):
                if k in w:
                    one[k] = one[k] + w[k] * smoothness_loss(imgs[i], f, order) / 2.0
        for k, v in one.items():                                       # add_loss_dicts
            total[k] = v + total[k] * gamma if k in total else v
    return sum(total.values()), total


# ------------------------------------------------------------------------------------------------------------ the cases
SHAPES = (                       # (B, H, W, frame or None, crop_yx or None)
    (1, 7, 7, None, None),       # one pixel inside the border
    (1, 7, 8, None, None),
    (1, 9, 70, None, None),      # one interior row wider than a wave
    (2, 37, 61, None, None),     # odd, off every tile
    (1, 70, 130, None, None),    # more than one tile both ways; halos cross tile edges
    (3, 24, 40, (48, 80), ((0, 0), (24, 40), (5, 7))),     # windows of full frames, one flush bottom-right
)
FAMILIES = ("zero", "integer", "subpixel", "large", "fold", "allout")
INTEGER_FAMILIES = ("zero", "integer", "allout")


def smooth_field(g, B, C, H, W, cells=4):
    low = torch.rand(B, C, max(2, H // cells + 1), max(2, W // cells + 1), generator=g, dtype=torch.float64)
    return F.interpolate(low, size=(H, W), mode="bilinear", align_corners=True)


def make_image(g, B, H, W):
    """A smooth random field plus a few hard edges, in [0, 1].  The field's slope times the edge constant 150 stays near 2, as
    in photographs: steeper, and the 'gaussian' edge weights underflow in fp32 everywhere, which leaves nothing to compare."""
    img = 0.3 + 0.1 * smooth_field(g, B, 3, H, W, cells=8)
    for _ in range(3):
        y0, x0 = int(torch.randint(0, H - 2, (1,), generator=g)), int(torch.randint(0, W - 2, (1,), generator=g))
        img[:, :, y0:y0 + max(2, H // 3), x0:x0 + max(2, W // 3)] += 0.12
    return img.clamp(0.0, 1.0).float()


def make_flow(g, family, B, H, W, Hf, Wf):
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    centred = torch.stack([xs - (W - 1) / 2, ys - (H - 1) / 2]).expand(B, 2, H, W)
    noise = smooth_field(g, B, 2, H, W) - 0.5
    if family == "zero":
        f = torch.zeros(B, 2, H, W, dtype=torch.float64)
    elif family == "integer":
        f = torch.tensor([2.0, -1.0], dtype=torch.float64).view(1, 2, 1, 1).expand(B, 2, H, W)
    elif family == "subpixel":           # a gentle expansion plus noise: |f| <= 3, the range map stays clear of 1
        f = centred * 0.04 + 0.6 * (smooth_field(g, B, 2, H, W, cells=16) - 0.5)
    elif family == "large":              # a strong expansion: most warps leave a frame of the image's own size
        f = centred * 0.8 + 2.0 * noise
    elif family == "fold":               # a contraction by two: four sources per target around the centre
        f = centred * -0.5 + 0.6 * noise
    else:                                # "allout": every warp lands beyond the frame
        f = torch.full((B, 2, H, W), float(Hf + Wf + 8), dtype=torch.float64)
    if family not in INTEGER_FAMILIES:
        # per-pixel jitter: an interpolated field is piecewise linear, its second differences are nothing but the rounding of the
        # fp32 inputs, and the second-order term's gradient would be all cancellation
        f = f + 0.02 * (torch.rand(B, 2, H, W, generator=g, dtype=torch.float64) - 0.5)
    return f.float().contiguous()


def input_conditions(case):
    """Share of pixels that break a condition under which fp32 and fp64 take the same decisions: a warp coordinate of a pixel
    inside the census border within 1e-3 px of a validity bound, or within 1e-5 px of an integer (a floor), or a range-map value
    within 1e-4 of the clip at 1 -- except in the families built to sit on these exactly (integer-valued flows)."""
    if case["family"] in INTEGER_FAMILIES:
        return 0.0
    bad = 0
    Hf, Wf = case["frames"][0].shape[-2:]
    for f in (case["flow"], case["flow_bw"]):
        sx, sy = coords(f.double(), case["crop_yx"])
        inner = torch.zeros_like(sx, dtype=torch.bool)
        inner[:, 3:-3, 3:-3] = True
        for s, hi in ((sx, Wf - 1), (sy, Hf - 1)):
            bad += int((inner & (((s - 0.0).abs() < 1e-3) | ((s - hi).abs() < 1e-3))).sum())
            bad += int(((s - torch.round(s)).abs() < 1e-5).sum())
        bad += int(((range_map(f.double()) - 1.0).abs() < 1e-4).sum())
    return bad / case["flow"].numel()


@functools.lru_cache(maxsize=None)
def cases():
    """Every (shape, family) case of the GPU tests: fp32 inputs, regenerated from the seed until input_conditions() is 0."""
    out = []
    for si, (B, H, W, frame, crop_yx) in enumerate(SHAPES):
        Hf, Wf = frame or (H, W)
        for fi, family in enumerate(FAMILIES):
            for attempt in range(200):
                g = torch.Generator().manual_seed(1000 * si + 100 * fi + attempt)
                case = dict(name=f"{B}x{H}x{W}{'in%dx%d' % (Hf, Wf) if frame else ''}-{family}", family=family, B=B, H=H, W=W, crop_yx=crop_yx,
                            frames=(make_image(g, B, Hf, Wf), make_image(g, B, Hf, Wf)),
                            flow=make_flow(g, family, B, H, W, Hf, Wf), flow_bw=make_flow(g, family, B, H, W, Hf, Wf))
                if input_conditions(case) == 0.0:
                    break
            out.append(case)
    return out


@functools.lru_cache(maxsize=None)
def sequence_case():
    """UnsupervisedLoss's case: 3 predictions per direction at 2x37x61, windows of 50x80 frames (same input conditions)."""
    B, H, W, Hf, Wf = 2, 37, 61, 50, 80
    fam = ("subpixel", "fold", "large")
    for attempt in range(200):
        g = torch.Generator().manual_seed(7700 + attempt)
        sc = dict(frames=(make_image(g, B, Hf, Wf), make_image(g, B, Hf, Wf)), crop_yx=((13, 19), (4, 0)),
                  fw=[make_flow(g, k, B, H, W, Hf, Wf) for k in fam], bw=[make_flow(g, k, B, H, W, Hf, Wf) for k in fam],
                  weights=dict(census=1.0, smooth1=2.5, smooth2=0.7))
        if all(input_conditions(dict(family=k, frames=sc["frames"], crop_yx=sc["crop_yx"], flow=a, flow_bw=b)) == 0.0
               for k, a, b in zip(fam, sc["fw"], sc["bw"])):
            break
    return sc


def evaluate(case, dtype):
    """Every quantity the GPU tests compare, of one case, computed in `dtype`."""
    frames = [t.to(dtype) for t in case["frames"]]
    flow = case["flow"].to(dtype).requires_grad_(True)
    mask = occlusion_mask(case["flow_bw"].to(dtype))
    out = {"range_map": range_map(case["flow_bw"].to(dtype)), "mask": mask}
    loss = census_loss(frames[0], frames[1], flow, mask, case["crop_yx"])
    out["census"], out["census_dflow"] = loss.detach(), torch.autograd.grad(loss, flow)[0]
    img = crop(frames[0], case["crop_yx"], case["H"], case["W"])
    for order in (1, 2):
        for weighting in ("exponential", "gaussian"):
            v = smoothness_loss(img, flow, order, 150.0, weighting)
            out[f"smooth{order}{weighting[0]}"], out[f"smooth{order}{weighting[0]}_dflow"] = v.detach(), torch.autograd.grad(v, flow)[0]
    return out


def evaluate_sequence(sc, dtype):
    fw = [t.to(dtype).requires_grad_(True) for t in sc["fw"]]
    bw = [t.to(dtype).requires_grad_(True) for t in sc["bw"]]
    loss, terms = unsup_loss([t.to(dtype) for t in sc["frames"]], fw, bw, sc["crop_yx"], **sc["weights"])
    grads = torch.autograd.grad(loss, fw + bw)
    return dict(loss=loss.detach(), terms={k: v.detach() for k, v in terms.items()}, grads=grads)


@functools.lru_cache(maxsize=None)
def reference(i):
    return evaluate(cases()[i], torch.float64)


@functools.lru_cache(maxsize=None)
def reference_sequence():
    return evaluate_sequence(sequence_case(), torch.float64)


def field_error(x, ref):
    """Worst absolute error in units of 2^-24 * max|ref| (0 where the reference is all zero and x is too)."""
    scale = float(ref.abs().max()) * 2.0 ** -24
    err = float((x.double() - ref.double()).abs().max())
    return err / scale if scale > 0 else (0.0 if err == 0 else float("inf"))


def scalar_error(x, ref):
    ref = float(ref)
    return abs(float(x) - ref) / abs(ref) if ref != 0 else (0.0 if float(x) == 0 else float("inf"))


QUANTITIES = {                   # quantity -> (keys of evaluate(), error measure)
    "range_map": (("range_map",), field_error),
    "census": (("census",), scalar_error),
    "census_dflow": (("census_dflow",), field_error),
    "smoothness": (("smooth1e", "smooth1g", "smooth2e", "smooth2g"), scalar_error),
    "smoothness_dflow": (("smooth1e_dflow", "smooth1g_dflow", "smooth2e_dflow", "smooth2g_dflow"), field_error),
}
FACTOR = 4.0                     # a different summation order and fused multiply-adds in the kernels (test_corr_bwd_kernels.py)


@functools.lru_cache(maxsize=None)
def twin_errors():
    """The fp32 twin's worst error against fp64 over the GPU cases, per quantity (fields: units of 2^-24 * max|ref|)."""
    worst = {q: 0.0 for q in QUANTITIES}
    for i, case in enumerate(cases()):
        ref, twin = reference(i), evaluate(case, torch.float32)
        for q, (keys, measure) in QUANTITIES.items():
            worst[q] = max([worst[q]] + [measure(twin[k], ref[k]) for k in keys])
    ref, twin = reference_sequence(), evaluate_sequence(sequence_case(), torch.float32)
    worst["sequence"] = max([scalar_error(twin["loss"], ref["loss"])] + [scalar_error(twin["terms"][k], ref["terms"][k]) for k in ref["terms"]])
    worst["sequence_dflow"] = max(field_error(a, b) for a, b in zip(twin["grads"], ref["grads"]))
    return worst


def limits():
    """LIMITS: FACTOR times the twin's worst error, per quantity."""
    return {q: FACTOR * e for q, e in twin_errors().items()}
