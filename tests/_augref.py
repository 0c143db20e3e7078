"""A restatement in plain torch of what csrc/augment.hip computes: the reference's UnsupAugmentor
(pytorch/raft_utils/augmentor.py:496-657, ColorJitter :15-37, the "* 255" of pytorch/train.py:251-258) applied with given
parameters.  The reference's augmentor is TensorFlow on the host and does not run here, so this file is the oracle: TF2's
tf.image.resize (BILINEAR and NEAREST_NEIGHBOR, half-pixel centres, no antialias) and its fused saturation / hue kernels,
written out.  It computes in the dtype it is given -- float64 is the reference, float32 the twin that rounds every operation
and gives the limits.  The index arithmetic TF does in float32 (the nearest-neighbour index, the scales, the rounding of the
resized size) is float32 in both.

Parameters are dicts with the field names of flow_supervisor_amd.augment.AugParams; sources are interleaved ([Hs,Ws,3] images,
uint8 or float in [0, 1]; [Hs,Ws,2] flow; [Hs,Ws] valid), results planar ([3,Hf,Wf] ...), images in [0, 255].
"""
import functools

import numpy as np
import torch

FACTOR = 4.0                     # a different summation order in the kernels' means (as in _unsupref.py)
IDENTITY = (1.0, 1.0, 1.0, 0.0)


# ------------------------------------------------------------------------------------------------------------- resizing
def resized_size(n, scale):
    """augmentor.py:583-587 in float32, tf.round = half to even: (t, float32(t) / float32(n))."""
    t = int(np.rint(np.float32(n) * np.float32(scale)))
    return t, float(np.float32(t) / np.float32(n))


def bilinear_taps(dst, n_in, n_out, dtype):
    """(lo, hi, weight) of the destination indices `dst` (int64): src = (dst + 0.5) * (in / out) - 0.5 in `dtype`."""
    scale = torch.tensor(n_in, dtype=dtype) / torch.tensor(n_out, dtype=dtype)
    src = (dst.to(dtype) + 0.5) * scale - 0.5
    fl = torch.floor(src)
    lo = fl.long().clamp(min=0)
    hi = torch.ceil(src).long().clamp(max=n_in - 1)
    return lo, hi, src - fl


def nearest_coordinate(dst, n_in, n_out, dtype=torch.float32):
    """(dst + 0.5) * (in / out): float32 in TF, whatever the data's dtype."""
    scale = torch.tensor(n_in, dtype=dtype) / torch.tensor(n_out, dtype=dtype)
    return (dst.to(dtype) + 0.5) * scale


def nearest_index(dst, n_in, n_out):
    return torch.floor(nearest_coordinate(dst, n_in, n_out)).long().clamp(max=n_in - 1)


def resize_bilinear(img, rows, cols, t_h, t_w):
    """Rows `rows` and columns `cols` of tf.image.resize(img [H,W,C], (t_h, t_w), BILINEAR): along x within the two rows, then y."""
    H, W, _ = img.shape
    y0, y1, wy = bilinear_taps(rows, H, t_h, img.dtype)
    x0, x1, wx = bilinear_taps(cols, W, t_w, img.dtype)
    wy, wx = wy[:, None, None], wx[None, :, None]
    tl, tr, bl, br = img[y0][:, x0], img[y0][:, x1], img[y1][:, x0], img[y1][:, x1]
    top = tl + (tr - tl) * wx
    bot = bl + (br - bl) * wx
    return top + (bot - top) * wy


def resize_nearest(x, rows, cols, t_h, t_w):
    H, W = x.shape[:2]
    return x[nearest_index(rows, H, t_h)][:, nearest_index(cols, W, t_w)]


def frame_coordinates(p):
    """The row and column, in the resized image, of every frame row and column: the flips act on the window."""
    Hf, Wf = p["full_hw"]
    rows, cols = torch.arange(Hf), torch.arange(Wf)
    if p.get("vflip"):
        rows = Hf - 1 - rows
    if p.get("hflip"):
        cols = Wf - 1 - cols
    return rows + p.get("win_y", 0), cols + p.get("win_x", 0)


def spatial(img1, img2, flow, valid, p, dtype):
    """-> (frame1, frame2 [3,Hf,Wf] in [0, 255], frame_flow [2,Hf,Wf], frame_valid [1,Hf,Wf])."""
    rows, cols = frame_coordinates(p)
    unit = 1.0 if img1.dtype == torch.uint8 else 255.0
    imgs = [t.to(dtype) for t in (img1, img2)]
    flow = flow.to(dtype)
    valid = torch.ones(flow.shape[:2], dtype=dtype) if valid is None else valid.to(dtype)
    if p.get("resize"):
        t_h, t_w = p["t_h"], p["t_w"]
        frames = [resize_bilinear(t, rows, cols, t_h, t_w) for t in imgs]
        f = resize_nearest(flow, rows, cols, t_h, t_w) * torch.tensor([p["scale_x"], p["scale_y"]], dtype=dtype)
        v = resize_nearest(valid, rows, cols, t_h, t_w)
    else:
        frames = [t[rows][:, cols] for t in imgs]
        f, v = flow[rows][:, cols], valid[rows][:, cols]
    f = f * torch.tensor([-1.0 if p.get("hflip") else 1.0, -1.0 if p.get("vflip") else 1.0], dtype=dtype)
    if unit != 1.0:
        frames = [t * unit for t in frames]
    return frames[0].permute(2, 0, 1), frames[1].permute(2, 0, 1), f.permute(2, 0, 1), v[None]


# --------------------------------------------------------------------------------------------------------------- colour
def rgb_to_hsv(rgb):
    """[3,...] -> (h, s, v): v = max, c = max - min, s = c / v (0 when v <= 0), h the hexcone sector in [0, 1), 0 when c = 0."""
    r, g, b = rgb[0], rgb[1], rgb[2]
    v = torch.maximum(r, torch.maximum(g, b))
    c = v - torch.minimum(r, torch.minimum(g, b))
    pos = v > 0
    s = torch.where(pos, c / torch.where(pos, v, torch.ones_like(v)), torch.zeros_like(v))
    cc = torch.where(c > 0, c, torch.ones_like(c))
    hr = ((g - b) / cc) / 6.0
    hr = torch.where(hr < 0, hr + 1.0, hr)
    hg = (2.0 + (b - r) / cc) / 6.0
    hb = (4.0 + (r - g) / cc) / 6.0
    h = torch.where(r == v, hr, torch.where(g == v, hg, hb))
    return torch.where(c > 0, h, torch.zeros_like(h)), s, v


def hsv_to_rgb(h, s, v):
    h6 = 6.0 * h
    d = torch.stack([(h6 - 3.0).abs() - 1.0, 2.0 - (h6 - 2.0).abs(), 2.0 - (h6 - 4.0).abs()]).clamp(0.0, 1.0)
    return ((d - 1.0) * s + 1.0) * v


def adjust_saturation(rgb, factor):
    h, s, v = rgb_to_hsv(rgb)
    return hsv_to_rgb(h, (s * factor).clamp(0.0, 1.0), v)


def adjust_hue(rgb, delta):
    h, s, v = rgb_to_hsv(rgb)
    h = h + delta
    return hsv_to_rgb(h - torch.floor(h), s, v)


def adjust_contrast(x, factor, mean):
    return (x - mean) * factor + mean


def colour(crop1, crop2, p):
    """The crops [3,h,w] in [0, 255] -> after ColorJitter, clipped, in [0, 255].  Symmetric: one contrast mean per channel over
    both crops (the reference stacks them into one 2h x w image); asymmetric: per image."""
    quads = p.get("colour", (IDENTITY, IDENTITY))
    xs = [c / 255.0 * q[0] for c, q in zip((crop1, crop2), quads)]
    if p.get("asymmetric"):
        means = [x.mean((1, 2), keepdim=True) for x in xs]
    else:
        means = [torch.cat(xs, 1).mean((1, 2), keepdim=True)] * 2
    out = []
    for x, m, q in zip(xs, means, quads):
        x = adjust_hue(adjust_saturation(adjust_contrast(x, q[1], m), q[2]), q[3])
        out.append(x.clamp(0.0, 1.0) * 255.0)
    return out


def eraser(crop2, rects):
    """The mean colour of the crop before any rectangle, written into every rectangle (x0, y0, dx, dy)."""
    mean = crop2.mean((1, 2), keepdim=True)
    out = crop2.clone()
    for x0, y0, dx, dy in rects:
        if dx > 0 and dy > 0:
            out[:, y0:y0 + dy, x0:x0 + dx] = mean
    return out


def augment_sample(img1, img2, flow, valid, p, dtype):
    """One sample -> dict of the eight outputs of fsraft_augment."""
    f1, f2, ff, fv = spatial(img1, img2, flow, valid, p, dtype)
    (h, w), cy, cx = p["crop_hw"], p.get("crop_y", 0), p.get("crop_x", 0)
    win = (slice(None), slice(cy, cy + h), slice(cx, cx + w))
    c1, c2 = colour(f1[win], f2[win], p)
    return dict(frame1=f1, frame2=f2, frame_flow=ff, frame_valid=fv, crop1=c1, crop2=eraser(c2, p.get("rects", ())),
                crop_flow=ff[win], crop_valid=fv[win])


def evaluate(case, dtype):
    """Every output of the case, [B, ...] each, computed in `dtype`."""
    per = [augment_sample(case["image1"][b], case["image2"][b], case["flow"][b], None if case["valid"] is None else case["valid"][b],
                          p, dtype) for b, p in enumerate(case["params"])]
    return {k: torch.stack([s[k] for s in per]) for k in per[0]}


# ------------------------------------------------------------------------------------------------------------ the cases
def params(src_hw, full_hw, crop_hw, resize_to=None, **kw):
    p = dict(src_hw=tuple(src_hw), full_hw=tuple(full_hw), crop_hw=tuple(crop_hw), t_h=src_hw[0], t_w=src_hw[1])
    if resize_to is not None:
        t_h, t_w = resize_to
        p.update(resize=True, t_h=t_h, t_w=t_w, scale_y=float(np.float32(t_h) / np.float32(src_hw[0])),
                 scale_x=float(np.float32(t_w) / np.float32(src_hw[1])))
    p.update(kw)
    return p


SYM = ((1.13, 0.82, 1.21, 0.057),) * 2
SYM2 = ((0.78, 1.27, 0.74, -0.081),) * 2
SYM3 = ((0.91, 1.06, 1.0, 0.0),) * 2
ASYM = ((1.22, 1.18, 0.83, -0.031), (0.74, 0.88, 1.29, 0.093))
S, F, C = (37, 53), (32, 48), (16, 24)

# name -> (parameter sets of the batch, valid map with holes?).  Every source has odd sides: (dst + 0.5) * in / out =
# (2 dst + 1) * in / (2 out) is then an odd number over an even one, at least 1 / (2 out) from an integer.
SPECS = (
    ("copy", [params(S, F, C, win_y=3, win_x=5, crop_y=8, crop_x=16, colour=SYM)], False),
    ("resize-hflip", [params(S, F, C, (51, 67), win_y=7, win_x=9, hflip=True, crop_y=16, crop_x=8, colour=SYM2,
                             rects=((3, 2, 9, 6),))], False),
    # both flips, asymmetric colour, two rectangles that overlap, the second ending on the crop's right and bottom edge
    ("resize-flips-asym-2rect", [params(S, F, C, (51, 67), win_y=19, win_x=19, hflip=True, vflip=True, crop_y=8, crop_x=24, asymmetric=True,
                                        colour=ASYM, rects=((10, 5, 8, 6), (14, 9, 10, 7)))], True),
    ("crop17x23", [params(S, F, (17, 23), (49, 71), win_y=11, win_x=2, crop_y=8, crop_x=16, colour=SYM, rects=((22, 16, 1, 1), (5, 5, 0, 9)))],
     False),
    ("batch3", [params(S, F, C),
                params(S, F, C, (51, 67), win_y=0, win_x=19, hflip=True, crop_y=16, crop_x=24, colour=SYM),
                params(S, F, C, win_y=5, win_x=0, vflip=True, crop_y=0, crop_x=8, asymmetric=True, colour=ASYM, rects=((0, 0, 24, 3),))], True),
    # a 40 x 72 crop of a 48 x 80 frame: 15 and 12 blocks of 256 pixels in the reductions
    ("blocks", [params((53, 85), (48, 80), (40, 72), (61, 97), win_y=13, win_x=17, crop_y=8, crop_x=0, colour=SYM2,
                       rects=((30, 20, 42, 20), (0, 0, 50, 40))),
                params((53, 85), (48, 80), (40, 72), (75, 120), win_y=0, win_x=40, vflip=True, crop_y=0, crop_x=8, asymmetric=True,
                       colour=ASYM)], True),
    # 17 samples: more than the 16 whose parameters one launch carries, so the second chunk's offsets are exercised
    ("chunks", [params(S, F, C, (51, 67) if b % 3 else None, win_y=b % 6, win_x=(5 * b) % 6, hflip=b % 2 == 1, vflip=b % 5 == 2,
                       crop_y=8 * (b % 3), crop_x=8 * (b % 4), asymmetric=b % 4 == 3, colour=ASYM if b % 4 == 3 else (SYM, SYM2, SYM3)[b % 3],
                       rects=(((b, 16 - b, 24 - b, b),) if b % 2 == 0 else ())) for b in range(17)], True),
)
# 736 x 736 = 541696 frame pixels and 728 x 728 = 529984 crop pixels: both beyond the 2048 blocks of 256 the grids stop at,
# so the scratch size is at its cap and the kernels stride
CAP = ("cap", [params((739, 741), (736, 736), (728, 728), win_y=3, win_x=4, crop_y=8, crop_x=0, colour=SYM, rects=((700, 650, 28, 78),))], True)
DTYPES = ("u8", "f32")


def make_case(name, plist, holes, kind, seed):
    g = torch.Generator().manual_seed(seed)
    B, (Hs, Ws) = len(plist), plist[0]["src_hw"]
    if kind == "u8":
        imgs = [torch.randint(0, 256, (B, Hs, Ws, 3), generator=g, dtype=torch.uint8) for _ in range(2)]
    else:
        imgs = [torch.rand(B, Hs, Ws, 3, generator=g, dtype=torch.float32) for _ in range(2)]
    flow = (20.0 * (torch.rand(B, Hs, Ws, 2, generator=g, dtype=torch.float64) - 0.5)).float()
    valid = (torch.rand(B, Hs, Ws, generator=g) > 0.3).float() if holes else None
    return dict(name=f"{name}-{kind}", kind=kind, image1=imgs[0], image2=imgs[1], flow=flow, valid=valid, params=plist)


@functools.lru_cache(maxsize=None)
def cases():
    out = [make_case(name, plist, holes, kind, 7100 + 10 * i + k) for i, (name, plist, holes) in enumerate(SPECS) for k, kind in enumerate(DTYPES)]
    return out + [make_case(*CAP, "u8", 7900)]


def nearest_margin(case):
    """The input condition of a case: the least distance of a nearest-neighbour coordinate (dst + 0.5) * scale from an integer,
    over every frame row and column of every resized sample (inf without one)."""
    worst = float("inf")
    for p in case["params"]:
        if not p.get("resize"):
            continue
        rows, cols = frame_coordinates(p)
        for dst, n_in, n_out in ((rows, p["src_hw"][0], p["t_h"]), (cols, p["src_hw"][1], p["t_w"])):
            for dtype in (torch.float32, torch.float64):
                c = nearest_coordinate(dst, n_in, n_out, dtype).double()
                worst = min(worst, float((c - torch.round(c)).abs().min()))
    return worst


@functools.lru_cache(maxsize=None)
def reference(i):
    return evaluate(cases()[i], torch.float64)


@functools.lru_cache(maxsize=None)
def twin(i):
    return evaluate(cases()[i], torch.float32)


def field_error(x, ref):
    """Worst absolute error in units of 2^-24 * max|ref| (0 where the reference is all zero and x is too)."""
    scale = float(ref.abs().max()) * 2.0 ** -24
    err = float((x.double() - ref.double()).abs().max())
    return err / scale if scale > 0 else (0.0 if err == 0 else float("inf"))


EXACT = ("frame_flow", "frame_valid", "crop_flow", "crop_valid")       # copies, one multiply and sign flips: the twin's bits
QUANTITIES = {"frame": ("frame1", "frame2"), "crop": ("crop1", "crop2")}


def resized(case):
    return any(p.get("resize") for p in case["params"])


@functools.lru_cache(maxsize=None)
def twin_errors():
    """The fp32 twin's worst error against fp64 over the GPU cases, per quantity, in units of 2^-24 * max|ref|."""
    worst = {q: 0.0 for q in QUANTITIES}
    for i in range(len(cases())):
        for q, keys in QUANTITIES.items():
            worst[q] = max([worst[q]] + [field_error(twin(i)[k], reference(i)[k]) for k in keys])
    return worst


def limits():
    """FACTOR times the twin's worst error, per quantity."""
    return {q: FACTOR * e for q, e in twin_errors().items()}
