"""A restatement in plain torch of what fsraft_augment_sup (csrc/augment.hip) computes: the reference's FlowAugmentor and
SparseFlowAugmentor (pytorch/raft_utils/augmentor.py:39-188, :191-330) applied with given parameters, in the order of their
__call__ -- colour, eraser, spatial -- so the colour step and the eraser act on the SOURCE and the resize interpolates pixels
that were already jittered, clipped and erased.  The resizes and the colour functions are those of _augref.py (TF2's
tf.image.resize with half-pixel centres, its fused saturation / hue kernels).  It computes in the dtype it is given: float64 is
the reference, float32 the twin that rounds every operation and gives the limits.

Parameters are dicts with the field names of flow_supervisor_amd.augment.AugParams (win_y = win_x = 0, full_hw = (t_h, t_w),
rects in source coordinates); sources are interleaved ([Hs,Ws,3] images, uint8 or float in [0, 1]; [Hs,Ws,2] flow; [Hs,Ws]
valid), results planar ([3,h,w] ...), images in [0, 255].  mode 'dense' is FlowAugmentor (bilinear flow, valid all ones),
'sparse' SparseFlowAugmentor (nearest-neighbour flow and valid).
"""
import functools

import numpy as np
import torch

from _augref import (ASYM, IDENTITY, SYM, SYM2, SYM3, adjust_contrast, adjust_hue, adjust_saturation, field_error, nearest_coordinate,
                     resize_bilinear, resize_nearest)

FACTOR = 4.0                     # a different summation order in the kernels' means (as in _augref.py)
MODES = ("dense", "sparse")
DTYPES = ("u8", "f32")


# ---------------------------------------------------------------------------------------------------------- the definition
def photometric(img1, img2, p, dtype):
    """P_1, P_2 [3,Hs,Ws] in [0, 1]: clip(hue(sat(contrast(x * brightness)))).  The contrast mean is per channel over the whole
    brightness-scaled source; symmetric: over both sources (the reference stacks them into one image, :73-75, :215-217)."""
    quads = p.get("colour", (IDENTITY, IDENTITY))
    xs = []
    for img, q in zip((img1, img2), quads):
        x = img.to(dtype) / 255.0 if img.dtype == torch.uint8 else img.to(dtype)
        xs.append(x.permute(2, 0, 1) * q[0])
    if p.get("asymmetric"):
        means = [x.mean((1, 2), keepdim=True) for x in xs]
    else:
        means = [torch.cat(xs, 1).mean((1, 2), keepdim=True)] * 2
    return [adjust_hue(adjust_saturation(adjust_contrast(x, q[1], m), q[2]), q[3]).clamp(0.0, 1.0) for x, m, q in zip(xs, means, quads)]


def eraser(img2, rects):
    """The mean colour of the whole image before any rectangle, written into every rectangle (x0, y0, dx, dy)."""
    mean = img2.mean((1, 2), keepdim=True)
    out = img2.clone()
    for x0, y0, dx, dy in rects:
        if dx > 0 and dy > 0:
            out[:, y0:y0 + dy, x0:x0 + dx] = mean
    return out


def crop_coordinates(p):
    """The row and column, in the resized image, of every crop row and column: the flips act on the whole resized image."""
    (h, w), t_h, t_w = p["crop_hw"], p["t_h"], p["t_w"]
    rows, cols = torch.arange(h) + p.get("crop_y", 0), torch.arange(w) + p.get("crop_x", 0)
    if p.get("vflip"):
        rows = t_h - 1 - rows
    if p.get("hflip"):
        cols = t_w - 1 - cols
    return rows, cols


def augment_sample(img1, img2, flow, valid, p, dtype, mode):
    """One sample -> dict of the four outputs of fsraft_augment_sup."""
    P1, P2 = photometric(img1, img2, p, dtype)
    E = [P1, eraser(P2, p.get("rects", ()))]
    rows, cols = crop_coordinates(p)
    t_h, t_w = p["t_h"], p["t_w"]
    flow = flow.to(dtype)
    # dense: d_m of flow_dataset.py:126 is all ones, a given valid map is ignored
    valid = torch.ones(flow.shape[:2], dtype=dtype) if valid is None or mode == "dense" else valid.to(dtype)
    if p.get("resize"):
        crops = [resize_bilinear(e.permute(1, 2, 0), rows, cols, t_h, t_w) * 255.0 for e in E]
        f = resize_bilinear(flow, rows, cols, t_h, t_w) if mode == "dense" else resize_nearest(flow, rows, cols, t_h, t_w)
        f = f * torch.tensor([p["scale_x"], p["scale_y"]], dtype=dtype)
        v = resize_nearest(valid, rows, cols, t_h, t_w)
    else:
        crops = [e.permute(1, 2, 0)[rows][:, cols] * 255.0 for e in E]
        f, v = flow[rows][:, cols], valid[rows][:, cols]
    f = f * torch.tensor([-1.0 if p.get("hflip") else 1.0, -1.0 if p.get("vflip") else 1.0], dtype=dtype)
    return dict(crop1=crops[0].permute(2, 0, 1), crop2=crops[1].permute(2, 0, 1), crop_flow=f.permute(2, 0, 1), crop_valid=v[None])


def evaluate(case, dtype):
    """Every output of the case, [B, ...] each, computed in `dtype`."""
    per = [augment_sample(case["image1"][b], case["image2"][b], case["flow"][b], None if case["valid"] is None else case["valid"][b],
                          p, dtype, case["mode"]) for b, p in enumerate(case["params"])]
    return {k: torch.stack([s[k] for s in per]) for k in per[0]}


# ------------------------------------------------------------------------------------------------------------ the cases
def params(src_hw, crop_hw, resize_to=None, **kw):
    p = dict(src_hw=tuple(src_hw), full_hw=tuple(src_hw), crop_hw=tuple(crop_hw), t_h=src_hw[0], t_w=src_hw[1])
    if resize_to is not None:
        t_h, t_w = resize_to
        p.update(resize=True, t_h=t_h, t_w=t_w, full_hw=(t_h, t_w), scale_y=float(np.float32(t_h) / np.float32(src_hw[0])),
                 scale_x=float(np.float32(t_w) / np.float32(src_hw[1])))
    p.update(kw)
    return p


S, C, S2 = (37, 53), (16, 24), (53, 85)
# the dense fallback (augmentor.py:145-154): source 21 x 29 under crop + 8 = 24 x 32, min_scale = max(24 / 21, 32 / 29) in float32,
# t = rint(n * min_scale) = 24 x 33, and the flow is multiplied by min_scale itself
MIN_SCALE = float(max(np.float32(24.0) / np.float32(21), np.float32(32.0) / np.float32(29)))
FALLBACK_T = (int(np.rint(np.float32(21) * np.float32(MIN_SCALE))), int(np.rint(np.float32(29) * np.float32(MIN_SCALE))))


def asym_if(dense, **kw):
    """Asymmetric colour for FlowAugmentor alone: SparseFlowAugmentor never draws it."""
    return dict(kw, asymmetric=True, colour=ASYM) if dense else dict(kw, colour=SYM2)


def specs(dense):
    """name -> (parameter sets of the batch, valid map with holes?).  Every source has odd sides and no resized side is above
    120: (dst + 0.5) * in / out = (2 dst + 1) * in / (2 out) is then an odd number over an even one, at least 1 / 240 from an
    integer."""
    return (
        ("copy", [params(S, C, crop_y=7, crop_x=11, colour=SYM, rects=((10, 6, 9, 7),))], True),
        ("up-hflip", [params(S, C, (51, 67), hflip=True, crop_y=13, crop_x=21, colour=SYM2, rects=((3, 2, 9, 6),))], False),
        ("down", [params(S, C, (31, 43), crop_y=9, crop_x=15, colour=SYM, rects=((20, 11, 17, 12),))], True),
        # both flips, two rectangles that overlap, the second ending on the source's right and bottom edge
        ("flips-2rect", [params(S, C, (51, 67), hflip=True, vflip=True, crop_y=3, crop_x=5,
                                **asym_if(dense, rects=((20, 10, 20, 12), (30, 18, 23, 19))))], True),
        ("crop17x23", [params(S, (17, 23), (49, 71), crop_y=21, crop_x=30, colour=SYM, rects=((22, 16, 1, 1), (5, 5, 0, 9)))], False),
        # three resized sizes in one batch
        ("batch3", [params(S, C, crop_y=21, crop_x=29),
                    params(S, C, (51, 67), hflip=True, crop_y=35, crop_x=43, colour=SYM),
                    params(S, C, (45, 71), vflip=True, crop_y=0, crop_x=1, **asym_if(dense, rects=((0, 0, 53, 3),)))], True),
        # a 53 x 85 source: 18 blocks of 256 pixels in the source reductions; a 40 x 72 crop: 12 blocks in the output kernel
        ("blocks", [params(S2, (40, 72), (61, 97), crop_y=13, crop_x=17, colour=SYM2, rects=((30, 20, 42, 20), (0, 0, 50, 40))),
                    params(S2, (40, 72), (75, 120), vflip=True, crop_y=35, crop_x=48, **asym_if(dense))], True),
        # 17 samples: more than the 16 whose parameters one launch carries, so the second chunk's offsets are exercised
        ("chunks", [params(S, C, ((51, 67), (45, 71))[b % 2] if b % 3 else None, hflip=b % 2 == 1, vflip=b % 5 == 2,
                           crop_y=(3 * b) % 20, crop_x=(5 * b) % 28, **(asym_if(dense) if b % 4 == 3 else dict(colour=(SYM, SYM2, SYM3)[b % 3])),
                           rects=(((b, 16 - b, 24 - b, b),) if b % 2 == 0 else ())) for b in range(17)], True),
    )


FALLBACK = ("fallback", [params((21, 29), C, FALLBACK_T, crop_y=5, crop_x=8, colour=SYM, rects=((4, 3, 11, 9),),
                                scale_x=MIN_SCALE, scale_y=MIN_SCALE)], False)
# 739 x 741 = 547599 source pixels: beyond the 2048 blocks of 256 the source reductions stop at, so the scratch size is at its
# cap and they stride; not resized, a 64 x 64 crop
CAP = ("cap", [params((739, 741), (64, 64), crop_y=601, crop_x=333, colour=SYM, rects=((320, 590, 60, 149),))], True)


def make_case(name, plist, holes, kind, mode, seed):
    g = torch.Generator().manual_seed(seed)
    B, (Hs, Ws) = len(plist), plist[0]["src_hw"]
    if kind == "u8":
        imgs = [torch.randint(0, 256, (B, Hs, Ws, 3), generator=g, dtype=torch.uint8) for _ in range(2)]
    else:
        imgs = [torch.rand(B, Hs, Ws, 3, generator=g, dtype=torch.float32) for _ in range(2)]
    flow = (20.0 * (torch.rand(B, Hs, Ws, 2, generator=g, dtype=torch.float64) - 0.5)).float()
    valid = (torch.rand(B, Hs, Ws, generator=g) > 0.3).float() if holes else None
    return dict(name=f"{name}-{mode}-{kind}", kind=kind, mode=mode, image1=imgs[0], image2=imgs[1], flow=flow, valid=valid, params=plist)


@functools.lru_cache(maxsize=None)
def cases():
    out, seed = [], 8100
    for mode in MODES:
        for name, plist, holes in specs(mode == "dense") + ((FALLBACK,) if mode == "dense" else ()):
            for kind in DTYPES:
                out.append(make_case(name, plist, holes, kind, mode, seed))
                seed += 1
    return out + [make_case(*CAP, "u8", "sparse", 8900)]


def nearest_margin(case):
    """The input condition of a case: the least distance of a nearest-neighbour coordinate (dst + 0.5) * scale from an integer,
    in float32 and in float64, over every crop row and column of every resized sample (inf without one)."""
    worst = float("inf")
    for p in case["params"]:
        if not p.get("resize"):
            continue
        rows, cols = crop_coordinates(p)
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


IMAGES = ("crop1", "crop2")


def bilinear_flow(case, b):
    """Whether sample b's flow is interpolated (held to a limit) -- else it is a copy or a nearest neighbour, times the scales and
    the signs: the twin's bits."""
    return case["mode"] == "dense" and bool(case["params"][b].get("resize"))


@functools.lru_cache(maxsize=None)
def twin_errors():
    """The fp32 twin's worst error against fp64 over the GPU cases, per quantity and sample, in units of 2^-24 * max|ref|."""
    worst = {"image": 0.0, "flow": 0.0}
    for i, case in enumerate(cases()):
        for b in range(len(case["params"])):
            worst["image"] = max([worst["image"]] + [field_error(twin(i)[k][b], reference(i)[k][b]) for k in IMAGES])
            if bilinear_flow(case, b):
                worst["flow"] = max(worst["flow"], field_error(twin(i)["crop_flow"][b], reference(i)["crop_flow"][b]))
    return worst


def limits():
    """FACTOR times the twin's worst error, per quantity."""
    return {q: FACTOR * e for q, e in twin_errors().items()}
