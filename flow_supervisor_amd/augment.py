"""UnsupAugmentor (pytorch/raft_utils/augmentor.py:496-657): what produces the tuple SemiTrainStep / L2L consume -- the
uncropped frame, the 8-aligned crop after colour and eraser augmentation, and the crop's offsets -- with the parameters drawn
on the host and applied on the device by csrc/augment.hip.

    UnsupAugmentor(crop_size, ...)          the reference's constructor and constants
        .sample(src_hw, generator)          -> AugParams, one sample's parameters from a CPU torch.Generator
        (image1, image2, flow, valid)       sample per sample, then apply: the reference's pair of dicts
    apply(image1, image2, flow, valid, params)      the kernels on already-drawn parameters -> dict
    as_step_input(out)                      -> (image1, image2, ci1, ci2, ox, oy, flow, valid) for SemiTrainStep
    add_noise(images, stdv)                 pytorch/train.py:263-268
    FlowAugmentor / SparseFlowAugmentor     the supervised augmentors (:39-188, :191-330; colour -> eraser -> spatial), what
        .sample, (image1, image2, flow[, valid])    FlowDataset.augment runs for every labelled sample -> (image1, image2, flow, valid)
    apply_supervised(image1, image2, flow, valid, params, dense)    their kernels (fsraft_augment_sup) on already-drawn parameters

The reference's class is TensorFlow on the host (tf.image.resize, tf.image.random_*).  TensorFlow does not run here, so nothing
is generated from it: the distributions and the arithmetic are restated from its source as written, quirks included, the bit
stream is torch's, and the formulas of include/fsraft.h (tf.image.resize BILINEAR / NEAREST_NEIGHBOR with half-pixel centres,
TF's fused saturation / hue kernels) are the definition.  PyTorch layout on the way out: planar fp32, images in [0, 255] (the
"* 255" of pytorch/train.py:251-258 is folded in).  CUDA (ROCm) tensors only: there is no CPU implementation of `apply`.

Not implemented: MultiFrameAugmentor, rotation (do_rotation is False everywhere), the OpenCV variants of
pytorch/core/utils/augmentor.py (they scatter sparse flow instead of resizing it), datasets.
"""
import dataclasses

import numpy as np
import torch

from . import _lib as L
from . import ops

_f32 = np.float32


@dataclasses.dataclass(frozen=True)
class AugParams:
    """One sample's parameters, plain Python numbers.  The frame is the full_hw window at (win_y, win_x) of the source resized
    to (t_h, t_w) (resize False: of the source), flipped; the crop the crop_hw window of the frame at (crop_y, crop_x);
    colour = ((brightness, contrast, saturation, hue_delta) of image 1, of image 2); rects = ((x0, y0, dx, dy), ...) of image 2;
    stretched records the sampler's stretch branch and changes nothing by itself."""
    src_hw: tuple
    full_hw: tuple
    crop_hw: tuple
    resize: bool = False
    t_h: int = 0
    t_w: int = 0
    scale_x: float = 1.0
    scale_y: float = 1.0
    win_y: int = 0
    win_x: int = 0
    hflip: bool = False
    vflip: bool = False
    crop_y: int = 0
    crop_x: int = 0
    asymmetric: bool = False
    colour: tuple = ((1.0, 1.0, 1.0, 0.0), (1.0, 1.0, 1.0, 0.0))
    rects: tuple = ()
    stretched: bool = False


def identity_params(src_hw, full_hw, crop_hw, **changes):
    """The parameters that change nothing: the top-left window of the source, no colour change, no rectangle."""
    return AugParams(tuple(src_hw), tuple(full_hw), tuple(crop_hw), **{**dict(t_h=src_hw[0], t_w=src_hw[1]), **changes})


def resized_size(n, scale):
    """(t, t / n): augmentor.py:583-587.  float32 arithmetic, and tf.round rounds half to even."""
    t = int(np.rint(_f32(n) * _f32(scale)))
    return t, float(_f32(t) / _f32(n))


def _uniform(g, lo=0.0, hi=1.0):
    """tf.random.uniform([], lo, hi) in float32: lo + (hi - lo) * u, which also holds when hi < lo."""
    u = _f32(torch.rand((), generator=g, dtype=torch.float32).item())
    return _f32(lo) + (_f32(hi) - _f32(lo)) * u


def _randint(g, lo, hi):
    """tf.random.uniform([], lo, hi, dtype=tf.int32): an integer in [lo, hi)."""
    return int(torch.randint(int(lo), int(hi), (), generator=g).item())


class ColorJitter:
    """augmentor.py:15-37: the four factors of one call, in its order of draws."""

    def __init__(self, brightness, contrast, saturation, hue):
        self.brightness, self.contrast, self.saturation, self.hue = brightness, contrast, saturation, hue

    def sample(self, g):
        b = _uniform(g, max(0.0, 1.0 - self.brightness), 1.0 + self.brightness)       # :24-25
        c = _uniform(g, max(0.0, 1.0 - self.contrast), 1.0 + self.contrast)           # :29 tf.image.random_contrast
        s = _uniform(g, max(0.0, 1.0 - self.saturation), 1.0 + self.saturation)       # :32 tf.image.random_saturation
        h = _uniform(g, -self.hue, self.hue)                                          # :35 tf.image.random_hue
        return float(b), float(c), float(s), float(h)


def _eraser_rects(g, prob, bounds, h, w):
    """The draws of eraser_transform (:83-106, :225-248, :523-550) on an h x w image -> ((x0, y0, dx, dy), ...)."""
    rects = []
    if _uniform(g) < prob:                                                             # :529
        for _ in range(_randint(g, 1, 3)):                                             # :531: 1 or 2 rectangles
            x0, y0 = _randint(g, 0, w), _randint(g, 0, h)
            size = []
            for n, o in ((w, x0), (h, y0)):                                            # :534-539
                lo, hi = min(bounds[0], n - o), min(bounds[1], n - o + 1)
                # where the bounds collapse (lo >= hi: an image under 100 pixels, or a rectangle that reaches the edge),
                # where TF would refuse the empty range, take lo
                size.append(lo if lo >= hi else _randint(g, lo, hi))
            rects.append((x0, y0, size[0], size[1]))
    return tuple(rects)


class UnsupAugmentor:
    """The reference's UnsupAugmentor (SparseFlowAugmentor's constructor, augmentor.py:192-211, and the overrides of :496-500)."""

    def __init__(self, crop_size, min_scale=-0.2, max_scale=0.5, do_flip=False, eraser_aug_prob=0.5, full_size=None):
        self.crop_size = (int(crop_size[0]), int(crop_size[1]))
        # quirk, :499: `self.min_scale = 1.` after the parent's constructor overrides the argument
        self.min_scale = 1.0
        self.max_scale = max_scale
        self.spatial_aug_prob = 0.8
        self.stretch_prob = 0.8
        self.max_stretch = 0.2
        self.do_flip = do_flip
        self.h_flip_prob = 0.5
        self.v_flip_prob = 0.1
        self.photo_aug = ColorJitter(brightness=0.3, contrast=0.3, saturation=0.3, hue=0.3 / 3.14)
        self.asymmetric_color_aug_prob = 0.2
        self.eraser_aug_prob = eraser_aug_prob
        self.eraser_bounds = (50, 100)
        # (:500 sets full_size to None after construction; the datasets assign it afterwards, which the argument stands for)
        self.full_size = None if full_size is None else (int(full_size[0]), int(full_size[1]))

    # ------------------------------------------------------------------------------------------------------------ sampler
    def _spatial(self, ht, wd, g):
        # :558-565 get_proc_size_floor: the source size floored to a multiple of 8, at most the full_size argument
        full_h, full_w = ht // 8 * 8, wd // 8 * 8
        if self.full_size is not None:
            full_h, full_w = min(full_h, self.full_size[0]), min(full_w, self.full_size[1])
        ch, cw = self.crop_size
        if full_h < ch or full_w < cw:
            raise ValueError(f"full_size {full_h} x {full_w} (source {ht} x {wd}) is smaller than crop_size {ch} x {cw}")
        # quirk, :571: uniform(min_scale = 1, max_scale) with max_scale < 1 is 1 + (max_scale - 1) * u
        scale = _f32(2.0) ** _uniform(g, self.min_scale, self.max_scale)
        scale_x = scale_y = scale
        stretched = bool(_uniform(g) < self.stretch_prob)
        if stretched:                                                                  # :574-576
            scale_x = scale_x * _f32(2.0) ** _uniform(g, -self.max_stretch, self.max_stretch)
            scale_y = scale_y * _f32(2.0) ** _uniform(g, -self.max_stretch, self.max_stretch)
        # quirk, :578-579: tf.clip_by_value(scale_x, min_scale, scale_x) is min(max(x, lo), x) = x; the min_scale of :567-569
        # has no effect, and there is no `min_scale > 1` fallback either
        p = dict(src_hw=(ht, wd), full_hw=(full_h, full_w), crop_hw=(ch, cw), t_h=ht, t_w=wd, stretched=stretched)
        if _uniform(g) < self.spatial_aug_prob:                                        # :581-598
            t_h, sy = resized_size(ht, scale_y)
            t_w, sx = resized_size(wd, scale_x)
            if t_h < full_h or t_w < full_w:
                raise ValueError(f"the resized frame {t_h} x {t_w} is smaller than full_size {full_h} x {full_w}")
            p.update(resize=True, t_h=t_h, t_w=t_w, scale_x=sx, scale_y=sy)
        # :593-594 / :600-601: the window, y before x, both ends included.  Without the spatial branch there is no resize at all.
        p["win_y"] = _randint(g, 0, p["t_h"] - full_h + 1)
        p["win_x"] = _randint(g, 0, p["t_w"] - full_w + 1)
        if self.do_flip:                                                               # :607-618
            p["hflip"] = bool(_uniform(g) < self.h_flip_prob)
            p["vflip"] = bool(_uniform(g) < self.v_flip_prob)
        p["crop_y"] = 8 * _randint(g, 0, (full_h - ch) // 8 + 1)                       # :621-622
        p["crop_x"] = 8 * _randint(g, 0, (full_w - cw) // 8 + 1)
        return p

    def _colour(self, g):
        if _uniform(g) < self.asymmetric_color_aug_prob:                               # :507-509: one quadruple per image
            return True, (self.photo_aug.sample(g), self.photo_aug.sample(g))
        q = self.photo_aug.sample(g)                                                   # :512-515: one for the stacked pair
        return False, (q, q)

    def _eraser(self, g):
        return _eraser_rects(g, self.eraser_aug_prob, self.eraser_bounds, *self.crop_size)

    def sample(self, src_hw, generator):
        """One sample's parameters, drawn in the reference's order: spatial, colour, eraser."""
        p = self._spatial(int(src_hw[0]), int(src_hw[1]), generator)
        asym, colour = self._colour(generator)
        return AugParams(asymmetric=asym, colour=colour, rects=self._eraser(generator), **p)

    # --------------------------------------------------------------------------------------------------------------- call
    @L.on_tensor_device
    def __call__(self, image1, image2, flow, valid, generator=None):
        """image1, image2 [B,Hs,Ws,3] (uint8, or fp32 in [0, 1]), flow [B,Hs,Ws,2], valid [B,Hs,Ws] or None ->
        ({'augmented_img', 'original_img', 'crop_x', 'crop_y'}, {'flows', 'original_flows', 'valids', 'original_valids'})."""
        g = generator if generator is not None else torch.default_generator
        out = apply(image1, image2, flow, valid, [self.sample(image1.shape[1:3], g) for _ in range(image1.shape[0])])
        return ({k: out[k] for k in ("augmented_img", "original_img", "crop_x", "crop_y")},
                {k: out[k] for k in ("flows", "original_flows", "valids", "original_valids")})


class FlowAugmentor:
    """The reference's FlowAugmentor (augmentor.py:39-188, dense ground truth).  __call__ is colour -> eraser -> spatial
    (:183-188) and the draws come in that order; the colour step and the eraser act on the source, the resize on their result."""
    dense = True

    def __init__(self, crop_size, min_scale=-0.2, max_scale=0.5, do_flip=True, eraser_aug_prob=0.5):
        self.crop_size = (int(crop_size[0]), int(crop_size[1]))
        self.min_scale = min_scale                      # (as given: the `= 1.` override is UnsupAugmentor's alone)
        self.max_scale = max_scale
        self.spatial_aug_prob = 0.8
        self.stretch_prob = 0.8
        self.max_stretch = 0.2
        self.do_flip = do_flip
        self.h_flip_prob = 0.5
        self.v_flip_prob = 0.1
        self.photo_aug = ColorJitter(brightness=0.4, contrast=0.4, saturation=0.4, hue=0.5 / 3.14)      # :58
        self.asymmetric_color_aug_prob = 0.2
        self.eraser_aug_prob = eraser_aug_prob
        self.eraser_bounds = (50, 100)

    # ------------------------------------------------------------------------------------------------------------ sampler
    def _colour(self, g):
        if _uniform(g) < self.asymmetric_color_aug_prob:                               # :67-69: one quadruple per image
            return True, (self.photo_aug.sample(g), self.photo_aug.sample(g))
        q = self.photo_aug.sample(g)                                                   # :73-75: one for the stacked pair
        return False, (q, q)

    def _spatial(self, ht, wd, g):
        ch, cw = self.crop_size
        # :118-120 / :271-273, float32
        min_scale = max(_f32(ch + 8.0) / _f32(ht), _f32(cw + 8.0) / _f32(wd))
        scale = _f32(2.0) ** _uniform(g, self.min_scale, self.max_scale)               # :122
        scale_x = scale_y = scale
        stretched = bool(_uniform(g) < self.stretch_prob)
        if stretched:                                                                  # :125-127
            scale_x = scale_x * _f32(2.0) ** _uniform(g, -self.max_stretch, self.max_stretch)
            scale_y = scale_y * _f32(2.0) ** _uniform(g, -self.max_stretch, self.max_stretch)
        # quirk, :129-130 / :282-283: tf.clip_by_value(scale_x, min_scale, scale_x) is min(max(x, lo), x) = x, the identity
        p = dict(src_hw=(ht, wd), crop_hw=(ch, cw), t_h=ht, t_w=wd, stretched=stretched)
        if _uniform(g) < self.spatial_aug_prob:                                        # :132-143 / :285-295
            t_h, sy = resized_size(ht, scale_y)                                        # quirk, :137-138: the scales are re-derived
            t_w, sx = resized_size(wd, scale_x)                                        # from the rounded sizes, f32(t) / f32(n)
            p.update(resize=True, t_h=t_h, t_w=t_w, scale_x=sx, scale_y=sy)
        elif self.dense and min_scale > 1.0:
            # quirk, :145-154, FlowAugmentor alone: a source under crop + 8 is resized by min_scale, and the flow is multiplied
            # by min_scale itself, not by the ratio of the rounded sizes
            p.update(resize=True, t_h=resized_size(ht, min_scale)[0], t_w=resized_size(wd, min_scale)[0], scale_x=float(min_scale),
                     scale_y=float(min_scale))
        if self.do_flip:                                                               # :157-166 / :297-308
            p["hflip"] = bool(_uniform(g) < self.h_flip_prob)
            p["vflip"] = bool(_uniform(g) < self.v_flip_prob)
        if p["t_h"] <= ch or p["t_w"] <= cw:                                           # :170-171: an empty range, where TF dies
            raise ValueError(f"the resized image {p['t_h']} x {p['t_w']} (source {ht} x {wd}) leaves no offset for crop_size {ch} x {cw}: "
                             "both sides must exceed the crop's")
        p["crop_y"] = _randint(g, 0, p["t_h"] - ch)                                    # :170-171 / :311-312: y before x, the upper
        p["crop_x"] = _randint(g, 0, p["t_w"] - cw)                                    # end excluded
        p["full_hw"] = (p["t_h"], p["t_w"])
        return p

    def sample(self, src_hw, generator):
        """One sample's parameters, drawn in the reference's order: colour, eraser, spatial.  full_hw is the resized size."""
        ht, wd = int(src_hw[0]), int(src_hw[1])
        asym, colour = self._colour(generator)
        rects = _eraser_rects(generator, self.eraser_aug_prob, self.eraser_bounds, ht, wd)     # :86 / :228: the SOURCE's size
        return AugParams(asymmetric=asym, colour=colour, rects=rects, **self._spatial(ht, wd, generator))

    # --------------------------------------------------------------------------------------------------------------- call
    @L.on_tensor_device
    def __call__(self, image1, image2, flow, valid=None, generator=None):
        """image1, image2 [B,Hs,Ws,3] (uint8, or fp32 in [0, 1]), flow [B,Hs,Ws,2], valid [B,Hs,Ws] or None ->
        (image1, image2 [B,3,h,w] in [0, 255], flow [B,2,h,w], valid [B,1,h,w])."""
        g = generator if generator is not None else torch.default_generator
        out = apply_supervised(image1, image2, flow, valid, [self.sample(image1.shape[1:3], g) for _ in range(image1.shape[0])],
                               self.dense)
        return out["image1"], out["image2"], out["flow"], out["valid"]


class SparseFlowAugmentor(FlowAugmentor):
    """The reference's SparseFlowAugmentor (augmentor.py:191-330, KITTI / HD1K): flow and valid by the nearest neighbour, never an
    asymmetric colour, no fallback for a small source."""
    dense = False

    def __init__(self, crop_size, min_scale=-0.2, max_scale=0.5, do_flip=False, eraser_aug_prob=0.5):
        super().__init__(crop_size, min_scale, max_scale, do_flip, eraser_aug_prob)
        self.photo_aug = ColorJitter(brightness=0.3, contrast=0.3, saturation=0.3, hue=0.3 / 3.14)      # :209

    def _colour(self, g):
        # quirk, :214-222: asymmetric_color_aug_prob is set (:210) and never read; there is no draw for it
        q = self.photo_aug.sample(g)
        return False, (q, q)


def pack_params(params):
    """list[AugParams] -> the ctypes array of fsraft_aug_params the entry point reads on the host."""
    arr = (L.AugParams * len(params))()
    for a, p in zip(arr, params):
        a.resize, a.th, a.tw = int(p.resize), int(p.t_h), int(p.t_w)
        a.scale_x, a.scale_y = p.scale_x, p.scale_y
        a.win_y, a.win_x, a.hflip, a.vflip, a.crop_y, a.crop_x = int(p.win_y), int(p.win_x), int(p.hflip), int(p.vflip), int(p.crop_y), int(p.crop_x)
        a.asym = int(p.asymmetric)
        for i in range(2):
            a.brightness[i], a.contrast[i], a.saturation[i], a.hue[i] = p.colour[i]
        if len(p.rects) > 2:
            raise ValueError(f"at most two eraser rectangles, got {len(p.rects)}")
        a.nrect = len(p.rects)
        for r, rect in enumerate(p.rects):
            for k in range(4):
                a.rect[r][k] = int(rect[k])
    return arr


@L.on_tensor_device
def apply(image1, image2, flow, valid, params):
    """Already-drawn parameters, one AugParams per sample, applied to a batch of equally sized sources in at most four
    launches on the current stream, without a host synchronisation (the parameters travel in the launch arguments, so the
    call can be captured; a parameter tensor on the device is refused, reading it would synchronise).
    image1, image2 [B,Hs,Ws,3] interleaved RGB, uint8 or fp32 in [0, 1]; flow [B,Hs,Ws,2]; valid [B,Hs,Ws] or None (ones).
    -> dict: original_img (2 x [B,3,Hf,Wf], [0, 255], no photometric change), augmented_img (2 x [B,3,h,w], [0, 255]), flows
    [B,2,h,w], valids [B,1,h,w], original_flows [B,2,Hf,Wf], original_valids [B,1,Hf,Wf], crop_x / crop_y (lists of ints)."""
    if isinstance(params, torch.Tensor) or any(isinstance(p, torch.Tensor) for p in params):
        raise RuntimeError("the augmentation parameters are read on the host (they are checked before any launch): pass AugParams")
    params = list(params)
    if not params:
        raise ValueError("apply: one AugParams per sample")
    first = params[0]
    for p in params:
        if (p.src_hw, p.full_hw, p.crop_hw) != (first.src_hw, first.full_hw, first.crop_hw):
            raise ValueError(f"all sources of a batch have equal size: {(p.src_hw, p.full_hw, p.crop_hw)} and "
                             f"{(first.src_hw, first.full_hw, first.crop_hw)}")
    if isinstance(image1, torch.Tensor) and image1.dim() == 4 and tuple(image1.shape[1:3]) != tuple(first.src_hw):
        raise ValueError(f"parameters drawn for a {first.src_hw} source, images {tuple(image1.shape)}")
    f1, f2, fflow, fvalid, c1, c2, cflow, cvalid = ops.augment(image1, image2, flow, valid, pack_params(params), first.full_hw,
                                                                first.crop_hw)
    return dict(original_img=(f1, f2), augmented_img=(c1, c2), flows=cflow, valids=cvalid, original_flows=fflow,
                original_valids=fvalid, crop_x=[p.crop_x for p in params], crop_y=[p.crop_y for p in params])


@L.on_tensor_device
def apply_supervised(image1, image2, flow, valid, params, dense):
    """Already-drawn parameters of FlowAugmentor (dense True) or SparseFlowAugmentor (dense False), one AugParams per sample,
    applied to a batch of equally sized sources in at most five launches on the current stream, without a host synchronisation
    (as `apply`: captured calls keep their parameters, a parameter tensor is refused).  The resized size (t_h, t_w) = full_hw
    may differ between the samples.  Sources as for `apply`; dense ignores valid.
    -> dict: image1, image2 [B,3,h,w] in [0, 255] after colour, eraser, resize, flips and crop; flow [B,2,h,w]; valid [B,1,h,w]
    (dense: ones)."""
    if isinstance(params, torch.Tensor) or any(isinstance(p, torch.Tensor) for p in params):
        raise RuntimeError("the augmentation parameters are read on the host (they are checked before any launch): pass AugParams")
    params = list(params)
    if not params:
        raise ValueError("apply_supervised: one AugParams per sample")
    first = params[0]
    for p in params:
        if (p.src_hw, p.crop_hw) != (first.src_hw, first.crop_hw):
            raise ValueError(f"all sources and crops of a batch have equal size: {(p.src_hw, p.crop_hw)} and "
                             f"{(first.src_hw, first.crop_hw)}")
    if isinstance(image1, torch.Tensor) and image1.dim() == 4 and tuple(image1.shape[1:3]) != tuple(first.src_hw):
        raise ValueError(f"parameters drawn for a {first.src_hw} source, images {tuple(image1.shape)}")
    c1, c2, cflow, cvalid = ops.augment_sup(image1, image2, flow, valid, pack_params(params), first.crop_hw,
                                            "bilinear" if dense else "nearest")
    return dict(image1=c1, image2=c2, flow=cflow, valid=cvalid)


def as_step_input(out):
    """apply()'s dict (or the two dicts of UnsupAugmentor.__call__) -> (image1, image2, ci1, ci2, ox, oy, flow, valid), what
    train.SemiTrainStep takes for a sample: the crop pair, the uncropped pair, the crop's offsets, the crop's flow and valid."""
    if isinstance(out, (tuple, list)):
        out = {**out[0], **out[1]}
    im1, im2 = out["augmented_img"]
    ci1, ci2 = out["original_img"]
    return im1, im2, ci1, ci2, out["crop_x"], out["crop_y"], out["flows"], out["valids"][:, 0]


def add_noise(images, stdv, generator=None):
    """pytorch/train.py:263-268: clamp(x + stdv * randn, 0, 255) of every image, with torch's device generator."""
    return tuple((x + stdv * torch.randn(x.shape, device=x.device, dtype=x.dtype, generator=generator)).clamp(0.0, 255.0)
                 for x in images)
