"""CPU-only checks of the supervised augmentors' host side (flow_supervisor_amd/augment.py, csrc/augment.hip): the samplers
restate the reference's FlowAugmentor and SparseFlowAugmentor (pytorch/raft_utils/augmentor.py:39-188, :191-330) with their
order of draws and their quirks, every refusal of the C entry points is host code and comes back as FS_ERR_ARG (1) without a
HIP call, and the Python surface refuses what it cannot run."""
import ctypes
import math

import numpy as np
import pytest
import torch

FS_ERR_ARG = 1
U8, F32 = 0, 1
BILINEAR, NEAREST = 0, 1
null, p, odd = ctypes.c_void_p(None), ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 2)
BIG = 1 << 16                         # BIG * BIG is beyond 2^31 - 1
SRC, CROP = (436, 1024), (256, 512)          # (every scale the samplers draw, down to 2^-0.4, leaves room for the crop)
N = 4000


def lib():
    from flow_supervisor_amd import _lib
    return _lib.load()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def classes():
    from flow_supervisor_amd.augment import FlowAugmentor, SparseFlowAugmentor
    return FlowAugmentor, SparseFlowAugmentor


# ------------------------------------------------------------------------------------------------------------ the samplers
def test_constructors_have_the_references_defaults():
    Dense, Sparse = classes()
    a, s = Dense((368, 496)), Sparse((288, 960))
    assert a.crop_size == (368, 496) and a.min_scale == -0.2 and a.max_scale == 0.5 and a.do_flip is True and a.dense is True
    assert s.crop_size == (288, 960) and s.min_scale == -0.2 and s.max_scale == 0.5 and s.do_flip is False and s.dense is False
    for x in (a, s):
        assert (x.spatial_aug_prob, x.stretch_prob, x.max_stretch, x.h_flip_prob, x.v_flip_prob) == (0.8, 0.8, 0.2, 0.5, 0.1)
        assert x.asymmetric_color_aug_prob == 0.2 and x.eraser_aug_prob == 0.5 and x.eraser_bounds == (50, 100)
    assert (a.photo_aug.brightness, a.photo_aug.contrast, a.photo_aug.saturation, a.photo_aug.hue) == (0.4, 0.4, 0.4, 0.5 / 3.14)
    assert (s.photo_aug.brightness, s.photo_aug.contrast, s.photo_aug.saturation, s.photo_aug.hue) == (0.3, 0.3, 0.3, 0.3 / 3.14)
    # min_scale as given: the `= 1.` override is UnsupAugmentor's alone
    b = Dense((8, 8), min_scale=-0.7, max_scale=0.1, do_flip=False, eraser_aug_prob=0.2)
    assert (b.min_scale, b.max_scale, b.do_flip, b.eraser_aug_prob) == (-0.7, 0.1, False, 0.2)
    assert Sparse((8, 8), min_scale=0.3).min_scale == 0.3


@pytest.mark.parametrize("which", [0, 1])
def test_sampler_is_deterministic_under_a_seed(which):
    from flow_supervisor_amd.augment import AugParams
    a = classes()[which](CROP, do_flip=True)
    g1, g2 = gen(5), gen(5)
    first, again = [a.sample(SRC, g1) for _ in range(20)], [a.sample(SRC, g2) for _ in range(20)]
    assert first == again and len(set(map(repr, first))) == 20
    assert [a.sample(SRC, gen(6))] != first[:1]
    q = first[0]
    assert isinstance(q, AugParams) and q.win_y == 0 and q.win_x == 0 and q.full_hw == (q.t_h, q.t_w)
    for v in (q.t_h, q.t_w, q.crop_y, q.crop_x):
        assert type(v) is int
    for v in (q.scale_x, q.scale_y) + q.colour[0] + q.colour[1]:
        assert type(v) is float
    for v in (q.resize, q.hflip, q.vflip, q.asymmetric):
        assert type(v) is bool


@pytest.mark.parametrize("which", [0, 1])
def test_colour_and_eraser_are_drawn_before_the_spatial_parameters(which):
    """The reference's __call__ is colour, eraser, spatial (:183-188, :325-330): two augmentors that differ only in crop_size agree
    in colour and rectangles under one seed (the eraser's bounds come from the source), and differ in the crop's offset."""
    cls = classes()[which]
    a, b = cls(CROP, do_flip=True, eraser_aug_prob=1.0), cls((64, 96), do_flip=True, eraser_aug_prob=1.0)
    differ = 0
    for seed in range(30):
        qa, qb = a.sample(SRC, gen(seed)), b.sample(SRC, gen(seed))
        assert (qa.asymmetric, qa.colour, qa.rects) == (qb.asymmetric, qb.colour, qb.rects) and qa.rects
        # the scale and flip draws follow and are the same too; only the offsets depend on the crop
        assert (qa.resize, qa.t_h, qa.t_w, qa.hflip, qa.vflip) == (qb.resize, qb.t_h, qb.t_w, qb.hflip, qb.vflip)
        differ += (qa.crop_y, qa.crop_x) != (qb.crop_y, qb.crop_x)
    assert differ >= 25
    # and the colour quadruple is the very first thing drawn after the asymmetry draw (dense) or at once (sparse)
    from flow_supervisor_amd.augment import _uniform
    g = gen(3)
    if which == 0:
        assert (float(_uniform(g)) < 0.2) == a.sample(SRC, gen(3)).asymmetric
    lo, hi = (0.6, 1.4) if which == 0 else (0.7, 1.3)
    assert a.sample(SRC, gen(3)).colour[0][0] == float(_uniform(g, lo, hi))


def within(count, n, prob):
    return abs(count / n - prob) <= 5.0 * math.sqrt(prob * (1.0 - prob) / n)


@pytest.mark.parametrize("which,prob", [(0, 0.5), (1, 0.15)])
def test_sampler_draws_the_references_distributions(which, prob):
    a = classes()[which](CROP, do_flip=True, eraser_aug_prob=prob)
    g = gen(100 + int(prob * 100))
    draws = [a.sample(SRC, g) for _ in range(N)]
    h, w = CROP
    jitter, hue = (0.4, 0.5 / 3.14) if which == 0 else (0.3, 0.3 / 3.14)
    for q in draws:
        assert q.src_hw == SRC and q.crop_hw == CROP and q.full_hw == (q.t_h, q.t_w) and (q.win_y, q.win_x) == (0, 0)
        # the offset's upper end is excluded (:170-171)
        assert 0 <= q.crop_y < q.t_h - h and 0 <= q.crop_x < q.t_w - w
        if q.resize:
            # scale = 2^u, u in [-0.2, 0.5), stretched by at most 2^0.2 (one more pixel for the rounding)
            for t, n, s in ((q.t_h, SRC[0], q.scale_y), (q.t_w, SRC[1], q.scale_x)):
                assert 2 ** -0.4 * n - 1 <= t <= 2 ** 0.7 * n + 1 and s == float(np.float32(t) / np.float32(n))
        else:
            assert (q.t_h, q.t_w, q.scale_x, q.scale_y) == (*SRC, 1.0, 1.0)
        for quad in q.colour:
            assert all(1 - jitter - 1e-6 <= v <= 1 + jitter + 1e-6 for v in quad[:3]) and abs(quad[3]) <= hue
        assert q.asymmetric or q.colour[0] == q.colour[1]
        assert len(q.rects) <= 2
        for x0, y0, dx, dy in q.rects:                                         # bounds from the SOURCE
            assert 0 <= x0 < SRC[1] and 0 <= y0 < SRC[0] and x0 + dx <= SRC[1] and y0 + dy <= SRC[0]
            assert min(50, SRC[1] - x0) <= dx <= 100 and min(50, SRC[0] - y0) <= dy <= 100
    assert within(sum(q.resize for q in draws), N, 0.8)
    assert within(sum(q.stretched for q in draws), N, 0.8)
    assert within(sum(q.hflip for q in draws), N, 0.5)
    assert within(sum(q.vflip for q in draws), N, 0.1)
    if which == 0:
        assert within(sum(q.asymmetric for q in draws), N, 0.2)
    else:
        assert not any(q.asymmetric for q in draws)                            # never asymmetric (:214-222)
    assert within(sum(bool(q.rects) for q in draws), N, prob)
    erased = [q for q in draws if q.rects]
    assert within(sum(len(q.rects) == 2 for q in erased), len(erased), 0.5)
    # rectangles reach beyond the crop's size: they live on the source
    assert any(x0 + dx > w or y0 + dy > h for q in erased for x0, y0, dx, dy in q.rects)
    for q in draws:
        if q.resize and not q.stretched:
            assert abs(q.scale_x - q.scale_y) <= 0.5 / SRC[0] + 0.5 / SRC[1] + 1e-6


def test_the_sparse_class_spends_no_draw_on_asymmetry():
    """SparseFlowAugmentor.color_transform (:214-222) has no asymmetric branch and no draw for it: its first draw is the
    brightness, where the dense class's first draw decides the asymmetry."""
    from flow_supervisor_amd.augment import _uniform
    Dense, Sparse = classes()
    q = Sparse(CROP).sample(SRC, gen(8))
    g = gen(8)
    assert q.colour[0][0] == float(_uniform(g, 0.7, 1.3)) and q.asymmetric is False
    d = Dense(CROP).sample(SRC, gen(8))
    g = gen(8)
    _uniform(g)
    assert d.colour[0][0] == float(_uniform(g, 0.6, 1.4))


@pytest.mark.parametrize("which", [0, 1])
def test_flips_never_occur_without_do_flip(which):
    a, g = classes()[which](CROP, do_flip=False), gen(9)
    assert not any(q.hflip or q.vflip for q in (a.sample(SRC, g) for _ in range(N // 4)))
    # and they cost no draw: the offsets follow the spatial draw directly
    b = classes()[which](CROP, do_flip=True)
    same = [(a.sample(SRC, gen(s)), b.sample(SRC, gen(s))) for s in range(20)]
    assert all((x.t_h, x.t_w, x.colour, x.rects) == (y.t_h, y.t_w, y.colour, y.rects) for x, y in same)
    assert any((x.crop_y, x.crop_x) != (y.crop_y, y.crop_x) for x, y in same)


def test_a_small_source_takes_the_dense_fallback_with_min_scale_itself():
    """augmentor.py:145-154: without the spatial draw, a source under crop + 8 is resized by min_scale = max((ch + 8) / ht,
    (cw + 8) / wd) in float32, t = rint(n * min_scale), and the flow is multiplied by min_scale, not by t / n.  FlowAugmentor
    alone: SparseFlowAugmentor has no such branch."""
    Dense, Sparse = classes()
    min_scale = max(np.float32(24.0) / np.float32(21), np.float32(32.0) / np.float32(29))
    a = Dense((16, 24))
    a.spatial_aug_prob = 0.0
    for seed in range(10):
        q = a.sample((21, 29), gen(seed))
        assert q.resize and (q.t_h, q.t_w) == (24, 33) and q.full_hw == (24, 33)
        assert q.scale_x == q.scale_y == float(min_scale) and q.scale_x != float(np.float32(33) / np.float32(29))
        assert 0 <= q.crop_y < 8 and 0 <= q.crop_x < 9
    # a source of crop + 8 or more is left alone
    q = a.sample((37, 53), gen(0))
    assert not q.resize and (q.t_h, q.t_w, q.scale_x, q.scale_y) == (37, 53, 1.0, 1.0)
    s = Sparse((16, 24))
    s.spatial_aug_prob = 0.0
    q = s.sample((21, 29), gen(0))
    assert not q.resize and (q.t_h, q.t_w) == (21, 29)
    # with the spatial draw the scale is re-derived from the rounded size (:137-138)
    a.spatial_aug_prob = 1.0
    q = a.sample((37, 53), gen(1))
    assert q.resize and q.scale_y == float(np.float32(q.t_h) / np.float32(37)) and q.scale_x == float(np.float32(q.t_w) / np.float32(53))


@pytest.mark.parametrize("which", [0, 1])
def test_sampler_raises_where_the_offsets_range_is_empty(which):
    """y0 = uniform([], 0, ht - crop, int32) has an empty range where the resized image is not larger than the crop."""
    cls = classes()[which]
    a, b = cls((37, 24)), cls((16, 53))
    a.spatial_aug_prob = b.spatial_aug_prob = 0.0
    if which == 1:
        with pytest.raises(ValueError, match=r"37 x 53 \(source 37 x 53\).*crop_size 37 x 24"):
            a.sample((37, 53), gen(0))
        with pytest.raises(ValueError, match=r"crop_size 16 x 53"):
            b.sample((37, 53), gen(0))
    else:
        # (the dense class's fallback makes room: min_scale = 45 / 37 and 61 / 53)
        assert a.sample((37, 53), gen(0)).full_hw == (45, 64) and b.sample((37, 53), gen(0)).full_hw == (43, 61)
    # max_scale far below zero shrinks the image under the crop whenever the spatial branch is taken
    c = cls((16, 24), min_scale=-60.0, max_scale=-50.0)
    c.spatial_aug_prob = 1.0
    with pytest.raises(ValueError, match=r"resized image 0 x 0"):
        c.sample((37, 53), gen(0))


def test_eraser_bounds_come_from_the_source():
    """Where lo >= hi (the rectangle reaches the source's edge, or the source is under 100 pixels) the size is lo."""
    Dense, _ = classes()
    a, g = Dense((16, 24), eraser_aug_prob=1.0), gen(2)
    rects = [r for _ in range(200) for r in a.sample((37, 53), g).rects]
    assert len(rects) >= 200
    for x0, y0, dx, dy in rects:
        assert min(50, 53 - x0) <= dx <= 53 - x0 and dy == 37 - y0 and dx >= 1 and dy >= 1
    assert any(x0 >= 24 or y0 >= 16 for x0, y0, _, _ in rects)               # beyond the crop's size


# ------------------------------------------------------------------------------------------------------ the C entry points
def test_scratch_sizes():
    size = lib().fsraft_augment_sup_scratch_bytes
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, -1), (1, BIG, BIG)):
        assert size(*bad) == FS_ERR_ARG, bad
    # per sample: 6 + 3 doubles per block of 256 source pixels and 12 for the means; rounded up to 64 bytes
    assert size(1, 1, 1) == (9 + 12) * 8 // 64 * 64 + 64
    assert size(3, 37, 53) == (3 * (8 * 9 + 12) * 8 + 63) // 64 * 64
    assert size(2, 53, 85) == (2 * (18 * 9 + 12) * 8 + 63) // 64 * 64
    assert size(8, 384, 512) == 8 * (768 * 9 + 12) * 8
    # the grids stop at 2048 blocks per sample
    cap = ((2048 * 9 + 12) * 8 + 63) // 64 * 64
    assert size(1, 739, 741) == size(1, 1024, 512) == size(1, 2000, 2000) == cap


def params_array(*changes, n=2):
    from flow_supervisor_amd.augment import identity_params, pack_params
    return pack_params([identity_params((37, 53), (37, 53), (16, 24), **(changes[i] if i < len(changes) else {})) for i in range(n)])


def test_entry_point_rejects_bad_arguments_before_touching_the_gpu():
    L = lib()
    B, Hs, Ws, h, w = 2, 37, 53, 16, 24
    need = L.fsraft_augment_sup_scratch_bytes(B, Hs, Ws)
    ok = params_array()
    ptrs = ("image1", "image2", "flow", "valid", "crop1", "crop2", "crop_flow", "crop_valid", "scratch")

    def call(dtype=U8, mode=BILINEAR, B=B, Hs=Hs, Ws=Ws, params=ok, h=h, w=w, nbytes=need, **kw):
        a = {k: kw.get(k, p) for k in ptrs}
        return L.fsraft_augment_sup(a["image1"], a["image2"], dtype, a["flow"], a["valid"], mode, B, Hs, Ws, params, h, w, a["crop1"],
                                    a["crop2"], a["crop_flow"], a["crop_valid"], a["scratch"], nbytes, None)

    for k in ptrs:
        if k != "valid":                                                     # (a null valid map stands for ones)
            assert call(**{k: null}) == FS_ERR_ARG, k
        if k not in ("image1", "image2"):
            assert call(**{k: odd}) == FS_ERR_ARG, k
    assert call(params=None) == FS_ERR_ARG
    assert call(dtype=F32, image1=odd) == call(dtype=F32, image2=odd) == FS_ERR_ARG          # (uint8 images need no alignment)
    assert call(scratch=ctypes.c_void_p(4096 + 4)) == FS_ERR_ARG                             # fp64 partial sums
    assert call(dtype=-1) == call(dtype=2) == FS_ERR_ARG
    assert call(mode=-1) == call(mode=2) == FS_ERR_ARG                                       # an unknown flow_mode
    assert call(B=0) == call(Hs=0) == call(Ws=-3) == call(h=0) == call(w=0) == FS_ERR_ARG
    assert call(Hs=BIG, Ws=BIG) == FS_ERR_ARG
    assert call(h=Hs + 1) == call(w=Ws + 1) == FS_ERR_ARG                                    # th < h, tw < w
    assert call(nbytes=need - 1) == call(nbytes=0) == FS_ERR_ARG
    assert call(B=3, params=params_array(n=3)) == FS_ERR_ARG                                 # scratch sized for two samples
    resized = dict(resize=True, t_h=51, t_w=67)
    bad = (dict(t_h=38), dict(t_w=52),                                                       # no resize, yet another size
           dict(resize=True, t_h=15, t_w=67), dict(resize=True, t_h=51, t_w=23),             # resized under the crop
           dict(resize=True, t_h=BIG, t_w=BIG),
           dict(win_y=1), dict(win_x=1), dict(win_y=-1), dict(resized, win_y=8), dict(resized, win_x=8),       # there is no window
           dict(crop_y=22), dict(crop_x=30), dict(crop_y=-1), dict(crop_x=-1), dict(resized, crop_y=36), dict(resized, crop_x=44),
           dict(rects=((0, 0, 54, 1),)), dict(rects=((0, 0, 1, 38),)), dict(rects=((50, 0, 4, 1),)), dict(rects=((0, 30, 1, 8),)),
           dict(rects=((-1, 0, 1, 1),)), dict(rects=((0, -1, 1, 1),)), dict(rects=((0, 0, -1, 1),)), dict(rects=((0, 0, 1, -1),)),
           dict(rects=((0, 0, 1, 1), (53, 37, 1, 1))),
           dict(resized, rects=((0, 0, 60, 1),)),                                            # inside the resized image, outside the source
           dict(scale_x=float("nan")), dict(scale_y=float("inf")),
           dict(colour=((1.1, 1.0, 1.0, 0.0), (1.0, 1.0, 1.0, 0.0))), dict(colour=((1.0, 1.0, 1.0, 0.0), (1.0, 1.0, 1.0, 0.01))),   # symmetric, yet two quadruples
           dict(colour=((float("nan"), 1.0, 1.0, 0.0), (1.0, 1.0, 1.0, 0.0))), dict(colour=((1.0, 1.0, 1.0, 0.0), (1.0, 1.0, 1.0, float("inf")))))
    for mode in (BILINEAR, NEAREST):
        for change in bad:
            assert call(mode=mode, params=params_array({}, change)) == FS_ERR_ARG, change
    for field, value in (("resize", 2), ("hflip", 2), ("vflip", -1), ("asym", 3), ("nrect", 3), ("nrect", -1)):
        arr = params_array()
        setattr(arr[1], field, value)
        assert call(params=arr) == FS_ERR_ARG, field


# ------------------------------------------------------------------------------------------------------ the Python surface
def test_cpu_tensors_are_refused():
    from flow_supervisor_amd import augment as A
    img, flow, valid = torch.zeros(1, 37, 53, 3, dtype=torch.uint8), torch.zeros(1, 37, 53, 2), torch.ones(1, 37, 53)
    q = A.identity_params((37, 53), (37, 53), (16, 24))
    for call in (lambda: A.apply_supervised(img, img, flow, valid, [q], True), lambda: A.apply_supervised(img.float(), img.float(), flow, None, [q], False),
                 lambda: A.FlowAugmentor((16, 24))(img, img, flow, generator=gen(0)),
                 lambda: A.SparseFlowAugmentor((16, 24))(img, img, flow, valid, generator=gen(0))):
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            call()


def test_apply_supervised_checks_its_parameters():
    from flow_supervisor_amd import augment as A
    img, flow = torch.zeros(2, 37, 53, 3, dtype=torch.uint8), torch.zeros(2, 37, 53, 2)
    q = A.identity_params((37, 53), (37, 53), (16, 24))
    with pytest.raises(RuntimeError, match="read on the host"):
        A.apply_supervised(img, img, flow, None, torch.zeros(2, 29), True)
    with pytest.raises(ValueError, match="equal size"):
        A.apply_supervised(img, img, flow, None, [q, A.identity_params((37, 53), (37, 53), (8, 24))], True)
    with pytest.raises(ValueError, match="drawn for"):
        A.apply_supervised(img, img, flow, None, [A.identity_params((45, 53), (45, 53), (16, 24))] * 2, False)
    with pytest.raises(ValueError, match="one AugParams per sample"):
        A.apply_supervised(img, img, flow, None, [], True)
    # different resized sizes in one batch are no error of the parameters: the refusal is the CPU tensors'
    r = A.identity_params((37, 53), (51, 67), (16, 24), resize=True, t_h=51, t_w=67)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        A.apply_supervised(img, img, flow, None, [q, r], True)
