"""CPU-only checks of the augmentation's host side (flow_supervisor_amd/augment.py, csrc/augment.hip): the parameter sampler
restates the reference's UnsupAugmentor (pytorch/raft_utils/augmentor.py:496-657) with its quirks, every refusal of the C
entry points is host code and comes back as FS_ERR_ARG (1) without a HIP call, and the Python surface refuses what it cannot
run."""
import ctypes
import math

import pytest
import torch

FS_ERR_ARG = 1
U8, F32 = 0, 1
null, p, odd = ctypes.c_void_p(None), ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 2)
BIG = 1 << 16                         # BIG * BIG is beyond 2^31 - 1
SRC, FULL, CROP = (436, 1024), (432, 1024), (368, 768)
N = 4000


def lib():
    from flow_supervisor_amd import _lib
    return _lib.load()


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------- the sampler
def test_constructor_has_the_references_defaults():
    from flow_supervisor_amd.augment import UnsupAugmentor
    a = UnsupAugmentor((368, 768))
    assert a.crop_size == (368, 768) and a.min_scale == 1.0 and a.max_scale == 0.5 and a.do_flip is False and a.full_size is None
    assert (a.spatial_aug_prob, a.stretch_prob, a.max_stretch, a.h_flip_prob, a.v_flip_prob) == (0.8, 0.8, 0.2, 0.5, 0.1)
    assert (a.photo_aug.brightness, a.photo_aug.contrast, a.photo_aug.saturation, a.photo_aug.hue) == (0.3, 0.3, 0.3, 0.3 / 3.14)
    assert a.asymmetric_color_aug_prob == 0.2 and a.eraser_aug_prob == 0.5 and a.eraser_bounds == (50, 100)
    # the min_scale argument is overridden (augmentor.py:499)
    assert UnsupAugmentor((8, 8), min_scale=-0.7, max_scale=0.1, do_flip=True, eraser_aug_prob=0.2, full_size=(16, 24)).min_scale == 1.0


def test_sampler_is_deterministic_under_a_seed():
    from flow_supervisor_amd.augment import AugParams, UnsupAugmentor
    a = UnsupAugmentor(CROP, do_flip=True)
    g1, g2 = gen(5), gen(5)
    first, again = [a.sample(SRC, g1) for _ in range(20)], [a.sample(SRC, g2) for _ in range(20)]
    assert first == again and len(set(map(repr, first))) == 20
    assert [a.sample(SRC, gen(6)) for _ in range(1)] != first[:1]
    q = first[0]
    assert isinstance(q, AugParams)
    for v in (q.t_h, q.win_y, q.crop_x):
        assert type(v) is int
    for v in (q.scale_x, q.scale_y) + q.colour[0] + q.colour[1]:
        assert type(v) is float
    for v in (q.resize, q.hflip, q.vflip, q.asymmetric):
        assert type(v) is bool


def within(count, n, prob):
    return abs(count / n - prob) <= 5.0 * math.sqrt(prob * (1.0 - prob) / n)


@pytest.mark.parametrize("prob", [0.5, 0.15])
def test_sampler_draws_the_references_distributions(prob):
    from flow_supervisor_amd.augment import UnsupAugmentor
    a = UnsupAugmentor(CROP, do_flip=True, eraser_aug_prob=prob)
    g = gen(100 + int(prob * 100))
    draws = [a.sample(SRC, g) for _ in range(N)]
    h, w = CROP
    for q in draws:
        assert q.src_hw == SRC and q.full_hw == FULL and q.crop_hw == CROP
        assert q.t_h >= FULL[0] and q.t_w >= FULL[1]
        assert 0 <= q.win_y <= q.t_h - FULL[0] and 0 <= q.win_x <= q.t_w - FULL[1]
        assert q.crop_y % 8 == 0 and q.crop_x % 8 == 0 and 0 <= q.crop_y <= FULL[0] - h and 0 <= q.crop_x <= FULL[1] - w
        if q.resize:
            # scale = 2^(1 + (max_scale - 1) u) in (2^0.5, 2], stretched by at most 2^0.2 (one more pixel for the rounding)
            for t, n, s in ((q.t_h, SRC[0], q.scale_y), (q.t_w, SRC[1], q.scale_x)):
                assert 2 ** 0.3 * n - 1 <= t <= 2 ** 1.2 * n + 1 and s == float(torch.tensor(t, dtype=torch.float32) / n)
        else:
            assert (q.t_h, q.t_w, q.scale_x, q.scale_y) == (*SRC, 1.0, 1.0)
        for quad in q.colour:
            assert all(0.7 <= v <= 1.3 for v in quad[:3]) and abs(quad[3]) <= 0.3 / 3.14
        assert q.asymmetric or q.colour[0] == q.colour[1]
        assert len(q.rects) <= 2
        for x0, y0, dx, dy in q.rects:
            assert 0 <= x0 < w and 0 <= y0 < h and x0 + dx <= w and y0 + dy <= h
            assert min(50, w - x0) <= dx <= 100 and min(50, h - y0) <= dy <= 100
    assert within(sum(q.resize for q in draws), N, 0.8)
    assert within(sum(q.stretched for q in draws), N, 0.8)
    assert within(sum(q.hflip for q in draws), N, 0.5)
    assert within(sum(q.vflip for q in draws), N, 0.1)
    assert within(sum(q.asymmetric for q in draws), N, 0.2)
    assert within(sum(bool(q.rects) for q in draws), N, prob)
    erased = [q for q in draws if q.rects]
    assert within(sum(len(q.rects) == 2 for q in erased), len(erased), 0.5)
    # an unstretched sample has one scale for both axes, up to the rounding of the sizes
    for q in draws:
        if q.resize and not q.stretched:
            assert abs(q.scale_x - q.scale_y) <= 0.5 / SRC[0] + 0.5 / SRC[1] + 1e-6


def test_flips_never_occur_without_do_flip():
    from flow_supervisor_amd.augment import UnsupAugmentor
    a, g = UnsupAugmentor(CROP), gen(9)
    assert not any(q.hflip or q.vflip for q in (a.sample(SRC, g) for _ in range(N // 4)))


def test_full_size_is_the_floor_to_eight_capped_by_the_argument():
    from flow_supervisor_amd.augment import UnsupAugmentor
    assert UnsupAugmentor((16, 24)).sample((37, 53), gen(1)).full_hw == (32, 48)
    assert UnsupAugmentor((16, 24), full_size=(24, 200)).sample((37, 53), gen(1)).full_hw == (24, 48)
    assert UnsupAugmentor((16, 24), full_size=(400, 40)).sample((37, 53), gen(1)).full_hw == (32, 40)


def test_a_crop_under_the_erasers_bounds_takes_the_lower_bound():
    """Where lo >= hi (the rectangle reaches the edge, or the crop is under 100 pixels) the size is lo = the rest of the crop."""
    from flow_supervisor_amd.augment import UnsupAugmentor
    a, g = UnsupAugmentor((16, 24), eraser_aug_prob=1.0), gen(2)
    rects = [r for _ in range(200) for r in a.sample((37, 53), g).rects]
    assert len(rects) >= 200
    for x0, y0, dx, dy in rects:
        assert dx == 24 - x0 and dy == 16 - y0 and dx >= 1 and dy >= 1


def test_rounding_is_half_to_even_in_float32():
    from flow_supervisor_amd.augment import resized_size
    assert resized_size(4, 0.625) == (2, 0.5) and resized_size(4, 0.875) == (4, 1.0) and resized_size(4, 1.125) == (4, 1.0)
    assert resized_size(4, 1.375) == (6, 1.5)
    # 0.5 + 2^-27 is 0.5 in float32: 5 * 0.5 is the tie 2.5 and goes to 2; in double the product is above the tie and goes to 3
    scale = 0.5 + 2.0 ** -27
    assert round(5 * scale) == 3 and resized_size(5, scale)[0] == 2
    # the scale is re-derived in float32
    t, s = resized_size(436, 1.7)
    assert t == 741 and s == float(torch.tensor(741.0) / torch.tensor(436.0)) and s != 741 / 436


def test_sampler_raises_where_tensorflow_would_die():
    from flow_supervisor_amd.augment import UnsupAugmentor
    with pytest.raises(ValueError, match=r"32 x 48.*crop_size 40 x 24"):
        UnsupAugmentor((40, 24)).sample((37, 53), gen(0))
    with pytest.raises(ValueError, match=r"16 x 48.*crop_size 24 x 24"):
        UnsupAugmentor((24, 24), full_size=(16, 64)).sample((37, 53), gen(0))
    # max_scale far below zero: 2^(1 + (max_scale - 1) u) shrinks the frame under full_size whenever the spatial branch is taken
    a = UnsupAugmentor((16, 24), max_scale=-60.0)
    raised = 0
    for seed in range(40):
        try:
            q = a.sample((37, 53), gen(seed))
            assert not q.resize or (q.t_h >= 32 and q.t_w >= 48)         # (a u next to 0 leaves a scale above 1)
        except ValueError as e:
            raised += 1
            assert "resized frame" in str(e) and "full_size 32 x 48" in str(e)
    assert 20 <= raised < 40


# ------------------------------------------------------------------------------------------------------ the C entry points
def test_scratch_sizes():
    size = lib().fsraft_augment_scratch_bytes
    for bad in ((0, 8, 8, 8, 8), (1, 0, 8, 8, 8), (1, 8, -1, 8, 8), (1, 8, 8, 0, 8), (1, 8, 8, 8, 0), (1, 8, 8, 9, 8), (1, 8, 8, 8, 9),
                (1, BIG, BIG, 8, 8)):
        assert size(*bad) == FS_ERR_ARG, bad
    # per sample: 6 doubles per block of 256 frame pixels, 8 for the means, 3 per block of 256 crop pixels; rounded up to 64 bytes
    assert size(1, 1, 1, 1, 1) == (6 + 8 + 3) * 8 // 64 * 64 + 64
    assert size(3, 32, 48, 16, 24) == (3 * (6 * 6 + 8 + 2 * 3) * 8 + 63) // 64 * 64
    assert size(2, 432, 1024, 368, 768) == 2 * (1728 * 6 + 8 + 1104 * 3) * 8
    # the grids stop at 2048 blocks per sample
    cap = (2048 * 6 + 8 + 2048 * 3) * 8
    assert size(1, 736, 736, 728, 728) == size(1, 1024, 1024, 1024, 512) == size(1, 2000, 2000, 1500, 1500) == cap


def params_array(*changes, n=2):
    from flow_supervisor_amd.augment import identity_params, pack_params
    return pack_params([identity_params((37, 53), (32, 48), (16, 24), **(changes[i] if i < len(changes) else {})) for i in range(n)])


def test_entry_point_rejects_bad_arguments_before_touching_the_gpu():
    L = lib()
    B, Hs, Ws, Hf, Wf, h, w = 2, 37, 53, 32, 48, 16, 24
    need = L.fsraft_augment_scratch_bytes(B, Hf, Wf, h, w)
    ok = params_array()
    ptrs = ("image1", "image2", "flow", "valid", "frame1", "frame2", "frame_flow", "frame_valid", "crop1", "crop2", "crop_flow", "crop_valid",
            "scratch")

    def call(dtype=U8, B=B, Hs=Hs, Ws=Ws, params=ok, Hf=Hf, Wf=Wf, h=h, w=w, nbytes=need, **kw):
        a = {k: kw.get(k, p) for k in ptrs}
        return L.fsraft_augment(a["image1"], a["image2"], dtype, a["flow"], a["valid"], B, Hs, Ws, params, Hf, Wf, h, w, a["frame1"], a["frame2"],
                                a["frame_flow"], a["frame_valid"], a["crop1"], a["crop2"], a["crop_flow"], a["crop_valid"], a["scratch"],
                                nbytes, None)

    for k in ptrs:
        if k != "valid":                                                     # (a null valid map stands for ones)
            assert call(**{k: null}) == FS_ERR_ARG, k
        if k not in ("image1", "image2"):
            assert call(**{k: odd}) == FS_ERR_ARG, k
    assert call(params=None) == FS_ERR_ARG
    assert call(dtype=F32, image1=odd) == call(dtype=F32, image2=odd) == FS_ERR_ARG          # (uint8 images need no alignment)
    assert call(scratch=ctypes.c_void_p(4096 + 4)) == FS_ERR_ARG                             # fp64 partial sums
    assert call(dtype=-1) == call(dtype=2) == FS_ERR_ARG
    assert call(B=0) == call(Hs=0) == call(Ws=-3) == call(Hf=0) == call(Wf=0) == call(h=0) == call(w=0) == FS_ERR_ARG
    assert call(Hs=BIG, Ws=BIG) == call(Hf=BIG, Wf=BIG) == FS_ERR_ARG
    assert call(h=Hf + 1) == call(w=Wf + 1) == FS_ERR_ARG                                    # a crop larger than the frame
    assert call(nbytes=need - 1) == call(nbytes=0) == FS_ERR_ARG
    assert call(B=3, params=params_array(n=3)) == FS_ERR_ARG                                 # scratch sized for two samples
    resized = dict(resize=True, t_h=51, t_w=67)
    bad = (dict(t_h=38), dict(t_w=52),                                                       # no resize, yet another size
           dict(resize=True, t_h=31, t_w=67), dict(resize=True, t_h=51, t_w=47),             # resized under the frame
           dict(resize=True, t_h=BIG, t_w=BIG),
           dict(win_y=6), dict(win_x=6), dict(win_y=-1), dict(win_x=-1), dict(resized, win_y=20), dict(resized, win_x=20),
           dict(crop_y=17), dict(crop_x=25), dict(crop_y=-8), dict(crop_x=-8),
           dict(rects=((0, 0, 25, 1),)), dict(rects=((0, 0, 1, 17),)), dict(rects=((20, 0, 5, 1),)), dict(rects=((0, 10, 1, 7),)),
           dict(rects=((-1, 0, 1, 1),)), dict(rects=((0, -1, 1, 1),)), dict(rects=((0, 0, -1, 1),)), dict(rects=((0, 0, 1, -1),)),
           dict(rects=((0, 0, 1, 1), (24, 16, 1, 1))),
           dict(scale_x=float("nan")), dict(scale_y=float("inf")),
           dict(colour=((1.1, 1.0, 1.0, 0.0), (1.0, 1.0, 1.0, 0.0))), dict(colour=((1.0, 1.0, 1.0, 0.0), (1.0, 1.0, 1.0, 0.01))),   # symmetric, yet two quadruples
           dict(colour=((float("nan"), 1.0, 1.0, 0.0), (1.0, 1.0, 1.0, 0.0))), dict(colour=((1.0, 1.0, 1.0, 0.0), (1.0, 1.0, 1.0, float("inf")))))
    for change in bad:
        assert call(params=params_array({}, change)) == FS_ERR_ARG, change
    for field, value in (("resize", 2), ("hflip", 2), ("vflip", -1), ("asym", 3), ("nrect", 3), ("nrect", -1)):
        arr = params_array()
        setattr(arr[1], field, value)
        assert call(params=arr) == FS_ERR_ARG, field


def test_params_mirror_matches_the_header():
    import os
    import re
    from flow_supervisor_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "fsraft.h")).read()
    body = txt[txt.index("typedef struct fsraft_aug_params {"):txt.index("} fsraft_aug_params;")].split("{", 1)[1]
    fields = [re.sub(r"\[\d+\]", "", part.split()[-1]) for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert fields == [f[0] for f in _lib.AugParams._fields_]
    assert ctypes.sizeof(_lib.AugParams) == 29 * 4


# ------------------------------------------------------------------------------------------------------ the Python surface
def test_cpu_tensors_are_refused():
    from flow_supervisor_amd import augment as A
    img, flow, valid = torch.zeros(1, 37, 53, 3, dtype=torch.uint8), torch.zeros(1, 37, 53, 2), torch.ones(1, 37, 53)
    q = A.identity_params((37, 53), (32, 48), (16, 24))
    for call in (lambda: A.apply(img, img, flow, valid, [q]), lambda: A.apply(img.float(), img.float(), flow, None, [q]),
                 lambda: A.UnsupAugmentor((16, 24))(img, img, flow, valid, generator=gen(0))):
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            call()


def test_apply_checks_its_parameters():
    from flow_supervisor_amd import augment as A
    img, flow = torch.zeros(2, 37, 53, 3, dtype=torch.uint8), torch.zeros(2, 37, 53, 2)
    q = A.identity_params((37, 53), (32, 48), (16, 24))
    with pytest.raises(RuntimeError, match="read on the host"):
        A.apply(img, img, flow, None, torch.zeros(2, 29))
    with pytest.raises(ValueError, match="equal size"):
        A.apply(img, img, flow, None, [q, A.identity_params((37, 53), (32, 48), (8, 24))])
    with pytest.raises(ValueError, match="drawn for"):
        A.apply(img, img, flow, None, [A.identity_params((45, 53), (32, 48), (16, 24))] * 2)
    with pytest.raises(ValueError, match="two eraser rectangles"):
        A.pack_params([A.identity_params((37, 53), (32, 48), (16, 24), rects=((0, 0, 1, 1),) * 3)])
    with pytest.raises(ValueError, match="one AugParams per sample"):
        A.apply(img, img, flow, None, [])


def test_as_step_input_is_in_the_train_steps_order():
    from flow_supervisor_amd import augment as A
    t = {k: torch.full((2, c, 2, 2), float(i)) for i, (k, c) in enumerate((("a1", 3), ("a2", 3), ("o1", 3), ("o2", 3), ("f", 2), ("v", 1)))}
    out = dict(augmented_img=(t["a1"], t["a2"]), original_img=(t["o1"], t["o2"]), flows=t["f"], valids=t["v"], original_flows=None,
               original_valids=None, crop_x=[8, 16], crop_y=[0, 24])
    for arg in (out, ({k: out[k] for k in ("augmented_img", "original_img", "crop_x", "crop_y")},
                      {k: out[k] for k in ("flows", "original_flows", "valids", "original_valids")})):
        step = A.as_step_input(arg)
        assert len(step) == 8
        im1, im2, ci1, ci2, ox, oy, flow, valid = step
        assert im1 is t["a1"] and im2 is t["a2"] and ci1 is t["o1"] and ci2 is t["o2"] and flow is t["f"]
        assert ox == [8, 16] and oy == [0, 24] and valid.shape == (2, 2, 2) and torch.equal(valid, t["v"][:, 0])
