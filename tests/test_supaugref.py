"""CPU-only checks that pin the restatement of the supervised augmentors (tests/_supaugref.py) independently of any kernel: its
identities and closed forms, that its order (colour, eraser, then resize) is the one that matters, and the input condition of
every GPU case.  The resizes and the colour functions it is made of are pinned in test_augref.py."""
import math

import pytest
import torch

import _supaugref as R

F64 = torch.float64


def one(kind, plist, mode="dense", holes=True, seed=21):
    return R.make_case("t", plist, holes, kind, mode, seed)


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("kind", R.DTYPES)
def test_identity_parameters_reproduce_the_source_window_times_255(kind, mode):
    case = one(kind, [R.params((37, 53), (16, 24), crop_y=5, crop_x=7)], mode)
    for dtype in (torch.float32, F64):
        out = R.evaluate(case, dtype)
        for k, src in (("crop1", case["image1"]), ("crop2", case["image2"])):
            window = src[0, 5:21, 7:31].permute(2, 0, 1).to(dtype)
            # the identity colour is the identity to rounding only (x / 255 * 255, two HSV trips)
            assert float((out[k][0] - (window if kind == "u8" else window * 255.0)).abs().max()) <= (1e-10 if dtype == F64 else 1e-3)
        assert torch.equal(out["crop_flow"][0], case["flow"][0, 5:21, 7:31].permute(2, 0, 1).to(dtype))
        want = torch.ones(16, 24, dtype=dtype) if mode == "dense" else case["valid"][0, 5:21, 7:31].to(dtype)
        assert torch.equal(out["crop_valid"][0, 0], want)


def test_a_constant_image_is_a_fixed_point():
    """Contrast about its own mean, a resize and an eraser that writes the mean leave a constant image as it is."""
    colour = torch.tensor([0.3125, 0.625, 0.15625])
    img = colour.expand(1, 37, 53, 3).contiguous()
    base = dict(name="c", kind="f32", mode="dense", image1=img, image2=img, flow=torch.zeros(1, 37, 53, 2), valid=None)
    p = R.params((37, 53), (16, 24), (51, 67), hflip=True, crop_y=9, crop_x=4, colour=((1.0, 1.7, 1.0, 0.0),) * 2, rects=((5, 5, 30, 20),))
    for dtype, tol in ((F64, 1e-12), (torch.float32, 1e-4)):
        out = R.evaluate(dict(base, params=[p]), dtype)
        want = (colour.to(dtype) * 255.0)[:, None, None].expand(3, 16, 24)
        assert float((out["crop1"][0] - want).abs().max()) <= tol and float((out["crop2"][0] - want).abs().max()) <= tol


def test_means_of_a_two_valued_image_are_those_of_the_sources():
    """Image 1 is 0.2 everywhere, image 2 is 0.6 with 7 of its 29 columns (away from the crop) at 0.2.  The symmetric contrast
    mean is over both SOURCES, not over the crops (0.4); the eraser's colour is the mean of the jittered second source."""
    img1 = torch.full((1, 21, 29, 3), 0.2, dtype=F64)
    img2 = torch.full((1, 21, 29, 3), 0.6, dtype=F64)
    img2[:, :, :7] = 0.2                                                       # 7 of 29 columns
    base = dict(name="m", kind="f32", mode="dense", image1=img1, image2=img2, flow=torch.zeros(1, 21, 29, 2), valid=None)
    crop = dict(crop_y=2, crop_x=12)                                           # columns 12..19: all 0.6 in image 2
    mean = (0.2 + (0.6 * 22 + 0.2 * 7) / 29) / 2
    sym = R.evaluate(dict(base, params=[R.params((21, 29), (8, 8), colour=((1.0, 0.5, 1.0, 0.0),) * 2, **crop)]), F64)
    assert float((sym["crop1"] - 255 * (mean + 0.5 * (0.2 - mean))).abs().max()) <= 1e-10
    assert float((sym["crop2"] - 255 * (mean + 0.5 * (0.6 - mean))).abs().max()) <= 1e-10
    asym = R.evaluate(dict(base, params=[R.params((21, 29), (8, 8), colour=((1.0, 0.5, 1.0, 0.0),) * 2, asymmetric=True, **crop)]), F64)
    m2 = (0.6 * 22 + 0.2 * 7) / 29
    assert float((asym["crop1"] - 255 * 0.2).abs().max()) <= 1e-10            # image 1 is constant: nothing moves
    assert float((asym["crop2"] - 255 * (m2 + 0.5 * (0.6 - m2))).abs().max()) <= 1e-10
    # the eraser writes the mean of the JITTERED source 2 (brightness 0.5 halves it), whole source, not the crop's
    er = R.evaluate(dict(base, params=[R.params((21, 29), (8, 8), colour=((0.5, 1.0, 1.0, 0.0),) * 2, rects=((12, 2, 8, 8),), **crop)]), F64)
    assert float((er["crop2"] - 255 * 0.5 * m2).abs().max()) <= 1e-10
    assert float((er["crop1"] - 255 * 0.5 * 0.2).abs().max()) <= 1e-10        # image 1 has no eraser


def test_a_rectangle_on_the_source_shows_up_scaled_in_an_upscaled_crop():
    """Source 15 x 23 doubled to 30 x 46: the rectangle (x0, y0, dx, dy) = (6, 4, 5, 3) of the source covers columns 12..21 and
    rows 8..13 of the resized image; one pixel inside that border every tap is in the rectangle and the value is the fill."""
    g = torch.Generator().manual_seed(5)
    img = torch.rand(1, 15, 23, 3, generator=g, dtype=F64)
    case = dict(name="r", kind="f32", mode="dense", image1=img, image2=img, flow=torch.zeros(1, 15, 23, 2), valid=None,
                params=[R.params((15, 23), (30, 46), (30, 46), rects=((6, 4, 5, 3),))])
    out = R.evaluate(case, F64)
    fill = img[0].mean((0, 1)) * 255.0
    inside = out["crop2"][0, :, 9:13, 13:21]
    assert float((inside - fill[:, None, None]).abs().max()) <= 1e-10
    changed = (out["crop2"][0] - out["crop1"][0]).abs().amax(0) > 1e-9
    ys, xs = torch.nonzero(changed, as_tuple=True)
    # (the bilinear taps spread the border by one resized pixel at the most)
    assert 7 <= int(ys.min()) <= 8 and 13 <= int(ys.max()) <= 14 and 11 <= int(xs.min()) <= 12 and 21 <= int(xs.max()) <= 22


def test_dense_flow_of_an_affine_field_is_the_same_field_times_the_scale():
    """Bilinear interpolation reproduces an affine function away from the border: crop pixel (y, x) of the resized image lies at
    (ry + 0.5) * in / out - 0.5 of the source."""
    Hs, Ws, t_h, t_w = 21, 29, 33, 41
    yy, xx = torch.meshgrid(torch.arange(Hs, dtype=F64), torch.arange(Ws, dtype=F64), indexing="ij")
    flow = torch.stack([1.5 + 0.25 * xx - 0.125 * yy, -2.0 + 0.5 * yy + 0.0625 * xx], -1)[None]
    img = torch.zeros(1, Hs, Ws, 3, dtype=F64)
    p = R.params((Hs, Ws), (16, 24), (t_h, t_w), crop_y=6, crop_x=7)
    out = R.evaluate(dict(name="a", kind="f32", mode="dense", image1=img, image2=img, flow=flow, valid=None, params=[p]), F64)
    sy = (torch.arange(16, dtype=F64) + 6 + 0.5) * (Hs / t_h) - 0.5
    sx = (torch.arange(24, dtype=F64) + 7 + 0.5) * (Ws / t_w) - 0.5
    sy, sx = sy[:, None], sx[None, :]
    want = torch.stack([(1.5 + 0.25 * sx - 0.125 * sy) * p["scale_x"], (-2.0 + 0.5 * sy + 0.0625 * sx) * p["scale_y"]])
    assert float((out["crop_flow"][0] - want).abs().max()) <= 1e-12
    assert bool((out["crop_valid"] == 1).all())


@pytest.mark.parametrize("mode", R.MODES)
def test_a_double_flip_of_a_symmetric_pattern_changes_nothing(mode):
    """Images symmetric under the half turn that the two flips make, a flow antisymmetric under it: with the whole (resized) image
    as the crop, both flips together change nothing.  The resizes commute with the flips: half-pixel centres, odd source sides."""
    g = torch.Generator().manual_seed(4)
    Hs, Ws = 15, 23
    a, b, f = torch.rand(1, Hs, Ws, 3, generator=g), torch.rand(1, Hs, Ws, 3, generator=g), torch.rand(1, Hs, Ws, 2, generator=g)
    img1, img2, flow = (a + a.flip(1, 2)) / 2, (b + b.flip(1, 2)) / 2, f - f.flip(1, 2)
    valid = (img1[..., 0] > 0.5).float()
    base = dict(name="s", kind="f32", mode=mode, image1=img1, image2=img2, flow=flow, valid=valid)
    kw = dict(colour=R.SYM, rects=((8, 5, 7, 5),))                              # a rectangle about the centre (11, 7): symmetric too
    for size, resize_to in (((Hs, Ws), None), ((21, 35), (21, 35))):
        plain = R.evaluate(dict(base, params=[R.params((Hs, Ws), size, resize_to, **kw)]), F64)
        both = R.evaluate(dict(base, params=[R.params((Hs, Ws), size, resize_to, hflip=True, vflip=True, **kw)]), F64)
        one_flip = R.evaluate(dict(base, params=[R.params((Hs, Ws), size, resize_to, hflip=True, **kw)]), F64)
        for k in plain:
            assert float((plain[k] - both[k]).abs().max()) <= 1e-12, (k, resize_to)
        # one flip alone mirrors the crop and negates the flow's x
        assert float((one_flip["crop2"] - plain["crop2"].flip(3)).abs().max()) <= 1e-12
        sign = torch.tensor([-1.0, 1.0], dtype=F64)[None, :, None, None]
        assert float((one_flip["crop_flow"] - sign * plain["crop_flow"].flip(3)).abs().max()) <= 1e-12


def test_the_order_matters():
    """colour(resize(x)) != resize(colour(x)) where clipping bites: a checkerboard of 0 and 1 under brightness 1.6 clips to
    (0, 1) before the resize and interpolates to 0.5; resized first it is 0.5 * 1.6 = 0.8."""
    Hs, Ws = 9, 11
    yy, xx = torch.meshgrid(torch.arange(Hs), torch.arange(Ws), indexing="ij")
    board = ((yy + xx) % 2).double()[None, :, :, None].expand(1, Hs, Ws, 3).contiguous()
    quad = ((1.6, 1.0, 1.0, 0.0),) * 2
    p = R.params((Hs, Ws), (18, 22), (18, 22), colour=quad)
    case = dict(name="o", kind="f32", mode="dense", image1=board, image2=board, flow=torch.zeros(1, Hs, Ws, 2), valid=None, params=[p])
    ours = R.evaluate(case, F64)["crop1"][0] / 255.0
    resized = R.resize_bilinear(board[0], torch.arange(18), torch.arange(22), 18, 22)
    other = R.photometric(resized, resized, dict(colour=quad), F64)[0]
    assert float(ours.max()) <= 1.0 and float((ours - other).abs().max()) >= 0.2
    # and it is the resize of the colour step's result
    first = R.photometric(board[0], board[0], dict(colour=quad), F64)[0]
    want = R.resize_bilinear(first.permute(1, 2, 0), torch.arange(18), torch.arange(22), 18, 22).permute(2, 0, 1)
    assert float((ours - want).abs().max()) <= 1e-12


def test_every_gpu_case_meets_the_input_condition():
    """Every source side is odd and every resized side of a nearest-mode case is at most 120, so every nearest-neighbour
    coordinate (dst + 0.5) * in / out is at least 1 / 240 from an integer; asserted >= 1e-3 in float32 and in float64, for every
    case (the dense ones too, which do not depend on it)."""
    cases = R.cases()
    n = len(R.specs(True))
    assert len(cases) == 2 * (2 * n + 1) + 1                                   # both modes and dtypes, the fallback dense only, the cap once
    assert len({c["name"] for c in cases}) == len(cases)
    for case in cases:
        assert R.nearest_margin(case) >= 1e-3, case["name"]
        for p in case["params"]:
            assert p["src_hw"][0] % 2 == 1 and p["src_hw"][1] % 2 == 1 and p.get("win_y", 0) == 0 and p.get("win_x", 0) == 0
            assert p["full_hw"] == (p["t_h"], p["t_w"])
            if case["mode"] == "sparse":
                assert p["t_h"] <= 120 and p["t_w"] <= 120 or not p.get("resize")
                assert not p.get("asymmetric")                                 # SparseFlowAugmentor never draws it
            if p.get("resize") and not case["name"].startswith("fallback"):
                assert p["scale_y"] == float(torch.tensor(float(p["t_h"])) / torch.tensor(float(p["src_hw"][0])))
    fallback = [c for c in cases if c["name"].startswith("fallback")]
    assert len(fallback) == 2 and all(c["mode"] == "dense" for c in fallback)
    p = fallback[0]["params"][0]
    assert (p["t_h"], p["t_w"]) == (24, 33) and p["scale_x"] == p["scale_y"] == R.MIN_SCALE and 1.14 < R.MIN_SCALE < 1.15
    assert any(c["mode"] == "dense" and any(q.get("asymmetric") for q in c["params"]) for c in cases)
    sizes = {(q["t_h"], q["t_w"]) for q in next(c for c in cases if c["name"].startswith("batch3"))["params"]}
    assert len(sizes) == 3


def test_limits_are_finite_and_non_zero():
    twin, lim = R.twin_errors(), R.limits()
    assert set(lim) == {"image", "flow"}
    for q in lim:
        assert math.isfinite(lim[q]) and lim[q] > 0 and lim[q] == R.FACTOR * twin[q]
    # the twin takes the reference's decisions (indices, signs): valid maps agree exactly, and so does every flow that is not
    # interpolated -- up to the rounding of the one multiply by the scale
    for i, case in enumerate(R.cases()):
        assert torch.equal(R.twin(i)["crop_valid"].double(), R.reference(i)["crop_valid"]), case["name"]
        for b, p in enumerate(case["params"]):
            if not R.bilinear_flow(case, b):
                err = R.field_error(R.twin(i)["crop_flow"][b], R.reference(i)["crop_flow"][b])
                assert err <= (1.0 if p.get("resize") else 0.0), (case["name"], b, err)
