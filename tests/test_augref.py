"""CPU-only checks that pin the restatement of the augmentation (tests/_augref.py) independently of any kernel: its resizes
against torch's own, its HSV pair against the standard library's, the identities and closed forms of its colour and eraser
steps, and the input condition of every GPU case."""
import colorsys
import math

import pytest
import torch
import torch.nn.functional as F

import _augref as R

F64 = torch.float64


@pytest.mark.parametrize("src,dst", [((37, 53), (51, 67)), ((37, 53), (23, 31)), ((8, 8), (8, 8)), ((5, 7), (40, 9)), ((53, 85), (75, 120))])
def test_bilinear_resize_is_torchs_half_pixel_bilinear(src, dst):
    img = torch.rand(*src, 3, generator=torch.Generator().manual_seed(1), dtype=F64)
    got = R.resize_bilinear(img, torch.arange(dst[0]), torch.arange(dst[1]), *dst)
    want = F.interpolate(img.permute(2, 0, 1)[None], size=dst, mode="bilinear", align_corners=False)[0].permute(1, 2, 0)
    assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-13


@pytest.mark.parametrize("src,dst", [((37, 53), (51, 67)), ((37, 53), (49, 71)), ((53, 85), (61, 97)), ((53, 85), (75, 120)), ((37, 53), (21, 30))])
def test_nearest_resize_is_torchs_nearest_exact(src, dst):
    for n_in, n_out in zip(src, dst):      # the condition under which a float32 and an exact index agree
        c = R.nearest_coordinate(torch.arange(n_out), n_in, n_out, F64)
        assert float((c - torch.round(c)).abs().min()) >= 1e-3
    x = torch.rand(*src, 2, generator=torch.Generator().manual_seed(2), dtype=F64)
    got = R.resize_nearest(x, torch.arange(dst[0]), torch.arange(dst[1]), *dst)
    want = F.interpolate(x.permute(2, 0, 1)[None], size=dst, mode="nearest-exact")[0].permute(1, 2, 0)
    assert torch.equal(got, want)


def colours(n=500, seed=3):
    g = torch.Generator().manual_seed(seed)
    rgb = torch.rand(3, n, generator=g, dtype=F64)
    rgb[:, :20] = rgb[:1, :20]                    # greys
    rgb[:, 20] = 0.0                              # black
    rgb[1, 21:40] = rgb[0, 21:40]                 # two channels tie at the top or the bottom
    rgb[2, 40:60] = rgb[1, 40:60]
    return rgb


def test_hsv_pair_is_the_standard_librarys():
    rgb = colours()
    h, s, v = R.rgb_to_hsv(rgb)
    back = R.hsv_to_rgb(h, s, v)
    for i in range(rgb.shape[1]):
        want = colorsys.rgb_to_hsv(*rgb[:, i].tolist())
        got = (float(h[i]), float(s[i]), float(v[i]))
        assert abs(got[1] - want[1]) <= 1e-12 and abs(got[2] - want[2]) <= 1e-12
        dh = abs(got[0] - want[0])
        assert min(dh, 1.0 - dh) <= 1e-12 and 0.0 <= got[0] < 1.0           # (the hue is a point of a circle)
        rgb_want = colorsys.hsv_to_rgb(*want)
        assert max(abs(float(back[k, i]) - rgb_want[k]) for k in range(3)) <= 1e-12


def test_saturation_one_and_hue_zero_are_the_identity():
    rgb = colours()
    assert float((R.adjust_saturation(rgb, 1.0) - rgb).abs().max()) <= 1e-14
    assert float((R.adjust_hue(rgb, 0.0) - rgb).abs().max()) <= 1e-14
    assert float((R.adjust_hue(rgb, 1.0) - rgb).abs().max()) <= 1e-12       # a whole turn: the identity to rounding
    assert float((R.adjust_hue(R.adjust_hue(rgb, 0.3), -0.3) - rgb).abs().max()) <= 1e-12
    grey = R.adjust_saturation(rgb, 0.0)
    assert float((grey - rgb.max(0).values).abs().max()) <= 1e-14           # saturation 0 leaves v in every channel


def test_a_constant_image_is_a_fixed_point_of_contrast():
    x = torch.full((3, 5, 7), 0.3125, dtype=F64) * torch.tensor([1.0, 2.0, 0.5], dtype=F64)[:, None, None]
    for dtype in (F64, torch.float32):
        crop = (x * 255.0).to(dtype)
        p = dict(colour=((1.0, 1.7, 1.0, 0.0),) * 2)
        c1, c2 = R.colour(crop, crop, p)
        assert float((c1 - crop).abs().max()) <= (1e-12 if dtype == F64 else 1e-4) and torch.equal(c1, c2)
    assert torch.equal(R.adjust_contrast(x, 1.7, x.mean((1, 2), keepdim=True)), x)


def test_symmetric_contrast_takes_its_mean_over_both_crops():
    a, b = torch.full((3, 4, 4), 51.0, dtype=F64), torch.full((3, 4, 4), 153.0, dtype=F64)
    sym = R.colour(a, b, dict(colour=((1.0, 0.5, 1.0, 0.0),) * 2))
    asym = R.colour(a, b, dict(colour=((1.0, 0.5, 1.0, 0.0),) * 2, asymmetric=True))
    # the pair's mean is 102: 51 -> 102 - 25.5, 153 -> 102 + 25.5; per image nothing moves
    assert float((sym[0] - 76.5).abs().max()) <= 1e-10 and float((sym[1] - 127.5).abs().max()) <= 1e-10
    assert float((asym[0] - 51.0).abs().max()) <= 1e-10 and float((asym[1] - 153.0).abs().max()) <= 1e-10


@pytest.mark.parametrize("kind", R.DTYPES)
def test_identity_parameters_reproduce_the_source_window_times_255(kind):
    case = R.make_case("w", [R.params((37, 53), (32, 48), (16, 24), win_y=4, win_x=5, crop_y=8, crop_x=16)], True, kind, 11)
    for dtype in (torch.float32, F64):
        out = R.evaluate(case, dtype)
        for k, src in (("frame1", case["image1"]), ("frame2", case["image2"])):
            window = src[0, 4:36, 5:53].permute(2, 0, 1).to(dtype)
            assert torch.equal(out[k][0], window if kind == "u8" else window * 255.0)
        assert torch.equal(out["frame_flow"][0], case["flow"][0, 4:36, 5:53].permute(2, 0, 1).to(dtype))
        assert torch.equal(out["frame_valid"][0, 0], case["valid"][0, 4:36, 5:53].to(dtype))
        assert torch.equal(out["crop_flow"], out["frame_flow"][:, :, 8:24, 16:40]) and torch.equal(out["crop_valid"], out["frame_valid"][:, :, 8:24, 16:40])
        # the identity colour is the identity to rounding only (x / 255 * 255, two HSV trips)
        assert float((out["crop1"] - out["frame1"][:, :, 8:24, 16:40]).abs().max()) <= (1e-10 if dtype == F64 else 1e-3)


def test_a_double_flip_of_a_symmetric_pattern_changes_nothing():
    """An image symmetric under the half turn that the two flips make, a flow antisymmetric under it (the flips' signs restore
    it): with the whole (resized) image as the frame, both flips together change nothing.  The resizes commute with the flips:
    half-pixel centres, and odd source sides keep the nearest-neighbour coordinates off the integers."""
    g = torch.Generator().manual_seed(4)
    Hs, Ws = 15, 23
    a, f = torch.rand(1, Hs, Ws, 3, generator=g), torch.rand(1, Hs, Ws, 2, generator=g)
    img, flow = (a + a.flip(1, 2)) / 2, f - f.flip(1, 2)
    valid = (img[..., 0] > 0.5).float()
    base = dict(name="s", kind="f32", image1=img, image2=img.flip(3), flow=flow, valid=valid)
    for frame, resize_to in (((Hs, Ws), None), ((21, 35), (21, 35))):
        plain = R.evaluate(dict(base, params=[R.params((Hs, Ws), frame, (8, 8), resize_to)]), F64)
        both = R.evaluate(dict(base, params=[R.params((Hs, Ws), frame, (8, 8), resize_to, hflip=True, vflip=True)]), F64)
        one = R.evaluate(dict(base, params=[R.params((Hs, Ws), frame, (8, 8), resize_to, hflip=True)]), F64)
        for k in ("frame1", "frame2", "frame_flow", "frame_valid"):
            assert float((plain[k] - both[k]).abs().max()) <= 1e-12, (k, resize_to)
        # one flip alone mirrors the frame and negates the flow's x
        assert float((one["frame1"] - plain["frame1"].flip(3)).abs().max()) <= 1e-12
        sign = torch.tensor([-1.0, 1.0], dtype=F64)[None, :, None, None]
        assert float((one["frame_flow"] - sign * plain["frame_flow"].flip(3)).abs().max()) <= 1e-12


def test_eraser_mean_of_a_two_valued_image():
    crop = torch.full((3, 10, 20), 40.0, dtype=F64)
    crop[:, :, :5] = 200.0                        # a quarter of the pixels
    crop[1] *= 0.5
    out = R.eraser(crop, ((3, 2, 6, 4), (18, 9, 2, 1), (0, 0, 0, 5)))
    mean = torch.tensor([80.0, 40.0, 80.0], dtype=F64)
    assert torch.equal(out[:, 2:6, 3:9], mean[:, None, None].expand(3, 4, 6)) and torch.equal(out[:, 9:, 18:], mean[:, None, None].expand(3, 1, 2))
    mask = torch.ones(10, 20, dtype=torch.bool)
    mask[2:6, 3:9] = False
    mask[9:, 18:] = False
    assert torch.equal(out[:, mask], crop[:, mask])          # the second rectangle has the first mean, not a mean of erased pixels


def test_every_gpu_case_meets_the_input_condition():
    """Every nearest-neighbour coordinate (dst + 0.5) * scale of every case, in float32 and in float64, is at least 1e-3 from an
    integer, so the float32 index is the exact one."""
    cases = R.cases()
    assert len(cases) == 2 * len(R.SPECS) + 1
    assert any(R.resized(c) for c in cases) and any(not R.resized(c) for c in cases)
    for case in cases:
        assert R.nearest_margin(case) >= 1e-3, case["name"]
        for p in case["params"]:
            if p.get("resize"):
                assert (p["t_h"], p["scale_y"]) == R.resized_size(p["src_hw"][0], p["t_h"] / p["src_hw"][0])


def test_limits_are_finite_and_non_zero():
    twin, lim = R.twin_errors(), R.limits()
    assert set(lim) == {"frame", "crop"}
    for q in lim:
        assert math.isfinite(lim[q]) and lim[q] > 0 and lim[q] == R.FACTOR * twin[q]
    # the twin takes the reference's decisions (indices, windows, signs): valid maps agree exactly, and so do the flows of the
    # cases without a resize, which are copies
    for i, case in enumerate(R.cases()):
        for k in ("frame_valid", "crop_valid") + (() if R.resized(case) else ("frame_flow", "crop_flow")):
            assert torch.equal(R.twin(i)[k].double(), R.reference(i)[k]), (case["name"], k)
