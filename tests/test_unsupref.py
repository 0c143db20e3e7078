"""CPU-only checks of the restatement of the unsupervised loss (tests/_unsupref.py), independent of any kernel: closed forms,
its autograd gradient against central differences, the input conditions of every GPU case, and the limits the GPU tests use
(four times the fp32 twin's worst error against float64)."""
import math

import torch
import torch.nn.functional as F

import _unsupref as R
from _util import _log_margin

D = torch.float64


def test_zero_flow_on_identical_images_is_the_closed_form():
    g = torch.Generator().manual_seed(1)
    B, H, W = 2, 11, 13
    img = R.make_image(g, B, H, W).double()
    loss, M, warped = R.census_parts(img, img, torch.zeros(B, 2, H, W, dtype=D), None)
    sm, n = B * (H - 6) * (W - 6), B * H * W
    assert torch.equal(warped, img) and float(M.sum()) == sm
    assert abs(float(loss) - 0.01 ** 0.4 * sm / (sm + 1e-6 * n)) <= 1e-12


def test_range_map_closed_forms():
    B, H, W = 2, 6, 9
    zero = torch.zeros(B, 2, H, W, dtype=D)
    assert torch.equal(R.range_map(zero), torch.ones(B, H, W, dtype=D))
    shift = zero.clone()
    shift[:, 0], shift[:, 1] = 2.0, -1.0
    want = torch.zeros(B, H, W, dtype=D)
    want[:, :H - 1, 2:] = 1.0                      # landed at (x + 2, y - 1): an empty strip on the left and at the bottom
    assert torch.equal(R.range_map(shift), want)
    half = zero.clone()
    half[:, 0] = 0.5
    want = torch.ones(B, H, W, dtype=D)
    want[:, :, 0] = 0.5                            # every pixel splits 0.5 / 0.5 between x and x + 1; the last half leaves
    assert (R.range_map(half) - want).abs().max() <= 1e-12
    assert torch.equal(R.occlusion_mask(half), want) and torch.equal(R.occlusion_mask(half, "none"), torch.ones(B, H, W, dtype=D))


def test_smoothness_closed_forms():
    B, H, W = 2, 8, 9
    const_img = torch.full((B, 3, H, W), 0.4, dtype=D)
    const_flow = torch.full((B, 2, H, W), 1.7, dtype=D)
    assert abs(float(R.smoothness_loss(const_img, const_flow, 1)) - 1e-3) <= 1e-12
    s, a = 0.004, 0.3
    xs = torch.arange(W, dtype=D).view(1, 1, 1, W)
    img = (0.1 + s * xs).expand(B, 3, H, W)
    flow = torch.cat([a * xs.expand(B, 1, H, W), torch.zeros(B, 1, H, W, dtype=D)], 1)
    for weighting, w1, w2 in (("exponential", math.exp(-150 * s), math.exp(-300 * s)),
                              ("gaussian", math.exp(-(150 * s) ** 2), math.exp(-(300 * s) ** 2))):
        want1 = (w1 * (math.sqrt(a * a + 1e-6) + 1e-3) / 2 + 1e-3) / 2
        assert abs(float(R.smoothness_loss(img, flow, 1, 150.0, weighting)) - want1) <= 1e-12
        assert abs(float(R.smoothness_loss(img, flow, 2, 150.0, weighting)) - (1e-3 * w2 + 1e-3) / 2) <= 1e-12


def test_resampler_is_grid_sample_in_pixel_units():
    """The hand-written four-tap resampler is grid_sample(align_corners=True, padding_mode='zeros') in pixel units, value and
    coordinate gradient, at points off the integers (on them grid_sample's normalisation decides the floor)."""
    g = torch.Generator().manual_seed(2)
    B, H, W = 2, 9, 10
    img = R.make_image(g, B, H, W).double()
    flow = (6.0 * (torch.rand(B, 2, H, W, generator=g, dtype=D) - 0.5)).requires_grad_(True)      # some taps leave the frame
    sx, sy = R.coords(flow)
    grid = torch.stack([2 * sx / (W - 1) - 1, 2 * sy / (H - 1) - 1], -1)
    up = torch.rand(B, 3, H, W, generator=g, dtype=D)
    a = R.resample(img, sx, sy)
    b = F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    assert (a - b).abs().max() <= 1e-12
    ga, gb = torch.autograd.grad((a * up).sum(), flow, retain_graph=True)[0], torch.autograd.grad((b * up).sum(), flow)[0]
    assert (ga - gb).abs().max() <= 1e-10


def test_autograd_gradient_against_central_differences():
    g = torch.Generator().manual_seed(3)
    B, H, W = 1, 9, 10
    f1, f2 = R.make_image(g, B, H, W).double(), R.make_image(g, B, H, W).double()
    flow = 2.0 * (torch.rand(B, 2, H, W, generator=g, dtype=D) - 0.5)
    mask = torch.rand(B, H, W, generator=g, dtype=D)

    def total(fl):
        return R.census_loss(f1, f2, fl, mask) + R.smoothness_loss(f1, fl, 1) + R.smoothness_loss(f1, fl, 2, 150.0, "gaussian")

    fl = flow.clone().requires_grad_(True)
    grad = torch.autograd.grad(total(fl), fl)[0]
    eps, worst = 1e-6, 0.0
    for idx in range(flow.numel()):
        d = torch.zeros(flow.numel(), dtype=D)
        d[idx] = eps
        d = d.view_as(flow)
        num = float(total(flow + d) - total(flow - d)) / (2 * eps)
        worst = max(worst, abs(num - float(grad.view(-1)[idx])))
    assert worst <= 1e-6 * max(1.0, float(grad.abs().max())), worst
    assert float(grad[:, :, :3].abs().max()) > 0           # the border pixels lie in the patches of the pixels inside it


def test_input_conditions_of_every_gpu_case():
    cases = R.cases()
    assert len(cases) == len(R.SHAPES) * len(R.FAMILIES)
    for c in cases:
        assert R.input_conditions(c) == 0.0, c["name"]
    sc = R.sequence_case()
    for a, b in zip(sc["fw"], sc["bw"]):
        assert R.input_conditions(dict(family="", frames=sc["frames"], crop_yx=sc["crop_yx"], flow=a, flow_bw=b)) == 0.0


def test_flow_families_do_what_they_are_for():
    for i, c in enumerate(R.cases()):
        ref = R.reference(i)
        inner = c["B"] * (c["H"] - 6) * (c["W"] - 6)
        _, M, _ = R.census_parts(c["frames"][0].double(), c["frames"][1].double(), c["flow"].double(), None, c["crop_yx"])
        if c["family"] == "subpixel":
            assert float(c["flow"].abs().max()) <= 3.0
        if c["family"] == "large" and inner >= 100:
            assert 0.1 <= float(M.sum()) / inner <= 0.9, c["name"]         # a share of the warps leaves the frame
        if c["family"] == "fold":
            assert float(ref["range_map"].max()) > 2.0
        if c["family"] == "allout":
            assert float(M.sum()) == 0 and float(ref["census"]) == 0 and not ref["census_dflow"].any()


def test_limits_are_derived_from_the_fp32_twin():
    twin, limits = R.twin_errors(), R.limits()
    assert set(limits) == {"range_map", "census", "census_dflow", "smoothness", "smoothness_dflow", "sequence", "sequence_dflow"}
    for q, e in twin.items():
        assert limits[q] == 4.0 * e and 0 < e < float("inf")
        # sanity of the twin itself: scalars within a few hundred ulps, fields within 1e-3 of their largest value
        assert e < (1e-4 if q in ("census", "smoothness", "sequence") else 2.0 ** 24 * 1e-3), (q, e)
    for q in sorted(limits):                       # with FSRAFT_PARITY_LOG: the derived limits next to the kernels' margins
        _log_margin(f"LIMITS[{q}]: the fp32 twin's worst error against float64", twin[q], limits[q], "4 x the twin's error")
