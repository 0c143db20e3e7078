"""GPU checks of flow visualisation and submission encoding (csrc/flow_viz.hip) and of what is built on it
(core/utils/flow_viz.py, raft_tf.visualize_flow(s), the *_vis drivers and demo of evaluate.py).

Wheel pictures are compared with outputs of the reference's own flow_viz.py (tests/golden/flow_viz.npz) at the small shapes and
with its restatement (_vizref, pinned to that fixture in test_vizref.py) at 436 x 1024, under a two-part rule: no channel value
may differ by more than 1 level, and at most max(1, ceil(1e-3 * n)) of a case's n values may differ at all.  The reference
evaluates everything behind the table lookup in float64, the kernel in float32, so a value within rounding of an integer may
fall on the other side of the floor; the cap is a condition, not a measurement: on the CPU an all-float32 evaluation agreed with
the reference on every value at the small shapes and differed on under 1e-5 of them at 436 x 1024, on under 1e-4 with the angle
perturbed by up to 16 ulp, never by more than 1 level, while a wrong wheel index, wrap, channel order or normaliser moves most
values by many levels.

HSV: the fp32 output is within 1e-5 absolute of the float64 restatement (a float32 NumPy evaluation is off by up to 7e-7, by
1.8e-6 with a 4-ulp angle error and by 6e-6 at 16 ulp; the device's atan2f is the only unknown and 1e-5 covers 16 ulp); the
uint8 variant is under the two-part rule.  The KITTI encoding is compared exactly.

The worst fraction of every limit goes to the parity log (profiles/flow_viz_margins.txt)."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import _evalref as E
import _vizref as R
from _util import T, _log_margin, load

pytestmark = pytest.mark.gpu
DEV = "cuda"
HSV_ATOL = 1e-5
BORDER = 1.0e6                 # what the frame around a view holds: it would wreck the maximum

# name: B, H, W, frame (Hp, Wp, top, left), fixture key (None: seeded flow, compared with the restatement)
CASES = {
    "1x1": (1, 1, 1, (1, 1, 0, 0), "1x1"),
    "3x5_less_than_a_wave": (1, 3, 5, (3, 5, 0, 0), "3x5"),
    "37x61_view_of_40x64": (1, 37, 61, (40, 64, 0, 1), "37x61"),          # odd pitch, base 4 bytes off 16, 3 * H * W % 4 == 3
    "37x61_view_of_40x64_b3": (3, 37, 61, (40, 64, 0, 1), "37x61"),       # sample b is the fixture's flow times (1, 0.5, 3)[b]
    "40x64_contiguous": (1, 40, 64, (40, 64, 0, 0), "40x64"),
    "436x1024_view_of_440x1024": (1, 436, 1024, (440, 1024, 2, 0), None),  # 109 blocks of the colouring, 7 trips of the maximum
}
B3_FACTORS = (1.0, 0.5, 3.0)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> frame [B,2,Hp,Wp] (host, float32), (top, left), flows [B,H,W,2] (numpy float32, the reference's layout)."""
    B, H, W, (Hp, Wp, top, left), key = CASES[name]
    if key is None:
        rng = np.random.default_rng(sum(map(ord, name)))
        flow = (rng.standard_normal((1, H, W, 2)) * 6.0).astype(np.float32)
        flow *= np.where(rng.random((1, H, W, 1)) < 0.1, 5.0, 1.0).astype(np.float32)
    else:
        base = load("flow_viz")[key + ".flow"]
        flow = np.stack([base * np.float32(B3_FACTORS[b]) for b in range(B)])
    frame = torch.full((B, 2, Hp, Wp), BORDER)
    frame[:, 0] += torch.arange(Wp)                                    # not constant, and larger than every flow
    frame[:, :, top:top + H, left:left + W] = T(flow).permute(0, 3, 1, 2)
    return frame, (top, left), flow


def view(name, samples=slice(None)):
    frame, (top, left), flow = case(name)
    H, W = flow.shape[1:3]
    return frame[samples].to(DEV)[:, :, top:top + H, left:left + W]


@functools.lru_cache(maxsize=None)
def wheel_reference(name, variant):
    """uint8 [B,H,W,3]: the fixture where it has the picture (sample 0 of the fixture cases), the restatement elsewhere."""
    B, H, W, _, key = CASES[name]
    _, _, flow = case(name)
    g = load("flow_viz")
    uv_scale = g["uv_scale"]
    out = []
    for b in range(B):
        if variant == "colors":
            f = flow[b] * uv_scale
            want = R.to_image(f, scale=1)
        else:
            want = R.to_image(flow[b], clip=10 if variant == "clip10" else None, bgr=variant == "bgr")
        if key is not None and b == 0:
            fixture = g[key + "." + {"plain": "image", "clip10": "image_clip10", "bgr": "image_bgr", "colors": "colors"}[variant]]
            assert np.array_equal(want, fixture)                       # (test_vizref.py; the fixture is what is compared below)
            want = fixture
        out.append(want)
    return np.stack(out)


def two_part(got, want, what):
    worst, differing, cap = R.two_part(got, want)
    print(f"{what}: {differing} of {got.size} values differ (cap {cap}), by at most {worst} level(s)")
    _log_margin(what + " largest level difference", worst, 1, "levels")
    _log_margin(what + " values that differ", differing, cap, f"max(1, ceil(1e-3 * {got.size}))")
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert worst <= 1 and differing <= cap, (what, worst, differing, cap)


def run_wheel(name, variant, samples=slice(None)):
    from flow_supervisor_amd.core.utils import flow_viz
    v = view(name, samples)
    if variant == "colors":
        s = float(load("flow_viz")["uv_scale"])
        return flow_viz.flow_uv_to_colors(v[:, 0] * s, v[:, 1] * s).cpu().numpy()
    return flow_viz.flow_to_image(v, clip_flow=10 if variant == "clip10" else None, convert_to_bgr=variant == "bgr").cpu().numpy()


@pytest.mark.parametrize("variant", ["plain", "clip10", "bgr", "colors"])
@pytest.mark.parametrize("name", list(CASES))
def test_wheel_matches_the_reference(name, variant):
    got = run_wheel(name, variant)
    two_part(got, wheel_reference(name, variant), f"wheel {variant} {name}")
    if name.startswith("37x61_view"):                                  # the view these cases are about is what they say it is
        v = view(name)
        assert v.data_ptr() % 16 == 4 and v.stride(2) == 64 and not v.is_contiguous() and 3 * 37 * 61 % 4 == 3
    if name.endswith("b3"):                                            # each sample on its own maximum
        from flow_supervisor_amd import ops
        rm = ops.flow_rad_max(view(name)).cpu().numpy()
        want = np.array([R.rad_max(f) for f in case(name)[2]], np.float32)
        assert rm.dtype == np.float32 and np.array_equal(rm, want) and len(set(rm.tolist())) == 3


def test_rad_max_is_the_float32_maximum_and_ignores_the_border():
    from flow_supervisor_amd import ops
    for name in CASES:
        flow = case(name)[2]
        got = ops.flow_rad_max(view(name)).cpu().numpy()
        assert np.array_equal(got, np.array([R.rad_max(f) for f in flow], np.float32)), name
        got = ops.flow_rad_max(view(name), clip=10.0).cpu().numpy()
        assert np.array_equal(got, np.array([R.rad_max(f, 10) for f in flow], np.float32)), name
        assert float(got.max()) < BORDER


def test_special_inputs():
    from flow_supervisor_amd.core.utils import flow_viz
    # all-zero flow: white, exactly
    img = flow_viz.flow_to_image(torch.zeros(2, 5, 7, device=DEV))
    assert img.shape == (5, 7, 3) and img.dtype == torch.uint8 and bool((img == 255).all())
    # axis-aligned flow, v = +0.0 and -0.0, u of both signs: atan2f(-v, -u) is -pi, +pi, -0 and +0 -- both ends of the table
    # (k0 = 0 and k0 = 54 with k1 wrapping to 0) and its middle
    # (magnitudes chosen so that no 255 * col lands within 1e-4 of an integer)
    uv = np.array([[[3.0, 0.0], [3.0, -0.0], [-3.0, 0.0], [-3.0, -0.0], [0.0, 2.5], [0.0, -2.5], [1.2, 0.0], [-1.2, -0.0]]], np.float32)
    a = np.arctan2(-uv[0, :, 1], -uv[0, :, 0]) / np.float32(np.pi)
    assert a.tolist()[:4] == [-1.0, 1.0, -0.0, 0.0]
    want = R.to_image(uv)
    got = flow_viz.flow_to_image(T(uv).permute(2, 0, 1).contiguous().to(DEV)).cpu().numpy()
    two_part(got, want, "wheel axis-aligned")
    assert tuple(got[0, 0]) == tuple(want[0, 0]) == (255, 0, 0)        # -pi: table entry 0
    # +pi: entry 54 (255, 0, 43) with weight 1 and entry 55 -> 0 with weight 0, as the reference has it: not the colour of -pi
    assert tuple(got[0, 1]) == tuple(want[0, 1]) and got[0, 1, 0] == 255 and got[0, 1, 1] == 0 and 40 <= got[0, 1, 2] <= 44
    assert tuple(got[0, 2]) == tuple(got[0, 3]) == tuple(want[0, 2])                        # the middle, from -0 and +0
    # the clip quirk: negative components go to 0, so a flow pointing up-left is coloured as zero flow: white
    neg = torch.full((2, 4, 6), -7.0, device=DEV)
    neg[:, 0, 0] = 4.0
    img = flow_viz.flow_to_image(neg, clip_flow=10).cpu().numpy()
    assert np.all(img[1:] == 255) and np.all(img[0, 1:] == 255) and not np.all(img[0, 0] == 255)
    assert np.array_equal(img, R.to_image(neg.permute(1, 2, 0).cpu().numpy(), clip=10))
    # the BGR flag is the channel swap
    v = view("40x64_contiguous")
    assert np.array_equal(flow_viz.flow_to_image(v, convert_to_bgr=True).cpu().numpy(), flow_viz.flow_to_image(v).cpu().numpy()[..., ::-1])
    # the given-scale path through the 0.75 branch; return_scale
    flow = case("40x64_contiguous")[2][0]
    got, scale = flow_viz.flow_to_image(v, scale=4.0, return_scale=True)
    assert np.mean(np.sqrt((flow ** 2).sum(-1)) / 4.0 > 1) > 0.2
    two_part(got.cpu().numpy(), R.to_image(flow, scale=4.0)[None], "wheel given scale 4")
    assert scale.is_cuda and scale.shape == (1,) and float(scale[0]) == float(R.rad_max(flow))
    # a NumPy [H,W,2] array, the reference's argument, comes back as NumPy
    out = flow_viz.flow_to_image(flow)
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8
    two_part(out, load("flow_viz")["40x64.image"], "wheel numpy in, numpy out")
    out = flow_viz.flow_uv_to_colors(flow[..., 0] / 8, flow[..., 1] / 8)
    two_part(out, load("flow_viz")["40x64.colors"], "colors numpy in, numpy out")


def test_non_finite_pixels_are_black_and_out_of_the_maximum():
    from flow_supervisor_amd import ops
    from flow_supervisor_amd.core.utils import flow_viz
    flow = case("37x61_view_of_40x64")[2][0].copy()
    flow[3, 4] = (np.nan, 1.0)
    flow[20, 60] = (2.0, -np.inf)
    clean = flow.copy()
    clean[3, 4] = clean[20, 60] = 0.0                                 # zero takes no part in a maximum either
    dev = T(flow).permute(2, 0, 1).contiguous().to(DEV)
    got = flow_viz.flow_to_image(dev).cpu().numpy()
    other = flow_viz.flow_to_image(T(clean).permute(2, 0, 1).contiguous().to(DEV)).cpu().numpy()
    assert tuple(got[3, 4]) == tuple(got[20, 60]) == (0, 0, 0)
    mask = np.ones((37, 61), bool)
    mask[3, 4] = mask[20, 60] = False
    assert np.array_equal(got[mask], other[mask])
    two_part(got[mask], R.to_image(clean)[mask], "wheel beside non-finite pixels")
    assert float(ops.flow_rad_max(dev[None])[0]) == float(R.rad_max(clean))
    assert float(ops.flow_rad_max(torch.full((1, 2, 3, 5), float("nan"), device=DEV))[0]) == 0.0     # no finite pixel: 0
    k = ops.flow_kitti16(dev[None])[0].cpu().numpy().view(np.uint16)
    assert k[3, 4].tolist() == [0, 64 + 32768, 1] and k[20, 60].tolist() == [128 + 32768, 0, 1]


@pytest.mark.parametrize("max_mag", [None, 0, 20])
@pytest.mark.parametrize("name", list(CASES))
def test_hsv_matches_the_restatement(name, max_mag):
    from flow_supervisor_amd import raft_tf
    flows = case(name)[2]
    nhwc = view(name).permute(0, 2, 3, 1)
    got = raft_tf.visualize_flows(nhwc, max_mag).cpu().numpy()
    want = np.stack([R.hsv(f, max_mag) for f in flows])
    assert got.dtype == np.float32 and got.shape == want.shape
    err = float(np.abs(got.astype(np.float64) - want).max())
    _log_margin(f"hsv max_mag={max_mag} {name}", err, HSV_ATOL, "absolute, against float64")
    assert err <= HSV_ATOL, (name, max_mag, err)
    assert got.min() >= 0.0 and got.max() <= 1.0
    got8 = raft_tf.visualize_flows(nhwc, max_mag, as_uint8=True).cpu().numpy()
    two_part(got8, np.stack([R.hsv_u8(f, max_mag) for f in flows]), f"hsv uint8 max_mag={max_mag} {name}")
    one = raft_tf.visualize_flow(nhwc[0], max_mag)
    assert one.shape == got.shape[1:] and np.array_equal(one.cpu().numpy(), got[0])


def test_hsv_of_a_zero_flow_is_white():
    from flow_supervisor_amd import raft_tf
    z = torch.zeros(3, 5, 2, device=DEV)
    for mm in (None, 0, 20):
        assert bool((raft_tf.visualize_flow(z, mm) == 1.0).all())
        assert bool((raft_tf.visualize_flow(z, mm, as_uint8=True) == 255).all())


@functools.lru_cache(maxsize=None)
def kitti_valid(name):
    B, H, W = CASES[name][:3]
    u = torch.rand(B, H, W, generator=torch.Generator().manual_seed(5 + H))
    valid = torch.where(u < 0.1, torch.full_like(u, 0.5), torch.where(u < 0.2, torch.full_like(u, 0.49999997), (u < 0.7).float()))
    valid[:, 0, 0] = 0.5
    return valid


@pytest.mark.parametrize("name", list(CASES))
def test_kitti_encoding_is_exact(name):
    from flow_supervisor_amd import ops
    flows = case(name)[2]
    assert np.abs(flows).max() < 512
    got = ops.flow_kitti16(view(name)).cpu().numpy().view(np.uint16)
    want = np.stack([R.kitti16(f) for f in flows])
    assert got.shape == want.shape and np.array_equal(got, want) and np.all(got[..., 2] == 1)
    assert np.array_equal(want[..., :2], (64.0 * flows + 2 ** 15).astype(np.uint16))          # the reference's expression
    valid = kitti_valid(name)
    got = ops.flow_kitti16(view(name), valid.to(DEV)).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, np.stack([R.kitti16(f, v) for f, v in zip(flows, valid.numpy())]))
    assert got[0, 0, 0, 2] == 1 and np.array_equal(got[..., 2], (valid.numpy() >= 0.5))        # an exact 0.5 counts


def test_kitti_encoding_saturates():
    from flow_supervisor_amd import ops
    flow = torch.tensor([[600.0, -600.0, 511.984375, -512.0, 0.0], [-600.0, 600.0, 512.0, -512.015625, -0.0]], device=DEV).view(1, 2, 1, 5)
    got = ops.flow_kitti16(flow)[0, 0].cpu().numpy().view(np.uint16)
    assert got.tolist() == [[65535, 0, 1], [0, 65535, 1], [65535, 65535, 1], [0, 0, 1], [32768, 32768, 1]]
    assert np.array_equal(got, R.kitti16(flow[0].permute(1, 2, 0).cpu().numpy())[0])


def all_four(name, samples=slice(None)):
    """The bytes of what the four entry points give for the case's samples."""
    from flow_supervisor_amd import ops
    v = view(name, samples)
    rm = ops.flow_rad_max(v)
    return [t.cpu().numpy().tobytes() for t in (rm, ops.flow_colors(v, rad_max=rm), ops.flow_hsv(v, rad_max=rm),
                                                ops.flow_hsv(v, rad_max=rm, as_uint8=True), ops.flow_kitti16(v))]


@pytest.mark.parametrize("name", ["37x61_view_of_40x64_b3", "436x1024_view_of_440x1024"])
def test_deterministic_and_batch_independent(name):
    first, second = all_four(name), all_four(name)
    assert first == second
    B = CASES[name][0]
    for b in range(B if B > 1 else 0):
        alone = all_four(name, slice(b, b + 1))
        for whole, part in zip(first, alone):
            n = len(part)
            assert whole[b * n:(b + 1) * n] == part, b


def test_flow_to_image_replays_from_a_graph():
    """No host read: captured on a static buffer and replayed after the buffer took a flow with another maximum, the graph gives
    the new flow's picture.  Everything is enqueued on the one capturing stream, so the capture is one linear chain."""
    from flow_supervisor_amd.core.utils import flow_viz
    frame, (top, left), flow = case("37x61_view_of_40x64_b3")
    H, W = flow.shape[1:3]
    static = frame[0:1].to(DEV).clone()
    v = static[:, :, top:top + H, left:left + W]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        flow_viz.flow_to_image(v)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured, scale = flow_viz.flow_to_image(v, return_scale=True)
    static.copy_(frame[2:3])                                           # three times the maximum
    graph.replay()
    torch.cuda.synchronize()
    replayed, replayed_scale = captured.clone(), scale.clone()
    del graph
    eager, eager_scale = flow_viz.flow_to_image(view("37x61_view_of_40x64_b3", slice(2, 3)), return_scale=True)
    assert torch.equal(replayed, eager) and torch.equal(replayed_scale, eager_scale)
    assert float(eager_scale[0]) == float(R.rad_max(flow[2])) != float(R.rad_max(flow[0]))
    two_part(replayed.cpu().numpy(), R.to_image(flow[2])[None], "wheel graph replay")


# ---------------------------------------------------------------------------------------------------------------- drivers
class ReplayModel:
    """model(image1, image2, iters=, flow_init=, test_mode=True) -> (None, the next image1.shape[0] stored predictions)"""

    def __init__(self, preds):
        self.preds, self.i = preds.to(DEV), 0

    def eval(self):
        return self

    def __call__(self, image1, image2, iters=None, flow_init=None, test_mode=False):
        B = image1.shape[0]
        out = self.preds[self.i:self.i + B]
        self.i += B
        assert test_mode and image1.is_cuda and image1.shape == image2.shape and image1.shape[-2:] == out.shape[-2:]
        return None, out


def padded_predictions(n, H, W, mode, seed):
    """n seeded padded predictions [n,2,Hp,Wp] whose border would wreck the maximum, and their un-padded parts [n,H,W,2]."""
    Hp, Wp = H + -H % 8, W + -W % 8
    top, left = E.pad_offsets(H, W, mode)
    g = torch.Generator().manual_seed(seed)
    preds = torch.full((n, 2, Hp, Wp), BORDER)
    inner = torch.randn(n, 2, H, W, generator=g) * 9.0 * torch.arange(1, n + 1).view(n, 1, 1, 1)
    preds[:, :, top:top + H, left:left + W] = inner
    return preds, inner.permute(0, 2, 3, 1).contiguous().numpy()


def test_kitti_submission_vis_writes_the_encoding_and_the_picture(tmp_path):
    from flow_supervisor_amd import evaluate as EV
    from flow_supervisor_amd.raft_utils.frame_utils import readFlowKITTI, readPNG
    H, W, n = 37, 61, 2
    preds, flows = padded_predictions(n, H, W, "kitti", 41)
    ds = [(torch.zeros(3, H, W), torch.zeros(3, H, W), ("%06d_10.png" % i,)) for i in range(n)]
    out, vis = str(tmp_path / "sub"), str(tmp_path / "vis")
    EV.create_kitti_submission_vis(ReplayModel(preds), ds, output_path=out, vis_path=vis)
    for i in range(n):
        raw = readPNG(os.path.join(out, "%06d_10.png" % i))
        assert raw.dtype == np.uint16 and np.array_equal(raw, R.kitti16(flows[i]))
        back, valid = readFlowKITTI(os.path.join(out, "%06d_10.png" % i))
        assert np.abs(back - flows[i]).max() < 1 / 64 and np.all(valid == 1)
        two_part(readPNG(os.path.join(vis, "flow", "%d.png" % i)), R.to_image(flows[i]), f"kitti vis {i}")


def test_sintel_submission_vis_writes_the_flow_and_the_picture(tmp_path):
    from flow_supervisor_amd import evaluate as EV
    from flow_supervisor_amd.raft_utils.frame_utils import readFlow, readPNG
    H, W = 37, 61
    frames = [("ambush_1", 0), ("ambush_1", 1), ("cave_3", 0)]
    preds, flows = padded_predictions(len(frames), H, W, "sintel", 42)
    ds = [(torch.zeros(3, H, W), torch.zeros(3, H, W), f) for f in frames]
    out, vis = str(tmp_path / "sub"), str(tmp_path / "vis")
    EV.create_sintel_submission_vis(ReplayModel(preds), ds, output_path=out, vis_path=vis)
    for i, (seq, frame) in enumerate(frames):
        assert np.array_equal(readFlow(os.path.join(out, seq, "frame%04d.flo" % (frame + 1))), flows[i])
        two_part(readPNG(os.path.join(vis, "flow", "%d.png" % i)), R.to_image(flows[i]), f"sintel vis {i}")


@pytest.mark.parametrize("style", ["wheel", "hsv"])
def test_demo_writes_flow_and_picture_per_pair(tmp_path, style):
    from flow_supervisor_amd import evaluate as EV
    from flow_supervisor_amd.raft_utils.frame_utils import readFlow, readPNG
    H, W = 37, 61
    preds, flows = padded_predictions(2, H, W, "sintel", 43)
    names = EV.demo(ReplayModel(preds), [torch.zeros(3, H, W)] * 3, str(tmp_path), style=style)
    assert names == ["000000", "000001"]
    assert sorted(os.listdir(str(tmp_path / "flo"))) == ["000000_flow.flo", "000001_flow.flo"]
    assert sorted(os.listdir(str(tmp_path / "vis"))) == ["000000_flow.png", "000001_flow.png"]
    for i in range(2):
        assert np.array_equal(readFlow(str(tmp_path / "flo" / ("%06d_flow.flo" % i))), flows[i])
        want = R.to_image(flows[i]) if style == "wheel" else R.hsv_u8(flows[i])
        two_part(readPNG(str(tmp_path / "vis" / ("%06d_flow.png" % i))), want, f"demo {style} {i}")


def test_demo_reads_a_directory_of_frames(tmp_path):
    from flow_supervisor_amd import evaluate as EV
    from flow_supervisor_amd.raft_utils.frame_utils import writePNG
    H, W = 37, 61
    src = tmp_path / "frames"
    src.mkdir()
    for k, nm in enumerate(["b_0002", "a_0001", "c_0003"]):            # taken in sorted order
        writePNG(str(src / (nm + ".png")), np.full((H, W, 3), 40 * k, np.uint8))
    preds, _ = padded_predictions(2, H, W, "sintel", 44)
    seen = []

    class Model(ReplayModel):
        def __call__(self, image1, image2, **kw):
            assert bool((image1 == image1[0, 0, 0, 0]).all()) and bool((image2 == image2[0, 0, 0, 0]).all())
            seen.append((float(image1[0, 0, 0, 0]), float(image2[0, 0, 0, 0])))
            return super().__call__(image1, image2, **kw)

    assert EV.demo(Model(preds), str(src), str(tmp_path / "out")) == ["a_0001", "b_0002"]
    assert seen == [(40.0, 0.0), (0.0, 80.0)]
    assert sorted(os.listdir(str(tmp_path / "out" / "vis"))) == ["a_0001_flow.png", "b_0002_flow.png"]


def test_validate_sintel_occ_and_things(capsys):
    from flow_supervisor_amd import evaluate as EV
    H, W, n = 37, 61, 3
    want, datasets, preds_all = {}, {}, []
    for k, dstype in enumerate(["clean", "final"]):
        preds, flows = padded_predictions(n, H, W, "sintel", 50 + k)
        g = torch.Generator().manual_seed(60 + k)
        gt = T(flows).permute(0, 3, 1, 2) + torch.randn(n, 2, H, W, generator=g) * 2.0
        occ = torch.rand(n, H, W, generator=g) < 0.3
        if dstype == "final":
            occ[:] = False                                             # an empty occluded region: its mean is NaN
        pred = T(flows).permute(0, 3, 1, 2)
        stats = [E.dataset_values(E.batch_stats(pred, gt, v)) if v is None or v.any() else None
                 for v in (None, occ.float(), (~occ).float())]
        want[dstype] = stats
        datasets[dstype] = [(torch.zeros(3, H, W), torch.zeros(3, H, W), gt[i], torch.ones(H, W), occ[i], "path%d" % i) for i in range(n)]
        preds_all.append(preds)
    for bs in (1, 3):
        res = EV.validate_sintel_occ(ReplayModel(torch.cat(preds_all)), datasets, batch_size=bs)
        out = capsys.readouterr().out
        assert list(res) == ["clean", "final"]
        for dstype, (a, o, noc) in want.items():
            assert abs(res[dstype] - a["epe"]) <= 1e-9 * a["epe"]
            assert "Validation (%s) EPE: %f, 1px: %f, 3px: %f, 5px: %f" % (dstype, res[dstype], a["1px"], a["3px"], a["5px"]) in out
        for (dstype, (a, o, noc)), m in zip(want.items(), re.findall(r"Occ epe: (\S+), Noc epe: (\S+)", out)):
            got_occ, got_noc = float(m[0]), float(m[1])                # printed with %f: six decimals
            assert (np.isnan(got_occ) if o is None else abs(got_occ - o["epe"]) <= 1e-6) and abs(got_noc - noc["epe"]) <= 1e-6
        assert out.count("Occ epe: ") == 2 and "Occ epe: nan" in out
    things = {"frames_cleanpass": [s[:4] for s in datasets["clean"]], "frames_finalpass": [s[:4] for s in datasets["final"]]}
    res = EV.validate_things(ReplayModel(torch.cat(preds_all)), things)
    out = capsys.readouterr().out
    assert list(res) == ["frames_cleanpass", "frames_finalpass"] and out.count("Dataset length 3") == 2
    for name, dstype in (("frames_cleanpass", "clean"), ("frames_finalpass", "final")):
        a = want[dstype][0]
        assert abs(res[name] - a["epe"]) <= 1e-9 * a["epe"]
        assert "Validation (%s) EPE: %f, 1px: %f, 3px: %f, 5px: %f" % (name, res[name], a["1px"], a["3px"], a["5px"]) in out
