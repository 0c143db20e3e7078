"""GPU checks of the augmentation kernels (csrc/augment.hip, flow_supervisor_amd/augment.py) against the float64 restatement
(tests/_augref.py, pinned in test_augref.py), through the C entry point on guarded, NaN-patterned buffers and through the
Python surface.  Flow, valid and the frames of samples that are not resized are copies, one multiply and sign flips: they equal
the fp32 twin bit for bit.  Resized frames and augmented crops lie within _augref.limits(), four times the twin's worst error
over these same cases, in units of 2^-24 * max|ref|.  The nearest-neighbour index is a decision; under the input condition
(test_augref.py) fp32 and fp64 take the same one."""
import pytest
import torch

import _augref as R
from _util import Buf, _log_margin

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = R.cases()
NAMES = [c["name"] for c in CASES]
OUTPUTS = ("frame1", "frame2", "frame_flow", "frame_valid", "crop1", "crop2", "crop_flow", "crop_valid")
BYTE = 0xA5


class ByteBuf:
    """A uint8 input between two guard rows of 256 bytes, one byte off any alignment."""

    def __init__(self, src):
        self.n, self.src = src.numel(), src.reshape(-1).clone()
        self.whole = torch.full((self.n + 513,), BYTE, dtype=torch.uint8, device=DEV)
        self.mid = self.whole[257:257 + self.n]
        self.mid.copy_(self.src)

    def unchanged(self):
        w = self.whole.cpu()
        assert bool((w[:257] == BYTE).all()) and bool((w[257 + self.n:] == BYTE).all()), "a guard row was written"
        assert torch.equal(w[257:257 + self.n], self.src), "an input was written"


class FloatIn:
    def __init__(self, src):
        self.src = src.reshape(-1).clone()
        self.buf = Buf(src=src)
        self.mid = self.buf.mid

    def unchanged(self):
        self.buf.intact()
        assert torch.equal(self.buf.cpu().view(torch.int32), self.src.view(torch.int32)), "an input was written"


def aug_params(case):
    from flow_supervisor_amd.augment import AugParams
    return [AugParams(**p) for p in case["params"]]


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return all(torch.equal(bits(a[k]), bits(b[k])) for k in a)


def run_case(case):
    """The entry point on one case, every output in a NaN-patterned guarded buffer -> dict of CPU tensors."""
    from flow_supervisor_amd import _lib
    from flow_supervisor_amd.augment import pack_params
    L = _lib.load()
    p0 = case["params"][0]
    B, (Hs, Ws), (Hf, Wf), (h, w) = len(case["params"]), p0["src_hw"], p0["full_hw"], p0["crop_hw"]
    wrap = ByteBuf if case["kind"] == "u8" else FloatIn
    img1, img2 = wrap(case["image1"]), wrap(case["image2"])
    flow = FloatIn(case["flow"])
    valid = FloatIn(case["valid"]) if case["valid"] is not None else None
    shapes = dict(frame1=(B, 3, Hf, Wf), frame2=(B, 3, Hf, Wf), frame_flow=(B, 2, Hf, Wf), frame_valid=(B, 1, Hf, Wf),
                  crop1=(B, 3, h, w), crop2=(B, 3, h, w), crop_flow=(B, 2, h, w), crop_valid=(B, 1, h, w))
    outs = {k: Buf(n=B * s[1] * s[2] * s[3]) for k, s in shapes.items()}
    nbytes = L.fsraft_augment_scratch_bytes(B, Hf, Wf, h, w)
    assert nbytes != 1 and nbytes % 64 == 0
    scratch = Buf(n=nbytes // 4)
    P = _lib.ptr
    _lib.check(L.fsraft_augment(P(img1.mid), P(img2.mid), 0 if case["kind"] == "u8" else 1, P(flow.mid), P(valid.mid) if valid else None,
                                B, Hs, Ws, pack_params(aug_params(case)), Hf, Wf, h, w, *[P(outs[k].mid) for k in OUTPUTS],
                                P(scratch.mid), nbytes, _lib.stream()), "augment")
    torch.cuda.synchronize()
    scratch.intact()
    for k in OUTPUTS:
        outs[k].written()
    for t in (img1, img2, flow, valid):
        if t is not None:
            t.unchanged()
    return {k: outs[k].cpu().view(shapes[k]) for k in OUTPUTS}


def check_field(got, ref, quantity, what):
    err, lim = R.field_error(got.cpu(), ref), R.limits()[quantity]
    _log_margin(what, err, lim, f"units of 2^-24 * max|ref| {float(ref.abs().max()):.3g}; twin {R.twin_errors()[quantity]:.4g}")
    assert torch.isfinite(got).all() and err <= lim, f"{what}: {err:.4g} > {lim:.4g}"


def check_against_restatement(case, i, got, tag=""):
    ref, twin, name = R.reference(i), R.twin(i), case["name"] + tag
    for k in R.EXACT:
        assert torch.equal(bits(got[k]), bits(twin[k])), f"{name} {k}: {int((bits(got[k]) != bits(twin[k])).sum())} elements differ"
    for b, p in enumerate(case["params"]):
        for k in R.QUANTITIES["frame"]:
            if p.get("resize"):
                check_field(got[k][b], ref[k][b], "frame", f"{name} {k}[{b}]")
            else:
                assert torch.equal(bits(got[k][b]), bits(twin[k][b])), f"{name} {k}[{b}]: a copy differs"
        for k in R.QUANTITIES["crop"]:
            check_field(got[k][b], ref[k][b], "crop", f"{name} {k}[{b}]")
    for k in ("crop1", "crop2", "frame1", "frame2"):
        assert float(got[k].min()) >= 0.0 and float(got[k].max()) <= 255.0
    assert set(got["frame_valid"].unique().tolist()) <= {0.0, 1.0}


@pytest.mark.parametrize("i", range(len(CASES)), ids=NAMES)
def test_entry_point_matches_the_restatement(i):
    case = CASES[i]
    got = run_case(case)
    check_against_restatement(case, i, got)
    # a second launch gives the same bits
    assert same_bits(got, run_case(case))


def on_device(case):
    return [None if case[k] is None else case[k].to(DEV) for k in ("image1", "image2", "flow", "valid")]


def as_outputs(out):
    """apply()'s dict under the keys of the entry point's outputs."""
    return dict(frame1=out["original_img"][0], frame2=out["original_img"][1], frame_flow=out["original_flows"],
                frame_valid=out["original_valids"], crop1=out["augmented_img"][0], crop2=out["augmented_img"][1],
                crop_flow=out["flows"], crop_valid=out["valids"])


@pytest.mark.parametrize("name", ["resize-flips-asym-2rect-u8", "batch3-f32", "blocks-u8"])
def test_python_surface_matches_the_restatement(name):
    from flow_supervisor_amd import augment as A
    i = NAMES.index(name)
    case = CASES[i]
    p0 = case["params"][0]
    B, (Hf, Wf), (h, w) = len(case["params"]), p0["full_hw"], p0["crop_hw"]
    out = A.apply(*on_device(case), aug_params(case))
    assert set(out) == {"original_img", "augmented_img", "flows", "valids", "original_flows", "original_valids", "crop_x", "crop_y"}
    assert out["crop_x"] == [p.get("crop_x", 0) for p in case["params"]] and out["crop_y"] == [p.get("crop_y", 0) for p in case["params"]]
    got = as_outputs(out)
    for k, shape in (("frame1", (B, 3, Hf, Wf)), ("frame_flow", (B, 2, Hf, Wf)), ("frame_valid", (B, 1, Hf, Wf)), ("crop2", (B, 3, h, w)),
                     ("crop_flow", (B, 2, h, w)), ("crop_valid", (B, 1, h, w))):
        assert got[k].shape == shape and got[k].dtype == torch.float32 and got[k].is_contiguous() and got[k].is_cuda
    check_against_restatement(case, i, {k: v.cpu() for k, v in got.items()}, " A.apply")
    step = A.as_step_input(out)
    assert len(step) == 8 and step[0] is out["augmented_img"][0] and step[3] is out["original_img"][1]
    assert step[4] == out["crop_x"] and step[5] == out["crop_y"] and step[6] is out["flows"] and step[7].shape == (B, h, w)


def test_a_missing_valid_map_is_all_ones():
    from flow_supervisor_amd import augment as A
    case = CASES[NAMES.index("resize-hflip-f32")]
    assert case["valid"] is None
    out = A.apply(*on_device(case), aug_params(case))
    assert bool((out["valids"] == 1).all()) and bool((out["original_valids"] == 1).all())


def test_call_under_a_seed_is_sample_then_apply():
    from flow_supervisor_amd import augment as A
    case = CASES[NAMES.index("batch3-u8")]
    img1, img2, flow, valid = on_device(case)
    aug = A.UnsupAugmentor((16, 24), do_flip=True, eraser_aug_prob=0.9)
    x, y = aug(img1, img2, flow, valid, generator=torch.Generator().manual_seed(31))
    assert set(x) == {"augmented_img", "original_img", "crop_x", "crop_y"} and set(y) == {"flows", "original_flows", "valids", "original_valids"}
    g = torch.Generator().manual_seed(31)
    params = [aug.sample((37, 53), g) for _ in range(3)]
    assert len({(p.win_y, p.win_x, p.crop_y, p.crop_x, p.colour) for p in params}) == 3
    want = A.apply(img1, img2, flow, valid, params)
    assert same_bits(as_outputs({**x, **y}), as_outputs(want))
    assert x["crop_x"] == want["crop_x"] == [p.crop_x for p in params] and x["crop_y"] == [p.crop_y for p in params]
    noisy = A.add_noise(x["augmented_img"], 3.0)
    assert len(noisy) == 2 and noisy[0].shape == x["augmented_img"][0].shape and float(noisy[0].min()) >= 0.0 and float(noisy[1].max()) <= 255.0
    assert not torch.equal(noisy[0], x["augmented_img"][0])
    assert torch.equal(A.add_noise(x["augmented_img"], 0.0)[1], x["augmented_img"][1])


@pytest.mark.parametrize("kind", R.DTYPES)
def test_identity_colour_leaves_the_frames_window(kind):
    """With a ColorJitter of zero ranges and no eraser the crops are the frames' windows -- to rounding: x / 255 * 255 and the
    two RGB -> HSV -> RGB trips are the identity in exact arithmetic only, in the restatement as in TF.  The bound is the crops'
    limit."""
    from flow_supervisor_amd import augment as A
    case = CASES[NAMES.index("batch3-" + kind)]
    aug = A.UnsupAugmentor((16, 24), do_flip=True, eraser_aug_prob=0.0)
    aug.photo_aug = A.ColorJitter(0.0, 0.0, 0.0, 0.0)
    g = torch.Generator().manual_seed(77)
    x, y = aug(*on_device(case), generator=g)
    for b, (cy, cx) in enumerate(zip(x["crop_y"], x["crop_x"])):
        for crop, frame in zip(x["augmented_img"], x["original_img"]):
            check_field(crop[b].cpu(), frame[b, :, cy:cy + 16, cx:cx + 24].cpu().double(), "crop", f"identity colour {kind} [{b}]")
        assert torch.equal(y["flows"][b], y["original_flows"][b, :, cy:cy + 16, cx:cx + 24])
        assert torch.equal(y["valids"][b], y["original_valids"][b, :, cy:cy + 16, cx:cx + 24])


def test_a_batch_replays_from_a_graph_on_refreshed_inputs():
    from flow_supervisor_amd import augment as A
    first = CASES[NAMES.index("blocks-u8")]
    params = aug_params(first)
    static = on_device(first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        before = as_outputs(A.apply(*static, params))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = as_outputs(A.apply(*static, params))
    # new inputs of the same shape, written in place
    g = torch.Generator().manual_seed(99)
    new = [torch.randint(0, 256, static[0].shape, generator=g, dtype=torch.uint8) for _ in range(2)]
    new += [torch.randn(static[2].shape, generator=g), (torch.rand(static[3].shape, generator=g) > 0.5).float()]
    for dst, src in zip(static, new):
        dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    replayed = {k: v.clone() for k, v in captured.items()}
    del graph
    eager = as_outputs(A.apply(*[t.to(DEV) for t in new], params))
    assert same_bits(replayed, eager)
    assert not torch.equal(eager["crop1"], before["crop1"]) and not torch.equal(eager["frame_flow"], before["frame_flow"])
