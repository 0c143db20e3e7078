"""GPU checks of the supervised augmentors' kernels (fsraft_augment_sup in csrc/augment.hip, FlowAugmentor / SparseFlowAugmentor in
flow_supervisor_amd/augment.py) against the float64 restatement (tests/_supaugref.py, pinned in test_supaugref.py), through the
C entry point on guarded, NaN-patterned buffers and through the Python surface.  Nearest-mode flow and valid, and flow and
valid of every sample that is not resized, are copies, one multiply and sign flips: they equal the fp32 twin bit for bit.  Images
and bilinear flow lie within _supaugref.limits(), four times the twin's worst error over these same cases, in units of
2^-24 * max|ref|.  The nearest-neighbour index is a decision; under the input condition (test_supaugref.py) fp32 and fp64 take
the same one."""
import pytest
import torch

import _supaugref as R
from _util import Buf, _log_margin
from test_augment_gpu import ByteBuf, FloatIn, aug_params, bits, same_bits      # the guarded inputs (uint8 one byte off any alignment)

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = R.cases()
NAMES = [c["name"] for c in CASES]
OUTPUTS = ("crop1", "crop2", "crop_flow", "crop_valid")
FLOW_MODES = {"dense": 0, "sparse": 1}


def run_case(case):
    """The entry point on one case, every output in a NaN-patterned guarded buffer -> dict of CPU tensors."""
    from flow_supervisor_amd import _lib
    from flow_supervisor_amd.augment import pack_params
    L = _lib.load()
    p0 = case["params"][0]
    B, (Hs, Ws), (h, w) = len(case["params"]), p0["src_hw"], p0["crop_hw"]
    wrap = ByteBuf if case["kind"] == "u8" else FloatIn
    img1, img2 = wrap(case["image1"]), wrap(case["image2"])
    flow = FloatIn(case["flow"])
    valid = FloatIn(case["valid"]) if case["valid"] is not None else None
    shapes = dict(crop1=(B, 3, h, w), crop2=(B, 3, h, w), crop_flow=(B, 2, h, w), crop_valid=(B, 1, h, w))
    outs = {k: Buf(n=B * s[1] * s[2] * s[3]) for k, s in shapes.items()}
    nbytes = L.fsraft_augment_sup_scratch_bytes(B, Hs, Ws)
    assert nbytes != 1 and nbytes % 64 == 0
    scratch = Buf(n=nbytes // 4)
    P = _lib.ptr
    _lib.check(L.fsraft_augment_sup(P(img1.mid), P(img2.mid), 0 if case["kind"] == "u8" else 1, P(flow.mid), P(valid.mid) if valid else None,
                                    FLOW_MODES[case["mode"]], B, Hs, Ws, pack_params(aug_params(case)), h, w,
                                    *[P(outs[k].mid) for k in OUTPUTS], P(scratch.mid), nbytes, _lib.stream()), "augment_sup")
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
    assert torch.equal(bits(got["crop_valid"]), bits(twin["crop_valid"])), f"{name} crop_valid"
    for b in range(len(case["params"])):
        for k in R.IMAGES:
            check_field(got[k][b], ref[k][b], "image", f"{name} {k}[{b}]")
        if R.bilinear_flow(case, b):
            check_field(got["crop_flow"][b], ref["crop_flow"][b], "flow", f"{name} crop_flow[{b}]")
        else:
            differ = int((bits(got["crop_flow"][b]) != bits(twin["crop_flow"][b])).sum())
            assert differ == 0, f"{name} crop_flow[{b}]: {differ} elements differ from the twin's bits"
    for k in R.IMAGES:
        assert float(got[k].min()) >= 0.0 and float(got[k].max()) <= 255.0
    if case["mode"] == "dense":
        assert bool((got["crop_valid"] == 1).all())                           # whatever valid map was given
    else:
        assert set(got["crop_valid"].unique().tolist()) <= {0.0, 1.0}


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
    """apply_supervised()'s dict under the keys of the entry point's outputs."""
    return dict(crop1=out["image1"], crop2=out["image2"], crop_flow=out["flow"], crop_valid=out["valid"])


@pytest.mark.parametrize("name", ["flips-2rect-dense-u8", "batch3-dense-f32", "fallback-dense-u8", "batch3-sparse-u8", "blocks-sparse-f32"])
def test_python_surface_matches_the_restatement(name):
    from flow_supervisor_amd import augment as A
    i = NAMES.index(name)
    case = CASES[i]
    B, (h, w) = len(case["params"]), case["params"][0]["crop_hw"]
    out = A.apply_supervised(*on_device(case), aug_params(case), case["mode"] == "dense")
    assert set(out) == {"image1", "image2", "flow", "valid"}
    got = as_outputs(out)
    for k, shape in (("crop1", (B, 3, h, w)), ("crop2", (B, 3, h, w)), ("crop_flow", (B, 2, h, w)), ("crop_valid", (B, 1, h, w))):
        assert got[k].shape == shape and got[k].dtype == torch.float32 and got[k].is_contiguous() and got[k].is_cuda
    check_against_restatement(case, i, {k: v.cpu() for k, v in got.items()}, " A.apply_supervised")


def test_a_missing_valid_map_is_all_ones():
    from flow_supervisor_amd import augment as A
    case = CASES[NAMES.index("up-hflip-sparse-f32")]
    assert case["valid"] is None
    assert bool((A.apply_supervised(*on_device(case), aug_params(case), False)["valid"] == 1).all())


@pytest.mark.parametrize("dense", [True, False])
def test_call_under_a_seed_is_sample_then_apply(dense):
    from flow_supervisor_amd import augment as A
    case = CASES[NAMES.index("batch3-dense-u8" if dense else "batch3-sparse-u8")]
    img1, img2, flow, valid = on_device(case)
    aug = (A.FlowAugmentor if dense else A.SparseFlowAugmentor)((16, 24), do_flip=True, eraser_aug_prob=0.9)
    got = aug(img1, img2, flow, valid, generator=torch.Generator().manual_seed(31))
    assert isinstance(got, tuple) and len(got) == 4
    assert got[0].shape == got[1].shape == (3, 3, 16, 24) and got[2].shape == (3, 2, 16, 24) and got[3].shape == (3, 1, 16, 24)
    g = torch.Generator().manual_seed(31)
    params = [aug.sample((37, 53), g) for _ in range(3)]
    assert len({(p.t_h, p.t_w, p.crop_y, p.crop_x, p.colour) for p in params}) == 3
    want = A.apply_supervised(img1, img2, flow, valid, params, dense)
    assert same_bits(dict(zip(OUTPUTS, got)), as_outputs(want))
    if dense:
        # valid is optional for the dense class, and ignored
        again = aug(img1, img2, flow, generator=torch.Generator().manual_seed(31))
        assert same_bits(dict(zip(OUTPUTS, got)), dict(zip(OUTPUTS, again)))


@pytest.mark.parametrize("dense", [True, False])
@pytest.mark.parametrize("kind", R.DTYPES)
def test_identity_parameters_give_the_source_window(kind, dense):
    """With the identity jitter, no eraser and no resize the images are the source's window times 255 -- to rounding: x / 255 *
    255 and the two RGB -> HSV -> RGB trips are the identity in exact arithmetic only, in the restatement as in TF; the bound is
    the images' limit -- and flow and valid are the window exactly."""
    from flow_supervisor_amd import augment as A
    case = CASES[NAMES.index(f"batch3-{'dense' if dense else 'sparse'}-{kind}")]
    img1, img2, flow, valid = on_device(case)
    params = [A.identity_params((37, 53), (37, 53), (16, 24), crop_y=y, crop_x=x, hflip=b == 1) for b, (y, x) in enumerate(((0, 0), (21, 29), (7, 13)))]
    out = A.apply_supervised(img1, img2, flow, valid, params, dense)
    unit = 1.0 if kind == "u8" else 255.0
    for b, p in enumerate(params):
        x0 = 53 - 24 - p.crop_x if p.hflip else p.crop_x                      # (the offset is counted in the flipped image)
        win = (b, slice(p.crop_y, p.crop_y + 16), slice(x0, x0 + 24))
        flip = (lambda t: t.flip(-1)) if p.hflip else (lambda t: t)
        for k, src in (("image1", img1), ("image2", img2)):
            check_field(out[k][b].cpu(), flip(src[win].permute(2, 0, 1).double().cpu() * unit), "image", f"identity {kind} {k}[{b}]")
        sign = torch.tensor([-1.0 if p.hflip else 1.0, 1.0], device=DEV)[:, None, None]
        assert torch.equal(out["flow"][b], flip(flow[win].permute(2, 0, 1)) * sign)
        assert torch.equal(out["valid"][b, 0], torch.ones(16, 24, device=DEV) if dense else flip(valid[win]))


def test_a_batch_replays_from_a_graph_on_refreshed_inputs():
    from flow_supervisor_amd import augment as A
    first = CASES[NAMES.index("blocks-sparse-u8")]
    params = aug_params(first)
    static = on_device(first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        before = as_outputs(A.apply_supervised(*static, params, False))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = as_outputs(A.apply_supervised(*static, params, False))
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
    eager = as_outputs(A.apply_supervised(*[t.to(DEV) for t in new], params, False))
    assert same_bits(replayed, eager)
    assert not torch.equal(eager["crop1"], before["crop1"]) and not torch.equal(eager["crop_flow"], before["crop_flow"])
