"""GPU checks of the unsupervised loss (csrc/unsup_loss.hip, flow_supervisor_amd/unsup_loss.py) against the float64 restatement
of the reference (tests/_unsupref.py, pinned in test_unsupref.py), through the C entry points on guarded buffers and through
the Python surface.  Limits: _unsupref.limits(), four times the fp32 twin's worst error over these same cases (fields in
units of 2^-24 * max|ref|, scalars relative).

The census gradient reaches a pixel through every patch it lies in, so a pixel outside the mask or on the 3-pixel border has a
gradient whenever one of its 7 x 7 neighbours is inside the mask (the restatement's autograd says the same,
test_unsupref.py::test_autograd_gradient_against_central_differences).  The exact-zero check is therefore on the pixels none of
whose neighbours has M != 0, and on the saved plane h wherever M = 0."""
import argparse
import ctypes

import pytest
import torch
import torch.nn.functional as F

import _unsupref as R
from _util import Buf, _log_margin

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = R.cases()
NAMES = [c["name"] for c in CASES]
SMOOTH = (("smooth1e", 1, 0), ("smooth1g", 1, 1), ("smooth2e", 2, 0), ("smooth2g", 2, 1))


def check_field(got, ref, quantity, what):
    err, lim = R.field_error(got.cpu(), ref), R.limits()[quantity]
    _log_margin(what, err, lim, f"units of 2^-24 * max|ref| {float(ref.abs().max()):.3g}; twin {R.twin_errors()[quantity]:.4g}")
    assert torch.isfinite(got).all() and err <= lim, f"{what}: {err:.4g} > {lim:.4g}"


def check_scalar(got, ref, quantity, what):
    err, lim = R.scalar_error(got, ref), R.limits()[quantity]
    _log_margin(what, err, lim, f"relative to |ref| {abs(float(ref)):.6g}; twin {R.twin_errors()[quantity]:.4g}")
    assert err <= lim, f"{what}: {float(got)!r} vs {float(ref)!r}, rel {err:.3g} > {lim:.3g}"


class Strided:
    """A [B,C,H,W] input as a view with a row pitch of W + 3, one row and one column into a guarded buffer whose padding is NaN."""

    def __init__(self, t):
        B, C, H, W = t.shape
        padded = torch.full((B, C, H + 2, W + 3), float("nan"))
        padded[:, :, 1:1 + H, 1:1 + W] = t
        self.buf, self.before = Buf(src=padded), padded.view(torch.int32).clone()
        self.view = self.buf.mid.view(B, C, H + 2, W + 3)[:, :, 1:1 + H, 1:1 + W]
        assert not self.view.is_contiguous() and self.view.stride(2) == W + 3

    def unchanged(self):
        self.buf.intact()
        assert torch.equal(self.buf.cpu().view(torch.int32), self.before.view(-1)), "an input was written"


def crop_array(crop_yx):
    if crop_yx is None:
        return None
    return (ctypes.c_int * (2 * len(crop_yx)))(*[v for pair in crop_yx for v in pair])


def run_case(case, ref, samples=None, den=None):
    """Every entry point on one case (or on its samples `samples`), outputs in NaN-patterned guarded buffers.  -> dict of CPU
    tensors.  den: the denominator the census backward divides by (default: the forward's own)."""
    from flow_supervisor_amd import _lib
    L = _lib.load()
    sel = slice(None) if samples is None else samples
    crop_yx = None if case["crop_yx"] is None else case["crop_yx"][sel]
    f1, f2, flow, flow_bw = (Strided(t[sel]) for t in (*case["frames"], case["flow"], case["flow_bw"]))
    mask = Buf(src=ref["mask"][sel].float().contiguous())
    B, _, H, W = flow.view.shape
    Hf, Wf = f1.view.shape[-2:]
    S, crop, P = _lib.stream(), crop_array(crop_yx), _lib.ptr
    out = {}

    def scratch(fn):
        n = fn(B, H, W)
        assert n != 1 and n % 8 == 0
        return Buf(n=n // 4), n

    rm, (sc, nbytes) = Buf(n=B * H * W), scratch(L.fsraft_range_map_scratch_bytes)
    for clip, key in ((0, "range_map"), (1, "mask")):
        _lib.check(L.fsraft_range_map(P(flow_bw.view), *flow_bw.view.stride()[:3], B, H, W, clip, P(rm.mid), P(sc.mid), nbytes, S), key)
        rm.written()
        out[key] = rm.cpu().view(B, H, W)
    sc.intact()

    gB, hp, dflow = Buf(n=B * H * W), Buf(n=B * H * W), Buf(n=2 * B * H * W)
    res, up = Buf(n=4), Buf(src=torch.ones(1))
    sc, nbytes = scratch(L.fsraft_census_scratch_bytes)
    views = (P(f1.view), *f1.view.stride()[:3], 1, P(f2.view), *f2.view.stride()[:3], Hf, Wf, crop, P(flow.view), *flow.view.stride()[:3])
    _lib.check(L.fsraft_census_fwd(*views, P(mask.mid), H * W, W, B, H, W, P(gB.mid), P(hp.mid), P(res.mid), P(sc.mid), nbytes, S), "fwd")
    for b in (gB, hp, res, sc):
        b.intact()
    gB.written(), hp.written()
    loss_den = res.mid.view(torch.float64).cpu()
    out["census"], out["den"], out["grayB"], out["h"] = loss_den[0], loss_den[1], gB.cpu().view(B, H, W), hp.cpu().view(B, H, W)
    if den is not None:
        res.mid.view(torch.float64)[1] = den
    _lib.check(L.fsraft_census_bwd(*views, P(gB.mid), P(hp.mid), P(up.mid), ctypes.c_void_p(res.mid.data_ptr() + 8), B, H, W,
                                   P(dflow.mid), S), "bwd")
    dflow.written()
    out["census_dflow"] = dflow.cpu().view(B, 2, H, W)

    sc, nbytes = scratch(L.fsraft_smoothness_scratch_bytes)
    for key, order, gaussian in SMOOTH:
        dflow, res = Buf(n=2 * B * H * W), Buf(n=2)
        _lib.check(L.fsraft_smoothness(P(f1.view), *f1.view.stride()[:3], Hf, Wf, crop, P(flow.view), *flow.view.stride()[:3], B, H, W,
                                       order, 150.0, gaussian, P(dflow.mid), P(res.mid), P(sc.mid), nbytes, S), key)
        dflow.written(), res.intact(), sc.intact()
        out[key], out[key + "_dflow"] = res.mid.view(torch.float64).cpu()[0], dflow.cpu().view(B, 2, H, W)
    for t in (f1, f2, flow, flow_bw):
        t.unchanged()
    mask.intact()
    return out


def same_bits(a, b):
    return all(torch.equal(a[k].contiguous().view(torch.int32 if a[k].dtype == torch.float32 else torch.int64),
                           b[k].contiguous().view(torch.int32 if b[k].dtype == torch.float32 else torch.int64)) for k in a)


@pytest.mark.parametrize("i", range(len(CASES)), ids=NAMES)
def test_entry_points_match_the_restatement(i):
    case, ref = CASES[i], R.reference(i)
    got = run_case(case, ref)
    name = case["name"]
    check_field(got["range_map"], ref["range_map"], "range_map", f"{name} range map")
    check_field(got["mask"], ref["mask"], "range_map", f"{name} clipped range map")
    assert float(got["mask"].max()) <= 1.0 and float(got["mask"].min()) >= 0.0
    check_scalar(got["census"], ref["census"], "census", f"{name} census")
    check_field(got["census_dflow"], ref["census_dflow"], "census_dflow", f"{name} census dflow")
    for key, _, _ in SMOOTH:
        check_scalar(got[key], ref[key], "smoothness", f"{name} {key}")
        check_field(got[key + "_dflow"], ref[key + "_dflow"], "smoothness_dflow", f"{name} {key} dflow")
    # exact: h is zero bits wherever M = 0 (border, mask, invalid warp); dflow is zero bits wherever no neighbour has M != 0
    _, M, _ = R.census_parts(case["frames"][0].double(), case["frames"][1].double(), case["flow"].double(), ref["mask"], case["crop_yx"])
    zero_h = got["h"].view(torch.int32)[M == 0]
    assert not zero_h.any() and (got["h"][M != 0] > 0).all()
    reach = F.max_pool2d((M != 0).float().unsqueeze(1), 7, stride=1, padding=3)
    untouched = (reach == 0).expand(-1, 2, -1, -1)
    assert not got["census_dflow"].view(torch.int32)[untouched].any()
    assert not ref["census_dflow"][untouched].any()
    if case["family"] == "allout":
        assert float(got["den"]) == 1e-6 * M.numel() and got["census"].view(torch.int64).item() == 0
        assert not got["census_dflow"].view(torch.int32).any()
    if case["family"] in ("zero", "integer"):        # exact weights: the fixed-point sum is the float64 one
        assert torch.equal(got["range_map"].double(), ref["range_map"])
    # a second launch gives the same bits
    assert same_bits(got, run_case(case, ref))


@pytest.mark.parametrize("name", [n for n in NAMES if n[0] in "23" and n.split("-")[1] in ("subpixel", "fold")])
def test_a_sample_gives_the_bits_it_gives_alone(name):
    i = NAMES.index(name)
    case, ref = CASES[i], R.reference(i)
    batch = run_case(case, ref)
    for b in range(case["B"]):
        alone = run_case(case, ref, slice(b, b + 1), den=float(batch["den"]))
        for k in ("range_map", "mask", "grayB", "h", "census_dflow"):
            assert torch.equal(alone[k][0].view(torch.int32), batch[k][b].view(torch.int32)), (k, b)


@pytest.mark.parametrize("name", ["2x37x61-subpixel", "3x24x40in48x80-fold", "1x7x8-large"])
def test_python_surface_matches_the_restatement(name):
    from flow_supervisor_amd import unsup_loss as U
    i = NAMES.index(name)
    case, ref = CASES[i], R.reference(i)
    H, W, crop_yx = case["H"], case["W"], case["crop_yx"]
    frames = [Strided(t).view for t in case["frames"]]
    flow_bw = Strided(case["flow_bw"]).view
    rm = U.range_map(flow_bw)
    mask = U.occlusion_mask(flow_bw)
    assert rm.shape == mask.shape == (case["B"], 1, H, W) and not mask.requires_grad
    check_field(rm[:, 0], ref["range_map"], "range_map", f"{name} U.range_map")
    check_field(mask[:, 0], ref["mask"], "range_map", f"{name} U.occlusion_mask")
    assert torch.equal(U.occlusion_mask(flow_bw, "none"), torch.ones_like(mask))
    flow = Strided(case["flow"]).view.detach().requires_grad_(True)
    full = dict(full_image2=frames[1], crop_yx=crop_yx) if crop_yx is not None else {}
    img1 = frames[0] if crop_yx is None else R.crop(frames[0], crop_yx, H, W)
    loss = U.census_loss(img1, None if crop_yx is not None else frames[1], flow, ref["mask"].float().to(DEV).unsqueeze(1), **full)
    assert loss.shape == () and loss.dtype == torch.float32
    (3.0 * loss).backward()
    assert flow.is_leaf and flow.grad is not None
    check_scalar(loss.detach(), ref["census"], "census", f"{name} U.census_loss")
    check_field(flow.grad, 3.0 * ref["census_dflow"], "census_dflow", f"{name} U.census_loss grad")
    if crop_yx is not None:                              # the window of image 1's frame read in place gives the same bits
        again = U.census_loss(None, None, flow, ref["mask"].float().to(DEV), full_image1=frames[0], **full)
        assert torch.equal(again, loss)
    for key, order, gaussian in SMOOTH:
        flow.grad = None
        v = U.smoothness_loss(img1, flow, order, 150.0, "gaussian" if gaussian else "exponential")
        (0.5 * v).backward()
        check_scalar(v.detach(), ref[key], "smoothness", f"{name} U.smoothness_loss {key}")
        check_field(flow.grad, 0.5 * ref[key + "_dflow"], "smoothness_dflow", f"{name} U.smoothness_loss {key} grad")


def sequence_on_device():
    sc = R.sequence_case()
    frames = [Strided(t).view for t in sc["frames"]]
    fw = [Strided(t).view.detach().requires_grad_(True) for t in sc["fw"]]
    bw = [Strided(t).view.detach().requires_grad_(True) for t in sc["bw"]]
    return sc, frames, fw, bw


def test_unsupervised_loss_matches_the_restatement():
    from flow_supervisor_amd.unsup_loss import UnsupervisedLoss
    sc, frames, fw, bw = sequence_on_device()
    ref = R.reference_sequence()
    fn = UnsupervisedLoss(**sc["weights"])
    loss, terms = fn(None, fw, bw, full_images=frames, crop_yx=torch.tensor(sc["crop_yx"]))
    loss.backward()
    check_scalar(loss.detach(), ref["loss"], "sequence", "UnsupervisedLoss loss")
    for k, v in ref["terms"].items():
        check_scalar(terms[k], v, "sequence", f"UnsupervisedLoss {k}")
    for t, (g, r) in enumerate(zip([f.grad for f in fw + bw], ref["grads"])):
        check_field(g, r, "sequence_dflow", f"UnsupervisedLoss grad {t}")
    # gamma: the sequence loss is the decayed sum of the three single-prediction losses.  Both sides add the same 18 non-negative
    # fp32 terms (3 predictions x 2 directions x 3 parts), each product and sum rounding once: at most ~64 * 2^-24 apart.
    singles = [float(fn(None, [a], [b], full_images=frames, crop_yx=sc["crop_yx"])[0]) for a, b in zip(fw, bw)]
    want = sum(0.8 ** (2 - t) * v for t, v in enumerate(singles))
    assert abs(float(loss) - want) <= 64 * 2.0 ** -24 * want, (float(loss), want)
    # without the frames: the images themselves, every mask from the range map, 'none' for all ones
    imgs = [R.crop(f, sc["crop_yx"], 37, 61) for f in frames]
    for occlusion in ("wang", "none"):
        got, _ = UnsupervisedLoss(occlusion=occlusion)(imgs, [f.detach() for f in fw[:1]], [b.detach() for b in bw[:1]])
        want, _ = R.unsup_loss([t.double().cpu() for t in imgs], [sc["fw"][0].double()], [sc["bw"][0].double()], occlusion=occlusion)
        check_scalar(got, want, "sequence", f"UnsupervisedLoss on the images, occlusion {occlusion}")


def test_raft_small_trains_on_the_unsupervised_loss():
    """The wiring: raft-small on 2 pairs of 64x96 fed as a batch of 4 (both directions), 2 iterations."""
    from flow_supervisor_amd.core.raft import RAFT
    from flow_supervisor_amd.unsup_loss import UnsupervisedLoss
    torch.manual_seed(0)
    model = RAFT(argparse.Namespace(small=True, mixed_precision=False, alternate_corr=False)).to(DEV).train()
    g = torch.Generator().manual_seed(5)
    im1, im2 = (R.make_image(g, 2, 64, 96).to(DEV) for _ in range(2))
    preds = model(255.0 * torch.cat([im1, im2]), 255.0 * torch.cat([im2, im1]), iters=2)
    assert len(preds) == 2 and preds[0].shape == (4, 2, 64, 96)
    loss, _ = UnsupervisedLoss()((im1, im2), [p[:2] for p in preds], [p[2:] for p in preds])
    loss.backward()
    params = [(k, p) for k, p in model.named_parameters() if k.startswith("update_block.")]
    assert params
    for k, p in params:
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, k
    cpu = [p.detach().double().cpu() for p in preds]
    want, _ = R.unsup_loss([im1.double().cpu(), im2.double().cpu()], [p[:2] for p in cpu], [p[2:] for p in cpu], smooth1=2.5)
    check_scalar(loss.detach(), want, "sequence", "raft-small unsupervised loss")


def test_forward_and_backward_replay_from_one_graph():
    from flow_supervisor_amd.unsup_loss import UnsupervisedLoss
    sc, frames, fw, bw = sequence_on_device()
    fn = UnsupervisedLoss(**sc["weights"])
    crop_yx = sc["crop_yx"]

    def step(a, b):
        loss, _ = fn(None, a, b, full_images=frames, crop_yx=crop_yx)
        return (loss, *torch.autograd.grad(loss, a + b))

    static_fw = [t.detach().clone().requires_grad_(True) for t in fw[:2]]
    static_bw = [t.detach().clone().requires_grad_(True) for t in bw[:2]]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(static_fw, static_bw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = step(static_fw, static_bw)
    new_fw, new_bw = [fw[2].detach(), fw[0].detach()], [bw[2].detach(), bw[0].detach()]
    with torch.no_grad():
        for dst, src in zip(static_fw + static_bw, new_fw + new_bw):
            dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in captured]
    del graph
    eager = step([t.clone().requires_grad_(True) for t in new_fw], [t.clone().requires_grad_(True) for t in new_bw])
    for a, b in zip(replayed, eager):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert float(eager[0]) > 0 and all(float(t.abs().max()) > 0 for t in eager[1:])
