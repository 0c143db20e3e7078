"""GPU checks of the forward-backward masks and the self-supervision term (csrc/selfsup_loss.hip,
flow_supervisor_amd/selfsup_loss.py) against the float64 restatement of the reference (tests/_selfsupref.py, pinned in
test_selfsupref.py), through the C entry points on guarded buffers and through the Python surface.  Limits:
_selfsupref.limits(), four times the fp32 twin's worst error over these same cases (fields in units of 2^-24 * max|ref|,
scalars relative).  The 'ddflow' and 'brox' masks are decisions and equal the float64 ones bit for bit under the input
conditions."""
import argparse
import ctypes

import pytest
import torch

import _selfsupref as R
import _unsupref as U
from _util import Buf, _log_margin

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = R.cases()
NAMES = [c["name"] for c in CASES]
FB = {"gaussian": 0, "ddflow": 1, "brox": 2, "none": 3}


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


def same_bits(a, b):
    return all(torch.equal(a[k].contiguous().view(torch.int32 if a[k].dtype == torch.float32 else torch.int64),
                           b[k].contiguous().view(torch.int32 if b[k].dtype == torch.float32 else torch.int64)) for k in a)


def check_field(got, ref, quantity, what):
    err, lim = R.field_error(got.cpu(), ref), R.limits()[quantity]
    _log_margin(what, err, lim, f"units of 2^-24 * max|ref| {float(ref.abs().max()):.3g}; twin {R.twin_errors()[quantity]:.4g}")
    assert torch.isfinite(got).all() and err <= lim, f"{what}: {err:.4g} > {lim:.4g}"


def check_scalar(got, ref, quantity, what):
    err, lim = R.scalar_error(got, ref), R.limits()[quantity]
    _log_margin(what, err, lim, f"relative to |ref| {abs(float(ref)):.6g}; twin {R.twin_errors()[quantity]:.4g}")
    assert err <= lim, f"{what}: {float(got)!r} vs {float(ref)!r}, rel {err:.3g} > {lim:.3g}"


def run_case(case, samples=None):
    """Every entry point on one case (or on its samples `samples`), outputs in NaN-patterned guarded buffers.  -> dict of CPU
    tensors under the keys of _selfsupref.evaluate()."""
    from flow_supervisor_amd import _lib
    L = _lib.load()
    sel = slice(None) if samples is None else samples
    crop_yx = None if case["crop_yx"] is None else case["crop_yx"][sel]
    T, Tb, S, Sb = (Strided(case[k][sel]) for k in ("T", "Tb", "S", "Sb"))
    B, _, H, W = S.view.shape
    Hf, Wf = T.view.shape[-2:]
    stream, crop, P = _lib.stream(), crop_array(crop_yx), _lib.ptr
    out = {}

    def fb_mask(pair, Hi, Wi, crop, mode, complement, norm):
        f, g = pair
        o = Buf(n=B * H * W)
        _lib.check(L.fsraft_fb_mask(P(f.view), *f.view.stride()[:3], P(g.view), *g.view.stride()[:3], Hi, Wi, crop, B, H, W, FB[mode],
                                    complement, norm, P(o.mid), stream), "fb_mask")
        o.written()
        return o

    out["tbrox"] = fb_mask((T, Tb), Hf, Wf, crop, "brox", 0, 1.0).cpu().view(B, H, W)
    out["sbrox"] = fb_mask((S, Sb), H, W, None, "brox", 1, 1.0).cpu().view(B, H, W)         # (complement has no say in 'brox')
    nbytes = L.fsraft_selfsup_scratch_bytes(B, H, W)
    assert nbytes != 1 and nbytes % 8 == 0
    scratch = Buf(n=nbytes // 4)
    for tag, kind, (st, ss) in R.MODES:
        nt, ns = R.normaliser(st, (Hf, Wf)), R.normaliser(ss, (Hf, Wf))
        tmask = None
        if kind != "none":
            tmask = fb_mask((T, Tb), Hf, Wf, crop, kind, 0, nt)
            out["tmask_" + tag] = tmask.cpu().view(B, H, W)
            out["smask_" + tag] = fb_mask((S, Sb), H, W, None, kind, 1, ns).cpu().view(B, H, W)
        dflow, res = Buf(n=2 * B * H * W), Buf(n=2)
        _lib.check(L.fsraft_selfsup(P(T.view), *T.view.stride()[:3], Hf, Wf, crop, P(tmask.mid) if tmask is not None else None, H * W, W,
                                    P(S.view), *S.view.stride()[:3], P(Sb.view), *Sb.view.stride()[:3], B, H, W, FB[kind], ns,
                                    P(dflow.mid), P(res.mid), P(scratch.mid), nbytes, stream), "selfsup " + kind)
        dflow.written(), res.intact(), scratch.intact()
        if tmask is not None:
            tmask.intact()
            assert torch.equal(tmask.cpu().view(B, H, W), out["tmask_" + tag]), "the teacher's mask was written"
        out["loss_" + tag], out["dflow_" + tag] = res.mid.view(torch.float64).cpu()[0], dflow.cpu().view(B, 2, H, W)
    for t in (T, Tb, S, Sb):
        t.unchanged()
    return out


@pytest.mark.parametrize("i", range(len(CASES)), ids=NAMES)
def test_entry_points_match_the_restatement(i):
    case, ref = CASES[i], R.reference(i)
    got = run_case(case)
    name = case["name"]
    for key in R.DECISIONS:
        assert torch.equal(got[key].double(), ref[key]), f"{name} {key}: {int((got[key].double() != ref[key]).sum())} decisions differ"
    for key in R.QUANTITIES["mask"][0]:
        check_field(got[key], ref[key], "mask", f"{name} {key}")
        assert float(got[key].min()) >= 0.0 and float(got[key].max()) <= 1.0
    for tag, _, _ in R.MODES:
        check_scalar(got["loss_" + tag], ref["loss_" + tag], "loss", f"{name} loss {tag}")
        check_field(got["dflow_" + tag], ref["dflow_" + tag], "dflow", f"{name} dflow {tag}")
        # exact: +0.0 wherever the reference's m is zero
        masked = (ref["m_" + tag] == 0).unsqueeze(1).expand(-1, 2, -1, -1)
        assert not got["dflow_" + tag].view(torch.int32)[masked].any()
        if case["family"] in ("zero", "allout") and tag != "n":
            assert got["loss_" + tag].view(torch.int64).item() == 0 and not got["dflow_" + tag].view(torch.int32).any()
    # a second launch gives the same bits
    assert same_bits(got, run_case(case))


@pytest.mark.parametrize("name", [n for n in NAMES if n[0] in "23" and n.split("-")[1] in ("consistent", "independent")])
def test_a_sample_gives_the_bits_it_gives_alone(name):
    case = CASES[NAMES.index(name)]
    batch = run_case(case)
    for b in range(case["B"]):
        alone = run_case(case, slice(b, b + 1))
        for k in batch:
            if k.startswith("loss_"):
                continue
            # dflow carries 1 / (2 H W) / B, divided in that order: the sample alone (B = 1), divided by the batch's B
            want = alone[k][0] / case["B"] if k.startswith("dflow_") else alone[k][0]
            assert torch.equal(want.view(torch.int32), batch[k][b].view(torch.int32)), (k, b)


@pytest.mark.parametrize("name", ["2x37x61-consistent", "3x24x40in48x80-independent", "1x1x70-consistent"])
def test_python_surface_matches_the_restatement(name):
    from flow_supervisor_amd import selfsup_loss as M
    i = NAMES.index(name)
    case, ref = CASES[i], R.reference(i)
    B, H, W, crop_yx = case["B"], case["H"], case["W"], case["crop_yx"]
    T, Tb, Sb = (Strided(case[k]).view for k in ("T", "Tb", "Sb"))
    S = Strided(case["S"]).view.detach().requires_grad_(True)
    window = dict(crop_yx=crop_yx, window_hw=(H, W)) if crop_yx is not None else {}
    brox = M.brox_occlusion_mask(S, Sb)
    assert brox.shape == (B, 1, H, W) and not brox.requires_grad
    assert torch.equal(brox[:, 0].cpu().double(), ref["sbrox"])
    for tag, kind, (st, ss) in R.MODES[:3]:
        tm = M.fb_consistency_mask(T, Tb, kind, st, **window)
        sm = M.fb_consistency_mask(S, Sb, kind, ss, frame_hw=T.shape[-2:], complement=True)
        assert tm.shape == sm.shape == (B, 1, H, W) and not sm.requires_grad
        if kind == "ddflow":
            assert torch.equal(tm[:, 0].cpu().double(), ref["tmask_d"]) and torch.equal(sm[:, 0].cpu().double(), ref["smask_d"])
        else:
            check_field(tm[:, 0], ref["tmask_" + tag], "mask", f"{name} M.fb_consistency_mask teacher {tag}")
            check_field(sm[:, 0], ref["smask_" + tag], "mask", f"{name} M.fb_consistency_mask student {tag}")
    for tag, kind, (st, ss) in R.MODES:
        S.grad = None
        loss = M.self_supervision_loss(T, Tb, S, Sb, crop_yx, kind, st, ss)
        assert loss.shape == () and loss.dtype == torch.float32
        (3.0 * loss).backward()
        assert S.is_leaf and S.grad is not None
        check_scalar(loss.detach(), ref["loss_" + tag], "loss", f"{name} M.self_supervision_loss {tag}")
        check_field(S.grad, 3.0 * ref["dflow_" + tag], "dflow", f"{name} M.self_supervision_loss {tag} grad")
    if crop_yx is not None:
        with pytest.raises(ValueError, match="student's size"):
            M.self_supervision_loss(T, Tb, S, Sb)


def sequence_on_device():
    sc = R.sequence_case()
    frames = [Strided(t).view for t in sc["frames"]]
    fw = [Strided(t).view.detach().requires_grad_(True) for t in sc["fw"]]
    bw = [Strided(t).view.detach().requires_grad_(True) for t in sc["bw"]]
    teacher = [Strided(t).view for t in sc["teacher"]]
    return sc, frames, fw, bw, teacher


def smurf(sc, **kwargs):
    from flow_supervisor_amd.selfsup_loss import SmurfLoss
    return SmurfLoss(**sc["weights"], fb_sigma_teacher=sc["sigmas"][0], fb_sigma_student=sc["sigmas"][1], **kwargs)


@pytest.mark.parametrize("occlusion", R.OCCLUSIONS)
def test_smurf_loss_matches_the_restatement(occlusion):
    sc, frames, fw, bw, teacher = sequence_on_device()
    ref = R.reference_sequence(occlusion)
    fn = smurf(sc, occlusion=occlusion)
    loss, terms = fn(None, fw, bw, *teacher, full_images=frames, crop_yx=torch.tensor(sc["crop_yx"]))
    loss.backward()
    check_scalar(loss.detach(), ref["loss"], "sequence", f"SmurfLoss {occlusion} loss")
    assert set(terms) == {"census", "smooth1", "smooth2", "selfsup"}
    for k, v in ref["terms"].items():
        check_scalar(terms[k], v, "sequence", f"SmurfLoss {occlusion} {k}")
    for t, (g, r) in enumerate(zip([f.grad for f in fw + bw], ref["grads"])):
        check_field(g, r, "sequence_dflow", f"SmurfLoss {occlusion} grad {t}")
    # gamma: the sequence loss is the decayed sum of the three single-prediction losses, the teacher the same for each.  Both
    # sides add the same 24 non-negative fp32 terms (3 predictions x 2 directions x 4 parts), each product and sum rounding
    # once: at most ~64 * 2^-24 apart.
    singles = [float(fn(None, [a], [b], *teacher, full_images=frames, crop_yx=sc["crop_yx"])[0].detach()) for a, b in zip(fw, bw)]
    want = sum(0.8 ** (2 - t) * v for t, v in enumerate(singles))
    assert abs(float(loss.detach()) - want) <= 64 * 2.0 ** -24 * want, (float(loss.detach()), want)


def test_smurf_loss_without_selfsup_is_the_unsupervised_loss():
    from flow_supervisor_amd.selfsup_loss import SmurfLoss
    from flow_supervisor_amd.unsup_loss import UnsupervisedLoss
    sc, frames, fw, bw, teacher = sequence_on_device()
    weights = {k: v for k, v in sc["weights"].items() if k != "selfsup"}
    for occlusion in ("wang", "none"):
        results = []
        for fn, extra in ((UnsupervisedLoss(occlusion=occlusion, **weights), ()), (SmurfLoss(selfsup=0, occlusion=occlusion, **weights), teacher)):
            loss, terms = fn(None, fw, bw, *extra, full_images=frames, crop_yx=sc["crop_yx"])
            grads = torch.autograd.grad(loss, fw + bw)
            results.append([loss.detach()] + [terms[k] for k in ("census", "smooth1", "smooth2")] + list(grads))
        for a, b in zip(*results):
            assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
        assert float(terms["selfsup"]) == 0.0


def test_raft_small_trains_on_the_smurf_loss():
    """The wiring: raft-small on 2 pairs, the student on 64x96 crops of 80x112 frames fed as a batch of 4 (both directions),
    the teacher without a gradient on the frames, 2 iterations."""
    from flow_supervisor_amd.core.raft import RAFT
    from flow_supervisor_amd.selfsup_loss import SmurfLoss
    torch.manual_seed(0)
    model = RAFT(argparse.Namespace(small=True, mixed_precision=False, alternate_corr=False)).to(DEV).train()
    g = torch.Generator().manual_seed(5)
    fr1, fr2 = (U.make_image(g, 2, 80, 112).to(DEV) for _ in range(2))
    crop_yx = ((16, 8), (3, 16))
    im1, im2 = (U.crop(f, crop_yx, 64, 96).contiguous() for f in (fr1, fr2))
    with torch.no_grad():
        teacher = model(255.0 * torch.cat([fr1, fr2]), 255.0 * torch.cat([fr2, fr1]), iters=2)[-1]
    preds = model(255.0 * torch.cat([im1, im2]), 255.0 * torch.cat([im2, im1]), iters=2)
    assert len(preds) == 2 and preds[0].shape == (4, 2, 64, 96) and teacher.shape == (4, 2, 80, 112) and not teacher.requires_grad
    loss, terms = SmurfLoss()(None, [p[:2] for p in preds], [p[2:] for p in preds], teacher[:2], teacher[2:], full_images=(fr1, fr2),
                              crop_yx=crop_yx)
    loss.backward()
    assert float(terms["selfsup"]) > 0
    params = [(k, p) for k, p in model.named_parameters() if k.startswith("update_block.")]
    assert params
    for k, p in params:
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, k
    cpu = [p.detach().double().cpu() for p in preds]
    tc = teacher.double().cpu()
    want, _ = R.smurf_loss([fr1.double().cpu(), fr2.double().cpu()], [p[:2] for p in cpu], [p[2:] for p in cpu], (tc[:2], tc[2:]), crop_yx)
    check_scalar(loss.detach(), want, "sequence", "raft-small smurf loss")


def test_forward_and_backward_replay_from_one_graph():
    sc, frames, fw, bw, teacher = sequence_on_device()
    fn = smurf(sc, occlusion="brox")
    crop_yx = sc["crop_yx"]

    def step(a, b):
        loss, _ = fn(None, a, b, *teacher, full_images=frames, crop_yx=crop_yx)
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
