"""A restatement in plain torch of the parts of the reference's SMURF loss that csrc/selfsup_loss.hip computes
(raft/smurf_models/smurf_utils.py compute_occlusions_brox :432-453, self_supervision_loss :735-829, and their place in
unsupervised_loss / unsupervised_sequence_loss as raft/unsup_loss.py calls them: selfsup_mask 'gaussian', fb_sigma_teacher
0.003, fb_sigma_student 0.03, the transform a plain crop).  PyTorch layout, flows [B,2,H,W] with channel 0 = x.  The
reference's TensorFlow does not run here, so this file is the oracle; it computes in the dtype of its inputs -- float64 is the
reference, float32 the twin that rounds every operation and gives the limits -- and takes its gradients from autograd.  The
resampler, the crop and the case generators are _unsupref's.
"""
import functools

import torch

import _unsupref as U
from _unsupref import FACTOR, coords, crop, field_error, make_flow, resample, scalar_error, smooth_field

REF_SIGMAS = (0.003, 0.03)        # (teacher, student): smurf_utils.py unsupervised_loss defaults
WIDE_SIGMAS = (0.01, 0.01)        # at these small frames the reference's teacher sigma leaves a mask of almost zero everywhere
MODES = (("g", "gaussian", REF_SIGMAS), ("w", "gaussian", WIDE_SIGMAS), ("d", "ddflow", REF_SIGMAS), ("n", "none", REF_SIGMAS))


# ------------------------------------------------------------------------------------------------------------- the loss
def normaliser(sigma, hw):
    """sigma^2 * (h^2 + w^2), :792-795; (h, w) is the TEACHER flow's size for both masks (:767-768)."""
    return float(sigma) ** 2 * (float(hw[0]) ** 2 + float(hw[1]) ** 2)


def fb_quantities(f, g):
    """(sq, ss, valid), [B,H,W] each, of the pair (f, g) over its own H x W image."""
    H, W = f.shape[-2:]
    sx, sy = coords(f)
    r = resample(g, sx, sy)
    sq = ((f + r) ** 2).sum(1)
    ss = (f ** 2 + r ** 2).sum(1)
    valid = ((sx >= 0) & (sx <= W - 1) & (sy >= 0) & (sy <= H - 1)).to(f.dtype)
    return sq, ss, valid


def threshold(ss):
    return 0.01 * ss + 0.5


def fb_mask(f, g, kind, norm=None, crop_yx=None, hw=None, complement=False):
    """c * valid of the pair (1 - that with `complement`), computed on the pair's image and then cropped: [B,H,W]."""
    f, g = f.detach(), g.detach()
    sq, ss, valid = fb_quantities(f, g)
    c = torch.exp(-sq / norm) if kind == "gaussian" else (sq < threshold(ss)).to(f.dtype)
    m = c * valid
    if crop_yx is not None:
        m = crop(m.unsqueeze(1), crop_yx, *hw)[:, 0]
    return 1.0 - m if complement else m


def brox_mask(f, g, crop_yx=None, hw=None):
    """compute_occlusions(f, g, 'brox', occlusions_are_zeros=True, boundaries_occluded=True): 1 = visible, [B,H,W]."""
    sq, ss, _ = fb_quantities(f.detach(), g.detach())
    m = 1.0 - (sq > threshold(ss)).to(f.dtype)
    return m if crop_yx is None else crop(m.unsqueeze(1), crop_yx, *hw)[:, 0]


def selfsup_parts(T, Tb, S, Sb, crop_yx=None, mask="gaussian", sigma_teacher=REF_SIGMAS[0], sigma_student=REF_SIGMAS[1]):
    """self_supervision_loss -> (loss, m [B,H,W]); the gradient goes to S only."""
    H, W = S.shape[-2:]
    hw = T.shape[-2:]
    if mask == "none":
        m = torch.ones_like(S[:, 0])
    else:
        student = fb_mask(S, Sb, mask, normaliser(sigma_student, hw), complement=True)
        teacher = fb_mask(T, Tb, mask, normaliser(sigma_teacher, hw), crop_yx, (H, W))
        m = (teacher * student).detach()
    err = ((crop(T, crop_yx, H, W).detach() - S) ** 2 + 0.001 ** 2) ** 0.5
    return (m.unsqueeze(1) * err).mean(), m


def selfsup_loss(*args, **kwargs):
    return selfsup_parts(*args, **kwargs)[0]


def smurf_loss(frames, flows_fw, flows_bw, teacher, crop_yx=None, census=1.0, smooth1=2.5, smooth2=0.0, selfsup=0.3, occlusion="wang",
               gamma=0.8, selfsup_mask="gaussian", sigmas=REF_SIGMAS):
    """UnsupervisedLoss.call with every term -> (loss, dict of the weighted terms); teacher = (fw, bw), the last predictions."""
    w = {k: v for k, v in (("census", census), ("smooth1", smooth1), ("smooth2", smooth2), ("selfsup", selfsup)) if v > 0}
    H, W = flows_fw[0].shape[-2:]
    imgs = [crop(f, crop_yx, H, W) for f in frames]
    total = {}
    for ffw, fbw in zip(flows_fw, flows_bw):
        one = {k: 0.0 for k in w}
        for i, j, f, g in ((0, 1, ffw, fbw), (1, 0, fbw, ffw)):
            if "census" in w:
                occ = brox_mask(f, g) if occlusion == "brox" else U.occlusion_mask(g.detach(), occlusion)
                one["census"] = one["census"] + w["census"] * U.census_loss(frames[i], frames[j], f, occ, crop_yx) / 2.0
            for k, order in (("smooth1", 1), ("smooth2", 2)):
                if k in w:
                    one[k] = one[k] + w[k] * U.smoothness_loss(imgs[i], f, order) / 2.0
            if "selfsup" in w:
                one["selfsup"] = one["selfsup"] + w["selfsup"] * selfsup_loss(teacher[i], teacher[j], f, g, crop_yx, selfsup_mask, *sigmas) / 2.0
        for k, v in one.items():                                       # add_loss_dicts
            total[k] = v + total[k] * gamma if k in total else v
    return sum(total.values()), total


# ------------------------------------------------------------------------------------------------------------ the cases
SHAPES = (                       # (B, H, W, frame or None, crop_yx or None)
    (1, 1, 1, None, None),       # a single pixel
    (1, 1, 70, None, None),      # a row wider than a wave
    (2, 37, 61, None, None),     # odd sizes
    (1, 70, 130, None, None),    # more than one block
    (3, 24, 40, (48, 80), ((0, 0), (24, 40), (5, 7))),     # windows of full frames, one flush bottom-right
    (1, 520, 520, None, None),   # more pixels than one pass of the grid covers (1024 blocks of 256)
)
FAMILIES = ("zero", "integer", "consistent", "independent", "allout")
INTEGER_FAMILIES = ("zero", "integer", "allout")


def bad_pixels(f, g):
    """[B,H,W]: the pixels of the pair at which fp32 and fp64 may take different decisions: a warp coordinate within 1e-3 px of
    a validity bound or within 1e-5 px of an integer (a floor), or sq within a relative 1e-4 of the ddflow / brox threshold."""
    f, g = f.double(), g.double()
    H, W = f.shape[-2:]
    sx, sy = coords(f)
    bad = torch.zeros_like(sx, dtype=torch.bool)
    for s, hi in ((sx, W - 1), (sy, H - 1)):
        bad |= ((s - 0.0).abs() < 1e-3) | ((s - hi).abs() < 1e-3) | ((s - torch.round(s)).abs() < 1e-5)
    sq, ss, _ = fb_quantities(f, g)
    thr = threshold(ss)
    return bad | ((sq - thr).abs() < 1e-4 * thr)


def make_pair(g, family, B, H, W):
    """(f, g) of one family over an H x W image, fp32."""
    if family in INTEGER_FAMILIES:
        f = make_flow(g, family, B, H, W, H, W)
        return f, (-f if family == "integer" else f.clone()).contiguous()
    jitter = 0.02 * (torch.rand(B, 2, H, W, generator=g, dtype=torch.float64) - 0.5)
    if family == "consistent":       # back = -forward plus smooth noise of up to 0.8 px a component: sq on both sides of 0.5
        f = make_flow(g, "subpixel", B, H, W, H, W).double()
        back = -f + 1.6 * (smooth_field(g, B, 2, H, W) - 0.5) + jitter
    else:                            # "independent": two unrelated fields of up to 3 px a component
        f = 6.0 * (smooth_field(g, B, 2, H, W) - 0.5) + jitter
        back = 6.0 * (smooth_field(g, B, 2, H, W) - 0.5)
    f, back = f.float().contiguous(), back.float().contiguous()
    # a pixel that sits on a decision is moved off it, a few times over: at 520 x 520 a draw without one is too rare to wait for
    for _ in range(8):
        bad = bad_pixels(f, back)
        if not bad.any():
            break
        f = f + 0.0137 * bad.unsqueeze(1).float()
    return f, back


def input_conditions(case):
    """Share of pixels of the case's two pairs that break a condition of bad_pixels(); the integer-valued families sit on the
    conditions on purpose and count as 0."""
    if case["family"] in INTEGER_FAMILIES:
        return 0.0
    bad = sum(int(bad_pixels(case[a], case[b]).sum()) for a, b in (("T", "Tb"), ("S", "Sb")))
    return bad / (case["T"][:, 0].numel() + case["S"][:, 0].numel())


@functools.lru_cache(maxsize=None)
def cases():
    """Every (shape, family) case of the GPU tests: the teacher's pair (T, Tb) on the frame, the student's (S, Sb) on the window,
    fp32, regenerated from the seed until input_conditions() is 0."""
    out = []
    for si, (B, H, W, frame, crop_yx) in enumerate(SHAPES):
        Hf, Wf = frame or (H, W)
        for fi, family in enumerate(FAMILIES):
            for attempt in range(200):
                g = torch.Generator().manual_seed(52000 + 1000 * si + 200 * fi + attempt)
                case = dict(name=f"{B}x{H}x{W}{'in%dx%d' % (Hf, Wf) if frame else ''}-{family}", family=family, B=B, H=H, W=W, crop_yx=crop_yx)
                case["T"], case["Tb"] = make_pair(g, family, B, Hf, Wf)
                case["S"], case["Sb"] = make_pair(g, family, B, H, W)
                if input_conditions(case) == 0.0:
                    break
            out.append(case)
    return out


OCCLUSIONS = ("wang", "brox", "none")


@functools.lru_cache(maxsize=None)
def sequence_case():
    """SmurfLoss's case: 3 predictions per direction at 2x37x61, windows of 50x80 frames, a teacher of the frames' size, all four
    weights > 0.  The census term's input conditions (_unsupref) and this file's hold for every pair."""
    B, H, W, Hf, Wf = 2, 37, 61, 50, 80
    fam = ("subpixel", "fold", "large")
    for attempt in range(200):
        g = torch.Generator().manual_seed(8800 + attempt)
        sc = dict(frames=(U.make_image(g, B, Hf, Wf), U.make_image(g, B, Hf, Wf)), crop_yx=((13, 19), (4, 0)),
                  fw=[make_flow(g, k, B, H, W, Hf, Wf) for k in fam], bw=[make_flow(g, k, B, H, W, Hf, Wf) for k in fam],
                  weights=dict(census=1.0, smooth1=2.5, smooth2=0.7, selfsup=0.3), sigmas=WIDE_SIGMAS)
        sc["teacher"] = make_pair(g, "consistent", B, Hf, Wf)
        ok = all(U.input_conditions(dict(family=k, frames=sc["frames"], crop_yx=sc["crop_yx"], flow=a, flow_bw=b)) == 0.0
                 for k, a, b in zip(fam, sc["fw"], sc["bw"]))
        pairs = list(zip(sc["fw"], sc["bw"])) + list(zip(sc["bw"], sc["fw"])) + [sc["teacher"], sc["teacher"][::-1]]
        if ok and not any(bool(bad_pixels(a, b).any()) for a, b in pairs):
            break
    return sc


def evaluate(case, dtype):
    """Every quantity the GPU tests compare, of one case, computed in `dtype`."""
    T, Tb, Sb = (case[k].to(dtype) for k in ("T", "Tb", "Sb"))
    S = case["S"].to(dtype).requires_grad_(True)
    crop_yx, hw = case["crop_yx"], (case["H"], case["W"])
    out = {"tbrox": brox_mask(T, Tb, crop_yx, hw), "sbrox": brox_mask(S, Sb)}
    for tag, kind, (st, ss) in MODES:
        if kind != "none":
            out["tmask_" + tag] = fb_mask(T, Tb, kind, normaliser(st, T.shape[-2:]), crop_yx, hw)
            out["smask_" + tag] = fb_mask(S, Sb, kind, normaliser(ss, T.shape[-2:]), complement=True)
        loss, m = selfsup_parts(T, Tb, S, Sb, crop_yx, kind, st, ss)
        out["loss_" + tag], out["m_" + tag], out["dflow_" + tag] = loss.detach(), m, torch.autograd.grad(loss, S)[0]
    return out


def evaluate_sequence(sc, occlusion, dtype):
    fw = [t.to(dtype).requires_grad_(True) for t in sc["fw"]]
    bw = [t.to(dtype).requires_grad_(True) for t in sc["bw"]]
    loss, terms = smurf_loss([t.to(dtype) for t in sc["frames"]], fw, bw, [t.to(dtype) for t in sc["teacher"]], sc["crop_yx"],
                             occlusion=occlusion, sigmas=sc["sigmas"], **sc["weights"])
    grads = torch.autograd.grad(loss, fw + bw)
    return dict(loss=loss.detach(), terms={k: v.detach() for k, v in terms.items()}, grads=grads)


@functools.lru_cache(maxsize=None)
def reference(i):
    return evaluate(cases()[i], torch.float64)


@functools.lru_cache(maxsize=None)
def reference_sequence(occlusion):
    return evaluate_sequence(sequence_case(), occlusion, torch.float64)


DECISIONS = ("tbrox", "sbrox", "tmask_d", "smask_d")       # equal to the fp64 ones bit for bit under the input conditions
QUANTITIES = {                   # quantity -> (keys of evaluate(), error measure)
    "mask": (("tmask_g", "tmask_w", "smask_g", "smask_w"), field_error),
    "loss": (tuple("loss_" + m[0] for m in MODES), scalar_error),
    "dflow": (tuple("dflow_" + m[0] for m in MODES), field_error),
}


@functools.lru_cache(maxsize=None)
def twin_errors():
    """The fp32 twin's worst error against fp64 over the GPU cases, per quantity (fields: units of 2^-24 * max|ref|)."""
    worst = {q: 0.0 for q in QUANTITIES}
    for i, case in enumerate(cases()):
        ref, twin = reference(i), evaluate(case, torch.float32)
        for q, (keys, measure) in QUANTITIES.items():
            worst[q] = max([worst[q]] + [measure(twin[k], ref[k]) for k in keys])
    worst["sequence"], worst["sequence_dflow"] = 0.0, 0.0
    for occlusion in OCCLUSIONS:
        ref, twin = reference_sequence(occlusion), evaluate_sequence(sequence_case(), occlusion, torch.float32)
        worst["sequence"] = max([worst["sequence"], scalar_error(twin["loss"], ref["loss"])]
                                + [scalar_error(twin["terms"][k], ref["terms"][k]) for k in ref["terms"]])
        worst["sequence_dflow"] = max([worst["sequence_dflow"]] + [field_error(a, b) for a, b in zip(twin["grads"], ref["grads"])])
    return worst


def limits():
    """FACTOR times the twin's worst error, per quantity."""
    return {q: FACTOR * e for q, e in twin_errors().items()}
