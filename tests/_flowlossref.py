"""float64 restatement of the flow losses of the reference's TensorFlow trainers -- raft/loss.py FlowLossL1 / FlowLossL2 /
FlowLossRobust (:4-93), the per-sample sums raft/metric.py EPE divides (:25-33) and the three flow terms of
Semisupervised.train_step (raft/semi.py:373-405, 447-471) -- in the form csrc/flow_loss.hip computes them, with the inputs that
make its routes visible, an fp32 twin and analytic error scales (tests/test_flowlossref.py on the CPU, tests/test_flow_loss_kernels.py
and tests/test_flow_loss_gpu.py against the kernel).  Plain torch on the CPU; flows are [B,H,W,2], masks [B,H,W].  TensorFlow is not
installed anywhere here: test_flowlossref.py holds the restatement to torch.autograd on the literal op sequence of raft/loss.py,
parity with TensorFlow itself is unpinned.

  m       = mask * (sqrt(t0^2 + t1^2) < max_flow)            the mask a float factor, the comparison strict (loss.py:25-29)
  psi(d)  = |d| (l1),  d^2 (l2),  sqrt(d^2 + eps^2) (robust), d = pred - target
  loss    = scale * sum_i w_i sum_{b,y,x,c} m psi(d)         scale 1 / (2 B H W): mean over the channel axis, then Keras'
                                                             SUM_OVER_BATCH_SIZE; 1 / 2: the sum of a Reduction.NONE map
  dpred_i = scale * w_i * m * psi'(d)                        sign(0) = 0
  stats   = (sum mask * |d|_2, sum mask) per sample of one prediction: without the cut (metric.py)
  pixel   = m * (psi(d_0) + psi(d_1)) / 2                    a single prediction: the Reduction.NONE value

Comparator: _tailref.need(got, ref, scale, slack) <= LIMITS[key], u = 2^-24, every scale elementwise:
  fl_loss   u * |scale| * sum_i |w_i| sum m psi(d): a sum of positive terms
  fl_dpred  u * |ref|: a chain of correctly rounded operations on d, itself one rounding of an exact difference
  fl_epe    u * sum mask * |d|_2        fl_pixel  u * |ref|
Exact (no limit): sum mask (the masks hold 0, 0.25 and 1: every partial sum is a multiple of 0.25 below 2^22), 0 where m == 0, 0 at d == 0 under l1, the pixel whose target has magnitude exactly 400.0 excluded.

The cut is decided in fp32 by the kernel and in float64 here.  Random targets are 4 N(0, 1), nowhere near 400; the designed
pixels hold (240, 320), exactly 400.0 in both, and (240, 319.999), 26 fp32 steps below it.

LIMITS are 4 x the worst value the fp32 TWIN (the same formulas, every operation rounded to fp32, in an order that is not the
kernel's: torch.sum over a whole prediction, predictions added one after the other, the scale applied last) reaches against
float64 over ALL_RUNS -- the very launches the two GPU files make -- rounded up to one significant digit (_tailref.limit_from_twin).
The kernel's own worst values are in profiles/flow_loss_margins.txt; they do not set the limits.
"""
import itertools

import torch

from _tailref import U24, _gen, limit_from_twin, need  # noqa: F401

MAX_FLOW = 400.0
EPS = 1e-3
PENALTIES = ("l1", "l2", "robust")
# the kernel's constants (csrc/flow_loss.hip FL_THREADS, FL_MAX_WG): a sample beyond 2048 x 256 pixels takes a second, strided trip
FL_THREADS, FL_MAX_WG = 256, 2048
BIG = (1, 513, 1024, 2)                  # 525312 = 2048 * 256 + 1024 pixels
CASES = ((1, 1, 1, 1), (2, 5, 7, 3), (1, 255, 1, 2), (1, 256, 1, 2), (1, 257, 1, 2), (2, 5, 7, 32), (3, 9, 31, 2), BIG)   # B, H, W, n
CROSSED = ((2, 5, 7, 3), (1, 257, 1, 2))
SURFACE = (2, 16, 24, 3)                 # tests/test_flow_loss_gpu.py
LAYOUTS = ("nhwc", "nchw")
OFFSETS = (0, 1, 2)                      # floats off the 16-byte alignment: 1 takes the 4-byte route, 2 keeps the 8-byte one
GT_FORMS = ("joint", "separate", "null_mask", "null_target")
LIVES = ("all", "mid_null", "none")
SCALES = ("mean", "sum")

TWIN_WORST = dict(fl_loss=2.18, fl_dpred=3.26, fl_epe=2.11, fl_pixel=3.71)
LIMITS = dict(fl_loss=9.0, fl_dpred=20.0, fl_epe=9.0, fl_pixel=20.0)


def scale_of(kind, B, H, W):
    return 1.0 / (2.0 * B * H * W) if kind == "mean" else 0.5


def live_list(kind, n):
    return [kind == "all" or (kind == "mid_null" and i != n // 2) for i in range(n)]


def inputs(B, H, W, n):
    """(preds [n][B,H,W,2], target [B,H,W,2], mask [B,H,W], w [n]) fp32.  The mask holds 0, 0.25 and 1.  With at least 8 pixels,
    sample 0 holds the designed pixels: 0 d == 0 on every prediction, 1 target (240, 320), magnitude exactly 400.0, 2 target
    (240, 319.999), just below, 3 mask 0, 4 mask 0.25, 5 d = (-1.5, -2)."""
    g = _gen(11, B, H, W, n)
    HW = H * W
    target = 4.0 * torch.randn(B, HW, 2, generator=g)
    mask = torch.tensor([0.0, 0.25, 1.0, 1.0])[torch.randint(0, 4, (B, HW), generator=g)]
    noise = [3.0 * torch.randn(B, HW, 2, generator=g) for _ in range(n)]
    if HW >= 8:
        target[0, 1] = torch.tensor([240.0, 320.0])
        target[0, 2] = torch.tensor([240.0, 319.999])
        mask[0, :6] = torch.tensor([1.0, 1.0, 1.0, 0.0, 0.25, 1.0])
        for d in noise:
            d[0, 0] = 0.0
            d[0, 5] = torch.tensor([-1.5, -2.0])
    else:
        mask[:] = 0.25
    preds = [(target + d).view(B, H, W, 2) for d in noise]
    if HW >= 8:
        assert all(torch.equal(p.view(B, HW, 2)[0, 0], target[0, 0]) for p in preds)
    w = torch.tensor([0.8 ** (n - i - 1) for i in range(n)], dtype=torch.float32)
    return preds, target.view(B, H, W, 2), mask.view(B, H, W), w


def _psi(d, penalty, eps):
    if penalty == "l1":
        return d.abs(), torch.sign(d)
    if penalty == "l2":
        return d * d, 2.0 * d
    s = (d * d + eps * eps).sqrt()
    return s, d / s


def flow_loss_ref(preds, w, target, mask, penalty, scale, live=None, metric_idx=None, max_flow=MAX_FLOW, eps=EPS, dtype=torch.float64):
    """dict(loss 0-d, dpred [n] (None where not live), stats [B,2] or None, pixel [B,H,W] of prediction 0, m [B,H,W]).  dtype
    float32: the twin."""
    B, H, W, _ = preds[0].shape
    n = len(preds)
    t = target.to(dtype) if target is not None else torch.zeros(B, H, W, 2, dtype=dtype)
    mk = mask.to(dtype) if mask is not None else torch.ones(B, H, W, dtype=dtype)
    if target is not None:
        inside = (t[..., 0] ** 2 + t[..., 1] ** 2).sqrt() < max_flow
    else:
        inside = torch.ones(B, H, W, dtype=torch.bool)
    m = mk * inside.to(dtype)
    live = [True] * n if live is None else live
    sc = torch.tensor(scale, dtype=dtype)
    total = torch.zeros((), dtype=dtype)
    dps, stats, pixel = [], None, None
    for i in range(n):
        d = preds[i].to(dtype) - t
        psi, dpsi = _psi(d, penalty, torch.tensor(eps, dtype=dtype))
        wi = w[i].to(dtype)
        total = total + wi * (psi * m[..., None]).sum()
        dps.append((dpsi * m[..., None]) * (wi * sc) if live[i] else None)
        if i == 0:
            pixel = m * ((psi[..., 0] + psi[..., 1]) / 2)
        if i == metric_idx:
            epe = (d[..., 0] ** 2 + d[..., 1] ** 2).sqrt()
            stats = torch.stack(((epe * mk).sum((1, 2)), mk.sum((1, 2))), 1)
    return dict(loss=total * sc, dpred=dps, stats=stats, pixel=pixel, m=m)


def expect(preds, w, target, mask, penalty, scale, live=None, metric_idx=None):
    """{loss: (ref, scale, 0, key), dpred: [entry or None], epe: entry or None, msum: the exact mask sums or None, pixel: entry, m: the weight map}."""
    r = flow_loss_ref(preds, w, target, mask, penalty, scale, live, metric_idx)
    pos = flow_loss_ref(preds, w.abs(), target, mask, penalty, abs(scale), [False] * len(preds))["loss"]
    out = dict(loss=(r["loss"], U24 * pos, 0.0, "fl_loss"), m=r["m"],
               dpred=[(d, U24 * d.abs(), 0.0, "fl_dpred") if d is not None else None for d in r["dpred"]],
               pixel=(r["pixel"], U24 * r["pixel"].abs(), 0.0, "fl_pixel"), epe=None, msum=None)
    if r["stats"] is not None:
        out["epe"] = (r["stats"][:, 0], U24 * r["stats"][:, 0], 0.0, "fl_epe")
        out["msum"] = r["stats"][:, 1]
    return out


def twin_needs(preds, w, target, mask, penalty, scale, live=None, metric_idx=None):
    """{key: need of the fp32 twin against the float64 restatement} on one launch."""
    exp = expect(preds, w, target, mask, penalty, scale, live, metric_idx)
    got = flow_loss_ref(preds, w, target, mask, penalty, scale, live, metric_idx, dtype=torch.float32)
    res = dict(fl_loss=need(got["loss"], *exp["loss"][:3])[0], fl_pixel=need(got["pixel"], *exp["pixel"][:3])[0], fl_dpred=0.0)
    for d, e in zip(got["dpred"], exp["dpred"]):
        if e is not None:
            res["fl_dpred"] = max(res["fl_dpred"], need(d, *e[:3])[0])
    if exp["epe"] is not None:
        res["fl_epe"] = need(got["stats"][:, 0], *exp["epe"][:3])[0]
        assert torch.equal(got["stats"][:, 1].double(), exp["msum"])
    return res


def launch_args(case, gt_form="joint", live="all", metric=True, scale="mean", single=False):
    """(preds, w, target or None, mask or None, scale, live list, metric_idx or None) of one launch of the GPU tests.  single: the
    first prediction alone under weight 1 (the per-pixel map, the Keras-shaped classes)."""
    B, H, W, n = case
    preds, target, mask, w = inputs(B, H, W, n)
    if single:
        preds, w, n = preds[:1], torch.ones(1), 1
    return (preds, w, None if gt_form == "null_target" else target, None if gt_form == "null_mask" else mask,
            scale_of(scale, B, H, W), live_list(live, n), (n - 1) if metric else None)


def crossed_variants():
    """(gt form, live, metric, scale) of the crossed cases: what the reference depends on (layout and base offset do not enter)."""
    return tuple(itertools.product(GT_FORMS, LIVES, (True, False), SCALES))


def all_runs():
    """Every launch_args tuple the GPU tests launch, per penalty."""
    runs = [(c, "joint", "all", True, "mean", c[3] == 1) for c in CASES]
    runs += [(c,) + v for c in CROSSED for v in crossed_variants()]
    runs += [(c, f, "all", True, s, True) for c in CROSSED for f in GT_FORMS for s in SCALES]
    runs += [(SURFACE, f, "all", True, s, single) for f in ("joint", "null_mask") for s in SCALES for single in (False, True)]
    return runs


# ------------------------------------------------------------------------------------------- the callers, as the reference writes them
def keras_loss_literal(y_true, y_pred, penalty, reduction="mean"):
    """raft/loss.py:8-31 / 38-61 / 67-93 op for op (torch for tf), then Keras' reduction of the [B,H,W] map."""
    if isinstance(y_true, torch.Tensor) and y_true.shape[-1] == 3:
        mask = y_true[..., 2:3]
        y_true = y_true[..., 0:2]
    elif isinstance(y_true, (list, tuple)):
        if len(y_true) == 2:
            y_true, mask = y_true
        else:
            y_true = y_true[0]
            mask = torch.ones_like(y_true)[..., 0:1]
    else:
        mask = torch.ones_like(y_true)[..., 0:1]
    y_true = y_true.to(y_pred.dtype)
    mask = mask.to(y_pred.dtype)
    if mask.dim() == 3:
        mask = mask[..., None]
    mag = torch.sqrt(torch.sum(y_true ** 2, dim=-1, keepdim=True))
    valid = mag < 400
    diff = y_pred - y_true
    if penalty == "l1":
        a = torch.abs(diff) * mask * valid.to(mask.dtype)
    elif penalty == "l2":
        a = torch.square(diff) * mask * valid.to(mask.dtype)
    else:
        a = (diff ** 2 + 0.001 ** 2) ** 0.5
        a = a * mask * valid.to(mask.dtype)
    loss = torch.mean(a, dim=3)
    if reduction == "none":
        return loss
    return loss.sum() / loss.numel() if reduction == "mean" else loss.sum()


def epe_metric_literal(updates):
    """raft/metric.py:8-40 over a list of (flow, mask, y_pred) updates in float64: the mean of the per-sample results."""
    results = []
    for flow, mask, y_pred in updates:
        mask = mask.double()[..., None]
        diff = y_pred.double() - flow.double()
        epes = torch.sqrt(torch.sum(torch.square(diff), dim=-1, keepdim=True)) * mask
        values = epes.sum((1, 2, 3))
        results.append(torch.full_like(values, -1.0) if bool((mask == 0).all()) else values / mask.sum((1, 2, 3)))
    return torch.cat(results).mean()


def semi_terms_literal(sup_preds, teacher_sup_preds, y_sup, fw, bw, tfw, tbw, main_loss, lfr_loss_type, loss_decay_rate, lfl_loss_decay_rate,
                       sup_label_loss_weight, lfl_weight, lfr_weight):
    """raft/semi.py:373-401, 447-468 in the dtype of its inputs: (sup_label_loss, lfl_loss, the SUM of the [B,H,W] lfr_loss)."""
    gamma = loss_decay_rate
    sup = sum(keras_loss_literal(y_sup, p, main_loss) * gamma ** (len(sup_preds) - i - 1) * sup_label_loss_weight
              for i, p in enumerate(sup_preds))
    gamma = lfl_loss_decay_rate
    lfl = sum(keras_loss_literal(y_sup, p, main_loss) * gamma ** (len(teacher_sup_preds) - i - 1) * lfl_weight
              for i, p in enumerate(teacher_sup_preds))
    gamma = loss_decay_rate
    lfr = 0.0
    for i, (p, pb) in enumerate(zip(fw, bw)):
        i_weight = gamma ** (len(fw) - i - 1)
        y_joint = torch.cat((tfw[-1], torch.ones_like(tfw[-1])[..., 0:1]), dim=3).detach()
        y_joint_bw = torch.cat((tbw[-1], torch.ones_like(tbw[-1])[..., 0:1]), dim=3).detach()
        loss = keras_loss_literal(y_joint, p, lfr_loss_type, "none") * i_weight
        loss = loss + keras_loss_literal(y_joint_bw, pb, lfr_loss_type, "none") * i_weight
        lfr = lfr + loss
    return sup, lfl, (lfr * lfr_weight).sum()
