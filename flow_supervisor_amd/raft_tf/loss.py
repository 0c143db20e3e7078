"""The flow losses of the reference's TensorFlow trainers on one HIP kernel (csrc/flow_loss.hip, fsraft_flow_loss):

    raft.loss.FlowLossL1 / FlowLossL2 / FlowLossRobust        raft/loss.py:4-93, compiled by train.py:184-186, semi.py:29-34
    flow_sequence_loss(preds, y_true, weights, ...)           the sum over a sequence of predictions the train steps form
                                                              (raft/baseline.py, raft/semi.py:373-385), one launch
    semi_objective(...)                                       the three flow terms of Semisupervised.train_step, semi.py:373-405, 447-471

Per pixel the three losses are  mean_c psi(y_pred - y_true) * mask * (|y_true| < 400)  with psi = |d|, d^2 or sqrt(d^2 + 0.001^2):
the mask is a float FACTOR (not thresholded) and the cut is strict.  Keras then reduces the [B,H,W] map: reduction 'mean' is its
default (SUM_OVER_BATCH_SIZE: the sum over the map divided by B*H*W), 'sum' the plain sum, 'none' the map itself.  The kernel
takes the reduction as one factor `scale` on the sum over pixels AND channels: 1 / (2*B*H*W) for 'mean', 1 / 2 for 'sum' and
for the map, whose gradient under tf.GradientTape is the gradient of its sum.

TensorFlow is not installed here: the oracle of these functions is a float64 restatement of raft/loss.py (tests/_flowlossref.py);
parity with TensorFlow itself is unpinned.  There is no CPU implementation.
"""
import torch

from .. import _lib as L
from .. import ops

MAX_FLOW = 400.0        # raft/loss.py:26
ROBUST_EPS = 0.001      # raft/loss.py:90


def _channel_dim(layout):
    return ops.FLOW_LAYOUTS[layout][2]


def split_y_true(y_true, layout="nhwc"):
    """(flow, mask or None) of the forms raft/loss.py:9-19 takes: a tensor with three channels (flow and mask, read in place), a
    (flow, mask) pair, a (flow,) tuple or a bare flow.  The mask comes back as [B,H,W]."""
    c = _channel_dim(layout)
    if isinstance(y_true, torch.Tensor):
        if y_true.dim() == 4 and y_true.shape[c] == 3:
            return y_true.narrow(c, 0, 2), y_true.select(c, 2)
        return y_true, None
    if isinstance(y_true, (list, tuple)):
        if len(y_true) == 2:
            flow, mask = y_true
            if mask.dim() == 4:
                if mask.shape[c] != 1:
                    raise ValueError(f"flow loss: a mask has one channel, got {tuple(mask.shape)}")
                mask = mask.select(c, 0)
            return flow, mask
        if len(y_true) >= 1:
            return y_true[0], None
    raise ValueError("flow loss: y_true is a tensor, a (flow, mask) pair or a (flow,) tuple")


def _dense(t, layout):
    """`t` as the kernel can address it: itself when its pixels share one stride, a contiguous copy otherwise."""
    return t if ops.flow_strides(t, layout) is not None else t.contiguous()


class _FlowLossFn(torch.autograd.Function):
    """n predictions against one target in one fsraft_flow_loss launch: the loss, its gradients (back to back in one buffer, as
    train._SeqLossFn keeps them), and on request the per-sample EPE sums or the per-pixel map of a single prediction."""

    @staticmethod
    def forward(ctx, weights, target, mask, penalty, scale, layout, metric_idx, want_map, *preds):
        L.require_cuda_f32(*preds, target, mask)
        n = len(preds)
        p0 = preds[0]
        strides = ops.flow_strides(p0, layout)
        packed = strides is not None and p0.numel() == 1 + sum((s - 1) * st for s, st in zip(p0.shape, p0.stride()))
        if not packed or any(p.stride() != p0.stride() for p in preds):
            preds = [p.contiguous() for p in preds]
            p0 = preds[0]
        need = [ctx.needs_input_grad[8 + i] for i in range(n)]
        dps = [None] * n
        if any(need):
            # one buffer, the gradients back to back, each laid out as its prediction is
            buf = torch.empty(sum(need), p0.numel(), device=p0.device, dtype=torch.float32)
            rows = iter(buf.unbind(0))
            dps = [next(rows).as_strided(p0.shape, p0.stride()) if nd else None for nd in need]
        if target is not None:
            target = _dense(target, layout)
        if mask is not None and ops._mask_strides(mask) is None:
            mask = mask.contiguous()
        out, stats, pix = ops.flow_loss(preds, weights, scale, target, mask, penalty, layout, dps if any(need) else None, metric_idx,
                                        want_map, MAX_FLOW, ROBUST_EPS)
        ctx.dps, ctx.want_map, ctx.cdim = dps, want_map, _channel_dim(layout)
        if stats is None:
            stats = out.new_zeros(0)
        if pix is None:
            pix = out.new_zeros(0)
        ctx.mark_non_differentiable(*((stats,) if want_map else (stats, pix)))
        return out[0], stats, pix

    @staticmethod
    def backward(ctx, g, _gstats, gmap):
        dps, ctx.dps = ctx.dps, None
        live = [d for d in dps if d is not None]
        if ctx.want_map:                                  # the map of one prediction: stored d map / d pred, times the upstream map
            live[0].mul_(gmap.unsqueeze(ctx.cdim))
        else:
            torch._foreach_mul_(live, g)                  # one multi-tensor kernel, not one multiply per prediction
        return (None,) * 8 + tuple(dps)


def _check(preds, flow, mask, layout):
    h, w, c = ops.FLOW_LAYOUTS[layout]
    shape = tuple(preds[0].shape)
    if len(shape) != 4 or shape[c] != 2:
        raise ValueError(f"flow loss: predictions are {'[B,H,W,2]' if layout == 'nhwc' else '[B,2,H,W]'}, got {shape}")
    for p in preds:
        if tuple(p.shape) != shape:
            raise ValueError(f"flow loss: predictions of {shape} and {tuple(p.shape)}")
    if flow is not None and tuple(flow.shape) != shape:
        raise ValueError(f"flow loss: y_true {tuple(flow.shape)} against y_pred {shape}")
    if mask is not None and tuple(mask.shape) != (shape[0], shape[h], shape[w]):
        raise ValueError(f"flow loss: mask {tuple(mask.shape)} against y_pred {shape}")
    return shape[0] * shape[h] * shape[w]


REDUCTIONS = ("mean", "sum", "none")


@L.on_tensor_device
def flow_sequence_loss(preds, y_true, weights, penalty="l2", reduction="mean", layout="nhwc", metric_idx=None):
    """sum_i weights[i] * FlowLoss{L1,L2,Robust}(reduction)(y_true, preds[i]) as ONE autograd node and one kernel launch, without a
    host synchronisation.  preds: up to 32 flows [B,H,W,2] (layout 'nhwc') or [B,2,H,W] ('nchw'); y_true in any form the classes
    take (the three-channel tensor is read in place); reduction 'mean' or 'sum' ('none' only for a single prediction: the
    weighted [B,H,W] map).  The gradients are written by the forward launch into one buffer, back to back; backward is a single
    _foreach_mul_ by the upstream scalar.  Differentiable in preds only.  metric_idx: also return the [B,2] per-sample sums
    (sum mask * epe, sum mask) of that prediction, as a second value (a device tensor: metric.EPE.update_stats takes it)."""
    preds = list(preds)
    if penalty not in ops.FLOW_PENALTIES:
        raise ValueError(f"flow loss: penalty is one of {sorted(ops.FLOW_PENALTIES)}, got {penalty!r}")
    if reduction not in REDUCTIONS:
        raise ValueError(f"flow loss: reduction is one of {REDUCTIONS}, got {reduction!r}")
    if layout not in ops.FLOW_LAYOUTS:
        raise ValueError(f"flow loss: layout is 'nhwc' or 'nchw', got {layout!r}")
    if not 1 <= len(preds) <= 32 or len(weights) != len(preds):
        raise ValueError(f"flow loss: 1 to 32 predictions and as many weights, got {len(preds)} and {len(weights)}")
    if reduction == "none" and len(preds) != 1:
        raise ValueError("flow loss: reduction 'none' returns the map of a single prediction")
    if metric_idx is not None and not 0 <= metric_idx < len(preds):
        raise ValueError(f"flow loss: metric_idx {metric_idx} outside the {len(preds)} predictions")
    flow, mask = split_y_true(y_true, layout)
    npix = _check(preds, flow, mask, layout)
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in preds + [flow]):
        raise RuntimeError("fsraft ops need CUDA (ROCm) tensors; the hot path has no CPU implementation")
    flow = flow.detach().float()
    mask = mask.detach().float() if mask is not None else None
    scale = 1.0 / (2.0 * npix) if reduction == "mean" else 0.5
    want_map = reduction == "none"
    w = [float(x) for x in weights]
    loss, stats, pix = _FlowLossFn.apply([1.0] if want_map else w, flow, mask, penalty, scale, layout, metric_idx, want_map, *preds)
    value = pix * w[0] if want_map and w[0] != 1.0 else pix if want_map else loss
    return value if metric_idx is None else (value, stats)


class _FlowLoss:
    """keras.losses.Loss-shaped: obj(y_true, y_pred) with y_pred [B,H,W,2] and y_true a [B,H,W,3] tensor (flow, mask), a
    (flow, mask) pair, a (flow,) tuple or a bare flow.  reduction 'mean' (Keras' default), 'sum' or 'none' (the [B,H,W] map)."""
    penalty = None

    def __init__(self, reduction="mean", name=None, **kwargs):
        if reduction not in REDUCTIONS:
            raise ValueError(f"flow loss: reduction is one of {REDUCTIONS}, got {reduction!r}")
        self.reduction, self.name = reduction, name

    def __call__(self, y_true, y_pred, sample_weight=None):
        if sample_weight is not None:
            raise NotImplementedError("sample_weight: the reference's train steps pass None")
        return flow_sequence_loss([y_pred], y_true, [1.0], self.penalty, self.reduction, "nhwc")

    call = __call__


class FlowLossL1(_FlowLoss):
    """raft/loss.py:4-31."""
    penalty = "l1"


class FlowLossL2(_FlowLoss):
    """raft/loss.py:34-61."""
    penalty = "l2"


class FlowLossRobust(_FlowLoss):
    """raft/loss.py:63-93."""
    penalty = "robust"


def _decay(gamma, n):
    return [gamma ** (n - i - 1) for i in range(n)]


@L.on_tensor_device
def semi_objective(sup_predictions, teacher_sup_predictions, y_sup, flow_predictions, flow_predictions_bw, teacher_predictions,
                   teacher_predictions_bw, main_loss="l1", lfr_loss_type="l2", loss_decay_rate=0.8, lfl_loss_decay_rate=0.8,
                   sup_label_loss_weight=1.0, lfl_weight=1.0, lfr_weight=1.0):
    """The three flow terms of Semisupervised.train_step (raft/semi.py:373-405, 447-471), each a device scalar, in a dict:

      sup_label_loss   sum_i loss_decay_rate^(n-i-1) * main(y_sup, sup_predictions[i]) * sup_label_loss_weight           :373-385
      lfl_loss         sum_i lfl_loss_decay_rate^(n-i-1) * main(y_sup, teacher_sup_predictions[i]) * lfl_weight           :387-401
      lfr_loss         lfr_weight * sum_i loss_decay_rate^(n-i-1) * (lfr(t_fw, flow_predictions[i]) + lfr(t_bw, flow_predictions_bw[i]))
                       with t = the teacher's LAST prediction of each direction, detached, under a ones mask                :447-471

    main is FlowLossL1 or FlowLossRobust under Keras' default reduction (train.py:183-186: `main_loss`); lfr is `lfr_loss_type`
    under Reduction.NONE, so the reference's lfr_loss is a [B,H,W] tensor and tape.gradient differentiates its SUM: lfr_loss here
    is that sum, whose gradient is the reference's.  Four launches (one per group and direction).  A term whose weight is 0 is
    left out (None), as the reference skips it; the labelled terms are skipped together with y_sup None.

    Not reproduced: the reference adds the teacher's scalar SMURF term to the [B,H,W] LFR tensor before differentiating
    (semi.py:443, 470), which broadcasts the scalar over the map and scales ITS gradient by B*H*W.  The SMURF term stays with
    selfsup_loss.SmurfLoss; add it to these scalars with the weight you mean."""
    out = {"sup_label_loss": None, "lfl_loss": None, "lfr_loss": None}
    if y_sup is not None and sup_predictions:
        n = len(sup_predictions)
        out["sup_label_loss"] = flow_sequence_loss(sup_predictions, y_sup, [w * sup_label_loss_weight for w in _decay(loss_decay_rate, n)],
                                                   main_loss, "mean")
        if lfl_weight > 0.0 and teacher_sup_predictions:
            n = len(teacher_sup_predictions)
            out["lfl_loss"] = flow_sequence_loss(teacher_sup_predictions, y_sup, [w * lfl_weight for w in _decay(lfl_loss_decay_rate, n)],
                                                 main_loss, "mean")
    if lfr_weight > 0.0 and flow_predictions:
        if len(flow_predictions_bw) != len(flow_predictions):
            raise ValueError("semi_objective: as many backward as forward predictions (semi.py:453 zips them)")
        w = [x * lfr_weight for x in _decay(loss_decay_rate, len(flow_predictions))]
        fw = flow_sequence_loss(flow_predictions, (teacher_predictions[-1].detach(),), w, lfr_loss_type, "sum")
        bw = flow_sequence_loss(flow_predictions_bw, (teacher_predictions_bw[-1].detach(),), w, lfr_loss_type, "sum")
        out["lfr_loss"] = fw + bw
    return out
