"""raft/metric.py:3-44 on the device: the end-point-error metric of the reference's TensorFlow trainers, fed by the per-sample sums
fsraft_flow_loss leaves (csrc/flow_loss.hip).  No TensorFlow oracle exists here: tested against a float64 restatement of
raft/metric.py (tests/_flowlossref.py), parity with TensorFlow itself unpinned."""
import torch

from .. import _lib as L
from .. import ops
from .loss import _check, split_y_true


class EPE:
    """keras.metrics.Metric-shaped.  update_state(y_true, y_pred): per sample  sum(mask * |y_pred - y_true|_2) / sum(mask), or -1
    for every sample when the whole batch's mask is zero (metric.py:31-33), accumulated into a running mean on the device;
    result() is the only read-back.  The |y_true| < 400 cut of the losses does not enter.  y_true: a [B,H,W,3] tensor (flow, mask),
    a (flow, mask) pair, a (flow,) tuple or a bare flow -- the last two under a ones mask (the reference's branch for a bare tensor
    indexes y_true[0], sample 0 of the batch, which is not reproduced).  A sample whose own mask is zero inside a batch that is
    not gives 0 / 0 = NaN, as the reference's division does.  Masks are taken to be non-negative: `all(mask == 0)` is read off
    sum(mask) == 0."""

    def __init__(self, name="epe", **kwargs):
        self.name = name
        self._acc = None                      # device [2]: sum of the per-sample results, their count

    @L.on_tensor_device
    def update_state(self, y_true, y_pred, sample_weight=None):
        flow, mask = split_y_true(y_true, "nhwc")
        _check([y_pred], flow, mask, "nhwc")
        y_pred = y_pred.detach()
        if ops.flow_strides(y_pred, "nhwc") is None:
            y_pred = y_pred.contiguous()
        flow = flow.detach().float()
        if ops.flow_strides(flow, "nhwc") is None:
            flow = flow.contiguous()
        if mask is not None:
            mask = mask.detach().float()
            if ops._mask_strides(mask) is None:
                mask = mask.contiguous()
        _, stats, _ = ops.flow_loss([y_pred], [0.0], 0.0, flow, mask, "l2", "nhwc", None, 0, False, float("inf"))
        self.update_stats(stats)

    def update_stats(self, sample_stats):
        """sample_stats [B,2] = (sum mask * epe, sum mask) per sample, as flow_sequence_loss(..., metric_idx=k) returns them."""
        s = sample_stats.detach()
        res = torch.where(s[:, 1].sum() == 0, torch.full_like(s[:, 0], -1.0), s[:, 0] / s[:, 1])
        add = torch.stack((res.sum(), torch.full_like(res[0], float(res.numel()))))
        self._acc = add if self._acc is None else self._acc + add

    def result(self):
        if self._acc is None:
            return 0.0
        total, count = self._acc.tolist()
        return total / count if count else 0.0

    def reset_state(self):
        self._acc = None


class SparseEPE(EPE):
    """raft/metric.py:47-87: the reference's update_state raises NotImplementedError before it accumulates anything."""

    def update_state(self, y_true, y_pred, sample_weight=None):
        raise NotImplementedError
