"""NHWC-shaped twins of the reference's TensorFlow hot-path API (API parity only):

    raft.corr.CorrBlock(num_levels=4, radius=4, is_max_disp=False).__call__(corr_pyramid, coords)   raft/corr.py:5-22
    raft.allfield.calc_all_field(a, b, num_pool)                                                     raft/allfield.py:61-92
    raft.allfield.build_pyramid(c_volume, num_pool)                                                  raft/allfield.py:94-106
    transpose_volume(c_volume)  == tf.transpose(c_volume, [0, 3, 4, 1, 2])                           raft/semi.py:250, 257
    raft.upsample.UpsampleConvexWithMask(scale=8).call([x, mask, ref])                               raft/upsample.py:4-41
    raft.smurf_models.raft_update.BasicUpdateBlock(args, hidden_dim).call([net, inp, corr, flow])    raft_update.py:180-212
    raft.loss.FlowLossL1 / FlowLossL2 / FlowLossRobust(reduction).__call__(y_true, y_pred)           raft/loss.py:4-93
    raft.metric.EPE / SparseEPE                                                                      raft/metric.py:3-87
    flow_sequence_loss, semi_objective: the sums Semisupervised.train_step forms of them             raft/semi.py:373-405, 447-471
    crop_bboxes, pad_bboxes (util/image.py:6-49), get_proc_size, resize, resize_flow (raft/__init__.py:199-222),
    pad_edge, pad_inputs, unpad_inputs (util/pad.py, util/validate.py:301-325): raft_tf/image.py, tensors or lists of them

TensorFlow is not installed here, so these take and return torch tensors laid out the way the TF code lays
them out (channels last, coords as [B,H,W,2] with (x, y) in the last dim) and run the same HIP kernels as the
PyTorch-shaped API.  Pooling: the fused build pools with PyTorch's floor halving; TF pools level 0 with padding='SAME'
(ceil sizes, partial edge windows averaged over their in-range elements: e.g. 55 rows at 1/8 of Sintel give 28 / 14 / 7 rows,
not 27 / 13 / 6).  When a pooled dimension is odd, calc_all_field and build_pyramid therefore build the pyramid with
fsraft_corr_pool_pyramid_same and CorrBlock looks it up with fsraft_corr_lookup_fwd_same.  No TF oracle exists in this
environment: the SAME path is tested against a restatement of TF's documented semantics (parity unpinned).
Its backward is opt-in: with raft_tf.same_grad() on, the three calls are differentiable on 'SAME' pyramids too (the exact
transpose of the forward above: fsraft_corr_unpool_same_bwd, fsraft_corr_lookup_bwd_same, fsraft_corr_lookup_dcoords_same);
with it off, the default, such a call that wants a gradient raises.
"""
from .api import (BasicUpdateBlock, CorrBlock, UpsampleConvexWithMask, build_pyramid, calc_all_field,  # noqa: F401
                  same_grad, transpose_volume)
from .image import (crop_bboxes, get_proc_size, pad_bboxes, pad_edge, pad_inputs, resize, resize_flow,  # noqa: F401
                    unpad_inputs)
from .loss import FlowLossL1, FlowLossL2, FlowLossRobust, flow_sequence_loss, semi_objective  # noqa: F401
from .metric import EPE, SparseEPE  # noqa: F401
from .visualize import visualize_flow, visualize_flows  # noqa: F401    util/visualize.py:5-27, 40-42 (HSV flow coding)
