"""Flow-supervisor two-phase forward (pytorch/core/l2l.py:24-133) on the HIP hot path.

First half of the iterations: the student `update_block` refines flow on the augmented crop.  At the half-way
point the hidden state and flow are zero-padded out to the uncropped frame, a second correlation volume is built
from the uncropped pair, everything is detached, and `grad_update_block` (the supervisor) carries on; its
predictions are cropped back to the student's window.  Both halves run the same kernels as RAFT.forward; the
padding happens directly on the channels-last hidden state.
"""
import torch
import torch.nn.functional as F

from . import streams
from .corr import CorrBlock
from .gma import mark_records
from .raft import RAFT, normalise, refine
from .update import BasicUpdateBlock, to_channels_last
from .. import image_ops
from .._lib import on_tensor_device

# The per-sample branches below on csrc/image_ops.hip (fsraft_box_copy): _pad_state is two launches (the hidden state channels
# last, the flow planar) instead of 2B F.pad and two cat, _crop_back of ALL the supervisor's predictions one list node instead of
# B strided copies per prediction (and a zero fill + B copies each in backward).  Copies: the same bits either way.  False:
# the framework composition.  The equal-offset branches (one F.pad, one slice view) do not depend on it.
BOX_OPS = True


def _offsets(v, B):
    """Crop offsets per sample.  The reference reads `ox[0]` / `oy[0]` for the whole batch (l2l.py:87-88): a tensor or a
    python int means that.  A python list / tuple gives every sample its own offset (extension: lets the labelled and the
    unlabelled sample of the flow-supervisor step share one batched forward, train.SemiTrainStep)."""
    if isinstance(v, (list, tuple)):
        if len(v) != B:
            raise ValueError(f"{len(v)} crop offsets for a batch of {B}")
        return [int(x) for x in v]
    return [int(v) if isinstance(v, int) else int(v[0])] * B


def _pad_state(net, flow, ox_l, oy_l, orig, targ):
    """Zero-pad the hidden state (channels-last) and the flow from the crop's grid into the uncropped frame's grid
    (l2l.py:90-93), sample by sample when the offsets differ."""
    (orig_h, orig_w), (targ_h, targ_w) = orig, targ

    def pads(ox_, oy_):
        return ox_ // 8, (targ_w - ox_ - orig_w) // 8, oy_ // 8, (targ_h - oy_ - orig_h) // 8
    if len(set(zip(ox_l, oy_l))) == 1:
        l, r, t, b = pads(ox_l[0], oy_l[0])
        return F.pad(net, (0, 0, l, r, t, b)), F.pad(flow, (l, r, t, b))
    every = [pads(ox_, oy_) for ox_, oy_ in zip(ox_l, oy_l)]
    frames = {(t + net.shape[1] + b, l + net.shape[2] + r) for l, r, t, b in every}
    if BOX_OPS and len(frames) == 1 and min(map(min, every)) >= 0:      # (frames of different sizes: the cat below says so)
        frame = frames.pop()
        yx = image_ops.window_offsets([(oy_ // 8, ox_ // 8) for ox_, oy_ in zip(ox_l, oy_l)], net.shape[0], frame, tuple(net.shape[1:3]))
        return (image_ops.BoxCopyFn.apply(yx, frame, True, "nhwc", net)[0],
                image_ops.BoxCopyFn.apply(yx, frame, True, "nchw", flow)[0])
    nets, flows = [], []
    for i, (ox_, oy_) in enumerate(zip(ox_l, oy_l)):
        l, r, t, b = pads(ox_, oy_)
        nets.append(F.pad(net[i:i + 1], (0, 0, l, r, t, b)))
        flows.append(F.pad(flow[i:i + 1], (l, r, t, b)))
    return torch.cat(nets, 0), torch.cat(flows, 0)


class _CropBackFn(torch.autograd.Function):
    """Per-sample windows of the full-frame prediction as ONE autograd node: a strided copy per sample forward, one zero
    fill + a copy per sample backward (slicing + cat costs five framework launches per prediction in backward: two
    zero-filled full frames, two copies, one add)."""

    @staticmethod
    def forward(ctx, flow_up, ox_l, oy_l, orig):
        h, w = orig
        out = torch.empty(flow_up.shape[0], flow_up.shape[1], h, w, device=flow_up.device, dtype=flow_up.dtype)
        for i, (ox_, oy_) in enumerate(zip(ox_l, oy_l)):
            out[i].copy_(flow_up[i, :, oy_: oy_ + h, ox_: ox_ + w])
        ctx.win = (tuple(ox_l), tuple(oy_l), h, w, tuple(flow_up.shape))
        return out

    @staticmethod
    def backward(ctx, g):
        ox_l, oy_l, h, w, shape = ctx.win
        d = torch.zeros(shape, device=g.device, dtype=g.dtype)
        for i, (ox_, oy_) in enumerate(zip(ox_l, oy_l)):
            d[i, :, oy_: oy_ + h, ox_: ox_ + w].copy_(g[i])
        return d, None, None, None


def _crop_back(flow_up, ox_l, oy_l, orig):
    """The supervisor's full-frame prediction(s) cut back to the student's window (l2l.py:124-125): a tensor, or a list of them
    (a list comes back as a list; with per-sample offsets and BOX_OPS it is one autograd node per 32 predictions)."""
    if isinstance(flow_up, (list, tuple)):
        preds = list(flow_up)
        if not BOX_OPS or not preds or len(set(zip(ox_l, oy_l))) == 1:
            return [_crop_back(p, ox_l, oy_l, orig) for p in preds]
        yx = image_ops.window_offsets(list(zip(oy_l, ox_l)), preds[0].shape[0], tuple(preds[0].shape[-2:]), orig)
        out = []
        for i in range(0, len(preds), image_ops.MAX_LIST):
            out += image_ops.BoxCopyFn.apply(yx, tuple(orig), False, "nchw", *preds[i:i + image_ops.MAX_LIST])
        return out
    orig_h, orig_w = orig
    if len(set(zip(ox_l, oy_l))) == 1:
        return flow_up[:, :, oy_l[0]: oy_l[0] + orig_h, ox_l[0]: ox_l[0] + orig_w]
    if BOX_OPS:
        return _crop_back([flow_up], ox_l, oy_l, orig)[0]
    return _CropBackFn.apply(flow_up, ox_l, oy_l, orig)


class _FlowSupervisor:
    """The two-phase forward of L2L and GMAL2L (mixed in before RAFT / RAFTGMA).  A class supplies `_supervisor` and
    `_uncropped_context`."""

    def _uncropped(self, ci1, ci2, sup_grad_samples):
        """Second feature pair, context (and attention) of the uncropped frames (l2l.py:95-101): (tfmap1, tfmap2, inp, attention, k)."""
        k = sup_grad_samples
        k = k if (k is not None and 0 < k < ci1.shape[0] and torch.is_grad_enabled()) else None
        if k is not None:
            # (extension) the caller's loss reaches the supervisor's predictions of the first k samples only (the flow-supervisor
            # step batches its labelled and its unlabelled sample: train.SemiTrainStep): the uncropped frames of the others are
            # encoded without a graph -- their gradient would be zeros pushed through the whole feature encoder
            ta1, ta2 = self._features(ci1[:k], ci2[:k])
            with torch.no_grad():
                tb1, tb2 = self._features(ci1[k:], ci2[k:])
            t1, t2 = torch.cat([ta1, tb1]), torch.cat([ta2, tb2])
        else:
            t1, t2 = self._features(ci1, ci2)
        with torch.no_grad():             # (detached by the reference, l2l.py:104: no graph, no saved activations)
            inp, attention = self._uncropped_context(ci1)
        return t1, t2, inp, attention, k

    def _switch(self, net, flow, crop, frame, uncropped, early):
        """Half-way (l2l.py:79-113): the student's state zero-padded into the uncropped frame's grid, the second volume and its
        first lookup, everything detached -> (corr_fn, net, inp, attention, flow, corr).  The crop's own volume is not looked up
        here (the reference does, l2l.py:73, and drops the result, :102).  early: the uncropped frames' encodings when the second
        stream already has them."""
        net, flow = _pad_state(net, flow.detach(), crop[0], crop[1], crop[2], frame)               # (l2l.py:90-93)
        if early is not None:
            streams.join(net.device, *early[:4])
        tfmap1, tfmap2, inp, attention, k = early if early is not None else uncropped()
        corr_fn = CorrBlock(tfmap1, tfmap2, radius=self.args.corr_radius, grad_samples=k)          # second volume (l2l.py:101)
        corr = corr_fn(flow, channels_last=True, is_flow=True)          # (outside any batch: its features are detached next)
        net, corr, inp, flow = net.detach(), corr.detach(), inp.detach(), flow.detach()
        if attention is not None:         # (GMAL2L: the uncropped frames' attention map, still marked as records)
            attention = mark_records(attention.detach(), like=attention)
        return corr_fn, net, inp, attention, flow, corr

    def _two_phase(self, image1, image2, ci1, ci2, ox, oy, iters, flow_init, test_mode, supervisor_grad, sup_grad_samples):
        image1, image2 = normalise(image1), normalise(image2)
        if ci1 is not None:
            ci1, ci2 = normalise(ci1), normalise(ci2)
        if test_mode:                     # the student alone (l2l.py:130-131); its context after the features, on the caller's stream
            return self._single_phase(image1, image2, iters, flow_init, True, overlap=False)
        if ci1 is None:
            # the reference reads oy_/ox_ in the second half without having set them (l2l.py:124-125)
            raise NameError(f"{type(self).__name__}.forward in training mode needs the uncropped pair ci1/ci2 and offsets ox/oy")
        if iters == 0:                    # (no iteration, no switch: nothing is predicted)
            return []
        grad_mode = torch.is_grad_enabled()
        uncropped = lambda: self._uncropped(ci1, ci2, sup_grad_samples)

        def early():
            # the uncropped frames' encodings depend on the inputs only: issued on the second stream behind the student's context,
            # joined at the switch where the reference computes them (core/streams.py; 56.0 -> 58.8 pairs/s at one pair per GPU)
            with torch.set_grad_enabled(grad_mode and supervisor_grad):
                return uncropped()
        corr_fn, (net, inp, attention), flow, side = self._encode(image1, image2, flow_init, side_work=early)
        half = iters // 2
        crop = (_offsets(ox, net.shape[0]), _offsets(oy, net.shape[0]), tuple(image1.shape[-2:]))
        net, flow, _, student = refine(self.update_block, corr_fn, net, inp, flow, half, attention, motion_iters=half)
        try:
            if not supervisor_grad:
                # (extension, default off) the caller's loss does not reach the supervisor's predictions -- sequence_loss_unsup
                # only reads the last one, detached (train.py:110-111) -- so the second half records no graph, and has no
                # HeadBatch: its predictions are upsampled per iteration
                torch.set_grad_enabled(False)
            corr_fn, net, inp, attention, flow, corr = self._switch(net, flow, crop, tuple(ci1.shape[-2:]), uncropped, side)
            block, motion_iters = self._supervisor(iters - half)
            supervisor = refine(block, corr_fn, net, inp, flow, iters - half, attention, grad_samples=sup_grad_samples,
                                first_corr=corr, motion_iters=motion_iters)[3]
        finally:
            torch.set_grad_enabled(grad_mode)
        # the deferred mask head + upsampler of each phase, after the caller's gradient mode is back (the unlabelled pass of the
        # flow-supervisor step switches it off for the supervisor's half); the student's first.  The supervisor's full-frame
        # predictions are cut back to the student's window here (l2l.py:124-125).
        return student() + _crop_back(supervisor(), *crop)


class L2L(_FlowSupervisor, RAFT):
    def __init__(self, args):
        super().__init__(args)
        self.grad_update_block = BasicUpdateBlock(self.args, hidden_dim=self.hidden_dim)   # l2l.py:27

    def _supervisor(self, n):
        """-> the block of the supervisor phase's n iterations and how many of them go through a MotionBatch: all but the first,
        whose correlation features are detached."""
        return self.grad_update_block, n - 1

    def _uncropped_context(self, img):
        """-> (inp, attention) of an uncropped frame; the hidden-state half of the context encoder's output is not used."""
        return to_channels_last(torch.relu(self._context_split(img)[1])), None

    @on_tensor_device
    def forward(self, image1, image2, ci1=None, ci2=None, ox=None, oy=None, iters=24, flow_init=None,
                upsample=True, test_mode=False, supervisor_grad=True, sup_grad_samples=None):
        return self._two_phase(image1, image2, ci1, ci2, ox, oy, iters, flow_init, test_mode, supervisor_grad, sup_grad_samples)
