"""RAFT model shell around the HIP hot path.  Same constructor, ``forward`` signature, return
values and state_dict keys as pytorch/core/raft.py:24-144; the loop body differs only in that
tensors between the lookup, the update block and the upsampler stay channels-last so no
layout conversion (and no torch.cat / softmax / unfold) runs per iteration.

Every forward of the package (RAFT, RAFTGMA, L2L, GMAL2L) is `_Shell._encode`, then one or two calls of `refine`.
"""
import torch
import torch.nn as nn

from .. import ops
from . import streams
from .corr import AlternateCorrBlock, CorrBlock
from .extractor import BasicEncoder, SmallEncoder, _prepare_packs
from .update import BasicUpdateBlock, SmallUpdateBlock, to_channels_last
from .utils.utils import coords_grid, upflow8
from .._lib import on_tensor_device

autocast = torch.autocast


class _ConvexUpsample(torch.autograd.Function):
    """upsample_flow on the HIP kernel; mask is channels-last [N,H,W,576]."""

    @staticmethod
    def forward(ctx, flow, mask_cl):
        ctx.save_for_backward(flow, mask_cl)
        return ops.upsample_fwd(flow, mask_cl)

    @staticmethod
    def backward(ctx, g):
        flow, mask_cl = ctx.saved_tensors
        dflow, dmask = ops.upsample_bwd(flow, mask_cl, g)
        return dflow, dmask


def convex_upsample(flow, mask, channels_last=False):
    """[N,2,H,W] x mask -> [N,2,8H,8W] (raft.py:72-83).  mask is [N,576,H,W] unless channels_last."""
    flow = flow.float()
    if not channels_last:
        mask = to_channels_last(mask.float())
    if flow.stride(2) != flow.shape[3] * flow.stride(3):
        flow = flow.contiguous()
    return _ConvexUpsample.apply(flow, mask)


def normalise(im):
    """0..255 -> -1..1 (raft.py:89-90)."""
    return (2 * (im / 255.0) - 1.0).contiguous()


def corr_block(args, fmap1, fmap2):
    """The correlation object `args` asks for (raft.py:104-107)."""
    if getattr(args, "alternate_corr", False):
        return AlternateCorrBlock(fmap1, fmap2, radius=args.corr_radius, coords_grad=getattr(args, "alt_coords_grad", False))
    return CorrBlock(fmap1, fmap2, radius=args.corr_radius)


def refine(block, corr_fn, net, inp, flow, iters, attention=None, test_mode=False, grad_samples=None, first_corr=None,
           motion_iters=None):
    """One refinement phase: `iters` calls of the update block `block` on one grid with one correlation object.
    -> (net, flow, flow_up, finish): the state after the phase, the last upsampled flow (test_mode; else None) and finish(), which
    returns the phase's upsampled predictions -- DEFERRED: in training the mask head and the upsampler of all iterations run as
    one launch each (update.HeadBatch) when finish() is called, under the gradient mode of that moment.

    The phase carries the FLOW, not coords1 = coords0 + flow (raft.py:121-131): the lookup adds the pixel grid itself, the update
    block and the upsampler want the flow anyway, so an iteration has one framework op (flow + delta) instead of three.  Same
    gradient structure: the flow entering an iteration is detached, delta_flow reaches the loss through the prediction.
    test_mode: only the last iteration's mask convolution and upsampler run (raft.py:141-142 returns that one alone; the
    reference computes the others and drops them).
    grad_samples: passed to every update-block call (and to the MotionBatch).
    first_corr: the correlation features of `flow`, looked up by the caller, who hands `flow` over detached: the first
    iteration's detach + lookup are the caller's.
    motion_iters: how many of the iterations (the last ones) write into a update.MotionBatch, whose motion-encoder backward is
    one launch per layer; None: no MotionBatch."""
    train = not test_mode
    hb = block.head_batch(iters, net) if train else None
    mb = block.motion_batch(motion_iters, net, grad_samples=grad_samples) if train and motion_iters is not None else None
    flows, ups, flow_up = [], [], None
    for i in range(iters):
        cur = mb if mb is not None and i >= iters - motion_iters else None
        if i == 0 and first_corr is not None:
            corr = first_corr
        else:
            flow = flow.detach()
            corr = corr_fn(flow, channels_last=True, is_flow=True, **({"out": cur.corr[cur.n]} if cur is not None else {}))
        want_up = train or i == iters - 1                   # (training: True, the default of need_mask)
        net, up_mask, delta_flow = block.forward_cl(net, inp, corr, flow, attention, need_mask=want_up, head_batch=hb,
                                                    grad_samples=grad_samples, motion_batch=cur)
        flow = flow + delta_flow
        if hb is not None:
            flows.append(flow)
        elif want_up:
            flow_up = upflow8(flow) if up_mask is None else convex_upsample(flow, up_mask, channels_last=True)
            ups.append(flow_up)
    return net, flow, flow_up, lambda: hb.finish(flows) if flows else ups


class _Shell(nn.Module):
    """What the four models share around their phases: the reference's helper methods and the encode step.  A subclass has
    fnet, cnet, hidden_dim, context_dim and args."""

    def freeze_bn(self):
        for m in self.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.eval()

    def initialize_flow(self, img):
        """coords0 == coords1 == pixel grid at 1/8 resolution; flow = coords1 - coords0 (raft.py:63-70)."""
        N, C, H, W = img.shape
        c = coords_grid(N, H // 8, W // 8, device=img.device)
        return c, c.clone()

    @on_tensor_device
    def upsample_flow(self, flow, mask):
        """[N,2,H,W], [N,576,H,W] -> [N,2,8H,8W] convex combination (raft.py:72-83)."""
        return convex_upsample(flow, mask)

    # (autocast off, also a caller's: args.mixed_precision is accepted and without effect, see utils.warn_mixed_precision --
    #  fp32 storage everywhere, at full speed)
    def _features(self, a, b):
        with autocast("cuda", enabled=False):
            f1, f2 = self.fnet([a, b])
        return f1.float(), f2.float()

    def _corr_block(self, fmap1, fmap2):
        return corr_block(self.args, fmap1, fmap2)

    def _context_split(self, img):
        with autocast("cuda", enabled=False):
            cnet = self.cnet(img)
        return torch.split(cnet.float(), [self.hidden_dim, self.context_dim], dim=1)

    def _context(self, img):
        """-> (net, inp, attention): hidden state and context features, channels-last as the loop keeps them; no attention."""
        net, inp = self._context_split(img)
        return to_channels_last(torch.tanh(net)), to_channels_last(torch.relu(inp)), None

    def _encode(self, image1, image2, flow_init, overlap=True, side_work=None):
        """Frames the calling `forward` has put through `normalise` -> corr_fn, (net, inp, attention), flow, side.  The context
        encoder reads image1 only: with `overlap` and core/streams.py on it runs on the second stream beside the feature encoder
        and the volume build (`_corr_block`: RAFT's follows args.alternate_corr, the GMA family's does not).  side_work (L2L,
        GMAL2L): further work for that stream, issued behind the context, which alone the caller's stream then waits for; `side`
        is what it returned (None where there is no second stream).  flow: flow_init, or zeros on the 1/8 grid."""
        overlap = overlap and streams.OVERLAP and image1.is_cuda
        side = ctx_done = None
        if overlap:
            if side_work is not None:       # (the packed weights both streams read are built on this one first)
                _prepare_packs(self.fnet)
                _prepare_packs(self.cnet)
            with torch.cuda.stream(streams.fork(image1.device)):
                state = self._context(image1)
                if side_work is not None:
                    ctx_done = streams.mark(image1.device)
                    side = side_work()
        corr_fn = self._corr_block(*self._features(image1, image2))
        if overlap:
            streams.join(image1.device, *state, event=ctx_done)
        else:
            state = self._context(image1)
        B, _, Hi, Wi = image1.shape
        flow = flow_init.float() if flow_init is not None else torch.zeros(B, 2, Hi // 8, Wi // 8, device=image1.device)
        return corr_fn, state, flow, side

    def _single_phase(self, image1, image2, iters, flow_init, test_mode, **encode):
        """Frames the calling `forward` has put through `normalise` -> encode, one phase of `update_block` over all iterations,
        finish: the forward of RAFT and RAFTGMA, and of the L2L models in test mode."""
        corr_fn, (net, inp, attention), flow, _ = self._encode(image1, image2, flow_init, **encode)
        _, flow, flow_up, finish = refine(self.update_block, corr_fn, net, inp, flow, iters, attention, test_mode, motion_iters=iters)
        return (flow, flow_up) if test_mode else finish()


class RAFT(_Shell):
    def __init__(self, args):
        super().__init__()
        self.args = args
        if args.small:
            self.hidden_dim, self.context_dim = 96, 64
            args.corr_levels, args.corr_radius = 4, 3
        else:
            self.hidden_dim, self.context_dim = 128, 128
            args.corr_levels, args.corr_radius = 4, 4
        if "dropout" not in self.args:
            self.args.dropout = 0
        if "alternate_corr" not in self.args:
            self.args.alternate_corr = False
        if "mixed_precision" not in self.args:
            self.args.mixed_precision = False
        from .utils.utils import warn_mixed_precision
        warn_mixed_precision(self.args)
        hdim, cdim = self.hidden_dim, self.context_dim
        if args.small:
            self.fnet = SmallEncoder(output_dim=128, norm_fn="instance", dropout=args.dropout)
            self.cnet = SmallEncoder(output_dim=hdim + cdim, norm_fn="none", dropout=args.dropout)
            self.update_block = SmallUpdateBlock(self.args, hidden_dim=hdim)
        else:
            self.fnet = BasicEncoder(output_dim=256, norm_fn="instance", dropout=args.dropout)
            self.cnet = BasicEncoder(output_dim=hdim + cdim, norm_fn="batch", dropout=args.dropout)
            self.cnet.out_channels_last = True   # the context features reach the update block channels_last (extractor._Encoder.forward)
            self.update_block = BasicUpdateBlock(self.args, hidden_dim=hdim)

    @on_tensor_device
    def forward(self, image1, image2, iters=12, flow_init=None, upsample=True, test_mode=False):
        return self._single_phase(normalise(image1), normalise(image2), iters, flow_init, test_mode)
