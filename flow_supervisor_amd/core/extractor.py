"""Feature / context encoders.  Module and parameter names are those of pytorch/core/extractor.py, so reference
checkpoints load (state_dict keys ``conv1``, ``norm1``, ``layer{1,2,3}.{0,1}.conv{1,2,3}``, ``...downsample.{0,1}``,
``conv2``).  What runs where, for an fp32 CUDA input outside autocast whose norms are non-affine InstanceNorm or BatchNorm on
running statistics (_norm_kind), or affine BatchNorm in training mode (_train_bn_ok):
  * the 7x7 stride-2 stem on csrc/stem.hip (_StemFn), channels_last from there on;
  * stride-1 1x1 / 3x3 convolutions on the implicit-GEMM kernels (_ConvCL), from weight images packed once per parameter
    version (_prepare_packs);
  * the two strided convolutions of a stride-2 residual unit on the same kernels over a space-to-depth input (_StridedPairFn);
  * norm + ReLU (+ the unit's add and outer ReLU) on csrc/norm_cl.hip (_InstNormReluCL, _FrozenBNReluCL) and, for BatchNorm
    on batch statistics, csrc/norm_bn.hip (_TrainBNReluCL), which also moves the running statistics.
MIOpen, on NCHW tensors behind a layout copy, is what these do not cover: stride-2 units at odd sizes, channel counts that are
no multiple of four, the stem at other shapes.  Other norms (GroupNorm, BatchNorm without affine parameters or running
statistics or with momentum=None, none), autocast and CPU tensors run the framework's modules throughout, as does
FSRAFT_ENCODER_CL=0 with the norm + ReLU on the NCHW kernels of csrc/norm.hip -- which have no training-mode BatchNorm: that
one is the framework's module wherever the chain is NCHW or the channels-last kernels do not take the channel count.  The
switches STATS_IN_EPILOGUE, STEM_KERNEL, S2D_UNITS, S2D_EMIT and TRAIN_BN turn single routes off.
"""
import os
from collections import namedtuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .._lib import on_tensor_device


class _InstNormRelu(torch.autograd.Function):
    """relu?(instance_norm(x)) for NCHW fp32 on the fsraft kernels (two passes over the data each way)."""

    @staticmethod
    def forward(ctx, x, eps, relu):
        x = x.contiguous()
        y, stats = ops.inorm_relu_fwd(x, eps, relu)
        ctx.save_for_backward(x, stats)
        ctx.relu = relu
        return y

    @staticmethod
    def backward(ctx, g):
        x, stats = ctx.saved_tensors
        return ops.inorm_relu_bwd(g.contiguous(), x, stats, ctx.relu), None, None


class _FrozenBNRelu(torch.autograd.Function):
    """relu?(batch_norm(x + cbias[c])) with running statistics (eval mode / freeze_bn): y = x * scale[c] + shift[c].
    `cbias` is the bias of the convolution that produced x (or None): the convolution runs without it, the constant is
    folded into the shift, and its gradient -- the per-channel sum of the convolution's output gradient -- falls out of
    the sums this backward computes anyway, instead of a separate [N,H,W] reduction inside the convolution backward."""

    @staticmethod
    def forward(ctx, x, cbias, weight, bias, rm, rv, eps, relu):
        x = x.contiguous()
        rs = torch.rsqrt(rv.float() + eps)
        scale = (weight.float() * rs).contiguous()
        rmc = rm.float() - cbias.float() if cbias is not None else rm.float()       # effective mean seen by x
        shift = (bias.float() - rmc * scale).contiguous()
        y = ops.affine_relu_fwd(x, scale, shift, relu)
        ctx.save_for_backward(x, scale, shift, rs, rmc)
        ctx.relu = relu
        ctx.has_cbias = cbias is not None
        return y

    @staticmethod
    def backward(ctx, g):
        x, scale, shift, rs, rm = ctx.saved_tensors
        dx, sums = ops.affine_relu_bwd(g.contiguous(), x, scale, shift, ctx.relu)
        dweight = rs * (sums[1] - rm * sums[0])               # sum g' * (x + cbias - rm) * rs
        dcbias = scale * sums[0] if ctx.has_cbias else None   # = sum over pixels of dx
        return dx, dcbias, dweight, sums[0], None, None, None, None


def _is_cl(x):
    return x.dim() == 4 and x.shape[1] > 1 and x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous()


def _cl_channels_ok(C):
    """Channel counts the channels_last norm kernels (csrc/norm_cl.hip) take."""
    return C % 4 == 0 and 4 <= C <= 256


def _fast(x):
    return x.is_cuda and x.dtype == torch.float32 and x.dim() == 4


def _as_cl(x):
    """x as a channels_last tensor (no autograd: for use inside Functions).  The tiled fsraft transposes move an NCHW
    activation at 4-6 TB/s; the framework's strided copy reaches 1.4-2 TB/s on the same tensors (round 2, docs/history)."""
    if _is_cl(x):
        return x
    if _fast(x) and x.is_contiguous():
        B, C, H, W = x.shape
        return ops.nchw_to_nhwc(x, torch.empty(B, H, W, C, device=x.device, dtype=torch.float32)).permute(0, 3, 1, 2)
    return x.contiguous(memory_format=torch.channels_last)


def _as_nchw(x):
    if x.is_contiguous():
        return x
    if _fast(x) and _is_cl(x):
        return ops.nhwc_to_nchw(x.permute(0, 2, 3, 1))
    return x.contiguous()


class _ToNCHW(torch.autograd.Function):
    """x.contiguous() for a channels_last activation whose consumer is an NCHW MIOpen call; the gradient goes back
    channels_last, the layout its producer works in."""

    @staticmethod
    def forward(ctx, x):
        return _as_nchw(x)

    @staticmethod
    def backward(ctx, g):
        return _as_cl(g)


class _ResLink:
    """Ties the two consumers of a residual unit's input x together in backward: the unit's last norm kernel writes the
    shortcut gradient dres and parks it HERE (autograd gets None from it for x); the first convolution's backward -- which always
    runs later: the norm sits downstream of it -- accumulates its data gradient into that tensor through its epilogue and
    returns the SUM as x's gradient.  Autograd would otherwise add the two x-sized tensors in a separate pass (12 of them per
    step, up to 230 MB each).  Autograd sees one ordinary gradient for x from the unit, so further consumers of x, tensor
    hooks and retain_grad behave as usual (round 3 handed dres to autograd and then added into it behind the engine's back,
    which was only right while x had exactly these two consumers: ADVICE r2).
    `armed` is set by the first convolution's forward (_ConvCL, the only consumer that looks into the link): a norm whose unit's
    first convolution took another route (F.conv2d / MIOpen never sees the link) hands dres to autograd as usual instead of
    parking it where nobody collects it."""
    __slots__ = ("dres", "armed")

    def __init__(self):
        self.dres = None
        self.armed = False


def _cl_norm_enter(ctx, x, res, link, s2d):
    """Start of the forward of both channels_last norm Functions -> (x, res) channels_last.  s2d: the result leaves in the
    space-to-depth layout of the stride-2 unit that consumes it -- a [N, 4C, H/2, W/2] channels_last tensor -- and the
    gradient comes back in it (see _S2D; ctx.s2w is the `s2w` of the ops wrappers)."""
    ctx.in_cl = _is_cl(x)
    ctx.link = link
    x = _as_cl(x)
    ctx.s2w = x.shape[3] if s2d else 0
    return x, (_as_cl(res) if res is not None else None)


def _cl_norm_leave(ctx, dx, dres):
    """End of their backward -> (x's gradient, the shortcut's gradient as autograd gets it)."""
    if ctx.link is not None and ctx.link.armed:
        dres, ctx.link.dres = None, dres      # the shortcut's gradient travels through the link: conv1's backward returns the sum
    return dx if ctx.in_cl else _as_nchw(dx), dres      # an NCHW producer (MIOpen) gets an NCHW gradient


class _InstNormReluCL(torch.autograd.Function):
    """_InstNormRelu for channels_last tensors (storage [N][H*W][C]): csrc/norm_cl.hip.  With `res` (the shortcut of a
    residual unit, channels_last) the result is relu(res + relu?(norm(x))) in the same pass -- the unit's add and final ReLU
    (and their backward) cost no extra trip over the tensor.  `sums`: the _NormSums of the convolution that produced x."""

    @staticmethod
    def forward(ctx, x, eps, relu, res=None, link=None, sums=None, s2d=False):
        x, res = _cl_norm_enter(ctx, x, res, link, s2d)
        y, stats = ops.inorm_relu_cl_fwd(x, res, eps, relu, sums.acc if sums is not None else None, ctx.s2w)
        ctx.save_for_backward(x, stats, y if res is not None else None)
        ctx.relu = relu
        return y

    @staticmethod
    def backward(ctx, g):
        x, stats, out = ctx.saved_tensors
        dx, dres = _cl_norm_leave(ctx, *ops.inorm_relu_cl_bwd(_as_cl(g), x, stats, out, ctx.relu, ctx.s2w))
        return dx, None, None, dres, None, None, None


class _FrozenBNReluCL(torch.autograd.Function):
    """_FrozenBNRelu for channels_last tensors; `res` as in _InstNormReluCL."""

    @staticmethod
    def forward(ctx, x, cbias, weight, bias, rm, rv, eps, relu, res=None, link=None, s2d=False):
        x, res = _cl_norm_enter(ctx, x, res, link, s2d)
        scale, shift, rs, rmc = ops.bn_fold(weight, bias, rm, rv, cbias, eps)
        y = ops.affine_relu_cl_fwd(x, res, scale, shift, relu, ctx.s2w)
        ctx.save_for_backward(x, scale, shift, rs, rmc, y if res is not None else None)
        ctx.relu = relu
        ctx.has_cbias = cbias is not None
        return y

    @staticmethod
    def backward(ctx, g):
        x, scale, shift, rs, rmc, out = ctx.saved_tensors
        dx, dres, part = ops.affine_relu_cl_bwd(_as_cl(g), x, scale, shift, out, ctx.relu, ctx.s2w)
        dweight, dbias, dcbias = ops.bn_fold_bwd(part, rs, rmc, scale, ctx.has_cbias)
        dx, dres = _cl_norm_leave(ctx, dx, dres)
        return dx, dcbias, dweight, dbias, None, None, None, None, dres, None, None


class _TrainBNReluCL(torch.autograd.Function):
    """relu?(batch_norm(x + cbias)) of an nn.BatchNorm2d in training mode (_train_bn_ok) for channels_last tensors, on
    csrc/norm_bn.hip; `res` / `link` / `s2d` as in _InstNormReluCL.  The forward moves the module's running statistics and
    counts the batch, on the device (capturable), with or without a graph.  cbias (the bias the convolution in front ran
    without) only enters the running mean; its gradient is exactly zero and None is returned for it."""

    @staticmethod
    def forward(ctx, x, cbias, weight, bias, norm, relu, res=None, link=None, s2d=False):
        x, res = _cl_norm_enter(ctx, x, res, link, s2d)
        if x.shape[0] * x.shape[2] * x.shape[3] < 2:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {x.shape}")
        rm, rv = norm.running_mean, norm.running_var
        fp32 = rm.dtype == torch.float32 and rv.dtype == torch.float32
        m, v = (rm, rv) if fp32 else (rm.float(), rv.float())
        y, stats = ops.bnorm_cl_fwd(x, res, weight, bias, cbias, m, v, norm.momentum, norm.eps, relu, ctx.s2w)
        if not fp32:
            rm.copy_(m), rv.copy_(v)
        norm.num_batches_tracked.add_(1)
        ctx.save_for_backward(x, stats, y if res is not None else None)
        ctx.relu = relu
        return y

    @staticmethod
    def backward(ctx, g):
        x, stats, out = ctx.saved_tensors
        dx, dres, dweight, dbias = ops.bnorm_cl_bwd(_as_cl(g), x, stats, out, ctx.relu, ctx.s2w)
        dx, dres = _cl_norm_leave(ctx, dx, dres)
        return dx, None, dweight, dbias, None, None, dres, None, None


# GEMM-ready images of one weight (ops.pack_weight modes): fwd = mode 0 and dgrad = mode 1 in fp32, *_split = modes 10 / 11 for
# the split-bf16 kernels.  An fp32 image no kernel will read is not built: the field then holds the split image itself.
_GemmPacks = namedtuple("_GemmPacks", "fwd fwd_split dgrad dgrad_split")
# ... of a stride-1 1x1 / 3x3 convolution, cached as module.__dict__["_fs_packs"]; *_frag = the split images in fragment order
# (ops.fragment_order) for the resident-patch kernel: 3x3 with 33..64 channels on the GEMM's k side, else None
_ConvPacks = namedtuple("_ConvPacks", "key fwd fwd_split dgrad dgrad_split fwd_frag dgrad_frag")
# ... of a stride-2 unit, cached as block.__dict__["_fs_pair_packs"]: conv3 = its 3x3 stride-2 convolution as the 2x2 stride-1
# one over the space-to-depth input (_s2d_weight), shortcut = its 1x1; a _GemmPacks each
_PairPacks = namedtuple("_PairPacks", "key conv3 shortcut")


def _conv_key(conv):
    w = conv.weight
    return (w.data_ptr(), w._version, ops.exact_mode())


def _pair_key(block):
    w3, wsc = block.conv1.weight, block.downsample[0].weight
    return (w3.data_ptr(), w3._version, wsc.data_ptr(), wsc._version, ops.exact_mode())


def _queue_gemm_packs(plan, w, cin, order, **how):
    """Queue the images of weight `w` seen as [Cout, cin, ...] (`how`: PackPlan.pack's cin_full / s2d) -> a _GemmPacks of plan
    handles.  The fp32 images are built in exact arithmetic and for a side of at most 32 rows, which stays on the fp32
    kernels.  `order`: the modes in the order their jobs enter the plan, which is the layout of the packed buffer."""
    exact = ops.exact_mode()
    want = {10: True, 11: True, 0: exact or w.shape[0] <= 32, 1: exact or cin <= 32}
    h = {mode: plan.pack([w], [cin], mode, **how) for mode in order if want[mode]}
    return _GemmPacks(h.get(0, h[10]), h[10], h.get(1, h[11]), h[11])


def _queue_conv_packs(plan, conv, key):
    """The _ConvPacks of a stride-1 1x1 / 3x3 convolution, as plan handles."""
    wd = conv.weight.detach()
    N, C, KH, KW = wd.shape
    g = _queue_gemm_packs(plan, wd, C, (10, 0, 11, 1))
    ff = plan.pack([wd], [C], 10, frag=True) if (KH, KW) == (3, 3) and 32 < C <= 64 else None
    df = plan.pack([wd], [C], 11, frag=True) if (KH, KW) == (3, 3) and 32 < N <= 64 else None
    return _ConvPacks(key, *g, ff, df)


def _queue_pair_packs(plan, block, key):
    """The _PairPacks of a stride-2 unit, as plan handles."""
    w3, ws = block.conv1.weight.detach(), block.downsample[0].weight.detach()
    C = w3.shape[1]
    # the 3x3 stride-2 weight seen as its 2x2 stride-1 equivalent over the space-to-depth input (flag s2d): [N][4C][2][2]
    return _PairPacks(key, _queue_gemm_packs(plan, w3, 4 * C, (10, 11, 0, 1), cin_full=C, s2d=True),
                      _queue_gemm_packs(plan, ws, ws.shape[1], (10, 11, 0, 1)))


def _packed(h, out):
    """A record of plan handles -> the same record of the packed tensors `out` (PackPlan.run)."""
    if isinstance(h, _PairPacks):
        return h._replace(conv3=_packed(h.conv3, out), shortcut=_packed(h.shortcut, out))
    return h._replace(**{f: out[v] for f, v in zip(h._fields, h) if isinstance(v, int)})      # (not the key, not None)


def _stale(module, slot, key):
    c = module.__dict__.get(slot)
    return c is None or c.key != key


def _prepare_packs(root):
    """Every packed weight image of an encoder (or of one convolution) whose parameter changed since it was packed, built by
    ONE batched launch per 16 matrices (fsraft_pack_conv_weights) instead of two to four launches per layer plus the torch
    ops of the space-to-depth rewrite and of the fragment-order permutation."""
    todo = []       # (cache slot, module, key), in module order
    for m in root.modules():
        if isinstance(m, _Block) and _pair_structure_ok(m):
            w3 = m.conv1.weight
            key = _pair_key(m)
            if _stale(m, "_fs_pair_packs", key) and w3.is_cuda and w3.dtype == torch.float32:
                todo.append(("_fs_pair_packs", m, key))
        if (isinstance(m, nn.Conv2d) and m.stride == (1, 1) and m.kernel_size in ((1, 1), (3, 3)) and m.groups == 1
                and m.weight.is_cuda and m.weight.dtype == torch.float32):
            key = _conv_key(m)
            if _stale(m, "_fs_packs", key):
                todo.append(("_fs_packs", m, key))
    if not todo:
        return
    with torch.no_grad():
        _, first, _ = todo[0]
        plan = ops.PackPlan((first.conv1 if isinstance(first, _Block) else first).weight.device)
        hs = [(_queue_pair_packs if slot == "_fs_pair_packs" else _queue_conv_packs)(plan, m, key) for slot, m, key in todo]
        out = plan.run()
        for (slot, m, key), h in zip(todo, hs):
            m.__dict__[slot] = _packed(h, out)


def _weight_packs(conv):
    """The _ConvPacks of a convolution, cached on the module and rebuilt whenever the weight tensor changes (optimizer step,
    load_state_dict).  The encoders build all of theirs at once (_prepare_packs at the top of forward); a convolution used on
    its own gets here with a stale cache and packs itself."""
    if _stale(conv, "_fs_packs", _conv_key(conv)):
        _prepare_packs(conv)
    return conv.__dict__["_fs_packs"]


class _ConvCL(torch.autograd.Function):
    """Stride-1 'same' convolution (1x1 or 3x3) of a channels_last tensor on the update block's implicit-GEMM kernels
    (csrc/conv_igemm.hip): forward and data gradient on fsraft_conv_forward, weight (+ bias) gradient on
    fsraft_conv_wgrad -- whose few-channel variant packs several taps into one tile for these 64/96-channel layers.
    The storage of a channels_last [B,C,H,W] tensor IS the kernels' [B,H,W,C] layout, so nothing is transposed."""

    @staticmethod
    def forward(ctx, x, weight, bias, packs, link=None, sums=None):
        ctx.link = link if _is_cl(x) else None       # (a converted copy of x is not the tensor the shortcut gradient belongs to)
        if ctx.link is not None:
            ctx.link.armed = True                    # this node's backward will collect the parked shortcut gradient
        x = _as_cl(x)
        B, C, H, W = x.shape
        N, _, KH, KW = weight.shape
        out = torch.empty(B, H, W, N, device=x.device, dtype=torch.float32)
        # sums (a _NormSums holder): the InstanceNorm behind this convolution wants the per-image column sums of the result; the
        # kernel adds them up in its epilogue where it can, and the norm then skips its own statistics pass
        acc = ops.norm_partial_rows(B, N, x.device) if (sums is not None and bias is None and STATS_IN_EPILOGUE) else None
        carried = ops.conv_forward([ops.V(x.permute(0, 2, 3, 1), C)], packs.fwd, bias, B, H, W, KH, KW, N, [ops.Dst.nhwc(out)],
                                   wpk_split=packs.fwd_split, wpk_frag=packs.fwd_frag, stats=acc)
        if sums is not None:
            sums.acc = acc if carried else None
        ctx.save_for_backward(x, weight)
        ctx.packs = packs
        ctx.has_bias = bias is not None
        return out.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        B, C, H, W = x.shape
        N, _, KH, KW = weight.shape
        g = _as_cl(g)
        gv = ops.V(g.permute(0, 2, 3, 1), N)
        p = ctx.packs
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dres = ctx.link.dres if ctx.link is not None else None
            if dres is not None and dres.shape == x.shape and _is_cl(dres) and dres.dtype == torch.float32:
                # residual unit: this data gradient is added into the parked shortcut gradient, the sum is x's gradient (see _ResLink)
                ctx.link.dres = None
                ops.conv_forward([gv], p.dgrad, None, B, H, W, KH, KW, C, [ops.Dst.nhwc(dres.permute(0, 2, 3, 1), acc=True)],
                                 wpk_split=p.dgrad_split, wpk_frag=p.dgrad_frag)
                dx = dres
            else:
                if dres is not None:          # (a parked gradient this route cannot add into: hand both over, the sum is made here)
                    ctx.link.dres = None
                dxb = torch.empty(B, H, W, C, device=x.device, dtype=torch.float32)
                ops.conv_forward([gv], p.dgrad, None, B, H, W, KH, KW, C, [ops.Dst.nhwc(dxb)], wpk_split=p.dgrad_split,
                                 wpk_frag=p.dgrad_frag)
                dx = dxb.permute(0, 3, 1, 2)
                if dres is not None:
                    dx = dx + dres
        elif ctx.link is not None:
            ctx.link.dres = None              # (nobody asked for x's gradient: autograd.grad w.r.t. other inputs)
        want_b = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or want_b:
            dwpk = ops.zeros(N, ops.conv_ktot([C], KH, KW), device=x.device)
            db = ops.zeros(N, device=x.device) if want_b else None
            ops.conv_wgrad(gv, [ops.V(x.permute(0, 2, 3, 1), C)], dwpk, B, H, W, KH, KW, dbias=db)
            dw = ops.unpack_weight_grad(dwpk, tuple(weight.shape), [C])
        return dx, dw, db, None, None, None


class _StemFn(torch.autograd.Function):
    """conv1 of the encoders (7x7, stride 2, 3 input channels; pytorch/core/extractor.py:135, :212) on csrc/stem.hip: NCHW image
    in, channels_last activation out; backward is the weight gradient only (the image is the network input)."""

    @staticmethod
    def forward(ctx, x, w):
        x = x.contiguous()
        ctx.save_for_backward(x)
        return ops.stem_fwd(x, w.detach()).permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return None, ops.stem_wgrad(x, _as_cl(g).permute(0, 2, 3, 1))


def _stem_ok(conv, x):
    return (STEM_KERNEL and conv.kernel_size == (7, 7) and conv.stride == (2, 2) and conv.padding == (3, 3)
            and conv.dilation == (1, 1) and conv.groups == 1 and conv.padding_mode == "zeros" and conv.in_channels == 3
            and conv.out_channels in (32, 64) and _fast(x) and not x.requires_grad and not torch.is_autocast_enabled()
            and x.shape[2] >= 7 and x.shape[3] >= 7)


STATS_IN_EPILOGUE = True   # False: every InstanceNorm runs its own statistics pass
STEM_KERNEL = True         # False: the 7x7 stride-2 stem as a MIOpen call
S2D_UNITS = True           # False: the stride-2 units fall back to MIOpen behind layout hops (the path odd-sized inputs take)
TRAIN_BN = True            # False: a training-mode BatchNorm keeps the whole encoder on the framework's NCHW modules


class _NormSums:
    """Hand-over between a convolution and the InstanceNorm behind it: `acc` = the partial rows (ops.norm_partial_rows) of the
    result's column sums / sums of squares when the convolution's kernel accumulated them in its epilogue, else None."""
    __slots__ = ("acc",)

    def __init__(self):
        self.acc = None


def _conv(conv, x, bias, link=None, stem_cl=False, sums=None):
    """conv(x) with the given bias (None: without).  A channels_last fp32 input of a stride-1 1x1 / 3x3 convolution takes
    the fsraft kernels; anything else is MIOpen on an NCHW tensor (its NHWC fp32 kernels are far slower than its NCHW
    ones on gfx950 -- the backward-weights one by two orders of magnitude -- so a channels_last input is converted)."""
    k = conv.kernel_size
    if (_is_cl(x) and x.is_cuda and x.dtype == torch.float32 and k in ((3, 3), (1, 1)) and conv.stride == (1, 1)
            and conv.padding == (k[0] // 2, k[1] // 2) and conv.dilation == (1, 1) and conv.groups == 1
            and conv.padding_mode == "zeros" and x.shape[1] % 4 == 0 and not torch.is_autocast_enabled()):
        return _ConvCL.apply(x, conv.weight, bias, _weight_packs(conv), link, sums)
    if stem_cl and bias is None and _stem_ok(conv, x):
        return _StemFn.apply(x, conv.weight)
    return F.conv2d(_ToNCHW.apply(x) if _is_cl(x) else x, conv.weight, bias, conv.stride, conv.padding, conv.dilation, conv.groups)


_S2D_TAP = ((0, 1), (1, 0), (1, 1))          # 3x3 tap index k -> (2x2 tap t, sub-pixel s): input row 2y - 1 + k = 2(y + t - 1) + s


def _s2d_weight(w3):
    """[N,C,3,3] stride-2 weights -> the equivalent stride-1 [N,4C,2,2] weights over the space-to-depth input (channel
    (sy*2+sx)*C + c = pixel (2y+sy, 2x+sx)); 7 of the 16 (tap, sub-pixel) slots stay zero.  Host statement of the rewrite that
    fsraft_pack_conv_weights performs in its address arithmetic (flag bit 1); the tests hold the kernel to it."""
    N, C = w3.shape[:2]
    w = w3.new_zeros(N, 2, 2, C, 2, 2)           # n, sy, sx, c, ty, tx
    for ky, (ty, sy) in enumerate(_S2D_TAP):
        for kx, (tx, sx) in enumerate(_S2D_TAP):
            w[:, sy, sx, :, ty, tx] = w3[:, :, ky, kx]
    return w.reshape(N, 4 * C, 2, 2)


def _s2d_weight_grad(dw, C):
    """Gradient of _s2d_weight: [N,4C,2,2] -> [N,C,3,3]."""
    N = dw.shape[0]
    d = dw.reshape(N, 2, 2, C, 2, 2)
    out = dw.new_empty(N, C, 3, 3)
    for ky, (ty, sy) in enumerate(_S2D_TAP):
        for kx, (tx, sx) in enumerate(_S2D_TAP):
            out[:, :, ky, kx] = d[:, sy, sx, :, ty, tx]
    return out


def _pair_structure_ok(block):
    """A unit whose first convolution is 3x3 / stride 2 / pad 1 with a 1x1 / stride 2 shortcut: the pair that runs on the
    stride-1 kernels over a space-to-depth copy of the input.  (Module structure only: what _prepare_packs goes by.)"""
    c1 = getattr(block, "conv1", None)
    ds = block.downsample[0] if getattr(block, "downsample", None) is not None else None
    return (block.n == 2 and c1 is not None and ds is not None and c1.kernel_size == (3, 3) and c1.stride == (2, 2)
            and c1.padding == (1, 1) and c1.dilation == (1, 1) and c1.groups == 1 and ds.kernel_size == (1, 1)
            and ds.stride == (2, 2) and ds.padding == (0, 0) and ds.groups == 1)


def _pair_ok(block, C, H, W):
    """Does `block` take the space-to-depth pair (_StridedPairFn) for a channels_last [B, C, H, W] input?  Even sizes, and
    channel counts its kernels and the norm kernels behind them take."""
    return (S2D_UNITS and _pair_structure_ok(block) and H % 2 == 0 and W % 2 == 0 and C % 4 == 0
            and _cl_channels_ok(block.conv1.out_channels))


def _pair_packs(block):
    """The _PairPacks of a stride-2 residual unit: its first convolution as 2x2 over space-to-depth (the rewrite
    `input row 2y - 1 + k = 2(y + t - 1) + s` maps 3x3 tap k to (2x2 tap t, sub-pixel s), 7 of the 16 (tap, sub-pixel) slots
    are structural zeros) and its 1x1 shortcut; cached and rebuilt like _weight_packs."""
    if _stale(block, "_fs_pair_packs", _pair_key(block)):
        _prepare_packs(block)
    return block.__dict__["_fs_pair_packs"]


class _StridedPairFn(torch.autograd.Function):
    """First convolution (3x3, stride 2, pad 1) and shortcut (1x1, stride 2) of a stride-2 ResidualBlock
    (pytorch/core/extractor.py:13, 39) on the stride-1 kernels: the channels_last input is permuted once to
    space-to-depth order ([B,H/2,W/2,4C], fsraft_space_to_depth2); over that tensor the 3x3 becomes a 2x2 convolution
    with 4C input channels (pad 1 forward, pad 0 in the data gradient) and the shortcut a 1x1 over its first C channels.
    Both data gradients land in one [B,H/2,W/2,4C] buffer (the shortcut's accumulates into channels [0, C)) that is
    permuted back once.  No MIOpen call, no NCHW hop.  Biases are the caller's business (dropped before InstanceNorm,
    folded into a frozen BatchNorm)."""

    @staticmethod
    def forward(ctx, x, w3, wsc, packs, pre=False):
        x = _as_cl(x)
        ctx.pre = pre
        if pre:         # x already IS the space-to-depth tensor [B, 4C, H/2, W/2] (written by the norm before it: _S2D)
            B, C4, h, w = x.shape
            C, H, W = C4 // 4, 2 * h, 2 * w
            xs = x.permute(0, 2, 3, 1)
        else:
            B, C, H, W = x.shape
            h, w = H // 2, W // 2
            xs = ops.space_to_depth2(x.permute(0, 2, 3, 1))
        N, Ns = w3.shape[0], wsc.shape[0]
        y1 = torch.empty(B, h, w, N, device=x.device, dtype=torch.float32)
        ys = torch.empty(B, h, w, Ns, device=x.device, dtype=torch.float32)
        p, q = packs.conv3, packs.shortcut
        ops.conv_forward([ops.V(xs, 4 * C)], p.fwd, None, B, h, w, 2, 2, N, [ops.Dst.nhwc(y1)], wpk_split=p.fwd_split)
        ops.conv_forward([ops.V(xs, C, 0)], q.fwd, None, B, h, w, 1, 1, Ns, [ops.Dst.nhwc(ys)], wpk_split=q.fwd_split)
        ctx.save_for_backward(xs, w3, wsc)
        ctx.packs = packs
        return y1.permute(0, 3, 1, 2), ys.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g1, gs):
        xs, w3, wsc = ctx.saved_tensors
        B, h, w, C4 = xs.shape
        C, N, Ns = C4 // 4, w3.shape[0], wsc.shape[0]
        p, q = ctx.packs.conv3, ctx.packs.shortcut
        g1v = ops.V(_as_cl(g1).permute(0, 2, 3, 1), N)
        gsv = ops.V(_as_cl(gs).permute(0, 2, 3, 1), Ns)
        dx = dw3 = dwsc = None
        if ctx.needs_input_grad[0]:
            dxs = torch.empty(B, h, w, C4, device=xs.device, dtype=torch.float32)
            ops.conv_forward([g1v], p.dgrad, None, B, h, w, 2, 2, C4, [ops.Dst.nhwc(dxs)], wpk_split=p.dgrad_split, pad=(0, 0))
            ops.conv_forward([gsv], q.dgrad, None, B, h, w, 1, 1, C, [ops.Dst.nhwc(dxs, 0, 0, True)], wpk_split=q.dgrad_split)
            dx = (dxs if ctx.pre else ops.space_to_depth2(dxs, inverse=True)).permute(0, 3, 1, 2)
        items = []
        if ctx.needs_input_grad[1]:
            dwpk = ops.zeros(N, ops.conv_ktot([C4], 2, 2), device=xs.device)
            ops.conv_wgrad(g1v, [ops.V(xs, C4)], dwpk, B, h, w, 2, 2)
            dw3 = torch.empty(N, C, 3, 3, device=xs.device, dtype=torch.float32)
            items.append((dwpk, [dw3], [C4], [0], C, 2, 2, 1.0, True))       # gradient of the space-to-depth rewrite: a gather
        if ctx.needs_input_grad[2]:
            dwpk = ops.zeros(Ns, ops.conv_ktot([C], 1, 1), device=xs.device)
            ops.conv_wgrad(gsv, [ops.V(xs, C, 0)], dwpk, B, h, w, 1, 1)
            dwsc = torch.empty(Ns, C, 1, 1, device=xs.device, dtype=torch.float32)
            items.append((dwpk, [dwsc], [C], [0], C, 1, 1, 1.0, False))
        ops.unpack_weight_grads(items, xs.device)
        return dx, dw3, dwsc, None, None


def _norm_kind(norm):
    """Which fsraft norm + ReLU kernels cover `norm`: "instance" (InstanceNorm2d without affine parameters or running
    statistics), "frozen_bn" (affine BatchNorm2d using its running statistics: eval mode / freeze_bn), or None."""
    if isinstance(norm, nn.InstanceNorm2d) and not norm.affine and not norm.track_running_stats:
        return "instance"
    if isinstance(norm, nn.BatchNorm2d) and not norm.training and norm.track_running_stats and norm.affine:
        return "frozen_bn"
    return None


def _train_bn_ok(norm):
    """An affine BatchNorm2d in training mode that tracks running statistics with a float momentum: what csrc/norm_bn.hip
    covers on channels_last tensors (_TrainBNReluCL).  momentum=None, the cumulative average, would need num_batches_tracked
    on the host, so it stays the framework's."""
    return (isinstance(norm, nn.BatchNorm2d) and norm.training and norm.affine and norm.track_running_stats
            and isinstance(norm.momentum, float))


def _covered(norm):
    """Does a fused norm + ReLU kernel cover `norm` on the channels_last path?"""
    return _norm_kind(norm) is not None or (TRAIN_BN and _train_bn_ok(norm))


def _norm_act(norm, y, cbias, relu, res=None, link=None, sums=None, s2d=False, cl=True):
    """relu?(norm(y + cbias)), or relu(res + that), for the output y of a convolution that ran without its bias cbias (or
    None) and a norm of a kind _norm_kind names, or a training-mode BatchNorm (_train_bn_ok) on the channels_last kernels.
    cl: on the channels_last kernels (where they take y's channel count),
    which fuse the residual and take `link` (the unit's _ResLink), `sums` (the convolution's _NormSums) and `s2d` (see _S2D);
    else on the NCHW ones.  An InstanceNorm removes a per-channel constant again, so cbias is dropped there."""
    kind = _norm_kind(norm)
    cl = cl and _cl_channels_ok(y.shape[1])
    if kind is None and cl and _covered(norm):       # training-mode BatchNorm: channels_last kernels only
        return _TrainBNReluCL.apply(y, cbias, norm.weight, norm.bias, norm, relu, res, link, s2d)
    if kind is None:
        raise RuntimeError(f"no fsraft norm kernel covers {norm!r}")
    assert cl or not s2d, "space-to-depth output is a feature of the fused channels_last norm kernels"
    if kind == "instance":
        if cl:
            return _InstNormReluCL.apply(y, norm.eps, relu, res, link, sums, s2d)
        y = _InstNormRelu.apply(y, norm.eps, relu)
    else:
        bn = (y, cbias, norm.weight, norm.bias, norm.running_mean, norm.running_var, norm.eps, relu)
        if cl:
            return _FrozenBNReluCL.apply(*bn, res, link, s2d)
        y = _FrozenBNRelu.apply(*bn)
    return y if res is None else F.relu(res + y)


S2D_EMIT = True   # False: the stride-2 units copy their input into the space-to-depth layout themselves


class _S2D:
    """A residual unit's output handed to the stride-2 unit behind it AS the space-to-depth tensor that unit's two convolutions
    read ([B, 4C, H/2, W/2] channels_last; sub-pixel (sy, sx) of pixel (2y + sy, 2x + sx) in channels (2 sy + sx) C ..): the
    unit's last norm kernel writes it in that layout and reads the gradient from it, so neither direction needs a copy."""
    __slots__ = ("t",)

    def __init__(self, t):
        self.t = t


def _conv_norm(conv, norm, x, relu, to_cl=False, res=None, link=None, res_link=None, s2d=False):
    """relu?(norm(conv(x))) of pytorch/core/extractor.py, or relu(res + that).  For an fp32 CUDA tensor outside autocast
    and a norm that _norm_kind names, the convolution runs WITHOUT its bias on the route _conv picks (fsraft kernels for a
    channels_last input or the stem, else MIOpen) and the norm + ReLU on the fsraft kernels (_norm_act):
      * non-affine InstanceNorm2d (feature encoder).  A per-channel constant added before it is removed again by its
        mean subtraction: same output (to rounding), one bias-add kernel less forward and one [N,H,W] reduction less
        backward.  The bias then receives no gradient (mathematically it is exactly zero; parallel.FlatGradients keeps a
        zero for it, so the optimizer treats it as the reference does);
      * BatchNorm2d using running statistics (context encoder after freeze_bn, or eval mode): the bias joins the shift;
      * BatchNorm2d in training mode (_train_bn_ok, switch TRAIN_BN) on a channels_last chain: csrc/norm_bn.hip.  The bias
        joins the running mean and, as in front of an InstanceNorm, receives no gradient.  On an NCHW chain it is the
        framework's module.
    Everything else (GroupNorm, autocast dtypes, CPU) is the framework's own modules.
    A channels_last input (or to_cl) keeps the chain channels_last: the [N][HW][C] twins of the norm kernels are used, and
    they convert the convolution's output if the library handed back NCHW.  link / res_link: the unit's _ResLink, for its
    first convolution / for the norm that fuses the shortcut `res`."""
    kind = _norm_kind(norm)
    if kind is not None and x.is_cuda and x.dtype == torch.float32 and not torch.is_autocast_enabled():
        cl = to_cl or _is_cl(x)
        sums = _NormSums() if (kind == "instance" and cl) else None
        y = _conv(conv, x, None, link, stem_cl=to_cl, sums=sums)
        return _norm_act(norm, y, conv.bias, relu, res, res_link, sums, s2d, cl)
    if (kind is None and _covered(norm) and x.is_cuda and x.dtype == torch.float32 and not torch.is_autocast_enabled()
            and (to_cl or _is_cl(x))):
        # training-mode BatchNorm on a channels_last chain: the batch mean removes the bias from the output, the kernel adds it to
        # the running mean; without a kernel for the channel count, the framework's module on conv(x) with its bias
        if _cl_channels_ok(conv.out_channels):
            return _norm_act(norm, _conv(conv, x, None, link, stem_cl=to_cl), conv.bias, relu, res, res_link, None, s2d)
        assert not s2d, "space-to-depth output is a feature of the fused channels_last norm kernels"
        y = norm(_conv(conv, x, conv.bias))
        y = F.relu(y, inplace=True) if relu else y
        return y if res is None else F.relu(res + y)
    assert not s2d, "space-to-depth output is a feature of the fused channels_last norm kernels"
    if kind == "instance" and conv.bias is not None:        # (as above: the bias changes nothing)
        y = F.conv2d(x, conv.weight, None, conv.stride, conv.padding, conv.dilation, conv.groups)
    else:
        y = conv(x)
    y = norm(y)
    y = F.relu(y, inplace=True) if relu else y
    return y if res is None else F.relu(res + y)


def _make_norm(kind, ch, groups):
    if kind == "group":
        return nn.GroupNorm(num_groups=groups, num_channels=ch)
    if kind == "batch":
        return nn.BatchNorm2d(ch)
    if kind == "instance":
        return nn.InstanceNorm2d(ch)
    if kind == "none":
        return nn.Sequential()
    raise ValueError(kind)


class _Block(nn.Module):
    """Residual unit.  `widths` lists (out_channels, kernel) of its convolutions; the first 3x3
    carries the stride.  The shortcut norm is the same module object as downsample[1], which is
    why it also appears under its own name (norm3 / norm4) in reference checkpoints."""

    def __init__(self, cin, cout, norm_fn, stride, bottleneck):
        super().__init__()
        mid = cout // 4
        if bottleneck:
            spec = [(cin, mid, 1, 1), (mid, mid, 3, stride), (mid, cout, 1, 1)]
        else:
            spec = [(cin, cout, 3, stride), (cout, cout, 3, 1)]
        groups = cout // 8
        self.n = len(spec)
        for i, (a, b, k, s) in enumerate(spec, 1):
            setattr(self, f"conv{i}", nn.Conv2d(a, b, kernel_size=k, padding=k // 2, stride=s))
        for i, (a, b, k, s) in enumerate(spec, 1):
            setattr(self, f"norm{i}", _make_norm(norm_fn, b, groups))
        self.relu = nn.ReLU(inplace=True)
        self.downsample = None
        if stride != 1:
            short = _make_norm(norm_fn, cout, groups)
            setattr(self, f"norm{self.n + 1}", short)
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, kernel_size=1, stride=stride), short)

    def forward(self, x, emit_for=None):
        """emit_for: the stride-2 unit that consumes this unit's output (the encoder's channels_last walk passes it): the output then
        leaves as an _S2D holder where that unit can take it."""
        if isinstance(x, _S2D):
            return self._strided_pair(x.t, True)
        cl = _is_cl(x)
        if cl and self.downsample is not None and _pair_ok(self, *x.shape[1:]):
            return self._strided_pair(x, False)
        if cl and self.downsample is not None:
            x = _ToNCHW.apply(x)        # the strided convolutions (first 3x3 / shortcut 1x1) are MIOpen NCHW calls: one copy for both
        y = x
        # stride-1 unit on the channels_last path: x feeds the first convolution AND the shortcut -- their two gradients are
        # merged inside the convolution's data-gradient epilogue instead of by an autograd add (_ResLink)
        link = _ResLink() if (cl and self.downsample is None and self.n >= 2 and torch.is_grad_enabled() and x.requires_grad) else None
        if self.downsample is not None:
            x = _conv_norm(self.downsample[0], self.downsample[1], x, False, to_cl=cl)
        for i in range(1, self.n):
            y = _conv_norm(getattr(self, f"conv{i}"), getattr(self, f"norm{i}"), y, True, to_cl=cl, link=link if i == 1 else None)
        # last convolution of the unit: relu(x + relu(norm(conv(y)))), the add and outer ReLU fused into the norm kernel
        last, norm = getattr(self, f"conv{self.n}"), getattr(self, f"norm{self.n}")
        # (whether a kernel covers the norm decides, not its class: _conv_norm asserts on s2d for a norm without one, a
        #  GroupNorm say, so a unit in front of a stride-2 unit emits only what its own norm kernel can write)
        emit = bool(cl and S2D_EMIT and emit_for is not None and self.downsample is None and _is_cl(y)
                    and _cl_channels_ok(last.out_channels) and _pair_ok(emit_for, last.out_channels, y.shape[2], y.shape[3])
                    and _covered(norm))
        out = _conv_norm(last, norm, y, True, to_cl=cl, res=x, res_link=link, s2d=emit)
        return _S2D(out) if emit else out

    def _strided_pair(self, x, pre):
        """Stride-2 unit, channels_last: both strided convolutions on the stride-1 kernels over the space-to-depth input.
        pre: x already is that tensor (the `t` of an _S2D)."""
        y1, ys = _StridedPairFn.apply(x, self.conv1.weight, self.downsample[0].weight, _pair_packs(self), pre)
        y = _norm_act(self.norm1, y1, self.conv1.bias, True)
        xs = _norm_act(self.downsample[1], ys, self.downsample[0].bias, False)
        return _conv_norm(self.conv2, self.norm2, y, True, to_cl=True, res=xs)


class ResidualBlock(_Block):
    def __init__(self, in_planes, planes, norm_fn="group", stride=1):
        super().__init__(in_planes, planes, norm_fn, stride, bottleneck=False)


class BottleneckBlock(_Block):
    def __init__(self, in_planes, planes, norm_fn="group", stride=1):
        super().__init__(in_planes, planes, norm_fn, stride, bottleneck=True)


def _channels_last_ok(enc, x):
    """Channels_last encoder path: fp32 CUDA, no autocast, norms that the fused channels_last kernels cover (non-affine
    InstanceNorm, BatchNorm on running statistics, training-mode BatchNorm while TRAIN_BN).  FSRAFT_ENCODER_CL=0 keeps the
    encoder NCHW on MIOpen throughout."""
    mode = int(os.environ.get("FSRAFT_ENCODER_CL", "1"))
    if mode == 0 or not (x.is_cuda and x.dtype == torch.float32) or torch.is_autocast_enabled():
        return 0
    return mode if _covered(enc.norm1) else 0


class _Encoder(nn.Module):
    def __init__(self, widths, block, stem_groups, output_dim, norm_fn, dropout):
        super().__init__()
        self.norm_fn = norm_fn
        c0, c1, c2 = widths
        self.norm1 = _make_norm(norm_fn, c0, stem_groups)
        self.conv1 = nn.Conv2d(3, c0, kernel_size=7, stride=2, padding=3)
        self.relu1 = nn.ReLU(inplace=True)
        self.layer1 = nn.Sequential(block(c0, c0, norm_fn, 1), block(c0, c0, norm_fn, 1))
        self.layer2 = nn.Sequential(block(c0, c1, norm_fn, 2), block(c1, c1, norm_fn, 1))
        self.layer3 = nn.Sequential(block(c1, c2, norm_fn, 2), block(c2, c2, norm_fn, 1))
        self.conv2 = nn.Conv2d(c2, output_dim, kernel_size=1)
        self.dropout = nn.Dropout2d(p=dropout) if dropout > 0 else None
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, (nn.BatchNorm2d, nn.InstanceNorm2d, nn.GroupNorm)):
                if m.weight is not None:
                    nn.init.constant_(m.weight, 1)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    @on_tensor_device
    def forward(self, x):
        pair = isinstance(x, (tuple, list))
        if pair:
            n = x[0].shape[0]
            x = torch.cat(x, dim=0)
        # channels_last after the stem (NCHW image in: _StemFn, or a MIOpen call): the stride-1 convolutions then run on the
        # fsraft implicit-GEMM kernels and the norm + ReLU kernels read and write [N][HW][C] directly
        cl = _channels_last_ok(self, x)
        if cl:
            _prepare_packs(self)         # all packed weight images of this encoder that are stale: one batched launch
        x = _conv_norm(self.conv1, self.norm1, x, True, to_cl=bool(cl))
        if cl:
            # (the Sequential containers walked by hand: a unit in front of a stride-2 unit is told so, see _S2D)
            stages = (self.layer1, self.layer2, self.layer3)
            for si, seq in enumerate(stages):
                units = list(seq)
                for ui, unit in enumerate(units):
                    nxt = stages[si + 1][0] if (ui == len(units) - 1 and si + 1 < len(stages)) else None
                    x = unit(x, nxt) if isinstance(unit, _Block) else unit(x)
        else:
            x = self.layer3(self.layer2(self.layer1(x)))
        if cl:
            x = _conv(self.conv2, x, self.conv2.bias)
            # out_channels_last (set by the models on their context encoder): the result stays a channels_last tensor -- its
            # consumers (split, tanh / ReLU, update.to_channels_last) work on it in place of three layout copies per direction
            if pair or not getattr(self, "out_channels_last", False) or not _is_cl(x):
                x = _ToNCHW.apply(x)
        else:
            x = self.conv2(x)
        if self.training and self.dropout is not None:
            x = self.dropout(x)
        if pair:
            x = torch.split(x, [n, n], dim=0)
        return x


class BasicEncoder(_Encoder):
    """extractor.py:118-192: 64/96/128 residual stages to 1/8 resolution."""

    def __init__(self, output_dim=128, norm_fn="batch", dropout=0.0):
        super().__init__((64, 96, 128), ResidualBlock, 8, output_dim, norm_fn, dropout)


class SmallEncoder(_Encoder):
    """extractor.py:195-267: 32/64/96 bottleneck stages."""

    def __init__(self, output_dim=128, norm_fn="batch", dropout=0.0):
        super().__init__((32, 64, 96), BottleneckBlock, 8, output_dim, norm_fn, dropout)
