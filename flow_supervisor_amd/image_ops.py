"""Per-sample box copies, bilinear resize and edge padding on csrc/image_ops.hip, in list form: the launches behind
raft_tf.image (the TF tree's util/image.py, resize / resize_flow, pad_inputs) and behind the per-sample branches of core/l2l.py.

Every function takes a LIST of tensors of one shape -- [B,H,W,C] under layout 'nhwc', [B,C,H,W] under 'nchw' -- and returns a
list: up to 32 tensors go through one launch, and their outputs are slices of one allocation.  Tensors are read through their
strides; a list whose members do not share them is made contiguous first.  There is no CPU implementation.
"""
import ctypes

import torch

from . import _lib as L
from . import ops

MAX_LIST = 32
LAYOUTS = ops.FLOW_LAYOUTS          # layout -> the dims of H, W and the channels


def _check_layout(layout):
    if layout not in LAYOUTS:
        raise ValueError(f"image ops: layout is 'nhwc' or 'nchw', got {layout!r}")


def _strides(t, layout):
    h, w, c = LAYOUTS[layout]
    return t.stride(0), t.stride(c), t.stride(h), t.stride(w)


def _dims(t, layout):
    """(B, C, H, W)"""
    h, w, c = LAYOUTS[layout]
    return t.shape[0], t.shape[c], t.shape[h], t.shape[w]


def _shape(B, C, H, W, layout):
    return (B, H, W, C) if layout == "nhwc" else (B, C, H, W)


def _prepare(srcs, layout, what):
    """The list as one launch takes it: 1..32 fp32 CUDA tensors of one 4-d shape and one set of strides."""
    srcs = list(srcs)
    if not 1 <= len(srcs) <= MAX_LIST:
        raise ValueError(f"{what}: 1 to {MAX_LIST} tensors per launch, got {len(srcs)}")
    L.require_cuda_f32(*srcs)
    shape = tuple(srcs[0].shape)
    if len(shape) != 4:
        raise ValueError(f"{what}: tensors are {'[B,H,W,C]' if layout == 'nhwc' else '[B,C,H,W]'}, got {shape}")
    for t in srcs:
        if tuple(t.shape) != shape:
            raise ValueError(f"{what}: the tensors of a list share one shape, got {shape} and {tuple(t.shape)}")
    if any(t.stride() != srcs[0].stride() for t in srcs):
        srcs = [t.contiguous() for t in srcs]
    return srcs


def _outputs(n, shape, like):
    """n outputs of `shape` as slices of one allocation."""
    return list(torch.empty((n,) + tuple(shape), device=like.device, dtype=torch.float32).unbind(0))


def window_offsets(offsets, B, frame, window):
    """The [B,2] (y, x) offsets as the host int array the entry takes.  A device tensor is refused (reading it would synchronise);
    a window that leaves the frame is a ValueError here, before anything is enqueued."""
    yx = ops.crop_offsets(offsets, B)
    if yx is None:
        raise ValueError("box copy: offsets [B,2] of (y, x) are needed")
    (Hf, Wf), (H, W) = frame, window
    for b in range(B):
        y, x = yx[2 * b], yx[2 * b + 1]
        if y < 0 or x < 0 or y + H > Hf or x + W > Wf:
            raise ValueError(f"box copy: the {H} x {W} window of sample {b} at (y, x) = ({y}, {x}) does not fit the {Hf} x {Wf} frame")
    return yx


def box_copy(srcs, yx, size, place, layout="nhwc"):
    """fsraft_box_copy, one launch.  place False: srcs are frames, the result their `size` = (H, W) windows at yx; place True: srcs
    are windows, the result `size` = (Hf, Wf) frames holding them at yx and +0.0 elsewhere.  yx: window_offsets()."""
    srcs = _prepare(srcs, layout, "box copy")
    B, C, Hs, Ws = _dims(srcs[0], layout)
    outs = _outputs(len(srcs), _shape(B, C, size[0], size[1], layout), srcs[0])
    (Hf, Wf), (H, W) = ((size, (Hs, Ws)) if place else ((Hs, Ws), size))
    fs, ws = (_strides(outs[0], layout), _strides(srcs[0], layout)) if place else (_strides(srcs[0], layout), _strides(outs[0], layout))
    sp, k1 = L.ptr_array(srcs)
    dp, k2 = L.ptr_array(outs)
    L.check(ops._lib().fsraft_box_copy(sp, dp, len(srcs), int(place), B, C, Hf, Wf, H, W, yx, *fs, *ws, L.stream()), "box_copy")
    return outs


def _factors(factors, C):
    if factors is None:
        return None
    if len(factors) != C:
        raise ValueError(f"resize: {len(factors)} factors for {C} channels")
    return (ctypes.c_float * C)(*factors)


def resize_bilinear(srcs, size, layout="nhwc", factors=None):
    """fsraft_resize_bilinear_fwd, one launch: tf.image.resize's default to `size` = (Ho, Wo), channel c times factors[c]."""
    srcs = _prepare(srcs, layout, "resize")
    B, C, Hi, Wi = _dims(srcs[0], layout)
    outs = _outputs(len(srcs), _shape(B, C, size[0], size[1], layout), srcs[0])
    sp, k1 = L.ptr_array(srcs)
    dp, k2 = L.ptr_array(outs)
    L.check(ops._lib().fsraft_resize_bilinear_fwd(sp, dp, len(srcs), B, C, Hi, Wi, size[0], size[1], *_strides(srcs[0], layout),
                                                  *_strides(outs[0], layout), _factors(factors, C), L.stream()), "resize_bilinear_fwd")
    return outs


def resize_bilinear_bwd(grads, size, layout="nhwc", factors=None):
    """fsraft_resize_bilinear_bwd, one launch: the gradients of the `size` = (Hi, Wi) sources from those of their resized forms."""
    grads = _prepare(grads, layout, "resize backward")
    B, C, Ho, Wo = _dims(grads[0], layout)
    outs = _outputs(len(grads), _shape(B, C, size[0], size[1], layout), grads[0])
    gp, k1 = L.ptr_array(grads)
    dp, k2 = L.ptr_array(outs)
    L.check(ops._lib().fsraft_resize_bilinear_bwd(gp, dp, len(grads), B, C, size[0], size[1], Ho, Wo, *_strides(outs[0], layout),
                                                  *_strides(grads[0], layout), _factors(factors, C), L.stream()), "resize_bilinear_bwd")
    return outs


def pad_edge(srcs, pads, layout="nhwc"):
    """fsraft_pad_edge, one launch: np.pad(..., 'edge') by pads = (top, bottom, left, right) on H and W."""
    srcs = _prepare(srcs, layout, "pad_edge")
    top, bottom, left, right = (int(p) for p in pads)
    if min(top, bottom, left, right) < 0:
        raise ValueError(f"pad_edge: negative padding {pads}")
    B, C, H, W = _dims(srcs[0], layout)
    outs = _outputs(len(srcs), _shape(B, C, H + top + bottom, W + left + right, layout), srcs[0])
    sp, k1 = L.ptr_array(srcs)
    dp, k2 = L.ptr_array(outs)
    L.check(ops._lib().fsraft_pad_edge(sp, dp, len(srcs), B, C, H, W, top, bottom, left, right, *_strides(srcs[0], layout),
                                       *_strides(outs[0], layout), L.stream()), "pad_edge")
    return outs


class BoxCopyFn(torch.autograd.Function):
    """A list of box copies as ONE autograd node: one launch forward, one backward (the copy the other way; a member whose result
    was not used receives zeros)."""

    @staticmethod
    def forward(ctx, yx, size, place, layout, *srcs):
        h, w, _ = LAYOUTS[layout]
        ctx.box = (yx, (srcs[0].shape[h], srcs[0].shape[w]), place, layout)
        return tuple(box_copy(srcs, yx, size, place, layout))

    @staticmethod
    def backward(ctx, *grads):
        yx, size, place, layout = ctx.box
        return (None, None, None, None) + tuple(box_copy(grads, yx, size, not place, layout))


class ResizeFn(torch.autograd.Function):
    """A list of bilinear resizes (with the flow factors, resize_flow) as ONE autograd node: one launch each way."""

    @staticmethod
    def forward(ctx, size, factors, layout, *srcs):
        h, w, _ = LAYOUTS[layout]
        ctx.geom = ((srcs[0].shape[h], srcs[0].shape[w]), factors, layout)
        return tuple(resize_bilinear(srcs, size, layout, factors))

    @staticmethod
    def backward(ctx, *grads):
        size, factors, layout = ctx.geom
        return (None, None, None) + tuple(resize_bilinear_bwd(grads, size, layout, factors))
