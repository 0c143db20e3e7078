"""The image plumbing of the reference's TensorFlow tree on csrc/image_ops.hip:

    crop_bboxes(images, offsets, target_size)      util/image.py:6-25      per-sample windows of a batch of frames
    pad_bboxes(images, offsets, target_size)       util/image.py:28-49     per-sample zero padding of windows into frames
    get_proc_size(size, multiple=8)                raft/__init__.py:199-203
    resize(im, size)                               raft/__init__.py:206-211 tf.image.resize's default; the input itself at `size`
    resize_flow(flow, size, scaling=True)          raft/__init__.py:213-222 resize, channel 0 * W_out / W_in, channel 1 * H_out / H_in
    pad_edge(tensor, paddings)                     util/pad.py:5-11        np.pad(..., 'edge')
    pad_inputs(*inputs, mode=None) / unpad_inputs(*inputs, pad=None)        util/validate.py:301-325

Tensors are [B,H,W,C] (layout 'nhwc', the TF tree's) or [B,C,H,W] ('nchw').  Where the reference loops over a list -- the 24
crop_bboxes of Semisupervised.call (raft/semi.py:215-293), `_r` over the 12 predictions of a model -- pass the list: up to 32
same-shaped tensors are ONE launch and one autograd node (longer lists are split), and a list comes back as a list.  crop_bboxes,
pad_bboxes, resize and resize_flow are differentiable, each backward one launch; pad_edge is not, as the reference's
tf.numpy_function is not.  Offsets are host integers ([B,2] of (y, x), a list or a CPU tensor).

Not provided: central_pad, central_crop, warp_image, create_outgoing_mask (util/image.py:52-114), compute_ae: the reference imports
or defines them and never calls them.  TensorFlow is not installed here: the oracle is a restatement of the documented semantics
(tests/_imageref.py); parity with TensorFlow itself is unpinned.  There is no CPU implementation.
"""
import ctypes

import torch

from .. import _lib as L
from .. import image_ops as I


def _listed(images, what):
    """(list of tensors, whether a single tensor was passed)"""
    single = isinstance(images, torch.Tensor)
    ts = [images] if single else list(images)
    if not ts or not all(isinstance(t, torch.Tensor) for t in ts):
        raise ValueError(f"{what}: a tensor or a non-empty list of tensors")
    if not all(t.is_cuda for t in ts):
        raise RuntimeError("fsraft ops need CUDA (ROCm) tensors; the hot path has no CPU implementation")
    shape = tuple(ts[0].shape)
    for t in ts:
        if tuple(t.shape) != shape:
            raise ValueError(f"{what}: the tensors of a list share one shape, got {shape} and {tuple(t.shape)}")
    if len(shape) != 4:
        raise ValueError(f"{what}: tensors are [B,H,W,C] or [B,C,H,W], got {shape}")
    return ts, single


def _chunks(ts):
    return [ts[i:i + I.MAX_LIST] for i in range(0, len(ts), I.MAX_LIST)]


def _hw(t, layout):
    h, w, _ = I.LAYOUTS[layout]
    return t.shape[h], t.shape[w]


def _size(size):
    if isinstance(size, torch.Tensor):
        if size.is_cuda:
            raise RuntimeError("a size is read on the host: pass a CPU tensor or a pair of integers")
        size = size.tolist()
    h, w = (int(v) for v in size)
    if h < 1 or w < 1:
        raise ValueError(f"size {(h, w)}")
    return h, w


def _box(images, offsets, target_size, layout, place, what):
    I._check_layout(layout)
    ts, single = _listed(images, what)
    size = _size(target_size)
    own = _hw(ts[0], layout)
    yx = I.window_offsets(offsets, ts[0].shape[0], *((size, own) if place else (own, size)))
    out = []
    for chunk in _chunks(ts):
        out += I.BoxCopyFn.apply(yx, size, place, layout, *chunk)
    return out[0] if single else out


@L.on_tensor_device
def crop_bboxes(images, offsets, target_size, layout="nhwc"):
    """images[b, y:y+h, x:x+w] with (y, x) = offsets[b] and (h, w) = target_size, for a tensor or a list of same-shaped tensors."""
    return _box(images, offsets, target_size, layout, False, "crop_bboxes")


@L.on_tensor_device
def pad_bboxes(images, offsets, target_size, layout="nhwc"):
    """Sample b zero-padded to (h, w) = target_size with its top-left corner at (y, x) = offsets[b]."""
    return _box(images, offsets, target_size, layout, True, "pad_bboxes")


def get_proc_size(size, multiple=8):
    """`size` rounded up to a multiple of `multiple`, as a tuple of ints."""
    if isinstance(size, torch.Tensor):
        size = size.tolist()
    return tuple(-(-int(s) // multiple) * multiple for s in size)


def _resize(im, size, layout, scaling, what):
    I._check_layout(layout)
    ts, single = _listed(im, what)
    size = _size(size)
    hi, wi = _hw(ts[0], layout)
    if (hi, wi) == size:                  # the reference's tf.cond: the input itself (the flow factors are both 1.0)
        return im
    factors = None
    if scaling:
        c = I.LAYOUTS[layout][2]
        if ts[0].shape[c] != 2:
            raise ValueError(f"resize_flow: a flow has two channels, got {tuple(ts[0].shape)}")
        # the quotients in float32 (raft/__init__.py:218); a double quotient of two integers below 2^24 rounds to the same float
        factors = tuple((ctypes.c_float * 2)(size[1] / wi, size[0] / hi))
    out = []
    for chunk in _chunks(ts):
        out += I.ResizeFn.apply(size, factors, layout, *chunk)
    return out[0] if single else out


@L.on_tensor_device
def resize(im, size, layout="nhwc"):
    """tf.image.resize(im, size) (bilinear, half-pixel centres, no antialias) of a tensor or a list; `im` itself when it is at `size`."""
    return _resize(im, size, layout, False, "resize")


@L.on_tensor_device
def resize_flow(flow, size, scaling=True, layout="nhwc"):
    """resize(flow, size) with channel 0 (x) multiplied by W_out / W_in and channel 1 (y) by H_out / H_in, in the same launch."""
    return _resize(flow, size, layout, scaling, "resize_flow")


def _pads(paddings):
    """(top, bottom, left, right) of [[0,0],[t,b],[l,r],[0,0]] (the H and W rows of an NHWC paddings list) or of a 4-tuple."""
    p = paddings.tolist() if isinstance(paddings, torch.Tensor) else list(paddings)
    if len(p) == 4 and all(isinstance(r, (list, tuple)) for r in p):
        if any(int(v) != 0 for v in list(p[0]) + list(p[3])):
            raise ValueError("pad_edge: only H and W are padded")
        return int(p[1][0]), int(p[1][1]), int(p[2][0]), int(p[2][1])
    if len(p) == 4:
        return tuple(int(v) for v in p)
    raise ValueError("pad_edge: paddings are [[0,0],[top,bottom],[left,right],[0,0]] or (top, bottom, left, right)")


@L.on_tensor_device
def pad_edge(tensor, paddings, layout="nhwc"):
    """np.pad(tensor, paddings, 'edge') on H and W, for a tensor or a list of same-shaped tensors.  Not differentiable."""
    I._check_layout(layout)
    ts, single = _listed(tensor, "pad_edge")
    pads = _pads(paddings)
    out = []
    with torch.no_grad():
        for chunk in _chunks([t.detach() for t in ts]):
            out += I.pad_edge(chunk, pads, layout)
    return out[0] if single else out


def input_padding(ht, wd, mode=None):
    """The paddings of pad_inputs for an ht x wd input (util/validate.py:302-309): up to the next multiple of 8; 'sintel' splits both
    dimensions, anything else pads the height at the bottom only."""
    pad_ht = (((ht // 8) + 1) * 8 - ht) % 8
    pad_wd = (((wd // 8) + 1) * 8 - wd) % 8
    if mode == "sintel":
        return [[0, 0], [pad_ht // 2, pad_ht - pad_ht // 2], [pad_wd // 2, pad_wd - pad_wd // 2], [0, 0]]
    return [[0, 0], [0, pad_ht], [pad_wd // 2, pad_wd - pad_wd // 2], [0, 0]]


@L.on_tensor_device
def pad_inputs(*inputs, mode=None, layout="nhwc"):
    """(the inputs edge-padded to multiples of 8, the paddings) -- inputs of one shape and one set of strides share a launch."""
    I._check_layout(layout)
    ts, _ = _listed(inputs[:1], "pad_inputs")
    pad = input_padding(*_hw(ts[0], layout), mode)
    groups = {}
    for i, t in enumerate(inputs):
        groups.setdefault((tuple(t.shape), t.stride()), []).append(i)
    out = [None] * len(inputs)
    for idx in groups.values():
        for i, o in zip(idx, pad_edge([inputs[i] for i in idx], pad, layout)):
            out[i] = o
    return out, pad


def unpad_inputs(*inputs, pad=None, layout="nhwc"):
    """The views inp[:, top:H-bottom, left:W-right] that undo pad_inputs."""
    I._check_layout(layout)
    h, w, _ = I.LAYOUTS[layout]
    ht, wd = inputs[0].shape[h], inputs[0].shape[w]
    top, bottom, left, right = _pads(pad)
    return [t.narrow(h, top, ht - bottom - top).narrow(w, left, wd - right - left) for t in inputs]
