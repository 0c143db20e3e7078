"""The Middlebury colour wheel with the reference's names and signatures (pytorch/core/utils/flow_viz.py, identical under
GMA/core/utils/), coloured on the device (csrc/flow_viz.hip: fsraft_flow_rad_max, fsraft_flow_wheel).

    make_colorwheel()                                       flow_viz.py:20-67     float64 [55,3], host
    flow_uv_to_colors(u, v, convert_to_bgr=False)           flow_viz.py:70-106
    flow_to_image(flow_uv, clip_flow=None, convert_to_bgr=False)      flow_viz.py:109-132

The reference takes the prediction after `.permute(1, 2, 0).cpu().numpy()` and colours it in NumPy.  Here a device tensor
[2,H,W] or [B,2,H,W] (planar, what the models return; any view with a unit x stride, so InputPadder.unpad of a padded
prediction is read in place) gives a device uint8 [H,W,3] or [B,H,W,3], every sample normalised by its own maximum, without
a host read: the call can be captured in a graph.  A NumPy [H,W,2] array, the reference's argument, is sent through the device
and comes back as NumPy uint8 [H,W,3], so a caller like GMA/train.py:30-33 runs unchanged.  The formula, the treatment of
non-finite pixels (black; the reference's np.max would be poisoned) and the `clip_flow` quirk (np.clip(flow_uv, 0, clip_flow):
negative components go to 0) are defined in include/fsraft.h.
"""
import numpy as np
import torch

from ... import ops
from ..._lib import on_tensor_device


def make_colorwheel():
    """The 55 x 3 colour wheel of Baker et al., "A Database and Evaluation Methodology for Optical Flow" (ICCV 2007):
    RY 15, YG 6, GC 4, CB 11, BM 13, MR 6 entries, float64 in 0 .. 255."""
    wheel = np.zeros((55, 3))
    col = 0
    for n, rising, falling in ((15, 1, None), (6, None, 0), (4, 2, None), (11, None, 1), (13, 0, None), (6, None, 2)):
        ramp = np.floor(255 * np.arange(n) / n)
        if rising is not None:            # one channel full, the next one rising
            wheel[col:col + n, (rising + 2) % 3] = 255
            wheel[col:col + n, rising] = ramp
        else:                             # one channel full, the previous one falling
            wheel[col:col + n, (falling + 1) % 3] = 255
            wheel[col:col + n, falling] = 255 - ramp
        col += n
    return wheel


def _planar(flow, what):
    """A device [B,2,H,W] fp32 view with unit x stride, and how to shape the result back."""
    if flow.dim() == 3:
        flow, single = flow[None], True
    else:
        single = False
    if flow.dim() != 4 or flow.shape[1] != 2:
        raise ValueError(f"{what}: a device flow is [2,H,W] or [B,2,H,W], got {tuple(flow.shape)}")
    flow = flow.detach()
    if flow.shape[-1] > 1 and flow.stride(-1) != 1:
        flow = flow.contiguous()
    return flow, single


@on_tensor_device
def _to_image(flow, clip_flow, convert_to_bgr, return_scale, scale):
    flow, single = _planar(flow, "flow_to_image")
    clip = 0.0 if clip_flow is None else float(clip_flow)
    if clip_flow is not None and not clip > 0.0:
        raise ValueError(f"flow_to_image: clip_flow must be positive, got {clip_flow}")
    rad_max = None
    if scale is None or return_scale:
        rad_max = ops.flow_rad_max(flow, clip)
    if scale is None:
        img = ops.flow_colors(flow, rad_max=rad_max, clip=clip, bgr=convert_to_bgr)
    else:
        img = ops.flow_colors(flow, scale=scale, clip=clip, bgr=convert_to_bgr)
    img = img[0] if single else img
    return (img, rad_max) if return_scale else img


def flow_to_image(flow_uv, clip_flow=None, convert_to_bgr=False, return_scale=False, scale=None):
    """flow_viz.py:109-132.  flow_uv: a device tensor [2,H,W] / [B,2,H,W] -> device uint8 [H,W,3] / [B,H,W,3]; or a NumPy
    [H,W,2] array -> NumPy uint8 [H,W,3].  clip_flow clamps both components to [0, clip_flow] first, as the reference does.
    Extras: return_scale=True also returns the device float[B] of the samples' maxima; scale= (a host number) replaces
    `rad_max + 1e-5` as the normaliser, for a sequence coloured on one scale."""
    if isinstance(flow_uv, np.ndarray):
        assert flow_uv.ndim == 3, 'input flow must have three dimensions'
        assert flow_uv.shape[2] == 2, 'input flow must have shape [H,W,2]'
        dev = torch.from_numpy(np.ascontiguousarray(flow_uv, dtype=np.float32)).cuda().permute(2, 0, 1).contiguous()
        res = _to_image(dev, clip_flow, convert_to_bgr, return_scale, scale)
        return (res[0].cpu().numpy(), res[1]) if return_scale else res.cpu().numpy()
    return _to_image(flow_uv, clip_flow, convert_to_bgr, return_scale, scale)


@on_tensor_device
def _uv_to_colors(u, v, convert_to_bgr):
    if u.shape != v.shape or u.dim() not in (2, 3):
        raise ValueError(f"flow_uv_to_colors: u {tuple(u.shape)} and v {tuple(v.shape)} must be equal [H,W] or [B,H,W] planes")
    flow = torch.stack([u.detach(), v.detach()], dim=-3)
    img = ops.flow_colors(flow[None] if u.dim() == 2 else flow, scale=1.0, bgr=convert_to_bgr)
    return img[0] if u.dim() == 2 else img


def flow_uv_to_colors(u, v, convert_to_bgr=False):
    """flow_viz.py:70-106: the wheel applied to components that are already normalised; a radius above 1 is painted at
    three quarters of its colour.  u, v: device tensors [H,W] (or [B,H,W]) -> device uint8 [H,W,3]; NumPy in, NumPy out."""
    if isinstance(u, np.ndarray):
        img = _uv_to_colors(torch.from_numpy(np.ascontiguousarray(u, dtype=np.float32)).cuda(),
                            torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda(), convert_to_bgr)
        return img.cpu().numpy()
    return _uv_to_colors(u, v, convert_to_bgr)
