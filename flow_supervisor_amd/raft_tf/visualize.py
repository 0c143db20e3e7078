"""NHWC twins of the TensorFlow tree's flow visualisation (util/visualize.py:5-27, 40-42), on the device
(csrc/flow_viz.hip: fsraft_flow_rad_max, fsraft_flow_hsv).

    visualize_flow(flow, max_mag=None)        flow [H,W,2] -> rgb [H,W,3] fp32 in [0, 1]
    visualize_flows(flows, max_mag=None)      flows [B,H,W,2] -> [B,H,W,3], every sample on its own maximum (tf.map_fn)

Hue is the direction, saturation the magnitude over `max_mag` (clipped to 1) or over the sample's own maximum, value 1, and
RGB as tf.image.hsv_to_rgb computes it.  `if max_mag:` has the reference's truthiness: 0 and None both mean "use the
maximum".  TensorFlow is not installed here: the formula is restated from its source in include/fsraft.h and parity with
TensorFlow is unpinned.  as_uint8=True (an extra) gives what extract_flow.py:154 makes of the result, np.uint8(vis * 255)."""
from .. import ops
from .._lib import on_tensor_device


@on_tensor_device
def visualize_flows(flows, max_mag=None, as_uint8=False):
    if flows.dim() != 4 or flows.shape[-1] != 2:
        raise ValueError(f"visualize_flows: flows is [B,H,W,2], got {tuple(flows.shape)}")
    planar = flows.detach().permute(0, 3, 1, 2).contiguous()
    if max_mag:
        return ops.flow_hsv(planar, max_mag=float(max_mag), as_uint8=as_uint8)
    return ops.flow_hsv(planar, rad_max=ops.flow_rad_max(planar), as_uint8=as_uint8)


def visualize_flow(flow, max_mag=None, as_uint8=False):
    if flow.dim() != 3 or flow.shape[-1] != 2:
        raise ValueError(f"visualize_flow: flow is [H,W,2], got {tuple(flow.shape)}")
    return visualize_flows(flow[None], max_mag, as_uint8)[0]
