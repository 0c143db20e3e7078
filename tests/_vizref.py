"""Restatement of the reference's flow visualisation and KITTI encoding, the oracle of the flow_viz tests.

Wheel (pytorch/core/utils/flow_viz.py:70-132) with the dtypes NumPy gives a float32 flow there: u, v, rad, the angle and fk
are float32; k0 is int32, so f = fk - k0 is float64, and so is everything from the table lookup on.  test_vizref.py pins it
to outputs of the reference's own functions (tests/golden/flow_viz.npz), exactly.

HSV (util/visualize.py:5-27 over tf.image.hsv_to_rgb) and the KITTI expression (pytorch/raft_utils/frame_utils.py:122-124)
are restatements only: there is no TensorFlow here and the reference's frame_utils cannot be imported without OpenCV."""
import numpy as np

# RY 15, YG 6, GC 4, CB 11, BM 13, MR 6: (length, channel at 255, channel on the ramp, ramp falls)
SEGMENTS = ((15, 0, 1, False), (6, 1, 0, True), (4, 1, 2, False), (11, 2, 1, True), (13, 2, 0, False), (6, 0, 2, True))


def colorwheel():
    """float64 [55,3]"""
    rows = []
    for n, full, ramp, falls in SEGMENTS:
        seg = np.zeros((n, 3))
        r = np.floor(255 * np.arange(n) / n)
        seg[:, full] = 255
        seg[:, ramp] = 255 - r if falls else r
        rows.append(seg)
    return np.concatenate(rows)


WHEEL = colorwheel()


def uv_to_colors(u, v, bgr=False):
    """u, v: float32 [H,W], already normalised -> uint8 [H,W,3] (flow_viz.py:70-106)."""
    u, v = np.asarray(u, np.float32), np.asarray(v, np.float32)
    rad = np.sqrt(u * u + v * v)                                         # float32
    a = np.arctan2(-v, -u) / np.float32(np.pi)                           # float32
    fk = (a + np.float32(1)) / np.float32(2) * np.float32(54)            # float32
    k0 = np.floor(fk).astype(np.int32)
    k1 = np.where(k0 + 1 == 55, 0, k0 + 1)
    f = fk.astype(np.float64) - k0                                       # float32 - int32 is float64 in NumPy
    inside = rad <= 1
    img = np.zeros(u.shape + (3,), np.uint8)
    for i in range(3):
        col = (1 - f) * (WHEEL[k0, i] / 255.0) + f * (WHEEL[k1, i] / 255.0)
        col = np.where(inside, 1 - rad.astype(np.float64) * (1 - col), col * 0.75)
        img[..., 2 - i if bgr else i] = np.floor(255 * col)
    return img


def rad_max(flow, clip=None):
    """flow float32 [H,W,2] -> the float32 maximum radius, after np.clip(flow, 0, clip) (the reference's lower bound 0)."""
    flow = np.asarray(flow, np.float32)
    if clip is not None:
        flow = np.clip(flow, np.float32(0), np.float32(clip))
    return np.max(np.sqrt(flow[..., 0] * flow[..., 0] + flow[..., 1] * flow[..., 1]))


def to_image(flow, clip=None, bgr=False, scale=None):
    """flow float32 [H,W,2] -> uint8 [H,W,3] (flow_viz.py:109-132).  scale: the normaliser in place of rad_max + 1e-5."""
    flow = np.asarray(flow, np.float32)
    if clip is not None:
        flow = np.clip(flow, np.float32(0), np.float32(clip))
    den = np.float32(scale) if scale is not None else np.float32(rad_max(flow)) + np.float32(1e-5)
    return uv_to_colors(flow[..., 0] / den, flow[..., 1] / den, bgr)


def hsv(flow, max_mag=None, dtype=np.float64):
    """flow [H,W,2] -> rgb [H,W,3] in `dtype` (util/visualize.py:5-27; tf.image.hsv_to_rgb restated from TF's kernel)."""
    flow = np.asarray(flow, np.float32).astype(dtype)
    x, y = flow[..., 0], flow[..., 1]
    two_pi = dtype(2 * np.pi)
    rho = np.sqrt(x * x + y * y)
    phi = np.arctan2(y, x)
    phi = np.where(phi < 0, phi + two_pi, phi)
    if max_mag:
        s = np.clip(rho / dtype(max_mag), 0, 1)
    else:
        m = rho.max()
        s = rho / (dtype(1) if m == 0 else m)
    h6 = phi / two_pi * dtype(6)
    d = np.stack([np.clip(np.abs(h6 - 3) - 1, 0, 1), np.clip(2 - np.abs(h6 - 2), 0, 1), np.clip(2 - np.abs(h6 - 4), 0, 1)], -1)
    return (((d - 1) * s[..., None] + 1) * dtype(1)).astype(dtype)


def hsv_u8(flow, max_mag=None):
    """np.uint8(vis * 255), extract_flow.py:154, on the float64 restatement."""
    return (hsv(flow, max_mag) * 255).astype(np.uint8)


def kitti16(flow, valid=None):
    """flow float32 [H,W,2] -> uint16 [H,W,3] = (64 u + 2^15, 64 v + 2^15, valid) computed in float32, truncated and clamped
    to [0, 65535] (frame_utils.py:122-124, which wraps or is undefined from |flow| >= 512 on)."""
    flow = np.asarray(flow, np.float32)
    t = np.float32(64.0) * flow + np.float32(2 ** 15)
    assert t.dtype == np.float32
    uv = np.clip(np.trunc(t), 0, 65535).astype(np.uint16)
    third = np.ones(flow.shape[:2], np.uint16) if valid is None else (np.asarray(valid, np.float32) >= 0.5).astype(np.uint16)
    return np.concatenate([uv, third[..., None]], -1)


def two_part(got, want):
    """The two-part rule of the uint8 pictures: (largest level difference, number of differing values, the cap on that number
    max(1, ceil(1e-3 * n)))."""
    diff = np.abs(np.asarray(got).astype(np.int32) - np.asarray(want).astype(np.int32))
    return int(diff.max()), int(np.count_nonzero(diff)), max(1, int(np.ceil(1e-3 * diff.size)))
