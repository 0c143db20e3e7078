"""Host-side checks of the flow visualisation entry points (csrc/flow_viz.hip): every one refuses bad arguments with
FS_ERR_ARG (1) before any HIP call -- so this runs without a GPU --, the Python functions carry the reference's signatures
and defaults, and they refuse CPU tensors."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

ERR = 1
P = ctypes.c_void_p(4096)          # a non-null, aligned pointer that is never dereferenced: the calls below all return first
NULL = ctypes.c_void_p(None)
ODD = ctypes.c_void_p(4097)
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    from flow_supervisor_amd import _lib
    return _lib.load()


def bad_sizes():
    # B, H, W below 1; H * W beyond 2^31 - 1; B beyond the grid's y dimension
    return [(0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, 65536, 32768), (65536, 4, 4)]


def test_rad_max_refuses_bad_arguments(lib):
    f = lib.fsraft_flow_rad_max
    assert f(NULL, 32, 16, 4, 1, 4, 4, 0.0, P, None) == ERR
    assert f(P, 32, 16, 4, 1, 4, 4, 0.0, NULL, None) == ERR
    assert f(P, 32, 16, 4, 1, 4, 4, 0.0, ODD, None) == ERR
    for B, H, W in bad_sizes():
        assert f(P, 32, 16, 4, B, H, W, 0.0, P, None) == ERR, (B, H, W)
    for clip in (-1.0, NAN, INF):
        assert f(P, 32, 16, 4, 1, 4, 4, clip, P, None) == ERR, clip


def test_wheel_refuses_bad_arguments(lib):
    f = lib.fsraft_flow_wheel
    assert f(NULL, 32, 16, 4, 1, 4, 4, 0.0, P, 0.0, 0, P, None) == ERR
    assert f(P, 32, 16, 4, 1, 4, 4, 0.0, P, 0.0, 0, NULL, None) == ERR
    assert f(P, 32, 16, 4, 1, 4, 4, 0.0, ODD, 0.0, 0, P, None) == ERR
    for B, H, W in bad_sizes():
        assert f(P, 32, 16, 4, B, H, W, 0.0, P, 0.0, 0, P, None) == ERR, (B, H, W)
    for clip in (-1.0, NAN, INF):
        assert f(P, 32, 16, 4, 1, 4, 4, clip, P, 0.0, 0, P, None) == ERR, clip
    for bgr in (-1, 2):
        assert f(P, 32, 16, 4, 1, 4, 4, 0.0, P, 0.0, bgr, P, None) == ERR, bgr
    for scale in (0.0, -1.0, NAN, INF):                  # without rad_max the scale is the normaliser
        assert f(P, 32, 16, 4, 1, 4, 4, 0.0, NULL, scale, 0, P, None) == ERR, scale


def test_hsv_refuses_bad_arguments(lib):
    f = lib.fsraft_flow_hsv
    assert f(NULL, 32, 16, 4, 1, 4, 4, P, 0.0, 0, P, None) == ERR
    assert f(P, 32, 16, 4, 1, 4, 4, P, 0.0, 0, NULL, None) == ERR
    assert f(P, 32, 16, 4, 1, 4, 4, NULL, 0.0, 0, P, None) == ERR          # no max_mag and no maximum
    assert f(P, 32, 16, 4, 1, 4, 4, ODD, 0.0, 0, P, None) == ERR
    assert f(P, 32, 16, 4, 1, 4, 4, P, 0.0, 0, ODD, None) == ERR           # a float output
    for B, H, W in bad_sizes():
        assert f(P, 32, 16, 4, B, H, W, P, 0.0, 0, P, None) == ERR, (B, H, W)
    for mm in (-1.0, NAN, INF):
        assert f(P, 32, 16, 4, 1, 4, 4, P, mm, 0, P, None) == ERR, mm
    for u8 in (-1, 2):
        assert f(P, 32, 16, 4, 1, 4, 4, P, 0.0, u8, P, None) == ERR, u8


def test_kitti16_refuses_bad_arguments(lib):
    f = lib.fsraft_flow_kitti16
    assert f(NULL, 32, 16, 4, NULL, 0, 0, 1, 4, 4, P, None) == ERR
    assert f(P, 32, 16, 4, NULL, 0, 0, 1, 4, 4, NULL, None) == ERR
    assert f(P, 32, 16, 4, NULL, 0, 0, 1, 4, 4, ODD, None) == ERR
    for B, H, W in bad_sizes():
        assert f(P, 32, 16, 4, NULL, 0, 0, B, H, W, P, None) == ERR, (B, H, W)


def _params(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def test_python_functions_have_the_reference_signatures():
    E = inspect.Parameter.empty
    from flow_supervisor_amd import evaluate, raft_tf
    from flow_supervisor_amd.core.utils import flow_viz
    from flow_supervisor_amd.raft_utils import frame_utils
    assert _params(flow_viz.make_colorwheel) == []
    assert _params(flow_viz.flow_uv_to_colors) == [("u", E), ("v", E), ("convert_to_bgr", False)]
    assert _params(flow_viz.flow_to_image)[:3] == [("flow_uv", E), ("clip_flow", None), ("convert_to_bgr", False)]
    assert _params(flow_viz.flow_to_image)[3:] == [("return_scale", False), ("scale", None)]          # the two extras
    assert _params(raft_tf.visualize_flow)[:2] == [("flow", E), ("max_mag", None)]
    assert _params(raft_tf.visualize_flows)[:2] == [("flows", E), ("max_mag", None)]
    assert all(d is not E for _, d in _params(raft_tf.visualize_flow)[2:] + _params(raft_tf.visualize_flows)[2:])
    assert _params(frame_utils.writePNG) == [("filename", E), ("array", E)]
    assert _params(frame_utils.readPNG) == [("filename", E)]
    assert _params(frame_utils.writeFlowKITTI16) == [("filename", E), ("rgb16", E)]
    assert _params(evaluate.validate_things)[:3] == [("model", E), ("datasets", E), ("iters", 6)]
    assert _params(evaluate.validate_sintel_occ)[:3] == [("model", E), ("datasets", E), ("iters", 6)]
    assert dict(_params(evaluate.create_sintel_submission_vis))["vis_path"] == "vis_test"
    assert dict(_params(evaluate.create_kitti_submission_vis))["vis_path"] == "vis_kitti"
    assert _params(evaluate.demo)[:5] == [("model", E), ("frames", E), ("output_path", E), ("iters", 12), ("style", "wheel")]


def test_python_functions_refuse_cpu_tensors():
    from flow_supervisor_amd import ops, raft_tf
    from flow_supervisor_amd.core.utils import flow_viz
    flow = torch.zeros(1, 2, 4, 4)
    calls = [lambda: ops.flow_rad_max(flow), lambda: ops.flow_colors(flow, scale=1.0), lambda: ops.flow_hsv(flow, max_mag=1.0),
             lambda: ops.flow_kitti16(flow), lambda: flow_viz.flow_to_image(flow), lambda: flow_viz.flow_to_image(flow[0]),
             lambda: flow_viz.flow_uv_to_colors(flow[0, 0], flow[0, 1]), lambda: raft_tf.visualize_flow(torch.zeros(4, 4, 2)),
             lambda: raft_tf.visualize_flows(torch.zeros(1, 4, 4, 2), max_mag=2.0)]
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            call()
    wheel = flow_viz.make_colorwheel()                   # host data, no device needed
    assert wheel.shape == (55, 3) and wheel.dtype == np.float64
