"""tests/_imageref.py -- the float64 restatement of the TF tree's image plumbing the GPU tests compare csrc/image_ops.hip with --
held to independent formulations, on the CPU:
  resize        F.interpolate(mode='bilinear', align_corners=False, antialias=False) in float64, value and autograd gradient.  The
                restatement forms its source coordinate in float32 (as TensorFlow does), F.interpolate in float64: the coordinate
                differs by at most 3 roundings of a number below n_in, d = 3 * 2^-24 * n_in, which moves a value by at most d times
                the largest difference of neighbouring sources per axis, and a gradient by at most d * |g| per tap and axis
  resize_flow   the literal op sequence of raft/__init__.py:213-222
  crop / pad    slicing and F.pad;  pad_edge: F.pad(mode='replicate') and np.pad(..., 'edge')
  pad_inputs    the arithmetic for heights and widths 1..17 in both modes, and the module's own input_padding
  limits        the twin-derived LIMITS are reproduced
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _imageref as R


def _ids(c):
    return "x".join(map(str, c))


@pytest.mark.parametrize("case", R.RESIZE_CASES, ids=_ids)
def test_resize_against_interpolate(case):
    hi, wi, ho, wo = case
    x, g = R.resize_inputs(case, 3)
    xd = x.double().requires_grad_(True)
    y = F.interpolate(xd.permute(0, 3, 1, 2), size=(ho, wo), mode="bilinear", align_corners=False, antialias=False).permute(0, 2, 3, 1)
    y.backward(g.double())
    d = 3.0 * R.U24 * max(hi, wi)
    spread = float(x.max() - x.min())
    assert float((R.resize_ref(x, (ho, wo)) - y.detach()).abs().max()) <= 2 * d * spread + 1e-12
    taps_per_source = (2 * -(-ho // hi) + 2) * (2 * -(-wo // wi) + 2)
    got = R.resize_bwd_ref(g, (hi, wi))
    assert float((got - xd.grad).abs().max()) <= 2 * d * float(g.abs().max()) * taps_per_source + 1e-12
    # the matrix form is the lerp form
    assert float((R.resize_matrix(x, (ho, wo)) - R.resize_ref(x, (ho, wo))).abs().max()) <= 1e-13 * float(x.abs().max())
    # sources no tap reaches: gradient exactly +0.0, and autograd agrees
    dead = ~(R.reached(hi, ho)[:, None] & R.reached(wi, wo)[None, :])
    assert bool((got[:, dead] == 0).all()) and bool((xd.grad[:, dead] == 0).all())
    assert not torch.signbit(got[:, dead]).any()


def test_skipping_case_skips_and_equal_sizes_are_the_identity():
    assert not R.reached(17, 4).all() and not R.reached(9, 3).all()
    assert R.reached(5, 8).all() and R.reached(255, 256).all()
    x, _ = R.resize_inputs((5, 7, 5, 7), 2)
    assert torch.equal(R.resize_ref(x, (5, 7)), x.double())
    assert torch.equal(R.resize_ref(x, (5, 7), dtype=torch.float32), x)


@pytest.mark.parametrize("case", R.RESIZE_CASES, ids=_ids)
def test_resize_flow_against_the_literal_op_sequence(case):
    hi, wi, ho, wo = case
    x, _ = R.resize_inputs(case, 2)
    lit = R.resize_flow_literal(x.double(), (ho, wo))
    got = R.resize_ref(x, (ho, wo), R.flow_factors(*case))
    assert torch.equal(got, lit)
    assert R.flow_factors(5, 7, 8, 8) == [float(np.float32(8) / np.float32(7)), float(np.float32(8) / np.float32(5))]
    assert torch.equal(R.resize_flow_literal(x.double(), (ho, wo), scaling=False), R.resize_ref(x, (ho, wo)))


def test_crop_and_pad_against_slicing_and_f_pad():
    x = R.box_values(3, 9, 11, 2)
    yx, size = [(0, 0), (4, 5), (2, 3)], (5, 6)
    got = R.crop_ref(x, yx, size)
    for b, (y0, x0) in enumerate(yx):
        assert torch.equal(got[b], x[b, y0:y0 + 5, x0:x0 + 6])
    back = R.pad_ref(got, yx, (9, 11))
    for b, (y0, x0) in enumerate(yx):
        want = F.pad(got[b].permute(2, 0, 1), (x0, 11 - x0 - 6, y0, 9 - y0 - 5)).permute(1, 2, 0)
        assert torch.equal(back[b], want)
        assert not torch.signbit(back[b]).any()
    assert torch.equal(R.crop_ref(back, yx, size), got)


@pytest.mark.parametrize("pads", ((0, 0, 0, 0), (7, 0, 0, 0), (0, 7, 0, 0), (0, 0, 7, 0), (0, 0, 0, 7), (2, 3, 1, 4)), ids=_ids)
@pytest.mark.parametrize("hw", ((1, 1), (5, 9)), ids=_ids)
def test_pad_edge_against_replicate_and_numpy(hw, pads):
    x = R.box_values(2, hw[0], hw[1], 3)
    got = R.pad_edge_ref(x, pads)
    t, b, l, r = pads
    assert torch.equal(got, F.pad(x.permute(0, 3, 1, 2), (l, r, t, b), mode="replicate").permute(0, 2, 3, 1))
    assert np.array_equal(got.numpy(), np.pad(x.numpy(), ((0, 0), (t, b), (l, r), (0, 0)), "edge"))


@pytest.mark.parametrize("mode", (None, "sintel", "kitti"))
def test_pad_inputs_arithmetic(mode):
    from flow_supervisor_amd.raft_tf import image
    for ht in range(1, 18):
        for wd in range(1, 18):
            pad = R.input_padding_ref(ht, wd, mode)
            assert pad == image.input_padding(ht, wd, mode)
            assert pad[0] == [0, 0] and pad[3] == [0, 0]
            (t, b), (l, r) = pad[1], pad[2]
            H, W = ht + t + b, wd + l + r
            assert H % 8 == 0 and W % 8 == 0 and ht <= H < ht + 8 and wd <= W < wd + 8
            assert l == (W - wd) // 2 and r == (W - wd) - l
            if mode == "sintel":
                assert t == (H - ht) // 2 and b == (H - ht) - t
            else:
                assert t == 0
            assert (H, W) == image.get_proc_size((ht, wd))


def test_twin_within_limits_and_limits_are_four_times_the_twins_worst():
    worst = dict.fromkeys(R.LIMITS, 0.0)
    for x, g, size, fac in R.all_runs():
        for k, v in R.twin_needs(x, g, size, fac).items():
            worst[k] = max(worst[k], v)
    assert set(worst) == set(R.LIMITS) == set(R.TWIN_WORST)
    for k, v in worst.items():
        assert v <= R.LIMITS[k], (k, v)
        assert R.LIMITS[k] == R.limit_from_twin(v), (k, v, R.LIMITS[k])
        assert abs(v - R.TWIN_WORST[k]) <= 0.06 * max(v, 0.1), (k, v)


def test_a_dropped_half_pixel_and_a_swapped_factor_exceed_four_times_the_limit():
    """What the limits are for: align-corners-style coordinates (no half-pixel shift) and the flow factors on the wrong channels
    each leave the restatement by more than 4 x the limit."""
    case = (5, 7, 8, 8)
    x, g = R.resize_inputs(case, 2)
    fac = R.flow_factors(*case)
    ev, _ = R.resize_expect(x, g, case[2:], fac)
    swapped = R.resize_ref(x, case[2:], fac[::-1])
    assert R.need(swapped, *ev[:3])[0] > 4 * R.LIMITS["rs_val"]
    xd = x.double().permute(0, 3, 1, 2)
    corners = F.interpolate(xd, size=case[2:], mode="bilinear", align_corners=True).permute(0, 2, 3, 1) * torch.tensor(fac, dtype=torch.float64)
    assert R.need(corners, *ev[:3])[0] > 4 * R.LIMITS["rs_val"]
