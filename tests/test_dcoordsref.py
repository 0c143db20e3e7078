"""tests/_dcoordsref.py -- the float64 restatement of the lookup's coordinate gradient that the GPU tests of csrc/corr_dcoords.hip
compare against -- checked on the CPU: against the reference's own CorrBlock backward (tests/golden/lookup_dcoords.npz), against
torch.autograd through the oracle's explicit four-tap gather in float64 (the convention at integer positions is the point),
and against central differences of the float64 lookup; and LIMITS against the fp32 twins over the GPU tests' cases.

The golden comparison.  The reference reaches grid_sample through 2 x / (w - 1) - 1, and grid_sample un-normalises again: an
integer position comes back as itself or one ulp to either side, so at an integer x (y) the reference takes the slope of the
right OR the left cell (115 of 768 gradient elements of the radius-3 fixture differ from the floor convention by up to 0.34 S).
That is rounding noise of the reference, not a convention: the comparison gives every query the slack between the two
conventions, sum |dout| |D_floor - D_left| (zero wherever no sample sits on an integer).  Beyond the slack: the round trip moves
a position by about 3 ulp of w - 1 (< 5e-6 cells at w = 24), which changes a slope by that times a cross difference <= A, and
the fp32 sums of 196 / 324 terms add ~1e-6 S: limit 5e-6 S.  Measured: 6.5e-7 S (radius 3), 1.8e-7 S (radius 4).
"""
import os

import numpy as np
import pytest
import torch

import _dcoordsref as R
from _util import G, _log_margin
from oracle import raft_torch as O


@pytest.fixture(scope="module")
def golden():
    g = dict(np.load(os.path.join(G, "lookup_dcoords.npz")))
    f1, f2 = torch.from_numpy(g["fmap1"]).double(), torch.from_numpy(g["fmap2"]).double()
    g["pyr"] = [lv[:, 0] for lv in O.corr_pyramid(f1, f2, 4)]
    return g


@pytest.mark.parametrize("radius", R.RADII)
def test_restatement_matches_the_reference_backward(golden, radius):
    coords = torch.from_numpy(golden["coords"])
    B, _, H, W = coords.shape
    dout = (torch.from_numpy(golden[f"dout_q_r{radius}"]).float() * float(golden["dout_scale"])).permute(0, 2, 3, 1).contiguous()
    got = torch.from_numpy(golden[f"coords_grad_r{radius}"]).double()
    _, dc, S = R.expect(golden["pyr"], coords, dout, radius)
    _, dxf, dyf, _ = R.jacobian(golden["pyr"], coords, radius)
    _, dxl, dyl, _ = R.jacobian(golden["pyr"], coords, radius, left=True)
    g = dout.reshape(B * H * W, -1).double().abs()
    slack = torch.stack([(g * (dxf - dxl).abs()).sum(1), (g * (dyf - dyl).abs()).sum(1)], 1).view(B, H, W, 2).permute(0, 3, 1, 2)
    on_kink = coords == coords.round()
    assert bool((slack[~on_kink] == 0).all()) and int(on_kink.sum()) >= coords.numel() // 4     # slack at integer positions only
    ex = ((got - dc).abs() - slack).clamp_min(0)
    w, i = R.need(dc + ex, dc, S.expand_as(dc))
    _log_margin(f"restatement vs reference coords.grad r{radius}", w, 5e-6, "beyond the kink slack, in S")
    print(f"radius {radius}: worst beyond the kink slack {w:.3e} S; elements off the floor convention "
          f"{int(((got - dc).abs() > 5e-6 * S).sum())} of {dc.numel()}")
    assert w <= 5e-6, (w, i)
    # away from integer positions the reference and the restatement agree outright
    w2, _ = R.need(torch.where(on_kink, dc, got), dc, S.expand_as(dc))
    assert w2 <= 5e-6, w2


@pytest.mark.parametrize("shape,nlev", R.SHAPES[:2] + R.SHAPES[5:6], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
@pytest.mark.parametrize("radius", R.RADII)
def test_restatement_matches_autograd_of_the_explicit_gather(shape, nlev, radius):
    """torch.autograd through oracle.raft_torch.corr_lookup in float64, integer positions and edges included: 1e-12 S."""
    B, H, W = shape
    c = R.case(shape, nlev, radius, "mixed")
    dout = R.dout_values(B, H, W, nlev, radius, "gauss")
    val, dc, S = R.expect(c["levels"], c["pos"], dout, radius)
    x = c["pos"].double().requires_grad_()
    out = O.corr_lookup([lv.double().unsqueeze(1) for lv in c["levels"]], x, radius)            # [B, CH, H, W]
    wv, _ = R.need(out.detach().permute(0, 2, 3, 1), val, val.abs().max())
    out.backward(dout.double().permute(0, 3, 1, 2))
    w, i = R.need(x.grad, dc, S.expand_as(dc))
    print(f"{shape} r{radius}: out {wv:.2e} of max|out|, dcoords {w:.2e} S")
    assert wv <= 1e-12 and w <= 1e-12, (wv, w, i)
    assert bool((dc[:, :, 0] == 0).all()) and bool((S[:, :, 0] == 0).all())                     # the +-1e6 row


@pytest.mark.parametrize("radius", R.RADII)
def test_restatement_matches_central_differences(radius):
    """At non-integer positions (multiples of 1/64 off every integer, at every level) the lookup is bilinear within 2^-20 of the
    position: central differences of the float64 lookup are exact up to its rounding, ~1e-16 / 2^-20 relative."""
    shape, nlev = R.SHAPES[1]
    B, H, W = shape
    c = R.case(shape, nlev, radius, "mixed")
    pos = c["pos"].double()
    dout = R.dout_values(B, H, W, nlev, radius, "gauss")
    _, dc, S = R.expect(c["levels"], pos, dout, radius)
    inside = ((pos != pos.round()).all(1, keepdim=True) & (pos.abs() < 1e5).all(1, keepdim=True)).expand_as(dc)
    assert int(inside.sum()) >= dc.numel() // 3
    eps = 2.0 ** -20
    lv64 = [lv.double() for lv in c["levels"]]
    for k in (0, 1):
        d = torch.zeros_like(pos)
        d[:, k] = eps
        vp = R.jacobian(lv64, pos + d, radius)[0]
        vm = R.jacobian(lv64, pos - d, radius)[0]
        fd = (((vp - vm) / (2 * eps)) * dout.reshape(B * H * W, -1).double()).sum(1).view(B, H, W)
        w, i = R.need(torch.where(inside[:, k], fd, dc[:, k]), dc[:, k], S[:, 0])
        print(f"r{radius} d/d{'xy'[k]}: central differences {w:.2e} S")
        assert w <= 1e-8, (k, w, i)


def test_limits_come_from_the_twins():
    """LIMITS = 4 x the worst either fp32 twin reaches over every case of the kernel tests, rounded up to one digit."""
    worst = 0.0
    for shape, nlev, radius, ckind, add_grid, dkind in R.kernel_cases():
        c = R.case(shape, nlev, radius, ckind, add_grid)
        dout, dc, S = R.case_expect(shape, nlev, radius, ckind, add_grid, dkind)
        for order in ("sequential", "pairwise"):
            w, _ = R.need(R.twin(c["levels"], c["pos"], dout, radius, order), dc, (S * R.U24).expand_as(dc))
            worst = max(worst, w)
    print(f"twins' worst {worst:.4f} units of 2^-24 S")
    assert 0.9 * R.TWIN_WORST["dcoords"] <= worst <= R.TWIN_WORST["dcoords"]
    assert R.LIMITS["dcoords"] == R.limit_from_twin(R.TWIN_WORST["dcoords"])


def test_entry_points_refuse_bad_arguments_before_touching_the_gpu():
    """Argument validation is host code: FS_ERR_ARG (1) without a HIP call, so this runs without a GPU (the pointers are never
    dereferenced)."""
    import ctypes
    from flow_supervisor_amd import _lib
    lib = _lib.load()
    p, null = ctypes.c_void_p(4096), ctypes.c_void_p(None)
    keep = (ctypes.c_void_p * 4)(4096, 4096, 4096, 4096)
    pp = ctypes.cast(keep, _lib._PP)
    s = (128, 64, 1)
    for radius, nlev, dc, shape in ((2, 4, p, (1, 8, 8)), (5, 4, p, (1, 8, 8)), (4, 0, p, (1, 8, 8)), (4, 5, p, (1, 8, 8)), (4, 4, null, (1, 8, 8)),
                                    (4, 1, p, (1 << 27, 4, 4)), (4, 4, p, (1, 4, 4))):          # (4x4 has no fourth level)
        assert lib.fsraft_corr_lookup_tiled_dcoords(p, nlev, p, *s, p, dc, *s, *shape, radius, 0, None) == 1, (radius, nlev, shape)
        assert lib.fsraft_corr_lookup_dcoords(pp, nlev, p, *s, p, 1, dc, *s, *shape, radius, None) == 1, (radius, nlev, shape)
    assert lib.fsraft_corr_lookup_tiled_dcoords(null, 4, p, *s, p, p, *s, 1, 8, 8, 4, 0, None) == 1
    assert lib.fsraft_corr_lookup_tiled_dcoords(p, 4, null, *s, p, p, *s, 1, 8, 8, 4, 0, None) == 1
    assert lib.fsraft_corr_lookup_tiled_dcoords(p, 4, p, *s, null, p, *s, 1, 8, 8, 4, 0, None) == 1
    assert lib.fsraft_corr_lookup_tiled_dcoords(ctypes.c_void_p(4100), 4, p, *s, p, p, *s, 1, 8, 8, 4, 0, None) == 1      # volume off 16 bytes
    assert lib.fsraft_corr_lookup_dcoords(ctypes.cast(null, _lib._PP), 4, p, *s, p, 1, p, *s, 1, 8, 8, 4, None) == 1
    keep[2] = None
    assert lib.fsraft_corr_lookup_dcoords(pp, 4, p, *s, p, 1, p, *s, 1, 8, 8, 4, None) == 1                               # a null level
    assert lib.fsraft_corr_lookup_dcoords(pp, 2, p, *s, p, 1, null, *s, 1, 8, 8, 4, None) == 1


def test_one_hot_gradients_tell_i_from_j_and_the_level_scale():
    """What the one-hot dout cases rest on: the first / last channel of level l is the window corner (-r, -r) / (+r, +r) at 2^-l,
    and d/dx differs from d/dy there."""
    shape, nlev = R.SHAPES[1]
    radius = 4
    c = R.case(shape, nlev, radius, "mixed")
    _, dx, dy, _ = c["jac"]
    n2 = (2 * radius + 1) ** 2
    for l in range(nlev):
        for ch in (l * n2, l * n2 + n2 - 1):
            dout, dc, _ = R.case_expect(shape, nlev, radius, "mixed", False, f"hot{l}{'f' if ch == l * n2 else 'l'}")
            assert torch.equal(dc[:, 0].reshape(-1), dx[:, ch]) and torch.equal(dc[:, 1].reshape(-1), dy[:, ch])
    assert not torch.equal(dx[:, 1], dx[:, 2 * radius + 1])          # channel 1 is (i, j) = (0, 1), channel 2r+1 is (1, 0)
