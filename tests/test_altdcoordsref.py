"""tests/_altdcoordsref.py -- the float64 restatement of the coordinate gradient of the memory-efficient lookup that the GPU tests
of csrc/altcorr_dcoords.hip compare against -- checked on the CPU: against _dcoordsref.expect and torch.autograd through the
oracle's explicit four-tap gather on a volume formed here, channel by channel, in float64; the weight-first form the kernel
computes against the restatement; the restatement on float64-pooled maps against the reference's own CorrBlock backward
(tests/golden/lookup_dcoords.npz, with the kink slack and the 5e-6 S limit of tests/test_dcoordsref.py, on that file's volume
scale: the alt formulation tied to the reference without a new fixture); LIMITS against the fp32 twins over the GPU tests'
cases; and the C entry's argument checks, which are host code.
"""
import ctypes
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _altdcoordsref as A
import _dcoordsref as R
from _util import G, _log_margin
from oracle import raft_torch as O

CASES = [((1, 10, 14), 4, 32), ((3, 5, 9), 2, 36), ((1, 8, 8), 3, 4)]


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def _explicit_volume(f1, f2_levels):
    """V_l [B*H*W, h_l, w_l] in float64, the products of one channel at a time added up (no matrix product)."""
    B, H, W, C = f1.shape
    out = []
    for f2 in f2_levels:
        v = torch.zeros(B, H * W, f2.shape[1] * f2.shape[2], dtype=torch.float64)
        for c in range(C):
            v += f1[..., c].double().reshape(B, -1, 1) * f2[..., c].double().reshape(B, 1, -1)
        out.append((v / math.sqrt(C)).reshape(B * H * W, f2.shape[1], f2.shape[2]))
    return out


@pytest.mark.parametrize("shape,nlev,C", CASES, ids=_ids)
@pytest.mark.parametrize("radius", R.RADII)
def test_restatement_matches_dcoordsref_and_autograd_on_the_formed_volume(shape, nlev, C, radius):
    B, H, W = shape
    c = A.case(shape, nlev, C, radius, "mixed")
    vol = _explicit_volume(c["f1"], c["f2"])
    x = c["pos"].double().requires_grad_()
    out = O.corr_lookup([v.unsqueeze(1) for v in vol], x, radius)                                # [B, CH, H, W]
    for dkind in ("gauss", "hot0f", f"hot{nlev - 1}l"):
        dout, dc, S = A.case_expect(shape, nlev, C, radius, "mixed", False, dkind)
        dc2, S2 = A.expect(c["f1"], c["f2"], c["pos"], dout, radius)
        assert torch.equal(dc, dc2) and torch.equal(S, S2)                                       # (case_expect is expect, cached)
        _, ref, Sv = R.expect(vol, c["pos"], dout, radius)
        w, i = R.need(dc, ref, S.expand_as(ref))
        assert w <= 1e-12, (dkind, w, i)
        assert bool((S >= Sv * (1 - 1e-12)).all())                                               # sum |a| |b| bounds |sum a b|
        x.grad = None
        out.backward(dout.double().permute(0, 3, 1, 2), retain_graph=True)
        w2, i2 = R.need(x.grad, dc, S.expand_as(dc))
        print(f"{shape} C{C} r{radius} {dkind}: vs _dcoordsref.expect {w:.2e} S, vs autograd {w2:.2e} S")
        assert w2 <= 1e-12, (dkind, w2, i2)
        assert bool((dc[:, :, 0] == 0).all()) and bool((S[:, :, 0] == 0).all())                  # the +-1e6 row


@pytest.mark.parametrize("shape,nlev,C", CASES, ids=_ids)
@pytest.mark.parametrize("radius", R.RADII)
@pytest.mark.parametrize("add_grid", (False, True))
def test_weight_first_form_matches_the_restatement(shape, nlev, C, radius, add_grid):
    """Integer positions, edges and the +-1e6 row included (the mixed positions), and a plane of zeros."""
    for ckind in R.COORD_KINDS:
        c = A.case(shape, nlev, C, radius, ckind, add_grid)
        trip = [A.case_expect(shape, nlev, C, radius, ckind, add_grid, dkind) for dkind in R.dout_kinds(nlev)]
        got = A.weight_first(c["f1"], c["f2"], c["pos"], torch.stack([t[0] for t in trip]), radius)
        for (_, dc, S), g in zip(trip, got):
            w, i = R.need(g, dc, S.expand_as(dc))
            assert w <= 1e-12, (ckind, w, i)
            if ckind == "mixed":
                assert bool((g[:, :, 0] == 0).all())


@pytest.mark.parametrize("radius", R.RADII)
def test_restatement_on_pooled_maps_matches_the_reference_backward(radius):
    g = dict(np.load(os.path.join(G, "lookup_dcoords.npz")))
    fmap1, fmap2 = torch.from_numpy(g["fmap1"]).double(), torch.from_numpy(g["fmap2"]).double()
    coords = torch.from_numpy(g["coords"])
    B, _, H, W = coords.shape
    f1 = fmap1.permute(0, 2, 3, 1).contiguous()
    f2, lv = [], fmap2
    for l in range(4):
        if l:
            lv = F.avg_pool2d(lv, 2, stride=2)
        f2.append(lv.permute(0, 2, 3, 1).contiguous())
    dout = (torch.from_numpy(g[f"dout_q_r{radius}"]).float() * float(g["dout_scale"])).permute(0, 2, 3, 1).contiguous()
    got = torch.from_numpy(g[f"coords_grad_r{radius}"]).double()
    vol = A.volumes(f1, f2)
    _, _, S = R.expect(vol, coords, dout, radius)                                                # that file's volume scale
    dc, _ = A.expect(f1, f2, coords, dout, radius)
    wf = A.weight_first(f1, f2, coords, dout.unsqueeze(0), radius)[0]
    _, dxf, dyf, _ = R.jacobian(vol, coords, radius)
    _, dxl, dyl, _ = R.jacobian(vol, coords, radius, left=True)
    ga = dout.reshape(B * H * W, -1).double().abs()
    slack = torch.stack([(ga * (dxf - dxl).abs()).sum(1), (ga * (dyf - dyl).abs()).sum(1)], 1).view(B, H, W, 2).permute(0, 3, 1, 2)
    on_kink = coords == coords.round()
    assert bool((slack[~on_kink] == 0).all()) and int(on_kink.sum()) >= coords.numel() // 4     # slack at integer positions only
    for name, mine in (("restatement", dc), ("weight-first", wf)):
        ex = ((got - mine).abs() - slack).clamp_min(0)
        w, i = R.need(mine + ex, mine, S.expand_as(mine))
        _log_margin(f"alt {name} vs reference coords.grad r{radius}", w, 5e-6, "beyond the kink slack, in S")
        print(f"radius {radius}: {name} worst beyond the kink slack {w:.3e} S")
        assert w <= 5e-6, (name, w, i)
        w2, _ = R.need(torch.where(on_kink, mine, got), mine, S.expand_as(mine))                 # away from integer positions: outright
        assert w2 <= 5e-6, (name, w2)


def test_limits_come_from_the_twins():
    """LIMITS = 4 x the worst either fp32 twin reaches over every case of the kernel tests, rounded up to one digit."""
    worst = A.worst_of_twins()
    print(f"twins' worst {worst:.4f} units of 2^-24 S")
    assert 0.9 * A.TWIN_WORST["dcoords"] <= worst <= A.TWIN_WORST["dcoords"]
    assert A.LIMITS["dcoords"] == R.limit_from_twin(A.TWIN_WORST["dcoords"])


def test_cases_cover_the_shapes_and_the_channel_sweep():
    keys = list(A.case_keys())
    assert {(k[0], k[1]) for k in keys if k[2] == A.C_BASE} == set(R.SHAPES)
    assert {k[2] for k in keys if (k[0], k[1]) in A.SWEEP_SHAPES} == set(A.SWEEP_C) | {A.C_BASE}
    assert {k[2] for k in keys if (k[0], k[1]) not in A.SWEEP_SHAPES} == {A.C_BASE}
    assert {k[3:] for k in keys} == {(r, ck, ag) for r in R.RADII for ck in R.COORD_KINDS for ag in (False, True)}
    assert len(list(A.kernel_cases())) == sum(len(R.dout_kinds(k[1])) for k in keys)


def test_entry_point_is_exported_with_its_signature():
    from flow_supervisor_amd import _lib
    assert "fsraft_altcorr_fused_dcoords" in _lib.SIGNATURES and len(_lib.SIGNATURES["fsraft_altcorr_fused_dcoords"]) == 19
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "fsraft_altcorr_fused_dcoords")
    txt = open(os.path.join(os.path.dirname(G), "..", "include", "fsraft.h")).read()
    assert "int fsraft_altcorr_fused_dcoords(" in txt


def test_entry_point_refuses_bad_arguments_before_touching_the_gpu():
    """Argument validation is host code: FS_ERR_ARG (1) without a HIP call, so this runs without a GPU (the pointers are never
    dereferenced)."""
    from flow_supervisor_amd import _lib
    lib = _lib.load()
    p, null = ctypes.c_void_p(4096), ctypes.c_void_p(None)
    keep = (ctypes.c_void_p * 4)(4096, 4096, 4096, 4096)
    pp = ctypes.cast(keep, _lib._PP)
    s = (128, 64, 1)

    def call(f1=p, levels=pp, nlev=4, coords=p, dout=p, dc=p, shape=(1, 8, 8), C=32, radius=4):
        return lib.fsraft_altcorr_fused_dcoords(f1, levels, nlev, coords, *s, 0, dout, dc, *s, *shape, C, radius, None)

    for kw in (dict(radius=2), dict(radius=5), dict(nlev=0), dict(nlev=5), dict(dc=null), dict(C=0), dict(C=260),
               dict(shape=(1, 4, 4)),                               # 4x4 has no fourth level
               dict(shape=(1 << 27, 4, 4), nlev=1),                 # 2^31 queries
               dict(f1=null), dict(coords=null), dict(dout=null), dict(levels=ctypes.cast(null, _lib._PP)),
               dict(shape=(0, 8, 8)), dict(shape=(1, 0, 8))):
        assert call(**kw) == 1, kw
    keep[2] = None
    assert call() == 1                                              # a null level
    assert call(nlev=2, dc=null) == 1
