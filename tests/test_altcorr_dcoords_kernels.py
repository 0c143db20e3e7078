"""altcorr_fused_dcoords_kernel of csrc/altcorr_dcoords.hip through ops.altcorr_fused_dcoords and the C entry
fsraft_altcorr_fused_dcoords, every element against the float64 restatement of tests/_altdcoordsref.py.  Cases
(_altdcoordsref.kernel_cases): the shapes of _dcoordsref.SHAPES at C = 32 -- 1x10x14 with four levels (10x14, 5x7, 2x3, 1x1), 2x16x24,
1x8x8 with one, two and three levels, 3x5x9 with two (135 queries: no multiple of a wave's four or sixteen), 2x8x16 -- and the
channel sweep C = 4, 36, 100, 128, 256 (one to four rounds of 64 lanes, ragged tails) on 1x10x14 and 3x5x9; radius 3 and 4;
positions across and beyond the plane, exact integers, edges, a row of +-1e6 and a plane of zeros; add_grid 0 / 1; dout gaussian,
zero, one-hot on the first / last channel of every level.  The far row and the zero dout give exactly 0.  Through the C entry:
every element of a NaN-filled dcoords is written and nothing beside it, in three layouts; maps handed in from inside NaN-filled
allocations give the same bits (nothing outside a level is read); a [B,H,W,2] view of the coordinates, the flow with add_grid
against grid + flow without, and two launches give the same bits.  Needs an MI355X: -m gpu.

Limit: _altdcoordsref.LIMITS (20 units of 2^-24 S, from the fp32 twins on the CPU: tests/test_altdcoordsref.py), not from the
kernel.  profiles/altcorr_dcoords_margins.txt lists every comparison (FSRAFT_PARITY_LOG).  Worst values measured on MI355X, in those
units:
  C = 32, all shapes      1.34  limit 20   (1x10x14, 4 levels, radius 3, a plane of zeros)
  channel sweep           1.62  limit 20   (1x10x14, C = 4, radius 3); 0.35 at C = 256
  far row, zero dout, written / unwritten elements, inputs unchanged, poisoned surroundings, views, add_grid, two launches: exact
"""
import pytest
import torch

import _altdcoordsref as A
import _dcoordsref as R
from _util import Buf, PATTERN, _log_margin

pytestmark = pytest.mark.gpu
DEV = "cuda"
GROUPS = [(shape, nlev, C) for shapes, cs in ((R.SHAPES, (A.C_BASE,)), (A.SWEEP_SHAPES, A.SWEEP_C)) for shape, nlev in shapes for C in cs]


@pytest.fixture(scope="module", autouse=True)
def _leave_no_cached_segments():
    """(as tests/test_gma_kernels.py: hand the free segments back, later modules count allocated bytes)"""
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("radius", R.RADII)
@pytest.mark.parametrize("shape,nlev,C", GROUPS, ids=_ids)
def test_dcoords_against_float64(shape, nlev, C, radius):
    from flow_supervisor_amd import ops
    worst, zeros_ok, failed = (-1.0, ""), True, []
    for ckind in R.COORD_KINDS:
        for add_grid in (False, True):
            c = A.case(shape, nlev, C, radius, ckind, add_grid)
            f1, f2, given = c["f1"].to(DEV), [f.to(DEV) for f in c["f2"]], c["given"].to(DEV)
            for dkind in R.dout_kinds(nlev):
                variant = f"{ckind} grid{int(add_grid)} {dkind}"
                dout, ref, S = A.case_expect(shape, nlev, C, radius, ckind, add_grid, dkind)
                got = ops.altcorr_fused_dcoords(f1, f2, given, dout.to(DEV), radius, is_flow=add_grid).cpu()
                w, i = R.need(got, ref, (S * A.U24).expand_as(ref))
                if w > worst[0]:
                    worst = (w, variant)
                if not w <= A.LIMITS["dcoords"]:
                    failed.append((variant, w, i))
                if (ckind == "mixed" and not bool((got[:, :, 0] == 0).all())) or (dkind == "zero" and not bool((got == 0).all())):
                    zeros_ok = False
                    failed.append((variant, "the far row / the zero dout must give exactly 0"))
    case = f"{_ids(shape)} L{nlev} C{C} r{radius}"
    _log_margin(f"alt dcoords {case}", worst[0], A.LIMITS["dcoords"], f"worst |got - ref| / (2^-24 S), {worst[1]}")
    _log_margin(f"alt far row and zero dout exactly 0 {case}", 0.0 if zeros_ok else 1.0, 0.0, "exact")
    print(f"{case}: worst {worst[0]:.3f} units of 2^-24 S (limit {A.LIMITS['dcoords']}), {worst[1]}")
    assert not failed, (case, failed)


# ---------------------------------------------------------------------------------------------------------------- the C entry
def _strides(B, H, W, layout):
    """(floats in the buffer, bs, cs, ps) of a 2-channel tensor: element (b, c, pix) at b bs + c cs + pix ps."""
    HW = H * W
    if layout == "planar":
        return B * 2 * HW, 2 * HW, HW, 1
    if layout == "interleaved":
        return B * 2 * HW, 2 * HW, 1, 2
    return B * (2 * HW + 8), 2 * HW + 8, HW, 1


def _index2(B, H, W, layout):
    _, bs, cs, ps = _strides(B, H, W, layout)
    return (torch.arange(B).view(B, 1, 1) * bs + torch.arange(2).view(1, 2, 1) * cs + torch.arange(H * W).view(1, 1, -1) * ps).reshape(-1)


def _entry(f1, f2, coords, cstr, add_grid, dout, out, ostr, shape, C, radius, nlev=None):
    from flow_supervisor_amd import _lib as L
    pp, keep = L.ptr_array(f2)
    rc = L.load().fsraft_altcorr_fused_dcoords(L.ptr(f1), pp, len(f2) if nlev is None else nlev, L.ptr(coords), *cstr, int(add_grid),
                                               L.ptr(dout), L.ptr(out), *ostr, *shape, C, radius, None)
    torch.cuda.synchronize()
    return rc


SHAPE, NLEV, CH = (3, 5, 9), 2, 100           # 135 queries, two rounds of lanes with a ragged tail


@pytest.mark.parametrize("radius", R.RADII)
@pytest.mark.parametrize("layout", ("planar", "interleaved", "planar_gap"))
def test_every_element_of_a_nan_filled_dcoords_is_written_and_nothing_else(layout, radius):
    from flow_supervisor_amd import ops
    B, H, W = SHAPE
    c = A.case(SHAPE, NLEV, CH, radius, "mixed", False)
    dout, ref, S = A.case_expect(SHAPE, NLEV, CH, radius, "mixed", False, "gauss")
    f1, f2 = Buf(c["f1"]), [Buf(f) for f in c["f2"]]
    cbuf, dbuf = Buf(c["given"]), Buf(dout)
    n, bs, cs, ps = _strides(B, H, W, layout)
    obuf = Buf(n=n)
    assert _entry(f1.mid, [b.mid for b in f2], cbuf.mid, (2 * H * W, H * W, 1), False, dbuf.mid, obuf.mid, (bs, cs, ps), SHAPE, CH, radius) == 0
    obuf.intact()
    o, idx = obuf.cpu(), _index2(B, H, W, layout)
    mask = torch.zeros(n, dtype=torch.bool)
    mask[idx] = True
    assert not bool((o[mask].view(torch.int32) == PATTERN).any()), "an element of dcoords was not written"
    assert bool((o[~mask].view(torch.int32) == PATTERN).all()), "a float that is no element of dcoords was written"
    got = o[idx].view(B, 2, H, W)
    w, i = R.need(got, ref, (S * A.U24).expand_as(ref))
    assert w <= A.LIMITS["dcoords"], (w, i)
    want = ops.altcorr_fused_dcoords(f1.mid.view(B, H, W, CH), [b.mid.view(f.shape) for b, f in zip(f2, c["f2"])], cbuf.mid.view(B, 2, H, W),
                                     dbuf.mid.view(dout.shape), radius)
    assert _same_bits(got, want.cpu())
    for b, src in [(f1, c["f1"]), (cbuf, c["given"]), (dbuf, dout)] + list(zip(f2, c["f2"])):      # inputs unchanged, guards intact
        b.intact()
        assert _same_bits(b.cpu(), src.reshape(-1))


@pytest.mark.parametrize("C", (36, 256))
@pytest.mark.parametrize("radius", R.RADII)
def test_nothing_outside_a_level_is_read(radius, C):
    """Every map sits inside an allocation that holds NaN for two image rows before and after it: a read outside a level (a window
    position beyond an edge, a channel beyond C, the row after the last) would reach the result."""
    from flow_supervisor_amd import ops
    shape, nlev = (1, 10, 14), 4
    B, H, W = shape
    c = A.case(shape, nlev, C, radius, "mixed", True)
    dout = R.dout_values(B, H, W, nlev, radius, "gauss").to(DEV)
    given = c["given"].to(DEV)

    def inside_nan(t):
        pad = 2 * t.shape[2] * t.shape[3]
        whole = torch.full((t.numel() + 2 * pad,), float("nan"), device=DEV)
        mid = whole[pad:pad + t.numel()].view(t.shape)
        mid.copy_(t)
        return whole, mid
    held = [inside_nan(t) for t in [c["f1"]] + c["f2"]]
    got = ops.altcorr_fused_dcoords(held[0][1], [m for _, m in held[1:]], given, dout, radius, is_flow=True)
    want = ops.altcorr_fused_dcoords(c["f1"].to(DEV), [f.to(DEV) for f in c["f2"]], given, dout, radius, is_flow=True)
    assert bool(torch.isfinite(got).all())
    assert _same_bits(got.cpu(), want.cpu())


@pytest.mark.parametrize("radius", R.RADII)
def test_views_add_grid_and_two_launches_give_the_same_bits(radius):
    from flow_supervisor_amd import ops
    shape, nlev, C = (2, 16, 24), 4, 32
    B, H, W = shape
    c = A.case(shape, nlev, C, radius, "mixed", True)
    f1, f2 = c["f1"].to(DEV), [f.to(DEV) for f in c["f2"]]
    dout = R.dout_values(B, H, W, nlev, radius, "gauss").to(DEV)
    flow, pos = c["given"].to(DEV), c["pos"].to(DEV)
    first = ops.altcorr_fused_dcoords(f1, f2, flow, dout, radius, is_flow=True)
    again = ops.altcorr_fused_dcoords(f1, f2, flow, dout, radius, is_flow=True)
    assert _same_bits(first, again), "two launches differ"
    assert _same_bits(first, ops.altcorr_fused_dcoords(f1, f2, pos, dout, radius)), "add_grid on the flow differs from grid + flow"
    view = pos.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)                 # a [B,H,W,2] tensor seen as [B,2,H,W]
    assert view.stride() == (2 * H * W, 1, 2 * W, 2)
    assert _same_bits(first, ops.altcorr_fused_dcoords(f1, f2, view, dout, radius)), "strided coordinates differ"
    assert _same_bits(first, ops.altcorr_fused_dcoords(f1, f2, pos, dout.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1), radius))


def test_refused_calls_write_nothing_and_the_wrapper_validates_shapes():
    from flow_supervisor_amd import ops
    B, H, W = SHAPE
    c = A.case(SHAPE, NLEV, CH, 4, "mixed", False)
    f1, f2 = c["f1"].to(DEV), [f.to(DEV) for f in c["f2"]]
    coords, dout = c["given"].to(DEV), R.dout_values(B, H, W, NLEV, 4, "gauss").to(DEV)
    obuf = Buf(n=B * 2 * H * W)
    s = (2 * H * W, H * W, 1)
    refused = [_entry(f1, f2, coords, s, False, dout, obuf.mid, s, SHAPE, CH, 2),
               _entry(f1, f2, coords, s, False, dout, obuf.mid, s, SHAPE, CH, 5),
               _entry(f1, f2, coords, s, False, dout, obuf.mid, s, SHAPE, 0, 4),
               _entry(f1, f2, coords, s, False, dout, obuf.mid, s, SHAPE, 260, 4),
               _entry(f1, f2, coords, s, False, dout, obuf.mid, s, SHAPE, CH, 4, nlev=0),
               _entry(f1, f2, coords, s, False, dout, obuf.mid, s, SHAPE, CH, 4, nlev=5),
               _entry(f1, f2, coords, s, False, dout, obuf.mid, s, (1, 1, 9), CH, 4),          # no second level
               _entry(f1, f2, coords, s, False, dout, None, s, SHAPE, CH, 4),
               _entry(None, f2, coords, s, False, dout, obuf.mid, s, SHAPE, CH, 4)]
    assert refused == [1] * len(refused), refused
    obuf.untouched()
    for bad in (dict(dout=dout[..., :-1]), dict(coords=coords[:, :1]), dict(f2=f2[::-1]), dict(f2=[f[..., :64] for f in f2]),
                dict(f1=f1.permute(0, 2, 1, 3))):
        a = dict(f1=f1, f2=f2, coords=coords, dout=dout)
        a.update(bad)
        with pytest.raises(ValueError):
            ops.altcorr_fused_dcoords(a["f1"], a["f2"], a["coords"], a["dout"], 4)
