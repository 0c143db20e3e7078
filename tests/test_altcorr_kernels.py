"""The five kernels of csrc/altcorr.hip through ops.altcorr_fused_fwd (forced onto the wave-per-query, the tile and the matrix-pipe
kernel), ops.altcorr_fwd / altcorr_bwd and the four C entries, every element against the float64 restatements of
tests/_altcorrref.py.  Cases (_altcorrref.groups / dropin_cases): the shapes of _dcoordsref.SHAPES -- 1x10x14 with four levels
(10x14, 5x7, 2x3, 1x1), 2x16x24, 1x8x8 with one to three levels, 3x5x9 with two (135 queries: ragged 4x4 and 6x4 tiles), 2x8x16 --
at the route's base channel count, the route's channel sweep (wave 1, 4, 36, 65, 100, 128, 256; tile 64 .. 256; matrix pipe 32,
96, 256) on 1x10x14 and 3x5x9, and the region plane 1x32x48 with the families the geometry model proves to reach both the staged
region and the fallback (smooth, jump, limit-K, far-K); radius 3 and 4; add_grid 0 / 1.  The drop-in entries: N = 1 and 3
coordinate sets, fmap2 of the same and of half the size, corr_grad gaussian, zero, one-hot.  The far rows, zero maps and a zero
corr_grad give exactly 0.  Through the C entries: every element of a pattern-filled output is written and nothing beside it, inputs
unchanged, three coordinate layouts / add_grid against grid + flow / two launches / maps and records inside pattern-filled
allocations give the same bits; misaligned maps take the wave-per-query kernel; fmap2_grad accumulates; refused calls write
nothing.  Needs an MI355X: -m gpu.

Limits: _altcorrref.LIMITS (fwd 20 and bwd 30 units of 2^-24 S, matrix pipe 2 units of 2^-16 S: from the fp32 twins on the CPU,
tests/test_altcorrref.py), not from the kernels.  profiles/altcorr_margins.txt lists every comparison (FSRAFT_PARITY_LOG).  Worst
values measured on MI355X, in those units:
  wave-per-query kernel   2.96  limit 20   (1x10x14, 4 levels, C = 4, radius 3, mixed + grid); 2.32 on the region plane; 0.70 at C = 256
  tile kernel             2.62  limit 20   (2x16x24, C = 64, radius 3, mixed); 2.45 on the region plane (mixed), 2.03 on `limit-tile` at C = 128
  matrix-pipe kernel      0.49  limit 2    (1x32x48, C = 32, radius 3, a plane of zeros; units of 2^-16 S); 0.20 at C = 96, 0.12 at C = 256
  drop-in forward         2.66  limit 20   (3x5x9, C = 4, three sets, fmap2 of half the size, radius 3)
  drop-in backward        4.12  limit 30   (1x8x8, C = 36, one set, radius 4, fmap2_grad, gaussian corr_grad)
  backward from a non-zero fmap2_grad   3.10  limit 30   (units of 2^-24 (S2 + |start|))
  far rows and far anchors, zero maps, zero corr_grad, written / unwritten elements, inputs unchanged, pattern-filled surroundings,
  layouts, views, add_grid, two forward launches, misaligned maps on the wave-per-query kernel, fmap1_grad of two runs: exact
"""
import contextlib
import ctypes

import pytest
import torch

import _altcorrref as A
import _dcoordsref as D
from _util import Buf, _log_margin

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _leave_no_cached_segments():
    """(as tests/test_gma_kernels.py: hand the free segments back, later modules count allocated bytes)"""
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32).cpu(), b.contiguous().view(torch.int32).cpu())


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


@contextlib.contextmanager
def _route(route):
    """Force ops.altcorr_fused_fwd / fsraft_altcorr_fused_fwd onto one kernel; the library's and the module's defaults (tile kernel
    on, matrix pipe on, split arithmetic) are put back whatever happens."""
    from flow_supervisor_amd import _lib as L
    from flow_supervisor_amd import ops
    lib = L.load()
    mfma, split = ops.ALT_MFMA, ops.SPLIT_VOLUME_BWD
    try:
        lib.fsraft_set_alt_tile(0 if route == "wave" else 1)
        ops.ALT_MFMA = True
        if route == "mfma":
            assert ops.SPLIT_VOLUME_BWD, "the matrix-pipe lookup needs the default arithmetic"
        yield
    finally:
        lib.fsraft_set_alt_tile(1)
        ops.ALT_MFMA, ops.SPLIT_VOLUME_BWD = mfma, split


def _records(f1, f2):
    from flow_supervisor_amd import ops
    B, C = f1.shape[0], f1.shape[-1]
    return ops.to_records(f1.view(B, -1, C)), [ops.to_records(f.view(B, -1, C)) for f in f2]


def _fused(route, f1, f2, given, radius, is_flow, recs=None, out=None):
    """ops.altcorr_fused_fwd on the kernel of `route`; a route that the arguments cannot take is an error, not another kernel."""
    from flow_supervisor_amd import ops
    C = f1.shape[-1]
    assert all(t.data_ptr() % 16 == 0 for t in [f1] + list(f2))
    if route == "tile":
        assert C % 64 == 0
    if route == "mfma":
        assert C % 32 == 0 and C <= 256
        recs = _records(f1, f2) if recs is None else recs
    with _route(route):
        return ops.altcorr_fused_fwd(f1, f2, given, radius, is_flow=is_flow, recs=recs if route == "mfma" else None, out=out)


GROUPS = [(route,) + g for route in A.ROUTES for g in A.groups(route)]


@pytest.mark.parametrize("radius", A.RADII)
@pytest.mark.parametrize("route,shape,nlev,C,families", GROUPS, ids=_ids)
def test_fused_forward_against_float64(route, shape, nlev, C, families, radius):
    key = A.limit_key(route)
    worst, failed = (-1.0, ""), []
    f1c, f2c = A.maps(shape, nlev, C)[:2]
    f1, f2 = f1c.to(DEV), [f.to(DEV) for f in f2c]
    recs = _records(f1, f2) if route == "mfma" else None
    for family in families:
        for add_grid in (False, True):
            variant = f"{family} grid{int(add_grid)}"
            c = A.case(shape, nlev, C, radius, family, add_grid)
            got = _fused(route, f1, f2, c["given"].to(DEV), radius, add_grid, recs).cpu()
            w, i = D.need(got, c["ref"], c["S"] * A.UNIT[key])
            if w > worst[0]:
                worst = (w, variant)
            if not w <= A.LIMITS[key]:
                failed.append((variant, w, i))
            if family == "mixed" and not bool((got[:, 0] == 0).all()):
                failed.append((variant, "the +-1e6 row must give exactly 0"))
    case = f"{route} {_ids(shape)} L{nlev} C{C} r{radius}"
    _log_margin(f"alt fused fwd {case}", worst[0], A.LIMITS[key], f"worst |got - ref| / ({'2^-16' if key == 'mfma' else '2^-24'} S), {worst[1]}")
    print(f"{case}: worst {worst[0]:.3f} (limit {A.LIMITS[key]}), {worst[1]}")
    assert not failed, (case, failed)


@pytest.mark.parametrize("radius", A.RADII)
@pytest.mark.parametrize("route", ("tile", "mfma"))
def test_far_anchors_leave_the_rest_of_their_tiles_correct_and_give_exactly_zero(route, radius):
    """(part of the comparison above; here on its own so that a failure names the tile) every query of the seven tiles whose
    anchoring query is NaN, +-inf, 1e6, +-30000 or 29999.984375: the far query exactly 0 at every level, the others within the limit."""
    C, key, family = A.BASE_C[route], A.limit_key(route), f"far-{route}"
    (B, H, W), nlev = A.PLANE
    f1c, f2c = A.maps(A.PLANE[0], nlev, C)[:2]
    f1, f2 = f1c.to(DEV), [f.to(DEV) for f in f2c]
    th, tw = A.TILE[route]
    for add_grid in (False, True):
        c = A.case(A.PLANE[0], nlev, C, radius, family, add_grid)
        got = _fused(route, f1, f2, c["given"].to(DEV), radius, add_grid).cpu()
        for m in A.plane_positions(family, radius)[1]:
            mask = A.tile_mask(route, m["tile"], H, W)
            ty, tx = divmod(m["tile"], W // tw)
            far = got[0, ty * th + A.ANCHOR[route][0], tx * tw + A.ANCHOR[route][1]]
            assert bool((far == 0).all()), (m, "the far query must give exactly 0")
            w, i = D.need(got[0][mask], c["ref"][0][mask], c["S"][0][mask] * A.UNIT[key])
            assert w <= A.LIMITS[key], (m, add_grid, w, i)


@pytest.mark.parametrize("route", A.ROUTES)
def test_zero_maps_give_exactly_zero(route):
    shape, nlev, C, radius = (3, 5, 9), 2, 64, 4
    c = A.case(shape, nlev, C, radius, "mixed", False)
    f1, f2 = c["f1"].to(DEV), [f.to(DEV) for f in c["f2"]]
    given = c["given"].to(DEV)
    assert bool((_fused(route, torch.zeros_like(f1), f2, given, radius, False) == 0).all())
    assert bool((_fused(route, f1, [torch.zeros_like(f) for f in f2], given, radius, False) == 0).all())


# ---------------------------------------------------------------------------------------------------------------- the fused C entries
def _strides(B, H, W, layout):
    """(floats in the buffer, bs, cs, ps) of a 2-channel tensor: element (b, c, pix) at b bs + c cs + pix ps."""
    HW = H * W
    if layout == "planar":
        return B * 2 * HW, 2 * HW, HW, 1
    if layout == "interleaved":
        return B * 2 * HW, 2 * HW, 1, 2
    return B * (2 * HW + 8), 2 * HW + 8, HW, 1


def _coords_buf(given, layout):
    """The coordinates in `layout` inside a pattern-filled buffer (the gaps of planar_gap keep the pattern)."""
    B, _, H, W = given.shape
    n, bs, cs, ps = _strides(B, H, W, layout)
    idx = (torch.arange(B).view(B, 1, 1) * bs + torch.arange(2).view(1, 2, 1) * cs + torch.arange(H * W).view(1, 1, -1) * ps).reshape(-1)
    buf = Buf(n=n)
    buf.mid[idx.to(DEV)] = given.reshape(-1).to(DEV)
    return buf, (bs, cs, ps)


def _entry(route, f1, f2, coords, cstr, add_grid, out, shape, C, radius, recs=None, nlev=None):
    """fsraft_altcorr_fused_fwd (wave / tile) or fsraft_altcorr_mfma_fwd on raw tensors; the status."""
    from flow_supervisor_amd import _lib as L
    pp, keep = L.ptr_array(f2)
    nl = len(f2) if nlev is None else nlev
    with _route(route):
        if route == "mfma":
            pr, keep2 = L.ptr_array(recs[1])
            rc = L.load().fsraft_altcorr_mfma_fwd(L.ptr(recs[0]), pr, L.ptr(f1), pp, nl, L.ptr(coords), *cstr, int(add_grid), L.ptr(out),
                                                  *shape, C, radius, None)
        else:
            rc = L.load().fsraft_altcorr_fused_fwd(L.ptr(f1), pp, nl, L.ptr(coords), *cstr, int(add_grid), L.ptr(out), *shape, C, radius, None)
        torch.cuda.synchronize()
    return rc


ENTRY_SHAPE, ENTRY_NLEV = (3, 5, 9), 2           # 135 queries: ragged tiles of either kind
ENTRY_C = dict(wave=100, tile=64, mfma=96)


@pytest.mark.parametrize("radius", A.RADII)
@pytest.mark.parametrize("route", A.ROUTES)
def test_fused_entries_write_every_element_and_nothing_else_in_every_layout(route, radius):
    """Maps, records and coordinates handed in from inside pattern-filled allocations (a read outside a level, a channel beyond C or
    a gap of the coordinates would reach the result); the output pattern-filled; the three coordinate layouts give the same bits
    as ops.altcorr_fused_fwd on clean tensors; the inputs are unchanged and every guard is intact."""
    B, H, W = ENTRY_SHAPE
    C, key = ENTRY_C[route], A.limit_key(route)
    c = A.case(ENTRY_SHAPE, ENTRY_NLEV, C, radius, "mixed", False)
    f1c, f2c = c["f1"].to(DEV), [f.to(DEV) for f in c["f2"]]
    want = _fused(route, f1c, f2c, c["given"].to(DEV), radius, False)
    w, i = D.need(want.cpu(), c["ref"], c["S"] * A.UNIT[key])
    assert w <= A.LIMITS[key], (w, i)
    f1, f2 = Buf(c["f1"]), [Buf(f) for f in c["f2"]]
    held = [(f1, c["f1"])] + list(zip(f2, c["f2"]))
    recs = None
    if route == "mfma":
        r1, r2 = _records(f1c, f2c)
        b1, b2 = Buf(r1), [Buf(r) for r in r2]
        recs = (b1.mid, [b.mid for b in b2])
        held += [(b1, r1)] + list(zip(b2, r2))
    for layout in ("planar", "interleaved", "planar_gap"):
        cbuf, cstr = _coords_buf(c["given"], layout)
        before = cbuf.whole.clone()
        obuf = Buf(n=want.numel())
        assert _entry(route, f1.mid, [b.mid for b in f2], cbuf.mid, cstr, False, obuf.mid, ENTRY_SHAPE, C, radius, recs) == 0
        obuf.written()
        assert _same_bits(obuf.mid, want.reshape(-1)), layout
        assert _same_bits(cbuf.whole, before), "the coordinates were written"
    for b, src in held:
        b.intact()
        assert _same_bits(b.mid, src.reshape(-1)), "an input was written"


@pytest.mark.parametrize("radius", A.RADII)
@pytest.mark.parametrize("route", A.ROUTES)
def test_add_grid_views_and_two_launches_give_the_same_bits(route, radius):
    from flow_supervisor_amd import ops
    shape, nlev, C = (2, 16, 24), 4, dict(wave=36, tile=64, mfma=32)[route]
    B, H, W = shape
    c = A.case(shape, nlev, C, radius, "mixed", True)
    f1, f2 = c["f1"].to(DEV), [f.to(DEV) for f in c["f2"]]
    flow, pos = c["given"].to(DEV), c["pos"].to(DEV)
    first = _fused(route, f1, f2, flow, radius, True)
    assert _same_bits(first, _fused(route, f1, f2, flow, radius, True)), "two launches differ"
    assert _same_bits(first, _fused(route, f1, f2, pos, radius, False)), "add_grid on the flow differs from grid + flow"
    view = pos.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)                 # a [B,H,W,2] tensor seen as [B,2,H,W]
    assert view.stride() == (2 * H * W, 1, 2 * W, 2)
    assert _same_bits(first, _fused(route, f1, f2, view, radius, False)), "strided coordinates differ"
    out = torch.empty_like(first)
    assert _fused(route, f1, f2, flow, radius, True, out=out) is out and _same_bits(first, out)
    wide = torch.empty(*out.shape[:3], out.shape[3] + 1, device=DEV)[..., :-1]      # the right shape, another stride
    assert wide.shape == out.shape and not wide.is_contiguous()
    for bad in (out[..., :-1], out.double(), wide, out.view(B, W, H, -1), out[:1]):
        with pytest.raises(ValueError):
            ops.altcorr_fused_fwd(f1, f2, flow, radius, is_flow=True, out=bad)


@pytest.mark.parametrize("radius", A.RADII)
@pytest.mark.parametrize("which", ("fmap1", "level0", "level1"))
def test_misaligned_maps_take_the_wave_per_query_kernel(which, radius):
    """The tile kernel reads fmap1 and every level 16 bytes at a time: fsraft_altcorr_fused_fwd hands a call whose fmap1, or any
    level, sits 4 bytes off a 16-byte boundary to the wave-per-query kernel -- the same bits as that kernel on aligned maps, which
    on this input are not the tile kernel's bits."""
    C = 64
    B, H, W = ENTRY_SHAPE
    c = A.case(ENTRY_SHAPE, ENTRY_NLEV, C, radius, "mixed", False)
    f1c, f2c, given = c["f1"].to(DEV), [f.to(DEV) for f in c["f2"]], c["given"].to(DEV)
    wave, tile = _fused("wave", f1c, f2c, given, radius, False), _fused("tile", f1c, f2c, given, radius, False)
    assert not _same_bits(wave, tile), "the two kernels cannot be told apart on this input"
    off = dict(fmap1=(1, 0, 0), level0=(0, 1, 0), level1=(0, 0, 1))[which]
    f1 = Buf(c["f1"], offset=off[0])
    f2 = [Buf(f, offset=o) for f, o in zip(c["f2"], off[1:])]
    assert sorted(b.mid.data_ptr() % 16 for b in [f1] + f2) == [0, 0, 4]
    obuf = Buf(n=wave.numel())
    s = (2 * H * W, H * W, 1)
    assert _entry("tile", f1.mid, [b.mid for b in f2], given, s, False, obuf.mid, ENTRY_SHAPE, C, radius) == 0
    obuf.written()
    assert _same_bits(obuf.mid, wave.reshape(-1))
    w, i = D.need(obuf.cpu().view(wave.shape), c["ref"], c["S"] * A.U24)
    assert w <= A.LIMITS["fwd"], (w, i)
    for b in [f1] + f2:
        b.intact()


def test_refused_fused_calls_write_nothing():
    """Argument checks on the host: no kernel is launched with a bad argument."""
    B, H, W = ENTRY_SHAPE
    C = 64
    c = A.case(ENTRY_SHAPE, ENTRY_NLEV, C, 4, "mixed", False)
    f1, f2, given = c["f1"].to(DEV), [f.to(DEV) for f in c["f2"]], c["given"].to(DEV)
    recs = _records(f1, f2)
    four = f2 + f2                                                     # (pointers only: a refused call reads none of them)
    recs4 = (recs[0], recs[1] + recs[1])
    obuf = Buf(n=B * H * W * 4 * 81)
    s = (2 * H * W, H * W, 1)
    odd_map, odd_rec = Buf(c["f2"][1], offset=1), Buf(recs[1][1], offset=1)

    def call(route, f1=f1, f2=f2, shape=ENTRY_SHAPE, C=C, radius=4, recs=recs, nlev=None):
        return _entry(route, f1, f2, given, s, False, obuf.mid, shape, C, radius, recs, nlev)

    refused = []
    for route in ("tile", "mfma"):
        r4 = recs4 if route == "mfma" else None
        refused += [call(route, radius=2), call(route, radius=5), call(route, C=0), call(route, C=257), call(route, nlev=0),
                    call(route, f2=four, recs=recs4, nlev=5), call(route, f2=four, recs=r4, shape=(1, 5, 7)),      # no fourth level
                    call(route, f1=None)]
    refused += [call("mfma", C=48), call("mfma", C=288),
                call("mfma", f2=[f2[0], odd_map.mid]), call("mfma", recs=(recs[0], [recs[1][0], odd_rec.mid])),
                call("mfma", f1=Buf(c["f1"], offset=1).mid), call("mfma", recs=(Buf(recs[0], offset=1).mid, recs[1]))]
    assert refused == [1] * len(refused), refused
    from flow_supervisor_amd import _lib as L
    for route in ("tile", "mfma"):                                     # a null level pointer
        arr = (ctypes.c_void_p * 2)(f2[0].data_ptr(), None)
        pp, pr = ctypes.cast(arr, L._PP), L.ptr_array(recs[1])[0]
        if route == "mfma":
            rc = L.load().fsraft_altcorr_mfma_fwd(L.ptr(recs[0]), pr, L.ptr(f1), pp, 2, L.ptr(given), *s, 0, L.ptr(obuf.mid), B, H, W, C, 4, None)
        else:
            rc = L.load().fsraft_altcorr_fused_fwd(L.ptr(f1), pp, 2, L.ptr(given), *s, 0, L.ptr(obuf.mid), B, H, W, C, 4, None)
        assert rc == 1, route
    torch.cuda.synchronize()
    obuf.untouched()


# ---------------------------------------------------------------------------------------------------------------- the drop-in entries
DROPIN = A.dropin_cases()


@pytest.mark.parametrize("radius", A.RADII)
@pytest.mark.parametrize("shape,C,N,half,family,kinds", DROPIN, ids=_ids)
def test_dropin_forward_and_backward_against_float64(shape, C, N, half, family, kinds, radius):
    from flow_supervisor_amd import ops
    c = A.dropin_case(shape, C, N, half, family)
    f1, f2, coords = c["f1"].to(DEV), c["f2"].to(DEV), c["coords"].to(DEV)
    case = f"{_ids(shape)} C{C} N{N} {'half' if half else 'same'} {family} r{radius}"
    ref, S = A.dropin_expect(c["f1"], c["f2"], c["coords"], radius)
    got = ops.altcorr_fwd(f1, f2, coords, radius).cpu()
    fw, i = D.need(got, ref, S * A.U24)
    _log_margin(f"alt drop-in fwd {case}", fw, A.LIMITS["fwd"], "worst |got - ref| / (2^-24 S)")
    assert fw <= A.LIMITS["fwd"], (case, fw, i)
    if family == "mixed":
        assert bool((got[:, :, :, 0] == 0).all()), "the +-1e6 row must give exactly 0"
    worst = (-1.0, "")
    for gk in kinds:
        g = A.grad_values(shape, N, radius, gk)
        g1, g2, S1, S2 = A.dropin_bwd(c["f1"], c["f2"], c["coords"], g, radius)
        o1, o2, o3 = ops.altcorr_bwd(f1, f2, coords, g.to(DEV), radius)
        assert o3.shape == coords.shape and bool((o3 == 0).all())
        for name, o, r, s in (("fmap1_grad", o1.cpu(), g1, S1), ("fmap2_grad", o2.cpu(), g2, S2)):
            w, i = D.need(o, r, s * A.U24)
            if w > worst[0]:
                worst = (w, f"{name} {gk}")
            assert w <= A.LIMITS["bwd"], (case, name, gk, w, i)
            if gk == "zero":
                assert bool((o == 0).all()), (case, name, "a zero corr_grad must give exactly 0")
        if family == "mixed":
            assert bool((o1[:, 0] == 0).all()), "the +-1e6 row must give exactly 0"
    _log_margin(f"alt drop-in bwd {case}", worst[0], A.LIMITS["bwd"], f"worst |got - ref| / (2^-24 S), {worst[1]}")
    print(f"{case}: fwd {fw:.3f}, bwd worst {worst[0]:.3f} (limit {A.LIMITS['bwd']}), {worst[1]}")


def _dropin_entry(name, tensors, dims, C, radius):
    from flow_supervisor_amd import _lib as L
    rc = getattr(L.load(), name)(*[L.ptr(t) for t in tensors], *dims, C, radius, None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("radius", A.RADII)
@pytest.mark.parametrize("N,half", [(1, False), (3, True)])
def test_dropin_entries_write_their_outputs_and_accumulate_fmap2_grad(N, half, radius):
    """corr and fmap1_grad from pattern-filled buffers: every element written, nothing beside them.  fmap2_grad is added into what
    the entry is handed (the contract is accumulate): from a non-zero start s the result is held to s + fmap2_grad with s as one
    more term of the sum, i.e. on the scale S2 + |s|.  Two runs agree within the backward limit (the atomics are not bit-stable);
    two forward runs give the same bits.  Inputs unchanged."""
    import flow_supervisor_amd.alt_cuda_corr as acc
    shape, C = (3, 5, 9), 100
    B, H, W = shape
    c = A.dropin_case(shape, C, N, half, "mixed")
    H2, W2 = c["f2"].shape[1:3]
    dims = (B, N, H, W, H2, W2)
    g = A.grad_values(shape, N, radius, "gauss")
    f1, f2, co, gb = Buf(c["f1"]), Buf(c["f2"]), Buf(c["coords"]), Buf(g)
    ref, S = A.dropin_expect(c["f1"], c["f2"], c["coords"], radius)
    g1, g2, S1, S2 = A.dropin_bwd(c["f1"], c["f2"], c["coords"], g, radius)
    corr = Buf(n=ref.numel())
    assert _dropin_entry("fsraft_altcorr_fwd", (f1.mid, f2.mid, co.mid, corr.mid), dims, C, radius) == 0
    corr.written()
    w, i = D.need(corr.cpu().view(ref.shape), ref, S * A.U24)
    assert w <= A.LIMITS["fwd"], (w, i)
    again = Buf(n=ref.numel())
    assert _dropin_entry("fsraft_altcorr_fwd", (f1.mid, f2.mid, co.mid, again.mid), dims, C, radius) == 0
    assert _same_bits(corr.mid, again.mid), "two forward launches differ"
    (mod,) = acc.forward(f1.mid.view(c["f1"].shape), f2.mid.view(c["f2"].shape), co.mid.view(c["coords"].shape), radius)
    assert _same_bits(mod.reshape(-1), corr.mid)

    start = torch.randn(g2.shape, generator=D._gen("start", N, radius), dtype=torch.float32)
    runs = []
    for _ in range(2):
        o1, o2 = Buf(n=g1.numel()), Buf(start)
        assert _dropin_entry("fsraft_altcorr_bwd", (f1.mid, f2.mid, co.mid, gb.mid, o1.mid, o2.mid), dims, C, radius) == 0
        o1.written()
        o2.intact()
        runs.append((o1.cpu().view(g1.shape), o2.cpu().view(g2.shape)))
    w1, i1 = D.need(runs[0][0], g1, S1 * A.U24)
    w2, i2 = D.need(runs[0][1], start.double() + g2, (S2 + start.double().abs()) * A.U24)
    _log_margin(f"alt bwd entry from a non-zero fmap2_grad N{N} r{radius}", max(w1, w2), A.LIMITS["bwd"], "2^-24 (S2 + |start|)")
    assert w1 <= A.LIMITS["bwd"] and w2 <= A.LIMITS["bwd"], (w1, i1, w2, i2)
    assert not torch.equal(runs[0][1], start), "fmap2_grad was not added to"
    assert _same_bits(runs[0][0], runs[1][0]), "fmap1_grad has no atomics: two runs give the same bits"
    wr, ir = D.need(runs[1][1], runs[0][1].double(), (S2 + start.double().abs()) * A.U24)
    assert wr <= A.LIMITS["bwd"], (wr, ir)
    m1, m2, m3 = acc.backward(f1.mid.view(c["f1"].shape), f2.mid.view(c["f2"].shape), co.mid.view(c["coords"].shape),
                              gb.mid.view(g.shape), radius)
    assert bool((m3 == 0).all()) and m3.shape == c["coords"].shape
    assert D.need(m2.cpu(), g2, S2 * A.U24)[0] <= A.LIMITS["bwd"] and _same_bits(m1, runs[0][0])
    for b, src in ((f1, c["f1"]), (f2, c["f2"]), (co, c["coords"]), (gb, g)):
        b.intact()
        assert _same_bits(b.mid, src.reshape(-1)), "an input was written"


def test_refused_dropin_calls_write_nothing():
    """Argument checks on the host, the backward's size check among them: no kernel is launched with a bad argument."""
    shape, C, N = (3, 5, 9), 36, 1
    B, H, W = shape
    c = A.dropin_case(shape, C, N, False, "mixed")
    f1, f2, co = c["f1"].to(DEV), c["f2"].to(DEV), c["coords"].to(DEV)
    g = A.grad_values(shape, N, 4, "gauss").to(DEV)
    corr, o1, o2 = Buf(n=g.numel()), Buf(n=f1.numel()), Buf(n=f2.numel())
    dims = (B, N, H, W, H, W)
    bad_dims = [(0, N, H, W, H, W), (B, 0, H, W, H, W), (B, N, 0, W, H, W), (B, N, H, 0, H, W), (B, N, H, W, 0, W), (B, N, H, W, H, 0),
                (B, N, -H, W, H, W)]
    refused = []
    for d, ch, r in [(dims, C, 2), (dims, C, 5), (dims, 0, 4), (dims, 257, 4)] + [(d, C, 4) for d in bad_dims]:
        refused.append(_dropin_entry("fsraft_altcorr_fwd", (f1, f2, co, corr.mid), d, ch, r))
        refused.append(_dropin_entry("fsraft_altcorr_bwd", (f1, f2, co, g, o1.mid, o2.mid), d, ch, r))
    refused.append(_dropin_entry("fsraft_altcorr_fwd", (f1, None, co, corr.mid), dims, C, 4))
    refused.append(_dropin_entry("fsraft_altcorr_bwd", (f1, f2, co, None, o1.mid, o2.mid), dims, C, 4))
    assert refused == [1] * len(refused), refused
    for b in (corr, o1, o2):
        b.untouched()
