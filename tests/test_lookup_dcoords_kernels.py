"""lookup_dcoords_kernel of csrc/corr_dcoords.hip behind both of its window loaders, called through the C entry points
fsraft_corr_lookup_tiled_dcoords (tiled-row volume) and fsraft_corr_lookup_dcoords (row-major levels), every element against the
float64 restatement of tests/_dcoordsref.py.  Shapes (_dcoordsref.SHAPES): 1x10x14 with four levels (10x14, 5x7, 2x3, 1x1: each
smaller than, or no multiple of, the 4x4 tile and the window), 2x16x24, 1x8x8 with one, two and three levels, 3x5x9 with two (135
queries: no multiple of a wave's four or a workgroup's sixteen), 2x8x16 (256: a multiple of both); radius 3 and 4.  Coordinates:
multiples of 1/64 across and beyond the plane, exact integers, positions within a cell of an edge, a row of +-1e6 (gradient exactly
0), and a plane of zeros; planar, planar-with-a-gap and [B,H,W,2] layouts through bs / cs / ps, for the coordinates and for
dcoords alike (the gap keeps the pattern).  add_grid 0 / 1 (tiled), nhwc_in 0 / 1 (row-major).  dout gaussian, zero, and a one on
the first / last channel of every level.  The row-major levels are copied out of the tiled volume with VolLayout.level_view and
the two entry points must agree within the same limit; two launches give the same bits; a refused call returns 1 and writes
nothing.  The test owns every buffer (_util.Buf: guard rows, pad cells of the volume and unwritten outputs hold a NaN pattern) and
compares the inputs bit for bit afterwards.  Needs an MI355X: -m gpu.

Limit: _dcoordsref.LIMITS (8 units of 2^-24 S, from the fp32 twins on the CPU: tests/test_dcoordsref.py), not from the kernel.
profiles/lookup_dcoords_margins.txt lists every comparison (FSRAFT_PARITY_LOG).  Worst values measured on MI355X, in those units:
  tiled dcoords = rows dcoords        1.80  limit 8   (2x16x24, 4 levels, radius 3)
  tiled vs rows                          0  limit 8   (every case: the two loaders feed the same arithmetic)
  far row, zero dout, written / unwritten elements, inputs unchanged, two launches: exact in every case
Two wrong kernels were run against this file once (built aside, not kept): with i and j swapped in the region offset 14 of the 17
tests fail, with the 2^-l factor dropped 12 fail (the one-level cases pass, as they must).
"""
import ctypes
import itertools

import pytest
import torch

import _dcoordsref as R
from _util import Buf, PATTERN, _log_margin

pytestmark = pytest.mark.gpu
FS_ERR_ARG = 1
LAYOUTS = ("planar", "interleaved", "planar_gap")


@pytest.fixture(scope="module", autouse=True)
def _leave_no_cached_segments():
    """(as tests/test_gma_kernels.py: hand the free segments back, later modules count allocated bytes)"""
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def L():
    from flow_supervisor_amd import _lib
    _lib.load()
    return _lib


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _nan_fill(n):
    return torch.full((n,), PATTERN, dtype=torch.int32).view(torch.float32)


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def _strides(B, H, W, layout):
    """(floats in the buffer, bs, cs, ps) of a 2-channel tensor: element (b, c, pix) at b bs + c cs + pix ps."""
    HW = H * W
    if layout == "planar":
        return B * 2 * HW, 2 * HW, HW, 1
    if layout == "interleaved":
        return B * 2 * HW, 2 * HW, 1, 2
    return B * (2 * HW + 8), 2 * HW + 8, HW, 1


def _pack2(t, layout):
    """[B,2,H,W] -> flat CPU tensor in `layout`; floats that are no element hold the NaN pattern."""
    B, _, H, W = t.shape
    n, bs, cs, ps = _strides(B, H, W, layout)
    flat = _nan_fill(n).clone()
    idx = (torch.arange(B).view(B, 1, 1) * bs + torch.arange(2).view(1, 2, 1) * cs + torch.arange(H * W).view(1, 1, -1) * ps)
    flat[idx.reshape(-1)] = t.reshape(-1).float()
    return flat, idx.reshape(-1)


class Tally:
    """The comparisons of one test: every figure is logged (the worst per output, with the variant it occurred in) before
    anything is asserted."""

    def __init__(self, case):
        self.case, self.worst, self.failed = case, {}, []

    def check(self, name, got, ref, S, variant):
        w, i = R.need(got, ref, (S * R.U24).expand_as(ref))
        if w >= self.worst.get(name, (-1.0,))[0]:
            self.worst[name] = (w, R.LIMITS["dcoords"], variant)
        if not w <= R.LIMITS["dcoords"]:
            self.failed.append((name, variant, w, i))

    def exact(self, name, ok, variant=""):
        self.worst[name] = max(self.worst.get(name, (0.0, 0.0, "")), (0.0 if ok else 1.0, 0.0, variant))
        if not ok:
            self.failed.append((name, variant))

    def done(self):
        for name, (w, lim, variant) in sorted(self.worst.items()):
            _log_margin(f"{name} {self.case}", w, lim, f"worst |got - ref| / (2^-24 S), {variant}" if lim else f"exact, {variant}")
        assert not self.failed, (self.case, self.failed)


class Volume:
    """The tiled volume of a case and the row-major levels copied out of it (VolLayout.level_view), each in guarded buffers."""

    def __init__(self, shape, nlev):
        from flow_supervisor_amd import ops
        B, H, W = shape
        self.levels = R.level_values(B, H, W, nlev)
        self.host = R.tile_rows(self.levels, H, W, PATTERN)
        self.vol = Buf(self.host)
        lay = ops.VolLayout.get(H, W, nlev)
        assert lay.P == self.host.shape[1]
        views = [lay.level_view(self.vol.mid.view(B * H * W, lay.P), l) for l in range(nlev)]
        for v, lv in zip(views, self.levels):
            assert _same_bits(v[:, 0].cpu(), lv), "level_view does not return the level that was packed"
        self.rows = [Buf(v) for v in views]
        self.keep = (ctypes.c_void_p * nlev)(*[b.mid.data_ptr() for b in self.rows])

    def row_pointers(self, L):
        return ctypes.cast(self.keep, L._PP)

    def unchanged(self):
        ok = _same_bits(self.vol.cpu(), self.host.reshape(-1))
        self.vol.intact()
        for b, lv in zip(self.rows, self.levels):
            ok = ok and _same_bits(b.cpu(), lv.reshape(-1))
            b.intact()
        return ok


def _launch(L, vol, kind, shape, nlev, radius, cbuf, cstr, dbuf, nhwc, obuf, ostr, add_grid):
    B, H, W = shape
    lib = L.load()
    if kind == "tiled":
        return lib.fsraft_corr_lookup_tiled_dcoords(L.ptr(vol.vol.mid), nlev, L.ptr(cbuf.mid), *cstr, L.ptr(dbuf.mid), L.ptr(obuf.mid), *ostr,
                                                    B, H, W, radius, int(add_grid), None)
    return lib.fsraft_corr_lookup_dcoords(vol.row_pointers(L), nlev, L.ptr(cbuf.mid), *cstr, L.ptr(dbuf.mid), int(nhwc), L.ptr(obuf.mid), *ostr,
                                          B, H, W, radius, None)


@pytest.mark.parametrize("radius", R.RADII)
@pytest.mark.parametrize("shape,nlev", R.SHAPES, ids=_ids)
def test_dcoords_against_float64(L, shape, nlev, radius):
    B, H, W = shape
    vol = Volume(shape, nlev)
    T = Tally(f"{_ids(shape)} L{nlev} r{radius}")
    layouts = itertools.cycle(itertools.product(LAYOUTS, LAYOUTS))
    for ckind in R.COORD_KINDS:
        for add_grid in (False, True):
            c = R.case(shape, nlev, radius, ckind, add_grid)
            for dkind in R.dout_kinds(nlev):
                dout, ref, S = R.case_expect(shape, nlev, radius, ckind, add_grid, dkind)
                # every pair of layouts for the gaussian dout, one pair in turn for the others
                for clay, olay in (itertools.product(LAYOUTS, LAYOUTS) if dkind == "gauss" and not add_grid else [next(layouts)]):
                    variant = f"{ckind} grid{int(add_grid)} {dkind} coords {clay} dcoords {olay}"
                    on, obs, ocs, ops_ = _strides(B, H, W, olay)
                    _, oidx = _pack2(torch.zeros(B, 2, H, W), olay)
                    got = {}
                    for kind in ("tiled", "rows"):
                        # the row-major entry has no add_grid: it is handed the positions themselves
                        given = c["given"] if kind == "tiled" else c["pos"]
                        chost, _ = _pack2(given, clay)
                        cbuf, obuf = Buf(chost), Buf(n=on)
                        nhwc = kind == "tiled" or (dkind != "gauss") or clay != "planar"          # NCHW dout: gaussian, planar coords
                        dhost = dout if nhwc else dout.permute(0, 3, 1, 2).contiguous()
                        dbuf = Buf(dhost)
                        rc = _launch(L, vol, kind, shape, nlev, radius, cbuf, _strides(B, H, W, clay)[1:], dbuf, nhwc, obuf, (obs, ocs, ops_),
                                     add_grid and kind == "tiled")
                        torch.cuda.synchronize()
                        assert rc == 0, (variant, kind, rc)
                        obuf.intact()
                        o = obuf.cpu()
                        mask = torch.zeros(on, dtype=torch.bool)
                        mask[oidx] = True
                        T.exact(f"{kind} every element written, nothing else", not bool((o[mask].view(torch.int32) == PATTERN).any())
                                and bool((o[~mask].view(torch.int32) == PATTERN).all()), variant)
                        g = o[oidx].view(B, 2, H, W)
                        got[kind] = g
                        T.check(f"{kind} dcoords", g, ref, S, variant)
                        if ckind == "mixed":
                            T.exact(f"{kind} far row exactly 0", bool((g[:, :, 0] == 0).all()), variant)
                        if dkind == "zero":
                            T.exact(f"{kind} zero dout gives 0", bool((g == 0).all()), variant)
                        T.exact(f"{kind} inputs unchanged", _same_bits(cbuf.cpu(), chost) and _same_bits(dbuf.cpu(), dhost.reshape(-1))
                                and vol.unchanged(), variant)
                        cbuf.intact()
                        dbuf.intact()
                    T.check("tiled vs rows", got["tiled"], got["rows"].double(), S, variant)
    T.done()


@pytest.mark.parametrize("kind", ("tiled", "rows"))
def test_two_launches_give_the_same_bits(L, kind):
    shape, nlev, radius = (2, 16, 24), 4, 4
    B, H, W = shape
    vol = Volume(shape, nlev)
    c = R.case(shape, nlev, radius, "mixed", False)
    dout = R.dout_values(B, H, W, nlev, radius, "gauss")
    cbuf, dbuf = Buf(c["given"]), Buf(dout)
    n, bs, cs, ps = _strides(B, H, W, "planar")
    outs = []
    for _ in range(2):
        obuf = Buf(n=n)
        assert _launch(L, vol, kind, shape, nlev, radius, cbuf, (bs, cs, ps), dbuf, True, obuf, (bs, cs, ps), False) == 0
        torch.cuda.synchronize()
        obuf.written()
        outs.append(obuf.cpu())
    assert _same_bits(outs[0], outs[1])


def test_refused_calls_write_nothing(L):
    shape, nlev, radius = (1, 8, 8), 3, 4
    B, H, W = shape
    vol = Volume(shape, nlev)
    n, bs, cs, ps = _strides(B, H, W, "planar")
    cbuf, obuf = Buf(R.coords_values(B, H, W, "mixed")), Buf(n=n)
    dbuf = Buf(torch.ones(B, H, W, 5 * 81))
    lib = L.load()
    null = ctypes.c_void_p(None)
    a = (L.ptr(cbuf.mid), bs, cs, ps, L.ptr(dbuf.mid))
    o = (bs, cs, ps)
    refused = [
        lib.fsraft_corr_lookup_tiled_dcoords(L.ptr(vol.vol.mid), nlev, *a, L.ptr(obuf.mid), *o, B, H, W, 2, 0, None),
        lib.fsraft_corr_lookup_tiled_dcoords(L.ptr(vol.vol.mid), 5, *a, L.ptr(obuf.mid), *o, B, H, W, radius, 0, None),
        lib.fsraft_corr_lookup_tiled_dcoords(L.ptr(vol.vol.mid), nlev, *a, null, *o, B, H, W, radius, 0, None),
        lib.fsraft_corr_lookup_tiled_dcoords(null, nlev, *a, L.ptr(obuf.mid), *o, B, H, W, radius, 0, None),
        lib.fsraft_corr_lookup_tiled_dcoords(L.ptr(vol.vol.mid), 1, *a, L.ptr(obuf.mid), *o, 1 << 27, 4, 4, radius, 0, None),
        lib.fsraft_corr_lookup_dcoords(vol.row_pointers(L), nlev, *a, 1, L.ptr(obuf.mid), *o, B, H, W, 2, None),
        lib.fsraft_corr_lookup_dcoords(vol.row_pointers(L), 5, *a, 1, L.ptr(obuf.mid), *o, B, H, W, radius, None),
        lib.fsraft_corr_lookup_dcoords(vol.row_pointers(L), nlev, *a, 1, null, *o, B, H, W, radius, None),
        lib.fsraft_corr_lookup_dcoords(ctypes.cast(null, L._PP), nlev, *a, 1, L.ptr(obuf.mid), *o, B, H, W, radius, None),
        lib.fsraft_corr_lookup_dcoords(vol.row_pointers(L), 1, *a, 1, L.ptr(obuf.mid), *o, 1 << 27, 4, 4, radius, None),
    ]
    torch.cuda.synchronize()
    assert refused == [FS_ERR_ARG] * len(refused), refused
    obuf.untouched()
    assert vol.unchanged()
