"""The forward kernels of csrc/corr_build.hip (volume + pyramid builds, pool kernels), lookup_tiled_fwd_kernel of csrc/corr_tiled.hip and
the forward kernels of csrc/corr_lookup.hip, called through their C entry points, every element against the float64 restatements of
tests/_corrref.py at the edges of their launch geometry.  The test owns every buffer (_util.Buf: guard rows, unwritten outputs and
the pad cells of hand-made volumes hold a NaN pattern) and compares the inputs bit for bit afterwards.  Needs an MI355X: -m gpu.  The backward kernels: tests/test_corr_bwd_kernels.py.

Build (_corrref.BUILD_SHAPES: 1x1 with C = 2, 3x5, 8x8 down to 1x1, 9x17, 10x14, 8x33, 15x17 / 16x16 / 1x257 = 255 / 256 / 257
queries, 2 x 13x22; C in {2, 14, 16, 18, 34}, records C in {32, 64, 96, 256}; gaussian maps, one sample scaled by 2^10 / 2^-10, a
single non-zero channel, a zero map).  fsraft_corr_build is handed an array of four level pointers every time and the number of
levels the shape has (1x1, 3x5 and 1x257 have no four levels; four on such a map is a refusal, tested as one).  Routes:
    fsraft_set_build_split(0) / (1)      corr_build_kernel / corr_build_split_kernel (fsraft_corr_build),
                                         corr_build_tiled_kernel / corr_build_tiled_split_kernel (fsraft_corr_build_tiled)
    fsraft_corr_build_rec                corr_build_rec_kernel on records made by _gmaref.records_encode on the CPU;
    fsraft_set_build_kernel(k << 16)     k = 1, 2, 3: plain / sc1 / nt stores (0: chosen by size, plain here); (1 << 8): stagger 1
    fsraft_corr_pool_pyramid[_same]      corr_pool_kernel (130x129 down to 1x1; 3 rows of 9x11; 4097 rows of 128x128, whose level 1 is
                                         16 workgroups past the 65536 cap: the second trip of the grid-stride loop), corr_pool_same_kernel
Tiled lookup (fsraft_corr_lookup_tiled_fwd; _corrref.TILED_SHAPES, radius 3 / 4, coordinates mixed / zero, planar / gap / interleaved,
add_grid 0 / 1, volume gaussian / one cell of a level 1): fsraft_set_lookup_policy -1, 0, 2, 16, 18 = lookup_tiled_fwd_kernel<R, 4, AUX>
with AUX 0 (-1 picks 0 below 300 MB), 0, 2, 16, 18 -- identical bits; the volume is hand-made with the NaN pattern in every pad cell
and in the tail of the row, and must give the bits of the same volume with zero pads.
Row-major lookup (fsraft_corr_lookup_fwd, and fsraft_corr_lookup_fwd_same on a 'SAME' pyramid), fsraft_set_lookup_qb -> kernel for
nhwc_out = 1 / 0 (ROUTES below, asserted against a restatement of fsraft_set_lookup_qb + dispatch_fwd + pick_qb):
    0   corr_lookup_fwd_cl_kernel<R, 8, 256> / corr_lookup_fwd_kernel<R, 4, 32>        8   cl<8, 256> / generic<8>
    16  cl<16, 256> / generic<16>                                                      32  cl<32, 256> / generic<32>
    108, 116, 132   generic<8>, <16>, <32> for both outputs
    208 cl<8, 128> / generic<8>                                                        308 cl<8, 320> / generic<8>
One chain: records -> fsraft_corr_build_rec -> fsraft_corr_lookup_tiled_fwd at 2 x 13x22, C = 64, bounded by the sum of the two stages'
bounds (the lookup's weights applied to the build's error scale).  Refused calls return 1 and write nothing.
Not covered: fsraft_set_lookup_policy(100) (the GATHER instantiation: measurement only, it writes nothing), and NaN coordinates (the
kernels map them to an empty window where the restatement would give NaN).

Limits: _corrref.LIMITS, from the fp32 twins on the CPU (tests/test_corrref.py), not from the kernels.  profiles/
corr_kernel_margins.txt lists every comparison (FSRAFT_PARITY_LOG).  Worst values measured on MI355X, in the units of _corrref's scales:
  rows / tiled build, exact (fp32 MFMA)              6.42  limit 30    (1x1x257, C 34, gaussian; the two layouts agree bit for bit)
  rows / tiled build, split (bf16x3)                 1.66  limit 7     (2x13x22, C 16, one channel)        [units of 2^-16 S]
  record build                                       1.70  limit 7     (1x16x16, C 96, one channel)        [units of 2^-16 S]
  pool                                               2.61  limit 20    (4097x128x128, level 1)
  pool_same                                          1.26  limit 6     (3x9x11, level 1);  = the floor pyramid at 8x8: 0.66
  tiled lookup (two lerps)                           27.7  limit 2000  (2x16x24, radius 3, one cell of level 2 is 1, mixed)
  rows lookup, channels-last kernels (two lerps)     27.7  limit 2000  (2x16x24, radius 3, qb 308: cl<8, 320>); 'SAME': 28.9 (1x9x9)
  rows lookup, generic kernels (four weights)        2.65  limit 20    (1x9x9, radius 4, qb 308 nhwc 0: generic<8>); 'SAME': 2.79
  rows vs tiled                                      27.9  limit 2000  (2x16x24, radius 3, generic<8> against the tiled kernel)
  chain records -> build -> tiled lookup            0.035  limit 1     (2x13x22, C 64, add_grid 1; a share of the summed bound)
  exact in every case (a count of mismatches, 0): every element / cell written, promised pad cells 0, zero map gives 0, far row 0,
  inputs unchanged, store policies + stagger + second launch of the record build, load policies + second launch of the tiled
  lookup, NaN-pattern pads = zero pads, refused calls write nothing
No value is above half its limit.  The two-lerp kernels stay at 28 where their twin reaches 438: the twin rounds fy * (bot - top) and
the sum separately, the compiler contracts the kernels' lerps into one fma each, and the twin's worst element is (1 - fy) v with
1 - fy = 2^-9 (a level-3 position just above the top edge), where that product rounding is the whole error.
A wrong library was run against this file once (built aside, not kept; three mutations that stay in bounds): the tiled lookup without
its pad mask fails 14 of the 18 tiled tests (8x8 with one and two levels has no pad column and passes, as it must) and every
rows-vs-tiled comparison; corr_lookup_fwd_kernel with i and j swapped fails all 10 row-major tests; corr_pool_kernel with its second
row at 2 floor(w / 2) instead of w fails 130x129 and 9x11 and passes 128x128, as it must: 26 of 57 fail.
One thing found while the refusal test was written, by reading the entries: fsraft_corr_pool_pyramid and fsraft_corr_pool_pyramid_same
looked at a level's pointer only when its turn came, so a call with a null level launched the levels before it and then returned 1;
both now check every level before the first launch (fixed before the first run: no output of the old code was recorded).
"""
import ctypes
import itertools

import pytest
import torch

import _corrref as R
import _dcoordsref as D
import _gmaref as G
from _util import Buf, PATTERN, _log_margin

pytestmark = pytest.mark.gpu
FS_ERR_ARG = 1
POLICIES = (0, 2, 16, 18)
QBS = (0, 8, 16, 32, 108, 116, 132, 208, 308)
# fsraft_set_lookup_qb value -> (kernel for nhwc_out = 1, kernel for nhwc_out = 0)
ROUTES = {0: ("cl<8,256>", "generic<32>"), 8: ("cl<8,256>", "generic<8>"), 16: ("cl<16,256>", "generic<16>"),
          32: ("cl<32,256>", "generic<32>"), 108: ("generic<8>", "generic<8>"), 116: ("generic<16>", "generic<16>"),
          132: ("generic<32>", "generic<32>"), 208: ("cl<8,128>", "generic<8>"), 308: ("cl<8,320>", "generic<8>")}


def _route(qb, nhwc):
    """fsraft_set_lookup_qb, pick_qb and dispatch_fwd of csrc/corr_lookup.hip restated."""
    nt = 256
    if qb >= 300:
        nt, qb = 320, qb - 300
    if qb >= 200:
        nt, qb = 128, qb - 200
    cl = qb < 100
    if qb >= 100:
        qb -= 100
    assert qb in (0, 8, 16, 32)
    q = qb if qb else (8 if nhwc else 32)
    if nhwc and cl:
        return f"cl<8,{nt}>" if q == 8 else "cl<32,256>" if q == 32 else "cl<16,256>"
    return f"generic<{q if q in (8, 16) else 32}>"


@pytest.fixture(scope="module")
def L():
    from flow_supervisor_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(scope="module", autouse=True)
def _restore_the_setters_and_leave_no_cached_segments(L):
    """(the cache as tests/test_gma_kernels.py: later modules count allocated bytes)"""
    yield
    lib = L.load()
    lib.fsraft_set_build_split(1)
    lib.fsraft_set_build_kernel(0)
    lib.fsraft_set_lookup_policy(-1)
    lib.fsraft_set_lookup_qb(0)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _no_pattern(t):
    return not bool((t.contiguous().view(torch.int32) == PATTERN).any())


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def _layout(L, H, W, nlev):
    out = (ctypes.c_int * 24)()
    assert L.load().fsraft_vol_layout(H, W, nlev, out) == 0
    lay = R.layout_from_ints(out)
    assert lay == R.vol_layout(H, W, nlev)
    return lay


def _pp(L, bufs, n=None):
    """(pointer to an array of n level pointers -- null beyond the buffers given --, the array to keep alive)."""
    n = n or len(bufs)
    keep = (ctypes.c_void_p * n)(*([b.mid.data_ptr() for b in bufs] + [None] * (n - len(bufs))))
    return ctypes.cast(keep, L._PP), keep


class Tally:
    """The comparisons of one test: every figure is logged (the worst per output, with the variant it occurred in) before
    anything is asserted."""

    def __init__(self, case):
        self.case, self.worst, self.failed = case, {}, []

    def _note(self, name, w, lim, variant, i):
        if w >= self.worst.get(name, (-1.0,))[0]:
            self.worst[name] = (w, lim, variant)
        if not w <= lim:
            self.failed.append((name, variant, w, lim, i))

    def check(self, name, got, ref, S, key, variant=""):
        """|got - ref| in units of UNIT[key] S against LIMITS[key]."""
        w, i = R.need(got.reshape(ref.shape), ref, S * R.UNIT[key])
        self._note(name, w, R.LIMITS[key], variant, i)

    def bounded(self, name, got, ref, bound, variant=""):
        """|got - ref| against an elementwise bound: limit 1."""
        w, i = R.need(got.reshape(ref.shape), ref, bound)
        self._note(name, w, 1.0, variant, i)

    def exact(self, name, ok, variant=""):
        """A bit-for-bit or count comparison: no limit, logged as 0 / 1."""
        self.worst[name] = max(self.worst.get(name, (0.0, 0.0, "")), (0.0 if ok else 1.0, 0.0, variant))
        if not ok:
            self.failed.append((name, variant))

    def done(self):
        for name, (w, lim, variant) in sorted(self.worst.items()):
            _log_margin(f"{name} {self.case}", w, lim, f"worst |got - ref| / (unit S), {variant}" if lim else f"exact, {variant}")
        assert not self.failed, (self.case, self.failed)


# ==================================================================================================================== build
def _promised_pads_are_zero(v, lay):
    """Levels 1 and 2 of a built row: the cells of a written tile row beyond the floor-halved size hold 0 (the build kernels pool out
    of a zero-padded patch and mask).  Level 1: every tile row is written; level 2: a patch of 8 target rows writes two rows."""
    full = R.from_tiled(v, lay, pads=True)
    ok = True
    for l in (1, 2):
        if l >= lay["nlev"]:
            continue
        t = full[l]
        rows = t.shape[1] if l == 1 else min(t.shape[1], 2 * ((lay["H"] + 7) // 8))
        pad = torch.ones(t.shape[1:], dtype=torch.bool)
        pad[:lay["h"][l], :lay["w"][l]] = False
        pad[rows:] = False
        ok = ok and bool((t[:, pad] == 0).all())
    return ok


def _check_tiled(T, what, v, lay, c, key, variant, kind):
    cells = R.cell_mask(lay)
    T.exact(f"{what} every cell written", _no_pattern(v[:, cells]), variant)
    T.exact(f"{what} promised pad cells are 0", _promised_pads_are_zero(v, lay), variant)
    levels = R.from_tiled(v, lay)
    for l, lv in enumerate(levels):
        T.check(f"{what} level {l}", lv, c["ref"][l], c["S"][l], key, variant)
        if kind == "zero":
            T.exact(f"{what} zero map gives 0", bool((lv == 0).all()), variant)
    return levels


@pytest.mark.parametrize("shape,nlev", R.BUILD_SHAPES, ids=_ids)
def test_build_against_float64(L, shape, nlev):
    lib = L.load()
    B, H, W = shape
    N = H * W
    lay = _layout(L, H, W, nlev)
    T = Tally(f"{_ids(shape)} L{nlev}")
    for s, _, C, kind in R.build_cases(False):
        if s != shape:
            continue
        c = R.build_case(shape, nlev, C, kind)
        f1b, f2b = Buf(c["f1"]), Buf(c["f2"])
        for split in (0, 1):
            assert lib.fsraft_set_build_split(split) == 0
            key, variant = ("build.split" if split else "build.exact"), f"C {C} {kind}"
            outs = [Buf(n=B * N * lay["h"][l] * lay["w"][l]) for l in range(nlev)]
            pp, keep = _pp(L, outs, 4)
            rc = lib.fsraft_corr_build(L.ptr(f1b.mid), L.ptr(f2b.mid), pp, nlev, B, C, H, W, None)
            torch.cuda.synchronize()
            assert rc == 0, (variant, rc)
            rows = []
            for l, o in enumerate(outs):
                o.intact()
                g = o.cpu().view(B * N, lay["h"][l], lay["w"][l])
                rows.append(g)
                T.exact(f"rows {key} every element written", _no_pattern(g), variant)
                T.check(f"rows {key} level {l}", g, c["ref"][l], c["S"][l], key, variant)
                if kind == "zero":
                    T.exact(f"rows {key} zero map gives 0", bool((g == 0).all()), variant)
            vol = Buf(n=B * N * lay["P"])
            rc = lib.fsraft_corr_build_tiled(L.ptr(f1b.mid), L.ptr(f2b.mid), L.ptr(vol.mid), nlev, B, C, H, W, None)
            torch.cuda.synchronize()
            assert rc == 0, (variant, rc)
            vol.intact()
            tiled = _check_tiled(T, f"tiled {key}", vol.cpu().view(B * N, lay["P"]), lay, c, key, variant, kind)
            if not split:
                for l in range(nlev):
                    T.check(f"tiled exact vs rows exact level {l}", tiled[l], rows[l].double(), c["S"][l], "build.exact", variant)
        T.exact("inputs unchanged", _same_bits(f1b.cpu(), c["f1"].reshape(-1)) and _same_bits(f2b.cpu(), c["f2"].reshape(-1)), f"C {C} {kind}")
        f1b.intact()
        f2b.intact()
    lib.fsraft_set_build_split(1)
    T.done()


def _records(f):
    """[B, C, H, W] fp32 -> the pixel-major records [B * H * W, C] (an fp32 container), made on the CPU."""
    B, C, H, W = f.shape
    return G.records_encode(f.permute(0, 2, 3, 1).reshape(B * H * W, C))


def _build_rec(L, r1, r2, shape, nlev, C, P):
    B, H, W = shape
    vol = Buf(n=B * H * W * P)
    rc = L.load().fsraft_corr_build_rec(L.ptr(r1.mid), L.ptr(r2.mid), L.ptr(vol.mid), nlev, B, C, H, W, None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    vol.intact()
    return vol


@pytest.mark.parametrize("shape,nlev", R.BUILD_SHAPES, ids=_ids)
def test_record_build_against_float64(L, shape, nlev):
    lib = L.load()
    B, H, W = shape
    lay = _layout(L, H, W, nlev)
    T = Tally(f"{_ids(shape)} L{nlev}")
    for s, _, C, kind in R.build_cases(True):
        if s != shape:
            continue
        c = R.build_case(shape, nlev, C, kind)
        h1, h2 = _records(c["f1"]), _records(c["f2"])
        assert G.records_wellformed(h1) and G.records_wellformed(h2)
        r1, r2 = Buf(h1), Buf(h2)
        variant = f"C {C} {kind}"
        assert lib.fsraft_set_build_kernel(0) == 0
        base = _build_rec(L, r1, r2, shape, nlev, C, lay["P"]).cpu()
        _check_tiled(T, "records", base.view(-1, lay["P"]), lay, c, "build.split", variant, kind)
        if C == 64 and kind == "gauss":
            # store policies plain / sc1 / nt, a stagger of 1, and a second launch of the default: the same bits
            for which in (1 << 16, 2 << 16, 3 << 16, 1 << 8, (3 << 16) | (1 << 8), 0):
                assert lib.fsraft_set_build_kernel(which) == 0
                again = _build_rec(L, r1, r2, shape, nlev, C, lay["P"]).cpu()
                T.exact("records: store policies, stagger, second launch give the same bits", _same_bits(again, base), f"{variant} setter {which:#x}")
            lib.fsraft_set_build_kernel(0)
        T.exact("records inputs unchanged", _same_bits(r1.cpu(), h1.reshape(-1)) and _same_bits(r2.cpu(), h2.reshape(-1)), variant)
        r1.intact()
        r2.intact()
    T.done()


# ==================================================================================================================== pools
def _pool(L, entry, x, sizes):
    rows = x.shape[0]
    bufs = [Buf(x)] + [Buf(n=rows * h * w) for h, w in sizes[1:]]
    pp, keep = _pp(L, bufs)
    rc = entry(pp, len(sizes), rows, x.shape[1], x.shape[2], None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    for b in bufs:
        b.intact()
    return bufs


@pytest.mark.parametrize("shape,nlev", R.POOL_CASES, ids=_ids)
def test_pool_pyramid_against_float64(L, shape, nlev):
    x = R.pool_input(shape)
    ref, S = R.pool_floor(x, nlev), R.pool_floor(x.abs(), nlev)
    bufs = _pool(L, L.load().fsraft_corr_pool_pyramid, x, [lv.shape[1:] for lv in ref])
    T = Tally(f"{_ids(shape)} L{nlev}")
    T.exact("pool level 0 unchanged", _same_bits(bufs[0].cpu(), x.reshape(-1)))
    for l in range(1, nlev):
        g = bufs[l].cpu()
        T.exact("pool every element written", _no_pattern(g), f"level {l}")
        T.check("pool", g, ref[l], S[l], "pool", f"level {l}")
    T.done()


@pytest.mark.parametrize("shape,nlev", R.POOL_SAME_CASES, ids=_ids)
def test_pool_pyramid_same_against_float64(L, shape, nlev):
    x = R.pool_input(shape)
    ref, S = R.pool_same(x, nlev), R.pool_same(x.abs(), nlev)
    bufs = _pool(L, L.load().fsraft_corr_pool_pyramid_same, x, [lv.shape[1:] for lv in ref])
    T = Tally(f"{_ids(shape)} L{nlev}")
    T.exact("pool_same level 0 unchanged", _same_bits(bufs[0].cpu(), x.reshape(-1)))
    for l in range(1, nlev):
        g = bufs[l].cpu()
        T.exact("pool_same every element written", _no_pattern(g), f"level {l}")
        T.check("pool_same", g, ref[l], S[l], "pool_same", f"level {l}")
    if shape[1:] == (8, 8):          # sizes that divide by 2^(L-1): the floor pyramid, within the limit
        fl, fS = R.pool_floor(x, nlev), R.pool_floor(x.abs(), nlev)
        for l in range(1, nlev):
            T.check("pool_same = floor pyramid at 8x8", bufs[l].cpu(), fl[l], fS[l], "pool_same", f"level {l}")
    T.done()


# ==================================================================================================================== tiled lookup
def _lookup_tiled(L, vol, nlev, cbuf, cstr, shape, radius, add_grid, policy=-1):
    B, H, W = shape
    lib = L.load()
    assert lib.fsraft_set_lookup_policy(policy) == 0
    obuf = Buf(n=B * H * W * nlev * (2 * radius + 1) ** 2)
    rc = lib.fsraft_corr_lookup_tiled_fwd(L.ptr(vol.mid), nlev, L.ptr(cbuf.mid), *cstr, L.ptr(obuf.mid), B, H, W, radius, int(add_grid), None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    obuf.intact()
    return obuf.cpu()


@pytest.mark.parametrize("radius", R.RADII)
@pytest.mark.parametrize("shape,nlev", R.TILED_SHAPES, ids=_ids)
def test_tiled_lookup_against_float64(L, shape, nlev, radius):
    B, H, W = shape
    lay = _layout(L, H, W, nlev)
    T = Tally(f"{_ids(shape)} L{nlev} r{radius}")
    full = (shape, nlev) == ((1, 8, 8), 1)            # the smallest shape takes every layout in every combination, the others take turns
    turn = itertools.cycle(R.LAYOUTS)
    for vkind in R.VOL_KINDS:
        levels = R.level_values(shape, nlev, vkind)
        host = R.to_tiled(levels, lay, PATTERN)
        assert _same_bits(host, D.tile_rows(levels, H, W, PATTERN))
        vnan, vzero = Buf(host), Buf(R.to_tiled(levels, lay, 0))
        for ckind in R.COORD_KINDS:
            for add_grid in (False, True):
                c = R.lookup_case(shape, nlev, radius, ckind, add_grid, vkind)
                for layout in (R.LAYOUTS if full else (next(turn),)):
                    variant = f"{vkind} {ckind} grid{int(add_grid)} {layout}"
                    chost = R.pack2(c["given"], layout, PATTERN)
                    cbuf, cstr = Buf(chost), R.strides(B, H, W, layout)[1:]
                    o = _lookup_tiled(L, vnan, nlev, cbuf, cstr, shape, radius, add_grid)
                    T.exact("tiled every element written, all finite", _no_pattern(o) and bool(torch.isfinite(o).all()), variant)
                    g = o.view(c["ref"].shape)
                    T.check("tiled lookup", g, c["ref"], c["S"], "lookup.lerp", variant)
                    if ckind == "mixed":
                        T.exact("tiled far row exactly 0", bool((g[:, 0] == 0).all()), variant)
                    for pol in POLICIES:
                        T.exact("tiled load policies give the same bits", _same_bits(_lookup_tiled(L, vnan, nlev, cbuf, cstr, shape, radius, add_grid, pol), o),
                                f"{variant} policy {pol}")
                    T.exact("tiled two launches give the same bits", _same_bits(_lookup_tiled(L, vnan, nlev, cbuf, cstr, shape, radius, add_grid), o), variant)
                    T.exact("tiled pattern pads = zero pads", _same_bits(_lookup_tiled(L, vzero, nlev, cbuf, cstr, shape, radius, add_grid), o), variant)
                    T.exact("tiled inputs unchanged", _same_bits(cbuf.cpu(), chost) and _same_bits(vnan.cpu(), host.reshape(-1)), variant)
                    cbuf.intact()
        vnan.intact()
        vzero.intact()
    L.load().fsraft_set_lookup_policy(-1)
    T.done()


# ==================================================================================================================== row-major lookup
def test_routes_table_restates_the_dispatch():
    for qb in QBS:
        assert ROUTES[qb] == (_route(qb, 1), _route(qb, 0)), qb
    reached = {k for pair in ROUTES.values() for k in pair}
    assert reached == {"generic<8>", "generic<16>", "generic<32>", "cl<8,128>", "cl<8,256>", "cl<8,320>", "cl<16,256>", "cl<32,256>"}


@pytest.mark.parametrize("radius", R.RADII)
@pytest.mark.parametrize("shape,nlev", R.ROW_SHAPES, ids=_ids)
def test_row_major_lookup_against_float64(L, shape, nlev, radius):
    lib = L.load()
    B, H, W = shape
    lay = _layout(L, H, W, nlev)
    T = Tally(f"{_ids(shape)} r{radius}")
    turn = itertools.cycle(R.LAYOUTS)
    for vkind in R.VOL_KINDS + ("same",):
        levels = R.level_values(shape, nlev, vkind, same=vkind == "same")
        if vkind == "same":
            assert [tuple(lv.shape[1:]) for lv in levels] == [(-(-H // (1 << l)), -(-W // (1 << l))) for l in range(4)]
        lbufs = [Buf(lv) for lv in levels]
        pp, keep = _pp(L, lbufs)
        entry = lib.fsraft_corr_lookup_fwd_same if vkind == "same" else lib.fsraft_corr_lookup_fwd
        vt = None if vkind == "same" else Buf(R.to_tiled(levels, lay, PATTERN))
        for ckind in R.COORD_KINDS:
            c = R.lookup_case(shape, nlev, radius, ckind, False, vkind)
            layout = next(turn)
            chost = R.pack2(c["given"], layout, PATTERN)
            cbuf, cstr = Buf(chost), R.strides(B, H, W, layout)[1:]
            tiled = None if vt is None else _lookup_tiled(L, vt, nlev, cbuf, cstr, shape, radius, False).view(c["ref"].shape)
            for qb in QBS:
                assert lib.fsraft_set_lookup_qb(qb) == 0
                for nhwc in (1, 0):
                    kern = ROUTES[qb][1 - nhwc]
                    key = "lookup.lerp" if kern.startswith("cl") else "lookup.weights"
                    variant = f"{vkind} {ckind} {layout} qb {qb} nhwc {nhwc}: {kern}"
                    obuf = Buf(n=c["ref"].numel())
                    rc = entry(pp, 4, L.ptr(cbuf.mid), *cstr, L.ptr(obuf.mid), nhwc, B, H, W, radius, None)
                    torch.cuda.synchronize()
                    assert rc == 0, (variant, rc)
                    obuf.intact()
                    o = obuf.cpu()
                    T.exact("rows every element written, all finite", _no_pattern(o) and bool(torch.isfinite(o).all()), variant)
                    g = o.view(c["ref"].shape) if nhwc else o.view(B, -1, H, W).permute(0, 2, 3, 1)
                    name = "rows lookup_same" if vkind == "same" else "rows lookup"
                    T.check(f"{name} {key}", g, c["ref"], c["S"], key, variant)
                    if ckind == "mixed":
                        T.exact("rows far row exactly 0", bool((g[:, 0] == 0).all()), variant)
                    if tiled is not None:
                        T.check("rows vs tiled", g, tiled.double(), c["S"], "lookup.lerp", variant)
            T.exact("rows inputs unchanged", _same_bits(cbuf.cpu(), chost) and all(_same_bits(b.cpu(), lv.reshape(-1)) for b, lv in zip(lbufs, levels)),
                    f"{vkind} {ckind}")
            cbuf.intact()
        for b in lbufs:
            b.intact()
    lib.fsraft_set_lookup_qb(0)
    T.done()


# ==================================================================================================================== chain
def test_record_build_then_tiled_lookup(L):
    """records -> fsraft_corr_build_rec -> fsraft_corr_lookup_tiled_fwd against lookup(build(.)).  Bound: the lookup's limit on its own
    scale plus the build's limit carried through the lookup -- the bilinear weights applied to the build's error scale."""
    shape, nlev, C = R.CHAIN
    B, H, W = shape
    radius = 4
    lay = _layout(L, H, W, nlev)
    c = R.build_case(shape, nlev, C, "gauss")
    r1, r2 = Buf(_records(c["f1"])), Buf(_records(c["f2"]))
    L.load().fsraft_set_build_kernel(0)
    vol = _build_rec(L, r1, r2, shape, nlev, C, lay["P"])
    T = Tally(f"{_ids(shape)} C {C} r{radius}")
    for add_grid in (False, True):
        given = D.coords_values(B, H, W, "mixed")
        pos = given + D.grid(B, H, W) if add_grid else given
        ref, S = R.lookup(c["ref"], pos, radius)
        carried, _ = R.lookup(c["S"], pos, radius)                       # (the scale pyramid is non-negative: this is sum w S_build)
        bound = R.LIMITS["lookup.lerp"] * R.U24 * S + R.LIMITS["build.split"] * R.G16 * carried
        cbuf = Buf(given)
        o = _lookup_tiled(L, vol, nlev, cbuf, R.strides(B, H, W, "planar")[1:], shape, radius, add_grid)
        T.exact("chain every element written, all finite", _no_pattern(o) and bool(torch.isfinite(o).all()), f"grid{int(add_grid)}")
        T.bounded("chain build_rec -> tiled lookup", o.view(ref.shape), ref, bound, f"grid{int(add_grid)}")
        T.exact("chain far row exactly 0", bool((o.view(ref.shape)[:, 0] == 0).all()), f"grid{int(add_grid)}")
    T.done()


# ==================================================================================================================== refusals
def test_refused_calls_write_nothing(L):
    lib = L.load()
    B, H, W, C, r = 1, 8, 8, 32, 4
    N = H * W
    lay = _layout(L, H, W, 4)
    null = ctypes.c_void_p(None)
    f = Buf(torch.ones(B * N * C))
    outs = [Buf(n=N * (H >> l) * (W >> l)) for l in range(4)]
    pp, keep = _pp(L, outs)
    pp_hole, keep_hole = _pp(L, outs)
    keep_hole[2] = None
    vol, vol_off = Buf(n=N * lay["P"]), Buf(n=N * lay["P"], offset=1)
    cbuf, cs = Buf(torch.zeros(2 * N)), (2 * N, N, 1)
    obuf = Buf(n=N * 4 * 81)
    fp, vp, cp, op = L.ptr(f.mid), L.ptr(vol.mid), L.ptr(cbuf.mid), L.ptr(obuf.mid)
    refused = dict(
        build_c_odd=lib.fsraft_corr_build(fp, fp, pp, 4, B, 3, H, W, None),
        build_c_zero=lib.fsraft_corr_build(fp, fp, pp, 4, B, 0, H, W, None),
        build_null_level=lib.fsraft_corr_build(fp, fp, pp_hole, 4, B, C, H, W, None),
        build_4_levels_on_4x4=lib.fsraft_corr_build(fp, fp, pp, 4, B, C, 4, 4, None),
        tiled_c_odd=lib.fsraft_corr_build_tiled(fp, fp, vp, 4, B, 3, H, W, None),
        tiled_c_zero=lib.fsraft_corr_build_tiled(fp, fp, vp, 4, B, 0, H, W, None),
        tiled_off_alignment=lib.fsraft_corr_build_tiled(fp, fp, L.ptr(vol_off.mid), 4, B, C, H, W, None),
        tiled_4_levels_on_4x4=lib.fsraft_corr_build_tiled(fp, fp, vp, 4, B, C, 4, 4, None),
        rec_c_48=lib.fsraft_corr_build_rec(fp, fp, vp, 4, B, 48, H, W, None),
        rec_c_zero=lib.fsraft_corr_build_rec(fp, fp, vp, 4, B, 0, H, W, None),
        rec_off_alignment=lib.fsraft_corr_build_rec(fp, fp, L.ptr(vol_off.mid), 4, B, C, H, W, None),
        rec_4_levels_on_4x4=lib.fsraft_corr_build_rec(fp, fp, vp, 4, B, C, 4, 4, None),
        pool_null_level=lib.fsraft_corr_pool_pyramid(pp_hole, 4, N, H, W, None),
        pool_same_null_level=lib.fsraft_corr_pool_pyramid_same(pp_hole, 4, N, H, W, None),
        lookup_tiled_radius_2=lib.fsraft_corr_lookup_tiled_fwd(vp, 4, cp, *cs, op, B, H, W, 2, 0, None),
        lookup_tiled_radius_5=lib.fsraft_corr_lookup_tiled_fwd(vp, 4, cp, *cs, op, B, H, W, 5, 0, None),
        lookup_tiled_off_alignment=lib.fsraft_corr_lookup_tiled_fwd(L.ptr(vol_off.mid), 4, cp, *cs, op, B, H, W, r, 0, None),
        lookup_tiled_4_levels_on_4x4=lib.fsraft_corr_lookup_tiled_fwd(vp, 4, cp, *cs, op, B, 4, 4, r, 0, None),
        lookup_tiled_null=lib.fsraft_corr_lookup_tiled_fwd(null, 4, cp, *cs, op, B, H, W, r, 0, None),
    )
    for name, entry in (("lookup", lib.fsraft_corr_lookup_fwd), ("lookup_same", lib.fsraft_corr_lookup_fwd_same)):
        refused[name + "_radius_2"] = entry(pp, 4, cp, *cs, op, 1, B, H, W, 2, None)
        refused[name + "_radius_5"] = entry(pp, 4, cp, *cs, op, 0, B, H, W, 5, None)
        refused[name + "_3_levels"] = entry(pp, 3, cp, *cs, op, 1, B, H, W, r, None)
        refused[name + "_null_level"] = entry(pp_hole, 4, cp, *cs, op, 1, B, H, W, r, None)
        refused[name + "_null_levels"] = entry(ctypes.cast(null, L._PP), 4, cp, *cs, op, 1, B, H, W, r, None)
    refused["lookup_4_levels_on_4x4"] = lib.fsraft_corr_lookup_fwd(pp, 4, cp, *cs, op, 1, B, 4, 4, r, None)
    torch.cuda.synchronize()
    assert all(rc == FS_ERR_ARG for rc in refused.values()), {k: v for k, v in refused.items() if v != FS_ERR_ARG}
    for b in outs + [vol, vol_off, obuf]:
        b.untouched()
    f.intact()
    cbuf.intact()
