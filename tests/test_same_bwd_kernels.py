"""The backward of the TensorFlow 'SAME' pyramid, called through its C entry points, every element against the float64 restatements of
tests/_samebwdref.py: fsraft_corr_unpool_same_bwd (corr_unpool_same_bwd_kernel / _vec_kernel, csrc/corr_build.hip), fsraft_corr_lookup_
bwd_same (the kernels of csrc/corr_lookup.hip on ceil-sized levels) and fsraft_corr_lookup_dcoords_same (lookup_dcoords_kernel of csrc/
corr_dcoords.hip on ceil-sized levels).  The test owns every buffer (_util.Buf: guard rows and unwritten outputs hold a NaN pattern)
and compares the inputs bit for bit afterwards.  Needs an MI355X: -m gpu.

fsraft_corr_unpool_same_bwd: _samebwdref.UNPOOL_CASES -- _corrref.POOL_SAME_CASES (3x9x11 scalar, 2x8x8 vector, 2x1x1); 5x6x12 with 4
levels (py = 1 at k = 4 and 8, px = 2 at k = 8, where the four x of one vector lie in two windows; the vector route) and the same with
level 0 four bytes off its alignment (the scalar route); 1, 2, 3, 4 and 8 levels at 2x9x11 -- and _samebwdref.UNPOOL_BIG, the second
trips of the grid-stride loops past their cap of 8192 blocks of 256: 21200x9x11 (2 098 800 cells, scalar route, 8.4 MB) and 19100x22x20
(2 101 000 float4, vector route, 34 MB of level 0 and 45 MB in all).  In place; a second launch on fresh copies gives identical bits;
levels >= 1 unchanged; the row after the last of level 0 and the guard rows intact; one level writes nothing.  2x8x8, where the two
pyramids agree, as the first two rows of a 64-row volume (the floor entry takes whole planes of queries) against fsraft_corr_unpool_bwd
within the sum of the two limits.  Refused calls (a null level, 0 and 9 levels, 0 rows) return 1 and write nothing.
fsraft_corr_lookup_bwd_same: _samebwdref.LOOKUP_SHAPES (1x9x11, 2x6x12, 3x5x9) with four ceil-sized levels, radius 3 / 4, every fsraft_
set_lookup_qb value of test_corr_kernels.QBS with nhwc_in 1 / 0, coordinates from _dcoordsref.mixed_positions (out of range and far
ones among them), two lookups in a row onto gaussian levels.
fsraft_corr_lookup_dcoords_same: the same shapes, 1 .. 4 levels, radius 3 / 4, nhwc_in 1 / 0, a second launch: identical bits.

Limits: _samebwdref.LIMITS, from the fp32 twins on the CPU (tests/test_samebwdref.py), not from the kernels.  profiles/
corr_same_bwd_margins.txt lists every comparison (FSRAFT_PARITY_LOG).  Worst values measured on MI355X, in units of 2^-24 S:
  unpool_same_bwd, vector kernel                      3.05  limit 20   (19100x22x20: the second trip; the twin's own figure, 3.052)
  unpool_same_bwd, scalar kernel                      2.56  limit 20   (21200x9x11: the second trip)
  unpool_same_bwd against fsraft_corr_unpool_bwd     0.067  limit 1    (2x8x8 in 64x8x8; a share of the sum of the two limits)
  lookup_bwd_same, channels-last kernels              2.71  limit 20   (2x6x12, radius 3, qb 308: cl<8, 320>, level 1)
  lookup_bwd_same, generic kernels                    2.37  limit 20   (2x6x12, radius 3, qb 308 nhwc 0: generic<8>, level 1)
  dcoords_same                                        1.87  limit 8    (2x6x12, radius 3, 2 levels, nhwc 0: the pairwise twin's figure)
  exact in every case (a count of mismatches, 0): second launches, levels >= 1, the row after the last and the guard rows, one level
  writes nothing, the far row's gradient, inputs unchanged, refused calls write nothing
No value is above a quarter of its limit.  On the parent commit every test here fails: the three entry points do not exist.
A wrong library was run against the un-pool tests once (built aside, not kept; a mutation that stays inside the buffers): the vector
kernel letting the four x of a vector share one window from k = 4 on fails 5x6x12 (vector route) and 19100x22x20, where px = 2 at k = 8
puts a window edge inside a vector -- and rightly passes the other twelve: 2x8x8 (px = 0: the windows are aligned with the vectors) and
every scalar-route case.
"""
import ctypes

import pytest
import torch

import _corrbwdref as B
import _corrref as R
import _samebwdref as M
import test_corr_kernels as F
from _util import Buf, PATTERN

pytestmark = pytest.mark.gpu
FS_ERR_ARG = 1
_ids = F._ids


@pytest.fixture(scope="module")
def L():
    from flow_supervisor_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(scope="module", autouse=True)
def _restore_the_setter_and_leave_no_cached_segments(L):
    yield
    L.load().fsraft_set_lookup_qb(0)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


class Tally(F.Tally):
    def check(self, name, got, ref, S, key, variant=""):
        """|got - ref| in units of 2^-24 S against _samebwdref.LIMITS[key]."""
        w, i = M.need(got.reshape(ref.shape), ref, S * M.U24)
        self._note(name, w, M.LIMITS[key], variant, i)


# ==================================================================================================================== unpool_same_bwd
def _unpool(L, lv, offset=0, entry="fsraft_corr_unpool_same_bwd", dims=None):
    """One launch on fresh copies: (level-0 buffer with one more row of the NaN pattern behind the last, the other levels' buffers)."""
    rows, H, W = lv[0].shape
    b0 = Buf(n=(rows + 1) * H * W, offset=offset)
    b0.mid[:rows * H * W].copy_(lv[0].reshape(-1))
    bufs = [b0] + [Buf(t) for t in lv[1:]]
    pp, keep = F._pp(L, bufs)
    rc = getattr(L.load(), entry)(pp, len(lv), *(dims or (rows, H, W)), None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    return bufs


def _level0(b, lv0):
    """(the rows of level 0, whether the row behind them still holds the pattern)"""
    n = lv0.numel()
    whole = b.cpu()
    return whole[:n], bool((whole[n:].view(torch.int32) == PATTERN).all())


@pytest.mark.parametrize("shape,nlev,offset", M.UNPOOL_CASES + M.UNPOOL_BIG, ids=_ids)
def test_unpool_same_bwd_against_float64(L, shape, nlev, offset):
    c = M.unpool_case(shape, nlev)
    lv = c["levels"]
    T = Tally(f"{_ids(shape)} L{nlev} off{offset}")
    runs = []
    for _ in range(2):
        bufs = _unpool(L, lv, offset)
        for b in bufs:
            b.intact()
        got, after = _level0(bufs[0], lv[0])
        T.exact("unpool_same_bwd the row after the last is intact", after)
        T.exact("unpool_same_bwd levels 1 and up unchanged", all(F._same_bits(b.cpu(), t.reshape(-1)) for b, t in zip(bufs[1:], lv[1:])))
        T.check("unpool_same_bwd level 0", got, c["ref"], c["S"], "unpool_same")
        runs.append(got)
        del bufs
    T.exact("unpool_same_bwd second launch: identical bits", F._same_bits(runs[0], runs[1]))
    if nlev == 1:
        T.exact("unpool_same_bwd with one level writes nothing", F._same_bits(runs[0], lv[0].reshape(-1)))
    T.done()


def test_unpool_same_bwd_agrees_with_the_floor_kernel_at_8x8(L):
    """The 2x8x8 case as rows 0 and 1 of a 64-row volume of 8x8 planes (one sample of the floor entry), both kernels on copies of it."""
    shape, nlev = (2, 8, 8), 4
    lv = [t.clone() for t in M.unpool_values((64, 8, 8), nlev)]
    for t, s in zip(lv, M.unpool_case(shape, nlev)["levels"]):
        t[:2] = s
    same = _level0(_unpool(L, lv)[0], lv[0])[0]
    floor = _level0(_unpool(L, lv, entry="fsraft_corr_unpool_bwd", dims=(1, 8, 8))[0], lv[0])[0]
    ref, S = M.unpool_same_bwd(lv), M.unpool_same_bwd(lv, absolute=True)
    T = Tally("2x8x8 in 64x8x8 L4")
    T.check("unpool_same_bwd level 0", same, ref, S, "unpool_same")
    T.bounded("unpool_same_bwd against fsraft_corr_unpool_bwd", same, floor.double().reshape(ref.shape),
              (M.LIMITS["unpool_same"] + B.LIMITS["unpool"]) * M.U24 * S)
    T.bounded("fsraft_corr_unpool_bwd against the 'SAME' restatement", floor, ref, B.LIMITS["unpool"] * M.U24 * S)
    T.done()


def test_unpool_same_bwd_refused_calls_write_nothing(L):
    lib = L.load()
    rows, H, W = 3, 9, 11
    outs = [Buf(n=rows * h * w) for h, w in M.same_sizes(H, W, 9)]
    pp, keep = F._pp(L, outs)
    pp_hole, keep_hole = F._pp(L, outs)
    keep_hole[2] = None
    refused = dict(null_level=lib.fsraft_corr_unpool_same_bwd(pp_hole, 4, rows, H, W, None),
                   null_level_0=lib.fsraft_corr_unpool_same_bwd(F._pp(L, [], 4)[0], 4, rows, H, W, None),
                   null_array=lib.fsraft_corr_unpool_same_bwd(ctypes.cast(ctypes.c_void_p(None), L._PP), 4, rows, H, W, None),
                   levels_0=lib.fsraft_corr_unpool_same_bwd(pp, 0, rows, H, W, None),
                   levels_9=lib.fsraft_corr_unpool_same_bwd(pp, 9, rows, H, W, None),
                   rows_0=lib.fsraft_corr_unpool_same_bwd(pp, 4, 0, H, W, None),
                   height_0=lib.fsraft_corr_unpool_same_bwd(pp, 4, rows, 0, W, None))
    torch.cuda.synchronize()
    assert all(rc == FS_ERR_ARG for rc in refused.values()), {k: v for k, v in refused.items() if v != FS_ERR_ARG}
    for b in outs:
        b.untouched()


# ==================================================================================================================== lookup_bwd_same
@pytest.mark.parametrize("radius", M.RADII)
@pytest.mark.parametrize("shape", M.LOOKUP_SHAPES, ids=_ids)
def test_lookup_bwd_same_against_float64(L, shape, radius):
    lib = L.load()
    Bn, H, W = shape
    c = M.lookup_bwd_case(shape, radius)
    T = Tally(f"{_ids(shape)} r{radius}")
    chost = [R.pack2(gv, R.LAYOUTS[(t + radius) % 3], PATTERN) for t, gv in enumerate(c["given"])]
    cbufs = [Buf(h) for h in chost]
    cstr = [R.strides(Bn, H, W, R.LAYOUTS[(t + radius) % 3])[1:] for t in range(2)]
    dhost = {1: c["dout"], 0: [d.permute(0, 3, 1, 2).contiguous() for d in c["dout"]]}
    dbufs = {k: [Buf(d) for d in v] for k, v in dhost.items()}
    for qb in F.QBS:
        assert lib.fsraft_set_lookup_qb(qb) == 0
        for nhwc in (1, 0):
            kern = F.ROUTES[qb][1 - nhwc]
            key = "lookup_bwd_same.cl" if kern.startswith("cl") else "lookup_bwd.four"
            variant = f"qb {qb} nhwc {nhwc}: {kern}"
            lbufs = [Buf(t) for t in c["old"]]
            pp, keep = F._pp(L, lbufs)
            for t in range(2):
                rc = lib.fsraft_corr_lookup_bwd_same(pp, 4, L.ptr(cbufs[t].mid), *cstr[t], L.ptr(dbufs[nhwc][t].mid), nhwc, Bn, H, W, radius, None)
                torch.cuda.synchronize()
                assert rc == 0, (variant, rc)
            for l, b in enumerate(lbufs):
                b.intact()
                T.check(f"lookup_bwd_same {key}", b.cpu(), c["ref"][l], c["S"][l], key, f"{variant} level {l}")
    ok = all(F._same_bits(b.cpu(), h) for b, h in zip(cbufs, chost))
    ok = ok and all(F._same_bits(b.cpu(), h.reshape(-1)) for k in (0, 1) for b, h in zip(dbufs[k], dhost[k]))
    T.exact("lookup_bwd_same inputs unchanged", ok)
    for b in cbufs + dbufs[0] + dbufs[1]:
        b.intact()
    lib.fsraft_set_lookup_qb(0)
    T.done()


def test_lookup_same_refused_calls_write_nothing(L):
    """Floor-sized buffers would be too small for ceil-sized levels, so the refusals are checked on ceil-sized ones."""
    lib = L.load()
    Bn, H, W, r = 1, 9, 11, 4
    N = H * W
    outs = [Buf(n=N * h * w) for h, w in M.same_sizes(H, W, 4)]
    pp, keep = F._pp(L, outs)
    pp_hole, keep_hole = F._pp(L, outs)
    keep_hole[2] = None
    cbuf, cs = Buf(torch.zeros(2 * N)), (2 * N, N, 1)
    dout, dc = Buf(torch.ones(N * 4 * 81)), Buf(n=2 * N)
    cp, dp, null = L.ptr(cbuf.mid), L.ptr(dout.mid), ctypes.c_void_p(None)
    refused = dict(three_levels=lib.fsraft_corr_lookup_bwd_same(pp, 3, cp, *cs, dp, 1, Bn, H, W, r, None),
                   null_level=lib.fsraft_corr_lookup_bwd_same(pp_hole, 4, cp, *cs, dp, 1, Bn, H, W, r, None),
                   radius_2=lib.fsraft_corr_lookup_bwd_same(pp, 4, cp, *cs, dp, 0, Bn, H, W, 2, None),
                   null_dout=lib.fsraft_corr_lookup_bwd_same(pp, 4, cp, *cs, null, 1, Bn, H, W, r, None),
                   dc_radius_2=lib.fsraft_corr_lookup_dcoords_same(pp, 4, cp, *cs, dp, 1, L.ptr(dc.mid), *cs, Bn, H, W, 2, None),
                   dc_5_levels=lib.fsraft_corr_lookup_dcoords_same(pp, 5, cp, *cs, dp, 1, L.ptr(dc.mid), *cs, Bn, H, W, r, None),
                   dc_null_level=lib.fsraft_corr_lookup_dcoords_same(pp_hole, 4, cp, *cs, dp, 1, L.ptr(dc.mid), *cs, Bn, H, W, r, None),
                   dc_null_out=lib.fsraft_corr_lookup_dcoords_same(pp, 4, cp, *cs, dp, 1, null, *cs, Bn, H, W, r, None))
    torch.cuda.synchronize()
    assert all(rc == FS_ERR_ARG for rc in refused.values()), {k: v for k, v in refused.items() if v != FS_ERR_ARG}
    for b in outs + [dc]:
        b.untouched()
    cbuf.intact()
    dout.intact()


# ==================================================================================================================== dcoords_same
@pytest.mark.parametrize("radius", M.RADII)
@pytest.mark.parametrize("shape", M.LOOKUP_SHAPES, ids=_ids)
def test_lookup_dcoords_same_against_float64(L, shape, radius):
    lib = L.load()
    Bn, H, W = shape
    N = H * W
    T = Tally(f"{_ids(shape)} r{radius}")
    for nlev in (1, 2, 3, 4):
        c = M.dcoords_case(shape, nlev, radius)
        layout = R.LAYOUTS[(nlev + radius) % 3]
        chost = R.pack2(c["pos"], layout, PATTERN)
        cbuf, cstr = Buf(chost), R.strides(Bn, H, W, layout)[1:]
        lbufs = [Buf(t) for t in c["levels"]]
        pp, keep = F._pp(L, lbufs)
        dhost = {1: c["dout"], 0: c["dout"].permute(0, 3, 1, 2).contiguous()}
        for nhwc in (1, 0):
            dbuf = Buf(dhost[nhwc])
            outs = []
            for _ in range(2):
                obuf = Buf(n=Bn * 2 * N)
                rc = lib.fsraft_corr_lookup_dcoords_same(pp, nlev, L.ptr(cbuf.mid), *cstr, L.ptr(dbuf.mid), nhwc, L.ptr(obuf.mid), 2 * N, N, 1,
                                                         Bn, H, W, radius, None)
                torch.cuda.synchronize()
                assert rc == 0, (nlev, nhwc, rc)
                obuf.written()
                outs.append(obuf.cpu())
            variant = f"L{nlev} nhwc {nhwc}"
            T.check("dcoords_same", outs[0], c["ref"], c["S"].expand_as(c["ref"]), "dcoords_same", variant)
            T.exact("dcoords_same the far row gets exactly 0", bool((outs[0].view(Bn, 2, H, W)[:, :, 0] == 0).all()), variant)
            T.exact("dcoords_same second launch: identical bits", F._same_bits(outs[0], outs[1]), variant)
            dbuf.intact()
            T.exact("dcoords_same dout unchanged", F._same_bits(dbuf.cpu(), dhost[nhwc].reshape(-1)), variant)
        ok = F._same_bits(cbuf.cpu(), chost) and all(F._same_bits(b.cpu(), t.reshape(-1)) for b, t in zip(lbufs, c["levels"]))
        T.exact("dcoords_same coordinates and levels unchanged", ok, f"L{nlev}")
        for b in [cbuf] + lbufs:
            b.intact()
    T.done()
