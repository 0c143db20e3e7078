"""The backward kernels of the correlation path, called through their C entry points, every element against the float64 restatements
of tests/_corrbwdref.py at the edges of their launch geometry: corr_dvol_kernel / corr_dvol_sep_kernel and the query list between
them (fsraft_corr_dvol_build), corr_f2cat_kernel, corr_f2cat_rec_kernel, corr_dfmap2_kernel / _v4_kernel (csrc/corr_tiled.hip),
corr_unpool_bwd_kernel / _vec_kernel (csrc/corr_build.hip), corr_lookup_bwd_kernel / _cl_kernel (csrc/corr_lookup.hip).  The forward
half is tests/test_corr_kernels.py.  The test owns every buffer (_util.Buf: guard rows and unwritten outputs hold a NaN pattern) and
compares the inputs bit for bit afterwards.  Needs an MI355X: -m gpu.

Gradient volume (_corrbwdref.DVOL_SHAPES: _corrref.TILED_SHAPES and 1x9x17, whose level 0 ends off a record; radius 3 and 4; fsraft_
set_dvol_box 0 and 1; fp32 rows and records; 1, 2, 6, 7 and 16 lookups, each with a coordinate layout of its own; add_grid 0 / 1).
Coordinate families whose route the CPU fixes (tests/test_corrbwdref.py asserts the shares): near (nobody on the list, origins that
repeat), alt (two origins one cell apart at level 0 only), limit (origins side - WIN apart and one more, in x and in y, the smaller
one 0 and 3 mod 4 and negative), jump (everybody on the list), edge (_dcoordsref.mixed_positions; the first row at +-1e6 in every
lookup, the last query far in one lookup only).  dout gaussian, zero, a one on a level's first / last channel.  A 17th lookup with
accumulate = 1 on top of 16, fp32 and records.  fsraft_set_dvol_policy 0 / 1 / 2 and a second launch: identical bits.  Exactly: pad
cells and the tail are zero bits, the row after the last and the guard rows are intact, qlist[0] and the set qlist[1 ..] are the
predicted ones.  Two shapes whose first run is longer than the 8192-float segment (the CLIP instantiations), as a chunk of 67 queries
from a first query that is no multiple of 32: 1x64x129 (level 0 alone) and 1x92x92 (all four levels in one run).
f2cat / f2cat_rec / dfmap2: the shapes above with C in 1, 3, 4, 32 (H W % 4 != 0: the scalar staging of f2cat_rec; C % 4 != 0 and a
d2 / d2cat 4 bytes off its alignment: the scalar dfmap2); 96x128 = 12288 pixels, the largest plane f2cat_rec takes; the second trips
of the three grid-stride loops; f2cat_rec against fsraft_corr_f2cat + fsraft_to_records.  d2cat holds the NaN pattern in its pads.
fsraft_corr_unpool_bwd: _corrbwdref.UNPOOL_CASES (1 to 4 levels, scalar / vector / scalar by alignment, both second trips), in place.
fsraft_corr_lookup_bwd: _corrref.ROW_SHAPES, radius 3 / 4, every fsraft_set_lookup_qb value of test_corr_kernels.QBS with nhwc_in 1 /
0 (ROUTES asserted against a restatement of dispatch_bwd), two lookups in a row onto gaussian levels.
k-tile lists (fsraft_corr_bwd_ktiles; fsraft_set_ktile_exact 0 / 1 / 2; the families above at radius 3 / 4): 127, 128 and 129 queries
(1x1x127, 1x8x16, 1x3x43) with the level counts each admits, B > 1, chunks off the 32- and 128-query grids with a ragged last tile,
1x64x129 whole (258 blocks of 32 queries: the second trip of corr_ktiles_tn_kernel; 44 cell tiles: two bitmap words; coordinates only).
Exactly against the integer restatement: counts, ascending lists, the slots beyond each count, tn_bits, wmask; independently of it:
every record that is non-zero in the float64 gradient volume is listed and masked, marked(2) within marked(1) within marked(0).
Masked rows: the gradient volume written under that wmask (2 x 32x48 whole, two chunks of it, a clipped chunk of 64x129) against the unmasked run.
One chain at _corrref.CHAIN (2x13x22, C = 64) through ops.corr_build_bwd_tiled(ktiles=...), bounded by the sum of the stages' bounds.
Refused calls return 1 and write nothing.

Not covered, and why.  The wmask path of corr_dvol_sep_kernel above 64 mask words is unreachable: ops.corr_bwd_ktiles returns None
there and fsraft_corr_bwd_ktiles refuses (P > 262144 floats).  NaN coordinates: the kernels map them to an empty window where the
restatement would give NaN (as the forward tests).

Limits: _corrbwdref.LIMITS, from the fp32 twins on the CPU (tests/test_corrbwdref.py), not from the kernels.  profiles/
corr_bwd_kernel_margins.txt lists every comparison (FSRAFT_PARITY_LOG).  Worst values measured on MI355X, in units of 2^-24 S:
  gradient volume, corr_dvol_kernel (fp32 rows)       2.83  limit 20   (2x16x24, radius 3, edge, 6 lookups, level 0)
  gradient volume, corr_dvol_sep_kernel (fp32 rows)   3.70  limit 20   (2x16x24, radius 3, alt, 7 lookups, level 1: the twin's own figure)
  16 + 1 lookups, accumulate = 1 (fp32 rows)          3.60  limit 20   (2x16x24, radius 4, near, level 1)
  records, either kernel                             0.241  limit 1    (2x32x48; a share of record_bound: the split is most of it)
  records, 16 + 1 lookups                            0.240  limit 1    (2x16x24, radius 4, near, level 1)
  f2cat                                               3.69  limit 20   (2 x 256 x 64x129, level 2)
  f2cat_rec / f2cat + to_records / one vs the other  0.246 / 0.241 / 0.233  limit 1  (2 x 256 x 64x129; shares of record_bound)
  dfmap2                                              2.93  limit 20   (8 x 64x129, C 256: the vector kernel's second trip)
  unpool_bwd                                          2.74  limit 20   (1x64x68: the vector kernel's second trip)
  lookup_bwd, channels-last kernels                   2.61  limit 20   (2x16x24, radius 4, qb 308: cl<8, 320>, level 1)
  lookup_bwd, generic kernels                         2.63  limit 20   (2x16x24, radius 4, qb 308 nhwc 0: generic<8>, level 1)
  chain dF1 / dF2                                    0.019 / 0.030  limit 1  (2x13x22, C 64; shares of the summed bound)
  exact in every case (a count of mismatches, 0): floats written, pads and tail zero, the row after the last and the guard rows, the
  query list, store policies + second launch, zero dout, k-tile counts / lists / untouched slots / tn_bits / wmask, coverage of the
  non-zero float64 records, marked(2) within marked(1) within marked(0), records inside / outside the mask, inputs unchanged,
  refused calls write nothing
No value is above a fifth of its limit; the kernels sit where their twins do (the twins round every operation, and so, it seems, do
the kernels: 3.70 against the twin's 3.698).
One thing the first run found, in the restatement and not in a kernel: the bound of a record row after an accumulating launch charged
both splits to the final value; the first split is of what the FIRST launch wrote, which the 17th lookup may largely cancel (2x16x24,
radius 4, near, level 1: 1.32 of that bound; 1x8x8 with 3 levels: 1.15).  record_bound(earlier=...) now charges each launch's split to
that launch's value, and tests/test_corrbwdref.py::test_record_bound_counts_the_split_of_every_launch reproduces both figures with an
fp32 twin of the record chain.
A wrong library was run against this file once (built aside, not kept; three mutations that stay inside the buffers): the x weights of
corr_dvol_sep_kernel taken from the wrong neighbour ((1 - fx) and fx exchanged) fails all 24 gradient-volume tests, the 8 masked-row
tests and the chain; the k-tile rectangle's high edge one cell short fails the k-tile tests of 1x3x43 (1 and 2 levels), 2x32x48 and the
chunk of 1x64x129 -- and rightly passes 1x1x127, 1x8x16, 2x16x24, 3x5x9, the chunks of 2x16x24 and 1x64x129 whole, where the union over
a tile of 128 queries marks the same records with either rectangle (tests/test_corrbwdref.py shows the same on the CPU); dfmap2
without its existence check at level 1 (the index clamped to the row) fails 3x5x9, 1x9x9, 1x9x17, both second trips and the chain, and
rightly passes every shape with even H and W, where every level-1 cell exists: 41 of 82 fail; the unpool, lookup-backward, refusal
and route tests do not run the mutated code and pass.
"""
import ctypes

import pytest
import torch

import _corrbwdref as B
import _corrref as R
import _gmaref as G
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
def _restore_the_setters_and_leave_no_cached_segments(L):
    """(the cache as tests/test_gma_kernels.py: later modules count allocated bytes)"""
    yield
    lib = L.load()
    lib.fsraft_set_dvol_box(1)
    lib.fsraft_set_dvol_policy(0)
    lib.fsraft_set_ktile_exact(0)
    lib.fsraft_set_lookup_qb(0)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


class Tally(F.Tally):
    def check(self, name, got, ref, S, key, variant=""):
        """|got - ref| in units of 2^-24 S against _corrbwdref.LIMITS[key]."""
        w, i = B.need(got.reshape(ref.shape), ref, S * B.U24)
        self._note(name, w, B.LIMITS[key], variant, i)


def _pattern_only(t):
    return bool((t.contiguous().view(torch.int32) == PATTERN).all())


# ==================================================================================================================== gradient volume
class Lookups:
    """A case's lookups on the device: the coordinates of lookup t in layout t % 3 (planar, planar with a gap, interleaved), dout."""

    def __init__(self, c, shape):
        Bn, H, W = shape
        self.chost = [R.pack2(gv, R.LAYOUTS[t % 3], PATTERN) for t, gv in enumerate(c["given"])]
        self.cb = [Buf(h) for h in self.chost]
        self.strides = [R.strides(Bn, H, W, R.LAYOUTS[t % 3])[1:] for t in range(len(self.cb))]
        self.dhost = c["dout"]
        self.db = [Buf(d) for d in self.dhost]

    def args(self, L, t0, t1):
        dpp, k1 = F._pp(L, self.db[t0:t1])
        cpp, k2 = F._pp(L, self.cb[t0:t1])
        st = (ctypes.c_int64 * (3 * (t1 - t0)))(*[v for s in self.strides[t0:t1] for v in s])
        return (dpp, cpp, st, t1 - t0), (k1, k2)

    def unchanged(self):
        for b in self.cb + self.db:
            b.intact()
        return all(F._same_bits(b.cpu(), h.reshape(-1)) for b, h in zip(self.cb + self.db, self.chost + self.dhost))


def _dvol(L, lk, t0, t1, shape, nlev, radius, add_grid, rows, P, records, box, q0=0, nq=0, onto=None, policy=0, wmask=None):
    """One call of fsraft_corr_dvol_build for lookups [t0, t1) -> (the output buffer: rows + 1 rows of P floats, the list buffer)."""
    lib = L.load()
    Bn, H, W = shape
    assert lib.fsraft_set_dvol_box(box) == 0 and lib.fsraft_set_dvol_policy(policy) == 0
    out = onto if onto is not None else Buf(n=(rows + 1) * P)
    ql = Buf(n=1 + rows)
    a, keep = lk.args(L, t0, t1)
    rc = lib.fsraft_corr_dvol_build(*a, L.ptr(out.mid), nlev, Bn, H, W, radius, int(onto is not None), records, add_grid, q0, nq,
                                    L.ptr(ql.mid), L.ptr(wmask.mid) if wmask is not None else None, None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    out.intact()
    ql.intact()
    return out, ql


def _check_rows(T, name, out, rows, lay, ref, S, records, unfit, variant, earlier=None):
    """Every cell against float64 (records decoded); exact: all floats written, pads and tail zero bits, the next row untouched.
    unfit: bool [rows], the queries the row kernel handled (None: all of them)."""
    P, cells = lay["P"], R.cell_mask(lay)
    flat = out.cpu()
    vol = flat[:rows * P].view(rows, P)
    T.exact(f"{name} the row after the last is untouched", _pattern_only(flat[rows * P:]), variant)
    T.exact(f"{name} every float written", F._no_pattern(vol), variant)
    if records:
        raw = vol.contiguous().view(torch.int16).view(rows, P // 32, 2, 32)
        pad = (~cells).view(P // 32, 32)
        T.exact(f"{name} pads and tail are zero bits", bool((raw[:, :, 0][:, pad] == 0).all()) and bool((raw[:, :, 1][:, pad] == 0).all()), variant)
        dec = G.records_decode(vol)
    else:
        T.exact(f"{name} pads and tail are zero bits", bool((vol[:, ~cells].contiguous().view(torch.int32) == 0).all()), variant)
        dec = vol
    groups = [("dvol.row", torch.ones(rows, dtype=torch.bool))] if unfit is None else [("dvol.sep", ~unfit), ("dvol.row", unfit)]
    for l, lv in enumerate(R.from_tiled(dec, lay)):
        for key, sel in groups:
            if not bool(sel.any()):
                continue
            g, r, s = lv[sel], ref[l][sel], S[l][sel]
            if records:
                T.bounded(f"{name} records {key}", g, r, B.record_bound(key, r, s, [earlier[l][sel]] if earlier else ()), f"{variant} level {l}")
            else:
                T.check(f"{name} {key}", g, r, s, key, f"{variant} level {l}")
    return vol


def _check_list(T, ql, unfit, box, variant):
    q = ql.cpu().view(torch.int32)
    if not box:
        T.exact("box 0 leaves the list alone", _pattern_only(q), variant)
        return
    want = unfit.nonzero().view(-1).to(torch.int32)
    n = int(q[0])
    ok = n == want.numel() and torch.equal(torch.sort(q[1:1 + max(n, 0)]).values, want) and _pattern_only(q[1 + max(n, 0):])
    T.exact("qlist[0] and the set qlist[1 ..] are the predicted ones", ok, f"{variant}: {n} listed, {want.numel()} predicted")


def _dvol_runs(L, T, shape, nlev, radius, runs, q0=0, nq=0, extras=True):
    Bn, H, W = shape
    lay = F._layout(L, H, W, nlev)
    P, rows = lay["P"], nq or Bn * H * W
    for case in runs:
        family, n, add_grid, dkind, extra = case[3], case[4], case[5], case[6], case[9]
        c = B.dvol_case(*case)
        lk = Lookups(c, shape)
        for box in (0, 1):
            for records in (0, 1):
                variant = f"{family} n{n} grid{add_grid} {dkind} box{box} rec{records}"
                out, ql = _dvol(L, lk, 0, n, shape, nlev, radius, add_grid, rows, P, records, box, q0, nq)
                vol = _check_rows(T, "dvol", out, rows, lay, c["ref"], c["S"], records, c["unfit"] if box else None, variant)
                _check_list(T, ql, c["unfit"], box, variant)
                if dkind == "zero":
                    T.exact("zero dout gives zero bits", bool((vol.contiguous().view(torch.int32) == 0).all()), variant)
                if extra:       # the 17th lookup on top: accumulate = 1 takes corr_dvol_kernel for every query, records decoded and re-split
                    out, ql2 = _dvol(L, lk, n, n + 1, shape, nlev, radius, add_grid, rows, P, records, box, q0, nq, onto=out)
                    _check_rows(T, "dvol 16 + 1", out, rows, lay, c["ref17"], c["S17"], records, None, variant, earlier=c["ref"])
                    T.exact("an accumulating call leaves the list alone", _pattern_only(ql2.cpu()), variant)
                if extras and family == "edge" and n == 6:
                    for pol in (1, 2, 0):       # sc1 / nt stores, then a second launch of the plain ones
                        again, _ = _dvol(L, lk, 0, n, shape, nlev, radius, add_grid, rows, P, records, box, q0, nq, policy=pol)
                        T.exact("store policies and a second launch give the same bits", F._same_bits(again.cpu()[:rows * P], vol.reshape(-1)),
                                f"{variant} policy {pol}")
        T.exact("inputs unchanged", lk.unchanged(), f"{family} n{n}")
    L.load().fsraft_set_dvol_box(1)
    L.load().fsraft_set_dvol_policy(0)


@pytest.mark.parametrize("radius", R.RADII)
@pytest.mark.parametrize("shape,nlev", B.DVOL_SHAPES, ids=_ids)
def test_gradient_volume_against_float64(L, shape, nlev, radius):
    T = Tally(f"{_ids(shape)} L{nlev} r{radius}")
    _dvol_runs(L, T, shape, nlev, radius, [c for c in B.dvol_cases() if c[:3] == (shape, nlev, radius) and c[8] == 0])
    T.done()


@pytest.mark.parametrize("radius", R.RADII)
@pytest.mark.parametrize("shape,nlev,q0,nq", B.CLIP_SHAPES, ids=_ids)
def test_gradient_volume_runs_longer_than_the_segment(L, shape, nlev, q0, nq, radius):
    """corr_dvol_kernel<., ., CLIP = true>: box 0 sends every query of the chunk there, box 1 the listed ones."""
    T = Tally(f"{_ids(shape)} L{nlev} r{radius} chunk {q0}+{nq}")
    _dvol_runs(L, T, shape, nlev, radius, [c for c in B.dvol_cases() if c[:3] == (shape, nlev, radius) and c[8] == nq], q0, nq, extras=False)
    T.done()


def test_gradient_volume_refused_calls_write_nothing(L):
    lib = L.load()
    shape, nlev, r = (2, 8, 8), 4, 4
    Bn, H, W = shape
    lay = F._layout(L, H, W, nlev)
    rows, P = Bn * H * W, lay["P"]
    c = B.dvol_case(shape, nlev, r, "near", 16, 0, "gauss", 0, 0, True)
    lk = Lookups(c, shape)
    out, off, ql = Buf(n=rows * P), Buf(n=rows * P, offset=1), Buf(n=1 + rows)
    wm = Buf(torch.zeros(Bn * ((H * W + 31) // 32) * ((P // 32 + 31) // 32)))
    (dpp, cpp, st, _), keep = lk.args(L, 0, 17)
    hole_d, kd = F._pp(L, lk.db[:4])
    hole_c, kc = F._pp(L, lk.cb[:4])
    kd[2] = None
    kc[1] = None
    op, qp, wp, null = L.ptr(out.mid), L.ptr(ql.mid), L.ptr(wm.mid), ctypes.c_void_p(None)
    lib.fsraft_set_dvol_box(1)

    def call(n=4, d=dpp, co=cpp, dv=op, radius=r, acc=0, rec=1, q0=0, nq=0, qlist=qp, wmask=null):
        return lib.fsraft_corr_dvol_build(d, co, st, n, dv, nlev, Bn, H, W, radius, acc, rec, 0, q0, nq, qlist, wmask, None)
    refused = dict(n_0=call(n=0), n_17=call(n=17), radius_2=call(radius=2), radius_5=call(radius=5), null_dout=call(d=hole_d),
                   null_coords=call(co=hole_c), misaligned_dvol=call(dv=L.ptr(off.mid)), past_the_end=call(q0=rows - 10, nq=11),
                   negative_q0=call(q0=-1, nq=4), wmask_accumulate=call(wmask=wp, acc=1), wmask_no_records=call(wmask=wp, rec=0),
                   wmask_no_qlist=call(wmask=wp, qlist=null), wmask_two_images=call(wmask=wp, q0=H * W - 10, nq=20))
    lib.fsraft_set_dvol_box(0)
    refused["wmask_box_0"] = call(wmask=wp)
    lib.fsraft_set_dvol_box(1)
    torch.cuda.synchronize()
    assert all(rc == FS_ERR_ARG for rc in refused.values()), {k: v for k, v in refused.items() if v != FS_ERR_ARG}
    for b in (out, off, ql):
        b.untouched()
    assert lk.unchanged()


# ==================================================================================================================== k-tile lists
def _i32(buf):
    return buf.cpu().view(torch.int32)


def _words(t):
    """int32 words as unsigned int64."""
    return t.long() & 0xFFFFFFFF


def _ktiles(L, lk, n, shape, nlev, radius, add_grid, lay, q0=0, nq=0, exact=0):
    """One call of fsraft_corr_bwd_ktiles (strides a few slots wider than the minimum) -> dict of int32 tensors per list set."""
    lib = L.load()
    Bn, H, W = shape
    sets, HW = (1, nq) if nq else (Bn, H * W)
    P = lay["P"]
    nrec, mt, ktq, ntile = P // 32, -(-P // 256), -(-HW // 32), -(-HW // 128)
    mw, nw, nts, tns = -(-mt // 32), -(-nrec // 32), nrec + 3, ktq + 5
    assert lib.fsraft_set_ktile_exact(exact) == 0
    b = dict(nt_list=Buf(n=sets * ntile * nts), nt_count=Buf(n=sets * ntile), tn_bits=Buf(n=sets * ktq * mw), tn_list=Buf(n=sets * mt * tns),
             tn_count=Buf(n=sets * mt), wmask=Buf(n=sets * ktq * nw))
    (_, cpp, st, _), keep = lk.args(L, 0, n)
    rc = lib.fsraft_corr_bwd_ktiles(cpp, st, n, nlev, Bn, H, W, radius, add_grid, q0, nq, L.ptr(b["nt_list"].mid), L.ptr(b["nt_count"].mid), nts,
                                    L.ptr(b["tn_bits"].mid), L.ptr(b["tn_list"].mid), L.ptr(b["tn_count"].mid), tns, L.ptr(b["wmask"].mid), None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    for v in b.values():
        v.intact()
    g = dict(nt_list=_i32(b["nt_list"]).view(sets, ntile, nts), nt_count=_i32(b["nt_count"]).view(sets, ntile),
             tn_bits=_i32(b["tn_bits"]).view(sets, ktq, mw), tn_list=_i32(b["tn_list"]).view(sets, mt, tns),
             tn_count=_i32(b["tn_count"]).view(sets, mt), wmask=_i32(b["wmask"]).view(sets, ktq, nw), wbuf=b["wmask"], sets=sets, HW=HW)
    return g


def _lists_as_sets(g, s):
    """(records per 128-query tile, blocks per cell tile) of list set s as Python sets; None where a count is out of range."""
    nt = [set(g["nt_list"][s, t, :int(c)].tolist()) for t, c in enumerate(g["nt_count"][s])]
    tn = [set(g["tn_list"][s, m, :int(c)].tolist()) for m, c in enumerate(g["tn_count"][s])]
    return nt, tn


def _check_ktiles(T, g, pos, lay, radius, exact, variant, nz=None):
    """Against the restatement, exactly: counts, ascending lists, untouched slots, the bit matrix, the record mask.  nz (bool
    [sets, HW, nrec], optional): the records whose float64 gradient is non-zero -- each must be listed, whatever the restatement says."""
    for s in range(g["sets"]):
        rec, tile = B.ktile_marks([p[s * g["HW"]:(s + 1) * g["HW"]] for p in pos], lay, radius, exact)
        k = B.ktile_lists(rec, tile)
        ok_nt = all(int(g["nt_count"][s, t]) == len(want) and g["nt_list"][s, t, :len(want)].tolist() == want and
                    _pattern_only(g["nt_list"][s, t, len(want):]) for t, want in enumerate(k["nt"]))
        ok_tn = all(int(g["tn_count"][s, m]) == len(want) and g["tn_list"][s, m, :len(want)].tolist() == want and
                    _pattern_only(g["tn_list"][s, m, len(want):]) for m, want in enumerate(k["tn"]))
        T.exact("NT counts, ascending lists, slots beyond the count untouched", ok_nt, f"{variant} set {s}")
        T.exact("TN counts, ascending lists, slots beyond the count untouched", ok_tn, f"{variant} set {s}")
        T.exact("tn_bits equals the restated matrix", torch.equal(_words(g["tn_bits"][s]), k["tn_bits"]), f"{variant} set {s}")
        T.exact("wmask equals the restatement", torch.equal(_words(g["wmask"][s]), k["wmask"]), f"{variant} set {s}")
        if nz is not None:
            nt, tn = _lists_as_sets(g, s)
            q, r = nz[s].nonzero(as_tuple=True)
            listed = all(b in nt[a // 128] and (a // 32) in tn[b // 8] for a, b in zip(q.tolist(), r.tolist()))
            wm = _words(g["wmask"][s])
            masked = bool(((wm[q // 32, r // 32] >> (r % 32)) & 1).all())
            T.exact("every record with a non-zero float64 gradient is listed, and in the mask", listed and masked, f"{variant} set {s}")


def _nonzero_records(c, lay, sets, HW):
    vol = R.to_tiled([x.float() for x in c["ref"]], lay)
    return (vol.view(sets, HW, lay["P"] // 32, 32) != 0).any(3)


def _ktile_runs(L, T, shape, nlev, q0=0, nq=0, runs=B.KT_RUNS, radii=R.RADII, ref=True):
    Bn, H, W = shape
    lay = F._layout(L, H, W, nlev)
    for radius in radii:
        for family, n, add_grid in runs:
            c = B.dvol_case(shape, nlev, radius, family, n, add_grid, "gauss", q0, nq) if ref else None
            if c is None:        # coordinates only (a shape whose float64 gradient volume would be too large)
                pos = B.positions(shape, radius, family, n)
                c = dict(given=pos, dout=[], pos=[B._flat(p) for p in pos])
            lk = Lookups(c, shape)
            got = []
            for exact in (0, 1, 2):
                g = _ktiles(L, lk, n, shape, nlev, radius, add_grid, lay, q0, nq, exact)
                variant = f"r{radius} {family} n{n} grid{add_grid} exact {exact}"
                _check_ktiles(T, g, c["pos"][:n], lay, radius, exact, variant, _nonzero_records(c, lay, g["sets"], g["HW"]) if ref else None)
                got.append(g)
            for a, b in zip(got, got[1:]):       # marked(2) within marked(1) within marked(0)
                sub = all(x <= y for s in range(a["sets"]) for x, y in zip(_lists_as_sets(b, s)[0], _lists_as_sets(a, s)[0]))
                sub = sub and bool((_words(b["tn_bits"]) & ~_words(a["tn_bits"]) == 0).all()) and bool((_words(b["wmask"]) & ~_words(a["wmask"]) == 0).all())
                T.exact("exact marks are a subset of the rectangle's", sub, f"r{radius} {family}")
            T.exact("k-tile inputs unchanged", lk.unchanged(), f"r{radius} {family}")
    L.load().fsraft_set_ktile_exact(0)


@pytest.mark.parametrize("shape,nlev", B.KT_SHAPES, ids=_ids)
def test_ktile_lists_against_the_restatement(L, shape, nlev):
    T = Tally(f"{_ids(shape)} L{nlev}")
    _ktile_runs(L, T, shape, nlev)
    T.done()


@pytest.mark.parametrize("shape,nlev,q0,nq", B.KT_CHUNKS, ids=_ids)
def test_ktile_lists_of_a_chunk(L, shape, nlev, q0, nq):
    T = Tally(f"{_ids(shape)} L{nlev} chunk {q0}+{nq}")
    _ktile_runs(L, T, shape, nlev, q0, nq, runs=[("edge", 6, 0), ("near", 16, 1)] if shape[1] < 64 else [("edge", 2, 0), ("near", 7, 1)])
    T.done()


def test_ktile_lists_second_trip_of_the_block_loop(L):
    """1x64x129 whole: 258 blocks of 32 queries (corr_ktiles_tn_kernel walks 256 per trip), 44 cell tiles (two bitmap words).
    Coordinates only."""
    shape, nlev = B.KT_BIG
    T = Tally(f"{_ids(shape)} L{nlev}")
    _ktile_runs(L, T, shape, nlev, runs=[("edge", 2, 0)], ref=False)
    T.done()


def test_ktile_lists_refused_calls_write_nothing(L):
    lib = L.load()
    shape, nlev, r = (2, 8, 8), 4, 4
    Bn, H, W = shape
    lay = F._layout(L, H, W, nlev)
    c = B.dvol_case(shape, nlev, r, "near", 16, 0, "gauss", 0, 0, True)
    lk = Lookups(c, shape)
    (_, cpp, st, _), keep = lk.args(L, 0, 17)
    hole, kh = F._pp(L, lk.cb[:4])
    kh[3] = None
    outs = [Buf(n=4096) for _ in range(6)]
    nt_list, nt_count, tn_bits, tn_list, tn_count, wm = (L.ptr(b.mid) for b in outs)
    nrec, ktq = lay["P"] // 32, 2

    def call(n=4, co=cpp, shp=(Bn, H, W), radius=r, q0=0, nq=0, nts=nrec, tns=ktq, ntl=nt_list):
        return lib.fsraft_corr_bwd_ktiles(co, st, n, nlev, *shp, radius, 0, q0, nq, ntl, nt_count, nts, tn_bits, tn_list, tn_count, tns, wm, None)
    refused = dict(rows_beyond_the_bitmaps=call(shp=(1, 512, 512), tns=8192, nts=11000), nt_stride_short=call(nts=nrec - 1),
                   tn_stride_short=call(tns=ktq - 1), chunk_across_two_images=call(q0=H * W - 10, nq=20), n_0=call(n=0), n_17=call(n=17),
                   radius_2=call(radius=2), null_coords=call(co=hole), null_list=call(ntl=ctypes.c_void_p(None)), past_the_end=call(q0=120, nq=9))
    assert lib.fsraft_set_ktile_exact(5) == FS_ERR_ARG and lib.fsraft_set_ktile_exact(-1) == FS_ERR_ARG
    torch.cuda.synchronize()
    assert all(rc == FS_ERR_ARG for rc in refused.values()), {k: v for k, v in refused.items() if v != FS_ERR_ARG}
    for b in outs:
        b.untouched()
    assert R.vol_layout(512, 512, 4)["P"] > 262144


# ==================================================================================================================== masked rows
@pytest.mark.parametrize("radius", R.RADII)
@pytest.mark.parametrize("shape,nlev,q0,nq", B.WMASK_SETS, ids=_ids)
def test_gradient_volume_written_under_the_record_mask(L, shape, nlev, q0, nq, radius):
    """wmask from fsraft_corr_bwd_ktiles handed to fsraft_corr_dvol_build (records, box 1).  The rows of corr_dvol_sep_kernel hold
    the unmasked run's bits inside the mask and the pattern outside; the queries on the list go to corr_dvol_kernel, which writes
    whole rows (ops.corr_dvol_build says so too): those equal the unmasked run throughout.  The mask covers every record whose
    float64 gradient is non-zero.  The unmasked run of the same chunk is itself held to the float64 bound."""
    Bn, H, W = shape
    lay = F._layout(L, H, W, nlev)
    P, rows, nrec = lay["P"], nq or Bn * H * W, lay["P"] // 32
    T = Tally(f"{_ids(shape)} L{nlev} r{radius} {q0}+{nq}")
    for family, n, add_grid, dkind in B.WMASK_RUNS:
        c = B.dvol_case(shape, nlev, radius, family, n, add_grid, dkind, q0, nq)
        lk = Lookups(c, shape)
        variant = f"{family} n{n} grid{add_grid}"
        g = _ktiles(L, lk, n, shape, nlev, radius, add_grid, lay, q0, nq)
        plain, _ = _dvol(L, lk, 0, n, shape, nlev, radius, add_grid, rows, P, 1, 1, q0, nq)
        base = _check_rows(T, "dvol (chunk)", plain, rows, lay, c["ref"], c["S"], 1, c["unfit"], variant)
        out, ql = _dvol(L, lk, 0, n, shape, nlev, radius, add_grid, rows, P, 1, 1, q0, nq, wmask=g["wbuf"])
        _check_list(T, ql, c["unfit"], 1, variant)
        vol = out.cpu()[:rows * P].view(rows, nrec, 32).view(torch.int32)
        want = base.reshape(rows, nrec, 32).view(torch.int32)
        q = torch.arange(rows)
        wm = _words(g["wmask"]).view(-1, g["wmask"].shape[2])[(q // g["HW"]) * g["wmask"].shape[1] + (q % g["HW"]) // 32]        # [rows, nw]
        bits = ((wm[:, torch.arange(nrec) // 32] >> (torch.arange(nrec) % 32).view(1, -1)) & 1).bool()                       # [rows, nrec]
        same = (vol == want).all(2)
        patt = (vol == PATTERN).all(2)
        fit = ~c["unfit"].view(-1, 1)
        T.exact("records inside the mask equal the unmasked run", bool(same[bits & fit].all()), variant)
        T.exact("records outside the mask still hold the pattern", bool(patt[~bits & fit].all()), variant)
        if family == "local":       # (tests/test_corrbwdref.py: the mask leaves records out, and both kernels get rows)
            T.exact("the mask leaves records of the fast kernel's rows out", bool((~bits & fit).any()) and bool(fit.any()) and bool((~fit).any()), variant)
        T.exact("listed queries' rows equal the unmasked run throughout", bool(same[~fit.expand_as(same)].all()), variant)
        nz = _nonzero_records(c, lay, 1, rows)[0]
        T.exact("the mask covers every record whose float64 gradient is non-zero", not bool((nz & ~bits).any()), variant)
        T.exact("masked run inputs unchanged", lk.unchanged(), variant)
    T.done()


# ==================================================================================================================== f2cat, dfmap2
def _f2cat(L, f2b, shape, C, nlev, P, rec, out=None):
    Bn, H, W = shape
    out = out or Buf(n=Bn * C * P)
    entry = L.load().fsraft_corr_f2cat_rec if rec else L.load().fsraft_corr_f2cat
    rc = entry(L.ptr(f2b.mid), L.ptr(out.mid), nlev, Bn, C, H, W, None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    out.written()
    return out


def _check_f2cat(L, T, shape, nlev, C):
    Bn, H, W = shape
    lay = F._layout(L, H, W, nlev)
    P, cells = lay["P"], R.cell_mask(lay)
    f2 = B.f2_values(shape, C)
    ref, S = B.f2cat(f2, nlev), B.f2cat(f2.abs(), nlev)
    f2b = Buf(f2)
    variant = f"C {C}"
    plain = _f2cat(L, f2b, shape, C, nlev, P, False)
    vol = plain.cpu().view(Bn * C, P)
    T.exact("f2cat pads and tail are zero bits", bool((vol[:, ~cells].contiguous().view(torch.int32) == 0).all()), variant)
    for l, lv in enumerate(R.from_tiled(vol, lay)):
        T.check("f2cat", lv, ref[l], S[l], "f2cat.block", f"{variant} level {l}")
    if H * W <= 12288:
        rv = _f2cat(L, f2b, shape, C, nlev, P, True).cpu().view(Bn * C, P)
        raw = rv.contiguous().view(torch.int16).view(Bn * C, P // 32, 2, 32)
        pad = (~cells).view(P // 32, 32)
        T.exact("f2cat_rec pads and tail are zero records", bool((raw[:, :, 0][:, pad] == 0).all()) and bool((raw[:, :, 1][:, pad] == 0).all()), variant)
        two = Buf(n=Bn * C * P)
        rc = L.load().fsraft_to_records(L.ptr(plain.mid), P, L.ptr(two.mid), 0, Bn * C, P, None)
        torch.cuda.synchronize()
        assert rc == 0, rc
        two.written()
        dec, dec2 = R.from_tiled(G.records_decode(rv), lay), R.from_tiled(G.records_decode(two.cpu().view(Bn * C, P)), lay)
        for l in range(nlev):
            b1, b2 = B.record_bound("f2cat.rec", ref[l], S[l]), B.record_bound("f2cat.block", ref[l], S[l])
            T.bounded("f2cat_rec records", dec[l], ref[l], b1, f"{variant} level {l}")
            T.bounded("f2cat + to_records", dec2[l], ref[l], b2, f"{variant} level {l}")
            T.bounded("f2cat_rec vs f2cat + to_records", dec[l], dec2[l], b1 + b2, f"{variant} level {l}")
    T.exact("f2cat input unchanged", F._same_bits(f2b.cpu(), f2.reshape(-1)), variant)
    f2b.intact()


def _check_dfmap2(L, T, shape, nlev, C, offsets=((0, 0),)):
    Bn, H, W = shape
    lay = F._layout(L, H, W, nlev)
    v = B.d2cat_values(shape, C, lay)
    ref, S = B.dfmap2(v, lay), B.dfmap2(v, lay, absolute=True)
    for oi, oo in offsets:
        src, out = Buf(v, offset=oi), Buf(n=Bn * H * W * C, offset=oo)
        rc = L.load().fsraft_corr_dfmap2(L.ptr(src.mid), L.ptr(out.mid), nlev, Bn, C, H, W, None)
        torch.cuda.synchronize()
        assert rc == 0, rc
        out.written()
        T.check("dfmap2", out.cpu(), ref, S, "dfmap2", f"C {C} d2cat +{oi} d2 +{oo} floats")
        T.exact("dfmap2 input unchanged", F._same_bits(src.cpu(), v.reshape(-1)), f"C {C}")
        src.intact()


@pytest.mark.parametrize("shape,nlev", B.DVOL_SHAPES + [(B.F2_MAXPLANE[0], 4)], ids=_ids)
def test_f2cat_and_dfmap2_against_float64(L, shape, nlev):
    T = Tally(f"{_ids(shape)} L{nlev}")
    for C in ((B.F2_MAXPLANE[1],) if shape == B.F2_MAXPLANE[0] else B.F2_C):
        _check_f2cat(L, T, shape, nlev, C)
        # C = 4: aligned (the vector kernel), then d2cat and d2 each 4 bytes off (the scalar kernel although C % 4 == 0)
        _check_dfmap2(L, T, shape, nlev, C, ((0, 0), (1, 0), (0, 1)) if C == 4 else ((0, 0),))
    T.done()


def test_f2cat_and_dfmap2_second_trips_of_the_grid_stride_loops(L):
    T = Tally("second trips")
    _check_f2cat(L, T, B.F2_BIG[0], 4, B.F2_BIG[1])
    for shape, C in B.DF_BIG:
        _check_dfmap2(L, T, shape, 4, C)
    T.done()


def test_f2cat_rec_refused_calls_write_nothing(L):
    lib = L.load()
    lay = R.vol_layout(1, 12289, 1)
    big, out = Buf(torch.ones(12289)), Buf(n=lay["P"])
    f, f_off = Buf(torch.ones(64)), Buf(torch.ones(64), offset=1)
    o, o_off = Buf(n=128), Buf(n=128, offset=1)
    refused = dict(plane_12289=lib.fsraft_corr_f2cat_rec(L.ptr(big.mid), L.ptr(out.mid), 1, 1, 1, 1, 12289, None),
                   misaligned_fmap2=lib.fsraft_corr_f2cat_rec(L.ptr(f_off.mid), L.ptr(o.mid), 4, 1, 1, 8, 8, None),
                   misaligned_f2r=lib.fsraft_corr_f2cat_rec(L.ptr(f.mid), L.ptr(o_off.mid), 4, 1, 1, 8, 8, None),
                   f2cat_5_levels=lib.fsraft_corr_f2cat(L.ptr(f.mid), L.ptr(o.mid), 5, 1, 1, 8, 8, None),
                   dfmap2_c_0=lib.fsraft_corr_dfmap2(L.ptr(f.mid), L.ptr(o.mid), 4, 1, 0, 8, 8, None))
    torch.cuda.synchronize()
    assert all(rc == FS_ERR_ARG for rc in refused.values()), {k: v for k, v in refused.items() if v != FS_ERR_ARG}
    for b in (out, o, o_off):
        b.untouched()


# ==================================================================================================================== chain
def test_masked_record_gradient_volume_then_listed_gemms_then_dfmap2(L):
    """dout -> fsraft_corr_bwd_ktiles -> the record gradient volume under its mask, into a buffer of NaN -> fsraft_corr_f2cat_rec,
    fsraft_gemm_rec_nt_list / _tn_list -> fsraft_corr_dfmap2, through ops.corr_build_bwd_tiled(ktiles=...), at _corrref.CHAIN against
    _corrbwdref.volume_bwd of the float64 gradient volume.  Bound: the stages' bounds, each carried through the stages after it (all
    of them linear with the other operand fixed): the gradient volume's record bound and f2cat_rec's through the contraction, the
    record GEMMs' own (hi hi + hi lo + lo hi in fp32: _corrref.LIMITS['build.split'] in units of 2^-16 of the sum of |products|, the
    figure of the record build, which is the same arithmetic), dfmap2's on the sum of its |terms|."""
    from flow_supervisor_amd import ops
    shape, nlev, C = R.CHAIN
    Bn, H, W = shape
    radius = B.CHAIN_CASE[2]
    c = B.dvol_case(*B.CHAIN_CASE)
    bc = R.build_case(shape, nlev, C, "gauss")
    f1, f2 = bc["f1"], bc["f2"]
    lay = ops.VolLayout.get(H, W, nlev)
    assert lay.P == R.vol_layout(H, W, nlev)["P"]
    given = [g.cuda().contiguous() for g in c["given"]]
    douts = [d.cuda().contiguous() for d in c["dout"]]
    kt = ops.corr_bwd_ktiles(given, lay, Bn, radius, True)
    assert kt is not None
    poison = torch.full((Bn * H * W, lay.P), float("nan"), device="cuda")
    dv = ops.corr_dvol_build(douts, given, lay, Bn, radius, records=True, is_flow=True, wmask=kt.wmask, out=poison)
    # (at 13x22 every mask is full -- a row has 17 records --: records that are read but not written are the masked-row tests' matter)
    d1, d2 = ops.corr_build_bwd_tiled(f1.cuda(), f2.cuda(), dv, lay, records=True, ktiles=kt)
    torch.cuda.synchronize()
    d1, d2 = d1.cpu().reshape(Bn, C, H * W), d2.cpu().reshape(Bn, C, H * W).permute(0, 2, 1)
    # float64 chain and the bound
    f2l, f2S = B.f2cat(f2, nlev), B.f2cat(f2.abs(), nlev)
    ref1, ref2 = B.volume_bwd(f1, f2l, c["ref"])
    af1, af2l, adv = f1.abs(), [t.abs() for t in f2l], [t.abs() for t in c["ref"]]
    S1, S2 = B.volume_bwd(af1, af2l, adv)
    un = c["unfit"].view(-1, 1, 1)
    e_dv = [torch.where(un, B.record_bound("dvol.row", c["ref"][l], c["S"][l]), B.record_bound("dvol.sep", c["ref"][l], c["S"][l])) for l in range(nlev)]
    e_f2 = [B.record_bound("f2cat.rec", f2l[l], f2S[l]) for l in range(nlev)]
    a1, a2 = B.volume_bwd(af1, af2l, e_dv)
    b1, _ = B.volume_bwd(af1, e_f2, adv)
    gemm = R.LIMITS["build.split"] * R.G16
    T = Tally(f"{_ids(shape)} C {C} r{radius}")
    T.exact("chain all finite (no unwritten record was read)", bool(torch.isfinite(d1).all()) and bool(torch.isfinite(d2).all()))
    T.bounded("chain dF1", d1, ref1, a1 + b1 + gemm * S1)
    T.bounded("chain dF2", d2, ref2, a2 + gemm * S2 + B.LIMITS["dfmap2"] * B.U24 * S2)
    T.done()


# ==================================================================================================================== unpool_bwd
@pytest.mark.parametrize("shape,nlev", B.UNPOOL_CASES, ids=_ids)
def test_unpool_bwd_against_float64(L, shape, nlev):
    Bn, H, W = shape
    lv = B.unpool_values(shape, nlev)
    ref, S = B.unpool_bwd(lv), B.unpool_bwd(lv, absolute=True)
    bufs = [Buf(lv[0], offset=1 if shape == (1, 8, 12) else 0)] + [Buf(t) for t in lv[1:]]
    pp, keep = F._pp(L, bufs)
    rc = L.load().fsraft_corr_unpool_bwd(pp, nlev, Bn, H, W, None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    T = Tally(f"{_ids(shape)} L{nlev}")
    for b in bufs:
        b.intact()
    T.exact("unpool_bwd levels 1 and up unchanged", all(F._same_bits(b.cpu(), t.reshape(-1)) for b, t in zip(bufs[1:], lv[1:])))
    T.check("unpool_bwd level 0", bufs[0].cpu(), ref, S, "unpool")
    if nlev == 1:
        T.exact("unpool_bwd with one level writes nothing", F._same_bits(bufs[0].cpu(), lv[0].reshape(-1)))
    T.done()


# ==================================================================================================================== lookup_bwd
def _route_bwd(qb, nhwc):
    """fsraft_set_lookup_qb, pick_qb and dispatch_bwd of csrc/corr_lookup.hip restated."""
    nt = 256
    if qb >= 300:
        nt, qb = 320, qb - 300
    if qb >= 200:
        nt, qb = 128, qb - 200
    cl = qb < 100
    qb = qb - 100 if qb >= 100 else qb
    assert qb in (0, 8, 16, 32)
    q = qb or (8 if nhwc else 32)
    if nhwc and cl:
        if q == 8:
            return f"cl<8,{nt}>"
        return "cl<32,256>" if q == 32 else "cl<16,256>"
    return "generic<8>" if q == 8 else "generic<16>" if q == 16 else "generic<32>"


def test_backward_routes_restate_the_dispatch():
    for qb in F.QBS:
        assert F.ROUTES[qb] == (_route_bwd(qb, 1), _route_bwd(qb, 0)), qb


@pytest.mark.parametrize("radius", R.RADII)
@pytest.mark.parametrize("shape,nlev", R.ROW_SHAPES, ids=_ids)
def test_lookup_bwd_against_float64(L, shape, nlev, radius):
    lib = L.load()
    Bn, H, W = shape
    c = B.lookup_bwd_case(shape, radius)
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
            key = "lookup_bwd.cl" if kern.startswith("cl") else "lookup_bwd.four"
            variant = f"qb {qb} nhwc {nhwc}: {kern}"
            lbufs = [Buf(t) for t in c["old"]]
            pp, keep = F._pp(L, lbufs)
            for t in range(2):
                rc = lib.fsraft_corr_lookup_bwd(pp, 4, L.ptr(cbufs[t].mid), *cstr[t], L.ptr(dbufs[nhwc][t].mid), nhwc, Bn, H, W, radius, None)
                torch.cuda.synchronize()
                assert rc == 0, (variant, rc)
            for l, b in enumerate(lbufs):
                b.intact()
                T.check(f"lookup_bwd {key}", b.cpu(), c["ref"][l], c["S"][l], key, f"{variant} level {l}")
    ok = all(F._same_bits(b.cpu(), h) for b, h in zip(cbufs, chost))
    ok = ok and all(F._same_bits(b.cpu(), h.reshape(-1)) for k in (0, 1) for b, h in zip(dbufs[k], dhost[k]))
    T.exact("lookup_bwd inputs unchanged", ok)
    for b in cbufs + dbufs[0] + dbufs[1]:
        b.intact()
    lib.fsraft_set_lookup_qb(0)
    T.done()


def test_lookup_bwd_and_unpool_refused_calls_write_nothing(L):
    lib = L.load()
    Bn, H, W, r = 1, 8, 8, 4
    N = H * W
    outs = [Buf(n=N * (H >> l) * (W >> l)) for l in range(4)]
    pp, keep = F._pp(L, outs)
    pp_hole, keep_hole = F._pp(L, outs)
    keep_hole[2] = None
    cbuf, cs = Buf(torch.zeros(2 * N)), (2 * N, N, 1)
    dout = Buf(torch.ones(N * 4 * 81))
    cp, dp = L.ptr(cbuf.mid), L.ptr(dout.mid)
    refused = dict(three_levels=lib.fsraft_corr_lookup_bwd(pp, 3, cp, *cs, dp, 1, Bn, H, W, r, None),
                   null_level=lib.fsraft_corr_lookup_bwd(pp_hole, 4, cp, *cs, dp, 1, Bn, H, W, r, None),
                   radius_2=lib.fsraft_corr_lookup_bwd(pp, 4, cp, *cs, dp, 0, Bn, H, W, 2, None),
                   null_dout=lib.fsraft_corr_lookup_bwd(pp, 4, cp, *cs, ctypes.c_void_p(None), 1, Bn, H, W, r, None),
                   unpool_5_levels=lib.fsraft_corr_unpool_bwd(pp, 5, Bn, H, W, None),
                   unpool_0_levels=lib.fsraft_corr_unpool_bwd(pp, 0, Bn, H, W, None))
    torch.cuda.synchronize()
    assert all(rc == FS_ERR_ARG for rc in refused.values()), {k: v for k, v in refused.items() if v != FS_ERR_ARG}
    for b in outs:
        b.untouched()
    cbuf.intact()
    dout.intact()
