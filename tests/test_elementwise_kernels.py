"""The 16 kernels of csrc/elementwise.hip called through their 13 C entry points, each against its float64 restatement
(tests/_ewref.py), at the edges of their launch geometry: the 32 x 32 tile of the layout pair one short / exact / one over on
either axis with every pitch and channel offset, accumulating or not, and as ops.transpose_batched uses it; space_to_depth2 both
ways; both im2col7 kernels (chosen by the alignment of cols) on images whose every pixel has taps outside, three pitches and three
flow layouts; col2im7 and the flow copies at 254 / 256 / 258 threads; relu_bwd with C % 4 != 0 inside wider rows whose further
columns hold live values; the ConvGRU gate backward on its 16-byte and 4-byte kernels -- the latter reached through hid % 4,
ldzr % 4 and each pointer in turn -- with and without running sums and the second summand, stage 2 on what stage 1 left; col_sum
over its row split up to the capped one with empty trailing row blocks; sum_n over one, two and three launches, bit for bit
against the list-order fp32 sum; axpby with b = 0 onto a NaN buffer; and every grid-stride kernel once on the second trip of its
capped grid.  The test owns every buffer (_util.Buf): guard rows, pitch pads, columns outside [coff, coff + C), the other half of
dzr and every float an entry must not write hold a NaN pattern (or a neighbour's live values) and are compared bit for bit
after each call, inputs included.  Needs an MI355X: -m gpu.

Limits: _ewref.LIMITS, set from the fp32 twins on the CPU (tests/test_ewref.py), not from the kernels.  profiles/
elementwise_kernel_margins.txt lists every comparison (FSRAFT_PARITY_LOG).  Worst values measured on MI355X, in the units of
_ewref's scales, and the module's wall time:
  nchw_to_nhwc dst                                         1  limit 4    (2-33-31-36-0-1)
  nhwc_to_nchw dst                                         1  limit 4    (2-33-31-36-0-1)
  space_to_depth2 dst                                      0  exact      (1-2-2-4-0)
  space_to_depth2 (round trip) dst                         0  exact      (1-2-2-4-1)
  space_to_depth2 inverse o forward                        0  exact      (1-2-2-4-0)
  im2col7 cols                                             0  exact      (2-1-1-100-0-planar)
  col2im7 dflow                                         1.97  limit 9    (2-3-3-100-0)
  flow_to_nhwc dst                                         0  exact      (1-127-128-126-planar-0)
  nhwc_to_flow dflow                                   0.995  limit 4    (2-64-4-0-planar-1)
  relu_bwd g                                               0  exact      (1-4-4-132)
  gru_bwd1 dzr                                          3.73  limit 20   (4194305-4-8-0-0-_)
  gru_bwd1 dq                                            2.6  limit 20   (255-4-8-1-1-_)
  gru_bwd1 dh                                           1.71  limit 7    (257-4-8-1-1-_)
  gru_bwd2 dzr                                          2.86  limit 20   (4194305-4-8-0-0-_)
  gru_bwd2 dh                                          0.999  limit 8    (4194305-4-8-0-0-_)
  gru_bwd1 dzr_sum                                      2.29  limit 9    (3-96-192-1-1-_)
  gru_bwd1 dq_sum                                       2.02  limit 9    (3-128-256-1-0-_)
  gru_bwd2 dzr_sum                                      1.37  limit 9    (257-4-8-1-1-_)
  col_sum out                                           2.01  limit 20   (257-64-71--0.5)
  sum_n out                                             3.97  limit 20   (16-1028-0-0)
  sum_n out = the fp32 sum in list order                   0  exact      (1-4-0-0)
  axpby y                                                  1  limit 8    (4194305--0.37-0.5)
(exact rows: 0 = every addressed float and every other float of the buffer bit for bit; cases are the fields of _ewref's case
tuples.)  31 tests, 10.2 s for the module; the slowest, the ConvGRU pair on the second trip of its grid, 5.3 s with its float64
reference, every other test 1.2 s or less.  col_sum's atomics make its figure vary from run to run (256-63-67-1.0: 0.89 and 1.30
in two runs); everything else repeats to the digit.  No kernel exceeded a limit; sum_n is bit for bit the list-order fp32 sum on the device.

relu_bwd's tail columns.  relu_bwd_kernel walked (C + 3) / 4 four-float chunks per row and masked all four lanes of the last
one, so with C % 4 != 0 it also zeroed columns C .. roundup4(C) - 1 of g wherever y was <= 0 there -- in UpdateBlock.bwd_motion
(C = 126 in 128-wide rows) the gradient of the two flow pass-through channels.
Before the fix (the parent's kernel behind the new entry checks): test_relu_bwd_vs_fp64 failed its exact comparison on the four
C = 126 cases and on no other -- `relu_bwd 1-126-128-132 g`, `3-126-128-132`, `1-126-132-128`, `3-126-132-128`: score inf.  At
3-126-128-132 the six floats (m, 126) and (m, 127), m = 0 .. 2, came back 0.0 in place of -0.2759, 2.516, 0.04189, 0.8892,
2.244, 1.415 (y <= 0 there by design); columns 0 .. 125 were right.  After: all 20 cases and the second-trip case exact.
The kernel now stores those lanes back as loaded.  The entries also gained the argument checks their kernels rely on (16-byte
aligned bases for relu_bwd and space_to_depth2, C <= ld and coff + C <= ld, ldzr >= 2 hid, col2im7's ld >= 98, positive sizes
where the grid is computed from them); the refusal tests below hold them.
"""
import ctypes

import pytest
import torch

import _ewref as R
from _util import Buf, _log_margin

pytestmark = pytest.mark.gpu
FS_ERR_ARG = 1


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


def _p(L, b, lo=0):
    """Pointer to float `lo` of a Buf's payload; NULL for None."""
    return L.ptr(b.mid[lo:]) if b is not None else None


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class Tally:
    """The comparisons of one test: every figure is logged before anything is asserted."""

    def __init__(self):
        self.rows, self.failed = [], []

    def check(self, what, got, o):
        w = R.score(got, o)
        lim = R.LIMITS[o.key] if o.scale is not None else 0.0
        self.rows.append((what, w, lim, "worst |got - ref| / scale; every other float of the buffer bit for bit" if lim else
                          "exact: 0 = the addressed floats and every other float of the buffer bit for bit"))
        if not w <= lim:
            self.failed.append((what, w, lim))

    def exact(self, what, ok):
        self.rows.append((what, 0.0 if ok else 1.0, 0.0, "exact: 0 = the same bits"))
        if not ok:
            self.failed.append((what,))

    def done(self):
        for what, w, lim, detail in self.rows:
            _log_margin(what, w, lim, detail)
        assert not self.failed, self.failed


CALLS = {
    "nchw_to_nhwc": lambda L, lib, b, c, a: lib.fsraft_nchw_to_nhwc(_p(L, b["src"]), _p(L, b["dst"]), *c, L.stream()),
    "nhwc_to_nchw": lambda L, lib, b, c, a: lib.fsraft_nhwc_to_nchw(_p(L, b["src"]), _p(L, b["dst"]), *c, L.stream()),
    "space_to_depth2": lambda L, lib, b, c, a: lib.fsraft_space_to_depth2(_p(L, b["src"]), _p(L, b["dst"]), *c, L.stream()),
    "im2col7": lambda L, lib, b, c, a: lib.fsraft_im2col7(_p(L, b["flow"], a["base"]), a["bs"], a["cs"], a["ps"], _p(L, b["cols"]), c.ld,
                                                        c.B, c.H, c.W, L.stream()),
    "col2im7": lambda L, lib, b, c, a: lib.fsraft_col2im7(_p(L, b["dcols"]), c.ld, _p(L, b["dflow"]), c.B, c.H, c.W, c.acc, L.stream()),
    "flow_to_nhwc": lambda L, lib, b, c, a: lib.fsraft_flow_to_nhwc(_p(L, b["flow"], a["base"]), a["bs"], a["cs"], a["ps"], _p(L, b["dst"]),
                                                                  c.ld, c.coff, c.B, c.HW, L.stream()),
    "nhwc_to_flow": lambda L, lib, b, c, a: lib.fsraft_nhwc_to_flow(_p(L, b["src"]), c.ld, c.coff, _p(L, b["dflow"]), c.B, c.HW, c.acc,
                                                                  L.stream()),
    "relu_bwd": lambda L, lib, b, c, a: lib.fsraft_relu_bwd(_p(L, b["g"]), c.ldg, _p(L, b["y"]), c.ldy, c.M, c.C, L.stream()),
    "gru_bwd1": lambda L, lib, b, c, a: lib.fsraft_gru_bwd1(_p(L, b["dhn"]), _p(L, b.get("dhn2")), _p(L, b["z"]), _p(L, b["q"]), _p(L, b["h"]),
                                                          _p(L, b["dzr"]), c.ldzr, _p(L, b["dq"]), _p(L, b["dh"]), _p(L, b.get("dzr_sum")),
                                                          _p(L, b.get("dq_sum")), c.M, c.hid, L.stream()),
    "gru_bwd2": lambda L, lib, b, c, a: lib.fsraft_gru_bwd2(_p(L, b["drh"]), _p(L, b["r"]), _p(L, b["h"]), _p(L, b["dzr"]), c.ldzr,
                                                          _p(L, b["dh"]), _p(L, b.get("dzr_sum")), c.M, c.hid, L.stream()),
    "col_sum": lambda L, lib, b, c, a: lib.fsraft_col_sum(_p(L, b["x"]), c.ld, c.M, c.C, _p(L, b["out"]), c.scale, L.stream()),
    "axpby": lambda L, lib, b, c, a: lib.fsraft_axpby(_p(L, b["x"]), _p(L, b["y"]), c.a, c.b, c.n, L.stream()),
}


def _ptr_array(L, ptrs):
    """(c_void_p array cast to the entry's pointer-to-pointer type, the array to keep alive); an entry None is NULL."""
    arr = (ctypes.c_void_p * len(ptrs))(*[p.value if p is not None else None for p in ptrs])
    return ctypes.cast(arr, L._PP), arr


def _call_sum_n(L, lib, b, c, a):
    pp, keep = _ptr_array(L, [_p(L, b[f"src{t}"]) for t in a["order"]])
    return lib.fsraft_sum_n(pp, c.n, _p(L, b["out"]), c.count, c.acc, L.stream())


CALLS["sum_n"] = _call_sum_n


def run(L, T, p, outs=None, label=""):
    """One call of p.op on buffers of its own.  Every output is scored (which covers each float the call must leave alone), every
    other buffer compared bit for bit with what it held, every guard row checked.  Returns {name: flat CPU tensor} afterwards."""
    lib = L.load()
    bufs = {k: Buf(v, offset=p.off.get(k, 0)) for k, v in p.bufs.items()}
    L.check(CALLS[p.op](L, lib, bufs, p.case, p.arg), p.op)
    torch.cuda.synchronize()
    got = {k: b.cpu() for k, b in bufs.items()}
    outs = R.expect(p) if outs is None else outs
    what = f"{p.op} {R.case_id(p.case)}{label}"
    for k, b in bufs.items():
        b.intact()
        if k in outs:
            T.check(f"{what} {k}", got[k], outs[k])
        else:
            assert _same_bits(got[k], p.bufs[k]), (what, k, "an input was written")
    return got


def refused(L, op, case, bufs, arg=None, off=None, null=()):
    """The entry refuses the call and writes nothing: every buffer keeps its bits."""
    off = off or {}
    dev = {k: Buf(v, offset=off.get(k, 0)) for k, v in bufs.items()}
    handed = {k: (None if k in null else b) for k, b in dev.items()}
    assert CALLS[op](L, L.load(), handed, case, arg or {}) == FS_ERR_ARG, (op, case, off, null)
    torch.cuda.synchronize()
    for k, b in dev.items():
        b.intact()
        assert _same_bits(b.cpu(), bufs[k]), (op, case, k)
        if bool((bufs[k].view(torch.int32) == R.PATTERN).all()):
            b.untouched()


def _small(op):
    return [c for c in R.cases(op) if c not in R.BIG_CASES]


def _big(op):
    return [c for c in R.cases(op) if c in R.BIG_CASES]


def _run_all(L, op, cases):
    T = Tally()
    for c in cases:
        run(L, T, R.build(op, c))
    T.done()


# ================================================================================================== NCHW <-> channels-last
@pytest.mark.parametrize("op", ("nchw_to_nhwc", "nhwc_to_nchw"))
def test_layout_pair_vs_fp64(L, op):
    """Without accumulate the moved bits; with it one fp32 add per element.  nhwc_to_nchw's table ends with ops.transpose_batched's
    use (B = 3, N = 33, M = 65) and both hold test_gemm_and_layout_kernels' 2 x 37 x 5 x 9 in rows of 40."""
    _run_all(L, op, R.cases(op))


@pytest.mark.parametrize("op", ("nchw_to_nhwc", "nhwc_to_nchw"))
def test_layout_pair_refusals(L, op):
    p = R.build(op, R.LayoutCase(2, 33, 31, 40, 3, 0))
    for bad in (dict(coff=8), dict(ld=32, coff=0), dict(coff=-1), dict(C=0), dict(HW=0), dict(B=0)):      # coff + C > ld, C > ld, ...
        refused(L, op, p.case._replace(**bad), p.bufs)
    refused(L, op, p.case, p.bufs, null=("src",))
    refused(L, op, p.case, p.bufs, null=("dst",))


# ========================================================================================================== space_to_depth2
def test_space_to_depth2_vs_fp64_and_back(L):
    """Both directions as moved bits, and inverse o forward on the device gives the source's bits back."""
    T = Tally()
    for c in _small("space_to_depth2"):
        p = R.build("space_to_depth2", c)
        got = run(L, T, p)
        back = R.build("space_to_depth2", c._replace(inverse=1 - c.inverse))
        back.bufs["src"] = got["dst"]
        again = run(L, T, back, label=" (round trip)")
        T.exact(f"space_to_depth2 {R.case_id(c)} inverse o forward", _same_bits(again["dst"], p.bufs["src"]))
    T.done()


@pytest.mark.parametrize("case", _big("space_to_depth2"), ids=R.case_id)
def test_space_to_depth2_second_trip(L, case):
    _run_all(L, "space_to_depth2", [case])


def test_space_to_depth2_refusals(L):
    op = "space_to_depth2"
    p = R.build(op, R.S2dCase(2, 6, 8, 12, 0))
    for bad in (dict(H=5), dict(W=7), dict(C=6), dict(C=0), dict(B=0), dict(H=0)):
        refused(L, op, p.case._replace(**bad), p.bufs)
    refused(L, op, p.case._replace(C=8), p.bufs, off=dict(src=1))          # 16-byte chunks on both sides
    refused(L, op, p.case._replace(C=8), p.bufs, off=dict(dst=2))
    src = Buf(p.bufs["src"])
    assert L.load().fsraft_space_to_depth2(_p(L, src), _p(L, src), 2, 6, 8, 12, 0, L.stream()) == FS_ERR_ARG             # src == dst
    torch.cuda.synchronize()
    src.intact()
    assert _same_bits(src.cpu(), p.bufs["src"])


# ================================================================================================================== im2col7
def test_im2col7_vs_fp64(L):
    """im2col7_v4_kernel (cols 16-byte aligned) and im2col7_kernel (cols one float off); columns 98 .. ld - 1 are written as zero."""
    _run_all(L, "im2col7", _small("im2col7"))


@pytest.mark.parametrize("case", R.IM2COL_BIG, ids=R.case_id)
def test_im2col7_second_trip(L, case):
    _run_all(L, "im2col7", [case])


def test_im2col7_refusals(L):
    p = R.build("im2col7", R.Im2colCase(2, 3, 3, 104, 0, "planar"))
    for bad in (dict(ld=98), dict(ld=102), dict(B=0), dict(H=0), dict(W=0)):
        refused(L, "im2col7", p.case._replace(**bad), p.bufs, p.arg)
    refused(L, "im2col7", p.case, p.bufs, p.arg, null=("flow",))
    refused(L, "im2col7", p.case, p.bufs, p.arg, null=("cols",))


# ================================================================================================================== col2im7
def test_col2im7_vs_fp64(L):
    """Not accumulating, dflow starts as the NaN pattern: the old value is loaded but must not reach the result."""
    _run_all(L, "col2im7", R.cases("col2im7"))


def test_col2im7_refusals(L):
    p = R.build("col2im7", R.Col2imCase(2, 3, 3, 100, 0))
    for bad in (dict(ld=97), dict(B=0), dict(H=0), dict(W=0)):
        refused(L, "col2im7", p.case._replace(**bad), p.bufs)
    refused(L, "col2im7", p.case, p.bufs, null=("dcols",))
    refused(L, "col2im7", p.case, p.bufs, null=("dflow",))


# ============================================================================================================== flow copies
def test_flow_copies_vs_fp64(L):
    """flow_to_nhwc into columns 126, 127 of 128-wide rows whose first 126 hold live values, and into rows of four; nhwc_to_flow
    from the same, accumulating or not."""
    _run_all(L, "flow_to_nhwc", R.cases("flow_to_nhwc"))
    _run_all(L, "nhwc_to_flow", R.cases("nhwc_to_flow"))


def test_flow_copies_refusals(L):
    for op, c in (("flow_to_nhwc", R.FLOW_TO_NHWC_CASES[0]), ("nhwc_to_flow", R.NHWC_TO_FLOW_CASES[0])):
        p = R.build(op, c)
        for bad in (dict(coff=127), dict(ld=1, coff=0), dict(coff=-1), dict(B=0), dict(HW=0)):            # coff + 2 > ld
            refused(L, op, c._replace(**bad), p.bufs, p.arg)
        for k in p.bufs:
            refused(L, op, c, p.bufs, p.arg, null=(k,))


# ================================================================================================================= relu_bwd
def test_relu_bwd_vs_fp64(L):
    """The mask as moved bits (the gradient or +0.0), and every column at and beyond C -- live gradients over y <= 0 -- bit for bit
    what it was."""
    _run_all(L, "relu_bwd", _small("relu_bwd"))


def test_relu_bwd_second_trip(L):
    _run_all(L, "relu_bwd", [R.RELU_BIG])


def test_relu_bwd_refusals(L):
    p = R.build("relu_bwd", R.ReluCase(3, 126, 128, 132))
    for bad in (dict(ldg=130), dict(ldy=134), dict(C=130), dict(C=129, ldy=128, ldg=132), dict(C=0)):      # pitches; C > ldg; C > ldy
        refused(L, "relu_bwd", p.case._replace(**bad), p.bufs)
    refused(L, "relu_bwd", p.case, p.bufs, off=dict(g=1))                  # the kernel moves 16-byte chunks of both
    refused(L, "relu_bwd", p.case, p.bufs, off=dict(y=3))
    refused(L, "relu_bwd", p.case, p.bufs, null=("g",))
    refused(L, "relu_bwd", p.case, p.bufs, null=("y",))


# ===================================================================================================== ConvGRU gate backward
def _gru_chain(L, T, c):
    """Stage 1, then stage 2 on the dzr, dh and dzr_sum stage 1 left on the device."""
    p1 = R.build("gru_bwd1", c)
    after1 = run(L, T, p1, label=f" [{R.gru_route(c, 1)}]")
    p2 = R._build_gru2("gru_bwd2", c, {k: after1[k] for k in ("dzr", "dh", "dzr_sum") if k in after1})
    run(L, T, p2, label=f" [{R.gru_route(c, 2)}]")


def test_gru_gate_backward_vs_fp64(L):
    """Both stages on the 16-byte kernels (hid 4, 96, 128; ldzr = 2 hid and 2 hid + 4; sums and dhn2 null and not) and on the
    4-byte ones (hid = 6, ldzr % 4 != 0, each pointer of either stage one float off).  After stage 1 the high half of dzr and its
    pitch pad are still the pattern; after stage 2 the low half is bit for bit what stage 1 wrote."""
    T = Tally()
    for c in _small("gru_bwd1"):
        _gru_chain(L, T, c)
    T.done()


def test_gru_gate_backward_second_trip(L):
    T = Tally()
    _gru_chain(L, T, R.GRU_BIG)
    T.done()


def test_gru_gate_backward_refusals(L):
    """dhn2 exists for the 16-byte kernel only: refused wherever the 4-byte one would run; and rows too short for two halves."""
    for c in (R.GruCase(5, 6, 12, 1, 1, ""), R.GruCase(5, 4, 9, 0, 1, ""), R.GruCase(5, 4, 8, 0, 1, "dhn2"), R.GruCase(5, 4, 8, 1, 1, "dq"),
              R.GruCase(5, 4, 8, 1, 1, "dzr_sum")):
        p = R.build("gru_bwd1", c)
        assert R.gru_route(c._replace(dhn2=0), 1) == "scalar" or c.off == "dhn2"
        refused(L, "gru_bwd1", c, p.bufs, off={c.off: 1} if c.off else None)
    c = R.GruCase(5, 4, 8, 1, 0, "")
    p1, p2 = R.build("gru_bwd1", c), R.build("gru_bwd2", c)
    for op, p in (("gru_bwd1", p1), ("gru_bwd2", p2)):
        for bad in (dict(ldzr=7), dict(ldzr=4), dict(hid=0)):
            refused(L, op, c._replace(**bad), p.bufs)
        for k in p.bufs:
            if not k.endswith("_sum"):
                refused(L, op, c, p.bufs, null=(k,))


# ================================================================================================================== col_sum
def test_col_sum_vs_fp64(L):
    """One row block (M < 256), two, the partial last block, 64-column workgroups one short / exact / one over; out holds prior
    values and three pattern floats behind its C; x's pitch pad holds NaNs that must not be read."""
    _run_all(L, "col_sum", _small("col_sum"))


def test_col_sum_past_the_row_split_cap(L):
    """M = 2048 x 128 + 1: 2048 row blocks of 129 rows, the last 15 of them empty."""
    _run_all(L, "col_sum", [R.COL_SUM_BIG])


def test_col_sum_refusals(L):
    p = R.build("col_sum", R.ColSumCase(3, 65, 68, 1.0))
    for bad in (dict(C=69), dict(C=0)):
        refused(L, "col_sum", p.case._replace(**bad), p.bufs)
    refused(L, "col_sum", p.case, p.bufs, null=("x",))
    refused(L, "col_sum", p.case, p.bufs, null=("out",))


# ==================================================================================================================== sum_n
def _sum_n(L, cases):
    T = Tally()
    for c in cases:
        p = R.build("sum_n", c)
        got = run(L, T, p)
        twin = R.sum_n_listorder(R._sum_n_list(p), p.bufs["out"], c.count, c.acc)
        T.exact(f"sum_n {R.case_id(c)} out = the fp32 sum in list order", _same_bits(got["out"][:c.count], twin))
    T.done()


def test_sum_n_vs_fp64_and_bit_exact_in_list_order(L):
    """1 .. 33 tensors (one, two and three launches), one chunk and 257, accumulating or not, a tensor listed twice; the four floats
    behind `count` stay the pattern."""
    _sum_n(L, _small("sum_n"))


def test_sum_n_second_trip(L):
    _sum_n(L, [R.SUM_N_BIG])


def test_sum_n_refusals(L):
    lib = L.load()
    srcs = [Buf(torch.full((8,), 1.0 + t)) for t in range(3)]
    moved = Buf(torch.full((8,), 9.0), offset=1)

    def call(ptrs, n, out, count, lo=0):
        pp, keep = _ptr_array(L, ptrs)
        rc = lib.fsraft_sum_n(pp if ptrs is not None else None, n, _p(L, out, lo) if out is not None else None, count, 0, L.stream())
        torch.cuda.synchronize()
        return rc
    good = [_p(L, s) for s in srcs]
    for ptrs, n, count in ((good, 3, 3), (good, 3, 6), (good, 3, 0), (good, 0, 8), (good[:2] + [_p(L, moved)], 3, 8), (good[:1] + [None] + good[2:], 3, 8)):
        out = Buf(n=8)
        assert call(ptrs, n, out, count) == FS_ERR_ARG, (n, count)
        out.untouched()
    out = Buf(n=12)
    assert call(good, 3, out, 8, lo=1) == FS_ERR_ARG                        # out off its alignment
    assert lib.fsraft_sum_n(None, 3, _p(L, out), 8, 0, L.stream()) == FS_ERR_ARG
    out.untouched()
    for s in srcs + [moved]:
        s.intact()


# ==================================================================================================================== axpby
def test_axpby_vs_fp64(L):
    """b = 0: y starts as the NaN pattern and ends as the finite a x."""
    _run_all(L, "axpby", _small("axpby"))


def test_axpby_second_trip(L):
    _run_all(L, "axpby", [R.AXPBY_BIG])


def test_axpby_refusals(L):
    p = R.build("axpby", R.AxpbyCase(255, 2.0, 0.0))
    refused(L, "axpby", p.case, p.bufs, null=("x",))
    refused(L, "axpby", p.case, p.bufs, null=("y",))
