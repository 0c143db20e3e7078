"""The five entry points of csrc/stem.hip and csrc/conv_small.hip called through _lib, each against its float64 restatement
(tests/_smallconvref.py), at the edges of their launch geometry: the stem forward on one clipped partial tile, around its 8 x 32
tile on both axes, across a batch, and with 513 and 1030 tiles on 512 persistent workgroups (two and three trips, both patch
buffers), N = 32 and 64, bias and none; the stem weight gradient at every boundary of its reduction's three loops (4 .. 513
partial matrices, two and three tiles per workgroup); the flow head's forward, weight gradient and data gradient over their
sliding-window runs (one short / exact / one over 8 and 16 pixels), both register sets (C <= 256, C > 256), sources inside
wider rows, strided outputs, 1 .. 33 segments, prior contents, and once past each grid cap.  The test owns every buffer
(_util.Buf): guard rows, pitch pads, channels outside the source slice, dy columns >= 2, the pad columns of dwpk, channels >= C of
dx and the gaps of a strided output hold a NaN pattern and are compared bit for bit after each call, inputs included.  Needs an
MI355X: -m gpu.

Limits: _convref's gamma / judge unchanged for the four GEMM-shaped entries (score: the largest used share of the elementwise
bound, 4 x the twin's Frobenius error + u ||ref||, and 1/16 of the bf16x1 twin's; <= 1 passes), _smallconvref.LIMITS from the fp32
twins for the data gradient -- all from the CPU (tests/test_smallconvref.py), none from the kernels.  The stem always runs
split-bf16: both settings of fsraft_set_arithmetic give the same bits, as does a second launch (the reduce order is fixed).

profiles/stem_small_kernel_margins.txt lists every comparison (FSRAFT_PARITY_LOG).  Worst used shares measured on MI355X
(elementwise: of the bound; frobenius: ||got - ref|| / (4 ||twin - ref|| + u ||ref||); dx: units of u sum |w| |dy|; score: the
largest used share of the call):
  stem_fwd out elementwise                                     0.297  limit 1     (1030-7-7-32-0)
  stem_fwd out frobenius vs bf16x3 twin                        0.249  limit 1     (3-17-65-32-0)
  stem_fwd score                                               0.297  limit 1     (1030-7-7-32-0)
  stem_fwd out: second launch, exact-fp32 setting                  0  exact      (every case)
  stem_wgrad dw elementwise                                    0.705  limit 1     (1-7-7-64)
  stem_wgrad dw frobenius vs bf16x3 twin                        0.25  limit 1     (1-1025-7-64)
  stem_wgrad score                                             0.705  limit 1     (1-7-7-64)
  stem_wgrad dw: second launch, exact-fp32 setting                 0  exact      (every case)
  small_fwd out elementwise                                    0.045  limit 1     (3-43-512-4-4-0-planar-1)
  small_fwd out frobenius vs fp32 twin                         0.142  limit 1     (3-43-512-4-4-0-planar-1)
  small_fwd score                                              0.142  limit 1     (3-43-512-4-4-0-planar-1)
  small_wgrad dwpk (+ dbias) elementwise                       0.816  limit 1     (1-1-1-256-260-4-2-7-1-0)
  small_wgrad dwpk (+ dbias) frobenius vs fp32 twin            0.672  limit 1     (1-1-9-260-520-260-33-7-1-1)
  small_wgrad score                                            0.816  limit 1     (1-1-1-256-260-4-2-7-1-0)
  small_dgrad dx                                                4.29  limit 30    (1-129-2048-4-4-2-4)
  small_dgrad score                                            0.143  limit 1     (1-129-2048-4-4-2-4)
(cases are the fields of _smallconvref's case tuples.)  36 tests, 4 s for the module, every test 0.4 s or less.  The stem's
Frobenius error is its bf16x3 twin's (the dropped lo x lo products: ratio 1.00 on every case).  The small weight gradient sums
each wave's pixels one after the other and every segment onto the same registers, so its Frobenius error is 0.13 .. 3.45 x that of
_convref's fp32 twin (a blocked fp32 GEMM per segment, the segments added in float64) -- 3.45 with 33 segments of nine pixels, 7.0
on 1-1-1-256-260-4-2-7-1-0, where the twin happens to be almost exact and the u ||ref|| floor carries the criterion -- and agrees
with _smallconvref's waves-then-atomics twin to two digits; it stays under 4 x + floor everywhere, so that order twin sets no limit.
small_wgrad's 0.816 is one correctly rounded add onto a prior value next to a power of two (the bound's u |prior| term); its atomics
make the Frobenius figures vary in the third digit from run to run.  No kernel exceeded a limit and none wrote a float it does not
own: no kernel change came out of these tests.
"""
import ctypes

import pytest
import torch

import _smallconvref as S
from _util import PATTERN, Buf, _log_margin

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


def _ptr_array(L, ptrs):
    arr = (ctypes.c_void_p * len(ptrs))(*[p.value if p is not None else None for p in ptrs])
    return ctypes.cast(arr, L._PP), arr


def _args(c, over):
    a = c._asdict()
    a.update(N=a.get("N", 2), KH=3, KW=3)
    a.update(over)
    return a


def _call_stem_fwd(L, b, c, **over):
    a = _args(c, over)
    return L.load().fsraft_stem7x7s2_fwd(_p(L, b["x"]), _p(L, b["w"]), _p(L, b.get("bias")), _p(L, b["out"]), a["B"], a["H"], a["W"], a["N"], L.stream())


def _call_stem_wgrad(L, b, c, **over):
    a = _args(c, over)
    return L.load().fsraft_stem7x7s2_wgrad(_p(L, b["x"]), _p(L, b["dy"]), _p(L, b["dw"]), _p(L, b["scratch"]), a["B"], a["H"], a["W"], a["N"], L.stream())


def _call_small_fwd(L, b, c, **over):
    a = _args(c, over)
    obs, ocs, ops = S.out_strides(c.olay, c.H * c.W)
    return L.load().fsraft_conv_small_fwd(_p(L, b["x"], c.coff), a["ld"], a["C"], _p(L, b["w"]), _p(L, b.get("bias")), _p(L, b["out"]), obs, ocs, ops,
                                          a["N"], a["B"], a["H"], a["W"], a["KH"], a["KW"], L.stream())


def _call_small_wgrad(L, b, c, **over):
    a = _args(c, over)
    pdy, k1 = _ptr_array(L, [_p(L, b[f"dy{t}"]) for t in range(c.nseg)])
    px, k2 = _ptr_array(L, [_p(L, b[f"x{t}"], c.coff) for t in range(c.nseg)])
    return L.load().fsraft_conv_small_wgrad(pdy, px, c.nseg, a["ldy"], a["ldx"], a["C"], _p(L, b["dwpk"]), _p(L, b.get("dbias")), a["N"], a["B"], a["H"],
                                            a["W"], a["KH"], a["KW"], L.stream())


def _call_small_dgrad(L, b, c, **over):
    a = _args(c, over)
    return L.load().fsraft_conv_small_dgrad(_p(L, b["dy"]), a["ldy"], _p(L, b["w"]), _p(L, b["dx"]), a["lddx"], _p(L, b.get("relu")), a["ldm"], a["C"],
                                            a["N"], a["B"], a["H"], a["W"], a["KH"], a["KW"], L.stream())


CALLS = dict(stem_fwd=_call_stem_fwd, stem_wgrad=_call_stem_wgrad, small_fwd=_call_small_fwd, small_wgrad=_call_small_wgrad,
             small_dgrad=_call_small_dgrad)


class Tally:
    """The comparisons of one test: every figure is logged before anything is asserted."""

    def __init__(self):
        self.rows, self.failed = [], []

    def check(self, what, got, outs):
        ok, s, rep = S.verdict(got, outs)
        for name, r in rep.items():
            if "units" in r:
                self.rows.append((f"{what} {name}", r["units"], S.LIMITS["dgrad"], "worst |got - ref| / (u sum |w| |dy|); masked elements +0.0; every other float of the buffer bit for bit"))
            else:
                self.rows.append((f"{what} {name} elementwise", r["elem"], 1.0, "|got - ref| / (gamma S + u |prior|); every other float of the buffer bit for bit"))
                self.rows.append((f"{what} {name} frobenius vs {r['twin']} twin", r["frob"], 1.0,
                                  f"||got - ref|| / (4 ||twin - ref|| + u ||ref||); ||got - ref|| / ||twin - ref|| = {r['ratio_twin']:.3g}; "
                                  f"bf16x1 ratio {r['ratio_b1']:.3e} (limit 1/16)"))
        self.rows.append((f"{what} score", s, 1.0, "the largest used share of the entry's criteria; inf: a float outside the addressed ones changed, a non-finite value, a masked element not +0.0"))
        if not ok:
            self.failed.append((what, s, rep))

    def exact(self, what, ok):
        self.rows.append((what, 0.0 if ok else 1.0, 0.0, "exact: 0 = the same bits"))
        if not ok:
            self.failed.append((what,))

    def done(self):
        for what, w, lim, detail in self.rows:
            _log_margin(what, w, lim, detail)
        assert not self.failed, self.failed


def run(L, T, op, c, label=""):
    """One call of `op` on buffers of its own.  The outputs meet the verdict (which covers each float the call must leave alone),
    every other buffer is compared bit for bit with what it held, every guard row checked.  Returns (buffers, their CPU images)."""
    p, outs = S.problem(op, c)
    bufs = {k: Buf(v) for k, v in p.bufs.items()}
    if op == "stem_wgrad":
        assert L.load().fsraft_stem_slots() * 64 * 192 == S.STEM_SCRATCH
        bufs["scratch"] = Buf(n=S.STEM_SCRATCH)
    L.check(CALLS[op](L, bufs, c), op)
    torch.cuda.synchronize()
    got = {k: b.cpu() for k, b in bufs.items() if k != "scratch"}
    what = f"{op} {S.case_id(c)}{label}"
    for k, b in bufs.items():
        b.intact()
        if k not in outs and k != "scratch":
            assert _same_bits(got[k], p.bufs[k]), (what, k, "an input was written")
    T.check(what, got, outs)
    return bufs, got


def again(L, T, op, c, bufs, got, label):
    """The same call once more onto outputs reset to the pattern: the same bits."""
    _, outs = S.problem(op, c)
    for k in list(outs) + (["scratch"] if "scratch" in bufs else []):
        bufs[k].mid.view(torch.int32).fill_(PATTERN)
    L.check(CALLS[op](L, bufs, c), op)
    torch.cuda.synchronize()
    for k in outs:
        bufs[k].intact()
        T.exact(f"{op} {S.case_id(c)} {k}: {label}", _same_bits(bufs[k].cpu(), got[k]))


def refused(L, op, c, over=None, off=None, null=()):
    """The entry refuses the call and writes nothing: every output stays the pattern, every input keeps its bits."""
    p, outs = S.problem(op, c)
    off = off or {}
    dev = {k: (Buf(n=v.numel(), offset=off.get(k, 0)) if k in outs else Buf(v, offset=off.get(k, 0))) for k, v in p.bufs.items()}
    if op == "stem_wgrad":
        dev["scratch"] = Buf(n=4096)                     # (never reached)
    handed = {k: (None if k in null else b) for k, b in dev.items()}
    assert CALLS[op](L, handed, c, **(over or {})) == FS_ERR_ARG, (op, c, over, off, null)
    torch.cuda.synchronize()
    for k, b in dev.items():
        if k in outs or k == "scratch":
            b.untouched()
        else:
            b.intact()
            assert _same_bits(b.cpu(), p.bufs[k]), (op, c, k)


def _both_arithmetics(L, T, op, c, bufs, got):
    from flow_supervisor_amd import ops
    again(L, T, op, c, bufs, got, "second launch")
    try:
        ops.set_arithmetic(False)
        again(L, T, op, c, bufs, got, "exact-fp32 setting")
    finally:
        ops.set_arithmetic(True)


# ============================================================================================================= stem forward
@pytest.mark.parametrize("shape", S.STEM_SHAPES, ids=S.case_id)
def test_stem_forward_vs_fp64(L, shape):
    """N = 32 / 64, bias and none.  out starts as the pattern and must be written everywhere; x and w keep their bits; a second
    launch and the other arithmetic setting give the same bits."""
    T = Tally()
    for c in S.STEM_FWD_CASES:
        if c[:3] == shape:
            bufs, got = run(L, T, "stem_fwd", c)
            bufs["out"].written()
            _both_arithmetics(L, T, "stem_fwd", c, bufs, got)
    T.done()


def test_stem_forward_refusals(L):
    c = S.StemFwdCase(1, 8, 8, 64, 1)
    for over in (dict(N=48), dict(N=0), dict(H=6), dict(W=6), dict(B=0)):
        refused(L, "stem_fwd", c, over)
    for k in ("x", "w", "out"):
        refused(L, "stem_fwd", c, null=(k,))


# ===================================================================================================== stem weight gradient
@pytest.mark.parametrize("case", S.STEM_WGRAD_CASES, ids=S.case_id)
def test_stem_weight_gradient_vs_fp64(L, case):
    """dw starts as the pattern and is overwritten; the scratch is exactly fsraft_stem_slots() x 64 x 192 floats between intact
    guards, handed over as the pattern (a partial matrix read before it is written shows as a NaN); second launch bit-equal."""
    T = Tally()
    bufs, got = run(L, T, "stem_wgrad", case)
    bufs["dw"].written()
    _both_arithmetics(L, T, "stem_wgrad", case, bufs, got)
    T.done()


def test_stem_weight_gradient_refusals(L):
    c = S.StemWgradCase(1, 9, 7, 64)
    for over in (dict(N=48), dict(H=6), dict(W=6), dict(B=0)):
        refused(L, "stem_wgrad", c, over)
    for k in ("x", "dy", "dw", "scratch"):
        refused(L, "stem_wgrad", c, null=(k,))
    refused(L, "stem_wgrad", c, off=dict(dy=1))          # 16-byte loads of dy


# ============================================================================================================ small forward
def _all(L, op, cases):
    T = Tally()
    for c in cases:
        run(L, T, op, c)
    T.done()


def test_small_forward_vs_fp64(L):
    """C on both register sets and their edges, sources at a column offset of wider rows, planar outputs with gaps between the
    planes and an interleaved one, runs of 1, 7, 8, 9 and 17 pixels."""
    _all(L, "small_fwd", [c for c in S.SMALL_FWD_CASES if c != S.SMALL_FWD_BIG])


def test_small_forward_past_the_grid_cap(L):
    """8256 runs on 2048 x 4 waves: the first 64 waves take a second run."""
    _all(L, "small_fwd", [S.SMALL_FWD_BIG])


def test_small_forward_refusals(L):
    c = S.SmallFwdCase(3, 2, 7, 36, 40, 4, "gap", 1)
    for over in (dict(N=3), dict(C=34), dict(C=516), dict(C=0), dict(ld=42), dict(KH=1), dict(KW=1), dict(B=0)):
        refused(L, "small_fwd", c, over)
    refused(L, "small_fwd", c, off=dict(w=1))            # 16-byte loads of the weights
    for k in ("x", "w", "out"):
        refused(L, "small_fwd", c, null=(k,))


# ==================================================================================================== small weight gradient
def test_small_weight_gradient_vs_fp64(L):
    """1, 2, 16, 17 and 33 segments (one launch per 16), dy pitches 2, 4, 7, dwpk / dbias onto prior contents and onto zeros, dbias
    null; the pad columns of dwpk (C = 4, 36, 252, 260) keep the pattern."""
    _all(L, "small_wgrad", [c for c in S.SMALL_WGRAD_CASES if c != S.SMALL_WGRAD_BIG])


def test_small_weight_gradient_past_the_grid_cap(L):
    """2080 runs on 512 x 4 waves."""
    _all(L, "small_wgrad", [S.SMALL_WGRAD_BIG])


def test_small_weight_gradient_refusals(L):
    c = S.SmallWgradCase(3, 2, 8, 36, 40, 4, 2, 4, 1, 1)
    for over in (dict(N=3), dict(C=34), dict(C=516), dict(C=0), dict(ldx=42), dict(KH=1), dict(KW=1)):
        refused(L, "small_wgrad", c, over)
    refused(L, "small_wgrad", c, null=("dwpk",))
    refused(L, "small_wgrad", c, null=("dy1",))
    refused(L, "small_wgrad", c, null=("x0",))


# ====================================================================================================== small data gradient
def test_small_data_gradient_vs_fp64(L):
    """dx inside rows of C, C + 4 and 512 floats (the further channels keep the pattern), dy pitches 2, 4, 5, no mask and a mask
    with +0.0, -0.0, the smallest denormal of either sign: masked elements are +0.0, a positive denormal lets the gradient pass."""
    _all(L, "small_dgrad", [c for c in S.SMALL_DGRAD_CASES if c != S.SMALL_DGRAD_BIG])


def test_small_data_gradient_past_the_grid_cap(L):
    """16512 runs on 4096 x 4 waves."""
    _all(L, "small_dgrad", [S.SMALL_DGRAD_BIG])


def test_small_data_gradient_refusals(L):
    c = S.SmallDgradCase(1, 2, 16, 36, 512, 5, 36)
    for over in (dict(C=260), dict(C=34), dict(ldy=1), dict(lddx=42), dict(ldm=38), dict(N=3), dict(KH=1), dict(B=0)):
        refused(L, "small_dgrad", c, over)
    refused(L, "small_dgrad", c, off=dict(dx=1))
    refused(L, "small_dgrad", c, off=dict(relu=2))
    for k in ("dy", "w", "dx"):
        refused(L, "small_dgrad", c, null=(k,))
