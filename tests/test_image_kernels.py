"""csrc/image_ops.hip called through the C ABI on tests/_util.Buf buffers -- guard rows and unwritten outputs hold the NaN pattern --
against tests/_imageref.py: box copies and edge padding bit for bit, the bilinear resize and its backward within LIMITS (4 x what the
fp32 twin needs on these very inputs; tests/test_imageref.py).  Every launch: nothing written outside the outputs, every output
element written, the inputs untouched; the backward twice for the same bits.  Every comparison goes to the parity log
(FSRAFT_PARITY_LOG; profiles/image_ops_margins.txt).  Worst values measured on MI355X, in the units of _imageref's scales:
  resize value     2.19  limit 9   (2x257x3x256, two channels with the flow factors, n = 32)
  resize gradient  3.34  limit 20  (2x255x3x256, two channels with the flow factors, n = 32)
  exact rows (box copies, edge padding, the backward twice, +0.0 where no tap reaches): no mismatch.
The kernels set none of the limits."""
import ctypes
import functools

import pytest
import torch

import _imageref as R
from _util import Buf, _log_margin

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _leave_no_cached_segments():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def L():
    from flow_supervisor_amd import _lib
    _lib.load()
    return _lib


def _ids(c):
    return "x".join(map(str, c)) if isinstance(c, tuple) else str(c)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _ptr_array(L, bufs):
    arr = (ctypes.c_void_p * len(bufs))(*[L.ptr(b.mid).value for b in bufs])
    return ctypes.cast(arr, L._PP), arr


def to_mem(t, layout):
    """A canonical [B,H,W,C] CPU tensor as the flat memory of `layout`."""
    return (t if layout == "nhwc" else t.permute(0, 3, 1, 2)).contiguous().reshape(-1)


def from_mem(flat, layout, B, H, W, C):
    return flat.view(B, H, W, C) if layout == "nhwc" else flat.view(B, C, H, W).permute(0, 2, 3, 1)


def strides(layout, H, W, C):
    """(batch, channel, row, x)"""
    return (H * W * C, 1, W * C, C) if layout == "nhwc" else (C * H * W, H * W, W, 1)


def log_exact(what, ok, detail):
    _log_margin(what, 0.0 if ok else 1.0, 0.0, f"exact, {detail}")


# =================================================================================================================== box copy
def three_offsets(Hf, Wf, H, W):
    """Flush with the top-left corner, flush with the bottom-right corner, interior."""
    return [(0, 0), (Hf - H, Wf - W), ((Hf - H) // 2, (Wf - W) // 2)]


# C, Hf, Wf, H, W, offsets (None: the three above)
BOX_CASES = (
    (1, 6, 9, 1, 1, None),                                  # a 1 x 1 window
    (2, 5, 7, 5, 7, None),                                  # the window is the frame
    (1, 7, 13, 3, 4, None), (2, 7, 9, 3, 3, None), (3, 6, 8, 2, 4, None), (3, 5, 6, 2, 1, None),
    (128, 5, 6, 2, 3, None),                                # always the 16-byte route interleaved
    (1, 4, 300, 2, 257, None), (2, 3, 261, 2, 257, None),   # more than one workgroup per row
    (1, 6, 16, 3, 8, [(0, 0), (1, 1), (2, 2), (3, 3)]),     # C = 1, x offsets 0..3: with the bases below both routes, mixed in one launch
    (1, 6, 16, 3, 8, [(0, 0), (3, 8), (1, 4)]),             # every start a multiple of 4: the launch sized for 16-byte units
    (2, 4, 16, 2, 8, [(0, 4), (2, 8), (1, 0)]),             # planar with channel strides that are multiples of 4
)
BASES = (0, 1, 2)                                           # floats off the 16-byte alignment


def box_launch(L, srcs, dsts, place, B, C, Hf, Wf, H, W, yx, layout):
    sp, k1 = _ptr_array(L, srcs)
    dp, k2 = _ptr_array(L, dsts)
    offs = (ctypes.c_int * (2 * B))(*[v for p in yx for v in p])
    L.check(L.load().fsraft_box_copy(sp, dp, len(srcs), place, B, C, Hf, Wf, H, W, offs, *strides(layout, Hf, Wf, C),
                                     *strides(layout, H, W, C), L.stream()), "box_copy")
    torch.cuda.synchronize()


@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("place", (0, 1), ids=("gather", "place"))
@pytest.mark.parametrize("case", BOX_CASES, ids=_ids)
def test_box_copy_is_exact(L, case, place, layout):
    C, Hf, Wf, H, W, yx = case
    yx = three_offsets(Hf, Wf, H, W) if yx is None else yx
    B = len(yx)
    bad = []
    for n, base in [(1, b) for b in BASES] + [(32, 0)]:
        if place:
            cpu = [R.box_values(B, H, W, C, i) for i in range(n)]
            want = [R.pad_ref(x, yx, (Hf, Wf)) for x in cpu]
            out_dims = (B, Hf, Wf, C)
        else:
            cpu = [R.box_values(B, Hf, Wf, C, i) for i in range(n)]
            want = [R.crop_ref(x, yx, (H, W)) for x in cpu]
            out_dims = (B, H, W, C)
        srcs = [Buf(to_mem(x, layout), offset=base) for x in cpu]
        nout = out_dims[0] * out_dims[1] * out_dims[2] * out_dims[3]
        twice = []
        for _ in range(2):
            dsts = [Buf(n=nout, offset=base) for _ in range(n)]
            box_launch(L, srcs, dsts, place, B, C, Hf, Wf, H, W, yx, layout)
            for d in dsts:
                d.written()
            twice.append([from_mem(d.cpu(), layout, *out_dims) for d in dsts])
        for s, x in zip(srcs, cpu):
            s.intact()
            assert _same_bits(s.cpu(), to_mem(x, layout)), "an input was written"
        ok = all(_same_bits(g, w) for g, w in zip(twice[0], want)) and all(_same_bits(a, b) for a, b in zip(*twice))
        if place:
            outside = want[0] == 0                        # (box_values holds no zero)
            ok = ok and all(bool((_bits(g)[outside] == 0).all()) for g in twice[0])
        if not ok:
            bad.append((n, base))
    log_exact(f"box_copy {'place' if place else 'gather'} {_ids(case[:5])} {layout}", not bad, "n = 1 at bases 0, 1, 2 and n = 32, twice")
    assert not bad, bad


# ====================================================================================================================== resize
@functools.lru_cache(maxsize=None)
def _resize_expect(case, C, fac, i):
    x, g = R.resize_inputs(case, C, i)
    return R.resize_expect(x, g, case[2:], R.case_factors(case, fac))


def resize_launch(L, fn, srcs, dsts, B, C, case, layout, fac):
    hi, wi, ho, wo = case
    sp, k1 = _ptr_array(L, srcs)
    dp, k2 = _ptr_array(L, dsts)
    f = (ctypes.c_float * C)(*fac) if fac is not None else None
    L.check(getattr(L.load(), fn)(sp, dp, len(srcs), B, C, hi, wi, ho, wo, *strides(layout, hi, wi, C), *strides(layout, ho, wo, C),
                                  f, L.stream()), fn)
    torch.cuda.synchronize()


@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("n", R.LIST_N)
@pytest.mark.parametrize("variant", R.resize_variants(), ids=lambda v: f"{_ids(v[0])}-c{v[1]}{'-flow' if v[2] else ''}")
def test_resize_and_its_backward_vs_fp64(L, variant, n, layout):
    case, C, with_fac = variant
    hi, wi, ho, wo = case
    B = R.B
    fac = R.case_factors(case, with_fac)
    ins = [R.resize_inputs(case, C, i) for i in range(n)]
    xs = [Buf(to_mem(x, layout)) for x, _ in ins]
    gs = [Buf(to_mem(g, layout)) for _, g in ins]
    out = [Buf(n=B * ho * wo * C) for _ in range(n)]
    resize_launch(L, "fsraft_resize_bilinear_fwd", xs, out, B, C, case, layout, fac)
    grads = []
    for _ in range(2):
        dx = [Buf(n=B * hi * wi * C) for _ in range(n)]
        resize_launch(L, "fsraft_resize_bilinear_bwd", gs, dx, B, C, case, layout, fac)
        grads.append(dx)
    dead = ~(R.reached(hi, ho)[:, None] & R.reached(wi, wo)[None, :])
    worst = dict(rs_val=(-1.0, 0), rs_grad=(-1.0, 0))
    exact = True
    for i in range(n):
        for b in (xs[i], gs[i]):
            b.intact()
        assert _same_bits(xs[i].cpu(), to_mem(ins[i][0], layout)) and _same_bits(gs[i].cpu(), to_mem(ins[i][1], layout)), "an input was written"
        out[i].written()
        grads[0][i].written()
        grads[1][i].written()
        ev, eg = _resize_expect(case, C, with_fac, i)
        v = from_mem(out[i].cpu(), layout, B, ho, wo, C)
        d = from_mem(grads[0][i].cpu(), layout, B, hi, wi, C)
        worst["rs_val"] = max(worst["rs_val"], (R.need(v, *ev[:3])[0], i))
        worst["rs_grad"] = max(worst["rs_grad"], (R.need(d, *eg[:3])[0], i))
        exact = exact and _same_bits(grads[0][i].cpu(), grads[1][i].cpu()) and bool((_bits(d)[:, dead] == 0).all())
        if (hi, wi) == (ho, wo) and fac is None:
            exact = exact and _same_bits(v, ins[i][0]) and _same_bits(d, ins[i][1])
    what = f"{_ids(case)} c{C}{' flow' if with_fac else ''} n={n} {layout}"
    for k, (w, i) in worst.items():
        _log_margin(f"{k} {what}", w, R.LIMITS[k], f"worst |got - ref| / scale, list member {i}")
    log_exact(f"resize backward twice, +0.0 where no tap reaches {what}", exact, f"{int(dead.sum())} sources unreached")
    assert all(w <= R.LIMITS[k] for k, (w, _) in worst.items()), worst
    assert exact


# ================================================================================================================ edge padding
def _input_pads(hw, mode):
    p = R.input_padding_ref(hw[0], hw[1], mode)
    return (p[1][0], p[1][1], p[2][0], p[2][1])


# B, C, H, W, pads (top, bottom, left, right), list lengths
PAD_CASES = (
    [(2, 3, 5, 9, p, (1,)) for p in ((0, 0, 0, 0), (7, 0, 0, 0), (0, 7, 0, 0), (0, 0, 7, 0), (0, 0, 0, 7))]
    + [(2, 2, 1, 1, (7, 7, 7, 7), (1, 32)), (1, 1, 1, 1, (0, 7, 7, 0), (1,))]
    + [(2, 3, 5, 9, _input_pads((5, 9), m), (1, 32)) for m in ("sintel", None)]
    + [(1, 3, 436, 1024, _input_pads((436, 1024), m), (1,)) for m in ("sintel", None)])


@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("case", PAD_CASES, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}x{c[3]}-pads{_ids(c[4])}")
def test_pad_edge_is_exact(L, case, layout):
    B, C, H, W, pads, lengths = case
    t, b, l, r = pads
    Hd, Wd = H + t + b, W + l + r
    ok = True
    for n in lengths:
        cpu = [R.box_values(B, H, W, C, i) for i in range(n)]
        srcs = [Buf(to_mem(x, layout)) for x in cpu]
        dsts = [Buf(n=B * Hd * Wd * C) for _ in range(n)]
        sp, k1 = _ptr_array(L, srcs)
        dp, k2 = _ptr_array(L, dsts)
        L.check(L.load().fsraft_pad_edge(sp, dp, n, B, C, H, W, t, b, l, r, *strides(layout, H, W, C), *strides(layout, Hd, Wd, C),
                                         L.stream()), "pad_edge")
        torch.cuda.synchronize()
        for s, d, x in zip(srcs, dsts, cpu):
            s.intact()
            d.written()
            ok = ok and _same_bits(from_mem(d.cpu(), layout, B, Hd, Wd, C), R.pad_edge_ref(x, pads))
    log_exact(f"pad_edge {B}x{C}x{H}x{W} pads {pads} {layout}", ok, f"n = {lengths}")
    assert ok
