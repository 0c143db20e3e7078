"""The kernels of csrc/upsample.hip (convex 8x upsampler on its 16-byte and 4-byte routes, forward, backward and the dflow gather;
the bilinear x8 pair), csrc/loss.hip (sequence_loss_kernel) and csrc/optim.hip (adamw_prepare_kernel, adamw_flat_kernel) called
through their C entry points, each against its float64 restatement (tests/_tailref.py), at the edges of their launch geometry:
H = 1 and W = 1, the 8- and 16-pixel workgroups one short / exact / one over, the 4-byte route reached through
fsraft_set_upsample_kernel(0) and through each pointer of the two alignment tests in turn, four flow layouts through
flow_bs / cs / ps, mask planes with a dominant, an underflowing and equal taps; the bilinear pair at H = 1 / W = 1 and with a partial
workgroup; the loss at 255 / 256 / 257 pixels, 32 predictions, the second trip of its capped grid, null gt / valid / dpred entries,
metric_idx outside the predictions, the two launches of train._SemiLossFn; AdamW at n < 4, with and without the n & 3 tail, on the
second trip of its capped grid, with skip tables, from step 999 and 99999.  The test owns every buffer (_util.Buf: guard rows and
unwritten outputs hold a NaN pattern).  Needs an MI355X: -m gpu.

Limits: _tailref.LIMITS, set from the fp32 twins on the CPU (tests/test_tailref.py), not from the kernels.  profiles/
tail_kernel_margins.txt lists every comparison (FSRAFT_PARITY_LOG).  Worst values measured on MI355X, in the units of _tailref's scales:
  upsample up, by alignment = by setter                 0  exact      (1x2x9; offset off_up)
  upsample dmask / dflow, by alignment = by setter      0  exact      (1x2x9; offset off_mask)
  upsample up                                        4.57  limit 20   (1x2x33; gaussian interleaved_wide off_dmask)
  upsample dmask                                     6.89  limit 30   (1x3x16; gaussian interleaved_wide off_dmask)
  upsample dflow                                     1.13  limit 5    (2x3x17; dominant planar off_dmask)
  upflow8 up                                          1.5  limit 6    (1x2x2x2)
  upflow8 dflow                                     0.065  limit 3    (1x1x1x1)
  loss epe sum                                       1.35  limit 6    (2x5x7x32-none-True-False-0-inf-plain; launch 0)
  loss counts                                           0  exact      (1x513x1024x2-all-True-True-1-400.0-plain; launch 0)
  loss dpred                                         3.55  limit 20   (1x3x85x3-all-True-False-3-400.0-plain; launch 0 prediction 2)
  loss                                               1.77  limit 9    (1x257x1x3-all-True-True--1-400.0-semi; launch 1)
  adamw step count                                      0  exact      (4194311-above-0.01-all_three-0; step 3)
  adamw state                                       0.959  limit 6    (65-above-0.01-None-999; step 1000)
  adamw g = g * coef                                    0  exact      (4194311-above-0.01-all_three-0; step 3)
  adamw skipped blocks                                  0  exact      (4194311-above-0.01-all_three-0; step 3)
  adamw p                                            5.54  limit 30   (4194311-above-0.01-all_three-0; step 3)
  adamw m                                            2.94  limit 30   (65-above-0.01-None-999; step 1000)
  adamw v                                            5.42  limit 30   (4194304-above-0.01-None-0; step 3)
(exact rows: a count of mismatches, 0.  loss / upflow8 dflow rows are B x H x W x n and N x C x H x W.)  Two things first missed:
the 2048 unordered fp32 atomicAdds of sequence_loss_kernel reached 11.1 units on the loss of the 525312-pixel case (6.4 on another
run; limit 9) -- it now adds its workgroups' partial sums in float64, in workgroup order; and csrc/optim.hip formed 1 - beta2 and
1 - beta2^t from the fp32-rounded beta2 (216 units in v at step 1, 108 in inv_sqrt_bias2; test_tailref.py keeps the arithmetic) --
the betas now reach it as doubles.  upflow8_bwd_kernel's row / column range divided by a zero scale at H = 1 / W = 1 (undefined
conversions; an emulation gave dflow = 0): fixed before its first run, so no measured value of the old code exists.
"""
import ctypes
import functools

import pytest
import torch

import _tailref as R
from _util import Buf, PATTERN, _log_margin

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


def _nan_fill(n):
    return torch.full((n,), PATTERN, dtype=torch.int32).view(torch.float32)


def _ids(c):
    return "x".join(map(str, c)) if isinstance(c, tuple) else str(c)


class Tally:
    """The comparisons of one test: every figure is logged (the worst per output, with the variant it occurred in) before
    anything is asserted."""

    def __init__(self, case):
        self.case, self.worst, self.failed = case, {}, []

    def check(self, name, got, entry, variant=""):
        ref, scale, slack, key = entry
        w, i = R.need(got.reshape(ref.shape), ref, scale, slack)
        if w >= self.worst.get(name, (-1.0,))[0]:
            self.worst[name] = (w, R.LIMITS[key], variant)
        if not w <= R.LIMITS[key]:
            self.failed.append((name, variant, w, R.LIMITS[key], i))

    def exact(self, name, ok, variant=""):
        """A bit-for-bit or count comparison: no limit, logged as 0 / 1."""
        self.worst[name] = max(self.worst.get(name, (0.0, 0.0, "")), (0.0 if ok else 1.0, 0.0, variant))
        if not ok:
            self.failed.append((name, variant))

    def done(self):
        for name, (w, lim, variant) in sorted(self.worst.items()):
            _log_margin(f"{name} {self.case}", w, lim, f"worst (|got - ref| - slack) / scale, {variant}" if lim else f"exact, {variant}")
        assert not self.failed, (self.case, self.failed)


# ============================================================================================================ convex upsampler
@functools.lru_cache(maxsize=None)
def _up_case(case, kind):
    flow, mask, dup = R.flow_values(*case), R.mask_plane(kind, *case), R.dup_values(*case)
    return flow, mask, dup, R.upsample_expect(flow, mask, dup)


def _flow_buffer(flow, layout):
    """(flat CPU tensor, base offset in floats, bs, cs, ps): element (n, c, pix) at base + n bs + c cs + pix ps; every float
    that is no element holds the NaN pattern."""
    N, _, H, W = flow.shape
    HW = H * W
    f = flow.reshape(N, 2, HW)
    if layout == "planar":
        return f.reshape(-1).clone(), 0, 2 * HW, HW, 1
    if layout == "planar_gap":
        bs = 2 * HW + 8
        flat = _nan_fill(N * bs).clone()
        flat.view(N, bs)[:, :2 * HW] = f.reshape(N, 2 * HW)
        return flat, 0, bs, HW, 1
    if layout == "interleaved":
        return f.permute(0, 2, 1).reshape(-1).clone(), 0, 2 * HW, 1, 2
    flat = _nan_fill(N * HW * 6).clone()                # interleaved inside rows of six floats, the pair at floats 3 and 4
    flat.view(N, HW, 6)[:, :, 3:5] = f.permute(0, 2, 1)
    return flat, 3, 6 * HW, 1, 6


ROUTES = ("v4", "setter0", "off_mask", "off_up", "off_dup", "off_dmask")


def run_upsample(L, T, case, kind, layout, route):
    """fsraft_upsample_fwd and _bwd on one case; route: the 16-byte kernels, the 4-byte ones through the setter, or through one
    payload moved a float off its alignment.  Returns the raw outputs."""
    lib = L.load()
    N, H, W = case
    HW = H * W
    flow, mask, dup, exp = _up_case(case, kind)
    v = f"{kind} {layout} {route}"
    flat, base, bs, cs, ps = _flow_buffer(flow, layout)
    bf = Buf(flat)
    off = {r: int(route == r) for r in ROUTES}
    bm, bup = Buf(mask, offset=off["off_mask"]), Buf(n=N * 2 * 64 * HW, offset=off["off_up"])
    bdup, bdm = Buf(dup, offset=off["off_dup"]), Buf(n=N * HW * 576, offset=off["off_dmask"])
    bdf, bT = Buf(n=N * 2 * HW), Buf(n=18 * N * HW)
    try:
        if route == "setter0":
            assert lib.fsraft_set_upsample_kernel(0) == 0
        L.check(lib.fsraft_upsample_fwd(_p(L, bf, base), bs, cs, ps, _p(L, bm), _p(L, bup), N, H, W, L.stream()), "upsample_fwd")
        L.check(lib.fsraft_upsample_bwd(_p(L, bf, base), bs, cs, ps, _p(L, bm), _p(L, bdup), _p(L, bdm), _p(L, bdf), _p(L, bT), N, H, W,
                                        L.stream()), "upsample_bwd")
        torch.cuda.synchronize()
    finally:
        assert lib.fsraft_set_upsample_kernel(1) == 0
    bup.written(), bdm.written(), bdf.written(), bT.written()
    for b in (bf, bm, bdup):
        b.intact()
    assert _same_bits(bf.cpu(), flat) and _same_bits(bm.cpu(), mask.reshape(-1)) and _same_bits(bdup.cpu(), dup.reshape(-1)), "an input was written"
    out = dict(up=bup.cpu(), dmask=bdm.cpu(), dflow=bdf.cpu())
    for name in ("up", "dmask", "dflow"):
        T.check("upsample " + name, out[name], exp[name], v)
    return out


@pytest.mark.parametrize("case", R.UP_CASES, ids=_ids)
def test_convex_upsampler_vs_fp64(L, case):
    """Every mask plane and flow layout on both kernel pairs; then the 4-byte pair reached by alignment, one payload at a time:
    its bits are those of the setter's run (the same kernels), whichever of mask / up / dup / dmask decided."""
    T = Tally(_ids(case))
    for ki, kind in enumerate(R.UP_MASKS):
        by_setter = None
        for layout in R.UP_LAYOUTS:
            a = run_upsample(L, T, case, kind, layout, "v4")
            b = run_upsample(L, T, case, kind, layout, "setter0")
            by_setter = by_setter or b
            for name in a:                              # the layout of the flow does not change a bit of the result
                assert _same_bits(b[name], by_setter[name]), (kind, layout, name)
        for ri, route in enumerate(ROUTES[2:]):
            c = run_upsample(L, T, case, kind, R.UP_LAYOUTS[(ki + ri) % 4], route)
            fwd_moved, bwd_moved = route in ("off_mask", "off_up"), route != "off_up"
            if fwd_moved:
                T.exact("upsample up, by alignment = by setter", _same_bits(c["up"], by_setter["up"]), f"{kind} {route}")
            if bwd_moved:
                ok = _same_bits(c["dmask"], by_setter["dmask"]) and _same_bits(c["dflow"], by_setter["dflow"])
                T.exact("upsample dmask / dflow, by alignment = by setter", ok, f"{kind} {route}")
    T.done()


def test_convex_upsampler_refusals(L):
    lib = L.load()
    N, H, W = 1, 2, 3
    flow, mask, dup, _ = _up_case((1, 2, 9), "gaussian")
    bf, bm, bdup = Buf(flow), Buf(mask), Buf(dup)
    for hole, (n, h, w) in ((None, (N, 0, W)), (None, (N, H, 0)), (None, (0, H, W)), (0, (N, H, W)), (1, (N, H, W)), (2, (N, H, W))):
        out = Buf(n=N * 2 * 64 * H * W)
        a = [_p(L, bf), _p(L, bm), _p(L, out)]
        if hole is not None:
            a[hole] = None
        assert lib.fsraft_upsample_fwd(a[0], 2 * H * W, H * W, 1, a[1], a[2], n, h, w, L.stream()) == FS_ERR_ARG
        out.untouched()
    for hole, (n, h, w) in ((None, (N, 0, W)), (None, (N, H, 0)), (None, (0, H, W))) + tuple((i, (N, H, W)) for i in range(6)):
        outs = [Buf(n=N * H * W * 576), Buf(n=N * 2 * H * W), Buf(n=18 * N * H * W)]
        a = [_p(L, bf), _p(L, bm), _p(L, bdup)] + [_p(L, o) for o in outs]
        if hole is not None:
            a[hole] = None
        assert lib.fsraft_upsample_bwd(a[0], 2 * H * W, H * W, 1, *a[1:], n, h, w, L.stream()) == FS_ERR_ARG
        torch.cuda.synchronize()
        for o in outs:
            o.untouched()


# ================================================================================================================== bilinear x8
@pytest.mark.parametrize("case", R.UPFLOW_CASES, ids=_ids)
def test_upflow8_vs_fp64(L, case):
    """upflow8_fwd_kernel and upflow8_bwd_kernel; at H = 1 (W = 1) every fine row (column) sits on source row (column) 0."""
    lib = L.load()
    N, C, H, W = case
    flow, dup = R.upflow8_inputs(*case)
    exp = R.upflow8_expect(flow, dup)
    T = Tally(_ids(case))
    bf, bup = Buf(flow), Buf(n=N * C * 64 * H * W)
    L.check(lib.fsraft_upflow8_fwd(_p(L, bf), _p(L, bup), N, C, H, W, L.stream()), "upflow8_fwd")
    bup.written(), bf.intact()
    T.check("upflow8 up", bup.cpu(), exp["up"])
    bd, bdf = Buf(dup), Buf(n=N * C * H * W)
    L.check(lib.fsraft_upflow8_bwd(_p(L, bd), _p(L, bdf), N, C, H, W, L.stream()), "upflow8_bwd")
    bdf.written(), bd.intact()
    assert _same_bits(bf.cpu(), flow.reshape(-1)) and _same_bits(bd.cpu(), dup.reshape(-1)), "an input was written"
    T.check("upflow8 dflow", bdf.cpu(), exp["dflow"])
    T.done()


def test_upflow8_refusals(L):
    lib = L.load()
    src = Buf(torch.ones(2 * 64 * 6))
    for args in ((1, 2, 0, 3), (1, 2, 2, 0), (0, 2, 2, 3), (1, 0, 2, 3)):
        out = Buf(n=2 * 64 * 6)
        assert lib.fsraft_upflow8_fwd(_p(L, src), _p(L, out), *args, L.stream()) == FS_ERR_ARG
        assert lib.fsraft_upflow8_bwd(_p(L, src), _p(L, out), *args, L.stream()) == FS_ERR_ARG
        out.untouched()
    out = Buf(n=2 * 64 * 6)
    assert lib.fsraft_upflow8_fwd(None, _p(L, out), 1, 2, 2, 3, L.stream()) == FS_ERR_ARG
    assert lib.fsraft_upflow8_bwd(None, _p(L, out), 1, 2, 2, 3, L.stream()) == FS_ERR_ARG
    assert lib.fsraft_upflow8_fwd(_p(L, src), None, 1, 2, 2, 3, L.stream()) == FS_ERR_ARG
    assert lib.fsraft_upflow8_bwd(_p(L, src), None, 1, 2, 2, 3, L.stream()) == FS_ERR_ARG
    out.untouched()


# ================================================================================================================ sequence loss
def _ptr_array(L, ptrs):
    """(c_void_p array cast to the entry's pointer-to-pointer type, the array to keep alive); an entry None is NULL."""
    arr = (ctypes.c_void_p * len(ptrs))(*[p.value if p is not None else None for p in ptrs])
    return ctypes.cast(arr, L._PP), arr


def _loss_id(run):
    return _ids(run[0]) + "-" + "-".join(map(str, run[1:]))


@pytest.mark.parametrize("run", R.LOSS_RUNS, ids=_loss_id)
def test_sequence_loss_vs_fp64(L, run):
    """One launch, or the two of a `semi` row on the halves of buffers that hold 2B samples.  A dead dpred is left untouched, a
    live one is written everywhere (zeros where masked: the reference holds exact zeros there and the scale is u |ref|)."""
    lib = L.load()
    (B, H, W, n), live_kind, _, _, _, _, mode = run
    launches = R.loss_launches(run)
    k = len(launches)
    half = B * 2 * H * W                                # floats from sample 0 to sample B
    T = Tally(_loss_id(run))
    bp = [Buf(torch.cat([a["preds"][i] for a in launches])) for i in range(n)]
    bd = [Buf(n=k * half) for _ in range(n)]
    live = launches[0]["live"]
    bout = Buf(launches[0]["out0"]) if mode == "prefilled" else Buf(n=6 * k, zero=True)
    keep = []
    for j, a in enumerate(launches):
        bgt = Buf(a["gt"]) if a["gt"] is not None and j == 0 else None
        bva = Buf(a["valid"]) if a["valid"] is not None else None
        gt_ptr = _p(L, bgt) if j == 0 else _p(L, bp[n - 1], half)             # the second launch: its own last prediction
        pp, k1 = _ptr_array(L, [_p(L, b, j * half) for b in bp])
        dd, k2 = _ptr_array(L, [_p(L, b, j * half) if lv else None for b, lv in zip(bd, live)])
        w = (ctypes.c_float * n)(*[float(x) for x in a["w"]])
        keep += [bgt, bva, k1, k2, w]
        L.check(lib.fsraft_sequence_loss(pp, dd if any(live) else None, w, n, a["metric"], gt_ptr, _p(L, bva), a["max_flow"], R.LOSS_EPS,
                                         B, H, W, _p(L, bout, 6 * j), L.stream()), "sequence_loss")
    torch.cuda.synchronize()
    bout.written()
    for b, src in zip(bp, range(n)):
        b.intact()
        assert _same_bits(b.cpu(), torch.cat([a["preds"][src] for a in launches]).reshape(-1)), "a prediction was written"
    for b in keep:
        if isinstance(b, Buf):
            b.intact()
    for b, lv in zip(bd, live):
        b.written() if lv else b.untouched()
    out = bout.cpu().double()
    for j, a in enumerate(launches):
        exp = R.loss_expect_of(a)
        ref, scale = exp["out"]
        o = out[6 * j:6 * j + 6]
        v = f"launch {j}"
        T.check("loss", o[0], (ref[0], scale[0], 0.0, "loss"), v)
        T.check("loss epe sum", o[1], (ref[1], scale[1], 0.0, "epe"), v)
        T.exact("loss counts", torch.equal(o[2:], ref[2:]), v)
        for i, e in enumerate(exp["dpred"]):
            if e is not None:
                T.check("loss dpred", bd[i].cpu()[j * half:(j + 1) * half], e, f"{v} prediction {i}")
    T.done()


def test_sequence_loss_sums_are_the_same_bits_twice(L):
    """The 2048 workgroups of the second-trip case leave partial sums that one of them adds in workgroup order: two launches give
    the same six floats, whatever order the workgroups retired in."""
    lib = L.load()
    (B, H, W, n), _, _, _, metric, max_flow, _ = R.LOSS_RUNS[-1]
    a = R.loss_launches(R.LOSS_RUNS[-1])[0]
    bp, bgt, bva = [Buf(p) for p in a["preds"]], Buf(a["gt"]), Buf(a["valid"])
    pp, k1 = _ptr_array(L, [_p(L, b) for b in bp])
    w = (ctypes.c_float * n)(*[float(x) for x in a["w"]])
    outs = []
    for _ in range(2):
        bout = Buf(n=6, zero=True)
        L.check(lib.fsraft_sequence_loss(pp, None, w, n, metric, _p(L, bgt), _p(L, bva), max_flow, R.LOSS_EPS, B, H, W, _p(L, bout),
                                         L.stream()), "sequence_loss")
        torch.cuda.synchronize()
        bout.written()
        outs.append(bout.cpu())
    assert _same_bits(outs[0], outs[1]), outs


@pytest.mark.parametrize("n", (0, 33))
def test_sequence_loss_refuses_prediction_counts_outside_1_to_32(L, n):
    lib = L.load()
    src = Buf(torch.ones(2 * 6))
    outs = [Buf(n=2 * 6) for _ in range(max(n, 1))]
    out = Buf(n=6)
    pp, k1 = _ptr_array(L, [_p(L, src)] * max(n, 1))
    dd, k2 = _ptr_array(L, [_p(L, o) for o in outs])
    w = (ctypes.c_float * max(n, 1))(*([1.0] * max(n, 1)))
    assert lib.fsraft_sequence_loss(pp, dd, w, n, 0, None, None, 400.0, 1e-3, 1, 2, 3, _p(L, out), L.stream()) == FS_ERR_ARG
    torch.cuda.synchronize()
    out.untouched()
    for o in outs:
        o.untouched()


# ======================================================================================================================== AdamW
def _adamw_id(run):
    return "-".join(map(str, run))


def _adamw_call(L, bufs, n, bstep, bnorm, blr, wd, bstate, skip):
    p, g, m, v = bufs
    return L.load().fsraft_adamw_flat(_p(L, p), _p(L, g), _p(L, m), _p(L, v), n, _p(L, bstep), _p(L, bnorm), R.MAX_NORM, _p(L, blr),
                                      R.BETAS[0], R.BETAS[1], R.ADAM_EPS, wd, _p(L, bstate),
                                      ctypes.c_void_p(skip.data_ptr()) if skip is not None else None, L.stream())


@pytest.mark.parametrize("run", R.ADAMW_RUNS, ids=_adamw_id)
def test_adamw_three_steps_vs_fp64(L, run):
    """Three consecutive steps; every step's reference starts from what the kernel left (p, m, v, the step count) and a fresh
    gradient, so one step's rounding is what is compared.  g: bits of the fp32 product with the kernel's own coef; skipped
    64-blocks: every buffer's bits."""
    n, norm_kind, wd, skip_kind, step0 = run
    T = Tally(_adamw_id(run))
    p0, _, m0, v0 = R.adamw_inputs(n)
    bufs = [Buf(p0), Buf(n=n, zero=True), Buf(m0), Buf(v0)]
    bstep, blr, bstate = Buf(torch.tensor([float(step0)])), Buf(n=1, zero=True), Buf(n=4)
    bnorm = Buf(n=1, zero=True) if norm_kind != "none" else None
    nb = (n + 63) // 64
    bskip = Buf(n=(nb + 3) // 4, zero=True) if skip_kind else None
    skip = bskip.mid.view(torch.uint8)[:nb] if skip_kind else None
    step = float(step0)
    for k in range(3):
        g, norm, lr, wd_k, table = R.adamw_step_setup(run, k)
        bufs[1].mid.copy_(g)
        blr.mid.fill_(lr)
        if bnorm is not None:
            bnorm.mid.copy_(norm.reshape(1))
        if skip is not None:
            skip.copy_(table)
        before = [b.cpu() for b in bufs]
        lr32 = float(blr.cpu()[0])
        L.check(_adamw_call(L, bufs, n, bstep, bnorm, blr, wd_k, bstate, skip), "adamw_flat")
        torch.cuda.synchronize()
        for b in bufs + [bstep, blr, bstate] + [x for x in (bnorm, bskip) if x is not None]:
            b.intact()
        bstate.written()
        after = [b.cpu() for b in bufs]
        st = bstate.cpu()
        exp = R.adamw_expect(before[0], g, before[2], before[3], step, norm, R.MAX_NORM, lr, R.BETAS, R.ADAM_EPS, wd_k, table)
        v = f"step {int(step) + 1}"
        T.exact("adamw step count", float(bstep.cpu()[0]) == exp["step"], v)
        T.check("adamw state", st, exp["state"], v)
        kept = exp["keep"]
        T.exact("adamw g = g * coef", _same_bits(after[1], torch.where(kept, g, g * st[0])), v)
        for name, i in (("p", 0), ("m", 2), ("v", 3)):
            T.check("adamw " + name, after[i], exp[name], v)
        if table is not None:
            ok = all(_same_bits(after[i][kept], before[i][kept]) for i in range(4))
            T.exact("adamw skipped blocks", ok, v)
            nxt = torch.zeros_like(kept)
            nxt[1:] |= kept[:-1]
            nxt[:-1] |= kept[1:]
            nxt &= ~kept
            assert bool(nxt.any()) and not bool((after[0][nxt] == before[0][nxt]).any()), "a neighbour of a skipped block did not update"
        assert abs(lr32 - lr) <= R.U24 * lr
        step = exp["step"]
    T.done()


@pytest.mark.parametrize("which", range(4), ids=("p", "g", "m", "v"))
def test_adamw_refuses_a_misaligned_buffer(L, which):
    n = 65
    src = [torch.full((n,), 0.5 + i) for i in range(4)]
    bufs = [Buf(s, offset=int(i == which)) for i, s in enumerate(src)]
    bstep, blr, bstate = Buf(torch.zeros(1)), Buf(torch.full((1,), 0.01)), Buf(n=4)
    assert _adamw_call(L, bufs, n, bstep, None, blr, 0.0, bstate, None) == FS_ERR_ARG
    torch.cuda.synchronize()
    for b, s in zip(bufs, src):
        b.intact()
        assert _same_bits(b.cpu(), s)
    assert float(bstep.cpu()[0]) == 0.0
    bstate.untouched()
    assert L.load().fsraft_adamw_flat(_p(L, bufs[which]), None, None, None, 0, None, None, 1.0, None, 0.9, 0.999, 1e-8, 0.0, None, None,
                                      L.stream()) == FS_ERR_ARG
