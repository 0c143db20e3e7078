"""csrc/flow_loss.hip (fsraft_flow_loss) called through the C ABI on tests/_util.Buf buffers -- guard rows and unwritten outputs hold
the NaN pattern -- against the float64 restatement of tests/_flowlossref.py, within its LIMITS (4 x what the fp32 twin needs on
these very launches; tests/test_flowlossref.py).  Every penalty at every case: one pixel, the workgroup edge at 255 / 256 / 257
pixels, 32 predictions, three samples with a partial last workgroup each, and 2048 x 256 + 1024 pixels for the strided second trip.
At 2x5x7x3 and 1x257x1x2 the variants are crossed: NHWC and planar, bases 0 / 1 / 2 floats off the 16-byte alignment (1 takes the
4-byte route, 0 and 2 the 8-byte one), the ground truth as one three-channel tensor read in place / with a separate mask / without a
mask / without a target, null dpred entries, the statistics on and off, both scales, and the per-pixel map at n = 1.
Asserted exactly: gradient 0 where m = 0, gradient 0 at d = 0 under l1, the pixel of magnitude 400.0 excluded, the mask sums,
nothing written outside the outputs, the workspace's counter left zero, the same bits twice.  Every comparison goes to the parity
log (FSRAFT_PARITY_LOG; profiles/flow_loss_margins.txt).  Worst values measured on MI355X, in the units of _flowlossref's scales:
  loss       3.42  limit 9    (1x255x1x2 robust)          epe sums   1.22  limit 9    (3x9x31x2)
  dpred      2.99  limit 20   (1x257x1x2 robust)          pixel map  2.87  limit 20   (1x257x1x2 l2 nhwc)
  exact rows (zeros where m = 0, sign(0), the 400.0 pixel, mask sums): no mismatch.  The kernel sets none of the limits."""
import ctypes
import functools
import itertools

import pytest
import torch

import _flowlossref as R
import _tailref
from _util import Buf, _log_margin

pytestmark = pytest.mark.gpu
PEN = {"l1": 0, "l2": 1, "robust": 2}


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


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _ptr(L, b, lo=0):
    return L.ptr(b.mid[lo:]) if b is not None else None


def _ptr_array(L, ptrs):
    arr = (ctypes.c_void_p * len(ptrs))(*[q.value if q is not None else None for q in ptrs])
    return ctypes.cast(arr, L._PP), arr


class Tally:
    """The comparisons of one test: the worst figure per output is logged, with the variant it occurred in, before anything is
    asserted."""

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
        self.worst[name] = max(self.worst.get(name, (0.0, 0.0, "")), (0.0 if ok else 1.0, 0.0, variant))
        if not ok:
            self.failed.append((name, variant))

    def done(self):
        for name, (w, lim, variant) in sorted(self.worst.items()):
            _log_margin(f"{name} {self.case}", w, lim, f"worst (|got - ref| - slack) / scale, {variant}" if lim else f"exact, {variant}")
        assert not self.failed, (self.case, self.failed[:8])


def _in_layout(t, layout):
    """A canonical [B,H,W,C] CPU tensor as the flat memory of `layout`."""
    return (t if layout == "nhwc" else t.permute(0, 3, 1, 2)).contiguous().reshape(-1)


def _from_layout(flat, layout, B, H, W):
    return flat.view(B, H, W, 2) if layout == "nhwc" else flat.view(B, 2, H, W).permute(0, 2, 3, 1)


class Inputs:
    """The device buffers of one (case, layout, offset): predictions, the [.,3] ground truth, the target and the mask alone."""

    def __init__(self, case, layout, offset):
        B, H, W, n = case
        self.case, self.layout, self.offset = case, layout, offset
        preds, target, mask, w = R.inputs(B, H, W, n)
        self.src = [_in_layout(q, layout) for q in preds]
        self.preds = [Buf(s, offset=offset) for s in self.src]
        self.joint = Buf(_in_layout(torch.cat((target, mask[..., None]), 3), layout), offset=offset)
        self.target = Buf(_in_layout(target, layout), offset=offset)
        self.mask = Buf(mask, offset=offset)
        self.w = w
        HW = H * W
        self.pstr = (2 * HW, 1, 2) if layout == "nhwc" else (2 * HW, HW, 1)

    def operands(self, L, gt_form):
        """(target pointer, its strides, mask pointer, its strides)"""
        B, H, W, _ = self.case
        HW = H * W
        if gt_form == "joint":
            if self.layout == "nhwc":
                return _ptr(L, self.joint), (3 * HW, 1, 3), _ptr(L, self.joint, 2), (3 * HW, 3)
            return _ptr(L, self.joint), (3 * HW, HW, 1), _ptr(L, self.joint, 2 * HW), (3 * HW, 1)
        t = None if gt_form == "null_target" else _ptr(L, self.target)
        m = None if gt_form == "null_mask" else _ptr(L, self.mask)
        return t, (self.pstr if t is not None else (0, 0, 0)), m, ((HW, 1) if m is not None else (0, 0))

    def unchanged(self):
        for b, s in zip(self.preds, self.src):
            b.intact()
            assert _same_bits(b.cpu(), s), "a prediction was written"
        for b in (self.joint, self.target, self.mask):
            b.intact()


def run(L, inp, penalty, gt_form="joint", live="all", metric=True, scale="mean", single=False, ws=None, stream=None):
    """One launch -> dict(out [1], dpred [n] canonical [B,H,W,2] or None, stats [B,2] or None, pixel [B,H,W] or None).  single: the
    first prediction alone, with the per-pixel map.  The outputs are fresh pattern-filled buffers; every one is checked for having
    been written whole, or not at all, with its guard rows intact."""
    lib = L.load()
    B, H, W, n = inp.case
    n = 1 if single else n
    lv = R.live_list(live, n)
    dp = [Buf(n=2 * B * H * W, offset=inp.offset) if x else None for x in lv]
    out, stats = Buf(n=1), (Buf(n=2 * B) if metric else None)
    pix = Buf(n=B * H * W) if single else None
    nbytes = lib.fsraft_flow_loss_workspace_bytes(B, H, W)
    ws = Buf(n=nbytes // 4, zero=True) if ws is None else ws
    pp, k1 = _ptr_array(L, [_ptr(L, b) for b in inp.preds[:n]])
    dd, k2 = _ptr_array(L, [_ptr(L, b) for b in dp])
    w = (ctypes.c_float * n)(*([1.0] if single else [float(x) for x in inp.w]))
    t, ts, m, ms = inp.operands(L, gt_form)
    if stream is not None:
        torch.cuda.synchronize()                        # the buffers were filled on the current stream
    L.check(lib.fsraft_flow_loss(pp, dd if any(lv) else None, w, n, *inp.pstr, t, *ts, m, *ms, PEN[penalty], R.MAX_FLOW, R.EPS,
                                 R.scale_of(scale, B, H, W), B, H, W, _ptr(L, out), _ptr(L, stats), (n - 1) if metric else -1, _ptr(L, pix),
                                 _ptr(L, ws), nbytes, stream if stream is not None else L.stream()), "flow_loss")
    if stream is not None:
        return dict(out=out, stats=stats, ws=ws, keep=(k1, k2, w, dp))
    torch.cuda.synchronize()
    out.written()
    ws.intact()
    assert int(ws.mid[:1].view(torch.int32)) == 0, "the arrival counter was not left zero"
    for b in dp:
        if b is not None:
            b.written()
    res = dict(out=out.cpu().double(), dpred=[_from_layout(b.cpu(), inp.layout, B, H, W) if b is not None else None for b in dp],
               stats=None, pixel=None)
    if metric:
        stats.written()
        res["stats"] = stats.cpu().double().view(B, 2)
    if single:
        pix.written()
        res["pixel"] = pix.cpu().view(B, H, W)
    return res


@functools.lru_cache(maxsize=None)
def _expect(case, penalty, gt_form, live, metric, scale, single=False):
    preds, w, target, mask, sc, lv, mi = R.launch_args(case, gt_form, live, metric, scale, single)
    return R.expect(preds, w, target, mask, penalty, sc, lv, mi)


def compare(T, res, exp, penalty, gt_form, case, variant):
    B, H, W, _ = case
    T.check("loss", res["out"][0], exp["loss"], variant)
    dead = (exp["m"] == 0)[..., None].expand(B, H, W, 2)
    for i, (d, e) in enumerate(zip(res["dpred"], exp["dpred"])):
        assert (d is None) == (e is None)
        if e is None:
            continue
        T.check("dpred", d, e, f"{variant} prediction {i}")
        T.exact("dpred is 0 where m is 0", bool((d[dead] == 0).all()), variant)
        if H * W >= 8:
            if gt_form != "null_target":
                T.exact("the pixel of magnitude 400.0 is excluded", bool((d.reshape(B, -1, 2)[0, 1] == 0).all()), variant)
            if penalty == "l1" and gt_form != "null_target":              # (without a target d is the prediction itself, not 0)
                T.exact("l1 gradient is 0 at d = 0", bool((d.reshape(B, -1, 2)[0, 0] == 0).all()), variant)
    if exp["epe"] is not None and res["stats"] is not None:
        T.check("epe sums", res["stats"][:, 0], exp["epe"], variant)
        T.exact("mask sums", torch.equal(res["stats"][:, 1], exp["msum"]), variant)
    if res["pixel"] is not None:
        T.check("pixel map", res["pixel"], exp["pixel"], variant)
        T.exact("pixel map is 0 where m is 0", bool((res["pixel"][exp["m"] == 0] == 0).all()), variant)


@pytest.mark.parametrize("penalty", R.PENALTIES)
@pytest.mark.parametrize("case", R.CASES, ids=_ids)
def test_flow_loss_vs_fp64(L, case, penalty):
    """NHWC, the ground truth read in place from its three-channel tensor, every gradient, the statistics of the last prediction,
    Keras' mean; with one prediction, the per-pixel map as well."""
    inp = Inputs(case, "nhwc", 0)
    T = Tally(f"{_ids(case)} {penalty}")
    single = case[3] == 1
    res = run(L, inp, penalty, single=single)
    compare(T, res, _expect(case, penalty, "joint", "all", True, "mean", single), penalty, "joint", case, "nhwc joint all mean")
    inp.unchanged()
    T.done()


@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("penalty", R.PENALTIES)
@pytest.mark.parametrize("case", R.CROSSED, ids=_ids)
def test_flow_loss_crossed_variants_vs_fp64(L, case, penalty, layout):
    T = Tally(f"{_ids(case)} {penalty} {layout}")
    for offset in R.OFFSETS:
        inp = Inputs(case, layout, offset)
        for gt_form, live, metric, scale in R.crossed_variants():
            v = f"offset {offset} {gt_form} {live} {'stats' if metric else 'nostats'} {scale}"
            compare(T, run(L, inp, penalty, gt_form, live, metric, scale), _expect(case, penalty, gt_form, live, metric, scale),
                    penalty, gt_form, case, v)
        for gt_form, scale in itertools.product(R.GT_FORMS, R.SCALES):             # the per-pixel map: one prediction
            v = f"offset {offset} {gt_form} n=1 {scale}"
            compare(T, run(L, inp, penalty, gt_form, "all", True, scale, single=True),
                    _expect(case, penalty, gt_form, "all", True, scale, True), penalty, gt_form, case, v)
        inp.unchanged()
    T.done()


@pytest.mark.parametrize("case", (R.BIG, (3, 9, 31, 2)), ids=_ids)
def test_flow_loss_sums_are_the_same_bits_twice(L, case):
    """The workgroups leave partial sums that the last one adds in workgroup order: two launches -- on ONE workspace, whose counter
    the first left zero -- give the same loss and the same per-sample sums, whatever order the workgroups retired in."""
    inp = Inputs(case, "nhwc", 0)
    B, H, W, _ = case
    ws = Buf(n=L.load().fsraft_flow_loss_workspace_bytes(B, H, W) // 4, zero=True)
    a, b = (run(L, inp, "l2", live="none", ws=ws) for _ in range(2))
    assert _same_bits(a["out"].float(), b["out"].float()) and _same_bits(a["stats"].float(), b["stats"].float()), (a, b)
    inp.unchanged()


def test_two_launches_on_two_streams_do_not_disturb_each_other(L):
    """Two workspaces, two streams, no ordering between them: each launch gives the bits it gives alone."""
    inp = Inputs(R.BIG, "nhwc", 0)
    alone = run(L, inp, "l2", live="none")
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(2)]
    got = [run(L, inp, "l2", live="none", stream=ctypes.c_void_p(s.cuda_stream)) for s in streams]
    torch.cuda.synchronize()
    for g in got:
        g["out"].written()
        g["stats"].written()
        g["ws"].intact()
        assert _same_bits(g["out"].cpu(), alone["out"].float()) and _same_bits(g["stats"].cpu().view(1, 2), alone["stats"].float())
    inp.unchanged()


@pytest.mark.parametrize("case", ((2, 5, 7, 3), (3, 9, 31, 2)), ids=_ids)
def test_robust_planar_mean_and_fsraft_sequence_loss_meet_the_same_fp64_result(L, case):
    """ROBUST, planar, scale 1 / (2 B H W), a 0 / 1 mask: the objective csrc/loss.hip computes.  The new entry and
    fsraft_sequence_loss are each held to the float64 result of this case, by the limits each has (the scales are the same:
    u * loss for the sum of positive terms, u * |ref| for a gradient)."""
    lib = L.load()
    B, H, W, n = case
    preds, target, mask, w = R.inputs(B, H, W, n)
    valid = (mask >= 0.5).float()
    exp = R.expect(preds, w, target, valid, "robust", R.scale_of("mean", B, H, W))
    T = Tally(f"{_ids(case)} robust planar against loss.hip")
    bp = [Buf(_in_layout(q, "nchw")) for q in preds]
    bt, bv = Buf(_in_layout(target, "nchw")), Buf(valid)
    pp, k1 = _ptr_array(L, [_ptr(L, b) for b in bp])
    wa = (ctypes.c_float * n)(*[float(x) for x in w])
    HW = H * W
    # the new entry
    dn, on = [Buf(n=2 * B * HW) for _ in range(n)], Buf(n=1)
    nbytes = lib.fsraft_flow_loss_workspace_bytes(B, H, W)
    ws = Buf(n=nbytes // 4, zero=True)
    dd, k2 = _ptr_array(L, [_ptr(L, b) for b in dn])
    L.check(lib.fsraft_flow_loss(pp, dd, wa, n, 2 * HW, HW, 1, _ptr(L, bt), 2 * HW, HW, 1, _ptr(L, bv), HW, 1, PEN["robust"], R.MAX_FLOW, R.EPS,
                                 R.scale_of("mean", B, H, W), B, H, W, _ptr(L, on), None, -1, None, _ptr(L, ws), nbytes, L.stream()), "flow_loss")
    # the parent's
    do, oo = [Buf(n=2 * B * HW) for _ in range(n)], Buf(n=6, zero=True)
    de, k3 = _ptr_array(L, [_ptr(L, b) for b in do])
    L.check(lib.fsraft_sequence_loss(pp, de, wa, n, -1, _ptr(L, bt), _ptr(L, bv), R.MAX_FLOW, R.EPS, B, H, W, _ptr(L, oo), L.stream()),
            "sequence_loss")
    torch.cuda.synchronize()
    on.written()
    oo.written()
    ref, scale = exp["loss"][0], exp["loss"][1]
    T.check("loss (flow_loss)", on.cpu().double()[0], exp["loss"])
    old = R.need(oo.cpu().double()[0], ref, scale)[0]
    _log_margin(f"loss (sequence_loss) {T.case}", old, _tailref.LIMITS["loss"], "worst |got - ref| / scale, limit of tests/_tailref.py")
    assert old <= _tailref.LIMITS["loss"], old
    for i, e in enumerate(exp["dpred"]):
        dn[i].written()
        do[i].written()
        T.check("dpred (flow_loss)", _from_layout(dn[i].cpu(), "nchw", B, H, W), e, f"prediction {i}")
        old = R.need(_from_layout(do[i].cpu(), "nchw", B, H, W), e[0], e[1])[0]
        _log_margin(f"dpred (sequence_loss) {T.case} prediction {i}", old, _tailref.LIMITS["dpred"], "limit of tests/_tailref.py")
        assert old <= _tailref.LIMITS["dpred"], (i, old)
    T.done()
