"""The kernels of csrc/norm_cl.hip (channels-last instance norm / frozen-BatchNorm affine + ReLU + residual, forward and backward,
the BatchNorm fold) and of csrc/norm.hip (the NCHW four) called through their C entry points, each against its float64
restatement (tests/_normref.py) on the designed planes, at every edge of their launch geometry: C / 4 that does not divide 256
(idle tail threads), one pixel per thread and empty lanes (C = 4), strips of 128 pixels one short / exact / one over, nine
workgroups on eight partial rows, PIX_PER_WG 192 and 1024 through fsraft_set_norm_blocks, the space-to-depth addressing in both
directions, partial rows handed in (have_sums), the second trip of the affine forward's capped grid, the scalar route of the
NCHW kernels from a misaligned base.  The test owns every buffer: each sits between two guard rows of the NaN pattern 0x7FC0FFEE,
outputs are pre-filled with it, and afterwards the guards are intact and no pattern is left inside an output.  Needs an MI355X: -m gpu.

Limits: _normref.LIMITS, set from the fp32 twins on the CPU (tests/test_normref.py), not from the kernels.  profiles/
norm_kernel_margins.txt lists every comparison (FSRAFT_PARITY_LOG).  Worst values measured on MI355X, in the units of _normref's scales:
  affine_cl dsum_g                           1.01  limit 20  (2x13x10x252; relu=0 res=1 cbias=0)
  affine_cl dsum_gx                          3.04  limit 20  (2x13x10x252; relu=0 res=0 cbias=0)
  affine_cl dx                              0.999  limit 1   (2x42x50x100 s2d; relu=1 res=1 cbias=1)
  affine_cl y                               0.993  limit 4   (2x42x50x100 s2d; relu=0 res=1 cbias=0)
  bn_fold rmc                               0.989  limit 10  (2x13x10x256; relu=1 res=1 cbias=1)
  bn_fold rs                                 1.56  limit 10  (2x13x10x100; relu=1 res=1 cbias=1)
  bn_fold scale                              2.07  limit 10  (2x13x10x252; relu=1 res=1 cbias=0)
  bn_fold shift                              2.48  limit 10  (1x132x250x256; relu=1 res=1 cbias=1)
  bn_fold_bwd dbias                          2.38  limit 9   (2x26x10x100 s2d; relu=0 res=0 cbias=0)
  bn_fold_bwd dcbias                         2.42  limit 9   (2x42x50x100 s2d; relu=1 res=1 cbias=1)
  bn_fold_bwd dweight                        3.38  limit 9   (3x41x25x64; relu=1 res=1 cbias=1)
  inorm_cl dx                                4.82  limit 20  (3x41x25x64 alternating; relu=1 res=1 have_sums)
  inorm_cl mean                              5.41  limit 20  (2x13x10x252; relu=1 res=1)
  inorm_cl rstd                              5.16  limit 20  (3x41x25x64 alternating; relu=0 res=0 have_sums)
  inorm_cl s1                                1.99  limit 20  (2x4x6x64 s2d; relu=1 res=0)
  inorm_cl s2                                1.31  limit 20  (2x3x43x64; relu=1 res=1)
  inorm_cl sums                              5.32  limit 20  (2x13x10x252; relu=1 res=1)
  inorm_cl sumsq                             3.48  limit 20  (2x13x10x256; relu=1 res=1)
  inorm_cl y                                 4.16  limit 20  (3x41x25x64 alternating; relu=0 res=0 have_sums)
  inorm_cl y, have_sums against own pass     4.53  limit 20  (3x41x25x64 alternating; relu=0 res=0)
  affine dsum_g                             0.873  limit 20  (2x3x1; relu=0)
  affine dsum_gx                             1.54  limit 20  (2x3x3; relu=0)
  affine dx                                 0.998  limit 1   (2x3x46000; relu=0)
  affine y                                  0.951  limit 4   (2x5x640; relu=1)
  inorm dx                                   1.63  limit 7   (2x3x46000; relu=0)
  inorm mean                                 7.57  limit 9   (2x3x46000; relu=1)
  inorm rstd                                 2.33  limit 7   (2x3x46000; relu=1)
  inorm y                                    7.56  limit 9   (2x3x46000; relu=1)
(inorm_cl / affine_cl: norm_cl.hip, the case is B x H x W x C; inorm / affine: norm.hip, B x C x HW.)  The channels-last statistics
first missed their limit: see cl_reduce_lanes in csrc/norm_cl.hip."""
import functools
import itertools

import pytest
import torch

import _normref as R
from _util import Buf, _log_margin

pytestmark = pytest.mark.gpu
DEV = "cuda"
FS_ERR_ARG = 1
VARIANTS = tuple(itertools.product((0, 1), (False, True)))          # (relu, with residual)


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

    def done(self):
        for name, (w, lim, variant) in sorted(self.worst.items()):
            _log_margin(f"{name} {self.case}", w, lim, f"worst (|got - ref| - slack) / scale, {variant}")
        assert not self.failed, (self.case, self.failed)


def _layout(flat, shape, s2d):
    B, C, H, W = shape
    return R.from_s2d(flat, B, H, W, C) if s2d else R.from_cl(flat, B, H, W, C)


def _store(t, s2d):
    return R.to_s2d(t) if s2d else R.to_cl(t)


@functools.lru_cache(maxsize=8)
def _inputs(shape):
    return R.designed(*shape), R.gradients(*shape), R.residual(*shape)


# ----------------------------------------------------------------------------------------------- channels-last instance norm
def run_cl_inorm(L, T, shape, relu, with_res, s2d, have=None):
    """fsraft_inorm_relu_cl_fwd, then _bwd from its own stats and y.  have: partial rows (sums, sumsq) [B * 8, C] to hand in.
    Returns the raw outputs."""
    lib = L.load()
    B, C, H, W = shape
    HW, n, s2w = H * W, B * C * H * W, (W if s2d else 0)
    x, g, res = _inputs(shape)
    res = res if with_res else None
    v = f"relu={relu} res={int(with_res)}" + (" have_sums" if have else "")
    bx, br = Buf(R.to_cl(x)), (Buf(R.to_cl(res)) if with_res else None)
    by, stats = Buf(n=n), Buf(n=B * C * 2)
    sums, sumsq = (Buf(have[0]), Buf(have[1])) if have else (Buf(n=B * 8 * C, zero=True), Buf(n=B * 8 * C, zero=True))
    L.check(lib.fsraft_inorm_relu_cl_fwd(_p(L, bx), _p(L, br), _p(L, by), _p(L, sums), _p(L, sumsq), _p(L, stats), B, HW, C, R.EPS,
                                         relu, int(bool(have)), s2w, L.stream()), "inorm_relu_cl_fwd")
    by.written(), stats.written(), sums.written(), sumsq.written()
    yflat, st = by.cpu(), stats.cpu().view(B, C, 1, 1, 2)
    y = _layout(yflat, shape, s2d)
    exp = R.inorm_expect(x, g, R.EPS, relu, res, "cl", y if with_res else None)
    T.check("inorm_cl y", y, exp["y"], v)
    T.check("inorm_cl mean", st[..., 0], exp["mean"], v)
    T.check("inorm_cl rstd", st[..., 1], exp["rstd"], v)
    if have:
        assert _same_bits(sums.cpu(), have[0].reshape(-1)) and _same_bits(sumsq.cpu(), have[1].reshape(-1)), "have_sums: the rows were written"
    else:
        T.check("inorm_cl sums", sums.cpu().double().view(B, 8, C).sum(1), exp["sums"], v)
        T.check("inorm_cl sumsq", sumsq.cpu().double().view(B, 8, C).sum(1), exp["sumsq"], v)
    bg = Buf(_store(g, s2d))
    s1, s2, bdx = Buf(n=B * 8 * C, zero=True), Buf(n=B * 8 * C, zero=True), Buf(n=n)
    bdres = Buf(n=n) if with_res else None
    L.check(lib.fsraft_inorm_relu_cl_bwd(_p(L, bg), _p(L, bx), _p(L, stats), _p(L, by) if with_res else None, _p(L, s1), _p(L, s2),
                                         _p(L, bdx), _p(L, bdres), B, HW, C, relu, s2w, L.stream()), "inorm_relu_cl_bwd")
    bdx.written(), s1.written(), s2.written()
    for b in (bx, br, by, stats, bg):
        if b is not None:
            b.intact()
    assert _same_bits(by.cpu(), yflat) and _same_bits(bx.cpu(), R.to_cl(x)), "the backward wrote an input"
    dxflat = bdx.cpu()
    T.check("inorm_cl dx", R.from_cl(dxflat, B, H, W, C), exp["dx"], v)
    T.check("inorm_cl s1", s1.cpu().double().view(B, 8, C).sum(1), exp["s1"], v)
    T.check("inorm_cl s2", s2.cpu().double().view(B, 8, C).sum(1), exp["s2"], v)
    dresflat = None
    if with_res:
        bdres.written()
        dresflat = bdres.cpu()
        assert _same_bits(R.from_cl(dresflat, B, H, W, C), torch.where(y > 0, g, torch.zeros_like(g))), f"dres is g where out > 0 ({v})"
    return dict(y=yflat, stats=stats.cpu(), dx=dxflat, dres=dresflat)


# --------------------------------------------------------------------------------------------- channels-last affine and fold
def run_fold(L, T, B, C, cbias, v):
    """fsraft_bn_fold on _normref.bn_params; returns (the Buf holding scale, shift, rs, rmc, their CPU copies [4, C])."""
    lib = L.load()
    par = R.bn_params(B, C, cbias)
    bufs = [Buf(p) if p is not None else None for p in par]
    fold = Buf(n=4 * C)
    L.check(lib.fsraft_bn_fold(*[_p(L, b) for b in bufs], R.EPS, C, _p(L, fold), _p(L, fold, C), _p(L, fold, 2 * C), _p(L, fold, 3 * C),
                               L.stream()), "bn_fold")
    fold.written()
    f = fold.cpu().view(4, C)
    exp = R.fold_expect(*par, R.EPS)
    for i, name in enumerate(("scale", "shift", "rs", "rmc")):
        T.check("bn_fold " + name, f[i], exp[name], v)
    assert bool((f[1][(R.plane_kinds(B, C) == 6).any(0)] == 0).all()), "the designed zero shifts"
    return fold, f


def run_cl_affine(L, T, shape, relu, with_res, s2d, cbias, backward=True):
    """fsraft_bn_fold, fsraft_affine_relu_cl_fwd on its scale / shift, then _bwd and fsraft_bn_fold_bwd on its partial rows."""
    lib = L.load()
    B, C, H, W = shape
    HW, n, s2w = H * W, B * C * H * W, (W if s2d else 0)
    x, g, res = _inputs(shape)
    res = res if with_res else None
    v = f"relu={relu} res={int(with_res)} cbias={int(cbias)}"
    fold, f = run_fold(L, T, B, C, cbias, v)
    bx, br, by = Buf(R.to_cl(x)), (Buf(R.to_cl(res)) if with_res else None), Buf(n=n)
    L.check(lib.fsraft_affine_relu_cl_fwd(_p(L, bx), _p(L, br), _p(L, fold), _p(L, fold, C), _p(L, by), B * HW, C, relu, HW, s2w,
                                          L.stream()), "affine_relu_cl_fwd")
    by.written()
    yflat = by.cpu()
    y = _layout(yflat, shape, s2d)
    exp = R.affine_expect(x, g, f[0], f[1], relu, res, y if with_res else None)
    T.check("affine_cl y", y, exp["y"], v)
    if not backward:
        return dict(y=yflat)
    bg, bdx, part = Buf(_store(g, s2d)), Buf(n=n), Buf(n=2 * B * 8 * C, zero=True)
    bdres = Buf(n=n) if with_res else None
    L.check(lib.fsraft_affine_relu_cl_bwd(_p(L, bg), _p(L, bx), _p(L, fold), _p(L, fold, C), _p(L, by) if with_res else None, _p(L, bdx),
                                          _p(L, bdres), _p(L, part), _p(L, part, B * 8 * C), B, HW, C, relu, s2w, L.stream()),
            "affine_relu_cl_bwd")
    bdx.written(), part.written()
    for b in (bx, br, by, bg, fold):
        if b is not None:
            b.intact()
    assert _same_bits(by.cpu(), yflat) and _same_bits(fold.cpu().view(4, C), f), "the backward wrote an input"
    dxflat, rows = bdx.cpu(), part.cpu().view(2, B * 8, C)
    T.check("affine_cl dx", R.from_cl(dxflat, B, H, W, C), exp["dx"], v)
    T.check("affine_cl dsum_g", rows[0].double().sum(0), exp["dsum_g"], v)
    T.check("affine_cl dsum_gx", rows[1].double().sum(0), exp["dsum_gx"], v)
    if with_res:
        bdres.written()
        assert _same_bits(R.from_cl(bdres.cpu(), B, H, W, C), torch.where(y > 0, g, torch.zeros_like(g))), f"dres is g where out > 0 ({v})"
    dpar = Buf(n=3 * C)
    L.check(lib.fsraft_bn_fold_bwd(_p(L, part), B * 8, C, _p(L, fold, 2 * C), _p(L, fold, 3 * C), _p(L, fold), _p(L, dpar), _p(L, dpar, C),
                                   _p(L, dpar, 2 * C) if cbias else None, L.stream()), "bn_fold_bwd")
    dpar.written(3 * C if cbias else 2 * C)
    d = dpar.cpu().view(3, C)
    bexp = R.fold_bwd_expect(rows, f[2], f[3], f[0])
    for i, name in enumerate(("dweight", "dbias", "dcbias")[:3 if cbias else 2]):
        T.check("bn_fold_bwd " + name, d[i], bexp[name], v)
    return dict(y=yflat, dx=dxflat)


def _whole_case(L, case, s2d):
    B, H, W, C = case
    shape = (B, C, H, W)
    T = Tally("x".join(map(str, case)) + (" s2d" if s2d else ""))
    for relu, with_res in VARIANTS:
        run_cl_inorm(L, T, shape, relu, with_res, s2d)
        run_cl_affine(L, T, shape, relu, with_res, s2d, cbias=bool(relu))
        run_cl_affine(L, T, shape, relu, with_res, s2d, cbias=not relu, backward=False)
    T.done()


@pytest.mark.parametrize("case", R.CL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_channels_last_kernels_vs_fp64(L, case):
    """Lane geometry at HW = 130 for C in 4 .. 256, C = 4 around one pixel per thread, the strip edges at C = 64."""
    _whole_case(L, case, False)


@pytest.mark.parametrize("case", R.S2D_CASES, ids=lambda c: "x".join(map(str, c)))
def test_space_to_depth_addressing_vs_fp64(L, case):
    """s2d_w = W: y leaves in [B][H/2][W/2][2][2][C] (compared through _normref.s2d_index), the backward is given g and out in that
    layout and returns dx and dres in the plain one."""
    _whole_case(L, case, True)


@pytest.mark.parametrize("case", R.CL_PPW, ids=lambda c: "x".join(map(str, c)))
def test_strips_above_the_floor_through_set_norm_blocks(L, case):
    """fsraft_set_norm_blocks(64): PIX_PER_WG 192 at 2 x 4100 pixels, the 1024 cap with a ragged last strip at 66000."""
    lib = L.load()
    assert lib.fsraft_set_norm_blocks(R.CL_PPW_TARGET - 1) == FS_ERR_ARG
    try:
        assert lib.fsraft_set_norm_blocks(R.CL_PPW_TARGET) == 0
        _whole_case(L, case, False)
    finally:
        assert lib.fsraft_set_norm_blocks(R.CL_TARGET_DEFAULT) == 0


# ----------------------------------------------------------------------------------------------------------------- have_sums
def _split_rows(S, how):
    """fp64 [B, C] -> fp32 [B * 8, C] partial rows whose float64 sum is S to the last place of the last row."""
    B, C = S.shape
    if how == "slot7":
        a = [0.0] * 7
    elif how == "alternating":
        a = [0.625, -0.375] * 3 + [0.625]
    else:
        a = [0.125] * 7
    rows = [(k * S).float() for k in a]
    rows.append((S - torch.stack(rows).double().sum(0)).float())
    return torch.stack(rows, 1).reshape(B * 8, C).contiguous()


@pytest.mark.parametrize("how", ("slot7", "alternating", "eighths"))
@pytest.mark.parametrize("case", R.HAVE_SUMS_CASES, ids=lambda c: "x".join(map(str, c)))
def test_statistics_handed_in_as_partial_rows(L, case, how):
    """have_sums = 1: the eight rows come from float64 sums, split unevenly; the result is the have_sums = 0 result within the
    forward limit, and the rows are left as they were."""
    B, H, W, C = case
    shape = (B, C, H, W)
    x, g, res = _inputs(shape)
    xd = x.double()
    have = (_split_rows(xd.sum((2, 3)), how), _split_rows((xd * xd).sum((2, 3)), how))
    T = Tally("x".join(map(str, case)) + " " + how)
    for relu, with_res in ((1, True), (0, False)):
        own = run_cl_inorm(L, T, shape, relu, with_res, False)
        got = run_cl_inorm(L, T, shape, relu, with_res, False, have=have)
        exp = R.inorm_expect(x, g, R.EPS, relu, res if with_res else None, "cl")
        ref, scale, slack, key = exp["y"]
        T.check("inorm_cl y, have_sums against own pass", R.from_cl(got["y"], B, H, W, C),
                (R.from_cl(own["y"], B, H, W, C).double(), scale, slack, key), f"relu={relu} res={int(with_res)}")
    T.done()


# --------------------------------------------------------------------------------------------------------- affine second trip
@pytest.mark.parametrize("s2d", (False, True), ids=("plain", "s2d"))
def test_affine_forward_second_grid_trip(L, s2d):
    """33000 pixels x 256 channels: 2 112 000 float4 against the 8192 x 256 the capped grid covers in one trip."""
    B, H, W, C = R.SECOND_TRIP
    T = Tally("x".join(map(str, R.SECOND_TRIP)) + (" s2d" if s2d else ""))
    run_cl_affine(L, T, (B, C, H, W), 1, True, s2d, cbias=True, backward=False)
    T.done()


# ------------------------------------------------------------------------------------------------------------------ refusals
def _cl_calls(L, B, HW, C, s2w, out=True, dres=True):
    """The four channels-last entry points on buffers large enough for any C <= 264; returns [(name, rc, output Bufs)]."""
    lib = L.load()
    n = B * HW * 264
    src = torch.ones(n)
    x, g, y = Buf(src), Buf(src), Buf(src)
    par, stats = Buf(torch.ones(4 * 264)), Buf(torch.ones(2 * B * 264))
    res = []
    o = [Buf(n=n), Buf(n=B * 8 * 264), Buf(n=B * 8 * 264), Buf(n=2 * B * 264)]
    rc = lib.fsraft_inorm_relu_cl_fwd(_p(L, x), None, _p(L, o[0]), _p(L, o[1]), _p(L, o[2]), _p(L, o[3]), B, HW, C, R.EPS, 1, 0, s2w, L.stream())
    res.append(("inorm_relu_cl_fwd", rc, o))
    o = [Buf(n=B * 8 * 264), Buf(n=B * 8 * 264), Buf(n=n), Buf(n=n)]
    rc = lib.fsraft_inorm_relu_cl_bwd(_p(L, g), _p(L, x), _p(L, stats), _p(L, y) if out else None, _p(L, o[0]), _p(L, o[1]), _p(L, o[2]),
                                      _p(L, o[3]) if dres else None, B, HW, C, 1, s2w, L.stream())
    res.append(("inorm_relu_cl_bwd", rc, o))
    o = [Buf(n=n)]
    rc = lib.fsraft_affine_relu_cl_fwd(_p(L, x), None, _p(L, par), _p(L, par, 264), _p(L, o[0]), B * HW, C, 1, HW, s2w, L.stream())
    res.append(("affine_relu_cl_fwd", rc, o))
    o = [Buf(n=n), Buf(n=n), Buf(n=B * 8 * 264), Buf(n=B * 8 * 264)]
    rc = lib.fsraft_affine_relu_cl_bwd(_p(L, g), _p(L, x), _p(L, par), _p(L, par, 264), _p(L, y) if out else None, _p(L, o[0]),
                                       _p(L, o[1]) if dres else None, _p(L, o[2]), _p(L, o[3]), B, HW, C, 1, s2w, L.stream())
    res.append(("affine_relu_cl_bwd", rc, o))
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("C", (0, 2, 6, 260))
def test_channel_counts_outside_the_route_are_refused(L, C):
    for name, rc, outs in _cl_calls(L, 1, 16, C, 0):
        assert rc == FS_ERR_ARG, (name, C, rc)
        for o in outs:
            o.untouched()


@pytest.mark.parametrize("HW,w", ((20, 5), (12, 4), (130, 4)), ids=("odd_W", "odd_H", "HW_not_a_multiple_of_W"))
def test_space_to_depth_refuses_odd_images(L, HW, w):
    for name, rc, outs in _cl_calls(L, 1, HW, 8, w):
        assert rc == FS_ERR_ARG, (name, HW, w, rc)
        for o in outs:
            o.untouched()


@pytest.mark.parametrize("out,dres", ((True, False), (False, True)), ids=("out_without_dres", "dres_without_out"))
def test_backward_refuses_half_a_residual(L, out, dres):
    for name, rc, outs in _cl_calls(L, 1, 16, 8, 0, out, dres):
        if name.endswith("bwd"):
            assert rc == FS_ERR_ARG, (name, rc)
            for o in outs:
                o.untouched()


# ---------------------------------------------------------------------------------------------------------------- NCHW route
def run_nchw(L, T, case, relu, offset=0):
    """The four entry points of csrc/norm.hip on B * C planes; offset: floats every tensor is moved off its alignment by."""
    lib = L.load()
    B, C, HW = case
    H, W = R.NCHW_HW[HW]
    shape = (B, C, H, W)
    n, planes = B * C * HW, B * C
    x, g, _ = _inputs(shape)
    v = f"relu={relu}" + (f" offset={offset}" if offset else "")
    bx, bg = Buf(x, offset=offset), Buf(g, offset=offset)
    by, stats = Buf(n=n, offset=offset), Buf(n=2 * planes)
    L.check(lib.fsraft_inorm_relu_fwd(_p(L, bx), _p(L, by), _p(L, stats), planes, HW, R.EPS, relu, L.stream()), "inorm_relu_fwd")
    by.written(), stats.written()
    y, st = by.cpu().view(shape), stats.cpu().view(B, C, 1, 1, 2)
    exp = R.inorm_expect(x, g, R.EPS, relu, None, "nchw")
    T.check("inorm y", y, exp["y"], v)
    T.check("inorm mean", st[..., 0], exp["mean"], v)
    T.check("inorm rstd", st[..., 1], exp["rstd"], v)
    bdx = Buf(n=n, offset=offset)
    L.check(lib.fsraft_inorm_relu_bwd(_p(L, bg), _p(L, bx), _p(L, stats), _p(L, bdx), planes, HW, relu, L.stream()), "inorm_relu_bwd")
    bdx.written()
    T.check("inorm dx", bdx.cpu().view(shape), exp["dx"], v)
    fold, f = run_fold(L, T, B, C, True, v)
    bay = Buf(n=n, offset=offset)
    L.check(lib.fsraft_affine_relu_fwd(_p(L, bx), _p(L, fold), _p(L, fold, C), _p(L, bay), planes, C, HW, relu, L.stream()), "affine_relu_fwd")
    bay.written()
    aexp = R.affine_expect(x, g, f[0], f[1], relu, None)
    T.check("affine y", bay.cpu().view(shape), aexp["y"], v)
    badx, dsum = Buf(n=n, offset=offset), Buf(n=2 * C, zero=True)
    L.check(lib.fsraft_affine_relu_bwd(_p(L, bg), _p(L, bx), _p(L, fold), _p(L, fold, C), _p(L, badx), _p(L, dsum), _p(L, dsum, C), planes, C,
                                       HW, relu, L.stream()), "affine_relu_bwd")
    badx.written(), dsum.written()
    for b in (bx, bg, stats, fold):
        b.intact()
    assert _same_bits(bx.cpu(), x.reshape(-1)) and _same_bits(bg.cpu(), g.reshape(-1)), "an input was written"
    T.check("affine dx", badx.cpu().view(shape), aexp["dx"], v)
    T.check("affine dsum_g", dsum.cpu()[:C], aexp["dsum_g"], v)
    T.check("affine dsum_gx", dsum.cpu()[C:], aexp["dsum_gx"], v)
    return dict(y=by.cpu(), ay=bay.cpu(), stats=stats.cpu())


@pytest.mark.parametrize("case", R.NCHW_CASES, ids=lambda c: "x".join(map(str, c)))
def test_nchw_kernels_vs_fp64(L, case):
    """HW below one float4, with a scalar tail, one and several strides; 2 x 5 planes for c = plane % C.  Held to the scale
    without the r^2 term: these kernels take two passes."""
    T = Tally("x".join(map(str, case)))
    for relu in (0, 1):
        run_nchw(L, T, case, relu)
    T.done()


def test_nchw_scalar_route_from_a_misaligned_base(L):
    """HW = 640 from a storage offset of one float: HW % 4 == 0 but no pointer is 16-byte aligned, so the scalar loops run.  The
    affine y is the aligned call's bits, the instance norm's y wherever the two calls' statistics agree; all is held to the limits."""
    case = (2, 5, 640)
    T = Tally("2x5x640 offset 1")
    for relu in (0, 1):
        a, m = run_nchw(L, T, case, relu), run_nchw(L, T, case, relu, offset=1)
        assert _same_bits(a["ay"], m["ay"]), "affine y: scalar route against vector route"
        # the instance norm sums a plane in another order on the scalar route, so mean / rstd may differ in the last place;
        # wherever they do not, its y has the aligned call's bits too
        same = (a["stats"].view(10, 2) == m["stats"].view(10, 2)).all(1)
        assert _same_bits(a["y"].view(10, 640)[same], m["y"].view(10, 640)[same]), "inorm y: scalar route against vector route"
        _log_margin(f"planes with equal statistics on both routes, relu={relu}", float(same.sum()), 10.0, "count of 10")
    T.done()


# ------------------------------------------------------------------------------------------------------------------ wrappers
def _cl_leaf(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)


def _s2d_tensor(flat, B, H, W, C):
    """The [B, 4C, H/2, W/2] channels_last tensor whose storage is the space-to-depth layout `flat`."""
    return flat.to(DEV).view(B, H // 2, W // 2, 4 * C).permute(0, 3, 1, 2)


def test_instance_norm_wrapper_runs_the_tested_kernels(L):
    """_InstNormReluCL with s2d and a residual: the forward's bits are the direct call's (the s2d output's allocation, ctx.s2w), and
    dx / dres (handed to autograd, no _ResLink) meet the direct call's limits."""
    from flow_supervisor_amd.core.extractor import _InstNormReluCL
    B, H, W, C = 2, 26, 10, 64
    shape = (B, C, H, W)
    x, g, res = _inputs(shape)
    T = Tally("wrapper 2x26x10x64 s2d")
    direct = run_cl_inorm(L, T, shape, 1, True, True)
    xl, rl = _cl_leaf(x), _cl_leaf(res)
    y = _InstNormReluCL.apply(xl, R.EPS, True, rl, None, None, True)
    assert tuple(y.shape) == (B, 4 * C, H // 2, W // 2)
    yflat = y.detach().permute(0, 2, 3, 1).reshape(-1).cpu()
    assert _same_bits(yflat, direct["y"]), "forward bits of the wrapper against the direct call"
    y.backward(_s2d_tensor(R.to_s2d(g), B, H, W, C))
    exp = R.inorm_expect(x, g, R.EPS, 1, res, "cl", R.from_s2d(yflat, B, H, W, C))
    T.check("inorm_cl dx (wrapper)", xl.grad.cpu(), exp["dx"], "relu=1 res=1")
    assert _same_bits(rl.grad.cpu(), R.from_cl(direct["dres"], B, H, W, C)), "dres of the wrapper against the direct call"
    T.done()


def test_frozen_batchnorm_wrapper_runs_the_tested_kernels(L):
    """_FrozenBNReluCL with cbias and s2d: forward bits and dx bits (an elementwise product) are the direct call's."""
    from flow_supervisor_amd.core.extractor import _FrozenBNReluCL
    B, H, W, C = 2, 26, 10, 100
    shape = (B, C, H, W)
    x, g, _ = _inputs(shape)
    T = Tally("wrapper 2x26x10x100 s2d")
    direct = run_cl_affine(L, T, shape, 1, False, True, cbias=True)
    w, b, rm, rv, cb = (p.to(DEV) for p in R.bn_params(B, C, True))
    xl = _cl_leaf(x)
    y = _FrozenBNReluCL.apply(xl, cb, w, b, rm, rv, R.EPS, True, None, None, True)
    assert tuple(y.shape) == (B, 4 * C, H // 2, W // 2)
    assert _same_bits(y.detach().permute(0, 2, 3, 1).reshape(-1).cpu(), direct["y"]), "forward bits of the wrapper against the direct call"
    y.backward(_s2d_tensor(R.to_s2d(g), B, H, W, C))
    assert _same_bits(xl.grad.cpu(), R.from_cl(direct["dx"], B, H, W, C)), "dx bits of the wrapper against the direct call"
    T.done()
