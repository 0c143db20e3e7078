"""The kernels of csrc/norm_bn.hip (training-mode BatchNorm + ReLU + residual on channels-last tensors, forward with running
statistics and backward with the parameter gradients) called through their C entry points, each against its float64 restatement
(tests/_bnref.py) on the designed planes, at every edge of their launch geometry: C / 4 that does not divide 256 (idle tail
threads), n = 2, strips of 128 pixels one short / exact / one over, more workgroups than partial rows, odd batch sizes, one long
accumulation, strips of 192 with a ragged end, the space-to-depth addressing in both directions; relu x shortcut x cbias with
momentum 0.1 / 1.0 / 0.0, running statistics handed in or NULL, weights of both signs and non-zero biases.  The test owns every
buffer: each sits between two guard rows of the NaN pattern, outputs are pre-filled with it, and afterwards the guards are intact
and no pattern is left inside an output.  The results depend on the arrival order of atomics: no bits are asserted on sums.  Needs
an MI355X: -m gpu.

Limits: _bnref.LIMITS, set from the fp32 twin on the CPU (tests/test_bnref.py), not from the kernels.  profiles/
bn_train_margins.txt lists every comparison (FSRAFT_PARITY_LOG).  Worst values measured on MI355X, in the units of _bnref's scales:
  bnorm y                                 3.01  limit 20  (2x13x10x256; relu=0 res=0 cbias=1 momentum=1.0)
  bnorm mean                              7.09  limit 20  (2x103x10x64; relu=1 res=1 cbias=1 momentum=0.1 no running)
  bnorm rstd                              4.15  limit 20  (2x13x10x256; relu=1 res=1 cbias=1 momentum=0.1 no running)
  bnorm scale                             3.17  limit 20  (2x13x10x252; relu=1 res=1 cbias=1 momentum=0.1 no running)
  bnorm shift                             3.17  limit 20  (2x13x10x252; relu=1 res=1 cbias=1 momentum=0.1 no running)
  bnorm running_mean                      3.95  limit 20  (2x103x10x64; relu=0 res=1 cbias=1 momentum=0.1)
  bnorm running_var                       5.02  limit 20  (2x13x10x252; relu=1 res=1 cbias=1 momentum=1.0)
  bnorm dx                                3.17  limit 20  (2x13x10x252; relu=0 res=1 cbias=1 momentum=0.1)
  bnorm dweight                           2.98  limit 7   (2x13x10x256; relu=1 res=1 cbias=1 momentum=0.1 no running)
  bnorm dbias                             1.48  limit 7   (2x2x2x100 s2d; relu=0 res=1 cbias=1 momentum=0.1)
(the case is B x H x W x C.)  With sixteen partial rows the mean of 1x520x512x4 measured 11.9: a chain of 87 atomic adds per row;
see bn_sum_rows in csrc/norm_bn.hip.
"""
import functools

import pytest
import torch

import _bnref as N
import _normref as R
from _util import Buf, _log_margin

pytestmark = pytest.mark.gpu
FS_ERR_ARG = 1


@pytest.fixture(scope="module", autouse=True)
def _leave_no_cached_segments():
    """(as tests/test_norm_kernels.py: hand the free segments back, later modules count allocated bytes)"""
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
        w, i = N.need(got.reshape(ref.shape), ref, scale, slack)
        if w >= self.worst.get(name, (-1.0,))[0]:
            self.worst[name] = (w, N.LIMITS[key], variant)
        if not w <= N.LIMITS[key]:
            self.failed.append((name, variant, w, N.LIMITS[key], i))

    def done(self):
        for name, (w, lim, variant) in sorted(self.worst.items()):
            _log_margin(f"{name} {self.case}", w, lim, f"worst (|got - ref| - slack) / scale, {variant}")
        assert not self.failed, (self.case, self.failed)


@functools.lru_cache(maxsize=4)
def _inputs(shape):
    return N.designed(*shape), N.gradients(*shape), N.residual(*shape)


def run_bnorm(L, T, shape, relu, with_res, cbias, momentum, s2d, running=True):
    """fsraft_bnorm_cl_fwd, then _bwd from its own stats and y.  Returns the raw outputs."""
    lib = L.load()
    B, C, H, W = shape
    HW, n, s2w = H * W, B * C * H * W, (W if s2d else 0)
    x, g, res = _inputs(shape)
    res = res if with_res else None
    w, b, rm, rv, cb = N.params(B, C)
    cb = cb if cbias else None
    v = f"relu={relu} res={int(with_res)} cbias={int(cbias)} momentum={momentum}" + ("" if running else " no running")
    bx, br = Buf(R.to_cl(x)), (Buf(R.to_cl(res)) if with_res else None)
    bw, bb, bc = Buf(w), Buf(b), (Buf(cb) if cbias else None)
    brm, brv = (Buf(rm), Buf(rv)) if running else (None, None)
    by, stats, acc = Buf(n=n), Buf(n=4 * C), Buf(n=2 * N.BN_ROWS * C, zero=True)
    L.check(lib.fsraft_bnorm_cl_fwd(_p(L, bx), _p(L, br), _p(L, bw), _p(L, bb), _p(L, bc), _p(L, brm), _p(L, brv), momentum, N.EPS,
                                    _p(L, acc), _p(L, by), _p(L, stats), B, HW, C, relu, s2w, L.stream()), "bnorm_cl_fwd")
    by.written(), stats.written(), acc.written()
    for q in (bx, br, bw, bb, bc, brm, brv):
        if q is not None:
            q.intact()
    assert _same_bits(bx.cpu(), R.to_cl(x)) and _same_bits(bw.cpu(), w) and _same_bits(bb.cpu(), b), "the forward wrote an input"
    yflat, st = by.cpu(), stats.cpu().view(4, C)
    y = R.from_s2d(yflat, B, H, W, C) if s2d else R.from_cl(yflat, B, H, W, C)
    exp = N.bn_expect(x, g, w, b, cb, rm, rv, momentum, N.EPS, relu, res, y if with_res else None)
    T.check("bnorm y", y, exp["y"], v)
    for i, name in enumerate(("mean", "rstd", "scale", "shift")):
        T.check("bnorm " + name, st[i], exp[name], v)
    if running:
        T.check("bnorm running_mean", brm.cpu(), exp["rm"], v)
        T.check("bnorm running_var", brv.cpu(), exp["rv"], v)
    bg = Buf(R.to_s2d(g) if s2d else R.to_cl(g))
    acc2, bdx, dpar = Buf(n=2 * N.BN_ROWS * C, zero=True), Buf(n=n), Buf(n=2 * C)
    bdres = Buf(n=n) if with_res else None
    L.check(lib.fsraft_bnorm_cl_bwd(_p(L, bg), _p(L, bx), _p(L, stats), _p(L, by) if with_res else None, _p(L, acc2), _p(L, bdx),
                                    _p(L, bdres), _p(L, dpar), _p(L, dpar, C), B, HW, C, relu, s2w, L.stream()), "bnorm_cl_bwd")
    bdx.written(), dpar.written(), acc2.written()
    for q in (bx, by, stats, bg):
        q.intact()
    assert _same_bits(by.cpu(), yflat) and _same_bits(stats.cpu().view(4, C), st) and _same_bits(bx.cpu(), R.to_cl(x)), \
        "the backward wrote an input"
    d = dpar.cpu().view(2, C)
    T.check("bnorm dx", R.from_cl(bdx.cpu(), B, H, W, C), exp["dx"], v)
    T.check("bnorm dweight", d[0], exp["dweight"], v)
    T.check("bnorm dbias", d[1], exp["dbias"], v)
    if with_res:
        bdres.written()
        assert _same_bits(R.from_cl(bdres.cpu(), B, H, W, C), torch.where(y > 0, g, torch.zeros_like(g))), f"dres is g where out > 0 ({v})"
    return dict(y=yflat, stats=st)


def _whole_case(L, case, s2d):
    B, H, W, C = case
    shape = (B, C, H, W)
    T = Tally("x".join(map(str, case)) + (" s2d" if s2d else ""))
    for relu, with_res, cbias, mom in N.VARIANTS:
        run_bnorm(L, T, shape, relu, with_res, cbias, mom, s2d)
    run_bnorm(L, T, shape, 1, True, True, 0.1, s2d, running=False)
    T.done()


@pytest.mark.parametrize("case", N.CASES, ids=lambda c: "x".join(map(str, c)))
def test_training_batchnorm_kernels_vs_fp64(L, case):
    _whole_case(L, case, False)


@pytest.mark.parametrize("case", N.S2D_CASES, ids=lambda c: "x".join(map(str, c)))
def test_space_to_depth_addressing_vs_fp64(L, case):
    """s2d_w = W: y leaves in [B][H/2][W/2][2][2][C], the backward is given g and out in that layout and returns dx and dres in the
    plain one."""
    _whole_case(L, case, True)


def test_output_does_not_depend_on_the_convolution_bias(L):
    """cbias moves the running mean only: y and the statistics of two calls with and without it agree within the forward limits
    (no bits: the sums are atomics)."""
    shape = (2, 64, 13, 10)
    T = Tally("2x13x10x64 cbias")
    a = run_bnorm(L, T, shape, 1, False, False, 0.1, False)
    c = run_bnorm(L, T, shape, 1, False, True, 0.1, False)
    x, g, _ = _inputs(shape)
    w, b, rm, rv, cb = N.params(2, 64)
    exp = N.bn_expect(x, g, w, b, None, rm, rv, 0.1, N.EPS, 1, None)
    ref, scale, slack, key = exp["y"]
    T.check("bnorm y, with cbias against without", R.from_cl(c["y"], 2, 13, 10, 64), (R.from_cl(a["y"], 2, 13, 10, 64).double(), scale, slack, key))
    T.done()


# ------------------------------------------------------------------------------------------------------------------ refusals
def _calls(L, B, HW, C, s2w, out=True, dres=True):
    """Both entry points on buffers large enough for any C <= 264; returns [(name, rc, output and running Bufs)]."""
    lib = L.load()
    n = B * HW * 264
    src = torch.ones(n)
    x, g, y = Buf(src), Buf(src), Buf(src)
    par, stats = Buf(torch.ones(3 * 264)), Buf(torch.ones(4 * 264))
    res = []
    o = [Buf(n=n), Buf(n=4 * 264), Buf(n=2 * N.BN_ROWS * 264), Buf(n=264), Buf(n=264)]
    rc = lib.fsraft_bnorm_cl_fwd(_p(L, x), None, _p(L, par), _p(L, par, 264), _p(L, par, 528), _p(L, o[3]), _p(L, o[4]), 0.1, N.EPS,
                                 _p(L, o[2]), _p(L, o[0]), _p(L, o[1]), B, HW, C, 1, s2w, L.stream())
    res.append(("bnorm_cl_fwd", rc, o))
    o = [Buf(n=2 * N.BN_ROWS * 264), Buf(n=n), Buf(n=n), Buf(n=264), Buf(n=264)]
    rc = lib.fsraft_bnorm_cl_bwd(_p(L, g), _p(L, x), _p(L, stats), _p(L, y) if out else None, _p(L, o[0]), _p(L, o[1]),
                                 _p(L, o[2]) if dres else None, _p(L, o[3]), _p(L, o[4]), B, HW, C, 1, s2w, L.stream())
    res.append(("bnorm_cl_bwd", rc, o))
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("B,HW,C,w", ((1, 16, 6, 0), (1, 16, 260, 0), (1, 1, 8, 0), (1, 20, 8, 5), (1, 12, 8, 4)),
                         ids=("C6", "C260", "n1", "odd_s2d_w", "odd_H"))
def test_refusals_write_nothing(L, B, HW, C, w):
    for name, rc, outs in _calls(L, B, HW, C, w):
        assert rc == FS_ERR_ARG, (name, rc)
        for o in outs:
            o.untouched()


def test_half_a_residual_and_half_the_running_statistics_are_refused(L):
    for name, rc, outs in _calls(L, 1, 16, 8, 0, True, False) + _calls(L, 1, 16, 8, 0, False, True):
        if name.endswith("bwd"):
            assert rc == FS_ERR_ARG, (name, rc)
            for o in outs:
                o.untouched()
    lib = L.load()
    x, par, rm = Buf(torch.ones(16 * 8)), Buf(torch.ones(16)), Buf(n=8)
    o = [Buf(n=16 * 8), Buf(n=32), Buf(n=2 * N.BN_ROWS * 8)]
    rc = lib.fsraft_bnorm_cl_fwd(_p(L, x), None, _p(L, par), _p(L, par, 8), None, _p(L, rm), None, 0.1, N.EPS, _p(L, o[2]), _p(L, o[0]),
                                 _p(L, o[1]), 1, 16, 8, 1, 0, L.stream())
    torch.cuda.synchronize()
    assert rc == FS_ERR_ARG
    for q in o + [rm]:
        q.untouched()


# ------------------------------------------------------------------------------------------------------------------- wrapper
def test_autograd_wrapper_runs_the_tested_kernels(L):
    """_TrainBNReluCL with cbias, a shortcut and s2d on an nn.BatchNorm2d: y, dx, the parameter gradients and the module's buffers
    meet the direct call's limits; dres has its bits; num_batches_tracked counts; the convolution bias gets no gradient."""
    from flow_supervisor_amd.core.extractor import _TrainBNReluCL
    B, H, W, C = 2, 26, 10, 64
    shape = (B, C, H, W)
    x, g, res = _inputs(shape)
    w, b, rm, rv, cb = N.params(B, C)
    bn = torch.nn.BatchNorm2d(C, eps=N.EPS, momentum=0.1).cuda().train()
    with torch.no_grad():
        bn.weight.copy_(w), bn.bias.copy_(b), bn.running_mean.copy_(rm), bn.running_var.copy_(rv)
    leaf = lambda t: t.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    xl, rl, cbl = leaf(x), leaf(res), cb.cuda().requires_grad_(True)
    y = _TrainBNReluCL.apply(xl, cbl, bn.weight, bn.bias, bn, True, rl, None, True)
    assert tuple(y.shape) == (B, 4 * C, H // 2, W // 2)
    yv = R.from_s2d(y.detach().permute(0, 2, 3, 1).reshape(-1).cpu(), B, H, W, C)
    y.backward(R.to_s2d(g).cuda().view(B, H // 2, W // 2, 4 * C).permute(0, 3, 1, 2))
    exp = N.bn_expect(x, g, w, b, cb, rm, rv, 0.1, N.EPS, 1, res, yv)
    T = Tally("wrapper 2x26x10x64 s2d")
    T.check("bnorm y (wrapper)", yv, exp["y"])
    T.check("bnorm dx (wrapper)", xl.grad.cpu(), exp["dx"])
    T.check("bnorm dweight (wrapper)", bn.weight.grad.cpu(), exp["dweight"])
    T.check("bnorm dbias (wrapper)", bn.bias.grad.cpu(), exp["dbias"])
    T.check("bnorm running_mean (wrapper)", bn.running_mean.cpu(), exp["rm"])
    T.check("bnorm running_var (wrapper)", bn.running_var.cpu(), exp["rv"])
    assert _same_bits(rl.grad.cpu(), torch.where(yv > 0, g, torch.zeros_like(g))) and cbl.grad is None
    assert int(bn.num_batches_tracked) == 1
    with torch.no_grad():                                  # without a graph the statistics still move
        _TrainBNReluCL.apply(xl, cbl, bn.weight, bn.bias, bn, True, rl, None, False)
    assert int(bn.num_batches_tracked) == 2 and not torch.equal(bn.running_mean.cpu(), exp["rm"][0].float())
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        _TrainBNReluCL.apply(torch.zeros(1, C, 1, 1, device="cuda"), None, bn.weight, bn.bias, bn, True)
    T.done()
