"""float64 restatement of the training-mode BatchNorm kernels (csrc/norm_bn.hip: fsraft_bnorm_cl_fwd / _bwd), running statistics
and the convolution bias `cbias` included, with analytic error scales, an fp32 twin and mutants (tests/test_bnref.py on the CPU,
tests/test_bn_train_kernels.py against the kernels).  The method, the designed planes, the comparator `need` and the layout helpers
are those of tests/_normref.py; every tensor here is NCHW [B, C, H, W], per-channel quantities are [C].

Scales (u = 2^-24; per channel over n = B HW: r = |mean| rstd, xhat = (x - mean) rstd; the variance is the instance route's
single-pass sumsq / n - mean^2, so _normref's (1 + r^2) carries over with HW -> n):
  Fx        u (|xhat| + 1) (1 + r^2)                       the error of xhat as the kernel has it
  y         |weight| Fx + u (|bias| + |t|), t = x scale + shift; with a shortcut + u |y|
  mean      u sum|x| / n
  rstd      rho rstd, rho = u (1 + r^2);  scale: (rho + u) |scale|
  shift     u (|bias| + |shift|) + |mean scale| (rho + 2 u) + |scale| u sum|x| / n
  running_mean   u (|(1 - m) rm| + m (sum|x| / n + |cbias|) + |result|)
  running_var    u (|(1 - m) rv| + m (var + 2 mean^2) n / (n - 1) + |result|)
  dx        |dx| (rho + u) + |scale| (u |g'| + u S1 + |xhat| (u S2 + SF) + Fx |m2| + u (|m1| + |xhat m2|)),
            S1 = sum|g'| / n, S2 = sum|g' xhat| / n, SF = sum|g'| Fx / n, m1 = sum g' / n, m2 = sum g' xhat / n
  dbias     u sum|g'|;   dweight: u sum|g' xhat| + sum|g'| Fx

The inner ReLU mask is decided on t in fp32 by the kernel and in fp64 here.  An element is ambiguous when |t| is within
LIMITS[bn_y] x its own forward scale of 0; it is not excluded but gets slack |g scale| in dx and |g| (|g xhat| + |g| Fx) in the
sums that contain it, which reaches every dx of the channel through m1 / m2.  A channel that is constant over the whole batch
(C = 252: planes of kind `constant` in every sample) has xhat = 0 in float64 and t = bias; it is ambiguous only where its bias
is, and such channels are left out of the share that `ambiguous_share` reports, as _normref leaves out its constant planes.

LIMITS are 4 x the worst value the fp32 TWIN reaches against float64 over CASES + S2D_CASES and all VARIANTS, rounded up to one
significant digit, floor 4 (_normref.limit_from_twin).  The kernels' own worst values are in tests/test_bn_train_kernels.py and
profiles/bn_train_margins.txt; they do not set the limits.
"""
import itertools

import torch

import _normref as R
from _normref import EPS, U24, designed, gradients, limit_from_twin, need, residual, to_cl, to_s2d  # noqa: F401 (re-exported)

BN_ROWS = 64                        # FSRAFT_BN_PARTIAL_ROWS
BN_TARGET_WGS = 2048                # csrc/norm_bn.hip


def strip(B, HW):
    """Pixels of one sample per workgroup, restated from bn_strip of csrc/norm_bn.hip."""
    p = (B * HW + BN_TARGET_WGS - 1) // BN_TARGET_WGS
    p = (p + 63) // 64 * 64
    return 128 if p < 128 else 2048 if p > 2048 else p


def workgroups(B, HW):
    return B * -(-HW // strip(B, HW))


# (B, H, W, C)
GEOMETRY = tuple((2, 13, 10, C) for C in (4, 12, 96, 100, 252, 256))          # idle tail threads
SMALL = ((2, 1, 1, 4), (1, 1, 2, 4))                                          # n = 2, the smallest legal
STRIPS = ((2, 1, 127, 64), (2, 8, 16, 64), (2, 3, 43, 64))                    # a strip of 128 one short / exact / one over
ROWS = ((3, 41, 25, 64), (5, 7, 9, 64), (2, 103, 10, 64), (5, 41, 40, 4))     # odd B, several strips; 65 workgroups on 64 rows
LONG = ((4, 92, 124, 64), (1, 520, 512, 4))                                   # one long accumulation; strips of 192, ragged end
CASES = GEOMETRY + SMALL + STRIPS + ROWS + LONG
S2D_CASES = tuple((2, H, W, C) for (H, W) in ((2, 2), (4, 6), (26, 10)) for C in (4, 64, 100))
MOMENTA = (0.1, 1.0, 0.0)
# (relu, with shortcut, with cbias, momentum)
VARIANTS = tuple((relu, res, cb, MOMENTA[i % 3]) for i, (relu, res, cb) in enumerate(itertools.product((0, 1), (False, True), (False, True))))

TWIN_WORST = dict(bn_y=2.6, bn_stat=3.9, bn_run=3.7, bn_dx=3.2, bn_sum=1.6)
LIMITS = dict(bn_y=20.0, bn_stat=20.0, bn_run=20.0, bn_dx=20.0, bn_sum=7.0)


def params(B, C, seed=0):
    """(weight, bias, running_mean, running_var, cbias) fp32 [C]: weights of both signs away from 0, non-zero biases."""
    g = torch.Generator().manual_seed(49979687 * seed + 7 * C + B)
    w = torch.randn(C, generator=g)
    w = torch.where(w.abs() < 0.1, torch.full_like(w, -0.5), w)
    b, rm, cb = (torch.randn(C, generator=g) for _ in range(3))
    b = torch.where(b.abs() < 0.05, torch.full_like(b, 0.25), b)
    return w, b, rm, torch.rand(C, generator=g) + 0.1, cb


def _csum(t, per_sample=False):
    return t.sum((2, 3), keepdim=True) if per_sample else t.sum((0, 2, 3), keepdim=True)


def _kept(H, W, strip_px, mut, like):
    """Pixels a mutated sums pass still adds: 'last_strip' drops the last strip of every sample."""
    k = torch.ones(H * W, dtype=like.dtype)
    if mut == "last_strip":
        k[(H * W - 1) // strip_px * strip_px:] = 0
    return k.view(1, 1, H, W)


def _c(v, C):
    return v.double().view(1, C, 1, 1)


# ---------------------------------------------------------------------------------------------------------- float64 reference
def bn_ref(x, w, b, cb, rm, rv, momentum, eps, relu, res=None, mut="", strip_px=128):
    """dict(y, t, xhat, mean, rstd, scale, shift [1, C, 1, 1] each; rm, rv [C] or None) of relu?(batch_norm(x + cbias)) in training
    mode, or of relu(res + that)."""
    xd = x.double()
    B, C, H, W = xd.shape
    ps = mut == "per_sample"
    n = H * W if ps else B * H * W
    k = _kept(H, W, strip_px, mut, xd)
    mean = _csum(xd * k, ps) / n
    var = _csum((xd - mean) ** 2 * k, ps) / n
    rstd = 1.0 / torch.sqrt(var + eps)
    scale = _c(w, C) * rstd
    shift = _c(b, C) - mean * scale
    xhat = (xd - mean) * rstd
    t = xhat * _c(w, C) + _c(b, C)
    y = t.clamp_min(0) if relu else t
    if res is not None:
        y = (y + res.double()).clamp_min(0)
    out = dict(y=y, t=t, xhat=xhat, mean=mean, rstd=rstd, scale=scale, shift=shift, var=var, rm=None, rv=None)
    if rm is not None:
        m = momentum
        mc, vc = mean.mean(0).reshape(C), var.mean(0).reshape(C)
        if cb is not None and mut != "no_cbias":
            mc = mc + cb.double()
        vc = vc if mut == "biased" else vc * n / (n - 1)
        keep, take = (m, 1.0 - m) if mut == "momentum_swapped" else (1.0 - m, m)
        out["rm"] = keep * rm.double() + take * mc
        out["rv"] = keep * rv.double() + take * vc
    return out


def bn_bwd_ref(g, x, w, b, eps, relu, res=None, y=None, mut="", strip_px=128):
    """dx, dres, dweight [C], dbias [C]; y: the forward result whose sign gates the shortcut's outer ReLU (the reference's own when
    None)."""
    f = bn_ref(x, w, b, None, None, None, 0.0, eps, relu, res)
    B, C, H, W = x.shape
    n = B * H * W
    gd = g.double()
    dres = None
    if res is not None:
        gd = gd * ((f["y"] if y is None else y.double()) > 0)
        dres = gd
    gp = gd
    if relu:
        gp = gd * ((f["xhat"] if mut == "mask_xhat" else f["t"]) > 0)
        if mut == "dres_inner" and res is not None:
            dres = gp
    k = _kept(H, W, strip_px, mut, gd)
    s1, s2 = _csum(gp * k), _csum(gp * f["xhat"] * k)
    d = H * W if mut == "div_hw" else n
    dx = f["scale"] * (gp - s1 / d - f["xhat"] * s2 / d)
    return dx, dres, s2.reshape(C), s1.reshape(C)


# ------------------------------------------------------------------------------------------------------------------ fp32 twin
def bn_twin(x, w, b, cb, rm, rv, momentum, eps, relu, res=None):
    """The kernel's formula in float32 (torch.sum for the column sums)."""
    x = x.float()
    B, C, H, W = x.shape
    n = float(B * H * W)
    v = lambda p: p.float().view(1, C, 1, 1)
    mean = _csum(x) / n
    var = (_csum(x * x) / n - mean * mean).clamp_min(0)
    rstd = torch.rsqrt(var + eps)
    scale = v(w) * rstd
    shift = v(b) - mean * scale
    t = x * scale + shift
    y = t.clamp_min(0) if relu else t
    if res is not None:
        y = (y + res.float()).clamp_min(0)
    out = dict(y=y, t=t, mean=mean, rstd=rstd, scale=scale, shift=shift, rm=None, rv=None)
    if rm is not None:
        one = torch.tensor(1.0) - torch.tensor(momentum, dtype=torch.float32)
        mom = torch.tensor(momentum, dtype=torch.float32)
        mc = mean.reshape(C) + (cb.float() if cb is not None else 0.0)
        out["rm"] = one * rm.float() + mom * mc
        out["rv"] = one * rv.float() + mom * (var.reshape(C) * torch.tensor(n / (n - 1.0), dtype=torch.float32))
    return out


def bn_bwd_twin(g, x, f, relu, y=None):
    """dx, dres, dweight, dbias in float32 from the forward twin's dict."""
    x, g = x.float(), g.float()
    B, C, H, W = x.shape
    n = float(B * H * W)
    dres = None
    if y is not None:
        g = torch.where(y > 0, g, torch.zeros_like(g))
        dres = g
    gp = torch.where(f["t"] <= 0, torch.zeros_like(g), g) if relu else g
    xhat = (x - f["mean"]) * f["rstd"]
    s1, s2 = _csum(gp), _csum(gp * xhat)
    dx = f["scale"] * (gp - s1 / n - xhat * (s2 / n))
    return dx, dres, s2.reshape(C), s1.reshape(C)


# ------------------------------------------------------------------------------------------------- expectations with scales
def bn_expect(x, g, w, b, cb, rm, rv, momentum, eps, relu, res, y=None):
    """{name: (ref, scale, slack, limit key)} for y, mean, rstd, scale, shift, rm, rv, dx, dweight, dbias; `ambiguous`: the mask of
    ambiguous elements, `whole`: the channels that are constant over the batch."""
    f = bn_ref(x, w, b, cb, rm, rv, momentum, eps, relu, res)
    dx, dres, dw, db = bn_bwd_ref(g, x, w, b, eps, relu, res, y)
    xd, gd = x.double(), g.double()
    B, C, H, W = x.shape
    n = B * H * W
    mean, rstd, xhat, t, scale = f["mean"], f["rstd"], f["xhat"], f["t"], f["scale"]
    r = mean.abs() * rstd
    rho = U24 * (1 + r * r)
    Fx = U24 * (xhat.abs() + 1) * (1 + r * r)
    Ft = _c(w, C).abs() * Fx + U24 * (_c(b, C).abs() + t.abs())
    Fy = Ft + U24 * f["y"].abs() if res is not None else Ft
    ax = _csum(xd.abs()) / n
    if res is not None:
        gd = gd * ((f["y"] if y is None else y.double()) > 0)
    amb = (t.abs() <= LIMITS["bn_y"] * Ft) if relu else torch.zeros_like(t, dtype=torch.bool)
    whole = (xd == mean).all(3, keepdim=True).all(2, keepdim=True).all(0, keepdim=True)
    gp = gd * (t > 0) if relu else gd
    S1, S2, SF = _csum(gp.abs()) / n, _csum((gp * xhat).abs()) / n, _csum(gp.abs() * Fx) / n
    m1, m2 = _c(db, C) / n, _c(dw, C) / n
    A1, A2 = _csum(gd.abs() * amb), _csum((gd * xhat).abs() * amb + gd.abs() * Fx * amb)
    sdx = dx.abs() * (rho + U24) + scale.abs() * (U24 * gp.abs() + U24 * S1 + xhat.abs() * (U24 * S2 + SF) + Fx * m2.abs()
                                                  + U24 * (m1.abs() + (xhat * m2).abs()))
    kdx = scale.abs() * (gd.abs() * amb + A1 / n + (xhat.abs() + Fx) * A2 / n)
    flat = lambda v: v.reshape(C)
    exp = dict(y=(f["y"], Fy, 0.0, "bn_y"), mean=(flat(mean), flat(U24 * ax), 0.0, "bn_stat"),
               rstd=(flat(rstd), flat(rho * rstd), 0.0, "bn_stat"), scale=(flat(scale), flat((rho + U24) * scale.abs()), 0.0, "bn_stat"),
               shift=(flat(f["shift"]), flat(U24 * (_c(b, C).abs() + f["shift"].abs()) + (mean * scale).abs() * (rho + 2 * U24)
                                             + scale.abs() * U24 * ax), 0.0, "bn_stat"),
               dx=(dx, sdx, kdx, "bn_dx"), dbias=(db, flat(U24 * S1 * n), flat(A1), "bn_sum"),
               dweight=(dw, flat(U24 * S2 * n + SF * n), flat(A2), "bn_sum"), ambiguous=amb, whole=whole)
    if rm is not None:
        m = momentum
        acb = cb.double().abs() if cb is not None else 0.0
        exp["rm"] = (f["rm"], U24 * (((1 - m) * rm.double()).abs() + m * (flat(ax) + acb) + f["rm"].abs()), 0.0, "bn_run")
        exp["rv"] = (f["rv"], U24 * (((1 - m) * rv.double()).abs() + m * flat(f["var"] + 2 * mean * mean) * n / (n - 1) + f["rv"].abs()),
                     0.0, "bn_run")
    return exp


def ambiguous_share(exp):
    """Share of ambiguous elements, the channels that are constant over the batch left out."""
    return float((exp["ambiguous"] & ~exp["whole"]).double().mean())
