"""float64 restatements of the encoder normalisation kernels (csrc/norm_cl.hip channels-last, csrc/norm.hip NCHW, and the frozen
BatchNorm fold), the designed planes that make their weak spots visible, analytic error scales, fp32 twins and mutants
(tests/test_normref.py on the CPU, tests/test_norm_kernels.py against the kernels).  Plain torch on the CPU; every tensor here is
NCHW [B, C, H, W], the layout transforms (to_cl / from_cl / s2d_index) are separate.

Comparator.  `need(got, ref, scale, slack)` is the worst  max(0, |got - ref| - slack_i) / scale_i  over the elements in float64; a
comparison passes when that number is at most its entry of LIMITS.  Scales (u = 2^-24, r = |mean| rstd of the plane,
xhat = (x - mean) rstd):
  y, instance norm   F = u (|xhat| + 1) (1 + r^2)  on the channels-last route: its variance is sumsq / HW - mean^2, whose rounding
                     is u (var + 2 mean^2), i.e. u (1/2 + r^2) relative in rstd;
                     F = u (|xhat| + 1 + r)  on the NCHW route (two passes: no r^2).  The r is the rounding of the mean, u |mean|,
                     times rstd: on a constant plane this is the whole error, rsqrt(eps) u |x|, and it is the same term on every
                     other plane (the single-pass scale already contains it: r <= (1 + r^2) / 2).
                     With a residual: + u |y| for the add.
  mean               u sum|x| / HW
  rstd               rho rstd with rho = u (1 + r^2) channels-last, u NCHW
  dx, instance norm  the above carried through rstd (g' - m1 - xhat m2):
                     |dx| rho + rstd (u |g'| + u S1 + |xhat| (u S2 + SF) + F |m2| + u (|m1| + |xhat m2|))
                     with S1 = sum|g'| / HW, S2 = sum|g' xhat| / HW, SF = sum|g'| F / HW
  sums               u sum|terms|  (s2 of the instance norm: + sum |g'| F, its terms carry the forward error)
  y, affine          u (|x scale| + |t|), t = x scale + shift (a product and an add, or one fma); residual as above
  dx, affine         u |dx|, limit 1 fixed: one fp32 product
  fold               rs: u rs; scale: u |scale|; rmc: u |rmc|; shift: u (|bias| + |rmc scale|);
                     dweight: u rs (sum|p1| + |rmc| sum|p0|); dbias: u sum|p0|; dcbias: u |scale| sum|p0|

ReLU masks are decided in fp32 by the kernel and in fp64 here.  An element is ambiguous when |xhat| (|t|) is within
LIMITS[forward] x its own forward scale of 0; it is not excluded but gets slack |g| rstd (|g| |scale|) in dx, and |g| (times |xhat|
or |x|) in the slack of the sums that contain it (through m1 / m2 that reaches every dx of the plane).  A value that is exactly 0 in
fp32 as well is not ambiguous and must be masked (`<= 0`, as torch does): the affine zeros (x = 0, shift = 0), and HW = 1.  A
constant plane at HW > 1 is NOT such a value: x - mean is 0 in float64, but the fp32 mean of HW equal numbers is not that number
(torch's own fp32 instance_norm gives +-1e-4 there), so with relu its inner mask is whatever the rounding of the mean says; those
planes are ambiguous as a whole on the instance-norm backward with relu (their relu = 0 backward and both forwards are held in
full) and are left out of the share that `ambiguous_share` reports and test_normref.py bounds by 1 %.
The mask of the residual's outer ReLU is taken from the forward result the backward is given (`y`), as the kernel does.

LIMITS are 4 x the worst value the fp32 TWIN (the kernel's formula in torch float32, torch.sum) reaches against float64 over the
case lists below, rounded up to one significant digit, floor 4 (the 4 covers the kernel's summation order: per-lane strides, the
LDS column, eight atomically filled rows).  Twin worst values: see TWIN_WORST.  The kernels' own worst values are in
tests/test_norm_kernels.py and profiles/norm_kernel_margins.txt; they do not set the limits.  test_normref.py proves every limit at
most a quarter of what each mutant produces on some case.
"""
import math

import torch

U24 = 2.0 ** -24
EPS = 1e-5
CL_NSLOT = 8
CL_TARGET_DEFAULT = 4096            # g_cl_target_wgs of csrc/norm_cl.hip

# ------------------------------------------------------------------------------------------------------------------ case lists
# (B, H, W, C) of the channels-last route
CL_GEOMETRY = tuple((2, 13, 10, C) for C in (4, 12, 96, 100, 252, 256))
CL_C4 = ((2, 1, 1, 4), (2, 1, 3, 4), (2, 15, 17, 4), (2, 16, 16, 4), (2, 1, 257, 4))
CL_STRIPS = ((2, 1, 127, 64), (2, 8, 16, 64), (2, 3, 43, 64), (3, 41, 25, 64), (2, 103, 10, 64))
CL_CASES = CL_GEOMETRY + CL_C4 + CL_STRIPS
CL_PPW = ((2, 41, 100, 8), (1, 264, 250, 4))          # under fsraft_set_norm_blocks(64): PIX_PER_WG 192 and 1024
CL_PPW_TARGET = 64
S2D_CASES = tuple((2, H, W, C) for (H, W) in ((2, 2), (4, 6), (26, 10), (42, 50)) for C in (4, 64, 100))
SECOND_TRIP = (1, 132, 250, 256)                      # affine forward: 33000 * 64 float4 > 8192 * 256
HAVE_SUMS_CASES = ((2, 13, 10, 12), (3, 41, 25, 64))
# (B, C, HW) of the NCHW route: six planes, and 2 x 5 planes at HW = 640
NCHW_CASES = tuple((2, 3, hw) for hw in (1, 2, 3, 63, 256, 1028, 46000)) + ((2, 5, 640),)
NCHW_HW = {1: (1, 1), 2: (1, 2), 3: (1, 3), 63: (7, 9), 256: (16, 16), 1028: (4, 257), 46000: (184, 250), 640: (20, 32)}

TWIN_WORST = dict(cl_y=3.3, cl_mean=4.3, cl_rstd=3.5, cl_dx=3.4, cl_sum=4.0,
                  nchw_y=2.2, nchw_mean=2.2, nchw_rstd=1.6, nchw_dx=1.7,
                  aff_y=1.0, aff_sum=4.5, fold=2.4, fold_bwd=2.2)
LIMITS = dict(cl_y=20.0, cl_mean=20.0, cl_rstd=20.0, cl_dx=20.0, cl_sum=20.0,
              nchw_y=9.0, nchw_mean=9.0, nchw_rstd=7.0, nchw_dx=7.0,
              aff_y=4.0, aff_dx=1.0, aff_sum=20.0, fold=10.0, fold_bwd=9.0)


def limit_from_twin(worst):
    """4 x the twin's worst, rounded up to one significant digit, floor 4."""
    v = 4.0 * worst
    if v <= 4.0:
        return 4.0
    p = 10.0 ** math.floor(math.log10(v))
    return math.ceil(v / p - 1e-9) * p


# ------------------------------------------------------------------------------------------------------------ route arithmetic
def pix_per_wg(B, HW, target=CL_TARGET_DEFAULT):
    p = (B * HW + target - 1) // target
    p = (p + 63) // 64 * 64
    return 128 if p < 128 else 1024 if p > 1024 else p


def cl_route(B, HW, C, target=CL_TARGET_DEFAULT):
    """The launch geometry of a channels-last call, restated from csrc/norm_cl.hip."""
    c4n = C // 4
    lanes_p = 256 // c4n
    ppw = pix_per_wg(B, HW, target)
    return dict(c4n=c4n, lanes_p=lanes_p, idle=256 - lanes_p * c4n, ppw=ppw, wgs=(HW + ppw - 1) // ppw,
                affine_blocks=min(8192, (B * HW * c4n + 255) // 256), affine_trips=-(-(B * HW * c4n) // (8192 * 256)))


# ----------------------------------------------------------------------------------------------------------------- layouts
def to_cl(x):
    """NCHW -> the channels-last storage [B][HW][C], flat."""
    return x.permute(0, 2, 3, 1).contiguous().reshape(-1)


def from_cl(flat, B, H, W, C):
    return flat.reshape(B, H, W, C).permute(0, 3, 1, 2)


def s2d_index(B, H, W, C, mut=""):
    """int64 [B, H, W, C]: the flat float offset of (b, y, x, c) in the space-to-depth storage [B][H/2][W/2][2][2][C], from
    ops.space_to_depth2's statement: channel (sy * 2 + sx) * C + c of output pixel (y', x') is pixel (2 y' + sy, 2 x' + sx)."""
    b = torch.arange(B).view(B, 1, 1, 1)
    y = torch.arange(H).view(1, H, 1, 1)
    x = torch.arange(W).view(1, 1, W, 1)
    c = torch.arange(C).view(1, 1, 1, C)
    sy, sx = y % 2, x % 2
    if mut == "parity":
        sy, sx = sx, sy
    return ((b * (H // 2) + y // 2) * (W // 2) + x // 2) * (4 * C) + (sy * 2 + sx) * C + c


def to_s2d(x):
    """NCHW -> the space-to-depth storage, flat."""
    B, C, H, W = x.shape
    out = torch.empty(B * H * W * C, dtype=x.dtype)
    out[s2d_index(B, H, W, C).reshape(-1)] = x.permute(0, 2, 3, 1).reshape(-1)
    return out


def from_s2d(flat, B, H, W, C, mut=""):
    return flat[s2d_index(B, H, W, C, mut)].permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------------------ designed planes
KINDS = ("normal", "ratio4", "ratio32", "constant", "tiny", "outlier", "zeros")


def plane_kinds(B, C):
    return (torch.arange(B * C) % len(KINDS)).view(B, C)


def designed(B, C, H, W, seed=0):
    """x [B, C, H, W] fp32: plane b C + c is of kind KINDS[(b C + c) % 7]."""
    g = torch.Generator().manual_seed(7919 * seed + 1009 * B + 31 * H * W + C)
    HW = H * W
    x = torch.randn(B, C, HW, generator=g)
    k = plane_kinds(B, C)
    x[k == 1] += 4.0
    x[k == 2] += 32.0
    x[k == 3] = 3.7
    x[k == 4] *= 3e-3
    sel = x[k == 5]
    sel[:, HW // 2] = 1e3
    x[k == 5] = sel
    sel = x[k == 6]
    sel[:, ::10] = 0.0
    x[k == 6] = sel
    return x.view(B, C, H, W)


def gradients(B, C, H, W, seed=0):
    g = torch.Generator().manual_seed(104729 * seed + 1013 * B + 37 * H * W + C + 5)
    return torch.randn(B, C, H, W, generator=g)


def residual(B, C, H, W, seed=0):
    g = torch.Generator().manual_seed(15485863 * seed + 1019 * B + 41 * H * W + C + 9)
    return torch.randn(B, C, H, W, generator=g)


def bn_params(B, C, cbias, seed=0):
    """(weight, bias, rm, rv, cbias or None) fp32 [C]; channels that hold a `zeros` plane in any sample get a shift of exactly 0
    (bias = 0, rm = cbias), so that x = 0 there has the affine image 0."""
    g = torch.Generator().manual_seed(32452843 * seed + C + 3 * B + (1 if cbias else 0))
    w = torch.randn(C, generator=g)
    w = torch.where(w.abs() < 0.1, torch.full_like(w, 0.5), w)
    b, rm, cb = (torch.randn(C, generator=g) for _ in range(3))
    rv = torch.rand(C, generator=g) + 0.1
    z = (plane_kinds(B, C) == 6).any(0)
    b[z] = 0.0
    if cbias:
        rm[z] = cb[z]
    else:
        rm[z] = 0.0
    return w, b, rm, rv, (cb if cbias else None)


# ---------------------------------------------------------------------------------------------------------------- comparator
def need(got, ref, scale, slack=0.0):
    """(worst max(0, |got - ref| - slack) / scale, flat index of it); inf for a non-finite value or an excess where scale is 0."""
    got = got.double()
    ex = ((got - ref).abs() - slack).clamp_min(0)
    r = torch.where(ex == 0, torch.zeros_like(ex), ex / scale)
    r = torch.where(torch.isfinite(got) & ~torch.isnan(r), r, torch.full_like(r, float("inf")))
    i = int(r.argmax())
    return float(r.reshape(-1)[i]), i


def _psum(t):
    return t.sum((2, 3), keepdim=True)


def _kept(H, W, ppw, mut, like):
    """Pixels a mutated statistics pass still sums: 'strip_last' drops the last pixel of the first strip, 'row0' every strip that
    lands in partial row 0 (strip % 8 == 0)."""
    HW = H * W
    k = torch.ones(HW, dtype=like.dtype)
    if mut == "strip_last":
        k[min(ppw, HW) - 1] = 0
    elif mut == "row0":
        k[(torch.arange(HW) // ppw) % CL_NSLOT == 0] = 0
    return k.view(1, 1, H, W)


# ---------------------------------------------------------------------------------------------------------- float64 references
def inorm_ref(x, eps, relu, res=None, mut="", ppw=128):
    """y, mean, rstd of relu?(instance_norm(x)), or of relu(res + relu?(instance_norm(x)))."""
    x = x.double()
    H, W = x.shape[2:]
    HW = H * W
    k = _kept(H, W, ppw, mut, x)
    mean = _psum(x * k) / HW
    var = _psum((x - mean) ** 2 * k) / (HW - 1 if mut == "hw-1" else HW)
    rstd = 1.0 / torch.sqrt(var + (0.0 if mut == "no_eps" else eps))
    y = (x - mean) * rstd
    if relu:
        y = y.clamp_min(0)
    if res is not None:
        y = (y + res.double()).clamp_min(0)
    return y, mean, rstd


def _gate(v, mut):
    return v >= 0 if mut == "lt" else v > 0


def inorm_bwd_ref(g, x, eps, relu, res=None, y=None, mut="", ppw=128, parts=False):
    """dx, dres of the above for the output gradient g; y: the forward result whose sign gates the residual's outer ReLU
    (the reference's own when None).  parts: also (s1, s2) = the plane sums of g' and g' xhat."""
    y0, mean, rstd = inorm_ref(x, eps, relu, res)
    x, g = x.double(), g.double()
    H, W = x.shape[2:]
    HW = H * W
    xhat = (x - mean) * rstd
    dres = None
    if res is not None:
        out = y0 if y is None else y.double()
        dres = g if mut == "dres_early" else None
        if mut != "no_out_mask":
            g = g * (out > 0)
        dres = g if dres is None else dres
    gp = g * _gate(xhat, mut) if relu else g
    k = _kept(H, W, ppw, mut, x)
    s1, s2 = _psum(gp * k), _psum(gp * xhat * k)
    m1, m2 = s1 / HW, s2 / HW
    dx = rstd * (gp - (0.0 if mut == "no_m1" else m1) - xhat * m2)
    return (dx, dres, s1, s2) if parts else (dx, dres)


def affine_ref(x, scale, shift, relu, res=None):
    t = x.double() * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    y = t.clamp_min(0) if relu else t
    if res is not None:
        y = (y + res.double()).clamp_min(0)
    return y


def affine_bwd_ref(g, x, scale, shift, relu, res=None, y=None, mut="", ppw=128):
    """dx, dres, dsum_g [C], dsum_gx [C]."""
    x, g = x.double(), g.double()
    H, W = x.shape[2:]
    a = scale.double().view(1, -1, 1, 1)
    t = x * a + shift.double().view(1, -1, 1, 1)
    dres = None
    if res is not None:
        out = affine_ref(x, scale, shift, relu, res) if y is None else y.double()
        dres = g if mut == "dres_early" else None
        if mut != "no_out_mask":
            g = g * (out > 0)
        dres = g if dres is None else dres
    gp = g * _gate(t, mut) if relu else g
    k = _kept(H, W, ppw, mut, x)
    return gp * a, dres, (gp * k).sum((0, 2, 3)), (gp * x * k).sum((0, 2, 3))


def fold_ref(weight, bias, rm, rv, cbias, eps, mut=""):
    """scale, shift, rs, rmc of a frozen BatchNorm behind a convolution that ran without its bias cbias."""
    w, b, rm, rv = (t.double() for t in (weight, bias, rm, rv))
    rs = 1.0 / torch.sqrt(rv + eps)
    cb = cbias.double() if cbias is not None else torch.zeros_like(rm)
    rmc = rm + cb if mut == "cbias_plus" else rm - cb
    scale = w * rs
    return scale, b - rmc * scale, rs, rmc


def fold_bwd_ref(part, rs, rmc, scale):
    """dweight, dbias, dcbias from part [2][R][C], the partial rows of sum g' and sum g' x."""
    s0, s1 = part[0].double().sum(0), part[1].double().sum(0)
    return rs.double() * (s1 - rmc.double() * s0), s0, scale.double() * s0


# ------------------------------------------------------------------------------------------------------------------ fp32 twins
def inorm_twin(x, eps, relu, res=None, route="cl"):
    """The kernel's formula in float32: single-pass variance on the channels-last route, two passes on the NCHW route."""
    x = x.float()
    HW = x.shape[2] * x.shape[3]
    mean = _psum(x) / HW
    if route == "cl":
        var = (_psum(x * x) / HW - mean * mean).clamp_min(0)
    else:
        d = x - mean
        var = _psum(d * d) / HW
    rstd = torch.rsqrt(var + eps)
    y = (x - mean) * rstd
    if relu:
        y = y.clamp_min(0)
    if res is not None:
        y = (y + res.float()).clamp_min(0)
    return y, mean, rstd


def inorm_bwd_twin(g, x, mean, rstd, relu, y=None):
    """dx, dres, s1, s2 in float32 from the forward twin's statistics and result."""
    x, g = x.float(), g.float()
    HW = x.shape[2] * x.shape[3]
    xhat = (x - mean) * rstd
    dres = None
    if y is not None:
        g = torch.where(y > 0, g, torch.zeros_like(g))
        dres = g
    gp = torch.where(xhat <= 0, torch.zeros_like(g), g) if relu else g
    s1, s2 = _psum(gp), _psum(gp * xhat)
    return rstd * (gp - s1 / HW - xhat * (s2 / HW)), dres, s1, s2


def affine_twin(x, scale, shift, relu, res=None):
    t = x.float() * scale.float().view(1, -1, 1, 1) + shift.float().view(1, -1, 1, 1)
    y = t.clamp_min(0) if relu else t
    if res is not None:
        y = (y + res.float()).clamp_min(0)
    return y


def affine_bwd_twin(g, x, scale, shift, relu, y=None):
    x, g = x.float(), g.float()
    a = scale.float().view(1, -1, 1, 1)
    t = x * a + shift.float().view(1, -1, 1, 1)
    dres = None
    if y is not None:
        g = torch.where(y > 0, g, torch.zeros_like(g))
        dres = g
    gp = torch.where(t <= 0, torch.zeros_like(g), g) if relu else g
    return gp * a, dres, gp.sum((0, 2, 3)), (gp * x).sum((0, 2, 3))


def fold_twin(weight, bias, rm, rv, cbias, eps):
    rs = torch.rsqrt(rv.float() + eps)
    rmc = rm.float() - (cbias.float() if cbias is not None else 0.0)
    scale = weight.float() * rs
    return scale, bias.float() - rmc * scale, rs, rmc


def fold_bwd_twin(part, rs, rmc, scale):
    s0, s1 = part[0].float().sum(0), part[1].float().sum(0)
    return rs * (s1 - rmc * s0), s0, scale * s0


# ------------------------------------------------------------------------------------------------------ expectations with scales
def _route_keys(route):
    return {k: f"{route}_{k}" for k in ("y", "mean", "rstd", "dx", "sum")}


def inorm_expect(x, g, eps, relu, res, route, y=None):
    """{name: (ref, scale, slack, limit key)} for y, mean, rstd, dx, s1, s2 (plane sums of g' and g' xhat) of an instance-norm
    forward + backward; `ambiguous`: the mask of ambiguous elements, `whole`: the planes that are ambiguous as a whole."""
    K = _route_keys(route)
    yr, mean, rstd = inorm_ref(x, eps, relu, res)
    dx, dres, s1, s2 = inorm_bwd_ref(g, x, eps, relu, res, y, parts=True)
    xd, gd = x.double(), g.double()
    HW = x.shape[2] * x.shape[3]
    xhat = (xd - mean) * rstd
    r = mean.abs() * rstd
    if route == "cl":
        rho = U24 * (1 + r * r)
        F = U24 * (xhat.abs() + 1) * (1 + r * r)
    else:
        rho = U24 * torch.ones_like(r)
        F = U24 * (xhat.abs() + 1 + r)
    Fy = F + U24 * yr.abs() if res is not None else F
    if res is not None:
        gd = gd * ((yr if y is None else y.double()) > 0)
    amb = torch.zeros_like(xhat, dtype=torch.bool)
    whole = torch.zeros_like(r, dtype=torch.bool)
    if relu and HW > 1:
        amb = xhat.abs() <= LIMITS[K["y"]] * F
        whole = (xd == mean).all(3, keepdim=True).all(2, keepdim=True)
    gp = gd * (xhat > 0) if relu else gd
    S1, S2, SF = _psum(gp.abs()) / HW, _psum((gp * xhat).abs()) / HW, _psum(gp.abs() * F) / HW
    m1, m2 = s1 / HW, s2 / HW
    A1, A2 = _psum(gd.abs() * amb), _psum((gd * xhat).abs() * amb + gd.abs() * F * amb)
    sdx = dx.abs() * rho + rstd * (U24 * gp.abs() + U24 * S1 + xhat.abs() * (U24 * S2 + SF) + F * m2.abs()
                                   + U24 * (m1.abs() + (xhat * m2).abs()))
    kdx = rstd * (gd.abs() * amb + A1 / HW + (xhat.abs() + F) * A2 / HW)
    exp = dict(y=(yr, Fy, 0.0, K["y"]), mean=(mean, U24 * _psum(xd.abs()) / HW, 0.0, K["mean"]),
               rstd=(rstd, rho * rstd, 0.0, K["rstd"]), dx=(dx, sdx, kdx, K["dx"]), ambiguous=amb, whole=whole)
    if route == "cl":                                    # the partial rows the caller owns (the NCHW kernels keep theirs in registers)
        exp.update(s1=(s1, U24 * S1 * HW, A1, K["sum"]), s2=(s2, U24 * S2 * HW + SF * HW, A2, K["sum"]),
                   sums=(_psum(xd), U24 * _psum(xd.abs()), 0.0, K["sum"]), sumsq=(_psum(xd * xd), U24 * _psum(xd * xd), 0.0, K["sum"]))
    return exp


def affine_expect(x, g, scale, shift, relu, res, y=None):
    """{name: (ref, scale, slack, limit key)} for y, dx, dsum_g, dsum_gx of an affine forward + backward."""
    yr = affine_ref(x, scale, shift, relu, res)
    dx, dres, sg, sgx = affine_bwd_ref(g, x, scale, shift, relu, res, y)
    xd, gd = x.double(), g.double()
    a = scale.double().view(1, -1, 1, 1)
    t = xd * a + shift.double().view(1, -1, 1, 1)
    F = U24 * ((xd * a).abs() + t.abs())
    Fy = F + U24 * yr.abs() if res is not None else F
    if res is not None:
        gd = gd * ((yr if y is None else y.double()) > 0)
    amb = (t.abs() <= LIMITS["aff_y"] * F) & (t != 0) if relu else torch.zeros_like(t, dtype=torch.bool)
    gp = gd * (t > 0) if relu else gd
    return dict(y=(yr, Fy, 0.0, "aff_y"), dx=(dx, U24 * dx.abs(), (gd * a).abs() * amb, "aff_dx"),
                dsum_g=(sg, U24 * gp.abs().sum((0, 2, 3)), (gd.abs() * amb).sum((0, 2, 3)), "aff_sum"),
                dsum_gx=(sgx, U24 * (gp * xd).abs().sum((0, 2, 3)), ((gd * xd).abs() * amb).sum((0, 2, 3)), "aff_sum"),
                ambiguous=amb)


def fold_expect(weight, bias, rm, rv, cbias, eps):
    scale, shift, rs, rmc = fold_ref(weight, bias, rm, rv, cbias, eps)
    return dict(scale=(scale, U24 * scale.abs(), 0.0, "fold"), rs=(rs, U24 * rs, 0.0, "fold"), rmc=(rmc, U24 * rmc.abs(), 0.0, "fold"),
                shift=(shift, U24 * (bias.double().abs() + (rmc * scale).abs()), 0.0, "fold"))


def fold_bwd_expect(part, rs, rmc, scale):
    dw, db, dcb = fold_bwd_ref(part, rs, rmc, scale)
    a0, a1 = part[0].double().abs().sum(0), part[1].double().abs().sum(0)
    return dict(dweight=(dw, U24 * rs.double() * (a1 + rmc.double().abs() * a0), 0.0, "fold_bwd"), dbias=(db, U24 * a0, 0.0, "fold_bwd"),
                dcbias=(dcb, U24 * scale.double().abs() * a0, 0.0, "fold_bwd"))


def ambiguous_share(exp):
    """Share of ambiguous elements, the planes that are ambiguous as a whole (constant, instance norm with relu) left out."""
    amb = exp["ambiguous"]
    if "whole" in exp:
        amb = amb & ~exp["whole"]
    return float(amb.double().mean())
