"""Float64 restatement of the coordinate gradient of the memory-efficient lookup (csrc/altcorr_dcoords.hip), its error scale, fp32
twins in two orders, and the cases the GPU tests run (tests/test_altcorr_dcoords_kernels.py, tests/test_altcorr_dcoords_autograd.py).
No GPU here.

The contract is that of tests/_dcoordsref.py, imported unmodified, applied to the volume the alt path never forms:
    V_l[q, y, x] = f1[q] . f2_l[y, x] / sqrt(C)          f1 [B,H,W,C], f2_l [B, H >> l, W >> l, C] channels-last
`expect` forms V_l in float64 from the fp32 inputs and hands the levels to _dcoordsref.jacobian.  `weight_first` is the form the
kernel computes -- the bilinear slopes moved onto the (2r+2)^2 window positions first, then one pass over the feature rows:
    Gx[iy][ix] = sum over aa, cc in {0, 1} of g[ix - cc][iy - aa] (aa ? fy : 1 - fy) (cc ? +1 : -1)
    Gy[iy][ix] = sum over aa, cc in {0, 1} of g[ix - cc][iy - aa] (cc ? fx : 1 - fx) (aa ? +1 : -1)
    dcoords_x  = 1 / sqrt(C) f1[q] . sum_l sum over the positions inside level l of 2^-l Gx[iy][ix] f2_l[y0 - r + iy, x0 - r + ix, :]
-- in float64 (tests/test_altdcoordsref.py holds it to the restatement) and, with every operation rounded to fp32, as a twin.

Error scale of a query.  The rounding of a dot product scales with sum |a| |b|, not with |sum a b|, so the scale is that of
_dcoordsref on the volume of absolute values:
    S = sum_l 2^-l sum_ij |dout| sum over the 4 taps in range of (sum_c |f1_c| |f2_l,c|) / sqrt(C)
Errors are counted in units of 2^-24 S.

LIMITS: _dcoordsref.limit_from_twin (4 x, rounded up to one digit) of the worst either fp32 twin reaches against float64 over
`kernel_cases()`: the weight-first order with the positions, the levels and then the channels added one after the other, and the
volume-first order (fp32 dots, then the slopes of _dcoordsref) with pairwise sums.  The kernel's order -- a lane over the positions
and levels, then up to four channels of a lane, then a tree over the 64 lanes -- is neither.  tests/test_altdcoordsref.py
recomputes the twins' worst; the kernel's own figures are in profiles/altcorr_dcoords_margins.txt and do not set the limit.
"""
import functools
import math

import torch

import _dcoordsref as R

U24 = R.U24
TWIN_WORST = dict(dcoords=2.51)         # weight-first 2.505 (2x16x24, 4 levels, C 32, radius 3, a plane of zeros), volume-first 1.648
LIMITS = dict(dcoords=20.0)             # limit_from_twin(2.51)

C_BASE = 32
SWEEP_SHAPES = [((1, 10, 14), 4), ((3, 5, 9), 2)]
# 4: fewer channels than lanes; 36: under 64 and no multiple of 32; 100: crosses one 64-lane stride, ragged tail; 128: two full
# strides; 256: the register limit
SWEEP_C = (4, 36, 100, 128, 256)


# ------------------------------------------------------------------------------------------------------------------ inputs
def fmap_values(B, H, W, nlev, C):
    """(f1 [B,H,W,C], [f2_l [B, H >> l, W >> l, C]]): independent gaussians per level (the kernel does not know that the levels are
    pooled)."""
    f1 = torch.randn(B, H, W, C, generator=R._gen("f1", B, H, W, nlev, C), dtype=torch.float32)
    f2 = [torch.randn(B, h, w, C, generator=R._gen("f2", B, H, W, nlev, C, l), dtype=torch.float32)
          for l, (h, w) in enumerate(R.level_sizes(H, W, nlev))]
    return f1, f2


# ------------------------------------------------------------------------------------------------------------------ the mathematics
def volumes(f1, f2_levels, dtype=torch.float64, absolute=False):
    """[V_l [B*H*W, h_l, w_l]] = f1 . f2_l / sqrt(C) in `dtype` (of |f1| and |f2_l| when absolute)."""
    B, H, W, C = f1.shape
    a = f1.to(dtype).reshape(B, H * W, C)
    out = []
    for f2 in f2_levels:
        b = f2.to(dtype).reshape(B, -1, C)
        if absolute:
            a_, b_ = a.abs(), b.abs()
        else:
            a_, b_ = a, b
        out.append((torch.einsum("bqc,bpc->bqp", a_, b_) / math.sqrt(C)).reshape(B * H * W, f2.shape[1], f2.shape[2]))
    return out


def expect(f1, f2_levels, coords, dout, radius, left=False):
    """(dcoords [B,2,H,W], S [B,1,H,W]) in float64: _dcoordsref.expect on the explicitly formed float64 volume, S on the volume of
    absolute values."""
    _, dc, _ = R.expect(volumes(f1, f2_levels), coords, dout, radius, left=left)
    _, _, S = R.expect(volumes(f1, f2_levels, absolute=True), coords, dout, radius, left=left)
    return dc, S


def weight_first(f1, f2_levels, coords, douts, radius, dtype=torch.float64):
    """dcoords [D,B,2,H,W] for douts [D,B,H,W,CH] in the order the kernel computes, every operation rounded to `dtype`: per level
    the slopes on the window positions (taps aa, cc in the kernel's order), the positions row by row into one accumulator per
    channel, the levels one after the other, then the channels one after the other, then 1 / sqrt(C)."""
    B, _, H, W = coords.shape
    Q, C, D = B * H * W, f1.shape[-1], douts.shape[0]
    r, n = radius, 2 * radius + 1
    win = n + 1
    xy = coords.permute(0, 2, 3, 1).reshape(Q, 2).to(dtype)
    a = f1.reshape(Q, C).to(dtype)
    g_all = douts.reshape(D, Q, -1).to(dtype)
    bq = torch.arange(Q) // (H * W)
    acc = torch.zeros(2, D, Q, C, dtype=dtype)
    far = torch.tensor(-R.FAR, dtype=dtype)
    for l, f2 in enumerate(f2_levels):
        h, w = f2.shape[1:3]
        s = 1.0 / (1 << l)
        cx, cy = xy[:, 0] * s, xy[:, 1] * s
        cx = torch.where((cx > -R.FAR) & (cx < R.FAR), cx, far)          # the kernels' clamp: the window misses the map
        cy = torch.where((cy > -R.FAR) & (cy < R.FAR), cy, far)
        flx, fly = torch.floor(cx), torch.floor(cy)
        fx, fy = (cx - flx).view(1, Q, 1, 1), (cy - fly).view(1, Q, 1, 1)
        x0, y0 = flx.long() - r, fly.long() - r
        gp = torch.zeros(D, Q, n + 2, n + 2, dtype=dtype)                 # g[i][j] at [i + 1][j + 1], zeros around
        gp[:, :, 1:-1, 1:-1] = g_all[:, :, l * n * n:(l + 1) * n * n].reshape(D, Q, n, n)
        Gx = torch.zeros(D, Q, win, win, dtype=dtype)                     # [ix][iy]
        Gy = torch.zeros(D, Q, win, win, dtype=dtype)
        for aa in (0, 1):
            for cc in (0, 1):
                v = gp[:, :, 1 - cc:1 - cc + win, 1 - aa:1 - aa + win]   # g[ix - cc][iy - aa]
                Gx = Gx + v * (fy if aa else 1 - fy) * (1.0 if cc else -1.0)
                Gy = Gy + v * (fx if cc else 1 - fx) * (1.0 if aa else -1.0)
        G = torch.stack([Gx, Gy]) * s                                     # [2, D, Q, ix, iy]
        rows = f2.to(dtype)
        for iy in range(win):
            y = y0 + iy
            for ix in range(win):
                x = x0 + ix
                ok = ((x >= 0) & (x < w) & (y >= 0) & (y < h)).to(dtype)
                row = rows[bq, y.clamp(0, h - 1), x.clamp(0, w - 1)]      # [Q, C]
                acc = acc + (G[:, :, :, ix, iy] * ok).unsqueeze(-1) * row
    tot = torch.zeros(2, D, Q, dtype=dtype)
    for c in range(C):
        tot = tot + a[:, c] * acc[..., c]
    tot = tot * torch.tensor(1.0 / math.sqrt(C), dtype=dtype)
    return tot.view(2, D, B, H, W).permute(1, 2, 0, 3, 4).contiguous()


def _dots_pairwise(f1, f2):
    """V [B*H*W, h, w] in fp32: products added pairwise over the channels, then times 1 / sqrt(C)."""
    B, H, W, C = f1.shape
    out = []
    for b in range(B):
        t = f1[b].reshape(H * W, 1, C) * f2[b].reshape(1, -1, C)
        n = 1 << (C - 1).bit_length()
        t = torch.cat([t, torch.zeros(t.shape[0], t.shape[1], n - C)], 2)
        while t.shape[2] > 1:
            t = t[:, :, 0::2] + t[:, :, 1::2]
        out.append(t[:, :, 0])
    return (torch.cat(out) * torch.tensor(1.0 / math.sqrt(C), dtype=torch.float32)).reshape(B * H * W, f2.shape[1], f2.shape[2])


def volume_first(f1, f2_levels, coords, douts, radius):
    """dcoords [D,B,2,H,W], every operation in fp32: the dots (pairwise over the channels), then the slopes of _dcoordsref on them,
    added pairwise over the output channels."""
    B, _, H, W = coords.shape
    _, dx, dy, _ = R.jacobian([_dots_pairwise(f1, f2) for f2 in f2_levels], coords, radius, dtype=torch.float32)
    out = []
    for dout in douts:
        g = dout.reshape(B * H * W, -1).float()
        out.append(torch.stack([R._sum_pairwise(g * dx), R._sum_pairwise(g * dy)], 1).view(B, H, W, 2).permute(0, 3, 1, 2))
    return torch.stack(out).contiguous()


# ------------------------------------------------------------------------------------------------------------------ the GPU tests' cases
def case_keys():
    """Every (shape, nlev, C, radius, coordinate kind, add_grid): _dcoordsref.SHAPES at C = 32, and the channel sweep on 1x10x14
    (4 levels) and 3x5x9 (2 levels: 135 queries, a multiple of neither the wave's 4 nor 16)."""
    for shapes, cs in ((R.SHAPES, (C_BASE,)), (SWEEP_SHAPES, SWEEP_C)):
        for shape, nlev in shapes:
            for C in cs:
                for radius in R.RADII:
                    for ckind in R.COORD_KINDS:
                        for add_grid in (False, True):
                            yield shape, nlev, C, radius, ckind, add_grid


def kernel_cases():
    """Every (shape, nlev, C, radius, coordinate kind, add_grid, dout kind) the kernel tests compare."""
    for key in case_keys():
        for dkind in R.dout_kinds(key[1]):
            yield key + (dkind,)


@functools.lru_cache(maxsize=4)
def case(shape, nlev, C, radius, ckind, add_grid=False):
    """Everything of one case that does not depend on dout: the maps, the positions, what the kernel is handed as `coords` (the
    flow when add_grid), the float64 Jacobian of the formed volume and the A of the volume of absolute values."""
    B, H, W = shape
    f1, f2 = fmap_values(B, H, W, nlev, C)
    given = R.coords_values(B, H, W, ckind)
    pos = given + R.grid(B, H, W) if add_grid else given       # (fp32, as the kernel adds them; exact for these values)
    _, dx, dy, _ = R.jacobian(volumes(f1, f2), pos, radius)
    A = R.jacobian(volumes(f1, f2, absolute=True), pos, radius)[3]
    return dict(f1=f1, f2=f2, given=given, pos=pos, jac=(dx, dy, A))


def case_expect(shape, nlev, C, radius, ckind, add_grid, dkind):
    """(dout [B,H,W,CH] fp32, dcoords float64 [B,2,H,W], S [B,1,H,W])."""
    B, H, W = shape
    dx, dy, A = case(shape, nlev, C, radius, ckind, add_grid)["jac"]
    dout = R.dout_values(B, H, W, nlev, radius, dkind)
    g = dout.reshape(B * H * W, -1).double()
    dc = torch.stack([(g * dx).sum(1), (g * dy).sum(1)], 1).view(B, H, W, 2).permute(0, 3, 1, 2).contiguous()
    return dout, dc, (g.abs() * A).sum(1).view(B, 1, H, W)


def worst_of_twins(report=None):
    """The worst either fp32 twin reaches against float64 over kernel_cases(), in units of 2^-24 S."""
    worst = 0.0
    for key in case_keys():
        shape, nlev, C, radius, ckind, add_grid = key
        c = case(*key)
        trip = [case_expect(*key, dkind) for dkind in R.dout_kinds(nlev)]
        douts = torch.stack([t[0] for t in trip])
        for name, got in (("weight-first sequential", weight_first(c["f1"], c["f2"], c["pos"], douts, radius, dtype=torch.float32)),
                          ("volume-first pairwise", volume_first(c["f1"], c["f2"], c["pos"], douts, radius))):
            for (_, dc, S), g in zip(trip, got):
                w, _ = R.need(g, dc, (S * U24).expand_as(dc))
                if report is not None and w > worst:
                    report(f"{w:.4f} {name} {key}")
                worst = max(worst, w)
    return worst
