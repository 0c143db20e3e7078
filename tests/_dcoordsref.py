"""Float64 restatement of the pyramid lookup and of its gradient w.r.t. the query coordinates, the error scale of a query, fp32
twins of the gradient in two summation orders, and the cases the GPU tests of csrc/corr_dcoords.hip run
(tests/test_lookup_dcoords_kernels.py, tests/test_lookup_dcoords_autograd.py).  No GPU here.

The contract (csrc/corr_dcoords.hip).  Level l, window entry (i, j), channel l (2r+1)^2 + i (2r+1) + j (i: the x offset, slow):
    p = c 2^-l + (i - r, j - r),   (x0, y0) = floor(p),   (fx, fy) = p - floor(p)
    v00 = V_l[y0, x0], v01 = V_l[y0, x0+1], v10 = V_l[y0+1, x0], v11 = V_l[y0+1, x0+1]        (0 outside the level)
    out            = (1-fy) ((1-fx) v00 + fx v01) + fy ((1-fx) v10 + fx v11)
    d out / d c_x  = 2^-l ((1-fy) (v01 - v00) + fy (v11 - v10))
    d out / d c_y  = 2^-l ((1-fx) (v10 - v00) + fx (v11 - v01))
    dcoords[b, 0|1, y, x] = sum over l, i, j of dout[b, y, x, channel] * the above
floor() picks, at an integer position, the slope of the cell to the right / below; the jump to zero at an edge of a level is
part of the slope; a level at which |c 2^-l| >= 30000 contributes nothing (the kernels clamp such positions to an all-zero
window).  `left=True` restates the OTHER convention at integer x / y (the cell to the left / above): what separates the two is
the slack a reference whose positions carry rounding noise (grid_sample behind a normalisation) must be given there.

Error scale of a query: S = sum_l 2^-l sum_ij |dout| (|v00| + |v01| + |v10| + |v11|); errors are counted in units of 2^-24 S.

LIMITS: 4 x the worst the fp32 twins (every operation of the expressions above rounded to fp32; the channels added one after
the other, and added pairwise) reach against float64 over `kernel_cases()`, rounded up to one significant digit.  The factor
is four because the kernel's order (per lane over the levels, then across the 64 lanes) is neither twin's.  tests/
test_dcoordsref.py recomputes the twins' worst; the kernels' own figures are in profiles/lookup_dcoords_margins.txt and do not
set the limit.
"""
import functools
import math

import torch

U24 = 2.0 ** -24
FAR = 30000.0

TWIN_WORST = dict(dcoords=1.81)         # sequential 1.803, pairwise 1.775: both at 2x16x24, 4 levels, radius 3, mixed + grid, gaussian
LIMITS = dict(dcoords=8.0)              # limit_from_twin(1.81)


def limit_from_twin(worst):
    """4 x the twin's worst, rounded up to one significant digit."""
    v = 4.0 * worst
    p = 10.0 ** math.floor(math.log10(v))
    return math.ceil(v / p - 1e-9) * p


def need(got, ref, scale):
    """(worst |got - ref| / scale, flat index of it); inf for a non-finite value or a difference where the scale is 0."""
    got = got.double()
    ex = (got - ref).abs()
    r = torch.where(ex == 0, torch.zeros_like(ex), ex / scale)
    r = torch.where(torch.isfinite(got) & ~torch.isnan(r), r, torch.full_like(r, float("inf")))
    i = int(r.argmax())
    return float(r.reshape(-1)[i]), i


# ------------------------------------------------------------------------------------------------------------------ layout
def level_sizes(H, W, nlev):
    return [(H >> l, W >> l) for l in range(nlev)]


def tiled_layout(H, W, nlev):
    """(P, off[l], th[l], tw[l]) of csrc/corr_layout.hpp: level l in 4x4-cell tiles, x-fastest, levels back to back."""
    off, th, tw, o = [], [], [], 0
    for h, w in level_sizes(H, W, nlev):
        off.append(o)
        th.append((h + 3) // 4)
        tw.append((w + 3) // 4)
        o += th[-1] * tw[-1] * 16
    return (o + 31) // 32 * 32, off, th, tw


def tile_rows(levels, H, W, pad_bits=0x7FC0FFEE):
    """levels[l] [Q, h_l, w_l] fp32 -> the tiled-row volume [Q, P]; every pad cell holds the bit pattern `pad_bits` (a NaN: the
    kernels never read them)."""
    P, off, th, tw = tiled_layout(H, W, len(levels))
    Q = levels[0].shape[0]
    vol = torch.full((Q, P), pad_bits, dtype=torch.int32).view(torch.float32)
    for l, lv in enumerate(levels):
        h, w = lv.shape[1:]
        full = torch.full((Q, th[l] * 4, tw[l] * 4), pad_bits, dtype=torch.int32).view(torch.float32)
        full[:, :h, :w] = lv
        t = full.reshape(Q, th[l], 4, tw[l], 4).permute(0, 1, 3, 2, 4).reshape(Q, -1)
        vol[:, off[l]:off[l] + t.shape[1]] = t
    return vol


# ------------------------------------------------------------------------------------------------------------------ inputs
def _gen(*key):
    s = 12345
    for k in key:
        s = (s * 1000003 + (hash(k) if not isinstance(k, str) else sum(ord(c) * 131 ** i for i, c in enumerate(k)))) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def level_values(B, H, W, nlev):
    """Independent gaussian levels [B*H*W, h_l, w_l] (the kernels do not know that a pyramid is pooled)."""
    return [torch.randn(B * H * W, h, w, generator=_gen("vol", B, H, W, nlev, l), dtype=torch.float32)
            for l, (h, w) in enumerate(level_sizes(H, W, nlev))]


def mixed_positions(n, H, W, gen):
    """n positions (x, y), multiples of 1/64: a third anywhere in [-6, W+6] x [-6, H+6], a third exact integers there, a third
    within one cell of an edge of the level-0 plane, inside or outside."""
    def anywhere(m):
        x = torch.randint(-6 * 64, (W + 6) * 64 + 1, (m,), generator=gen).float() / 64
        y = torch.randint(-6 * 64, (H + 6) * 64 + 1, (m,), generator=gen).float() / 64
        return x, y
    k = n // 3
    x0, y0 = anywhere(n - 2 * k)
    x1, y1 = anywhere(k)
    x1, y1 = torch.round(x1), torch.round(y1)
    x2, y2 = anywhere(k)
    d = torch.randint(-64, 65, (2, k), generator=gen).float() / 64
    side = torch.randint(0, 4, (k,), generator=gen)
    x2 = torch.where(side == 0, d[0], torch.where(side == 1, W - 1 + d[0], x2))
    y2 = torch.where(side == 2, d[1], torch.where(side == 3, H - 1 + d[1], y2))
    x, y = torch.cat([x0, x1, x2]), torch.cat([y0, y1, y2])
    p = torch.randperm(n, generator=gen)
    return x[p], y[p]


def coords_values(B, H, W, kind):
    """[B, 2, H, W] fp32 POSITIONS.  mixed: mixed_positions, with the first row of every sample at +-1e6 (all-zero windows:
    the gradient there is exactly 0); zero: a plane of zeros."""
    if kind == "zero":
        return torch.zeros(B, 2, H, W)
    x, y = mixed_positions(B * H * W, H, W, _gen("coords", B, H, W))
    c = torch.stack([x.view(B, H, W), y.view(B, H, W)], 1).contiguous()
    far = torch.tensor([1e6, -1e6]).repeat((W + 1) // 2)[:W]
    c[:, 0, 0, :] = far
    c[:, 1, 0, :] = -far
    return c


def grid(B, H, W):
    ys = torch.arange(H, dtype=torch.float32).view(1, 1, H, 1).expand(B, 1, H, W)
    xs = torch.arange(W, dtype=torch.float32).view(1, 1, 1, W).expand(B, 1, H, W)
    return torch.cat([xs, ys], 1).contiguous()


def dout_kinds(nlev):
    """gaussian, zero, and a one on a single channel for every level's first and last channel (a swapped i / j or a wrong 2^-l
    shows there)."""
    return ["gauss", "zero"] + [f"hot{l}{e}" for l in range(nlev) for e in "fl"]


def dout_values(B, H, W, nlev, radius, kind):
    """[B, H, W, CH] fp32."""
    n2 = (2 * radius + 1) ** 2
    ch = nlev * n2
    if kind == "gauss":
        return torch.randn(B, H, W, ch, generator=_gen("dout", B, H, W, nlev, radius), dtype=torch.float32)
    d = torch.zeros(B, H, W, ch)
    if kind.startswith("hot"):
        l = int(kind[3])
        d[..., l * n2 + (0 if kind[4] == "f" else n2 - 1)] = 1.0
    return d


# ------------------------------------------------------------------------------------------------------------------ the mathematics
def _taps(lv, x0, y0):
    """V[y0 + a, x0 + b] for a, b in {0, 1}: lv [Q, h, w], x0 / y0 [Q, K] integer tensors; zero outside."""
    Q, h, w = lv.shape
    flat = lv.reshape(Q, h * w)
    out = []
    for a in (0, 1):
        for b in (0, 1):
            xi, yi = x0 + b, y0 + a
            ok = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
            v = torch.gather(flat, 1, yi.clamp(0, h - 1) * w + xi.clamp(0, w - 1))
            out.append(torch.where(ok, v, torch.zeros_like(v)))
    return out      # v00, v01, v10, v11


def jacobian(levels, coords, radius, dtype=torch.float64, left=False):
    """Per query and channel: (out weightless value, d out / d c_x, d out / d c_y, A = 2^-l (|v00| + |v01| + |v10| + |v11|)), each
    [Q, CH] in `dtype` with every operation rounded to it.  levels[l] [Q, h, w]; coords [B, 2, H, W] positions."""
    B, _, H, W = coords.shape
    r, n = radius, 2 * radius + 1
    xy = coords.permute(0, 2, 3, 1).reshape(B * H * W, 2).to(dtype)
    off = torch.arange(-r, r + 1, dtype=dtype)
    ox = off.view(n, 1).expand(n, n).reshape(1, n * n)      # slow index: the x offset
    oy = off.view(1, n).expand(n, n).reshape(1, n * n)
    val, dx, dy, A = [], [], [], []
    for l, lv in enumerate(levels):
        s = 1.0 / (1 << l)
        cx, cy = xy[:, 0:1] * s, xy[:, 1:2] * s
        near = (cx.abs() < FAR) & (cy.abs() < FAR)
        cx, cy = torch.where(near, cx, torch.zeros_like(cx)), torch.where(near, cy, torch.zeros_like(cy))
        flx, fly = (torch.ceil(cx) - 1, torch.ceil(cy) - 1) if left else (torch.floor(cx), torch.floor(cy))
        fx, fy = cx - flx, cy - fly
        x0, y0 = flx.long() + ox.long(), fly.long() + oy.long()
        v00, v01, v10, v11 = _taps(lv.to(dtype), x0, y0)
        z = near.to(dtype)
        val.append(z * ((1 - fy) * ((1 - fx) * v00 + fx * v01) + fy * ((1 - fx) * v10 + fx * v11)))
        dx.append(z * (s * ((1 - fy) * (v01 - v00) + fy * (v11 - v10))))
        dy.append(z * (s * ((1 - fx) * (v10 - v00) + fx * (v11 - v01))))
        A.append(z * (s * (v00.abs() + v01.abs() + v10.abs() + v11.abs())))
    return tuple(torch.cat(t, 1) for t in (val, dx, dy, A))


def expect(levels, coords, dout, radius, left=False):
    """(out [B,H,W,CH], dcoords [B,2,H,W], S [B,1,H,W]) in float64."""
    B, _, H, W = coords.shape
    val, dx, dy, A = jacobian(levels, coords, radius, left=left)
    g = dout.reshape(B * H * W, -1).double()
    dc = torch.stack([(g * dx).sum(1), (g * dy).sum(1)], 1).view(B, H, W, 2).permute(0, 3, 1, 2).contiguous()
    S = (g.abs() * A).sum(1).view(B, 1, H, W)
    return val.view(B, H, W, -1), dc, S


def _sum_sequential(t):
    acc = torch.zeros_like(t[:, 0])
    for k in range(t.shape[1]):
        acc = acc + t[:, k]
    return acc


def _sum_pairwise(t):
    n = 1 << (t.shape[1] - 1).bit_length()
    t = torch.cat([t, torch.zeros(t.shape[0], n - t.shape[1], dtype=t.dtype)], 1)
    while t.shape[1] > 1:
        t = t[:, 0::2] + t[:, 1::2]
    return t[:, 0]


def twin(levels, coords, dout, radius, order):
    """dcoords [B,2,H,W] with every operation in fp32; order: 'sequential' or 'pairwise' over the channels."""
    B, _, H, W = coords.shape
    _, dx, dy, _ = jacobian(levels, coords, radius, dtype=torch.float32)
    g = dout.reshape(B * H * W, -1).float()
    add = _sum_sequential if order == "sequential" else _sum_pairwise
    return torch.stack([add(g * dx), add(g * dy)], 1).view(B, H, W, 2).permute(0, 3, 1, 2).contiguous()


# ------------------------------------------------------------------------------------------------------------------ the GPU tests' cases
# B x H x W, num_levels.  1x10x14: levels 10x14, 5x7, 2x3, 1x1 -- each smaller than, or no multiple of, the 4x4 tile and the
# window; 2x16x24; 1x8x8 with 1, 2, 3 levels; 3x5x9 with 2 levels: 135 queries, no multiple of the wave's 4 or the workgroup's 16;
# 2x8x16: 256 queries, an exact multiple of both.
SHAPES = [((1, 10, 14), 4), ((2, 16, 24), 4), ((1, 8, 8), 1), ((1, 8, 8), 2), ((1, 8, 8), 3), ((3, 5, 9), 2), ((2, 8, 16), 4)]
RADII = (3, 4)
COORD_KINDS = ("mixed", "zero")


@functools.lru_cache(maxsize=None)
def case(shape, nlev, radius, ckind, add_grid=False):
    """Everything of one case that does not depend on dout: levels, positions, what the kernel is handed as `coords` (the flow
    when add_grid) and the float64 Jacobian."""
    B, H, W = shape
    levels = level_values(B, H, W, nlev)
    given = coords_values(B, H, W, ckind)
    pos = given + grid(B, H, W) if add_grid else given       # (fp32, as the kernel adds them; exact for these values)
    return dict(levels=levels, given=given, pos=pos, jac=jacobian(levels, pos, radius))


def case_expect(shape, nlev, radius, ckind, add_grid, dkind):
    """(dout [B,H,W,CH] fp32, dcoords float64 [B,2,H,W], S [B,1,H,W])."""
    B, H, W = shape
    c = case(shape, nlev, radius, ckind, add_grid)
    dout = dout_values(B, H, W, nlev, radius, dkind)
    _, dx, dy, A = c["jac"]
    g = dout.reshape(B * H * W, -1).double()
    dc = torch.stack([(g * dx).sum(1), (g * dy).sum(1)], 1).view(B, H, W, 2).permute(0, 3, 1, 2).contiguous()
    return dout, dc, (g.abs() * A).sum(1).view(B, 1, H, W)


def kernel_cases():
    """Every (shape, nlev, radius, coordinate kind, add_grid, dout kind) the kernel tests compare."""
    for shape, nlev in SHAPES:
        for radius in RADII:
            for ckind in COORD_KINDS:
                for add_grid in (False, True):
                    for dkind in dout_kinds(nlev):
                        yield shape, nlev, radius, ckind, add_grid, dkind
