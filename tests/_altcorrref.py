"""Float64 restatements of the memory-efficient correlation lookup (csrc/altcorr.hip: the fused forward on its three kernels, and
the alt_cuda_corr.forward / .backward drop-ins), their error scales, fp32 twins, a host model of the two region geometries, the
coordinate families and the cases the GPU tests run (tests/test_altcorr_kernels.py).  Checked on the CPU by
tests/test_altcorrref.py.  No GPU here.

The contract.
    fused forward   out = _corrref.lookup(_altdcoordsref.volumes(f1, f2_levels), pos, radius): the lookup of the volume the alt path
                    never forms, V_l[q, y, x] = f1[q] . f2_l[y, x] / sqrt(C); channel l (2r+1)^2 + i (2r+1) + j, i the x offset
                    (slow); zero outside a level; a level at which |pos 2^-l| >= 30000 (or pos is not finite) gives exactly 0.
    drop-in forward fsraft_altcorr_fwd: one level, UNSCALED, N coordinate sets per pixel, fmap2 of any size H2 x W2:
                    corr[b, n, i (2r+1) + j, y, x] = bilinear(f1[b, y, x] . f2[b], coords[b, n, y, x] + (i - r, j - r))
    drop-in backward fmap1_grad, fmap2_grad = torch.autograd through the float64 drop-in forward (`dropin_bwd`); `dropin_bwd_explicit`
                    is the order the kernel computes in -- the blend transposed onto the (2r+2)^2 window positions first, then one
                    pass over the feature rows -- and tests/test_altcorrref.py holds it to the autograd result.

Error scales, u = 2^-24.  Forward: S = the same lookup on the volume of |f1| . |f2_l| (the rounding of a dot product scales with
sum |a| |b|).  Backward: S1 = sum |g| w |f2| per element of fmap1_grad, S2 = the scatter of |g| w |f1| per element of fmap2_grad (the
gradient of the forward of the absolute values under |g|).  The fp32 routes count in units of u S, the matrix-pipe route in units of
_corrref.G16 S (2^-16: bf16x3 products), for every element, the ones its fp32 fallback serves included.

LIMITS[key] = limit_from_twin(TWIN_WORST[key]) (4 x, rounded up to one digit) of the worst the fp32 twins reach against float64 over
exactly the cases the GPU tests run; tests/test_altcorrref.py recomputes them.  The kernels' orders -- a lane over every 64th channel
and a butterfly over the lanes; four channels at a time from LDS; fp32 atomics -- are none of these.  The twins:
    fwd    dots over the channels in order, and pairwise; the four-weight blend in the kernels' expression order; * fp32(1/sqrt(C))
    mfma   hi = bf16(x), lo = bf16(x - hi); hi hi + hi lo + lo hi in one fp32 chain; blend and scale as above
    bwd    the weights-onto-positions form in fp32; fmap1_grad over (set, position) in order, and pairwise; fmap2_grad with every
           query's contributions added in query order, and pairwise over the queries
Twins' worst, in the units above, and the case each occurred in (the kernels' own figures, which set nothing, are in
profiles/altcorr_margins.txt and in the docstring of tests/test_altcorr_kernels.py):
    fwd     4.999  limit 20   1x32x48, 4 levels, C 36, radius 3, mixed (the in-order chain; pairwise stays below it)
    mfma    0.4987 limit 2    1x32x48, 4 levels, C 32, radius 3, a plane of zeros (the dropped lo lo products and the two lo
                              roundings, which no order of the fp32 accumulation changes; 32 gaussian products average them)
    bwd     5.033  limit 30   1x10x14, C 256, one set, fmap2 of the same size, mixed, radius 3, gaussian corr_grad (in-order)
The kernels' worst on MI355X, for comparison only: wave-per-query 2.96, tile 2.62, drop-in forward 2.66 (of 20); matrix pipe 0.49 (of
2); backward 4.12 (of 30).

The region plane is PLANE = 1x32x48 with four levels (32x48, 16x24, 8x12, 4x6): the smallest plane on which the model below proves
the conditions the region families must meet (on 1x10x14 about 81 % of the outputs have S = 0: the coarse levels are tiny -- fine for
the wave-per-query kernels, no ground for a statement about regions).

The model (`origins`, `region`, `states`): for positions, a level and a radius, every (query, window position) is outside the level,
inside and covered by its tile's staged region, or inside and on the fallback.
    tile kernel         4x4 queries, region 16x16 at (window origin of the tile's query 0) - 1
    matrix-pipe kernel  6x4 queries, region RW x RH (17x15 at radius 4 / 15x13 at radius 3 for level 0; 14x13, 13x12, 12x12 for levels
                        1..3) at the component-wise minimum of the window origins of the tile's in-image queries
It only proves that the inputs reach both branches (and drives the mutants); it is never the expected value.

Coordinate families (multiples of 1/64; `given` is what the kernel is handed: the positions, or positions - grid with add_grid):
    mixed, zero   _dcoordsref.coords_values (any plane)
    smooth        grid + (3.25, -1.75) + a stretch of 1/64 per pixel: no fallback in either kernel
    jump          smooth + 11 in x from column 26, - 7 in y from row 14: motion boundaries through the middle of tiles
    limit-K       K in tile, mfma: smooth, and per level 0 / 1, axis and side two tiles whose queries all sit at one position but one,
                  which sits at the last fully covered offset / one cell beyond it (displacement d 2^l); for levels 2 and 3 a tile
                  whose region ends in the middle of the level
    far-K         smooth, and seven tiles whose anchoring query (tile: query 0; mfma: query (1, 1)) holds NaN, +inf, -inf, 1e6, 30000,
                  -30000, 29999.984375 in x and y
"""
import functools

import torch

import _altdcoordsref as AD
import _corrref as K
import _dcoordsref as D
from _convref import bf16_hi_lo

U24, G16, FAR = D.U24, K.G16, D.FAR
UNIT = dict(fwd=U24, mfma=G16, bwd=U24)
TWIN_WORST = dict(fwd=5.0, mfma=0.499, bwd=5.04)
LIMITS = {k: D.limit_from_twin(v) for k, v in TWIN_WORST.items()}        # 20, 2, 30

PLANE = ((1, 32, 48), 4)
RADII = D.RADII
ROUTES = ("wave", "tile", "mfma")
# wave: 1 / 4 fewer channels than lanes, 36 no multiple of 32, 65 one over a round of lanes, 100 ragged, 128, 256 the register limit;
# tile: one to four staged chunks of 64; mfma: 96 gives an odd trip count of the ring
ROUTE_C = dict(wave=(1, 4, 36, 65, 100, 128, 256), tile=(64, 128, 192, 256), mfma=(32, 96, 256))
BASE_C = dict(wave=36, tile=64, mfma=32)
PLANE_FAMILIES = dict(wave=("mixed", "smooth", "jump"),
                      tile=("mixed", "zero", "smooth", "jump", "limit-tile", "far-tile"),
                      mfma=("mixed", "zero", "smooth", "jump", "limit-mfma", "far-mfma"))
FAR_VALUES = (float("nan"), float("inf"), float("-inf"), 1e6, 30000.0, -30000.0, 29999.984375)
TILE = dict(tile=(4, 4), mfma=(4, 6))           # (queries high, queries wide)
ANCHOR = dict(tile=(0, 0), mfma=(1, 1))         # the query of a tile the far family moves; (1, 1) is also the one `limit` displaces


def limit_key(route):
    return "mfma" if route == "mfma" else "fwd"


# ------------------------------------------------------------------------------------------------------------------ the mathematics
def expect_fused(f1, f2_levels, pos, radius):
    """(out [B,H,W,CH], S [B,H,W,CH]) in float64."""
    ref, _ = K.lookup(AD.volumes(f1, f2_levels), pos, radius)
    S, _ = K.lookup(AD.volumes(f1, f2_levels, absolute=True), pos, radius)
    return ref, S


def volume1(f1, f2, dtype=torch.float64):
    """V [B*H1*W1, H2, W2] = f1 . f2, unscaled, in `dtype` (differentiable in both maps)."""
    B, H1, W1, C = f1.shape
    v = torch.einsum("bqc,bpc->bqp", f1.to(dtype).reshape(B, H1 * W1, C), f2.to(dtype).reshape(B, -1, C))
    return v.reshape(B * H1 * W1, f2.shape[1], f2.shape[2])


def dropin_fwd(f1, f2, coords, radius, dtype=torch.float64):
    """corr [B,N,(2r+1)^2,H1,W1] of fsraft_altcorr_fwd: f1 [B,H1,W1,C], f2 [B,H2,W2,C], coords [B,N,H1,W1,2] (x, y)."""
    V = volume1(f1, f2, dtype)
    outs = []
    for n in range(coords.shape[1]):
        o, _ = K.lookup([V], coords[:, n].permute(0, 3, 1, 2), radius, dtype=dtype)
        outs.append(o.permute(0, 3, 1, 2))
    return torch.stack(outs, 1)


def dropin_expect(f1, f2, coords, radius):
    """(corr, S) in float64."""
    return dropin_fwd(f1, f2, coords, radius), dropin_fwd(f1.abs(), f2.abs(), coords, radius)


def dropin_bwd(f1, f2, coords, g, radius):
    """(fmap1_grad, fmap2_grad, S1, S2) in float64, by torch.autograd through dropin_fwd."""
    a, b = f1.double().requires_grad_(), f2.double().requires_grad_()
    g1, g2 = torch.autograd.grad(dropin_fwd(a, b, coords, radius), (a, b), g.double())
    a, b = f1.double().abs().requires_grad_(), f2.double().abs().requires_grad_()
    S1, S2 = torch.autograd.grad(dropin_fwd(a, b, coords, radius), (a, b), g.double().abs())
    return g1, g2, S1, S2


def _clamped(c):
    """The kernels' clamp in the dtype of c: a position that is not inside (-30000, 30000) -- NaN included -- becomes -30000."""
    return torch.where((c > -FAR) & (c < FAR), c, torch.full_like(c, -FAR))


def _position_weights(coords_n, g_n, radius, dtype):
    """Per query the (2r+2)^2 position weights G [Q, iy, ix] = blend^T(corr_grad) in the kernel's expression order, and the window
    origins (x0, y0) [Q]: coords_n [B,H1,W1,2], g_n [B,(2r+1)^2,H1,W1]."""
    B, H1, W1, _ = coords_n.shape
    Q, r, n = B * H1 * W1, radius, 2 * radius + 1
    xy = _clamped(coords_n.reshape(Q, 2).to(dtype))
    fl = torch.floor(xy)
    fx, fy = (xy[:, 0] - fl[:, 0]).view(Q, 1, 1), (xy[:, 1] - fl[:, 1]).view(Q, 1, 1)
    gp = torch.zeros(Q, n + 2, n + 2, dtype=dtype)                      # gout[ixo][iyo] at [ixo + 1][iyo + 1], zeros around
    gp[:, 1:-1, 1:-1] = g_n.to(dtype).reshape(B, n, n, H1 * W1).permute(0, 3, 1, 2).reshape(Q, n, n)
    G = torch.zeros(Q, n + 1, n + 1, dtype=dtype)                       # [iy][ix]
    one = torch.ones((), dtype=dtype)
    for aa in (0, 1):
        for cc in (0, 1):
            v = gp[:, 1 - cc:n + 2 - cc, 1 - aa:n + 2 - aa].transpose(1, 2)     # gout[ix - cc][iy - aa] as [iy][ix]
            G = G + v * (fy if aa else one - fy) * (fx if cc else one - fx)
    return G, fl[:, 0].long() - r, fl[:, 1].long() - r


def dropin_bwd_explicit(f1, f2, coords, g, radius, dtype=torch.float64, order="seq"):
    """(fmap1_grad, fmap2_grad) in the weights-onto-positions-first form, every operation rounded to `dtype`.  order 'seq':
    fmap1_grad over (set, position) in order, fmap2_grad query after query; 'pair': both sums pairwise."""
    B, H1, W1, C = f1.shape
    H2, W2 = f2.shape[1:3]
    N, Qb, win = coords.shape[1], H1 * W1, 2 * radius + 2
    a_all, rows_all = f1.to(dtype).reshape(B, Qb, C), f2.to(dtype).reshape(B, H2 * W2, C)
    per_set = [_position_weights(coords[:, n], g[:, n], radius, dtype) for n in range(N)]
    g1, g2 = [], []
    for b in range(B):
        a, rows = a_all[b], rows_all[b]
        sl = slice(b * Qb, (b + 1) * Qb)
        terms = []
        contrib = torch.zeros(Qb, H2 * W2, C, dtype=dtype)              # what every query adds to fmap2_grad
        qi = torch.arange(Qb)
        for G, x0, y0 in per_set:
            for iy in range(win):
                for ix in range(win):
                    x, y = x0[sl] + ix, y0[sl] + iy
                    ok = (x >= 0) & (x < W2) & (y >= 0) & (y < H2)
                    cell = y.clamp(0, H2 - 1) * W2 + x.clamp(0, W2 - 1)
                    w = (G[sl, iy, ix] * ok.to(dtype)).unsqueeze(1)
                    terms.append(w * rows[cell])
                    contrib[qi, cell] = contrib[qi, cell] + w * a
        t = torch.stack(terms, 1)                                       # [Qb, N win^2, C]
        if order == "seq":
            acc1 = torch.zeros(Qb, C, dtype=dtype)
            for k in range(t.shape[1]):
                acc1 = acc1 + t[:, k]
            acc2 = torch.zeros(H2 * W2, C, dtype=dtype)
            for q in range(Qb):
                acc2 = acc2 + contrib[q]
        else:
            acc1 = D._sum_pairwise(t.permute(0, 2, 1).reshape(Qb * C, -1)).view(Qb, C)
            acc2 = D._sum_pairwise(contrib.reshape(Qb, -1).t()).view(H2 * W2, C)
        g1.append(acc1)
        g2.append(acc2)
    return torch.stack(g1).view(B, H1, W1, C), torch.stack(g2).view(B, H2, W2, C)


# ------------------------------------------------------------------------------------------------------------------ fp32 twins
def _pairwise_dots(a, b, C):
    """sum_c a[:, c] (x) b[:, c] added pairwise over the channels (zero-padded to a power of two), nothing larger than the result
    kept: a [Q, C], b [P, C] fp32 -> [Q, P]."""
    def rec(lo, n):
        if lo >= C:
            return None
        if n == 1:
            return a[:, lo:lo + 1] * b[:, lo].unsqueeze(0)
        left, right = rec(lo, n // 2), rec(lo + n // 2, n // 2)
        return left if right is None else left + right
    return rec(0, 1 << (C - 1).bit_length() if C > 1 else 1)


def dots32(f1, f2_levels, order):
    """[V_l [B*H*W, h_l, w_l]] unscaled, every operation in fp32.  order: 'seq' (channels in order), 'pair' (pairwise), 'bf16x3'
    (hi hi + hi lo + lo hi in one chain; the product of two bf16 numbers is exact in fp32), 'bf16x1' (hi hi only: a mutant)."""
    B, H, W, C = f1.shape
    out = []
    for f2 in f2_levels:
        lv = []
        for bb in range(B):
            a, b = f1[bb].reshape(H * W, C).float(), f2[bb].reshape(-1, C).float()
            if order == "pair":
                acc = _pairwise_dots(a, b, C)
            else:
                acc = torch.zeros(a.shape[0], b.shape[0])
                (ah, al), (bh, bl) = bf16_hi_lo(a), bf16_hi_lo(b)
                for c in range(C):
                    if order == "seq":
                        acc = acc + a[:, c:c + 1] * b[:, c].unsqueeze(0)
                    else:
                        acc = acc + ah[:, c:c + 1] * bh[:, c].unsqueeze(0)
                        if order == "bf16x3":
                            acc = acc + ah[:, c:c + 1] * bl[:, c].unsqueeze(0)
                            acc = acc + al[:, c:c + 1] * bh[:, c].unsqueeze(0)
            lv.append(acc)
        out.append(torch.cat(lv).reshape(B * H * W, f2.shape[1], f2.shape[2]))
    return out


def blend32(vols32, pos, radius, C):
    """The four-weight blend of the kernels in fp32 on unscaled fp32 dots, then * fp32(1 / sqrt(C))."""
    o, _ = K.lookup(vols32, pos, radius, dtype=torch.float32, form="weights")
    return o * (1.0 / torch.tensor(float(C), dtype=torch.float32).sqrt())


# ------------------------------------------------------------------------------------------------------------------ the geometry model
def region_size(kernel, l, radius):
    """(RW, RH) of a tile's staged region at level l."""
    if kernel == "tile":
        return 16, 16
    return (6 + 2 * radius + 3 if l == 0 else (14, 13, 12)[l - 1]), (4 + 2 * radius + 3 if l == 0 else 13 if l == 1 else 12)


def origins(pos, l, radius):
    """Window origins (wx0, wy0) [B,H,W] (long) of every query at level l, as the kernels compute them in fp32."""
    c = _clamped(pos.float() * (1.0 / (1 << l)))
    fl = torch.floor(c).long() - radius
    return fl[:, 0], fl[:, 1]


def region(pos, l, radius, kernel, clamp=True):
    """Region origins (rx0, ry0) [B,H,W]: every query's own tile's.  clamp=False: the mutant that takes far positions as given
    (non-finite ones stay at -30000)."""
    if clamp:
        wx0, wy0 = origins(pos, l, radius)
    else:
        c = pos.float() * (1.0 / (1 << l))
        c = torch.where(torch.isfinite(c), c, torch.full_like(c, -FAR))
        wx0, wy0 = torch.floor(c[:, 0]).long() - radius, torch.floor(c[:, 1]).long() - radius
    B, H, W = wx0.shape
    th, tw = TILE[kernel]
    yy, xx = torch.arange(H), torch.arange(W)
    if kernel == "tile":
        y0, x0 = (yy // th) * th, (xx // tw) * tw
        return wx0[:, y0][:, :, x0] - 1, wy0[:, y0][:, :, x0] - 1
    Hp, Wp = -(-H // th) * th, -(-W // tw) * tw
    out = []
    for w0 in (wx0, wy0):
        p = torch.full((B, Hp, Wp), 2 ** 40, dtype=torch.long)
        p[:, :H, :W] = w0
        m = p.view(B, Hp // th, th, Wp // tw, tw).amin((2, 4))
        out.append(m[:, yy // th][:, :, xx // tw])
    return out[0], out[1]


OUTSIDE, COVERED, FALLBACK = 0, 1, 2


def states(pos, l, radius, hw, kernel, clamp=True):
    """[B,H,W,iy,ix] of OUTSIDE / COVERED / FALLBACK for every (query, window position) at level l of size hw."""
    h, w = hw
    wx0, wy0 = origins(pos, l, radius)
    rx0, ry0 = region(pos, l, radius, kernel, clamp)
    RW, RH = region_size(kernel, l, radius)
    k = torch.arange(2 * radius + 2)
    gx = wx0[..., None, None] + k.view(1, -1)
    gy = wy0[..., None, None] + k.view(-1, 1)
    inimg = (gx >= 0) & (gx < w) & (gy >= 0) & (gy < h)
    ux, uy = gx - rx0[..., None, None], gy - ry0[..., None, None]
    cov = (ux >= 0) & (ux < RW) & (uy >= 0) & (uy < RH)
    return torch.where(inimg, torch.where(cov, COVERED, FALLBACK), OUTSIDE)


def cell_cover(pos, l, radius, hw, kernel):
    """[B*H*W, h, w] bool: the query's tile's region holds the cell."""
    h, w = hw
    rx0, ry0 = region(pos, l, radius, kernel)
    RW, RH = region_size(kernel, l, radius)
    x, y = torch.arange(w).view(1, 1, w), torch.arange(h).view(1, h, 1)
    rx0, ry0 = rx0.reshape(-1, 1, 1), ry0.reshape(-1, 1, 1)
    return (x >= rx0) & (x < rx0 + RW) & (y >= ry0) & (y < ry0 + RH)


def element_use(pos, l, radius, hw, kernel):
    """Per output element [B,H,W,(2r+1)^2] (x offset slow) of level l: (taps inside the level 0..4, a tap with weight > 0 is covered,
    a tap with weight > 0 is on the fallback)."""
    st = states(pos, l, radius, hw, kernel)
    n = 2 * radius + 1
    c = _clamped(pos.float() * (1.0 / (1 << l)))
    fr = c - torch.floor(c)
    fx, fy = fr[:, 0, ..., None, None], fr[:, 1, ..., None, None]
    inside = torch.zeros(st.shape[:3] + (n, n), dtype=torch.long)
    cov = torch.zeros_like(inside, dtype=torch.bool)
    fb = torch.zeros_like(cov)
    for aa in (0, 1):
        for cc in (0, 1):
            s = st[..., aa:aa + n, cc:cc + n]                           # [iyo][ixo]
            wgt = (fy if aa else 1 - fy) * (fx if cc else 1 - fx) > 0
            inside += (s != OUTSIDE).long()
            cov |= (s == COVERED) & wgt
            fb |= (s == FALLBACK) & wgt
    flat = lambda t: t.transpose(-1, -2).reshape(t.shape[:3] + (n * n,))   # noqa: E731  (channel = iyo + n ixo)
    return flat(inside), flat(cov), flat(fb)


# ------------------------------------------------------------------------------------------------------------------ coordinate families
def _smooth(H, W):
    g = D.grid(1, H, W)
    x, y = g[:, 0], g[:, 1]
    return torch.stack([x + 3.25 + (x + 2 * y) / 64, y - 1.75 + y / 64], 1)


def _put(pos, kernel, t, P, local=None):
    """Every query of tile t (or its query `local`) of the plane to position P = (x, y)."""
    th, tw = TILE[kernel]
    ty, tx = divmod(t, -(-pos.shape[3] // tw))
    if local is None:
        pos[0, 0, ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw] = P[0]
        pos[0, 1, ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw] = P[1]
    else:
        pos[0, 0, ty * th + local[0], tx * tw + local[1]] = P[0]
        pos[0, 1, ty * th + local[0], tx * tw + local[1]] = P[1]


def limit_offsets(kernel, l, radius, axis):
    """The last fully covered offset of a displaced query on either side: (low, high).  tile: the origin may differ from query
    0's by -1 .. 15 - (2r+2); mfma: the spread may reach RW - (2r+2) in x, RH - (2r+2) in y, in either direction."""
    if kernel == "tile":
        return -1, 15 - (2 * radius + 2)
    d = region_size(kernel, l, radius)[axis] - (2 * radius + 2)
    return -d, d


@functools.lru_cache(maxsize=None)
def plane_positions(family, radius):
    """(pos [1,2,32,48], meta): meta lists what each special tile is for -- dict(tile, level, kind, ...)."""
    (B, H, W), nlev = PLANE
    sizes = D.level_sizes(H, W, nlev)
    pos, meta = _smooth(H, W), []
    if family == "smooth":
        return pos, meta
    if family == "jump":
        pos[:, 0, :, 26:] += 11.0
        pos[:, 1, 14:, :] -= 7.0
        return pos, meta
    name, kernel = family.split("-")
    r, t = radius, 0
    if name == "far":
        for v in FAR_VALUES:
            _put(pos, kernel, t, (v, v), ANCHOR[kernel])
            meta.append(dict(tile=t, kind="far", value=v))
            t += 1
        return pos, meta
    assert name == "limit"
    for l in (0, 1):
        k = float(1 << l)
        for axis in (0, 1):
            lo, hi = limit_offsets(kernel, l, r, axis)
            for side, last, step in (("low", lo, -1), ("high", hi, 1)):
                for beyond in (0, 1):
                    # positions in cells of level l: the window of the tile's queries and of the displaced one, and the first
                    # position beyond the region, stay inside the level; the fraction .5 gives every tap a weight
                    F = [5.5, 5.5]
                    F[axis] = (r + 3 if side == "low" else 1) + 0.5
                    _put(pos, kernel, t, (F[0] * k, F[1] * k))
                    F[axis] += last + step * beyond
                    _put(pos, kernel, t, (F[0] * k, F[1] * k), (1, 1))
                    meta.append(dict(tile=t, kind="limit", level=l, axis=axis, side=side, beyond=beyond))
                    t += 1
    for l in (2, 3):
        # the region ends in the middle of the level: cells left of w_l / 2 covered, the others on the fallback
        k = float(1 << l)
        h, w = sizes[l]
        RW, _ = region_size(kernel, l, r)
        rx0 = w // 2 - RW
        Fy = h // 2 - 1 + 0.5
        _put(pos, kernel, t, ((w // 2 - 1 + 0.5) * k, Fy * k))
        _put(pos, kernel, t, ((rx0 + r + (1 if kernel == "tile" else 0) + 0.5) * k, Fy * k), ANCHOR[kernel])
        meta.append(dict(tile=t, kind="split", level=l))
        t += 1
    return pos, meta


def tile_mask(kernel, t, H, W):
    """[H, W] bool: the queries of tile t."""
    th, tw = TILE[kernel]
    ty, tx = divmod(t, -(-W // tw))
    m = torch.zeros(H, W, dtype=torch.bool)
    m[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw] = True
    return m


def positions(shape, family, radius, add_grid):
    """(given, pos) [B,2,H,W] fp32: what the kernel is handed and the positions it must use.  mixed / zero: pos = given + grid in
    fp32 as the kernel adds them (exact: multiples of 1/64); the plane's families fix pos and hand over pos - grid."""
    B, H, W = shape
    if family in D.COORD_KINDS:
        given = D.coords_values(B, H, W, family)
        return given, (given + D.grid(B, H, W) if add_grid else given)
    assert (shape, 4) == PLANE, "the region families are defined on the region plane"
    pos = plane_positions(family, radius)[0]
    given = pos - D.grid(B, H, W) if add_grid else pos
    if add_grid:
        back = given + D.grid(B, H, W)
        assert bool(((back == pos) | (back.isnan() & pos.isnan())).all())
    return given.clone(), pos.clone()


# ------------------------------------------------------------------------------------------------------------------ the GPU tests' cases
def groups(route):
    """[(shape, nlev, C, families)]: _dcoordsref.SHAPES at the route's base channel count and the channel sweep on 1x10x14 (4 levels)
    and 3x5x9 (2 levels), mixed / zero; the region plane with every family of the route at the base count and the families that
    claim fallbacks (jump, limit-K, far-K) at the others.  The wave-per-query kernel has no region: the plane at its base count."""
    base = BASE_C[route]
    out = [(shape, nlev, base, D.COORD_KINDS) for shape, nlev in D.SHAPES]
    out += [(shape, nlev, C, D.COORD_KINDS) for shape, nlev in AD.SWEEP_SHAPES for C in ROUTE_C[route] if C != base]
    out += [(PLANE[0], PLANE[1], C, PLANE_FAMILIES[route] if C == base else PLANE_FAMILIES[route][3:]) for C in ROUTE_C[route]
            if route != "wave" or C == base]
    return out


@functools.lru_cache(maxsize=2)
def maps(shape, nlev, C):
    f1, f2 = AD.fmap_values(*shape, nlev, C)
    return f1, f2, AD.volumes(f1, f2), AD.volumes(f1, f2, absolute=True)


def case(shape, nlev, C, radius, family, add_grid):
    """dict(f1, f2, given, pos, ref, S): the float64 lookup of the formed volume and its scale, [B,H,W,CH]."""
    f1, f2, vol, avol = maps(shape, nlev, C)
    given, pos = positions(shape, family, radius, add_grid)
    return dict(f1=f1, f2=f2, given=given, pos=pos, ref=K.lookup(vol, pos, radius)[0], S=K.lookup(avol, pos, radius)[0])


def worst_of_forward_twins(report=None):
    """{'fwd': worst of the in-order and the pairwise fp32 twin over the wave and tile groups, 'mfma': of the bf16x3 twin over the
    matrix-pipe groups}, in units of UNIT[key] S."""
    worst = dict(fwd=0.0, mfma=0.0)
    done = set()
    for route in ROUTES:
        key = limit_key(route)
        for shape, nlev, C, families in groups(route):
            if (key, shape, nlev, C, families) in done:
                continue
            done.add((key, shape, nlev, C, families))
            f1, f2 = maps(shape, nlev, C)[:2]
            twins = [(o, dots32(f1, f2, o)) for o in (("bf16x3",) if key == "mfma" else ("seq", "pair"))]
            for radius in RADII:
                for family in families:
                    for add_grid in (False, True):
                        c = case(shape, nlev, C, radius, family, add_grid)
                        for o, v in twins:
                            w, _ = D.need(blend32(v, c["pos"], radius, C), c["ref"], c["S"] * UNIT[key])
                            if report is not None and w > worst[key]:
                                report(f"{key} {w:.4f} {o} {shape} L{nlev} C{C} r{radius} {family} grid{int(add_grid)}")
                            worst[key] = max(worst[key], w)
    return worst


# ---- the drop-in entries
DROPIN_C = 36
DROPIN_SHAPES = [(1, 10, 14), (2, 16, 24), (1, 8, 8), (3, 5, 9), (2, 8, 16)]
DROPIN_SWEEP = [(1, 10, 14), (3, 5, 9)]
GRAD_KINDS = ("gauss", "zero", "hotf", "hotl")


def dropin_cases():
    """[(shape, C, N, half, family, grad kinds)]: N = 1 and 3 coordinate sets; fmap2 of the same size, and of half the size with the
    coordinates halved.  Every plane of _dcoordsref.SHAPES at C = 36 with all four combinations on `mixed`, and a plane of zeros;
    the wave-per-query channel sweep on 1x10x14 and 3x5x9 with one set on the same size and three sets on half the size."""
    out = []
    for s in DROPIN_SHAPES:
        out += [(s, DROPIN_C, N, half, "mixed", GRAD_KINDS) for N in (1, 3) for half in (False, True)]
        out.append((s, DROPIN_C, 1, False, "zero", GRAD_KINDS))
    for s in DROPIN_SWEEP:
        for C in ROUTE_C["wave"]:
            if C != DROPIN_C:
                out += [(s, C, 1, False, "mixed", GRAD_KINDS[:2]), (s, C, 3, True, "mixed", GRAD_KINDS[:2])]
    return out


@functools.lru_cache(maxsize=4)
def dropin_case(shape, C, N, half, family):
    """dict(f1 [B,H1,W1,C], f2 [B,H2,W2,C], coords [B,N,H1,W1,2]): set n of `mixed` has its own positions, the +-1e6 row included."""
    B, H, W = shape
    H2, W2 = (H // 2, W // 2) if half else (H, W)
    f1 = torch.randn(B, H, W, C, generator=D._gen("d1", B, H, W, C, half), dtype=torch.float32)
    f2 = torch.randn(B, H2, W2, C, generator=D._gen("d2", B, H, W, C, half), dtype=torch.float32)
    sets = []
    for n in range(N):
        if family == "zero":
            c = torch.zeros(B, 2, H, W)
        else:
            x, y = D.mixed_positions(B * H * W, H, W, D._gen("dcoords", B, H, W, n))
            c = torch.stack([x.view(B, H, W), y.view(B, H, W)], 1)
            far = torch.tensor([1e6, -1e6]).repeat((W + 1) // 2)[:W]
            c[:, 0, 0, :], c[:, 1, 0, :] = far, -far
        sets.append((c * 0.5 if half else c).permute(0, 2, 3, 1))
    return dict(f1=f1, f2=f2, coords=torch.stack(sets, 1).contiguous())


def grad_values(shape, N, radius, kind):
    """corr_grad [B,N,(2r+1)^2,H1,W1]: gaussian, zero, a one on the first / the last channel of every set."""
    B, H, W = shape
    n2 = (2 * radius + 1) ** 2
    if kind == "gauss":
        return torch.randn(B, N, n2, H, W, generator=D._gen("dgrad", B, H, W, N, radius), dtype=torch.float32)
    g = torch.zeros(B, N, n2, H, W)
    if kind.startswith("hot"):
        g[:, :, 0 if kind == "hotf" else n2 - 1] = 1.0
    return g


def worst_of_backward_twins(report=None):
    """The worst either fp32 twin of the backward reaches against float64 over the drop-in cases, in units of 2^-24 S1 / S2."""
    worst = 0.0
    for shape, C, N, half, family, kinds in dropin_cases():
        c = dropin_case(shape, C, N, half, family)
        for radius in RADII:
            for gk in kinds:
                if gk == "zero":
                    continue                                            # (every term is an exact zero in any order)
                g = grad_values(shape, N, radius, gk)
                g1, g2, S1, S2 = dropin_bwd(c["f1"], c["f2"], c["coords"], g, radius)
                for order in ("seq", "pair"):
                    t1, t2 = dropin_bwd_explicit(c["f1"], c["f2"], c["coords"], g, radius, torch.float32, order)
                    w = max(D.need(t1, g1, S1 * U24)[0], D.need(t2, g2, S2 * U24)[0])
                    if report is not None and w > worst:
                        report(f"bwd {w:.4f} {order} {shape} C{C} N{N} half{int(half)} {family} r{radius} {gk}")
                    worst = max(worst, w)
    return worst
