"""Float64 restatements of the all-pairs correlation volume, of its two pyramids (floor halving; TensorFlow 'SAME') and of the
radius-r pyramid lookup; the tiled-row layout of csrc/corr_layout.hpp restated; fp32 twins of each; the error scale of every
output; and the cases the GPU tests of csrc/corr_build.hip, corr_tiled.hip (forward lookup) and corr_lookup.hip (forward
kernels) run (tests/test_corr_kernels.py).  Checked on the CPU by tests/test_corrref.py.  No GPU here.

The contract.
    V0[b, i, j] = sum_c f1[b, c, i] f2[b, c, j] / sqrt(C)                      i, j pixels of the H x W plane
    V(l+1)      = 2x2 mean of V(l) over the plane of j, sizes floor(h / 2), floor(w / 2)             (pool_floor)
    'SAME'      : level l = mean of level 0 over k x k windows, k = 2^l, size ceil(h / k), the padding ceil(h / k) k - h split
                  floor / ceil between the leading and the trailing side, the mean over the in-range cells only   (pool_same)
    lookup      : out[q, l (2r+1)^2 + i (2r+1) + j] = bilinear(V_l[q], pos_q 2^-l + (i - r, j - r)), zero outside the level, i the
                  x offset (slow); where the kernel is handed a flow the position is the fp32 sum flow + grid.  A level at which
                  |pos 2^-l| >= 30000 gives exactly 0 (the kernels clamp such positions to an all-zero window).
    tiled row   : cell (y, x) of level l at off[l] + ((y >> 2) tw[l] + (x >> 2)) 16 + (y & 3) 4 + (x & 3), th / tw = ceil(h / 4),
                  ceil(w / 4), levels back to back, P rounded up to 32 floats.

Error scales (elementwise), u = 2^-24:  build level 0: S0 = sum_c |f1| |f2| / sqrt(C); level l: pool_floor of S0; the pool kernels:
the pool of |level 0|; the lookup: sum of the four bilinear weights times |tap|.  The fp32-MFMA ("exact") build and everything
else is counted in units of u S, the bf16x3 builds (split, records) in units of 2^-16 S (_convref.GAMMA_PROD["bf16x3"]).

LIMITS[key] = limit_from_twin(TWIN_WORST[key]): 4 x the worst the fp32 twins reach against float64 over exactly the cases the GPU
tests run, rounded up to one digit (tests/test_corrref.py::test_limits_come_from_the_twins recomputes and prints them; the
kernels' own figures are in profiles/corr_kernel_margins.txt and set nothing).  The twins:
    build.exact   level 0 as an fp32 chain over c in order, and in 16-channel k-tiles; levels >= 1 by the kernels' own pool
                  expression (((a + b) + c) + d) * 0.25f, level by level
    build.split   hi = bf16(x), lo = bf16(x - hi); hi hi + hi lo + lo hi with fp32 accumulation; pooled as above
    pool          the pool expression level by level, against the float64 pyramid of the fp32 level 0
    pool_same     the window added cell by cell in fp32, divided by the fp32 count
    lookup.lerp / lookup.weights   the two blends found in the code, one entry each: two lerps (top + fy (bot - top): the tiled and
                  the channels-last kernels), and four weights (corr_lookup_fwd_kernel)
Twins' worst, in the units above, and the case each occurred in:
    build.exact     5.685  limit 30    1x15x17, C 34, gaussian, level 0 (the in-order chain; 34 channels)
    build.split     1.699  limit 7     1x16x16, C 96, one channel, level 0 (one product: 2^-16 S is the bound of a typical product,
                                       not of the worst one -- two lo roundings of 2^-17 and the dropped lo lo of 2^-16)
    pool            2.607  limit 20    4097x128x128, level 1
    pool_same       1.259  limit 6     3x9x11, level 1
    lookup.lerp     438.5  limit 2000  2x8x16, 4 levels, radius 3, mixed, gaussian: a lerp rounds v01 - v00 to u |v01 - v00| whatever
                                       the weights are, so against a scale that weighs every tap it costs up to 1 / weight units
                                       (coordinates are multiples of 1/64: weights down to 2^-12; the worst element is
                                       (1 - fy) v with 1 - fy = 2^-9 at level 3).  The twin rounds every operation; a compiler
                                       that contracts a lerp into one fma does better
    lookup.weights  2.827  limit 20    2x16x24, radius 3, mixed, 'SAME' pyramid
"""
import functools
import math

import torch

import _dcoordsref as D
from _convref import GAMMA_PROD, bf16_hi_lo
from _dcoordsref import FAR, U24, limit_from_twin, need  # noqa: F401  (re-exported: the tests use R.need, R.limit_from_twin)

G16 = GAMMA_PROD["bf16x3"]
UNIT = {"build.exact": U24, "build.split": G16, "pool": U24, "pool_same": U24, "lookup.lerp": U24, "lookup.weights": U24}

TWIN_WORST = {"build.exact": 5.69, "build.split": 1.70, "pool": 2.61, "pool_same": 1.26, "lookup.lerp": 439.0, "lookup.weights": 2.83}
LIMITS = {k: limit_from_twin(v) for k, v in TWIN_WORST.items()}      # 30, 7, 20, 6, 2000, 20


# ------------------------------------------------------------------------------------------------------------------ layout
def vol_layout(H, W, nlev):
    """vol_layout_make of csrc/corr_layout.hpp: dict(nlev, H, W, P, h, w, th, tw, off) with four entries per list, or None where
    the C function refuses."""
    if nlev < 1 or nlev > 4 or H < 1 or W < 1:
        return None
    L = dict(nlev=nlev, H=H, W=W, h=[], w=[], th=[], tw=[], off=[])
    h, w, o = H, W, 0
    for l in range(4):
        on = l < nlev
        if on and (h < 1 or w < 1):
            return None
        L["h"].append(h if on else 0)
        L["w"].append(w if on else 0)
        L["th"].append((h + 3) // 4 if on else 0)
        L["tw"].append((w + 3) // 4 if on else 0)
        L["off"].append(o)
        o += L["th"][l] * L["tw"][l] * 16
        h //= 2
        w //= 2
    L["P"] = (o + 31) // 32 * 32
    return L


def layout_from_ints(v):
    """The 24 ints fsraft_vol_layout writes -> the same dict."""
    v = [int(x) for x in v]
    return dict(nlev=v[0], H=v[1], W=v[2], P=v[3], h=v[4:8], w=v[8:12], th=v[12:16], tw=v[16:20], off=v[20:24])


def cell_index(L, l, y, x):
    return L["off"][l] + ((y >> 2) * L["tw"][l] + (x >> 2)) * 16 + (y & 3) * 4 + (x & 3)


def to_tiled(levels, L, pad_bits=0):
    """levels[l] [Q, h_l, w_l] (any sizes that fit the layout's tiles) -> the tiled rows [Q, P] fp32; every pad cell and the tail up
    to P hold the bit pattern `pad_bits`."""
    Q = levels[0].shape[0]
    vol = torch.full((Q, L["P"]), pad_bits, dtype=torch.int32).view(torch.float32)
    for l, lv in enumerate(levels):
        h, w = lv.shape[1:]
        th, tw = L["th"][l], L["tw"][l]
        full = torch.full((Q, th * 4, tw * 4), pad_bits, dtype=torch.int32).view(torch.float32)
        full[:, :h, :w] = lv.float()
        t = full.reshape(Q, th, 4, tw, 4).permute(0, 1, 3, 2, 4).reshape(Q, -1)
        vol[:, L["off"][l]:L["off"][l] + t.shape[1]] = t
    return vol


def from_tiled(vol, L, pads=False):
    """The tiled rows [Q, P] -> levels[l] [Q, h_l, w_l]; pads=True: the whole tiles, [Q, 4 th_l, 4 tw_l]."""
    Q = vol.shape[0]
    out = []
    for l in range(L["nlev"]):
        th, tw = L["th"][l], L["tw"][l]
        t = vol[:, L["off"][l]:L["off"][l] + th * tw * 16].reshape(Q, th, tw, 4, 4).permute(0, 1, 3, 2, 4).reshape(Q, th * 4, tw * 4)
        out.append(t if pads else t[:, :L["h"][l], :L["w"][l]])
    return out


def cell_mask(L):
    """bool [P]: the floats of a row that are cells of the pyramid (not pad, not tail)."""
    ones = [torch.ones(1, L["h"][l], L["w"][l]) for l in range(L["nlev"])]
    return to_tiled(ones, L)[0] == 1


# ------------------------------------------------------------------------------------------------------------------ the mathematics
def _pool2(a, pitch_bug=False):
    """2x2 mean with floor sizes in the dtype of `a`, in the kernels' order (((a + b) + c) + d) * 0.25.  pitch_bug: the second row
    taken 2 floor(w / 2) floats after the first instead of w (the same thing for an even w)."""
    R, h, w = a.shape
    h2, w2 = h // 2, w // 2
    if pitch_bug:
        flat = a.reshape(R, h * w)
        y, x = torch.arange(h2).view(-1, 1), torch.arange(w2).view(1, -1)
        i = ((2 * y) * w + 2 * x).reshape(-1)
        p = 2 * w2
        return ((((flat[:, i] + flat[:, i + 1]) + flat[:, i + p]) + flat[:, i + p + 1]) * 0.25).reshape(R, h2, w2)
    a = a[:, :2 * h2, :2 * w2]
    return (((a[:, 0::2, 0::2] + a[:, 0::2, 1::2]) + a[:, 1::2, 0::2]) + a[:, 1::2, 1::2]) * 0.25


def pool_floor(level0, nlev, dtype=torch.float64, pitch_bug=False):
    """[R, h, w] -> nlev levels, each the 2x2 mean of the one before (floor sizes)."""
    levels = [level0.to(dtype)]
    for _ in range(1, nlev):
        levels.append(_pool2(levels[-1], pitch_bug))
    return levels


def pool_same(level0, nlev, dtype=torch.float64):
    """[R, h, w] -> nlev levels with TensorFlow 'SAME' semantics, every level pooled from level 0; the window is added cell by cell
    in row-major order in `dtype` and divided by the count (corr_pool_same_kernel's order)."""
    a = level0.to(dtype)
    R, h, w = a.shape
    levels = [a]
    for l in range(1, nlev):
        k = 1 << l
        h2, w2 = (h + k - 1) // k, (w + k - 1) // k
        py, px = (h2 * k - h) // 2, (w2 * k - w) // 2
        ys, xs = torch.arange(h2) * k - py, torch.arange(w2) * k - px
        acc, cnt = torch.zeros(R, h2, w2, dtype=dtype), torch.zeros(h2, w2, dtype=dtype)
        for dy in range(k):
            for dx in range(k):
                yy, xx = ys + dy, xs + dx
                ok = ((yy >= 0) & (yy < h)).view(-1, 1) & ((xx >= 0) & (xx < w)).view(1, -1)
                v = a[:, yy.clamp(0, h - 1)][:, :, xx.clamp(0, w - 1)]
                acc = torch.where(ok, acc + v, acc)
                cnt = cnt + ok.to(dtype)
        levels.append(acc / cnt)
    return levels


def pool_ceil_mutant(level0, nlev):
    """WRONG on purpose: ceil level sizes, the partial windows averaged over what is there."""
    levels = [level0.double()]
    for _ in range(1, nlev):
        a = levels[-1]
        R, h, w = a.shape
        p = torch.zeros(R, h + (h & 1), w + (w & 1), dtype=a.dtype)
        c = torch.zeros(1, h + (h & 1), w + (w & 1), dtype=a.dtype)
        p[:, :h, :w], c[:, :h, :w] = a, 1
        s = p[:, 0::2, 0::2] + p[:, 0::2, 1::2] + p[:, 1::2, 0::2] + p[:, 1::2, 1::2]
        n = c[:, 0::2, 0::2] + c[:, 0::2, 1::2] + c[:, 1::2, 0::2] + c[:, 1::2, 1::2]
        levels.append(s / n)
    return levels


def volume0(f1, f2, scale=True):
    """V0 [B*N, H, W] in float64 from fp32 maps [B, C, H, W]."""
    B, C, H, W = f1.shape
    v = torch.einsum("bci,bcj->bij", f1.reshape(B, C, -1).double(), f2.reshape(B, C, -1).double())
    return (v / math.sqrt(C) if scale else v).reshape(B * H * W, H, W)


def build(f1, f2, nlev, scale=True):
    return pool_floor(volume0(f1, f2, scale), nlev)


def build_scale(f1, f2, nlev):
    """The error scale of every level: the floor pyramid of S0 = sum_c |f1| |f2| / sqrt(C)."""
    return pool_floor(volume0(f1.abs(), f2.abs()), nlev)


def build0_twin(f1, f2, arith, order="seq"):
    """Level 0 in fp32.  arith 'fp32': order 'seq' (over c in order) or 'ktile' (16 channels at a time, the partial sums added);
    'bf16x3': hi hi + hi lo + lo hi in one fp32 chain (the products of two bf16 numbers are exact in fp32); 'bf16x1': hi hi only.
    The scale is the fp32 1 / sqrt(C) the entry points pass."""
    B, C, H, W = f1.shape
    N = H * W
    a, b = f1.reshape(B, C, N, 1).float(), f2.reshape(B, C, 1, N).float()
    acc = torch.zeros(B, N, N)
    if arith == "fp32" and order == "seq":
        for c in range(C):
            acc = acc + a[:, c] * b[:, c]
    elif arith == "fp32":
        for k0 in range(0, C, 16):
            part = torch.zeros(B, N, N)
            for c in range(k0, min(k0 + 16, C)):
                part = part + a[:, c] * b[:, c]
            acc = acc + part
    else:
        (ah, al), (bh, bl) = bf16_hi_lo(a), bf16_hi_lo(b)
        for c in range(C):
            acc = acc + ah[:, c] * bh[:, c]
            if arith == "bf16x3":
                acc = acc + ah[:, c] * bl[:, c]
                acc = acc + al[:, c] * bh[:, c]
    s = 1.0 / torch.tensor(float(C), dtype=torch.float32).sqrt()
    return (acc * s).reshape(B * N, H, W)


def lookup(levels, pos, radius, dtype=torch.float64, form="weights", level_scale=True, swap=False):
    """(out [B, H, W, CH], S [B, H, W, CH]) in `dtype`, every operation rounded to it.  levels[l] [Q, h_l, w_l] (any sizes); pos
    [B, 2, H, W] fp32 positions.  form: 'weights' (corr_lookup_fwd_kernel: four weights) or 'lerp' (the channels-last and the tiled
    kernels: two lerps).  level_scale=False and swap=True are the mutants."""
    B, _, H, W = pos.shape
    r, n = radius, 2 * radius + 1
    xy = pos.permute(0, 2, 3, 1).reshape(B * H * W, 2).to(dtype)
    off = torch.arange(-r, r + 1, dtype=dtype)
    ox = off.view(n, 1).expand(n, n).reshape(1, n * n)      # slow index: the x offset
    oy = off.view(1, n).expand(n, n).reshape(1, n * n)
    if swap:
        ox, oy = oy, ox
    val, S = [], []
    for l, lv in enumerate(levels):
        s = 1.0 / (1 << l) if level_scale else 1.0
        cx, cy = xy[:, 0:1] * s, xy[:, 1:2] * s
        near = (cx.abs() < FAR) & (cy.abs() < FAR)
        cx, cy = torch.where(near, cx, torch.zeros_like(cx)), torch.where(near, cy, torch.zeros_like(cy))
        flx, fly = torch.floor(cx), torch.floor(cy)
        fx, fy = cx - flx, cy - fly
        v00, v01, v10, v11 = D._taps(lv.to(dtype), flx.long() + ox.long(), fly.long() + oy.long())
        w00, w01, w10, w11 = (1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy
        if form == "lerp":
            top, bot = v00 + fx * (v01 - v00), v10 + fx * (v11 - v10)
            o = top + fy * (bot - top)
        else:
            o = ((v00 * w00 + v01 * w01) + v10 * w10) + v11 * w11
        z = near.expand_as(o)
        val.append(torch.where(z, o, torch.zeros_like(o)))
        sc = v00.abs() * w00 + v01.abs() * w01 + v10.abs() * w10 + v11.abs() * w11
        S.append(torch.where(z, sc, torch.zeros_like(sc)))
    return torch.cat(val, 1).view(B, H, W, -1), torch.cat(S, 1).view(B, H, W, -1)


# ------------------------------------------------------------------------------------------------------------------ build cases
# B x H x W, levels (the constants of csrc/corr_build.hip: target patches 8x32 and 8x16 (records), 64 / 256 queries per workgroup,
# the record kernel's halves of 128, 4x4 tiles): the smallest legal call; level 1 is 1x2; last level 1x1; one over the 8-row and the
# 16-column patch; no level a multiple of a tile (10x14, 5x7, 2x3, 1x1); one over the 32-column patch; 255 / 256 / 257 queries; B > 1.
BUILD_SHAPES = [((1, 1, 1), 1), ((1, 3, 5), 2), ((1, 8, 8), 4), ((1, 9, 17), 4), ((1, 10, 14), 4), ((1, 8, 33), 4),
                ((1, 15, 17), 4), ((1, 16, 16), 4), ((1, 1, 257), 1), ((2, 13, 22), 4)]
C_FP32 = (2, 14, 16, 18, 34)        # a partial 16- / 32-channel k-tile, an exact one, one over
C_REC = (32, 64, 96, 256)           # 96: an odd trip count of the three-slot ring
VALUE_KINDS = ("gauss", "scaled", "onechan", "zero")
CHAIN = ((2, 13, 22), 4, 64)


def build_cases(rec):
    """(shape, nlev, C, value kind): gaussian maps at every C; the other kinds at one C each."""
    cs = C_REC if rec else C_FP32
    for shape, nlev in BUILD_SHAPES:
        for C in cs:
            yield shape, nlev, C, "gauss"
        for C, kind in zip((cs[1], cs[2], cs[0]), VALUE_KINDS[1:]):
            yield shape, nlev, C, kind


def fmaps(shape, C, kind):
    """(f1, f2) [B, C, H, W] fp32.  scaled: sample 0 has f1 * 2^10 and f2 * 2^-10 (the hi / lo split must not care); onechan: one
    channel is the only non-zero one; zero: f2 is zero (the volume is exactly 0)."""
    B, H, W = shape
    f1 = torch.randn(B, C, H, W, generator=D._gen("f1", B, H, W, C, kind))
    f2 = torch.randn(B, C, H, W, generator=D._gen("f2", B, H, W, C, kind))
    if kind == "scaled":
        f1[0] *= 2.0 ** 10
        f2[0] *= 2.0 ** -10
    elif kind == "onechan":
        keep = torch.zeros(C).index_fill_(0, torch.tensor([C // 2]), 1.0).view(1, C, 1, 1)
        f1, f2 = f1 * keep, f2 * keep
    elif kind == "zero":
        f2 = torch.zeros_like(f2)
    return f1, f2


@functools.lru_cache(maxsize=None)
def build_case(shape, nlev, C, kind):
    f1, f2 = fmaps(shape, C, kind)
    return dict(f1=f1, f2=f2, ref=build(f1, f2, nlev), S=build_scale(f1, f2, nlev))


# ------------------------------------------------------------------------------------------------------------------ pool cases
# rows x h x w, levels.  floor: one row down to 1x1 in 8 levels; 3 rows of 9x11; 4097 rows of 128x128 -- level 1 has 65552
# workgroups of 256 cells, 16 over the cap of the grid-stride loop: the smallest round size that takes a second trip.
POOL_CASES = [((1, 130, 129), 8), ((3, 9, 11), 4), ((4097, 128, 128), 2)]
POOL_SAME_CASES = [((3, 9, 11), 4), ((2, 8, 8), 4), ((2, 1, 1), 3)]


def pool_input(shape):
    return torch.randn(*shape, generator=D._gen("pool", *shape))


# ------------------------------------------------------------------------------------------------------------------ lookup cases
# the tiled lookup: _dcoordsref.SHAPES and the two below; the row-major entries take exactly four levels and H, W >= 8:
# 1x8x10 = 80 queries (a multiple of 8 and 16, not of 32), 1x9x9 = 81.
EXTRA_SHAPES = [((1, 8, 10), 4), ((1, 9, 9), 4)]
TILED_SHAPES = D.SHAPES + EXTRA_SHAPES
ROW_SHAPES = [(s, n) for s, n in TILED_SHAPES if n == 4 and s[1] >= 8 and s[2] >= 8]
RADII = D.RADII
COORD_KINDS = D.COORD_KINDS
VOL_KINDS = ("gauss", "onehot")
LAYOUTS = ("planar", "planar_gap", "interleaved")


def level_values(shape, nlev, kind, same=False):
    """[Q, h_l, w_l] fp32 per level, NOT made by a build kernel.  gauss: independent gaussian levels (_dcoordsref.level_values);
    onehot: the same with level nlev // 2 zero but for a 1 in exactly one cell, another cell for every query.  same: a 'SAME'
    pyramid (ceil sizes) pooled from a gaussian level 0."""
    B, H, W = shape
    if same:
        lv0 = torch.randn(B * H * W, H, W, generator=D._gen("same", B, H, W))
        return [lv.float() for lv in pool_same(lv0, nlev)]
    levels = [lv.clone() for lv in D.level_values(B, H, W, nlev)]
    if kind == "onehot":
        l = nlev // 2
        Q, h, w = levels[l].shape
        q = torch.arange(Q)
        levels[l].zero_()
        levels[l][q, q % h, (q * 7 + 3) % w] = 1.0
    return levels


def strides(B, H, W, layout):
    """(floats in the buffer, bs, cs, ps) of a 2-channel tensor: element (b, c, pix) at b bs + c cs + pix ps."""
    HW = H * W
    if layout == "planar":
        return B * 2 * HW, 2 * HW, HW, 1
    if layout == "interleaved":
        return B * 2 * HW, 2 * HW, 1, 2
    return B * (2 * HW + 8), 2 * HW + 8, HW, 1


def pack2(t, layout, fill_bits):
    """[B, 2, H, W] -> the flat tensor in `layout`; floats that are no element hold `fill_bits`."""
    B, _, H, W = t.shape
    n, bs, cs, ps = strides(B, H, W, layout)
    flat = torch.full((n,), fill_bits, dtype=torch.int32).view(torch.float32).clone()
    idx = torch.arange(B).view(B, 1, 1) * bs + torch.arange(2).view(1, 2, 1) * cs + torch.arange(H * W).view(1, 1, -1) * ps
    flat[idx.reshape(-1)] = t.reshape(-1).float()
    return flat


@functools.lru_cache(maxsize=None)
def lookup_case(shape, nlev, radius, ckind, add_grid, vkind):
    """levels, what the kernel is handed as coords (`given`: the flow when add_grid), the positions (the fp32 sum), the float64
    output and its scale.  vkind 'same': the ceil-sized pyramid."""
    B, H, W = shape
    levels = level_values(shape, nlev, vkind, same=vkind == "same")
    given = D.coords_values(B, H, W, ckind)
    pos = given + D.grid(B, H, W) if add_grid else given
    ref, S = lookup(levels, pos, radius)
    return dict(levels=levels, given=given, pos=pos, ref=ref, S=S)


def lookup_cases():
    """Every (shape, nlev, radius, coordinate kind, add_grid, volume kind) the lookup kernels are compared on."""
    for shape, nlev in TILED_SHAPES:
        for radius in RADII:
            for ckind in COORD_KINDS:
                for add_grid in (False, True):
                    for vkind in VOL_KINDS:
                        yield shape, nlev, radius, ckind, add_grid, vkind
    for shape, nlev in ROW_SHAPES:
        for radius in RADII:
            for ckind in COORD_KINDS:
                yield shape, nlev, radius, ckind, False, "same"


# ------------------------------------------------------------------------------------------------------------------ the twins' worst
def twins_worst():
    """{key: (worst figure in the key's unit, the case)} of every twin against float64 over the cases above."""
    worst = {k: (0.0, "") for k in LIMITS}

    def see(key, got, ref, scale, case):
        w, _ = need(got, ref, scale * UNIT[key])
        if w > worst[key][0]:
            worst[key] = (w, case)

    for rec in (False, True):
        for shape, nlev, C, kind in build_cases(rec):
            c = build_case(shape, nlev, C, kind)
            twins = [("build.split", build0_twin(c["f1"], c["f2"], "bf16x3"))]
            if not rec:
                twins += [("build.exact", build0_twin(c["f1"], c["f2"], "fp32", o)) for o in ("seq", "ktile")]
            for key, t0 in twins:
                for l, lv in enumerate(pool_floor(t0, nlev, torch.float32)):
                    see(key, lv, c["ref"][l], c["S"][l], f"{shape} C {C} {kind} level {l}")
    for shape, nlev in POOL_CASES:
        x = pool_input(shape)
        ref, S, tw = pool_floor(x, nlev), pool_floor(x.abs(), nlev), pool_floor(x, nlev, torch.float32)
        for l in range(1, nlev):
            see("pool", tw[l], ref[l], S[l], f"{shape} level {l}")
    for shape, nlev in POOL_SAME_CASES:
        x = pool_input(shape)
        ref, S, tw = pool_same(x, nlev), pool_same(x.abs(), nlev), pool_same(x, nlev, torch.float32)
        for l in range(1, nlev):
            see("pool_same", tw[l], ref[l], S[l], f"{shape} level {l}")
    for case in lookup_cases():
        shape, nlev, radius = case[:3]
        c = lookup_case(*case)
        for form in ("lerp", "weights"):
            got, _ = lookup(c["levels"], c["pos"], radius, torch.float32, form)
            see("lookup." + form, got, c["ref"], c["S"], f"{case}")
    return worst
