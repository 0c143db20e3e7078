"""Float64 restatements of the backward of the TensorFlow 'SAME' pyramid -- the un-pooling of the level gradients into level 0
(csrc/corr_build.hip: corr_unpool_same_bwd_kernel / _vec_kernel) and the lookup backward and coordinate gradient on ceil-sized levels
(the kernels of csrc/corr_lookup.hip and csrc/corr_dcoords.hip through their _same entries) --, fp32 twins in the kernels' order of
operations, the error scale of every output, and the cases tests/test_same_bwd_kernels.py and tests/test_same_autograd.py run.
Checked on the CPU by tests/test_samebwdref.py.  No GPU here.  The forward ('SAME' pooling, lookup) is tests/_corrref.py; the scatter's
window arithmetic is tests/_corrbwdref.py's, the Jacobian tests/_dcoordsref.py's (both read the level sizes off the levels).

The contract.  Level l >= 1 of a 'SAME' pyramid of an h x w level 0: k = 2^l, h_l = ceil(h / k), w_l = ceil(w / k), leading padding
py = (h_l k - h) // 2, px = (w_l k - w) // 2; window (Y, X) covers the cells y in [Y k - py, Y k - py + k) and x likewise that lie in
the level, count(Y, X) of them, and holds their mean (_corrref.pool_same).  Its transpose:
    unpool_same_bwd : g0[y][x] += sum_{l >= 1} g_l[(y + py) >> l][(x + px) >> l] / count of that window
    scale S         : the same sum with |g|
    twin (fp32)     : acc = 0; for l = 1, 2, ...: acc = acc + g_l[Y][X] * (1.0f / (float)count); out = g0 + acc  -- the level sum in
                      ascending order, the weight as the rounded reciprocal of the count, every operation rounded (the kernels')
    scatter_same    : _corrbwdref.scatter with levels of the ceil sizes
    dcoords         : _dcoordsref.expect / twin on levels of the ceil sizes

Units: u = 2^-24 times S.  LIMITS[key] = limit_from_twin(TWIN_WORST[key]) over exactly the cases of the GPU tests (twins_worst();
tests/test_samebwdref.py::test_limits_come_from_the_twins recomputes and prints them).  Twins' worst and where:
    unpool_same         3.052  limit 20    19100x22x20, 4 levels (the vector kernel's second trip)
    lookup_bwd_same.cl  3.100  limit 20    2x6x12, radius 4, level 1   (above _corrbwdref's 2.73 for lookup_bwd.cl: a key of its own)
    dcoords_same        1.873  limit 8     2x6x12, 2 levels, radius 3, pairwise   (above _dcoordsref's 1.81: a key of its own)
    lookup_bwd.four     2.370  under _corrbwdref's 2.75 (2x6x12, radius 3, level 1): that key and its limit of 20 apply
"""
import functools

import torch

import _corrbwdref as B
import _corrref as R
import _dcoordsref as D
from _dcoordsref import U24, limit_from_twin, need  # noqa: F401

TWIN_WORST = {"unpool_same": 3.06, "lookup_bwd_same.cl": 3.10, "dcoords_same": 1.88}
LIMITS = {k: limit_from_twin(v) for k, v in TWIN_WORST.items()}      # 20, 20, 8
# a key of the floor-sized cases that applies here: its twin on the ceil sizes stays under the worst recorded there
SHARED = {"lookup_bwd.four": (B.TWIN_WORST["lookup_bwd.four"], B.LIMITS["lookup_bwd.four"])}
LIMITS.update({k: lim for k, (_, lim) in SHARED.items()})


def same_sizes(h, w, nlev):
    return [(-(-h // (1 << l)), -(-w // (1 << l))) for l in range(nlev)]


# ------------------------------------------------------------------------------------------------------------------ unpool_same_bwd
def _windows(size, l):
    """(window index, in-range count of that window) of every cell 0 .. size - 1 along one axis at level l."""
    k = 1 << l
    n = -(-size // k)
    pad = (n * k - size) // 2
    i = (torch.arange(size) + pad) >> l
    lo = i * k - pad
    return i, (lo + k).clamp(max=size) - lo.clamp(min=0)


def unpool_same_bwd(levels, dtype=torch.float64, absolute=False):
    """levels[l] [Q, h_l, w_l] (ceil sizes) -> the new level 0 in `dtype`, every operation rounded to it, in the kernels' order (the
    docstring's twin; in float64 the restatement).  absolute: the scale S."""
    lv = [(t.abs() if absolute else t).to(dtype) for t in levels]
    Q, H, W = lv[0].shape
    acc = torch.zeros_like(lv[0])
    for l in range(1, len(lv)):
        assert tuple(lv[l].shape[1:]) == same_sizes(H, W, l + 1)[l], (lv[l].shape, H, W, l)
        (Y, cy), (X, cx) = _windows(H, l), _windows(W, l)
        wgt = torch.ones((), dtype=dtype) / (cy.view(H, 1) * cx.view(1, W)).to(dtype)
        acc = acc + lv[l][:, Y.view(H, 1), X.view(1, W)] * wgt
    return lv[0] + acc


# rows x h x w, levels, floats level 0 is moved off its alignment by.  _corrref.POOL_SAME_CASES (3x9x11 scalar, 2x8x8 vector and equal
# to the floor pyramid, 2x1x1: one cell in every window up to k = 4); 5x6x12 (py = 1 at k = 4 and k = 8, px = 2 at k = 8, where x =
# 4 .. 7 lies in two windows; vector), and the same 4 bytes off (scalar); 1, 2, 3, 4 and 8 levels at 2x9x11; the second trips of the
# two grid-stride loops past 8192 blocks of 256: 21200x9x11 (2 098 800 cells, scalar) and 19100x22x20 (2 101 000 float4, vector).
UNPOOL_CASES = [(s, n, 0) for s, n in R.POOL_SAME_CASES] + [((5, 6, 12), 4, 0), ((5, 6, 12), 4, 1)] + \
    [((2, 9, 11), n, 0) for n in (1, 2, 3, 4, 8)]
UNPOOL_BIG = [((21200, 9, 11), 4, 0), ((19100, 22, 20), 4, 0)]
BLOCK_CAP = 8192 * 256


def unpool_values(shape, nlev):
    Q, H, W = shape
    return [torch.randn(Q, h, w, generator=D._gen("unpool_same", Q, H, W, nlev, l)) for l, (h, w) in enumerate(same_sizes(H, W, nlev))]


@functools.lru_cache(maxsize=None)
def unpool_case(shape, nlev):
    lv = unpool_values(shape, nlev)
    return dict(levels=lv, ref=unpool_same_bwd(lv), S=unpool_same_bwd(lv, absolute=True))


# ------------------------------------------------------------------------------------------------------------------ the scatter
def scatter_same(pos, dout, plane, nlev, radius, dtype=torch.float64, form="four", old=None, scale=True):
    """_corrbwdref.scatter onto levels of the 'SAME' sizes: (levels, S), levels[l] [Q, ceil(H / 2^l), ceil(W / 2^l)] in `dtype` = old[l]
    + the scatter of the lookups in order; S: sum |w| |G| + |old|.  pos: n x [Q, 2] fp32; dout: n x [Q, nlev N2] fp32."""
    H, W = plane
    Q = pos[0].shape[0]
    n1 = 2 * radius + 1
    n2 = n1 * n1
    levels, S = [], []
    for l, (h, w) in enumerate(same_sizes(H, W, nlev)):
        lv = (old[l].to(dtype).clone() if old is not None else torch.zeros(Q, h, w, dtype=dtype)).reshape(Q, h * w)
        sc = (old[l].double().abs() if old is not None else torch.zeros(Q, h, w, dtype=torch.float64)).reshape(Q, h * w).clone()
        for p, g in zip(pos, dout):
            G = g[:, l * n2:(l + 1) * n2].reshape(Q, n1, n1)
            wx0, wy0, fx, fy = B.level_query(p, l, radius, dtype)
            B._add_window(lv, h, w, wx0, wy0, B.window_grad(G.to(dtype), fx, fy, form))
            if scale:
                x0, y0, ax, ay = B.level_query(p, l, radius, torch.float64)
                B._add_window(sc, h, w, x0, y0, B.window_grad(G.double().abs(), ax, ay, "four"))
        levels.append(lv.view(Q, h, w))
        S.append(sc.view(Q, h, w))
    return levels, (S if scale else None)


# B x H x W: an odd plane (levels 9x11, 5x6, 3x3, 2x2), one whose width is a multiple of 4 (6x12, 3x6, 2x3, 1x2) and 3x5x9 (135
# queries, no multiple of 8, 16 or 32; 5x9, 3x5, 2x3, 1x2); four levels where the pyramid is written, 1 .. 4 where it is read.
LOOKUP_SHAPES = [(1, 9, 11), (2, 6, 12), (3, 5, 9)]
RADII = R.RADII


@functools.lru_cache(maxsize=None)
def lookup_bwd_case(shape, radius):
    """dlevels (ceil sizes) start gaussian; two lookups (_dcoordsref.mixed_positions, two draws; the first row far) one after the other."""
    Bn, H, W = shape
    old = [torch.randn(Bn * H * W, h, w, generator=D._gen("dlev_same", Bn, H, W, l)) for l, (h, w) in enumerate(same_sizes(H, W, 4))]
    pos = B.positions(shape, radius, "edge", 2)
    dout = B.douts(shape, 4, radius, "gauss", 2)
    fp, fd = [B._flat(p) for p in pos], [d.reshape(Bn * H * W, -1) for d in dout]
    ref, S = scatter_same(fp, fd, (H, W), 4, radius, old=old)
    return dict(old=old, given=pos, dout=dout, pos=fp, fdout=fd, ref=ref, S=S)


def level_values(shape, nlev):
    """Independent gaussian levels of the ceil sizes [B H W, h_l, w_l]."""
    Bn, H, W = shape
    return [torch.randn(Bn * H * W, h, w, generator=D._gen("vol_same", Bn, H, W, nlev, l)) for l, (h, w) in enumerate(same_sizes(H, W, nlev))]


@functools.lru_cache(maxsize=None)
def dcoords_case(shape, nlev, radius):
    """levels, positions (_dcoordsref.coords_values 'mixed'), gaussian dout [B, H, W, CH], the float64 gradient and its scale."""
    Bn, H, W = shape
    levels = level_values(shape, nlev)
    pos = D.coords_values(Bn, H, W, "mixed")
    dout = D.dout_values(Bn, H, W, nlev, radius, "gauss")
    _, dc, S = D.expect(levels, pos, dout, radius)
    return dict(levels=levels, pos=pos, dout=dout, ref=dc, S=S)


# ------------------------------------------------------------------------------------------------------------------ the chain
CHAIN = R.CHAIN                # 2x13x22, 4 levels (13x22, 7x11, 4x6, 2x3), C = 64
CHAIN_RADIUS = 4


@functools.lru_cache(maxsize=None)
def chain_case():
    """calc_all_field -> CorrBlock -> cotangent at CHAIN in float64: the feature maps, the positions, the cotangent, the 'SAME'
    pyramid, the level gradients (scatter_same), the gradient of level 0 (unpool_same_bwd) and of the two maps (volume_bwd of that one
    level), each with its scale."""
    shape, nlev, C = CHAIN
    Bn, H, W = shape
    bc = R.build_case(shape, nlev, C, "gauss")
    f1, f2 = bc["f1"], bc["f2"]
    pos = D.coords_values(Bn, H, W, "mixed")
    dout = torch.randn(Bn, H, W, nlev * (2 * CHAIN_RADIUS + 1) ** 2, generator=D._gen("chain_same", Bn, H, W))
    dlev, S = scatter_same([B._flat(pos)], [dout.reshape(Bn * H * W, -1)], (H, W), nlev, CHAIN_RADIUS)
    return dict(f1=f1, f2=f2, pos=pos, dout=dout, pyr=R.pool_same(R.volume0(f1, f2), nlev), dlev=dlev, S=S)


# ------------------------------------------------------------------------------------------------------------------ the twins' worst
def twins_worst(big=True):
    """{key: (worst figure in units of 2^-24 S, the case)} of every twin against float64 over the cases above."""
    worst = {k: (0.0, "") for k in LIMITS}

    def see(key, got, ref, scale, case):
        w, _ = need(got, ref, scale * U24)
        if w > worst[key][0]:
            worst[key] = (w, case)

    for shape, nlev, _ in UNPOOL_CASES + (UNPOOL_BIG if big else []):
        c = unpool_case(shape, nlev)
        see("unpool_same", unpool_same_bwd(c["levels"], torch.float32), c["ref"], c["S"], f"{shape} L{nlev}")
    for shape in LOOKUP_SHAPES:
        for radius in RADII:
            c = lookup_bwd_case(shape, radius)
            for form in ("four", "cl"):
                tw, _ = scatter_same(c["pos"], c["fdout"], shape[1:], 4, radius, torch.float32, form, old=c["old"], scale=False)
                for l in range(4):
                    see("lookup_bwd.four" if form == "four" else "lookup_bwd_same.cl", tw[l], c["ref"][l], c["S"][l], f"{shape} r{radius} level {l}")
            for nlev in (1, 2, 3, 4):
                d = dcoords_case(shape, nlev, radius)
                for order in ("sequential", "pairwise"):
                    see("dcoords_same", D.twin(d["levels"], d["pos"], d["dout"], radius, order), d["ref"], d["S"].expand_as(d["ref"]),
                        f"{shape} L{nlev} r{radius} {order}")
    return worst
