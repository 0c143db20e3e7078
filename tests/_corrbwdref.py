"""Float64 restatements of the backward half of the correlation path -- the gradient volume of a step's lookups (csrc/corr_tiled.hip:
corr_dvol_kernel, corr_dvol_sep_kernel), the query list handed between the two, f2cat / f2cat_rec / dfmap2, the un-pooling of the
level gradients (csrc/corr_build.hip) and the row-major lookup backward (csrc/corr_lookup.hip) --, an fp32 twin of every distinct
arithmetic form found in those kernels, the error scale of every output, the k-tile marks of fsraft_corr_bwd_ktiles as integer logic,
the float64 chain down to the feature maps' gradients (volume_bwd), and the cases tests/test_corr_bwd_kernels.py runs.
Checked on the CPU by tests/test_corrbwdref.py.  No GPU here.  Layout, forward lookup and pooling come from tests/_corrref.py.

The contract.  G_t[i][j] = dout_t[q, l N2 + i N1 + j] (N1 = 2r + 1, i the x offset, slow), (wx0, wy0) = floor(pos_t 2^-l) - r the
window origin of lookup t at level l, (fx, fy) the fractions; a coordinate with |pos 2^-l| >= 30000 is moved to -30000, whose
window lies outside every level.  Window cell (wy, wx), 0 <= wy, wx <= N1, of that lookup receives
    Wd[wy][wx] = sum over ay, ax in {0, 1} of (ay ? fy : 1 - fy) (ax ? fx : 1 - fx) G_t[wx - ax][wy - ay]      (absent entries 0)
    dV_l[q][wy0 + wy][wx0 + wx] (+)= Wd[wy][wx]   where the cell exists;     dvol row = the levels in the tiled layout, pads 0
    scale S = the same sum with |G| (plus |old| when accumulating); cells no window reaches have S = 0: they must be exactly 0
    query list  : q leaves corr_dvol_sep_kernel iff at some level max_t wx0 - min_t wx0 + WIN > side(l) (or the same in y),
                  WIN = 2r + 2, side = 24, 18, 14, 12
    f2cat       : [B][C][P]: level-l cell = 4^-l (sum of fmap2 over its 2^l x 2^l pixels); pads and tail 0
    dfmap2      : d2[b][y W + x][c] = sum_l 4^-l d2cat[b][cell_l(y >> l, x >> l)][c] over the levels where that cell exists
    unpool_bwd  : g0[y][x] += sum_{l >= 1} 4^-l g_l[y >> l][x >> l] where that cell exists (the transpose of pool_floor)
    lookup_bwd  : dlevels[l] (row-major) += the scatter above, one lookup per call

Forms (form=...): 'four'  acc = 0; acc += G (wy wx) for the four taps in turn                     contract; corr_lookup_bwd_kernel
                  'row'   wy1 (wx1 G + wx0 G) + wy0 (wx1 G + wx0 G), lookup by lookup             corr_dvol_kernel
                  'sep'   T = (1 - fx) G_i + fx G_{i-1};  acc += (1 - fy) T[wy];  acc += fy T[wy - 1]; lookups with one window
                          origin are summed in acc before they meet the level                     corr_dvol_sep_kernel
                  'cl'    s = G[.][wy] (1 - fy) + G[.][wy - 1] fy;  d = s[wx] (1 - fx) + s[wx - 1] fx   corr_lookup_bwd_cl_kernel
f2cat: 'block' (one sum over the block in row-major order, (a + b) + (c + d) at level 1; corr_f2cat_kernel) and 'rec' (level by
level 0.25 ((a + b) + (c + d)); corr_f2cat_rec_kernel).  unpool_bwd: 'chain' (up = g_l + 0.25 up from the top; g0 + 0.25 up).

Units: u = 2^-24 times S for everything fp32.  Records (hi = bf16(x), lo = bf16(x - hi)): |x - (hi + lo)| in units of 2^-17 |x|,
key 'split', measured on the twins' outputs with _convref.bf16_hi_lo; a record output is bounded by the fp32 limit plus one split,
plus one more split per accumulating launch, each of the value that launch wrote (record_bound).

LIMITS[key] = limit_from_twin(TWIN_WORST[key]) over exactly the cases of the GPU tests (twins_worst(); tests/test_corrbwdref.py::
test_limits_come_from_the_twins recomputes and prints them).  Twins' worst and where:
    dvol.row            3.653  limit 20    1x64x129, queries 1037 .. 1103, radius 4, local, 7 lookups, level 3
                                           (16 + 1 lookups after the wave-per-query twin, 2x16x24 radius 4 near: 3.596)
    dvol.sep            3.698  limit 20    2x16x24, radius 3, alt, 7 lookups, level 1
    split               0.998  limit 4     2x16x24, radius 3, limit  (units of 2^-17 |x|: hi is exact to 2^-9 |x|, lo to 2^-9 of that)
    f2cat.block         3.693  limit 20    2 x 256 x 64x129, level 2 (sixteen additions in order)
    f2cat.rec           1.889  limit 8     2 x 256 x 64x129, level 1
    dfmap2              2.929  limit 20    8 x 64x129, C 256
    unpool              2.738  limit 20    1x64x68, 4 levels
    lookup_bwd.four     2.746  limit 20    1x9x9, radius 3, level 0
    lookup_bwd.cl       2.722  limit 20    2x16x24, radius 3, level 3
k-tile marks (fsraft_corr_bwd_ktiles): integer logic only, ktile_marks / ktile_lists -- no limit, every comparison is exact.
"""
import functools

import torch

import _corrref as R
import _dcoordsref as D
from _convref import bf16_hi_lo
from _dcoordsref import FAR, U24, limit_from_twin, need  # noqa: F401

SPLIT_UNIT = 2.0 ** -17
DVS_SIDE = (24, 18, 14, 12)

TWIN_WORST = {"dvol.row": 3.66, "dvol.sep": 3.70, "split": 0.999, "f2cat.block": 3.70, "f2cat.rec": 1.89, "dfmap2": 2.93,
              "unpool": 2.74, "lookup_bwd.four": 2.75, "lookup_bwd.cl": 2.73}
LIMITS = {k: limit_from_twin(v) for k, v in TWIN_WORST.items()}


# ------------------------------------------------------------------------------------------------------------------ level_query
def level_query(pos, l, radius, dtype=torch.float32, level_scale=True):
    """level_query of csrc/corr_tiled_dev.hpp (query_setup of corr_lookup.hip is the same): pos [Q, 2] fp32 -> window origins
    wx0, wy0 (int64 [Q]) and fractions fx, fy ([Q], dtype).  2^-l is exact in either dtype."""
    c = pos.to(dtype) * ((1.0 / (1 << l)) if level_scale else 1.0)
    c = torch.where((c > -FAR) & (c < FAR), c, torch.full_like(c, -FAR))
    fl = torch.floor(c)
    return fl[:, 0].long() - radius, fl[:, 1].long() - radius, c[:, 0] - fl[:, 0], c[:, 1] - fl[:, 1]


def unfit(pos, nlev, radius):
    """bool [Q]: the queries corr_dvol_sep_kernel appends to the list.  pos: the n lookups' positions, each [Q, 2] fp32."""
    win = 2 * radius + 2
    out = torch.zeros(pos[0].shape[0], dtype=torch.bool)
    for l in range(nlev):
        o = [level_query(p, l, radius)[:2] for p in pos]
        for a in (0, 1):
            v = torch.stack([t[a] for t in o])
            out |= (v.max(0).values - v.min(0).values + win) > DVS_SIDE[l]
    return out


# ------------------------------------------------------------------------------------------------------------------ the scatter
def _taps(G):
    """G [Q, N1 (i), N1 (j)] -> t[(ax, ay)] [Q, WIN (wy), WIN (wx)] = G[wx - ax][wy - ay], 0 where there is no such entry."""
    Q, n, _ = G.shape
    P = torch.zeros(Q, n + 2, n + 2, dtype=G.dtype)
    P[:, 1:n + 1, 1:n + 1] = G
    return {(ax, ay): P[:, 1 - ax:n + 2 - ax, 1 - ay:n + 2 - ay].transpose(1, 2) for ax in (0, 1) for ay in (0, 1)}


def window_grad(G, fx, fy, form, acc=None):
    """Wd [Q, WIN, WIN] (wy, wx) of one lookup at one level in the dtype of G, every operation rounded to it.  'sep' adds into `acc`
    (what the kernel's registers hold) and returns it."""
    t = _taps(G)
    fx, fy = fx.view(-1, 1, 1), fy.view(-1, 1, 1)
    gx, gy = 1 - fx, 1 - fy
    if form == "four":
        a = torch.zeros_like(t[0, 0])
        for ay in (0, 1):
            for ax in (0, 1):
                a = a + t[ax, ay] * ((fy if ay else gy) * (fx if ax else gx))
        return a
    if form == "row":
        return gy * (gx * t[0, 0] + fx * t[1, 0]) + fy * (gx * t[0, 1] + fx * t[1, 1])
    if form == "cl":
        s0, s1 = t[0, 0] * gy + t[0, 1] * fy, t[1, 0] * gy + t[1, 1] * fy           # s[wx], s[wx - 1]
        return s0 * gx + s1 * fx
    assert form == "sep"
    T0, T1 = gx * t[0, 0] + fx * t[1, 0], gx * t[0, 1] + fx * t[1, 1]               # T[wy], T[wy - 1]
    acc = acc + gy * T0
    return acc + fy * T1


def _add_window(flat, h, w, wx0, wy0, Wd, on=None):
    """flat [Q, h w] += the window Wd [Q, WIN, WIN] at origin (wx0, wy0), cells outside the level dropped (their slots add an
    exact 0 to a cell of the row: the cells of one window are distinct).  on: bool [Q], the queries that hand in."""
    Q, win, _ = Wd.shape
    ar = torch.arange(win)
    gy, gx = wy0.view(-1, 1, 1) + ar.view(1, -1, 1), wx0.view(-1, 1, 1) + ar.view(1, 1, -1)
    ok = (gy >= 0) & (gy < h) & (gx >= 0) & (gx < w)
    if on is not None:
        ok = ok & on.view(-1, 1, 1)
    idx = (gy.clamp(0, h - 1) * w + gx.clamp(0, w - 1)).reshape(Q, -1)
    flat.scatter_add_(1, idx, torch.where(ok, Wd, torch.zeros_like(Wd)).reshape(Q, -1))


def scatter(pos, dout, plane, nlev, radius, dtype=torch.float64, form="four", old=None, swap=False, level_scale=True, scale=True):
    """(levels, S): levels[l] [Q, h_l, w_l] in `dtype` = old[l] + the scatter of the n lookups in order; S (float64, None unless
    `scale`): sum |w| |G| + |old|.  pos: n x [Q, 2] fp32 positions; dout: n x [Q, nlev N2] fp32; plane (H, W).  swap / level_scale:
    the mutants (i and j swapped; the 2^-l dropped)."""
    H, W = plane
    Q = pos[0].shape[0]
    n1 = 2 * radius + 1
    n2, win = n1 * n1, n1 + 1
    levels, S = [], []
    for l in range(nlev):
        h, w = H >> l, W >> l
        lv = (old[l].to(dtype).clone() if old is not None else torch.zeros(Q, h, w, dtype=dtype)).reshape(Q, h * w)
        sc = (old[l].double().abs() if old is not None else torch.zeros(Q, h, w, dtype=torch.float64)).reshape(Q, h * w).clone()
        acc, cur, have = torch.zeros(Q, win, win, dtype=dtype), None, False
        for p, g in zip(pos, dout):
            G = g[:, l * n2:(l + 1) * n2].reshape(Q, n1, n1)
            if swap:
                G = G.transpose(1, 2)
            wx0, wy0, fx, fy = level_query(p, l, radius, dtype, level_scale)
            if form == "sep":
                if have:
                    moved = (wx0 != cur[0]) | (wy0 != cur[1])
                    _add_window(lv, h, w, cur[0], cur[1], acc, moved)
                    acc = torch.where(moved.view(-1, 1, 1), torch.zeros_like(acc), acc)
                cur, have = (wx0, wy0), True
                acc = window_grad(G.to(dtype), fx, fy, "sep", acc)
            else:
                _add_window(lv, h, w, wx0, wy0, window_grad(G.to(dtype), fx, fy, form))
            if scale:
                x0, y0, ax, ay = level_query(p, l, radius, torch.float64, level_scale)
                _add_window(sc, h, w, x0, y0, window_grad(G.double().abs(), ax, ay, "four"))
        if form == "sep":
            _add_window(lv, h, w, cur[0], cur[1], acc)
        levels.append(lv.view(Q, h, w))
        S.append(sc.view(Q, h, w))
    return levels, (S if scale else None)


def split_error(x):
    """|x - (hi + lo)| / (2^-17 |x|), worst over x (fp32): what writing x as a record costs."""
    x = x.float()
    hi, lo = bf16_hi_lo(x)
    return need((hi.double() + lo.double()), x.double(), x.double().abs() * SPLIT_UNIT)[0]


def through_records(x):
    """fp32 -> what a record holds of it, decoded: hi + lo (exact in fp32: lo is below half an ulp of the bf16 hi)."""
    hi, lo = bf16_hi_lo(x.float())
    return hi + lo


def record_bound(key, ref, S, earlier=()):
    """Elementwise bound of a record output decoded (hi + lo): the fp32 limit of `key` plus one split of a value that close to
    `ref`, plus, per accumulating launch before this one, one split of what THAT launch wrote -- `earlier`: the float64 values of
    the launches before (a split costs in proportion to the value split, and the sum of 16 lookups may be far larger than the
    sum of 17 where the last one cancels it)."""
    b = LIMITS[key] * U24 * S
    cost = ref.abs() + b
    for e in earlier:
        cost = cost + e.abs() + b
    return b + LIMITS["split"] * SPLIT_UNIT * cost


# ------------------------------------------------------------------------------------------------------------------ k-tile marks
KT_NQ, KT_MC = 128, 256        # queries per NT list, cells per TN list (csrc/corr_tiled.hip)


def ktile_marks(pos, L, radius, exact=0, short=False):
    """corr_ktiles_mark_kernel per query, integer logic on level_query: (rec bool [Q, P / 32], tile bool [Q, ceil(P / 256)]) -- the
    records and the 256-cell tiles query q marks.  Per level the bounding rectangle of the lookups' windows, clipped to the level
    (levels below `exact`: each window on its own); every row of 4x4 tiles the rectangle overlaps is one run of cells from the
    first tile's first to the last tile's last.  pos: n x [Q, 2] fp32.  short: the mutant whose high edge is one cell short."""
    Q = pos[0].shape[0]
    nrec, mt = L["P"] // 32, (L["P"] + KT_MC - 1) // KT_MC
    rec, tile = torch.zeros(Q, nrec, dtype=torch.bool), torch.zeros(Q, mt, dtype=torch.bool)
    ar, at = torch.arange(nrec).view(1, -1), torch.arange(mt).view(1, -1)
    ext = 2 * radius + (0 if short else 1)
    for l in range(L["nlev"]):
        o = [level_query(p, l, radius)[:2] for p in pos]
        xs, ys = torch.stack([t[0] for t in o]), torch.stack([t[1] for t in o])
        if l < exact:
            rects = [(xs[t], xs[t], ys[t], ys[t]) for t in range(len(pos))]
        else:
            rects = [(xs.min(0).values, xs.max(0).values, ys.min(0).values, ys.max(0).values)]
        for mnx, mxx, mny, mxy in rects:
            x0, x1 = mnx.clamp(min=0), (mxx + ext).clamp(max=L["w"][l] - 1)
            y0, y1 = mny.clamp(min=0), (mxy + ext).clamp(max=L["h"][l] - 1)
            ok = (x0 <= x1) & (y0 <= y1)
            for ty in range(L["th"][l]):
                on = (ok & ((y0 >> 2) <= ty) & (ty <= (y1 >> 2))).view(-1, 1)
                c0 = (L["off"][l] + (ty * L["tw"][l] + (x0 >> 2)) * 16).view(-1, 1)
                c1 = (L["off"][l] + (ty * L["tw"][l] + (x1 >> 2)) * 16 + 15).view(-1, 1)
                rec |= on & (ar >= (c0 >> 5)) & (ar <= (c1 >> 5))
                tile |= on & (at >= c0 // KT_MC) & (at <= c1 // KT_MC)
    return rec, tile


def _pack_bits(m):
    """bool [R, n] -> int64 [R, ceil(n / 32)] words (bit k of word w = column 32 w + k), values as unsigned."""
    R_, n = m.shape
    nw = (n + 31) // 32
    p = torch.zeros(R_, nw * 32, dtype=torch.int64)
    p[:, :n] = m.long()
    return (p.view(R_, nw, 32) << torch.arange(32).view(1, 1, 32)).sum(2)


def ktile_lists(rec, tile):
    """One list set (an image, or a chunk) from the per-query marks: dict(nt: ascending records per 128-query tile; tn_bits
    [ceil(Q / 32), ceil(mtiles / 32)] words; tn: ascending 32-query blocks per 256-cell tile; wmask [ceil(Q / 32), ceil(nrec / 32)]
    words = the 128-query tile's records | eight records per cell tile the 32-query block marks)."""
    Q, nrec = rec.shape
    mt = tile.shape[1]
    ktq, nw = (Q + 31) // 32, (nrec + 31) // 32
    nt_rows = torch.stack([rec[t:t + KT_NQ].any(0) for t in range(0, Q, KT_NQ)])
    blocks = torch.stack([tile[k:k + 32].any(0) for k in range(0, Q, 32)])                   # [ktq, mt]
    eight = torch.zeros(ktq, nw * 32, dtype=torch.bool)
    rep = blocks.repeat_interleave(8, 1)[:, :nw * 32]
    eight[:, :rep.shape[1]] = rep
    rb = torch.zeros(ktq, nw * 32, dtype=torch.bool)
    rb[:, :nrec] = nt_rows.repeat_interleave(KT_NQ // 32, 0)[:ktq]
    return dict(nt=[r.nonzero().view(-1).tolist() for r in nt_rows], tn_bits=_pack_bits(blocks),
                tn=[blocks[:, m].nonzero().view(-1).tolist() for m in range(mt)], wmask=_pack_bits(rb | eight), wbits=(rb | eight)[:, :nrec])


# B x H x W, levels; query counts 127, 128, 129 around the 128-query tile with the level counts each admits; B > 1 with a ragged
# last tile; 2x32x48, where a small flow ('local') leaves most of a tile's records unmarked; 1x64x129: 8256 queries = 258 blocks of 32 (the second trip of corr_ktiles_tn_kernel's 256-block loop), 44 cell tiles
# (two words of the tile bitmap)
KT_SHAPES = [((1, 1, 127), 1), ((1, 8, 16), 1), ((1, 8, 16), 2), ((1, 8, 16), 3), ((1, 8, 16), 4), ((1, 3, 43), 1), ((1, 3, 43), 2),
             ((2, 16, 24), 4), ((3, 5, 9), 2), ((2, 32, 48), 4)]
KT_BIG = ((1, 64, 129), 4)
# chunks (shape, levels, q0, nq): q0 no multiple of 32 or 128, a ragged last tile; the second inside image 1
KT_CHUNKS = [((2, 16, 24), 4, 37, 200), ((2, 16, 24), 4, 384 + 133, 131), ((1, 64, 129), 4, 1037, 67)]
KT_RUNS = [("near", 16, 1), ("alt", 7, 0), ("limit", 2, 0), ("jump", 6, 1), ("edge", 6, 0), ("local", 7, 1)]


# ------------------------------------------------------------------------------------------------------------------ f2cat, dfmap2
def f2cat(f2, nlev, dtype=torch.float64, form="block"):
    """fmap2 [B, C, H, W] -> levels[l] [B C, h_l, w_l] in `dtype`."""
    B, C, H, W = f2.shape
    a = f2.reshape(B * C, H, W).to(dtype)
    levels = [a]
    for l in range(1, nlev):
        h, w, k = H >> l, W >> l, 1 << l
        if form == "rec":
            p = levels[-1][:, :2 * h, :2 * w]
            levels.append(0.25 * ((p[:, 0::2, 0::2] + p[:, 0::2, 1::2]) + (p[:, 1::2, 0::2] + p[:, 1::2, 1::2])))
            continue
        blk = a[:, :h * k, :w * k].reshape(B * C, h, k, w, k).permute(0, 1, 3, 2, 4).reshape(-1, k * k)       # row-major in the block
        s = (blk[:, 0] + blk[:, 1]) + (blk[:, 2] + blk[:, 3]) if l == 1 else D._sum_sequential(blk)
        levels.append((s * (1.0 / (1 << (2 * l)))).reshape(B * C, h, w))
    return levels


def _cells(L, l):
    """(exists bool [H W], cell index int64 [H W]) of level-l cell (y >> l, x >> l) for every pixel of the plane."""
    H, W = L["H"], L["W"]
    y = torch.arange(H).view(H, 1).expand(H, W).reshape(-1) >> l
    x = torch.arange(W).view(1, W).expand(H, W).reshape(-1) >> l
    return (y < L["h"][l]) & (x < L["w"][l]), L["off"][l] + ((y >> 2) * L["tw"][l] + (x >> 2)) * 16 + (y & 3) * 4 + (x & 3)


def dfmap2(d2cat, L, dtype=torch.float64, twice=False, unchecked=None, absolute=False):
    """d2cat [B, P, C] -> d2 [B, H W, C]: acc += wgt v over the levels in order, wgt = 4^-l.  twice (4^-l applied twice) and
    unchecked (a level whose existence check is missing) are the mutants; absolute: the scale (sum of |terms|)."""
    B, P, C = d2cat.shape
    acc, wgt = torch.zeros(B, L["H"] * L["W"], C, dtype=dtype), 1.0
    for l in range(L["nlev"]):
        ok, cell = _cells(L, l)
        if l == unchecked:
            ok = torch.ones_like(ok)
        v = d2cat[:, cell.clamp(max=P - 1), :].to(dtype)
        acc = torch.where(ok.view(1, -1, 1), acc + wgt * (v.abs() if absolute else v), acc)
        wgt *= 0.0625 if twice else 0.25
    return acc


def volume_bwd(f1, f2l, dvl):
    """The two contractions of the volume's backward and the un-pooling, in float64, level by level:
        dF1[b, c, i] = s sum_l sum_cells f2cat_l[b, c, cell] dV_l[b, i, cell],          s = 1 / sqrt(C)
        dF2[b, i, c] = sum_l 4^-l d2cat_l[b, cell_l(i), c] where the cell exists,       d2cat_l[b, cell, c] = s sum_i dV_l[b, i, cell] f1[b, c, i]
    f1 [B, C, H, W]; f2l[l] [B C, h_l, w_l] (f2cat's levels); dvl[l] [B H W, h_l, w_l].  Handed absolute values it gives the scale, handed
    an error in one operand and absolute values in the others what that error grows to."""
    Bn, C, H, W = f1.shape
    N, s = H * W, 1.0 / C ** 0.5
    f1m = f1.double().reshape(Bn, C, N)
    d1, d2 = torch.zeros(Bn, C, N, dtype=torch.float64), torch.zeros(Bn, N, C, dtype=torch.float64)
    for l, v in enumerate(dvl):
        h, w = v.shape[1:]
        v = v.double().reshape(Bn, N, h * w)
        d1 += s * torch.einsum("bcp,bip->bci", f2l[l].double().reshape(Bn, C, h * w), v)
        d2cat = s * torch.einsum("bip,bci->bpc", v, f1m)
        y, x = torch.arange(H) >> l, torch.arange(W) >> l
        idx = (y.clamp(max=h - 1).view(H, 1) * w + x.clamp(max=w - 1).view(1, W)).reshape(-1)
        ok = ((y < h).view(H, 1) & (x < w).view(1, W)).reshape(1, N, 1)
        d2 += 0.25 ** l * d2cat[:, idx, :] * ok
    return d1, d2


# ------------------------------------------------------------------------------------------------------------------ unpool_bwd
def unpool_bwd(levels, dtype=torch.float64, form="sum", absolute=False):
    """levels[l] [Q, h_l, w_l] -> the new level 0.  'sum': g0 + sum_l 4^-l g_l[y >> l][x >> l] where the cell exists; 'chain': the
    kernels' up = g_l + 0.25 up from the top, cut where a cell does not exist, then g0 + 0.25 up."""
    Q, H, W = levels[0].shape
    lv = [(t.abs() if absolute else t).to(dtype) for t in levels]
    y, x = torch.arange(H).view(H, 1).expand(H, W), torch.arange(W).view(1, W).expand(H, W)
    pick = lambda l: lv[l][:, (y >> l).clamp(max=lv[l].shape[1] - 1), (x >> l).clamp(max=lv[l].shape[2] - 1)]      # noqa: E731
    ok = lambda l: (((y >> l) < lv[l].shape[1]) & ((x >> l) < lv[l].shape[2])).view(1, H, W)                        # noqa: E731
    if form == "sum":
        out = lv[0].clone()
        for l in range(1, len(lv)):
            out = out + torch.where(ok(l), pick(l) * (0.25 ** l), torch.zeros_like(out))
        return out
    up = torch.zeros_like(lv[0])
    for l in range(len(lv) - 1, 0, -1):
        up = torch.where(ok(l), pick(l) + 0.25 * up, torch.zeros_like(up))
    return lv[0] + 0.25 * up


# ------------------------------------------------------------------------------------------------------------------ coordinates
def _flat(c):
    """[B, 2, H, W] -> [B H W, 2]"""
    return c.permute(0, 2, 3, 1).reshape(-1, 2).contiguous()


def positions(shape, radius, family, n):
    """n x [B, 2, H, W] fp32 POSITIONS (multiples of 1/64, so that position - grid is exact).  Families:
    near   a base (integer + 1/4) plus a jitter in [0, 1/2]: the level-0 origin of a query stays where it is but for every third
           lookup, which is one cell to the right -- nothing spreads beyond a box, origins repeat over consecutive lookups
    alt    origins A, B, A, B, ... one cell apart in x at level 0 (base even: the coarser levels do not move)
    limit  two lookups whose level-0 origins differ by side - WIN (variant even) or one more (odd), in x (variants 0..5) or in y
           (6..11); the smaller origin is 0 mod 4, 3 mod 4 or negative; variant = query % 12
    jump   every second lookup 40 px to the right and down
    local  near, with the query's own pixel as the base (a small flow: the windows of neighbouring queries overlap, and a tile of
           128 queries reaches a band of the plane only); every fifth query jumps 40 px in lookup 1 and so leaves the fast kernel
    edge   _dcoordsref.mixed_positions, another draw per lookup; the first row of every sample at +-1e6 in every lookup; the last
           query of every sample far in lookup 0 only"""
    B, H, W = shape
    Q = B * H * W
    g = D._gen("bwdpos", B, H, W, radius, family, n)
    out = []
    if family in ("near", "alt", "jump", "local"):
        bx = torch.randint(-2, W + 3, (Q,), generator=g).float()
        by = torch.randint(-2, H + 3, (Q,), generator=g).float()
        if family == "local":
            grid = _flat(D.grid(B, H, W))
            bx, by = grid[:, 0], grid[:, 1]
        if family == "alt":
            bx = torch.floor(bx / 2) * 2
        for t in range(n):
            j = torch.randint(0, 33, (Q, 2), generator=g).float() / 64
            if family in ("near", "local"):
                dx, dy = j[:, 0] + (1.0 if t % 3 == 2 else 0.0), j[:, 1]
                if family == "local" and t == 1:
                    dx = dx + 40.0 * (torch.arange(Q) % 5 == 0)
            elif family == "alt":
                dx, dy = j[:, 0] * 0 + float(t % 2), j[:, 1]
            else:
                dx, dy = j[:, 0] + 40.0 * (t % 2), j[:, 1] + 40.0 * (t % 2)
            out.append(torch.stack([bx + 0.25 + dx, by + 0.25 + dy], 1))
    elif family == "limit":
        assert n == 2
        v = torch.arange(Q) % 12
        axis, k = v // 6, v % 6
        delta = (DVS_SIDE[0] - (2 * radius + 2)) + (k % 2)
        o = torch.tensor([4, 7, -5])[k // 2] + radius                      # floor(c) of the smaller origin: origin = 4, 7, -5
        other = torch.randint(0, max(min(H, W) - 1, 1), (Q,), generator=g).float() + 0.5
        a, b = o.float() + 0.5, (o + delta).float() + 0.25
        first = torch.where(axis.view(-1, 1) == 0, torch.stack([a, other], 1), torch.stack([other, a], 1))
        second = torch.where(axis.view(-1, 1) == 0, torch.stack([b, other], 1), torch.stack([other, b], 1))
        out = [first, second]
    else:
        assert family == "edge"
        far = torch.tensor([1e6, -1e6]).repeat((W + 1) // 2)[:W]
        for t in range(n):
            x, y = D.mixed_positions(Q, H, W, g)
            c = torch.stack([x.view(B, H, W), y.view(B, H, W)], 1).contiguous()
            c[:, 0, 0, :] = far
            c[:, 1, 0, :] = -far
            if t == 0 and n > 1:
                c[:, 0, H - 1, W - 1] = 1e6
            out.append(_flat(c))
    return [p.view(B, H, W, 2).permute(0, 3, 1, 2).contiguous() for p in out]


def douts(shape, nlev, radius, kind, n):
    """n x [B, H, W, CH] fp32: gaussian (another draw per lookup), or _dcoordsref.dout_values' zero / hot kinds for every lookup."""
    B, H, W = shape
    ch = nlev * (2 * radius + 1) ** 2
    if kind == "gauss":
        return [torch.randn(B, H, W, ch, generator=D._gen("bwddout", B, H, W, nlev, radius, t)) for t in range(n)]
    return [D.dout_values(B, H, W, nlev, radius, kind) for _ in range(n)]


# ------------------------------------------------------------------------------------------------------------------ dvol cases
# B x H x W, levels: _corrref.TILED_SHAPES; 1x9x17 (level 0 is 3 x 5 = 15 tiles = 240 floats, no multiple of 32: level 1 is pulled
# into the first job of the record route); two shapes whose first run is longer than the 8192-float segment, run as a chunk of 67
# queries (67 % 4 = 3) from a first query that is no multiple of 32: 1x64x129 (level 0 alone: 8448 floats) and 1x92x92 (8464,
# 10768, 11344 and 11488 floats: no level but the last ends on a multiple of 32, so all four form one run).
DVOL_SHAPES = R.TILED_SHAPES + [((1, 9, 17), 4)]
CLIP_SHAPES = [((1, 64, 129), 4, 1037, 67), ((1, 92, 92), 4, 4231, 67)]
# (family, lookups, add_grid, dout kind) per shape and radius.  Lookup counts 1, 6, 7, 16: the prefetch ring of 6 at its wrap, the
# launch limit.  The 'near' run is followed by a 17th lookup with accumulate = 1 (`extra`); 'hot': zero, or a one on the first / last
# channel of a level, another kind per shape and radius (hot_kind).
RUNS = [("near", 16, 1, "gauss"), ("alt", 7, 0, "gauss"), ("limit", 2, 0, "gauss"), ("jump", 6, 1, "gauss"), ("edge", 6, 0, "gauss"),
        ("edge", 1, 1, "hot")]
CLIP_RUNS = [("edge", 2, 0, "gauss"), ("near", 7, 1, "gauss")]


# the masked runs of the gradient volume (wmask from fsraft_corr_bwd_ktiles): a whole batch of 32x48 planes (64 records a row: at
# 16x24 every mask is full), two chunks of it off the 32- and 128-query grids, the second in image 1, and the first clipped chunk
WMASK_SETS = [((2, 32, 48), 4, 0, 0), ((2, 32, 48), 4, 37, 200), ((2, 32, 48), 4, 1536 + 133, 131), ((1, 64, 129), 4, 1037, 67)]
WMASK_RUNS = [("local", 7, 1, "gauss"), ("edge", 2, 0, "gauss")]


CHAIN_CASE = (R.CHAIN[0], R.CHAIN[1], 4, "local", 7, 1, "gauss", 0, 0, False)       # the lookups of the chain test, at _corrref.CHAIN


def hot_kind(nlev, radius, i):
    kinds = D.dout_kinds(nlev)[1:]
    return kinds[i % len(kinds)]


@functools.lru_cache(maxsize=None)
def dvol_case(shape, nlev, radius, family, n, add_grid, dkind, q0=0, nq=0, extra=False):
    """given (what the kernel is handed: the flow when add_grid), pos / dout of the queries [q0, q0 + nq) flat, the float64 levels
    and scales, the predicted list.  extra: one more lookup (the accumulating launch): ref17 / S17 cover all n + 1."""
    B, H, W = shape
    n_all = n + (1 if extra else 0)
    pos = positions(shape, radius, family, n) + (positions(shape, radius, "edge", 1) if extra else [])
    grid = D.grid(B, H, W)
    given = [p - grid if add_grid else p for p in pos]
    if add_grid:
        far = [p.abs() >= 1e5 for p in pos]
        given = [torch.where(f, p, gv) for f, p, gv in zip(far, pos, given)]        # (+-1e6 stays far with the grid added)
        pos = [gv + grid for gv in given]
    dout = douts(shape, nlev, radius, dkind, n_all)
    sl = slice(q0, q0 + nq) if nq else slice(None)
    fp = [_flat(p)[sl] for p in pos]
    fd = [d.reshape(B * H * W, -1)[sl] for d in dout]
    ref, S = scatter(fp[:n], fd[:n], (H, W), nlev, radius)
    c = dict(given=given, dout=dout, pos=fp, fdout=fd, ref=ref, S=S, unfit=unfit(fp[:n], nlev, radius), n=n)
    if extra:
        c["ref17"], c["S17"] = scatter(fp, fd, (H, W), nlev, radius)
    return c


def dvol_cases():
    """(shape, nlev, radius, family, n, add_grid, dout kind, q0, nq, extra)"""
    for shape, nlev in DVOL_SHAPES:
        for radius in R.RADII:
            for family, n, add_grid, dkind in RUNS:
                if dkind == "hot":
                    dkind = hot_kind(nlev, radius, DVOL_SHAPES.index((shape, nlev)) + radius)
                yield shape, nlev, radius, family, n, add_grid, dkind, 0, 0, family == "near"
    for shape, nlev, q0, nq in CLIP_SHAPES:
        for radius in R.RADII:
            for family, n, add_grid, dkind in CLIP_RUNS:
                yield shape, nlev, radius, family, n, add_grid, dkind, q0, nq, False
    yield CHAIN_CASE
    for shape, nlev, q0, nq in WMASK_SETS:
        for radius in R.RADII:
            for family, n, add_grid, dkind in WMASK_RUNS:
                yield shape, nlev, radius, family, n, add_grid, dkind, q0, nq, False


# ------------------------------------------------------------------------------------------------------------------ other cases
F2_C = (1, 3, 4, 32)
# the second trips of the grid-stride loops (16384 blocks of 256): f2cat 2 x 256 planes of 64x129 (B C P = 5.7 M), the scalar dfmap2
# 2 x 8256 x 255 (4.21 M), the vector one 8 x 8256 x 256 / 4 (4.23 M)
F2_BIG = ((2, 64, 129), 256)
DF_BIG = [((2, 64, 129), 255), ((8, 64, 129), 256)]
F2_MAXPLANE = ((1, 96, 128), 1)                       # exactly 12288 pixels: the largest plane corr_f2cat_rec_kernel takes


def f2_values(shape, C):
    B, H, W = shape
    return torch.randn(B, C, H, W, generator=D._gen("f2", B, H, W, C))


def d2cat_values(shape, C, L):
    """[B, P, C] gaussian, the NaN pattern in every pad cell and in the tail (the kernels must not read them)."""
    from _util import PATTERN
    B = shape[0]
    v = torch.randn(B, L["P"], C, generator=D._gen("d2cat", *shape, C))
    v[:, ~R.cell_mask(L), :] = torch.tensor(PATTERN, dtype=torch.int32).view(torch.float32)
    return v


# rows x h x w, levels: 3x9x11 (floor pooling drops the last column and row at every level; scalar); 2x8x8 (vector); 1x8x12 (vector
# by its width, scalar because the test moves level 0 off its alignment); 1x37x41 (1517 rows: 2.30 M cells, the scalar kernel's
# second trip past 8192 blocks); 1x64x68 (4352 rows: 4.73 M float4, the vector kernel's second trip past 16384 blocks)
UNPOOL_CASES = [((3, 9, 11), n) for n in (1, 2, 3, 4)] + [((2, 8, 8), 4), ((1, 8, 12), 4), ((1, 37, 41), 4), ((1, 64, 68), 4)]


def unpool_values(shape, nlev):
    B, H, W = shape
    return [torch.randn(B * H * W, H >> l, W >> l, generator=D._gen("unpool", B, H, W, nlev, l)) for l in range(nlev)]


@functools.lru_cache(maxsize=None)
def lookup_bwd_case(shape, radius):
    """dlevels start gaussian; two lookups (mixed positions, two draws) are applied one after the other."""
    B, H, W = shape
    old = [torch.randn(B * H * W, H >> l, W >> l, generator=D._gen("dlev", B, H, W, l)) for l in range(4)]
    pos = positions(shape, radius, "edge", 2)
    dout = douts(shape, 4, radius, "gauss", 2)
    fp, fd = [_flat(p) for p in pos], [d.reshape(B * H * W, -1) for d in dout]
    ref, S = scatter(fp, fd, (H, W), 4, radius, old=old)
    return dict(old=old, given=pos, dout=dout, pos=fp, fdout=fd, ref=ref, S=S)


# ------------------------------------------------------------------------------------------------------------------ the twins' worst
def twins_worst(big=True):
    """{key: (worst figure in the key's unit, the case)} of every twin against float64 over the cases above."""
    worst = {k: (0.0, "") for k in LIMITS}

    def see(key, got, ref, scale, case):
        w, _ = need(got, ref, scale * U24)
        if w > worst[key][0]:
            worst[key] = (w, case)

    def see_split(x, case):
        w = split_error(x)
        if w > worst["split"][0]:
            worst["split"] = (w, case)

    for case in dvol_cases():
        shape, nlev, radius, family, n, add_grid, dkind, q0, nq, extra = case
        c = dvol_case(*case)
        plane = shape[1:]
        for form in ("row", "sep"):
            tw, _ = scatter(c["pos"][:n], c["fdout"][:n], plane, nlev, radius, torch.float32, form, scale=False)
            for l in range(nlev):
                see("dvol." + form, tw[l], c["ref"][l], c["S"][l], f"{case} level {l}")
                see_split(tw[l], f"dvol {case}")
            if extra:
                tw, _ = scatter(c["pos"][n:], c["fdout"][n:], plane, nlev, radius, torch.float32, "row", old=tw, scale=False)
                for l in range(nlev):
                    see("dvol.row", tw[l], c["ref17"][l], c["S17"][l], f"{case} level {l}, 16 + 1 lookups after {form}")
                    see_split(tw[l], f"dvol {case}")
    f2_cases = [(s, n, C) for s, n in DVOL_SHAPES for C in F2_C] + [(F2_MAXPLANE[0], 4, F2_MAXPLANE[1]), R.CHAIN]
    if big:
        f2_cases.append((F2_BIG[0], 4, F2_BIG[1]))
    for shape, nlev, C in f2_cases:
        f2 = f2_values(shape, C)
        ref, S = f2cat(f2, nlev), f2cat(f2.abs(), nlev)
        for form in ("block", "rec"):
            tw = f2cat(f2, nlev, torch.float32, form)
            for l in range(nlev):
                see("f2cat." + form, tw[l], ref[l], S[l], f"{shape} C {C} level {l}")
                see_split(tw[l], f"f2cat {shape} C {C}")
    for shape, nlev, C in [(s, n, C) for s, n in DVOL_SHAPES for C in F2_C] + [R.CHAIN] + ([(s, 4, C) for s, C in DF_BIG] if big else []):
        L = R.vol_layout(shape[1], shape[2], nlev)
        v = d2cat_values(shape, C, L)
        see("dfmap2", dfmap2(v, L, torch.float32), dfmap2(v, L), dfmap2(v, L, absolute=True), f"{shape} L{nlev} C {C}")
    for shape, nlev in UNPOOL_CASES:
        if not big and shape[1] * shape[2] > 1000:
            continue
        lv = unpool_values(shape, nlev)
        see("unpool", unpool_bwd(lv, torch.float32, "chain"), unpool_bwd(lv), unpool_bwd(lv, absolute=True), f"{shape} L{nlev}")
    for shape, nlev in R.ROW_SHAPES:
        for radius in R.RADII:
            c = lookup_bwd_case(shape, radius)
            for form in ("four", "cl"):
                tw, _ = scatter(c["pos"], c["fdout"], shape[1:], 4, radius, torch.float32, form, old=c["old"], scale=False)
                for l in range(4):
                    see("lookup_bwd." + form, tw[l], c["ref"][l], c["S"][l], f"{shape} r{radius} level {l}")
    return worst
