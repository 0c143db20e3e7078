"""tests/_corrbwdref.py -- the float64 restatements of the correlation path's backward kernels -- checked on the CPU, without a
kernel: every transpose against the forward restatement of tests/_corrref.py (<dout, A V> = <A^T dout, V> in float64), the scatter
against torch.autograd through _corrref.lookup, the query-list prediction against a brute-force search for a box, the coordinate
families against the routes they are built for, the k-tile marks against loops and against the float64 gradient's non-zero records,
volume_bwd against autograd down to the feature maps, LIMITS against the fp32 twins over the GPU tests' cases, the record bound
against an fp32 twin of the record chain, and every mutant (a wrong restatement) against the limits or the lists.
"""
import pytest
import torch

import _corrbwdref as B
import _corrref as R
import _dcoordsref as D
from _util import PATTERN

_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)      # noqa: E731
SMALL = [((1, 10, 14), 4), ((3, 5, 9), 2), ((1, 9, 17), 4)]


def _dot(a, b):
    return float(sum((x.double() * y.double()).sum() for x, y in zip(a, b)))


def _close(a, b, what):
    print(f"{what}: {a!r} vs {b!r}")
    assert abs(a - b) <= 1e-12 * max(abs(a), abs(b), 1e-300), what


# ------------------------------------------------------------------------------------------------ transposes
@pytest.mark.parametrize("radius", R.RADII)
@pytest.mark.parametrize("shape,nlev", SMALL, ids=_ids)
def test_scatter_is_the_transpose_of_the_lookup(shape, nlev, radius):
    """sum_t <dout_t, lookup_t(V)> = <scatter(dout), V> for random V, and the scatter = autograd through _corrref.lookup."""
    Bn, H, W = shape
    for family, n in (("edge", 3), ("near", 2), ("limit", 2)):
        pos = B.positions(shape, radius, family, n)
        dout = B.douts(shape, nlev, radius, "gauss", n)
        V = [lv.double().requires_grad_(True) for lv in D.level_values(Bn, H, W, nlev)]
        fwd = sum((R.lookup(V, p, radius)[0] * d.double()).sum() for p, d in zip(pos, dout))
        got, S = B.scatter([B._flat(p) for p in pos], [d.reshape(Bn * H * W, -1) for d in dout], (H, W), nlev, radius)
        _close(float(fwd.detach()), _dot(got, [v.detach() for v in V]), f"{shape} r{radius} {family}")
        grads = torch.autograd.grad(fwd, V)
        for l in range(nlev):
            assert float((grads[l] - got[l]).abs().max()) <= 1e-12 * max(float(S[l].max()), 1e-300), (family, l)
            assert bool((got[l][S[l] == 0] == 0).all())
        for form in ("row", "sep", "cl"):                               # every form is the same mathematics
            alt, _ = B.scatter([B._flat(p) for p in pos], [d.reshape(Bn * H * W, -1) for d in dout], (H, W), nlev, radius, form=form, scale=False)
            assert max(B.need(alt[l], got[l], S[l] * 2.0 ** -53)[0] for l in range(nlev)) <= 64, form


@pytest.mark.parametrize("shape,nlev", [((3, 9, 11), 4), ((2, 8, 8), 4), ((1, 5, 7), 2), ((3, 9, 11), 1)], ids=_ids)
def test_unpool_bwd_is_the_transpose_of_pool_floor(shape, nlev):
    g = B.unpool_values(shape, nlev)
    V = torch.randn(*g[0].shape, generator=D._gen("V", *shape), dtype=torch.float64)
    lhs = _dot(g, R.pool_floor(V, nlev))
    out = B.unpool_bwd(g)
    _close(lhs, _dot([out], [V]), f"{shape} L{nlev}")
    assert float((B.unpool_bwd(g, form="chain") - out).abs().max()) <= 1e-14


@pytest.mark.parametrize("shape,nlev", SMALL + [((1, 8, 8), 1)], ids=_ids)
def test_dfmap2_is_the_transpose_of_f2cat(shape, nlev):
    Bn, H, W = shape
    C = 3
    L = R.vol_layout(H, W, nlev)
    f2 = B.f2_values(shape, C).double()
    lv = B.f2cat(f2, nlev)
    for a, b in zip(lv, R.pool_floor(f2.reshape(Bn * C, H, W), nlev)):        # the block sum is the floor pyramid
        assert float((a - b).abs().max()) <= 1e-15
    for a, b in zip(lv, B.f2cat(f2, nlev, form="rec")):
        assert float((a - b).abs().max()) <= 1e-15
    d2cat = torch.randn(Bn, L["P"], C, generator=D._gen("tr", *shape), dtype=torch.float64)
    d2 = B.dfmap2(d2cat, L)
    exact = torch.zeros(Bn * C, L["P"], dtype=torch.float64)                     # f2cat's rows by the documented cell formula
    for l, t in enumerate(lv):
        for y in range(t.shape[1]):
            for xx in range(t.shape[2]):
                exact[:, R.cell_index(L, l, y, xx)] = t[:, y, xx]
    cells = R.cell_mask(L)
    assert bool((exact[:, ~cells] == 0).all())
    x = f2.reshape(Bn, C, H * W)
    lhs = float((d2cat.permute(0, 2, 1).reshape(Bn * C, -1)[:, cells] * exact[:, cells]).sum())
    rhs = float((d2.permute(0, 2, 1) * x).sum())
    _close(lhs, rhs, f"{shape} L{nlev}")


def test_volume_bwd_is_the_gradient_of_build_and_lookup():
    """_corrbwdref.volume_bwd of the scatter = autograd through _corrref.pool_floor and _corrref.lookup down to the feature maps."""
    shape, nlev, C, r = (1, 10, 14), 4, 3, 3
    f1, f2 = R.fmaps(shape, C, "gauss")
    f1d, f2d = f1.double().requires_grad_(True), f2.double().requires_grad_(True)
    c = B.dvol_case(shape, nlev, r, "edge", 2, 0, "gauss")
    v = torch.einsum("bci,bcj->bij", f1d.reshape(1, C, -1), f2d.reshape(1, C, -1)) / C ** 0.5
    levels = R.pool_floor(v.reshape(140, 10, 14), nlev)
    loss = sum((R.lookup(levels, p, r)[0] * d.double()).sum() for p, d in zip(B.positions(shape, r, "edge", 2), c["dout"]))
    g1, g2 = torch.autograd.grad(loss, [f1d, f2d])
    d1, d2 = B.volume_bwd(f1, B.f2cat(f2, nlev), c["ref"])
    assert float((g1.reshape(1, C, -1) - d1).abs().max()) <= 1e-12 * float(d1.abs().max())
    assert float((g2.reshape(1, C, -1).permute(0, 2, 1) - d2).abs().max()) <= 1e-12 * float(d2.abs().max())


# ------------------------------------------------------------------------------------------------ the query list
def _fits_brute(pos, nlev, radius):
    """A query stays on the fast kernel iff at every level some side x side box holds all its windows: searched origin by origin."""
    win = 2 * radius + 2
    Q = pos[0].shape[0]
    fit = torch.ones(Q, dtype=torch.bool)
    for l in range(nlev):
        side = B.DVS_SIDE[l]
        o = [B.level_query(p, l, radius)[:2] for p in pos]
        for q in range(Q):
            for a in (0, 1):
                v = [int(t[a][q]) for t in o]
                found = any(all(b0 <= x and x + win <= b0 + side for x in v) for b0 in range(min(v) - side, min(v) + 1))
                fit[q] &= found
    return fit


def test_query_list_prediction_and_the_families_routes():
    seen = {}
    for shape, nlev in [((1, 10, 14), 4), ((2, 8, 16), 4), ((3, 5, 9), 2)]:
        Q = shape[0] * shape[1] * shape[2]
        for radius in R.RADII:
            for family, n in (("near", 16), ("alt", 7), ("limit", 2), ("jump", 6), ("edge", 6)):
                pos = [B._flat(p) for p in B.positions(shape, radius, family, n)]
                u = B.unfit(pos, nlev, radius)
                assert torch.equal(~u, _fits_brute(pos, nlev, radius)), (shape, radius, family)
                seen[family] = seen.get(family, 0) + int(u.sum())
                if family in ("near", "alt"):
                    assert int(u.sum()) == 0
                elif family == "jump":
                    assert int(u.sum()) == Q
                elif family == "limit":
                    v = torch.arange(Q) % 12
                    assert torch.equal(u, v % 2 == 1)                     # side - WIN fits, one more does not, in x and in y
                    o0, o1 = (B.level_query(p, 0, radius) for p in pos)
                    d = torch.where(v < 6, o1[0] - o0[0], o1[1] - o0[1])
                    assert torch.equal(d, (24 - 2 * radius - 2) + v % 2)
                    small = torch.where(v < 6, o0[0], o0[1])
                    assert torch.equal(small, torch.tensor([4, 7, -5])[(v % 6) // 2])
                    assert 0 < int(u.sum()) < Q
                else:
                    assert 0 < int(u.sum()) < Q                           # far in one lookup only: on the list; all far: not
                    far_all = torch.zeros(Q, dtype=torch.bool).view(shape)
                    far_all[:, 0, :] = True
                    assert not bool(u[far_all.view(-1)].any())
                    assert bool(u.view(shape)[:, -1, -1].all())
                if family == "alt":       # level 0 alternates between two origins one cell apart; the coarser levels stay
                    o = [[B.level_query(p, l, radius)[0] for p in pos] for l in range(nlev)]
                    assert all(torch.equal(o[0][t] - o[0][0], torch.full((Q,), t % 2)) for t in range(n))
                    assert all(torch.equal(o[l][t], o[l][0]) for l in range(1, nlev) for t in range(n))
                if family == "near":      # origins repeat over consecutive lookups, and change at every third
                    o = [B.level_query(p, 0, radius)[0] for p in pos]
                    assert torch.equal(o[0], o[1]) and torch.equal(o[2], o[0] + 1) and torch.equal(o[3], o[0])
    print(seen)


def test_the_cases_reach_what_they_are_meant_to():
    """The shapes at the edges of the launch geometry (csrc/corr_tiled.hip: DV_SEG = 8192 floats, records of 32, grid caps)."""
    L = R.vol_layout(9, 17, 4)
    assert L["off"][1] == 240 and L["off"][1] % 32 != 0                  # level 0 ends off a record: level 1 joins its job
    L = R.vol_layout(64, 129, 4)
    assert L["off"][1] == 8448 > 8192 and L["off"][1] % 32 == 0          # level 0 alone, clipped
    L = R.vol_layout(92, 92, 4)
    assert [o % 32 for o in L["off"][1:]] == [16, 16, 16] and L["P"] == 11488 > 8192       # one run of four levels, clipped
    for _, _, q0, nq in B.CLIP_SHAPES:
        assert q0 % 32 != 0 and nq % 4 == 3
    assert 2 * 256 * R.vol_layout(64, 129, 4)["P"] > 16384 * 256
    assert 2 * 64 * 129 * 255 > 16384 * 256 and 255 % 4 != 0
    assert 8 * 64 * 129 * 256 // 4 > 16384 * 256
    assert (37 * 41) ** 2 > 8192 * 256 and 41 % 4 != 0
    assert (64 * 68) ** 2 // 4 > 16384 * 256 and 68 % 4 == 0
    assert B.F2_MAXPLANE[0][1] * B.F2_MAXPLANE[0][2] == 12288
    assert sorted({c[4] for c in B.dvol_cases()}) == [1, 2, 6, 7, 16]
    assert {c[3] for c in B.dvol_cases()} == {"near", "alt", "limit", "jump", "edge", "local"}
    for shape, nlev, q0, nq in B.WMASK_SETS:       # the masked runs: records left out of rows of the fast kernel; rows for both kernels
        L = R.vol_layout(shape[1], shape[2], nlev)
        for radius in R.RADII:
            c = B.dvol_case(shape, nlev, radius, *B.WMASK_RUNS[0], q0, nq)
            HW = nq or shape[1] * shape[2]
            left = 0
            for s in range(c["pos"][0].shape[0] // HW):
                k = B.ktile_lists(*B.ktile_marks([p[s * HW:(s + 1) * HW] for p in c["pos"]], L, radius))
                fit = ~c["unfit"][s * HW:(s + 1) * HW]
                left += int((~k["wbits"].repeat_interleave(32, 0)[:HW] & fit.view(-1, 1)).sum())
            print(f"masked run {shape} {q0}+{nq} r{radius}: {left} records left out, {int(c['unfit'].sum())} queries listed")
            assert left > 0 and 0 < int(c["unfit"].sum()) < c["unfit"].numel()
    hot = {c[6] for c in B.dvol_cases()} - {"gauss"}
    assert len(hot) >= 6, hot                                            # zero and first / last channels of several levels


# ------------------------------------------------------------------------------------------------ limits
def test_limits_come_from_the_twins():
    """LIMITS = 4 x the worst the fp32 twins reach over every case of the kernel tests, rounded up to one digit."""
    worst = B.twins_worst()
    for key, (w, case) in sorted(worst.items()):
        print(f"{key}: twins' worst {w:.4f} (limit {B.LIMITS[key]:g}) at {case}")
    assert set(worst) == set(B.LIMITS) == set(B.TWIN_WORST)
    for key, (w, _) in worst.items():
        assert 0.9 * B.TWIN_WORST[key] <= w <= B.TWIN_WORST[key], (key, w)
        assert B.LIMITS[key] == B.limit_from_twin(B.TWIN_WORST[key])


# ------------------------------------------------------------------------------------------------ mutants
def test_every_mutant_is_rejected():
    shape, nlev, radius = (1, 10, 14), 4, 3
    c = B.dvol_case(shape, nlev, radius, "edge", 6, 0, "gauss")
    lim = max(B.LIMITS["dvol.row"], B.LIMITS["dvol.sep"])

    def worst(levels, ref=c["ref"], S=c["S"]):
        return max(B.need(levels[l], ref[l], S[l] * B.U24)[0] for l in range(len(ref)))
    args = (c["pos"], c["fdout"], shape[1:], nlev, radius)
    assert worst(B.scatter(*args)[0]) == 0.0                                                  # (the restatement itself passes)
    assert worst(B.scatter(*args, swap=True)[0]) > lim                                         # i and j swapped in the scatter
    assert worst(B.scatter(*args, level_scale=False)[0]) > lim                                 # the 2^-l dropped
    assert worst(B.scatter(*args, dtype=torch.float32, form="row")[0]) <= B.LIMITS["dvol.row"]
    assert worst(B.scatter(*args, dtype=torch.float32, form="sep")[0]) <= B.LIMITS["dvol.sep"]
    # a one on the last channel of level 1 alone shows the dropped 2^-l (the entry is on the diagonal: a swap does not move it)
    h = B.dvol_case(shape, nlev, radius, "edge", 1, 0, "hot1l")
    hargs = (h["pos"], h["fdout"], shape[1:], nlev, radius)
    assert worst(B.scatter(*hargs, level_scale=False)[0], h["ref"], h["S"]) > lim
    assert worst(B.scatter(*hargs, swap=True)[0], h["ref"], h["S"]) == 0.0
    # dfmap2: 4^-l applied twice; the existence check of level 1 missing (9x17: level 1 is 4x8, row 8 of the plane has no cell)
    L = R.vol_layout(9, 17, 4)
    v = B.d2cat_values((1, 9, 17), 3, L)
    ref, S = B.dfmap2(v, L), B.dfmap2(v, L, absolute=True)
    assert B.need(B.dfmap2(v, L, twice=True), ref, S * B.U24)[0] > B.LIMITS["dfmap2"]
    assert B.need(B.dfmap2(v, L, unchecked=1), ref, S * B.U24)[0] > B.LIMITS["dfmap2"]
    finite = torch.where(torch.isnan(v), torch.ones_like(v), v)                               # (and with readable pads: a value, not a NaN)
    assert B.need(B.dfmap2(finite, L, unchecked=1), ref, S * B.U24)[0] > B.LIMITS["dfmap2"]
    assert B.need(B.dfmap2(v, L, torch.float32), ref, S * B.U24)[0] <= B.LIMITS["dfmap2"]
    # unpool_bwd without the cut (9x11: column 10 and row 8 have no level-1 cell); f2cat with 2^-l for 4^-l
    g = B.unpool_values((3, 9, 11), 4)
    ref, S = B.unpool_bwd(g), B.unpool_bwd(g, absolute=True)
    uncut = g[0].double() + sum(0.25 ** l * g[l].double()[:, (torch.arange(9) >> l).clamp(max=g[l].shape[1] - 1)][:, :, (torch.arange(11) >> l).clamp(max=g[l].shape[2] - 1)]
                                for l in range(1, 4))
    assert B.need(uncut, ref, S * B.U24)[0] > B.LIMITS["unpool"]
    f2 = B.f2_values((1, 9, 17), 3)
    ref, S = B.f2cat(f2, 4), B.f2cat(f2.abs(), 4)
    wrong = [lv * (2.0 ** l) for l, lv in enumerate(ref)]
    assert B.need(wrong[1], ref[1], S[1] * B.U24)[0] > max(B.LIMITS["f2cat.block"], B.LIMITS["f2cat.rec"])
    # a record whose lo half is dropped does not pass the split's limit
    x = torch.randn(4096, generator=D._gen("split"))
    assert B.split_error(x) <= B.LIMITS["split"]
    hi = x.bfloat16().float()
    assert B.need(hi, x.double(), x.double().abs() * B.SPLIT_UNIT)[0] > B.LIMITS["split"]


# ------------------------------------------------------------------------------------------------ sentinels
def test_far_rows_and_zero_gradients_give_exact_zeros():
    for radius in R.RADII:
        c = B.dvol_case((2, 16, 24), 4, radius, "edge", 6, 0, "gauss")
        for l in range(4):
            far = c["ref"][l].view(2, 16, 24, -1)[:, 0]
            assert bool((far == 0).all()) and bool((c["S"][l].view(2, 16, 24, -1)[:, 0] == 0).all())
            assert bool((c["ref"][l] != 0).any())
        for form in ("row", "sep"):
            tw, _ = B.scatter(c["pos"], c["fdout"], (16, 24), 4, radius, torch.float32, form, scale=False)
            assert all(bool((tw[l].view(2, 16, 24, -1)[:, 0] == 0).all()) for l in range(4))
    z = B.dvol_case((1, 10, 14), 4, 4, "edge", 1, 1, "zero")
    assert all(bool((lv == 0).all()) for lv in z["ref"]) and all(bool((s == 0).all()) for s in z["S"])
    assert PATTERN == 0x7FC0FFEE


def test_record_bound_counts_the_split_of_every_launch():
    """The accumulating launch on records, as an fp32 twin: 16 lookups -> records -> hi + lo -> + the 17th -> records.  A bound that
    charges both splits to the final value fails (found on MI355X at 2x16x24 radius 4, near, level 1: 1.32; 1x8x8 with 3 levels:
    1.15 -- where the 17th lookup cancels most of the sum the first split was taken of); record_bound(earlier=...) holds."""
    worst_new, old_fails = 0.0, []
    for case in B.dvol_cases():
        if not case[9]:
            continue
        shape, nlev, radius, family, n = case[:5]
        c = B.dvol_case(*case)
        for form in ("row", "sep"):
            tw, _ = B.scatter(c["pos"][:n], c["fdout"][:n], shape[1:], nlev, radius, torch.float32, form, scale=False)
            tw, _ = B.scatter(c["pos"][n:], c["fdout"][n:], shape[1:], nlev, radius, torch.float32, "row",
                              old=[B.through_records(t) for t in tw], scale=False)
            for l in range(nlev):
                got, ref, S = B.through_records(tw[l]).double(), c["ref17"][l], c["S17"][l]
                worst_new = max(worst_new, B.need(got, ref, B.record_bound("dvol.row", ref, S, [c["ref"][l]]))[0])
                b = B.LIMITS["dvol.row"] * B.U24 * S
                if B.need(got, ref, b + 2 * B.LIMITS["split"] * B.SPLIT_UNIT * (ref.abs() + b))[0] > 1:
                    old_fails.append((shape, nlev, radius))
    print(f"records twin of 16 + 1 lookups: {worst_new:.3f} of record_bound; the one-value bound fails at {sorted(set(old_fails))}")
    assert worst_new <= 1.0
    assert ((2, 16, 24), 4, 4) in old_fails and ((1, 8, 8), 3, 4) in old_fails


# ------------------------------------------------------------------------------------------------ k-tile marks
def _marks_brute(pos, L, radius, exact):
    """ktile_marks with loops: per query and rectangle, every cell of every tile row's run, one by one."""
    Q = pos[0].shape[0]
    rec, tile = torch.zeros(Q, L["P"] // 32, dtype=torch.bool), torch.zeros(Q, (L["P"] + 255) // 256, dtype=torch.bool)
    for q in range(Q):
        for l in range(L["nlev"]):
            o = [(int(a[q]), int(b[q])) for a, b in (B.level_query(p, l, radius)[:2] for p in pos)]
            groups = [[w] for w in o] if l < exact else [o]
            for g in groups:
                x0, x1 = max(min(w[0] for w in g), 0), min(max(w[0] for w in g) + 2 * radius + 1, L["w"][l] - 1)
                y0, y1 = max(min(w[1] for w in g), 0), min(max(w[1] for w in g) + 2 * radius + 1, L["h"][l] - 1)
                if x0 > x1 or y0 > y1:
                    continue
                for ty in range(y0 // 4, y1 // 4 + 1):
                    for tx in range(x0 // 4, x1 // 4 + 1):
                        for cell in range(16):
                            c = L["off"][l] + (ty * L["tw"][l] + tx) * 16 + cell
                            rec[q, c // 32] = True
                            tile[q, c // 256] = True
    return rec, tile


def test_ktile_marks_cover_the_gradient_and_the_short_rectangle_does_not():
    shape, nlev = (2, 16, 24), 4
    L = R.vol_layout(16, 24, nlev)
    for radius in R.RADII:
        for family, n, add_grid in B.KT_RUNS:
            c = B.dvol_case(shape, nlev, radius, family, n, add_grid, "gauss")
            nz = (R.to_tiled([x.float() for x in c["ref"]], L).view(768, -1, 32) != 0).any(2)       # records with a non-zero cell
            marks = [B.ktile_marks(c["pos"][:n], L, radius, e) for e in (0, 1, 2)]
            for rec, tile in marks:
                assert not bool((nz & ~rec).any()), (family, radius)
                assert not bool((nz & ~tile.repeat_interleave(8, 1)[:, :nz.shape[1]]).any())
            for (r0, t0), (r1, t1) in zip(marks, marks[1:]):                                      # exact marks less, never more
                assert not bool((r1 & ~r0).any()) and not bool((t1 & ~t0).any())
            if family == "near":        # the named case: a rectangle one cell short on the high side misses records of the last column
                short, _ = B.ktile_marks(c["pos"][:n], L, radius, 0, short=True)
                assert int((nz & ~short).sum()) > 300
    # ... and the LISTS tell it apart where a tile of 128 queries does not reach everything anyway: 2x32x48 with a small flow (at
    # 16x24 and below the union over a tile marks every record with either rectangle)
    L2 = R.vol_layout(32, 48, 4)
    pos = [B._flat(p)[:1536] for p in B.positions((2, 32, 48), 4, "local", 7)]
    a, b = B.ktile_lists(*B.ktile_marks(pos, L2, 4)), B.ktile_lists(*B.ktile_marks(pos, L2, 4, short=True))
    assert a["nt"] != b["nt"] and a["tn"] != b["tn"] and not torch.equal(a["wmask"], b["wmask"])
    assert all(len(x) < L2["P"] // 32 for x in a["nt"])
    # the vectorised marks = the loops, a shape with pads and B > 1, and a chunk = the rows of the whole
    shape, nlev = (3, 5, 9), 2
    L = R.vol_layout(5, 9, nlev)
    pos = [B._flat(p) for p in B.positions(shape, 3, "edge", 6)]
    for e in (0, 1, 2):
        a, b = B.ktile_marks(pos, L, 3, e), _marks_brute(pos, L, 3, e)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    sl = [p[50:81] for p in pos]
    assert torch.equal(B.ktile_marks(sl, L, 3)[0], B.ktile_marks(pos, L, 3)[0][50:81])


def test_ktile_lists_from_marks():
    """Words, lists and the record mask from hand-made marks: 130 queries (two 128-query tiles, five 32-query blocks), 40 records,
    five cell tiles."""
    rec, tile = torch.zeros(130, 40, dtype=torch.bool), torch.zeros(130, 5, dtype=torch.bool)
    rec[0, 3] = rec[127, 39] = rec[129, 0] = True
    tile[33, 4] = tile[129, 0] = True
    k = B.ktile_lists(rec, tile)
    assert k["nt"] == [[3, 39], [0]]
    assert k["tn"] == [[4], [], [], [], [1]]
    assert k["tn_bits"].tolist() == [[0], [16], [0], [0], [1]]
    w = k["wmask"]
    assert w.shape == (5, 2)
    bits = k["wbits"]
    assert bits[1].nonzero().view(-1).tolist() == [3, 32, 33, 34, 35, 36, 37, 38, 39]           # tile 4 = records 32..39
    assert bits[4].nonzero().view(-1).tolist() == [0, 1, 2, 3, 4, 5, 6, 7]
    assert w[1].tolist() == [8, 0xFF] and w[4].tolist() == [0xFF, 0]
