"""tests/_altcorrref.py -- the float64 restatements the GPU tests of csrc/altcorr.hip compare against -- checked on the CPU: the
forward restatement against F.grid_sample on the formed volume; the explicit weights-onto-positions backward against torch.autograd;
LIMITS against the fp32 twins over the GPU tests' cases; the mutants, each beyond the limit on the cases meant to catch it; the
conditions the coordinate families must meet, proved with the geometry model; the C-ABI signatures and the entries' argument
checks, which are host code.
"""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

import _altcorrref as A
import _altdcoordsref as AD
import _corrref as K
import _dcoordsref as D
from _util import G

PLANE, PLEV = A.PLANE
SIZES = D.level_sizes(PLANE[1], PLANE[2], PLEV)


def _level(t, l, radius):
    n2 = (2 * radius + 1) ** 2
    return t[..., l * n2:(l + 1) * n2]


# ---------------------------------------------------------------------------------------------------------------- the restatements
@pytest.mark.parametrize("radius", A.RADII)
def test_forward_restatement_matches_grid_sample_on_the_formed_volume(radius):
    """float64, align_corners=True, zero padding; positions across and beyond the plane, odd multiples of 1/64 -- at no level an
    integer, so no tap has the weight 0 that the rounding of grid_sample's normalisation would turn into 1e-16 -- and a +-1e6 row."""
    shape, nlev, C = (1, 10, 14), 3, 36
    B, H, W = shape
    f1, f2, vol, avol = A.maps(shape, nlev, C)
    gen = D._gen("grid_sample", radius)
    pos = torch.stack([(2 * torch.randint(-6 * 32, (W + 6) * 32, (B, H, W), generator=gen) + 1).float() / 64,
                       (2 * torch.randint(-6 * 32, (H + 6) * 32, (B, H, W), generator=gen) + 1).float() / 64], 1)
    pos[:, 0, 0], pos[:, 1, 0] = 1e6, -1e6
    c = dict(pos=pos, ref=K.lookup(vol, pos, radius)[0], S=K.lookup(avol, pos, radius)[0])
    r, n = radius, 2 * radius + 1
    off = torch.arange(-r, r + 1, dtype=torch.float64)
    xy = c["pos"].double().permute(0, 2, 3, 1).reshape(-1, 2)
    outs = []
    for l, v in enumerate(vol):
        h, w = v.shape[1:]
        px = xy[:, 0].view(-1, 1, 1) / (1 << l) + off.view(1, n, 1)            # [Q, i (x offset), j]
        py = xy[:, 1].view(-1, 1, 1) / (1 << l) + off.view(1, 1, n)
        grid = torch.stack([2 * px.expand(-1, n, n) / (w - 1) - 1, 2 * py.expand(-1, n, n) / (h - 1) - 1], -1)
        outs.append(F.grid_sample(v.unsqueeze(1), grid, mode="bilinear", padding_mode="zeros", align_corners=True).reshape(-1, n * n))
    got = torch.cat(outs, 1).view(B, H, W, -1)
    w, i = D.need(got, c["ref"], c["S"])
    print(f"radius {radius}: restatement vs grid_sample {w:.2e} S")
    assert w <= 1e-9, (w, i)
    assert bool((c["ref"][:, 0] == 0).all()) and bool((c["S"][:, 0] == 0).all())     # the +-1e6 row


@pytest.mark.parametrize("shape,C,N,half", [((1, 10, 14), 36, 3, False), ((3, 5, 9), 65, 3, True), ((1, 8, 8), 4, 1, False)])
@pytest.mark.parametrize("radius", A.RADII)
def test_explicit_backward_matches_autograd(shape, C, N, half, radius):
    for family in D.COORD_KINDS:
        c = A.dropin_case(shape, C, N, half, family)
        for gk in A.GRAD_KINDS:
            g = A.grad_values(shape, N, radius, gk)
            g1, g2, S1, S2 = A.dropin_bwd(c["f1"], c["f2"], c["coords"], g, radius)
            for order in ("seq", "pair"):
                e1, e2 = A.dropin_bwd_explicit(c["f1"], c["f2"], c["coords"], g, radius, order=order)
                w1, w2 = D.need(e1, g1, S1)[0], D.need(e2, g2, S2)[0]
                assert w1 <= 1e-12 and w2 <= 1e-12, (family, gk, order, w1, w2)
            if gk == "zero":
                assert bool((g1 == 0).all()) and bool((g2 == 0).all())
            if family == "mixed":
                assert bool((g1[:, 0] == 0).all()) and bool((S1[:, 0] == 0).all())      # the +-1e6 row of every set
            assert bool((S1 >= g1.abs() * (1 - 1e-12)).all()) and bool((S2 >= g2.abs() * (1 - 1e-12)).all())


def test_dropin_forward_is_the_fused_lookup_of_one_unscaled_level():
    shape, C, radius = (1, 10, 14), 36, 4
    c = A.dropin_case(shape, C, 1, False, "mixed")
    ref, S = A.dropin_expect(c["f1"], c["f2"], c["coords"], radius)
    fused, Sf = A.expect_fused(c["f1"], [c["f2"]], c["coords"][:, 0].permute(0, 3, 1, 2), radius)
    assert D.need(ref[:, 0].permute(0, 2, 3, 1) / C ** 0.5, fused, Sf)[0] <= 1e-12
    assert bool((S >= ref.abs() * (1 - 1e-12)).all())


# ---------------------------------------------------------------------------------------------------------------- the limits
def test_forward_limits_come_from_the_twins():
    worst = A.worst_of_forward_twins()
    print(f"twins' worst: fwd {worst['fwd']:.4f} units of 2^-24 S, mfma {worst['mfma']:.4f} units of 2^-16 S")
    for k in ("fwd", "mfma"):
        assert 0.9 * A.TWIN_WORST[k] <= worst[k] <= A.TWIN_WORST[k], (k, worst[k])
        assert A.LIMITS[k] == D.limit_from_twin(A.TWIN_WORST[k])


def test_backward_limit_comes_from_the_twins():
    worst = A.worst_of_backward_twins()
    print(f"twins' worst: bwd {worst:.4f} units of 2^-24 S1 / S2")
    assert 0.9 * A.TWIN_WORST["bwd"] <= worst <= A.TWIN_WORST["bwd"], worst
    assert A.LIMITS["bwd"] == D.limit_from_twin(A.TWIN_WORST["bwd"])


def test_cases_cover_the_shapes_channels_and_families():
    for route in A.ROUTES:
        g = A.groups(route)
        assert {(s, n) for s, n, _, _ in g} == set(D.SHAPES) | {A.PLANE}
        assert {C for _, _, C, _ in g} == set(A.ROUTE_C[route])
        assert {C for s, n, C, _ in g if (s, n) in AD.SWEEP_SHAPES} == set(A.ROUTE_C[route])
        fams = {f for s, n, _, ff in g if (s, n) == A.PLANE for f in ff}
        assert fams == set(A.PLANE_FAMILIES[route]) and {"smooth", "jump"} <= fams
        if route != "wave":
            assert {C for s, n, C, ff in g if (s, n) == A.PLANE and "jump" in ff} == set(A.ROUTE_C[route])
            assert {f"limit-{route}", f"far-{route}"} <= fams
    d = A.dropin_cases()
    assert {s for s, *_ in d} == set(A.DROPIN_SHAPES) == {s for s, _ in D.SHAPES}
    assert {C for _, C, *_ in d} == set(A.ROUTE_C["wave"])
    assert {(N, half) for _, _, N, half, _, _ in d} == {(1, False), (1, True), (3, False), (3, True)}


# ---------------------------------------------------------------------------------------------------------------- the mutants
def _beyond(got, c, key):
    return D.need(got, c["ref"], c["S"] * A.UNIT[key])[0] > A.LIMITS[key]


@pytest.mark.parametrize("radius", A.RADII)
def test_mutants_of_the_lookup_exceed_the_limit(radius):
    """i / j swapped in the channel order; 2^-l missing; hi hi only on the matrix-pipe route."""
    for shape, nlev, C in (((1, 10, 14), 4, 36), ((3, 5, 9), 2, 100), (PLANE, PLEV, 32)):
        f1, f2, vol, _ = A.maps(shape, nlev, C)
        for add_grid in (False, True):
            c = A.case(shape, nlev, C, radius, "mixed", add_grid)
            assert _beyond(K.lookup(vol, c["pos"], radius, swap=True)[0], c, "fwd")
            assert _beyond(K.lookup(vol, c["pos"], radius, level_scale=False)[0], c, "fwd")
    f1, f2 = A.maps(PLANE, PLEV, 32)[:2]
    x1, x3 = A.dots32(f1, f2, "bf16x1"), A.dots32(f1, f2, "bf16x3")
    for family in ("smooth", "jump"):
        c = A.case(PLANE, PLEV, 32, radius, family, True)
        assert _beyond(A.blend32(x1, c["pos"], radius, 32), c, "mfma")
        assert not _beyond(A.blend32(x3, c["pos"], radius, 32), c, "mfma")


@pytest.mark.parametrize("kernel", ("tile", "mfma"))
@pytest.mark.parametrize("radius", A.RADII)
def test_mutants_of_the_region_exceed_the_limit(kernel, radius):
    """Fallback positions read as 0, on every family that claims fallbacks; a region taken one cell off, on the smooth family (every
    position covered).  The model says which cells of a query's level its tile's region holds."""
    C = A.BASE_C[kernel]
    f1, f2, vol, _ = A.maps(PLANE, PLEV, C)
    key = A.limit_key(kernel)
    for family in ("jump", f"limit-{kernel}", f"far-{kernel}", "mixed"):
        c = A.case(PLANE, PLEV, C, radius, family, False)
        cover = [A.cell_cover(c["pos"], l, radius, SIZES[l], kernel) for l in range(PLEV)]
        got = K.lookup([v * m for v, m in zip(vol, cover)], c["pos"], radius)[0]
        assert _beyond(got, c, key), family
        if family.startswith("limit"):                                  # every level the family claims, on its own
            for l in range(PLEV):
                one = K.lookup([v * m if k == l else v for k, (v, m) in enumerate(zip(vol, cover))], c["pos"], radius)[0]
                assert _beyond(one, c, key), (family, l)
    c = A.case(PLANE, PLEV, C, radius, "smooth", False)
    cover = [A.cell_cover(c["pos"], l, radius, SIZES[l], kernel) for l in range(PLEV)]
    shifted = [torch.where(m, F.pad(v, (0, 1))[:, :, 1:], v) for v, m in zip(vol, cover)]
    assert _beyond(K.lookup(shifted, c["pos"], radius)[0], c, key)


def test_the_clamp_decides_the_route_of_a_tile_not_its_value():
    """Every level is far smaller than 30000 cells, so a finite far position gives 0 with or without the clamp: no value mutant
    exists for it.  What the clamp at 30000 decides is the region of the matrix-pipe kernel -- the level-1 position 60000 / 2 is
    clamped to -30000, becomes the tile's minimum and puts every other query of the tile on the fallback; taken as given it would
    leave them covered -- and the model shows that.  A non-finite position without the clamp is a NaN in the output."""
    radius = 4
    pos = A.plane_positions("smooth", radius)[0].clone()
    pos[0, :, 1, 1] = 60000.0
    tile = A.tile_mask("mfma", 0, PLANE[1], PLANE[2])
    tile[1, 1] = False
    with_clamp = A.states(pos, 1, radius, SIZES[1], "mfma")[0][tile]
    without = A.states(pos, 1, radius, SIZES[1], "mfma", clamp=False)[0][tile]
    assert int((with_clamp == A.COVERED).sum()) == 0 and int((with_clamp == A.FALLBACK).sum()) > 0
    assert int((without == A.FALLBACK).sum()) == 0 and int((without == A.COVERED).sum()) > 0
    f1, f2, vol, avol = A.maps(PLANE, PLEV, 32)
    assert bool((K.lookup(vol, pos, radius)[0][0, 1, 1] == 0).all()) and bool((K.lookup(avol, pos, radius)[0][0, 1, 1] == 0).all())
    c = A.case(PLANE, PLEV, 32, radius, "far-mfma", False)
    unclamped = K.lookup(vol, torch.nan_to_num(c["pos"], nan=0.0, posinf=0.0, neginf=0.0), radius)[0]   # the window at cell 0
    assert _beyond(unclamped, c, "mfma")


@pytest.mark.parametrize("radius", A.RADII)
def test_mutants_of_the_dropin_entry_exceed_the_limit(radius):
    """The output scaled by 1 / sqrt(C); N sets written to set 0."""
    shape, C = (1, 10, 14), 36
    c = A.dropin_case(shape, C, 3, False, "mixed")
    ref, S = A.dropin_expect(c["f1"], c["f2"], c["coords"], radius)
    assert D.need(ref / C ** 0.5, ref, S * A.U24)[0] > A.LIMITS["fwd"]
    set0 = torch.zeros_like(ref)
    set0[:, 0] = ref[:, 2]
    assert D.need(set0, ref, S * A.U24)[0] > A.LIMITS["fwd"]
    g = A.grad_values(shape, 3, radius, "gauss")
    g1, g2, S1, S2 = A.dropin_bwd(c["f1"], c["f2"], c["coords"], g, radius)
    m1, m2, _, _ = A.dropin_bwd(c["f1"], c["f2"], c["coords"][:, :1], g[:, :1], radius)      # a backward that forgets sets 1, 2
    assert D.need(m1, g1, S1 * A.U24)[0] > A.LIMITS["bwd"] and D.need(m2, g2, S2 * A.U24)[0] > A.LIMITS["bwd"]


# ---------------------------------------------------------------------------------------------------------------- the families
def test_every_level_of_every_case_has_elements_inside_and_across_its_edge():
    """Every level of at least 2x2 cells, in every case of every route: elements with all four taps inside, and elements with
    some taps outside."""
    seen = set()
    for route in A.ROUTES:
        for shape, nlev, _, families in A.groups(route):
            for radius in A.RADII:
                for family in families:
                    for add_grid in (False, True):
                        if (shape, nlev, radius, family, add_grid) in seen:
                            continue
                        seen.add((shape, nlev, radius, family, add_grid))
                        pos = A.positions(shape, family, radius, add_grid)[1]
                        for l, (h, w) in enumerate(D.level_sizes(shape[1], shape[2], nlev)):
                            if h < 2 or w < 2:
                                continue
                            inside = A.element_use(pos, l, radius, (h, w), "tile")[0]
                            assert bool((inside == 4).any()) and bool((inside < 4).any()), (shape, nlev, radius, family, add_grid, l)


@pytest.mark.parametrize("kernel", ("tile", "mfma"))
@pytest.mark.parametrize("radius", A.RADII)
def test_the_region_families_reach_both_branches(kernel, radius):
    _, H, W = PLANE
    C = A.BASE_C[kernel]

    def use(family):
        c = A.case(PLANE, PLEV, C, radius, family, False)
        return c, [A.element_use(c["pos"], l, radius, SIZES[l], kernel) for l in range(PLEV)]

    def both_in(u, S, mask):
        """In the queries of `mask`: an element with S > 0 that takes a fallback position, and one that takes a covered one."""
        _, cov, fb = u
        return bool((fb[0][mask] & (S[0][mask] > 0)).any()) and bool((cov[0][mask] & (S[0][mask] > 0)).any())

    c, u = use("smooth")
    for l in range(PLEV):
        assert int((A.states(c["pos"], l, radius, SIZES[l], kernel) == A.FALLBACK).sum()) == 0, ("smooth", l)
        assert bool(u[l][1].any())

    c, u = use("jump")                                                   # claims level 0
    tiles = [A.tile_mask(kernel, t, H, W) for t in range((H // A.TILE[kernel][0]) * (W // A.TILE[kernel][1]))]
    assert any(both_in(u[0], _level(c["S"], 0, radius), m) for m in tiles)

    c, u = use(f"limit-{kernel}")
    meta = A.plane_positions(f"limit-{kernel}", radius)[1]
    assert {(m["level"], m["axis"], m["side"], m["beyond"]) for m in meta if m["kind"] == "limit"} == \
        {(l, a, s, b) for l in (0, 1) for a in (0, 1) for s in ("low", "high") for b in (0, 1)}
    assert {m["level"] for m in meta if m["kind"] == "split"} == {2, 3}
    for m in meta:
        mask, l = A.tile_mask(kernel, m["tile"], H, W), m["level"]
        st = A.states(c["pos"], l, radius, SIZES[l], kernel)[0][mask]
        if m["kind"] == "limit" and not m["beyond"]:
            assert int((st == A.FALLBACK).sum()) == 0 and int((st == A.COVERED).sum()) > 0, m      # the last fully covered offset
        else:
            assert both_in(u[l], _level(c["S"], l, radius), mask), m                                # one cell beyond / split

    c, u = use(f"far-{kernel}")
    meta = A.plane_positions(f"far-{kernel}", radius)[1]
    assert [m["value"] for m in meta][3:] == list(A.FAR_VALUES[3:]) and len(meta) == len(A.FAR_VALUES)
    th, tw = A.TILE[kernel]
    for m in meta:
        mask = A.tile_mask(kernel, m["tile"], H, W)
        ty, tx = divmod(m["tile"], W // tw)
        ay, ax = ty * th + A.ANCHOR[kernel][0], tx * tw + A.ANCHOR[kernel][1]
        assert bool((c["ref"][0, ay, ax] == 0).all()) and bool((c["S"][0, ay, ax] == 0).all())    # the far query: exactly 0
        others = mask.clone()
        others[ay, ax] = False
        # the tile kernel anchors at query 0 whatever it holds; the matrix-pipe kernel at the minimum, which a far query is at the
        # levels that clamp it to -30000 (level 0 for all but 29999.984375, which stays a large positive position)
        levels = range(PLEV) if kernel == "tile" else ([0] if m["value"] != 29999.984375 else [])
        for l in levels:
            st = A.states(c["pos"], l, radius, SIZES[l], kernel)[0][others]
            assert int((st == A.COVERED).sum()) == 0 and int((st == A.FALLBACK).sum()) > 0, (m, l)
            _, _, fb = u[l]
            assert bool((fb[0][others] & (_level(c["S"], l, radius)[0][others] > 0)).any()), (m, l)
    rest = ~torch.stack([A.tile_mask(kernel, m["tile"], H, W) for m in meta]).any(0)
    for l in range(PLEV):
        assert bool((u[l][1][0][rest] & (_level(c["S"], l, radius)[0][rest] > 0)).any())         # covered positions elsewhere


def test_add_grid_hands_over_exactly_the_positions():
    for family in ("jump", "limit-tile", "far-mfma"):
        given, pos = A.positions(PLANE, family, 4, True)
        back = given + D.grid(*PLANE)
        assert bool(((back == pos) | (back.isnan() & pos.isnan())).all())
        assert bool((pos * 64 == (pos * 64).round())[pos.isfinite()].all())


# ---------------------------------------------------------------------------------------------------------------- the C entries
ENTRIES = {"fsraft_altcorr_fwd": 13, "fsraft_altcorr_bwd": 15, "fsraft_altcorr_fused_fwd": 15, "fsraft_altcorr_mfma_fwd": 17}


def test_entry_points_are_exported_with_their_signatures():
    from flow_supervisor_amd import _lib
    txt = open(os.path.join(os.path.dirname(G), "..", "include", "fsraft.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in ENTRIES.items():
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == nargs, name
        assert hasattr(lib, name) and f"int {name}(" in txt, name
    assert "fsraft_set_alt_tile" in _lib.SIGNATURES and hasattr(lib, "fsraft_set_alt_tile")      # (a test switch: not in the header)


def test_entry_points_refuse_bad_arguments_before_touching_the_gpu():
    """Argument validation is host code: FS_ERR_ARG (1) without a HIP call, so this runs without a GPU (the pointers are never
    dereferenced).  The backward's size check is among them."""
    from flow_supervisor_amd import _lib
    lib = _lib.load()
    p, null, odd = ctypes.c_void_p(4096), ctypes.c_void_p(None), ctypes.c_void_p(4100)
    keep = (ctypes.c_void_p * 4)(4096, 4096, 4096, 4096)
    bad = (ctypes.c_void_p * 4)(4096, 4100, 4096, 4096)
    holed = (ctypes.c_void_p * 4)(4096, 4096, None, 4096)
    pp, pbad, pholed = (ctypes.cast(k, _lib._PP) for k in (keep, bad, holed))
    s = (128, 64, 1)

    def fwd(f1=p, f2=p, co=p, out=p, dims=(1, 1, 8, 8, 8, 8), C=32, radius=4):
        return lib.fsraft_altcorr_fwd(f1, f2, co, out, *dims, C, radius, None)

    def bwd(f1=p, f2=p, co=p, g=p, g1=p, g2=p, dims=(1, 1, 8, 8, 8, 8), C=32, radius=4):
        return lib.fsraft_altcorr_bwd(f1, f2, co, g, g1, g2, *dims, C, radius, None)

    def fused(f1=p, lv=pp, nlev=4, co=p, out=p, shape=(1, 8, 8), C=32, radius=4):
        return lib.fsraft_altcorr_fused_fwd(f1, lv, nlev, co, *s, 0, out, *shape, C, radius, None)

    def mfma(f1r=p, lr=pp, f1=p, lv=pp, nlev=4, co=p, out=p, shape=(1, 8, 8), C=32, radius=4):
        return lib.fsraft_altcorr_mfma_fwd(f1r, lr, f1, lv, nlev, co, *s, 0, out, *shape, C, radius, None)

    sizes = [dict(dims=d) for d in ((0, 1, 8, 8, 8, 8), (1, 0, 8, 8, 8, 8), (1, 1, 0, 8, 8, 8), (1, 1, 8, 0, 8, 8), (1, 1, 8, 8, 0, 8),
                                    (1, 1, 8, 8, 8, 0), (1, 1, -1, 8, 8, 8))]
    common = [dict(radius=2), dict(radius=5), dict(C=0), dict(C=257), dict(f1=null), dict(co=null)]
    for kw in common + sizes + [dict(f2=null), dict(out=null)]:
        assert fwd(**kw) == 1, kw
    for kw in common + sizes + [dict(f2=null), dict(g=null), dict(g1=null), dict(g2=null)]:
        assert bwd(**kw) == 1, kw
    levels = [dict(nlev=0), dict(nlev=5), dict(shape=(1, 5, 7)),                 # 5x7 has no fourth level
              dict(lv=pholed), dict(lv=ctypes.cast(null, _lib._PP)), dict(out=null), dict(shape=(0, 8, 8)), dict(shape=(1, 0, 8))]
    for kw in common + levels:
        assert fused(**kw) == 1, kw
    for kw in common + levels + [dict(C=48), dict(C=288), dict(C=16), dict(f1r=null), dict(f1r=odd), dict(f1=odd), dict(lr=pbad),
                                 dict(lv=pbad), dict(lr=pholed), dict(lr=ctypes.cast(null, _lib._PP))]:
        assert mfma(**kw) == 1, kw
