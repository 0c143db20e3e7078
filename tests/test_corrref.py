"""tests/_corrref.py -- the float64 restatements of the correlation volume, its pyramids and the lookup that the GPU tests of
csrc/corr_build.hip, corr_tiled.hip and corr_lookup.hip compare against -- checked on the CPU: against the reference's own outputs
(tests/golden/corr_{tiny,odd,mid}.npz: pyr0..3 and out), against torch's avg_pool2d / grid_sample in float64, against a brute-force
'SAME' pool; the layout helpers against the documented cell formula; LIMITS against the fp32 twins over the GPU tests' cases; and
every mutant (a wrong restatement) against the limits.

The golden comparison.  The reference forms the volume with an fp32 matmul over C channels and pools in fp32: |error| <= (C + 2) u S0
for the dot product and its scaling, 3 u more per pooled level -- limit (C + 16) u S, rigorous.  Its lookup reaches grid_sample through
2 x / (w - 1) - 1 and back, which moves a position by a few ulp of w - 1 (< 5e-6 cells here) and so a value by that times a tap
difference, and blends in fp32: limit 2e-5 of the largest |V_l| of the query's level.  Measured: printed by the tests.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _corrref as R
import _dcoordsref as D
from _util import PATTERN, load
from oracle.weights import rand_tensor

_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)      # noqa: E731


# ------------------------------------------------------------------------------------------------ against the reference's outputs
@pytest.mark.parametrize("name", ["corr_tiny", "corr_odd", "corr_mid"])
def test_restatement_matches_the_reference_outputs(name):
    g = load(name)
    B, C, H, W, r, seed = (int(g[k]) for k in ("B", "C", "H", "W", "radius", "seed"))
    f1, f2 = rand_tensor((B, C, H, W), seed), rand_tensor((B, C, H, W), seed + 1)       # (as tests/test_gpu_parity.py)
    ref, S = R.build(f1, f2, 4), R.build_scale(f1, f2, 4)
    for l in range(4):
        got = torch.from_numpy(g[f"pyr{l}"])[:, 0]
        assert got.shape == ref[l].shape
        w, i = R.need(got, ref[l], S[l] * R.U24)
        print(f"{name} pyr{l}: {w:.2f} u S (limit {C + 16})")
        assert w <= C + 16, (l, w, i)
    out, _ = R.lookup(ref, torch.from_numpy(g["coords"]), r)
    got = torch.from_numpy(g["out"]).permute(0, 2, 3, 1)
    n2 = (2 * r + 1) ** 2
    vmax = torch.cat([lv.abs().amax((1, 2)).view(B, H, W, 1).expand(B, H, W, n2) for lv in ref], 3)
    w, i = R.need(got, out, vmax)
    print(f"{name} out: {w:.2e} of max|V_l| (limit 2e-5)")
    assert w <= 2e-5, (w, i)


@pytest.mark.parametrize("shape,nlev", [((1, 10, 14), 4), ((3, 5, 9), 2)], ids=_ids)
def test_restatement_matches_torch_in_float64(shape, nlev):
    """avg_pool2d(2, 2) level by level and grid_sample(align_corners=True, zeros) at pos / 2^l + offsets, both in float64."""
    B, H, W = shape
    f1, f2 = R.fmaps(shape, 18, "gauss")
    levels = R.build(f1, f2, nlev)
    a = R.volume0(f1, f2).unsqueeze(1)
    for l in range(nlev):
        assert a.shape[2:] == levels[l].shape[1:]
        assert float((a[:, 0] - levels[l]).abs().max()) <= 1e-14 * float(levels[l].abs().max())
        if l + 1 < nlev:
            a = F.avg_pool2d(a, 2, stride=2)
    for radius in R.RADII:
        pos = D.coords_values(B, H, W, "mixed")
        out, _ = R.lookup(levels, pos, radius)
        n = 2 * radius + 1
        d = torch.arange(-radius, radius + 1, dtype=torch.float64)
        dx, dy = d.view(n, 1).expand(n, n), d.view(1, n).expand(n, n)                 # the x offset is the slow index
        xy = pos.permute(0, 2, 3, 1).reshape(B * H * W, 1, 1, 2).double()
        near = (pos.abs() < 1e5).all(1).reshape(-1)                                    # (grid_sample has no far clamp: skip that row)
        for l, lv in enumerate(levels):
            h, w = lv.shape[1:]
            gx, gy = xy[..., 0] / 2 ** l + dx, xy[..., 1] / 2 ** l + dy
            grid = torch.stack([2 * gx / max(w - 1, 1) - 1, 2 * gy / max(h - 1, 1) - 1], -1)
            if h == 1 or w == 1:
                continue        # (the normalisation divides by w - 1: a one-cell axis has no grid_sample counterpart)
            ts = F.grid_sample(lv.unsqueeze(1), grid, mode="bilinear", padding_mode="zeros", align_corners=True).reshape(B * H * W, n * n)
            mine = out.reshape(B * H * W, -1)[:, l * n * n:(l + 1) * n * n]
            err = float((ts - mine)[near].abs().max())
            print(f"{shape} r{radius} level {l}: {err:.2e}")
            assert err <= 1e-12 * float(lv.abs().max())


@pytest.mark.parametrize("shape,nlev", R.POOL_SAME_CASES + [((2, 5, 7), 3)], ids=_ids)
def test_pool_same_matches_a_brute_force_loop(shape, nlev):
    x = R.pool_input(shape)
    got = R.pool_same(x, nlev)
    rows, h, w = shape
    for l in range(1, nlev):
        k = 1 << l
        h2, w2 = -(-h // k), -(-w // k)
        py, px = (h2 * k - h) // 2, (w2 * k - w) // 2
        assert got[l].shape == (rows, h2, w2)
        for y in range(h2):
            for xx in range(w2):
                win = x[:, max(y * k - py, 0):min(y * k - py + k, h), max(xx * k - px, 0):min(xx * k - px + k, w)].double()
                assert win.numel() > 0
                assert float((win.mean((1, 2)) - got[l][:, y, xx]).abs().max()) <= 1e-15 * k * k
    if h % (1 << (nlev - 1)) == 0 and w % (1 << (nlev - 1)) == 0:        # sizes that divide: the floor pyramid
        for a, b in zip(got, R.pool_floor(x, nlev)):
            assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-15


# ------------------------------------------------------------------------------------------------ layout
def _all_layout_shapes():
    s = {(sh[1], sh[2], n) for sh, n in R.BUILD_SHAPES + R.TILED_SHAPES}
    return sorted(s)


def test_layout_restatement_and_round_trip():
    for H, W, nlev in _all_layout_shapes():
        L = R.vol_layout(H, W, nlev)
        assert L is not None and L["P"] % 32 == 0
        levels = [torch.randn(3, H >> l, W >> l, generator=D._gen("rt", H, W, l)) for l in range(nlev)]
        assert [tuple(lv.shape[1:]) for lv in levels] == list(zip(L["h"], L["w"]))[:nlev]
        vol = R.to_tiled(levels, L, PATTERN)
        back = R.from_tiled(vol, L)
        assert all(torch.equal(a, b) for a, b in zip(levels, back))
        # the documented formula, cell by cell; everything else holds the pattern
        seen = torch.zeros(L["P"], dtype=torch.bool)
        for l, lv in enumerate(levels):
            assert L["off"][l] == sum(L["th"][k] * L["tw"][k] * 16 for k in range(l))
            for y in range(lv.shape[1]):
                for x in range(lv.shape[2]):
                    i = L["off"][l] + ((y >> 2) * L["tw"][l] + (x >> 2)) * 16 + (y & 3) * 4 + (x & 3)
                    assert i == R.cell_index(L, l, y, x) and not seen[i]
                    seen[i] = True
                    assert torch.equal(vol[:, i], lv[:, y, x])
        assert torch.equal(seen, R.cell_mask(L))
        assert bool((vol[:, ~seen].view(torch.int32) == PATTERN).all())
        assert D.tiled_layout(H, W, nlev) == (L["P"], L["off"][:nlev], L["th"][:nlev], L["tw"][:nlev])
    assert R.vol_layout(4, 4, 4) is None and R.vol_layout(8, 8, 5) is None and R.vol_layout(0, 8, 1) is None


def test_layout_restatement_equals_the_library():
    """fsraft_vol_layout is host code: no GPU needed."""
    import ctypes
    from flow_supervisor_amd import _lib
    lib = _lib.load()
    for H, W, nlev in _all_layout_shapes() + [(4, 4, 4), (8, 8, 5)]:
        out = (ctypes.c_int * 24)()
        rc = lib.fsraft_vol_layout(H, W, nlev, out)
        L = R.vol_layout(H, W, nlev)
        assert (rc == 0) == (L is not None)
        if L is not None:
            assert R.layout_from_ints(out) == L


def test_entry_points_refuse_bad_arguments_before_touching_the_gpu():
    """Argument validation is host code: FS_ERR_ARG (1) without a HIP call, so this runs without a GPU (the pointers are never
    dereferenced).  The pool entries check every level before their first launch."""
    import ctypes
    from flow_supervisor_amd import _lib
    lib = _lib.load()
    p, off, null = ctypes.c_void_p(4096), ctypes.c_void_p(4100), ctypes.c_void_p(None)
    keep = (ctypes.c_void_p * 4)(4096, 4096, 4096, 4096)
    hole = (ctypes.c_void_p * 4)(4096, 4096, None, 4096)
    pp, pph = ctypes.cast(keep, _lib._PP), ctypes.cast(hole, _lib._PP)
    s = (128, 64, 1)
    for C, shape in ((3, (8, 8)), (0, (8, 8)), (32, (4, 4))):                                    # (4x4 has no fourth level)
        assert lib.fsraft_corr_build(p, p, pp, 4, 1, C, *shape, None) == 1
        assert lib.fsraft_corr_build_tiled(p, p, p, 4, 1, C, *shape, None) == 1
    for C, shape in ((48, (8, 8)), (0, (8, 8)), (32, (4, 4))):
        assert lib.fsraft_corr_build_rec(p, p, p, 4, 1, C, *shape, None) == 1
    assert lib.fsraft_corr_build(p, p, pph, 4, 1, 32, 8, 8, None) == 1
    assert lib.fsraft_corr_build_tiled(p, p, off, 4, 1, 32, 8, 8, None) == 1
    assert lib.fsraft_corr_build_rec(p, p, off, 4, 1, 32, 8, 8, None) == 1
    assert lib.fsraft_corr_pool_pyramid(pph, 4, 64, 8, 8, None) == 1
    assert lib.fsraft_corr_pool_pyramid(pp, 4, 64, 4, 4, None) == 1
    assert lib.fsraft_corr_pool_pyramid_same(pph, 4, 64, 8, 8, None) == 1
    for radius, nlev, vol, shape in ((2, 4, p, (8, 8)), (5, 4, p, (8, 8)), (4, 4, off, (8, 8)), (4, 4, null, (8, 8)), (4, 4, p, (4, 4))):
        assert lib.fsraft_corr_lookup_tiled_fwd(vol, nlev, p, *s, p, 1, *shape, radius, 0, None) == 1
    for entry in (lib.fsraft_corr_lookup_fwd, lib.fsraft_corr_lookup_fwd_same):
        for radius, nlev, lv in ((2, 4, pp), (5, 4, pp), (4, 3, pp), (4, 4, pph), (4, 4, ctypes.cast(null, _lib._PP))):
            assert entry(lv, nlev, p, *s, p, 1, 1, 8, 8, radius, None) == 1
    assert lib.fsraft_corr_lookup_fwd(pp, 4, p, *s, p, 1, 1, 4, 4, 4, None) == 1


# ------------------------------------------------------------------------------------------------ limits
def test_limits_come_from_the_twins():
    """LIMITS = 4 x the worst the fp32 twins reach over every case of the kernel tests, rounded up to one digit."""
    worst = R.twins_worst()
    for key, (w, case) in sorted(worst.items()):
        print(f"{key}: twins' worst {w:.4f} (limit {R.LIMITS[key]:g}) at {case}")
    assert set(worst) == set(R.LIMITS) == set(R.TWIN_WORST)
    for key, (w, _) in worst.items():
        assert 0.9 * R.TWIN_WORST[key] <= w <= R.TWIN_WORST[key], (key, w)
        assert R.LIMITS[key] == R.limit_from_twin(R.TWIN_WORST[key])


# ------------------------------------------------------------------------------------------------ mutants
def _worst_lookup(mutant, key="lookup.weights"):
    """Worst figure of mutant(levels, pos, radius) against the restatement over the gaussian / onehot cases of two shapes."""
    worst = 0.0
    for shape, nlev in (R.TILED_SHAPES[0], R.TILED_SHAPES[5]):
        for vkind in R.VOL_KINDS:
            c = R.lookup_case(shape, nlev, 3, "mixed", False, vkind)
            worst = max(worst, R.need(mutant(c["levels"], c["pos"], 3), c["ref"], c["S"] * R.U24)[0])
    return worst


def test_every_mutant_is_rejected():
    lim = max(R.LIMITS["lookup.lerp"], R.LIMITS["lookup.weights"])
    assert _worst_lookup(lambda lv, p, r: R.lookup(lv, p, r)[0]) == 0.0                              # (the restatement itself passes)
    assert _worst_lookup(lambda lv, p, r: R.lookup(lv, p, r, swap=True)[0]) > lim                    # i and j swapped
    assert _worst_lookup(lambda lv, p, r: R.lookup(lv, p, r, level_scale=False)[0]) > lim            # the 2^-l scale dropped

    # pad cells read as stored instead of as zero
    def pads_as_stored(levels, pos, r):
        B, _, H, W = pos.shape
        L = R.vol_layout(H, W, len(levels))
        return R.lookup(R.from_tiled(R.to_tiled(levels, L, PATTERN), L, pads=True), pos, r)[0]
    assert _worst_lookup(pads_as_stored) > lim

    shape, nlev = (1, 9, 17), 4
    c = R.build_case(shape, nlev, 18, "gauss")
    f1, f2 = c["f1"], c["f2"]

    def worst_levels(levels, key):
        assert [lv.shape for lv in levels] == [lv.shape for lv in c["ref"]]
        return max(R.need(lv, c["ref"][l], c["S"][l] * R.UNIT[key])[0] for l, lv in enumerate(levels))
    assert worst_levels(R.build(f1, f2, nlev), "build.exact") == 0.0
    assert worst_levels(R.build(f1, f2, nlev, scale=False), "build.exact") > R.LIMITS["build.exact"]             # 1 / sqrt(C) dropped
    assert worst_levels(R.pool_floor(R.volume0(f1, f2), nlev, pitch_bug=True), "build.exact") > R.LIMITS["build.exact"]   # wrong pitch
    # ceil instead of floor level sizes: another shape, and another lookup where the shapes are forced to agree
    ceil = R.pool_ceil_mutant(R.volume0(f1, f2), nlev)
    assert [lv.shape for lv in ceil] != [lv.shape for lv in c["ref"]]
    pos = D.coords_values(*shape, "mixed")
    out, S = R.lookup(c["ref"], pos, 4)
    assert R.need(R.lookup(ceil, pos, 4)[0], out, S * R.U24)[0] > lim
    # bf16x1 (the lo terms dropped) must not pass the split limit; bf16x3 does
    pooled = lambda a: R.pool_floor(R.build0_twin(f1, f2, a), nlev, torch.float32)      # noqa: E731
    assert worst_levels(pooled("bf16x1"), "build.split") > R.LIMITS["build.split"]
    assert worst_levels(pooled("bf16x3"), "build.split") <= R.LIMITS["build.split"]


# ------------------------------------------------------------------------------------------------ sentinels
def test_far_rows_and_zero_inputs_give_exact_zeros():
    for shape, nlev in R.TILED_SHAPES[:2]:
        for add_grid in (False, True):
            c = R.lookup_case(shape, nlev, 4, "mixed", add_grid, "gauss")
            assert bool((c["ref"][:, 0] == 0).all()) and bool((c["S"][:, 0] == 0).all())           # the +-1e6 row
            assert bool((c["ref"][:, 1:] != 0).any())
            for form in ("lerp", "weights"):
                assert bool((R.lookup(c["levels"], c["pos"], 4, torch.float32, form)[0][:, 0] == 0).all())
    c = R.build_case((1, 9, 17), 4, 14, "zero")
    assert all(bool((lv == 0).all()) for lv in c["ref"]) and all(bool((lv == 0).all()) for lv in c["S"])
    zero = [torch.zeros_like(lv) for lv in R.level_values((1, 10, 14), 4, "gauss")]
    out, S = R.lookup(zero, D.coords_values(1, 10, 14, "mixed"), 3)
    assert bool((out == 0).all()) and bool((S == 0).all())


def test_the_cases_reach_what_they_are_meant_to():
    """Query counts around the workgroups, level sizes off the tiles, a last level of 1x1."""
    q = sorted(s[0] * s[1] * s[2] for s, _ in R.BUILD_SHAPES)
    assert {1, 255, 256, 257} <= set(q)
    assert R.vol_layout(10, 14, 4)["h"] == [10, 5, 2, 1] and R.vol_layout(10, 14, 4)["w"] == [14, 7, 3, 1]
    assert R.vol_layout(8, 8, 4)["h"][3] == 1 and R.vol_layout(3, 5, 2)["w"][1] == 2
    assert sorted(s[0] * s[1] * s[2] for s, _ in R.ROW_SHAPES) == [80, 81, 140, 256, 768]
    assert len(list(R.build_cases(False))) == 80 and len(list(R.build_cases(True))) == 70
    x = np.prod(R.POOL_CASES[2][0]) // 4
    assert 65536 * 256 < x <= 65536 * 256 + 4096                          # one short trip past the cap
