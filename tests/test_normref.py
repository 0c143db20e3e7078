"""tests/_normref.py on the CPU: the float64 restatements against torch and autograd, s2d_index against a reshape / permute
space-to-depth, and -- over the case lists tests/test_norm_kernels.py runs on the GPU -- that the comparator accepts the fp32 twins
under the committed limits, that the limits are what the twins' worst values give, that every mutant exceeds 4 x its limit on
some case, that at most 1 % of any case's elements are ambiguous, and that the lists hold every route edge."""
import functools
import itertools

import pytest
import torch
import torch.nn.functional as F

import _normref as R

VARIANTS = tuple(itertools.product((0, 1), (False, True)))          # (relu, with residual)
CL_ALL = R.CL_CASES + R.CL_PPW + R.S2D_CASES
D53 = 2.0 ** -53


def _nchw_shape(case):
    B, C, HW = case
    return (B, C) + R.NCHW_HW[HW]


@functools.lru_cache(maxsize=None)
def _inputs(B, C, H, W):
    return R.designed(B, C, H, W), R.gradients(B, C, H, W), R.residual(B, C, H, W)


def _twin_needs(B, C, H, W, route, variants):
    """{limit key: worst need of the fp32 twins over the variants of one case}, and the worst ambiguous share."""
    x, g, res0 = _inputs(B, C, H, W)
    worst, share = {}, 0.0

    def put(exp, got):
        for name, t in got.items():
            if name not in exp:
                continue
            ref, scale, slack, key = exp[name]
            worst[key] = max(worst.get(key, 0.0), R.need(t, ref, scale, slack)[0])
    for relu, with_res in variants:
        res = res0 if with_res else None
        y, mean, rstd = R.inorm_twin(x, R.EPS, relu, res, route)
        dx, dres, s1, s2 = R.inorm_bwd_twin(g, x, mean, rstd, relu, y if with_res else None)
        exp = R.inorm_expect(x, g, R.EPS, relu, res, route, y if with_res else None)
        put(exp, dict(y=y, mean=mean, rstd=rstd, dx=dx, s1=s1, s2=s2, sums=x.sum((2, 3), keepdim=True),
                      sumsq=(x * x).sum((2, 3), keepdim=True)))
        share = max(share, R.ambiguous_share(exp))
        for cbias in (False, True):
            par = R.bn_params(B, C, cbias)
            fold = R.fold_twin(*par, R.EPS)
            put(R.fold_expect(*par, R.EPS), dict(zip(("scale", "shift", "rs", "rmc"), fold)))
            scale, shift, rs, rmc = fold
            y = R.affine_twin(x, scale, shift, relu, res)
            dx, dres, sg, sgx = R.affine_bwd_twin(g, x, scale, shift, relu, y if with_res else None)
            exp = R.affine_expect(x, g, scale, shift, relu, res, y if with_res else None)
            put(exp, dict(y=y, dx=dx, dsum_g=sg, dsum_gx=sgx))
            share = max(share, R.ambiguous_share(exp))
            # the partial rows the channels-last backward would leave: the sums split over B * 8 rows
            part = torch.stack([sg, sgx]).view(2, 1, C) * torch.linspace(-1.0, 2.0, B * 8).view(1, -1, 1)
            put(R.fold_bwd_expect(part, rs, rmc, scale), dict(zip(("dweight", "dbias", "dcbias"), R.fold_bwd_twin(part, rs, rmc, scale))))
    return worst, share


def twin_worst():
    """{limit key: (worst, case)} of the twins over every case list."""
    out = {}
    todo = [((B, C, H, W), "cl", VARIANTS) for (B, H, W, C) in CL_ALL]
    todo += [(_nchw_shape(c), "nchw", ((0, False), (1, False))) for c in R.NCHW_CASES]
    for shape, route, variants in todo:
        worst, _ = _twin_needs(*shape, route, variants)
        for k, v in worst.items():
            if v > out.get(k, (-1.0, None))[0]:
                out[k] = (v, shape)
    return out


# ------------------------------------------------------------------------------------------------------------ restatements
@pytest.mark.parametrize("relu,with_res", VARIANTS)
def test_instance_norm_restatement_equals_torch_and_autograd(relu, with_res):
    B, C, H, W = 2, 7, 5, 6
    x, g, res = _inputs(B, C, H, W)
    # (no constant plane here: torch's float64 mean of equal numbers is not that number either, and with relu the sign of its
    #  rounding decides the whole plane's mask -- see _normref on ambiguity)
    x = torch.where((R.plane_kinds(B, C) == 3).view(B, C, 1, 1), res, x)
    xd = x.double().requires_grad_(True)
    rd = res.double().requires_grad_(True)
    y = F.instance_norm(xd, eps=R.EPS)
    y = torch.relu(y) if relu else y
    y = torch.relu(rd + y) if with_res else y
    y.backward(g.double())
    yr, mean, rstd = R.inorm_ref(x, R.EPS, relu, res if with_res else None)
    dx, dres = R.inorm_bwd_ref(g, x, R.EPS, relu, res if with_res else None)
    big = float(rstd.max())
    assert (yr - y.detach()).abs().max().item() <= 64 * D53 * big * 40
    assert (dx - xd.grad).abs().max().item() <= 4096 * D53 * big * big * 40
    if with_res:
        assert torch.equal(dres, rd.grad)
    else:
        assert dres is None
    assert torch.equal(mean.reshape(B, C), x.double().mean((2, 3)))


@pytest.mark.parametrize("relu,with_res,cbias", [v + (c,) for v in VARIANTS for c in (False, True)])
def test_affine_and_fold_restatements_equal_torch_and_autograd(relu, with_res, cbias):
    B, C, H, W = 2, 7, 5, 6
    x, g, res = _inputs(B, C, H, W)
    w, b, rm, rv, cb = R.bn_params(B, C, cbias)
    if cbias:       # torch evaluates (x + cbias) alpha - rm alpha with an fma: +-1e-17 where this restatement (and fp32) has an exact 0
        x = torch.where(x == 0, res, x)
    xd = x.double().requires_grad_(True)
    rd = res.double().requires_grad_(True)
    wd, bd = w.double().requires_grad_(True), b.double().requires_grad_(True)
    cd = cb.double().requires_grad_(True) if cbias else None
    xin = xd + cd.view(1, C, 1, 1) if cbias else xd
    y = F.batch_norm(xin, rm.double(), rv.double(), wd, bd, training=False, eps=R.EPS)
    y = torch.relu(y) if relu else y
    y = torch.relu(rd + y) if with_res else y
    y.backward(g.double())
    scale, shift, rs, rmc = R.fold_ref(w, b, rm, rv, cb, R.EPS)
    yr = R.affine_ref(x, scale, shift, relu, res if with_res else None)
    dx, dres, sg, sgx = R.affine_bwd_ref(g, x, scale, shift, relu, res if with_res else None)
    tol = 4096 * D53 * 200
    assert (yr - y.detach()).abs().max().item() <= tol
    assert (dx - xd.grad).abs().max().item() <= tol
    assert (dres is None and not with_res) or torch.equal(dres, rd.grad)
    part = torch.stack([sg, sgx]).view(2, 1, C) * torch.tensor([0.25, 0.75], dtype=torch.float64).view(1, 2, 1)
    dw, db, dcb = R.fold_bwd_ref(part, rs, rmc, scale)
    assert (dw - wd.grad).abs().max().item() <= tol * H * W and (db - bd.grad).abs().max().item() <= tol * H * W
    if cbias:
        assert (dcb - cd.grad).abs().max().item() <= tol * H * W


@pytest.mark.parametrize("H,W", ((2, 2), (4, 6), (6, 4)))
def test_s2d_index_equals_reshape_permute(H, W):
    B, C = 2, 3
    x = torch.arange(B * H * W * C, dtype=torch.float32).view(B, H, W, C)
    s2d = x.view(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).contiguous().view(B, H // 2, W // 2, 4 * C)
    idx = R.s2d_index(B, H, W, C)
    assert sorted(idx.reshape(-1).tolist()) == list(range(B * H * W * C))
    assert torch.equal(s2d.reshape(-1)[idx], x)
    nchw = x.permute(0, 3, 1, 2)
    assert torch.equal(R.to_s2d(nchw), s2d.reshape(-1)) and torch.equal(R.from_s2d(s2d.reshape(-1), B, H, W, C), nchw)
    assert not torch.equal(R.from_s2d(s2d.reshape(-1), B, H, W, C, mut="parity"), nchw)
    assert torch.equal(R.from_cl(R.to_cl(nchw), B, H, W, C), nchw)


# ------------------------------------------------------------------------------------------------------------ twins and limits
@pytest.mark.parametrize("case", CL_ALL, ids=lambda c: "x".join(map(str, c)))
def test_channels_last_twins_within_limits_and_ambiguity(case):
    B, H, W, C = case
    worst, share = _twin_needs(B, C, H, W, "cl", VARIANTS)
    for k, v in worst.items():
        assert v <= R.LIMITS[k], (k, v, R.LIMITS[k])
    assert share <= 0.01, share


@pytest.mark.parametrize("case", R.NCHW_CASES, ids=lambda c: "x".join(map(str, c)))
def test_nchw_twins_within_limits_and_ambiguity(case):
    worst, share = _twin_needs(*_nchw_shape(case), "nchw", ((0, False), (1, False)))
    for k, v in worst.items():
        assert v <= R.LIMITS[k], (k, v, R.LIMITS[k])
    assert share <= 0.01, share


def test_second_trip_twin_within_limits():
    """The 33000 x 256 affine forward: the twin against float64 on every eighth sample row (the kernel test compares all)."""
    B, H, W, C = R.SECOND_TRIP
    x, _, res = _inputs(B, C, 8, W)
    par = R.bn_params(B, C, True)
    scale, shift, _, _ = R.fold_twin(*par, R.EPS)
    exp = R.affine_expect(x, torch.zeros_like(x), scale, shift, 1, res)
    ref, sc, slack, key = exp["y"]
    assert R.need(R.affine_twin(x, scale, shift, 1, res), ref, sc, slack)[0] <= R.LIMITS[key]


def test_limits_are_four_times_the_twins_worst():
    """LIMITS = limit_from_twin(worst value of the twin over the lists); TWIN_WORST records those values to two digits."""
    got = twin_worst()
    for k, (v, case) in got.items():
        if k == "aff_dx":
            assert v <= 1.0, (v, case)               # one fp32 product: fixed
            continue
        assert R.LIMITS[k] == R.limit_from_twin(v), (k, v, case, R.LIMITS[k])
        assert abs(v - R.TWIN_WORST[k]) <= 0.06 * max(v, 0.1), (k, v, case)
    assert set(got) == set(R.LIMITS)


# --------------------------------------------------------------------------------------------------------------------- mutants
MUTANT_CASES = tuple((B, C, H, W) for (B, H, W, C) in R.CL_CASES + R.S2D_CASES)


def _mutant_worst(mut):
    """The worst need / limit a mutant reaches over the cases, on the outputs it touches."""
    best = 0.0
    for B, C, H, W in MUTANT_CASES:
        x, g, res0 = _inputs(B, C, H, W)
        ppw = R.pix_per_wg(B, H * W)
        for relu, with_res in VARIANTS:
            res = res0 if with_res else None
            if mut in ("no_out_mask", "dres_early") and not with_res or mut == "lt" and not relu:
                continue
            if mut == "parity":
                if (B, H, W, C) not in R.S2D_CASES:
                    continue
                exp = R.inorm_expect(x, g, R.EPS, relu, res, "cl")
                ref, scale, slack, key = exp["y"]
                got = R.from_s2d(R.to_s2d(ref), B, H, W, C, mut)
                best = max(best, R.need(got, ref, scale, slack)[0] / R.LIMITS[key])
                continue
            if mut == "cbias_plus":
                par = R.bn_params(B, C, True)
                exp = R.fold_expect(*par, R.EPS)
                _, shift, _, rmc = R.fold_ref(*par, R.EPS, mut)
                for name, t in (("shift", shift), ("rmc", rmc)):
                    ref, scale, slack, key = exp[name]
                    best = max(best, R.need(t, ref, scale, slack)[0] / R.LIMITS[key])
                continue
            exp = R.inorm_expect(x, g, R.EPS, relu, res, "cl")
            y, mean, rstd = R.inorm_ref(x, R.EPS, relu, res, mut, ppw)
            dx, dres, s1, s2 = R.inorm_bwd_ref(g, x, R.EPS, relu, res, None, mut, ppw, parts=True)
            got = dict(y=y, mean=mean, rstd=rstd, dx=dx, s1=s1, s2=s2)
            if mut not in ("hw-1", "no_eps", "no_m1"):
                par = R.bn_params(B, C, True)
                scale, shift, _, _ = R.fold_twin(*par, R.EPS)
                aexp = R.affine_expect(x, g, scale, shift, relu, res)
                adx, adres, sg, sgx = R.affine_bwd_ref(g, x, scale, shift, relu, res, None, mut, ppw)
                for name, t in (("dx", adx), ("dsum_g", sg), ("dsum_gx", sgx)):
                    ref, sc, slack, key = aexp[name]
                    best = max(best, R.need(t, ref, sc, slack)[0] / R.LIMITS[key])
                if with_res:
                    gate = g.double() * (aexp["y"][0] > 0)
                    best = max(best, float("inf") if not torch.equal(adres, gate) else 0.0)
            for name, t in got.items():
                ref, sc, slack, key = exp[name]
                best = max(best, R.need(t, ref, sc, slack)[0] / R.LIMITS[key])
            if with_res:
                gate = g.double() * (exp["y"][0] > 0)
                best = max(best, float("inf") if not torch.equal(dres, gate) else 0.0)
    return best


MUTANTS = ("strip_last", "row0", "hw-1", "no_eps", "lt", "no_out_mask", "dres_early", "parity", "no_m1", "cbias_plus")


@pytest.mark.parametrize("mut", MUTANTS)
def test_every_mutant_exceeds_four_times_its_limit(mut):
    assert _mutant_worst(mut) > 4.0, mut


def test_unmutated_references_are_inside_their_own_limits():
    assert _mutant_worst("") == 0.0


# ------------------------------------------------------------------------------------------------------------------ coverage
def test_case_lists_cover_every_route_edge():
    rt = {c: R.cl_route(c[0], c[1] * c[2], c[3]) for c in R.CL_CASES + R.S2D_CASES}
    at130 = {c[3]: rt[c] for c in R.CL_GEOMETRY}
    assert all(c[1] * c[2] == 130 for c in R.CL_GEOMETRY) and set(at130) == {4, 12, 96, 100, 252, 256}
    assert at130[4]["lanes_p"] == 256 and at130[12]["lanes_p"] == 85 and at130[256]["lanes_p"] == 4
    assert at130[12]["idle"] == 1 and at130[100]["idle"] == 6 and at130[252]["idle"] == 4 and at130[96]["idle"] == 16
    assert at130[4]["idle"] == 0 and at130[256]["idle"] == 0
    # C = 4: one pixel per thread; fewer pixels than lanes, exactly as many, one more
    assert {c[1] * c[2] for c in R.CL_C4} == {1, 3, 255, 256, 257} and all(c[3] == 4 for c in R.CL_C4)
    # strips of 128 pixels: one short, exact, one over; nine workgroups (the slot index wraps); a remainder of the unroll by four
    hw = {c[1] * c[2]: rt[c] for c in R.CL_STRIPS}
    assert all(v["ppw"] == 128 and v["lanes_p"] == 16 for v in hw.values())
    assert [hw[n]["wgs"] for n in (127, 128, 129)] == [1, 1, 2]
    assert hw[1025]["wgs"] == 9 > R.CL_NSLOT and hw[1030]["wgs"] == 9
    assert ((1030 - 8 * 128) + 15) // 16 % 4 != 0                          # steps of the last strip: not a multiple of the unroll
    # PIX_PER_WG above its floor needs the tuning hook at these sizes; the workload's first stage gets there by itself
    (B1, H1, W1, C1), (B2, H2, W2, C2) = R.CL_PPW
    assert all(R.cl_route(B, H * W, C)["ppw"] == 128 for (B, H, W, C) in R.CL_PPW)
    r1, r2 = R.cl_route(B1, H1 * W1, C1, R.CL_PPW_TARGET), R.cl_route(B2, H2 * W2, C2, R.CL_PPW_TARGET)
    assert r1["ppw"] == 192 and r1["wgs"] == 22
    assert r2["ppw"] == 1024 and r2["wgs"] == 65 and (H2 * W2) % 1024 != 0 and (B2 * H2 * W2 + 63) // 64 > 1024
    assert R.pix_per_wg(1, 6 * 368 * 496 // 4 * 4) > 128
    # s2d: every (H, W) at every C, more than one workgroup, W / 2 odd, H / 2 odd
    assert {(c[1], c[2]) for c in R.S2D_CASES} == {(2, 2), (4, 6), (26, 10), (42, 50)} and {c[3] for c in R.S2D_CASES} == {4, 64, 100}
    assert all(c[1] % 2 == 0 and c[2] % 2 == 0 for c in R.S2D_CASES) and rt[(2, 42, 50, 64)]["wgs"] == 17
    # the affine forward's grid is capped at 8192 blocks: a second trip
    B, H, W, C = R.SECOND_TRIP
    r = R.cl_route(B, H * W, C)
    assert B * H * W == 33000 and r["affine_blocks"] == 8192 and r["affine_trips"] == 2 and H % 2 == 0 and W % 2 == 0
    assert all(R.cl_route(c[0], c[1] * c[2], c[3])["affine_trips"] == 1 for c in CL_ALL)
    # NCHW: below one float4, the scalar tail, one and several strides of 256 float4, C that does not divide 256
    assert {c[2] for c in R.NCHW_CASES} == {1, 2, 3, 63, 256, 1028, 46000, 640}
    assert all(c[0] * c[1] == 6 for c in R.NCHW_CASES if c[2] != 640) and (2, 5, 640) in R.NCHW_CASES and 256 % 5
    assert all(h * w == hw for hw, (h, w) in R.NCHW_HW.items()) and R.NCHW_HW[46000] == (184, 250)
    assert 1028 // 4 > 256 and 46000 // 4 > 256 and 63 % 4 and 640 % 4 == 0
    # every kind of plane is in every case with at least seven planes (C = 4 with B = 2: 8)
    for (B, H, W, C) in CL_ALL:
        if B * C >= len(R.KINDS):
            assert set(R.plane_kinds(B, C).reshape(-1).tolist()) == set(range(len(R.KINDS)))


def test_designed_planes_are_what_they_say():
    B, C, H, W = 2, 7, 26, 10
    x = R.designed(B, C, H, W).double()
    par = R.bn_params(B, C, True)
    scale, shift, _, _ = R.fold_twin(*par, R.EPS)
    m, s = x.mean((2, 3)), x.std((2, 3), unbiased=False)
    k = R.plane_kinds(B, C)
    assert ((m / s)[k == 1] - 4).abs().max() < 0.5 and ((m / s)[k == 2] - 32).abs().max() < 4
    assert (s[k == 3] == 0).all() and (x[k == 3] == float(torch.tensor(3.7))).all()
    assert ((s[k == 4] / 3e-3) - 1).abs().max() < 0.2 and (x[k == 5].amax((1, 2)) == 1e3).all()
    zero = (x == 0) & (k == 6).view(B, C, 1, 1)
    assert zero.sum().item() == 2 * H * W // 10 and (shift[(k == 6).any(0)] == 0).all()
    t = R.affine_twin(x, scale, shift, 0)
    assert (t[zero] == 0).all()
