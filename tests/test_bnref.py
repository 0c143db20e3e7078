"""tests/_bnref.py on the CPU: the float64 restatement of the training-mode BatchNorm kernels against torch's batch_norm and
autograd in float64, and -- over the case lists tests/test_bn_train_kernels.py runs on the GPU -- that the comparator accepts the
fp32 twin under the committed limits, that the limits are what the twin's worst values give, that every mutant exceeds 4 x its
limit on some case, that at most 1 % of any case's elements are ambiguous, and that the lists hold every route edge."""
import functools

import pytest
import torch
import torch.nn.functional as F

import _bnref as N
import _normref as R

ALL = N.CASES + N.S2D_CASES


@functools.lru_cache(maxsize=None)
def _inputs(B, C, H, W):
    return N.designed(B, C, H, W), N.gradients(B, C, H, W), N.residual(B, C, H, W)


def _twin_needs(B, C, H, W):
    """{limit key: worst need of the fp32 twin over the variants of one case}, and the worst ambiguous share."""
    x, g, res0 = _inputs(B, C, H, W)
    w, b, rm, rv, cb0 = N.params(B, C)
    worst, share = {}, 0.0
    for relu, with_res, cbias, mom in N.VARIANTS:
        res, cb = (res0 if with_res else None), (cb0 if cbias else None)
        f = N.bn_twin(x, w, b, cb, rm, rv, mom, N.EPS, relu, res)
        dx, dres, dw, db = N.bn_bwd_twin(g, x, f, relu, f["y"] if with_res else None)
        exp = N.bn_expect(x, g, w, b, cb, rm, rv, mom, N.EPS, relu, res, f["y"] if with_res else None)
        got = dict(f, dx=dx, dweight=dw, dbias=db)
        for name in ("y", "mean", "rstd", "scale", "shift", "rm", "rv", "dx", "dweight", "dbias"):
            ref, scale, slack, key = exp[name]
            worst[key] = max(worst.get(key, 0.0), N.need(got[name].reshape(ref.shape), ref, scale, slack)[0])
        share = max(share, N.ambiguous_share(exp))
    return worst, share


# ---------------------------------------------------------------------------------------------------------------- restatement
@pytest.mark.parametrize("relu,with_res,cbias,mom", N.VARIANTS)
def test_restatement_equals_torch_batch_norm_and_autograd(relu, with_res, cbias, mom):
    """F.batch_norm(x + cbias, training=True) in float64: y, dx, dweight, dbias, running_mean, running_var within 1e-11 of each
    quantity's scale (fp64 rounding of sums of at most a few thousand terms)."""
    B, C, H, W = 3, 7, 5, 6
    x, g, res = _inputs(B, C, H, W)
    x = torch.where((R.plane_kinds(B, C) == 3).view(B, C, 1, 1), res + 3.7, x)     # (no constant plane: its mask is rounding)
    w, b, rm, rv, cb = N.params(B, C)
    xd, rd = x.double().requires_grad_(True), res.double().requires_grad_(True)
    wd, bd = w.double().requires_grad_(True), b.double().requires_grad_(True)
    cd = cb.double().requires_grad_(True)
    trm, trv = rm.double().clone(), rv.double().clone()
    y = F.batch_norm(xd + cd.view(1, C, 1, 1) if cbias else xd, trm, trv, wd, bd, training=True, momentum=mom, eps=N.EPS)
    y = torch.relu(y) if relu else y
    y = torch.relu(rd + y) if with_res else y
    y.backward(g.double())
    f = N.bn_ref(x, w, b, cb if cbias else None, rm, rv, mom, N.EPS, relu, res if with_res else None)
    dx, dres, dw, db = N.bn_bwd_ref(g, x, w, b, N.EPS, relu, res if with_res else None)

    def close(a, ref):
        assert (a - ref).abs().max().item() <= 1e-11 * max(ref.abs().max().item(), 1e-30)
    close(f["y"], y.detach()), close(dx, xd.grad), close(dw, wd.grad), close(db, bd.grad), close(f["rm"], trm), close(f["rv"], trv)
    if cbias:
        assert cd.grad.abs().max().item() <= 1e-11 * xd.grad.abs().sum().item()     # the convolution bias: exactly zero
    assert (dres is None and not with_res) or torch.equal(dres, rd.grad)


# ------------------------------------------------------------------------------------------------------------ twin and limits
@pytest.mark.parametrize("case", ALL, ids=lambda c: "x".join(map(str, c)))
def test_twin_within_limits_and_ambiguity(case):
    """The share is computed from the float64 reference alone (bn_expect): designed() planes stay under the 1 % cap."""
    B, H, W, C = case
    worst, share = _twin_needs(B, C, H, W)
    for k, v in worst.items():
        assert v <= N.LIMITS[k], (k, v, N.LIMITS[k])
    assert share <= 0.01, share


def test_limits_are_four_times_the_twins_worst():
    got = {}
    for (B, H, W, C) in ALL:
        for k, v in _twin_needs(B, C, H, W)[0].items():
            if v > got.get(k, (-1.0, None))[0]:
                got[k] = (v, (B, H, W, C))
    for k, (v, case) in got.items():
        assert N.LIMITS[k] == N.limit_from_twin(v), (k, v, case, N.LIMITS[k])
        assert abs(v - N.TWIN_WORST[k]) <= 0.06 * max(v, 0.1), (k, v, case)
    assert set(got) == set(N.LIMITS)


# --------------------------------------------------------------------------------------------------------------------- mutants
MUTANT_CASES = tuple(c for c in ALL if c not in N.LONG)
MUTANTS = ("biased", "no_cbias", "momentum_swapped", "per_sample", "div_hw", "mask_xhat", "dres_inner", "last_strip", "parity")


def _mutant_worst(mut):
    """The worst need / limit a mutant reaches over the cases, on the outputs it touches."""
    best = 0.0
    for (B, H, W, C) in MUTANT_CASES:
        x, g, res0 = _inputs(B, C, H, W)
        w, b, rm, rv, cb0 = N.params(B, C)
        sp = N.strip(B, H * W)
        for relu, with_res, cbias, mom in N.VARIANTS:
            res, cb = (res0 if with_res else None), (cb0 if cbias else None)
            if (mut == "dres_inner" and not (with_res and relu)) or (mut == "mask_xhat" and not relu) or (mut == "no_cbias" and not cbias):
                continue
            exp = N.bn_expect(x, g, w, b, cb, rm, rv, mom, N.EPS, relu, res)
            if mut == "parity":
                if (B, H, W, C) not in N.S2D_CASES:
                    continue
                ref, scale, slack, key = exp["y"]
                got = R.from_s2d(R.to_s2d(ref), B, H, W, C, mut)
                best = max(best, N.need(got, ref, scale, slack)[0] / N.LIMITS[key])
                continue
            f = N.bn_ref(x, w, b, cb, rm, rv, mom, N.EPS, relu, res, mut, sp)
            dx, dres, dw, db = N.bn_bwd_ref(g, x, w, b, N.EPS, relu, res, None, mut, sp)
            got = dict(y=f["y"], rm=f["rm"], rv=f["rv"], dx=dx, dweight=dw, dbias=db)
            if mut != "per_sample":
                got.update(mean=f["mean"], rstd=f["rstd"], scale=f["scale"], shift=f["shift"])
            for name, t in got.items():
                ref, sc, slack, key = exp[name]
                best = max(best, N.need(t.reshape(ref.shape), ref, sc, slack)[0] / N.LIMITS[key])
            if with_res:
                gate = g.double() * (exp["y"][0] > 0)
                best = max(best, float("inf") if not torch.equal(dres, gate) else 0.0)
    return best


@pytest.mark.parametrize("mut", MUTANTS)
def test_every_mutant_exceeds_four_times_its_limit(mut):
    assert _mutant_worst(mut) > 4.0, mut


def test_unmutated_reference_is_inside_its_own_limits():
    assert _mutant_worst("") == 0.0


# -------------------------------------------------------------------------------------------------------------------- coverage
def test_case_lists_cover_every_route_edge():
    assert [c[3] for c in N.GEOMETRY] == [4, 12, 96, 100, 252, 256] and all(c[:3] == (2, 13, 10) for c in N.GEOMETRY)
    assert [256 - (256 // (C // 4)) * (C // 4) for C in (4, 12, 96, 100, 252, 256)] == [0, 1, 16, 6, 4, 0]        # idle tail threads
    assert [c[0] * c[1] * c[2] for c in N.SMALL] == [2, 2]
    assert all(N.strip(c[0], c[1] * c[2]) == 128 for c in N.CASES[:-1] + N.S2D_CASES)
    assert N.strip(1, 520 * 512) == 192 and (520 * 512) % 192 != 0
    assert [c[1] * c[2] for c in N.STRIPS] == [127, 128, 129]
    assert N.workgroups(3, 41 * 25) == 27 and N.workgroups(2, 1030) == 18 and N.workgroups(5, 63) == 5
    # more workgroups than partial rows (the row index wraps): by one, several times over, and by a number that is no multiple
    assert N.workgroups(5, 41 * 40) == 65 == N.BN_ROWS + 1 and N.workgroups(4, 92 * 124) == 360 and N.workgroups(1, 520 * 512) == 1387
    assert N.strip(8, 184 * 248) == 192 and N.strip(64, 1 << 20) == 2048                                        # above the floor, the cap
    assert {(c[1], c[2]) for c in N.S2D_CASES} == {(2, 2), (4, 6), (26, 10)} and {c[3] for c in N.S2D_CASES} == {4, 64, 100}
    assert {(r, s, c) for r, s, c, _ in N.VARIANTS} == {(r, s, c) for r in (0, 1) for s in (False, True) for c in (False, True)}
    assert {m for *_, m in N.VARIANTS} == set(N.MOMENTA)
    w, b, *_ = N.params(2, 64)
    assert bool((w < 0).any()) and bool((w > 0).any()) and bool((b != 0).all())
    # a channel constant over the whole batch needs the `constant` kind in every sample: C a multiple of 7
    x = N.designed(2, 252, 13, 10)
    const = (x == x[:1, :, :1, :1]).all(3).all(2).all(0)
    assert int(const.sum()) == 36
