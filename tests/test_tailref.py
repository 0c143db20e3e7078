"""tests/_tailref.py on the CPU: every float64 restatement against an independent route (autograd through F.unfold + softmax +
pixel shuffle, F.interpolate(align_corners=True), torch.optim.AdamW + clip_grad_norm_ on float64 parameters, autograd through the
loss as pytorch/train.py writes it, the upsample.npz and sequence_loss.npz outputs of the reference's own functions), and -- over
the case lists tests/test_tail_kernels.py runs on the GPU -- that the fp32 twins pass the committed limits, that the limits are
what the twins' worst values give, that every mutant exceeds 4 x its limit on some case, and the input conditions on thresholds."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _tailref as R
from _util import load

D53 = 2.0 ** -53


def _rand(shape, seed, scale=1.0):
    """(the seeded inputs tests/golden/make_golden.py drew)"""
    return torch.from_numpy((np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32))


def _mutant_rule(mut, devs):
    """devs: the deviation / limit a mutant reaches on every case of its list.  It exceeds 4 on some case, and on every case it
    either exceeds 4 or is nil (the mutation does not reach that case: float64 noise, below 1e-6) -- no limit is more than a
    quarter of the smallest deviation an applicable mutant produces."""
    assert max(devs) > 4.0, (mut, max(devs))
    assert all(d > 4.0 or d < 1e-6 for d in devs), (mut, sorted(d for d in devs if 1e-6 <= d <= 4.0))


def _ids(c):
    return "x".join(map(str, c)) if isinstance(c, tuple) else str(c)


# ============================================================================================================ convex upsampler
def _unfold_route(flow, mask_nhwc):
    """pytorch/core/raft.py:72-83 in float64."""
    N, _, H, W = flow.shape
    mask = mask_nhwc.permute(0, 3, 1, 2).reshape(N, 1, 9, 8, 8, H, W)
    mask = torch.softmax(mask, dim=2)
    up = F.unfold(8 * flow, [3, 3], padding=1).view(N, 2, 9, 1, 1, H, W)
    up = torch.sum(mask * up, dim=2).permute(0, 1, 4, 2, 5, 3)
    return up.reshape(N, 2, 8 * H, 8 * W)


@functools.lru_cache(maxsize=None)
def _up_inputs(case, kind):
    return R.flow_values(*case), R.mask_plane(kind, *case), R.dup_values(*case)


@pytest.mark.parametrize("kind", R.UP_MASKS)
@pytest.mark.parametrize("case", R.UP_CASES, ids=_ids)
def test_upsampler_restatement_equals_autograd_through_unfold(case, kind):
    flow, mask, dup = _up_inputs(case, kind)
    fd, md = flow.double().requires_grad_(True), mask.double().requires_grad_(True)
    up = _unfold_route(fd, md)
    (up * dup.double()).sum().backward()
    dmask, dflow = R.upsample_bwd_ref(flow, mask, dup)
    big = 8 * float(flow.abs().max()) * max(1.0, float(dup.abs().max()))
    assert (R.upsample_ref(flow, mask) - up.detach()).abs().max().item() <= 64 * D53 * big
    assert (dmask - md.grad).abs().max().item() <= 64 * D53 * big
    assert (dflow - fd.grad).abs().max().item() <= 64 * 64 * D53 * big
    assert flow.reshape(-1).unique().numel() == flow.numel() and bool((flow != 0).all())


def test_upsampler_restatement_equals_the_reference_outputs():
    g = load("upsample")
    N, H, W = int(g["N"]), int(g["H"]), int(g["W"])
    flow, mask = _rand((N, 2, H, W), 401, 2.0), _rand((N, 576, H, W), 402, 1.5)
    nhwc = mask.permute(0, 2, 3, 1).contiguous()
    dup = _rand((N, 2, 8 * H, 8 * W), 403)
    dmask, dflow = R.upsample_bwd_ref(flow, nhwc, dup)
    for got, name in ((R.upsample_ref(flow, nhwc), "up"), (dflow, "dflow"), (dmask.permute(0, 3, 1, 2), "dmask")):
        ref = torch.from_numpy(g[name]).double()
        assert (got - ref).abs().max().item() <= 1e-5 * ref.abs().max().item(), name


def _up_needs(case, kind, mut=None):
    """{limit key: need of the twin (mut None) or of a mutant against the float64 restatement}."""
    flow, mask, dup = _up_inputs(case, kind)
    exp = R.upsample_expect(flow, mask, dup)
    if mut is None:
        dm, df = R.upsample_bwd_twin(flow, mask, dup)
        got = dict(up=R.upsample_twin(flow, mask), dmask=dm, dflow=df)
    else:
        dm, df = R.upsample_bwd_ref(flow, mask, dup, mut)
        got = dict(up=R.upsample_ref(flow, mask, mut), dmask=dm, dflow=df)
    return {key: R.need(got[name], ref, scale, slack)[0] for name, (ref, scale, slack, key) in exp.items()}


@pytest.mark.parametrize("kind", R.UP_MASKS)
@pytest.mark.parametrize("case", R.UP_CASES, ids=_ids)
def test_upsampler_twin_within_limits(case, kind):
    for k, v in _up_needs(case, kind).items():
        assert v <= R.LIMITS[k], (k, v)


UP_MUTANTS = ("kswap", "sswap", "clamp", "nomax", "gather_plus")


@pytest.mark.parametrize("mut", UP_MUTANTS)
def test_upsampler_mutants_exceed_four_times_the_limit(mut):
    kinds = ("offset",) if mut == "nomax" else R.UP_MASKS
    _mutant_rule(mut, [max(v / R.LIMITS[k] for k, v in _up_needs(case, kind, mut).items()) for case in R.UP_CASES for kind in kinds])


# ================================================================================================================== bilinear x8
@pytest.mark.parametrize("case", R.UPFLOW_CASES, ids=_ids)
def test_upflow8_restatement_equals_interpolate(case):
    N, C, H, W = case
    flow, dup = R.upflow8_inputs(*case)
    fd = flow.double().requires_grad_(True)
    up = 8 * F.interpolate(fd, size=(8 * H, 8 * W), mode="bilinear", align_corners=True)
    up.backward(dup.double())
    assert (R.upflow8_ref(flow) - up.detach()).abs().max().item() <= 1e-12 * 8 * float(flow.abs().max())
    assert (R.upflow8_bwd_ref(dup) - fd.grad).abs().max().item() <= 1e-11 * 8 * float(dup.abs().max()) * 64


def test_upflow8_restatement_equals_the_reference_output():
    h = load("helpers")
    ref = torch.from_numpy(h["upflow8"]).double()
    assert (R.upflow8_ref(_rand((2, 2, 5, 7), 411, 2.0)) - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()


def _upflow_needs(case, mut=None):
    flow, dup = R.upflow8_inputs(*case)
    exp = R.upflow8_expect(flow, dup)
    got = dict(up=R.upflow8_twin(flow), dflow=R.upflow8_bwd_twin(dup)) if mut is None else \
        dict(up=R.upflow8_ref(flow, mut), dflow=R.upflow8_bwd_ref(dup, mut))
    return {key: R.need(got[name], ref, scale, slack)[0] for name, (ref, scale, slack, key) in exp.items()}


@pytest.mark.parametrize("case", R.UPFLOW_CASES, ids=_ids)
def test_upflow8_twin_within_limits(case):
    for k, v in _upflow_needs(case).items():
        assert v <= R.LIMITS[k], (k, v)


@pytest.mark.parametrize("mut", ("half", "one_is_zero"))
def test_upflow8_mutants_exceed_four_times_the_limit(mut):
    for key in ("upflow8", "upflow8_bwd"):
        _mutant_rule(mut, [_upflow_needs(case, mut)[key] / R.LIMITS[key] for case in R.UPFLOW_CASES])
    if mut == "one_is_zero":                            # what the backward kernel's undefined loop bounds emulate to: every H == 1 / W == 1 case
        for case in R.UPFLOW_CASES:
            if case[2] == 1 or case[3] == 1:
                assert _upflow_needs(case, mut)["upflow8_bwd"] > 4.0 * R.LIMITS["upflow8_bwd"], case


# ================================================================================================================ sequence loss
def _train_py_loss(preds, gt, valid, w, max_flow):
    """pytorch/train.py:60-96 in float64, the weights given."""
    mag = torch.sum(gt ** 2, dim=1).sqrt()
    mask = (valid >= 0.5) & (mag < max_flow)
    loss = 0.0
    for i, p in enumerate(preds):
        diff = p - gt
        loss = loss + float(w[i]) * (mask[:, None] * (diff ** 2 + R.LOSS_EPS ** 2) ** 0.5).mean()
    return loss


@pytest.mark.parametrize("run", R.LOSS_RUNS[:-1], ids=lambda r: _ids(r[0]) + "-" + "-".join(map(str, r[1:])))
def test_loss_restatement_equals_autograd(run):
    for a in R.loss_launches(run):
        B, _, H, W = a["preds"][0].shape
        n = len(a["preds"])
        pd = [p.double().requires_grad_(True) for p in a["preds"]]
        gt = a["gt"].double() if a["gt"] is not None else torch.zeros(B, 2, H, W, dtype=torch.float64)
        valid = a["valid"].double() if a["valid"] is not None else torch.ones(B, H, W, dtype=torch.float64)
        if a["gt"] is not None and torch.equal(a["gt"], a["preds"][-1]):
            gt = pd[-1].detach()
        loss = _train_py_loss(pd, gt, valid, a["w"], a["max_flow"])
        loss.backward()
        out, dps = R.seqloss_ref(a["preds"], [True] * n, a["w"], a["metric"], a["gt"], a["valid"], a["max_flow"], R.LOSS_EPS, a["out0"])
        o0 = a["out0"].double() if a["out0"] is not None else torch.zeros(6, dtype=torch.float64)
        assert abs(float(out[0] - o0[0]) - float(loss.detach())) <= 1e-13 * max(1.0, float(loss.detach()))
        for d, p in zip(dps, pd):
            assert (d - p.grad).abs().max().item() <= 1e-15
        if 0 <= a["metric"] < n:
            e = torch.sum((pd[a["metric"]].detach() - gt) ** 2, dim=1).sqrt().view(-1)[(valid > 0.5).view(-1)]
            stats = torch.tensor([e.sum(), (e < 1).sum(), (e < 3).sum(), (e < 5).sum(), e.numel()], dtype=torch.float64)
            assert (out[1:] - o0[1:] - stats).abs().max().item() <= 1e-12 * max(1.0, float(e.sum()))
        else:
            assert torch.equal(out[1:], o0[1:])
        dead = R.seqloss_ref(a["preds"], a["live"], a["w"], a["metric"], a["gt"], a["valid"], a["max_flow"], R.LOSS_EPS)[1]
        assert [d is None for d in dead] == [not l for l in a["live"]]


def test_loss_restatement_equals_the_reference_outputs():
    g = load("sequence_loss")
    for name in ("a", "b", "c"):
        B, H, W, n, seed = (int(v) for v in g[name + "_cfg"])
        gamma, gamma2 = (float(v) for v in g[name + "_gamma"])
        preds = [_rand((B, 2, H, W), seed + 10 + i, 3.0) for i in range(n)]
        gt = _rand((B, 2, H, W), seed + 1, 4.0)
        gt[:, :, 0, :3] = 500.0
        gt[:, 0, 1, 1] = 300.0
        gt[:, 1, 1, 1] = 300.0
        valid = (torch.from_numpy(np.random.default_rng(seed + 2).uniform(0.0, 1.0, (B, H, W)).astype(np.float32)) > 0.2).float()
        valid[:, 2, 2] = 0.5
        h = n // 2
        w = torch.tensor([gamma ** (h - i - 1) if i < h else gamma2 ** (h - (i - h) - 1) for i in range(n)], dtype=torch.float64)
        out, dps = R.seqloss_ref(preds, [True] * n, w, h - 1, gt, valid, 400.0, R.LOSS_EPS)
        ref = float(g[name + "_loss"])
        assert abs(float(out[0]) - ref) <= 1e-6 * abs(ref), name
        for got, r in zip((out[1] / out[5], out[2] / out[5], out[3] / out[5], out[4] / out[5]), g[name + "_metrics"]):
            assert abs(float(got) - float(r)) <= 1e-6 + 1e-6 * abs(float(r)), name
        for i, d in enumerate(dps):
            r = torch.from_numpy(g[f"{name}_dpred{i}"]).double()
            assert (d - r).abs().max().item() <= 1e-9 + 1e-5 * r.abs().max().item(), (name, i)


@pytest.mark.parametrize("run", R.LOSS_RUNS, ids=lambda r: _ids(r[0]) + "-" + "-".join(map(str, r[1:])))
def test_loss_inputs_keep_off_the_thresholds(run):
    for a in R.loss_launches(run):
        assert R.loss_conditions(a["preds"], a["gt"], a["valid"], a["max_flow"]) == 0
    (B, H, W, n), *_ = run
    if H * W >= 8:
        p, gt, valid, _ = R.loss_inputs(B, H, W, n)
        d = (p[0] - gt).view(B, 2, -1)[0, :, :3]
        assert torch.equal(d, torch.tensor(R.DESIGNED_D).T) and float(valid.view(B, -1)[0, 4]) == 0.5
        assert torch.equal(gt.view(B, 2, -1)[0, :, 3], torch.tensor([240.0, 320.0]))


def _loss_needs(a, mut=None):
    """{key: need}: loss, epe, counts (0 or inf), dpred of the twin or a mutant on one launch."""
    exp = R.loss_expect_of(a)
    kw = dict(dtype=torch.float32) if mut is None else dict(mut=mut)
    out, dps = R.seqloss_ref(a["preds"], a["live"], a["w"], a["metric"], a["gt"], a["valid"], a["max_flow"], R.LOSS_EPS, a["out0"], **kw)
    ref, scale = exp["out"]
    res = dict(loss=R.need(out[0], ref[0], scale[0])[0], epe=R.need(out[1], ref[1], scale[1])[0],
               counts=0.0 if torch.equal(out[2:].double(), ref[2:]) else float("inf"), dpred=0.0)
    for d, e in zip(dps, exp["dpred"]):
        if e is not None:
            res["dpred"] = max(res["dpred"], R.need(d, e[0], e[1], e[2])[0])
    return res


@pytest.mark.parametrize("run", R.LOSS_RUNS, ids=lambda r: _ids(r[0]) + "-" + "-".join(map(str, r[1:])))
def test_loss_twin_within_limits(run):
    for a in R.loss_launches(run):
        res = _loss_needs(a)
        assert res.pop("counts") == 0.0
        for k, v in res.items():
            assert v <= R.LIMITS[k], (k, v)


LOSS_MUTANTS = ("valid_gt", "le", "stats_lossmask", "no_numel", "eps")


@pytest.mark.parametrize("mut", LOSS_MUTANTS)
def test_loss_mutants_exceed_four_times_the_limit(mut):
    devs = []
    for run in R.LOSS_RUNS[:-1]:
        for a in R.loss_launches(run):
            res = _loss_needs(a, mut)
            devs.append(max([res.pop("counts")] + [v / R.LIMITS[k] for k, v in res.items()]))
    _mutant_rule(mut, devs)


# ======================================================================================================================== AdamW
def _torch_adamw(n, steps, norm_kind, wd, skip):
    """torch.optim.AdamW + clip_grad_norm_ on three float64 parameters that tile the flat buffer at multiples of 64."""
    p0 = R.adamw_inputs(n)[0].double()
    cuts = [0, 64, 128, n] if n > 128 else [0, n]
    params = [p0[a:b].clone().requires_grad_(True) for a, b in zip(cuts[:-1], cuts[1:])]
    opt = torch.optim.AdamW(params, lr=R.ADAMW_LRS[0], betas=R.BETAS, eps=R.ADAM_EPS, weight_decay=wd)
    norms = []
    for k in range(steps):
        g = R.adamw_grad(n, k).double()
        for i, (q, a, b) in enumerate(zip(params, cuts[:-1], cuts[1:])):
            q.grad = None if (skip and i == 0) else g[a:b].clone()
        opt.param_groups[0]["lr"] = R.ADAMW_LRS[k]
        if norm_kind != "none":
            norms.append(torch.nn.utils.clip_grad_norm_(params, R.MAX_NORM if norm_kind == "above" else 1e3).clone())
        opt.step()
    return torch.cat([q.detach() for q in params]), opt, params, norms


@pytest.mark.parametrize("n,norm_kind,wd,skip", ((5, "none", 0.0, False), (1027, "above", 1e-2, False), (1027, "below", 1e-2, True)))
def test_adamw_restatement_equals_torch(n, norm_kind, wd, skip):
    want, opt, params, norms = _torch_adamw(n, 3, norm_kind, wd, skip)
    p, _, m, v = (t.double() for t in R.adamw_inputs(n))
    table = torch.zeros((n + 63) // 64, dtype=torch.uint8)
    table[0] = 1
    step = 0.0
    for k in range(3):
        g = R.adamw_grad(n, k).double()
        gn = torch.where(R._keep(table, n), torch.zeros_like(g), g) if skip else g
        norm = None if norm_kind == "none" else gn.norm()
        if norms:
            assert abs(float(norm) - float(norms[k])) <= 1e-12
        p, _, m, v, step, st, _ = R.adamw_ref(p, g, m, v, step, norm, R.MAX_NORM if norm_kind == "above" else 1e3, R.ADAMW_LRS[k],
                                               R.BETAS, R.ADAM_EPS, wd, table if skip else None)
    assert step == 3.0 and (p - want).abs().max().item() <= 1e-13
    if not skip:
        assert (m - torch.cat([opt.state[q]["exp_avg"] for q in params])).abs().max().item() <= 1e-15
        assert (v - torch.cat([opt.state[q]["exp_avg_sq"] for q in params])).abs().max().item() <= 1e-15
    else:
        assert torch.equal(p[:64], R.adamw_inputs(n)[0].double()[:64]) and not bool((p[64:] == R.adamw_inputs(n)[0].double()[64:]).any())


@functools.lru_cache(maxsize=None)
def _adamw_twin_needs(run):
    """{key: worst need of the fp32 twin over the three steps of a run}; every step starts from the twin's own fp32 state."""
    n, _, _, _, step0 = run
    p, _, m, v = R.adamw_inputs(n)
    step, worst = float(step0), {}
    for k in range(3):
        g, norm, lr, wd, table = R.adamw_step_setup(run, k)
        args = (p, g, m, v, step, norm, R.MAX_NORM, lr, R.BETAS, R.ADAM_EPS, wd, table)
        exp = R.adamw_expect(*args)
        p1, g1, m1, v1, t, st = R.adamw_twin(*args)
        assert t == exp["step"] and torch.equal(g1, torch.where(exp["keep"], g, g * st[0]))
        for name, got in (("p", p1), ("m", m1), ("v", v1), ("state", st)):
            ref, scale, slack, key = exp[name]
            worst[key] = max(worst.get(key, 0.0), R.need(got, ref, scale, slack)[0])
        p, m, v, step = p1, m1, v1, t
    return worst


@pytest.mark.parametrize("run", R.ADAMW_RUNS, ids=lambda r: "-".join(map(str, r)))
def test_adamw_twin_within_limits(run):
    for k, v in _adamw_twin_needs(run).items():
        assert v <= R.LIMITS[k], (k, v)


ADAMW_MUTANTS = ("decay_after", "v_unclipped", "no_clamp", "skip_decays", "t-1")


@pytest.mark.parametrize("mut", ADAMW_MUTANTS)
def test_adamw_mutants_exceed_four_times_the_limit(mut):
    devs = []
    for run in R.ADAMW_RUNS:
        n, _, _, _, step0 = run
        if n > 4096:
            continue
        p, _, m, v = R.adamw_inputs(n)
        step = float(step0)
        for k in range(3):
            g, norm, lr, wd, table = R.adamw_step_setup(run, k)
            args = (p, g, m, v, step, norm, R.MAX_NORM, lr, R.BETAS, R.ADAM_EPS, wd, table)
            exp = R.adamw_expect(*args)
            p1, g1, m1, v1, t, st, _ = R.adamw_ref(*args, mut=mut)
            worst = float("inf") if not torch.equal(g1, exp["g"]) else 0.0
            for name, got in (("p", p1), ("m", m1), ("v", v1), ("state", torch.tensor(st, dtype=torch.float64))):
                ref, scale, slack, key = exp[name]
                worst = max(worst, R.need(got, ref, scale, slack)[0] / R.LIMITS[key])
            r = R.adamw_ref(*args)
            p, m, v, step = r[0].float(), r[2].float(), r[3].float(), r[4]
            devs.append(worst)
    _mutant_rule(mut, devs)


def test_prepare_kernel_formula_in_fp32_misses_the_state_limit():
    """What csrc/optim.hip computed before its corrections moved to double: 1 - powf(fp32(beta2), 1) against 1 - 0.999."""
    b2 = torch.tensor(R.BETAS[1], dtype=torch.float32)
    old = 1.0 / torch.sqrt(1.0 - b2)
    ref = 1.0 / (1.0 - R.BETAS[1]) ** 0.5
    units = abs(float(old) - ref) / (R.U24 * ref)
    assert 100 < units < 116 and units > 4 * R.LIMITS["adam_state"]
    # and 1.f - fp32(beta2), the weight of g^2 in v: at step 1, v = (1 - beta2) g^2 and the scale is u |v|
    omb2 = float(torch.tensor(1.0, dtype=torch.float32) - b2)
    units = abs(omb2 - (1.0 - R.BETAS[1])) / (R.U24 * (1.0 - R.BETAS[1]))
    assert 200 < units < 230 and units > 4 * R.LIMITS["adam_mv"]


# ====================================================================================================================== limits
def twin_worst():
    out = {}

    def put(d):
        for k, v in d.items():
            out[k] = max(out.get(k, 0.0), v)
    for case in R.UP_CASES:
        for kind in R.UP_MASKS:
            put(_up_needs(case, kind))
    for case in R.UPFLOW_CASES:
        put(_upflow_needs(case))
    for run in R.LOSS_RUNS:
        for a in R.loss_launches(run):
            res = _loss_needs(a)
            res.pop("counts")
            put(res)
    for run in R.ADAMW_RUNS:
        put(_adamw_twin_needs(run))
    return out


def test_limits_are_four_times_the_twins_worst():
    got = twin_worst()
    assert set(got) == set(R.LIMITS)
    for k, v in got.items():
        assert R.LIMITS[k] == R.limit_from_twin(v), (k, v, R.LIMITS[k])
        assert abs(v - R.TWIN_WORST[k]) <= 0.06 * max(v, 0.1), (k, v)


def test_case_lists_hold_what_the_issue_names():
    assert set(R.UP_CASES) == {(1, 1, 1), (1, 1, 17), (2, 2, 15), (1, 3, 16), (2, 3, 17), (1, 2, 33), (1, 2, 7), (1, 2, 8), (1, 2, 9)}
    assert set(R.UPFLOW_CASES) == {(1, 1, 1, 1), (1, 2, 1, 5), (2, 2, 4, 1), (1, 2, 2, 2), (2, 2, 5, 7), (1, 3, 9, 33)}
    assert 3 * 72 * 264 % 256 and 3 * 9 * 33 % 256                         # 1x3x9x33: a partial workgroup in both upflow8 kernels
    assert {r[0] for r in R.LOSS_RUNS} == set(R.LOSS_CASES)
    B, H, W, n = R.LOSS_BIG
    assert B * H * W == 525312 > 2048 * 256 and B * H * W - 2048 * 256 == 1024
    assert {c[1] * c[2] for c in R.LOSS_SMALL} == {1, 255, 256, 257, 35}
    for what in ("all", "mid_null", "none"):
        assert any(r[1] == what and r[0][3] >= 3 for r in R.LOSS_RUNS)
    assert any(not r[2] and r[0][3] >= 3 for r in R.LOSS_RUNS) and any(not r[3] and r[0][3] >= 3 for r in R.LOSS_RUNS)
    assert {(r[4] - r[0][3] if r[4] > 0 else r[4]) for r in R.LOSS_RUNS if r[0][3] >= 3} >= {-1, 0}
    assert any(r[4] == r[0][3] - 1 and r[0][3] >= 3 for r in R.LOSS_RUNS) and any(r[4] == r[0][3] >= 3 for r in R.LOSS_RUNS)
    assert any(r[5] == R.INF and r[0][3] >= 3 for r in R.LOSS_RUNS)
    assert {r[6] for r in R.LOSS_RUNS if r[0][3] >= 3} == {"plain", "prefilled", "semi"}
    assert {r[0] for r in R.ADAMW_RUNS} == set(R.ADAMW_N) == {1, 3, 4, 5, 63, 64, 65, 1027, 4194304, 4194308, 4194311}
    assert 4194304 // 4 == 4096 * 256 and 4194311 & 3 and {r[1] for r in R.ADAMW_RUNS} == set(R.ADAMW_NORMS)
    assert {r[2] for r in R.ADAMW_RUNS} == {0.0, 1e-2} and {r[4] for r in R.ADAMW_RUNS} == {0, 999, 99999}
    for n in R.ADAMW_SKIP_N:
        assert {r[3] for r in R.ADAMW_RUNS if r[0] == n} == set(R.ADAMW_SKIPS) | {None}
        t = R.skip_table("all_three", n)
        assert t.numel() == (n + 63) // 64 and int(t.sum()) == 3 and t[0] and t[n // 64 - 1] and t[-1] and (n // 4 * 4) // 64 == t.numel() - 1
