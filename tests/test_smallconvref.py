"""tests/_smallconvref.py on the CPU: the restatements of the stem and small-convolution entries against F.conv2d / its autograd in
float64, the case tables against the edges they are there for, and the proof of the comparator -- every twin passes every case,
the bf16x1 twin fails, the data gradient's limit is what its fp32 twins' worst gives, every mutant scores 4 x its limit or
infinite, the un-mutated restatement scores 0."""
import pytest
import torch
import torch.nn.functional as F

import _smallconvref as S

OPS = sorted(S.OPS)


def _close64(a, b, tol=1e-12):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return bool(((a - b).abs() <= tol * (a.abs() + b.abs()) + tol * float(b.abs().max())).all())


# ------------------------------------------------------------------------------------------------------------ restatements
def test_stem_restatements_equal_conv2d_and_its_autograd():
    for c in S.STEM_FWD_CASES:
        p, outs = S.problem("stem_fwd", c)
        B, H, W, N, bias = c
        Ho, Wo = S.stem_dims(H, W)
        y = F.conv2d(p.bufs["x"].double().view(B, 3, H, W), p.bufs["w"].double().view(N, 3, 7, 7),
                     p.bufs["bias"].double() if bias else None, stride=2, padding=3)
        assert y.shape == (B, N, Ho, Wo) and _close64(outs["out"].ref, y.permute(0, 2, 3, 1), 1e-13), c
        assert outs["out"].idx.numel() == outs["out"].init.numel() == B * Ho * Wo * N
    for c in S.STEM_WGRAD_CASES:
        p, outs = S.problem("stem_wgrad", c)
        B, H, W, N = c
        Ho, Wo = S.stem_dims(H, W)
        w = torch.zeros(N, 3, 7, 7, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(p.bufs["x"].double().view(B, 3, H, W), w, stride=2, padding=3)
        y.backward(p.bufs["dy"].double().view(B, Ho, Wo, N).permute(0, 3, 1, 2))
        assert _close64(outs["dw"].ref, w.grad, 1e-13), c


def test_small_restatements_equal_conv2d_and_its_autograd():
    for c in S.SMALL_FWD_CASES:
        p, outs = S.problem("small_fwd", c)
        B, H, W, C, ld, coff, olay, bias = c
        x = S._live(p.bufs["x"], B, H, W, C, ld, coff).double().permute(0, 3, 1, 2)
        assert torch.isfinite(x).all() and int(torch.isnan(p.bufs["x"]).sum()) == B * H * W * (ld - C)
        y = F.conv2d(x, p.bufs["w"].double().view(2, C, 3, 3), p.bufs["bias"].double() if bias else None, padding=1)
        o = outs["out"]
        assert _close64(o.ref, y.permute(0, 2, 3, 1).reshape(-1, 2), 1e-13), c
        obs, ocs, ops = S.out_strides(olay, H * W)
        img = o.image().float()
        got = torch.as_strided(img, (B, 2, H * W), (obs, ocs, ops))
        assert torch.equal(got, y.reshape(B, 2, H * W).float()) and int(torch.isnan(img).sum()) == img.numel() - 2 * B * H * W
    for c in S.SMALL_WGRAD_CASES:
        p, outs = S.problem("small_wgrad", c)
        B, H, W, C = c[:4]
        dys, xs = S._segs(p)
        w = torch.zeros(2, C, 3, 3, dtype=torch.float64, requires_grad=True)
        b = torch.zeros(2, dtype=torch.float64, requires_grad=True)
        for dy, x in zip(dys, xs):
            assert torch.isfinite(dy).all() and torch.isfinite(x).all()
            F.conv2d(x.double().permute(0, 3, 1, 2), w, b, padding=1).backward(dy.double().permute(0, 3, 1, 2))
        idx, ktot = S.dwpk_index(C)
        o = outs["dwpk"]
        assert ktot == 9 * ((C + 31) // 32 * 32) and o.init.numel() == 2 * ktot
        assert _close64(o.ref - o.init[idx].double(), w.grad.permute(0, 2, 3, 1).reshape(2, 9, C), 1e-12), c
        assert int(torch.isnan(o.image()).sum()) == 2 * ktot - 18 * C          # the pad columns
        assert bool((o.init[idx] != 0).all()) == bool(c.prior)
        if c.dbias:
            assert _close64(outs["dbias"].ref - outs["dbias"].init[:2].double(), b.grad, 1e-12), c
        for t in range(c.nseg):
            assert int(torch.isnan(p.bufs[f"dy{t}"]).sum()) == B * H * W * (c.ldy - 2)
    for c in S.SMALL_DGRAD_CASES:
        p, outs = S.problem("small_dgrad", c)
        B, H, W, C, lddx, ldy, ldm = c
        dy, w, keep = S._dgrad_parts(p)
        x = torch.zeros(B, C, H, W, dtype=torch.float64, requires_grad=True)
        F.conv2d(x, w, padding=1).backward(dy)
        o = outs["dx"]
        want = x.grad.permute(0, 2, 3, 1) * keep
        assert _close64(o.ref, want, 1e-13) and bool((o.ref[o.zero] == 0).all()), c
        assert bool((o.scale >= S.U24 * o.ref.abs() * (1 - 1e-9)).all())
        assert int(torch.isnan(o.image()).sum()) == B * H * W * (lddx - C)


# -------------------------------------------------------------------------------------------------------------- case tables
def test_case_tables_reach_the_edges_they_name():
    sf = S.STEM_FWD_CASES
    assert {c[:3] for c in sf} == set(S.STEM_SHAPES) and all({(c.N, c.bias) for c in sf if c[:3] == s} == {(32, 0), (32, 1), (64, 0), (64, 1)} for s in S.STEM_SHAPES)
    tiles = {s: S.stem_fwd_tiles(*s) for s in S.STEM_SHAPES}
    assert tiles[(1, 7, 7)] == (1, 1, 1) and tiles[(3, 17, 65)] == (12, 2, 2) and tiles[(513, 7, 7)][0] == 513 and tiles[(1030, 7, 7)][0] == 1030
    assert {S.stem_dims(*s[1:]) for s in S.STEM_SHAPES} >= {(4, 4), (8, 32), (9, 33)}
    assert 1030 - 2 * 512 == 6                          # workgroups 0 .. 5 take three tiles, the rest two
    sw = S.STEM_WGRAD_CASES
    slots = [S.stem_wgrad_slots(*c[:3]) for c in sw]
    assert slots[:15] == [4, 5, 12, 13, 16, 17, 60, 61, 64, 65, 77, 511, 512, 512, 512]
    assert [S.stem_wgrad_tiles(*c[:3])[0] for c in sw[11:15]] == [511, 512, 513, 1025] and S.stem_wgrad_tiles(3, 9, 131)[1] == 3
    loops = {s: S.reduce_loops(s) for s in set(slots)}
    for s, l in loops.items():                          # every slot exactly once
        assert sorted(l["x16"] + l["x4"] + l["tail"]) == list(range(s)), s
    assert not loops[60]["x16"] and loops[61]["x16"] and not loops[12]["x4"] and loops[13]["x4"] and not loops[64]["tail"] and loops[65]["tail"]
    assert any(c.N == 32 for c in sw) and S.STEM_SCRATCH == 512 * 64 * 192
    f = S.SMALL_FWD_CASES
    assert {c.C for c in f} == {4, 36, 252, 256, 260, 512} and {c.W for c in f} >= {1, 7, 8, 9, 17} and {c.H for c in f} >= {1, 2, 3}
    assert {c.B for c in f} == {1, 3} and {c.olay for c in f} == {"planar", "gap", "inter"} and {c.bias for c in f} == {0, 1}
    assert {("C", "C+4", "2C")[(c.ld > c.C) + (c.ld == 2 * c.C)] for c in f} == {"C", "C+4", "2C"} and any(c.coff for c in f)
    assert all(c.coff + c.C <= c.ld and c.coff % 4 == 0 and c.ld % 4 == 0 for c in f)
    b = S.SMALL_FWD_BIG
    assert b.B * b.H * ((b.W + S.FWD_RUN - 1) // S.FWD_RUN) == 8256 > S.FWD_WAVES
    g = S.SMALL_WGRAD_CASES
    assert {c.C for c in g} == {4, 36, 252, 256, 260, 512} and {c.W for c in g} >= {1, 8, 9, 16, 17, 25}
    assert {c.nseg for c in g} == {1, 2, 16, 17, 33} and {c.ldy for c in g} == {2, 4, 7} and {c.prior for c in g} == {0, 1} == {c.dbias for c in g}
    b = S.SMALL_WGRAD_BIG
    assert b.B * b.H * ((b.W + S.WG_RUN - 1) // S.WG_RUN) == 2080 > S.WG_WAVES
    d = S.SMALL_DGRAD_CASES
    assert {c.C for c in d} == {4, 36, 252, 256} and {c.W for c in d} >= {1, 15, 16, 17, 33} and {c.H for c in d} >= {1, 2, 3}
    assert {c.ldy for c in d} == {2, 4, 5} and any(c.lddx == c.C for c in d) and any(c.lddx == c.C + 4 for c in d) and any(c.lddx == 512 for c in d)
    assert any(not c.ldm for c in d) and any(c.ldm > c.C for c in d)
    b = S.SMALL_DGRAD_BIG
    assert b.B * b.H * ((b.W + S.DG_RUN - 1) // S.DG_RUN) == 16512 > S.DG_WAVES
    p, _ = S.problem("small_dgrad", S.SMALL_DGRAD_CASES[2])
    m = p.bufs["relu"].view(-1, 256)[:, :252]
    assert bool(((m == 0) & ~torch.signbit(m)).any()) and bool(((m == 0) & torch.signbit(m)).any())
    assert bool((m == S.DENORMAL).any()) and bool((m == -S.DENORMAL).any()) and bool((m > 1e-3).any()) and bool((m < -1e-3).any())


# ------------------------------------------------------------------------------------------------------------------- limits
@pytest.mark.parametrize("op", OPS)
def test_every_twin_passes_and_the_bf16x1_twin_fails(op):
    for c in S.cases(op):
        p, outs = S.problem(op, c)
        tw = S.twins(p, outs)
        assert tw, (op, c)
        for variant, res in tw.items():
            ok, s, _ = S.verdict({k: o.image(res[k]) for k, o in outs.items()}, outs)
            assert ok and s <= 1.0, (op, c, variant, s)
        if op != "small_dgrad":
            ok, s, _ = S.verdict({k: o.image(o.twins["bf16x1"]) for k, o in outs.items()}, outs)
            assert not ok and s >= 4.0, (op, c, s)


def test_the_data_gradient_limit_is_four_times_its_twins_worst():
    got = S.twin_worst()
    assert set(got) == set(S.LIMITS) == set(S.TWIN_WORST)
    for k, v in got.items():
        assert S.LIMITS[k] == S.limit_from_twin(v), (k, v, S.LIMITS[k])
        assert abs(v - S.TWIN_WORST[k]) <= 0.06 * v, (k, v)


def test_the_order_twins_are_what_they_say():
    """Lanes-and-tree and waves-then-atomics are fp32 sums of the same products: equal to float64 within the elementwise bound, and
    bit-equal to a plain sum where only one term is live."""
    p, outs = S.problem("small_fwd", S.SMALL_FWD_CASES[0])         # one pixel, four channels: lane 0 only
    x, w = S._live(p.bufs["x"], 1, 1, 1, 4, 4, 0).reshape(4), p.bufs["w"].view(2, 4, 3, 3)[:, :, 1, 1]
    a = [S._fma(x, w[o], torch.zeros(4)) for o in range(2)]
    want = torch.stack([((v[0] + v[1]) + (v[2] + v[3])) + p.bufs["bias"][o] for o, v in enumerate(a)])
    assert torch.equal(outs["out"].alt["lanes and tree"].reshape(-1).float(), want)
    p, outs = S.problem("small_wgrad", S.SMALL_WGRAD_CASES[0])     # one pixel, one segment: one product onto a zero prior
    dys, xs = S._segs(p)
    want = dys[0].reshape(2)[:, None] * xs[0].reshape(4)[None, :]
    got = outs["dwpk"].alt["waves then atomics"].view(2, 3, 3, 4)
    assert torch.equal(got[:, 1, 1].float(), want) and float(got.abs().sum()) == float(want.double().abs().sum())


# ------------------------------------------------------------------------------------------------------------------ mutants
def test_the_unmutated_restatement_scores_zero():
    for op in OPS:
        for c in S.cases(op):
            _, outs = S.problem(op, c)
            ok, s, _ = S.verdict({k: o.image() for k, o in outs.items()}, outs)
            assert ok and s == 0.0, (op, c)


def test_one_changed_bit_outside_the_addressed_floats_scores_infinite():
    for op, k, c in (("small_fwd", "out", S.SMALL_FWD_CASES[1]), ("small_wgrad", "dwpk", S.SMALL_WGRAD_CASES[1]), ("small_dgrad", "dx", S.SMALL_DGRAD_CASES[1])):
        _, outs = S.problem(op, c)
        got = {n: o.image().float() for n, o in outs.items()}
        assert S.verdict(got, outs)[1] <= 1.0               # (rounded to fp32: within every limit)
        o = outs[k]
        outside = torch.ones(o.init.numel(), dtype=torch.bool)
        outside[o.idx.reshape(-1)] = False
        i = int(outside.nonzero()[0])
        got[k].view(torch.int32)[i] ^= 1
        assert S.verdict(got, outs)[1] == S.INF, op


@pytest.mark.parametrize("name", sorted(S.MUTANTS))
def test_every_mutant_is_rejected(name):
    op, fn = S.MUTANTS[name]
    best, applied = 0.0, 0
    for c in S.cases(op):
        p, outs = S.problem(op, c)
        got = fn(p)
        if got is None:
            continue
        applied += 1
        ok, s, _ = S.verdict({k: got.get(k, o.image()) for k, o in outs.items()}, outs)
        assert ok == (s <= 1.0)
        best = max(best, s)
    assert applied and best >= 4.0, (name, best, applied)


def test_the_listed_mutants_are_all_there():
    per = {op: sum(1 for o, _ in S.MUTANTS.values() if o == op) for op in OPS}
    assert per == dict(stem_fwd=4, stem_wgrad=3, small_fwd=2, small_wgrad=5, small_dgrad=3)
