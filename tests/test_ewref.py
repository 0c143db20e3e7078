"""tests/_ewref.py on the CPU: every restatement of the elementwise and layout entries against an independent float64 torch
expression (permute, F.unfold, the adjoint identity, autograd through the ConvGRU formula, x.sum), the case tables against the
boundaries they are there for, and the proof of the limits -- every twin passes every case, LIMITS are what the twins' worst
values give, every mutant reaches 4 x its limit or fails an exact comparison, the un-mutated restatement scores 0."""
import functools

import pytest
import torch
import torch.nn.functional as F

import _ewref as R

OPS = sorted(R.OPS)
SMALL = {op: [c for c in R.cases(op) if c not in R.BIG_CASES] for op in OPS}


@functools.lru_cache(maxsize=None)
def _small(op, c):
    p = R.build(op, c)
    return p, R.expect(p)


def _pe(op, c):
    if c in R.BIG_CASES:
        p = R.build(op, c)
        return p, R.expect(p)
    return _small(op, c)


def _close64(a, b, rtol=1e-12):
    a, b = a.double(), b.double()
    return bool(((a - b).abs() <= rtol * (a.abs() + b.abs()) + 1e-300).all())


# ------------------------------------------------------------------------------------------------------------ restatements
@pytest.mark.parametrize("op", ("nchw_to_nhwc", "nhwc_to_nchw"))
def test_layout_restatements_equal_permute(op):
    for c in SMALL[op]:
        p, outs = _pe(op, c)
        B, C, HW, ld, coff, acc = c
        cl = lambda t: torch.as_strided(t, (B, HW, C), (HW * ld, ld, 1), coff)
        if op == "nchw_to_nhwc":
            want = p.bufs["dst"].double()
            v = p.bufs["src"].view(B, C, HW).permute(0, 2, 1).double()
            cl(want).copy_(cl(want) + v if acc else v)
        else:
            v = cl(p.bufs["src"]).permute(0, 2, 1).double()
            want = (p.bufs["dst"].view(B, C, HW).double() + v if acc else v).reshape(-1)
        img = outs["dst"].image().double()
        assert torch.equal(torch.nan_to_num(img, nan=-7.0), torch.nan_to_num(want, nan=-7.0)), c
        assert int(torch.isnan(img).sum()) == img.numel() - B * C * HW, c


def test_space_to_depth_restatement_equals_a_view_permute_and_inverts():
    for c in SMALL["space_to_depth2"]:
        p, outs = _pe("space_to_depth2", c)
        B, H, W, C, inv = c
        x = p.bufs["src"]
        if inv:
            want = x.view(B, H // 2, W // 2, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(-1)
        else:
            want = x.view(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(-1)
        got = outs["dst"].image()
        assert torch.equal(got, want), c
        idx, back = R.ref_space_to_depth2(got, B, H, W, C, 1 - inv)
        assert torch.equal(back[torch.argsort(idx)], x), c
    # and F.pixel_unshuffle, whose channel order is (c, dy, dx): ours is (dy, dx, c)
    B, H, W, C = 2, 6, 8, 12
    x = torch.randn(B, H, W, C)
    idx, v = R.ref_space_to_depth2(x.reshape(-1), B, H, W, C, 0)
    ours = torch.empty(B * H * W * C)
    ours[idx] = v
    pu = F.pixel_unshuffle(x.permute(0, 3, 1, 2), 2).view(B, C, 2, 2, H // 2, W // 2).permute(0, 4, 5, 2, 3, 1)
    assert torch.equal(ours.view(B, H // 2, W // 2, 2, 2, C), pu)


def _flow_of(p, B, H, W):
    a = p.arg
    return p.bufs["flow"][R.flow_index(a["base"], a["bs"], a["cs"], a["ps"], B, H * W)].view(B, 2, H, W)


def test_im2col7_restatement_equals_unfold():
    for c in SMALL["im2col7"]:
        p, outs = _pe("im2col7", c)
        flow = _flow_of(p, c.B, c.H, c.W)
        want = torch.zeros(c.B, c.H * c.W, c.ld)
        want[:, :, :98] = F.unfold(flow, 7, padding=3).transpose(1, 2)
        assert torch.equal(outs["cols"].image(), want.reshape(-1)), c
        assert outs["cols"].scale is None and outs["cols"].idx.numel() == want.numel()


def test_col2im7_restatement_is_the_adjoint_of_im2col7():
    g = torch.Generator().manual_seed(5)
    for c in SMALL["col2im7"]:
        p, outs = _pe("col2im7", c)
        B, H, W, ld, acc = c
        f = torch.randn(B * 2 * H * W, generator=g, dtype=torch.float64)
        _, cols = R.ref_im2col7(f, 0, 2 * H * W, H * W, 1, ld, B, H, W)
        d = torch.nan_to_num(p.bufs["dcols"].double(), nan=0.0)          # (the pad columns meet im2col7's zeros)
        _, s, sa = R.ref_col2im7(p.bufs["dcols"], ld, p.bufs["dflow"], B, H, W, 0)
        lhs, rhs = float((cols * d).sum()), float((f * s).sum())
        assert abs(lhs - rhs) <= 1e-12 * float((cols.abs() * d.abs()).sum()) + 1e-300, (c, lhs, rhs)
        want = s + p.bufs["dflow"].double() if acc else s
        assert _close64(outs["dflow"].ref, want) and torch.isfinite(outs["dflow"].ref).all(), c
        fold = F.fold(d.view(B, H * W, ld)[:, :, :98].transpose(1, 2), (H, W), 7, padding=3).reshape(-1)
        assert _close64(s, fold, 1e-10) or float((s - fold).abs().max()) <= 1e-12 * float(sa.max()), c
        assert bool((sa >= s.abs() * (1 - 1e-12)).all()), c


def test_flow_copy_restatements_equal_slices():
    for c in R.FLOW_TO_NHWC_CASES:
        p, outs = _pe("flow_to_nhwc", c)
        flow = _flow_of(p, c.B, c.HW, 1).view(c.B, 2, c.HW)
        want = p.bufs["dst"].clone().view(c.B, c.HW, c.ld)
        want[:, :, c.coff:c.coff + 2] = flow.permute(0, 2, 1)
        assert R._same(outs["dst"].image(), want.reshape(-1)).all(), c
    for c in R.NHWC_TO_FLOW_CASES:
        p, outs = _pe("nhwc_to_flow", c)
        v = p.bufs["src"].view(c.B, c.HW, c.ld)[:, :, c.coff:c.coff + 2].permute(0, 2, 1).double()
        want = (p.bufs["dflow"].view(c.B, 2, c.HW).double() + v) if c.acc else v
        assert torch.equal(outs["dflow"].image().double(), want.reshape(-1)), c


def test_relu_restatement_equals_autograd_through_relu():
    for c in SMALL["relu_bwd"]:
        p, outs = _pe("relu_bwd", c)
        M, C, ldg, ldy = c
        a = p.bufs["y"].view(M, ldy)[:, :C].clone().requires_grad_(True)
        g = p.bufs["g"].view(M, ldg)
        torch.relu(a).backward(g[:, :C])
        want = g.clone()
        want[:, :C] = a.grad
        img = outs["g"].image()
        assert torch.equal(img, want.reshape(-1)) and not torch.signbit(img.view(M, ldg)[:, :C][a.detach() <= 0]).any(), c
        assert R._same(img.view(M, ldg)[:, C:], g[:, C:]).all()


def test_gru_restatements_equal_autograd_through_the_convgru_formula():
    """h' = (1 - z) h + z q, z = sigmoid(a_z), q = tanh(a_q), r = sigmoid(a_r), the q convolution fed r h (core/update.py's ConvGRU):
    stage 1 holds dL/da_z, dL/da_q and the direct dL/dh for L = <dh', h'>; stage 2 dL/da_r and dL/dh for L = <d(rh), r h>."""
    for c in SMALL["gru_bwd1"]:
        M, hid = c.M, c.hid
        p1, o1 = _pe("gru_bwd1", c)
        p2, o2 = _pe("gru_bwd2", c)
        x = {k: v.double() for k, v in R.gru_inputs(c).items()}
        az = torch.logit(x["z"]).requires_grad_(True)                       # (+-inf at the saturated gates: sigmoid gives 0 / 1 back)
        aq = torch.atanh(x["q"]).requires_grad_(True)
        h = x["h"].clone().requires_grad_(True)
        z, q = torch.sigmoid(az), torch.tanh(aq)
        assert _close64(z, x["z"], 1e-15) and _close64(q, x["q"], 1e-15)
        g = x["dhn"] + (x["dhn2"] if c.dhn2 else 0.0)
        (((1 - z) * h + z * q) * g).sum().backward()
        nn = lambda t: torch.nan_to_num(t, nan=0.0)      # (autograd's 0 * inf at the four saturated pre-activations: the gradient is 0)
        assert int(torch.isnan(az.grad).sum()) <= 2 and int(torch.isnan(aq.grad).sum()) <= 2
        assert _close64(o1["dzr"].ref.reshape(-1), nn(az.grad), 1e-9), c
        assert _close64(o1["dq"].ref.reshape(-1), nn(aq.grad), 1e-9), c
        assert _close64(o1["dh"].ref.reshape(-1), h.grad), c
        ar_ = torch.logit(x["r"]).requires_grad_(True)
        h2 = x["h"].clone().requires_grad_(True)
        (torch.sigmoid(ar_) * h2 * x["drh"]).sum().backward()
        assert _close64(o2["dzr"].ref.reshape(-1), nn(ar_.grad), 1e-9), c
        dh0 = p2.bufs["dh"].double()
        assert bool(((o2["dh"].ref.reshape(-1) - (dh0 + h2.grad)).abs() <= 1e-12 * (dh0.abs() + h2.grad.abs())).all()), c
        # stage 2 starts from what stage 1 left: dh is its output, the low half of dzr is written, the high half still the pattern
        assert torch.equal(p2.bufs["dh"], o1["dh"].ref.float().reshape(-1))
        lo, hi = o1["dzr"].idx.reshape(-1), o2["dzr"].idx.reshape(-1)
        assert not torch.isnan(p2.bufs["dzr"][lo]).any() and torch.isnan(p2.bufs["dzr"][hi]).all()
        assert torch.equal(hi, lo + hid) and int(torch.isnan(o2["dzr"].image()).sum()) == M * (c.ldzr - 2 * hid)
        if c.sums:
            assert _close64(o1["dzr_sum"].ref, p1.bufs["dzr_sum"][lo].view(M, hid).double() + o1["dzr"].ref, 1e-9)
            assert _close64(o1["dq_sum"].ref, p1.bufs["dq_sum"].view(M, hid).double() + o1["dq"].ref, 1e-9)
            assert _close64(o2["dzr_sum"].ref, p2.bufs["dzr_sum"][hi].view(M, hid).double() + o2["dzr"].ref, 1e-9)


def test_reduction_and_axpby_restatements_equal_torch():
    for c in R.COL_SUM_CASES:
        p, outs = _pe("col_sum", c)
        M, C, ld, scale = c
        want = p.bufs["out"][:C].double() + scale * p.bufs["x"].view(M, ld)[:, :C].double().sum(0)
        o = outs["out"]
        assert bool(((o.ref - want).abs() <= 1e-6 * o.scale).all()), c                 # 1e-6 units: float64 summation order only
        assert torch.isnan(o.image()[C:]).all()
    for c in SMALL["sum_n"]:
        p, outs = _pe("sum_n", c)
        L_ = R._sum_n_list(p)
        assert len(L_) == c.n
        want = torch.stack(L_).double().sum(0) + (p.bufs["out"][:c.count].double() if c.acc else 0.0)
        o = outs["out"]
        assert bool(((o.ref - want).abs() <= 1e-6 * o.scale).all()), c
        if c.dup:
            assert L_[-1] is L_[0]
    for c in SMALL["axpby"]:
        p, outs = _pe("axpby", c)
        a, b = R.f32(c.a), R.f32(c.b)
        want = a * p.bufs["x"].double() if c.b == 0 else torch.add(a * p.bufs["x"].double(), p.bufs["y"].double(), alpha=b)
        assert _close64(outs["y"].ref, want) and torch.isfinite(outs["y"].ref).all(), c
        if c.b != 0:                                    # nothing cancels: |ref| = |a x| + |b y|
            assert _close64(outs["y"].ref.abs(), (a * p.bufs["x"].double()).abs() + (b * p.bufs["y"].double()).abs())


# -------------------------------------------------------------------------------------------------------------- case tables
def test_case_tables_cross_the_boundaries_they_name():
    CAP = 16384 * 256
    # layout pair: the 32 x 32 tile one short / exact / one over on either axis, against a ragged other; pitches and offsets
    lay = R.LAYOUT_CASES
    for v in (1, 31, 32, 33):
        assert any(c.C == v and c.HW % 32 for c in lay) and any(c.HW == v and c.C % 32 for c in lay)
    for c in lay:
        assert c.coff + c.C <= c.ld
    assert {(c.ld - c.C, c.coff) for c in lay if c.C == 33} == {(0, 0), (3, 0), (7, 0), (7, 3)}
    assert {c.acc for c in lay} == {0, 1} and all(c.B == 2 for c in lay) and R.LayoutCase(2, 37, 45, 40, 0, 0) in lay
    assert R.TRANSPOSE_CASE[:4] == (3, 33, 65, 33)
    # space_to_depth2: one chunk; the first count past the cap that even H and W allow
    assert R.S2dCase(1, 2, 2, 4, 0) in R.S2D_CASES and {c.C for c in R.S2D_CASES} == {4, 8, 12}
    B, H, W, C = R.S2D_BIG
    assert B * H * W * C // 4 == CAP + 4 and H % 2 == 0 and W % 2 == 0
    # im2col7: both kernels on every image, every pitch and layout; every pixel of every image has a tap outside it
    small = SMALL["im2col7"]
    assert {(c.H, c.W, c.ld, c.off) for c in small} == {(h, w, ld, o) for h, w in R.IMAGES for ld in (100, 104, 128) for o in (0, 1)}
    assert {(c.off, c.layout) for c in small} == {(o, l) for o in (0, 1) for l in R.FLOW_LAYOUTS}
    assert all(min(h, w) < 7 or (h, w) == (7, 7) for h, w in R.IMAGES)
    v4, sc = R.IM2COL_BIG
    assert v4.off == 0 and v4.B * v4.H * v4.W * (v4.ld // 4) > CAP >= v4.B * (v4.H - 1) * v4.W * (v4.ld // 4)
    assert sc.off == 1 and sc.B * sc.H * sc.W * sc.ld > CAP >= sc.B * (sc.H - 1) * sc.W * sc.ld
    # col2im7 and the flow copies: 254 / 256 / 258 threads
    assert {2 * c.B * c.H * c.W for c in R.COL2IM_CASES} >= {254, 256, 258}
    assert {(c.ld, c.acc) for c in R.COL2IM_CASES} == {(100, 0), (100, 1), (104, 0), (104, 1)}
    for tab in (R.FLOW_TO_NHWC_CASES, R.NHWC_TO_FLOW_CASES):
        assert {2 * c.B * c.HW for c in tab} == {254, 256, 258} and {(c.ld, c.coff) for c in tab} == {(128, 126), (4, 0)}
    assert {c.layout for c in R.FLOW_TO_NHWC_CASES} == set(R.FLOW_LAYOUTS) and {c.acc for c in R.NHWC_TO_FLOW_CASES} == {0, 1}
    # relu_bwd: C % 4 != 0 inside a wider row, pitches that differ, the second trip
    rl = R.RELU_CASES
    assert {c.C for c in rl} == {4, 80, 126, 128} and all(c.ldg != c.ldy and c.ldg >= c.C <= c.ldy and c.ldg % 4 == c.ldy % 4 == 0 for c in rl)
    assert {c.ldg for c in rl if c.C == 126} == {128, 132} and {c.M for c in rl} >= {1, 3}
    assert R.RELU_BIG.M * (R.RELU_BIG.C // 4) > CAP >= (R.RELU_BIG.M - 3) * (R.RELU_BIG.C // 4)
    # ConvGRU: both kernels of both stages, each reason for the scalar one, each pointer in turn
    gr = R.GRU_CASES
    assert {c.hid for c in gr if R.gru_route(c, 1) == "v4"} == {4, 96, 128}
    assert {(c.sums, c.dhn2) for c in gr if R.gru_route(c, 1) == "v4" and c.hid == 96} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert all(not c.dhn2 for c in gr if R.gru_route(c, 1) == "scalar")
    assert any(c.hid % 4 for c in gr) and any(c.hid % 4 == 0 and c.ldzr % 4 for c in gr)
    assert {c.off for c in gr if R.gru_route(c, 1) == "scalar" and c.off} == set(R.GRU_B1_PTRS)
    assert {c.off for c in gr if R.gru_route(c, 2) == "scalar" and c.off} == set(R.GRU_B2_PTRS)
    assert {c.M * c.hid // 4 for c in gr if c.hid == 4 and not c.off} >= {255, 256, 257, CAP + 1}
    assert {c.ldzr - 2 * c.hid for c in gr if R.gru_route(c, 1) == "v4"} == {0, 4}
    # col_sum: the row split (M / 128 blocks), 64-column workgroups, the ysplit cap with empty trailing row blocks
    cs = R.COL_SUM_CASES
    assert {c.M for c in cs} == {1, 3, 127, 128, 129, 255, 256, 257, 2048 * 128 + 1} and {c.C for c in cs} == {1, 63, 64, 65, 4}
    assert all(c.ld > c.C for c in cs) and {c.scale for c in cs} == {1.0, -0.5}
    ys, per = R.col_sum_geometry(R.COL_SUM_BIG.M)
    assert ys == 2048 and (ys - 1) * per >= R.COL_SUM_BIG.M                 # the last row block starts past the end
    assert R.col_sum_geometry(255) == (1, 255) and R.col_sum_geometry(256) == (2, 128) and R.col_sum_geometry(257) == (2, 129)
    # sum_n: one launch / two / three, the 16-tensor boundary, counts of one chunk and 257
    sn = R.SUM_N_CASES
    assert {c.n for c in sn} == {1, 2, 15, 16, 17, 32, 33} and {c.count for c in sn} == {4, 1028, 4 * (CAP + 1)}
    assert any(c.dup for c in sn) and R.SUM_N_BIG.n == 2
    assert {c.n for c in R.AXPBY_CASES} == {1, 255, 256, 257, CAP + 1} and any(c.b == 0 for c in R.AXPBY_CASES)


def test_designed_values_are_where_the_docstrings_say():
    for c in SMALL["relu_bwd"]:
        p, _ = _pe("relu_bwd", c)
        y, g = p.bufs["y"].view(c.M, c.ldy), p.bufs["g"].view(c.M, c.ldg)
        yc = y[:, :c.C]
        assert bool(((yc == 0) & ~torch.signbit(yc)).any()) and bool(((yc == 0) & torch.signbit(yc)).any()), c
        assert bool((y[:, c.C:] <= 0).all()) and bool((g != 0).sum() >= g.numel() - 1) and torch.isfinite(g).all(), c
    for c in SMALL["gru_bwd1"]:
        x = R.gru_inputs(c)
        assert (x["z"][0], x["z"][1], x["r"][2], x["r"][3], x["q"][4], x["q"][5]) == (0.0, 1.0, 0.0, 1.0, 1.0, -1.0)
        for k in ("z", "r"):
            assert bool(((x[k][6:] > 0) & (x[k][6:] < 1)).all())
        assert bool((x["q"][6:].abs() < 1).all())
    p, _ = _pe("col_sum", R.COL_SUM_CASES[4])
    X = p.bufs["x"].view(129, -1)[:, :65].abs()
    assert float(X[0].median() / X[1].median()) > 2.0 ** 20


# ------------------------------------------------------------------------------------------------------------------- limits
@functools.lru_cache(maxsize=None)
def _twin_scores():
    """{(op, case, variant, output): (limit key, score)} over every case."""
    out = {}
    for op in OPS:
        for c in R.cases(op):
            p, outs = _pe(op, c)
            for variant, res in R.twins(p).items():
                for name, vals in res.items():
                    o = outs[name]
                    out[(op, c, variant, name)] = (o.key, R.score(o.image(vals.float()), o))
    return out


@pytest.mark.parametrize("op", OPS)
def test_every_twin_passes_every_case(op):
    mine = {k: v for k, v in _twin_scores().items() if k[0] == op}
    moving = op in ("space_to_depth2", "im2col7", "flow_to_nhwc", "relu_bwd")
    assert bool(mine) != moving
    for k, (key, w) in mine.items():
        assert w <= R.LIMITS[key], (k, w)
    for c in R.cases(op):                               # an output with a scale has a twin, an exact one has none
        if c in R.BIG_CASES:
            continue
        for name, o in _pe(op, c)[1].items():
            assert (o.scale is None) != any(k[1] == c and k[3] == name for k in mine), (op, c, name)


def test_limits_are_four_times_the_twins_worst():
    got = {}
    for key, w in _twin_scores().values():
        got[key] = max(got.get(key, 0.0), w)
    assert set(got) == set(R.LIMITS) == set(R.TWIN_WORST)
    for k, v in got.items():
        assert R.LIMITS[k] == R.limit_from_twin(v), (k, v, R.LIMITS[k])
        assert abs(v - R.TWIN_WORST[k]) <= 0.06 * max(v, 0.1), (k, v)


def test_sum_n_list_order_twin_is_a_plain_left_to_right_sum():
    c = R.SumNCase(17, 1028, 1, 0)
    p, _ = _pe("sum_n", c)
    L_ = R._sum_n_list(p)
    s = p.bufs["out"][:c.count].clone()
    for x in L_[:16]:
        s += x
    s += L_[16]                                         # the second launch: onto what the first left
    assert torch.equal(s, R.sum_n_listorder(L_, p.bufs["out"], c.count, 1))
    z = R.sum_n_listorder([torch.full((4,), -0.0)], R.pattern(8), 4, 0)
    assert not torch.signbit(z).any()                   # (+0.0) + (-0.0)


# ------------------------------------------------------------------------------------------------------------------ mutants
def test_the_unmutated_restatement_scores_zero():
    for op in OPS:
        for c in SMALL[op]:
            for name, o in _pe(op, c)[1].items():
                assert R.score(o.image(), o) == 0.0, (op, c, name)


@pytest.mark.parametrize("name", sorted(R.MUTANTS))
def test_every_mutant_is_rejected(name):
    """On at least one case the mutant changes a float outside the addressed region, fails an exact comparison (both: inf) or
    reaches 4 x the limit of an output."""
    op, fn = R.MUTANTS[name]
    best, shown, applied = 0.0, 0, 0
    for c in SMALL[op]:
        p, outs = _pe(op, c)
        got = fn(p)
        if got is None:
            continue
        applied += 1
        ratio = 0.0
        for out_name, img in got.items():
            o = outs[out_name]
            w = R.score(img, o)
            ratio = max(ratio, w if o.scale is None else w / R.LIMITS[o.key])
        shown += ratio >= 4.0
        best = max(best, ratio)
    assert applied and shown >= 1 and best >= 4.0, (name, best, shown, applied)


def test_the_listed_mutants_are_all_there():
    assert len(R.MUTANTS) == 22 and {op for op, _ in R.MUTANTS.values()} == set(OPS) - {"flow_to_nhwc", "nhwc_to_flow"}
