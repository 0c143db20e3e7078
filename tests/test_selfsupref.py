"""CPU checks that pin tests/_selfsupref.py, the oracle of csrc/selfsup_loss.hip: closed forms, the autograd gradient against
float64 central differences, the two places where the reference is easy to restate wrongly (the normaliser's size, the strict
comparisons at equality), the input conditions of every GPU case and the derivation of the limits."""
import math

import pytest
import torch

import _selfsupref as R

CASES = R.cases()
NAMES = [c["name"] for c in CASES]


def case(name):
    return CASES[NAMES.index(name)]


def test_zero_flows_give_loss_zero_and_student_mask_zero():
    for name in ("1x1x1-zero", "2x37x61-zero", "3x24x40in48x80-zero"):
        ref = R.reference(NAMES.index(name))
        for tag in "gwd":
            assert not ref["smask_" + tag].any() and (ref["tmask_" + tag] == 1).all()
            assert float(ref["loss_" + tag]) == 0.0 and not ref["dflow_" + tag].any()
        assert (ref["tbrox"] == 1).all() and (ref["sbrox"] == 1).all()


def test_allout_gives_teacher_mask_zero_and_brox_occluded():
    for name in ("1x1x1-allout", "2x37x61-allout", "3x24x40in48x80-allout"):
        ref = R.reference(NAMES.index(name))
        for tag in "gwd":
            assert not ref["tmask_" + tag].any() and (ref["smask_" + tag] == 1).all() and float(ref["loss_" + tag]) == 0.0
        assert not ref["tbrox"].any() and not ref["sbrox"].any()
    # with r = 0 (what a warp beyond the image resamples) a pixel is occluded iff |f|^2 > 0.01 |f|^2 + 0.5, i.e. |f|^2 > 0.505...
    f = torch.zeros(1, 2, 4, 4, dtype=torch.float64)
    f[0, 0, 1, 1], f[0, 0, 2, 2], f[0, 1, 2, 2] = 0.71, 0.6, -0.39        # 0.5041 and 0.5121
    assert 0.71 ** 2 < 0.5 / 0.99 < 0.6 ** 2 + 0.39 ** 2
    vis = R.brox_mask(f, torch.zeros_like(f))
    assert vis[0, 1, 1] == 1 and vis[0, 2, 2] == 0 and vis.sum() == 15
    far = torch.full((1, 2, 4, 4), 9.0, dtype=torch.float64)              # beyond the image: r = 0 whatever the back flow holds
    assert not R.brox_mask(far, torch.full_like(far, -9.0)).any()


def test_constant_difference_without_masks():
    T = torch.zeros(2, 2, 5, 6, dtype=torch.float64)
    T[:, 0], T[:, 1] = 3.5, -1.0
    S = T - torch.tensor([3.0, 4.0], dtype=torch.float64).view(1, 2, 1, 1)
    loss, m = R.selfsup_parts(T, T, S, S, mask="none")
    assert (m == 1).all()
    assert abs(float(loss) - (math.sqrt(9 + 1e-6) + math.sqrt(16 + 1e-6)) / 2) < 1e-15


@pytest.mark.parametrize("name", ["3x24x40in48x80-consistent", "2x37x61-independent"])
def test_autograd_gradient_against_central_differences(name):
    c = case(name)
    T, Tb, Sb = (c[k].double().requires_grad_(True) for k in ("T", "Tb", "Sb"))
    S = c["S"].double().requires_grad_(True)
    st, ss = R.WIDE_SIGMAS
    loss, m = R.selfsup_parts(T, Tb, S, Sb, c["crop_yx"], "gaussian", st, ss)
    grads = torch.autograd.grad(loss, (S, T, Tb, Sb), allow_unused=True)
    assert grads[1] is None and grads[2] is None and grads[3] is None       # the teacher and the mask are stopped
    assert 0.0 < float(m.mean()) < 1.0
    # the mask is a constant of the differentiation (stop_gradient), so the differences are taken with it frozen
    Tc = R.crop(T.detach(), c["crop_yx"], c["H"], c["W"])

    def frozen(s):
        return float((m.unsqueeze(1) * ((Tc - s) ** 2 + 1e-6) ** 0.5).mean())

    g = torch.Generator().manual_seed(3)
    flat = S.detach().reshape(-1)
    for idx in torch.randint(0, flat.numel(), (40,), generator=g).tolist():
        h = 1e-6
        up, dn = flat.clone(), flat.clone()
        up[idx] += h
        dn[idx] -= h
        fd = (frozen(up.view_as(S)) - frozen(dn.view_as(S))) / (2 * h)
        assert abs(fd - float(grads[0].reshape(-1)[idx])) <= 1e-7 * float(grads[0].abs().max()) + 1e-12, idx
    # and it is the closed form the kernel writes: -m * d / sqrt(d^2 + 1e-6) / (2 B H W)
    d = Tc - S.detach()
    closed = -m.unsqueeze(1) * d / torch.sqrt(d ** 2 + 1e-6) / d.numel()
    assert torch.allclose(grads[0], closed, rtol=1e-12, atol=0)


def test_the_normaliser_is_the_teachers_size():
    c = case("3x24x40in48x80-consistent")
    T, Tb, S, Sb = (c[k].double() for k in ("T", "Tb", "S", "Sb"))
    st, ss = R.WIDE_SIGMAS
    _, m = R.selfsup_parts(T, Tb, S, Sb, c["crop_yx"], "gaussian", st, ss)
    sq, _, valid = R.fb_quantities(S, Sb)
    tsq, _, tvalid = R.fb_quantities(T, Tb)
    size = 48.0 ** 2 + 80.0 ** 2                                          # the frame, for the student's mask too
    student = 1.0 - torch.exp(-sq / (ss ** 2 * size)) * valid
    teacher = R.crop((torch.exp(-tsq / (st ** 2 * size)) * tvalid).unsqueeze(1), c["crop_yx"], 24, 40)[:, 0]
    assert torch.allclose(m, teacher * student, rtol=1e-13, atol=0)
    wrong = 1.0 - torch.exp(-sq / (ss ** 2 * (24.0 ** 2 + 40.0 ** 2))) * valid
    assert float((wrong - student).abs().max()) > 0.05


def test_ddflow_and_brox_differ_at_equality():
    # f = (9, 2) lands on an integer, where r is the back flow (-8, -1) itself: sq = 1 + 1, ss = 145 + 5, and
    # 0.01 * 150 + 0.5 rounds to 2 exactly, in float64 and in float32
    for dtype in (torch.float64, torch.float32):
        f = torch.zeros(1, 2, 16, 16, dtype=dtype)
        f[:, 0], f[:, 1] = 9.0, 2.0
        g = torch.zeros_like(f)
        g[:, 0], g[:, 1] = -8.0, -1.0
        sq, ss, valid = R.fb_quantities(f, g)
        assert valid[0, 3, 3] == 1 and sq[0, 3, 3] == 2 and ss[0, 3, 3] == 150 and R.threshold(ss)[0, 3, 3] == sq[0, 3, 3]
        assert R.fb_mask(f, g, "ddflow")[0, 3, 3] == 0                    # not strictly below: inconsistent
        assert R.brox_mask(f, g)[0, 3, 3] == 1                            # not strictly above: visible


def test_input_conditions_hold_for_every_gpu_case():
    assert [c["family"] for c in CASES[:5]] == list(R.FAMILIES) and len(CASES) == len(R.SHAPES) * len(R.FAMILIES)
    for c in CASES:
        assert R.input_conditions(c) == 0.0, c["name"]
        if c["family"] not in R.INTEGER_FAMILIES:
            assert not R.bad_pixels(c["T"], c["Tb"]).any() and not R.bad_pixels(c["S"], c["Sb"]).any()
    sc = R.sequence_case()
    for a, b in list(zip(sc["fw"], sc["bw"])) + list(zip(sc["bw"], sc["fw"])) + [sc["teacher"], sc["teacher"][::-1]]:
        assert not R.bad_pixels(a, b).any()


def test_both_outcomes_occur_and_the_wide_sigmas_open_the_teacher_mask():
    for name in NAMES:
        if name.split("-")[1] != "consistent" or case(name)["H"] < 24:
            continue
        ref = R.reference(NAMES.index(name))
        for key in ("tbrox", "sbrox", "tmask_d"):
            assert 0.02 < float(ref[key].mean()) < 0.98, (name, key)     # both sides of the threshold
        assert 0.1 < float(ref["tmask_w"].mean()) < 0.95, name
        assert 0.0 < float(ref["m_w"].mean()) < 1.0 and float(ref["loss_w"]) > 0
    small = R.reference(NAMES.index("2x37x61-consistent"))
    assert float(small["tmask_g"].mean()) < float(small["tmask_w"].mean())


def test_decisions_of_the_twin_are_those_of_the_reference():
    for i, c in enumerate(CASES):
        twin, ref = R.evaluate(c, torch.float32), R.reference(i)
        for key in R.DECISIONS:
            assert torch.equal(twin[key].double(), ref[key]), (c["name"], key)


def test_limits_are_finite_and_derived_from_the_twin():
    twin, lim = R.twin_errors(), R.limits()
    assert set(lim) == {"mask", "loss", "dflow", "sequence", "sequence_dflow"}
    for q, v in lim.items():
        assert math.isfinite(v) and v == R.FACTOR * twin[q] and twin[q] > 0, q
    assert R.FACTOR == 4.0
    assert lim["loss"] < 1e-5 and lim["sequence"] < 1e-5              # relative; a few fp32 roundings, not a tolerance


def test_sequence_reference_has_every_term():
    for occlusion in R.OCCLUSIONS:
        ref = R.reference_sequence(occlusion)
        assert set(ref["terms"]) == {"census", "smooth1", "smooth2", "selfsup"} and all(float(v) > 0 for v in ref["terms"].values())
        assert len(ref["grads"]) == 6 and all(float(g.abs().max()) > 0 for g in ref["grads"])
    assert float(R.reference_sequence("brox")["terms"]["census"]) != float(R.reference_sequence("wang")["terms"]["census"])
    # the teacher supervises every prediction: one single-prediction call per t, decayed, gives the sequence's term
    sc = R.sequence_case()
    frames, teacher = [t.double() for t in sc["frames"]], [t.double() for t in sc["teacher"]]
    singles = [R.smurf_loss(frames, [a.double()], [b.double()], teacher, sc["crop_yx"], sigmas=sc["sigmas"], **sc["weights"])[1]["selfsup"]
               for a, b in zip(sc["fw"], sc["bw"])]
    want = sum(0.8 ** (2 - t) * float(v.detach()) for t, v in enumerate(singles))
    assert abs(float(R.reference_sequence("wang")["terms"]["selfsup"]) - want) < 1e-12 * want
