"""tests/_gmaref.py on the CPU: the float64 restatements against torch and autograd, the record codec, and -- for every case of
the lists tests/test_gma_kernels.py runs on the GPU -- that the comparator accepts the fp32 twin (the same formula in torch
float32) under the committed limits and rejects every applicable mutant, each limit being at most a quarter of the smallest
deviation a mutant produces on the case's designed rows."""
import pytest
import torch

import _gmaref as R

U24 = R.U24


# ------------------------------------------------------------------------------------------------------------ restatements
@pytest.mark.parametrize("n", (1, 5, 257, 1030))
def test_restatements_equal_torch_and_autograd(n):
    x, _ = R.logit_rows(n)
    xd = x.double().requires_grad_(True)
    A = torch.softmax(xd, -1)
    assert (R.softmax_ref(x) - A.detach()).abs().max().item() <= 4 * 2.0 ** -53
    _, dA, _ = R.bwd_rows(n)
    A.backward(dA.double())
    ref = R.softmax_bwd_ref(A.detach(), dA)
    assert (ref - xd.grad).abs().max().item() <= 64 * 2.0 ** -53 * dA.abs().max().item()


def test_mix_restatements_equal_autograd():
    M, C = 7, 12
    d, y, dx0 = R.mix_inputs(M, C)
    x = dx0.double().requires_grad_(True)
    yd = y.double().requires_grad_(True)
    g = torch.tensor(R.GAMMA, dtype=torch.float64, requires_grad=True)
    out = x + g * yd
    assert torch.equal(out.detach(), R.mix_fwd_ref(dx0, y, R.GAMMA))
    out.backward(d.double())
    dx, dy, dg = R.mix_bwd_ref(d, y, R.GAMMA, torch.zeros(M, C), 0.0)
    assert torch.equal(dx, x.grad) and torch.equal(dy, yd.grad)
    assert abs(dg - g.grad.item()) <= 1e-12 * (d * y).abs().sum().item()
    dx, _, dg1 = R.mix_bwd_ref(d, y, R.GAMMA, dx0, R.DGAMMA0)
    assert torch.equal(dx, dx0.double() + d.double()) and dg1 == R.DGAMMA0 + dg


# ------------------------------------------------------------------------------------------------------------------ records
def test_record_codec():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(5, 96, generator=g) * torch.exp(8 * torch.randn(5, 96, generator=g))
    x[0, :4] = torch.tensor([0.0, 1.0, -2.0 ** -100, 3.0e38])
    t = R.records_encode(x)
    assert t.shape == x.shape and t.dtype == torch.float32 and R.records_wellformed(t)
    back = R.records_decode(t)
    # hi keeps 8 significant bits, so |x - hi| <= 2^-8 |x|; lo keeps 8 bits of that: half an ulp of lo is at most 2^-17 |x|.
    # (2^-18 does not hold: uniform values on [1, 2) reach 2^-17.003.)
    assert ((back - x.double()).abs() <= 2.0 ** -17 * x.double().abs()).all()
    u = torch.rand(64, 1024, generator=g) + 1.0
    rel = ((R.records_decode(R.records_encode(u)) - u.double()).abs() / u.double()).max().item()
    assert 2.0 ** -18 < rel <= 2.0 ** -17
    # the layout of ops.to_records: per 32 columns 32 bf16 hi, then 32 bf16 lo
    b = t.view(torch.bfloat16).view(5, 3, 64)
    assert torch.equal(b[:, :, :32].reshape(5, 96), x.bfloat16())
    # a value of the form hi + lo is encoded exactly, bits included
    again = R.records_encode(back.float())
    assert torch.equal(again.view(torch.int32), t.view(torch.int32)) and torch.equal(R.records_decode(again), back)
    # the swapped container decodes to the same sums: only the order test sees it
    sw = R.records_swapped(t)
    assert torch.equal(R.records_decode(sw), back) and not R.records_wellformed(sw)


# ---------------------------------------------------------------------------------------- twins and mutants, softmax forward
def _fwd_case(n, records):
    x, names = R.logit_rows(n)
    ref = R.softmax_ref(x)
    scale, slack = R.fwd_scale(x, ref, records)
    return x, names, ref, scale, slack


def _quarter(limit, devs, what):
    """limit <= a quarter of the smallest mutant deviation (each the worst over the designed rows)."""
    assert devs, what
    name, dev = min(devs.items(), key=lambda kv: kv[1])
    assert limit <= dev / 4, (what, name, dev, limit)


@pytest.mark.parametrize("n", R.FWD_N)
def test_forward_twin_accepted_mutants_rejected(n):
    x, names, ref, scale, slack = _fwd_case(n, False)
    a = R.LIMITS["fwd_a"]
    twin = R.softmax_twin(x)
    got, i = R.need(twin, ref, scale, slack)
    assert got <= a, (n, names[i // n], got)
    assert ((twin.double().sum(-1) - 1).abs() <= n * U24).all()
    muts = R.fwd_mutants(n)
    assert set(muts) >= ({"normaliser misses last"} if n >= 2 else set())
    devs = {k: R.need(f(x)[1:], ref[1:], scale[1:], slack[1:])[0] for k, f in muts.items()}
    assert all(v > a for v in devs.values()), devs
    if devs:
        _quarter(a, devs, f"forward n = {n}")
        # the all-equal row alone: one dropped column moves every probability by 1 / n relative (6.1e-5 at n = 16388)
        eq = names.index("equal")
        one = R.need(muts["normaliser misses last"](x)[eq], ref[eq], scale[eq], slack[eq])[0]
        assert a <= one / 4 and abs(one * U24 * (n - 1) - 1) < 1e-3, (n, one)


@pytest.mark.parametrize("n", R.REC_FWD_N)
def test_record_forward_twin_accepted_mutants_rejected(n):
    x, names, ref, scale, slack = _fwd_case(n, True)
    a = R.LIMITS["fwd_a"]
    rec = R.records_encode(R.softmax_twin(x))
    got, i = R.need(R.records_decode(rec), ref, scale, slack)
    assert got <= a and R.records_wellformed(rec), (n, names[i // n], got)
    assert not R.records_wellformed(R.records_swapped(rec)), "hi and lo exchanged"
    devs = {k: R.need(R.records_decode(R.records_encode(f(x).float()))[1:], ref[1:], scale[1:], slack[1:])[0]
            for k, f in R.fwd_mutants(n).items()}
    if n > 2048:
        devs["second stride left as logits"] = R.need(R.records_decode(R.records_second_stride_left(rec, x))[1:], ref[1:], scale[1:],
                                                      slack[1:])[0]
    assert all(v > a for v in devs.values()), devs
    _quarter(a, devs, f"record forward n = {n}")


# --------------------------------------------------------------------------------------- twins and mutants, softmax backward
@pytest.mark.parametrize("n", R.BWD_N)
def test_backward_twin_accepted_mutants_rejected(n):
    A, dA, names = R.bwd_rows(n)
    ref = R.softmax_bwd_ref(A, dA)
    scale, slack = R.bwd_scale(A, dA, ref)
    k = R.LIMITS["bwd"]
    got, i = R.need(R.softmax_bwd_twin(A, dA), ref, scale, slack)
    assert got <= k, (n, names[i // n], got)
    devs = {m: R.need(f(A, dA)[1:], ref[1:], scale[1:], slack[1:])[0] for m, f in R.bwd_mutants(n).items()}
    assert all(v > k for v in devs.values()), devs
    _quarter(k, devs, f"backward n = {n}")


@pytest.mark.parametrize("n", R.REC_BWD_N)
def test_record_backward_twin_accepted_mutants_rejected(n):
    A0, dA, names = R.bwd_rows(n)
    Ar = R.records_encode(A0)
    A = R.records_decode(Ar)                                   # what the kernel reads: hi + lo, exact in fp32
    ref = R.softmax_bwd_ref(A, dA)
    scale, slack = R.bwd_scale(A, dA, ref, True)
    k = R.LIMITS["rec_bwd"]
    rec = R.records_encode(R.softmax_bwd_twin(A, dA))
    got, i = R.need(R.records_decode(rec), ref, scale, slack)
    assert got <= k and R.records_wellformed(rec), (n, names[i // n], got)
    assert not R.records_wellformed(R.records_swapped(rec))
    devs = {m: R.need(R.records_decode(R.records_encode(f(A, dA).float()))[1:], ref[1:], scale[1:], slack[1:])[0]
            for m, f in R.bwd_mutants(n).items()}
    if n > 2048:
        devs["second stride left as dA"] = R.need(R.records_decode(R.records_second_stride_left(rec, dA))[1:], ref[1:], scale[1:],
                                                  slack[1:])[0]
    assert all(v > k for v in devs.values()), devs
    _quarter(k, devs, f"record backward n = {n}")


# ------------------------------------------------------------------------------------------------------------------------ mix
@pytest.mark.parametrize("cfg", R.MIX_FWD)
def test_mix_forward_twin_accepted(cfg):
    M, C = cfg[:2]
    x, y, _ = R.mix_inputs(M, C)
    ref = R.mix_fwd_ref(x, y, R.GAMMA)
    g = torch.tensor(R.GAMMA)
    scale = 2 * U24 * (x.double().abs() + (float(g) * y.double()).abs())
    assert R.need(x + g * y, R.mix_fwd_ref(x, y, g), scale)[0] <= 1.0
    assert R.need(x + y, ref, scale)[0] > 4.0, "gamma ignored"


@pytest.mark.parametrize("cfg", R.MIX_BWD)
def test_mix_backward_twin_accepted_mutants_rejected(cfg):
    M, C = cfg[:2]
    d, y, dx0 = R.mix_inputs(M, C)
    g = torch.tensor(R.GAMMA)
    dx, dy, dg = R.mix_bwd_ref(d, y, g, dx0, R.DGAMMA0)
    sdx, sdg = U24 * dx.abs(), U24 * float((d.double() * y.double()).abs().sum())
    k = R.LIMITS["dgamma"]
    assert R.need(dx0 + d, dx, sdx)[0] <= 1.0
    assert R.need(g * d, dy, U24 * dy.abs())[0] <= 1.0          # (the kernel's dy is this fp32 product, bit for bit)
    twin = (torch.tensor(R.DGAMMA0) + (d * y).sum()).item()
    assert abs(twin - dg) <= k * sdg, (abs(twin - dg) / sdg, k)
    muts = R.mix_bwd_mutants()
    mdx = R.need(muts["dx not accumulated"](d, y, g, dx0, R.DGAMMA0)[0], dx, sdx)[0]
    mdg = abs(muts["dgamma overwritten"](d, y, g, dx0, R.DGAMMA0)[2] - dg) / sdg
    assert 1.0 <= mdx / 4 and k <= mdg / 4, (mdx, mdg)


def test_case_lists_cover_every_route_edge():
    """Both sides of the LDS / big threshold, the scalar path, the second record stride and the record bounds are in the lists."""
    def ceil4(n):
        return (n + 3) & ~3
    for last, ns, per in ((R.FWD_LDS_LAST, R.FWD_N, 4), (R.BWD_LDS_LAST, R.BWD_N, 8)):
        assert last in ns and last + 1 in ns and per * ceil4(last) + 16 <= 65536 < per * ceil4(last + 1) + 16
    assert any(n % 4 and n > 1024 for n in R.FWD_N) and any(n % 4 and n > 1024 for n in R.BWD_N)
    assert 2080 in R.REC_FWD_N and 2080 in R.REC_BWD_N and 2080 // 8 > 256
    assert max(R.REC_FWD_N) == 16352 and max(R.REC_BWD_N) == 8160
    M, C = R.MIX_FWD[-1][:2]
    assert M * C // 4 > 4096 * 256
    M, C = R.MIX_BWD[-1][:2]
    assert M * C // 4 > 512 * 256
