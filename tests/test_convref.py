"""CPU checks of the fp64 convolution reference and of the comparator tests/test_conv_routes.py holds the HIP kernels to:
the reference against torch's float64 convolution and autograd, the epilogue restatements, the arithmetic twins, the packed
K layout, and the comparator's detection power on the two mutants (no GPU needed)."""
import pytest
import torch
import torch.nn.functional as F

import _convref as R


def _srcs(B, H, W, Cs, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, H, W, C, generator=g, dtype=torch.float64) for C in Cs]


def _nchw(xs):
    return torch.cat(xs, -1).permute(0, 3, 1, 2)


def _torch_conv(xs, w, pad):
    KH, KW = w.shape[2:]
    PH, PW = pad
    x = F.pad(_nchw(xs), (PW, KW - 1 - PW, PH, KH - 1 - PH))
    return F.conv2d(x, w).permute(0, 2, 3, 1).reshape(-1, w.shape[0])


@pytest.mark.parametrize("Cs,KH,KW,pad", [([37], 3, 3, (1, 1)), ([128, 96, 2], 3, 3, (1, 1)), ([20, 45], 1, 5, (0, 2)),
                                          ([33], 5, 1, (2, 0)), ([12], 2, 2, (1, 1)), ([12], 2, 2, (0, 0)), ([70], 1, 1, (0, 0))])
def test_reference_gemm_is_torch_conv2d_in_fp64(Cs, KH, KW, pad):
    B, H, W, N = 2, 5, 7, 11
    xs = _srcs(B, H, W, Cs, 1)
    w = torch.randn(N, sum(Cs), KH, KW, dtype=torch.float64)
    rows = torch.arange(B * H * W)
    got = R.conv_gemm(xs, w, B, H, W, pad, rows)
    torch.testing.assert_close(got, _torch_conv(xs, w, pad), rtol=1e-12, atol=1e-12)
    some = torch.tensor([0, 6, 34, B * H * W - 1])        # a row subset is the same rows of the whole
    torch.testing.assert_close(R.conv_gemm(xs, w, B, H, W, pad, some), got[some], rtol=1e-12, atol=1e-12)
    assert (R.conv_gemm(xs, w, B, H, W, pad, rows, "abs") >= got.abs() - 1e-12).all()


@pytest.mark.parametrize("KH,KW,pad", [(3, 3, (1, 1)), (1, 5, (0, 2)), (2, 2, (1, 1))])
def test_data_gradient_restatement_is_autograd(KH, KW, pad):
    """Flipped packs (modes 1 / 11) with padding (KH-1-PH, KW-1-PW): the data gradient of the forward convolution."""
    B, H, W, Cin, N = 2, 6, 5, 9, 7
    x = torch.randn(B, Cin, H, W, dtype=torch.float64, requires_grad=True)
    w = torch.randn(N, Cin, KH, KW, dtype=torch.float64)
    y = F.conv2d(F.pad(x, (pad[1], KW - 1 - pad[1], pad[0], KH - 1 - pad[0])), w)
    gy = torch.randn_like(y)
    y.backward(gy)
    dpad = (KH - 1 - pad[0], KW - 1 - pad[1])
    got = R.conv_gemm([gy.permute(0, 2, 3, 1)], R.dgrad_weight(w), B, H, W, dpad, torch.arange(B * H * W))
    torch.testing.assert_close(got, x.grad.permute(0, 2, 3, 1).reshape(-1, Cin), rtol=1e-12, atol=1e-12)


def test_weight_gradient_restatement_is_autograd_over_segments():
    B, H, W, KH, KW, Cs, N = 2, 5, 6, 3, 3, [5, 40], 8
    w = torch.randn(N, sum(Cs), KH, KW, dtype=torch.float64, requires_grad=True)
    dys, xss = [], []
    for seg in range(3):
        xs = _srcs(B, H, W, Cs, 10 + seg)
        y = F.conv2d(_nchw(xs), w, padding=1)
        gy = torch.randn_like(y)
        (y * gy).sum().backward()
        dys.append(gy.permute(0, 2, 3, 1))
        xss.append(xs)
    got = R.wgrad_gemm(dys, xss, B, H, W, KH, KW)
    torch.testing.assert_close(got, w.grad, rtol=1e-12, atol=1e-12)
    for mode in ("fp32", "bf16x1", "bf16x3"):
        assert (R.wgrad_gemm(dys, xss, B, H, W, KH, KW, mode) - got).abs().max() < 0.05 * got.abs().max()


def test_packed_k_layout_round_trip():
    """Per source: taps x 32-padded channels; padding columns stay zero and the gather inverts the scatter."""
    srcC = [37, 2, 64]
    idx, ktot = R.packed_k_index(srcC, 1, 5)
    assert ktot == 5 * (64 + 32 + 64)
    assert idx[0, 0] == 0 and idx[1, 0] == 64 and idx[0, 37] == 5 * 64 and idx[0, 39] == 5 * 64 + 5 * 32
    w = torch.randn(6, sum(srcC), 1, 5)
    pk = R.pack_ref(w, srcC)
    assert torch.equal(R.unpack_ref(pk, srcC, 1, 5), w)
    assert int((pk != 0).sum()) == w.numel()


def test_epilogue_restatements_are_one_conv_gru_step():
    """EPI_ZR / EPI_Q of two convolutions = the ConvGRU cell (z, r = sigmoid(conv[h, x]); q = tanh(conv[r h, x]);
    h' = (1 - z) h + z q) with the context addend `pre`."""
    B, H, W, hid, cx = 1, 4, 5, 6, 3
    h = torch.tanh(torch.randn(B, H, W, hid, dtype=torch.float64))
    x = torch.randn(B, H, W, cx, dtype=torch.float64)
    wzr = torch.randn(2 * hid, hid + cx, 3, 3, dtype=torch.float64) * 0.2
    wq = torch.randn(hid, hid + cx, 3, 3, dtype=torch.float64) * 0.2
    bzr, bq = torch.randn(2 * hid, dtype=torch.float64), torch.randn(hid, dtype=torch.float64)
    pzr, pq = torch.randn(B * H * W, 2 * hid, dtype=torch.float64), torch.randn(B * H * W, hid, dtype=torch.float64)
    rows = torch.arange(B * H * W)
    G = R.conv_gemm([h, x], wzr, B, H, W, (1, 1), rows)
    zr = R.Epi(2, bias=bzr, pre=pzr, h=h.reshape(-1, hid), hid=hid).apply(G, torch.zeros_like(G))
    a = torch.sigmoid(_torch_conv([h, x], wzr, (1, 1)) + bzr + pzr)
    torch.testing.assert_close(zr["z"][0], a[:, :hid])
    torch.testing.assert_close(zr["r"][0], a[:, hid:])
    torch.testing.assert_close(zr["rh"][0], a[:, hid:] * h.reshape(-1, hid))
    rh = zr["rh"][0].reshape(B, H, W, hid)
    Gq = R.conv_gemm([rh, x], wq, B, H, W, (1, 1), rows)
    qo = R.Epi(3, bias=bq, pre=pq, h=h.reshape(-1, hid), z=zr["z"][0]).apply(Gq, torch.zeros_like(Gq))
    q = torch.tanh(_torch_conv([rh, x], wq, (1, 1)) + bq + pq)
    torch.testing.assert_close(qo["q"][0], q)
    torch.testing.assert_close(qo["hn"][0], (1 - a[:, :hid]) * h.reshape(-1, hid) + a[:, :hid] * q)


def test_plain_epilogue_destinations_accumulate_mask_relu():
    G = torch.tensor([[1.0, -2.0, 3.0, -4.0, 5.0]], dtype=torch.float64)
    old = torch.full((1, 2), 10.0, dtype=torch.float64)
    mask = torch.tensor([[1.0, -1.0]], dtype=torch.float64)
    out = R.Epi(0, bias=torch.ones(5, dtype=torch.float64), alpha=2.0, relu=True,
                dsts=((0, None, mask), (3, old, None))).apply(G, torch.zeros_like(G))
    assert out["dst0"][0].tolist() == [[4.0, 0.0, 8.0]]       # (G + 1) * 2, ReLU, column 1 masked
    assert out["dst1"][0].tolist() == [[10.0, 22.0]]          # ReLU(-6) + 10, 12 + 10


def test_twins_order_their_errors():
    """bf16x3 is ~2^-16 relative per product, bf16x1 ~2^-8: their errors against fp64 are ~2^8 apart."""
    B, H, W = 2, 8, 8
    xs = [x.float() for x in _srcs(B, H, W, [64], 3)]
    w = torch.randn(32, 64, 3, 3) / 24
    rows = torch.arange(B * H * W)
    G = R.conv_gemm(xs, w, B, H, W, (1, 1), rows)
    e = {m: R.frob(R.conv_gemm(xs, w, B, H, W, (1, 1), rows, m), G) for m in ("fp32", "bf16x3", "bf16x1")}
    assert e["bf16x1"] > 100 * e["bf16x3"] > 0
    assert e["bf16x3"] > 2 * e["fp32"] > 0
    hi, lo = R.bf16_hi_lo(w.double())
    assert ((hi + lo - w.double()).abs() <= 2.0 ** -16 * w.double().abs()).all()


def _case(Cs, KH, KW, N, B, H, W, epi_kind=0, seed=5):
    xs = [x.float() for x in _srcs(B, H, W, Cs, seed)]
    w = (torch.randn(N, sum(Cs), KH, KW, generator=torch.Generator().manual_seed(seed + 1)) / (sum(Cs) * KH * KW) ** 0.5)
    pad = (KH // 2, KW // 2)
    M = B * H * W
    rows = torch.arange(M)
    G = R.conv_gemm(xs, w, B, H, W, pad, rows)
    S = R.conv_gemm(xs, w, B, H, W, pad, rows, "abs")
    twins = {m: R.conv_gemm(xs, w, B, H, W, pad, rows, m) for m in ("fp32", "bf16x3", "bf16x1")}
    last = R.last_tile_rows(rows, M)
    mut = G.clone()
    mut[last] -= R.chunk_contribution(xs, w, B, H, W, pad, rows[last], 0, KH * KW // 2, 0)
    hid = N // 2
    h = torch.tanh(torch.randn(M, N, dtype=torch.float64))
    if epi_kind == 2:
        epi = R.Epi(2, bias=torch.randn(N) * 0.1, pre=torch.randn(M, N), h=h, hid=hid)
    elif epi_kind == 3:
        epi = R.Epi(3, bias=torch.randn(N) * 0.1, pre=torch.randn(M, N), h=h, z=torch.rand(M, N, dtype=torch.float64))
    else:
        epi = R.Epi(0, bias=torch.randn(N) * 0.1, relu=True)
    K = KH * KW * sum(Cs)
    return epi, G, S, K, twins, mut


@pytest.mark.parametrize("Cs,KH,KW,N,epi_kind", [([70], 3, 3, 40, 0), ([128, 96], 3, 3, 36, 2), ([256], 1, 5, 20, 3),
                                                 ([37, 4, 9], 5, 1, 100, 0)])
def test_comparator_accepts_each_arithmetic_and_rejects_both_mutants(Cs, KH, KW, N, epi_kind):
    """A kernel whose error is its arithmetic's passes; mutant (a) -- one 32-channel chunk of one tap dropped in the last,
    ragged M tile -- and mutant (b) -- the bf16x1 twin -- are rejected.  In exact mode a bf16x3 result is rejected too
    (what 'exact mode silently ran the split core' would look like), at these K."""
    B, H, W = 1, 9, 11                         # M = 99: the last 64-pixel tile is ragged
    epi, G, S, K, twins, mut = _case(Cs, KH, KW, N, B, H, W, epi_kind)
    outs = epi.apply(G, torch.zeros_like(G))
    for arith in ("fp32", "bf16x3"):
        got = {k: epi.apply(twins[arith], torch.zeros_like(G))[k][0] for k in outs}
        ok, rejected, rep = R.verdict(got, epi, G, S, K, arith, twins, mut)
        assert ok, (arith, rep)
        assert rejected, arith
    got = {k: epi.apply(twins["bf16x3"], torch.zeros_like(G))[k][0] for k in outs}
    assert not R.verdict(got, epi, G, S, K, "fp32", twins, mut)[0]
    # a structural error outside the last tile (wrong output column) is an elementwise failure, too
    bad = G.clone()
    bad[3, N - 1] = G[3, N - 2]
    got = {k: epi.apply(bad, torch.zeros_like(G))[k][0] for k in outs}
    assert not R.verdict(got, epi, G, S, K, "bf16x3", twins, mut)[0]


def test_sampled_rows_cover_borders_tile_edges_and_the_last_tile():
    B, H, W = 2, 40, 50
    rows = R.sample_rows(B, H, W, 100, tile=64)
    s = set(rows.tolist())
    M = B * H * W
    assert {0, M - 1, 63, 64, 127, 128, W - 1, W, H * W - 1, H * W}.issubset(s)
    assert all(m in s for m in range((M - 1) // 64 * 64, M))
    assert rows.numel() < M and torch.equal(rows, torch.unique(rows))
    assert torch.equal(R.sample_rows(1, 3, 5, 100), torch.arange(15))
