"""Relative-position GMA attention (--position_only / --position_and_content) on the HIP path: routing, records, parity against
the reference-generated fixtures (tests/golden/make_golden_gma_pos.py) in both arithmetic modes, the torch-composed route as
comparator, and the memory the route was built to save.  Needs an MI355X: -m gpu.

Elementwise limits (POS_TOL).  The ops fixtures hold the reference run in float64 and the fp32 floor of every comparison (the
reference in float32 against itself in float64).  The limits started from the content-only ones of
test_gpu_parity.py::test_gma_attention_and_aggregate_vs_reference (2e-6 map / 2e-5 dctx / 2e-4 parameter gradients, times 8
under the split arithmetic, plus 2e-5 / 1e-3 of max|ref|), under which every comparison measured on MI355X used less than a fifth
of its limit.  The errors scale with the magnitude of the compared tensor (the probabilities of a peaked row, a gradient with a
large entry), so each limit is  atol + rtol * max|ref|  with rtol about 4x the worst  err / max|ref|  observed and atol a few
fp32 ulps of the smallest tensors, and never below the fixture's floor (`_close`).  All of them are tighter than their
content-only counterparts.  profiles/gma_pos_parity_margins.txt lists every comparison with the share of its limit it used.
Worst err / max|ref| observed, exact / split: map 2.2e-6 / 1.4e-5, dctx 4.9e-6 / 1.2e-5, dto_qk 5.2e-6 / 1.1e-5, table
gradients 1.3e-6 / 1.3e-5."""
import pytest
import torch

from _gma_pos import FLAGS, OPS_FIXTURES, P, attention_state, context_input, pos_ns, table_attention, with_embeddings
from _util import T, close, grad_digest_check, load, rel_check, shapes
from oracle import raft_torch as O
from oracle.weights import procedural_state_dict, rand_tensor, synthetic_pair

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (atol, rtol of max|ref|) of the attention map, dctx, the sampled dto_qk and the embedding-table gradients
POS_TOL = {"exact": dict(attn=(1e-7, 1e-5), dctx=(1e-7, 2e-5), dto_qk=(1e-6, 2e-5), drel=(1e-7, 1e-5)),
           "split": dict(attn=(1e-7, 6e-5), dctx=(1e-7, 5e-5), dto_qk=(1e-6, 4e-5), drel=(1e-7, 5e-5))}
# the train-step digests use test_gpu_parity.TRAIN_TOL unchanged
TRAIN_TOL = {"exact": dict(loss=5e-6, pred=5e-4, gnorm=1.5e-3, ghead=1e-2, gnorm_fnet=5e-3, ghead_fnet=3e-2),
             "split": dict(loss=3e-5, pred=1e-3, gnorm=1.5e-3, ghead=1.5e-2, gnorm_fnet=5e-3, ghead_fnet=3e-2)}


@pytest.fixture(params=["exact", "split"])
def precision(request):
    """The two arithmetic modes of the GEMM-shaped kernels (as test_gpu_parity.precision): exact fp32 MFMA, or bf16x3 products."""
    from flow_supervisor_amd import ops as _ops
    _ops.set_arithmetic(request.param == "split")
    yield request.param
    _ops.set_arithmetic(True)


@pytest.fixture
def pos_calls(monkeypatch):
    """Counts the launches of the positional softmax pair: a silent fall-back to the torch route must fail a test."""
    from flow_supervisor_amd import ops
    n = {"fwd": 0, "bwd": 0}
    fwd, bwd = ops.softmax_rows_pos_, ops.softmax_rows_pos_bwd_

    def cf(*a, **k):
        n["fwd"] += 1
        return fwd(*a, **k)

    def cb(*a, **k):
        n["bwd"] += 1
        return bwd(*a, **k)
    monkeypatch.setattr(ops, "softmax_rows_pos_", cf)
    monkeypatch.setattr(ops, "softmax_rows_pos_bwd_", cb)
    return n


def _close(a, b, tol, what, floor=0.0):
    """|a - b| <= max(atol + rtol * max|b|, floor) through _util.close (which logs the margin)."""
    ref = (b if isinstance(b, torch.Tensor) else T(b)).detach().abs().max().item()
    return close(a, b, max(tol[0] + tol[1] * ref, float(floor)), rtol=0.0, what=what)


def _attention(flag, sd=None):
    from flow_supervisor_amd.core.gma import Attention
    att = Attention(args=pos_ns(flag), dim=128, heads=1, max_pos_size=P, dim_head=128)
    if sd is not None:
        missing = att.load_state_dict(sd, strict=False)
        assert all(k.endswith("rel_ind") for k in missing.missing_keys) and not missing.unexpected_keys
    return att.to(DEV)


def _random_attention(flag, seed):
    att = _attention(flag)
    with torch.no_grad():
        att.to_qk.weight.copy_(rand_tensor(tuple(att.to_qk.weight.shape), seed, 0.08).to(DEV))
        att.pos_emb.rel_height.weight.copy_(rand_tensor((2 * P - 1, 128), seed + 5).to(DEV))
        att.pos_emb.rel_width.weight.copy_(rand_tensor((2 * P - 1, 128), seed + 6).to(DEV))
    return att


def _sample(gr):
    gr = gr.reshape(-1)
    return gr if gr.numel() <= 4096 else gr[:: gr.numel() // 4096][:4096]


def _params(att):
    return (att.to_qk.weight, att.pos_emb.rel_height.weight, att.pos_emb.rel_width.weight)


# ----------------------------------------------------------------------------- routing and records
@pytest.mark.parametrize("flag", list(FLAGS))
def test_positional_map_is_kept_once_as_records(flag, pos_calls):
    """Split arithmetic, 12 x 16 (N = 192): forward_cl(records=True) returns records written by the positional softmax itself,
    bit for bit ops.to_records of the dense-route map; the backward reads / writes records, with the gradient buffer handed over
    (`_fs_owned`) or foreign (copied, left untouched)."""
    from flow_supervisor_amd import ops
    from flow_supervisor_amd.core.gma import is_records
    assert ops.SPLIT_VOLUME_BWD
    B, H, W, seed = 2, 12, 16, 5150
    N = H * W
    att = _random_attention(flag, seed)
    x = torch.relu(rand_tensor((B, H, W, 128), seed + 1, 1.5)).to(DEV)
    G = rand_tensor((B, 1, N, N), seed + 2).to(DEV)
    res = {}
    for mode in ("dense", "records_owned", "records_foreign"):
        xa = x.clone().requires_grad_(True)
        for p in _params(att):
            p.grad = None
        before = dict(pos_calls)
        A = att.forward_cl(xa, records=mode != "dense")
        assert pos_calls["fwd"] == before["fwd"] + 1, "the positional softmax kernel did not run"
        assert is_records(A) == (mode != "dense") and tuple(A.shape) == (B, 1, N, N)
        g = G.clone()
        if mode == "records_owned":
            g._fs_owned = True
        A.backward(g)
        assert pos_calls["bwd"] == before["bwd"] + 1
        if mode == "records_foreign":
            assert torch.equal(g, G), "a gradient buffer that was not handed over must not be overwritten"
        res[mode] = (A.detach().clone(), xa.grad.clone()) + tuple(p.grad.clone() for p in _params(att))
    dense = ops.to_records(res["dense"][0].view(B, N, N))
    for mode in ("records_owned", "records_foreign"):
        assert torch.equal(res[mode][0].view(B, N, N).view(torch.int32), dense.view(torch.int32)), mode
        for got, ref, what in zip(res[mode][1:], res["dense"][1:], ("dx", "dto_qk", "drel_height", "drel_width")):
            err = (got - ref).abs().max().item()
            assert err <= 2e-5 * ref.abs().max().item() + 1e-9, (mode, what, err, ref.abs().max().item())
    # the dense map is the table formulation's
    with torch.no_grad():
        ref = table_attention({k: v.detach().cpu() for k, v in att.state_dict().items()}, x.permute(0, 3, 1, 2).cpu(), flag)
    _close(res["dense"][0], ref, POS_TOL["split"]["attn"], "dense map vs fp64 table formulation")
    if flag == "only":
        assert not res["dense"][2][128:].any(), "position_only: the k half of dto_qk is exactly zero"


@pytest.mark.parametrize("flag", list(FLAGS))
def test_shapes_outside_the_kernel_pair_take_the_old_route(flag, pos_calls):
    """N = 120 with records=True (dense kernels, still HIP), POS_HIP = False and rows over the LDS budget (torch route): dense,
    correct maps."""
    from flow_supervisor_amd import ops
    from flow_supervisor_amd.core import gma
    seed = 5250
    att = _random_attention(flag, seed)
    sd = {k: v.detach().cpu() for k, v in att.state_dict().items()}
    x = torch.relu(rand_tensor((2, 8, 15, 128), seed + 1, 1.5)).to(DEV)
    with torch.no_grad():
        A = att.forward_cl(x, records=True)                    # N = 120: not a multiple of 32 -> the dense positional kernel
        assert not gma.is_records(A) and pos_calls["fwd"] == 1
        _close(A, table_attention(sd, x.permute(0, 3, 1, 2).cpu(), flag), POS_TOL["split"]["attn"], "N = 120")
        x16 = torch.relu(rand_tensor((2, 8, 16, 128), seed + 2, 1.5)).to(DEV)
        old = gma.POS_HIP
        try:
            gma.POS_HIP = False
            A = att.forward_cl(x16, records=True)
        finally:
            gma.POS_HIP = old
        assert not gma.is_records(A) and pos_calls["fwd"] == 1, "POS_HIP = False is the torch route"
        _close(A, table_attention(sd, x16.permute(0, 3, 1, 2).cpu(), flag), POS_TOL["split"]["attn"], "POS_HIP off")
        H, W = 64, 128                                         # 8 * 8192 + 4 * 192 > 65520
        assert not ops.softmax_rows_pos_fits(H, W)
        xb = torch.relu(rand_tensor((1, H, W, 128), seed + 3, 1.5)).to(DEV)
        A = att.forward_cl(xb, records=True)
        assert not gma.is_records(A) and pos_calls["fwd"] == 1, "rows over the LDS budget are the torch route"
        assert tuple(A.shape) == (1, 1, H * W, H * W)
        rows = torch.tensor([0, 127, 4000, H * W - 1])
        ref = table_attention_rows(sd, xb.permute(0, 3, 1, 2).cpu(), flag, rows)
        _close(A[0, 0, rows.to(DEV)], ref, POS_TOL["split"]["attn"], "over the LDS budget")
    with pytest.raises(ValueError, match="max_pos_size is 160"):
        att.forward_cl(torch.zeros(1, 2, 161, 128, device=DEV))


def table_attention_rows(sd, ctx, flag, rows):
    """_gma_pos.table_attention for a few query rows of one sample (the full map of a 64 x 128 grid is 0.5 GB in fp64)."""
    B, C, h, w = ctx.shape
    assert B == 1
    Wqk = sd["to_qk.weight"].double()[:, :, 0, 0]
    D = Wqk.shape[0] // 2
    s = D ** -0.5
    x = ctx.double().permute(0, 2, 3, 1).reshape(h * w, C)
    q, k = x[rows] @ Wqk[:D].T, x @ Wqk[D:].T
    Tb = torch.cat([sd["pos_emb.rel_height.weight"].double()[P - h:P + h - 1], sd["pos_emb.rel_width.weight"].double()[P - w:P + w - 1]])
    G = s * q @ Tb.T
    j = torch.arange(h * w)
    col_h = (j // w)[None, :] - (rows // w)[:, None] + h - 1
    col_w = (2 * h - 1) + (j % w)[None, :] - (rows % w)[:, None] + w - 1
    S = torch.gather(G, 1, col_h) + torch.gather(G, 1, col_w)
    if FLAGS[flag]["position_and_content"]:
        S = s * q @ k.T + S
    return S.softmax(-1)


# ----------------------------------------------------------------------------- parity vs the reference fixtures
@pytest.mark.parametrize("name", OPS_FIXTURES)
def test_positional_attention_vs_reference(name, precision, pos_calls):
    """Attention map and the gradients of sum(attn * R) against the reference's Attention (float64 run): 12 x 16 and 9 x 15
    (N = 135: the dense kernels' scalar tails), both flags, through the reference API (NCHW, dense map)."""
    g = load(name)
    flag = name.rsplit("_", 1)[1]
    tol = POS_TOL[precision]
    att = _attention(flag, attention_state(g))
    assert {k: list(v.shape) for k, v in att.state_dict().items() if not k.endswith("rel_ind")} == shapes("gma_pos_ops")
    seed, H, W = int(g["seed"]), int(g["H"]), int(g["W"])
    ctx = context_input(g).to(DEV).requires_grad_(True)
    A = att(ctx)
    assert pos_calls["fwd"] == 1 and tuple(A.shape) == tuple(g["attn"].shape)
    _close(A, g["attn"], tol["attn"], f"{name} attention", g["floor.attn"])
    (A * rand_tensor(tuple(A.shape), seed + 3).to(DEV)).sum().backward()
    assert pos_calls["bwd"] == 1
    _close(ctx.grad, g["dctx"], tol["dctx"], f"{name} dctx", g["floor.dctx"])
    _close(_sample(att.to_qk.weight.grad), g["dparam.att.to_qk.weight"], tol["dto_qk"], f"{name} dto_qk", g["floor.dto_qk"])
    if flag == "only":
        assert float(g["dto_qk_k_half_absmax"]) == 0.0 and not att.to_qk.weight.grad[128:].any(), "k half of dto_qk: exactly zero"
    for axis, n in (("height", H), ("width", W)):
        gr = getattr(att.pos_emb, "rel_" + axis).weight.grad
        _close(gr[P - n:P + n - 1], g["drel_" + axis], tol["drel"], f"{name} drel_{axis}", g["floor.drel_" + axis])
        outside = gr.clone()
        outside[P - n:P + n - 1] = 0
        assert not outside.any(), "table rows the grid does not index have a zero gradient"


def _pos_model(flag, g):
    from flow_supervisor_amd.core.gma_network import RAFTGMA
    seed = int(g["seed"])
    m = RAFTGMA(pos_ns(flag))
    sd = with_embeddings(procedural_state_dict(shapes("raft_gma"), seed), float(g["emb_scale"]), seed)
    missing = m.load_state_dict(sd, strict=False)
    assert all(k.endswith("rel_ind") for k in missing.missing_keys) and not missing.unexpected_keys
    with torch.no_grad():
        m.update_block.aggregator.gamma.fill_(float(g["gamma"]))
    return m.to(DEV)


@pytest.mark.parametrize("flag", list(FLAGS))
def test_positional_gma_train_step_vs_reference(flag, precision, pos_calls):
    """RAFTGMA with the flag, one pair at 128 x 192 (16 x 24, N = 384), 4 iterations, gamma = 0.1: loss, predictions and every
    parameter-gradient digest -- the pos_emb tables included -- against the reference's train step."""
    g = load(f"train_step_gma_pos_small_{flag}")
    m = _pos_model(flag, g).train()
    m.freeze_bn()
    im1, im2 = (t.to(DEV) for t in synthetic_pair(1, int(g["H"]), int(g["W"]), int(g["seed"]) + 1))
    preds = m(im1, im2, iters=int(g["iters"]))
    tol = TRAIN_TOL[precision]
    loss = O.sequence_loss_zero_gt(preds)
    rel_check(loss.item(), g["loss"], tol["loss"], f"{flag} loss")
    loss.backward()
    assert pos_calls == {"fwd": 1, "bwd": 1}
    s = int(g["stride"])
    close(preds[0][:, :, ::s, ::s], g["first"], tol["pred"], rtol=0.0, what=f"{flag} first prediction")
    close(preds[-1][:, :, ::s, ::s], g["last"], tol["pred"], rtol=0.0, what=f"{flag} last prediction")
    assert float(g["gnorm.att.pos_emb.rel_height.weight"]) > 0 and m.att.pos_emb.rel_width.weight.grad is not None
    bad = grad_digest_check(m.named_parameters(), g, tol)
    assert not bad, bad[:8]


def test_positional_gma_at_bench_scale_epe(precision, pos_calls):
    """440 x 1024 (55 x 128, N = 7040), --position_and_content, 12 iterations in test mode: EPE against the reference under the
    project's gate of 1e-3 (BASELINE.json)."""
    g = load("e2e_gma_pos_440x1024_both")
    s = int(g["stride"])
    m = _pos_model("both", g).eval()
    im1, im2 = (t.to(DEV) for t in synthetic_pair(1, int(g["H"]), int(g["W"]), int(g["seed"]) + 1))
    with torch.no_grad():
        low, up = m(im1, im2, iters=int(g["iters"]), test_mode=True)
    assert pos_calls["fwd"] == 1
    e_low = O.epe(low.cpu(), T(g["flow_low"])).item()
    e_up = O.epe(up[:, :, ::s, ::s].cpu(), T(g["flow_up_strided"])).item()
    print("gma positional 440x1024", precision, "EPE low", e_low, "EPE up", e_up)
    assert e_low <= 1e-3 and e_up <= 1e-3, (e_low, e_up)


# ----------------------------------------------------------------------------- the old route as comparator, memory
def _fwd_bwd(att, x, dA, records):
    """forward_cl + backward of one attention call; returns (dense map or None, dx, parameter gradients)."""
    xa = x.clone().requires_grad_(True)
    for p in _params(att):
        p.grad = None
    A = att.forward_cl(xa, records=records)
    dense = None if records else A.detach().clone()
    g = dA.clone()
    g._fs_owned = True
    A.backward(g)
    del A, g
    return dense, xa.grad, tuple(None if p.grad is None else p.grad.clone() for p in _params(att))


@pytest.mark.parametrize("flag", list(FLAGS))
def test_hip_route_agrees_with_the_torch_route_at_bench_shape(flag, precision, pos_calls):
    """55 x 128, B = 1, POS_HIP toggled in one process: map and all gradients within the limits of the reference comparisons."""
    from flow_supervisor_amd.core import gma
    tol = POS_TOL[precision]
    H, W, seed = 55, 128, 5350
    N = H * W
    att = _random_attention(flag, seed)
    x = torch.relu(rand_tensor((1, H, W, 128), seed + 1, 1.5)).to(DEV)
    dA = rand_tensor((1, 1, N, N), seed + 2).to(DEV)
    A1, dx1, gp1 = _fwd_bwd(att, x, dA, False)
    assert pos_calls == {"fwd": 1, "bwd": 1}
    old = gma.POS_HIP
    try:
        gma.POS_HIP = False
        A0, dx0, gp0 = _fwd_bwd(att, x, dA, False)
    finally:
        gma.POS_HIP = old
    assert pos_calls == {"fwd": 1, "bwd": 1}
    _close(A1, A0, tol["attn"], f"{flag} map, HIP vs torch route")
    _close(dx1, dx0, tol["dctx"], f"{flag} dx, HIP vs torch route")
    _close(gp1[0], gp0[0], tol["dto_qk"], f"{flag} dto_qk, HIP vs torch route")
    _close(gp1[1], gp0[1], tol["drel"], f"{flag} drel_height, HIP vs torch route")
    _close(gp1[2], gp0[2], tol["drel"], f"{flag} drel_width, HIP vs torch route")


def _peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


@pytest.mark.parametrize("flag", list(FLAGS))
def test_positional_route_keeps_the_content_only_memory(flag, pos_calls):
    """Peak allocated bytes over forward + backward at 55 x 128, B = 1, records=True: at most the content-only HIP path's peak
    (measured here, same inputs) + G and dG (2 * B * N * ldg * 4) + the table + 16 MB of allocator slack.  The torch-composed
    route holds several 198 MB [N, N] intermediates and exceeds that limit -- asserted too: it is what the kernels bought."""
    from flow_supervisor_amd import ops
    from flow_supervisor_amd.core import gma
    assert ops.SPLIT_VOLUME_BWD
    B, H, W, seed = 1, 55, 128, 5450
    N = H * W
    ldg = (2 * H + 2 * W - 2 + 3) & ~3
    att = _random_attention(flag, seed)
    from flow_supervisor_amd.core.gma import Attention
    import argparse
    plain = Attention(args=argparse.Namespace(position_only=False, position_and_content=False), dim=128, heads=1, max_pos_size=P,
                      dim_head=128).to(DEV)
    plain.load_state_dict(att.state_dict())
    x = torch.relu(rand_tensor((B, H, W, 128), seed + 1, 1.5)).to(DEV)
    dA = rand_tensor((B, 1, N, N), seed + 2).to(DEV)
    for a in (plain, att):                                   # warm-up: code objects, weight packs
        _fwd_bwd(a, x, dA, True)
    content_only = _peak(lambda: _fwd_bwd(plain, x, dA, True))
    calls = dict(pos_calls)
    hip = _peak(lambda: _fwd_bwd(att, x, dA, True))
    assert pos_calls == {"fwd": calls["fwd"] + 1, "bwd": calls["bwd"] + 1}
    limit = content_only + 2 * B * N * ldg * 4 + ldg * 128 * 4 + (16 << 20)
    old = gma.POS_HIP
    try:
        gma.POS_HIP = False
        torch_route = _peak(lambda: _fwd_bwd(att, x, dA, True))
    finally:
        gma.POS_HIP = old
    print(f"peak bytes {flag}: content-only {content_only / 2**20:.1f} MB, positional HIP {hip / 2**20:.1f} MB, "
          f"limit {limit / 2**20:.1f} MB, torch route {torch_route / 2**20:.1f} MB")
    assert hip <= limit, (hip, limit)
    assert torch_route > limit, (torch_route, limit)
