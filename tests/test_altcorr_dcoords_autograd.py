"""coords.grad through core.corr.AlternateCorrBlock(coords_grad=True) -- NCHW and channels_last outputs, coordinates and flows,
with and without out=, a block built under no_grad or from maps without grad -- against the float64 restatement of
tests/_altdcoordsref.py on the very maps the block holds (blk.pyramid[l][1], channels-last), within _altdcoordsref.LIMITS; one
backward that needs the feature-map and the coordinate gradients: the feature backward is handed the same bits as by the same
graph with detached coordinates and its results are the same bits (a coords_grad=True block adds in a fixed order); the default (coords_grad=False) keeps giving the
coordinates no gradient; a RAFT step on the alt path with alt_coords_grad=True and the loop's detached coordinates never reaches
ops.altcorr_fused_dcoords; and the lookup with its backward to coords.grad allocates far less than the N x N volume it never
forms.  Needs an MI355X: -m gpu.
"""
import argparse

import pytest
import torch

import _altdcoordsref as A
import _dcoordsref as R
from _util import _log_margin

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, C, H, W = 2, 32, 16, 24


@pytest.fixture(scope="module", autouse=True)
def _leave_no_cached_segments():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def _fmaps(requires_grad, seed=0):
    g = torch.Generator().manual_seed(1920 + seed)
    f1, f2 = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    return f1.to(DEV).requires_grad_(requires_grad), f2.to(DEV).requires_grad_(requires_grad)


def _positions():
    return R.coords_values(B, H, W, "mixed")


def _check(what, grad, blk, pos, dout_nhwc, radius):
    """grad [B,2,H,W] (device) against the restatement on the maps `blk` holds."""
    f1 = blk.pyramid[0][0].detach().cpu().permute(0, 2, 3, 1).contiguous()
    f2 = [blk.pyramid[l][1].detach().cpu().permute(0, 2, 3, 1).contiguous() for l in range(blk.num_levels)]
    dc, S = A.expect(f1, f2, pos, dout_nhwc.cpu(), radius)
    w, i = R.need(grad.detach().cpu(), dc, (S * A.U24).expand_as(dc))
    _log_margin(what, w, A.LIMITS["dcoords"], "worst |got - ref| / (2^-24 S)")
    print(f"{what}: {w:.3f} units of 2^-24 S (limit {A.LIMITS['dcoords']})")
    assert w <= A.LIMITS["dcoords"], (what, w, i)
    assert bool((grad[:, :, 0] == 0).all()), "the +-1e6 row must get exactly 0"


@pytest.mark.parametrize("radius", R.RADII)
@pytest.mark.parametrize("is_flow", (False, True))
@pytest.mark.parametrize("channels_last", (False, True))
def test_alternate_corrblock_coords_grad(channels_last, is_flow, radius):
    from flow_supervisor_amd.core.corr import AlternateCorrBlock
    f1, f2 = _fmaps(True)
    blk = AlternateCorrBlock(f1, f2, num_levels=4, radius=radius, coords_grad=True)
    pos = _positions()
    given = pos - R.grid(B, H, W) if is_flow else pos           # (exact: multiples of 1/64 and +-1e6 less a small integer)
    assert torch.equal(given + R.grid(B, H, W), pos) if is_flow else given is pos
    c = given.to(DEV).requires_grad_()
    out = blk(c, channels_last=channels_last, is_flow=is_flow)
    assert out.grad_fn is not None
    dout = R.dout_values(B, H, W, 4, radius, "gauss")
    out.backward(dout.to(DEV) if channels_last else dout.permute(0, 3, 1, 2).contiguous().to(DEV))
    assert c.grad is not None and f1.grad is not None and f2.grad is not None
    _check(f"AlternateCorrBlock cl{int(channels_last)} flow{int(is_flow)} r{radius}", c.grad, blk, pos, dout, radius)


@pytest.mark.parametrize("radius", R.RADII)
def test_coords_grad_with_an_out_buffer(radius):
    from flow_supervisor_amd.core.corr import AlternateCorrBlock
    f1, f2 = _fmaps(True)
    blk = AlternateCorrBlock(f1, f2, radius=radius, coords_grad=True)
    pos = _positions()
    c = pos.to(DEV).requires_grad_()
    buf = torch.empty(B, H, W, 4 * (2 * radius + 1) ** 2, device=DEV)
    out = blk(c, channels_last=True, out=buf)
    assert out.grad_fn is not None and out.data_ptr() == buf.data_ptr()
    dout = R.dout_values(B, H, W, 4, radius, "gauss")
    out.backward(dout.to(DEV))
    assert f1.grad is not None
    _check(f"AlternateCorrBlock out= r{radius}", c.grad, blk, pos, dout, radius)


@pytest.mark.parametrize("with_out", (False, True))
@pytest.mark.parametrize("how", ("no_grad", "maps_without_grad"))
def test_block_without_feature_gradients_gives_the_coordinate_gradient(how, with_out):
    from flow_supervisor_amd.core.corr import AlternateCorrBlock
    f1, f2 = _fmaps(how == "no_grad")
    if how == "no_grad":
        with torch.no_grad():
            blk = AlternateCorrBlock(f1, f2, coords_grad=True)
    else:
        blk = AlternateCorrBlock(f1, f2, coords_grad=True)
    pos = _positions()
    c = pos.to(DEV).requires_grad_()
    buf = torch.empty(B, H, W, 324, device=DEV) if with_out else None
    out = blk(c, channels_last=True, out=buf) if with_out else blk(c)
    assert out.grad_fn is not None, "only the coordinates require grad: the output must still be differentiable"
    dout = R.dout_values(B, H, W, 4, 4, "gauss")
    out.backward(dout.to(DEV) if with_out else dout.permute(0, 3, 1, 2).contiguous().to(DEV))
    assert f1.grad is None and f2.grad is None
    _check(f"AlternateCorrBlock {how} out{int(with_out)}", c.grad, blk, pos, dout, 4)
    with torch.no_grad():                                         # and nothing is recorded where nothing is asked for
        assert blk(c).grad_fn is None
    assert blk(c.detach()).grad_fn is None


def _two_lookups_backward(coords_grad):
    """One backward through a coordinate lookup and a flow lookup of one block: (f1.grad, f2.grad, c.grad, flow.grad)."""
    from flow_supervisor_amd.core.corr import AlternateCorrBlock
    pos = _positions()
    dout = R.dout_values(B, H, W, 4, 4, "gauss").to(DEV)
    f1, f2 = _fmaps(True)
    blk = AlternateCorrBlock(f1, f2, coords_grad=True)
    c = pos.to(DEV).requires_grad_(coords_grad)
    flow = (pos - R.grid(B, H, W)).to(DEV).requires_grad_(coords_grad)
    (blk(c, channels_last=True) * dout).sum().add((blk(flow, channels_last=True, is_flow=True) * dout).sum()).backward()
    assert (c.grad is not None) == coords_grad and (flow.grad is not None) == coords_grad
    return f1.grad.clone(), f2.grad.clone(), c.grad, flow.grad


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_the_gradient_in_the_flow_is_the_gradient_in_the_coordinates():
    _, _, gc, gf = _two_lookups_backward(True)
    assert _same_bits(gc, gf) and float(gc.abs().max()) > 0


def test_the_feature_backward_is_handed_the_same_bits_when_the_coordinates_take_a_gradient(monkeypatch):
    """What the lookups contribute to the feature gradients is the (coords, dOut) list they hand to ops.corr_bwd_chunked: bit for
    bit the same whether or not the coordinates take a gradient."""
    from flow_supervisor_amd import ops
    seen, chunked = [], ops.corr_bwd_chunked

    def spy(fmap1, fmap2, douts, coords, *a, **k):
        seen.append((fmap1, fmap2, list(douts), list(coords), a, k))
        return chunked(fmap1, fmap2, douts, coords, *a, **k)
    monkeypatch.setattr(ops, "corr_bwd_chunked", spy)
    for coords_grad in (False, True):
        _two_lookups_backward(coords_grad)
    (a1, a2, ad, ac, aa, ak), (b1, b2, bd, bc, ba, bk) = seen
    assert len(ad) == len(bd) == 2 and len(ac) == len(bc) == 2 and aa == ba and ak == bk
    assert not any(t.requires_grad for t in bd + bc)
    for x, y in zip([a1, a2] + ad + ac, [b1, b2] + bd + bc):
        assert _same_bits(x, y)


def test_feature_gradients_do_not_change_when_the_coordinates_take_one():
    """f1.grad / f2.grad of the same graph with and without coordinate gradients, bit for bit.  This needs the feature backward of
    a coords_grad=True block to add in a fixed order (ops.corr_bwd_chunked(fixed_order=True)): the default block's adds the
    k-slices of its two record GEMMs with fp32 atomics as they arrive, and two backward passes of one and the same graph then
    differ in the last bit (measured at this shape on a default block, coordinates detached: 2222 .. 6901 of the 24576 elements
    of either gradient, by at most 9.5e-7)."""
    grads = [_two_lookups_backward(coords_grad)[:2] for coords_grad in (False, True)]
    for a, b in zip(*grads):
        print(f"{int((a.view(torch.int32) != b.view(torch.int32)).sum())} of {a.numel()} elements differ, by at most {float((a - b).abs().max()):.2e}")
    for a, b in zip(*grads):
        assert _same_bits(a, b)


def test_the_default_keeps_giving_the_coordinates_no_gradient(monkeypatch):
    from flow_supervisor_amd import ops
    from flow_supervisor_amd.core.corr import AlternateCorrBlock

    def refuse(*a, **k):
        raise AssertionError("coords_grad=False reached the coordinate gradient")
    monkeypatch.setattr(ops, "altcorr_fused_dcoords", refuse)
    pos = _positions()
    f1, f2 = _fmaps(True)
    c = pos.to(DEV).requires_grad_()
    blk = AlternateCorrBlock(f1, f2, coords_grad=False)
    assert blk.coords_grad is False and AlternateCorrBlock(f1, f2).coords_grad is False
    out = blk(c)
    assert out.grad_fn is not None
    out.sum().backward()
    assert c.grad is None and f1.grad is not None
    g1, g2 = _fmaps(False)
    assert AlternateCorrBlock(g1, g2)(c).grad_fn is None          # only the coordinates require grad: no node, as before


def test_detached_coordinates_never_reach_the_new_function(monkeypatch):
    from flow_supervisor_amd import ops
    from flow_supervisor_amd.core.raft import RAFT

    def refuse(*a, **k):
        raise AssertionError("the coordinate gradient was asked for by a loop that detaches its coordinates")
    monkeypatch.setattr(ops, "altcorr_fused_dcoords", refuse)
    torch.manual_seed(7)
    model = RAFT(argparse.Namespace(small=False, mixed_precision=False, alternate_corr=True, alt_coords_grad=True)).to(DEV).train()
    model.freeze_bn()
    im1 = torch.rand(1, 3, 128, 192, device=DEV) * 255            # (the alt block pools once more than it has levels: 16 x 24 maps)
    im2 = torch.rand(1, 3, 128, 192, device=DEV) * 255
    preds = model(im1, im2, iters=2)
    sum(p.abs().mean() for p in preds).backward()
    g = next(model.fnet.parameters()).grad                        # (reached through the chunked feature backward)
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0


def test_no_volume_is_formed():
    """1 x 32 x 32 x 48, N = 1536: the lookup and its backward to coords.grad may raise the peak by out, dout and the like (under
    3 MB), never by the level-0 volume's N^2 4 bytes = 9.4 MB."""
    from flow_supervisor_amd.core.corr import AlternateCorrBlock
    h, w = 32, 48
    N = h * w
    g = torch.Generator().manual_seed(5)
    f1, f2 = torch.randn(1, C, h, w, generator=g).to(DEV), torch.randn(1, C, h, w, generator=g).to(DEV)
    blk = AlternateCorrBlock(f1, f2, coords_grad=True)
    c = (R.grid(1, h, w) + torch.randn(1, 2, h, w, generator=g)).to(DEV).requires_grad_()
    dout = torch.randn(1, h, w, 324, generator=g).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    blk(c, channels_last=True).backward(dout)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise {rise / 1e6:.2f} MB; the level-0 volume would be {N * N * 4 / 1e6:.2f} MB")
    assert c.grad is not None and bool(torch.isfinite(c.grad).all()) and float(c.grad.abs().max()) > 0
    assert rise < N * N * 4, rise
