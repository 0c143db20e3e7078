"""coords.grad through the public lookups -- core.corr.CorrBlock (NCHW and channels_last outputs, coordinates and flows, a block
built under no_grad) and raft_tf.CorrBlock (a differentiable and a detached pyramid) -- against the float64 restatement of
tests/_dcoordsref.py on the very volume the block holds (corr_pyramid), within _dcoordsref.LIMITS; one backward that needs the
feature-map and the coordinate gradients, whose feature-map gradients are bit for bit those of the same graph with detached
coordinates; detached coordinates never reach the new ops functions (one RAFT forward / backward with them patched to raise);
AlternateCorrBlock keeps giving the coordinates no gradient.  Needs an MI355X: -m gpu.
"""
import argparse

import pytest
import torch

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
    g = torch.Generator().manual_seed(920 + seed)
    f1, f2 = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    return f1.to(DEV).requires_grad_(requires_grad), f2.to(DEV).requires_grad_(requires_grad)


def _positions():
    return R.coords_values(B, H, W, "mixed")


def _check(what, grad, levels, pos, dout_nhwc, radius):
    """grad [B,2,H,W] (device) against the restatement on `levels` (device tensors [Q,1,h,w])."""
    lv = [t.detach().cpu()[:, 0] for t in levels]
    _, dc, S = R.expect(lv, pos, dout_nhwc.cpu(), radius)
    w, i = R.need(grad.detach().cpu(), dc, (S * R.U24).expand_as(dc))
    _log_margin(what, w, R.LIMITS["dcoords"], "worst |got - ref| / (2^-24 S)")
    print(f"{what}: {w:.3f} units of 2^-24 S (limit {R.LIMITS['dcoords']})")
    assert w <= R.LIMITS["dcoords"], (what, w, i)
    assert bool((grad[:, :, 0] == 0).all()), "the +-1e6 row must get exactly 0"


@pytest.mark.parametrize("radius", R.RADII)
@pytest.mark.parametrize("is_flow", (False, True))
@pytest.mark.parametrize("channels_last", (False, True))
def test_corrblock_coords_grad(channels_last, is_flow, radius):
    from flow_supervisor_amd.core.corr import CorrBlock
    f1, f2 = _fmaps(True)
    blk = CorrBlock(f1, f2, num_levels=4, radius=radius)
    pos = _positions()
    given = pos - R.grid(B, H, W) if is_flow else pos           # (exact: multiples of 1/64 and +-1e6 less a small integer)
    assert torch.equal(given + R.grid(B, H, W), pos) if is_flow else given is pos
    c = given.to(DEV).requires_grad_()
    out = blk(c, channels_last=channels_last, is_flow=is_flow)
    assert out.grad_fn is not None
    dout = R.dout_values(B, H, W, 4, radius, "gauss")
    out.backward(dout.to(DEV) if channels_last else dout.permute(0, 3, 1, 2).contiguous().to(DEV))
    assert c.grad is not None and f1.grad is not None and f2.grad is not None
    _check(f"CorrBlock cl{int(channels_last)} flow{int(is_flow)} r{radius}", c.grad, blk.corr_pyramid, pos, dout, radius)


@pytest.mark.parametrize("with_out", (False, True))
def test_block_built_under_no_grad_gives_the_coordinate_gradient(with_out):
    from flow_supervisor_amd.core.corr import CorrBlock
    f1, f2 = _fmaps(True)
    with torch.no_grad():
        blk = CorrBlock(f1, f2)
    pos = _positions()
    c = pos.to(DEV).requires_grad_()
    buf = torch.empty(B, H, W, 324, device=DEV) if with_out else None
    out = blk(c, channels_last=with_out, out=buf) if with_out else blk(c)
    assert out.grad_fn is not None, "only the coordinates require grad: the output must still be differentiable"
    dout = R.dout_values(B, H, W, 4, 4, "gauss")
    out.backward(dout.to(DEV) if with_out else dout.permute(0, 3, 1, 2).contiguous().to(DEV))
    assert f1.grad is None and f2.grad is None
    _check(f"CorrBlock built under no_grad out{int(with_out)}", c.grad, blk.corr_pyramid, pos, dout, 4)
    with torch.no_grad():                                         # and nothing is recorded where nothing is asked for
        assert blk(c).grad_fn is None
    assert blk(c.detach()).grad_fn is None


@pytest.mark.parametrize("pyramid_grad", (True, False))
def test_tf_corrblock_coords_grad(pyramid_grad):
    from flow_supervisor_amd import raft_tf
    f1, f2 = _fmaps(pyramid_grad)
    pyr = raft_tf.calc_all_field(f1.permute(0, 2, 3, 1), f2.permute(0, 2, 3, 1), num_pool=3)
    assert pyr[0].requires_grad == pyramid_grad
    pos = _positions()
    c = pos.permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_()
    out = raft_tf.CorrBlock(4, 4)(pyr, c)
    assert out.grad_fn is not None
    dout = R.dout_values(B, H, W, 4, 4, "gauss")
    out.backward(dout.to(DEV))
    assert (f1.grad is not None) == pyramid_grad
    levels = [lv.reshape(B * H * W, 1, lv.shape[-2], lv.shape[-1]) for lv in pyr]
    _check(f"raft_tf.CorrBlock pyramid grad {int(pyramid_grad)}", c.grad.permute(0, 3, 1, 2), levels, pos, dout, 4)


def test_feature_gradients_do_not_change_when_the_coordinates_take_one():
    from flow_supervisor_amd.core.corr import CorrBlock
    pos = _positions()
    dout = R.dout_values(B, H, W, 4, 4, "gauss").to(DEV)
    grads = []
    for coords_grad in (False, True):
        f1, f2 = _fmaps(True)
        blk = CorrBlock(f1, f2)
        c = pos.to(DEV).requires_grad_(coords_grad)
        flow = (pos - R.grid(B, H, W)).to(DEV).requires_grad_(coords_grad)
        (blk(c, channels_last=True) * dout).sum().add((blk(flow, channels_last=True, is_flow=True) * dout).sum()).backward()
        assert (c.grad is not None) == coords_grad and (flow.grad is not None) == coords_grad
        if coords_grad:
            assert torch.equal(c.grad, flow.grad)                 # the gradient w.r.t. the flow is the gradient w.r.t. the coordinates
        grads.append((f1.grad.clone(), f2.grad.clone()))
    for a, b in zip(*grads):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_detached_coordinates_never_reach_the_new_functions(monkeypatch):
    from flow_supervisor_amd import ops
    from flow_supervisor_amd.core.raft import RAFT

    def refuse(*a, **k):
        raise AssertionError("the coordinate gradient was asked for by a loop that detaches its coordinates")
    monkeypatch.setattr(ops, "corr_lookup_tiled_dcoords", refuse)
    monkeypatch.setattr(ops, "corr_lookup_dcoords", refuse)
    torch.manual_seed(7)
    model = RAFT(argparse.Namespace(small=False, mixed_precision=False, alternate_corr=False)).to(DEV).train()
    model.freeze_bn()
    im1 = torch.rand(1, 3, 64, 96, device=DEV) * 255
    im2 = torch.rand(1, 3, 64, 96, device=DEV) * 255
    preds = model(im1, im2, iters=2)
    sum(p.abs().mean() for p in preds).backward()
    g = next(model.fnet.parameters()).grad                        # (reached through the volume backward)
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0


def test_alternate_corrblock_keeps_giving_the_coordinates_no_gradient():
    from flow_supervisor_amd.core.corr import AlternateCorrBlock
    pos = _positions()
    f1, f2 = _fmaps(True)
    c = pos.to(DEV).requires_grad_()
    out = AlternateCorrBlock(f1, f2)(c)
    assert out.grad_fn is not None
    out.sum().backward()
    assert c.grad is None and f1.grad is not None
    g1, g2 = _fmaps(False)
    assert AlternateCorrBlock(g1, g2)(c).grad_fn is None          # only the coordinates require grad: no node, as before
