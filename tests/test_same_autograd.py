"""raft_tf.calc_all_field / build_pyramid / CorrBlock on TensorFlow 'SAME' pyramids with raft_tf.same_grad() on, against the float64
chain of tests/_samebwdref.py at _corrref.CHAIN (2x13x22, C = 64: both sizes odd at some level; levels 13x22, 7x11, 4x6, 2x3): the
gradients w.r.t. both feature maps through calc_all_field(num_pool=3) -> CorrBlock(4, 4) -> a gaussian cotangent ('SAME' scatter ->
unpool_same_bwd -> _corrbwdref.volume_bwd of the one level), bounded by the sum of the stages' bounds, each carried through the stages
after it; coords.grad against the float64 Jacobian on the very pyramid the call holds, attached and detached; the gradient of
build_pyramid(transpose_volume(volume), 3) w.r.t. the volume; with the switch off the same calls raise "forward-only"; a floor-sized
call (1x8x16) gives bit-identical gradients with the switch on and off.  Needs an MI355X: -m gpu.

Worst values measured on MI355X:
  chain dF1 / dF2                      0.0036 / 0.0038  limit 1  (shares of the summed bound; the GEMMs' bf16x3 term is most of it)
  the 'SAME' pyramid the chain built   0.028            limit 1  (level 1; a share of the build's and the pooling's bounds)
  coords.grad, attached / detached     0.78 / 0.78      limit 8  (units of 2^-24 S)
  build_pyramid gradient               2.44             limit 20 (units of 2^-24 S; one coarse level alone: 1.33)
  bit for bit: the floor-sized call with the switch on and off.
On the parent commit every test here fails: raft_tf.same_grad does not exist.
"""
import pytest
import torch

import _corrbwdref as B
import _corrref as R
import _dcoordsref as D
import _samebwdref as M
from _util import _log_margin

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _leave_no_cached_segments():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


@pytest.fixture()
def tf():
    from flow_supervisor_amd import raft_tf
    from flow_supervisor_amd.raft_tf import api
    assert api._SAME_GRAD is False
    yield raft_tf
    api._SAME_GRAD = False


def _bounded(what, got, ref, bound):
    w, i = M.need(got.detach().cpu().reshape(ref.shape), ref, bound)
    _log_margin(what, w, 1.0, "worst |got - ref| / bound")
    print(f"{what}: {w:.4f} of its bound")
    assert w <= 1.0, (what, w, i)


def _in_units(what, got, ref, S, key):
    w, i = M.need(got.detach().cpu().reshape(ref.shape), ref, S * M.U24)
    _log_margin(what, w, M.LIMITS[key], "worst |got - ref| / (2^-24 S)")
    print(f"{what}: {w:.3f} units of 2^-24 S (limit {M.LIMITS[key]:g})")
    assert w <= M.LIMITS[key], (what, w, i)


def _maps(c, requires_grad):
    return (c["f1"].permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_(requires_grad),
            c["f2"].permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_(requires_grad))


def test_feature_map_gradients_through_a_same_pyramid(tf):
    (Bn, H, W), nlev, C = M.CHAIN
    c = M.chain_case()
    a, b = _maps(c, True)
    coords = c["pos"].permute(0, 2, 3, 1).contiguous().to(DEV)
    with tf.same_grad():
        pyr = tf.calc_all_field(a, b, num_pool=nlev - 1)
        assert [tuple(lv.shape[-2:]) for lv in pyr] == M.same_sizes(H, W, nlev) and all(lv.requires_grad for lv in pyr)
        out = tf.CorrBlock(nlev, M.CHAIN_RADIUS)(pyr, coords)
        out.backward(c["dout"].to(DEV))
    torch.cuda.synchronize()
    d1 = a.grad.permute(0, 3, 1, 2).reshape(Bn, C, H * W)
    d2 = b.grad.reshape(Bn, H * W, C)
    # the float64 chain and the bound
    f1, f2l = c["f1"], B.f2cat(c["f2"], 1)
    dv0 = M.unpool_same_bwd(c["dlev"])
    ref1, ref2 = B.volume_bwd(f1, f2l, [dv0])
    e_lev = [M.LIMITS["lookup_bwd_same.cl"] * M.U24 * S for S in c["S"]]                   # (channels-last dout: the cl kernels)
    S_un = M.unpool_same_bwd([g.abs() + e for g, e in zip(c["dlev"], e_lev)])
    e_dv0 = M.unpool_same_bwd(e_lev) + M.LIMITS["unpool_same"] * M.U24 * S_un
    af1, af2l = f1.abs(), [f2l[0].abs()]
    a1, a2 = B.volume_bwd(af1, af2l, [e_dv0])
    S1, S2 = B.volume_bwd(af1, af2l, [dv0.abs() + e_dv0])
    gemm = R.LIMITS["build.split"] * R.G16         # both GEMMs: at most hi hi + hi lo + lo hi with fp32 accumulation, as the build
    assert bool(torch.isfinite(d1).all()) and bool(torch.isfinite(d2).all())
    _bounded("same chain dF1", d1, ref1, a1 + gemm * S1)
    _bounded("same chain dF2", d2, ref2, a2 + gemm * S2)
    # the forward the gradient belongs to: the pyramid is the 'SAME' pooling of the volume
    ref_pyr, S_pyr = c["pyr"], R.pool_same(R.volume0(f1.abs(), c["f2"].abs()), nlev)
    for l in range(1, nlev):
        bound = (R.LIMITS["build.split"] * R.G16 + R.LIMITS["pool_same"] * M.U24) * S_pyr[l]
        _bounded(f"same chain pyramid level {l}", pyr[l].reshape(Bn * H * W, *pyr[l].shape[-2:]), ref_pyr[l], bound)


@pytest.mark.parametrize("pyramid_grad", (True, False))
def test_coords_grad_on_a_same_pyramid(tf, pyramid_grad):
    (Bn, H, W), nlev, C = M.CHAIN
    c = M.chain_case()
    a, b = _maps(c, pyramid_grad)
    coords = c["pos"].permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_()
    with tf.same_grad():
        pyr = tf.calc_all_field(a, b, num_pool=nlev - 1)
        assert pyr[0].requires_grad == pyramid_grad
        out = tf.CorrBlock(nlev, M.CHAIN_RADIUS)(pyr, coords)
        assert out.grad_fn is not None
        out.backward(c["dout"].to(DEV))
    assert (a.grad is not None) == pyramid_grad
    levels = [lv.detach().cpu().reshape(Bn * H * W, *lv.shape[-2:]) for lv in pyr]
    _, dc, S = D.expect(levels, c["pos"], c["dout"], M.CHAIN_RADIUS)
    got = coords.grad.permute(0, 3, 1, 2)
    _in_units(f"same coords.grad, pyramid grad {int(pyramid_grad)}", got, dc, S.expand_as(dc), "dcoords_same")
    assert bool((got[:, :, 0] == 0).all()), "the +-1e6 row must get exactly 0"


def test_build_pyramid_gradient_on_a_same_shape(tf):
    (Bn, H, W), nlev, C = M.CHAIN
    c = M.chain_case()
    a, b = _maps(c, False)
    vol = tf.transpose_volume(tf.calc_all_field(a, b, num_pool=0)[0]).detach().requires_grad_()
    rows = Bn * H * W
    cot = M.unpool_values((rows, H, W), nlev)
    before = [g.clone() for g in cot]
    with tf.same_grad():
        lv = tf.build_pyramid(vol, nlev - 1)
        assert [tuple(t.shape[-2:]) for t in lv] == M.same_sizes(H, W, nlev)
        torch.autograd.backward(lv, [g.view(Bn, H, W, *g.shape[1:]).to(DEV) for g in cot])
    _in_units("same build_pyramid dvolume", vol.grad.reshape(rows, H, W), M.unpool_same_bwd(cot), M.unpool_same_bwd(cot, absolute=True), "unpool_same")
    assert all(torch.equal(x, y) for x, y in zip(before, cot))
    # only a coarse level takes a cotangent: the others count as zero
    vol.grad = None
    with tf.same_grad():
        tf.build_pyramid(vol, nlev - 1)[2].backward(cot[2].view(Bn, H, W, *cot[2].shape[1:]).to(DEV))
    only = [torch.zeros_like(g) if l != 2 else g for l, g in enumerate(cot)]
    _in_units("same build_pyramid dvolume, level 2 only", vol.grad.reshape(rows, H, W), M.unpool_same_bwd(only), M.unpool_same_bwd(only, absolute=True),
              "unpool_same")


def test_switch_off_the_same_calls_raise(tf):
    (Bn, H, W), nlev, C = M.CHAIN
    c = M.chain_case()
    a, b = _maps(c, True)
    with pytest.raises(RuntimeError, match="forward-only"):
        tf.calc_all_field(a, b, num_pool=nlev - 1)
    pyr = tf.calc_all_field(a.detach(), b.detach(), num_pool=nlev - 1)
    with pytest.raises(RuntimeError, match="forward-only"):
        tf.build_pyramid(tf.transpose_volume(pyr[0]).requires_grad_(), nlev - 1)
    coords = c["pos"].permute(0, 2, 3, 1).contiguous().to(DEV)
    with pytest.raises(RuntimeError, match="forward-only"):
        tf.CorrBlock(nlev, M.CHAIN_RADIUS)([lv.clone().requires_grad_() for lv in pyr], coords)
    with tf.same_grad():                       # and with it on, nothing is recorded where nothing is asked for
        assert tf.CorrBlock(nlev, M.CHAIN_RADIUS)(pyr, coords).grad_fn is None
        with torch.no_grad():
            assert tf.calc_all_field(a, b, num_pool=nlev - 1)[1].grad_fn is None


def test_floor_sized_gradients_do_not_depend_on_the_switch(tf):
    Bn, H, W, C = 1, 8, 16, 32
    g = D._gen("floor_switch", Bn, H, W, C)
    f1, f2 = torch.randn(Bn, H, W, C, generator=g), torch.randn(Bn, H, W, C, generator=g)
    pos = D.coords_values(Bn, H, W, "mixed").permute(0, 2, 3, 1).contiguous()
    dout = D.dout_values(Bn, H, W, 4, 4, "gauss").to(DEV)
    grads = []
    for on in (False, True):
        tf.same_grad(on)
        a, b, coords = f1.to(DEV).requires_grad_(), f2.to(DEV).requires_grad_(), pos.to(DEV).requires_grad_()
        pyr = tf.calc_all_field(a, b, num_pool=3)
        assert [tuple(lv.shape[-2:]) for lv in pyr] == [(8, 16), (4, 8), (2, 4), (1, 2)]
        out = tf.CorrBlock(4, 4)(pyr, coords)
        lv = tf.build_pyramid(tf.transpose_volume(pyr[0]), 3)
        (out * dout).sum().add(sum(t.sum() * (l + 1) for l, t in enumerate(lv))).backward()
        grads.append((out.detach().clone(), a.grad.clone(), b.grad.clone(), coords.grad.clone()))
    for x, y in zip(*grads):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
