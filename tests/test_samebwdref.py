"""tests/_samebwdref.py checked on the CPU: the float64 un-pooling of the 'SAME' pyramid is the transpose of _corrref.pool_same (torch's
own derivative of it), cells nothing reaches are exactly 0, it equals the floor un-pooling where the two pyramids agree, the 'SAME'
scatter and coordinate gradient are the transposes / derivatives of _corrref.lookup on ceil-sized levels, the limits are those the
fp32 twins give, and raft_tf.same_grad is a switch that is off by default.  No GPU."""
import pytest
import torch

import _corrbwdref as B
import _corrref as R
import _dcoordsref as D
import _samebwdref as M


def _pool_same_grad(shape, nlev, cot):
    """torch.autograd.grad of <pool_same(x)_l, cot_l> summed over l >= 1, w.r.t. x."""
    x = torch.randn(*shape, dtype=torch.float64, generator=D._gen("adj", *shape)).requires_grad_()
    lv = R.pool_same(x, nlev)
    (g,) = torch.autograd.grad(sum((a * c.double()).sum() for a, c in zip(lv[1:], cot[1:])), x)
    return g


@pytest.mark.parametrize("shape,nlev", [(s, n) for s, n, _ in M.UNPOOL_CASES if n > 1] + [((2, 13, 22), 4), ((1, 46, 96), 4), ((1, 7, 5), 8)])
def test_unpool_same_bwd_is_the_transpose_of_pool_same(shape, nlev):
    cot = M.unpool_values(shape, nlev)
    got = M.unpool_same_bwd(cot) - cot[0].double()
    ref = _pool_same_grad(shape, nlev, cot)
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


def test_a_cell_with_zero_scale_is_exactly_zero():
    shape, nlev = (3, 9, 11), 4
    lv = [t.clone() for t in M.unpool_values(shape, nlev)]
    lv[0][1] = 0
    for l in range(1, nlev):
        lv[l][1] = 0                     # row 1: nothing anywhere
        lv[l][2, 0, 0] = 0               # row 2: the windows of cell (0, 0) at every level
    lv[0][2, 0, 0] = 0
    for dtype in (torch.float64, torch.float32):
        out, S = M.unpool_same_bwd(lv, dtype), M.unpool_same_bwd(lv, absolute=True)
        assert bool((S[1] == 0).all()) and S[2, 0, 0] == 0 and bool((S[0] > 0).all())
        assert bool((out[S == 0] == 0).all())
        assert M.need(out, M.unpool_same_bwd(lv), S * M.U24)[0] <= M.LIMITS["unpool_same"]


def test_equals_the_floor_unpooling_where_the_pyramids_agree():
    lv = M.unpool_values((2, 8, 8), 4)
    assert [tuple(t.shape[1:]) for t in lv] == [(8, 8), (4, 4), (2, 2), (1, 1)]
    a, b, S = M.unpool_same_bwd(lv), B.unpool_bwd(lv), B.unpool_bwd(lv, absolute=True)
    assert float(((a - b).abs() / S).max()) <= 4 * 2.0 ** -53


def test_window_geometry_of_the_named_case():
    """5x6x12 with 4 levels: py = 1 at k = 4 and 8, px = 2 at k = 8, and x = 4 .. 7 lies in two windows there."""
    assert M.same_sizes(6, 12, 4) == [(6, 12), (3, 6), (2, 3), (1, 2)]
    Y4, c4 = M._windows(6, 2)
    assert Y4.tolist() == [0, 0, 0, 1, 1, 1] and c4.tolist() == [3, 3, 3, 3, 3, 3]
    Y8, c8 = M._windows(6, 3)
    assert Y8.tolist() == [0] * 6 and c8.tolist() == [6] * 6
    X8, d8 = M._windows(12, 3)
    assert X8.tolist() == [0] * 6 + [1] * 6 and d8.tolist() == [6] * 12 and len(set(X8[4:8].tolist())) == 2
    for (Q, H, W), nlev, _ in M.UNPOOL_BIG:
        n = Q * H * W // (4 if W % 4 == 0 else 1)
        assert M.BLOCK_CAP < n < 1.01 * M.BLOCK_CAP            # the grid-stride loop's second trip, and no larger than it has to be
        assert 4 * sum(Q * h * w for h, w in M.same_sizes(H, W, nlev)) < 100e6


def test_scatter_same_is_the_transpose_of_the_lookup():
    """<lookup(V, pos), dout> = <V, scatter_same(pos, dout)> on ceil-sized levels, out-of-range and far positions included."""
    shape, radius = (2, 6, 12), 3
    Bn, H, W = shape
    c = M.lookup_bwd_case(shape, radius)
    zero = [torch.zeros_like(t) for t in c["old"]]
    V = M.level_values(shape, 4)
    for t in range(2):
        out, _ = R.lookup(V, c["given"][t], radius)
        lhs = float((out.reshape(Bn * H * W, -1) * c["fdout"][t].double()).sum())
        dl, _ = M.scatter_same(c["pos"][t:t + 1], c["fdout"][t:t + 1], (H, W), 4, radius, old=zero)
        rhs = float(sum((a.double() * b).sum() for a, b in zip(V, dl)))
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)
    assert [tuple(t.shape[1:]) for t in c["ref"]] == M.same_sizes(H, W, 4) != [(H >> l, W >> l) for l in range(4)]


def test_dcoords_on_ceil_levels_is_the_derivative_of_the_lookup():
    """A central difference of _corrref.lookup on ceil-sized levels at positions off the integers (the lookup is bilinear in between)."""
    shape, nlev, radius = (1, 9, 11), 4, 3
    Bn, H, W = shape
    V = M.level_values(shape, nlev)
    g = D._gen("fd", *shape)
    pos = (torch.randint(-6 * 64, (W + 6) * 64, (Bn, 2, H, W), generator=g).float() + 0.5) / 64
    dout = D.dout_values(Bn, H, W, nlev, radius, "gauss")
    _, dc, S = D.expect(V, pos, dout, radius)
    e = 2.0 ** -12
    for a in (0, 1):
        d = torch.zeros(1, 2, 1, 1, dtype=torch.float64)
        d[0, a] = e
        hi, _ = R.lookup(V, pos.double() + d, radius)
        lo, _ = R.lookup(V, pos.double() - d, radius)
        fd = ((hi - lo) * dout.double()).sum(-1) / (2 * e)
        assert float((fd - dc[:, a]).abs().max()) <= 1e-9 * float(S.max())


def test_limits_come_from_the_twins():
    """LIMITS = 4 x the worst the fp32 twins reach over every case of the GPU tests, rounded up to one digit; a key borrowed from
    the floor-sized cases applies because its twin on the ceil sizes stays under the worst recorded there."""
    worst = M.twins_worst()
    for key, (w, case) in sorted(worst.items()):
        print(f"{key}: twins' worst {w:.4f} (limit {M.LIMITS[key]:g}) at {case}")
    assert set(worst) == set(M.LIMITS) == set(M.TWIN_WORST) | set(M.SHARED)
    for key, rec in M.TWIN_WORST.items():
        assert 0.9 * rec <= worst[key][0] <= rec, (key, worst[key])
        assert M.LIMITS[key] == M.limit_from_twin(rec)
    for key, (rec, lim) in M.SHARED.items():
        assert 0 < worst[key][0] <= rec, (key, worst[key])
        assert M.LIMITS[key] == lim == M.limit_from_twin(rec)


def test_the_chain_case_is_a_same_pyramid():
    c = M.chain_case()
    (Bn, H, W), nlev, C = M.CHAIN
    assert H % 2 and W % 8 and [tuple(t.shape[1:]) for t in c["pyr"]] == M.same_sizes(H, W, nlev) == [tuple(t.shape[1:]) for t in c["dlev"]]


# ------------------------------------------------------------------------------------------------ the switch
def test_same_grad_is_off_by_default_and_returns_the_previous_value():
    from flow_supervisor_amd import raft_tf
    from flow_supervisor_amd.raft_tf import api
    assert api._SAME_GRAD is False
    try:
        assert raft_tf.same_grad() == False and api._SAME_GRAD is True           # noqa: E712
        assert raft_tf.same_grad(True) == True and api._SAME_GRAD is True        # noqa: E712
        assert raft_tf.same_grad(False) == True and api._SAME_GRAD is False      # noqa: E712
        assert not raft_tf.same_grad(False) and repr(raft_tf.same_grad(False)) == "False"
    finally:
        api._SAME_GRAD = False


def test_same_grad_as_a_context_manager_restores_also_after_an_exception():
    from flow_supervisor_amd import raft_tf
    from flow_supervisor_amd.raft_tf import api
    try:
        with raft_tf.same_grad():
            assert api._SAME_GRAD is True
            with raft_tf.same_grad(False):
                assert api._SAME_GRAD is False
            assert api._SAME_GRAD is True
        assert api._SAME_GRAD is False
        with pytest.raises(KeyError):
            with raft_tf.same_grad():
                assert api._SAME_GRAD is True
                raise KeyError("x")
        assert api._SAME_GRAD is False
        raft_tf.same_grad(True)
        with pytest.raises(KeyError):
            with raft_tf.same_grad(False):
                raise KeyError("x")
        assert api._SAME_GRAD is True
    finally:
        api._SAME_GRAD = False


def test_forward_only_message_names_the_switch():
    from flow_supervisor_amd import raft_tf
    a = torch.zeros(1, 6, 6, 4, requires_grad=True)
    with pytest.raises(RuntimeError, match="forward-only.*same_grad"):
        raft_tf.calc_all_field(a, a.detach(), num_pool=2)
    v = torch.zeros(1, 2, 2, 5, 6, requires_grad=True)
    with pytest.raises(RuntimeError, match="forward-only.*same_grad"):
        raft_tf.build_pyramid(v, num_pool=1)
