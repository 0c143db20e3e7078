"""tests/_flowlossref.py on the CPU: the float64 restatement against torch.autograd on the literal op sequence of raft/loss.py for
the three penalties, the three reductions and every y_true form; the fp32 twin against the committed limits over the launches
the GPU files make, and the limits against what the twin's worst values give; the conditions on the inputs; the host-side
refusals of fsraft_flow_loss and its workspace query; and the Python surface's refusals (no CPU implementation)."""
import ctypes

import pytest
import torch

import _flowlossref as R

FS_ERR_ARG = 1
L1, L2, ROBUST = 0, 1, 2
null, p, odd = ctypes.c_void_p(None), ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 4)


def _ids(c):
    return "x".join(map(str, c)) if isinstance(c, tuple) else str(c)


# ================================================================================================= restatement against autograd
@pytest.mark.parametrize("reduction", ("mean", "sum", "none"))
@pytest.mark.parametrize("form", ("joint", "pair", "pair3d", "single", "bare"))
@pytest.mark.parametrize("penalty", R.PENALTIES)
def test_restatement_equals_autograd_through_the_literal_ops(penalty, form, reduction):
    B, H, W, n = R.CROSSED[0]
    preds, target, mask, w = R.inputs(B, H, W, n)
    y_true = {"joint": torch.cat((target, mask[..., None]), 3).double(), "pair": (target.double(), mask[..., None].double()),
              "pair3d": (target.double(), mask.double()), "single": (target.double(),), "bare": target.double()}[form]
    has_mask = form in ("joint", "pair", "pair3d")
    pd = preds[0].double().requires_grad_(True)
    lit = R.keras_loss_literal(y_true, pd, penalty, reduction)
    up = torch.randn(B, H, W, dtype=torch.float64, generator=torch.Generator().manual_seed(3)) if reduction == "none" else None
    (lit * up).sum().backward() if reduction == "none" else lit.backward()
    scale = R.scale_of("mean" if reduction == "mean" else "sum", B, H, W)
    r = R.flow_loss_ref(preds[:1], torch.ones(1), target, mask if has_mask else None, penalty, scale)
    if reduction == "none":
        assert (2.0 * scale * r["pixel"] - lit.detach()).abs().max().item() <= 1e-13 * float(lit.detach().abs().max())
        assert (r["dpred"][0] * up[..., None] - pd.grad).abs().max().item() <= 1e-13 * float(pd.grad.abs().max())
    else:
        assert abs(float(r["loss"]) - float(lit.detach())) <= 1e-13 * float(lit.detach())
        assert (r["dpred"][0] - pd.grad).abs().max().item() <= 1e-13 * float(pd.grad.abs().max())
    # what the GPU tests assert exactly holds of the restatement
    m = r["m"].view(B, -1)
    assert m[0, 1] == 0 and m[0, 2] == 1.0 and r["dpred"][0].view(B, -1, 2)[0, 1].abs().max() == 0
    if penalty == "l1":
        assert r["dpred"][0].view(B, -1, 2)[0, 0].abs().max() == 0


def test_sequence_weights_and_null_operands():
    B, H, W, n = R.CROSSED[0]
    preds, target, mask, w = R.inputs(B, H, W, n)
    for penalty in R.PENALTIES:
        r = R.flow_loss_ref(preds, w, target, mask, penalty, 0.5)
        one = [R.flow_loss_ref([q], torch.ones(1), target, mask, penalty, 0.5)["loss"] for q in preds]
        assert abs(float(r["loss"]) - sum(float(w[i]) * float(one[i]) for i in range(n))) <= 1e-12 * float(r["loss"])
        z = R.flow_loss_ref(preds, w, None, None, penalty, 0.5)
        zz = R.flow_loss_ref(preds, w, torch.zeros_like(target), torch.ones_like(mask), penalty, 0.5)
        assert float(z["loss"]) == float(zz["loss"])
        big = R.flow_loss_ref(preds, w, None, None, penalty, 0.5, max_flow=0.0)          # a NULL target: the cut is trivially true
        assert float(big["loss"]) == float(z["loss"])


def test_epe_statistics_are_what_the_metric_divides():
    B, H, W, n = R.CASES[6]
    preds, target, mask, w = R.inputs(B, H, W, n)
    r = R.flow_loss_ref(preds, w, target, mask, "l2", 0.5, metric_idx=1)
    want = R.epe_metric_literal([(target, mask, preds[1])])
    assert abs(float((r["stats"][:, 0] / r["stats"][:, 1]).mean()) - float(want)) <= 1e-13 * float(want)
    zero = R.epe_metric_literal([(target, torch.zeros_like(mask), preds[1]), (target, mask, preds[1])])
    assert abs(float(zero) - (float(want) * B - B) / (2 * B)) <= 1e-13


# ============================================================================================================ inputs and case lists
@pytest.mark.parametrize("case", R.CASES + (R.SURFACE,), ids=_ids)
def test_inputs_hold_what_the_issue_names(case):
    B, H, W, n = case
    preds, target, mask, w = R.inputs(B, H, W, n)
    assert set(mask.unique().tolist()) <= {0.0, 0.25, 1.0}
    mag = (target.double() ** 2).sum(-1).sqrt()
    off = (mag - 400.0).abs()
    # every |target| is exactly 400.0 or at least 6 fp32 steps (3e-5 each at 400) off it: fp32 and float64 decide the cut alike
    assert not bool(((off < 2e-4) & (off != 0)).any())
    if H * W >= 8:
        assert set(mask.unique().tolist()) == {0.0, 0.25, 1.0}
        t = target.view(B, -1, 2)
        assert float(mag.view(B, -1)[0, 1]) == 400.0 and 399.99 < float(mag.view(B, -1)[0, 2]) < 400.0
        assert float((t[0, 1].float() ** 2).sum().sqrt()) == 400.0 and float((t[0, 2].float() ** 2).sum().sqrt()) < 400.0     # in fp32 too
        for q in preds:
            d = (q - target).view(B, -1, 2)
            assert bool((d[0, 0] == 0).all()) and bool((d[0, 5] < 0).all()) and bool((d < 0).any())
            assert int((d == 0).sum()) == 2                       # no other difference is exactly zero (sign(0) is decided there only)


def test_case_lists_hold_what_the_issue_names():
    assert set(R.CASES) == {(1, 1, 1, 1), (2, 5, 7, 3), (1, 255, 1, 2), (1, 256, 1, 2), (1, 257, 1, 2), (2, 5, 7, 32), (3, 9, 31, 2), R.BIG}
    B, H, W, n = R.BIG
    assert B == 1 and H * W > R.FL_MAX_WG * R.FL_THREADS and 0 < H * W - R.FL_MAX_WG * R.FL_THREADS < R.FL_THREADS * R.FL_MAX_WG
    assert 9 * 31 % R.FL_THREADS and 9 * 31 > R.FL_THREADS                     # a partial last workgroup in every sample
    assert set(R.CROSSED) == {(2, 5, 7, 3), (1, 257, 1, 2)} and len(R.crossed_variants()) == 4 * 3 * 2 * 2
    from flow_supervisor_amd import _lib
    size = _lib.load().fsraft_flow_loss_workspace_bytes
    assert size(*R.BIG[:3]) == 64 + R.FL_MAX_WG * 12 == size(1, 1024, 1024)    # the grid stops at FL_MAX_WG workgroups per sample
    assert size(1, 512, 1024) == 64 + R.FL_MAX_WG * 12 and size(1, 256, 1024) == 64 + R.FL_MAX_WG // 2 * 12


# ================================================================================================================ twin and limits
def _twin_worst():
    worst = {}
    for penalty in R.PENALTIES:
        for run in R.all_runs():
            a = R.launch_args(*run)
            for k, v in R.twin_needs(a[0], a[1], a[2], a[3], penalty, a[4], a[5], a[6]).items():
                worst[k] = max(worst.get(k, 0.0), v)
    return worst


def test_twin_within_limits_and_limits_are_four_times_the_twins_worst():
    got = _twin_worst()
    assert set(got) == set(R.LIMITS) == set(R.TWIN_WORST)
    for k, v in got.items():
        assert v <= R.LIMITS[k], (k, v)
        assert R.LIMITS[k] == R.limit_from_twin(v), (k, v, R.LIMITS[k])
        assert abs(v - R.TWIN_WORST[k]) <= 0.06 * max(v, 0.1), (k, v)


@pytest.mark.parametrize("mut", ("threshold_mask", "le", "no_half", "l1_sign_one"))
def test_mutants_exceed_four_times_the_limit(mut):
    """What the limits are for: a thresholded mask, `<=` in the cut, a mean that forgets the channel axis and sign(0) = 1 each leave
    the restatement by more than 4 x the limit of some output of the designed case."""
    B, H, W, n = R.CROSSED[0]
    preds, target, mask, w = R.inputs(B, H, W, n)
    penalty = "l1" if mut == "l1_sign_one" else "l2"
    scale = R.scale_of("mean", B, H, W)
    exp = R.expect(preds, w, target, mask, penalty, scale)
    if mut == "threshold_mask":
        r = R.flow_loss_ref(preds, w, target, (mask >= 0.5).float(), penalty, scale)
    elif mut == "le":
        r = R.flow_loss_ref(preds, w, target, mask, penalty, scale, max_flow=400.0 + 1e-9)
    elif mut == "no_half":
        r = R.flow_loss_ref(preds, w, target, mask, penalty, 2.0 * scale)
    else:
        r = R.flow_loss_ref(preds, w, target, mask, penalty, scale)
        r["dpred"][0].view(B, -1, 2)[0, 0] = float(w[0]) * scale
    dev = max([R.need(r["loss"], *exp["loss"][:3])[0] / R.LIMITS["fl_loss"]]
              + [R.need(d, *e[:3])[0] / R.LIMITS["fl_dpred"] for d, e in zip(r["dpred"], exp["dpred"])])
    assert dev > 4.0, (mut, dev)


# ================================================================================================================ host refusals
def lib():
    from flow_supervisor_amd import _lib
    return _lib.load()


def test_workspace_sizes():
    size = lib().fsraft_flow_loss_workspace_bytes
    assert size(0, 8, 8) == FS_ERR_ARG and size(1, 0, 8) == FS_ERR_ARG and size(1, 8, -1) == FS_ERR_ARG
    assert size(1, 1 << 16, 1 << 16) == FS_ERR_ARG and size(65536, 1, 1) == FS_ERR_ARG
    assert size(1, 1, 1) == 64 + 64                                         # one workgroup: three floats, rounded up to 64
    assert size(3, 9, 31) == 64 + (3 * 2 * 12 + 63) // 64 * 64              # two workgroups of 256 pixels per sample
    for shape in ((1, 1, 1), (2, 5, 7), (8, 368, 768), (65535, 1, 1)):
        assert size(*shape) % 64 == 0 and size(*shape) >= 128


def test_flow_loss_rejects_bad_arguments_before_touching_the_gpu():
    L = lib()
    B, H, W = 2, 5, 7
    need = L.fsraft_flow_loss_workspace_bytes(B, H, W)

    def call(n=3, pred=True, dpred=True, weights=True, penalty=L2, out=p, stats=null, metric_idx=-1, pixel_out=null, ws=p, nbytes=need,
             B=B, H=H, W=W, hole=None):
        k = max(n, 1)
        pa = (ctypes.c_void_p * k)(*[None if i == hole else 4096 for i in range(k)])
        da = (ctypes.c_void_p * k)(*([4096] * k))
        wa = (ctypes.c_float * k)(*([1.0] * k))
        from flow_supervisor_amd import _lib
        return L.fsraft_flow_loss(ctypes.cast(pa, _lib._PP) if pred else None, ctypes.cast(da, _lib._PP) if dpred else None,
                                  wa if weights else None, n, 2 * H * W, 1, 2, p, 3 * H * W, 1, 3, p, 3 * H * W, 3, penalty, 400.0, 1e-3,
                                  0.5, B, H, W, out, stats, metric_idx, pixel_out, ws, nbytes, None)

    assert call(n=0) == call(n=-1) == call(n=33) == FS_ERR_ARG
    assert call(penalty=-1) == call(penalty=3) == FS_ERR_ARG
    assert call(pred=False) == call(weights=False) == call(out=null) == call(ws=null) == FS_ERR_ARG
    assert call(hole=0) == call(hole=2) == FS_ERR_ARG                        # a null entry of pred
    assert call(pixel_out=p) == call(n=2, pixel_out=p) == FS_ERR_ARG         # the per-pixel map: a single prediction
    assert call(stats=p, metric_idx=-1) == call(stats=p, metric_idx=3) == FS_ERR_ARG
    assert call(nbytes=need - 1) == call(ws=odd) == FS_ERR_ARG
    assert call(B=0) == call(H=0) == call(W=0) == call(B=65536, nbytes=1 << 30) == call(H=1 << 16, W=1 << 16, nbytes=1 << 30) == FS_ERR_ARG


# ============================================================================================================== Python surface
def test_cpu_tensors_are_refused():
    from flow_supervisor_amd import raft_tf
    y, q = torch.zeros(1, 4, 6, 3), torch.zeros(1, 4, 6, 2)
    for call in (lambda: raft_tf.FlowLossL2()(y, q), lambda: raft_tf.FlowLossL1(reduction="none")((y[..., :2], y[..., 2:]), q),
                 lambda: raft_tf.FlowLossRobust(reduction="sum")((y[..., :2],), q),
                 lambda: raft_tf.flow_sequence_loss([q, q], y, [0.8, 1.0], metric_idx=1),
                 lambda: raft_tf.semi_objective([q], [q], y, [q], [q], [q], [q]),
                 lambda: raft_tf.EPE().update_state(y, q)):
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            call()


def test_python_surface_checks_its_arguments():
    from flow_supervisor_amd import raft_tf
    y, q = torch.zeros(1, 4, 6, 3), torch.zeros(1, 4, 6, 2)
    with pytest.raises(ValueError, match="y_true"):
        raft_tf.FlowLossL2()(torch.zeros(1, 4, 5, 3), q)
    with pytest.raises(ValueError, match="mask"):
        raft_tf.FlowLossL2()((y[..., :2], torch.zeros(1, 4, 5)), q)
    with pytest.raises(ValueError, match="predictions"):
        raft_tf.flow_sequence_loss([q, torch.zeros(1, 4, 5, 2)], y, [1.0, 1.0])
    with pytest.raises(ValueError, match="predictions are"):
        raft_tf.flow_sequence_loss([q.permute(0, 3, 1, 2)], y, [1.0])
    with pytest.raises(ValueError, match="reduction"):
        raft_tf.FlowLossL1(reduction="auto")
    with pytest.raises(ValueError, match="single prediction"):
        raft_tf.flow_sequence_loss([q, q], y, [1.0, 1.0], reduction="none")
    with pytest.raises(ValueError, match="penalty"):
        raft_tf.flow_sequence_loss([q], y, [1.0], penalty="huber")
    with pytest.raises(ValueError, match="as many weights"):
        raft_tf.flow_sequence_loss([q] * 33, y, [1.0] * 33)
    with pytest.raises(ValueError, match="metric_idx"):
        raft_tf.flow_sequence_loss([q], y, [1.0], metric_idx=1)
    with pytest.raises(NotImplementedError):
        raft_tf.SparseEPE().update_state(y, q)
    assert raft_tf.EPE().result() == 0.0
