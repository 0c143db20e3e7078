"""Training-mode BatchNorm on the channels-last encoder route (core/extractor.py: _train_bn_ok, TRAIN_BN, _TrainBNReluCL on
csrc/norm_bn.hip): which route a training-mode encoder takes, parity with the framework's NCHW route and with a float64 CPU copy
over two steps (outputs, gradients, running statistics, num_batches_tracked), the hand-over to the frozen route at eval(), graph
capture of a residual unit, and the flow-supervisor step on a model whose BatchNorm is not frozen.  Needs an MI355X: -m gpu.
Limits: those of test_gpu_parity.test_encoder_channels_last_path_matches_nchw_path and test_gpu_parity.TRAIN_TOL, unchanged."""
import argparse
import copy

import pytest
import torch

from _util import close
from test_gpu_parity import TRAIN_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(params=["exact", "split"])
def precision(request):
    """The arithmetic mode of the convolutions (test_gpu_parity.precision); split, the default, is restored."""
    from flow_supervisor_amd import ops
    ops.set_arithmetic(request.param == "split")
    yield request.param
    ops.set_arithmetic(True)


def _rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _bns(m):
    return [q for q in m.modules() if isinstance(q, torch.nn.BatchNorm2d)]


# ----------------------------------------------------------------------------------------------------------------------- route
@pytest.mark.parametrize("kind", ("basic", "small"))
def test_training_mode_encoder_takes_the_batchnorm_kernels(kind, monkeypatch):
    """TRAIN_BN on: no call of torch.nn.functional.batch_norm, one ops.bnorm_cl_fwd per BatchNorm2d; off: the other way round."""
    import torch.nn.functional as F
    import flow_supervisor_amd.core.extractor as X
    from flow_supervisor_amd import ops
    torch.manual_seed(3)
    enc = (X.BasicEncoder if kind == "basic" else X.SmallEncoder)(norm_fn="batch").to(DEV).train()
    nbn = len(_bns(enc))
    assert nbn == (15 if kind == "basic" else 21)
    calls = {"framework": 0, "kernel": 0}
    f_bn, k_bn = F.batch_norm, ops.bnorm_cl_fwd
    monkeypatch.setattr(F, "batch_norm", lambda *a, **k: (calls.__setitem__("framework", calls["framework"] + 1), f_bn(*a, **k))[1])
    monkeypatch.setattr(ops, "bnorm_cl_fwd", lambda *a, **k: (calls.__setitem__("kernel", calls["kernel"] + 1), k_bn(*a, **k))[1])
    x = torch.randn(2, 3, 64, 96, device=DEV)
    y = enc(x)
    assert torch.isfinite(y).all() and calls == {"framework": 0, "kernel": nbn}, calls
    assert all(int(m.num_batches_tracked) == 1 for m in _bns(enc))
    calls.update(framework=0, kernel=0)
    monkeypatch.setattr(X, "TRAIN_BN", False)
    enc(x)
    assert calls == {"framework": nbn, "kernel": 0}, calls


# ---------------------------------------------------------------------------------------------------------------------- parity
def _two_steps(enc, x, dtype=torch.float32):
    """Two forward / backward passes -> (output, input gradient, parameter gradients) of the second."""
    for _ in range(2):
        enc.zero_grad(set_to_none=True)
        xi = x.to(dtype).clone().requires_grad_(True)
        y = enc(xi)
        (y[:1].square().sum() + (y[1:] * 0.5).sum()).backward()
    return y.detach(), xi.grad.clone(), {k: p.grad.clone() for k, p in enc.named_parameters() if p.grad is not None}


def _conv_biases_before_a_norm(enc):
    """Names of the biases of the convolutions a norm follows: all but the output projection conv2."""
    return {k for k, _ in enc.named_parameters() if k.endswith("bias") and k != "conv2.bias" and
            (k.split(".")[-2].startswith("conv") or k.endswith("downsample.0.bias"))}


def _bias_gradients_are_zero(enc64, grads64):
    """In float64 the gradient of every convolution bias in front of a BatchNorm is zero to rounding, against a weight gradient
    of the same convolution that is not."""
    for k in _conv_biases_before_a_norm(enc64):
        b, w = grads64[k].norm().item(), grads64[k[:-4] + "weight"].norm().item()
        assert b <= 1e-9 * w, (k, b, w)


def _compare(got, ref, enc_got, enc_ref, precision, what):
    tol = 1e-5 if precision == "exact" else 2e-4
    gtol = 1e-2 if precision == "exact" else 6e-2
    close(got[0], ref[0], 2e-4, what=f"{what}: encoder out")
    assert _rel_l2(got[0], ref[0]) < tol, (what, _rel_l2(got[0], ref[0]))
    e = _rel_l2(got[1], ref[1])
    assert e < gtol, f"{what}: encoder dx: relative L2 error {e:.3e}"
    assert set(got[2]) <= set(ref[2])
    for k, v in ref[2].items():
        if k not in got[2]:
            # a convolution bias in front of a BatchNorm gets no gradient from the kernels' route: the batch mean removes it, the
            # gradient is exactly zero.  The float64 copy has to say so (_bias_gradients_are_zero); the framework's fp32 value is the
            # rounding of a sum that cancels, at the scale of the objective, and no reference for anything
            assert k in _conv_biases_before_a_norm(enc_got), k
            continue
        e = _rel_l2(got[2][k], v)
        assert e < gtol or v.norm().item() < 1e-3, f"{what}: encoder grad {k}: relative L2 error {e:.3e}"
    for (k, a), (_, b) in zip(enc_got.named_buffers(), enc_ref.named_buffers()):
        if k.endswith("num_batches_tracked"):
            assert int(a) == int(b) == 2, (k, int(a), int(b))
        else:       # first and second moments of the same activations: the output's limit
            e = _rel_l2(a, b)
            assert e < tol, f"{what}: {k}: relative L2 error {e:.3e}"
            close(a, b, 2e-4, what=f"{what}: {k}")


@pytest.mark.parametrize("H,W", ((72, 104), (88, 100)), ids=("72x104", "88x100_odd_last_unit"))
def test_training_mode_encoder_matches_the_framework_route(H, W, precision, monkeypatch):
    """The kernels' route against FSRAFT_ENCODER_CL=0 (the framework's BatchNorm on MIOpen's NCHW convolutions) on the same weights,
    two steps; in exact mode also against a float64 CPU copy of the module.  Then eval(): the frozen route takes over the buffers
    the training route left, and gives the framework's eval output on them."""
    from flow_supervisor_amd.core.extractor import BasicEncoder
    torch.manual_seed(21)
    enc = BasicEncoder(output_dim=128, norm_fn="batch").to(DEV).train()
    for m in _bns(enc):
        with torch.no_grad():
            m.weight.normal_(1.0, 0.3), m.bias.normal_(0.0, 0.3)
    ref, ref64 = copy.deepcopy(enc), copy.deepcopy(enc).double().cpu()
    x = torch.randn(2, 3, H, W, device=DEV)
    monkeypatch.setenv("FSRAFT_ENCODER_CL", "1")
    got = _two_steps(enc, x)
    monkeypatch.setenv("FSRAFT_ENCODER_CL", "0")
    want = _two_steps(ref, x)
    _compare(got, want, enc, ref, precision, "against the framework route")
    want64 = _two_steps(ref64, x.cpu(), torch.float64)
    _bias_gradients_are_zero(ref64, want64[2])
    assert set(want64[2]) - set(got[2]) == _conv_biases_before_a_norm(enc)
    if precision == "exact":
        _compare(got, want64, enc, ref64, precision, "against float64")
    # hand-over
    enc.eval()
    with torch.no_grad():
        monkeypatch.setenv("FSRAFT_ENCODER_CL", "1")
        a = enc(x)
        monkeypatch.setenv("FSRAFT_ENCODER_CL", "0")
        b = enc(x)
    close(a, b, 2e-4, what="eval after training: encoder out")
    assert _rel_l2(a, b) < (1e-5 if precision == "exact" else 2e-4)


# --------------------------------------------------------------------------------------------------------------------- capture
def test_residual_unit_with_training_batchnorm_is_capturable():
    """One eager pass, then forward + backward captured on one stream and replayed twice: the running statistics and
    num_batches_tracked are those of three eager passes."""
    from flow_supervisor_amd.core.extractor import ResidualBlock
    torch.manual_seed(7)
    blk = ResidualBlock(64, 64, "batch", 1).to(DEV).train()
    ref = copy.deepcopy(blk)
    x = torch.randn(2, 64, 24, 40, device=DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    gout = torch.randn(2, 64, 24, 40, device=DEV).contiguous(memory_format=torch.channels_last)

    def run(b):
        # (the convolution biases in front of a BatchNorm are not part of the graph: their gradient is exactly zero)
        wanted = [p for k, p in b.named_parameters() if not (k.startswith("conv") and k.endswith("bias"))]
        return torch.autograd.grad(b(x), [x] + wanted, gout)

    for _ in range(3):
        eager = run(ref)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(blk)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        grads = run(blk)
    graph.replay(), graph.replay()
    torch.cuda.synchronize()
    for (k, a), (_, b) in zip(blk.named_buffers(), ref.named_buffers()):
        if k.endswith("num_batches_tracked"):
            assert int(a) == int(b) == 3, (k, int(a), int(b))
        else:
            assert _rel_l2(a, b) < 2e-4, (k, _rel_l2(a, b))
            close(a, b, 2e-4, what=k)
    for a, b in zip(grads, eager):
        assert _rel_l2(a, b) < 6e-2, _rel_l2(a, b)
    del graph


# ---------------------------------------------------------------------------------------------------------------------- wiring
def test_semi_train_step_with_unfrozen_batchnorm(precision, monkeypatch):
    """SemiTrainStep on L2L in train() without freeze_bn(): the sequential two-pass route, and the same two losses with the
    BatchNorm kernels as with the framework's modules."""
    import flow_supervisor_amd.core.extractor as X
    from flow_supervisor_amd.core.l2l import L2L
    from flow_supervisor_amd.train import SemiTrainStep
    torch.manual_seed(0)
    model0 = L2L(argparse.Namespace(small=False, mixed_precision=False, alternate_corr=False)).to(DEV).train()
    g = torch.Generator(device=DEV).manual_seed(3)
    H, W, h, w = 80, 112, 64, 96

    def sample(oy, ox):
        f1 = torch.rand(1, 3, H, W, device=DEV, generator=g) * 255
        f2 = torch.rand(1, 3, H, W, device=DEV, generator=g) * 255
        return [f1[:, :, oy:oy + h, ox:ox + w].contiguous(), f2[:, :, oy:oy + h, ox:ox + w].contiguous(), f1, f2, ox, oy,
                torch.randn(1, 2, h, w, device=DEV, generator=g), torch.ones(1, h, w, device=DEV)]

    sup, unsup = sample(8, 8), sample(16, 8)
    losses, kernel_calls = {}, {}
    for on in (True, False):
        monkeypatch.setattr(X, "TRAIN_BN", on)
        model = copy.deepcopy(model0)
        assert any(m.training for m in _bns(model))
        step = SemiTrainStep(model, lr=0.0, iters=2)
        seq, n = [], [0]
        orig, k_bn = step._sequential, X.ops.bnorm_cl_fwd
        monkeypatch.setattr(step, "_sequential", lambda *a, **k: (seq.append(1), orig(*a, **k))[1])
        monkeypatch.setattr(X.ops, "bnorm_cl_fwd", lambda *a, **k: (n.__setitem__(0, n[0] + 1), k_bn(*a, **k))[1])
        ls, lu = step(sup, unsup)
        monkeypatch.setattr(X.ops, "bnorm_cl_fwd", k_bn)
        losses[on], kernel_calls[on] = (float(ls), float(lu)), n[0]
        assert seq == [1], "a training-mode BatchNorm takes the sequential two-pass step"
    assert kernel_calls[True] > 0 and kernel_calls[False] == 0, kernel_calls
    tol = TRAIN_TOL[precision]["loss"]
    for a, b, what in zip(losses[True], losses[False], ("sup loss", "unsup loss")):
        assert abs(a - b) <= tol * abs(b), f"{what}: {a!r} with the kernels, {b!r} with the framework's modules (rel {abs(a - b) / abs(b):.2e} > {tol:g})"
