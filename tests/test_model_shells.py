"""The model shells (core/raft.py, gma_network.py, l2l.py, gma_l2l.py) against the CPU oracle run live, at the smallest shapes at
which four pyramid levels exist: what the fixture-based tests of test_gpu_parity.py leave open -- `flow_init`, the flow-supervisor
schedule with an empty student phase (iters=1) and with unequal phases (iters=3), for L2L and GMAL2L, and per-sample crop offsets
for both.  Needs an MI355X: -m gpu.  Limits: the project's EPE gate (BASELINE.json) and test_gpu_parity.TRAIN_TOL, unchanged."""
import functools

import pytest
import torch

from _util import close, grad_digest_check, rel_check, shapes
from oracle import raft_torch as O
from oracle.weights import procedural_state_dict, rand_tensor, synthetic_pair
from test_gpu_parity import TRAIN_TOL, gma_ns, ns, precision  # noqa: F401  (precision: the arithmetic-mode fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 31
H, W = 64, 96                            # 8 x 12 grid: 8 -> 4 -> 2 -> 1, the smallest with four pyramid levels
FH, FW, OX, OY = 96, 128, 16, 8          # the L2L family's uncropped frame and the crop's place in it


@functools.lru_cache(maxsize=None)
def _weights(kind):
    """kind: raft / gma / l2l / gma_l2l -> the procedural CPU state_dict (shared, never modified)."""
    from flow_supervisor_amd.core.gma_l2l import GMAL2L
    from flow_supervisor_amd.core.gma_network import RAFTGMA
    from flow_supervisor_amd.core.l2l import L2L
    from flow_supervisor_amd.core.raft import RAFT
    cls, args, fixture = {"raft": (RAFT, ns(False), "raft_basic"), "gma": (RAFTGMA, gma_ns(), "raft_gma"),
                          "l2l": (L2L, ns(False), "l2l_basic"), "gma_l2l": (GMAL2L, gma_ns(), "l2l_recipe_gma")}[kind]
    m = cls(args)
    missing, unexpected = m.load_state_dict(procedural_state_dict(shapes(fixture), SEED), strict=False)
    assert not unexpected and all("rel_ind" in k for k in missing), (missing, unexpected)
    if "gma" in kind:
        with torch.no_grad():
            m.update_block.aggregator.gamma.fill_(0.1)          # (as bench.py sets it: the aggregated branch takes part)
    return cls, args, {k: v.detach().clone() for k, v in m.state_dict().items()}


def _model(kind, train):
    cls, args, sd = _weights(kind)
    m = cls(args)
    m.load_state_dict(sd)
    m = m.to(DEV)
    if not train:
        return m.eval()
    m.train()
    m.freeze_bn()
    return m


# ----------------------------------------------------------------------------- flow_init
@functools.lru_cache(maxsize=None)
def _flow_init_case(kind):
    im1, im2 = synthetic_pair(1, H, W, SEED + 1)
    init = rand_tensor((1, 2, H // 8, W // 8), SEED + 2, 2.0)
    with torch.no_grad():
        ref = O.raft_forward(_weights(kind)[2], im1, im2, iters=3, flow_init=init, test_mode=True, gma=kind == "gma")
    return im1, im2, init, ref


@pytest.mark.parametrize("kind", ["raft", "gma"])
def test_flow_init_reaches_the_first_lookup(kind, precision):
    """evaluate.py warm-starts Sintel from the previous pair's flow (flow_init): test_mode, 3 iterations from a seeded 2 px
    initial flow, against the oracle given the same one.  (The oracle's outputs with and without it differ by EPE 2.6 / 5.6.)"""
    im1, im2, init, (ref_low, ref_up) = _flow_init_case(kind)
    m = _model(kind, train=False)
    with torch.no_grad():
        low, up = m(im1.to(DEV), im2.to(DEV), iters=3, flow_init=init.to(DEV), test_mode=True)
    e_low, e_up = O.epe(low.cpu(), ref_low).item(), O.epe(up.cpu(), ref_up).item()
    print(kind, precision, "flow_init EPE low", e_low, "EPE up", e_up)
    assert e_low <= 1e-3 and e_up <= 1e-3, (e_low, e_up)         # BASELINE.json gate


# ----------------------------------------------------------------------------- the flow-supervisor schedule
def _frames(B):
    return synthetic_pair(B, FH, FW, SEED + 3)


def _cut(c, ox, oy):
    return torch.cat([c[i:i + 1, :, oy[i]:oy[i] + H, ox[i]:ox[i] + W] for i in range(c.shape[0])]).contiguous()


@functools.lru_cache(maxsize=None)
def _schedule_case(kind, iters):
    """The oracle's training step: predictions, loss and every parameter-gradient norm (None: no gradient arrived)."""
    ci1, ci2 = _frames(2)
    im1, im2 = _cut(ci1, [OX] * 2, [OY] * 2), _cut(ci2, [OX] * 2, [OY] * 2)
    sd = {k: v.clone().requires_grad_(v.is_floating_point() and "running_" not in k) for k, v in _weights(kind)[2].items()}
    preds = O.l2l_forward(sd, im1, im2, ci1, ci2, [OX] * 2, [OY] * 2, iters=iters, gma=kind == "gma_l2l")
    loss = O.sequence_loss_zero_gt(preds)
    loss.backward()
    gn = {k: (None if v.grad is None else v.grad.norm().item()) for k, v in sd.items() if v.requires_grad}
    return (im1, im2, ci1, ci2), [p.detach() for p in preds], loss.item(), gn


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("kind", ["l2l", "gma_l2l"])
def test_flow_supervisor_schedule_with_empty_and_unequal_phases(kind, iters, precision):
    """iters=1: no student iteration, the switch is the first thing the loop does; iters=3: one student and two supervisor
    iterations.  Predictions, loss and parameter gradients against the oracle's L2L / GMAL2L, and the same SET of parameters
    with a gradient: the student's block and encoders only where a student iteration ran, grad_update_block for L2L only."""
    (im1, im2, ci1, ci2), ref, ref_loss, ref_gn = _schedule_case(kind, iters)
    m = _model(kind, train=True)
    off = lambda v: torch.tensor([v] * 2)
    preds = m(im1.to(DEV), im2.to(DEV), ci1.to(DEV), ci2.to(DEV), off(OX), off(OY), iters=iters)
    assert len(preds) == len(ref) == iters and all(tuple(p.shape) == (2, 2, H, W) for p in preds)
    tol = TRAIN_TOL[precision]
    loss = O.sequence_loss_zero_gt(preds)
    print(kind, iters, precision, "loss", loss.item(), "oracle", ref_loss)
    rel_check(loss.item(), ref_loss, tol["loss"], "loss")
    loss.backward()
    half = iters // 2
    if half:
        close(preds[half - 1], ref[half - 1], tol["pred"], rtol=0.0, what="last student prediction")
    close(preds[-1], ref[-1], tol["pred"], rtol=0.0, what="last supervisor prediction")
    named = list(m.named_parameters())
    ref_gn = {k: ref_gn[k] for k, _ in named}       # (the state_dict also holds frozen BatchNorm's affine pairs: buffers here)
    bad = grad_digest_check(named, {"gnorm." + k: (v or 0.0) for k, v in ref_gn.items()}, tol, hprefix=None)
    assert not bad, bad[:8]
    # who receives a gradient.  A norm at or under grad_digest_check's absolute allowance (1e-5: biases in front of InstanceNorm,
    # zero in exact arithmetic, rounding noise in either implementation) says nothing either way and is left out.
    got = {k for k, p in named if p.grad is not None and p.grad.norm().item() > 0}
    want = {k for k, v in ref_gn.items() if v}
    noise = {k for k, v in ref_gn.items() if v is not None and v <= 1e-5} | {k for k, p in named if p.grad is not None and p.grad.norm().item() <= 1e-5}
    assert got - noise == want - noise, sorted((got ^ want) - noise)[:8]
    sup = {k for k in got if k.startswith("grad_update_block.")}
    assert (not sup) if kind == "gma_l2l" else sup, "GMAL2L's supervisor phase stays on update_block; L2L's runs grad_update_block"


# ----------------------------------------------------------------------------- per-sample crop offsets
OFFS = ([0, 24], [16, 8])


@functools.lru_cache(maxsize=None)
def _offsets_case(kind):
    """The oracle once per sample with that sample's offset (the samples are independent: instance norm in the feature encoder,
    frozen BatchNorm in the context encoder)."""
    ci1, ci2 = _frames(2)
    im1, im2 = _cut(ci1, *OFFS), _cut(ci2, *OFFS)
    sd = _weights(kind)[2]
    with torch.no_grad():
        per = [O.l2l_forward(sd, im1[i:i + 1], im2[i:i + 1], ci1[i:i + 1], ci2[i:i + 1], [OFFS[0][i]], [OFFS[1][i]], iters=3,
                             gma=kind == "gma_l2l") for i in range(2)]
    return (im1, im2, ci1, ci2), [torch.cat([per[0][t], per[1][t]]) for t in range(3)]


@pytest.mark.parametrize("kind", ["l2l", "gma_l2l"])
def test_per_sample_crop_offsets_against_one_oracle_run_per_sample(kind, precision):
    (im1, im2, ci1, ci2), ref = _offsets_case(kind)
    m = _model(kind, train=True)
    preds = m(im1.to(DEV), im2.to(DEV), ci1.to(DEV), ci2.to(DEV), list(OFFS[0]), list(OFFS[1]), iters=3)
    assert len(preds) == 3 and all(tuple(p.shape) == (2, 2, H, W) for p in preds)
    for t, (p, r) in enumerate(zip(preds, ref)):
        close(p, r, TRAIN_TOL[precision]["pred"], rtol=0.0, what=f"prediction {t}")
