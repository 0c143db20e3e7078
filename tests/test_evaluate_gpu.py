"""GPU checks of the evaluation module: fsraft_flow_metrics (csrc/flow_metrics.hip) against the restatement of the
reference's metric code (_evalref, pinned to the reference in test_evaluate_host.py), its determinism and batch
independence, the FlowMetrics accumulator, the validate_* drivers against the values the reference's own functions returned
on tests/golden/eval_metrics.npz, and the Sintel submission loop with the real warm start.

Counts are compared exactly: the per-pixel arithmetic is the reference's fp32 bit for bit, so no threshold decision may
differ.  The epe sum is compared to relative 1e-9: an fp64 sum of N <= 5e5 non-negative fp32 terms is off by at most about
N * 2^-53 = 5e-11 relative, whatever its order, and the oracle's sum is correctly rounded."""
import functools
import os

import numpy as np
import pytest
import torch

import _evalref as R
from _util import T, load

pytestmark = pytest.mark.gpu
DEV = "cuda"
SUM_RTOL = 1e-9
REF_RTOL = 2e-6        # see test_evaluate_host.py: the rounding of the reference's own float32 means


def _flows(seed, B, H, W, Hp, Wp, top, left):
    """gt ~ N(0, 8 px) with a quarter of it twelve times larger, errors of 0.2 .. 8 px, valid ~70 % with exact 0.5 entries; the
    prediction sits inside a [B,2,Hp,Wp] frame whose border holds values that would wreck every sum."""
    g = torch.Generator().manual_seed(seed)
    gt = torch.randn(B, 2, H, W, generator=g) * 8.0 * torch.where(torch.rand(B, 1, H, W, generator=g) < 0.25, 12.0, 1.0)
    err = torch.randn(B, 2, H, W, generator=g) * torch.exp(torch.empty(B, 1, H, W).uniform_(-1.6, 2.08, generator=g))
    frame = 1000.0 + torch.randn(B, 2, Hp, Wp, generator=g)
    frame[:, :, top:top + H, left:left + W] = gt + err
    u = torch.rand(B, H, W, generator=g)
    valid = torch.where(u < 0.05, torch.full_like(u, 0.5), (u < 0.7).float())
    valid[:, 0, 0] = 0.5                                     # every sample has a pixel that counts, at exactly 0.5
    return frame, gt, valid


# name: B, H, W, padded frame (Hp, Wp, top, left), valid: "mask" / None / "zero1" (the last sample all invalid)
CASES = {
    "1x1": (1, 1, 1, (1, 1, 0, 0), "mask"),
    "3x5_less_than_a_wave": (1, 3, 5, (3, 5, 0, 0), "mask"),
    "37x61_view_of_40x64": (1, 37, 61, (40, 64, 0, 1), "mask"),              # odd left offset, row pitch != W, 4-byte aligned base
    "37x61_view_of_40x64_b3": (3, 37, 61, (40, 64, 0, 1), "mask"),
    "40x64_contiguous": (1, 40, 64, (40, 64, 0, 0), "mask"),                 # aligned rows (the kernel has one path for all)
    # 446464 pixels: seven trips of the grid-stride loop (256 blocks of 256 threads per sample cover 65536 a trip)
    "436x1024_view_of_440x1024": (1, 436, 1024, (440, 1024, 2, 0), "mask"),
    "37x61_valid_none": (2, 37, 61, (40, 64, 1, 1), None),
    "37x61_last_sample_all_invalid": (2, 37, 61, (40, 64, 1, 1), "zero1"),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """Host inputs and the restatement's [B,8] statistics, computed once per session and shared."""
    if name == "boundary_3x5":
        pred, gt, valid = R.boundary_frame()
        frame, box = pred, (0, 0)
    else:
        B, H, W, (Hp, Wp, top, left), vmode = CASES[name]
        frame, gt, valid = _flows(sum(map(ord, name)), B, H, W, Hp, Wp, top, left)
        box = (top, left)
        if vmode is None:
            valid = None
        elif vmode == "zero1":
            valid[-1] = 0.0
    H, W = gt.shape[-2:]
    view = frame[:, :, box[0]:box[0] + H, box[1]:box[1] + W]
    return frame, box, gt, valid, R.batch_stats(view, gt, valid)


def run_kernel(name, samples=None):
    """-> sample_stats [B,8], acc [8] (from a zero accumulator) as float64 numpy, for the case's samples (default: all)."""
    from flow_supervisor_amd import ops
    frame, (top, left), gt, valid, _ = case(name)
    sel = slice(None) if samples is None else samples
    H, W = gt.shape[-2:]
    view = frame[sel].to(DEV)[:, :, top:top + H, left:left + W]
    B = view.shape[0]
    stats = torch.full((B, 8), -1.0, device=DEV, dtype=torch.float64)
    acc = torch.zeros(8, device=DEV, dtype=torch.float64)
    ops.flow_metrics(view, gt[sel].to(DEV), None if valid is None else valid[sel].to(DEV), stats, acc)
    return stats.cpu().numpy(), acc.cpu().numpy()


def check_stats(got, ref, what):
    print(what, "kernel", got.tolist(), "restatement", ref.tolist())
    assert np.array_equal(got[:, [0, 2, 3, 4, 5, 6, 7]], ref[:, [0, 2, 3, 4, 5, 6, 7]]), what
    assert np.all(np.abs(got[:, 1] - ref[:, 1]) <= SUM_RTOL * ref[:, 1]), (what, got[:, 1], ref[:, 1])


@pytest.mark.parametrize("name", list(CASES) + ["boundary_3x5"])
def test_kernel_matches_the_restatement(name):
    frame, (top, left), gt, valid, ref = case(name)
    got, acc = run_kernel(name)
    check_stats(got, ref, name)
    if name.startswith("37x61_view"):                      # the view these cases are about is what they say it is
        v = frame.to(DEV)[:, :, top:top + 37, left:left + 61]
        assert v.data_ptr() % 16 == 4 and v.stride(2) == 64 and not v.is_contiguous()
    if name.endswith("all_invalid"):
        assert not got[-1].any() and got[0, 0] > 0
    # the accumulator, from zero: the samples' statistics added in ascending order, per-image means of samples with pixels
    want = np.zeros(8)
    for s in got:
        want[:6] += s[:6]
        if s[0] > 0:
            want[6] += s[1] / s[0]
            want[7] += 1
    assert np.array_equal(acc, want), (acc, want)


@pytest.mark.parametrize("name", ["37x61_view_of_40x64_b3", "436x1024_view_of_440x1024"])
def test_kernel_is_deterministic_and_batch_independent(name):
    s1, a1 = run_kernel(name)
    s2, a2 = run_kernel(name)
    assert s1.tobytes() == s2.tobytes() and a1.tobytes() == a2.tobytes()
    for b in range(s1.shape[0] if s1.shape[0] > 1 else 0):
        alone, _ = run_kernel(name, slice(b, b + 1))
        assert alone[0].tobytes() == s1[b].tobytes(), b


def test_flow_metrics_accumulates_like_the_restatement():
    from flow_supervisor_amd.evaluate import FlowMetrics
    g = load("eval_metrics")
    n, H, W = (int(v) for v in g["kitti_shape"])
    pred, gt, valid = T(g["kitti_pred"]).to(DEV), T(g["kitti_gt"]), T(g["kitti_valid"])
    want = R.dataset_values(R.batch_stats(R.unpadded(T(g["kitti_pred"]), H, W, "kitti"), gt, valid))
    m = FlowMetrics()
    assert m.last_samples() is None
    for i in range(n):                                       # [2,H,W] views of the padded prediction; gt and valid from the host
        m.update(R.unpadded(pred[i], H, W, "kitti"), gt[i], valid[i])
        assert m.last_samples().shape == (1, 8) and m.last_samples().is_cuda
    got = m.compute()
    print("FlowMetrics", got, "restatement", want)
    assert sorted(got) == sorted(want)
    for k in ("pixels", "images", "1px", "3px", "5px", "f1"):     # ratios of exact counts
        assert got[k] == want[k], k
    assert got["images"] == 3
    for k in ("epe", "epe_per_image"):
        assert abs(got[k] - want[k]) <= SUM_RTOL * want[k], k
    # a sample without a valid pixel changes neither the means nor `images`
    m.update(R.unpadded(pred[0], H, W, "kitti"), gt[0], torch.zeros(H, W))
    assert not m.last_samples().cpu().any()
    assert m.compute() == got
    # the batched update gives the very same totals, and reset() starts over
    mb = FlowMetrics(DEV)
    mb.update(R.unpadded(pred, H, W, "kitti"), gt, valid)
    assert mb.compute() == got
    mb.reset()
    assert mb.compute()["pixels"] == 0 and mb.compute()["images"] == 0


class ReplayModel:
    """model(image1, image2, iters=, flow_init=, test_mode=True) -> (None, the next image1.shape[0] stored predictions)"""

    def __init__(self, preds):
        self.preds, self.i = preds.to(DEV), 0

    def eval(self):
        return self

    def __call__(self, image1, image2, iters=None, flow_init=None, test_mode=False):
        B = image1.shape[0]
        out = self.preds[self.i:self.i + B]
        self.i += B
        assert test_mode and image1.is_cuda and image1.shape == image2.shape and image1.shape[-2:] == out.shape[-2:]
        return None, out


def _dataset(g, name, with_valid):
    n, H, W = (int(v) for v in g[name + "_shape"])
    gt = T(g[name + "_gt"])
    valid = T(g[name + "_valid"]) if with_valid else [None] * n
    return [(torch.zeros(3, H, W), torch.zeros(3, H, W), gt[i], valid[i]) for i in range(n)]


def test_validators_return_the_reference_values(capsys):
    from flow_supervisor_amd import evaluate as E
    g = load("eval_metrics")
    results = {}
    for bs in (1, 3):
        kitti = E.validate_kitti(ReplayModel(T(g["kitti_pred"])), _dataset(g, "kitti", True), batch_size=bs)
        sintel = E.validate_sintel(ReplayModel(torch.cat([T(g["sintel_pred_clean"]), T(g["sintel_pred_final"])])),
                                   {"clean": _dataset(g, "sintel", False), "final": _dataset(g, "sintel", False)}, batch_size=bs)
        chairs = E.validate_chairs(ReplayModel(T(g["chairs_pred"])), _dataset(g, "chairs", False), batch_size=bs)
        results[bs] = (kitti, sintel, chairs)
    kitti, sintel, chairs = results[1]
    print(results[1], g["kitti_ref"], g["sintel_ref"], g["chairs_ref"])
    assert list(kitti) == ["kitti-epe", "kitti-f1"] and list(sintel) == ["clean", "final"] and list(chairs) == ["chairs"]
    assert all(type(v) is float for r in results[1] for v in r.values())
    for got, ref in ((kitti["kitti-epe"], g["kitti_ref"][0]), (kitti["kitti-f1"], g["kitti_ref"][1]),
                     (sintel["clean"], g["sintel_ref"][0]), (sintel["final"], g["sintel_ref"][1]), (chairs["chairs"], g["chairs_ref"][0])):
        assert abs(got - ref) <= REF_RTOL * abs(ref), (got, ref)
    assert results[3] == results[1]                          # bit-identical: floats compared with ==
    k12 = E.validate_kitti2012(ReplayModel(T(g["kitti_pred"])), _dataset(g, "kitti", True))
    assert k12 == kitti
    out = capsys.readouterr().out
    assert "Validation KITTI: %f, %f" % (kitti["kitti-epe"], kitti["kitti-f1"]) in out
    assert "Validation Chairs EPE: %f" % chairs["chairs"] in out and "Validation (final) EPE: %f, 1px: " % sintel["final"] in out


class WarmModel:
    """Replays seeded flow_low / flow_up pairs on the device and records the flow_init of every call."""

    def __init__(self):
        self.inits, self.lows, self.ups = [], [], []

    def __call__(self, image1, image2, iters=None, flow_init=None, test_mode=False):
        assert test_mode and image1.is_cuda
        H, W = image1.shape[-2:]
        g = torch.Generator().manual_seed(300 + len(self.inits))
        self.inits.append(flow_init)
        self.lows.append((torch.randn(1, 2, H // 8, W // 8, generator=g) * 2.0).to(DEV))
        self.ups.append(torch.randn(1, 2, H, W, generator=g).to(DEV))
        return self.lows[-1], self.ups[-1]


def test_sintel_submission_on_the_device(tmp_path):
    from flow_supervisor_amd import evaluate as E
    from flow_supervisor_amd.core.utils.utils import InputPadder, forward_interpolate
    from flow_supervisor_amd.raft_utils.frame_utils import readFlow
    H, W = 37, 61
    frames = [("ambush_1", 0), ("ambush_1", 1), ("cave_3", 0)]
    model = WarmModel()
    E.create_sintel_submission(model, [(torch.zeros(3, H, W), torch.zeros(3, H, W), f) for f in frames], iters=2, warm_start=True,
                               output_path=str(tmp_path))
    assert model.inits[0] is None and model.inits[2] is None
    assert model.inits[1].is_cuda and torch.equal(model.inits[1], forward_interpolate(model.lows[0][0])[None])
    padder = InputPadder((3, H, W))
    for k, (seq, frame) in enumerate(frames):
        back = readFlow(os.path.join(str(tmp_path), seq, "frame%04d.flo" % (frame + 1)))
        assert np.array_equal(back, padder.unpad(model.ups[k][0]).permute(1, 2, 0).cpu().numpy())
