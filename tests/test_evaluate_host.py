"""CPU-only checks of the evaluation module (flow_supervisor_amd/evaluate.py, csrc/flow_metrics.hip): the restatement the
GPU tests use as their oracle (_evalref) is the reference's -- it reproduces what the reference's own validate_kitti /
validate_sintel / validate_chairs returned on the fixture of tests/golden/make_eval_golden.py --, its threshold semantics at
the boundaries are settled, the two C-ABI entries refuse bad arguments on the host, and the submission loop's bookkeeping
(warm start, sequence change, file names) is the reference's."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _evalref as R
from _util import T, load

FS_ERR_ARG = 1
# The reference returns float32 means out of numpy's pairwise sum (evaluate.py:121, 127, 165) or torch's fp32 mean (:158) over
# N ~ 7e3 values: relative error <= eps32 * (log2 N + slack) = 1.2e-7 * (13 + 4) = 2e-6.  Not a property of the code under test.
REF_RTOL = 2e-6


def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def fixture_stats(g, name, pred_key, mode, with_valid):
    n, H, W = (int(v) for v in g[name + "_shape"])
    pred = T(g[pred_key])
    if mode is not None:
        pred = R.unpadded(pred, H, W, mode)
    return R.batch_stats(pred, T(g[name + "_gt"]), T(g[name + "_valid"]) if with_valid else None)


def test_restatement_reproduces_the_reference_values():
    g = load("eval_metrics")
    kitti = R.dataset_values(fixture_stats(g, "kitti", "kitti_pred", "kitti", True))
    assert rel(kitti["epe_per_image"], g["kitti_ref"][0]) <= REF_RTOL, (kitti, g["kitti_ref"])
    assert rel(kitti["f1"], g["kitti_ref"][1]) <= REF_RTOL, (kitti, g["kitti_ref"])
    assert kitti["images"] == 3 and 0.6 * 3 * 37 * 61 < kitti["pixels"] < 0.8 * 3 * 37 * 61
    for i, dstype in enumerate(("clean", "final")):
        v = R.dataset_values(fixture_stats(g, "sintel", "sintel_pred_" + dstype, "sintel", False))
        assert rel(v["epe"], g["sintel_ref"][i]) <= REF_RTOL, (dstype, v, g["sintel_ref"])
        assert v["pixels"] == 3 * 37 * 61
    chairs = R.dataset_values(fixture_stats(g, "chairs", "chairs_pred", None, False))
    assert rel(chairs["epe"], g["chairs_ref"][0]) <= REF_RTOL, (chairs, g["chairs_ref"])
    # the fixture has members on both sides of every threshold, and of the KITTI ratio rule
    for v in (kitti, chairs):
        assert 0 < v["1px"] < v["3px"] < v["5px"] < 1 and 0 < v["f1"] < 100
    s = fixture_stats(g, "kitti", "kitti_pred", "kitti", True).sum(0)
    assert s[5] < s[0] - s[3]                 # some pixel has epe >= 3 and is no outlier: epe / |gt| <= 0.05 occurs


def test_boundary_semantics_of_the_restatement():
    for name, gt, d, lt1, lt3, lt5, outlier in R.BOUNDARY:
        g = torch.tensor(gt).view(2, 1, 1)
        p = g + torch.tensor(d).view(2, 1, 1)
        s = R.sample_stats(p, g)
        assert list(s[[0, 2, 3, 4, 5]]) == [1, lt1, lt3, lt5, outlier], (name, s)
    # d = (3, 0): neither < 3 nor > 3; d = (3, 4): epe 5 is not < 5
    epe, out = R.pixel_terms(torch.tensor([13., 0.]).view(2, 1, 1), torch.tensor([10., 0.]).view(2, 1, 1))
    assert epe.item() == 3.0 and not (epe < 3).item() and not (epe > 3).item() and not out.item()
    epe, _ = R.pixel_terms(torch.tensor([13., 4.]).view(2, 1, 1), torch.tensor([10., 0.]).view(2, 1, 1))
    assert epe.item() == 5.0 and not (epe < 5).item()
    # gt = (100, 0), d = (5, 0): the ratio is fl32(0.05), which float64 would call > 0.05; torch compares in float32
    epe, out = R.pixel_terms(torch.tensor([105., 0.]).view(2, 1, 1), torch.tensor([100., 0.]).view(2, 1, 1))
    assert epe.item() == 5.0 and float(np.float32(5.0) / np.float32(100.0)) > 0.05 and not out.item()
    # valid == 0.5 counts, anything below does not
    one = torch.ones(2, 1, 1)
    assert R.sample_stats(one, 0 * one, torch.tensor([[0.5]]))[0] == 1
    assert R.sample_stats(one, 0 * one, torch.tensor([[0.49999997]]))[0] == 0
    pred, gt, valid = R.boundary_frame()
    s = R.sample_stats(pred[0], gt[0], valid[0])
    assert list(s) == [14, 3 + 5 + 5 + 4 + 1, 14 - 5, 14 - 4, 14 - 2, 2, 0, 0], s


def test_flow_metrics_entries_reject_bad_arguments_before_touching_the_gpu():
    """Argument validation is host code: FS_ERR_ARG without a HIP call, so no kernel is ever handed one of these pointers."""
    from flow_supervisor_amd import _lib
    lib = _lib.load()
    size, run = lib.fsraft_flow_metrics_scratch_bytes, lib.fsraft_flow_metrics
    assert size(0, 4, 4) == FS_ERR_ARG and size(1, 0, 4) == FS_ERR_ARG and size(1, 4, -1) == FS_ERR_ARG
    assert size(1, 1 << 16, 1 << 16) == FS_ERR_ARG                   # H * W beyond 2^31 - 1
    assert size(1, 1, 1) == 64 and size(3, 37, 61) == 3 * 9 * 64
    assert size(1, 256, 256) == size(1, 436, 1024) == 256 * 64       # the blocks per sample stop growing at 256
    null, p, odd = ctypes.c_void_p(None), ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 4)
    H, W = 37, 61
    need = size(2, H, W)

    def call(pred=p, gt=p, stats=p, acc=p, scratch=p, B=2, H=H, W=W, nbytes=need):
        return run(pred, 2 * H * W, H * W, W, gt, 2 * H * W, H * W, W, null, 0, 0, B, H, W, stats, acc, scratch, nbytes, None)

    assert call(pred=null) == FS_ERR_ARG and call(gt=null) == FS_ERR_ARG
    assert call(stats=null) == FS_ERR_ARG and call(scratch=null) == FS_ERR_ARG
    assert call(B=0) == FS_ERR_ARG and call(H=0) == FS_ERR_ARG and call(W=0) == FS_ERR_ARG
    assert call(nbytes=need - 1) == FS_ERR_ARG and call(nbytes=0) == FS_ERR_ARG
    assert call(B=3) == FS_ERR_ARG                                    # scratch sized for two samples
    assert call(stats=odd) == FS_ERR_ARG and call(acc=odd) == FS_ERR_ARG and call(scratch=odd) == FS_ERR_ARG


def test_flow_metrics_refuses_cpu_predictions():
    from flow_supervisor_amd import ops
    from flow_supervisor_amd.evaluate import FlowMetrics
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        FlowMetrics().update(torch.zeros(2, 4, 4), torch.zeros(2, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        ops.flow_metrics(torch.zeros(1, 2, 4, 4), torch.zeros(1, 2, 4, 4), None, torch.zeros(1, 8, dtype=torch.float64))


class RecordingModel:
    """Stub with the reference's call signature: remembers every flow_init, returns a flow_low / flow_up pair of its own."""

    def __init__(self):
        self.inits, self.lows, self.ups = [], [], []

    def __call__(self, image1, image2, iters=None, flow_init=None, test_mode=False):
        assert test_mode and image1.shape == image2.shape and image1.shape[-2] % 8 == 0 and image1.shape[-1] % 8 == 0
        k = len(self.inits)
        g = torch.Generator().manual_seed(100 + k)
        H, W = image1.shape[-2:]
        self.inits.append(flow_init)
        self.lows.append(torch.randn(1, 2, H // 8, W // 8, generator=g))
        self.ups.append(torch.randn(1, 2, H, W, generator=g))
        return self.lows[-1], self.ups[-1]


def test_sintel_submission_bookkeeping(tmp_path, monkeypatch):
    """evaluate.py:30-52: flow_prev restarts with every sequence, is made from the previous frame's flow_low[0], and the files
    are frame%04d.flo numbered from 1.  Pure host: forward_interpolate (a HIP entry) is replaced by the identity here only."""
    from flow_supervisor_amd import evaluate as E
    from flow_supervisor_amd.raft_utils.frame_utils import readFlow
    monkeypatch.setattr(E, "forward_interpolate", lambda flow: flow)
    H, W = 37, 61
    frames = [("alley_1", 0), ("alley_1", 1), ("bamboo_2", 0), ("bamboo_2", 1), ("bamboo_2", 2)]
    dataset = [(torch.zeros(3, H, W), torch.zeros(3, H, W), f) for f in frames]
    model = RecordingModel()
    E.create_sintel_submission(model, dataset, iters=2, warm_start=True, output_path=str(tmp_path / "warm"), device="cpu")
    assert [i is None for i in model.inits] == [True, False, True, False, False]
    for k in (1, 3, 4):
        assert model.inits[k].shape == model.lows[k - 1].shape and torch.equal(model.inits[k], model.lows[k - 1][0][None])
    written = sorted(os.path.relpath(os.path.join(d, f), tmp_path / "warm") for d, _, fs in os.walk(tmp_path / "warm") for f in fs)
    assert written == ["alley_1/frame0001.flo", "alley_1/frame0002.flo", "bamboo_2/frame0001.flo", "bamboo_2/frame0002.flo",
                       "bamboo_2/frame0003.flo"]
    top, left = R.pad_offsets(H, W, "sintel")
    for k, (seq, frame) in enumerate(frames):
        back = readFlow(str(tmp_path / "warm" / seq / ("frame%04d.flo" % (frame + 1))))
        assert np.array_equal(back, model.ups[k][0, :, top:top + H, left:left + W].permute(1, 2, 0).numpy())
    cold = RecordingModel()
    E.create_sintel_submission(cold, dataset, warm_start=False, output_path=str(tmp_path / "cold"), device="cpu")
    assert all(i is None for i in cold.inits) and len(cold.inits) == len(frames)
