"""CPU-only checks of the unsupervised-loss boundary (csrc/unsup_loss.hip, flow_supervisor_amd/unsup_loss.py): every refusal of
the C entry points is host code and comes back as FS_ERR_ARG (1) without a HIP call, and the Python surface refuses what it
does not implement."""
import ctypes

import pytest
import torch

FS_ERR_ARG = 1
null, p, odd = ctypes.c_void_p(None), ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 4)
BIG = 1 << 16                         # BIG * BIG is beyond 2^31 - 1


def lib():
    from flow_supervisor_amd import _lib
    return _lib.load()


def crops(*pairs):
    return (ctypes.c_int * (2 * len(pairs)))(*[v for pair in pairs for v in pair])


def test_scratch_sizes():
    L = lib()
    for size in (L.fsraft_range_map_scratch_bytes, L.fsraft_census_scratch_bytes, L.fsraft_smoothness_scratch_bytes):
        assert size(0, 8, 8) == FS_ERR_ARG and size(1, 0, 8) == FS_ERR_ARG and size(1, 8, -1) == FS_ERR_ARG
        assert size(1, BIG, BIG) == FS_ERR_ARG
        assert size(2, 37, 61) % 8 == 0 and size(2, 37, 61) > 0
    assert L.fsraft_range_map_scratch_bytes(2, 37, 61) == 2 * 37 * 61 * 8
    assert L.fsraft_census_scratch_bytes(1, 6, 9) == FS_ERR_ARG and L.fsraft_census_scratch_bytes(1, 9, 6) == FS_ERR_ARG
    assert L.fsraft_census_scratch_bytes(1, 7, 7) == 64                       # one 32 x 16 tile: two doubles, rounded up to 64
    assert L.fsraft_census_scratch_bytes(2, 37, 61) == 2 * 3 * 2 * 16            # 3 x 2 tiles per sample
    assert L.fsraft_smoothness_scratch_bytes(3, 37, 61) == (3 * 9 * 16 + 63) // 64 * 64


def test_range_map_rejects_bad_arguments_before_touching_the_gpu():
    L = lib()
    H, W = 37, 61
    need = L.fsraft_range_map_scratch_bytes(2, H, W)

    def call(flow=p, out=p, scratch=p, B=2, H=H, W=W, nbytes=need):
        return L.fsraft_range_map(flow, 2 * H * W, H * W, W, B, H, W, 0, out, scratch, nbytes, None)

    assert call(flow=null) == call(out=null) == call(scratch=null) == call(scratch=odd) == FS_ERR_ARG
    assert call(B=0) == call(H=0) == call(W=0) == call(H=BIG, W=BIG) == FS_ERR_ARG
    assert call(nbytes=need - 1) == call(B=3) == FS_ERR_ARG


def test_census_entries_reject_bad_arguments_before_touching_the_gpu():
    L = lib()
    B, H, W, Hf, Wf = 2, 24, 40, 48, 80
    need = L.fsraft_census_scratch_bytes(B, H, W)
    good = crops((24, 40), (5, 7))

    def fwd(img1=p, img2=p, crop=good, flow=p, gB=p, hp=p, out=p, scratch=p, B=B, H=H, W=W, Hf=Hf, Wf=Wf, nbytes=need, frame1=1):
        return L.fsraft_census_fwd(img1, 3 * Hf * Wf, Hf * Wf, Wf, frame1, img2, 3 * Hf * Wf, Hf * Wf, Wf, Hf, Wf, crop,
                                   flow, 2 * H * W, H * W, W, null, 0, 0, B, H, W, gB, hp, out, scratch, nbytes, None)

    def bwd(img1=p, img2=p, crop=good, flow=p, gB=p, hp=p, up=p, den=p, dflow=p, B=B, H=H, W=W, Hf=Hf, Wf=Wf):
        return L.fsraft_census_bwd(img1, 3 * Hf * Wf, Hf * Wf, Wf, 1, img2, 3 * Hf * Wf, Hf * Wf, Wf, Hf, Wf, crop,
                                   flow, 2 * H * W, H * W, W, gB, hp, up, den, B, H, W, dflow, None)

    for k in ("img1", "img2", "flow", "gB", "hp", "out", "scratch"):
        assert fwd(**{k: null}) == FS_ERR_ARG, k
    for k in ("img1", "img2", "flow", "gB", "hp", "up", "den", "dflow"):
        assert bwd(**{k: null}) == FS_ERR_ARG, k
    assert fwd(out=odd) == fwd(scratch=odd) == bwd(den=odd) == FS_ERR_ARG
    assert fwd(nbytes=need - 1) == fwd(B=3, crop=crops((0, 0), (0, 0), (0, 0))) == FS_ERR_ARG
    for call in (fwd, bwd):
        assert call(B=0) == call(H=0) == call(W=0) == FS_ERR_ARG
        assert call(H=6) == call(W=6) == FS_ERR_ARG                         # no pixel survives the 3-pixel border
        assert call(H=BIG, W=BIG, Hf=BIG, Wf=BIG) == call(Hf=BIG, Wf=BIG) == FS_ERR_ARG
        assert call(Hf=H - 1) == call(Wf=W - 1) == FS_ERR_ARG               # a frame smaller than the window
        for bad in (crops((25, 40), (5, 7)), crops((24, 41), (5, 7)), crops((0, 0), (-1, 0)), crops((0, 0), (0, -1))):
            assert call(crop=bad) == FS_ERR_ARG                              # a window outside the frame


def test_smoothness_rejects_bad_arguments_before_touching_the_gpu():
    L = lib()
    B, H, W = 2, 24, 40
    need = L.fsraft_smoothness_scratch_bytes(B, H, W)

    def call(img=p, flow=p, dflow=p, out=p, scratch=p, crop=None, B=B, H=H, W=W, Hf=H, Wf=W, order=1, gaussian=0, nbytes=need):
        return L.fsraft_smoothness(img, 3 * Hf * Wf, Hf * Wf, Wf, Hf, Wf, crop, flow, 2 * H * W, H * W, W, B, H, W, order, 150.0, gaussian,
                                   dflow, out, scratch, nbytes, None)

    for k in ("img", "flow", "dflow", "out", "scratch"):
        assert call(**{k: null}) == FS_ERR_ARG, k
    assert call(out=odd) == call(scratch=odd) == call(nbytes=need - 1) == FS_ERR_ARG
    assert call(B=0) == call(H=0) == call(W=0) == call(H=BIG, W=BIG, Hf=BIG, Wf=BIG) == FS_ERR_ARG
    assert call(order=0) == call(order=3) == call(gaussian=2) == FS_ERR_ARG
    assert call(H=1, Hf=1) == call(order=2, W=2, Wf=2) == FS_ERR_ARG         # an empty mean
    assert call(crop=crops((1, 0), (0, 0))) == call(Hf=H + 4, Wf=W + 4, crop=crops((4, 4), (5, 0))) == FS_ERR_ARG


def test_python_surface_refuses_what_is_not_implemented():
    from flow_supervisor_amd import unsup_loss as U
    with pytest.raises(NotImplementedError, match="crop-and-resize"):
        U.UnsupervisedLoss(selfsup=0.3)
    with pytest.raises(NotImplementedError, match="brox"):
        U.UnsupervisedLoss(occlusion="brox")
    with pytest.raises(NotImplementedError, match="brox"):
        U.occlusion_mask(torch.zeros(1, 2, 8, 8), "brox")
    with pytest.raises(NotImplementedError, match="unsup_final_update"):
        U.UnsupervisedLoss(mode="unsup_final_update")
    loss = U.UnsupervisedLoss()
    assert loss.weights == {"census": 1.0, "smooth1": 2.5} and loss.gamma == 0.8 and loss.occlusion == "wang"
    assert "0.3" in U.UnsupervisedLoss.__doc__


def test_cpu_tensors_are_refused():
    from flow_supervisor_amd import unsup_loss as U
    img, flow = torch.zeros(1, 3, 8, 8), torch.zeros(1, 2, 8, 8)
    for call in (lambda: U.range_map(flow), lambda: U.occlusion_mask(flow), lambda: U.occlusion_mask(flow, "none"),
                 lambda: U.census_loss(img, img, flow, None), lambda: U.smoothness_loss(img, flow),
                 lambda: U.UnsupervisedLoss()((img, img), [flow], [flow])):
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            call()
