"""CPU-only checks of the self-supervision boundary (csrc/selfsup_loss.hip, flow_supervisor_amd/selfsup_loss.py): every refusal
of the C entry points is host code and comes back as FS_ERR_ARG (1) without a HIP call, and the Python surface has the
reference's defaults and refuses what it cannot run."""
import ctypes

import pytest
import torch

FS_ERR_ARG = 1
GAUSSIAN, DDFLOW, BROX, NONE = 0, 1, 2, 3
null, p, odd = ctypes.c_void_p(None), ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 4)
BIG = 1 << 16                         # BIG * BIG is beyond 2^31 - 1


def lib():
    from flow_supervisor_amd import _lib
    return _lib.load()


def crops(*pairs):
    return (ctypes.c_int * (2 * len(pairs)))(*[v for pair in pairs for v in pair])


BAD_CROPS = (crops((25, 40), (5, 7)), crops((24, 41), (5, 7)), crops((0, 0), (-1, 0)), crops((0, 0), (0, -1)))


def test_scratch_sizes():
    size = lib().fsraft_selfsup_scratch_bytes
    assert size(0, 8, 8) == FS_ERR_ARG and size(1, 0, 8) == FS_ERR_ARG and size(1, 8, -1) == FS_ERR_ARG
    assert size(1, BIG, BIG) == FS_ERR_ARG
    assert size(1, 1, 1) == 64                                               # one block: one double, rounded up to 64
    assert size(3, 37, 61) == (3 * 9 * 8 + 63) // 64 * 64                    # 9 blocks of 256 pixels per sample
    assert size(1, 512, 512) == size(1, 520, 520) == 1024 * 8                # the grid stops at 1024 blocks per sample
    for shape in ((1, 1, 1), (2, 37, 61), (3, 24, 40), (1, 520, 520), (5, 368, 768)):
        assert size(*shape) % 8 == 0 and size(*shape) > 0


def test_fb_mask_rejects_bad_arguments_before_touching_the_gpu():
    L = lib()
    B, H, W, Hf, Wf = 2, 24, 40, 48, 80

    def call(flow=p, back=p, out=p, crop=crops((24, 40), (5, 7)), B=B, H=H, W=W, Hf=Hf, Wf=Wf, mode=GAUSSIAN, complement=0, norm=0.5):
        return L.fsraft_fb_mask(flow, 2 * Hf * Wf, Hf * Wf, Wf, back, 2 * Hf * Wf, Hf * Wf, Wf, Hf, Wf, crop, B, H, W, mode, complement,
                                norm, out, None)

    for k in ("flow", "back", "out"):
        assert call(**{k: null}) == FS_ERR_ARG, k
    assert call(B=0) == call(H=0) == call(W=0) == FS_ERR_ARG
    assert call(H=BIG, W=BIG, Hf=BIG, Wf=BIG, crop=None) == call(Hf=BIG, Wf=BIG) == FS_ERR_ARG
    assert call(Hf=H - 1) == call(Wf=W - 1) == FS_ERR_ARG                    # a frame smaller than the window
    for bad in BAD_CROPS:
        assert call(crop=bad) == FS_ERR_ARG                                  # a window outside the frame
    assert call(mode=-1) == call(mode=NONE) == call(mode=4) == FS_ERR_ARG
    assert call(complement=2) == call(complement=-1) == FS_ERR_ARG
    assert call(norm=0.0) == call(norm=-1.0) == call(norm=float("nan")) == FS_ERR_ARG


def test_selfsup_rejects_bad_arguments_before_touching_the_gpu():
    L = lib()
    B, H, W, Hf, Wf = 2, 24, 40, 48, 80
    need = L.fsraft_selfsup_scratch_bytes(B, H, W)

    def call(teacher=p, tmask=p, student=p, sback=p, dflow=p, out=p, scratch=p, crop=crops((24, 40), (5, 7)), B=B, H=H, W=W, Hf=Hf, Wf=Wf,
             mode=GAUSSIAN, norm=0.5, nbytes=need):
        return L.fsraft_selfsup(teacher, 2 * Hf * Wf, Hf * Wf, Wf, Hf, Wf, crop, tmask, H * W, W, student, 2 * H * W, H * W, W,
                                sback, 2 * H * W, H * W, W, B, H, W, mode, norm, dflow, out, scratch, nbytes, None)

    for k in ("teacher", "student", "sback", "dflow", "out", "scratch"):
        assert call(**{k: null}) == FS_ERR_ARG, k
    assert call(out=odd) == call(scratch=odd) == call(nbytes=need - 1) == FS_ERR_ARG
    assert call(B=0) == call(H=0) == call(W=0) == FS_ERR_ARG
    assert call(H=BIG, W=BIG, Hf=BIG, Wf=BIG, crop=None) == call(Hf=BIG, Wf=BIG) == FS_ERR_ARG
    assert call(Hf=H - 1) == call(Wf=W - 1) == FS_ERR_ARG
    for bad in BAD_CROPS:
        assert call(crop=bad) == FS_ERR_ARG
    assert call(mode=-1) == call(mode=BROX) == call(mode=4) == FS_ERR_ARG
    assert call(norm=0.0) == call(norm=-2.0) == call(norm=float("nan")) == FS_ERR_ARG
    assert call(B=3, crop=crops((0, 0), (0, 0), (0, 0))) == FS_ERR_ARG       # scratch sized for two samples


def test_smurf_loss_has_the_references_defaults():
    from flow_supervisor_amd.selfsup_loss import SmurfLoss
    loss = SmurfLoss()
    assert loss.weights == {"census": 1.0, "smooth1": 2.5, "selfsup": 0.3}
    assert loss.gamma == 0.8 and loss.occlusion == "wang" and loss.selfsup_mask == "gaussian"
    assert (loss.sigma_teacher, loss.sigma_student) == (0.003, 0.03)
    assert SmurfLoss(occlusion="brox").occlusion == "brox" and SmurfLoss(selfsup=0).weights == {"census": 1.0, "smooth1": 2.5}
    with pytest.raises(ValueError, match="occlusion"):
        SmurfLoss(occlusion="fb")
    with pytest.raises(ValueError, match="selfsup_mask"):
        SmurfLoss(selfsup_mask="brox")


def test_selfsup_without_teacher_flows_is_a_value_error():
    from flow_supervisor_amd.selfsup_loss import SmurfLoss
    img, flow = torch.zeros(1, 3, 8, 8), torch.zeros(1, 2, 8, 8)
    with pytest.raises(ValueError, match="teacher"):
        SmurfLoss(selfsup=0.3)((img, img), [flow], [flow])
    with pytest.raises(ValueError, match="teacher"):
        SmurfLoss()((img, img), [flow], [flow], teacher_fw=flow)


def test_cpu_tensors_are_refused():
    from flow_supervisor_amd import selfsup_loss as S
    img, flow = torch.zeros(1, 3, 8, 8), torch.zeros(1, 2, 8, 8)
    for call in (lambda: S.fb_consistency_mask(flow, flow), lambda: S.fb_consistency_mask(flow, flow, "ddflow", complement=True),
                 lambda: S.brox_occlusion_mask(flow, flow), lambda: S.self_supervision_loss(flow, flow, flow, flow),
                 lambda: S.self_supervision_loss(flow, flow, flow, flow, mask="none"),
                 lambda: S.SmurfLoss()((img, img), [flow], [flow], flow, flow),
                 lambda: S.SmurfLoss(selfsup=0, occlusion="brox")((img, img), [flow], [flow])):
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            call()


def test_python_surface_checks_its_arguments():
    from flow_supervisor_amd import selfsup_loss as S
    flow, frame = torch.zeros(1, 2, 8, 8), torch.zeros(1, 2, 12, 12)
    with pytest.raises(ValueError, match="consistency mask"):
        S.fb_consistency_mask(flow, flow, "brox")
    with pytest.raises(ValueError, match="come together"):
        S.fb_consistency_mask(frame, frame, crop_yx=[(0, 0)])
    with pytest.raises(ValueError, match="selfsup_mask"):
        S.self_supervision_loss(flow, flow, flow, flow, mask="brox")
    assert S._normaliser(0.003, (432, 1024)) == 0.003 ** 2 * (432.0 ** 2 + 1024.0 ** 2)
