"""The complete unsupervised (SMURF) loss of the reference's third trainer: unsup_loss.py's census and smoothness terms plus
the two parts it refuses, the teacher / student self-supervision term and the 'brox' occlusion, on csrc/selfsup_loss.hip
(raft/smurf_models/smurf_utils.py self_supervision_loss, compute_occlusions_brox; raft/unsup_loss.py UnsupervisedLoss).

    fb_consistency_mask(flow, flow_back, kind, ...)         the 'gaussian' / 'ddflow' forward-backward consistency times valid
    brox_occlusion_mask(flow_fw, flow_bw)                   compute_occlusions(..., 'brox', occlusions_are_zeros=True)
    self_supervision_loss(teacher_fw, teacher_bw, ...)      self_supervision_loss with a crop as the transform
    SmurfLoss(...)                                          UnsupervisedLoss.call with the reference's own defaults

The reference's self-supervision transform (raft/unsup_loss.py:62-69) is a plain crop of the teacher's full-frame flow and
mask at the (crop_y, crop_x) window the census term reads in place; there is no resize.  PyTorch layout as in unsup_loss.py:
flows [B,2,H,W] with channel 0 = x.  The term is differentiable in the student's forward flow only: the teacher and the mask
are stopped, as in the reference.  CUDA (ROCm) fp32 tensors only: there is no CPU implementation.

Not implemented: mode 'unsup_final_update', smoothness above level 0 and resize=True transforms.
"""
import torch

from . import _lib as L
from . import ops
from .unsup_loss import _Census, _Smoothness

MASKS = ("gaussian", "ddflow", "none")


def _normaliser(sigma, hw):
    """sigma^2 * (h^2 + w^2) of smurf_utils.py:792-795."""
    return float(sigma) ** 2 * (float(hw[0]) ** 2 + float(hw[1]) ** 2)


@L.on_tensor_device
def fb_consistency_mask(flow, flow_back, kind="gaussian", sigma=0.003, frame_hw=None, crop_yx=None, complement=False,
                        window_hw=None):
    """c * valid of the pair (flow, flow_back), [B,2,H,W] each -> [B,1,H,W], no gradient; complement: 1 - c * valid.
    kind 'gaussian': c = exp(-|f + r|^2 / (sigma^2 * (h^2 + w^2))) with (h, w) = frame_hw (None: the flows' own size; the
    reference normalises the student's mask by the teacher's size); 'ddflow': c = [|f + r|^2 < 0.01 (|f|^2 + |r|^2) + 0.5].
    With crop_yx [B,2] = (y, x) (host integers) and window_hw = (H, W) the flows are frames and the mask is that of the frame,
    evaluated on the window only."""
    if kind not in ("gaussian", "ddflow"):
        raise ValueError(f"unknown consistency mask {kind!r}: 'gaussian' or 'ddflow'")
    if (crop_yx is None) != (window_hw is None):
        raise ValueError("crop_yx and window_hw come together")
    norm = _normaliser(sigma, frame_hw or flow.shape[-2:]) if kind == "gaussian" else 1.0
    with torch.no_grad():
        return ops.fb_mask(flow.detach(), flow_back.detach(), kind, norm, complement, window_hw,
                           ops.crop_offsets(crop_yx, flow.shape[0])).unsqueeze(1)


@L.on_tensor_device
def brox_occlusion_mask(flow_fw, flow_bw):
    """The 'brox' mask of the direction of flow_fw (1 = visible), [B,1,H,W], no gradient."""
    with torch.no_grad():
        return ops.fb_mask(flow_fw.detach(), flow_bw.detach(), "brox").unsqueeze(1)


class _SelfSup(torch.autograd.Function):
    @staticmethod
    def forward(ctx, student, teacher, teacher_mask, student_back, mode, norm, crop):
        out, dflow = ops.selfsup(teacher, teacher_mask, student, student_back, mode, norm, crop)
        ctx.save_for_backward(dflow)
        return out[0].float()

    @staticmethod
    def backward(ctx, up):
        # the kernel left d value / d student next to the value; what remains is the scalar from upstream
        return ctx.saved_tensors[0] * up, None, None, None, None, None, None


def _teacher_mask(teacher, teacher_back, mask, sigma_teacher, hw, crop):
    if mask == "none":
        return None
    norm = _normaliser(sigma_teacher, teacher.shape[-2:]) if mask == "gaussian" else 1.0
    return ops.fb_mask(teacher, teacher_back, mask, norm, False, hw, crop)


def _selfsup(student, student_back, teacher, teacher_mask, mask, sigma_student, crop):
    norm = _normaliser(sigma_student, teacher.shape[-2:]) if mask == "gaussian" else 1.0
    return _SelfSup.apply(student, teacher, teacher_mask, student_back.detach(), mask, norm, crop)


def _check_teacher(teacher_fw, teacher_bw, student, cropped):
    B, _, H, W = student.shape
    for t in (teacher_fw, teacher_bw):
        ok = t.dim() == 4 and t.shape[:2] == (B, 2) and (t.shape[2] >= H and t.shape[3] >= W if cropped else t.shape[2:] == (H, W))
        if not ok:
            raise ValueError(f"teacher flow {tuple(t.shape)} for student flow {tuple(student.shape)}"
                             + ("" if cropped else ": without crop_yx the teacher has the student's size"))
    if teacher_fw.shape != teacher_bw.shape:
        raise ValueError(f"teacher flows {tuple(teacher_fw.shape)} and {tuple(teacher_bw.shape)}")


@L.on_tensor_device
def self_supervision_loss(teacher_fw, teacher_bw, student_fw, student_bw, crop_yx=None, mask="gaussian", sigma_teacher=0.003,
                          sigma_student=0.03):
    """mean(m * sqrt((crop(teacher_fw) - student_fw)^2 + 1e-6)) with m = crop(c_t * valid_t) * (1 - c_s * valid_s), a scalar,
    differentiable in student_fw only.  The teacher's flows are [B,2,Hf,Wf] frames of which crop_yx [B,2] = (y, x) (host
    integers) gives the student's H x W window; without crop_yx they have the student's size.  Both gaussian masks are
    normalised by the teacher's size."""
    if mask not in MASKS:
        raise ValueError(f"unknown selfsup_mask {mask!r}")
    L.require_cuda_f32(teacher_fw, teacher_bw, student_fw, student_bw)
    _check_teacher(teacher_fw, teacher_bw, student_fw, crop_yx is not None)
    crop = ops.crop_offsets(crop_yx, student_fw.shape[0])
    teacher_fw, teacher_bw = teacher_fw.detach(), teacher_bw.detach()
    tmask = _teacher_mask(teacher_fw, teacher_bw, mask, sigma_teacher, student_fw.shape[-2:], crop)
    return _selfsup(student_fw, student_bw, teacher_fw, tmask, mask, sigma_student, crop)


class SmurfLoss:
    """raft/unsup_loss.py UnsupervisedLoss with every term, at the reference's defaults (mode 'unsup_per_update', smoothness
    and self-supervision at level 0, 'exponential' edge weighting with constant 150, gradient of every mask stopped;
    fb_sigma_teacher / fb_sigma_student are smurf_utils.py unsupervised_loss's arguments of that name).

    __call__(images, flows_fw, flows_bw, teacher_fw=None, teacher_bw=None, full_images=None, crop_yx=None)
            -> (loss, {'census', 'smooth1', 'smooth2', 'selfsup'})
        images, flows_fw/bw, full_images, crop_yx   as UnsupervisedLoss takes them
        teacher_fw/bw   the teacher's last predictions 0 -> 1 and 1 -> 0, [B,2,Hf,Wf] (the frames' size when full_images is
                        given, else the students'); needed when selfsup > 0.  Every prediction t is supervised by them.
    The dict holds the weighted, gamma-summed terms; loss is their sum.  With selfsup = 0 the result is UnsupervisedLoss's."""

    def __init__(self, census=1.0, smooth1=2.5, smooth2=0.0, selfsup=0.3, occlusion="wang", gamma=0.8, selfsup_mask="gaussian",
                 fb_sigma_teacher=0.003, fb_sigma_student=0.03):
        if occlusion not in ("wang", "brox", "none"):
            raise ValueError(f"unknown occlusion estimation {occlusion!r}")
        if selfsup_mask not in MASKS:
            raise ValueError(f"unknown selfsup_mask {selfsup_mask!r}")
        self.weights = {k: float(v) for k, v in (("census", census), ("smooth1", smooth1), ("smooth2", smooth2), ("selfsup", selfsup))
                        if v > 0}
        self.occlusion, self.gamma, self.selfsup_mask = occlusion, float(gamma), selfsup_mask
        self.sigma_teacher, self.sigma_student = float(fb_sigma_teacher), float(fb_sigma_student)

    def _census_mask(self, f, g):
        if self.occlusion == "none":
            return None
        if self.occlusion == "brox":
            return ops.fb_mask(f.detach(), g.detach(), "brox")
        return ops.range_map(g.detach(), clip=True)

    @L.on_tensor_device
    def __call__(self, images, flows_fw, flows_bw, teacher_fw=None, teacher_bw=None, full_images=None, crop_yx=None):
        if len(flows_fw) != len(flows_bw) or not flows_fw:
            raise ValueError("flows_fw and flows_bw: two lists of the same, non-zero length")
        selfsup = "selfsup" in self.weights
        if selfsup and (teacher_fw is None or teacher_bw is None):
            raise ValueError("selfsup > 0 needs the teacher's flows (teacher_fw, teacher_bw)")
        L.require_cuda_f32(*flows_fw, *flows_bw)
        B = flows_fw[0].shape[0]
        crop = ops.crop_offsets(crop_yx, B)
        if (full_images is None) != (crop is None):
            raise ValueError("full_images and crop_yx come together")
        frames = full_images is not None
        imgs = [t.detach() for t in (full_images if frames else images)]
        teachers = tmasks = None
        if selfsup:
            L.require_cuda_f32(teacher_fw, teacher_bw)
            _check_teacher(teacher_fw, teacher_bw, flows_fw[0], frames)
            teachers = (teacher_fw.detach(), teacher_bw.detach())
            # one mask per direction, shared by every prediction
            tmasks = [_teacher_mask(teachers[i], teachers[j], self.selfsup_mask, self.sigma_teacher, flows_fw[0].shape[-2:], crop)
                      for i, j in ((0, 1), (1, 0))]
        n = len(flows_fw)
        terms = {k: None for k in self.weights}
        for t, (ffw, fbw) in enumerate(zip(flows_fw, flows_bw)):
            decay = self.gamma ** (n - 1 - t)
            for i, j, f, g in ((0, 1, ffw, fbw), (1, 0, fbw, ffw)):
                one = {}
                if "census" in self.weights:
                    one["census"] = _Census.apply(f, imgs[i], imgs[j], self._census_mask(f, g), crop, frames)
                for k, order in (("smooth1", 1), ("smooth2", 2)):
                    if k in self.weights:
                        one[k] = _Smoothness.apply(f, imgs[i], order, 150.0, False, crop)
                if selfsup:
                    one["selfsup"] = _selfsup(f, g, teachers[i], tmasks[i], self.selfsup_mask, self.sigma_student, crop)
                for k, v in one.items():
                    v = v * (self.weights[k] * decay / 2.0)
                    terms[k] = v if terms[k] is None else terms[k] + v
        loss = None
        for v in terms.values():
            loss = v if loss is None else loss + v
        if loss is None:
            raise ValueError("every loss weight is zero")
        return loss, {k: terms[k].detach() if k in terms else torch.zeros((), device=flows_fw[0].device)
                      for k in ("census", "smooth1", "smooth2", "selfsup")}
