"""The unsupervised (SMURF) loss of the reference's third trainer on the device: raft/unsup_loss.py UnsupervisedLoss over
raft/smurf_models/smurf_utils.py (census_loss, first / second_order_smoothness_loss, compute_range_map,
compute_occlusions_wang), on csrc/unsup_loss.hip.

    range_map(flow)                                  compute_range_map(flow, downsampling_factor=1)
    occlusion_mask(flow_bw, method)                  compute_occlusions(..., occlusions_are_zeros=True)
    census_loss(image1, image2, flow, mask, ...)     warp + mask_invalid + census_loss
    smoothness_loss(image, flow, order, ...)         first / second_order_smoothness_loss at level 0
    UnsupervisedLoss(...)                            UnsupervisedLoss.call with mode='unsup_per_update'

PyTorch layout: images [B,3,H,W] in [0,1], flows [B,2,H,W] with channel 0 = x (the reference reverses its flows to (row, col)
first; that is absorbed).  Everything is differentiable with respect to the flows; images and masks are constants (the
reference stops the gradient of the mask).  CUDA (ROCm) fp32 tensors only: there is no CPU implementation.

Not implemented, and refused with NotImplementedError: selfsup > 0 (needs the teacher / student crop-and-resize machinery),
occlusion 'brox' and mode 'unsup_final_update'.  The first two are what selfsup_loss.SmurfLoss adds (the reference's transform
turned out to be a plain crop); this module's behaviour is unchanged.
"""
import torch

from . import _lib as L
from . import ops


@L.on_tensor_device
def range_map(flow):
    """[B,2,H,W] -> [B,1,H,W]: how often every pixel is hit by q + flow(q), with bilinear weights."""
    with torch.no_grad():
        return ops.range_map(flow.detach()).unsqueeze(1)


@L.on_tensor_device
def occlusion_mask(flow_bw, method="wang"):
    """The mask of the direction opposite to `flow_bw` (1 = visible): 'wang' clip(range_map(flow_bw), 0, 1), 'none' all ones."""
    if method == "brox":
        raise NotImplementedError("occlusion 'brox' (forward-backward consistency) is not implemented; use 'wang' or 'none'")
    if method not in ("wang", "none"):
        raise ValueError(f"unknown occlusion estimation {method!r}")
    with torch.no_grad():
        if method == "none":
            L.require_cuda_f32(flow_bw)
            return torch.ones_like(flow_bw[:, :1])
        return ops.range_map(flow_bw.detach(), clip=True).unsqueeze(1)


class _Census(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flow, img1, img2, mask, crop, img1_frame):
        out, grayB, hplane = ops.census_fwd(img1, img2, flow, mask, crop, img1_frame)
        ctx.save_for_backward(flow, img1, img2, grayB, hplane, out)
        ctx.crop, ctx.img1_frame = crop, img1_frame
        return out[0].float()

    @staticmethod
    def backward(ctx, up):
        flow, img1, img2, grayB, hplane, out = ctx.saved_tensors
        dflow = ops.census_bwd(img1, img2, flow, grayB, hplane, up.contiguous(), out[1:], ctx.crop, ctx.img1_frame)
        return dflow, None, None, None, None, None


class _Smoothness(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flow, img, order, edge_constant, gaussian, crop):
        out, dflow = ops.smoothness(img, flow, order, edge_constant, gaussian, crop)
        ctx.save_for_backward(dflow)
        return out[0].float()

    @staticmethod
    def backward(ctx, up):
        # the kernel left d value / d flow next to the value; what remains is the scalar from upstream
        return ctx.saved_tensors[0] * up, None, None, None, None, None


def _mask3(mask):
    if mask is None:
        return None
    return (mask[:, 0] if mask.dim() == 4 else mask).detach()


@L.on_tensor_device
def census_loss(image1, image2, flow, mask, full_image2=None, crop_yx=None, full_image1=None):
    """The census loss of image1 against image2 warped by `flow` [B,2,H,W], weighted by mask * valid ([B,1,H,W] or [B,H,W], None:
    ones; no gradient).  With full_image2 [B,3,Hf,Wf] and crop_yx [B,2] (y, x; host integers) the warp samples the full frame at
    crop + p + flow(p) and tests validity against it (image2 is then unused and may be None); full_image1 likewise replaces
    image1 by the window of its frame, read in place."""
    B = flow.shape[0]
    if full_image2 is None and crop_yx is not None:
        raise ValueError("crop_yx needs full_image2")
    img2 = image2 if full_image2 is None else full_image2
    frame1 = full_image1 is not None
    if frame1 and full_image2 is None:
        raise ValueError("full_image1 needs full_image2 and crop_yx")
    return _Census.apply(flow, (full_image1 if frame1 else image1).detach(), img2.detach(), _mask3(mask),
                         ops.crop_offsets(crop_yx, B), frame1)


@L.on_tensor_device
def smoothness_loss(image, flow, order=1, edge_constant=150.0, weighting="exponential", full_image=None, crop_yx=None):
    """Edge-aware first (order=1) or second (order=2) order smoothness of `flow` under the edges of `image` (or of the window
    of full_image at crop_yx)."""
    if order not in (1, 2):
        raise ValueError(f"smoothness order {order!r}: 1 or 2")
    if weighting not in ("exponential", "gaussian"):
        raise ValueError("Only gaussian or exponential edge weighting implemented.")
    img = image if full_image is None else full_image
    if full_image is None and crop_yx is not None:
        raise ValueError("crop_yx needs full_image")
    return _Smoothness.apply(flow, img.detach(), order, float(edge_constant), weighting == "gaussian",
                             ops.crop_offsets(crop_yx, flow.shape[0]))


class UnsupervisedLoss:
    """raft/unsup_loss.py UnsupervisedLoss (mode 'unsup_per_update', smoothness at level 0, 'exponential' edge weighting with
    constant 150, gradient of the mask stopped).  selfsup defaults to 0 here -- the reference's default is 0.3 -- because the
    self-supervision term is not implemented; any value > 0 is refused.

    __call__(images, flows_fw, flows_bw, full_images=None, crop_yx=None) -> (loss, {'census', 'smooth1', 'smooth2'})
        images       (image1, image2), [B,3,H,W] each (may be None when full_images is given)
        flows_fw/bw  the models' full-resolution predictions 0 -> 1 and 1 -> 0, lists of [B,2,H,W]
        full_images  (frame1, frame2), [B,3,Hf,Wf] each, with crop_yx [B,2] = (y, x) of the window (host integers)
    The dict holds the weighted, gamma-summed terms; loss is their sum."""

    def __init__(self, census=1.0, smooth1=2.5, smooth2=0.0, selfsup=0.0, occlusion="wang", gamma=0.8, mode="unsup_per_update"):
        if selfsup > 0:
            raise NotImplementedError("selfsup > 0 needs the teacher / student crop-and-resize machinery, which is not implemented "
                                      "here (the reference's default is 0.3; pass 0, or use selfsup_loss.SmurfLoss)")
        if occlusion == "brox":
            raise NotImplementedError("occlusion 'brox' (forward-backward consistency) is not implemented; use 'wang' or 'none'")
        if occlusion not in ("wang", "none"):
            raise ValueError(f"unknown occlusion estimation {occlusion!r}")
        if mode != "unsup_per_update":
            raise NotImplementedError(f"mode {mode!r} is not implemented: only 'unsup_per_update'")
        self.weights = {k: float(v) for k, v in (("census", census), ("smooth1", smooth1), ("smooth2", smooth2)) if v > 0}
        self.occlusion, self.gamma = occlusion, float(gamma)

    @L.on_tensor_device
    def __call__(self, images, flows_fw, flows_bw, full_images=None, crop_yx=None):
        if len(flows_fw) != len(flows_bw) or not flows_fw:
            raise ValueError("flows_fw and flows_bw: two lists of the same, non-zero length")
        L.require_cuda_f32(*flows_fw, *flows_bw)
        B = flows_fw[0].shape[0]
        crop = ops.crop_offsets(crop_yx, B)
        if (full_images is None) != (crop is None):
            raise ValueError("full_images and crop_yx come together")
        frames = full_images is not None
        imgs = [t.detach() for t in (full_images if frames else images)]
        n = len(flows_fw)
        terms = {k: None for k in self.weights}
        for t, (ffw, fbw) in enumerate(zip(flows_fw, flows_bw)):
            decay = self.gamma ** (n - 1 - t)
            for i, j, f, g in ((0, 1, ffw, fbw), (1, 0, fbw, ffw)):
                one = {}
                if "census" in self.weights:
                    mask = None if self.occlusion == "none" else ops.range_map(g.detach(), clip=True)
                    one["census"] = _Census.apply(f, imgs[i], imgs[j], mask, crop, frames)
                for k, order in (("smooth1", 1), ("smooth2", 2)):
                    if k in self.weights:
                        one[k] = _Smoothness.apply(f, imgs[i], order, 150.0, False, crop)
                for k, v in one.items():
                    v = v * (self.weights[k] * decay / 2.0)
                    terms[k] = v if terms[k] is None else terms[k] + v
        loss = None
        for v in terms.values():
            loss = v if loss is None else loss + v
        if loss is None:
            raise ValueError("every loss weight is zero")
        return loss, {k: terms[k].detach() if k in terms else torch.zeros((), device=flows_fw[0].device)
                      for k in ("census", "smooth1", "smooth2")}
