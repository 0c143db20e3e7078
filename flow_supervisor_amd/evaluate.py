"""Validation and submission drivers with the reference's names (pytorch/evaluate.py), metrics reduced on the device.

    FlowMetrics                                   running EPE / 1px / 3px / 5px / F1 statistics (fsraft_flow_metrics)
    validate_chairs / validate_sintel / validate_kitti / validate_kitti2012      evaluate.py:76-207
    create_sintel_submission / create_kitti_submission                           evaluate.py:23-73
    validate_things / validate_sintel_occ                                        GMA/evaluate.py:174-207, 247-292
    create_sintel_submission_vis / create_kitti_submission_vis                   GMA/evaluate.py:53-96, 121-149
    demo                                                                         GMA/evaluate_single.py:45-75, extract_flow.py:118-156

The reference copies every full-resolution prediction to the host (`padder.unpad(flow_pr[0]).cpu()`, one sync per frame)
and reduces there.  Here the prediction stays where it is: csrc/flow_metrics.hip reads the un-padded view of the padded
prediction in place, does the reference's fp32 arithmetic per pixel, sums in fp64 and keeps the running totals in a device
accumulator; a dataset pass synchronises once, in FlowMetrics.compute().

The reference's functions build their own datasets (core/datasets.py, not part of this package); these take them as an
argument: any iterable of `(image1, image2, flow_gt, valid_or_None)` -- what the reference's dataset classes yield -- and a
`model` callable as `model(image1, image2, iters=, flow_init=, test_mode=True) -> (flow_low, flow_up)`.
"""
import os

import torch

from . import _lib as L
from . import ops
from .core.utils.utils import InputPadder, forward_interpolate
from .raft_utils import frame_utils


class FlowMetrics:
    """Running flow statistics on the device.

    update() enqueues one fsraft_flow_metrics call on the current stream and returns: no device -> host copy, no sync.
    compute() synchronises once and returns plain Python numbers:
        epe             mean end-point error over all valid pixels (evaluate.py:121, Sintel / Chairs)
        1px, 3px, 5px   fraction of valid pixels with epe < 1 / 3 / 5 (evaluate.py:122-124)
        f1              100 * outliers / valid pixels, outlier = epe > 3 and epe / |gt| > 0.05 (evaluate.py:157, 165)
        epe_per_image   mean over images of the image's own mean epe (evaluate.py:158, 164: KITTI's EPE)
        pixels, images  valid pixels counted, images that had at least one
    A sample without a valid pixel contributes to no mean and is not counted in `images` (the reference would put a NaN
    into its list there; its datasets have no such frame).  Before any valid pixel the means are NaN."""

    def __init__(self, device=None):
        self.device = torch.device(device) if device is not None else None
        self._acc = None
        self._last = None
        self._scratch = {}

    def reset(self):
        if self._acc is not None:
            self._acc.zero_()
        self._last = None

    def _operand(self, t, dims, what):
        if t.dim() == dims - 1:
            t = t[None]
        if t.dim() != dims:
            raise ValueError(f"FlowMetrics.update: {what} has shape {tuple(t.shape)}")
        t = t.detach()
        if t.device != self.device or t.dtype != torch.float32:
            t = t.to(device=self.device, dtype=torch.float32)
        return t if t.stride(-1) == 1 or t.shape[-1] == 1 else t.contiguous()

    def update(self, flow_pred, flow_gt, valid=None):
        """flow_pred, flow_gt: [2,H,W] or [B,2,H,W]; valid: [H,W] / [B,H,W] or None (every pixel counts).  flow_pred must be
        on the device and may be any view with a unit x stride (InputPadder.unpad of the padded prediction is read in place);
        flow_gt and valid are moved to the device when they are on the host."""
        L.require_cuda_f32(flow_pred)
        if self.device is None:
            self.device = flow_pred.device
        elif self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if flow_pred.device != self.device:
            raise RuntimeError(f"FlowMetrics on {self.device} got a prediction on {flow_pred.device}")
        pred = self._operand(flow_pred, 4, "flow_pred")
        gt = self._operand(flow_gt, 4, "flow_gt")
        val = self._operand(valid, 3, "valid") if valid is not None else None
        B, _, H, W = pred.shape
        with torch.cuda.device(self.device):
            if self._acc is None:
                self._acc = torch.zeros(8, device=self.device, dtype=torch.float64)
            scratch = self._scratch.get((B, H * W))
            if scratch is None:
                scratch = self._scratch[(B, H * W)] = torch.empty(ops.flow_metrics_scratch_bytes(B, H, W) // 8, device=self.device,
                                                                  dtype=torch.float64)
            self._last = torch.empty(B, 8, device=self.device, dtype=torch.float64)
            ops.flow_metrics(pred, gt, val, self._last, self._acc, scratch)

    def last_samples(self):
        """[B,8] fp64 device tensor of the last update: per sample n valid, epe sum, n(<1), n(<3), n(<5), n outliers, 0, 0."""
        return self._last

    def compute(self):
        a = self._acc.cpu().tolist() if self._acc is not None else [0.0] * 8
        n, images = a[0], a[7]
        nan = float("nan")
        return {"epe": a[1] / n if n else nan, "1px": a[2] / n if n else nan, "3px": a[3] / n if n else nan,
                "5px": a[4] / n if n else nan, "f1": 100.0 * a[5] / n if n else nan,
                "epe_per_image": a[6] / images if images else nan, "pixels": int(n), "images": int(images)}


def _device(device):
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def _eval_mode(model):
    if hasattr(model, "eval"):
        model.eval()


def _batches(dataset, batch_size):
    """Consecutive samples of equal shapes, stacked: lists of at most batch_size samples."""
    group, key = [], None
    for sample in dataset:
        k = tuple(None if t is None else tuple(t.shape) for t in sample[:4])
        if group and (k != key or len(group) == batch_size):
            yield group
            group = []
        group.append(sample)
        key = k
    if group:
        yield group


def _stack(group, i, device):
    return torch.stack([s[i] for s in group]).to(device)


def _validate(model, dataset, iters, batch_size, device, pad_mode, use_valid):
    """One dataset pass: the FlowMetrics result.  pad_mode None: no padding (Chairs)."""
    _eval_mode(model)
    device = _device(device)
    metrics = FlowMetrics(device)
    for group in _batches(dataset, max(1, int(batch_size))):
        image1, image2 = _stack(group, 0, device), _stack(group, 1, device)
        flow_gt = _stack(group, 2, device)
        valid = _stack(group, 3, device) if use_valid else None
        if pad_mode is not None:
            padder = InputPadder(image1.shape, mode=pad_mode)
            image1, image2 = padder.pad(image1, image2)
        _, flow_pr = model(image1, image2, iters=iters, test_mode=True)
        metrics.update(padder.unpad(flow_pr) if pad_mode is not None else flow_pr, flow_gt, valid)
    return metrics.compute()


@torch.no_grad()
def validate_chairs(model, dataset, iters=24, batch_size=1, device=None):
    """Evaluation on the FlyingChairs validation split (evaluate.py:76-94); `valid` is ignored, as there."""
    epe = _validate(model, dataset, iters, batch_size, device, None, False)["epe"]
    print("Validation Chairs EPE: %f" % epe)
    return {"chairs": epe}


@torch.no_grad()
def validate_sintel(model, datasets, iters=32, batch_size=1, device=None):
    """Validation on the Sintel training split (evaluate.py:97-129).  datasets: a mapping dstype -> dataset (the reference
    walks 'clean' and 'final'), visited in the mapping's order; `valid` is ignored, as there."""
    results = {}
    for dstype, dataset in datasets.items():
        m = _validate(model, dataset, iters, batch_size, device, "sintel", False)
        print("Validation (%s) EPE: %f, 1px: %f, 3px: %f, 5px: %f" % (dstype, m["epe"], m["1px"], m["3px"], m["5px"]))
        results[dstype] = m["epe"]
    return results


@torch.no_grad()
def validate_kitti(model, dataset, iters=24, batch_size=1, device=None):
    """Validation on the KITTI-2015 training split (evaluate.py:132-168): EPE is the mean of the images' means, F1 the
    outlier percentage over all valid pixels."""
    m = _validate(model, dataset, iters, batch_size, device, "kitti", True)
    print("Validation KITTI: %f, %f" % (m["epe_per_image"], m["f1"]))
    return {"kitti-epe": m["epe_per_image"], "kitti-f1": m["f1"]}


validate_kitti2012 = validate_kitti      # evaluate.py:171-207 is the same function over another dataset


@torch.no_grad()
def create_sintel_submission(model, dataset, iters=32, warm_start=False, output_path="sintel_submission", device=None):
    """Sintel leaderboard files (evaluate.py:23-52) for one pass (the reference loops over dstype and writes below
    output_path/dstype: pass that directory here).  dataset yields (image1, image2, (sequence, frame)); the frames are
    written to output_path/sequence/frame%04d.flo, numbered frame + 1.  warm_start: the next frame of a sequence starts
    from forward_interpolate of this frame's low-resolution flow (evaluate.py:42-43), on the device."""
    _eval_mode(model)
    device = _device(device)
    flow_prev, sequence_prev = None, None
    for image1, image2, (sequence, frame) in dataset:
        if sequence != sequence_prev:
            flow_prev = None
        padder = InputPadder(image1.shape)
        image1, image2 = padder.pad(image1[None].to(device), image2[None].to(device))
        flow_low, flow_pr = model(image1, image2, iters=iters, flow_init=flow_prev, test_mode=True)
        flow = padder.unpad(flow_pr[0]).permute(1, 2, 0).cpu().numpy()
        if warm_start:
            flow_prev = forward_interpolate(flow_low[0])[None].to(device)
        output_dir = os.path.join(output_path, sequence)
        os.makedirs(output_dir, exist_ok=True)
        frame_utils.writeFlow(os.path.join(output_dir, "frame%04d.flo" % (frame + 1)), flow)
        sequence_prev = sequence


@torch.no_grad()
def create_kitti_submission(model, dataset, iters=24, output_path="kitti_submission", device=None):
    """KITTI leaderboard files (evaluate.py:55-73).  dataset yields (image1, image2, (frame_id,)); written through
    frame_utils.writeFlowKITTI (OpenCV where installed, frame_utils.writePNG otherwise)."""
    _eval_mode(model)
    device = _device(device)
    os.makedirs(output_path, exist_ok=True)
    for image1, image2, (frame_id,) in dataset:
        padder = InputPadder(image1.shape, mode="kitti")
        image1, image2 = padder.pad(image1[None].to(device), image2[None].to(device))
        _, flow_pr = model(image1, image2, iters=iters, test_mode=True)
        flow = padder.unpad(flow_pr[0]).permute(1, 2, 0).cpu().numpy()
        frame_utils.writeFlowKITTI(os.path.join(output_path, frame_id), flow)


# ---------------------------------------------------------------------------------------------------------------------
# The GMA tree's drivers (pytorch/GMA/evaluate.py, GMA/evaluate_single.py) and the TF tree's extract_flow.py: validation on
# further splits, and submission / demo loops that also leave a picture of every flow.  Colouring (core/utils/flow_viz.py,
# raft_tf.visualize_flows) and the KITTI encoding (ops.flow_kitti16) run on the device on the un-padded view of the padded
# prediction; 3 bytes a pixel come back for a picture, 6 for a KITTI file, where the reference copies 8 and colours in NumPy.

@torch.no_grad()
def validate_things(model, datasets, iters=6, batch_size=1, device=None):
    """Validation on the FlyingThings3D test split (GMA/evaluate.py:174-207).  datasets: a mapping dstype -> dataset (the
    reference walks 'frames_cleanpass' and 'frames_finalpass'), visited in the mapping's order; `valid` is ignored, as there."""
    results = {}
    for dstype, dataset in datasets.items():
        print(f"Dataset length {len(dataset)}")
        m = _validate(model, dataset, iters, batch_size, device, "sintel", False)
        print("Validation (%s) EPE: %f, 1px: %f, 3px: %f, 5px: %f" % (dstype, m["epe"], m["1px"], m["3px"], m["5px"]))
        results[dstype] = m["epe"]
    return results


@torch.no_grad()
def validate_sintel_occ(model, datasets, iters=6, batch_size=1, device=None):
    """Validation on the Sintel training split with occlusion masks (GMA/evaluate.py:247-292).  datasets: a mapping
    dstype -> dataset yielding (image1, image2, flow_gt, valid, occ[, path]), occ a [H,W] mask that is true (non-zero) on
    occluded pixels.  Prints the reference's two lines per dstype -- EPE and 1 / 3 / 5 px over all pixels, then EPE over the
    occluded and the non-occluded ones -- from three FlowMetrics (valid = None, occ, ~occ), and returns {dstype: epe}.  The
    mean over an empty region is NaN, as NumPy's is."""
    _eval_mode(model)
    device = _device(device)
    results = {}
    for dstype, dataset in datasets.items():
        m_all, m_occ, m_noc = FlowMetrics(device), FlowMetrics(device), FlowMetrics(device)
        for group in _batches(dataset, max(1, int(batch_size))):
            image1, image2 = _stack(group, 0, device), _stack(group, 1, device)
            flow_gt = _stack(group, 2, device)
            occ = (_stack(group, 4, device) != 0).float()
            padder = InputPadder(image1.shape)
            image1, image2 = padder.pad(image1, image2)
            _, flow_pr = model(image1, image2, iters=iters, test_mode=True)
            flow = padder.unpad(flow_pr)
            m_all.update(flow, flow_gt)
            m_occ.update(flow, flow_gt, occ)
            m_noc.update(flow, flow_gt, 1.0 - occ)
        m = m_all.compute()
        print("Validation (%s) EPE: %f, 1px: %f, 3px: %f, 5px: %f" % (dstype, m["epe"], m["1px"], m["3px"], m["5px"]))
        print("Occ epe: %f, Noc epe: %f" % (m_occ.compute()["epe"], m_noc.compute()["epe"]))
        results[dstype] = m["epe"]
    return results


def _save_picture(path, img):
    """img: device uint8 [H,W,3] -> an 8-bit RGB PNG (3 bytes a pixel cross to the host)."""
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    frame_utils.writePNG(path, img.cpu().numpy())


@torch.no_grad()
def create_sintel_submission_vis(model, dataset, iters=32, warm_start=False, output_path="sintel_submission",
                                 vis_path="vis_test", device=None):
    """create_sintel_submission plus one picture per frame (GMA/evaluate.py:53-96): the .flo files as above, and
    vis_path/flow/<test_id>.png, the flow on the colour wheel, test_id counting the dataset's frames from 0 (the reference
    hard-codes vis_test/RAFT/<dstype>/flow/; pass that directory here).  The picture is coloured on the device."""
    from .core.utils import flow_viz
    _eval_mode(model)
    device = _device(device)
    flow_prev, sequence_prev = None, None
    for test_id, (image1, image2, (sequence, frame)) in enumerate(dataset):
        if sequence != sequence_prev:
            flow_prev = None
        padder = InputPadder(image1.shape)
        image1, image2 = padder.pad(image1[None].to(device), image2[None].to(device))
        flow_low, flow_pr = model(image1, image2, iters=iters, flow_init=flow_prev, test_mode=True)
        flow_dev = padder.unpad(flow_pr[0])
        _save_picture(os.path.join(vis_path, "flow", "%d.png" % test_id), flow_viz.flow_to_image(flow_dev))
        flow = flow_dev.permute(1, 2, 0).cpu().numpy()
        if warm_start:
            flow_prev = forward_interpolate(flow_low[0])[None].to(device)
        output_dir = os.path.join(output_path, sequence)
        os.makedirs(output_dir, exist_ok=True)
        frame_utils.writeFlow(os.path.join(output_dir, "frame%04d.flo" % (frame + 1)), flow)
        sequence_prev = sequence


@torch.no_grad()
def create_kitti_submission_vis(model, dataset, iters=24, output_path="kitti_submission", vis_path="vis_kitti", device=None):
    """create_kitti_submission plus one picture per frame (GMA/evaluate.py:121-149): output_path/<frame_id>, the 16-bit PNG,
    encoded on the device (ops.flow_kitti16) and written by frame_utils.writeFlowKITTI16, and vis_path/flow/<test_id>.png, the
    flow on the colour wheel (the reference hard-codes vis_kitti/flow/)."""
    from .core.utils import flow_viz
    _eval_mode(model)
    device = _device(device)
    os.makedirs(output_path, exist_ok=True)
    for test_id, (image1, image2, (frame_id,)) in enumerate(dataset):
        padder = InputPadder(image1.shape, mode="kitti")
        image1, image2 = padder.pad(image1[None].to(device), image2[None].to(device))
        _, flow_pr = model(image1, image2, iters=iters, test_mode=True)
        flow_dev = padder.unpad(flow_pr)
        with torch.cuda.device(device):
            rgb16 = ops.flow_kitti16(flow_dev.detach())
        frame_utils.writeFlowKITTI16(os.path.join(output_path, frame_id), rgb16[0].cpu().numpy())
        _save_picture(os.path.join(vis_path, "flow", "%d.png" % test_id), flow_viz.flow_to_image(flow_dev[0]))


def _load_image(path):
    """An image file -> float [3,H,W] in 0 .. 255 on the host (evaluate_single.py:24-27).  PIL where importable; PNG files
    through frame_utils.readPNG otherwise."""
    import numpy as np
    try:
        from PIL import Image
    except ImportError:
        if not path.lower().endswith(".png"):
            raise RuntimeError(f"demo: reading {path} needs PIL (only PNG files are decoded without it)")
        img = frame_utils.readPNG(path)
        if img.dtype == np.uint16:
            img = (img >> 8).astype(np.uint8)
    else:
        img = np.array(Image.open(path).convert("RGB")).astype(np.uint8)
    if img.ndim == 2:
        img = np.stack([img] * 3, axis=-1)
    return torch.from_numpy(np.ascontiguousarray(img[:, :, :3])).permute(2, 0, 1).float()


@torch.no_grad()
def demo(model, frames, output_path, iters=12, style="wheel", device=None):
    """Flow and a picture of it for every consecutive pair of frames (GMA/evaluate_single.py:45-75 with style 'wheel',
    extract_flow.py:118-156 with style 'hsv').  frames: a directory, whose *.png and *.jpg files are taken in sorted order, or
    a list of image tensors [3,H,W] in 0 .. 255.  Writes output_path/flo/<name>_flow.flo and output_path/vis/<name>_flow.png,
    <name> being the first frame's file name without its extension, or its index as %06d for tensors.  Returns the names."""
    import glob
    from .core.utils import flow_viz
    from .raft_tf.visualize import visualize_flows
    if style not in ("wheel", "hsv"):
        raise ValueError(f"demo: style is 'wheel' or 'hsv', got {style!r}")
    _eval_mode(model)
    device = _device(device)
    if isinstance(frames, (str, os.PathLike)):
        files = sorted(glob.glob(os.path.join(frames, "*.png")) + glob.glob(os.path.join(frames, "*.jpg")))
        names = [os.path.splitext(os.path.basename(f))[0] for f in files]
        load = _load_image
    else:
        files, names, load = list(frames), ["%06d" % i for i in range(len(frames))], (lambda t: t)
    os.makedirs(os.path.join(output_path, "flo"), exist_ok=True)
    written = []
    for k in range(len(files) - 1):
        image1, image2 = load(files[k])[None].float().to(device), load(files[k + 1])[None].float().to(device)
        padder = InputPadder(image1.shape)
        image1, image2 = padder.pad(image1, image2)
        _, flow_up = model(image1, image2, iters=iters, test_mode=True)
        flow = padder.unpad(flow_up[0])
        if style == "wheel":
            img = flow_viz.flow_to_image(flow)
        else:
            img = visualize_flows(flow.permute(1, 2, 0)[None], as_uint8=True)[0]
        frame_utils.writeFlow(os.path.join(output_path, "flo", names[k] + "_flow.flo"), flow.permute(1, 2, 0).cpu().numpy())
        _save_picture(os.path.join(output_path, "vis", names[k] + "_flow.png"), img)
        written.append(names[k])
    return written
