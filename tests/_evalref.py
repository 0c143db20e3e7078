"""Restatement of the reference's validation metrics (pytorch/evaluate.py:117-124 Sintel / Chairs, :150-165 KITTI), the
oracle of the flow-metrics tests: the per-pixel arithmetic in torch fp32 on the CPU, exactly the reference's expressions,
and the sums in float64 (math.fsum: correctly rounded, so the oracle itself carries no summation error).
test_evaluate_host.py pins it to values the reference's own functions returned (tests/golden/eval_metrics.npz)."""
import math

import numpy as np
import torch


def sqrt_rn(x):
    """Correctly rounded fp32 square root.  torch's fp32 `.sqrt()` on the CPU is not one on every build: the AVX-512 kernels of
    torch 2.10 return the neighbour below for about 0.7 % of arguments (13479 of 2e6 against numpy and against the float64
    root rounded to fp32), other builds do not, so an oracle written with it would change with the host.  The float64 root
    rounded to fp32 is the correctly rounded fp32 root (53 >= 2 * 24 + 2 bits: the double rounding is innocuous) everywhere;
    subtraction, multiplication, addition and division of torch's CPU kernels are IEEE and stay as the reference has them."""
    return x.double().sqrt().float()


def pixel_terms(pred, gt):
    """pred, gt: [2,H,W] fp32 CPU -> epe [H,W] fp32, outlier [H,W] bool (evaluate.py:150-151, 157)."""
    epe = sqrt_rn(torch.sum((pred - gt) ** 2, dim=0))
    mag = sqrt_rn(torch.sum(gt ** 2, dim=0))
    out = (epe > 3.0) & ((epe / mag) > 0.05)
    return epe, out


def sample_stats(pred, gt, valid=None):
    """The eight numbers fsraft_flow_metrics leaves per sample: n valid, epe sum, n(<1), n(<3), n(<5), n outliers, 0, 0."""
    epe, out = pixel_terms(pred.float().cpu(), gt.float().cpu())
    val = valid.cpu() >= 0.5 if valid is not None else torch.ones_like(out)         # evaluate.py:155
    e = epe[val].numpy()
    return np.array([e.size, math.fsum(e.astype(np.float64)), np.count_nonzero(e < 1), np.count_nonzero(e < 3),
                     np.count_nonzero(e < 5), int(out[val].sum()), 0, 0], dtype=np.float64)


def batch_stats(pred, gt, valid=None):
    return np.stack([sample_stats(pred[b], gt[b], None if valid is None else valid[b]) for b in range(pred.shape[0])])


def dataset_values(stats):
    """stats [S,8] of a dataset's samples -> what FlowMetrics.compute() reports."""
    stats = np.asarray(stats, dtype=np.float64)
    s = [math.fsum(stats[:, k]) for k in range(6)]
    with_pixels = stats[stats[:, 0] > 0]
    return {"epe": s[1] / s[0], "1px": s[2] / s[0], "3px": s[3] / s[0], "5px": s[4] / s[0], "f1": 100.0 * s[5] / s[0],
            "epe_per_image": math.fsum(with_pixels[:, 1] / with_pixels[:, 0]) / len(with_pixels),
            "pixels": int(s[0]), "images": len(with_pixels)}


def pad_offsets(H, W, mode):
    """(top, left) of the image inside its padded frame (core/utils/utils.py:10-17)."""
    ph, pw = -H % 8, -W % 8
    return (ph // 2 if mode == "sintel" else 0), pw // 2


def unpadded(pred, H, W, mode):
    top, left = pad_offsets(H, W, mode)
    return pred[..., top:top + H, left:left + W]


# Boundary pixels (gt, d = pred - gt) and what the reference's expressions make of them:
#   name            gt          d        <1  <3  <5  outlier
BOUNDARY = [
    ("epe==3",      (10., 0.),  (3., 0.), 0,  0,  1,  0),      # neither < 3 nor > 3
    ("epe==5",      (10., 0.),  (3., 4.), 0,  0,  0,  1),      # 5 is not < 5; 5 / 10 > 0.05
    ("ratio==0.05", (100., 0.), (5., 0.), 0,  0,  0,  0),      # fl32(5 / 100) == fl32(0.05): not >, torch compares in fp32
    ("gt==0",       (0., 0.),   (4., 0.), 0,  0,  1,  1),      # 4 / 0 = inf > 0.05
    ("epe==1",      (10., 0.),  (0., 1.), 0,  1,  1,  0),
]


def boundary_frame(H=3, W=5):
    """A 3 x 5 frame holding the BOUNDARY pixels in its first places and exact zeros of error elsewhere, with valid == 0.5 on
    the first pixel (counts) and a value just below 0.5 on the last (does not).  -> pred, gt [1,2,H,W], valid [1,H,W]"""
    gt = torch.full((1, 2, H, W), 7.0)
    pred = gt.clone()
    for i, (_, g, d, *_rest) in enumerate(BOUNDARY):
        y, x = divmod(i, W)
        gt[0, :, y, x] = torch.tensor(g)
        pred[0, :, y, x] = torch.tensor(g) + torch.tensor(d)
    valid = torch.ones(1, H, W)
    valid[0, 0, 0] = 0.5
    valid[0, H - 1, W - 1] = 0.49999997
    return pred, gt, valid
