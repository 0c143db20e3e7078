#!/usr/bin/env python3
"""Generate tests/golden/eval_metrics.npz by running the REFERENCE's own validation functions (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_eval_golden.py --reference <reference checkout>

pytorch/evaluate.py imports matplotlib, PIL and the dataset module at module level and builds its datasets inside each
function, so it cannot be imported or pointed at other data.  As make_golden.py does for sequence_loss, the FunctionDefs
of validate_kitti, validate_sintel and validate_chairs are taken out of the module's syntax tree and executed in a small
scope: torch, np, the reference's InputPadder, and a stub `datasets` namespace whose classes return seeded samples.  The
images are a torch.Tensor subclass whose .cuda() returns itself, the model is a stub that replays stored full-resolution
(padded) predictions, so everything runs on the CPU and what is measured is the reference's metric code alone.

Stored: ground truth, valid masks, the replayed padded predictions, the image shapes and the values the reference
returned.  No reference source is copied; the fixture is data.
"""
import argparse
import ast
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
N = 3                                    # samples per dataset
SEED = 20240


class Image(torch.Tensor):
    def cuda(self, *args, **kwargs):
        return self


class ReplayModel:
    """model(image1, image2, iters=, test_mode=True) -> (None, the next stored prediction [1,2,Hp,Wp])"""

    def __init__(self, preds):
        self.preds, self.i = preds, 0

    def eval(self):
        return self

    def __call__(self, image1, image2, iters=None, flow_init=None, test_mode=False):
        pred = self.preds[self.i]
        self.i += 1
        assert test_mode and image1.shape == image2.shape and tuple(image1.shape[-2:]) == tuple(pred.shape[-2:]), image1.shape
        return None, pred[None]


def reference_functions(root, names, scope):
    tree = ast.parse(open(os.path.join(root, "pytorch", "evaluate.py")).read())
    for name in names:
        fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name][0]
        exec(compile(ast.Module(body=[fn], type_ignores=[]), "evaluate.py:" + name, "exec"), scope)
    return [scope[n] for n in names]


def make_case(rng, H, W, Hp, Wp, top, left, big_gt):
    """gt ~ N(0, 8 px) (a quarter of the pixels twelve times that when big_gt: |gt| large enough for epe / |gt| <= 0.05 at
    epe > 3); the error's scale is log-uniform in [0.2, 8] px per pixel, so every threshold has members on both sides.  The
    padding of the prediction holds values far from any flow: a kernel that reads it shows."""
    gt = rng.standard_normal((N, 2, H, W)) * 8.0
    if big_gt:
        gt *= np.where(rng.random((N, 1, H, W)) < 0.25, 12.0, 1.0)
    err = rng.standard_normal((N, 2, H, W)) * np.exp(rng.uniform(np.log(0.2), np.log(8.0), (N, 1, H, W)))
    pred = 1000.0 + rng.standard_normal((N, 2, Hp, Wp))
    pred[:, :, top:top + H, left:left + W] = gt + err
    return torch.from_numpy(gt.astype(np.float32)), torch.from_numpy(pred.astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("FSRAFT_REFERENCE"), required="FSRAFT_REFERENCE" not in os.environ,
                    help="checkout of the reference project (the directory that holds pytorch/)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(a.reference, "pytorch"))
    from core.utils.utils import InputPadder            # the reference's

    rng = np.random.default_rng(SEED)
    image = lambda H, W: torch.zeros(3, H, W).as_subclass(Image)          # noqa: E731  (content is never looked at)
    out = {}

    # KITTI: 37 x 61 pads to 40 x 64 at the bottom and 1 / 2 columns left / right; masks ~70 % valid
    H, W = 37, 61
    gt, pred = make_case(rng, H, W, 40, 64, 0, 1, True)
    valid = torch.from_numpy((rng.random((N, H, W)) < 0.7).astype(np.float32))
    kitti = [(image(H, W), image(H, W), gt[i], valid[i]) for i in range(N)]
    out.update(kitti_gt=gt, kitti_valid=valid, kitti_pred=pred, kitti_shape=np.array([N, H, W]))

    # Sintel: the same size pads 1 / 2 rows top / bottom; one set of predictions per dstype
    gt, pred_c = make_case(rng, H, W, 40, 64, 1, 1, False)
    pred_f = pred_c.clone()
    pred_f[:, :, 1:1 + H, 1:1 + W] += torch.from_numpy(rng.standard_normal((N, 2, H, W)).astype(np.float32))
    sintel = [(image(H, W), image(H, W), gt[i], None) for i in range(N)]
    out.update(sintel_gt=gt, sintel_pred_clean=pred_c, sintel_pred_final=pred_f, sintel_shape=np.array([N, H, W]))

    # Chairs: 40 x 64, no padding
    Hc, Wc = 40, 64
    gtc, predc = make_case(rng, Hc, Wc, Hc, Wc, 0, 0, False)
    chairs = [(image(Hc, Wc), image(Hc, Wc), gtc[i], None) for i in range(N)]
    out.update(chairs_gt=gtc, chairs_pred=predc, chairs_shape=np.array([N, Hc, Wc]))

    models = {"kitti": ReplayModel(pred), "chairs": ReplayModel(predc), "sintel": ReplayModel(torch.cat([pred_c, pred_f]))}
    datasets = types.SimpleNamespace(
        KITTI=lambda split: kitti, FlyingChairs=lambda split: chairs,
        MpiSintel=lambda split, dstype: sintel)                                          # 'clean' is walked first, then 'final'
    scope = {"torch": torch, "np": np, "InputPadder": InputPadder, "datasets": datasets}
    v_kitti, v_sintel, v_chairs = reference_functions(a.reference, ["validate_kitti", "validate_sintel", "validate_chairs"], scope)

    r = v_kitti(models["kitti"])
    out["kitti_ref"] = np.array([r["kitti-epe"], r["kitti-f1"]], dtype=np.float64)
    r = v_sintel(models["sintel"])
    out["sintel_ref"] = np.array([r["clean"], r["final"]], dtype=np.float64)
    r = v_chairs(models["chairs"])
    out["chairs_ref"] = np.array([r["chairs"]], dtype=np.float64)
    assert models["kitti"].i == N and models["sintel"].i == 2 * N and models["chairs"].i == N

    path = os.path.join(HERE, "eval_metrics.npz")
    np.savez_compressed(path, **{k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()})
    print(f"eval_metrics.npz  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
