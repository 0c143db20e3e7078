#!/usr/bin/env python3
"""Generate tests/golden/flow_viz.npz by running the REFERENCE's own pytorch/core/utils/flow_viz.py (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_flow_viz.py --reference <reference checkout>

The module is pure NumPy and is loaded by path.  Stored: make_colorwheel(), and per shape (1x1, 3x5, 37x61, 40x64) a seeded
float32 flow [H,W,2] with what flow_to_image returned for it plain, with clip_flow=10 and with convert_to_bgr=True, and
what flow_uv_to_colors returned for the un-normalised pair (u, v) = flow * uv_scale (0.125: exact in float32, so the pair is
not stored), at least a fifth of whose pixels have a radius above 1.
No reference source is copied; the fixture is data.
"""
import argparse
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = ((1, 1), (3, 5), (37, 61), (40, 64))
SEED = 5512
UV_SCALE = np.float32(0.125)


def flows(h, w, rng):
    """Flow of a few pixels with a tenth of it several times larger, and some exactly axis-aligned and zero vectors."""
    flow = (rng.standard_normal((h, w, 2)) * 6.0).astype(np.float32)
    flow *= np.where(rng.random((h, w, 1)) < 0.1, 5.0, 1.0).astype(np.float32)
    if h * w >= 15:
        flat = flow.reshape(-1, 2)
        flat[1] = (0.0, 0.0)
        flat[2] = (3.0, 0.0)
        flat[3] = (-3.0, 0.0)
        flat[4] = (0.0, 2.0)
        flat[5] = (0.0, -2.0)
        flat[6] = (3.0, -0.0)
        flat[7] = (-3.0, -0.0)
    if h * w == 1:
        flow[0, 0] = (12.0, -5.5)
    return flow, flow * UV_SCALE          # sigma 0.75 (a tenth 3.75): P(|uv| > 1) is above 0.4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("ref_flow_viz", os.path.join(args.reference, "pytorch", "core", "utils", "flow_viz.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    rng = np.random.default_rng(SEED)
    out = {"colorwheel": ref.make_colorwheel(), "uv_scale": UV_SCALE}
    for h, w in SHAPES:
        flow, uv = flows(h, w, rng)
        k = f"{h}x{w}"
        out[k + ".flow"] = flow
        out[k + ".image"] = ref.flow_to_image(flow)
        out[k + ".image_clip10"] = ref.flow_to_image(flow, clip_flow=10)
        out[k + ".image_bgr"] = ref.flow_to_image(flow, convert_to_bgr=True)
        out[k + ".colors"] = ref.flow_uv_to_colors(uv[:, :, 0], uv[:, :, 1])
        frac = float(np.mean(np.sqrt(uv[:, :, 0] ** 2 + uv[:, :, 1] ** 2) > 1))
        assert frac >= 0.2, (k, frac)
        print(k, "rad > 1 on", frac)
    path = os.path.join(HERE, "flow_viz.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
