#!/usr/bin/env python3
"""Generate tests/golden/lookup_dcoords.npz by running the REFERENCE itself (container only).

Usage (build container, where /root/reference exists):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dcoords.py

Same pattern as make_golden_gma_pos.py: the reference's core.corr.CorrBlock is imported and run on the CPU -- CorrBlock(fmap1,
fmap2, num_levels=4, radius=r)(coords) with coords.requires_grad_(), then out.backward(dout) -- and its INPUTS, dout and
coords.grad are stored; no reference source is copied.  B = 1, C = 8, 16x24 (levels down to 2x3: grid_sample's
normalisation never divides by zero), radius 3 and 4 on the same feature maps and coordinates.  Coordinates
(tests/_dcoordsref.mixed_positions): a third multiples of 1/64 in [-6, W+6] x [-6, H+6], a third exact integers, a third
within one cell of an edge.  dout is stored as int8 multiples of 1/4 (dout = dout_q / 4) to keep the file small.
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, "/root/reference/pytorch")
warnings.filterwarnings("ignore")

from core.corr import CorrBlock                       # noqa: E402  (reference)

import _dcoordsref as R                               # noqa: E402

B, C, H, W = 1, 8, 16, 24


def main():
    gen = torch.Generator().manual_seed(910)
    fmap1 = torch.randn(B, C, H, W, generator=gen)
    fmap2 = torch.randn(B, C, H, W, generator=gen)
    x, y = R.mixed_positions(B * H * W, H, W, gen)
    coords = torch.stack([x.view(B, H, W), y.view(B, H, W)], 1).contiguous()
    out = dict(fmap1=fmap1.numpy(), fmap2=fmap2.numpy(), coords=coords.numpy(), dout_scale=np.float32(0.25))
    for r in (3, 4):
        ch = 4 * (2 * r + 1) ** 2
        dq = torch.randint(-8, 9, (B, ch, H, W), generator=gen, dtype=torch.int8)
        c = coords.clone().requires_grad_()
        o = CorrBlock(fmap1, fmap2, num_levels=4, radius=r)(c)
        o.backward(dq.float() * 0.25)
        out[f"dout_q_r{r}"] = dq.numpy()
        out[f"coords_grad_r{r}"] = c.grad.numpy()
        out[f"out_absmax_r{r}"] = o.detach().abs().max().numpy()
    path = os.path.join(HERE, "lookup_dcoords.npz")
    np.savez_compressed(path, **out)
    print(f"lookup_dcoords.npz  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
