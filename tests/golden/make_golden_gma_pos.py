#!/usr/bin/env python3
"""Generate the relative-position GMA fixtures (tests/golden/*gma_pos*.npz) by running the REFERENCE itself (container only).

Usage (build container, where /root/reference exists):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gma_pos.py [ops] [train] [e2e]

Same pattern as make_golden.py: the reference's core.gma / core.gma_network are imported, fed oracle.weights procedural weights
and inputs, and their OUTPUTS are stored; no reference source is copied.  The reference runs with --position_only ("only")
and --position_and_content ("both").

The ops fixtures hold the reference run in float64 (`attn`, gradients) together with the fp32 floor of every comparison: the
largest difference between the same reference run in float32 and in float64 (`floor.*`), which no fp32 implementation can be
asked to beat.  The nn.Embedding tables are emb_scale * N(0, 1) (`scale_embeddings`), emb_scale chosen by
`pick_scale` so that the softmax is not one-hot (smallest row maximum below 0.5) and stored with the map's row maxima.
"""
import argparse
import json
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference/pytorch")
warnings.filterwarnings("ignore")

from core.gma import Attention                       # noqa: E402  (reference)
from core.gma_network import RAFTGMA                 # noqa: E402

from oracle.weights import procedural_state_dict, rand_tensor, synthetic_pair  # noqa: E402

torch.manual_seed(0)
torch.set_num_threads(8)

FLAGS = {"only": dict(position_only=True, position_and_content=False),
         "both": dict(position_only=False, position_and_content=True)}
OPS_CASES = [("gma_pos_ops", 2, 12, 16, 840), ("gma_pos_ops_9x15", 2, 9, 15, 850)]


def gma_ns(flag):
    return argparse.Namespace(small=False, mixed_precision=False, dropout=0, num_heads=1, corr_levels=4, corr_radius=4,
                              **FLAGS[flag])


def save(name, **arrs):
    out = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in arrs.items()}
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}.npz  {os.path.getsize(path) / 1024:.1f} KiB")


def scale_embeddings(sd, scale, seed=0):
    """The state dict with the two RelPosEmb tables replaced by scale * N(0, 1) (rand_tensor, seeds seed + 5 / seed + 6).
    procedural_state_dict fills every 2-D `weight` with ones, and a constant table adds the same number to every logit of a
    row: the softmax would not see it."""
    out = dict(sd)
    for i, k in enumerate(sorted(k for k in sd if ".pos_emb.rel_" in "." + k and k.endswith(".weight"))):
        out[k] = rand_tensor(tuple(sd[k].shape), seed + 5 + i, scale)
    return out


def _sample(g):
    g = g.reshape(-1)
    return g if g.numel() <= 4096 else g[:: g.numel() // 4096][:4096].clone()


def run_attention(flag, sd, B, H, W, seed, dtype):
    """The reference's Attention forward + backward of sum(attn * R); returns the dict of comparisons."""
    att = Attention(args=gma_ns(flag), dim=128, heads=1, max_pos_size=160, dim_head=128)
    att.load_state_dict(sd, strict=False)
    att = att.to(dtype)
    ctx = torch.relu(rand_tensor((B, 128, H, W), seed + 1, 1.5)).to(dtype).requires_grad_(True)
    A = att(ctx)
    (A * rand_tensor(tuple(A.shape), seed + 3).to(dtype)).sum().backward()
    P = 160
    outside = att.pos_emb.rel_height.weight.grad.clone()
    outside[P - H:P + H - 1] = 0
    return dict(attn=A.detach(), dctx=ctx.grad, dto_qk_full=att.to_qk.weight.grad,
                drel_height=att.pos_emb.rel_height.weight.grad[P - H:P + H - 1].clone(),
                drel_width=att.pos_emb.rel_width.weight.grad[P - W:P + W - 1].clone(),
                drel_height_outside=outside.abs().max())


def pick_scale(flag, sd, B, H, W, seed):
    """Largest of 1 (nn.Embedding's own N(0, 1)), 0.5, 0.25, ... for which the smallest row maximum of the map is below 0.5."""
    scale = 1.0
    while True:
        A = run_attention(flag, scale_embeddings(sd, scale, seed), B, H, W, seed, torch.float64)["attn"]
        if A.max(-1).values.min().item() < 0.5 or scale < 1e-3:
            return scale
        scale /= 2


def gen_ops():
    shapes = None
    for name, B, H, W, seed in OPS_CASES:
        for flag in FLAGS:
            att = Attention(args=gma_ns(flag), dim=128, heads=1, max_pos_size=160, dim_head=128)
            shapes = {k: tuple(v.shape) for k, v in att.state_dict().items()}
            sd0 = procedural_state_dict(shapes, seed)
            scale = pick_scale(flag, sd0, B, H, W, seed)
            sd = scale_embeddings(sd0, scale, seed)
            r64 = run_attention(flag, sd, B, H, W, seed, torch.float64)
            r32 = run_attention(flag, sd, B, H, W, seed, torch.float32)
            assert r64["drel_height_outside"].item() == 0.0
            rowmax = r64["attn"].max(-1).values
            d = dict(B=B, H=H, W=W, seed=seed, emb_scale=scale, attn=r64["attn"], dctx=r64["dctx"].float(),
                     drel_height=r64["drel_height"].float(), drel_width=r64["drel_width"].float(),
                     attn_max=r64["attn"].max(), min_row_max=rowmax.min(), mean_row_max=rowmax.mean())
            d["dparam.att.to_qk.weight"] = _sample(r64["dto_qk_full"]).float()
            d["dto_qk_k_half_absmax"] = r64["dto_qk_full"][128:].abs().max()
            for k in ("attn", "dctx", "drel_height", "drel_width"):
                d["floor." + k] = (r32[k].double() - r64[k]).abs().max()
            d["floor.dto_qk"] = (_sample(r32["dto_qk_full"]).double() - _sample(r64["dto_qk_full"])).abs().max()
            print(name, flag, "scale", scale, "attn max", float(d["attn_max"]), "min row max", float(d["min_row_max"]),
                  {k: float(v) for k, v in d.items() if k.startswith("floor.")})
            save(f"{name}_{flag}", **d)
    with open(os.path.join(HERE, "gma_pos_ops_shapes.json"), "w") as f:
        json.dump({k: list(v) for k, v in shapes.items() if not k.endswith("rel_ind")}, f, indent=0)


def _model(flag, seed, scale):
    model = RAFTGMA(gma_ns(flag))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(scale_embeddings(procedural_state_dict(shapes, seed), scale, seed), strict=False)
    with torch.no_grad():
        model.update_block.aggregator.gamma.fill_(0.1)     # zero gamma would leave the aggregate path (and dattn) unexercised
    stats = {}

    def hook(_m, _i, out):
        rowmax = out.detach().max(-1).values
        stats.update(attn_max=out.detach().max(), min_row_max=rowmax.min(), mean_row_max=rowmax.mean())
    model.att.register_forward_hook(hook)
    return model, stats


def _train_digest(model, preds, stride=4):
    """loss of the benchmark objective (sum_i 0.8^(n-1-i) mean sqrt(p^2 + 1e-6), zero gt) + backward digests, the format of
    make_golden.py::_train_digest, every parameter included (the pos_emb tables too)."""
    n = len(preds)
    loss = 0.0
    for i, p in enumerate(preds):
        loss = loss + (0.8 ** (n - i - 1)) * torch.sqrt(p * p + 1e-6).mean()
    loss.backward()
    d = dict(loss=loss.detach(), last=preds[-1].detach()[:, :, ::stride, ::stride].contiguous(),
             first=preds[0].detach()[:, :, ::stride, ::stride].contiguous(), stride=stride)
    for k, p in model.named_parameters():
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        d["gnorm." + k] = g.norm()
        d["ghead." + k] = g.reshape(-1)[:32].clone()
    return d


def pick_net_scale(flag, seed, H, W):
    """pick_scale for the whole network: one test-mode iteration per candidate, the map's row maxima read by the hook."""
    scale = 1.0
    while True:
        model, stats = _model(flag, seed, scale)
        model.eval()
        with torch.no_grad():
            model(*synthetic_pair(1, H, W, seed + 1), iters=1, test_mode=True)
        if stats["min_row_max"].item() < 0.5 or scale < 1e-3:
            return scale
        scale /= 2


def gen_train():
    for flag in FLAGS:
        seed, H, W, iters = 860, 128, 192, 4
        scale = pick_net_scale(flag, seed, H, W)
        model, stats = _model(flag, seed, scale)
        model.train()
        model.freeze_bn()
        im1, im2 = synthetic_pair(1, H, W, seed + 1)
        preds = model(im1, im2, iters=iters)
        d = _train_digest(model, preds)
        print("train", flag, {k: float(v) for k, v in stats.items()})
        save(f"train_step_gma_pos_small_{flag}", H=H, W=W, iters=iters, seed=seed, B=1, gamma=0.1, emb_scale=scale, **stats, **d)


def gen_e2e():
    flag, seed, H, W = "both", 870, 440, 1024
    scale = pick_net_scale(flag, seed, H, W)
    model, stats = _model(flag, seed, scale)
    model.eval()
    im1, im2 = synthetic_pair(1, H, W, seed + 1)
    with torch.no_grad():
        low, up = model(im1, im2, iters=12, test_mode=True)
    print("e2e", flag, {k: float(v) for k, v in stats.items()})
    save(f"e2e_gma_pos_440x1024_{flag}", B=1, H=H, W=W, iters=12, seed=seed, stride=4, gamma=0.1, emb_scale=scale,
         flow_low=low, flow_up_strided=up[:, :, ::4, ::4].contiguous(), flow_up_absmean=up.abs().mean(), **stats)


if __name__ == "__main__":
    which = set(sys.argv[1:]) or {"ops", "train", "e2e"}
    if "ops" in which:
        gen_ops()
    if "train" in which:
        gen_train()
    if "e2e" in which:
        gen_e2e()
