"""Shared by the relative-position GMA tests: the inputs of tests/golden/make_golden_gma_pos.py regenerated, and the table
formulation of the positional logits restated in torch (independent of any kernel and of the package's own composition)."""
import argparse

import torch

from _util import shapes
from oracle.weights import procedural_state_dict, rand_tensor

FLAGS = {"only": dict(position_only=True, position_and_content=False),
         "both": dict(position_only=False, position_and_content=True)}
OPS_FIXTURES = [f"{name}_{flag}" for name in ("gma_pos_ops", "gma_pos_ops_9x15") for flag in FLAGS]
P = 160          # max_pos_size of RAFTGMA's Attention


def pos_ns(flag):
    return argparse.Namespace(small=False, mixed_precision=False, dropout=0, num_heads=1, corr_levels=4, corr_radius=4,
                              **FLAGS[flag])


def with_embeddings(sd, scale, seed):
    """make_golden_gma_pos.py::scale_embeddings: the two RelPosEmb tables are scale * N(0, 1), seeds seed + 5 / seed + 6."""
    out = dict(sd)
    for i, k in enumerate(sorted(k for k in sd if ".pos_emb.rel_" in "." + k and k.endswith(".weight"))):
        out[k] = rand_tensor(tuple(sd[k].shape), seed + 5 + i, scale)
    return out


def attention_state(g):
    """State dict of the Attention module of an ops fixture."""
    return with_embeddings(procedural_state_dict(shapes("gma_pos_ops"), int(g["seed"])), float(g["emb_scale"]), int(g["seed"]))


def context_input(g):
    B, H, W, seed = int(g["B"]), int(g["H"]), int(g["W"]), int(g["seed"])
    return torch.relu(rand_tensor((B, 128, H, W), seed + 1, 1.5))


def table_attention(sd, ctx, flag, dtype=torch.float64):
    """softmax of  [content +] G[i, u - x + h - 1] + G[i, (2h - 1) + v - y + w - 1],  G = s q T^T,
    T = [rel_height.weight[P-h : P+h-1] ; rel_width.weight[P-w : P+w-1]],  for ctx [B, C, h, w]  ->  [B, 1, N, N]."""
    B, C, h, w = ctx.shape
    Wqk = sd["to_qk.weight"].to(dtype)[:, :, 0, 0]
    D = Wqk.shape[0] // 2
    s = D ** -0.5
    x = ctx.to(dtype).permute(0, 2, 3, 1).reshape(B, h * w, C)
    q, k = x @ Wqk[:D].T, x @ Wqk[D:].T
    T = torch.cat([sd["pos_emb.rel_height.weight"].to(dtype)[P - h:P + h - 1], sd["pos_emb.rel_width.weight"].to(dtype)[P - w:P + w - 1]])
    G = s * q @ T.T                                                         # [B, N, 2h + 2w - 2]
    i = torch.arange(h * w)
    xi, yi = i // w, i % w                                                  # query (x, y), key (u, v)
    col_h = xi[None, :] - xi[:, None] + h - 1                               # [i, j] -> u - x + h - 1
    col_w = (2 * h - 1) + yi[None, :] - yi[:, None] + w - 1
    S = torch.gather(G, 2, col_h.expand(B, -1, -1)) + torch.gather(G, 2, col_w.expand(B, -1, -1))
    if FLAGS[flag]["position_and_content"]:
        S = s * q @ k.transpose(1, 2) + S
    return S.softmax(-1)[:, None]
