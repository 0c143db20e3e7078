"""Host side of the training-mode BatchNorm route: which norms _train_bn_ok names, the two C entries in the header, the ctypes
table and the built library, and that on the CPU the switch TRAIN_BN changes nothing."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

import flow_supervisor_amd.core.extractor as X
from flow_supervisor_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fsraft_bnorm_cl_fwd", "fsraft_bnorm_cl_bwd")


def test_train_bn_ok_truth_table():
    ok = X._train_bn_ok
    assert ok(nn.BatchNorm2d(8).train()) and ok(nn.BatchNorm2d(8, momentum=0.01).train())
    assert not ok(nn.BatchNorm2d(8).eval())
    assert not ok(nn.BatchNorm2d(8, affine=False).train())
    assert not ok(nn.BatchNorm2d(8, track_running_stats=False).train())
    assert not ok(nn.BatchNorm2d(8, momentum=None).train())               # cumulative average: needs num_batches_tracked on the host
    assert not ok(nn.BatchNorm1d(8).train()) and not ok(nn.BatchNorm3d(8).train())
    assert not ok(nn.InstanceNorm2d(8).train()) and not ok(nn.InstanceNorm2d(8, affine=True, track_running_stats=True).train())
    assert not ok(nn.GroupNorm(2, 8).train()) and not ok(nn.Sequential())
    # the contract of _norm_kind is untouched: a training-mode BatchNorm has no kind, a frozen one is not a training one
    assert X._norm_kind(nn.BatchNorm2d(8).train()) is None and X._norm_kind(nn.BatchNorm2d(8).eval()) == "frozen_bn"
    bn = nn.BatchNorm2d(8).train()
    assert X._covered(bn) and X._covered(nn.BatchNorm2d(8).eval()) and not X._covered(nn.GroupNorm(2, 8))


def test_switch_off_uncovers_only_the_training_mode_batchnorm(monkeypatch):
    monkeypatch.setattr(X, "TRAIN_BN", False)
    assert not X._covered(nn.BatchNorm2d(8).train())
    assert X._covered(nn.BatchNorm2d(8).eval()) and X._covered(nn.InstanceNorm2d(8))


@pytest.mark.parametrize("name", ENTRIES)
def test_header_signatures_and_library_carry_the_entry(name):
    header = open(os.path.join(ROOT, "include", "fsraft.h")).read()
    m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
    assert m, f"{name} is not declared in include/fsraft.h"
    nargs = len([a for a in m.group(1).split(",") if a.strip()])
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == nargs
    assert "extractor.py:13-57, 118-170" in header[header.rfind("/*", 0, m.start()):m.start()]
    src = open(os.path.join(ROOT, "flow_supervisor_amd", "csrc", "Makefile")).read()
    assert "norm_bn.hip" in src
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built")
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)


@pytest.mark.parametrize("kind", ("basic", "small"))
def test_cpu_encoder_is_bitwise_the_same_with_the_switch_on_and_off(kind, monkeypatch):
    torch.manual_seed(1)
    enc = (X.BasicEncoder if kind == "basic" else X.SmallEncoder)(output_dim=32, norm_fn="batch").train()
    state = {k: v.clone() for k, v in enc.state_dict().items()}
    x = torch.randn(2, 3, 32, 48)
    res = {}
    for on in (True, False):
        monkeypatch.setattr(X, "TRAIN_BN", on)
        enc.load_state_dict(state)
        enc.zero_grad(set_to_none=True)
        y = enc(x)
        y.square().sum().backward()
        res[on] = [y.detach().clone()] + [p.grad.clone() for p in enc.parameters()] + [b.clone() for b in enc.buffers()]
    assert len(res[True]) == len(res[False]) and all(torch.equal(a, b) for a, b in zip(res[True], res[False]))
    assert int(enc.norm1.num_batches_tracked) == 1
