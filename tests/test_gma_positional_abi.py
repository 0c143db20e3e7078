"""CPU-only checks of the relative-position attention (--position_only / --position_and_content): the two C-ABI entries are
declared, exported and validate their arguments on the host, and the table formulation the kernels implement (restated in torch
fp64 in _gma_pos.table_attention) is the reference's: it reproduces the `attn` of every ops fixture, which
tests/golden/make_golden_gma_pos.py stored from the reference's own Attention run in float64."""
import ctypes
import os
import re

import pytest
import torch

from _gma_pos import FLAGS, OPS_FIXTURES, attention_state, context_input, table_attention
from _util import T, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fsraft_softmax_rows_pos", "fsraft_softmax_rows_pos_bwd")
FS_ERR_ARG = 1


def test_header_declares_and_library_exports_the_positional_softmax_pair():
    from flow_supervisor_amd import _lib
    txt = open(os.path.join(ROOT, "include", "fsraft.h")).read()
    declared = set(re.findall(r"^int (fsraft_\w+)\(", txt, flags=re.M))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name


def test_positional_softmax_pair_rejects_bad_arguments_on_the_host():
    """Every case is refused before a launch (FS_ERR_ARG), so this runs without a GPU and never hands a kernel a bad pointer."""
    from flow_supervisor_amd import _lib
    lib = _lib.load()
    null, p16, p8 = ctypes.c_void_p(None), ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 8)
    h, w = 4, 8
    n, ldg = h * w, 2 * h + 2 * w - 2
    fwd, bwd = lib.fsraft_softmax_rows_pos, lib.fsraft_softmax_rows_pos_bwd
    # null pointers
    assert fwd(null, null, ldg, n, n, h, w, 1, 0, None) == FS_ERR_ARG
    assert fwd(p16, null, ldg, n, n, h, w, 1, 0, None) == FS_ERR_ARG
    assert fwd(null, p16, ldg, n, n, h, w, 0, 1, None) == FS_ERR_ARG
    assert bwd(null, null, null, ldg, n, n, h, w, 0, None) == FS_ERR_ARG
    assert bwd(p16, p16, null, ldg, n, n, h, w, 0, None) == FS_ERR_ARG
    assert bwd(p16, null, p16, ldg, n, n, h, w, 1, None) == FS_ERR_ARG
    # h * w != n, rows not a multiple of n, a score matrix narrower than 2h + 2w - 2
    assert fwd(p16, p16, ldg, n, n + 1, h, w, 1, 0, None) == FS_ERR_ARG
    assert bwd(p16, p16, p16, ldg, n, n + 1, h, w, 0, None) == FS_ERR_ARG
    assert fwd(p16, p16, ldg, n + 1, n, h, w, 1, 0, None) == FS_ERR_ARG
    assert bwd(p16, p16, p16, ldg, n + 1, n, h, w, 0, None) == FS_ERR_ARG
    assert fwd(p16, p16, ldg - 1, n, n, h, w, 1, 0, None) == FS_ERR_ARG
    assert bwd(p16, p16, p16, ldg - 1, n, n, h, w, 0, None) == FS_ERR_ARG
    # records: misaligned buffers, n % 32 != 0
    assert fwd(p8, p16, ldg, n, n, h, w, 1, 1, None) == FS_ERR_ARG
    assert bwd(p8, p16, p16, ldg, n, n, h, w, 1, None) == FS_ERR_ARG
    assert bwd(p16, p8, p16, ldg, n, n, h, w, 1, None) == FS_ERR_ARG
    assert fwd(p16, p16, 2 * 3 + 2 * 5 - 2, 15, 15, 3, 5, 1, 1, None) == FS_ERR_ARG
    assert bwd(p16, p16, p16, 2 * 3 + 2 * 5 - 2, 15, 15, 3, 5, 1, None) == FS_ERR_ARG
    # rows over the LDS limit: forward 4 ceil4(n) + 4 (h + w) <= 65520, backward 8 ceil4(n) + 4 (h + w) <= 65520
    assert fwd(p16, p16, 512, 128 * 128, 128 * 128, 128, 128, 1, 0, None) == FS_ERR_ARG
    assert bwd(p16, p16, p16, 2 * 64 + 2 * 128 - 2, 64 * 128, 64 * 128, 64, 128, 0, None) == FS_ERR_ARG
    assert bwd(p16, p16, p16, 2 * 60 + 2 * 136 - 2, 60 * 136, 60 * 136, 60, 136, 1, None) == FS_ERR_ARG      # 65280 + 784


def test_lds_budget_and_table_helper_host_logic():
    from flow_supervisor_amd import ops
    assert ops.softmax_rows_pos_fits(55, 128)                  # 7040 * 8 + 183 * 4 = 57 052 bytes (+ 16 static)
    assert not ops.softmax_rows_pos_fits(64, 128) and not ops.softmax_rows_pos_fits(60, 136)
    rh = torch.arange(319 * 4, dtype=torch.float32).view(319, 4)
    rw = -rh
    Tb, rows, sh, sw = ops.rel_pos_table(rh, rw, 9, 15)
    assert rows == 48 and tuple(Tb.shape) == (48, 4) and (sh, sw) == (slice(151, 168), slice(145, 174))
    assert torch.equal(Tb[:17], rh[151:168]) and torch.equal(Tb[17:46], rw[145:174]) and not Tb[46:].any()
    with pytest.raises(ValueError, match="max_pos_size is 160"):
        ops.rel_pos_table(rh, rw, 161, 4)


@pytest.mark.parametrize("name", OPS_FIXTURES)
def test_table_formulation_is_the_reference_attention(name):
    g = load(name)
    flag = name.rsplit("_", 1)[1]
    assert flag in FLAGS and g["attn"].dtype.name == "float64"
    assert float(g["min_row_max"]) < 0.5 and float(g["attn_max"]) > 4.0 / (int(g["H"]) * int(g["W"]))     # neither one-hot nor flat
    A = table_attention(attention_state(g), context_input(g), flag)
    err = (A - T(g["attn"])).abs().max().item()
    assert err <= 1e-14, err          # probabilities <= 1 in float64: a few ulps of reordered sums
