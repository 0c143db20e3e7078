"""The wide tiles of the per-tap weight-gradient kernel (fsraft_set_wgrad_wide; 256x256 and 128x256, csrc/conv_wgrad.hip) against
the fp64 reference of tests/_convref.py, under the two criteria and the constants test_conv_routes.py applies to routes 5 and 8: the
arithmetic is the same bf16x3 with fp32 sums, only the order of the sums changes.  Each case asserts the tile that ran
(fsraft_conv_wgrad_last_tile: a silent fallback to the 128x128 tile is a failure) and the unchanged route code, and that dwpk and
dbias are untouched outside the layer: NaN-pattern guard rows on both sides, and a marker value in the channel padding of the
packed-K layout (the kernel adds exact zeros there).

Shapes are the smallest at which the tile can go wrong: B = 2, H in {5, 9}, W in {33, 40} (M no multiple of 32, tap shifts across
every border, 256-pixel splits that end inside a row and inside an image), one case with M below one split; x tiles made of two
sources, of two taps of one source, of a partial and a full column group, of a channel slice; Cout = 256, 260 (a remainder on the
128x128 tile), 128 (the 128x256 tile) and a slice of a wider dY; 1, 2 and 12 segments; bias gradient on and off."""
import pytest
import torch

import _convref as R
from _util import GUARD, PATTERN, _log_margin

pytestmark = pytest.mark.gpu
DEV = "cuda"
W256, W128, T128 = 256 << 16 | 256, 128 << 16 | 256, 128 << 16 | 128
MARK = 1234.5            # what the channel-padding columns of dwpk hold before and after


def _ops():
    from flow_supervisor_amd import ops
    return ops


def _lib():
    from flow_supervisor_amd import _lib
    return _lib.load()


class wide:
    """fsraft_set_wgrad_wide(mode) for the duration of a case; the default (1: by shape) is put back in `finally`."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        assert _lib().fsraft_set_wgrad_wide(self.mode) == 0

    def __exit__(self, *exc):
        _lib().fsraft_set_wgrad_wide(1)


def _src(B, H, W, ld, kind, g):
    x = torch.randn(B, H, W, ld, device=DEV, generator=g)
    return torch.tanh(x) if kind == 0 else torch.relu(x) if kind == 1 else x


def _guarded(rows, cols, fill):
    """[rows, cols] view (filled) between two guard blocks of the NaN pattern; returns (view, whole buffer, copy of the buffer)."""
    g = (GUARD + cols - 1) // cols
    full = torch.full(((rows + 2 * g) * cols,), 0, dtype=torch.int32, device=DEV)
    full[:] = PATTERN
    full = full.view(torch.float32).view(rows + 2 * g, cols)
    view = full[g:g + rows]
    view[:] = fill
    return view, full, g


def run(case, mode):
    """case: dict(B, H, W, KH, KW, Cout, ldy, srcs=[(C, ld, off)], nseg, multi, bias).  Returns what _check needs."""
    ops = _ops()
    B, H, W, KH, KW, Cout = (case[k] for k in ("B", "H", "W", "KH", "KW", "Cout"))
    M = B * H * W
    g = torch.Generator(device=DEV).manual_seed(hash((B, H, W, KH, KW, Cout, 11)) % (1 << 31))
    srcC = [c for c, _, _ in case["srcs"]]
    dys, dyv, xss, srcss = [], [], [], []
    for _ in range(case["nseg"]):
        t = torch.randn(B, H, W, case["ldy"], device=DEV, generator=g) * 0.1
        dys.append(t[..., :Cout])
        dyv.append(ops.V(t, Cout))
        xs, vs = [], []
        for i, (C, ld, off) in enumerate(case["srcs"]):
            x = _src(B, H, W, ld, min(i, 2) if len(case["srcs"]) > 1 else 1, g)
            xs.append(x[..., off:off + C])
            vs.append(ops.V(x, C, off))
        xss.append(xs)
        srcss.append(vs)
    idx, ktot = R.packed_k_index(srcC, KH, KW)
    assert ktot == ops.conv_ktot(srcC, KH, KW)
    dwpk, dw_full, gw = _guarded(Cout, ktot, MARK)
    dwpk[:, idx.reshape(-1).to(DEV)] = 0.0
    # (a source is read in 16-byte chunks, so up to three columns past C take products of its row padding: they are not checked)
    idx4, _ = R.packed_k_index([(c + 3) // 4 * 4 for c in srcC], KH, KW)
    pad_cols = torch.ones(ktot, dtype=torch.bool, device=DEV)
    pad_cols[idx4.reshape(-1).to(DEV)] = False
    dbias = db_full = None
    if case["bias"]:
        dbias, db_full, gb = _guarded(Cout, 1, 0.0)
        dbias = dbias.view(Cout)
    with wide(mode):
        if case["multi"]:
            ops.conv_wgrad_multi(dyv, srcss, dwpk, B, H, W, KH, KW, dbias=dbias)
        else:
            ops.conv_wgrad(dyv[0], srcss[0], dwpk, B, H, W, KH, KW, dbias=dbias)
        route, tile = _lib().fsraft_conv_last_route(1), _lib().fsraft_conv_wgrad_last_tile()
    torch.cuda.synchronize()
    # nothing outside the layer moved
    pat = torch.tensor(PATTERN, dtype=torch.int32, device=DEV)
    assert bool((dw_full[:gw].view(torch.int32) == pat).all()) and bool((dw_full[gw + Cout:].view(torch.int32) == pat).all()), "dwpk guard rows"
    assert bool((dwpk[:, pad_cols] == MARK).all()), "channel padding of dwpk"
    if dbias is not None:
        assert bool((db_full[:gb].view(torch.int32) == pat).all()) and bool((db_full[gb + Cout:].view(torch.int32) == pat).all()), "dbias guards"
    Cin = sum(srcC)
    dw = ops.unpack_weight_grad(dwpk.contiguous(), (Cout, Cin, KH, KW), srcC)
    torch.cuda.synchronize()
    G = R.wgrad_gemm(dys, xss, B, H, W, KH, KW).reshape(Cout, -1)
    S = R.wgrad_gemm(dys, xss, B, H, W, KH, KW, "abs").reshape(Cout, -1)
    twins = {m: R.wgrad_gemm(dys, xss, B, H, W, KH, KW, m).reshape(Cout, -1) for m in ("fp32", "bf16x3", "bf16x1")}
    # mutant (a) of test_conv_routes.run_wgrad: the last 64-pixel tile of the last segment loses one 32-channel chunk of the centre tap
    lo = (M - 1) // 64 * 64
    rows = torch.arange(lo, M, device=DEV)
    a = R.columns([x.reshape(B, H, W, -1).double() for x in xss[-1]], B, H, W, KH, KW, (KH // 2, KW // 2), rows)
    cut = torch.zeros(KH * KW, Cin, dtype=torch.float64, device=DEV)
    cut[KH * KW // 2, :min(32, Cin)] = 1
    dmut = (dys[-1].reshape(M, Cout)[lo:].double().t() @ (a * cut.reshape(1, -1))).reshape(Cout, KH, KW, Cin)
    mut = G - dmut.permute(0, 3, 1, 2).reshape(Cout, -1)
    ok_bias = True
    if dbias is not None:
        bref = sum(d.reshape(M, Cout).double().sum(0) for d in dys)
        babs = sum(d.reshape(M, Cout).double().abs().sum(0) for d in dys)
        ok_bias = bool(((dbias.double() - bref).abs() <= R.gamma("fp32", M * len(dys)) * babs + 1e-30).all())
    return route, tile, {"dst0": dw.reshape(Cout, -1)}, G, S, M * len(dys), twins, mut, ok_bias


def _check(name, case, mode, tile_expected):
    route, tile, got, G, S, K, twins, mut, ok_bias = run(case, mode)
    route_expected = 8 if case["multi"] and case["nseg"] > 1 else 5
    assert route == route_expected, f"{name}: route {route}, expected {route_expected}"
    assert tile == tile_expected, f"{name}: tile {tile >> 16}x{tile & 0xffff}, expected {tile_expected >> 16}x{tile_expected & 0xffff}"
    ok, rejected, rep = R.verdict(got, R.Epi(0), G, S, K, "bf16x3", twins, mut, log=_log_margin,
                                  what=f"{name} [{tile >> 16}x{tile & 0xffff} wide={mode}]")
    assert rejected, f"{name}: the comparator did not reject both mutants ({rep})"
    assert ok, f"{name}: {rep}"
    assert ok_bias, f"{name}: fused bias gradient"


def C(name, tile, B, H, W, KH, KW, srcs, Cout, nseg=1, multi=False, bias=True, ldy=None):
    c = dict(B=B, H=H, W=W, KH=KH, KW=KW, Cout=Cout, ldy=ldy or (Cout + 3) // 4 * 4, nseg=nseg, multi=multi, bias=bias, tile=tile)
    c["srcs"] = [tuple(s) if isinstance(s, (list, tuple)) else (s, (s + 3) // 4 * 4, 0) for s in srcs]
    return pytest.param(c, id=name)


CASES = [
    # 256x256: a pair of sources per x tile (1x5, ten column groups), two segments
    C("w256_two_sources_1x5_x2", W256, 2, 5, 33, 1, 5, [128, 128], 256, nseg=2, multi=True),
    # a pair of taps per x tile, an odd fifth group and Cout = 260 (four rows beyond the wide tile): three launches, twelve segments
    C("w256_tap_pairs_5x1_cout260_x12", W256, 2, 9, 40, 5, 1, [128], 260, nseg=12, multi=True),
    # one source of 256 channels given as a channel slice; dY a slice of a wider buffer; single segment (route 5), no bias
    C("w256_slices_1x1", W256, 2, 9, 33, 1, 1, [(256, 288, 32)], 256, ldy=320, bias=False),
    # 324 channels = 352 padded: one pair and a 96-column remainder group
    C("w256_c324_1x1", W256, 2, 5, 40, 1, 1, [324], 256),
    # three sources; the first pair is a partial (98 of 128) and a full group
    C("w256_three_sources_x2", W256, 2, 5, 40, 1, 1, [98, 128, (256, 260, 4)], 256, nseg=2, multi=True, bias=False),
    # 98 channels with five taps: every group partial, odd count
    C("w256_c98_1x5", W256, 2, 9, 33, 1, 5, [98], 256),
    # 128x256 (Cout <= 128): taps of one source (1x5 and 5x1), pairs of sources, twelve segments
    C("w128_tap_pairs_1x5", W128, 2, 9, 40, 1, 5, [128], 128, bias=False),
    C("w128_tap_pairs_5x1_cout100", W128, 2, 5, 33, 5, 1, [128], 100),
    C("w128_two_sources_1x5_x12", W128, 2, 5, 40, 1, 5, [128, 128], 128, nseg=12, multi=True),
    C("w128_2x2_c384", W128, 2, 9, 33, 2, 2, [384], 128),
    # one segment through the multi entry point: it hands over to the single-segment entry (route 5)
    C("w128_multi_entry_one_segment", W128, 2, 5, 33, 5, 1, [128], 128, nseg=1, multi=True),
    # M = 165 pixels: less than one 256-pixel split
    C("w256_m_below_one_split", W256, 1, 5, 33, 1, 5, [128, 128], 256, nseg=2, multi=True),
    # one column group only (98 -> 128, 1x1): nothing to pair, the 128x128 tile runs and says so
    C("single_group_stays_128", T128, 2, 5, 33, 1, 1, [98], 128),
]


@pytest.mark.parametrize("case", CASES)
def test_wide_tile(case, request):
    _check(request.node.callspec.id, case, 2, case["tile"])


@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[8]])
def test_switch_off_runs_the_128_tile(case, request):
    """fsraft_set_wgrad_wide(0): the same calls on the 128x128 tile, same route codes, same criteria."""
    _check(request.node.callspec.id, case, 0, T128)


def test_switch_rejects_unknown_modes_and_is_back_at_its_default():
    lib = _lib()
    assert lib.fsraft_set_wgrad_wide(3) != 0 and lib.fsraft_set_wgrad_wide(-1) != 0
    assert lib.fsraft_set_wgrad_wide(1) == 0
