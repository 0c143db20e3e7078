"""Every kernel route of fsraft_conv_forward / fsraft_conv_wgrad[_multi] against the fp64 reference of tests/_convref.py, at the
step's shapes and at the selection thresholds, in both arithmetic modes.  Each case asserts the route it expects
(fsraft_conv_last_route: a silent fallback to another kernel is a failure), passes both criteria of the comparator
(elementwise against gamma * |X||W|, Frobenius against the arithmetic's twin and the bf16x1 twin) and shows that the same
comparator rejects its two mutants.  The coverage guard runs one eager step of each benchmark configuration with the
convolution entry points wrapped and fails on any call whose shape or route this file does not test.

Key-only routes covered by a forced case: key 0 = 1..5 (exact tiles), key 3 = 3 / 4 / 5, key 9, key 1 = 3, key 4 = 1,
key 15, key 27 = 2, key 28 = 2 / 3, key 32 (forced slices).  Deliberately untested: key 26 = 2 (the 128-pixel patch tiles for
every N > 64 layer: the same kernel as route 10, which the default knobs reach), keys 5 / 8 / 12 / 7 (addressing variants of
routes that are tested: they change how a tile loads, not which tile runs)."""
import argparse
import json
import os

import pytest
import torch

import _convref as R
from _util import TUNING_DEFAULTS, _log_margin

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROWS_CAP = 12288         # sampled output pixels per forward case (plus borders, tile edges, first / last tiles)


def _ops():
    from flow_supervisor_amd import ops
    return ops


def _lib():
    from flow_supervisor_amd import _lib
    return _lib


def last_route(which):
    return _lib().load().fsraft_conv_last_route(which)


@pytest.fixture(params=["exact", "split"])
def precision(request):
    """Both arithmetic modes (fsraft_set_arithmetic), as in test_gpu_parity.py."""
    _ops().set_arithmetic(request.param == "split")
    yield request.param
    _ops().set_arithmetic(True)


class tuning:
    """fsraft_set_tuning(key, value) for the duration of a case; what fsraft_get_tuning read before is put back in `finally`
    (the defaults of csrc/conv_common.hpp; keys 3 / 4: the arithmetic mode the case started in)."""

    def __init__(self, knobs):
        self.knobs = dict(knobs or {})

    def __enter__(self):
        lib = _lib().load()
        self.saved = {k: lib.fsraft_get_tuning(k) for k in self.knobs}
        for k, v in self.knobs.items():
            assert lib.fsraft_set_tuning(k, v) == 0

    def __exit__(self, *exc):
        lib = _lib().load()
        for k, v in self.saved.items():
            lib.fsraft_set_tuning(k, v)


def _log_case(rec):
    path = os.environ.get("FSRAFT_ROUTE_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")


# ------------------------------------------------------------------------------------------------------------ case runners
def _src_tensor(B, H, W, ld, kind, g):
    x = torch.randn(B, H, W, ld, device=DEV, generator=g)
    if kind == 0:
        return torch.tanh(x)                   # hidden state
    if kind == 1:
        return torch.relu(x)                   # context / encoder activations
    return x                                   # correlation features, gradients: O(1) of both signs


def _gather_dst(flat, off, bs, ps, cs, B, H, W, width, rows):
    b = rows // (H * W)
    p = rows % (H * W)
    base = off + b * bs + p * ps
    idx = base[:, None] + torch.arange(width, device=DEV)[None, :] * cs
    return flat[idx]


def run_fwd(case, arith_mode):
    """case: dict(B, H, W, KH, KW, srcs=[(C, ld, off)], N, epi, relu, alpha, bias, dsts=[(bs, ps, cs, off, n0, acc, maskC)],
    pad, split (a split pack is passed), frag, lds (GRU epilogues: h, z, aux1, aux2, pre pitches), knobs)."""
    ops = _ops()
    B, H, W, KH, KW, N = (case[k] for k in ("B", "H", "W", "KH", "KW", "N"))
    M = B * H * W
    g = torch.Generator(device=DEV).manual_seed(hash((B, H, W, KH, KW, N)) % (1 << 31))
    srcs, xs = [], []
    for i, (C, ld, off) in enumerate(case["srcs"]):
        t = _src_tensor(B, H, W, ld, min(i, 2) if len(case["srcs"]) > 1 else 2, g)
        srcs.append(ops.V(t, C, off))
        xs.append(t[..., off:off + C])
    Cin = sum(c for c, _, _ in case["srcs"])
    w = torch.randn(N, Cin, KH, KW, device=DEV, generator=g) * (1.0 / (Cin * KH * KW)) ** 0.5
    bias = torch.randn(N, device=DEV, generator=g) * 0.1 if case.get("bias") else None
    srcC = [c for c, _, _ in case["srcs"]]
    with tuning(case.get("knobs")):              # (packs as the forced mode needs them: pack_pair asks for the mode)
        wpk, wps = ops.pack_pair(w, srcC)
    if not case.get("split", True):
        wpk, wps = ops.pack_weight(w, srcC, 0), None
    frag = ops.fragment_order(wps) if case.get("frag") and wps is not None else None
    epi_kind = case.get("epi", 0)
    kw = {}
    outs = {}
    lds = case.get("lds", {})
    dsts = []
    if epi_kind == 0:
        for j, (bs, ps, cs, off, n0, acc, maskC) in enumerate(case["dsts"]):
            n1 = case["dsts"][j + 1][4] if j + 1 < len(case["dsts"]) else N
            width = n1 - n0
            size = off + (B - 1) * bs + (H * W - 1) * ps + (width - 1) * cs + 1
            flat = torch.randn(size, device=DEV, generator=g) if acc else torch.zeros(size, device=DEV)
            d = ops.Dst(flat, off, bs, ps, cs, n0, bool(acc))
            mask = None
            if maskC:
                mt = torch.randn(B, H, W, (maskC + 3) // 4 * 4, device=DEV, generator=g)
                d.masked(ops.V(mt, maskC))
                mask = mt[..., :maskC]
            dsts.append(d)
            outs[f"dst{j}"] = (flat, off, bs, ps, cs, width, flat.clone() if acc else None, mask)
    else:
        hid = N // 2 if epi_kind == 2 else N
        h = torch.tanh(torch.randn(B, H, W, lds.get("h", hid), device=DEV, generator=g))
        pre = torch.randn(B, H, W, lds.get("pre", N), device=DEV, generator=g) if lds.get("pre") else None
        kw.update(h=h, pre=pre)
        if epi_kind == 2:
            z = torch.zeros(B, H, W, (hid + 3) // 4 * 4, device=DEV)
            r = torch.zeros(B, H, W, lds.get("aux2", hid), device=DEV)
            rh = torch.zeros(B, H, W, lds.get("aux1", hid), device=DEV)
            kw.update(aux1=rh, aux2=r, hid=hid)
            dsts = [ops.Dst.nhwc(z)]
            got_t = {"z": z[..., :hid], "r": r[..., :hid], "rh": rh[..., :hid]}
        else:
            z = torch.rand(B, H, W, lds.get("z", N), device=DEV, generator=g)
            q = torch.zeros(B, H, W, lds.get("aux1", N), device=DEV)
            hn = torch.zeros(B, H, W, (N + 3) // 4 * 4, device=DEV)
            kw.update(z=z, aux1=q)
            dsts = [ops.Dst.nhwc(hn)]
            got_t = {"q": q[..., :N], "hn": hn[..., :N]}
    with tuning(case.get("knobs")):
        ops.conv_forward(srcs, wpk, bias, B, H, W, KH, KW, N, dsts, relu=case.get("relu", False), alpha=case.get("alpha", 1.0),
                         epi=epi_kind, wpk_split=wps, wpk_frag=frag, pad=case.get("pad"), **kw)
        route = last_route(0)
    torch.cuda.synchronize()
    rows = R.sample_rows(B, H, W, ROWS_CAP, device=DEV)
    pad = tuple(case["pad"]) if case.get("pad") is not None else (KH // 2, KW // 2)
    G = R.conv_gemm(xs, w, B, H, W, pad, rows)
    S = R.conv_gemm(xs, w, B, H, W, pad, rows, "abs")
    twins = {m: R.conv_gemm(xs, w, B, H, W, pad, rows, m) for m in ("fp32", "bf16x3", "bf16x1")}
    last = R.last_tile_rows(rows, M)
    mut = G.clone()
    # (the tap that reads the output pixel itself: in the image for every pixel of the last tile, whatever the padding)
    mut[last] -= R.chunk_contribution(xs, w, B, H, W, pad, rows[last], len(xs) - 1, pad[0] * KW + pad[1], 0)
    if epi_kind == 0:
        got, dspec = {}, []
        for name, (flat, off, bs, ps, cs, width, old, mask) in outs.items():
            got[name] = _gather_dst(flat, off, bs, ps, cs, B, H, W, width, rows)
            n0 = case["dsts"][int(name[3:])][4]
            dspec.append((n0, _gather_dst(old, off, bs, ps, cs, B, H, W, width, rows) if old is not None else None,
                          mask.reshape(M, -1)[rows] if mask is not None else None))
        epi = R.Epi(0, bias=bias, alpha=case.get("alpha", 1.0), relu=case.get("relu", False), dsts=tuple(dspec))
    else:
        got = {k: v.reshape(M, -1)[rows] for k, v in got_t.items()}
        pre_r = kw["pre"][..., :N].reshape(M, N)[rows] if kw["pre"] is not None else None
        if epi_kind == 2:
            epi = R.Epi(2, bias=bias, pre=pre_r, h=kw["h"][..., :N // 2].reshape(M, -1)[rows], hid=N // 2)
        else:
            epi = R.Epi(3, bias=bias, pre=pre_r, h=kw["h"][..., :N].reshape(M, -1)[rows], z=kw["z"][..., :N].reshape(M, -1)[rows])
    return route, got, epi, G, S, KH * KW * Cin, twins, mut


def run_wgrad(case):
    """case: dict(B, H, W, KH, KW, Cout, ldy, srcs=[(C, ld, off)], nseg, multi, bias, knobs)."""
    ops = _ops()
    B, H, W, KH, KW, Cout = (case[k] for k in ("B", "H", "W", "KH", "KW", "Cout"))
    M = B * H * W
    g = torch.Generator(device=DEV).manual_seed(hash((B, H, W, KH, KW, Cout, 7)) % (1 << 31))
    srcC = [c for c, _, _ in case["srcs"]]
    dys, dyv, xss, srcss = [], [], [], []
    for _ in range(case.get("nseg", 1)):
        t = torch.randn(B, H, W, case["ldy"], device=DEV, generator=g) * 0.1
        dys.append(t[..., :Cout])
        dyv.append(ops.V(t, Cout))
        xs, vs = [], []
        for i, (C, ld, off) in enumerate(case["srcs"]):
            x = _src_tensor(B, H, W, ld, min(i, 2) if len(case["srcs"]) > 1 else 1, g)
            xs.append(x[..., off:off + C])
            vs.append(ops.V(x, C, off))
        xss.append(xs)
        srcss.append(vs)
    dwpk = torch.zeros(Cout, ops.conv_ktot(srcC, KH, KW), device=DEV)
    dbias = torch.zeros(Cout, device=DEV) if case.get("bias", True) else None
    with tuning(case.get("knobs")):
        if case.get("multi"):
            ops.conv_wgrad_multi(dyv, srcss, dwpk, B, H, W, KH, KW, dbias=dbias)
        else:
            ops.conv_wgrad(dyv[0], srcss[0], dwpk, B, H, W, KH, KW, dbias=dbias)
        route = last_route(1)
    Cin = sum(srcC)
    dw = ops.unpack_weight_grad(dwpk, (Cout, Cin, KH, KW), srcC)
    torch.cuda.synchronize()
    G = R.wgrad_gemm(dys, xss, B, H, W, KH, KW).reshape(Cout, -1)
    S = R.wgrad_gemm(dys, xss, B, H, W, KH, KW, "abs").reshape(Cout, -1)
    twins = {m: R.wgrad_gemm(dys, xss, B, H, W, KH, KW, m).reshape(Cout, -1) for m in ("fp32", "bf16x3", "bf16x1")}
    # mutant (a): the last (ragged) 64-pixel tile of the last segment loses one 32-channel chunk of the centre tap
    lo = (M - 1) // 64 * 64
    rows = torch.arange(lo, M, device=DEV)
    a = R.columns([x.reshape(B, H, W, -1).double() for x in xss[-1]], B, H, W, KH, KW, (KH // 2, KW // 2), rows)
    tap = KH * KW // 2
    cut = torch.zeros(KH * KW, Cin, dtype=torch.float64, device=DEV)
    cut[tap, :min(32, Cin)] = 1
    dmut = (dys[-1].reshape(M, Cout)[lo:].double().t() @ (a * cut.reshape(1, -1))).reshape(Cout, KH, KW, Cin)
    mut = G - dmut.permute(0, 3, 1, 2).reshape(Cout, -1)
    got = {"dst0": dw.reshape(Cout, -1)}
    ok_bias = True
    if dbias is not None:
        bref = sum(d.reshape(M, Cout).double().sum(0) for d in dys)
        babs = sum(d.reshape(M, Cout).double().abs().sum(0) for d in dys)
        ok_bias = bool(((dbias.double() - bref).abs() <= R.gamma("fp32", M * len(dys)) * babs + 1e-30).all())
    return route, got, R.Epi(0), G, S, M * len(dys), twins, mut, ok_bias


def _judge(kind, name, route, expect, precision, res, arith_knob=False):
    got, epi, G, S, K, twins, mut = res
    table = _lib().CONV_ROUTES if kind == "fwd" else _lib().WGRAD_ROUTES
    if precision == "split" or arith_knob:
        assert route == expect, f"{name}: route {route} ({table.get(route)}), table says {expect} ({table.get(expect)})"
    assert route in table, f"{name}: unknown route {route}"
    rname, arith = table[route]
    if precision == "exact" and not arith_knob:
        assert arith == "fp32", f"{name}: exact mode ran {rname} ({arith})"
    ok, rejected, rep = R.verdict(got, epi, G, S, K, arith, twins, mut, log=_log_margin, what=f"{name} [{rname} {precision}]")
    _log_case(dict(case=name, kind=kind, precision=precision, route=route, route_name=rname, K=K,
                   **{f"{o}.{k}": v for o, r in rep.items() for k, v in r.items() if not isinstance(v, str)}))
    assert rejected, f"{name}: the comparator did not reject both mutants ({rep})"
    assert ok, f"{name} on {rname} ({precision}): {rep}"


# ------------------------------------------------------------------------------------------------------------ case table
def nhwc(width, ld=None, off=0, n0=0, acc=0, maskC=0):
    """Dst spec of a [B, H, W, ld] destination (bs / ps resolved by _fix)."""
    return ["nhwc", ld or (width + 3) // 4 * 4, off, n0, acc, maskC]


def _fix(c):
    c = dict(c)
    c.setdefault("srcs", [])
    c["srcs"] = [tuple(s) if isinstance(s, (list, tuple)) else (s, (s + 3) // 4 * 4, 0) for s in c["srcs"]]
    HW = c["H"] * c["W"]
    dsts = []
    for d in c.get("dsts") or [nhwc(c["N"])]:
        if d[0] == "nhwc":
            _, ld, off, n0, acc, maskC = d
            dsts.append((HW * ld, ld, 1, off, n0, acc, maskC))
        elif d[0] == "nchw":
            _, ctot, off, n0, acc, maskC = d
            dsts.append((ctot * HW, 1, HW, off * HW, n0, acc, maskC))
        else:
            dsts.append(tuple(d))
    c["dsts"] = dsts
    return c


def F(name, route, B, H, W, KH, KW, srcs, N, **kw):
    return pytest.param(_fix(dict(B=B, H=H, W=W, KH=KH, KW=KW, srcs=srcs, N=N, route=route, **kw)), id=name)


def Wg(name, route, B, H, W, KH, KW, srcs, Cout, **kw):
    c = dict(B=B, H=H, W=W, KH=KH, KW=KW, Cout=Cout, ldy=(Cout + 3) // 4 * 4, route=route, **kw)
    c["srcs"] = [tuple(s) if isinstance(s, (list, tuple)) else (s, (s + 3) // 4 * 4, 0) for s in srcs]
    return pytest.param(c, id=name)


GRU_ZR = dict(epi=2, bias=True, lds=dict(pre=256))
GRU_Q = dict(epi=3, bias=True, lds=dict(pre=128))

# Threshold and forced cases (route = the split-mode route of include/fsraft_tuning.h; exact mode must run an fp32 route).
FWD_CASES = [
    # resident-patch kernel: 256-pixel tiles once wg8 >= 200, 128-pixel tiles on small grids with N > 128, from M = 8192 (key 31)
    F("patch256_zr_bench", 11, 4, 55, 128, 3, 3, [128, 256], 256, **GRU_ZR),
    F("patch256_1x5", 11, 4, 55, 128, 1, 5, [128, (128, 128, 0), 128], 256, bias=True),
    F("patch256_5x1", 11, 4, 55, 128, 5, 1, [128, 256], 256, bias=True, relu=True),
    F("patch128_at_8192", 10, 1, 64, 128, 3, 3, [96], 256, bias=True),
    F("patch128_ragged_8281", 10, 1, 91, 91, 3, 3, [96, 37], 256),
    F("below_patch_8190", 33, 1, 91, 90, 3, 3, [96, 37], 256),
    F("patch64_at_8192", 12, 1, 64, 128, 3, 3, [128], 64, bias=True, relu=True),
    F("patch64_ragged_n36", 12, 1, 91, 91, 3, 3, [128, 64], 36),
    F("patch64_th4_forced_key28_2", 12, 1, 256, 256, 3, 3, [64], 64, knobs={28: 2}),
    F("patch64_th8_forced_key28_3", 13, 1, 256, 256, 3, 3, [64], 64, knobs={28: 3}),
    # conv3x3_halo_kernel (fragment-order pack, one source of 33..64 channels) and the 256x64 tiles, from M = 65536
    F("halo21_at_65536", 20, 2, 128, 256, 3, 3, [64], 64, frag=True, bias=True, relu=True),
    F("halo22_at_65536", 21, 2, 128, 256, 3, 3, [64], 96, frag=True, dsts=[nhwc(96, acc=1)]),
    F("halo_below_65535", 11, 1, 255, 257, 3, 3, [64], 96, frag=True),
    F("split256x64_at_65536", 31, 1, 256, 256, 3, 3, [64], 64),
    F("split256x64_ragged_1x1", 31, 2, 181, 182, 1, 1, [100], 60, bias=True),
    F("below_256x64_65535", 33, 1, 255, 257, 1, 1, [64], 64),
    # sixteen-wave 256x128 tiles for N in 192..512 from M = 16384; eight-wave 128x128 tiles when they fill the machine
    F("w16_at_16384", 32, 1, 128, 128, 1, 1, [324], 256, bias=True, relu=True),
    F("w16_ragged_n500", 32, 1, 129, 131, 1, 1, [(130, 132, 0), 126], 500),
    F("w8_below_16383", 33, 1, 43, 381, 1, 1, [324], 256, bias=True),
    F("w8_bench_q", 33, 4, 55, 128, 3, 3, [128, 256], 128, **GRU_Q),
    # 64x128 tiles, split-K slices + conv_finish_kernel (small grids, M <= 16384 workspace)
    F("ksplit_m64_n126", 134, 1, 46, 96, 3, 3, [256], 126, bias=True),
    F("ksplit_w8_zr", 133, 1, 47, 156, 3, 3, [128, 256], 256, **GRU_ZR),
    F("ksplit_m64_q", 134, 1, 47, 156, 3, 3, [128, 256], 128, **GRU_Q),
    F("ksplit_w8_multi_dst", 133, 1, 46, 96, 1, 5, [384], 256, relu=True, alpha=0.5,
      dsts=[["nchw", 200, 8, 0, 1, 0], nhwc(64, ld=68, n0=192, acc=0, maskC=64)]),
    F("ksplit_forced_16384", 133, 1, 128, 128, 1, 1, [384], 100, knobs={32: 2}),
    F("ksplit_forced_over_ws_16385", 33, 1, 29, 565, 1, 1, [384], 100, knobs={32: 2}),
    F("m64_no_ksplit_1x1", 34, 1, 46, 96, 1, 1, [324], 128, bias=True),
    F("m64_ragged_w7", 134, 2, 70, 7, 3, 3, [37, 45, 82], 100, bias=True),
    F("m64_ragged_w30", 134, 2, 70, 30, 3, 3, [(37, 40, 0), (45, 48, 0)], 126, relu=True),
    F("m64_pad_s2d_2x2", 134, 4, 27, 64, 2, 2, [256], 96),
    F("w8_pad0_s2d_2x2_dgrad", 33, 4, 27, 64, 2, 2, [96], 256, pad=(0, 0)),
    # N <= 32 (exact 128x32 in both modes), N <= 64 without a split pack (exact 128x64)
    F("gemm32_n2", 1, 4, 55, 128, 3, 3, [256], 2, bias=True),
    F("gemm32_n2_ragged", 1, 1, 46, 97, 3, 3, [128], 2),
    F("gemm64_no_split_pack", 2, 1, 46, 96, 3, 3, [64], 36, split=False),
    # forced tiles
    F("forced_key3_3_m64", 34, 1, 128, 128, 3, 3, [128], 128, knobs={3: 3}),
    F("forced_key3_4_128", 35, 1, 128, 128, 3, 3, [128], 128, knobs={3: 4}),
    F("forced_key3_5_n256", 130, 1, 46, 96, 3, 3, [128], 256, knobs={3: 5}),
    F("forced_key9_n256", 30, 1, 128, 128, 1, 1, [128], 256, knobs={9: 1}),
    F("ksplit_forced_w16_16384", 132, 1, 128, 128, 1, 1, [384], 256, bias=True, knobs={32: 2}),
    F("ksplit_forced_key3_4_128", 135, 1, 46, 96, 3, 3, [128], 128, knobs={3: 4, 5: 2, 32: 2}),
    # exact tiles a tuning key selects (key 0; key 3 = 0 keeps the case in exact mode whatever the fixture says)
    F("forced_key0_3_exact64x64", 5, 1, 46, 97, 3, 3, [96, 37], 100, knobs={3: 0, 0: 3}),
    F("forced_key0_4_exact64x64k16", 6, 1, 46, 97, 3, 3, [96, 37], 100, knobs={3: 0, 0: 4}),
    F("forced_key0_5_exact64x128k16", 7, 1, 46, 97, 3, 3, [96, 37], 100, knobs={3: 0, 0: 5}),
    F("forced_key0_1_exact128", 4, 1, 46, 97, 1, 5, [128], 200, knobs={3: 0, 0: 1}),
    F("forced_key0_2_exact64x128", 3, 4, 55, 128, 1, 1, [324], 256, knobs={3: 0, 0: 2}),
]

WGRAD_CASES = [
    Wg("patch_single_at_8192", 7, 1, 64, 128, 3, 3, [64], 64),
    Wg("patch_single_ragged_2src", 7, 2, 45, 93, 3, 3, [96, 33], 100),
    Wg("pack_below_8190", 6, 1, 91, 90, 3, 3, [64], 64),
    Wg("pack_ragged_w7", 6, 2, 70, 7, 3, 3, [(37, 40, 0)], 36),
    Wg("split128S_3src", 5, 1, 46, 96, 3, 3, [37, 45, 82], 100),
    Wg("split128S_1x1_bench", 5, 4, 55, 128, 1, 1, [324], 256),
    Wg("exact32_n2", 1, 4, 55, 128, 3, 3, [256], 2),
    Wg("multi_patch_3x3", 7, 1, 46, 96, 3, 3, [128, (64, 68, 0)], 128, nseg=3, multi=True),
    Wg("multi_1x5", 8, 1, 46, 96, 1, 5, [128, 128], 126, nseg=3, multi=True),
    Wg("multi_1x5_key27_2", 7, 1, 46, 96, 1, 5, [128, 128], 128, nseg=2, multi=True, knobs={27: 2}),
    Wg("multi_w8_key15", 9, 1, 46, 96, 1, 1, [256], 128, nseg=3, multi=True, knobs={15: 1}),
    Wg("exact64_key1_3", 2, 1, 46, 96, 3, 3, [128], 128, knobs={1: 3}),
    Wg("split128_key4_1", 4, 1, 46, 96, 1, 1, [256], 128, knobs={4: 1}),
    Wg("exact128_key4_0", 3, 1, 46, 96, 1, 1, [256], 128, knobs={4: 0}),
]
ARITH_KNOBS = (3, 4)


def _arith_knob(case):
    return any(k in ARITH_KNOBS for k in (case.get("knobs") or {}))


def _case_id(request):
    return request.node.callspec.id.split("-", 1)[1]


@pytest.mark.parametrize("case", FWD_CASES)
def test_forward_route(case, precision, request):
    route, *res = run_fwd(case, precision)
    _judge("fwd", _case_id(request), route, case["route"], precision, res, _arith_knob(case))


@pytest.mark.parametrize("case", WGRAD_CASES)
def test_weight_gradient_route(case, precision, request):
    route, *res, ok_bias = run_wgrad(case)
    _judge("wgrad", _case_id(request), route, case["route"], precision, res, _arith_knob(case))
    assert ok_bias, "fused / separate bias gradient"


def test_weight_unpack_is_the_packed_k_layout():
    """ops.unpack_weight_grad (pack kernel mode 2) and ops.pack_weight (mode 0) against the Python restatement of the K layout:
    per source, taps x 32-padded channels.  Bit-exact (a permutation)."""
    ops = _ops()
    for srcC, KH, KW in (([37, 2, 64], 1, 5), ([128, 96], 3, 3), ([4 * 24], 2, 2), ([324], 1, 1)):
        Cout = 70
        wpk = torch.randn(Cout, ops.conv_ktot(srcC, KH, KW), device=DEV)
        got = ops.unpack_weight_grad(wpk, (Cout, sum(srcC), KH, KW), srcC)
        assert torch.equal(got, R.unpack_ref(wpk, srcC, KH, KW)), (srcC, KH, KW)
        w = torch.randn(Cout, sum(srcC), KH, KW, device=DEV)
        assert torch.equal(ops.pack_weight(w, srcC, 0), R.pack_ref(w, srcC)), (srcC, KH, KW)


# ------------------------------------------------------------------------------------------------------------ coverage guard
def _fwd_key(srcs, B, H, W, KH, KW, N, dsts, relu=False, alpha=1.0, epi=0, h=None, z=None, aux1=None, aux2=None, hid=0,
             wpk_split=None, pre=None, wpk_frag=None, pad=None, bias=None, **_):
    k = dict(B=B, H=H, W=W, KH=KH, KW=KW, srcs=[(v.C, v.ld, v.off) for v in srcs], N=N)
    if epi:
        k["epi"] = epi
        k["lds"] = {n: t.shape[-1] for n, t in (("h", h), ("z", z), ("aux1", aux1), ("aux2", aux2), ("pre", pre)) if t is not None}
    else:
        k["dsts"] = [(d.bs, d.ps, d.cs, d.off, d.n0, int(d.acc), d.mask.C if d.mask is not None else 0) for d in dsts]
    for name, v, dflt in (("relu", bool(relu), False), ("alpha", float(alpha), 1.0), ("bias", bias is not None, False),
                          ("split", wpk_split is not None, True), ("frag", wpk_frag is not None, False),
                          ("pad", list(pad) if pad is not None else None, None)):
        if v != dflt:
            k[name] = v
    return k


def _canon(k):
    return json.dumps(k, sort_keys=True)


def record_step(workload):
    """One eager step of a benchmark configuration with the three convolution entry points wrapped: [(kind, key, route)] of
    every call (metadata and route only: no copies, no syncs)."""
    import flow_supervisor_amd.ops as ops
    from flow_supervisor_amd.core import streams
    calls = []
    f0, w0, m0 = ops.conv_forward, ops.conv_wgrad, ops.conv_wgrad_multi

    def fwd(srcs, wpk, bias, B, H, W, KH, KW, N, dsts, **kw):
        r = f0(srcs, wpk, bias, B, H, W, KH, KW, N, dsts, **kw)
        calls.append(("fwd", _fwd_key(srcs, B, H, W, KH, KW, N, dsts, bias=bias, **kw), last_route(0)))
        return r

    def _wkey(dy, srcs, B, H, W, KH, KW, dbias, nseg, multi):
        return dict(B=B, H=H, W=W, KH=KH, KW=KW, Cout=dy.C, ldy=dy.ld, srcs=[(v.C, v.ld, v.off) for v in srcs], nseg=nseg,
                    multi=multi, bias=dbias is not None)

    def wg(dy, srcs, dwpk, B, H, W, KH, KW, dbias=None):
        w0(dy, srcs, dwpk, B, H, W, KH, KW, dbias=dbias)
        calls.append(("wgrad", _wkey(dy, srcs, B, H, W, KH, KW, dbias, 1, False), last_route(1)))

    def wm(dys, srcs, dwpk, B, H, W, KH, KW, dbias=None):
        m0(dys, srcs, dwpk, B, H, W, KH, KW, dbias=dbias)
        calls.append(("wgrad", _wkey(dys[0], srcs[0], B, H, W, KH, KW, dbias, len(dys), True), last_route(1)))

    saved = streams.OVERLAP
    streams.OVERLAP = False              # one host thread, one stream: the thread-local route is this call's
    ops.conv_forward, ops.conv_wgrad, ops.conv_wgrad_multi = fwd, wg, wm
    try:
        WORKLOADS[workload]()
    finally:
        ops.conv_forward, ops.conv_wgrad, ops.conv_wgrad_multi = f0, w0, m0
        streams.OVERLAP = saved
    torch.cuda.synchronize()
    return calls


def _images(B, H, W, seed=1234):
    g = torch.Generator(device=DEV).manual_seed(seed)
    i1 = torch.rand(B, 3, H, W, device=DEV, generator=g) * 255.0
    i2 = (torch.roll(i1, shifts=(3, -5), dims=(2, 3)) + 2.0 * torch.randn(B, 3, H, W, device=DEV, generator=g)).clamp(0, 255)
    return i1, i2


def _raft_step(B, H, W, small=False, alt=False, gma=False, iters=12):
    from flow_supervisor_amd.train import TrainStep
    torch.manual_seed(0)
    if gma:
        from flow_supervisor_amd.core.gma_network import RAFTGMA
        model = RAFTGMA(argparse.Namespace(mixed_precision=False, num_heads=1, position_only=False, position_and_content=False))
    else:
        from flow_supervisor_amd.core.raft import RAFT
        model = RAFT(argparse.Namespace(small=small, mixed_precision=False, alternate_corr=alt))
    model = model.to(DEV).train()
    model.freeze_bn()
    TrainStep(model, lr=1.6e-5, iters=iters)(*_images(B, H, W))


def _l2l_step(B=1, H=432, W=1024, ch=368, cw=768, iters=12):
    from flow_supervisor_amd.core.l2l import L2L
    from flow_supervisor_amd.train import SemiTrainStep
    torch.manual_seed(0)
    model = L2L(argparse.Namespace(small=False, mixed_precision=False, alternate_corr=False)).to(DEV).train()
    model.freeze_bn()
    sstep = SemiTrainStep(model, lr=5e-6, wdecay=0.0, iters=iters, gamma=0.8, unsup_lambda=1.0)
    g = torch.Generator(device=DEV).manual_seed(7)

    def sample(f1, f2, oy, ox):
        c1 = f1[:, :, oy:oy + ch, ox:ox + cw].contiguous()
        c2 = f2[:, :, oy:oy + ch, ox:ox + cw].contiguous()
        flow = torch.randn(B, 2, ch, cw, device=DEV, generator=g) * 4.0
        valid = (torch.rand(B, ch, cw, device=DEV, generator=g) > 0.1).float()
        return (c1, c2, f1, f2, ox, oy, flow, valid)
    i1, i2 = _images(B, H, W)
    j1, j2 = _images(B, H, W, 99)
    sstep(sample(i1, i2, 40, 136), sample(j1, j2, 16, 200))


WORKLOADS = {
    "raft_b4_440x1024": lambda: _raft_step(4, 440, 1024),
    "raft_b1_440x1024": lambda: _raft_step(1, 440, 1024),
    "chairs_b8_368x496": lambda: _raft_step(8, 368, 496),
    "kitti_alt_b4_376x1248": lambda: _raft_step(4, 376, 1248, alt=True),
    "gma_b4_440x1024": lambda: _raft_step(4, 440, 1024, gma=True),
    "l2l_368x768": lambda: _l2l_step(),
    "small_b4_440x1024": lambda: _raft_step(4, 440, 1024, small=True),
}


def dump_production(path):
    """Every distinct convolution call of one eager step of each workload, with its route (the source of PROD below)."""
    seen = {}
    for name in WORKLOADS:
        for kind, key, route in record_step(name):
            e = seen.setdefault((kind, _canon(key)), dict(kind=kind, key=key, routes=set(), workloads=set()))
            e["routes"].add(route)
            e["workloads"].add(name)
    out = [dict(kind=e["kind"], key=e["key"], routes=sorted(e["routes"]), workloads=sorted(e["workloads"])) for e in seen.values()]
    with open(path, "w") as f:
        json.dump(out, f)
    return out


def _prod_case(kind, route, key):
    c = json.loads(json.dumps(key))            # private copy
    c["route"] = route
    c["srcs"] = [tuple(s) for s in c["srcs"]]
    if kind == "fwd" and "dsts" in c:
        c["dsts"] = [tuple(d) for d in c["dsts"]]
    return c


def _prod_id(i, kind, route, key):
    src = "+".join(str(s[0]) for s in key["srcs"])
    out = key["N"] if kind == "fwd" else key["Cout"]
    return f"{kind}{i}_{key['B']}x{key['H']}x{key['W']}_{key['KH']}x{key['KW']}_{src}to{out}_r{route}"


@pytest.mark.parametrize("workload", list(WORKLOADS))
def test_coverage_guard(workload):
    """Every convolution call of one eager step of `workload` is a PROD entry and took PROD's route.  A model or dispatch
    change that reaches an untested shape or route fails here with the missing entry (add it to PROD: the case then runs)."""
    table = {(kind, _canon(key)): route for kind, route, _, key in PROD}
    letter = WORKLOAD_LETTERS[workload]
    missing, moved = [], []
    for kind, key, route in record_step(workload):
        t = table.get((kind, _canon(key)))
        if t is None:
            missing.append(f"({kind!r}, {route}, {letter!r}, {_canon(key)}),")
        elif t != route:
            moved.append(f"{kind} {_canon(key)}: route {route}, PROD says {t}")
    assert not missing, "calls with no PROD entry:\n" + "\n".join(sorted(set(missing)))
    assert not moved, "calls on another route than PROD's:\n" + "\n".join(sorted(set(moved)))


def test_every_default_route_has_a_case():
    """Every route code the default knobs can reach is exercised by a PROD entry or by a threshold case of its own; every
    other code by a forced case, or it is listed in UNTESTED_ROUTES with its reason."""
    cases = [("fwd", p.values[0]) for p in FWD_CASES] + [("wgrad", p.values[0]) for p in WGRAD_CASES]
    have = {(kind, route) for kind, route, _, _ in PROD}
    have |= {(kind, c["route"]) for kind, c in cases if not c.get("knobs")}
    want = {("fwd", r) for r in DEFAULT_FWD_ROUTES} | {("wgrad", r) for r in DEFAULT_WGRAD_ROUTES}
    assert want <= have, sorted(want - have)
    forced = {(kind, c["route"]) for kind, c in cases if c.get("knobs")}
    known = {("fwd", r) for r in _lib().CONV_ROUTES} | {("wgrad", r) for r in _lib().WGRAD_ROUTES}
    assert known - have - forced == UNTESTED_ROUTES, sorted((known - have - forced) ^ UNTESTED_ROUTES)


# Reachable with the default knobs in split mode: patch, halo, 256x64, sixteen- / eight-wave and 64x128 split tiles, split-K on
# the 64-row and eight-wave tiles, the fp32 tiles of N <= 32 and of calls without a split pack.  (The exact-mode routes -- fp32
# 64x128 / 128x128 forward tiles, 128x128 weight-gradient tiles -- run in the exact half of every case and have forced cases.)
DEFAULT_FWD_ROUTES = (1, 2, 10, 11, 12, 20, 21, 31, 32, 33, 34, 133, 134)
DEFAULT_WGRAD_ROUTES = (1, 5, 6, 7, 8)
# Codes no case reaches: 131 (unreachable: the 256x64 tiles have a plain-epilogue launcher without split-K).
UNTESTED_ROUTES = {("fwd", 131)}
WORKLOAD_LETTERS = {"raft_b4_440x1024": "A", "raft_b1_440x1024": "B", "chairs_b8_368x496": "C", "kitti_alt_b4_376x1248": "K",
                    "gma_b4_440x1024": "G", "l2l_368x768": "L", "small_b4_440x1024": "S"}

# Every distinct convolution call of one eager train step (forward + backward) of the seven benchmark configurations, with the
# route it takes in split mode (exact mode: any fp32 route).  Workloads: A RAFT B=4 440x1024, B RAFT B=1 440x1024, C chairs
# B=8 368x496, K KITTI 376x1248 alt-corr B=4, G RAFT-GMA B=4 440x1024, L the L2L recipe (one labelled + one unlabelled 368x768
# crop of 432x1024 frames), S the small model B=4 440x1024.  Entries: (kind, route, workloads, key); dump_production() on an
# MI355X regenerates them.
PROD = [
    ('fwd', 1, 'S', {"B":4,"H":55,"KH":3,"KW":3,"N":32,"W":128,"bias":True,"dsts":[[901120,128,1,96,0,0,0]],"relu":True,"srcs":[[64,64,0]]}),
    ('fwd', 1, 'S', {"B":8,"H":55,"KH":1,"KW":1,"N":24,"W":128,"dsts":[[168960,24,1,0,0,0,0]],"srcs":[[96,96,0]]}),
    ('fwd', 1, 'S', {"B":8,"H":55,"KH":3,"KW":3,"N":24,"W":128,"dsts":[[168960,24,1,0,0,0,0]],"srcs":[[24,24,0]]}),
    ('fwd', 1, 'S', {"B":8,"H":110,"KH":1,"KW":1,"N":16,"W":256,"dsts":[[450560,16,1,0,0,0,0]],"srcs":[[64,64,0]]}),
    ('fwd', 1, 'S', {"B":8,"H":110,"KH":3,"KW":3,"N":16,"W":256,"dsts":[[450560,16,1,0,0,0,0]],"srcs":[[16,16,0]]}),
    ('fwd', 1, 'S', {"B":8,"H":220,"KH":1,"KW":1,"N":32,"W":512,"dsts":[[3604480,32,1,0,0,0,0]],"srcs":[[8,8,0]]}),
    ('fwd', 1, 'S', {"B":8,"H":220,"KH":1,"KW":1,"N":32,"W":512,"dsts":[[3604480,32,1,0,0,1,0]],"srcs":[[8,8,0]]}),
    ('fwd', 1, 'S', {"B":8,"H":220,"KH":1,"KW":1,"N":8,"W":512,"dsts":[[901120,8,1,0,0,0,0]],"srcs":[[32,32,0]]}),
    ('fwd', 1, 'S', {"B":8,"H":220,"KH":3,"KW":3,"N":8,"W":512,"dsts":[[901120,8,1,0,0,0,0]],"srcs":[[8,8,0]]}),
    ('fwd', 10, 'L', {"B":2,"H":46,"KH":3,"KW":3,"N":192,"W":96,"bias":True,"dsts":[[1130496,256,1,0,0,0,0]],"relu":True,"srcs":[[256,256,0]]}),
    ('fwd', 10, 'L', {"B":2,"H":46,"KH":3,"KW":3,"N":512,"W":96,"bias":True,"dsts":[[2260992,512,1,0,0,0,0]],"relu":True,"srcs":[[128,128,0]]}),
    ('fwd', 10, 'L', {"B":2,"H":54,"KH":3,"KW":3,"N":192,"W":128,"bias":True,"dsts":[[1769472,256,1,0,0,0,0]],"relu":True,"srcs":[[256,256,0]]}),
    ('fwd', 10, 'C', {"B":8,"H":46,"KH":3,"KW":3,"N":192,"W":62,"bias":True,"dsts":[[730112,256,1,0,0,0,0]],"relu":True,"srcs":[[256,256,0]]}),
    ('fwd', 11, 'L', {"B":2,"H":54,"KH":3,"KW":3,"N":512,"W":128,"bias":True,"dsts":[[3538944,512,1,0,0,0,0]],"relu":True,"srcs":[[128,128,0]]}),
    ('fwd', 11, 'C', {"B":8,"H":46,"KH":3,"KW":3,"N":512,"W":62,"bias":True,"dsts":[[1460224,512,1,0,0,0,0]],"relu":True,"srcs":[[128,128,0]]}),
    ('fwd', 11, 'AG', {"B":4,"H":55,"KH":1,"KW":5,"N":256,"W":128,"bias":True,"dsts":[[1802240,256,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 11, 'A', {"B":4,"H":55,"KH":1,"KW":5,"N":256,"W":128,"dsts":[[901120,128,1,0,0,0,0],[901120,128,1,0,128,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 11, 'A', {"B":4,"H":55,"KH":1,"KW":5,"N":256,"W":128,"dsts":[[901120,128,1,0,0,1,0],[901120,128,1,0,128,1,126]],"srcs":[[256,256,0]]}),
    ('fwd', 11, 'A', {"B":4,"H":55,"KH":1,"KW":5,"N":256,"W":128,"epi":2,"lds":{"aux1":128,"aux2":128,"h":128,"pre":256},"srcs":[[128,128,0],[128,128,0]]}),
    ('fwd', 11, 'G', {"B":4,"H":55,"KH":1,"KW":5,"N":256,"W":128,"epi":2,"lds":{"aux1":128,"aux2":128,"h":128,"pre":256},"srcs":[[128,128,0],[256,256,0]]}),
    ('fwd', 11, 'G', {"B":4,"H":55,"KH":1,"KW":5,"N":384,"W":128,"dsts":[[901120,128,1,0,0,0,0],[1802240,256,1,0,128,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 11, 'G', {"B":4,"H":55,"KH":1,"KW":5,"N":384,"W":128,"dsts":[[901120,128,1,0,0,1,0],[1802240,256,1,0,128,1,0]],"srcs":[[256,256,0]]}),
    ('fwd', 11, 'S', {"B":4,"H":55,"KH":3,"KW":3,"N":178,"W":128,"dsts":[[675840,96,1,0,0,0,0],[591360,84,1,0,96,0,0]],"srcs":[[96,96,0]]}),
    ('fwd', 11, 'S', {"B":4,"H":55,"KH":3,"KW":3,"N":178,"W":128,"dsts":[[675840,96,1,0,0,1,0],[591360,84,1,0,96,1,80]],"srcs":[[192,192,0]]}),
    ('fwd', 11, 'S', {"B":4,"H":55,"KH":3,"KW":3,"N":192,"W":128,"bias":True,"dsts":[[1351680,192,1,0,0,0,0]],"srcs":[[64,64,0]]}),
    ('fwd', 11, 'AG', {"B":4,"H":55,"KH":3,"KW":3,"N":192,"W":128,"bias":True,"dsts":[[1802240,256,1,0,0,0,0]],"relu":True,"srcs":[[256,256,0]]}),
    ('fwd', 11, 'S', {"B":4,"H":55,"KH":3,"KW":3,"N":192,"W":128,"epi":2,"lds":{"aux1":96,"aux2":96,"h":96,"pre":192},"srcs":[[96,96,0],[82,84,0]]}),
    ('fwd', 11, 'AG', {"B":4,"H":55,"KH":3,"KW":3,"N":512,"W":128,"bias":True,"dsts":[[3604480,512,1,0,0,0,0]],"relu":True,"srcs":[[128,128,0]]}),
    ('fwd', 11, 'AG', {"B":4,"H":55,"KH":5,"KW":1,"N":256,"W":128,"bias":True,"dsts":[[1802240,256,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 11, 'A', {"B":4,"H":55,"KH":5,"KW":1,"N":256,"W":128,"dsts":[[901120,128,1,0,0,0,0],[901120,128,1,0,128,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 11, 'A', {"B":4,"H":55,"KH":5,"KW":1,"N":256,"W":128,"dsts":[[901120,128,1,0,0,1,0],[901120,128,1,0,128,1,0]],"srcs":[[256,256,0]]}),
    ('fwd', 11, 'A', {"B":4,"H":55,"KH":5,"KW":1,"N":256,"W":128,"epi":2,"lds":{"aux1":128,"aux2":128,"h":128,"pre":256},"srcs":[[128,128,0],[128,128,0]]}),
    ('fwd', 11, 'G', {"B":4,"H":55,"KH":5,"KW":1,"N":256,"W":128,"epi":2,"lds":{"aux1":128,"aux2":128,"h":128,"pre":256},"srcs":[[128,128,0],[256,256,0]]}),
    ('fwd', 11, 'G', {"B":4,"H":55,"KH":5,"KW":1,"N":384,"W":128,"dsts":[[901120,128,1,0,0,0,0],[1802240,256,1,0,128,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 11, 'G', {"B":4,"H":55,"KH":5,"KW":1,"N":384,"W":128,"dsts":[[901120,128,1,0,0,1,0],[1802240,256,1,0,128,1,0]],"srcs":[[256,256,0]]}),
    ('fwd', 11, 'K', {"B":4,"H":47,"KH":1,"KW":5,"N":256,"W":156,"bias":True,"dsts":[[1876992,256,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 11, 'K', {"B":4,"H":47,"KH":1,"KW":5,"N":256,"W":156,"dsts":[[938496,128,1,0,0,0,0],[938496,128,1,0,128,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 11, 'K', {"B":4,"H":47,"KH":1,"KW":5,"N":256,"W":156,"dsts":[[938496,128,1,0,0,1,0],[938496,128,1,0,128,1,126]],"srcs":[[256,256,0]]}),
    ('fwd', 11, 'K', {"B":4,"H":47,"KH":1,"KW":5,"N":256,"W":156,"epi":2,"lds":{"aux1":128,"aux2":128,"h":128,"pre":256},"srcs":[[128,128,0],[128,128,0]]}),
    ('fwd', 11, 'K', {"B":4,"H":47,"KH":3,"KW":3,"N":192,"W":156,"bias":True,"dsts":[[1876992,256,1,0,0,0,0]],"relu":True,"srcs":[[256,256,0]]}),
    ('fwd', 11, 'K', {"B":4,"H":47,"KH":3,"KW":3,"N":512,"W":156,"bias":True,"dsts":[[3753984,512,1,0,0,0,0]],"relu":True,"srcs":[[128,128,0]]}),
    ('fwd', 11, 'K', {"B":4,"H":47,"KH":5,"KW":1,"N":256,"W":156,"bias":True,"dsts":[[1876992,256,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 11, 'K', {"B":4,"H":47,"KH":5,"KW":1,"N":256,"W":156,"dsts":[[938496,128,1,0,0,0,0],[938496,128,1,0,128,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 11, 'K', {"B":4,"H":47,"KH":5,"KW":1,"N":256,"W":156,"dsts":[[938496,128,1,0,0,1,0],[938496,128,1,0,128,1,0]],"srcs":[[256,256,0]]}),
    ('fwd', 11, 'K', {"B":4,"H":47,"KH":5,"KW":1,"N":256,"W":156,"epi":2,"lds":{"aux1":128,"aux2":128,"h":128,"pre":256},"srcs":[[128,128,0],[128,128,0]]}),
    ('fwd', 11, 'L', {"B":2,"H":108,"KH":3,"KW":3,"N":96,"W":256,"dsts":[[2654208,96,1,0,0,0,0]],"srcs":[[96,96,0]]}),
    ('fwd', 11, 'L', {"B":2,"H":108,"KH":3,"KW":3,"N":96,"W":256,"dsts":[[2654208,96,1,0,0,1,0]],"srcs":[[96,96,0]]}),
    ('fwd', 11, 'B', {"B":2,"H":110,"KH":3,"KW":3,"N":96,"W":256,"dsts":[[2703360,96,1,0,0,0,0]],"srcs":[[96,96,0]]}),
    ('fwd', 11, 'B', {"B":2,"H":110,"KH":3,"KW":3,"N":96,"W":256,"dsts":[[2703360,96,1,0,0,1,0]],"srcs":[[96,96,0]]}),
    ('fwd', 11, 'AG', {"B":8,"H":55,"KH":3,"KW":3,"N":128,"W":128,"dsts":[[901120,128,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 11, 'AG', {"B":8,"H":55,"KH":3,"KW":3,"N":128,"W":128,"dsts":[[901120,128,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 11, 'K', {"B":8,"H":47,"KH":3,"KW":3,"N":128,"W":156,"dsts":[[938496,128,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 11, 'K', {"B":8,"H":47,"KH":3,"KW":3,"N":128,"W":156,"dsts":[[938496,128,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 11, 'L', {"B":4,"H":92,"KH":3,"KW":3,"N":96,"W":192,"dsts":[[1695744,96,1,0,0,0,0]],"srcs":[[96,96,0]]}),
    ('fwd', 11, 'L', {"B":4,"H":92,"KH":3,"KW":3,"N":96,"W":192,"dsts":[[1695744,96,1,0,0,1,0]],"srcs":[[96,96,0]]}),
    ('fwd', 11, 'B', {"B":12,"H":55,"KH":3,"KW":3,"N":128,"W":128,"dsts":[[901120,128,1,0,0,0,0]],"srcs":[[512,512,0]]}),
    ('fwd', 11, 'B', {"B":12,"H":55,"KH":3,"KW":3,"N":128,"W":128,"dsts":[[901120,128,1,0,0,0,128]],"srcs":[[64,256,192]]}),
    ('fwd', 11, 'B', {"B":12,"H":55,"KH":3,"KW":3,"N":256,"W":128,"dsts":[[1802240,256,1,0,0,0,256]],"srcs":[[126,128,0]]}),
    ('fwd', 11, 'B', {"B":12,"H":55,"KH":3,"KW":3,"N":256,"W":128,"dsts":[[1802240,256,1,0,0,0,256]],"srcs":[[192,256,0]]}),
    ('fwd', 11, 'C', {"B":8,"H":92,"KH":3,"KW":3,"N":96,"W":124,"dsts":[[1095168,96,1,0,0,0,0]],"srcs":[[96,96,0]]}),
    ('fwd', 11, 'C', {"B":8,"H":92,"KH":3,"KW":3,"N":96,"W":124,"dsts":[[1095168,96,1,0,0,1,0]],"srcs":[[96,96,0]]}),
    ('fwd', 11, 'L', {"B":24,"H":46,"KH":3,"KW":3,"N":128,"W":96,"dsts":[[565248,128,1,0,0,0,0]],"srcs":[[512,512,0]]}),
    ('fwd', 11, 'L', {"B":24,"H":46,"KH":3,"KW":3,"N":128,"W":96,"dsts":[[565248,128,1,0,0,0,128]],"srcs":[[64,256,192]]}),
    ('fwd', 11, 'L', {"B":24,"H":46,"KH":3,"KW":3,"N":256,"W":96,"dsts":[[1130496,256,1,0,0,0,256]],"srcs":[[126,128,0]]}),
    ('fwd', 11, 'L', {"B":24,"H":46,"KH":3,"KW":3,"N":256,"W":96,"dsts":[[1130496,256,1,0,0,0,256]],"srcs":[[192,256,0]]}),
    ('fwd', 11, 'AG', {"B":4,"H":110,"KH":3,"KW":3,"N":96,"W":256,"dsts":[[2703360,96,1,0,0,0,0]],"srcs":[[96,96,0]]}),
    ('fwd', 11, 'AG', {"B":4,"H":110,"KH":3,"KW":3,"N":96,"W":256,"dsts":[[2703360,96,1,0,0,1,0]],"srcs":[[96,96,0]]}),
    ('fwd', 11, 'K', {"B":4,"H":94,"KH":3,"KW":3,"N":96,"W":312,"dsts":[[2815488,96,1,0,0,0,0]],"srcs":[[96,96,0]]}),
    ('fwd', 11, 'K', {"B":4,"H":94,"KH":3,"KW":3,"N":96,"W":312,"dsts":[[2815488,96,1,0,0,1,0]],"srcs":[[96,96,0]]}),
    ('fwd', 11, 'L', {"B":22,"H":54,"KH":3,"KW":3,"N":128,"W":128,"dsts":[[884736,128,1,0,0,0,128]],"srcs":[[64,256,192]]}),
    ('fwd', 11, 'L', {"B":22,"H":54,"KH":3,"KW":3,"N":256,"W":128,"dsts":[[1769472,256,1,0,0,0,256]],"srcs":[[126,128,0]]}),
    ('fwd', 11, 'L', {"B":22,"H":54,"KH":3,"KW":3,"N":256,"W":128,"dsts":[[1769472,256,1,0,0,0,256]],"srcs":[[192,256,0]]}),
    ('fwd', 11, 'L', {"B":24,"H":54,"KH":3,"KW":3,"N":128,"W":128,"dsts":[[884736,128,1,0,0,0,0]],"srcs":[[512,512,0]]}),
    ('fwd', 11, 'C', {"B":16,"H":92,"KH":3,"KW":3,"N":96,"W":124,"dsts":[[1095168,96,1,0,0,0,0]],"srcs":[[96,96,0]]}),
    ('fwd', 11, 'C', {"B":16,"H":92,"KH":3,"KW":3,"N":96,"W":124,"dsts":[[1095168,96,1,0,0,1,0]],"srcs":[[96,96,0]]}),
    ('fwd', 11, 'AG', {"B":8,"H":110,"KH":3,"KW":3,"N":96,"W":256,"dsts":[[2703360,96,1,0,0,0,0]],"srcs":[[96,96,0]]}),
    ('fwd', 11, 'AG', {"B":8,"H":110,"KH":3,"KW":3,"N":96,"W":256,"dsts":[[2703360,96,1,0,0,1,0]],"srcs":[[96,96,0]]}),
    ('fwd', 11, 'K', {"B":8,"H":94,"KH":3,"KW":3,"N":96,"W":312,"dsts":[[2815488,96,1,0,0,0,0]],"srcs":[[96,96,0]]}),
    ('fwd', 11, 'K', {"B":8,"H":94,"KH":3,"KW":3,"N":96,"W":312,"dsts":[[2815488,96,1,0,0,1,0]],"srcs":[[96,96,0]]}),
    ('fwd', 11, 'C', {"B":96,"H":46,"KH":3,"KW":3,"N":128,"W":62,"dsts":[[365056,128,1,0,0,0,0]],"srcs":[[512,512,0]]}),
    ('fwd', 11, 'C', {"B":96,"H":46,"KH":3,"KW":3,"N":128,"W":62,"dsts":[[365056,128,1,0,0,0,128]],"srcs":[[64,256,192]]}),
    ('fwd', 11, 'C', {"B":96,"H":46,"KH":3,"KW":3,"N":256,"W":62,"dsts":[[730112,256,1,0,0,0,256]],"srcs":[[126,128,0]]}),
    ('fwd', 11, 'C', {"B":96,"H":46,"KH":3,"KW":3,"N":256,"W":62,"dsts":[[730112,256,1,0,0,0,256]],"srcs":[[192,256,0]]}),
    ('fwd', 11, 'AG', {"B":48,"H":55,"KH":3,"KW":3,"N":128,"W":128,"dsts":[[901120,128,1,0,0,0,0]],"srcs":[[512,512,0]]}),
    ('fwd', 11, 'AG', {"B":48,"H":55,"KH":3,"KW":3,"N":128,"W":128,"dsts":[[901120,128,1,0,0,0,128]],"srcs":[[64,256,192]]}),
    ('fwd', 11, 'A', {"B":48,"H":55,"KH":3,"KW":3,"N":256,"W":128,"dsts":[[1802240,256,1,0,0,0,256]],"srcs":[[126,128,0]]}),
    ('fwd', 11, 'G', {"B":48,"H":55,"KH":3,"KW":3,"N":256,"W":128,"dsts":[[1802240,256,1,0,0,0,256]],"srcs":[[126,256,0]]}),
    ('fwd', 11, 'AG', {"B":48,"H":55,"KH":3,"KW":3,"N":256,"W":128,"dsts":[[1802240,256,1,0,0,0,256]],"srcs":[[192,256,0]]}),
    ('fwd', 11, 'K', {"B":48,"H":47,"KH":3,"KW":3,"N":128,"W":156,"dsts":[[938496,128,1,0,0,0,0]],"srcs":[[512,512,0]]}),
    ('fwd', 11, 'K', {"B":48,"H":47,"KH":3,"KW":3,"N":128,"W":156,"dsts":[[938496,128,1,0,0,0,128]],"srcs":[[64,256,192]]}),
    ('fwd', 11, 'K', {"B":48,"H":47,"KH":3,"KW":3,"N":256,"W":156,"dsts":[[1876992,256,1,0,0,0,256]],"srcs":[[126,128,0]]}),
    ('fwd', 11, 'K', {"B":48,"H":47,"KH":3,"KW":3,"N":256,"W":156,"dsts":[[1876992,256,1,0,0,0,256]],"srcs":[[192,256,0]]}),
    ('fwd', 12, 'L', {"B":2,"H":46,"KH":3,"KW":3,"N":64,"W":96,"bias":True,"dsts":[[1130496,256,1,192,0,0,0]],"relu":True,"srcs":[[128,128,0]]}),
    ('fwd', 12, 'L', {"B":2,"H":54,"KH":3,"KW":3,"N":64,"W":128,"bias":True,"dsts":[[1769472,256,1,192,0,0,0]],"relu":True,"srcs":[[128,128,0]]}),
    ('fwd', 12, 'C', {"B":8,"H":46,"KH":3,"KW":3,"N":64,"W":62,"bias":True,"dsts":[[730112,256,1,192,0,0,0]],"relu":True,"srcs":[[128,128,0]]}),
    ('fwd', 12, 'AG', {"B":4,"H":55,"KH":3,"KW":3,"N":64,"W":128,"bias":True,"dsts":[[1802240,256,1,192,0,0,0]],"relu":True,"srcs":[[128,128,0]]}),
    ('fwd', 12, 'S', {"B":4,"H":55,"KH":3,"KW":3,"N":64,"W":128,"dsts":[[450560,64,1,0,0,0,0]],"srcs":[[192,192,0]]}),
    ('fwd', 12, 'S', {"B":4,"H":55,"KH":3,"KW":3,"N":64,"W":128,"dsts":[[450560,64,1,0,0,0,64]],"srcs":[[32,128,96]]}),
    ('fwd', 12, 'S', {"B":4,"H":55,"KH":3,"KW":3,"N":64,"W":128,"dsts":[[450560,64,1,0,0,1,0]],"srcs":[[96,96,0]]}),
    ('fwd', 12, 'K', {"B":4,"H":47,"KH":3,"KW":3,"N":64,"W":156,"bias":True,"dsts":[[1876992,256,1,192,0,0,0]],"relu":True,"srcs":[[128,128,0]]}),
    ('fwd', 20, 'B', {"B":1,"H":220,"KH":3,"KW":3,"N":64,"W":512,"dsts":[[7208960,64,1,0,0,0,0]],"frag":True,"srcs":[[64,64,0]]}),
    ('fwd', 20, 'B', {"B":1,"H":220,"KH":3,"KW":3,"N":64,"W":512,"dsts":[[7208960,64,1,0,0,1,0]],"frag":True,"srcs":[[64,64,0]]}),
    ('fwd', 20, 'L', {"B":2,"H":184,"KH":3,"KW":3,"N":64,"W":384,"dsts":[[4521984,64,1,0,0,0,0]],"frag":True,"srcs":[[64,64,0]]}),
    ('fwd', 20, 'L', {"B":2,"H":184,"KH":3,"KW":3,"N":64,"W":384,"dsts":[[4521984,64,1,0,0,1,0]],"frag":True,"srcs":[[64,64,0]]}),
    ('fwd', 20, 'L', {"B":2,"H":216,"KH":3,"KW":3,"N":64,"W":512,"dsts":[[7077888,64,1,0,0,0,0]],"frag":True,"srcs":[[64,64,0]]}),
    ('fwd', 20, 'L', {"B":2,"H":216,"KH":3,"KW":3,"N":64,"W":512,"dsts":[[7077888,64,1,0,0,1,0]],"frag":True,"srcs":[[64,64,0]]}),
    ('fwd', 20, 'B', {"B":2,"H":220,"KH":3,"KW":3,"N":64,"W":512,"dsts":[[7208960,64,1,0,0,0,0]],"frag":True,"srcs":[[64,64,0]]}),
    ('fwd', 20, 'B', {"B":2,"H":220,"KH":3,"KW":3,"N":64,"W":512,"dsts":[[7208960,64,1,0,0,1,0]],"frag":True,"srcs":[[64,64,0]]}),
    ('fwd', 20, 'L', {"B":4,"H":184,"KH":3,"KW":3,"N":64,"W":384,"dsts":[[4521984,64,1,0,0,0,0]],"frag":True,"srcs":[[64,64,0]]}),
    ('fwd', 20, 'L', {"B":4,"H":184,"KH":3,"KW":3,"N":64,"W":384,"dsts":[[4521984,64,1,0,0,1,0]],"frag":True,"srcs":[[64,64,0]]}),
    ('fwd', 20, 'C', {"B":8,"H":184,"KH":3,"KW":3,"N":64,"W":248,"dsts":[[2920448,64,1,0,0,0,0]],"frag":True,"srcs":[[64,64,0]]}),
    ('fwd', 20, 'C', {"B":8,"H":184,"KH":3,"KW":3,"N":64,"W":248,"dsts":[[2920448,64,1,0,0,1,0]],"frag":True,"srcs":[[64,64,0]]}),
    ('fwd', 20, 'AG', {"B":4,"H":220,"KH":3,"KW":3,"N":64,"W":512,"dsts":[[7208960,64,1,0,0,0,0]],"frag":True,"srcs":[[64,64,0]]}),
    ('fwd', 20, 'AG', {"B":4,"H":220,"KH":3,"KW":3,"N":64,"W":512,"dsts":[[7208960,64,1,0,0,1,0]],"frag":True,"srcs":[[64,64,0]]}),
    ('fwd', 20, 'K', {"B":4,"H":188,"KH":3,"KW":3,"N":64,"W":624,"dsts":[[7507968,64,1,0,0,0,0]],"frag":True,"srcs":[[64,64,0]]}),
    ('fwd', 20, 'K', {"B":4,"H":188,"KH":3,"KW":3,"N":64,"W":624,"dsts":[[7507968,64,1,0,0,1,0]],"frag":True,"srcs":[[64,64,0]]}),
    ('fwd', 20, 'C', {"B":16,"H":184,"KH":3,"KW":3,"N":64,"W":248,"dsts":[[2920448,64,1,0,0,0,0]],"frag":True,"srcs":[[64,64,0]]}),
    ('fwd', 20, 'C', {"B":16,"H":184,"KH":3,"KW":3,"N":64,"W":248,"dsts":[[2920448,64,1,0,0,1,0]],"frag":True,"srcs":[[64,64,0]]}),
    ('fwd', 20, 'AG', {"B":8,"H":220,"KH":3,"KW":3,"N":64,"W":512,"dsts":[[7208960,64,1,0,0,0,0]],"frag":True,"srcs":[[64,64,0]]}),
    ('fwd', 20, 'AG', {"B":8,"H":220,"KH":3,"KW":3,"N":64,"W":512,"dsts":[[7208960,64,1,0,0,1,0]],"frag":True,"srcs":[[64,64,0]]}),
    ('fwd', 20, 'K', {"B":8,"H":188,"KH":3,"KW":3,"N":64,"W":624,"dsts":[[7507968,64,1,0,0,0,0]],"frag":True,"srcs":[[64,64,0]]}),
    ('fwd', 20, 'K', {"B":8,"H":188,"KH":3,"KW":3,"N":64,"W":624,"dsts":[[7507968,64,1,0,0,1,0]],"frag":True,"srcs":[[64,64,0]]}),
    ('fwd', 31, 'L', {"B":4,"H":92,"KH":1,"KW":1,"N":64,"W":192,"dsts":[[4521984,256,1,0,0,1,0]],"srcs":[[96,96,0]]}),
    ('fwd', 31, 'C', {"B":8,"H":92,"KH":1,"KW":1,"N":64,"W":124,"dsts":[[2920448,256,1,0,0,1,0]],"srcs":[[96,96,0]]}),
    ('fwd', 31, 'AG', {"B":4,"H":110,"KH":1,"KW":1,"N":64,"W":256,"dsts":[[7208960,256,1,0,0,1,0]],"srcs":[[96,96,0]]}),
    ('fwd', 31, 'K', {"B":4,"H":94,"KH":1,"KW":1,"N":64,"W":312,"dsts":[[7507968,256,1,0,0,1,0]],"srcs":[[96,96,0]]}),
    ('fwd', 31, 'C', {"B":16,"H":92,"KH":1,"KW":1,"N":64,"W":124,"dsts":[[2920448,256,1,0,0,1,0]],"srcs":[[96,96,0]]}),
    ('fwd', 31, 'S', {"B":8,"H":110,"KH":1,"KW":1,"N":64,"W":256,"dsts":[[1802240,64,1,0,0,0,0]],"srcs":[[16,16,0]]}),
    ('fwd', 31, 'S', {"B":8,"H":110,"KH":1,"KW":1,"N":64,"W":256,"dsts":[[1802240,64,1,0,0,1,0]],"srcs":[[16,16,0]]}),
    ('fwd', 31, 'AG', {"B":8,"H":110,"KH":1,"KW":1,"N":64,"W":256,"dsts":[[7208960,256,1,0,0,1,0]],"srcs":[[96,96,0]]}),
    ('fwd', 31, 'K', {"B":8,"H":94,"KH":1,"KW":1,"N":64,"W":312,"dsts":[[7507968,256,1,0,0,1,0]],"srcs":[[96,96,0]]}),
    ('fwd', 32, 'L', {"B":4,"H":46,"KH":1,"KW":1,"N":256,"W":96,"bias":True,"dsts":[[1130496,256,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 32, 'L', {"B":4,"H":46,"KH":2,"KW":2,"N":384,"W":96,"dsts":[[1695744,384,1,0,0,0,0]],"pad":[0,0],"srcs":[[128,128,0]]}),
    ('fwd', 32, 'C', {"B":8,"H":46,"KH":1,"KW":1,"N":256,"W":62,"bias":True,"dsts":[[730112,256,1,0,0,0,0]],"relu":True,"srcs":[[324,324,0]]}),
    ('fwd', 32, 'C', {"B":8,"H":46,"KH":1,"KW":1,"N":256,"W":62,"bias":True,"dsts":[[730112,256,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 32, 'C', {"B":8,"H":46,"KH":1,"KW":5,"N":256,"W":62,"bias":True,"dsts":[[730112,256,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 32, 'C', {"B":8,"H":46,"KH":1,"KW":5,"N":256,"W":62,"dsts":[[365056,128,1,0,0,0,0],[365056,128,1,0,128,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 32, 'C', {"B":8,"H":46,"KH":1,"KW":5,"N":256,"W":62,"dsts":[[365056,128,1,0,0,1,0],[365056,128,1,0,128,1,126]],"srcs":[[256,256,0]]}),
    ('fwd', 32, 'C', {"B":8,"H":46,"KH":1,"KW":5,"N":256,"W":62,"epi":2,"lds":{"aux1":128,"aux2":128,"h":128,"pre":256},"srcs":[[128,128,0],[128,128,0]]}),
    ('fwd', 32, 'C', {"B":8,"H":46,"KH":2,"KW":2,"N":384,"W":62,"dsts":[[1095168,384,1,0,0,0,0]],"pad":[0,0],"srcs":[[128,128,0]]}),
    ('fwd', 32, 'C', {"B":8,"H":46,"KH":5,"KW":1,"N":256,"W":62,"bias":True,"dsts":[[730112,256,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 32, 'C', {"B":8,"H":46,"KH":5,"KW":1,"N":256,"W":62,"dsts":[[365056,128,1,0,0,0,0],[365056,128,1,0,128,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 32, 'C', {"B":8,"H":46,"KH":5,"KW":1,"N":256,"W":62,"dsts":[[365056,128,1,0,0,1,0],[365056,128,1,0,128,1,0]],"srcs":[[256,256,0]]}),
    ('fwd', 32, 'C', {"B":8,"H":46,"KH":5,"KW":1,"N":256,"W":62,"epi":2,"lds":{"aux1":128,"aux2":128,"h":128,"pre":256},"srcs":[[128,128,0],[128,128,0]]}),
    ('fwd', 32, 'B', {"B":1,"H":110,"KH":2,"KW":2,"N":256,"W":256,"dsts":[[7208960,256,1,0,0,0,0]],"pad":[0,0],"srcs":[[96,96,0]]}),
    ('fwd', 32, 'S', {"B":4,"H":55,"KH":1,"KW":1,"N":196,"W":128,"dsts":[[1379840,196,1,0,0,0,0]],"srcs":[[96,128,0]]}),
    ('fwd', 32, 'AG', {"B":4,"H":55,"KH":1,"KW":1,"N":256,"W":128,"bias":True,"dsts":[[1802240,256,1,0,0,0,0]],"relu":True,"srcs":[[324,324,0]]}),
    ('fwd', 32, 'AG', {"B":4,"H":55,"KH":1,"KW":1,"N":256,"W":128,"bias":True,"dsts":[[1802240,256,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 32, 'G', {"B":4,"H":55,"KH":1,"KW":1,"N":256,"W":128,"dsts":[[1802240,256,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 32, 'AG', {"B":4,"H":55,"KH":2,"KW":2,"N":384,"W":128,"dsts":[[2703360,384,1,0,0,0,0]],"pad":[0,0],"srcs":[[128,128,0]]}),
    ('fwd', 32, 'K', {"B":4,"H":47,"KH":1,"KW":1,"N":256,"W":156,"bias":True,"dsts":[[1876992,256,1,0,0,0,0]],"relu":True,"srcs":[[324,324,0]]}),
    ('fwd', 32, 'K', {"B":4,"H":47,"KH":1,"KW":1,"N":256,"W":156,"bias":True,"dsts":[[1876992,256,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 32, 'K', {"B":4,"H":47,"KH":2,"KW":2,"N":384,"W":156,"dsts":[[2815488,384,1,0,0,0,0]],"pad":[0,0],"srcs":[[128,128,0]]}),
    ('fwd', 32, 'L', {"B":2,"H":92,"KH":2,"KW":2,"N":256,"W":192,"dsts":[[4521984,256,1,0,0,0,0]],"pad":[0,0],"srcs":[[96,96,0]]}),
    ('fwd', 32, 'C', {"B":16,"H":46,"KH":1,"KW":1,"N":256,"W":62,"bias":True,"dsts":[[730112,256,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 32, 'C', {"B":16,"H":46,"KH":2,"KW":2,"N":384,"W":62,"dsts":[[1095168,384,1,0,0,0,0]],"pad":[0,0],"srcs":[[128,128,0]]}),
    ('fwd', 32, 'L', {"B":2,"H":108,"KH":2,"KW":2,"N":256,"W":256,"dsts":[[7077888,256,1,0,0,0,0]],"pad":[0,0],"srcs":[[96,96,0]]}),
    ('fwd', 32, 'B', {"B":2,"H":110,"KH":2,"KW":2,"N":256,"W":256,"dsts":[[7208960,256,1,0,0,0,0]],"pad":[0,0],"srcs":[[96,96,0]]}),
    ('fwd', 32, 'AG', {"B":8,"H":55,"KH":1,"KW":1,"N":256,"W":128,"bias":True,"dsts":[[1802240,256,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 32, 'AG', {"B":8,"H":55,"KH":2,"KW":2,"N":384,"W":128,"dsts":[[2703360,384,1,0,0,0,0]],"pad":[0,0],"srcs":[[128,128,0]]}),
    ('fwd', 32, 'K', {"B":8,"H":47,"KH":1,"KW":1,"N":256,"W":156,"bias":True,"dsts":[[1876992,256,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 32, 'K', {"B":8,"H":47,"KH":2,"KW":2,"N":384,"W":156,"dsts":[[2815488,384,1,0,0,0,0]],"pad":[0,0],"srcs":[[128,128,0]]}),
    ('fwd', 32, 'L', {"B":4,"H":92,"KH":2,"KW":2,"N":256,"W":192,"dsts":[[4521984,256,1,0,0,0,0]],"pad":[0,0],"srcs":[[96,96,0]]}),
    ('fwd', 32, 'B', {"B":12,"H":55,"KH":1,"KW":1,"N":256,"W":128,"alpha":0.25,"dsts":[[3604480,512,1,256,0,0,256]],"srcs":[[576,576,0]]}),
    ('fwd', 32, 'B', {"B":12,"H":55,"KH":1,"KW":1,"N":324,"W":128,"dsts":[[2280960,324,1,0,0,0,0]],"srcs":[[256,256,0]]}),
    ('fwd', 32, 'C', {"B":8,"H":92,"KH":2,"KW":2,"N":256,"W":124,"dsts":[[2920448,256,1,0,0,0,0]],"pad":[0,0],"srcs":[[96,96,0]]}),
    ('fwd', 32, 'L', {"B":24,"H":46,"KH":1,"KW":1,"N":256,"W":96,"alpha":0.25,"dsts":[[2260992,512,1,256,0,0,256]],"srcs":[[576,576,0]]}),
    ('fwd', 32, 'L', {"B":24,"H":46,"KH":1,"KW":1,"N":324,"W":96,"dsts":[[1430784,324,1,0,0,0,0]],"srcs":[[256,256,0]]}),
    ('fwd', 32, 'AG', {"B":4,"H":110,"KH":2,"KW":2,"N":256,"W":256,"dsts":[[7208960,256,1,0,0,0,0]],"pad":[0,0],"srcs":[[96,96,0]]}),
    ('fwd', 32, 'K', {"B":4,"H":94,"KH":2,"KW":2,"N":256,"W":312,"dsts":[[7507968,256,1,0,0,0,0]],"pad":[0,0],"srcs":[[96,96,0]]}),
    ('fwd', 32, 'L', {"B":22,"H":54,"KH":1,"KW":1,"N":324,"W":128,"dsts":[[2239488,324,1,0,0,0,0]],"srcs":[[256,256,0]]}),
    ('fwd', 32, 'L', {"B":24,"H":54,"KH":1,"KW":1,"N":256,"W":128,"alpha":0.25,"dsts":[[3538944,512,1,256,0,0,256]],"srcs":[[576,576,0]]}),
    ('fwd', 32, 'C', {"B":16,"H":92,"KH":2,"KW":2,"N":256,"W":124,"dsts":[[2920448,256,1,0,0,0,0]],"pad":[0,0],"srcs":[[96,96,0]]}),
    ('fwd', 32, 'AG', {"B":8,"H":110,"KH":2,"KW":2,"N":256,"W":256,"dsts":[[7208960,256,1,0,0,0,0]],"pad":[0,0],"srcs":[[96,96,0]]}),
    ('fwd', 32, 'K', {"B":8,"H":94,"KH":2,"KW":2,"N":256,"W":312,"dsts":[[7507968,256,1,0,0,0,0]],"pad":[0,0],"srcs":[[96,96,0]]}),
    ('fwd', 32, 'C', {"B":96,"H":46,"KH":1,"KW":1,"N":256,"W":62,"alpha":0.25,"dsts":[[1460224,512,1,256,0,0,256]],"srcs":[[576,576,0]]}),
    ('fwd', 32, 'C', {"B":96,"H":46,"KH":1,"KW":1,"N":324,"W":62,"dsts":[[924048,324,1,0,0,0,0]],"srcs":[[256,256,0]]}),
    ('fwd', 32, 'AG', {"B":48,"H":55,"KH":1,"KW":1,"N":256,"W":128,"alpha":0.25,"dsts":[[3604480,512,1,256,0,0,256]],"srcs":[[576,576,0]]}),
    ('fwd', 32, 'AG', {"B":48,"H":55,"KH":1,"KW":1,"N":324,"W":128,"dsts":[[2280960,324,1,0,0,0,0]],"srcs":[[256,256,0]]}),
    ('fwd', 32, 'K', {"B":48,"H":47,"KH":1,"KW":1,"N":256,"W":156,"alpha":0.25,"dsts":[[3753984,512,1,256,0,0,256]],"srcs":[[576,576,0]]}),
    ('fwd', 32, 'K', {"B":48,"H":47,"KH":1,"KW":1,"N":324,"W":156,"dsts":[[2375568,324,1,0,0,0,0]],"srcs":[[256,256,0]]}),
    ('fwd', 33, 'L', {"B":1,"H":54,"KH":1,"KW":5,"N":256,"W":128,"dsts":[[884736,128,1,0,0,0,0],[884736,128,1,0,128,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'L', {"B":1,"H":54,"KH":1,"KW":5,"N":256,"W":128,"dsts":[[884736,128,1,0,0,1,0],[884736,128,1,0,128,1,126]],"srcs":[[256,256,0]]}),
    ('fwd', 33, 'L', {"B":1,"H":54,"KH":3,"KW":3,"N":256,"W":128,"dsts":[[1769472,256,1,0,0,0,256]],"srcs":[[126,128,0]]}),
    ('fwd', 33, 'L', {"B":1,"H":54,"KH":5,"KW":1,"N":256,"W":128,"dsts":[[884736,128,1,0,0,0,0],[884736,128,1,0,128,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'L', {"B":1,"H":54,"KH":5,"KW":1,"N":256,"W":128,"dsts":[[884736,128,1,0,0,1,0],[884736,128,1,0,128,1,0]],"srcs":[[256,256,0]]}),
    ('fwd', 33, 'B', {"B":1,"H":55,"KH":1,"KW":1,"N":256,"W":128,"bias":True,"dsts":[[1802240,256,1,0,0,0,0]],"relu":True,"srcs":[[324,324,0]]}),
    ('fwd', 33, 'B', {"B":1,"H":55,"KH":1,"KW":1,"N":256,"W":128,"bias":True,"dsts":[[1802240,256,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'B', {"B":1,"H":55,"KH":1,"KW":5,"N":256,"W":128,"bias":True,"dsts":[[1802240,256,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'B', {"B":1,"H":55,"KH":1,"KW":5,"N":256,"W":128,"dsts":[[901120,128,1,0,0,0,0],[901120,128,1,0,128,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'B', {"B":1,"H":55,"KH":1,"KW":5,"N":256,"W":128,"dsts":[[901120,128,1,0,0,1,0],[901120,128,1,0,128,1,126]],"srcs":[[256,256,0]]}),
    ('fwd', 33, 'B', {"B":1,"H":55,"KH":1,"KW":5,"N":256,"W":128,"epi":2,"lds":{"aux1":128,"aux2":128,"h":128,"pre":256},"srcs":[[128,128,0],[128,128,0]]}),
    ('fwd', 33, 'B', {"B":1,"H":55,"KH":2,"KW":2,"N":384,"W":128,"dsts":[[2703360,384,1,0,0,0,0]],"pad":[0,0],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'B', {"B":1,"H":55,"KH":3,"KW":3,"N":512,"W":128,"bias":True,"dsts":[[3604480,512,1,0,0,0,0]],"relu":True,"srcs":[[128,128,0]]}),
    ('fwd', 33, 'B', {"B":1,"H":55,"KH":5,"KW":1,"N":256,"W":128,"bias":True,"dsts":[[1802240,256,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'B', {"B":1,"H":55,"KH":5,"KW":1,"N":256,"W":128,"dsts":[[901120,128,1,0,0,0,0],[901120,128,1,0,128,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'B', {"B":1,"H":55,"KH":5,"KW":1,"N":256,"W":128,"dsts":[[901120,128,1,0,0,1,0],[901120,128,1,0,128,1,0]],"srcs":[[256,256,0]]}),
    ('fwd', 33, 'B', {"B":1,"H":55,"KH":5,"KW":1,"N":256,"W":128,"epi":2,"lds":{"aux1":128,"aux2":128,"h":128,"pre":256},"srcs":[[128,128,0],[128,128,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":46,"KH":1,"KW":1,"N":128,"W":96,"bias":True,"dsts":[[565248,128,1,0,0,0,0]],"relu":True,"srcs":[[98,100,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":46,"KH":1,"KW":1,"N":128,"W":96,"dsts":[[565248,128,1,0,0,0,0]],"srcs":[[256,256,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":46,"KH":1,"KW":1,"N":128,"W":96,"dsts":[[565248,128,1,0,0,0,0]],"srcs":[[96,384,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":46,"KH":1,"KW":1,"N":256,"W":96,"bias":True,"dsts":[[1130496,256,1,0,0,0,0]],"relu":True,"srcs":[[324,324,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":46,"KH":1,"KW":1,"N":256,"W":96,"bias":True,"dsts":[[1130496,256,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":46,"KH":1,"KW":1,"N":96,"W":96,"dsts":[[1695744,384,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":46,"KH":1,"KW":5,"N":128,"W":96,"bias":True,"dsts":[[565248,128,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":46,"KH":1,"KW":5,"N":128,"W":96,"dsts":[[565248,128,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":46,"KH":1,"KW":5,"N":256,"W":96,"bias":True,"dsts":[[1130496,256,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":46,"KH":1,"KW":5,"N":256,"W":96,"dsts":[[565248,128,1,0,0,0,0],[565248,128,1,0,128,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":46,"KH":1,"KW":5,"N":256,"W":96,"dsts":[[565248,128,1,0,0,1,0],[565248,128,1,0,128,1,126]],"srcs":[[256,256,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":46,"KH":1,"KW":5,"N":256,"W":96,"epi":2,"lds":{"aux1":128,"aux2":128,"h":128,"pre":256},"srcs":[[128,128,0],[128,128,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":46,"KH":2,"KW":2,"N":384,"W":96,"dsts":[[1695744,384,1,0,0,0,0]],"pad":[0,0],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":46,"KH":5,"KW":1,"N":128,"W":96,"bias":True,"dsts":[[565248,128,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":46,"KH":5,"KW":1,"N":128,"W":96,"dsts":[[565248,128,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":46,"KH":5,"KW":1,"N":256,"W":96,"bias":True,"dsts":[[1130496,256,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":46,"KH":5,"KW":1,"N":256,"W":96,"dsts":[[565248,128,1,0,0,0,0],[565248,128,1,0,128,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":46,"KH":5,"KW":1,"N":256,"W":96,"dsts":[[565248,128,1,0,0,1,0],[565248,128,1,0,128,1,0]],"srcs":[[256,256,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":46,"KH":5,"KW":1,"N":256,"W":96,"epi":2,"lds":{"aux1":128,"aux2":128,"h":128,"pre":256},"srcs":[[128,128,0],[128,128,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":54,"KH":1,"KW":1,"N":128,"W":128,"bias":True,"dsts":[[884736,128,1,0,0,0,0]],"relu":True,"srcs":[[98,100,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":54,"KH":1,"KW":1,"N":128,"W":128,"dsts":[[884736,128,1,0,0,0,0]],"srcs":[[256,256,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":54,"KH":1,"KW":1,"N":128,"W":128,"dsts":[[884736,128,1,0,0,0,0]],"srcs":[[96,384,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":54,"KH":1,"KW":1,"N":256,"W":128,"bias":True,"dsts":[[1769472,256,1,0,0,0,0]],"relu":True,"srcs":[[324,324,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":54,"KH":1,"KW":1,"N":256,"W":128,"bias":True,"dsts":[[1769472,256,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":54,"KH":1,"KW":1,"N":96,"W":128,"dsts":[[2654208,384,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":54,"KH":1,"KW":5,"N":128,"W":128,"bias":True,"dsts":[[884736,128,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":54,"KH":1,"KW":5,"N":128,"W":128,"dsts":[[884736,128,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":54,"KH":1,"KW":5,"N":256,"W":128,"bias":True,"dsts":[[1769472,256,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":54,"KH":1,"KW":5,"N":256,"W":128,"epi":2,"lds":{"aux1":128,"aux2":128,"h":128,"pre":256},"srcs":[[128,128,0],[128,128,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":54,"KH":2,"KW":2,"N":384,"W":128,"dsts":[[2654208,384,1,0,0,0,0]],"pad":[0,0],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":54,"KH":5,"KW":1,"N":128,"W":128,"bias":True,"dsts":[[884736,128,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":54,"KH":5,"KW":1,"N":128,"W":128,"dsts":[[884736,128,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":54,"KH":5,"KW":1,"N":256,"W":128,"bias":True,"dsts":[[1769472,256,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":54,"KH":5,"KW":1,"N":256,"W":128,"epi":2,"lds":{"aux1":128,"aux2":128,"h":128,"pre":256},"srcs":[[128,128,0],[128,128,0]]}),
    ('fwd', 33, 'B', {"B":2,"H":55,"KH":1,"KW":1,"N":128,"W":128,"dsts":[[901120,128,1,0,0,0,0]],"srcs":[[256,256,0]]}),
    ('fwd', 33, 'B', {"B":2,"H":55,"KH":1,"KW":1,"N":128,"W":128,"dsts":[[901120,128,1,0,0,0,0]],"srcs":[[96,384,0]]}),
    ('fwd', 33, 'B', {"B":2,"H":55,"KH":1,"KW":1,"N":256,"W":128,"bias":True,"dsts":[[1802240,256,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'B', {"B":2,"H":55,"KH":1,"KW":1,"N":96,"W":128,"dsts":[[2703360,384,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'B', {"B":2,"H":55,"KH":2,"KW":2,"N":384,"W":128,"dsts":[[2703360,384,1,0,0,0,0]],"pad":[0,0],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'L', {"B":4,"H":46,"KH":1,"KW":1,"N":128,"W":96,"dsts":[[565248,128,1,0,0,0,0]],"srcs":[[256,256,0]]}),
    ('fwd', 33, 'L', {"B":4,"H":46,"KH":1,"KW":1,"N":128,"W":96,"dsts":[[565248,128,1,0,0,0,0]],"srcs":[[96,384,0]]}),
    ('fwd', 33, 'L', {"B":4,"H":46,"KH":1,"KW":1,"N":96,"W":96,"dsts":[[1695744,384,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'L', {"B":4,"H":46,"KH":2,"KW":2,"N":128,"W":96,"dsts":[[565248,128,1,0,0,0,0]],"srcs":[[384,384,0]]}),
    ('fwd', 33, 'L', {"B":4,"H":46,"KH":3,"KW":3,"N":128,"W":96,"dsts":[[565248,128,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'L', {"B":4,"H":46,"KH":3,"KW":3,"N":128,"W":96,"dsts":[[565248,128,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'C', {"B":8,"H":46,"KH":1,"KW":1,"N":128,"W":62,"bias":True,"dsts":[[365056,128,1,0,0,0,0]],"relu":True,"srcs":[[98,100,0]]}),
    ('fwd', 33, 'C', {"B":8,"H":46,"KH":1,"KW":1,"N":128,"W":62,"dsts":[[365056,128,1,0,0,0,0]],"srcs":[[256,256,0]]}),
    ('fwd', 33, 'C', {"B":8,"H":46,"KH":1,"KW":1,"N":128,"W":62,"dsts":[[365056,128,1,0,0,0,0]],"srcs":[[96,384,0]]}),
    ('fwd', 33, 'C', {"B":8,"H":46,"KH":1,"KW":1,"N":96,"W":62,"dsts":[[1095168,384,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'C', {"B":8,"H":46,"KH":1,"KW":5,"N":128,"W":62,"bias":True,"dsts":[[365056,128,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'C', {"B":8,"H":46,"KH":1,"KW":5,"N":128,"W":62,"dsts":[[365056,128,1,0,0,0,0]],"srcs":[[256,256,0]]}),
    ('fwd', 33, 'C', {"B":8,"H":46,"KH":1,"KW":5,"N":128,"W":62,"dsts":[[365056,128,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'C', {"B":8,"H":46,"KH":1,"KW":5,"N":128,"W":62,"epi":3,"lds":{"aux1":128,"h":128,"pre":128,"z":128},"srcs":[[128,128,0],[128,128,0]]}),
    ('fwd', 33, 'C', {"B":8,"H":46,"KH":2,"KW":2,"N":128,"W":62,"dsts":[[365056,128,1,0,0,0,0]],"srcs":[[384,384,0]]}),
    ('fwd', 33, 'C', {"B":8,"H":46,"KH":3,"KW":3,"N":126,"W":62,"bias":True,"dsts":[[365056,128,1,0,0,0,0]],"relu":True,"srcs":[[256,256,0]]}),
    ('fwd', 33, 'C', {"B":8,"H":46,"KH":3,"KW":3,"N":128,"W":62,"dsts":[[365056,128,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'C', {"B":8,"H":46,"KH":3,"KW":3,"N":128,"W":62,"dsts":[[365056,128,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'C', {"B":8,"H":46,"KH":5,"KW":1,"N":128,"W":62,"bias":True,"dsts":[[365056,128,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'C', {"B":8,"H":46,"KH":5,"KW":1,"N":128,"W":62,"dsts":[[365056,128,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'C', {"B":8,"H":46,"KH":5,"KW":1,"N":128,"W":62,"dsts":[[365056,128,1,0,0,1,0]],"srcs":[[256,256,0]]}),
    ('fwd', 33, 'C', {"B":8,"H":46,"KH":5,"KW":1,"N":128,"W":62,"epi":3,"lds":{"aux1":128,"h":128,"pre":128,"z":128},"srcs":[[128,128,0],[128,128,0]]}),
    ('fwd', 33, 'B', {"B":1,"H":110,"KH":1,"KW":1,"N":64,"W":256,"dsts":[[7208960,256,1,0,0,1,0]],"srcs":[[96,96,0]]}),
    ('fwd', 33, 'B', {"B":1,"H":110,"KH":1,"KW":1,"N":96,"W":256,"dsts":[[2703360,96,1,0,0,0,0]],"srcs":[[64,256,0]]}),
    ('fwd', 33, 'B', {"B":1,"H":110,"KH":2,"KW":2,"N":96,"W":256,"dsts":[[2703360,96,1,0,0,0,0]],"srcs":[[256,256,0]]}),
    ('fwd', 33, 'B', {"B":1,"H":110,"KH":3,"KW":3,"N":96,"W":256,"dsts":[[2703360,96,1,0,0,0,0]],"srcs":[[96,96,0]]}),
    ('fwd', 33, 'B', {"B":1,"H":110,"KH":3,"KW":3,"N":96,"W":256,"dsts":[[2703360,96,1,0,0,1,0]],"srcs":[[96,96,0]]}),
    ('fwd', 33, 'AG', {"B":4,"H":55,"KH":1,"KW":1,"N":128,"W":128,"bias":True,"dsts":[[901120,128,1,0,0,0,0]],"relu":True,"srcs":[[98,100,0]]}),
    ('fwd', 33, 'G', {"B":4,"H":55,"KH":1,"KW":1,"N":128,"W":128,"dsts":[[1802240,256,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'G', {"B":4,"H":55,"KH":1,"KW":1,"N":128,"W":128,"dsts":[[901120,128,1,0,0,0,0]],"srcs":[[128,256,0]]}),
    ('fwd', 33, 'AG', {"B":4,"H":55,"KH":1,"KW":1,"N":128,"W":128,"dsts":[[901120,128,1,0,0,0,0]],"srcs":[[256,256,0]]}),
    ('fwd', 33, 'AG', {"B":4,"H":55,"KH":1,"KW":1,"N":128,"W":128,"dsts":[[901120,128,1,0,0,0,0]],"srcs":[[96,384,0]]}),
    ('fwd', 33, 'S', {"B":4,"H":55,"KH":1,"KW":1,"N":64,"W":128,"bias":True,"dsts":[[450560,64,1,0,0,0,0]],"relu":True,"srcs":[[98,100,0]]}),
    ('fwd', 33, 'S', {"B":4,"H":55,"KH":1,"KW":1,"N":96,"W":128,"bias":True,"dsts":[[901120,128,1,0,0,0,0]],"relu":True,"srcs":[[196,196,0]]}),
    ('fwd', 33, 'AG', {"B":4,"H":55,"KH":1,"KW":1,"N":96,"W":128,"dsts":[[2703360,384,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'AG', {"B":4,"H":55,"KH":1,"KW":5,"N":128,"W":128,"bias":True,"dsts":[[901120,128,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'AG', {"B":4,"H":55,"KH":1,"KW":5,"N":128,"W":128,"dsts":[[901120,128,1,0,0,0,0]],"srcs":[[256,256,0]]}),
    ('fwd', 33, 'AG', {"B":4,"H":55,"KH":1,"KW":5,"N":128,"W":128,"dsts":[[901120,128,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'A', {"B":4,"H":55,"KH":1,"KW":5,"N":128,"W":128,"epi":3,"lds":{"aux1":128,"h":128,"pre":128,"z":128},"srcs":[[128,128,0],[128,128,0]]}),
    ('fwd', 33, 'G', {"B":4,"H":55,"KH":1,"KW":5,"N":128,"W":128,"epi":3,"lds":{"aux1":128,"h":128,"pre":128,"z":128},"srcs":[[128,128,0],[256,256,0]]}),
    ('fwd', 33, 'AG', {"B":4,"H":55,"KH":2,"KW":2,"N":128,"W":128,"dsts":[[901120,128,1,0,0,0,0]],"srcs":[[384,384,0]]}),
    ('fwd', 33, 'G', {"B":4,"H":55,"KH":3,"KW":3,"N":126,"W":128,"bias":True,"dsts":[[1802240,256,1,0,0,0,0]],"relu":True,"srcs":[[256,256,0]]}),
    ('fwd', 33, 'A', {"B":4,"H":55,"KH":3,"KW":3,"N":126,"W":128,"bias":True,"dsts":[[901120,128,1,0,0,0,0]],"relu":True,"srcs":[[256,256,0]]}),
    ('fwd', 33, 'S', {"B":4,"H":55,"KH":3,"KW":3,"N":128,"W":128,"bias":True,"dsts":[[901120,128,1,0,0,0,0]],"relu":True,"srcs":[[96,96,0]]}),
    ('fwd', 33, 'AG', {"B":4,"H":55,"KH":3,"KW":3,"N":128,"W":128,"dsts":[[901120,128,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'S', {"B":4,"H":55,"KH":3,"KW":3,"N":128,"W":128,"dsts":[[901120,128,1,0,0,0,128]],"srcs":[[80,84,0]]}),
    ('fwd', 33, 'AG', {"B":4,"H":55,"KH":3,"KW":3,"N":128,"W":128,"dsts":[[901120,128,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'S', {"B":4,"H":55,"KH":3,"KW":3,"N":80,"W":128,"bias":True,"dsts":[[591360,84,1,0,0,0,0]],"relu":True,"srcs":[[128,128,0]]}),
    ('fwd', 33, 'S', {"B":4,"H":55,"KH":3,"KW":3,"N":96,"W":128,"bias":True,"dsts":[[675840,96,1,0,0,0,0]],"srcs":[[64,64,0]]}),
    ('fwd', 33, 'S', {"B":4,"H":55,"KH":3,"KW":3,"N":96,"W":128,"dsts":[[675840,96,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'S', {"B":4,"H":55,"KH":3,"KW":3,"N":96,"W":128,"epi":3,"lds":{"aux1":96,"h":96,"pre":96,"z":96},"srcs":[[96,96,0],[82,84,0]]}),
    ('fwd', 33, 'AG', {"B":4,"H":55,"KH":5,"KW":1,"N":128,"W":128,"bias":True,"dsts":[[901120,128,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'AG', {"B":4,"H":55,"KH":5,"KW":1,"N":128,"W":128,"dsts":[[901120,128,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'AG', {"B":4,"H":55,"KH":5,"KW":1,"N":128,"W":128,"dsts":[[901120,128,1,0,0,1,0]],"srcs":[[256,256,0]]}),
    ('fwd', 33, 'A', {"B":4,"H":55,"KH":5,"KW":1,"N":128,"W":128,"epi":3,"lds":{"aux1":128,"h":128,"pre":128,"z":128},"srcs":[[128,128,0],[128,128,0]]}),
    ('fwd', 33, 'G', {"B":4,"H":55,"KH":5,"KW":1,"N":128,"W":128,"epi":3,"lds":{"aux1":128,"h":128,"pre":128,"z":128},"srcs":[[128,128,0],[256,256,0]]}),
    ('fwd', 33, 'K', {"B":4,"H":47,"KH":1,"KW":1,"N":128,"W":156,"bias":True,"dsts":[[938496,128,1,0,0,0,0]],"relu":True,"srcs":[[98,100,0]]}),
    ('fwd', 33, 'K', {"B":4,"H":47,"KH":1,"KW":1,"N":128,"W":156,"dsts":[[938496,128,1,0,0,0,0]],"srcs":[[256,256,0]]}),
    ('fwd', 33, 'K', {"B":4,"H":47,"KH":1,"KW":1,"N":128,"W":156,"dsts":[[938496,128,1,0,0,0,0]],"srcs":[[96,384,0]]}),
    ('fwd', 33, 'K', {"B":4,"H":47,"KH":1,"KW":1,"N":96,"W":156,"dsts":[[2815488,384,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'K', {"B":4,"H":47,"KH":1,"KW":5,"N":128,"W":156,"bias":True,"dsts":[[938496,128,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'K', {"B":4,"H":47,"KH":1,"KW":5,"N":128,"W":156,"dsts":[[938496,128,1,0,0,0,0]],"srcs":[[256,256,0]]}),
    ('fwd', 33, 'K', {"B":4,"H":47,"KH":1,"KW":5,"N":128,"W":156,"dsts":[[938496,128,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'K', {"B":4,"H":47,"KH":1,"KW":5,"N":128,"W":156,"epi":3,"lds":{"aux1":128,"h":128,"pre":128,"z":128},"srcs":[[128,128,0],[128,128,0]]}),
    ('fwd', 33, 'K', {"B":4,"H":47,"KH":2,"KW":2,"N":128,"W":156,"dsts":[[938496,128,1,0,0,0,0]],"srcs":[[384,384,0]]}),
    ('fwd', 33, 'K', {"B":4,"H":47,"KH":3,"KW":3,"N":126,"W":156,"bias":True,"dsts":[[938496,128,1,0,0,0,0]],"relu":True,"srcs":[[256,256,0]]}),
    ('fwd', 33, 'K', {"B":4,"H":47,"KH":3,"KW":3,"N":128,"W":156,"dsts":[[938496,128,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'K', {"B":4,"H":47,"KH":3,"KW":3,"N":128,"W":156,"dsts":[[938496,128,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'K', {"B":4,"H":47,"KH":5,"KW":1,"N":128,"W":156,"bias":True,"dsts":[[938496,128,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'K', {"B":4,"H":47,"KH":5,"KW":1,"N":128,"W":156,"dsts":[[938496,128,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'K', {"B":4,"H":47,"KH":5,"KW":1,"N":128,"W":156,"dsts":[[938496,128,1,0,0,1,0]],"srcs":[[256,256,0]]}),
    ('fwd', 33, 'K', {"B":4,"H":47,"KH":5,"KW":1,"N":128,"W":156,"epi":3,"lds":{"aux1":128,"h":128,"pre":128,"z":128},"srcs":[[128,128,0],[128,128,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":92,"KH":1,"KW":1,"N":64,"W":192,"dsts":[[4521984,256,1,0,0,1,0]],"srcs":[[96,96,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":92,"KH":1,"KW":1,"N":96,"W":192,"dsts":[[1695744,96,1,0,0,0,0]],"srcs":[[64,256,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":92,"KH":2,"KW":2,"N":96,"W":192,"dsts":[[1695744,96,1,0,0,0,0]],"srcs":[[256,256,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":92,"KH":3,"KW":3,"N":96,"W":192,"dsts":[[1695744,96,1,0,0,0,0]],"srcs":[[96,96,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":92,"KH":3,"KW":3,"N":96,"W":192,"dsts":[[1695744,96,1,0,0,1,0]],"srcs":[[96,96,0]]}),
    ('fwd', 33, 'C', {"B":16,"H":46,"KH":1,"KW":1,"N":128,"W":62,"dsts":[[365056,128,1,0,0,0,0]],"srcs":[[256,256,0]]}),
    ('fwd', 33, 'C', {"B":16,"H":46,"KH":1,"KW":1,"N":128,"W":62,"dsts":[[365056,128,1,0,0,0,0]],"srcs":[[96,384,0]]}),
    ('fwd', 33, 'C', {"B":16,"H":46,"KH":1,"KW":1,"N":96,"W":62,"dsts":[[1095168,384,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'C', {"B":16,"H":46,"KH":2,"KW":2,"N":128,"W":62,"dsts":[[365056,128,1,0,0,0,0]],"srcs":[[384,384,0]]}),
    ('fwd', 33, 'C', {"B":16,"H":46,"KH":3,"KW":3,"N":128,"W":62,"dsts":[[365056,128,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'C', {"B":16,"H":46,"KH":3,"KW":3,"N":128,"W":62,"dsts":[[365056,128,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":108,"KH":1,"KW":1,"N":64,"W":256,"dsts":[[7077888,256,1,0,0,1,0]],"srcs":[[96,96,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":108,"KH":1,"KW":1,"N":96,"W":256,"dsts":[[2654208,96,1,0,0,0,0]],"srcs":[[64,256,0]]}),
    ('fwd', 33, 'L', {"B":2,"H":108,"KH":2,"KW":2,"N":96,"W":256,"dsts":[[2654208,96,1,0,0,0,0]],"srcs":[[256,256,0]]}),
    ('fwd', 33, 'B', {"B":2,"H":110,"KH":1,"KW":1,"N":64,"W":256,"dsts":[[7208960,256,1,0,0,1,0]],"srcs":[[96,96,0]]}),
    ('fwd', 33, 'B', {"B":2,"H":110,"KH":1,"KW":1,"N":96,"W":256,"dsts":[[2703360,96,1,0,0,0,0]],"srcs":[[64,256,0]]}),
    ('fwd', 33, 'B', {"B":2,"H":110,"KH":2,"KW":2,"N":96,"W":256,"dsts":[[2703360,96,1,0,0,0,0]],"srcs":[[256,256,0]]}),
    ('fwd', 33, 'S', {"B":8,"H":55,"KH":1,"KW":1,"N":128,"W":128,"bias":True,"dsts":[[901120,128,1,0,0,0,0]],"srcs":[[96,96,0]]}),
    ('fwd', 33, 'AG', {"B":8,"H":55,"KH":1,"KW":1,"N":128,"W":128,"dsts":[[901120,128,1,0,0,0,0]],"srcs":[[256,256,0]]}),
    ('fwd', 33, 'AG', {"B":8,"H":55,"KH":1,"KW":1,"N":128,"W":128,"dsts":[[901120,128,1,0,0,0,0]],"srcs":[[96,384,0]]}),
    ('fwd', 33, 'AG', {"B":8,"H":55,"KH":1,"KW":1,"N":96,"W":128,"dsts":[[2703360,384,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'S', {"B":8,"H":55,"KH":1,"KW":1,"N":96,"W":128,"dsts":[[675840,96,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'S', {"B":8,"H":55,"KH":1,"KW":1,"N":96,"W":128,"dsts":[[675840,96,1,0,0,0,0]],"srcs":[[24,24,0]]}),
    ('fwd', 33, 'S', {"B":8,"H":55,"KH":1,"KW":1,"N":96,"W":128,"dsts":[[675840,96,1,0,0,1,0]],"srcs":[[24,24,0]]}),
    ('fwd', 33, 'AG', {"B":8,"H":55,"KH":2,"KW":2,"N":128,"W":128,"dsts":[[901120,128,1,0,0,0,0]],"srcs":[[384,384,0]]}),
    ('fwd', 33, 'K', {"B":8,"H":47,"KH":1,"KW":1,"N":128,"W":156,"dsts":[[938496,128,1,0,0,0,0]],"srcs":[[256,256,0]]}),
    ('fwd', 33, 'K', {"B":8,"H":47,"KH":1,"KW":1,"N":128,"W":156,"dsts":[[938496,128,1,0,0,0,0]],"srcs":[[96,384,0]]}),
    ('fwd', 33, 'K', {"B":8,"H":47,"KH":1,"KW":1,"N":96,"W":156,"dsts":[[2815488,384,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 33, 'K', {"B":8,"H":47,"KH":2,"KW":2,"N":128,"W":156,"dsts":[[938496,128,1,0,0,0,0]],"srcs":[[384,384,0]]}),
    ('fwd', 33, 'L', {"B":4,"H":92,"KH":1,"KW":1,"N":96,"W":192,"dsts":[[1695744,96,1,0,0,0,0]],"srcs":[[64,256,0]]}),
    ('fwd', 33, 'L', {"B":4,"H":92,"KH":2,"KW":2,"N":96,"W":192,"dsts":[[1695744,96,1,0,0,0,0]],"srcs":[[256,256,0]]}),
    ('fwd', 33, 'B', {"B":12,"H":55,"KH":1,"KW":1,"N":576,"W":128,"alpha":0.25,"bias":True,"dsts":[[4055040,576,1,0,0,0,0]],"srcs":[[256,512,256]]}),
    ('fwd', 33, 'C', {"B":8,"H":92,"KH":1,"KW":1,"N":96,"W":124,"dsts":[[1095168,96,1,0,0,0,0]],"srcs":[[64,256,0]]}),
    ('fwd', 33, 'C', {"B":8,"H":92,"KH":2,"KW":2,"N":96,"W":124,"dsts":[[1095168,96,1,0,0,0,0]],"srcs":[[256,256,0]]}),
    ('fwd', 33, 'L', {"B":24,"H":46,"KH":1,"KW":1,"N":576,"W":96,"alpha":0.25,"bias":True,"dsts":[[2543616,576,1,0,0,0,0]],"srcs":[[256,512,256]]}),
    ('fwd', 33, 'AG', {"B":4,"H":110,"KH":1,"KW":1,"N":96,"W":256,"dsts":[[2703360,96,1,0,0,0,0]],"srcs":[[64,256,0]]}),
    ('fwd', 33, 'AG', {"B":4,"H":110,"KH":2,"KW":2,"N":96,"W":256,"dsts":[[2703360,96,1,0,0,0,0]],"srcs":[[256,256,0]]}),
    ('fwd', 33, 'K', {"B":4,"H":94,"KH":1,"KW":1,"N":96,"W":312,"dsts":[[2815488,96,1,0,0,0,0]],"srcs":[[64,256,0]]}),
    ('fwd', 33, 'K', {"B":4,"H":94,"KH":2,"KW":2,"N":96,"W":312,"dsts":[[2815488,96,1,0,0,0,0]],"srcs":[[256,256,0]]}),
    ('fwd', 33, 'L', {"B":24,"H":54,"KH":1,"KW":1,"N":576,"W":128,"alpha":0.25,"bias":True,"dsts":[[3981312,576,1,0,0,0,0]],"srcs":[[256,512,256]]}),
    ('fwd', 33, 'C', {"B":16,"H":92,"KH":1,"KW":1,"N":96,"W":124,"dsts":[[1095168,96,1,0,0,0,0]],"srcs":[[64,256,0]]}),
    ('fwd', 33, 'C', {"B":16,"H":92,"KH":2,"KW":2,"N":96,"W":124,"dsts":[[1095168,96,1,0,0,0,0]],"srcs":[[256,256,0]]}),
    ('fwd', 33, 'AG', {"B":8,"H":110,"KH":1,"KW":1,"N":96,"W":256,"dsts":[[2703360,96,1,0,0,0,0]],"srcs":[[64,256,0]]}),
    ('fwd', 33, 'AG', {"B":8,"H":110,"KH":2,"KW":2,"N":96,"W":256,"dsts":[[2703360,96,1,0,0,0,0]],"srcs":[[256,256,0]]}),
    ('fwd', 33, 'K', {"B":8,"H":94,"KH":1,"KW":1,"N":96,"W":312,"dsts":[[2815488,96,1,0,0,0,0]],"srcs":[[64,256,0]]}),
    ('fwd', 33, 'K', {"B":8,"H":94,"KH":2,"KW":2,"N":96,"W":312,"dsts":[[2815488,96,1,0,0,0,0]],"srcs":[[256,256,0]]}),
    ('fwd', 33, 'C', {"B":96,"H":46,"KH":1,"KW":1,"N":576,"W":62,"alpha":0.25,"bias":True,"dsts":[[1642752,576,1,0,0,0,0]],"srcs":[[256,512,256]]}),
    ('fwd', 33, 'AG', {"B":48,"H":55,"KH":1,"KW":1,"N":576,"W":128,"alpha":0.25,"bias":True,"dsts":[[4055040,576,1,0,0,0,0]],"srcs":[[256,512,256]]}),
    ('fwd', 33, 'K', {"B":48,"H":47,"KH":1,"KW":1,"N":576,"W":156,"alpha":0.25,"bias":True,"dsts":[[4223232,576,1,0,0,0,0]],"srcs":[[256,512,256]]}),
    ('fwd', 34, 'B', {"B":1,"H":55,"KH":1,"KW":1,"N":128,"W":128,"bias":True,"dsts":[[901120,128,1,0,0,0,0]],"relu":True,"srcs":[[98,100,0]]}),
    ('fwd', 34, 'B', {"B":1,"H":55,"KH":1,"KW":1,"N":128,"W":128,"dsts":[[901120,128,1,0,0,0,0]],"srcs":[[256,256,0]]}),
    ('fwd', 34, 'B', {"B":1,"H":55,"KH":1,"KW":1,"N":128,"W":128,"dsts":[[901120,128,1,0,0,0,0]],"srcs":[[96,384,0]]}),
    ('fwd', 34, 'B', {"B":1,"H":55,"KH":1,"KW":1,"N":96,"W":128,"dsts":[[2703360,384,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 133, 'L', {"B":1,"H":54,"KH":3,"KW":3,"N":256,"W":128,"dsts":[[1769472,256,1,0,0,0,256]],"srcs":[[192,256,0]]}),
    ('fwd', 133, 'B', {"B":1,"H":55,"KH":3,"KW":3,"N":192,"W":128,"bias":True,"dsts":[[1802240,256,1,0,0,0,0]],"relu":True,"srcs":[[256,256,0]]}),
    ('fwd', 133, 'L', {"B":2,"H":46,"KH":1,"KW":5,"N":128,"W":96,"dsts":[[565248,128,1,0,0,0,0]],"srcs":[[256,256,0]]}),
    ('fwd', 133, 'L', {"B":2,"H":46,"KH":1,"KW":5,"N":128,"W":96,"epi":3,"lds":{"aux1":128,"h":128,"pre":128,"z":128},"srcs":[[128,128,0],[128,128,0]]}),
    ('fwd', 133, 'L', {"B":2,"H":46,"KH":2,"KW":2,"N":128,"W":96,"dsts":[[565248,128,1,0,0,0,0]],"srcs":[[384,384,0]]}),
    ('fwd', 133, 'L', {"B":2,"H":46,"KH":3,"KW":3,"N":126,"W":96,"bias":True,"dsts":[[565248,128,1,0,0,0,0]],"relu":True,"srcs":[[256,256,0]]}),
    ('fwd', 133, 'L', {"B":2,"H":46,"KH":3,"KW":3,"N":128,"W":96,"dsts":[[565248,128,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 133, 'L', {"B":2,"H":46,"KH":3,"KW":3,"N":128,"W":96,"dsts":[[565248,128,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 133, 'L', {"B":2,"H":46,"KH":5,"KW":1,"N":128,"W":96,"dsts":[[565248,128,1,0,0,1,0]],"srcs":[[256,256,0]]}),
    ('fwd', 133, 'L', {"B":2,"H":46,"KH":5,"KW":1,"N":128,"W":96,"epi":3,"lds":{"aux1":128,"h":128,"pre":128,"z":128},"srcs":[[128,128,0],[128,128,0]]}),
    ('fwd', 133, 'L', {"B":2,"H":54,"KH":1,"KW":5,"N":128,"W":128,"dsts":[[884736,128,1,0,0,0,0]],"srcs":[[256,256,0]]}),
    ('fwd', 133, 'L', {"B":2,"H":54,"KH":1,"KW":5,"N":128,"W":128,"epi":3,"lds":{"aux1":128,"h":128,"pre":128,"z":128},"srcs":[[128,128,0],[128,128,0]]}),
    ('fwd', 133, 'L', {"B":2,"H":54,"KH":2,"KW":2,"N":128,"W":128,"dsts":[[884736,128,1,0,0,0,0]],"srcs":[[384,384,0]]}),
    ('fwd', 133, 'L', {"B":2,"H":54,"KH":3,"KW":3,"N":126,"W":128,"bias":True,"dsts":[[884736,128,1,0,0,0,0]],"relu":True,"srcs":[[256,256,0]]}),
    ('fwd', 133, 'L', {"B":2,"H":54,"KH":3,"KW":3,"N":128,"W":128,"dsts":[[884736,128,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 133, 'L', {"B":2,"H":54,"KH":3,"KW":3,"N":128,"W":128,"dsts":[[884736,128,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 133, 'L', {"B":2,"H":54,"KH":5,"KW":1,"N":128,"W":128,"dsts":[[884736,128,1,0,0,1,0]],"srcs":[[256,256,0]]}),
    ('fwd', 133, 'L', {"B":2,"H":54,"KH":5,"KW":1,"N":128,"W":128,"epi":3,"lds":{"aux1":128,"h":128,"pre":128,"z":128},"srcs":[[128,128,0],[128,128,0]]}),
    ('fwd', 133, 'B', {"B":2,"H":55,"KH":2,"KW":2,"N":128,"W":128,"dsts":[[901120,128,1,0,0,0,0]],"srcs":[[384,384,0]]}),
    ('fwd', 133, 'B', {"B":2,"H":55,"KH":3,"KW":3,"N":128,"W":128,"dsts":[[901120,128,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 133, 'B', {"B":2,"H":55,"KH":3,"KW":3,"N":128,"W":128,"dsts":[[901120,128,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 134, 'L', {"B":1,"H":54,"KH":3,"KW":3,"N":128,"W":128,"dsts":[[884736,128,1,0,0,0,128]],"srcs":[[64,256,192]]}),
    ('fwd', 134, 'B', {"B":1,"H":55,"KH":1,"KW":5,"N":128,"W":128,"bias":True,"dsts":[[901120,128,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 134, 'B', {"B":1,"H":55,"KH":1,"KW":5,"N":128,"W":128,"dsts":[[901120,128,1,0,0,0,0]],"srcs":[[256,256,0]]}),
    ('fwd', 134, 'B', {"B":1,"H":55,"KH":1,"KW":5,"N":128,"W":128,"dsts":[[901120,128,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 134, 'B', {"B":1,"H":55,"KH":1,"KW":5,"N":128,"W":128,"epi":3,"lds":{"aux1":128,"h":128,"pre":128,"z":128},"srcs":[[128,128,0],[128,128,0]]}),
    ('fwd', 134, 'B', {"B":1,"H":55,"KH":2,"KW":2,"N":128,"W":128,"dsts":[[901120,128,1,0,0,0,0]],"srcs":[[384,384,0]]}),
    ('fwd', 134, 'B', {"B":1,"H":55,"KH":3,"KW":3,"N":126,"W":128,"bias":True,"dsts":[[901120,128,1,0,0,0,0]],"relu":True,"srcs":[[256,256,0]]}),
    ('fwd', 134, 'B', {"B":1,"H":55,"KH":3,"KW":3,"N":128,"W":128,"dsts":[[901120,128,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 134, 'B', {"B":1,"H":55,"KH":3,"KW":3,"N":128,"W":128,"dsts":[[901120,128,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 134, 'B', {"B":1,"H":55,"KH":3,"KW":3,"N":64,"W":128,"bias":True,"dsts":[[1802240,256,1,192,0,0,0]],"relu":True,"srcs":[[128,128,0]]}),
    ('fwd', 134, 'B', {"B":1,"H":55,"KH":5,"KW":1,"N":128,"W":128,"bias":True,"dsts":[[901120,128,1,0,0,0,0]],"srcs":[[128,128,0]]}),
    ('fwd', 134, 'B', {"B":1,"H":55,"KH":5,"KW":1,"N":128,"W":128,"dsts":[[901120,128,1,0,0,1,0]],"srcs":[[128,128,0]]}),
    ('fwd', 134, 'B', {"B":1,"H":55,"KH":5,"KW":1,"N":128,"W":128,"dsts":[[901120,128,1,0,0,1,0]],"srcs":[[256,256,0]]}),
    ('fwd', 134, 'B', {"B":1,"H":55,"KH":5,"KW":1,"N":128,"W":128,"epi":3,"lds":{"aux1":128,"h":128,"pre":128,"z":128},"srcs":[[128,128,0],[128,128,0]]}),
    ('wgrad', 1, 'S', {"B":8,"Cout":24,"H":55,"KH":1,"KW":1,"W":128,"bias":False,"ldy":24,"multi":False,"nseg":1,"srcs":[[96,96,0]]}),
    ('wgrad', 1, 'S', {"B":8,"Cout":16,"H":110,"KH":1,"KW":1,"W":256,"bias":False,"ldy":16,"multi":False,"nseg":1,"srcs":[[64,64,0]]}),
    ('wgrad', 1, 'S', {"B":8,"Cout":32,"H":220,"KH":1,"KW":1,"W":512,"bias":False,"ldy":32,"multi":False,"nseg":1,"srcs":[[8,8,0]]}),
    ('wgrad', 1, 'S', {"B":8,"Cout":8,"H":220,"KH":1,"KW":1,"W":512,"bias":False,"ldy":8,"multi":False,"nseg":1,"srcs":[[32,32,0]]}),
    ('wgrad', 5, 'L', {"B":1,"Cout":126,"H":54,"KH":3,"KW":3,"W":128,"bias":True,"ldy":128,"multi":True,"nseg":1,"srcs":[[256,256,0]]}),
    ('wgrad', 5, 'L', {"B":1,"Cout":128,"H":54,"KH":1,"KW":1,"W":128,"bias":True,"ldy":128,"multi":True,"nseg":1,"srcs":[[98,100,0]]}),
    ('wgrad', 5, 'L', {"B":1,"Cout":192,"H":54,"KH":3,"KW":3,"W":128,"bias":True,"ldy":256,"multi":True,"nseg":1,"srcs":[[256,256,0]]}),
    ('wgrad', 5, 'L', {"B":1,"Cout":256,"H":54,"KH":1,"KW":1,"W":128,"bias":True,"ldy":256,"multi":True,"nseg":1,"srcs":[[324,324,0]]}),
    ('wgrad', 5, 'L', {"B":1,"Cout":64,"H":54,"KH":3,"KW":3,"W":128,"bias":True,"ldy":256,"multi":True,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'B', {"B":1,"Cout":128,"H":55,"KH":1,"KW":1,"W":128,"bias":False,"ldy":128,"multi":False,"nseg":1,"srcs":[[96,384,0]]}),
    ('wgrad', 5, 'B', {"B":1,"Cout":128,"H":55,"KH":1,"KW":5,"W":128,"bias":True,"ldy":128,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'B', {"B":1,"Cout":128,"H":55,"KH":2,"KW":2,"W":128,"bias":False,"ldy":128,"multi":False,"nseg":1,"srcs":[[384,384,0]]}),
    ('wgrad', 5, 'B', {"B":1,"Cout":128,"H":55,"KH":3,"KW":3,"W":128,"bias":False,"ldy":128,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'B', {"B":1,"Cout":128,"H":55,"KH":5,"KW":1,"W":128,"bias":True,"ldy":128,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'B', {"B":1,"Cout":256,"H":55,"KH":1,"KW":1,"W":128,"bias":True,"ldy":256,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'B', {"B":1,"Cout":256,"H":55,"KH":1,"KW":5,"W":128,"bias":True,"ldy":256,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'B', {"B":1,"Cout":256,"H":55,"KH":5,"KW":1,"W":128,"bias":True,"ldy":256,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'L', {"B":2,"Cout":128,"H":46,"KH":1,"KW":1,"W":96,"bias":False,"ldy":128,"multi":False,"nseg":1,"srcs":[[96,384,0]]}),
    ('wgrad', 5, 'L', {"B":2,"Cout":128,"H":46,"KH":1,"KW":5,"W":96,"bias":True,"ldy":128,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'L', {"B":2,"Cout":128,"H":46,"KH":2,"KW":2,"W":96,"bias":False,"ldy":128,"multi":False,"nseg":1,"srcs":[[384,384,0]]}),
    ('wgrad', 5, 'L', {"B":2,"Cout":128,"H":46,"KH":5,"KW":1,"W":96,"bias":True,"ldy":128,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'L', {"B":2,"Cout":256,"H":46,"KH":1,"KW":1,"W":96,"bias":True,"ldy":256,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'L', {"B":2,"Cout":256,"H":46,"KH":1,"KW":5,"W":96,"bias":True,"ldy":256,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'L', {"B":2,"Cout":256,"H":46,"KH":5,"KW":1,"W":96,"bias":True,"ldy":256,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'L', {"B":2,"Cout":128,"H":54,"KH":1,"KW":1,"W":128,"bias":False,"ldy":128,"multi":False,"nseg":1,"srcs":[[96,384,0]]}),
    ('wgrad', 5, 'L', {"B":2,"Cout":128,"H":54,"KH":1,"KW":5,"W":128,"bias":True,"ldy":128,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'L', {"B":2,"Cout":128,"H":54,"KH":2,"KW":2,"W":128,"bias":False,"ldy":128,"multi":False,"nseg":1,"srcs":[[384,384,0]]}),
    ('wgrad', 5, 'L', {"B":2,"Cout":128,"H":54,"KH":5,"KW":1,"W":128,"bias":True,"ldy":128,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'L', {"B":2,"Cout":256,"H":54,"KH":1,"KW":1,"W":128,"bias":True,"ldy":256,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'L', {"B":2,"Cout":256,"H":54,"KH":1,"KW":5,"W":128,"bias":True,"ldy":256,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'L', {"B":2,"Cout":256,"H":54,"KH":5,"KW":1,"W":128,"bias":True,"ldy":256,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'B', {"B":2,"Cout":128,"H":55,"KH":1,"KW":1,"W":128,"bias":False,"ldy":128,"multi":False,"nseg":1,"srcs":[[96,384,0]]}),
    ('wgrad', 5, 'B', {"B":2,"Cout":128,"H":55,"KH":2,"KW":2,"W":128,"bias":False,"ldy":128,"multi":False,"nseg":1,"srcs":[[384,384,0]]}),
    ('wgrad', 5, 'B', {"B":2,"Cout":256,"H":55,"KH":1,"KW":1,"W":128,"bias":True,"ldy":256,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'L', {"B":4,"Cout":128,"H":46,"KH":1,"KW":1,"W":96,"bias":False,"ldy":128,"multi":False,"nseg":1,"srcs":[[96,384,0]]}),
    ('wgrad', 5, 'L', {"B":4,"Cout":128,"H":46,"KH":2,"KW":2,"W":96,"bias":False,"ldy":128,"multi":False,"nseg":1,"srcs":[[384,384,0]]}),
    ('wgrad', 5, 'L', {"B":4,"Cout":256,"H":46,"KH":1,"KW":1,"W":96,"bias":True,"ldy":256,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'C', {"B":8,"Cout":128,"H":46,"KH":1,"KW":1,"W":62,"bias":False,"ldy":128,"multi":False,"nseg":1,"srcs":[[96,384,0]]}),
    ('wgrad', 5, 'C', {"B":8,"Cout":128,"H":46,"KH":1,"KW":5,"W":62,"bias":True,"ldy":128,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'C', {"B":8,"Cout":128,"H":46,"KH":2,"KW":2,"W":62,"bias":False,"ldy":128,"multi":False,"nseg":1,"srcs":[[384,384,0]]}),
    ('wgrad', 5, 'C', {"B":8,"Cout":128,"H":46,"KH":5,"KW":1,"W":62,"bias":True,"ldy":128,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'C', {"B":8,"Cout":256,"H":46,"KH":1,"KW":1,"W":62,"bias":True,"ldy":256,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'C', {"B":8,"Cout":256,"H":46,"KH":1,"KW":5,"W":62,"bias":True,"ldy":256,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'C', {"B":8,"Cout":256,"H":46,"KH":5,"KW":1,"W":62,"bias":True,"ldy":256,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'B', {"B":1,"Cout":96,"H":110,"KH":1,"KW":1,"W":256,"bias":False,"ldy":96,"multi":False,"nseg":1,"srcs":[[64,256,0]]}),
    ('wgrad', 5, 'B', {"B":1,"Cout":96,"H":110,"KH":2,"KW":2,"W":256,"bias":False,"ldy":96,"multi":False,"nseg":1,"srcs":[[256,256,0]]}),
    ('wgrad', 5, 'AG', {"B":4,"Cout":128,"H":55,"KH":1,"KW":1,"W":128,"bias":False,"ldy":128,"multi":False,"nseg":1,"srcs":[[96,384,0]]}),
    ('wgrad', 5, 'AG', {"B":4,"Cout":128,"H":55,"KH":1,"KW":5,"W":128,"bias":True,"ldy":128,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'AG', {"B":4,"Cout":128,"H":55,"KH":2,"KW":2,"W":128,"bias":False,"ldy":128,"multi":False,"nseg":1,"srcs":[[384,384,0]]}),
    ('wgrad', 5, 'AG', {"B":4,"Cout":128,"H":55,"KH":5,"KW":1,"W":128,"bias":True,"ldy":128,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'G', {"B":4,"Cout":256,"H":55,"KH":1,"KW":1,"W":128,"bias":False,"ldy":256,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'AG', {"B":4,"Cout":256,"H":55,"KH":1,"KW":1,"W":128,"bias":True,"ldy":256,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'AG', {"B":4,"Cout":256,"H":55,"KH":1,"KW":5,"W":128,"bias":True,"ldy":256,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'AG', {"B":4,"Cout":256,"H":55,"KH":5,"KW":1,"W":128,"bias":True,"ldy":256,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'K', {"B":4,"Cout":128,"H":47,"KH":1,"KW":1,"W":156,"bias":False,"ldy":128,"multi":False,"nseg":1,"srcs":[[96,384,0]]}),
    ('wgrad', 5, 'K', {"B":4,"Cout":128,"H":47,"KH":1,"KW":5,"W":156,"bias":True,"ldy":128,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'K', {"B":4,"Cout":128,"H":47,"KH":2,"KW":2,"W":156,"bias":False,"ldy":128,"multi":False,"nseg":1,"srcs":[[384,384,0]]}),
    ('wgrad', 5, 'K', {"B":4,"Cout":128,"H":47,"KH":5,"KW":1,"W":156,"bias":True,"ldy":128,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'K', {"B":4,"Cout":256,"H":47,"KH":1,"KW":1,"W":156,"bias":True,"ldy":256,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'K', {"B":4,"Cout":256,"H":47,"KH":1,"KW":5,"W":156,"bias":True,"ldy":256,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'K', {"B":4,"Cout":256,"H":47,"KH":5,"KW":1,"W":156,"bias":True,"ldy":256,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'L', {"B":2,"Cout":96,"H":92,"KH":1,"KW":1,"W":192,"bias":False,"ldy":96,"multi":False,"nseg":1,"srcs":[[64,256,0]]}),
    ('wgrad', 5, 'L', {"B":2,"Cout":96,"H":92,"KH":2,"KW":2,"W":192,"bias":False,"ldy":96,"multi":False,"nseg":1,"srcs":[[256,256,0]]}),
    ('wgrad', 5, 'C', {"B":16,"Cout":128,"H":46,"KH":1,"KW":1,"W":62,"bias":False,"ldy":128,"multi":False,"nseg":1,"srcs":[[96,384,0]]}),
    ('wgrad', 5, 'C', {"B":16,"Cout":128,"H":46,"KH":2,"KW":2,"W":62,"bias":False,"ldy":128,"multi":False,"nseg":1,"srcs":[[384,384,0]]}),
    ('wgrad', 5, 'C', {"B":16,"Cout":256,"H":46,"KH":1,"KW":1,"W":62,"bias":True,"ldy":256,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'L', {"B":2,"Cout":96,"H":108,"KH":1,"KW":1,"W":256,"bias":False,"ldy":96,"multi":False,"nseg":1,"srcs":[[64,256,0]]}),
    ('wgrad', 5, 'L', {"B":2,"Cout":96,"H":108,"KH":2,"KW":2,"W":256,"bias":False,"ldy":96,"multi":False,"nseg":1,"srcs":[[256,256,0]]}),
    ('wgrad', 5, 'B', {"B":2,"Cout":96,"H":110,"KH":1,"KW":1,"W":256,"bias":False,"ldy":96,"multi":False,"nseg":1,"srcs":[[64,256,0]]}),
    ('wgrad', 5, 'B', {"B":2,"Cout":96,"H":110,"KH":2,"KW":2,"W":256,"bias":False,"ldy":96,"multi":False,"nseg":1,"srcs":[[256,256,0]]}),
    ('wgrad', 5, 'AG', {"B":8,"Cout":128,"H":55,"KH":1,"KW":1,"W":128,"bias":False,"ldy":128,"multi":False,"nseg":1,"srcs":[[96,384,0]]}),
    ('wgrad', 5, 'S', {"B":8,"Cout":128,"H":55,"KH":1,"KW":1,"W":128,"bias":True,"ldy":128,"multi":False,"nseg":1,"srcs":[[96,96,0]]}),
    ('wgrad', 5, 'AG', {"B":8,"Cout":128,"H":55,"KH":2,"KW":2,"W":128,"bias":False,"ldy":128,"multi":False,"nseg":1,"srcs":[[384,384,0]]}),
    ('wgrad', 5, 'AG', {"B":8,"Cout":256,"H":55,"KH":1,"KW":1,"W":128,"bias":True,"ldy":256,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'S', {"B":8,"Cout":96,"H":55,"KH":1,"KW":1,"W":128,"bias":False,"ldy":96,"multi":False,"nseg":1,"srcs":[[24,24,0]]}),
    ('wgrad', 5, 'K', {"B":8,"Cout":128,"H":47,"KH":1,"KW":1,"W":156,"bias":False,"ldy":128,"multi":False,"nseg":1,"srcs":[[96,384,0]]}),
    ('wgrad', 5, 'K', {"B":8,"Cout":128,"H":47,"KH":2,"KW":2,"W":156,"bias":False,"ldy":128,"multi":False,"nseg":1,"srcs":[[384,384,0]]}),
    ('wgrad', 5, 'K', {"B":8,"Cout":256,"H":47,"KH":1,"KW":1,"W":156,"bias":True,"ldy":256,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 5, 'L', {"B":4,"Cout":96,"H":92,"KH":1,"KW":1,"W":192,"bias":False,"ldy":96,"multi":False,"nseg":1,"srcs":[[64,256,0]]}),
    ('wgrad', 5, 'L', {"B":4,"Cout":96,"H":92,"KH":2,"KW":2,"W":192,"bias":False,"ldy":96,"multi":False,"nseg":1,"srcs":[[256,256,0]]}),
    ('wgrad', 5, 'B', {"B":12,"Cout":128,"H":55,"KH":1,"KW":1,"W":128,"bias":True,"ldy":128,"multi":True,"nseg":1,"srcs":[[98,100,0]]}),
    ('wgrad', 5, 'B', {"B":12,"Cout":256,"H":55,"KH":1,"KW":1,"W":128,"bias":True,"ldy":256,"multi":True,"nseg":1,"srcs":[[324,324,0]]}),
    ('wgrad', 5, 'B', {"B":12,"Cout":576,"H":55,"KH":1,"KW":1,"W":128,"bias":True,"ldy":576,"multi":True,"nseg":1,"srcs":[[256,512,256]]}),
    ('wgrad', 5, 'C', {"B":8,"Cout":96,"H":92,"KH":1,"KW":1,"W":124,"bias":False,"ldy":96,"multi":False,"nseg":1,"srcs":[[64,256,0]]}),
    ('wgrad', 5, 'C', {"B":8,"Cout":96,"H":92,"KH":2,"KW":2,"W":124,"bias":False,"ldy":96,"multi":False,"nseg":1,"srcs":[[256,256,0]]}),
    ('wgrad', 5, 'L', {"B":24,"Cout":128,"H":46,"KH":1,"KW":1,"W":96,"bias":True,"ldy":128,"multi":True,"nseg":1,"srcs":[[98,100,0]]}),
    ('wgrad', 5, 'L', {"B":24,"Cout":256,"H":46,"KH":1,"KW":1,"W":96,"bias":True,"ldy":256,"multi":True,"nseg":1,"srcs":[[324,324,0]]}),
    ('wgrad', 5, 'L', {"B":24,"Cout":576,"H":46,"KH":1,"KW":1,"W":96,"bias":True,"ldy":576,"multi":True,"nseg":1,"srcs":[[256,512,256]]}),
    ('wgrad', 5, 'AG', {"B":4,"Cout":96,"H":110,"KH":1,"KW":1,"W":256,"bias":False,"ldy":96,"multi":False,"nseg":1,"srcs":[[64,256,0]]}),
    ('wgrad', 5, 'AG', {"B":4,"Cout":96,"H":110,"KH":2,"KW":2,"W":256,"bias":False,"ldy":96,"multi":False,"nseg":1,"srcs":[[256,256,0]]}),
    ('wgrad', 5, 'K', {"B":4,"Cout":96,"H":94,"KH":1,"KW":1,"W":312,"bias":False,"ldy":96,"multi":False,"nseg":1,"srcs":[[64,256,0]]}),
    ('wgrad', 5, 'K', {"B":4,"Cout":96,"H":94,"KH":2,"KW":2,"W":312,"bias":False,"ldy":96,"multi":False,"nseg":1,"srcs":[[256,256,0]]}),
    ('wgrad', 5, 'L', {"B":22,"Cout":128,"H":54,"KH":1,"KW":1,"W":128,"bias":True,"ldy":128,"multi":True,"nseg":1,"srcs":[[98,100,0]]}),
    ('wgrad', 5, 'L', {"B":22,"Cout":256,"H":54,"KH":1,"KW":1,"W":128,"bias":True,"ldy":256,"multi":True,"nseg":1,"srcs":[[324,324,0]]}),
    ('wgrad', 5, 'L', {"B":24,"Cout":576,"H":54,"KH":1,"KW":1,"W":128,"bias":True,"ldy":576,"multi":True,"nseg":1,"srcs":[[256,512,256]]}),
    ('wgrad', 5, 'C', {"B":16,"Cout":96,"H":92,"KH":1,"KW":1,"W":124,"bias":False,"ldy":96,"multi":False,"nseg":1,"srcs":[[64,256,0]]}),
    ('wgrad', 5, 'C', {"B":16,"Cout":96,"H":92,"KH":2,"KW":2,"W":124,"bias":False,"ldy":96,"multi":False,"nseg":1,"srcs":[[256,256,0]]}),
    ('wgrad', 5, 'S', {"B":8,"Cout":64,"H":110,"KH":1,"KW":1,"W":256,"bias":False,"ldy":64,"multi":False,"nseg":1,"srcs":[[16,16,0]]}),
    ('wgrad', 5, 'AG', {"B":8,"Cout":96,"H":110,"KH":1,"KW":1,"W":256,"bias":False,"ldy":96,"multi":False,"nseg":1,"srcs":[[64,256,0]]}),
    ('wgrad', 5, 'AG', {"B":8,"Cout":96,"H":110,"KH":2,"KW":2,"W":256,"bias":False,"ldy":96,"multi":False,"nseg":1,"srcs":[[256,256,0]]}),
    ('wgrad', 5, 'K', {"B":8,"Cout":96,"H":94,"KH":1,"KW":1,"W":312,"bias":False,"ldy":96,"multi":False,"nseg":1,"srcs":[[64,256,0]]}),
    ('wgrad', 5, 'K', {"B":8,"Cout":96,"H":94,"KH":2,"KW":2,"W":312,"bias":False,"ldy":96,"multi":False,"nseg":1,"srcs":[[256,256,0]]}),
    ('wgrad', 5, 'C', {"B":96,"Cout":128,"H":46,"KH":1,"KW":1,"W":62,"bias":True,"ldy":128,"multi":True,"nseg":1,"srcs":[[98,100,0]]}),
    ('wgrad', 5, 'C', {"B":96,"Cout":256,"H":46,"KH":1,"KW":1,"W":62,"bias":True,"ldy":256,"multi":True,"nseg":1,"srcs":[[324,324,0]]}),
    ('wgrad', 5, 'C', {"B":96,"Cout":576,"H":46,"KH":1,"KW":1,"W":62,"bias":True,"ldy":576,"multi":True,"nseg":1,"srcs":[[256,512,256]]}),
    ('wgrad', 5, 'AG', {"B":48,"Cout":128,"H":55,"KH":1,"KW":1,"W":128,"bias":True,"ldy":128,"multi":True,"nseg":1,"srcs":[[98,100,0]]}),
    ('wgrad', 5, 'AG', {"B":48,"Cout":256,"H":55,"KH":1,"KW":1,"W":128,"bias":True,"ldy":256,"multi":True,"nseg":1,"srcs":[[324,324,0]]}),
    ('wgrad', 5, 'AG', {"B":48,"Cout":576,"H":55,"KH":1,"KW":1,"W":128,"bias":True,"ldy":576,"multi":True,"nseg":1,"srcs":[[256,512,256]]}),
    ('wgrad', 5, 'K', {"B":48,"Cout":128,"H":47,"KH":1,"KW":1,"W":156,"bias":True,"ldy":128,"multi":True,"nseg":1,"srcs":[[98,100,0]]}),
    ('wgrad', 5, 'K', {"B":48,"Cout":256,"H":47,"KH":1,"KW":1,"W":156,"bias":True,"ldy":256,"multi":True,"nseg":1,"srcs":[[324,324,0]]}),
    ('wgrad', 5, 'K', {"B":48,"Cout":576,"H":47,"KH":1,"KW":1,"W":156,"bias":True,"ldy":576,"multi":True,"nseg":1,"srcs":[[256,512,256]]}),
    ('wgrad', 6, 'S', {"B":4,"Cout":32,"H":55,"KH":3,"KW":3,"W":128,"bias":True,"ldy":128,"multi":True,"nseg":12,"srcs":[[64,64,0]]}),
    ('wgrad', 6, 'S', {"B":8,"Cout":24,"H":55,"KH":3,"KW":3,"W":128,"bias":False,"ldy":24,"multi":False,"nseg":1,"srcs":[[24,24,0]]}),
    ('wgrad', 6, 'S', {"B":8,"Cout":16,"H":110,"KH":3,"KW":3,"W":256,"bias":False,"ldy":16,"multi":False,"nseg":1,"srcs":[[16,16,0]]}),
    ('wgrad', 6, 'S', {"B":8,"Cout":8,"H":220,"KH":3,"KW":3,"W":512,"bias":False,"ldy":8,"multi":False,"nseg":1,"srcs":[[8,8,0]]}),
    ('wgrad', 7, 'L', {"B":2,"Cout":128,"H":46,"KH":3,"KW":3,"W":96,"bias":False,"ldy":128,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 7, 'L', {"B":2,"Cout":128,"H":54,"KH":3,"KW":3,"W":128,"bias":False,"ldy":128,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 7, 'B', {"B":2,"Cout":128,"H":55,"KH":3,"KW":3,"W":128,"bias":False,"ldy":128,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 7, 'L', {"B":4,"Cout":128,"H":46,"KH":3,"KW":3,"W":96,"bias":False,"ldy":128,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 7, 'C', {"B":8,"Cout":128,"H":46,"KH":3,"KW":3,"W":62,"bias":False,"ldy":128,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 7, 'B', {"B":1,"Cout":96,"H":110,"KH":3,"KW":3,"W":256,"bias":False,"ldy":96,"multi":False,"nseg":1,"srcs":[[96,96,0]]}),
    ('wgrad', 7, 'AG', {"B":4,"Cout":128,"H":55,"KH":3,"KW":3,"W":128,"bias":False,"ldy":128,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 7, 'S', {"B":4,"Cout":128,"H":55,"KH":3,"KW":3,"W":128,"bias":True,"ldy":128,"multi":True,"nseg":12,"srcs":[[96,96,0]]}),
    ('wgrad', 7, 'S', {"B":4,"Cout":192,"H":55,"KH":3,"KW":3,"W":128,"bias":False,"ldy":192,"multi":True,"nseg":12,"srcs":[[96,96,0],[82,84,0]]}),
    ('wgrad', 7, 'S', {"B":4,"Cout":192,"H":55,"KH":3,"KW":3,"W":128,"bias":True,"ldy":192,"multi":False,"nseg":1,"srcs":[[64,64,0]]}),
    ('wgrad', 7, 'S', {"B":4,"Cout":80,"H":55,"KH":3,"KW":3,"W":128,"bias":True,"ldy":84,"multi":True,"nseg":12,"srcs":[[128,128,0]]}),
    ('wgrad', 7, 'S', {"B":4,"Cout":96,"H":55,"KH":3,"KW":3,"W":128,"bias":False,"ldy":96,"multi":True,"nseg":12,"srcs":[[96,96,0],[82,84,0]]}),
    ('wgrad', 7, 'S', {"B":4,"Cout":96,"H":55,"KH":3,"KW":3,"W":128,"bias":True,"ldy":96,"multi":False,"nseg":1,"srcs":[[64,64,0]]}),
    ('wgrad', 7, 'K', {"B":4,"Cout":128,"H":47,"KH":3,"KW":3,"W":156,"bias":False,"ldy":128,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 7, 'L', {"B":2,"Cout":96,"H":92,"KH":3,"KW":3,"W":192,"bias":False,"ldy":96,"multi":False,"nseg":1,"srcs":[[96,96,0]]}),
    ('wgrad', 7, 'C', {"B":16,"Cout":128,"H":46,"KH":3,"KW":3,"W":62,"bias":False,"ldy":128,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 7, 'L', {"B":2,"Cout":96,"H":108,"KH":3,"KW":3,"W":256,"bias":False,"ldy":96,"multi":False,"nseg":1,"srcs":[[96,96,0]]}),
    ('wgrad', 7, 'B', {"B":2,"Cout":96,"H":110,"KH":3,"KW":3,"W":256,"bias":False,"ldy":96,"multi":False,"nseg":1,"srcs":[[96,96,0]]}),
    ('wgrad', 7, 'AG', {"B":8,"Cout":128,"H":55,"KH":3,"KW":3,"W":128,"bias":False,"ldy":128,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 7, 'K', {"B":8,"Cout":128,"H":47,"KH":3,"KW":3,"W":156,"bias":False,"ldy":128,"multi":False,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 7, 'L', {"B":4,"Cout":96,"H":92,"KH":3,"KW":3,"W":192,"bias":False,"ldy":96,"multi":False,"nseg":1,"srcs":[[96,96,0]]}),
    ('wgrad', 7, 'B', {"B":12,"Cout":126,"H":55,"KH":3,"KW":3,"W":128,"bias":True,"ldy":128,"multi":True,"nseg":1,"srcs":[[256,256,0]]}),
    ('wgrad', 7, 'B', {"B":12,"Cout":192,"H":55,"KH":3,"KW":3,"W":128,"bias":True,"ldy":256,"multi":True,"nseg":1,"srcs":[[256,256,0]]}),
    ('wgrad', 7, 'B', {"B":12,"Cout":512,"H":55,"KH":3,"KW":3,"W":128,"bias":True,"ldy":512,"multi":True,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 7, 'B', {"B":12,"Cout":64,"H":55,"KH":3,"KW":3,"W":128,"bias":True,"ldy":256,"multi":True,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 7, 'C', {"B":8,"Cout":96,"H":92,"KH":3,"KW":3,"W":124,"bias":False,"ldy":96,"multi":False,"nseg":1,"srcs":[[96,96,0]]}),
    ('wgrad', 7, 'L', {"B":24,"Cout":126,"H":46,"KH":3,"KW":3,"W":96,"bias":True,"ldy":128,"multi":True,"nseg":1,"srcs":[[256,256,0]]}),
    ('wgrad', 7, 'L', {"B":24,"Cout":192,"H":46,"KH":3,"KW":3,"W":96,"bias":True,"ldy":256,"multi":True,"nseg":1,"srcs":[[256,256,0]]}),
    ('wgrad', 7, 'L', {"B":24,"Cout":512,"H":46,"KH":3,"KW":3,"W":96,"bias":True,"ldy":512,"multi":True,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 7, 'L', {"B":24,"Cout":64,"H":46,"KH":3,"KW":3,"W":96,"bias":True,"ldy":256,"multi":True,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 7, 'B', {"B":1,"Cout":64,"H":220,"KH":3,"KW":3,"W":512,"bias":False,"ldy":64,"multi":False,"nseg":1,"srcs":[[64,64,0]]}),
    ('wgrad', 7, 'AG', {"B":4,"Cout":96,"H":110,"KH":3,"KW":3,"W":256,"bias":False,"ldy":96,"multi":False,"nseg":1,"srcs":[[96,96,0]]}),
    ('wgrad', 7, 'K', {"B":4,"Cout":96,"H":94,"KH":3,"KW":3,"W":312,"bias":False,"ldy":96,"multi":False,"nseg":1,"srcs":[[96,96,0]]}),
    ('wgrad', 7, 'L', {"B":2,"Cout":64,"H":184,"KH":3,"KW":3,"W":384,"bias":False,"ldy":64,"multi":False,"nseg":1,"srcs":[[64,64,0]]}),
    ('wgrad', 7, 'L', {"B":22,"Cout":126,"H":54,"KH":3,"KW":3,"W":128,"bias":True,"ldy":128,"multi":True,"nseg":1,"srcs":[[256,256,0]]}),
    ('wgrad', 7, 'L', {"B":22,"Cout":192,"H":54,"KH":3,"KW":3,"W":128,"bias":True,"ldy":256,"multi":True,"nseg":1,"srcs":[[256,256,0]]}),
    ('wgrad', 7, 'L', {"B":22,"Cout":64,"H":54,"KH":3,"KW":3,"W":128,"bias":True,"ldy":256,"multi":True,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 7, 'L', {"B":24,"Cout":512,"H":54,"KH":3,"KW":3,"W":128,"bias":True,"ldy":512,"multi":True,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 7, 'C', {"B":16,"Cout":96,"H":92,"KH":3,"KW":3,"W":124,"bias":False,"ldy":96,"multi":False,"nseg":1,"srcs":[[96,96,0]]}),
    ('wgrad', 7, 'L', {"B":2,"Cout":64,"H":216,"KH":3,"KW":3,"W":512,"bias":False,"ldy":64,"multi":False,"nseg":1,"srcs":[[64,64,0]]}),
    ('wgrad', 7, 'B', {"B":2,"Cout":64,"H":220,"KH":3,"KW":3,"W":512,"bias":False,"ldy":64,"multi":False,"nseg":1,"srcs":[[64,64,0]]}),
    ('wgrad', 7, 'AG', {"B":8,"Cout":96,"H":110,"KH":3,"KW":3,"W":256,"bias":False,"ldy":96,"multi":False,"nseg":1,"srcs":[[96,96,0]]}),
    ('wgrad', 7, 'K', {"B":8,"Cout":96,"H":94,"KH":3,"KW":3,"W":312,"bias":False,"ldy":96,"multi":False,"nseg":1,"srcs":[[96,96,0]]}),
    ('wgrad', 7, 'C', {"B":96,"Cout":126,"H":46,"KH":3,"KW":3,"W":62,"bias":True,"ldy":128,"multi":True,"nseg":1,"srcs":[[256,256,0]]}),
    ('wgrad', 7, 'C', {"B":96,"Cout":192,"H":46,"KH":3,"KW":3,"W":62,"bias":True,"ldy":256,"multi":True,"nseg":1,"srcs":[[256,256,0]]}),
    ('wgrad', 7, 'C', {"B":96,"Cout":512,"H":46,"KH":3,"KW":3,"W":62,"bias":True,"ldy":512,"multi":True,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 7, 'C', {"B":96,"Cout":64,"H":46,"KH":3,"KW":3,"W":62,"bias":True,"ldy":256,"multi":True,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 7, 'L', {"B":4,"Cout":64,"H":184,"KH":3,"KW":3,"W":384,"bias":False,"ldy":64,"multi":False,"nseg":1,"srcs":[[64,64,0]]}),
    ('wgrad', 7, 'A', {"B":48,"Cout":126,"H":55,"KH":3,"KW":3,"W":128,"bias":True,"ldy":128,"multi":True,"nseg":1,"srcs":[[256,256,0]]}),
    ('wgrad', 7, 'G', {"B":48,"Cout":126,"H":55,"KH":3,"KW":3,"W":128,"bias":True,"ldy":256,"multi":True,"nseg":1,"srcs":[[256,256,0]]}),
    ('wgrad', 7, 'AG', {"B":48,"Cout":192,"H":55,"KH":3,"KW":3,"W":128,"bias":True,"ldy":256,"multi":True,"nseg":1,"srcs":[[256,256,0]]}),
    ('wgrad', 7, 'AG', {"B":48,"Cout":512,"H":55,"KH":3,"KW":3,"W":128,"bias":True,"ldy":512,"multi":True,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 7, 'AG', {"B":48,"Cout":64,"H":55,"KH":3,"KW":3,"W":128,"bias":True,"ldy":256,"multi":True,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 7, 'K', {"B":48,"Cout":126,"H":47,"KH":3,"KW":3,"W":156,"bias":True,"ldy":128,"multi":True,"nseg":1,"srcs":[[256,256,0]]}),
    ('wgrad', 7, 'K', {"B":48,"Cout":192,"H":47,"KH":3,"KW":3,"W":156,"bias":True,"ldy":256,"multi":True,"nseg":1,"srcs":[[256,256,0]]}),
    ('wgrad', 7, 'K', {"B":48,"Cout":512,"H":47,"KH":3,"KW":3,"W":156,"bias":True,"ldy":512,"multi":True,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 7, 'K', {"B":48,"Cout":64,"H":47,"KH":3,"KW":3,"W":156,"bias":True,"ldy":256,"multi":True,"nseg":1,"srcs":[[128,128,0]]}),
    ('wgrad', 7, 'C', {"B":8,"Cout":64,"H":184,"KH":3,"KW":3,"W":248,"bias":False,"ldy":64,"multi":False,"nseg":1,"srcs":[[64,64,0]]}),
    ('wgrad', 7, 'AG', {"B":4,"Cout":64,"H":220,"KH":3,"KW":3,"W":512,"bias":False,"ldy":64,"multi":False,"nseg":1,"srcs":[[64,64,0]]}),
    ('wgrad', 7, 'K', {"B":4,"Cout":64,"H":188,"KH":3,"KW":3,"W":624,"bias":False,"ldy":64,"multi":False,"nseg":1,"srcs":[[64,64,0]]}),
    ('wgrad', 7, 'C', {"B":16,"Cout":64,"H":184,"KH":3,"KW":3,"W":248,"bias":False,"ldy":64,"multi":False,"nseg":1,"srcs":[[64,64,0]]}),
    ('wgrad', 7, 'AG', {"B":8,"Cout":64,"H":220,"KH":3,"KW":3,"W":512,"bias":False,"ldy":64,"multi":False,"nseg":1,"srcs":[[64,64,0]]}),
    ('wgrad', 7, 'K', {"B":8,"Cout":64,"H":188,"KH":3,"KW":3,"W":624,"bias":False,"ldy":64,"multi":False,"nseg":1,"srcs":[[64,64,0]]}),
    ('wgrad', 8, 'L', {"B":1,"Cout":128,"H":54,"KH":1,"KW":5,"W":128,"bias":False,"ldy":128,"multi":True,"nseg":12,"srcs":[[128,128,0],[128,128,0]]}),
    ('wgrad', 8, 'L', {"B":1,"Cout":128,"H":54,"KH":5,"KW":1,"W":128,"bias":False,"ldy":128,"multi":True,"nseg":12,"srcs":[[128,128,0],[128,128,0]]}),
    ('wgrad', 8, 'L', {"B":1,"Cout":256,"H":54,"KH":1,"KW":5,"W":128,"bias":False,"ldy":256,"multi":True,"nseg":12,"srcs":[[128,128,0],[128,128,0]]}),
    ('wgrad', 8, 'L', {"B":1,"Cout":256,"H":54,"KH":5,"KW":1,"W":128,"bias":False,"ldy":256,"multi":True,"nseg":12,"srcs":[[128,128,0],[128,128,0]]}),
    ('wgrad', 8, 'B', {"B":1,"Cout":128,"H":55,"KH":1,"KW":5,"W":128,"bias":False,"ldy":128,"multi":True,"nseg":12,"srcs":[[128,128,0],[128,128,0]]}),
    ('wgrad', 8, 'B', {"B":1,"Cout":128,"H":55,"KH":5,"KW":1,"W":128,"bias":False,"ldy":128,"multi":True,"nseg":12,"srcs":[[128,128,0],[128,128,0]]}),
    ('wgrad', 8, 'B', {"B":1,"Cout":256,"H":55,"KH":1,"KW":5,"W":128,"bias":False,"ldy":256,"multi":True,"nseg":12,"srcs":[[128,128,0],[128,128,0]]}),
    ('wgrad', 8, 'B', {"B":1,"Cout":256,"H":55,"KH":5,"KW":1,"W":128,"bias":False,"ldy":256,"multi":True,"nseg":12,"srcs":[[128,128,0],[128,128,0]]}),
    ('wgrad', 8, 'L', {"B":2,"Cout":128,"H":46,"KH":1,"KW":5,"W":96,"bias":False,"ldy":128,"multi":True,"nseg":12,"srcs":[[128,128,0],[128,128,0]]}),
    ('wgrad', 8, 'L', {"B":2,"Cout":128,"H":46,"KH":5,"KW":1,"W":96,"bias":False,"ldy":128,"multi":True,"nseg":12,"srcs":[[128,128,0],[128,128,0]]}),
    ('wgrad', 8, 'L', {"B":2,"Cout":256,"H":46,"KH":1,"KW":5,"W":96,"bias":False,"ldy":256,"multi":True,"nseg":12,"srcs":[[128,128,0],[128,128,0]]}),
    ('wgrad', 8, 'L', {"B":2,"Cout":256,"H":46,"KH":5,"KW":1,"W":96,"bias":False,"ldy":256,"multi":True,"nseg":12,"srcs":[[128,128,0],[128,128,0]]}),
    ('wgrad', 8, 'C', {"B":8,"Cout":128,"H":46,"KH":1,"KW":5,"W":62,"bias":False,"ldy":128,"multi":True,"nseg":12,"srcs":[[128,128,0],[128,128,0]]}),
    ('wgrad', 8, 'C', {"B":8,"Cout":128,"H":46,"KH":5,"KW":1,"W":62,"bias":False,"ldy":128,"multi":True,"nseg":12,"srcs":[[128,128,0],[128,128,0]]}),
    ('wgrad', 8, 'C', {"B":8,"Cout":256,"H":46,"KH":1,"KW":5,"W":62,"bias":False,"ldy":256,"multi":True,"nseg":12,"srcs":[[128,128,0],[128,128,0]]}),
    ('wgrad', 8, 'C', {"B":8,"Cout":256,"H":46,"KH":5,"KW":1,"W":62,"bias":False,"ldy":256,"multi":True,"nseg":12,"srcs":[[128,128,0],[128,128,0]]}),
    ('wgrad', 8, 'G', {"B":4,"Cout":128,"H":55,"KH":1,"KW":1,"W":128,"bias":False,"ldy":128,"multi":True,"nseg":12,"srcs":[[128,256,0]]}),
    ('wgrad', 8, 'A', {"B":4,"Cout":128,"H":55,"KH":1,"KW":5,"W":128,"bias":False,"ldy":128,"multi":True,"nseg":12,"srcs":[[128,128,0],[128,128,0]]}),
    ('wgrad', 8, 'G', {"B":4,"Cout":128,"H":55,"KH":1,"KW":5,"W":128,"bias":False,"ldy":128,"multi":True,"nseg":12,"srcs":[[128,128,0],[256,256,0]]}),
    ('wgrad', 8, 'A', {"B":4,"Cout":128,"H":55,"KH":5,"KW":1,"W":128,"bias":False,"ldy":128,"multi":True,"nseg":12,"srcs":[[128,128,0],[128,128,0]]}),
    ('wgrad', 8, 'G', {"B":4,"Cout":128,"H":55,"KH":5,"KW":1,"W":128,"bias":False,"ldy":128,"multi":True,"nseg":12,"srcs":[[128,128,0],[256,256,0]]}),
    ('wgrad', 8, 'A', {"B":4,"Cout":256,"H":55,"KH":1,"KW":5,"W":128,"bias":False,"ldy":256,"multi":True,"nseg":12,"srcs":[[128,128,0],[128,128,0]]}),
    ('wgrad', 8, 'G', {"B":4,"Cout":256,"H":55,"KH":1,"KW":5,"W":128,"bias":False,"ldy":256,"multi":True,"nseg":12,"srcs":[[128,128,0],[256,256,0]]}),
    ('wgrad', 8, 'A', {"B":4,"Cout":256,"H":55,"KH":5,"KW":1,"W":128,"bias":False,"ldy":256,"multi":True,"nseg":12,"srcs":[[128,128,0],[128,128,0]]}),
    ('wgrad', 8, 'G', {"B":4,"Cout":256,"H":55,"KH":5,"KW":1,"W":128,"bias":False,"ldy":256,"multi":True,"nseg":12,"srcs":[[128,128,0],[256,256,0]]}),
    ('wgrad', 8, 'S', {"B":4,"Cout":64,"H":55,"KH":1,"KW":1,"W":128,"bias":True,"ldy":64,"multi":True,"nseg":12,"srcs":[[98,100,0]]}),
    ('wgrad', 8, 'S', {"B":4,"Cout":96,"H":55,"KH":1,"KW":1,"W":128,"bias":True,"ldy":128,"multi":True,"nseg":12,"srcs":[[196,196,0]]}),
    ('wgrad', 8, 'K', {"B":4,"Cout":128,"H":47,"KH":1,"KW":5,"W":156,"bias":False,"ldy":128,"multi":True,"nseg":12,"srcs":[[128,128,0],[128,128,0]]}),
    ('wgrad', 8, 'K', {"B":4,"Cout":128,"H":47,"KH":5,"KW":1,"W":156,"bias":False,"ldy":128,"multi":True,"nseg":12,"srcs":[[128,128,0],[128,128,0]]}),
    ('wgrad', 8, 'K', {"B":4,"Cout":256,"H":47,"KH":1,"KW":5,"W":156,"bias":False,"ldy":256,"multi":True,"nseg":12,"srcs":[[128,128,0],[128,128,0]]}),
    ('wgrad', 8, 'K', {"B":4,"Cout":256,"H":47,"KH":5,"KW":1,"W":156,"bias":False,"ldy":256,"multi":True,"nseg":12,"srcs":[[128,128,0],[128,128,0]]}),
]


@pytest.mark.parametrize("i", [pytest.param(i, id=_prod_id(i, e[0], e[1], e[3])) for i, e in enumerate(PROD)])
def test_production_call(i, precision, request):
    """One distinct convolution call of a benchmark step (PROD) on synthetic inputs shaped like the layer's."""
    kind, route, _, key = PROD[i]
    case = _prod_case(kind, route, key)
    if kind == "fwd":
        r, *res = run_fwd(case, precision)
        _judge(kind, _case_id(request), r, route, precision, res)
    else:
        r, *res, ok_bias = run_wgrad(case)
        _judge(kind, _case_id(request), r, route, precision, res)
        assert ok_bias, "bias gradient"


def test_every_knob_is_back_at_its_default():
    """Last in the file: whatever the cases above switched (`tuning`, the `precision` fixture) was put back -- every key reads
    its default again, so the tests that run after this file see the library as it loads."""
    lib = _lib().load()
    got = {k: lib.fsraft_get_tuning(k) for k in list(TUNING_DEFAULTS) + [3, 4]}
    assert got == {**TUNING_DEFAULTS, 3: 1, 4: 2}
