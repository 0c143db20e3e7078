"""float64 restatements of the five entry points of csrc/stem.hip and csrc/conv_small.hip -- the encoders' 7x7 stride-2 stem
(forward, weight gradient) and the flow head's 3x3 C -> 2 convolution (forward, weight gradient, data gradient) -- with their case
tables, twins, limits and mutants (tests/test_smallconvref.py on the CPU, tests/test_stem_small_kernels.py against the kernels).
Plain torch on the CPU; nothing here touches a GPU.

Restatements.  Written from the operation through tests/_convref.py (one GEMM reference for the whole suite):
  stem forward      conv_gemm of the channels-last image at the even pixels (b, 2 oy, 2 ox), taps 7 x 7, padding 3
  stem wgrad        wgrad_gemm of dy scattered to the even pixels of a zero [B][H][W][N] tensor, taps 7 x 7
  small forward     conv_gemm, taps 3 x 3, padding 1, + bias
  small wgrad       wgrad_gemm over the segments, laid out through packed_k_index([C], 3, 3); dbias = sum dy
  small dgrad       mask * conv_transpose2d(dy, w, padding = 1), mask = relu_src > 0
ref_* take what the C entry takes (flat buffers, pitches, offsets, sizes) and return the flat positions of the output buffer the
call addresses and what they hold afterwards.  build(op, case) lays every buffer out as the entry will see it: the NaN pattern
0x7FC0FFEE in every float that must not be read (pitch pads, channels outside [coff, coff + C) of a wider source, dy columns >= 2)
and in every output float (the pad columns of dwpk, channels >= C of dx, the gaps of a strided output, all of a plain output);
prior values where the entry accumulates.  expect(p) returns per output buffer an Out.

Comparator.  verdict(got, outs) -> (ok, score, report).  A single changed bit outside an output's positions, a non-finite value
inside, a masked dx element that is not +0.0: score inf.  Otherwise
  stem_fwd, stem_wgrad, small_fwd, small_wgrad   _convref's two criteria unchanged (judge): elementwise against gamma(arith, K) S
      (+ u |prior| where the entry accumulates; the bias enters S as |bias|), Frobenius against the twin (<= 4 x the twin's error
      + u ||ref||, <= 1/16 of the bf16x1 twin's).  arith = bf16x3 for the stem (K = 147, B Ho Wo), fp32 for the small
      convolutions (K = 9 C, nseg B H W).  The score is the largest of the three used shares: <= 1 passes.  dwpk and dbias of one
      call are one GEMM result (dbias: the weight gradient against a constant-one tap) and meet the Frobenius criterion together.
  small_dgrad    need() in units of the elementwise scale u sum |w| |dy| over the 18 products, against LIMITS["dgrad"] =
      limit_from_twin of the worst the fp32 twins reach over the case table (TWIN_WORST; test_smallconvref.py pins it).
The twin judge gets is _convref's own (mode fp32 for the small convolutions, bf16x3 for the stem).  The small convolutions have a
second fp32 twin that sums in the kernel's stated order -- 64 lane partials of fused multiply-adds and a shuffle tree (forward);
per-wave sequential sums, the four waves of a workgroup as (0 + 1) + (2 + 3), then one add per workgroup onto the destination, one
launch per 16 segments (weight gradient) -- which sets no limit: it is one more twin that has to pass the comparator itself
(twins()), i.e. the proof that a correct kernel summing this way fits under 4 x _convref's twin.  Limits come from the CPU, never
from the kernels.
dbias.  Its two sums cannot carry a twin ratio of their own: the Frobenius error of two elements is one or two rounding draws, a
twin's can be exactly zero, and 4 x that would reject a correct kernel by luck.  Concatenated with the 18 C values of dwpk they
have next to no weight in the norm either, so what holds dbias is the elementwise criterion, gamma(fp32, K) S + u |prior| with
S = sum |dy| -- for K = 33 x 9 about 140 u sum |dy|, 1e-5 relative, which a lost or doubled wave sum (mutant) misses by 1e4.

Mutants.  MUTANTS: name -> (op, function of a problem returning {output: corrupted buffer image} or None where the case cannot
show it).  Each scores at least 4 (x its limit) or inf on at least one case.
"""
import functools
from collections import namedtuple
from dataclasses import dataclass

import torch
import torch.nn.functional as F

import _convref as R
from _ewref import INF, PATTERN, Prob, _fma, _rand, _same, ar, pattern  # noqa: F401  (PATTERN, Prob: re-exported)
from _tailref import TINY, U24, limit_from_twin, need  # noqa: F401  (limit_from_twin: re-exported)

STEM_GRID = 512                         # workgroups of both stem kernels = partial matrices of the weight gradient (fsraft_stem_slots)
STEM_SCRATCH = STEM_GRID * 64 * 192
FWD_RUN, FWD_WAVES = 8, 2048 * 4
WG_RUN, WG_WAVES, WG_MAX_SEG = 16, 512 * 4, 16
DG_RUN, DG_WAVES = 16, 4096 * 4


@dataclass
class Out:
    init: torch.Tensor          # the flat fp32 buffer before the call
    idx: torch.Tensor           # flat positions the call addresses
    ref: torch.Tensor           # float64: what they hold afterwards
    bound: object = None        # judged outputs: elementwise gamma S (+ u |prior|)
    twins: object = None        # judged outputs: {"fp32" | "bf16x3" | "bf16x1": float64 values at idx}
    arith: str = ""
    alt: object = None          # every fp32 twin by name: _convref's (the one judge gets) and the kernel-order one
    scale: object = None        # small_dgrad: elementwise scale
    key: str = ""
    zero: object = None         # small_dgrad: bool, the shape of ref -- elements that must be +0.0

    def image(self, values=None):
        """The whole buffer after the call, float64: init with `values` (default ref) at idx."""
        v = self.ref if values is None else values
        img = self.init.double()
        img[self.idx.reshape(-1)] = v.reshape(-1).double()
        return img


def _inside(got, o):
    """The addressed values, or None: a float outside idx changed, a value inside is not finite, a masked element is not +0.0."""
    got = got.reshape(-1)
    assert got.numel() == o.init.numel()
    outside = torch.ones(got.numel(), dtype=torch.bool)
    outside[o.idx.reshape(-1)] = False
    if not bool(_same(got[outside], o.init[outside]).all()):
        return None
    g = got[o.idx.reshape(-1)].reshape(o.ref.shape)
    if not bool(torch.isfinite(g.double()).all()):
        return None
    if o.zero is not None:
        z = g[o.zero]
        if bool(((z != 0) | torch.signbit(z)).any()):
            return None
    return g


def judged(g, ref, bound, twins, arith):
    """_convref.judge and the largest used share of its three criteria (<= 1: passes)."""
    ok, rep = R.judge(g, ref, bound, twins, arith)
    eg = R.frob(g, ref)
    floor = R.U32 * float(ref.norm()) + 1e-30
    e_tw = R.frob(twins["fp32" if arith == "fp32" else "bf16x3"], ref)
    e_b1 = R.frob(twins["bf16x1"], ref)
    rep = dict(rep, frob=eg / (4 * e_tw + floor), b1=eg / (e_b1 / 16 + 1e-300))          # the used shares of judge's two Frobenius criteria
    s = max(rep["elem"], rep["frob"], rep["b1"])
    assert ok == (s <= 1.0), (ok, s, rep)
    return ok, s, rep


def verdict(got, outs):
    """got: {name: flat buffer after the call}; outs: expect(p).  (ok, score, {name: report})."""
    inside = {k: _inside(got[k], o) for k, o in outs.items()}
    if any(v is None for v in inside.values()):
        return False, INF, {}
    names = list(outs)
    o0 = outs[names[0]]
    if o0.twins is not None:                            # one GEMM result, possibly in two buffers
        cat = lambda f: torch.cat([f(k).reshape(-1).double() for k in names])
        tw = {t: cat(lambda k: outs[k].twins[t]) for t in o0.twins}
        ok, s, rep = judged(cat(lambda k: inside[k]), cat(lambda k: outs[k].ref), cat(lambda k: outs[k].bound), tw, o0.arith)
        return ok, s, {"+".join(names): rep}
    assert len(names) == 1 and o0.scale is not None
    w = need(inside[names[0]], o0.ref, o0.scale)[0]
    return w <= LIMITS[o0.key], w / LIMITS[o0.key], {names[0]: dict(units=w)}


def case_id(c):
    return "-".join(str(v) for v in c)


# ============================================================================================================= stem forward
StemFwdCase = namedtuple("StemFwdCase", "B H W N bias")
STEM_SHAPES = ((1, 7, 7), (1, 8, 8), (1, 15, 63), (1, 16, 64), (1, 17, 65), (3, 17, 65), (513, 7, 7), (1030, 7, 7))
STEM_FWD_CASES = [StemFwdCase(*s, N, b) for s in STEM_SHAPES for N in (32, 64) for b in (1, 0)]


def stem_dims(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def stem_fwd_tiles(B, H, W):
    """(tiles, tiles per row, tiles per column): 8 x 32 output pixels each."""
    Ho, Wo = stem_dims(H, W)
    tx, ty = (Wo + 31) // 32, (Ho + 7) // 8
    return B * tx * ty, tx, ty


def stem_rows(B, H, W):
    """Flat indices of the even pixels (b, 2 oy, 2 ox)."""
    Ho, Wo = stem_dims(H, W)
    return ((ar(B)[:, None, None] * H + 2 * ar(Ho)[None, :, None]) * W + 2 * ar(Wo)[None, None, :]).reshape(-1)


def _nhwc(x, B, H, W):
    return x.view(B, 3, H, W).permute(0, 2, 3, 1)


def ref_stem_fwd(x, w, bias, B, H, W, N, mode="fp64"):
    """out[b][oy][ox][n] = bias[n] + sum_{c, ky, kx} w[n][c][ky][kx] x[b][c][2 oy + ky - 3][2 ox + kx - 3], zero outside."""
    G = R.conv_gemm([_nhwc(x, B, H, W)], w.view(N, 3, 7, 7), B, H, W, (3, 3), stem_rows(B, H, W), mode)
    if bias is not None:
        G = G + (bias.double().abs() if mode == "abs" else bias.double())
    return ar(G.numel()), G.reshape(-1)


def _build_stem_fwd(op, c):
    B, H, W, N, bias = c
    Ho, Wo = stem_dims(H, W)
    bufs = dict(x=_rand((B * 3 * H * W,), 101, B, H, W), w=_rand((N * 147,), 102, N, mag=0.1), out=pattern(B * Ho * Wo * N))
    if bias:
        bufs["bias"] = _rand((N,), 103, N, mag=0.5)
    return Prob(op, c, bufs)


def _expect_stem_fwd(p):
    B, H, W, N, _ = p.case
    f = lambda mode: ref_stem_fwd(p.bufs["x"], p.bufs["w"], p.bufs.get("bias"), B, H, W, N, mode)
    idx, ref = f("fp64")
    tw = {m: f(m)[1] for m in ("fp32", "bf16x3", "bf16x1")}
    return dict(out=Out(p.bufs["out"], idx, ref, R.gamma("bf16x3", 147) * f("abs")[1], tw, "bf16x3", dict(fp32=tw["fp32"])))


def _conv64(p, w8=None):
    """F.conv2d restatement in float64, [B][Ho][Wo][N]; w8: an [N][3][7][8] kernel (the padded eighth tap given a weight)."""
    B, H, W, N, _ = p.case
    Ho, Wo = stem_dims(H, W)
    x = p.bufs["x"].double().view(B, 3, H, W)
    w = p.bufs["w"].double().view(N, 3, 7, 7) if w8 is None else w8
    y = F.conv2d(F.pad(x, (3, 5, 3, 3)), w, p.bufs["bias"].double() if "bias" in p.bufs else None, stride=2)[:, :, :Ho, :Wo]
    return y.permute(0, 2, 3, 1).contiguous()


def _m_stem_fwd_eighth_tap(p):
    N = p.case.N
    w = p.bufs["w"].double().view(N, 3, 7, 7)
    w8 = torch.cat([w, w[..., :1]], -1)
    return dict(out=_conv64(p, w8).reshape(-1))


def _m_stem_fwd_stale_patch(p):
    B, H, W, N, _ = p.case
    nt, tx, ty = stem_fwd_tiles(B, H, W)
    if nt <= STEM_GRID or tx * ty != 1:
        return None
    y = _conv64(p)
    y[STEM_GRID:] = y[:B - STEM_GRID].clone()
    return dict(out=y.reshape(-1))


def _m_stem_fwd_no_bias_on_high_half(p):
    if not p.case.bias or p.case.N != 64:
        return None
    y = _conv64(p)
    y[..., 32:] -= p.bufs["bias"].double()[32:]
    return dict(out=y.reshape(-1))


def _m_stem_fwd_last_column(p):
    B, H, W, N, _ = p.case
    Ho, Wo = stem_dims(H, W)
    if Wo % 32 == 0:
        return None
    y = _conv64(p)
    y[:, :, Wo - 1] = float("nan")
    return dict(out=y.reshape(-1))


# ===================================================================================================== stem weight gradient
StemWgradCase = namedtuple("StemWgradCase", "B H W N")
STEM_WGRAD_SLOTS = (4, 5, 12, 13, 16, 17, 60, 61, 64, 65, 77, 511, 512, 513, 1025)          # tiles of the B = 1, W = 7 cases
STEM_WGRAD_CASES = [StemWgradCase(1, 2 * s - 1, 7, 64) for s in STEM_WGRAD_SLOTS] + [StemWgradCase(2, 17, 65, 32), StemWgradCase(3, 9, 131, 64)]


def stem_wgrad_tiles(B, H, W):
    """(tiles, tiles per row): 1 x 32 output pixels each."""
    Ho, Wo = stem_dims(H, W)
    tx = (Wo + 31) // 32
    return B * tx * Ho, tx


def stem_wgrad_slots(B, H, W):
    return min(stem_wgrad_tiles(B, H, W)[0], STEM_GRID)


def stem_wgrad_slot_of_pixel(B, H, W):
    """[B][Ho][Wo]: the partial matrix the output pixel's products go to."""
    Ho, Wo = stem_dims(H, W)
    _, tx = stem_wgrad_tiles(B, H, W)
    tile = (ar(B)[:, None, None] * Ho + ar(Ho)[None, :, None]) * tx + ar(Wo)[None, None, :] // 32
    return tile % STEM_GRID


def reduce_loops(slots):
    """stem_wgrad_reduce_kernel's three loops: the slot indices each takes ({"x16", "x4", "tail"} -> sorted list)."""
    out = dict(x16=[], x4=[], tail=[])
    for pr in range(4):
        i = pr
        while i + 60 < slots:
            out["x16"] += [i + 4 * j for j in range(16)]
            i += 64
        while i + 12 < slots:
            out["x4"] += [i, i + 4, i + 8, i + 12]
            i += 16
        while i < slots:
            out["tail"].append(i)
            i += 4
    return {k: sorted(v) for k, v in out.items()}


def ref_stem_wgrad(x, dy, B, H, W, N, mode="fp64", weight=None):
    """dw[n][c][ky][kx] = sum_{b, oy, ox} dy[b][oy][ox][n] x[b][c][2 oy + ky - 3][2 ox + kx - 3].  weight: [B][Ho][Wo] factors on dy."""
    Ho, Wo = stem_dims(H, W)
    d = dy.view(B, Ho, Wo, N)
    if weight is not None:
        d = d.double() * weight[..., None].double()
    full = torch.zeros(B, H, W, N, dtype=d.dtype)
    full[:, ::2, ::2] = d
    G = R.wgrad_gemm([full], [[_nhwc(x, B, H, W)]], B, H, W, 7, 7, mode)
    return ar(N * 147), G.reshape(-1)


def _build_stem_wgrad(op, c):
    B, H, W, N = c
    Ho, Wo = stem_dims(H, W)
    return Prob(op, c, dict(x=_rand((B * 3 * H * W,), 111, B, H, W), dy=_rand((B * Ho * Wo * N,), 112, B, H, W, N), dw=pattern(N * 147)))


def _expect_stem_wgrad(p):
    B, H, W, N = p.case
    Ho, Wo = stem_dims(H, W)
    f = lambda mode: ref_stem_wgrad(p.bufs["x"], p.bufs["dy"], B, H, W, N, mode)
    idx, ref = f("fp64")
    tw = {m: f(m)[1] for m in ("fp32", "bf16x3", "bf16x1")}
    return dict(dw=Out(p.bufs["dw"], idx, ref, R.gamma("bf16x3", B * Ho * Wo) * f("abs")[1], tw, "bf16x3", dict(fp32=tw["fp32"])))


def _stem_wgrad_weighted(p, slot_weight):
    B, H, W, N = p.case
    wt = slot_weight[stem_wgrad_slot_of_pixel(B, H, W)]
    return dict(dw=ref_stem_wgrad(p.bufs["x"], p.bufs["dy"], B, H, W, N, weight=wt)[1])


def _m_stem_wgrad_last_slot(p):
    s = stem_wgrad_slots(*p.case[:3])
    wt = torch.ones(STEM_GRID)
    wt[s - 1] = 0.0
    return _stem_wgrad_weighted(p, wt)


def _m_stem_wgrad_tail_twice(p):
    tail = reduce_loops(stem_wgrad_slots(*p.case[:3]))["tail"]
    if not tail:
        return None
    wt = torch.ones(STEM_GRID)
    wt[tail] = 2.0
    return _stem_wgrad_weighted(p, wt)


def _m_stem_wgrad_padded_taps(p):
    N = p.case.N
    ref = _expect_stem_wgrad(p)["dw"].ref.view(N, 3, 7, 7)
    pad = torch.zeros(N, 3, 8, 8, dtype=torch.float64)
    pad[:, :, :7, :7] = ref
    return dict(dw=pad.reshape(N, 192)[:, :147].reshape(-1))


# ====================================================================================================== small convolutions
def _wide(rows, C, ld, coff, *key, mag=1.0):
    """[rows][ld]: live values in columns [coff, coff + C), the NaN pattern elsewhere."""
    t = pattern(rows * ld).view(rows, ld)
    t[:, coff:coff + C] = _rand((rows, C), *key, mag=mag)
    return t.reshape(-1)


def _live(buf, B, H, W, C, ld, coff):
    return buf.view(B * H * W, ld)[:, coff:coff + C].reshape(B, H, W, C)


def run_ends(W, run):
    """bool [W]: the pixel is the last of its run."""
    x = ar(W)
    return (x % run == run - 1) | (x == W - 1)


# ------------------------------------------------------------------------------------------------------------- small forward
SmallFwdCase = namedtuple("SmallFwdCase", "B H W C ld coff olay bias")
SMALL_FWD_BIG = SmallFwdCase(3, 43, 512, 4, 4, 0, "planar", 1)
SMALL_FWD_CASES = [SmallFwdCase(*t) for t in (
    (1, 1, 1, 4, 4, 0, "planar", 1), (3, 2, 7, 36, 40, 4, "gap", 0), (1, 3, 8, 252, 504, 252, "inter", 1), (3, 1, 9, 256, 256, 0, "planar", 0),
    (1, 2, 17, 260, 264, 0, "gap", 1), (3, 3, 8, 512, 512, 0, "inter", 0), (1, 3, 9, 512, 516, 4, "planar", 1), (1, 2, 17, 4, 8, 4, "inter", 0),
    (3, 3, 17, 36, 36, 0, "inter", 1), (1, 1, 7, 260, 520, 260, "planar", 0), (3, 2, 1, 256, 260, 4, "gap", 1), (1, 3, 1, 252, 252, 0, "gap", 0),
    (1, 2, 9, 512, 1024, 512, "gap", 1))] + [SMALL_FWD_BIG]


def out_strides(olay, HW):
    """(obs, ocs, ops, floats of the buffer per batch element)."""
    if olay == "planar":
        return 2 * HW, HW, 1
    if olay == "gap":                                   # five floats behind each plane, three more behind each sample
        return 2 * (HW + 5) + 3, HW + 5, 1
    return 2 * HW, 1, 2                                 # interleaved


def ref_small_fwd(x, ld, coff, C, w, bias, B, H, W, obs, ocs, ops, mode="fp64", w4=None, rows=None):
    """out[b obs + o ocs + pix ops] = bias[o] + sum_{c, ky, kx} w[o][c][ky][kx] x[b][y + ky - 1][x + kx - 1][c], zero outside."""
    rows = ar(B * H * W) if rows is None else rows
    w4 = w.view(2, C, 3, 3) if w4 is None else w4
    G = R.conv_gemm([_live(x, B, H, W, C, ld, coff)], w4, B, H, W, (1, 1), rows, mode)
    if bias is not None:
        G = G + (bias.double().abs() if mode == "abs" else bias.double())
    idx = (rows // (H * W))[:, None] * obs + ar(2)[None, :] * ocs + (rows % (H * W))[:, None] * ops
    return idx, G


def _build_small_fwd(op, c):
    B, H, W, C, ld, coff, olay, bias = c
    obs = out_strides(olay, H * W)[0]
    bufs = dict(x=_wide(B * H * W, C, ld, coff, 121, *c[:6]), w=_rand((2 * C * 9,), 122, C, mag=0.1), out=pattern(B * obs + 3))
    if bias:
        bufs["bias"] = _rand((2,), 123, C, mag=0.5)
    return Prob(op, c, bufs)


def twin_small_fwd_lanes(p):
    """fp32 in the kernel's stated order: lane l owns channels 4 l .. 4 l + 3 (+ 256), four running sums of fused multiply-adds
    over (row, register set, column of the window), (s0 + s1) + (s2 + s3), a xor-shuffle tree over the 64 lanes, + bias."""
    B, H, W, C, ld, coff, olay, _ = p.case
    M = B * H * W
    cols = R.columns([_live(p.bufs["x"], B, H, W, C, ld, coff)], B, H, W, 3, 3, (1, 1), ar(M)).view(M, 9, C)
    wt = p.bufs["w"].view(2, C, 9).permute(0, 2, 1)                                # [2][9][C]
    live = min(C, 256)                                  # only the live lanes are carried: the others add exact zeros to the tree
    out = []
    for o in range(2):
        a = torch.zeros(M, live)
        for r in range(3):
            for c0 in range(0, C, 256):                 # the register sets
                n = min(C - c0, 256)
                for kx in range(3):
                    t = 3 * r + kx
                    a[:, :n] = _fma(cols[:, t, c0:c0 + n], wt[o, t, c0:c0 + n].expand(M, n), a[:, :n])
        a = a.view(M, live // 4, 4)
        s = torch.zeros(M, 64)
        s[:, :live // 4] = (a[..., 0] + a[..., 1]) + (a[..., 2] + a[..., 3])
        for sft in (32, 16, 8, 4, 2, 1):
            s = s + s[:, ar(64) ^ sft]
        out.append(s[:, 0] + (p.bufs["bias"][o] if "bias" in p.bufs else 0.0))
    return torch.stack(out, 1).double()


def _expect_small_fwd(p):
    B, H, W, C, ld, coff, olay, _ = p.case
    st = out_strides(olay, H * W)
    f = lambda mode: ref_small_fwd(p.bufs["x"], ld, coff, C, p.bufs["w"], p.bufs.get("bias"), B, H, W, *st, mode)
    idx, ref = f("fp64")
    alt = {"torch fp32": f("fp32")[1], "lanes and tree": twin_small_fwd_lanes(p)}
    tw = dict(fp32=alt["torch fp32"], bf16x1=f("bf16x1")[1])
    return dict(out=Out(p.bufs["out"], idx, ref, R.gamma("fp32", 9 * C) * f("abs")[1], tw, "fp32", alt))


def _small_fwd_with(p, w4=None, w4_rows=None):
    """The restatement with other weights everywhere (w4) or at some pixels (w4_rows: (w4, bool [B H W]))."""
    B, H, W, C, ld, coff, olay, _ = p.case
    st = out_strides(olay, H * W)
    a = (p.bufs["x"], ld, coff, C, p.bufs["w"], p.bufs.get("bias"), B, H, W, *st)
    idx, G = ref_small_fwd(*a, w4=w4)
    if w4_rows is not None:
        rows = w4_rows[1].reshape(-1).nonzero().flatten()
        G[rows] = ref_small_fwd(*a, w4=w4_rows[0], rows=rows)[1]
    return dict(out=Out(p.bufs["out"], idx, G).image())


def _m_small_fwd_run_end(p):
    B, H, W, C = p.case[:4]
    w4 = p.bufs["w"].view(2, C, 3, 3).clone()
    w4[..., 2] = 0.0
    return _small_fwd_with(p, w4_rows=(w4, run_ends(W, FWD_RUN).expand(B, H, W)))


def _m_small_fwd_high_channels(p):
    C = p.case.C
    if C <= 256:
        return None
    w4 = p.bufs["w"].view(2, C, 3, 3).clone()
    w4[:, 256:] = 0.0
    return _small_fwd_with(p, w4=w4)


# ---------------------------------------------------------------------------------------------------- small weight gradient
SmallWgradCase = namedtuple("SmallWgradCase", "B H W C ldx coff nseg ldy prior dbias")
SMALL_WGRAD_BIG = SmallWgradCase(1, 65, 512, 4, 4, 0, 1, 2, 1, 1)
SMALL_WGRAD_CASES = [SmallWgradCase(*t) for t in (
    (1, 1, 1, 4, 4, 0, 1, 2, 0, 1), (3, 2, 8, 36, 40, 4, 2, 4, 1, 1), (1, 3, 9, 252, 504, 252, 16, 7, 1, 0), (1, 2, 16, 256, 256, 0, 17, 2, 0, 1),
    (3, 1, 17, 260, 264, 0, 1, 4, 1, 1), (1, 2, 25, 512, 512, 0, 2, 7, 1, 0), (1, 3, 25, 4, 8, 4, 33, 2, 1, 1), (3, 3, 16, 36, 36, 0, 17, 4, 0, 0),
    (1, 1, 9, 260, 520, 260, 33, 7, 1, 1), (3, 2, 17, 512, 516, 4, 16, 2, 0, 1), (1, 2, 8, 252, 252, 0, 1, 4, 1, 1),
    (1, 1, 1, 256, 260, 4, 2, 7, 1, 0))] + [SMALL_WGRAD_BIG]


def dwpk_index(C):
    """([2][9][C] flat positions of (o, tap, c) in dwpk, Ktot)."""
    kidx, ktot = R.packed_k_index([C], 3, 3)
    return ar(2)[:, None, None] * ktot + kidx[None], ktot


def _segs(p):
    c = p.case
    dys = [p.bufs[f"dy{t}"].view(c.B * c.H * c.W, c.ldy)[:, :2].reshape(c.B, c.H, c.W, 2) for t in range(c.nseg)]
    xs = [_live(p.bufs[f"x{t}"], c.B, c.H, c.W, c.C, c.ldx, c.coff) for t in range(c.nseg)]
    return dys, xs


def ref_small_wgrad(dys, xs, C, B, H, W, mode="fp64"):
    """dw[o][tap][c] = sum over segments and pixels of dy[pix][o] x[pix + shift(tap)][c]  ([2][9][C]);  db[o] = sum dy[pix][o]."""
    G = R.wgrad_gemm(dys, [[x] for x in xs], B, H, W, 3, 3, mode)                  # [2][C][3][3]
    d = torch.stack([t.reshape(-1, 2) for t in dys])
    if mode == "fp32":
        db = sum(t.float().sum(0).double() for t in d)
    elif mode == "bf16x1":
        db = R.bf16_hi_lo(d.double())[0].sum((0, 1))
    else:
        db = (d.double().abs() if mode == "abs" else d.double()).sum((0, 1))
    return G.permute(0, 2, 3, 1).reshape(2, 9, C), db


def _build_small_wgrad(op, c):
    B, H, W, C, ldx, coff, nseg, ldy, prior, dbias = c
    M = B * H * W
    bufs = {}
    for t in range(nseg):
        bufs[f"x{t}"] = _wide(M, C, ldx, coff, 131, *c[:6], t)
        bufs[f"dy{t}"] = _wide(M, 2, ldy, 0, 132, *c[:4], ldy, t, mag=0.5)
    idx, ktot = dwpk_index(C)
    dw = pattern(2 * ktot)
    dw[idx] = _rand((2, 9, C), 133, *c[:4], mag=3.0) if prior else torch.zeros(2, 9, C)
    bufs["dwpk"] = dw
    if dbias:
        db = pattern(6)
        db[:2] = _rand((2,), 134, *c[:4], mag=3.0) if prior else torch.zeros(2)
        bufs["dbias"] = db
    return Prob(op, c, bufs)


def twin_small_wgrad_waves(p):
    """fp32 in the kernel's stated order.  Per launch (16 segments): wave v takes runs v, v + 2048, ... of 16 pixels of an image
    row, of every segment in turn, and adds dy x products (fused) onto its own sums pixel by pixel; a workgroup adds its four
    waves as (0 + 1) + (2 + 3); the workgroups add onto dwpk one after the other (here: in index order), the waves onto dbias."""
    c = p.case
    B, H, W, C = c[:4]
    M = B * H * W
    dys, xs = _segs(p)
    idx, _ = dwpk_index(C)
    dw = p.bufs["dwpk"][idx].clone()
    db = p.bufs["dbias"][:2].clone() if c.dbias else torch.zeros(2)
    rpr = (W + WG_RUN - 1) // WG_RUN
    nrun = B * H * rpr
    nw = min(nrun, WG_WAVES)
    nwp = (nw + 3) // 4 * 4
    for base in range(0, c.nseg, WG_MAX_SEG):
        acc, bs = torch.zeros(nwp, 2, 9, C), torch.zeros(nwp, 2)
        for t in range(base, min(base + WG_MAX_SEG, c.nseg)):
            cols = R.columns([xs[t]], B, H, W, 3, 3, (1, 1), ar(M)).view(M, 9, C)
            g = dys[t].reshape(M, 2)
            for trip in range((nrun + WG_WAVES - 1) // WG_WAVES):
                run = trip * WG_WAVES + ar(nw)
                run = run[run < nrun]
                x0 = (run % rpr) * WG_RUN
                row = run // rpr
                for i in range(WG_RUN):
                    ok = x0 + i < W
                    v, m = ar(run.numel())[ok], (row * W + x0 + i)[ok]
                    bs[v] = bs[v] + g[m]
                    acc[v] = _fma(g[m][:, :, None, None].expand(-1, 2, 9, C), cols[m][:, None].expand(-1, 2, 9, C), acc[v])
        a4 = acc.view(nwp // 4, 4, 2, 9, C)
        blk = (a4[:, 0] + a4[:, 1]) + (a4[:, 2] + a4[:, 3])
        for s in blk:
            dw = dw + s
        for s in bs:
            db = db + s
    return dw.double(), db.double()


def _expect_small_wgrad(p):
    c = p.case
    B, H, W, C = c[:4]
    dys, xs = _segs(p)
    idx, _ = dwpk_index(C)
    f = lambda mode: ref_small_wgrad(dys, xs, C, B, H, W, mode)
    prior = (p.bufs["dwpk"][idx].double(), p.bufs["dbias"][:2].double() if c.dbias else torch.zeros(2, dtype=torch.float64))
    ref = [a + b for a, b in zip(prior, f("fp64"))]
    S = f("abs")
    gam = R.gamma("fp32", c.nseg * B * H * W)
    alt = {"torch fp32": [a + b for a, b in zip(prior, f("fp32"))], "waves then atomics": twin_small_wgrad_waves(p)}
    b1 = [a + b for a, b in zip(prior, f("bf16x1"))]
    outs = {}
    for i, (name, ix) in enumerate((("dwpk", idx), ("dbias", ar(2)))[:2 if c.dbias else 1]):
        outs[name] = Out(p.bufs[name], ix, ref[i], gam * S[i] + U24 * prior[i].abs(), dict(fp32=alt["torch fp32"][i], bf16x1=b1[i]), "fp32",
                         {k: v[i] for k, v in alt.items()})
    return outs


def _small_wgrad_image(p, dw=None, at=None, db=None):
    """{dwpk, dbias} images: prior + dw (a [2][9][C] sum) at flat positions `at` (default the packed ones), dbias prior + db."""
    c = p.case
    idx, _ = dwpk_index(c.C)
    dys, xs = _segs(p)
    full = ref_small_wgrad(dys, xs, c.C, c.B, c.H, c.W)
    dw = full[0] if dw is None else dw
    img = p.bufs["dwpk"].double()
    img[(idx if at is None else at).reshape(-1)] += dw.reshape(-1)
    out = dict(dwpk=img)
    if c.dbias:
        b = p.bufs["dbias"].double()
        b[:2] += full[1] if db is None else db
        out["dbias"] = b
    return out


def _m_small_wgrad_run_end(p):
    c = p.case
    dys, xs = _segs(p)
    ends = run_ends(c.W, WG_RUN)[None, None, :, None]
    lost = ref_small_wgrad([d.double() * ends for d in dys], xs, c.C, c.B, c.H, c.W)[0].clone()
    lost.view(2, 3, 3, c.C)[:, :, :2] = 0.0                                       # only the right-hand column (kx = 2) is lost
    if not bool((lost != 0).any()):
        return None
    full = ref_small_wgrad(dys, xs, c.C, c.B, c.H, c.W)[0]
    return _small_wgrad_image(p, dw=full - lost)


def _m_small_wgrad_high_channels(p):
    c = p.case
    if c.C <= 256:
        return None
    dys, xs = _segs(p)
    dw = ref_small_wgrad(dys, xs, c.C, c.B, c.H, c.W)[0].clone()
    dw[:, :, 256:] = 0.0
    return _small_wgrad_image(p, dw=dw)


def _m_small_wgrad_segment_16(p):
    c = p.case
    if c.nseg < 17:
        return None
    dys, xs = _segs(p)
    keep = [t for t in range(c.nseg) if t != 16]
    dw, db = ref_small_wgrad([dys[t] for t in keep], [xs[t] for t in keep], c.C, c.B, c.H, c.W)
    return _small_wgrad_image(p, dw=dw, db=db)


def _m_small_wgrad_dbias_first_wave_only(p):
    """Only the first wave of each workgroup adds its bias sum: dbias holds the pixels of runs 0, 4, 8, ... (mod 2048) alone; dwpk
    is right."""
    c = p.case
    rpr = (c.W + WG_RUN - 1) // WG_RUN
    if not c.dbias or c.B * c.H * rpr < 2:
        return None
    run = (ar(c.B * c.H)[:, None] * rpr + ar(c.W)[None, :] // WG_RUN).view(c.B, c.H, c.W)
    keep = (run % WG_WAVES) % 4 == 0
    dys, _ = _segs(p)
    return _small_wgrad_image(p, db=sum((d.double() * keep[..., None]).sum((0, 1, 2)) for d in dys))


def _m_small_wgrad_tap_pitch(p):
    c = p.case
    if c.C % 32 == 0:
        return None
    _, ktot = dwpk_index(c.C)
    at = ar(2)[:, None, None] * ktot + ar(9)[None, :, None] * c.C + ar(c.C)[None, None, :]
    return _small_wgrad_image(p, at=at)


# ------------------------------------------------------------------------------------------------------ small data gradient
SmallDgradCase = namedtuple("SmallDgradCase", "B H W C lddx ldy ldm")                     # ldm 0: no mask
SMALL_DGRAD_BIG = SmallDgradCase(1, 129, 2048, 4, 4, 2, 4)
SMALL_DGRAD_CASES = [SmallDgradCase(*t) for t in (
    (1, 1, 1, 4, 4, 2, 4), (3, 2, 15, 36, 40, 4, 0), (1, 3, 16, 252, 512, 5, 256), (3, 1, 17, 256, 256, 2, 256), (1, 2, 33, 256, 260, 5, 0),
    (1, 3, 33, 4, 8, 4, 8), (3, 3, 15, 252, 252, 2, 0), (1, 2, 16, 36, 512, 5, 36), (3, 1, 1, 256, 512, 4, 260), (1, 3, 17, 4, 512, 2, 0))] + [SMALL_DGRAD_BIG]
DENORMAL = 2.0 ** -149


def relu_source(M, C, ldm, *key):
    """[M][ldm]: random values with +0.0, -0.0, the smallest denormal and its negative at every seventh element by turns; the
    pattern in the pitch pad."""
    m = _rand((M, C), *key)
    k = ar(M * C).view(M, C) % 7
    for r, v in ((0, 0.0), (1, -0.0), (2, DENORMAL), (3, -DENORMAL)):
        m = torch.where(k == r, torch.full_like(m, v), m)
    t = pattern(M * ldm).view(M, ldm)
    t[:, :C] = m
    return t.reshape(-1)


def _dgrad_parts(p, dtype=torch.float64):
    B, H, W, C, lddx, ldy, ldm = p.case
    dy = p.bufs["dy"].view(B, H, W, ldy)[..., :2].permute(0, 3, 1, 2).to(dtype)
    w = p.bufs["w"].view(2, C, 3, 3).to(dtype)
    keep = p.bufs["relu"].view(B, H, W, ldm)[..., :C] > 0 if ldm else torch.ones(B, H, W, C, dtype=torch.bool)
    return dy, w, keep


def ref_small_dgrad(p, ge=False, noflip=False, row_above=False):
    """dx[pix][c] = mask * sum_{o, ky, kx} w[o][c][ky][kx] dy[pix - (ky - 1, kx - 1)][o] = mask * conv_transpose2d(dy, w, padding 1);
    returns (idx, ref, sum |w| |dy| over the same 18 products, the mask's zeros)."""
    B, H, W, C, lddx, ldy, ldm = p.case
    dy, w, keep = _dgrad_parts(p)
    if ge and ldm:
        keep = p.bufs["relu"].view(B, H, W, ldm)[..., :C] >= 0
    if noflip:
        v = F.conv2d(dy, w.transpose(0, 1), padding=1)
    elif row_above:                                     # the row above the image reads row 0
        v = F.conv_transpose2d(torch.cat([dy[:, :, :1], dy], 2), w, padding=1)[:, :, 1:]
    else:
        v = F.conv_transpose2d(dy, w, padding=1)
    s = F.conv_transpose2d(dy.abs(), w.abs(), padding=1).permute(0, 2, 3, 1)
    v = torch.where(keep, v.permute(0, 2, 3, 1), torch.zeros((), dtype=torch.float64))
    idx = ar(B * H * W)[:, None] * lddx + ar(C)[None, :]
    return idx, v.reshape(-1, C), s.reshape(-1, C), ~keep.reshape(-1, C)


def _build_small_dgrad(op, c):
    B, H, W, C, lddx, ldy, ldm = c
    M = B * H * W
    bufs = dict(dy=_wide(M, 2, ldy, 0, 141, *c[:4], ldy), w=_rand((2 * C * 9,), 142, C, mag=0.3), dx=pattern(M * lddx))
    if ldm:
        bufs["relu"] = relu_source(M, C, ldm, 143, *c[:4])
    return Prob(op, c, bufs)


def _expect_small_dgrad(p):
    idx, v, s, z = ref_small_dgrad(p)
    return dict(dx=Out(p.bufs["dx"], idx, v, scale=U24 * s + TINY, key="dgrad", zero=z))


def _dgrad_terms(p):
    """The 18 fp32 products [B][H][W][C] in the order (ky, kx, o)."""
    B, H, W, C = p.case[:4]
    dy, w, _ = _dgrad_parts(p, torch.float32)
    dyp = F.pad(dy, (1, 1, 1, 1))
    return [(w[o, :, ky, kx], dyp[:, o, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W][..., None]) for ky in range(3) for kx in range(3) for o in range(2)]


def _twins_small_dgrad(p):
    B, H, W, C = p.case[:4]
    _, _, keep = _dgrad_parts(p)
    T = _dgrad_terms(p)
    res = {}
    for name, order in (("tap order", T), ("reversed", T[::-1])):
        s = torch.zeros(B, H, W, C)
        for wv, g in order:
            s = s + wv * g
        res[name] = s
    s = torch.zeros(B, H, W, C)
    for wv, g in T:
        s = _fma(wv.expand(B, H, W, C), g.expand(B, H, W, C), s)
    res["fused"] = s
    return {k: dict(dx=torch.where(keep, v, torch.zeros(())).reshape(-1, C)) for k, v in res.items()}


def _dgrad_mutant(**kw):
    def fn(p):
        if kw.get("ge") and not p.case.ldm:
            return None
        idx, v, _, _ = ref_small_dgrad(p, **kw)
        return dict(dx=Out(p.bufs["dx"], idx, v).image())
    return fn


# ============================================================================================================ the tables
OPS = {
    "stem_fwd": (STEM_FWD_CASES, _build_stem_fwd, _expect_stem_fwd),
    "stem_wgrad": (STEM_WGRAD_CASES, _build_stem_wgrad, _expect_stem_wgrad),
    "small_fwd": (SMALL_FWD_CASES, _build_small_fwd, _expect_small_fwd),
    "small_wgrad": (SMALL_WGRAD_CASES, _build_small_wgrad, _expect_small_wgrad),
    "small_dgrad": (SMALL_DGRAD_CASES, _build_small_dgrad, _expect_small_dgrad),
}


def cases(op):
    return OPS[op][0]


def build(op, case):
    return OPS[op][1](op, case)


@functools.lru_cache(maxsize=None)
def problem(op, case):
    """(problem, expected outputs), computed once and shared: nobody changes them."""
    p = build(op, case)
    return p, OPS[op][2](p)


def twins(p, outs):
    """{variant: {output: float64 values at that output's idx}}: the twins that must pass the comparator themselves."""
    if p.op == "small_dgrad":
        return _twins_small_dgrad(p)
    names = set(outs[next(iter(outs))].alt) | ({"bf16x3"} if p.op.startswith("stem") else set())
    return {v: {k: (o.twins["bf16x3"] if v == "bf16x3" else o.alt[v]) for k, o in outs.items()} for v in names}


MUTANTS = {
    "stem_fwd: the padded eighth tap leaks": ("stem_fwd", _m_stem_fwd_eighth_tap),
    "stem_fwd: a second-trip tile from the first trip's patch": ("stem_fwd", _m_stem_fwd_stale_patch),
    "stem_fwd: no bias on channels >= 32": ("stem_fwd", _m_stem_fwd_no_bias_on_high_half),
    "stem_fwd: column Wo - 1 of a ragged tile not written": ("stem_fwd", _m_stem_fwd_last_column),
    "stem_wgrad: the last slot dropped": ("stem_wgrad", _m_stem_wgrad_last_slot),
    "stem_wgrad: the tail loop's slots counted twice": ("stem_wgrad", _m_stem_wgrad_tail_twice),
    "stem_wgrad: padded taps not dropped": ("stem_wgrad", _m_stem_wgrad_padded_taps),
    "small_fwd: right-hand column of a run's last pixel missing": ("small_fwd", _m_small_fwd_run_end),
    "small_fwd: channels >= 256 missing": ("small_fwd", _m_small_fwd_high_channels),
    "small_wgrad: right-hand column of a run's last pixel missing": ("small_wgrad", _m_small_wgrad_run_end),
    "small_wgrad: channels >= 256 missing": ("small_wgrad", _m_small_wgrad_high_channels),
    "small_wgrad: segment 16 lost": ("small_wgrad", _m_small_wgrad_segment_16),
    "small_wgrad: tap pitch C in place of cpad": ("small_wgrad", _m_small_wgrad_tap_pitch),
    "small_wgrad: dbias from the first wave of each workgroup only": ("small_wgrad", _m_small_wgrad_dbias_first_wave_only),
    "small_dgrad: taps not flipped": ("small_dgrad", _dgrad_mutant(noflip=True)),
    "small_dgrad: mask tested as >= 0": ("small_dgrad", _dgrad_mutant(ge=True)),
    "small_dgrad: the row above is read on y = 0": ("small_dgrad", _dgrad_mutant(row_above=True)),
}

TWIN_WORST = dict(dgrad=5.06)
LIMITS = dict(dgrad=30.0)


def twin_worst():
    """{limit key: the worst need() any fp32 twin of the data gradient reaches on any case}."""
    worst = 0.0
    for c in SMALL_DGRAD_CASES:
        p, outs = problem("small_dgrad", c)
        o = outs["dx"]
        for res in _twins_small_dgrad(p).values():
            worst = max(worst, need(res["dx"], o.ref, o.scale)[0])
    return dict(dgrad=worst)
