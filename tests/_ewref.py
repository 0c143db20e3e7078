"""float64 restatements of the 13 entry points of csrc/elementwise.hip -- the NCHW <-> channels-last pair, space_to_depth2, the
two-channel flow copies, im2col7 / col2im7, relu_bwd, the two ConvGRU gate-backward stages, col_sum, sum_n and axpby -- with their
case tables, fp32 twins, limits and mutants (tests/test_ewref.py on the CPU, tests/test_elementwise_kernels.py against the
kernels).  Plain torch on the CPU; nothing here touches a GPU.

Restatements.  ref_* take what the C entry takes -- flat buffers starting at the pointer the entry gets, pitches, offsets, sizes --
and return (idx, values): the flat positions of the output buffer the operation addresses and what they hold afterwards.  They
are written from the index formulas in the kernel comments (gathers through index tensors, a sliding-window view for im2col7, a
scatter over the 49 taps for col2im7), not from the kernels' loops.  A pure move returns the moved fp32 values themselves; an
operation that does arithmetic returns float64.

Problems.  build(op, case) lays every buffer out as the entry will see it (Prob.bufs: name -> flat fp32): inputs with the NaN
pattern 0x7FC0FFEE in every float that must not be read (pitch pads, columns outside [coff, coff + C), the gaps of a strided flow),
outputs with the pattern everywhere the call must write without reading, prior values where it accumulates, and live finite
values where a neighbour's data sits (relu_bwd's columns at and beyond C, the motion features in front of the flow channels).
expect(prob) returns per output buffer an Out: init (the buffer before the call), idx, ref, scale (None: exact bits), limit key.

Comparator.  score(got, out): infinite if any float outside idx differs from init in a single bit; inside, 0 / inf for an exact
output, else _tailref.need(got, ref, scale) -- the worst |got - ref| / scale, scales elementwise in units of u = 2^-24:
  lay_acc, flow_acc   dst0 + v, one correctly rounded add of two exact operands:  u |ref| + 2^-126
  col2im              u (|dflow0| + sum |terms|) over the live taps
  gru_dz              dh' (q - h) z (1 - z):  u |ref| + 2^-126.  q - h, 1 - z and dhn + dhn2 are differences / sums of EXACT fp32
                      inputs, so each is correctly rounded -- relative u however much cancels -- and the product chain keeps that
  gru_dq              dh' z (1 - q^2):  here the cancellation is real, 1 - fl(q^2) carries u q^2 absolute:  u |dh' z| (q^2 + |1 - q^2|)
  gru_dh              dh' (1 - z):  u |ref| + 2^-126
  gru_sum             sum0 + d:  u (|sum0| + |d|) (d's own error is a few u |d|), for dq_sum with gru_dq's scale in place of u |d|
  gru_dr              d(rh) h r (1 - r):  u |ref| + 2^-126
  gru_dh2             dh0 + d(rh) r:  u (|dh0| + |d(rh) r|)
  col_sum             u (|out0| + |scale| sum_m |x|)
  sum_n               u (|out0| + sum_t |src_t|)
  axpby               a x + b y:  u |ref| + 2^-126 -- the inputs give a x and b y one sign, so |ref| = |a x| + |b y|
Saturated gates (z, r exactly 0 / 1, q exactly +-1) make factors vanish exactly in fp32 and float64 alike: need() counts an
exact result as 0 whatever the scale.

Twins.  The same formulas with every operation rounded to fp32, in an order that is not the kernel's, plus the fused forms a
compiler may contract to (1 - q q, dh0 + g r, a x + b y as one fma); col_sum, whose atomics fix no order: sequential, reversed,
torch.sum and per-row-block partials added in both block orders; sum_n: reversed, torch.sum and the list order.  sum_n is also
compared bit for bit with sum_n_listorder (adds only, in list order: nothing for a compiler to reassociate or fuse) -- which
holds on the device, on every case; the limit against float64 stays as the second, independent check.
LIMITS = 4 x the worst a twin reaches over the case tables (TWIN_WORST), rounded up to one significant digit -- from the twins on
the CPU, never from the kernels.

Mutants.  MUTANTS: name -> (op, function of a problem returning {output: corrupted buffer image} or None where the case cannot
show it).  Each reaches at least 4 x its limit, or fails an exact comparison, on at least one case (tests/test_ewref.py).

Work-item counts.  col2im7, flow_to_nhwc and nhwc_to_flow launch 2 B H W threads, an even number: `one short / exact / one over`
a 256-thread workgroup is 254 / 256 / 258 (B H W = 127 / 128 / 129).
"""
import functools
from collections import namedtuple
from dataclasses import dataclass, field

import torch

from _tailref import TINY, U24, _gen, limit_from_twin, need  # noqa: F401  (limit_from_twin: re-exported)

PATTERN = 0x7FC0FFEE
CAP = 16384 * 256                       # work items of one trip of a capped grid (grid_for)
INF = float("inf")


def pattern(n):
    return torch.full((n,), PATTERN, dtype=torch.int32).view(torch.float32)


def r4(c):
    return (c + 3) // 4 * 4


def ar(n):
    return torch.arange(n)


def f32(x):
    """The fp32 value a C float argument takes."""
    return float(torch.tensor(x, dtype=torch.float32))


def _rand(shape, *key, mag=1.0):
    """Finite fp32 values, none zero."""
    x = mag * torch.randn(shape, generator=_gen(*key))
    return torch.where(x == 0, torch.full_like(x, 0.25), x)


@dataclass
class Out:
    init: torch.Tensor          # the flat fp32 buffer before the call
    idx: torch.Tensor           # flat positions the operation addresses
    ref: torch.Tensor           # what they hold afterwards: fp32 (a pure move) or float64
    scale: object = None        # None: exact bits; else elementwise, the shape of ref
    key: str = ""

    def image(self, values=None):
        """The whole buffer after the call, float64 (fp32 where both sides are): init with `values` (default ref) at idx."""
        v = self.ref if values is None else values
        img = self.init.clone() if v.dtype == torch.float32 else self.init.double()
        img[self.idx.reshape(-1)] = v.reshape(-1)
        return img


@dataclass
class Prob:
    op: str
    case: tuple
    bufs: dict                  # name -> flat fp32 buffer as the device will hold it before the call
    off: dict = field(default_factory=dict)          # name -> floats the payload is moved off its 16-byte alignment by
    arg: dict = field(default_factory=dict)          # further scalars of the call


def _same(a, b):
    """Elementwise identity: bits for two fp32 tensors; value and sign (NaN equal to NaN) otherwise."""
    if a.dtype == torch.float32 and b.dtype == torch.float32:
        return a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)
    a, b = a.double(), b.double()
    return ((a == b) & (torch.signbit(a) == torch.signbit(b))) | (torch.isnan(a) & torch.isnan(b))


def score(got, o):
    """inf: a float outside idx changed, or an exact output differs; else the worst |got - ref| / scale inside."""
    got = got.reshape(-1)
    assert got.numel() == o.init.numel()
    outside = torch.ones(got.numel(), dtype=torch.bool)
    outside[o.idx.reshape(-1)] = False
    if not bool(_same(got[outside], o.init[outside]).all()):
        return INF
    g = got[o.idx.reshape(-1)].reshape(o.ref.shape)
    if o.scale is None:
        return 0.0 if bool(_same(g, o.ref).all()) else INF
    return need(g, o.ref, o.scale)[0]


# ================================================================================================== NCHW <-> channels-last
LayoutCase = namedtuple("LayoutCase", "B C HW ld coff acc")


def _layout_cases():
    out = []
    shapes = [(v, 33 if v != 33 else 31) for v in (1, 31, 32, 33)] + [(33 if v != 33 else 31, v) for v in (1, 31, 32, 33)]
    for C, HW in shapes:
        for ld, coff in ((C, 0), (r4(C), 0), (C + 7, 0), (C + 7, 3)):
            for acc in (0, 1):
                out.append(LayoutCase(2, C, HW, ld, coff, acc))
    out.append(LayoutCase(2, 37, 45, 40, 0, 0))          # test_gemm_and_layout_kernels' shape: 2x37x5x9, C padded to 40
    return list(dict.fromkeys(out))


LAYOUT_CASES = _layout_cases()
TRANSPOSE_CASE = LayoutCase(3, 33, 65, 33, 0, 0)         # ops.transpose_batched of [3][65][33]: nhwc_to_nchw with ld = C = N, HW = M


def layout_index(B, C, HW, ld, coff):
    """Flat positions of element (b, p, c), [B][HW][C]: in the NCHW tensor and in the channels-last one."""
    b, p, c = ar(B)[:, None, None], ar(HW)[None, :, None], ar(C)[None, None, :]
    return (b * C + c) * HW + p, (b * HW + p) * ld + coff + c


def ref_nchw_to_nhwc(src, dst0, B, C, HW, ld, coff, acc):
    """dst[(b HW + p) ld + coff + c] (=|+=) src[(b C + c) HW + p]"""
    i_s, i_d = layout_index(B, C, HW, ld, coff)
    v = src[i_s]
    return i_d, (dst0[i_d].double() + v.double() if acc else v)


def ref_nhwc_to_nchw(src, dst0, B, C, HW, ld, coff, acc):
    """dst[(b C + c) HW + p] (=|+=) src[(b HW + p) ld + coff + c]"""
    i_d, i_s = layout_index(B, C, HW, ld, coff)
    v = src[i_s]
    return i_d, (dst0[i_d].double() + v.double() if acc else v)


def _build_layout(op, c):
    B, C, HW, ld, coff, acc = c
    i_n, i_c = layout_index(B, C, HW, ld, coff)
    nchw, nhwc = pattern(B * C * HW), pattern(B * HW * ld)
    src_idx, dst_idx = (i_n, i_c) if op == "nchw_to_nhwc" else (i_c, i_n)
    src, dst = (nchw, nhwc) if op == "nchw_to_nhwc" else (nhwc, nchw)
    src[src_idx] = _rand((B, HW, C), 11, *c)
    if acc:
        dst[dst_idx] = _rand((B, HW, C), 12, *c, mag=3.0)
    return Prob(op, c, dict(src=src, dst=dst))


def _expect_layout(p):
    ref = ref_nchw_to_nhwc if p.op == "nchw_to_nhwc" else ref_nhwc_to_nchw
    idx, v = ref(p.bufs["src"], p.bufs["dst"], *p.case)
    if not p.case.acc:
        return dict(dst=Out(p.bufs["dst"], idx, v))
    return dict(dst=Out(p.bufs["dst"], idx, v, U24 * v.abs() + TINY, "lay_acc"))


def _twins_layout(p):
    if not p.case.acc:
        return {}
    B, C, HW, ld, coff, _ = p.case
    i_n, i_c = layout_index(B, C, HW, ld, coff)
    i_s, i_d = (i_n, i_c) if p.op == "nchw_to_nhwc" else (i_c, i_n)
    return {"v + dst0": dict(dst=p.bufs["src"][i_s] + p.bufs["dst"][i_d])}


def _m_layout_coff_ignored(p):
    if not p.case.coff:
        return None
    ref = ref_nchw_to_nhwc if p.op == "nchw_to_nhwc" else ref_nhwc_to_nchw
    idx, v = ref(p.bufs["src"], p.bufs["dst"], *p.case._replace(coff=0))
    return dict(dst=Out(p.bufs["dst"], idx, v).image())


def _m_layout_accumulate_ignored(p):
    if not p.case.acc:
        return None
    ref = ref_nchw_to_nhwc if p.op == "nchw_to_nhwc" else ref_nhwc_to_nchw
    idx, v = ref(p.bufs["src"], p.bufs["dst"], *p.case._replace(acc=0))
    return dict(dst=Out(p.bufs["dst"], idx, v).image())


# ========================================================================================================== space_to_depth2
S2dCase = namedtuple("S2dCase", "B H W C inverse")
S2D_SHAPES = ((1, 2, 2, 4), (2, 2, 6, 8), (2, 6, 8, 4), (2, 6, 8, 12), (2, 4, 2, 12))
S2D_BIG = (1, 2, 2097154, 4)            # 4194308 chunks: the smallest count past the cap (even H and W: B H W is a multiple of 4)
S2D_CASES = [S2dCase(*s, inv) for s in S2D_SHAPES + (S2D_BIG,) for inv in (0, 1)]


def s2d_pixel_index(B, H, W, swap=False):
    """(raster pixel index p, block-major pixel index q) of pixel (b, y, x), [B][H][W]:
    q = ((b H/2 + y/2) W/2 + x/2) 4 + (y % 2) 2 + x % 2."""
    b, y, x = ar(B)[:, None, None], ar(H)[None, :, None], ar(W)[None, None, :]
    sub = (x % 2) * 2 + y % 2 if swap else (y % 2) * 2 + x % 2
    return (b * H + y) * W + x, ((b * (H // 2) + y // 2) * (W // 2) + x // 2) * 4 + sub


def ref_space_to_depth2(src, B, H, W, C, inverse, swap=False):
    """dst[b][y/2][x/2][(y%2) 2 + x%2][c] = src[b][y][x][c]; inverse: the other way."""
    p, q = s2d_pixel_index(B, H, W, swap)
    c = ar(C)
    ip, iq = (p[..., None] * C + c).reshape(-1), (q[..., None] * C + c).reshape(-1)
    return (ip, src[iq]) if inverse else (iq, src[ip])


def _build_s2d(op, c):
    n = c.B * c.H * c.W * c.C
    return Prob(op, c, dict(src=_rand((n,), 21, *c), dst=pattern(n)))


def _expect_s2d(p):
    idx, v = ref_space_to_depth2(p.bufs["src"], *p.case)
    return dict(dst=Out(p.bufs["dst"], idx, v))


def _m_s2d_sub_bits_swapped(p):
    idx, v = ref_space_to_depth2(p.bufs["src"], *p.case, swap=True)
    return dict(dst=Out(p.bufs["dst"], idx, v).image())


# ============================================================================================================ flow layouts
FLOW_LAYOUTS = ("planar", "interleaved", "wide")


def flow_buffer(flow, layout):
    """(flat fp32, base, bs, cs, ps): element (b, c, pix) of flow [B][2][HW] at base + b bs + c cs + pix ps; every other float
    holds the NaN pattern.  wide: the pair at floats 3 and 4 of rows of six (a slice of a wider channels-last tensor)."""
    B, _, HW = flow.shape
    if layout == "planar":
        return flow.reshape(-1).clone(), 0, 2 * HW, HW, 1
    if layout == "interleaved":
        return flow.permute(0, 2, 1).reshape(-1).clone(), 0, 2 * HW, 1, 2
    flat = pattern(B * HW * 6)
    flat.view(B, HW, 6)[:, :, 3:5] = flow.permute(0, 2, 1)
    return flat, 3, 6 * HW, 1, 6


def flow_index(base, bs, cs, ps, B, HW):
    """[B][2][HW] flat positions of the strided flow."""
    return base + ar(B)[:, None, None] * bs + ar(2)[None, :, None] * cs + ar(HW)[None, None, :] * ps


# ================================================================================================================== im2col7
Im2colCase = namedtuple("Im2colCase", "B H W ld off layout")
IMAGES = ((1, 1), (1, 9), (3, 3), (7, 7), (8, 5))
IM2COL_BIG = (Im2colCase(1, 410, 410, 100, 0, "planar"),          # 168100 x 25 chunks = 4202500 > CAP: im2col7_v4_kernel's second trip
              Im2colCase(1, 205, 205, 100, 1, "planar"))          # 42025 x 100 floats = 4202500 > CAP: im2col7_kernel's
IM2COL_CASES = [Im2colCase(2, H, W, ld, off, FLOW_LAYOUTS[(i + j + off) % 3])
                for i, (H, W) in enumerate(IMAGES) for j, ld in enumerate((100, 104, 128)) for off in (0, 1)] + list(IM2COL_BIG)


def _windows(P):
    """[B][2][H+6][W+6] -> [B][H][W][98]: the 7x7 window whose corner is (y, x), channel-major."""
    B, _, Hp, Wp = P.shape
    w = P.unfold(2, 7, 1).unfold(3, 7, 1)               # [B][2][H][W][7][7]
    return w.permute(0, 2, 3, 1, 4, 5).reshape(B, Hp - 6, Wp - 6, 98)


def _padded(fl, clamp=False):
    B, _, H, W = fl.shape
    if clamp:
        yy, xx = (ar(H + 6) - 3).clamp(0, H - 1), (ar(W + 6) - 3).clamp(0, W - 1)
        return fl[:, :, yy][:, :, :, xx]
    P = torch.zeros(B, 2, H + 6, W + 6, dtype=fl.dtype)
    P[:, :, 3:3 + H, 3:3 + W] = fl
    return P


def ref_im2col7(flow, base, bs, cs, ps, ld, B, H, W, mut=""):
    """cols[m][ci 49 + ky 7 + kx] = flow[b, ci, y + ky - 3, x + kx - 3], zero outside the image; columns 98 .. ld - 1 zero."""
    fl = flow[flow_index(base, bs, cs, ps, B, H * W)].view(B, 2, H, W)
    win = _windows(_padded(fl, mut == "clamp"))
    if mut == "flip":                                   # y - (ky - 3)
        win = win.view(B, H, W, 2, 7, 7).flip(4).reshape(B, H, W, 98)
    cols = torch.zeros(B, H, W, ld, dtype=flow.dtype)
    cols[..., :98] = win
    return ar(B * H * W * ld), cols.reshape(-1)


def _build_im2col(op, c):
    flow = _rand((c.B, 2, c.H * c.W), 31, c.B, c.H, c.W)
    flat, base, bs, cs, ps = flow_buffer(flow, c.layout)
    return Prob(op, c, dict(flow=flat, cols=pattern(c.B * c.H * c.W * c.ld)), dict(cols=c.off), dict(base=base, bs=bs, cs=cs, ps=ps))


def _expect_im2col(p, mut=""):
    c, a = p.case, p.arg
    idx, v = ref_im2col7(p.bufs["flow"], a["base"], a["bs"], a["cs"], a["ps"], c.ld, c.B, c.H, c.W, mut)
    return dict(cols=Out(p.bufs["cols"], idx, v))


def _m_im2col_tap_sign_flipped(p):
    return dict(cols=_expect_im2col(p, "flip")["cols"].image())


def _m_im2col_border_clamped(p):
    return dict(cols=_expect_im2col(p, "clamp")["cols"].image())


# ================================================================================================================== col2im7
Col2imCase = namedtuple("Col2imCase", "B H W ld acc")
COL2IM_CASES = ([Col2imCase(2, H, W, ld, acc) for (H, W) in IMAGES for ld in (100, 104) for acc in (0, 1)]
                + [Col2imCase(1, 1, n, 100, n % 2) for n in (127, 128, 129)])


def _taps64(dcols, ld, B, H, W):
    return dcols.view(B, H, W, ld)[..., :98].reshape(B, H, W, 2, 7, 7)


def _scatter49(D, order=None):
    """sum over the taps of D[b, y, x, ci, ky, kx] landing on pixel (y + ky - 3, x + kx - 3), in D's dtype, tap by tap."""
    B, H, W = D.shape[:3]
    P = torch.zeros(B, 2, H + 6, W + 6, dtype=D.dtype)
    for t in (range(49) if order is None else order):
        ky, kx = t // 7, t % 7
        P[:, :, ky:ky + H, kx:kx + W] += D[:, :, :, :, ky, kx].permute(0, 3, 1, 2)
    return P[:, :, 3:3 + H, 3:3 + W]


def ref_col2im7(dcols, ld, dflow0, B, H, W, acc):
    """dflow[b, ci, y, x] (=|+=) the sum over the taps (ky, kx) whose source pixel (y - (ky - 3), x - (kx - 3)) lies in the image
    of dcols[that pixel][ci 49 + ky 7 + kx]: the adjoint of im2col7, as a scatter.  Returns (idx, ref, sum of |terms|)."""
    D = _taps64(dcols, ld, B, H, W).double()
    s, sa = _scatter49(D), _scatter49(D.abs())
    if acc:
        d0 = dflow0.view(B, 2, H, W).double()
        s, sa = s + d0, sa + d0.abs()
    return ar(B * 2 * H * W), s.reshape(-1), sa.reshape(-1)


def _build_col2im(op, c):
    B, H, W, ld, acc = c
    dcols = pattern(B * H * W * ld)
    dcols.view(B, H, W, ld)[..., :98] = _rand((B, H, W, 98), 41, *c)
    return Prob(op, c, dict(dcols=dcols, dflow=_rand((B * 2 * H * W,), 42, *c, mag=5.0) if acc else pattern(B * 2 * H * W)))


def _expect_col2im(p):
    B, H, W, ld, acc = p.case
    idx, s, sa = ref_col2im7(p.bufs["dcols"], ld, p.bufs["dflow"], B, H, W, acc)
    return dict(dflow=Out(p.bufs["dflow"], idx, s, U24 * sa + TINY, "col2im"))


def _col2im_terms(p):
    """[49][B][2][H][W] fp32: the term of tap t at every pixel, zero where its source lies outside."""
    B, H, W, ld, _ = p.case
    D = _taps64(p.bufs["dcols"], ld, B, H, W)
    out = []
    for t in range(49):
        ky, kx = t // 7, t % 7
        Z = torch.zeros(B, 2, H + 6, W + 6)
        Z[:, :, ky:ky + H, kx:kx + W] = D[:, :, :, :, ky, kx].permute(0, 3, 1, 2)
        out.append(Z[:, :, 3:3 + H, 3:3 + W])
    return torch.stack(out)


def _twins_col2im(p):
    B, H, W, ld, acc = p.case
    T = _col2im_terms(p)
    d0 = p.bufs["dflow"].view(B, 2, H, W)
    res = {}
    s = torch.zeros(B, 2, H, W)
    for t in reversed(range(49)):
        s = s + T[t]
    res["taps last to first"] = s
    res["torch.sum"] = T.sum(0)
    rows = [T[7 * k:7 * k + 7].sum(0) for k in range(7)]
    s = rows[0]
    for r_ in rows[1:]:
        s = s + r_
    res["row partials"] = s
    return {k: dict(dflow=(v + d0 if acc else v).reshape(-1)) for k, v in res.items()}


def _col2im_gather(p, flip=False, clamp=False):
    """The sum as a gather over the taps, float64, with the mutations."""
    B, H, W, ld, acc = p.case
    D = _taps64(p.bufs["dcols"], ld, B, H, W).double()
    out = torch.zeros(B, 2, H, W, dtype=torch.float64)
    y, x = ar(H), ar(W)
    for t in range(49):
        ky, kx = t // 7, t % 7
        yy, xx = (y + (ky - 3) if flip else y - (ky - 3)), x - (kx - 3)
        oky, okx = (yy >= 0) & (yy < H), (xx >= 0) & (xx < W)
        term = D[:, yy.clamp(0, H - 1)][:, :, xx.clamp(0, W - 1)][:, :, :, :, ky, kx].permute(0, 3, 1, 2)
        if not clamp:
            term = term * (oky[:, None] & okx[None, :])
        out += term
    if acc:
        out += p.bufs["dflow"].view(B, 2, H, W).double()
    return dict(dflow=out.reshape(-1))


def _m_col2im_tap_sign_flipped(p):
    return _col2im_gather(p, flip=True)


def _m_col2im_border_clamped(p):
    return _col2im_gather(p, clamp=True)


# ========================================================================================== flow_to_nhwc / nhwc_to_flow
FlowCase = namedtuple("FlowCase", "B HW ld coff layout acc")
_FLOW_SHAPES = ((1, 127), (2, 64), (3, 43))            # 2 M = 254, 256, 258
FLOW_TO_NHWC_CASES = [FlowCase(B, HW, ld, coff, FLOW_LAYOUTS[(i + j) % 3], 0)
                      for i, (B, HW) in enumerate(_FLOW_SHAPES) for j, (ld, coff) in enumerate(((128, 126), (4, 0), (128, 126)))]
NHWC_TO_FLOW_CASES = [FlowCase(B, HW, ld, coff, "planar", acc)
                      for (B, HW) in _FLOW_SHAPES for (ld, coff) in ((128, 126), (4, 0)) for acc in (0, 1)]


def ref_flow_to_nhwc(flow, base, bs, cs, ps, ld, coff, B, HW):
    """dst[(b HW + p) ld + coff + c] = flow[b, c, p]"""
    b, c, p = ar(B)[:, None, None], ar(2)[None, :, None], ar(HW)[None, None, :]
    return (b * HW + p) * ld + coff + c, flow[flow_index(base, bs, cs, ps, B, HW)]


def ref_nhwc_to_flow(src, ld, coff, dflow0, B, HW, acc):
    """dflow[(b 2 + c) HW + p] (=|+=) src[(b HW + p) ld + coff + c]"""
    b, c, p = ar(B)[:, None, None], ar(2)[None, :, None], ar(HW)[None, None, :]
    idx = (b * 2 + c) * HW + p
    v = src[(b * HW + p) * ld + coff + c]
    return idx, (dflow0[idx].double() + v.double() if acc else v)


def _nhwc_with_live_front(B, HW, ld, coff, *key):
    """A channels-last buffer: live values in the columns in front of coff (the motion features), pattern from coff on."""
    t = pattern(B * HW * ld).view(B * HW, ld)
    t[:, :coff] = _rand((B * HW, coff), *key)
    return t.reshape(-1)


def _build_flow_to_nhwc(op, c):
    flat, base, bs, cs, ps = flow_buffer(_rand((c.B, 2, c.HW), 51, *c[:4]), c.layout)
    return Prob(op, c, dict(flow=flat, dst=_nhwc_with_live_front(c.B, c.HW, c.ld, c.coff, 52, *c[:4])), {}, dict(base=base, bs=bs, cs=cs, ps=ps))


def _expect_flow_to_nhwc(p):
    c, a = p.case, p.arg
    idx, v = ref_flow_to_nhwc(p.bufs["flow"], a["base"], a["bs"], a["cs"], a["ps"], c.ld, c.coff, c.B, c.HW)
    return dict(dst=Out(p.bufs["dst"], idx, v))


def _build_nhwc_to_flow(op, c):
    src = _nhwc_with_live_front(c.B, c.HW, c.ld, c.coff, 53, *c[:4]).view(-1, c.ld)
    src[:, c.coff:c.coff + 2] = _rand((c.B * c.HW, 2), 54, *c[:4])
    n = c.B * 2 * c.HW
    return Prob(op, c, dict(src=src.reshape(-1), dflow=_rand((n,), 55, *c[:4], mag=3.0) if c.acc else pattern(n)))


def _expect_nhwc_to_flow(p):
    c = p.case
    idx, v = ref_nhwc_to_flow(p.bufs["src"], c.ld, c.coff, p.bufs["dflow"], c.B, c.HW, c.acc)
    return dict(dflow=Out(p.bufs["dflow"], idx, v, U24 * v.abs() + TINY, "flow_acc") if c.acc else Out(p.bufs["dflow"], idx, v))


def _twins_nhwc_to_flow(p):
    c = p.case
    if not c.acc:
        return {}
    idx, v = ref_nhwc_to_flow(p.bufs["src"], c.ld, c.coff, p.bufs["dflow"], c.B, c.HW, 0)
    return {"v + dflow0": dict(dflow=v + p.bufs["dflow"][idx])}


# ================================================================================================================= relu_bwd
ReluCase = namedtuple("ReluCase", "M C ldg ldy")
RELU_BIG = ReluCase(CAP + 3, 4, 4, 8)


def _relu_cases():
    out = []
    for C in (4, 80, 126, 128):
        for ldg in sorted({r4(C), 128, 132}):
            if ldg >= C:
                for M in (1, 3):
                    out.append(ReluCase(M, C, ldg, 132 if ldg != 132 else 128))
    return out + [RELU_BIG]


RELU_CASES = _relu_cases()


def ref_relu_bwd(g, ldg, y, ldy, M, C, ge=False, tail=False):
    """g[m ldg + c] = g[m ldg + c] where y[m ldy + c] > 0, else +0.0, for c < C: the incoming gradient or a zero, nothing computed."""
    Ce = r4(C) if tail else C
    m, c = ar(M)[:, None], ar(Ce)[None, :]
    idx = m * ldg + c
    yv = y[m * ldy + c]
    return idx, torch.where((yv >= 0) if ge else (yv > 0), g[idx], torch.zeros((), dtype=g.dtype))


def _build_relu(op, c):
    M, C, ldg, ldy = c
    g = _rand((M, ldg), 61, *c, mag=2.0)
    y = torch.randn(M, ldy, generator=_gen(62, *c))
    y = torch.where(y == 0, torch.full_like(y, 0.5), y)
    # designed: exact +0.0 and -0.0 (both masked: not > 0) under non-zero gradients, in the first columns of row 0 and on the
    # last columns below C of the last row; the columns at and beyond C hold y <= 0 under non-zero g -- a kernel that masks them
    # too destroys them
    y[0, 0], y[0, 1] = 0.0, -0.0
    y[M - 1, C - 1], y[M - 1, C - 2] = -0.0, 0.0
    y[:, C:] = -y[:, C:].abs()
    if ldy > C:
        y[0, C] = 0.0
    g[0, 2] = -0.0                                      # a negative zero that survives (y > 0 there)
    y[0, 2] = 1.5
    return Prob(op, c, dict(g=g.reshape(-1), y=y.reshape(-1)))


def _expect_relu(p, **mut):
    M, C, ldg, ldy = p.case
    idx, v = ref_relu_bwd(p.bufs["g"], ldg, p.bufs["y"], ldy, M, C, **mut)
    return dict(g=Out(p.bufs["g"], idx, v))


def _m_relu_ge(p):
    return dict(g=_expect_relu(p, ge=True)["g"].image())


def _m_relu_touches_tail_columns(p):
    return dict(g=_expect_relu(p, tail=True)["g"].image()) if p.case.C % 4 else None


# ===================================================================================================== ConvGRU gate backward
GruCase = namedtuple("GruCase", "M hid ldzr sums dhn2 off")
GRU_B1_PTRS = ("dhn", "z", "q", "h", "dzr", "dq", "dh", "dzr_sum", "dq_sum")
GRU_B2_PTRS = ("drh", "r", "h", "dzr", "dh", "dzr_sum")
GRU_BIG = GruCase(CAP + 1, 4, 8, 0, 0, "")


def _gru_cases():
    out = []
    for hid in (4, 96, 128):
        for ldzr in (2 * hid, 2 * hid + 4):
            for sums, dhn2 in ((0, 0), (1, 1), (1, 0), (0, 1)):
                out.append(GruCase(3, hid, ldzr, sums, dhn2, ""))
    out += [GruCase(M, 4, ldzr, 1, 1, "") for M, ldzr in ((255, 8), (256, 12), (257, 8))]       # M hid / 4 = 255, 256, 257
    out += [GruCase(5, 6, 12, 1, 0, ""), GruCase(5, 6, 16, 0, 0, ""), GruCase(5, 6, 13, 1, 0, ""),   # hid % 4
            GruCase(65, 4, 9, 1, 0, ""), GruCase(3, 96, 193, 0, 0, "")]                               # ldzr % 4
    out += [GruCase(65, 4, 8 + 4 * (i % 2), 1, 0, name) for i, name in enumerate(dict.fromkeys(GRU_B1_PTRS + GRU_B2_PTRS))]
    return out + [GRU_BIG]


GRU_CASES = _gru_cases()


def gru_route(c, stage):
    """`v4` / `scalar`: the kernel the entry of stage 1 / 2 picks."""
    ptrs = GRU_B1_PTRS if stage == 1 else GRU_B2_PTRS
    live = c.off in ptrs and (c.sums or not c.off.endswith("_sum"))
    return "v4" if (c.hid % 4 == 0 and c.ldzr % 4 == 0 and not live) else "scalar"


def ref_gru_bwd1(dhn, dhn2, z, q, h, zsum0, qsum0, ldzr, M, hid, mut=""):
    """With g = dhn (+ dhn2) and h' = (1 - z) h + z q:  dzr[m][c] = g (q - h) z (1 - z),  dq = g z (1 - q^2),  dh = g (1 - z)
    for c < hid; dzr_sum[m][c] += dzr[m][c], dq_sum += dq.  Returns {name: (idx, ref)} and the scales' ingredients."""
    d = lambda t: t[:M * hid].double().view(M, hid)
    g = d(dhn) + (d(dhn2) if (dhn2 is not None and mut != "no_dhn2") else 0.0)
    zz, qq, hh = d(z), d(q), d(h)
    dz = g * (qq - hh) * (1.0 if mut == "no_zz" else zz * (1 - zz))
    dq = g * zz * (1 - qq * qq)
    dh = g * (1 - zz)
    iz = ar(M)[:, None] * ldzr + ar(hid)[None, :]
    ie = ar(M * hid).view(M, hid)
    out = dict(dzr=(iz, dz), dq=(ie, dq), dh=(ie, dh))
    if zsum0 is not None:
        out["dzr_sum"] = (iz, zsum0[iz].double() + (0.0 if mut == "no_sum" else dz))
    if qsum0 is not None:
        out["dq_sum"] = (ie, qsum0[ie].double() + (0.0 if mut == "no_sum" else dq))
    return out, dict(gz=(g * zz).abs(), q2=qq * qq)


def ref_gru_bwd2(drh, r, h, dh0, zsum0, ldzr, M, hid, mut=""):
    """dzr[m][hid + c] = d(rh) h r (1 - r),  dh[m][c] += d(rh) r;  dzr_sum[m][hid + c] += dzr[m][hid + c]."""
    d = lambda t: t[:M * hid].double().view(M, hid)
    g, rr, hh = d(drh), d(r), d(h)
    dr, add = g * hh * rr * (1 - rr), g * rr
    iz = ar(M)[:, None] * ldzr + (0 if mut == "low_half" else hid) + ar(hid)[None, :]
    ie = ar(M * hid).view(M, hid)
    out = dict(dzr=(iz, dr), dh=(ie, add if mut == "overwrite" else d(dh0) + add))
    if zsum0 is not None:
        out["dzr_sum"] = (iz, zsum0[iz].double() + dr)
    return out, dict(add=add.abs())


def gru_inputs(c):
    """{name: flat fp32} of both stages' inputs: gates strictly inside (0, 1) / (-1, 1) but for the designed first elements --
    z = 0, 1, r = 0, 1, q = +1, -1 exactly (positions 0 .. 5 of z, r, q: each saturated value under unsaturated partners)."""
    M, hid = c.M, c.hid
    n = M * hid
    k = (71, M, hid)
    uni = lambda i: torch.rand(n, generator=_gen(*k, i)).clamp(2.0 ** -20, 1 - 2.0 ** -20)          # (no libm call: the same bits anywhere)
    z, r, q = uni(1), uni(2), 2.0 * uni(3) - 1.0
    z[0], z[1], r[2], r[3], q[4], q[5] = 0.0, 1.0, 0.0, 1.0, 1.0, -1.0
    return dict(dhn=_rand((n,), *k, 4), dhn2=_rand((n,), *k, 5, mag=0.5), z=z, q=q, h=_rand((n,), *k, 6, mag=0.7), r=r,
                drh=_rand((n,), *k, 7))


def _build_gru1(op, c):
    M, hid, ldzr = c.M, c.hid, c.ldzr
    x = gru_inputs(c)
    bufs = dict(dhn=x["dhn"], z=x["z"], q=x["q"], h=x["h"], dzr=pattern(M * ldzr), dq=pattern(M * hid), dh=pattern(M * hid))
    if c.dhn2:
        bufs["dhn2"] = x["dhn2"]
    if c.sums:                                          # prior sums in the columns of both halves, pattern in the pitch pad
        zs = pattern(M * ldzr).view(M, ldzr)
        zs[:, :2 * hid] = _rand((M, 2 * hid), 72, M, hid, ldzr, mag=4.0)
        bufs["dzr_sum"], bufs["dq_sum"] = zs.reshape(-1), _rand((M * hid,), 73, M, hid, mag=4.0)
    return Prob(op, c, bufs, {c.off: 1} if c.off in bufs else {})


def _expect_gru1(p, mut=""):
    c, b = p.case, p.bufs
    r_, s = ref_gru_bwd1(b["dhn"], b.get("dhn2"), b["z"], b["q"], b["h"], b.get("dzr_sum"), b.get("dq_sum"), c.ldzr, c.M, c.hid, mut)
    s_dq = U24 * s["gz"] * (s["q2"] + (1 - s["q2"]).abs()) + TINY
    out = dict(dzr=Out(b["dzr"], *r_["dzr"], U24 * r_["dzr"][1].abs() + TINY, "gru_dz"), dq=Out(b["dq"], *r_["dq"], s_dq, "gru_dq"),
               dh=Out(b["dh"], *r_["dh"], U24 * r_["dh"][1].abs() + TINY, "gru_dh"))
    if c.sums:
        iz, ie = r_["dzr"][0], r_["dq"][0]
        out["dzr_sum"] = Out(b["dzr_sum"], *r_["dzr_sum"], U24 * (b["dzr_sum"][iz].double().abs() + r_["dzr"][1].abs()) + TINY, "gru_sum")
        out["dq_sum"] = Out(b["dq_sum"], *r_["dq_sum"], U24 * b["dq_sum"][ie].double().abs() + s_dq, "gru_sum")
    return out


def _fma(a, b, c):
    """fl32(a b + c)"""
    return (a.double() * b.double() + c.double()).float()


def _twins_gru1(p):
    c, b = p.case, p.bufs
    n = c.M * c.hid
    v = lambda k: b[k][:n].view(c.M, c.hid)
    g = v("dhn2") + v("dhn") if c.dhn2 else v("dhn")
    z, q, h = v("z"), v("q"), v("h")
    one = torch.ones(())
    dz = (g * z) * ((q - h) * (one - z))
    dh = (one - z) * g
    res = {}
    for name, omq in (("plain", one - q * q), ("fused", _fma(-q, q, one.expand_as(q)))):
        dq = omq * (z * g)
        o = dict(dzr=dz, dq=dq, dh=dh)
        if c.sums:
            iz = ar(c.M)[:, None] * c.ldzr + ar(c.hid)[None, :]
            o["dzr_sum"], o["dq_sum"] = dz + b["dzr_sum"][iz], dq + b["dq_sum"][:n].view(c.M, c.hid)
        res[name] = o
    return res


def _build_gru2(op, c, after1=None):
    """after1: {dzr, dh, dzr_sum} as stage 1 left them (default: its restatement rounded to fp32)."""
    p1 = _build_gru1("gru_bwd1", c)
    if after1 is None:
        after1 = {k: o.image().float() for k, o in _expect_gru1(p1).items() if k in ("dzr", "dh", "dzr_sum")}
    x = gru_inputs(c)
    bufs = dict(drh=x["drh"], r=x["r"], h=x["h"], dzr=after1["dzr"], dh=after1["dh"])
    if c.sums:
        bufs["dzr_sum"] = after1["dzr_sum"]
    return Prob(op, c, bufs, {c.off: 1} if c.off in bufs else {})


def _expect_gru2(p, mut=""):
    c, b = p.case, p.bufs
    r_, s = ref_gru_bwd2(b["drh"], b["r"], b["h"], b["dh"], b.get("dzr_sum"), c.ldzr, c.M, c.hid, mut)
    ie = r_["dh"][0]
    out = dict(dzr=Out(b["dzr"], *r_["dzr"], U24 * r_["dzr"][1].abs() + TINY, "gru_dr"),
               dh=Out(b["dh"], *r_["dh"], U24 * (b["dh"][ie].double().abs() + s["add"]) + TINY, "gru_dh2"))
    if c.sums:
        iz = r_["dzr"][0]
        out["dzr_sum"] = Out(b["dzr_sum"], *r_["dzr_sum"], U24 * (b["dzr_sum"][iz].double().abs() + r_["dzr"][1].abs()) + TINY, "gru_sum")
    return out


def _twins_gru2(p):
    c, b = p.case, p.bufs
    n = c.M * c.hid
    v = lambda k: b[k][:n].view(c.M, c.hid)
    g, r, h, dh0 = v("drh"), v("r"), v("h"), v("dh")
    dr = (g * r) * (h * (torch.ones(()) - r))
    res = {}
    for name, dh in (("plain", r * g + dh0), ("fused", _fma(g, r, dh0))):
        o = dict(dzr=dr, dh=dh)
        if c.sums:
            iz = ar(c.M)[:, None] * c.ldzr + c.hid + ar(c.hid)[None, :]
            o["dzr_sum"] = dr + b["dzr_sum"][iz]
        res[name] = o
    return res


def _gru1_mutant(mut, needs=None):
    """needs: the case field that has to be set for the mutation to change anything."""
    def fn(p):
        if needs and not getattr(p.case, needs):
            return None
        return {k: o.image() for k, o in _expect_gru1(p, mut).items()}
    return fn


def _gru2_mutant(mut):
    def fn(p):
        clean = _expect_gru2(p)
        bad = _expect_gru2(p, mut)
        return {k: Out(clean[k].init, bad[k].idx, bad[k].ref).image() for k in bad}
    return fn


# ================================================================================================================== col_sum
ColSumCase = namedtuple("ColSumCase", "M C ld scale")
COL_SUM_BIG = ColSumCase(2048 * 128 + 1, 4, 8, -0.5)
COL_SUM_CASES = [ColSumCase(M, C, C + (1, 3, 4, 7)[i % 4], (1.0, -0.5)[i % 2])
                 for i, (M, C) in enumerate(zip((1, 3, 127, 128, 129, 255, 256, 257), (65, 1, 63, 64, 65, 1, 63, 64)))] + [COL_SUM_BIG]


def col_sum_geometry(M):
    """(row blocks the entry launches, rows per block): ysplit = clamp(M / 128, 1, 2048)."""
    ys = min(max(M // 128, 1), 2048)
    return ys, (M + ys - 1) // ys


def ref_col_sum(x, ld, M, C, out0, scale, rows=None, mut=""):
    """out[c] += scale sum_m x[m ld + c] for c < C.  Returns (idx, ref, scale ingredient |out0| + |scale| sum |x|)."""
    X = x[ar(M if rows is None else rows)[:, None] * ld + ar(C)[None, :]].double()
    o0 = out0[:C].double()
    s = (1.0 if mut == "no_scale" else f32(scale)) * X.sum(0)
    return ar(C), (s if mut == "overwrite" else o0 + s), o0.abs() + abs(f32(scale)) * X.abs().sum(0)


def _build_col_sum(op, c):
    M, C, ld, _ = c
    x = pattern(M * ld).view(M, ld)
    v = _rand((M, C), 81, M, C)
    v = v * (2.0 ** (12.0 * ((ar(M) % 7 == 0).float() - (ar(M) % 7 == 1).float())))[:, None]          # large rows next to tiny ones
    x[:, :C] = v
    out = pattern(C + 3)
    out[:C] = _rand((C,), 82, M, C, mag=30.0)
    return Prob(op, c, dict(x=x.reshape(-1), out=out))


def _expect_col_sum(p, **kw):
    M, C, ld, scale = p.case
    idx, ref, s = ref_col_sum(p.bufs["x"], ld, M, C, p.bufs["out"], scale, **kw)
    return dict(out=Out(p.bufs["out"], idx, ref, U24 * s, "col_sum"))


def _seq(rows):
    """Sequential fp32 sum over dim 0."""
    s = torch.zeros(rows.shape[1:])
    for r_ in rows:
        s = s + r_
    return s


def _twins_col_sum(p):
    M, C, ld, scale = p.case
    X = p.bufs["x"].view(M, ld)[:, :C]
    o0, sc = p.bufs["out"][:C], torch.tensor(scale, dtype=torch.float32)
    res = {"torch.sum": o0 + sc * X.sum(0)}
    if M <= 4096:
        res["sequential"] = o0 + sc * _seq(X)
        res["reversed"] = sc * _seq(X.flip(0)) + o0
    ys, per = col_sum_geometry(M)                       # per block: four strided partials, their sum, scaled, added to out
    per4 = (per + 3) // 4 * 4
    Xp = torch.zeros(ys * per, C)
    Xp[:M] = X
    Xb = torch.zeros(ys, per4, C)
    Xb[:, :per] = Xp.view(ys, per, C)
    w = torch.zeros(ys, 4, C)
    for i in range(per4 // 4):
        w = w + Xb[:, 4 * i:4 * i + 4]
    part = sc * (((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3])
    for name, order in (("blocks in order", part), ("blocks reversed", part.flip(0))):
        o = o0.clone()
        for b_ in order:
            o = o + b_
        res[name] = o
    return {k: dict(out=v) for k, v in res.items()}


def _m_col_sum_last_row_block_dropped(p):
    M = p.case.M
    _, per = col_sum_geometry(M)
    last = (M - 1) // per * per                         # first row of the last block that holds rows
    return dict(out=_expect_col_sum(p, rows=last)["out"].image()) if last > 0 else None


def _m_col_sum_overwrites(p):
    return dict(out=_expect_col_sum(p, mut="overwrite")["out"].image())


def _m_col_sum_without_scale(p):
    return dict(out=_expect_col_sum(p, mut="no_scale")["out"].image()) if p.case.scale != 1.0 else None


# ==================================================================================================================== sum_n
SumNCase = namedtuple("SumNCase", "n count acc dup")
SUM_N_BIG = SumNCase(2, 4 * (CAP + 1), 1, 0)
SUM_N_CASES = ([SumNCase(n, count, acc, 0) for n in (1, 2, 15, 16, 17, 32, 33) for count in (4, 1028) for acc in (0, 1)]
               + [SumNCase(17, 1028, 0, 1), SumNCase(2, 4, 1, 1), SUM_N_BIG])          # dup: the last entry is the first tensor again


def sum_n_sources(c):
    """The list as indices into the distinct tensors, and those: magnitudes 2^+-10 by turns."""
    k = c.n - 1 if (c.dup and c.n > 1) else c.n
    srcs = [_rand((c.count,), 91, c.n, c.count, t) * 2.0 ** (10 * (t % 3 - 1)) for t in range(k)]
    return list(range(k)) + ([0] if k < c.n else []), srcs


def ref_sum_n(srcs, out0, count, acc, skip=(), second_launch_overwrites=False):
    """out[0 .. count) = (acc ? out : 0) + sum_t src_t[0 .. count).  Returns (idx, ref, |out0| + sum |src|)."""
    s = out0[:count].double() if acc else torch.zeros(count, dtype=torch.float64)
    sa = s.abs()
    for t, x in enumerate(srcs):
        if second_launch_overwrites and t == 16:
            s = torch.zeros_like(s)
        if t not in skip:
            s = s + x[:count].double()
        sa = sa + x[:count].double().abs()
    return ar(count), s, sa


def sum_n_listorder(srcs, out0, count, acc):
    """fp32, the kernel's stated order: (acc ? out : +0.0) + src_0 + src_1 + ... left to right."""
    s = out0[:count].clone() if acc else torch.zeros(count)
    for x in srcs:
        s = s + x[:count]
    return s


def _build_sum_n(op, c):
    order, srcs = sum_n_sources(c)
    out = pattern(c.count + 4)
    if c.acc:
        out[:c.count] = _rand((c.count,), 92, c.n, c.count, mag=100.0)
    bufs = {f"src{t}": s for t, s in enumerate(srcs)}
    bufs["out"] = out
    return Prob(op, c, bufs, {}, dict(order=order))


def _sum_n_list(p):
    return [p.bufs[f"src{t}"] for t in p.arg["order"]]


def _expect_sum_n(p, **kw):
    idx, ref, sa = ref_sum_n(_sum_n_list(p), p.bufs["out"], p.case.count, p.case.acc, **kw)
    return dict(out=Out(p.bufs["out"], idx, ref, U24 * sa + TINY, "sum_n"))


def _twins_sum_n(p):
    c, L_ = p.case, _sum_n_list(p)
    o0 = p.bufs["out"][:c.count] if c.acc else torch.zeros(c.count)
    rev = torch.zeros(c.count)
    for x in reversed(L_):
        rev = rev + x
    return {"list order": dict(out=sum_n_listorder(L_, p.bufs["out"], c.count, c.acc)), "reversed": dict(out=rev + o0),
            "torch.sum": dict(out=torch.stack(L_).sum(0) + o0)}


def _m_sum_n_tensor_16_of_17_dropped(p):
    return dict(out=_expect_sum_n(p, skip=(16,))["out"].image()) if p.case.n == 17 else None


def _m_sum_n_second_launch_overwrites(p):
    return dict(out=_expect_sum_n(p, second_launch_overwrites=True)["out"].image()) if p.case.n > 16 else None


# ==================================================================================================================== axpby
AxpbyCase = namedtuple("AxpbyCase", "n a b")
AXPBY_BIG = AxpbyCase(CAP + 1, -0.37, 0.5)
AXPBY_CASES = [AxpbyCase(n, a, b) for n in (1, 255, 256, 257) for a, b in ((1.0, 1.0), (-0.37, 0.5), (2.0, 0.0))] + [AXPBY_BIG]


def ref_axpby(x, y0, a, b, n, reads_y=False):
    """y = a x + b y over n floats; b == 0: a x, whatever y held."""
    ax = f32(a) * x[:n].double()
    return ar(n), (ax if (b == 0.0 and not reads_y) else ax + f32(b) * y0[:n].double())


def _build_axpby(op, c):
    x = _rand((c.n,), 95, c.n)
    y = pattern(c.n)
    if c.b != 0.0:                                      # b y takes the sign of a x: nothing cancels, |ref| = |a x| + |b y|
        sgn = torch.where(x < 0, -1.0, 1.0) * (1.0 if c.a * c.b > 0 else -1.0)
        y = _rand((c.n,), 96, c.n, mag=2.0).abs() * sgn
    return Prob(op, c, dict(x=x, y=y))


def _expect_axpby(p, **kw):
    c = p.case
    idx, ref = ref_axpby(p.bufs["x"], p.bufs["y"], c.a, c.b, c.n, **kw)
    return dict(y=Out(p.bufs["y"], idx, ref, U24 * ref.abs() + TINY, "axpby"))


def _twins_axpby(p):
    c = p.case
    x, y = p.bufs["x"], p.bufs["y"]
    a, b = torch.tensor(c.a, dtype=torch.float32), torch.tensor(c.b, dtype=torch.float32)
    if c.b == 0.0:
        return {"a x": dict(y=x * a)}
    return {"b y + a x": dict(y=b * y + a * x), "fma(a, x, b y)": dict(y=_fma(a.expand_as(x), x, b * y)),
            "fma(b, y, a x)": dict(y=_fma(b.expand_as(y), y, a * x))}


def _m_axpby_b0_reads_y(p):
    return dict(y=_expect_axpby(p, reads_y=True)["y"].image()) if p.case.b == 0.0 else None


# ============================================================================================================ the tables
OPS = {
    "nchw_to_nhwc": (LAYOUT_CASES, _build_layout, _expect_layout, _twins_layout),
    "nhwc_to_nchw": (LAYOUT_CASES + [TRANSPOSE_CASE], _build_layout, _expect_layout, _twins_layout),
    "space_to_depth2": (S2D_CASES, _build_s2d, _expect_s2d, None),
    "im2col7": (IM2COL_CASES, _build_im2col, _expect_im2col, None),
    "col2im7": (COL2IM_CASES, _build_col2im, _expect_col2im, _twins_col2im),
    "flow_to_nhwc": (FLOW_TO_NHWC_CASES, _build_flow_to_nhwc, _expect_flow_to_nhwc, None),
    "nhwc_to_flow": (NHWC_TO_FLOW_CASES, _build_nhwc_to_flow, _expect_nhwc_to_flow, _twins_nhwc_to_flow),
    "relu_bwd": (RELU_CASES, _build_relu, _expect_relu, None),
    "gru_bwd1": (GRU_CASES, _build_gru1, _expect_gru1, _twins_gru1),
    "gru_bwd2": (GRU_CASES, _build_gru2, _expect_gru2, _twins_gru2),
    "col_sum": (COL_SUM_CASES, _build_col_sum, _expect_col_sum, _twins_col_sum),
    "sum_n": (SUM_N_CASES, _build_sum_n, _expect_sum_n, _twins_sum_n),
    "axpby": (AXPBY_CASES, _build_axpby, _expect_axpby, _twins_axpby),
}
BIG_CASES = {S2dCase(*S2D_BIG, 0), S2dCase(*S2D_BIG, 1), *IM2COL_BIG, RELU_BIG, GRU_BIG, COL_SUM_BIG, SUM_N_BIG, AXPBY_BIG}


def cases(op):
    return OPS[op][0]


def case_id(c):
    return "-".join(str(v) if v != "" else "_" for v in c)


def build(op, case):
    return OPS[op][1](op, case)


def expect(p):
    return OPS[p.op][2](p)


def twins(p):
    """{variant: {output: fp32 values at that output's idx}}; empty for an operation that only moves."""
    f = OPS[p.op][3]
    return f(p) if f else {}


MUTANTS = {
    "relu_bwd: >= instead of >": ("relu_bwd", _m_relu_ge),
    "relu_bwd: touches the tail columns": ("relu_bwd", _m_relu_touches_tail_columns),
    "im2col7: tap offset sign flipped on y": ("im2col7", _m_im2col_tap_sign_flipped),
    "im2col7: border taps clamped": ("im2col7", _m_im2col_border_clamped),
    "col2im7: tap offset sign flipped on y": ("col2im7", _m_col2im_tap_sign_flipped),
    "col2im7: border taps clamped": ("col2im7", _m_col2im_border_clamped),
    "gru_bwd1: without dhn2": ("gru_bwd1", _gru1_mutant("no_dhn2", "dhn2")),
    "gru_bwd1: z (1 - z) dropped": ("gru_bwd1", _gru1_mutant("no_zz")),
    "gru_bwd1: without dzr_sum": ("gru_bwd1", _gru1_mutant("no_sum", "sums")),
    "gru_bwd2: writes columns [0, hid)": ("gru_bwd2", _gru2_mutant("low_half")),
    "gru_bwd2: overwrites dh": ("gru_bwd2", _gru2_mutant("overwrite")),
    "col_sum: last row block dropped": ("col_sum", _m_col_sum_last_row_block_dropped),
    "col_sum: overwrites out": ("col_sum", _m_col_sum_overwrites),
    "col_sum: without scale": ("col_sum", _m_col_sum_without_scale),
    "sum_n: tensor 16 of 17 dropped": ("sum_n", _m_sum_n_tensor_16_of_17_dropped),
    "sum_n: second launch does not accumulate": ("sum_n", _m_sum_n_second_launch_overwrites),
    "axpby: b = 0 still reads y": ("axpby", _m_axpby_b0_reads_y),
    "nchw_to_nhwc: coff ignored": ("nchw_to_nhwc", _m_layout_coff_ignored),
    "nhwc_to_nchw: coff ignored": ("nhwc_to_nchw", _m_layout_coff_ignored),
    "nchw_to_nhwc: accumulate ignored": ("nchw_to_nhwc", _m_layout_accumulate_ignored),
    "nhwc_to_nchw: accumulate ignored": ("nhwc_to_nchw", _m_layout_accumulate_ignored),
    "space_to_depth2: sub's bits swapped": ("space_to_depth2", _m_s2d_sub_bits_swapped),
}

TWIN_WORST = dict(lay_acc=1.0, flow_acc=0.995, col2im=2.12, gru_dz=3.67, gru_dq=2.6, gru_dh=1.71, gru_sum=2.09, gru_dr=2.84, gru_dh2=1.96,
                  col_sum=4.43, sum_n=3.97, axpby=1.91)
LIMITS = dict(lay_acc=4.0, flow_acc=4.0, col2im=9.0, gru_dz=20.0, gru_dq=20.0, gru_dh=7.0, gru_sum=9.0, gru_dr=20.0, gru_dh2=8.0,
              col_sum=20.0, sum_n=20.0, axpby=8.0)


@functools.lru_cache(maxsize=None)
def twin_worst():
    """{limit key: the worst score any twin reaches on any case}."""
    worst = {}
    for op in OPS:
        for c in cases(op):
            p = build(op, c)
            outs = expect(p)
            for variant, res in twins(p).items():
                for name, vals in res.items():
                    o = outs[name]
                    w = score(o.image(vals.float()), o)
                    worst[o.key] = max(worst.get(o.key, 0.0), w)
    return worst
