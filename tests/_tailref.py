"""float64 restatements of the three kernel files every training step ends in -- csrc/upsample.hip (the convex 8x upsampler, its
backward and dflow gather, the bilinear x8 pair), csrc/loss.hip (sequence_loss_kernel) and csrc/optim.hip (adamw_prepare_kernel,
adamw_flat_kernel) -- with the inputs that make their routes visible, fp32 twins, mutants and analytic error scales
(tests/test_tailref.py on the CPU, tests/test_tail_kernels.py against the kernels).  Plain torch on the CPU.  Every restatement
is written from the formula in its kernel file's header and the reference lines cited there (pytorch/core/raft.py:72-83,
core/utils/utils.py:80-82, pytorch/train.py:60-96, 137, 280-282).

Comparator.  `need(got, ref, scale, slack)` is the worst  max(0, |got - ref| - slack_i) / scale_i  over the elements in float64;
a comparison passes when that number is at most its entry of LIMITS.  u = 2^-24; every scale is elementwise.
  up          p_k the softmax over the nine taps, f_k the zero-padded neighbours of the flow:  u sum_k p_k |8 f_k|, every product
              and add of the weighted sum.  Slack: the exponent of tap k is rounded twice (m_k - max and its product with log2 e),
              each worth u (max - m_k) relative, doubled as in _gmaref: sum_k (4 (max - m_k) u p_k + 2^-126) |8 f_k|.
  dmask       p_k (dp_k - sum_j p_j dp_j) with dp_k = sum_c dup_c 8 f_ck:  u p_k (|dp_k| + sum_j p_j |dp_j|); the slack is the
              same exponent term carried through:  e_k |dp_k - dot| + p_k sum_j e_j |dp_j| + 2^-126,  e_k = 4 (max - m_k) u p_k + 2^-126
              (the last 2^-126: a product of two underflowing taps is below fp32's range altogether).
  dflow       8 sum over the nine neighbours and their 64 sub-pixels of p dup:  u 8 sum p |dup| over those 9 x 64 terms.
  upflow8     8 sum of four weights times four values:  u 8 sum w |f|.  The kernels form the source coordinate sy * Y in fp32
              (sy itself a rounded quotient): 2 u fy absolute, which moves the row weight by as much and the result by that times
              the difference of the two rows:  8 * 2u (fy |f[y1] - f[y0]| + fx |f[x1] - f[x0]|), each difference interpolated along
              the other axis.  At a node (fy an integer in float64) the fp32 coordinate may fall short of it, so the interval
              below counts as well.
  upflow8 bwd u 8 sum w |dup| over the fine pixels whose stencil holds the coarse pixel; slack 8 * 2u sum fy w_x |dup| (and
              the same along x) over the fine pixels whose row pair (at a node: row triple) holds the coarse row.
  loss        u (|out0| + sum_i w_i sum_pixels mask (s0 + s1) / numel): a sum of positive terms (out0: what `out` held before)
  epe sum     u (|out0| + sum epe)
  counts      exact (integers below 2^24)
  dpred       u |ref|: w / numel * d / sqrt(d^2 + eps^2) is a chain of correctly rounded operations on an exact d
  AdamW g     the fp32 product g * coef, bit for bit, with coef as the kernel left it in its state
  AdamW m, v  u (|old| + |ref|): m + (1 - b1) (g - m), b2 v + (1 - b2) g^2
  AdamW p     u (|p| + |update|), update = step_size m / (sqrt(v) inv_sqrt_bias2 + eps)
  AdamW state u |ref| for coef, step_size, inv_sqrt_bias2, decay; the step count is exact

Thresholds (the loss mask, the EPE counts) are decided in fp32 by the kernel and in float64 here.  The inputs keep every epe at
least 1e-3 off 1, 3, 5, every |gt| off max_flow and every valid off 0.5 -- except the designed pixels, whose values are small
integers, so that fp32 and float64 agree exactly: d = (0, 1), (0, 3), (3, 4); gt = (240, 320) under max_flow = 400; valid = 0.5.
tests/test_tailref.py asserts this on every case, so no comparison needs an exclusion.

LIMITS are 4 x the worst value the fp32 TWIN of a restatement (the same formula, every operation rounded to fp32, in an order that
is not the kernel's: separable interpolation matrices, torch.sum, the b1 m + (1 - b1) g form of the moment) reaches against float64
over the case lists below, rounded up to one significant digit (TWIN_WORST).  The kernels' own worst values are in
tests/test_tail_kernels.py and profiles/tail_kernel_margins.txt; they do not set the limits.  test_tailref.py proves every limit
at most a quarter of what each mutant produces on every case it reaches at all.  Where the two rules met, the inputs gave way,
not the limit: see flow_values, adamw_grad and ADAMW_LRS.
"""
import math

import torch

U24 = 2.0 ** -24
TINY = 2.0 ** -126
LOSS_EPS = 1e-3
MAX_FLOW = 400.0

# ------------------------------------------------------------------------------------------------------------------ case lists
UP_CASES = ((1, 1, 1), (1, 1, 17), (2, 2, 15), (1, 3, 16), (2, 3, 17), (1, 2, 33), (1, 2, 7), (1, 2, 8), (1, 2, 9))   # N, H, W
UP_LAYOUTS = ("planar", "planar_gap", "interleaved", "interleaved_wide")
UP_MASKS = ("gaussian", "dominant", "equal", "offset")
UPFLOW_CASES = ((1, 1, 1, 1), (1, 2, 1, 5), (2, 2, 4, 1), (1, 2, 2, 2), (2, 2, 5, 7), (1, 3, 9, 33))                   # N, C, H, W
LOSS_SMALL = ((1, 1, 1, 1), (1, 3, 85, 3), (1, 16, 16, 3), (1, 257, 1, 3), (2, 5, 7, 32))                              # B, H, W, n
LOSS_BIG = (1, 513, 1024, 2)
LOSS_CASES = LOSS_SMALL + (LOSS_BIG,)
ADAMW_SMALL = (1, 3, 4, 5, 63, 64, 65, 1027)
ADAMW_BIG = (4194304, 4194308, 4194311)
ADAMW_N = ADAMW_SMALL + ADAMW_BIG
ADAMW_NORMS = ("none", "below", "above", "zero")
ADAMW_SKIP_N = (1027, 4194311)
ADAMW_SKIPS = ("first", "last_full", "tail", "all_three")
BETAS, ADAM_EPS, MAX_NORM = (0.9, 0.999), 1e-8, 1.0
# the learning rate changes between the three steps.  It is large so that lr * wd >= 1e-3 of an update shows next to u |p| (the
# `decay after the update` mutant, on every case down to n = 1); the formula does not care
ADAMW_LRS = (0.2, 0.1, 0.3)
INF = float("inf")
# (n, norm, wd, skip table, first step)
ADAMW_RUNS = (tuple((n, ADAMW_NORMS[i % 4], (0.0, 1e-2)[i % 2], None, 0) for i, n in enumerate(ADAMW_SMALL))
              + tuple((1027, k, 1e-2, None, 0) for k in ADAMW_NORMS[:3])
              + tuple((1027, "above", 1e-2, s, 0) for s in ADAMW_SKIPS)
              + ((65, "above", 1e-2, None, 999), (1027, "below", 0.0, None, 99999))
              + ((4194304, "above", 1e-2, None, 0), (4194308, "none", 0.0, None, 0), (4194311, "zero", 1e-2, None, 0))
              + tuple((4194311, "above", 1e-2, s, 0) for s in ADAMW_SKIPS))
# (case, live dpred: all / mid_null / none, gt given, valid given, metric_idx, max_flow, mode).  mode `prefilled`: out holds sums
# already; `semi`: the two launches of train._SemiLossFn on buffers of 2B samples -- the first half as the row says into out, the
# second half against its own last prediction (gt = pred[n - 1] + half a batch, valid null, max_flow inf) into out + 6
LOSS_RUNS = (((1, 1, 1, 1), "all", True, True, 0, MAX_FLOW, "plain"),
             ((1, 1, 1, 1), "none", False, False, -1, INF, "plain"),
             ((1, 3, 85, 3), "all", True, True, 2, MAX_FLOW, "plain"),
             ((1, 3, 85, 3), "mid_null", True, True, 0, MAX_FLOW, "prefilled"),
             ((1, 3, 85, 3), "all", True, False, 3, MAX_FLOW, "plain"),
             ((1, 16, 16, 3), "none", True, True, 2, MAX_FLOW, "plain"),
             ((1, 16, 16, 3), "all", False, True, -1, MAX_FLOW, "plain"),
             ((1, 16, 16, 3), "all", True, True, 0, INF, "prefilled"),
             ((1, 257, 1, 3), "all", True, True, -1, MAX_FLOW, "semi"),
             ((1, 257, 1, 3), "mid_null", False, False, 2, MAX_FLOW, "plain"),
             ((2, 5, 7, 32), "all", True, True, 31, MAX_FLOW, "plain"),
             ((2, 5, 7, 32), "mid_null", True, True, 32, MAX_FLOW, "semi"),
             ((2, 5, 7, 32), "none", True, False, 0, INF, "plain"),
             (LOSS_BIG, "all", True, True, 1, MAX_FLOW, "plain"))
OUT0 = (0.25, 3.0, 2.0, 5.0, 7.0, 11.0)                # what a prefilled `out` holds

TWIN_WORST = dict(up=4.1, dmask=5.4, dflow=1.14, upflow8=1.47, upflow8_bwd=0.63, loss=2.25, epe=1.4, dpred=3.66,
                  adam_mv=5.4, adam_p=6.0, adam_state=1.31)
LIMITS = dict(up=20.0, dmask=30.0, dflow=5.0, upflow8=6.0, upflow8_bwd=3.0, loss=9.0, epe=6.0, dpred=20.0,
              adam_mv=30.0, adam_p=30.0, adam_state=6.0)


def limit_from_twin(worst):
    """4 x the twin's worst, rounded up to one significant digit."""
    v = 4.0 * worst
    p = 10.0 ** math.floor(math.log10(v))
    return math.ceil(v / p - 1e-9) * p


def need(got, ref, scale, slack=0.0):
    """(worst max(0, |got - ref| - slack) / scale, flat index of it); inf for a non-finite value or an excess where scale is 0."""
    got = got.double()
    ex = ((got - ref).abs() - slack).clamp_min(0)
    r = torch.where(ex == 0, torch.zeros_like(ex), ex / scale)
    r = torch.where(torch.isfinite(got) & ~torch.isnan(r), r, torch.full_like(r, float("inf")))
    i = int(r.argmax())
    return float(r.reshape(-1)[i]), i


def _gen(*key):
    s = 0
    for k in key:
        s = (s * 1000003 + int(k) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


# ============================================================================================================ convex upsampler
def flow_values(N, H, W):
    """[N, 2, H, W] fp32, distinct per (n, c, y, x), none zero.  The two channels share their sign at every pixel, and so do the
    two of dup_values: dp_k = dup_0 8 f_0k + dup_1 8 f_1k then never cancels.  Its own rounding, u (|dup_0 8 f_0k| + |dup_1 8 f_1k|),
    is a term the dmask scale -- which has |dp_k| -- does not hold."""
    f = 2.0 * torch.randn(N, 2, H, W, generator=_gen(1, N, H, W))
    f = torch.where(f.abs() < 0.05, f + 0.5, f)
    f[:, 1] = f[:, 1].abs() * f[:, 0].sign()
    return f


def mask_plane(kind, N, H, W):
    """[N, H, W, 576] fp32, channel k * 64 + sy * 8 + sx."""
    m = 1.5 * torch.randn(N, H, W, 9, 64, generator=_gen(2, N, H, W, UP_MASKS.index(kind)))
    k = torch.arange(64) % 9
    pick = torch.zeros(9, 64, dtype=torch.bool)
    pick[k, torch.arange(64)] = True                    # tap (sy * 8 + sx) % 9 of every sub-pixel
    if kind == "dominant":
        m = torch.where(pick, m.amax(3, keepdim=True) + 60.0, m)
    elif kind == "equal":
        m = m[:, :, :, :1].expand(N, H, W, 9, 64).clone()
    elif kind == "offset":
        m = torch.where(pick, torch.full_like(m, -1e4), m + 1e4)
    return m.reshape(N, H, W, 576).contiguous()


def dup_values(N, H, W):
    g = torch.randn(N, 2, 8 * H, 8 * W, generator=_gen(3, N, H, W))
    g[:, 1] = g[:, 1].abs() * torch.where(g[:, 0] < 0, -1.0, 1.0)
    return g


def _taps(flow, mut=""):
    """[N, 2, 9, H, W] float64: 8 * flow at (y + ky - 1, x + kx - 1), zero outside."""
    f = 8.0 * flow.double()
    N, _, H, W = f.shape
    out = torch.zeros(N, 2, 9, H, W, dtype=torch.float64)
    ys, xs = torch.arange(H), torch.arange(W)
    for k in range(9):
        ky, kx = (k % 3, k // 3) if mut == "kswap" else (k // 3, k % 3)
        yy, xx = ys + ky - 1, xs + kx - 1
        if mut == "clamp":
            out[:, :, k] = f[:, :, yy.clamp(0, H - 1)][:, :, :, xx.clamp(0, W - 1)]
            continue
        oky, okx = (yy >= 0) & (yy < H), (xx >= 0) & (xx < W)
        if oky.any() and okx.any():
            out[:, :, k][:, :, oky.nonzero()[:, 0][:, None], okx.nonzero()[:, 0][None, :]] = f[:, :, yy[oky]][:, :, :, xx[okx]]
    return out


def _softmax9(mask_nhwc, mut="", dtype=torch.float64):
    """(p, max - m) as [N, H, W, 9, 8, 8]."""
    N, H, W, _ = mask_nhwc.shape
    m = mask_nhwc.to(dtype).view(N, H, W, 9, 8, 8)
    mx = m.amax(3, keepdim=True)
    e = torch.exp(m if mut == "nomax" else m - mx)
    return e / e.sum(3, keepdim=True), (mx - m).double()


def upsample_ref(flow, mask_nhwc, mut=""):
    """up [N, 2, 8H, 8W]: up[n, c, 8y + sy, 8x + sx] = sum_k p_k[n, y, x, sy, sx] * 8 flow[n, c, y + ky - 1, x + kx - 1]."""
    N, _, H, W = flow.shape
    p, _ = _softmax9(mask_nhwc, mut)
    t = _taps(flow, mut)
    return torch.einsum("nyxkab,nckyx->ncybxa" if mut == "sswap" else "nyxkab,nckyx->ncyaxb", p, t).reshape(N, 2, 8 * H, 8 * W)


def _gather9(T, mut=""):
    """sum_k T[n, c, k, y - (ky - 1), x - (kx - 1)], zero outside."""
    N, C, _, H, W = T.shape
    out = torch.zeros(N, C, H, W, dtype=T.dtype)
    sgn = 1 if mut == "gather_plus" else -1
    for k in range(9):
        dy, dx = sgn * (k // 3 - 1), sgn * (k % 3 - 1)
        for y in range(H):
            if not 0 <= y + dy < H:
                continue
            x0, x1 = max(0, -dx), min(W, W - dx)
            if x1 > x0:
                out[:, :, y, x0:x1] += T[:, :, k, y + dy, x0 + dx:x1 + dx]
    return out


def upsample_bwd_ref(flow, mask_nhwc, dup, mut=""):
    """(dmask_nhwc, dflow) in closed form."""
    N, _, H, W = flow.shape
    p, _ = _softmax9(mask_nhwc, mut)
    t = _taps(flow, mut)
    g = dup.double().view(N, 2, H, 8, W, 8)
    dp = torch.einsum("ncyaxb,nckyx->nyxkab", g, t)
    dot = (p * dp).sum(3, keepdim=True)
    T = torch.einsum("nyxkab,ncyaxb->nckyx", p, g)
    return (p * (dp - dot)).reshape(N, H, W, 576), 8.0 * _gather9(T, mut)


def upsample_twin(flow, mask_nhwc):
    N, _, H, W = flow.shape
    p, _ = _softmax9(mask_nhwc, "", torch.float32)
    t = _taps(flow).float()                             # (the product by 8 is exact in either precision)
    up = torch.zeros(N, 2, H, 8, W, 8)
    for k in reversed(range(9)):                        # taps added last to first
        up = up + p[:, :, :, k].permute(0, 1, 3, 2, 4)[:, None] * t[:, :, k][:, :, :, None, :, None]
    return up.reshape(N, 2, 8 * H, 8 * W)


def upsample_bwd_twin(flow, mask_nhwc, dup):
    N, _, H, W = flow.shape
    p, _ = _softmax9(mask_nhwc, "", torch.float32)
    t = _taps(flow).float()
    g = dup.float().view(N, 2, H, 8, W, 8).permute(0, 1, 2, 4, 3, 5)          # n c y x a b
    dp = g[:, 1][:, :, :, None] * t[:, 1].permute(0, 2, 3, 1)[..., None, None] + g[:, 0][:, :, :, None] * t[:, 0].permute(0, 2, 3, 1)[..., None, None]
    dot = (p * dp).sum(3, keepdim=True)
    T = (p[:, None] * g[:, :, :, :, None]).reshape(N, 2, H, W, 9, 64).sum(-1).permute(0, 1, 4, 2, 3)
    return (p * (dp - dot)).reshape(N, H, W, 576), 8.0 * _gather9(T.contiguous())


def upsample_expect(flow, mask_nhwc, dup):
    """{name: (ref, scale, slack, limit key)} for up, dmask, dflow."""
    N, _, H, W = flow.shape
    p, d = _softmax9(mask_nhwc)
    t = _taps(flow)
    e = 4.0 * d * U24 * p + TINY
    g = dup.double().view(N, 2, H, 8, W, 8)
    up = upsample_ref(flow, mask_nhwc)
    dmask, dflow = upsample_bwd_ref(flow, mask_nhwc, dup)

    def shuffle(a):
        return a.reshape(N, 2, 8 * H, 8 * W)
    s_up = U24 * shuffle(torch.einsum("nyxkab,nckyx->ncyaxb", p, t.abs()))
    k_up = shuffle(torch.einsum("nyxkab,nckyx->ncyaxb", e, t.abs()))
    dp = torch.einsum("ncyaxb,nckyx->nyxkab", g, t)
    dot = (p * dp).sum(3, keepdim=True)
    s_dm = U24 * p * (dp.abs() + (p * dp.abs()).sum(3, keepdim=True))
    k_dm = e * (dp - dot).abs() + p * (e * dp.abs()).sum(3, keepdim=True) + TINY        # (+ 2^-126: a result below fp32's normal range)
    Tabs = torch.einsum("nyxkab,ncyaxb->nckyx", p, g.abs())
    return dict(up=(up, s_up, k_up, "up"), dmask=(dmask, s_dm.reshape(N, H, W, 576), k_dm.reshape(N, H, W, 576), "dmask"),
                dflow=(dflow, U24 * 8.0 * _gather9(Tabs), 0.0, "dflow"))


# ================================================================================================================== bilinear x8
def _axis(n, mut="", dtype=torch.float64):
    """Along one axis of n source nodes: (A [8n, n] the interpolation weights, S [8n, n] 1 where a node's weight depends on the
    fine coordinate, f [8n] the coordinate)."""
    n8 = 8 * n
    Y = torch.arange(n8, dtype=dtype)
    if mut == "half":
        f = Y * n / n8
    else:
        s = torch.tensor(n - 1, dtype=dtype) / torch.tensor(n8 - 1, dtype=dtype) if n8 > 1 else torch.tensor(0.0, dtype=dtype)
        f = s * Y
    y0 = f.floor().long().clamp(0, n - 1)
    y1 = (y0 + 1).clamp_max(n - 1)
    l = f - y0
    A = torch.zeros(n8, n, dtype=dtype)
    r = torch.arange(n8)
    A[r, y0] += 1 - l
    A[r, y1] += l
    S = torch.zeros(n8, n, dtype=torch.float64)
    S[r, y0] = 1
    S[r, y1] = 1
    node = l == 0
    S[r[node], (y0[node] - 1).clamp_min(0)] = 1
    return A, S, f.double()


def upflow8_ref(flow, mut=""):
    """8 * bilinear(flow, align_corners=True): scale (H - 1) / (8H - 1); all rows on source row 0 when H == 1."""
    H, W = flow.shape[2:]
    if mut == "one_is_zero" and (H == 1 or W == 1):
        return torch.zeros(flow.shape[:2] + (8 * H, 8 * W), dtype=torch.float64)
    Ay, Ax = _axis(H, mut)[0], _axis(W, mut)[0]
    return 8.0 * (Ay @ flow.double() @ Ax.T)


def upflow8_bwd_ref(dup, mut=""):
    H, W = dup.shape[2] // 8, dup.shape[3] // 8
    if mut == "one_is_zero" and (H == 1 or W == 1):
        return torch.zeros(dup.shape[:2] + (H, W), dtype=torch.float64)
    Ay, Ax = _axis(H, mut)[0], _axis(W, mut)[0]
    return 8.0 * (Ay.T @ dup.double() @ Ax)


def upflow8_twin(flow):
    H, W = flow.shape[2:]
    Ay, Ax = _axis(H, "", torch.float32)[0], _axis(W, "", torch.float32)[0]
    return 8.0 * (Ay @ (flow.float() @ Ax.T))


def upflow8_bwd_twin(dup):
    H, W = dup.shape[2] // 8, dup.shape[3] // 8
    Ay, Ax = _axis(H, "", torch.float32)[0], _axis(W, "", torch.float32)[0]
    return 8.0 * ((Ay.T @ dup.float()) @ Ax)


def _pair_diff(n):
    """[8n, n] rows f[y1] - f[y0] (at a node: also the interval below, stacked as a second matrix)."""
    A, S, f = _axis(n)
    n8 = 8 * n
    y0 = f.floor().long().clamp(0, n - 1)
    r = torch.arange(n8)
    D1 = torch.zeros(n8, n, dtype=torch.float64)
    D1[r, (y0 + 1).clamp_max(n - 1)] += 1
    D1[r, y0] -= 1
    D0 = torch.zeros(n8, n, dtype=torch.float64)
    node = (f - y0) == 0
    D0[r[node], y0[node]] += 1
    D0[r[node], (y0[node] - 1).clamp_min(0)] -= 1
    return D1, D0


def upflow8_expect(flow, dup):
    """{name: (ref, scale, slack, limit key)} for up and dflow."""
    H, W = flow.shape[2:]
    f, g = flow.double(), dup.double()
    (Ay, Sy, fy), (Ax, Sx, fx) = _axis(H), _axis(W)
    up, dflow = upflow8_ref(flow), upflow8_bwd_ref(dup)
    s_up = U24 * 8.0 * (Ay @ f.abs() @ Ax.T)
    Dy1, Dy0 = _pair_diff(H)
    Dx1, Dx0 = _pair_diff(W)
    ky = torch.maximum((Dy1 @ f).abs(), (Dy0 @ f).abs()) @ Ax.T * fy.view(-1, 1)
    kx = Ay @ torch.maximum((f @ Dx1.T).abs(), (f @ Dx0.T).abs()) * fx.view(1, -1)
    s_d = U24 * 8.0 * (Ay.T @ g.abs() @ Ax)
    k_d = (Sy * fy.view(-1, 1)).T @ g.abs() @ Ax + Ay.T @ g.abs() @ (Sx * fx.view(-1, 1))
    return dict(up=(up, s_up, 8.0 * 2 * U24 * (ky + kx), "upflow8"), dflow=(dflow, s_d, 8.0 * 2 * U24 * k_d, "upflow8_bwd"))


def upflow8_inputs(N, C, H, W):
    g = _gen(4, N, C, H, W)
    return 2.0 * torch.randn(N, C, H, W, generator=g), torch.randn(N, C, 8 * H, 8 * W, generator=g)


# ================================================================================================================ sequence loss
DESIGNED_D = ((0.0, 1.0), (0.0, 3.0), (3.0, 4.0))


def live_list(kind, n):
    return [kind == "all" or (kind == "mid_null" and i != n // 2) for i in range(n)]


def loss_inputs(B, H, W, n, alias=False):
    """(preds [n][B, 2, H, W], gt, valid [B, H, W], w [n]) fp32.  With at least 8 pixels, sample 0 holds the designed pixels
    0 .. 5: d = (0, 1), (0, 3), (3, 4) on every prediction, gt = (240, 320), valid = 0.5, gt = (500, 0).  alias: gt is the last
    prediction (train._SemiLossFn's second launch)."""
    g = _gen(5, B, H, W, n, alias)
    HW = H * W
    gt = 4.0 * torch.randn(B, 2, HW, generator=g)
    valid = (torch.rand(B, HW, generator=g) > 0.2).float()
    noise = [3.0 * torch.randn(B, 2, HW, generator=g) for _ in range(n)]
    designed = HW >= 8
    if designed:
        gt[0, :, :6] = torch.tensor([[2.0, -3.0, 1.0, 240.0, 5.0, 500.0], [-1.0, 4.0, 2.0, 320.0, -6.0, 0.0]])
        valid[0, :6] = torch.tensor([1.0, 1.0, 1.0, 1.0, 0.5, 1.0])
        for d in noise:
            for j, (d0, d1) in enumerate(DESIGNED_D):
                d[0, 0, j], d[0, 1, j] = d0, d1
            d[0, :, 3:6] = d[0, :, 3:6].round()
    preds = [gt + d for d in noise]
    if alias:
        gt = preds[-1].clone()
    for i, p in enumerate(preds):                       # no epe within 2e-3 of a threshold, the designed pixels apart
        d = p - gt
        epe = d.double().pow(2).sum(1, keepdim=True).sqrt()
        near = ((epe - 1).abs() < 2e-3) | ((epe - 3).abs() < 2e-3) | ((epe - 5).abs() < 2e-3)
        if designed:
            near[0, :, :3] = False
        preds[i] = torch.where(near, gt + 1.01 * d, p)
    w = torch.tensor([0.8 ** (n - i - 1) for i in range(n)], dtype=torch.float32)
    return [p.view(B, 2, H, W) for p in preds], gt.view(B, 2, H, W), valid.view(B, H, W), w


def seqloss_ref(preds, dmask_of_live, w, metric_idx, gt, valid, max_flow, eps, out0=None, mut="", dtype=torch.float64):
    """(out [6] = out0 + (loss, epe sum, n(<1), n(<3), n(<5), n valid), dpred list with None for a dead entry).
    loss = sum_i w_i mean(mask sqrt((p_i - gt)^2 + eps^2)), mask = valid >= 0.5 and |gt| < max_flow; the statistics of prediction
    metric_idx (none outside [0, n)) under valid > 0.5.  dtype float32: the twin."""
    B, _, H, W = preds[0].shape
    n = len(preds)
    g = gt.to(dtype) if gt is not None else torch.zeros(B, 2, H, W, dtype=dtype)
    v = valid.to(dtype) if valid is not None else torch.ones(B, H, W, dtype=dtype)
    mag = (g[:, 0] ** 2 + g[:, 1] ** 2).sqrt()
    mask = ((v > 0.5) if mut == "valid_gt" else (v >= 0.5)) & ((mag <= max_flow) if mut == "le" else (mag < max_flow))
    smask = mask if mut == "stats_lossmask" else v > 0.5
    numel = 1.0 if mut == "no_numel" else float(B * 2 * H * W)
    e2 = eps if mut == "eps" else eps * eps
    out = torch.zeros(6, dtype=dtype) if out0 is None else out0.to(dtype).clone()
    dps = []
    for i in range(n):
        d = preds[i].to(dtype) - g
        s = (d * d + e2).sqrt()
        wi = w[i].to(dtype)
        out[0] += wi * (s * mask[:, None]).sum() / numel
        dps.append(wi / numel * mask[:, None] * d / s if dmask_of_live[i] else None)
        if i == metric_idx:
            epe = (d[:, 0] ** 2 + d[:, 1] ** 2).sqrt()
            out[1] += (epe * smask).sum()
            out[2] += ((epe < 1) & smask).sum()
            out[3] += ((epe < 3) & smask).sum()
            out[4] += ((epe < 5) & smask).sum()
            out[5] += smask.sum()
    return out, dps


def seqloss_expect(preds, dmask_of_live, w, metric_idx, gt, valid, max_flow, eps, out0=None):
    """{out: (ref [6], scale [6], 0, keys [6]), dpred: [(ref, scale, 0, key) or None]}; the counts have scale 0: exact."""
    out, dps = seqloss_ref(preds, dmask_of_live, w, metric_idx, gt, valid, max_flow, eps, out0)
    base, _ = seqloss_ref(preds, dmask_of_live, w, metric_idx, gt, valid, max_flow, eps, None)
    o0 = torch.zeros(6, dtype=torch.float64) if out0 is None else out0.double().abs()
    scale = torch.zeros(6, dtype=torch.float64)
    scale[0], scale[1] = U24 * (o0[0] + base[0]), U24 * (o0[1] + base[1])
    return dict(out=(out, scale), dpred=[(d, U24 * d.abs(), 0.0, "dpred") if d is not None else None for d in dps])


def loss_conditions(preds, gt, valid, max_flow):
    """The worst offences against the three input conditions: (epe, |gt|, valid) distances below 1e-3 that are not exactly 0."""
    bad = 0
    g = gt.double() if gt is not None else torch.zeros_like(preds[0], dtype=torch.float64)
    for p in preds:
        d = p.double() - g
        epe = (d[:, 0] ** 2 + d[:, 1] ** 2).sqrt()
        for t in (1.0, 3.0, 5.0):
            off = (epe - t).abs()
            bad += int(((off < 1e-3) & (off != 0)).sum())
    if math.isfinite(max_flow):
        off = ((g[:, 0] ** 2 + g[:, 1] ** 2).sqrt() - max_flow).abs()
        bad += int(((off < 1e-3) & (off != 0)).sum())
    if valid is not None:
        off = (valid.double() - 0.5).abs()
        bad += int(((off < 1e-3) & (off != 0)).sum())
    return bad


# ======================================================================================================================== AdamW
def adamw_inputs(n):
    """p, g, m, v fp32 [n] of a first step: |p| >= 0.05, zero moments."""
    gen = _gen(6, n)
    p = torch.randn(n, generator=gen)
    p = torch.where(p.abs() < 0.05, p.sign() * 0.05 + p, p)
    p = torch.where(p == 0, torch.full_like(p, 0.07), p)
    return p, 0.3 * torch.randn(n, generator=gen), torch.zeros(n), torch.zeros(n)


def adamw_grad(n, k):
    """The gradient of step k (0, 1, 2): fresh every step, as a training step's is, with the sign of step 0's in every element.
    m + (1 - b1) (g - m) then never cancels: a moment that lost its leading digits carries an error of u |old| into the update,
    which the scale of p -- u (|p| + |update|) -- does not hold."""
    g0 = 0.3 * torch.randn(n, generator=_gen(7, n, 0))
    if k == 0:
        return g0
    return (0.3 * torch.randn(n, generator=_gen(7, n, k))).abs() * torch.where(g0 < 0, -1.0, 1.0)


def adamw_norm(kind, g):
    """The fp32 scalar handed in as the gradient norm (None: no clipping)."""
    if kind == "none":
        return None
    if kind == "zero":
        return torch.zeros(())
    nrm = g.double().norm().float()
    return nrm if kind == "above" else torch.minimum(nrm, torch.tensor(0.5))


def adamw_norm_for(kind, g):
    """'above': the true norm if it exceeds MAX_NORM, else 2.5 (short buffers)."""
    nrm = adamw_norm(kind, g)
    if kind == "above" and float(nrm) <= MAX_NORM:
        return torch.tensor(2.5)
    return nrm


def skip_table(kind, n):
    """uint8 [ceil(n / 64)]: the first block, the last full block, the block holding the n & 3 tail, or all three."""
    nb = (n + 63) // 64
    t = torch.zeros(nb, dtype=torch.uint8)
    first, last_full, tail = 0, n // 64 - 1, (n // 4 * 4) // 64
    for name, b in (("first", first), ("last_full", last_full), ("tail", tail)):
        if kind in (name, "all_three"):
            t[b] = 1
    return t


def _keep(skip64, n):
    if skip64 is None:
        return torch.zeros(n, dtype=torch.bool)
    return skip64.bool().repeat_interleave(64)[:n]


def adamw_ref(p, g, m, v, step, norm, max_norm, lr, betas, eps, wd, skip64=None, mut=""):
    """One step of clip_grad_norm_ + torch.optim.AdamW on flat buffers, float64, from the double hyper-parameters:
    (p, g, m, v, step, (coef, step_size, inv_sqrt_bias2, decay), update).  A skipped 64-block is returned unchanged."""
    p0, g0, m0, v0 = (t.double() for t in (p, g, m, v))
    b1, b2 = betas
    t = float(step) + 1.0
    coef = 1.0
    if norm is not None:
        coef = max_norm / (float(norm) + 1e-6)
        coef = coef if (coef < 1.0 or mut == "no_clamp") else 1.0
    tc = t - 1.0 if mut == "t-1" else t
    bias1, bias2 = 1.0 - b1 ** tc, 1.0 - b2 ** tc
    step_size = lr / bias1 if bias1 else float("inf")
    isb2 = 1.0 / math.sqrt(bias2) if bias2 else float("inf")
    decay = 1.0 - lr * wd
    g1 = g0 * coef
    m1 = m0 + (1.0 - b1) * (g1 - m0)
    gv = g0 if mut == "v_unclipped" else g1
    v1 = b2 * v0 + (1.0 - b2) * gv * gv
    upd = step_size * m1 / (v1.sqrt() * isb2 + eps)
    p1 = (p0 - upd) * decay if mut == "decay_after" else p0 * decay - upd
    keep = _keep(skip64, p0.numel())
    pk = p0 * decay if mut == "skip_decays" else p0
    p1, g1, m1, v1 = torch.where(keep, pk, p1), torch.where(keep, g0, g1), torch.where(keep, m0, m1), torch.where(keep, v0, v1)
    return p1, g1, m1, v1, t, (coef, step_size, isb2, decay), torch.where(keep, torch.zeros_like(upd), upd)


def adamw_twin(p, g, m, v, step, norm, max_norm, lr, betas, eps, wd, skip64=None):
    """The same step in fp32 (the corrections in double, as torch forms them), in torch's own order of operations."""
    f = torch.float32
    p0, g0, m0, v0 = (t.float() for t in (p, g, m, v))
    b1, b2 = betas
    t = float(step) + 1.0
    one = torch.ones((), dtype=f)
    coef = one
    if norm is not None:
        coef = torch.tensor(max_norm, dtype=f) / (norm.float() + torch.tensor(1e-6, dtype=f))
        coef = torch.minimum(coef, one)
    lr32, wd32, eps32 = (torch.tensor(x, dtype=f) for x in (lr, wd, eps))
    bias1, bias2 = torch.tensor(1.0 - b1 ** t, dtype=f), torch.tensor(1.0 - b2 ** t, dtype=f)
    step_size, isb2, decay = lr32 / bias1, one / bias2.sqrt(), one - lr32 * wd32
    g1 = g0 * coef
    m1 = m0 * torch.tensor(b1, dtype=f) + g1 * torch.tensor(1.0 - b1, dtype=f)
    v1 = g1 * g1 * torch.tensor(1.0 - b2, dtype=f) + v0 * torch.tensor(b2, dtype=f)
    p1 = p0 - p0 * (lr32 * wd32) - (step_size * m1) / (v1.sqrt() / bias2.sqrt() + eps32)
    keep = _keep(skip64, p0.numel())
    p1, g1, m1, v1 = torch.where(keep, p0, p1), torch.where(keep, g0, g1), torch.where(keep, m0, m1), torch.where(keep, v0, v1)
    return p1, g1, m1, v1, t, torch.stack([coef, step_size, isb2, decay])


def adamw_expect(p, g, m, v, step, norm, max_norm, lr, betas, eps, wd, skip64=None):
    """{name: (ref, scale, 0, limit key)} for p, m, v, state; g: the float64 product (the kernel test compares bits), step."""
    p1, g1, m1, v1, t, st, upd = adamw_ref(p, g, m, v, step, norm, max_norm, lr, betas, eps, wd, skip64)
    st = torch.tensor(st, dtype=torch.float64)
    return dict(p=(p1, U24 * (p.double().abs() + upd.abs()), 0.0, "adam_p"), m=(m1, U24 * (m.double().abs() + m1.abs()), 0.0, "adam_mv"),
                v=(v1, U24 * (v.double().abs() + v1.abs()), 0.0, "adam_mv"), state=(st, U24 * st.abs(), 0.0, "adam_state"),
                g=g1, step=t, keep=_keep(skip64, p.numel()))


# ============================================================================================================ runs, expanded
def loss_launches(run):
    """The launches of a LOSS_RUNS row: dicts of preds, gt, valid, live, w, metric, max_flow, out0 (`semi`: two of them, the second
    on the other half of the batch with gt its own last prediction)."""
    (B, H, W, n), live, has_gt, has_valid, metric, max_flow, mode = run
    preds, gt, valid, w = loss_inputs(B, H, W, n)
    first = dict(preds=preds, gt=gt if has_gt else None, valid=valid if has_valid else None, live=live_list(live, n), w=w,
                 metric=metric, max_flow=max_flow, out0=torch.tensor(OUT0) if mode == "prefilled" else None)
    if mode != "semi":
        return [first]
    p2, g2, _, w2 = loss_inputs(B, H, W, n, alias=True)
    assert torch.equal(g2, p2[-1])
    return [first, dict(preds=p2, gt=g2, valid=None, live=live_list(live, n), w=0.5 * w2, metric=-1, max_flow=INF, out0=None)]


def loss_expect_of(launch):
    a = launch
    return seqloss_expect(a["preds"], a["live"], a["w"], a["metric"], a["gt"], a["valid"], a["max_flow"], LOSS_EPS, a["out0"])


def adamw_step_setup(run, k):
    """(g, norm or None, lr, wd, skip table or None) of step k of an ADAMW_RUNS row."""
    n, norm_kind, wd, skip, _ = run
    g = adamw_grad(n, k)
    return g, adamw_norm_for(norm_kind, g), ADAMW_LRS[k], wd, (skip_table(skip, n) if skip else None)
