"""float64 restatements of the kernels of csrc/gma.hip (six row softmaxes, the `motion + gamma * agg` mix and its backward), the
inputs that make their loops visible, and an elementwise comparator whose limits every case proves on mutants
(tests/test_gmaref.py on the CPU, tests/test_gma_kernels.py against the kernels).  Plain torch on the CPU.

Comparator.  `need(got, ref, scale, slack)` is the worst  max(0, |got - ref| - slack_i) / scale_i  over the elements, in
float64; a comparison passes when that number is at most its entry of LIMITS.  Scales (u = 2^-24):
  softmax forward   scale_i = ref_i u, slack_i = 4 (max - x_i) ref_i u + 2^-126.  The limit `fwd_a` is the constant a of
                    |err_i| <= ref_i u (a + 4 (max - x_i)) + 2^-126: the exponent argument is rounded twice (x - m, and its
                    product with log2 e), each worth |x - m| u relative; that sum of 2 is doubled to 4.  2^-126: flushed denormals.
  softmax backward  scale_i = A_i (|dA_i| + sum_j |A_j dA_j|) u
  records           the same, with 2^-17 |ref_i| added to the slack: hi keeps 8 bits, the remainder is at most 2^-8 |x| and lo
                    keeps 8 bits of it, so a decoded value is within 2^-17 |x| (reached: 2^-17.003 on [1, 2)); no margin in it
  dst = x + g y     2^-23 (|x| + |g y|): one contraction to fma allowed.  Fixed (limit 1).
  dy = g d          torch's fp32 product, bit for bit
  dx += d           2^-24 |result| of the fp64 sum.  Fixed (limit 1).
  dgamma            u sum |d y|

LIMITS: fwd_a, bwd and rec_bwd are 4 x the worst value any case of the kernel's list reached on MI355X against these restatements,
rounded up to one significant digit (worst values: 6.6, 4.7, 0.53; tests/test_gma_kernels.py, profiles/gma_kernel_margins.txt).
dgamma is NOT 4 x the kernel's measured worst (0.088 -> 0.4): the fp32 twin, which rounds every product where the kernel's dot
products are contracted to fma, reaches 0.78 on the 7 x 4 case, and the comparator has to accept it.  The same rule is applied to
the twin's worst instead: 4 x 0.78, rounded up, 4.  (An fp32 evaluation guarantees no better than about 2.4 units on the 1 x 4 case:
u sum|d y| from the products and u |result| = 1.4 units from the final add.)
Every limit is at most a quarter of the smallest deviation any applicable mutant produces on the designed rows of any case
(test_gmaref.py, the *_twin_accepted_mutants_rejected tests).
"""
import torch

U24 = 2.0 ** -24
TINY = 2.0 ** -126
REC_REL = 2.0 ** -17

# row lengths / (M, C, ldx, ldy, ldd) of every kernel route (the lists of tests/test_gma_kernels.py)
FWD_N = (1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1028, 1030, 7332, 16380, 16381, 16384, 16388, 20001)
BWD_N = (1, 3, 4, 5, 255, 257, 1024, 1030, 7332, 8188, 8189, 8192, 8196, 12001)
REC_FWD_N = (32, 64, 2048, 2080, 8160, 16352)
REC_BWD_N = (32, 2048, 2080, 8160)
MIX_FWD = ((1, 4, 4, 4, 4), (7, 4, 12, 8, 20), (192, 128, 256, 128, 256), (8200, 512, 512, 512, 512))
MIX_BWD = ((1, 4, 4, 4, 4), (7, 4, 12, 8, 20), (192, 128, 256, 128, 256), (1100, 512, 512, 512, 512))
FWD_LDS_LAST, BWD_LDS_LAST = 16380, 8188          # the last rows the dense pair holds in LDS (4 / 8 ceil4(n) + 16 <= 65536)

LIMITS = dict(fwd_a=30.0, bwd=20.0, rec_bwd=3.0, dgamma=4.0)
GAMMA, DGAMMA0 = 0.37, 1.5                         # gamma is not 1; dgamma is pre-filled


# ------------------------------------------------------------------------------------------------------------ restatements
def softmax_ref(x):
    x = x.double()
    e = torch.exp(x - x.max(-1, keepdim=True).values)
    return e / e.sum(-1, keepdim=True)


def softmax_bwd_ref(A, dA):
    A, dA = A.double(), dA.double()
    return A * (dA - (A * dA).sum(-1, keepdim=True))


def mix_fwd_ref(x, y, g):
    return x.double() + float(g) * y.double()


def mix_bwd_ref(d, y, g, dx0, dgamma0):
    """(dx0 + d, g * d, dgamma0 + sum d y) in float64."""
    d, y = d.double(), y.double()
    return dx0.double() + d, float(g) * d, float(dgamma0) + float((d * y).sum())


# ------------------------------------------------------------------------------------------------------------------ records
def records_decode(t):
    """fp32 container [rows, n] (n % 32 == 0) holding [32 bf16 hi | 32 bf16 lo] per 32 columns -> hi + lo in float64."""
    rows, n = t.shape
    b = t.contiguous().view(torch.bfloat16).view(rows, n // 32, 2, 32).double()
    return (b[:, :, 0] + b[:, :, 1]).reshape(rows, n)


def records_encode(x):
    """fp32 values [rows, n] -> the container: hi = bf16_rne(x), lo = bf16_rne(x - hi) (rec_split4 on the host)."""
    x = x.float()
    rows, n = x.shape
    hi = x.bfloat16()
    lo = (x - hi.float()).bfloat16()                     # the difference is exact in fp32
    b = torch.stack([hi.view(rows, n // 32, 32), lo.view(rows, n // 32, 32)], 2).contiguous()
    return b.view(torch.float32).reshape(rows, n)


def records_wellformed(t):
    """Every record value has its leading part in hi: |lo| <= 2^-8 |hi| (half a bf16 ulp of hi).  The record GEMMs drop the
    lo * lo product, which is only small under this order."""
    rows, n = t.shape
    b = t.contiguous().view(torch.bfloat16).view(rows, n // 32, 2, 32).double()
    return bool((b[:, :, 1].abs() <= 2.0 ** -8 * b[:, :, 0].abs() + TINY).all())


# --------------------------------------------------------------------------------------------------------- row constructors
def logit_rows(n, seed=0):
    """(fp32 [R, n], names): row 0 gaussian (std 2.5); the designed rows after it."""
    g = torch.Generator().manual_seed(1000003 * seed + n)
    names, rows = [], []

    def add(name, r):
        names.append(name)
        rows.append(r)

    def base():
        return torch.randn(n, generator=g)
    add("gaussian", 2.5 * base())
    add("equal", torch.full((n,), 0.75))
    r = torch.full((n,), -30.0)
    r[n // 2] = 30.0
    add("peaked", r)
    r = base()
    r[0] = r.max() + 6
    add("max_first", r)
    r = base()
    r[n - 1] = r.max() + 6
    add("max_last", r)
    if n % 4 and n > 4:
        r = base()
        r[n - n % 4] = r.max() + 6
        add("max_tail", r)
    if n > 1024:
        r = base()
        r[1024 + (2 * (n - 1025)) // 3] = r.max() + 8
        add("beyond_1024", r)
    return torch.stack(rows), names


def bwd_rows(n, seed=0):
    """(A fp32 = the rounding of softmax_ref(logit_rows), dA fp32: gaussian, +-50 at the column where A is largest, names)."""
    x, names = logit_rows(n, seed)
    A = softmax_ref(x).float()
    g = torch.Generator().manual_seed(1000003 * seed + n + 500009)
    dA = torch.randn(A.shape, generator=g)
    col = A.argmax(-1)
    for r in range(A.shape[0]):
        dA[r, col[r]] = 50.0 * (-1) ** r
    return A, dA, names


def mix_inputs(M, C, seed=0):
    """x / d, y, dx0 as [M, C] fp32."""
    g = torch.Generator().manual_seed(7919 * seed + 31 * M + C)
    return torch.randn(M, C, generator=g), torch.randn(M, C, generator=g), 2.0 * torch.randn(M, C, generator=g)


# ------------------------------------------------------------------------------------------------------------------ scales
def fwd_scale(x, ref, records=False):
    """(scale, slack) of a softmax forward comparison."""
    x = x.double()
    d = x.max(-1, keepdim=True).values - x
    scale = ref * U24
    slack = 4 * d * scale + TINY
    return scale, slack + REC_REL * ref if records else slack


def bwd_scale(A, dA, ref, records=False):
    A, dA = A.double(), dA.double()
    scale = A * (dA.abs() + (A * dA).abs().sum(-1, keepdim=True)) * U24
    return scale, REC_REL * ref.abs() if records else torch.zeros_like(ref)


def need(got, ref, scale, slack=0.0):
    """(worst max(0, |got - ref| - slack) / scale, flat index of it); inf for a non-finite value or an excess where scale is 0."""
    got = got.double()
    ex = ((got - ref).abs() - slack).clamp_min(0)
    r = torch.where(ex == 0, torch.zeros_like(ex), ex / scale)
    r = torch.where(torch.isfinite(got) & ~torch.isnan(r), r, torch.full_like(r, float("inf")))
    i = int(r.argmax())
    return float(r.reshape(-1)[i]), i


# ----------------------------------------------------------------------------------------------------------------- fp32 twins
def softmax_twin(x):
    x = x.float()
    e = torch.exp(x - x.max(-1, keepdim=True).values)
    return e / e.sum(-1, keepdim=True)


def softmax_bwd_twin(A, dA):
    A, dA = A.float(), dA.float()
    return A * (dA - (A * dA).sum(-1, keepdim=True))


# -------------------------------------------------------------------------------------------------------------------- mutants
def _keep(n, which):
    k = torch.ones(n, dtype=torch.float64)
    if which == "last":
        k[n - 1:] = 0
    elif which == "tail":
        k[n - n % 4:] = 0
    elif which == "1024":
        k[1024:] = 0
    return k


def _applicable(n, records=False):
    out = []
    if n >= 2:
        out.append("last")
    if n % 4 and n > 4:
        out.append("tail")
    if n > 1024:
        out.append("1024")
    return out


def fwd_mutants(n):
    """{name: f(x) -> wrong softmax in float64} for a row length."""
    def miss(which):
        def f(x):
            x = x.double()
            e = torch.exp(x - x.max(-1, keepdim=True).values)
            return e / (e * _keep(n, which)).sum(-1, keepdim=True)
        return f

    def max256(x):
        x = x.double()
        e = torch.exp(x - x[:, :256].max(-1, keepdim=True).values).clamp_max(1.0)
        return e / e.sum(-1, keepdim=True)
    m = {"normaliser misses " + w: miss(w) for w in _applicable(n)}
    if n > 256:
        m["max over columns < 256, clamped"] = max256
    return m


def bwd_mutants(n):
    """{name: f(A, dA) -> wrong dS in float64}."""
    def miss(which):
        def f(A, dA):
            A, dA = A.double(), dA.double()
            return A * (dA - (A * dA * _keep(n, which)).sum(-1, keepdim=True))
        return f
    return {"dot misses " + w: miss(w) for w in (["last"] if n == 1 else _applicable(n))}


def records_swapped(t):
    """The container with hi and lo exchanged."""
    rows, n = t.shape
    b = t.contiguous().view(torch.bfloat16).view(rows, n // 32, 2, 32).flip(2).contiguous()
    return b.view(torch.float32).reshape(rows, n)


def records_second_stride_left(t, before):
    """The container whose units 256.. (columns 2048..) still hold what the buffer held before the call."""
    out = t.clone()
    out[:, 2048:] = before[:, 2048:]
    return out


def mix_bwd_mutants():
    """{name: f(d, y, g, dx0, dgamma0) -> (dx, dy, dgamma) wrong in one place}."""
    def no_acc(d, y, g, dx0, dgamma0):
        dx, dy, dg = mix_bwd_ref(d, y, g, dx0, dgamma0)
        return d.double(), dy, dg

    def overwritten(d, y, g, dx0, dgamma0):
        dx, dy, dg = mix_bwd_ref(d, y, g, dx0, dgamma0)
        return dx, dy, dg - float(dgamma0)
    return {"dx not accumulated": no_acc, "dgamma overwritten": overwritten}
