"""The eight kernels of csrc/gma.hip called directly through ops.*, each against its float64 restatement (tests/_gmaref.py) at the
row lengths and pitches where its loops change: the scalar path (n % 4 != 0), one and several 256-thread strides, both sides of
the LDS / big-kernel threshold (forward 16380 | 16381, backward 8188 | 8189), the second 256-unit stride of the record pair and
its bounds (16352 / 8160), the grid-stride second trip of the mix pair, C = 4, pitched slices, pre-filled accumulators.  Every
case stacks the designed rows of _gmaref.logit_rows (5 to 7 rows) between two guard rows.  Needs an MI355X: -m gpu.

Limits: _gmaref.LIMITS, 4 x the worst value measured on MI355X over each kernel's whole list, one significant digit, in the
units of _gmaref's scales (dgamma: from the fp32 twin, see there); tests/test_gmaref.py proves each at most a quarter of what any
mutant produces.  profiles/gma_kernel_margins.txt lists every comparison (FSRAFT_PARITY_LOG).  Worst values measured:
  softmax_rows          a = 6.6 (n = 16388, big kernel; 2.3 at most on the LDS kernel)      limit 30
  softmax_rows_bwd      4.7 (n = 12001, big kernel; 3.9 at most on the LDS kernel)           limit 20
  softmax_rows_rec      0 beyond the records' 2^-17 |ref|; bits equal to to_records(dense)   limit a = 30
  softmax_rows_bwd_rec  0.53 (n = 2080)                                                      limit 3
  gma_mix_bwd dgamma    0.088 (7 x 4)                                                        limit 4
  gma_mix_fwd 0.50 and dx 1.000 of their fixed bounds (one fma, one correctly rounded add); dx at N = 8192: 0.24 / 0.10 of the limit.
All eight kernels, the big pair and the second record stride included, agreed with float64 on their first run."""
import functools

import pytest
import torch

import _gmaref as R
from _util import _log_margin

pytestmark = pytest.mark.gpu
DEV = "cuda"
PATTERN = 0x7FC0FFEE            # guard rows: a NaN, so a read of a guard row shows as well


@pytest.fixture(scope="module", autouse=True)
def _leave_no_cached_segments():
    """The N = 8192 case alone leaves about 2 GB of free segments in the caching allocator.  Long-lived allocations of later
    modules would be carved out of them and pin them, which changes the block sizes torch.cuda.memory_allocated() counts there
    (test_gpu_parity's allocation-flatness check compares those to 1 MB): hand them back when the module is done."""
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


@pytest.fixture
def ops():
    from flow_supervisor_amd import ops as _ops
    return _ops


@pytest.fixture(params=["exact", "split"])
def precision(request):
    """The two arithmetic modes of the GEMM-shaped kernels (as test_gpu_parity.precision)."""
    from flow_supervisor_amd import ops as _ops
    _ops.set_arithmetic(request.param == "split")
    yield request.param
    _ops.set_arithmetic(True)


def _guarded(t):
    """CPU [R, n] -> (device buffer [R + 2, n] whose first and last rows hold PATTERN, its contiguous middle slice = t)."""
    buf = torch.empty(t.shape[0] + 2, t.shape[1], device=DEV, dtype=torch.float32)
    buf.view(torch.int32).fill_(PATTERN)
    mid = buf[1:-1]
    mid.copy_(t)
    assert mid.is_contiguous()
    return buf, mid


def _guards_intact(buf):
    g = buf.view(torch.int32)
    assert bool((g[0] == PATTERN).all()) and bool((g[-1] == PATTERN).all()), "a guard row was written"


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check(what, got, ref, scale, slack, limit, names=None):
    worst, i = R.need(got, ref, scale, slack)
    row = f", row {names[i // ref.shape[-1]]}" if names else ""
    _log_margin(what, worst, limit, f"worst (|got - ref| - slack) / scale{row}")
    assert worst <= limit, f"{what}: {worst:.3g} > {limit:g}{row}, column {i % ref.shape[-1]}"


# ---------------------------------------------------------------------------------------------- references, computed once
@functools.lru_cache(maxsize=None)
def _fwd_case(n, records=False):
    x, names = R.logit_rows(n)
    ref = R.softmax_ref(x)
    return (x, names, ref) + R.fwd_scale(x, ref, records)


@functools.lru_cache(maxsize=None)
def _bwd_case(n):
    A, dA, names = R.bwd_rows(n)
    ref = R.softmax_bwd_ref(A, dA)
    return (A, dA, names, ref) + R.bwd_scale(A, dA, ref)


# ------------------------------------------------------------------------------------------------------------- dense softmax
@pytest.mark.parametrize("n", R.FWD_N)
def test_softmax_rows_vs_fp64(ops, n):
    """softmax_rows_kernel up to n = 16380, softmax_rows_big_kernel beyond."""
    x, names, ref, scale, slack = _fwd_case(n)
    buf, S = _guarded(x)
    assert ops.softmax_rows_(S) is S
    got = S.cpu()
    _guards_intact(buf)
    _check(f"softmax_rows n={n}", got, ref, scale, slack, R.LIMITS["fwd_a"], names)
    dev = (got.double().sum(-1) - 1).abs().max().item()
    _log_margin(f"softmax_rows n={n} row sums", dev, n * R.U24, "|sum - 1|, limit n * 2^-24")
    assert dev <= n * R.U24, (n, dev)


@pytest.mark.parametrize("n", R.BWD_N)
def test_softmax_rows_bwd_vs_fp64(ops, n):
    """softmax_rows_bwd_kernel up to n = 8188, softmax_rows_bwd_big_kernel beyond."""
    A, dA, names, ref, scale, slack = _bwd_case(n)
    Ad = A.to(DEV)
    buf, D = _guarded(dA)
    assert ops.softmax_rows_bwd_(Ad, D) is D
    got = D.cpu()
    _guards_intact(buf)
    assert _same_bits(Ad.cpu(), A), "A was written"
    _check(f"softmax_rows_bwd n={n}", got, ref, scale, slack, R.LIMITS["bwd"], names)


# ------------------------------------------------------------------------------------------------------------ record softmax
@pytest.mark.parametrize("n", R.REC_FWD_N)
def test_softmax_rows_rec_vs_fp64(ops, n):
    """Bit for bit ops.to_records of the dense kernel's map (the contract of test_attention_map_kept_once_as_records), and the
    decoded values against float64; n = 2080 is the first row with a second stride of 256 units, 16352 the bound."""
    x, names, ref, scale, slack = _fwd_case(n, True)
    buf, S = _guarded(x)
    assert ops.softmax_rows_rec_(S) is S
    got = S.cpu()
    _guards_intact(buf)
    dense = ops.to_records(ops.softmax_rows_(x.to(DEV)))
    assert tuple(dense.shape) == tuple(S.shape) and _same_bits(got, dense.cpu()), "records differ from to_records(dense softmax)"
    assert R.records_wellformed(got)
    _check(f"softmax_rows_rec n={n}", R.records_decode(got), ref, scale, slack, R.LIMITS["fwd_a"], names)


@pytest.mark.parametrize("n", R.REC_BWD_N)
def test_softmax_rows_bwd_rec_vs_fp64(ops, n):
    """A given as ops.to_records of an fp32 map; the reference is built from what those records decode to."""
    A0, dA, names = R.bwd_rows(n)
    Ar = ops.to_records(A0.to(DEV))
    before = Ar.cpu()
    assert _same_bits(before, R.records_encode(A0)), "ops.to_records against the host statement of rec_split4"
    A = R.records_decode(before)
    ref = R.softmax_bwd_ref(A, dA)
    scale, slack = R.bwd_scale(A, dA, ref, True)
    buf, D = _guarded(dA)
    assert ops.softmax_rows_bwd_rec_(Ar, D) is D
    got = D.cpu()
    _guards_intact(buf)
    assert _same_bits(Ar.cpu(), before), "the A records were written"
    assert R.records_wellformed(got)
    _check(f"softmax_rows_bwd_rec n={n}", R.records_decode(got), ref, scale, slack, R.LIMITS["rec_bwd"], names)


def _refused(call, *bufs):
    before = [b.clone() for b in bufs]
    with pytest.raises(RuntimeError, match="bad argument"):
        call(*bufs)
    torch.cuda.synchronize()
    for b, b0 in zip(bufs, before):
        assert _same_bits(b, b0), "a refused call wrote its buffer"


def _misaligned(rows, n):
    t = torch.randn(rows * n + 1, device=DEV)[1:].view(rows, n)
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


@pytest.mark.parametrize("n", (16, 48, 16384))
def test_softmax_rows_rec_refuses(ops, n):
    """Below one record, not whole records, a row over the LDS budget: an error before any launch, the logits untouched."""
    _refused(ops.softmax_rows_rec_, torch.randn(2, n, device=DEV))


@pytest.mark.parametrize("n", (40, 8192))
def test_softmax_rows_bwd_rec_refuses(ops, n):
    _refused(ops.softmax_rows_bwd_rec_, torch.randn(2, n, device=DEV), torch.randn(2, n, device=DEV))


def test_record_softmax_refuses_a_misaligned_base(ops):
    _refused(ops.softmax_rows_rec_, _misaligned(2, 64))
    _refused(ops.softmax_rows_bwd_rec_, _misaligned(2, 64), torch.randn(2, 64, device=DEV))
    _refused(ops.softmax_rows_bwd_rec_, torch.randn(2, 64, device=DEV), _misaligned(2, 64))


# ----------------------------------------------------------------------------------------------------------------------- mix
# channel offsets of the slices (x / d, y, dst / dx, dy) and whether x and dst (d and dx) are the halves of ONE buffer
MIX_OFFSETS = {(1, 4, 4, 4, 4): (0, 0, 0, 0, False), (7, 4, 12, 8, 20): (4, 4, 8, 8, False),
               (192, 128, 256, 128, 256): (0, 0, 128, 0, True)}


def _pitched(M, ld, seed):
    g = torch.Generator().manual_seed(seed)
    return (3.0 * torch.randn(M, ld, generator=g)).to(DEV)


def _put(buf, off, t):
    buf[:, off:off + t.shape[1]] = t.to(DEV)


def _outside_unchanged(after, before, off, C):
    a = after.clone()
    a[:, off:off + C] = before[:, off:off + C]
    return _same_bits(a, before)


@pytest.mark.parametrize("cfg", R.MIX_FWD, ids=lambda c: "x".join(map(str, c)))
def test_gma_mix_fwd_vs_fp64(ops, cfg):
    """dst = x + gamma y on pitched slices; (192, 128, 256, 128, 256) is the update block's call (x and dst the halves of one
    buffer), 8200 x 512 takes one more trip than 4096 workgroups cover."""
    M, C, ldx, ldy, ldd = cfg
    ox, oy, od, _, shared = MIX_OFFSETS.get(cfg, (0, 0, 0, 0, False))
    x, y, _ = R.mix_inputs(M, C)
    bx, by = _pitched(M, ldx, 1), _pitched(M, ldy, 2)
    bd = bx if shared else _pitched(M, ldd, 3)
    _put(bx, ox, x)
    _put(by, oy, y)
    g = torch.tensor([R.GAMMA], device=DEV)
    bx0, by0, bd0 = bx.clone(), by.clone(), bd.clone()
    ops.gma_mix_fwd(ops.V(bx, C, ox), ops.V(by, C, oy), g, ops.V(bd, C, od))
    torch.cuda.synchronize()
    assert _same_bits(by, by0) and _outside_unchanged(bd, bd0, od, C) and (shared or _same_bits(bx, bx0))
    gf = g.cpu()
    scale = 2 * R.U24 * (x.double().abs() + (float(gf) * y.double()).abs())
    _check(f"gma_mix_fwd {cfg}", bd[:, od:od + C].cpu(), R.mix_fwd_ref(x, y, gf), scale, 0.0, 1.0)


@pytest.mark.parametrize("cfg", R.MIX_BWD, ids=lambda c: "x".join(map(str, c)))
def test_gma_mix_bwd_vs_fp64(ops, cfg):
    """dx += d, dy = gamma d, dgamma += sum d y with dx and dgamma pre-filled; (192, 128, 256, 128, 256) is the update block's
    call (d and dx the halves of one buffer), 1100 x 512 takes more than one trip of the 512 workgroups."""
    M, C, ldx, ldy, ldd = cfg
    od, oy, ox, ody, shared = MIX_OFFSETS.get(cfg, (0, 0, 0, 0, False))
    if shared:
        od, ox = ox, od                                   # update.py: d is the upper half, dx the lower
    d, y, dx0 = R.mix_inputs(M, C)
    bd, by, bdy = _pitched(M, ldd, 1), _pitched(M, ldy, 2), _pitched(M, ldy + ody, 4)
    bdx = bd if shared else _pitched(M, ldx, 3)
    _put(bd, od, d)
    _put(by, oy, y)
    _put(bdx, ox, dx0)
    g = torch.tensor([R.GAMMA], device=DEV)
    dgamma = torch.tensor([R.DGAMMA0], device=DEV)
    bd0, by0, bdx0, bdy0 = bd.clone(), by.clone(), bdx.clone(), bdy.clone()
    ops.gma_mix_bwd(ops.V(bd, C, od), ops.V(by, C, oy), g, ops.V(bdx, C, ox), ops.V(bdy, C, ody), dgamma)
    torch.cuda.synchronize()
    assert _same_bits(by, by0) and _outside_unchanged(bdx, bdx0, ox, C) and _outside_unchanged(bdy, bdy0, ody, C)
    assert shared or _same_bits(bd, bd0)
    gf = g.cpu()
    dx, dy, dg = R.mix_bwd_ref(d, y, gf, dx0, R.DGAMMA0)
    _check(f"gma_mix_bwd {cfg} dx", bdx[:, ox:ox + C].cpu(), dx, R.U24 * dx.abs(), 0.0, 1.0)
    assert _same_bits(bdy[:, ody:ody + C].cpu(), gf * d), "dy is the fp32 product gamma * d"
    sdg = R.U24 * float((d.double() * y.double()).abs().sum())
    err = abs(dgamma.item() - dg)
    _log_margin(f"gma_mix_bwd {cfg} dgamma", err / sdg, R.LIMITS["dgamma"], "|got - ref| / (2^-24 sum |d y|)")
    assert err <= R.LIMITS["dgamma"] * sdg, (err / sdg, R.LIMITS["dgamma"])


# ------------------------------------------------------------------------------------------------------- dispatch at N = 8192
def test_attention_backward_at_n_8192(ops, precision, monkeypatch):
    """An 8 x 1024 grid (N = 8192, the 512 x 1024 crop): two rows of the map and the kernel's static words are 65552 bytes, over
    the LDS a launch gets, so the dense backward must take the big kernel.  dx against the autograd of the torch-composed map,
    under the content-only dctx limit of test_gpu_parity (2e-5 of max|ref|, x 8 under the split arithmetic)."""
    from flow_supervisor_amd.core.gma import Attention
    import argparse
    B, H, W, C = 1, 8, 1024, 128
    N = H * W
    seen = []
    bwd = ops.softmax_rows_bwd_

    def spy(A, dA):
        seen.append(A.shape[-1])
        return bwd(A, dA)
    monkeypatch.setattr(ops, "softmax_rows_bwd_", spy)
    g = torch.Generator(device=DEV).manual_seed(8192)
    att = Attention(args=argparse.Namespace(position_only=False, position_and_content=False), dim=C, heads=1, max_pos_size=160,
                    dim_head=128).to(DEV)
    with torch.no_grad():
        att.to_qk.weight.copy_(0.08 * torch.randn(att.to_qk.weight.shape, device=DEV, generator=g))
    x = torch.relu(1.5 * torch.randn(B, H, W, C, device=DEV, generator=g))
    G = torch.randn(B, 1, N, N, device=DEV, generator=g)
    xa = x.clone().requires_grad_(True)
    A = att.forward_cl(xa)
    assert tuple(A.shape) == (B, 1, N, N)
    A.backward(G)
    assert seen == [N], "the dense softmax backward did not run"
    del A
    fm = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    att._forward_general(fm).backward(G)
    ref = fm.grad.permute(0, 2, 3, 1)
    err = (xa.grad - ref).abs().max().item()
    lim = 2e-5 * (1.0 if precision == "exact" else 8.0) * ref.abs().max().item()
    _log_margin(f"dx at N = {N}, {precision}", err, lim, f"max abs error, limit relative to max|ref| {ref.abs().max().item():.3g}")
    assert torch.isfinite(xa.grad).all() and err <= lim, (err, lim)
