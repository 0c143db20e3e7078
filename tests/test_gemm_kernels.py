"""The seven GEMM entry points (csrc/gemm.hip, csrc/gemm_rec.hip) called through ops.*_raw / the C ABI on guarded flat buffers, each
case of tests/_gemmref.py against its float64 restatement.  Needs an MI355X: -m gpu.

Every case: operands between NaN guard rows with the NaN pattern in every pitch pad and batch gap, the output pre-filled with the
pattern (or C0); the error in units of 2^-24 S_mn (per element) is at most limit(case) = 4 x the fp32 twin's error on the same
data; every element of [M][N] is written; pads, gaps, the neighbouring column slice and the guard rows keep their bits; the inputs
are unchanged; an all-zero row of A gives a zero output row; a second launch gives the same bits unless the route adds with
atomics (K splits, or accumulate on the record entries).  The switches fsraft_set_gemm_split / fsraft_set_rec_mfma16 are set per
case by a fixture that restores 1 / 0.  tests/test_gemmref.py proves every limit on mutants.  profiles/gemm_kernel_margins.txt
lists every comparison (FSRAFT_PARITY_LOG).

Worst measured error per route next to that case's twin and limit (units of 2^-24 S_mn; MI355X):
  gemm_kernel<NN> A=scalar B=scalar          4 cases   worst  4.994   twin  4.992   limit  19.97   (f32_nn-lda+1)
  gemm_kernel<NN> A=scalar B=vec             1 cases   worst  3.177   twin  3.178   limit  12.71   (f32_nn-misaligned_A)
  gemm_kernel<NN> A=vec B=scalar            23 cases   worst  3.729   twin  3.728   limit  14.91   (f32_nn-129x127x132)
  gemm_kernel<NN> A=vec B=vec                6 cases   worst  3.291   twin   3.29   limit  13.16   (f32_nn-128x128x36)
  gemm_kernel<NT> A=scalar B=scalar          6 cases   worst 0.9936   twin 0.9935   limit  3.974   (f32_nt_split-129x127x1)
  gemm_kernel<NT> A=scalar B=vec             4 cases   worst  4.589   twin  4.588   limit  18.35   (f32_nt_split-lda+1_ldb+4)
  gemm_kernel<NT> A=vec B=scalar             4 cases   worst  3.521   twin   3.52   limit  14.08   (f32_nt_plain-misaligned_B)
  gemm_kernel<NT> A=vec B=vec               26 cases   worst  3.174   twin  3.172   limit  12.69   (f32_nt_plain-accumulate)
  gemm_rec_nt_kernel                        19 cases   worst  38.02   twin  37.48   limit  149.9   (rec_nt-sC_gap_ksplit1)
  gemm_rec_nt_kernel, atomic adds           11 cases   worst  32.84   twin   32.4   limit  129.6   (rec_nt-accumulate)
  gemm_rec_nt_kernel<list>                   6 cases   worst  29.24   twin     29   limit    116   (rec_nt_list-full_by_m)
  gemm_rec_nt_kernel<list>, atomic adds      3 cases   worst  36.27   twin  36.27   limit  145.1   (rec_nt_list-ksplit2)
  gemm_rec_nt_kernel<mfma16>                19 cases   worst  33.35   twin  33.23   limit  132.9   (rec_nt16-255x129x96)
  gemm_rec_nt_kernel<mfma16>, atomic adds   11 cases   worst   26.1   twin  25.85   limit  103.4   (rec_nt16-K160_ksplit3)
  gemm_rec_tn_kernel                        16 cases   worst  42.31   twin  41.85   limit  167.4   (rec_tn-alpha-0.37)
  gemm_rec_tn_kernel, atomic adds           10 cases   worst  30.99   twin  30.77   limit  123.1   (rec_tn-K129_ksplit4)
  gemm_rec_tn_kernel<list>                   6 cases   worst  37.49   twin     37   limit    148   (rec_tn_list-sparse_by_n)
  gemm_rec_tn_kernel<list>, atomic adds      3 cases   worst     44   twin  43.25   limit    173   (rec_tn_list-ksplit2)
  gemm_split_nt_kernel                      26 cases   worst  105.5   twin  105.1   limit  420.4   (f32_nt_split-ldc+3)
  gemm_split_tn_kernel                      23 cases   worst  53.25   twin  52.52   limit  210.1   (tn_split-260x8x65)
The exact routes (gemm_kernel) show the fma-chain twin's own error to three digits in every case; the split and record routes
stay within 1.03 x their twin: the dropped a_lo b_lo product and the rounding of lo are shared, the summation order is the rest.
All 227 cases, the to_records cases and the refusals passed on their first run.
"""
import ctypes

import pytest
import torch

import _gemmref as R
from _gmaref import records_decode
from _util import Buf, PATTERN, _log_margin

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from flow_supervisor_amd import _lib as L
    return L.load()


@pytest.fixture
def ops():
    from flow_supervisor_amd import ops as _ops
    return _ops


@pytest.fixture
def switches(lib):
    """set(split, mfma16) for the case at hand; the library's defaults (1, 0) come back whatever happens."""
    def set_(split, mfma16):
        assert lib.fsraft_set_gemm_split(int(split)) == 0 and lib.fsraft_set_rec_mfma16(int(mfma16)) == 0
    try:
        yield set_
    finally:
        lib.fsraft_set_gemm_split(1)
        lib.fsraft_set_rec_mfma16(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _device_buffers(p):
    c = p.case
    return {name: Buf(src=buf, offset={"A": c.offA, "B": c.offB}.get(name, 0)) for name, buf in p.bufs.items()}


def _launch(lib, ops, p, dev):
    """The case's entry on the device buffers (the ops wrappers raise on a non-zero status)."""
    c, L = p.case, p.lay
    ptr = {X: dev[L[X]["buf"]].mid.data_ptr() + 4 * L[X]["off"] for X in "ABC"}
    fl = (ptr["A"], L["A"]["ld"], L["A"]["s"], ptr["B"], L["B"]["ld"], L["B"]["s"], ptr["C"], L["C"]["ld"], L["C"]["s"], c.batch, c.M, c.N, c.K)
    k = R.kind(c)
    if k == "f32":
        ops.gemm_raw(*fl, bool(c.trans_b), c.alpha, bool(c.acc))
    elif k == "tn_split":
        ops.gemm_tn_raw(*fl, c.alpha, bool(c.acc))
    elif not R.is_list(c):
        (ops.gemm_rec_tn_raw if k == "rec_tn" else ops.gemm_rec_nt_raw)(*fl, c.alpha, c.ksplit, bool(c.acc))
    else:
        kl, kc, stride = R.list_arrays(c)
        kl, kc = kl.cuda(), kc.cuda()
        lda, sA, ldb, sB, ldc, sC = R.entry_args(c, L)
        fn = lib.fsraft_gemm_rec_tn_list if k == "rec_tn" else lib.fsraft_gemm_rec_nt_list
        rc = fn(ctypes.c_void_p(ptr["A"]), lda, sA, ctypes.c_void_p(ptr["B"]), ldb, sB, ctypes.c_void_p(ptr["C"]), ldc, sC, c.batch, c.M,
                c.N, c.K, c.alpha, c.ksplit, c.acc, ctypes.c_void_p(kl.data_ptr()), ctypes.c_void_p(kc.data_ptr()), stride, c.by_n, _stream())
        torch.cuda.synchronize()
        assert rc == 0, (c.id, rc)
    torch.cuda.synchronize()


def _run(lib, ops, p):
    dev = _device_buffers(p)
    _launch(lib, ops, p, dev)
    for name, d in dev.items():
        d.intact()
        if name != "C":
            assert torch.equal(_bits(d.cpu()), _bits(p.bufs[name])), f"{p.case.id}: input {name} changed"
    return dev["C"].cpu()


@pytest.mark.parametrize("c", R.ALL_CASES, ids=lambda c: c.id)
def test_gemm_case_vs_fp64(lib, ops, switches, c):
    p = R.build(c)
    ref, un = R.ref_and_unit(c)
    twin, lim = R.twin_error(c), R.limit(c)
    switches(c.split, c.mfma16)
    flat = _run(lib, ops, p)
    # everything but [M][N] keeps its bits; every element of [M][N] is written
    out = torch.zeros(flat.numel(), dtype=torch.bool)
    out[p.cidx.reshape(-1)] = True
    assert torch.equal(_bits(flat)[~out], _bits(p.bufs["C"])[~out]), f"{c.id}: a pad, gap or the neighbouring slice of C was written"
    got = flat[p.cidx]
    assert not bool((_bits(got) == PATTERN).any()), f"{c.id}: an output element was not written"
    err = R.error(got, ref, un)
    print(f"{c.id}: {R.route(c)}: err {err:.4g} twin {twin:.4g} limit {lim:.4g}")
    _log_margin(f"{R.route(c)} | {c.id}", err, lim, f"4 x twin {twin:.4g}, units of 2^-24 S_mn")
    assert err <= lim, f"{c.id} ({R.route(c)}): {err:.4g} units > 4 x twin {twin:.4g}"
    if c.M >= 3 and not c.acc:
        z = got[:, c.M - 2]
        assert bool((z == 0).all()), f"{c.id}: the all-zero row of A gave a non-zero output row"
        if c.alpha > 0 or R.is_atomic(c):
            assert not bool(_bits(z).any()), f"{c.id}: the all-zero row of A did not give zero bits"
    if not R.is_atomic(c):
        again = _run(lib, ops, p)
        assert torch.equal(_bits(again), _bits(flat)), f"{c.id}: a second launch gave other bits"


def test_rec_pitch_restated(ops):
    for C in (1, 31, 32, 33, 64, 96, 100, 128, 256, 300):
        assert R.rec_pitch(C) == ops.rec_pitch(C)


# --------------------------------------------------------------------------------------------------------------- to_records
@pytest.mark.parametrize("K", R.TO_RECORDS_K)
def test_to_records_bits(lib, K):
    """Scalar path (ld = K, K % 4 != 0) and vector path (ld rounded up to 4, the tail unit scalar), dense and rec_pitch rows:
    records_encode bit for bit, the zero tail of the last record, records beyond ceil(K / 32) untouched."""
    KR = R.ceil32(K)
    for rows in R.TO_RECORDS_ROWS:
        x = R.to_records_input(rows, K)
        want = R.ref_to_records(x, K)
        assert not bool(records_decode(want)[:, K:].any())
        if K % 32:                                          # the zero tail as bits: floats h .. 15 of the hi half and of the lo half
            r0, h = K // 32 * 32, (K % 32 + 1) // 2
            assert not bool(_bits(want[:, r0 + h:r0 + 16]).any()) and not bool(_bits(want[:, r0 + 16 + h:r0 + 32]).any())
        for ld in sorted({K, (K + 3) // 4 * 4}):
            src_cpu = R.pattern(rows * ld).reshape(rows, ld).clone()
            src_cpu[:, :K] = x
            for dst_ld, arg in ((KR, 0), (KR, KR), (R.rec_pitch(K), R.rec_pitch(K)), (R.rec_pitch(K) + 32, R.rec_pitch(K) + 32)):
                src, dst = Buf(src=src_cpu), Buf(n=rows * dst_ld)
                rc = lib.fsraft_to_records(ctypes.c_void_p(src.mid.data_ptr()), ld, ctypes.c_void_p(dst.mid.data_ptr()), arg, rows, K, _stream())
                torch.cuda.synchronize()
                assert rc == 0
                src.intact(), dst.intact()
                assert torch.equal(_bits(src.cpu()), _bits(src_cpu.reshape(-1)))
                exp = R.pattern(rows * dst_ld).reshape(rows, dst_ld).clone()
                exp[:, :KR] = want
                assert torch.equal(_bits(dst.cpu()), _bits(exp.reshape(-1))), (rows, K, ld, dst_ld)


def test_to_records_grid_stride(ops):
    """8200 x 4096: more 8-float units than 16384 blocks x 256 threads, so the kernel's loop takes a second trip.  Generated and
    compared on the device with the restatement test_gemmref.py pins on the CPU."""
    rows, K = R.TO_RECORDS_BIG
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(rows, K, device="cuda", generator=g)
    h = R.halfway_values().cuda()
    x[-1, -h.numel():] = h                                  # the last units of the second trip
    x[0, :h.numel()] = h
    x[rows // 2, ::3] = 0.0
    out = Buf(n=rows * K)
    got = ops.to_records(x)
    assert got.shape == (rows, K)
    want = R.ref_to_records(x, K)
    assert torch.equal(_bits(got), _bits(want))
    from flow_supervisor_amd import _lib as L
    assert L.load().fsraft_to_records(L.ptr(x), K, ctypes.c_void_p(out.mid.data_ptr()), 0, rows, K, L.stream()) == 0
    torch.cuda.synchronize()
    out.written()
    assert torch.equal(_bits(out.mid), _bits(want).reshape(-1))
    del out, got, want, x
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------ refusals
def _refused(rc, *outs):
    torch.cuda.synchronize()
    assert rc == 1
    for o in outs:
        o.untouched()


P = ctypes.c_void_p


def test_tn_split_refusals(lib):
    """fsraft_gemm_tn_split: M, N, lda, ldb, sA, sB not multiples of 4; a misaligned base.  Real buffers, large enough for every
    reading of the arguments."""
    A, B = Buf(src=torch.randn(4096)), Buf(src=torch.randn(4096))
    ok = dict(a=0, b=0, lda=8, sA=64, ldb=8, sB=64, M=8, N=8)
    for bad in (dict(M=6), dict(N=6), dict(lda=10), dict(ldb=10), dict(sA=66), dict(sB=66), dict(a=4), dict(b=4), dict(a=8)):
        q = dict(ok, **bad)
        C = Buf(n=4096)
        rc = lib.fsraft_gemm_tn_split(P(A.mid.data_ptr() + q["a"]), q["lda"], q["sA"], P(B.mid.data_ptr() + q["b"]), q["ldb"], q["sB"],
                                      P(C.mid.data_ptr()), 8, 64, 2, q["M"], q["N"], 8, 1.0, 0, _stream())
        _refused(rc, C)
    C = Buf(n=4096)
    assert lib.fsraft_gemm_tn_split(P(A.mid.data_ptr()), 8, 64, P(B.mid.data_ptr()), 8, 64, P(C.mid.data_ptr()), 8, 64, 2, 8, 8, 8, 1.0, 0, _stream()) == 0
    torch.cuda.synchronize()
    C.written(128)                                          # the unrefused call of the same shape does write


def test_rec_nt_refusals(lib):
    """fsraft_gemm_rec_nt: K < 32, K % 32, lda / ldb < K, lda / ldb % 32, ksplit < 1, a misaligned base."""
    A, B = Buf(n=8192, zero=True), Buf(n=8192, zero=True)
    ok = dict(a=0, b=0, lda=64, ldb=64, K=64, ksplit=1)
    for bad in (dict(K=16, lda=32, ldb=32), dict(K=48), dict(K=80, lda=96, ldb=96),
                dict(lda=32), dict(ldb=32), dict(lda=80), dict(ldb=80), dict(ksplit=0), dict(ksplit=-1), dict(a=4), dict(b=8)):
        q = dict(ok, **bad)
        C = Buf(n=1024)
        rc = lib.fsraft_gemm_rec_nt(P(A.mid.data_ptr() + q["a"]), q["lda"], 4 * 16 * q["lda"], P(B.mid.data_ptr() + q["b"]), q["ldb"],
                                    4 * 16 * q["ldb"], P(C.mid.data_ptr()), 16, 256, 2, 16, 16, q["K"], 1.0, q["ksplit"], 0, _stream())
        _refused(rc, C)
    C = Buf(n=1024)
    assert lib.fsraft_gemm_rec_nt(P(A.mid.data_ptr()), 64, 4 * 16 * 64, P(B.mid.data_ptr()), 64, 4 * 16 * 64, P(C.mid.data_ptr()), 16, 256, 2, 16,
                                  16, 64, 1.0, 1, 0, _stream()) == 0
    torch.cuda.synchronize()
    C.written(512)


def test_rec_tn_refusals(lib):
    """fsraft_gemm_rec_tn: lda < M, ldb < N, lda / ldb not whole records."""
    A, B = Buf(n=8192, zero=True), Buf(n=8192, zero=True)
    ok = dict(lda=64, ldb=64, a=0, b=0, ksplit=1)
    for bad in (dict(lda=32), dict(ldb=32), dict(lda=48), dict(ldb=80), dict(ksplit=0), dict(a=4), dict(b=4)):
        q = dict(ok, **bad)
        C = Buf(n=4096)
        rc = lib.fsraft_gemm_rec_tn(P(A.mid.data_ptr() + q["a"]), q["lda"], 4 * 8 * q["lda"], P(B.mid.data_ptr() + q["b"]), q["ldb"],
                                    4 * 8 * q["ldb"], P(C.mid.data_ptr()), 40, 1600, 2, 40, 40, 8, 1.0, q["ksplit"], 0, _stream())
        _refused(rc, C)


def test_to_records_refusals(lib):
    """fsraft_to_records: dst_ld too small or not whole records; misaligned src or dst."""
    S = Buf(src=torch.randn(4096))
    ok = dict(s=0, d=0, dst_ld=64)
    for bad in (dict(dst_ld=32), dict(dst_ld=80), dict(dst_ld=-32), dict(s=4), dict(d=4), dict(d=8)):
        q = dict(ok, **bad)
        D = Buf(n=4096)
        rc = lib.fsraft_to_records(P(S.mid.data_ptr() + q["s"]), 40, P(D.mid.data_ptr() + q["d"]), q["dst_ld"], 16, 40, _stream())
        _refused(rc, D)


def test_list_refusals(lib):
    """_list entries: a null list or count, kl_stride < 1, more k-tiles than the kernels hold in LDS (K = 65568 for rec_nt: 2049)."""
    null = P(0)
    kl, kc = torch.zeros(4096, dtype=torch.int32, device="cuda"), torch.ones(16, dtype=torch.int32, device="cuda")
    A, B = Buf(n=65537 * 32, zero=True), Buf(n=65537 * 32, zero=True)          # whole operands of the largest K below
    for fn, K, big, ld in ((lib.fsraft_gemm_rec_nt_list, 64, 65568, 0), (lib.fsraft_gemm_rec_tn_list, 64, 65537, 32)):
        for klp, kcp, stride, k in ((null, P(kc.data_ptr()), 2, K), (P(kl.data_ptr()), null, 2, K), (P(kl.data_ptr()), P(kc.data_ptr()), 0, K),
                                    (P(kl.data_ptr()), P(kc.data_ptr()), -1, K), (P(kl.data_ptr()), P(kc.data_ptr()), 2049, big)):
            C = Buf(n=1024)
            lda = ld or k
            rc = fn(P(A.mid.data_ptr()), lda, 0, P(B.mid.data_ptr()), lda, 0, P(C.mid.data_ptr()), 1, 1, 1, 1, 1, k, 1.0, 1, 0, klp, kcp, stride, 0,
                    _stream())
            _refused(rc, C)
    assert R.REC_LIST_MAX == 2048 and 65568 // 32 == 2049


def test_zero_matrices_refusal(lib):
    """The pitched branch of the split-K clear launches one grid row per matrix row: M = 65536 does not fit, the call is refused
    before anything is launched."""
    M = 65536
    A, B, C = Buf(n=M * 64, zero=True), Buf(n=64, zero=True), Buf(n=M * 2)
    rc = lib.fsraft_gemm_rec_nt(P(A.mid.data_ptr()), 64, 0, P(B.mid.data_ptr()), 64, 0, P(C.mid.data_ptr()), 2, M * 2, 1, M, 1, 64, 1.0, 2, 0, _stream())
    _refused(rc, C)


def test_switches_restored_last(lib):
    """No getter: set the defaults once more, so whatever runs next sees the library as it was loaded."""
    assert lib.fsraft_set_gemm_split(1) == 0 and lib.fsraft_set_rec_mfma16(0) == 0
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
