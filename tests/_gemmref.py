"""float64 restatements of the seven GEMM entry points (csrc/gemm.hip: fsraft_gemm_f32, fsraft_gemm_tn_split; csrc/gemm_rec.hip:
fsraft_to_records, fsraft_gemm_rec_nt / _tn and their _list variants), the case tables that cross every route and tile edge, the
fp32 twins that set each case's limit, and the mutants that prove the limits (tests/test_gemmref.py on the CPU,
tests/test_gemm_kernels.py against the kernels).  Plain torch on the CPU; nothing here touches a GPU.

Restatements.  ref_* take what the C entry takes: operands as flat buffers starting at the pointer the entry gets, pitch and
batch stride (in floats; the record entries' sA / sB in BYTES, as in the C ABI), M, N, K, alpha, accumulate, and the initial C.
Elements are gathered by index arithmetic (b * s + row * ld + col) and contracted with a loop over k in float64; record operands
go through _gmaref.records_decode (hi + lo), so the reference of a record GEMM is the exact product of the decoded values.

Error unit.  For output element (m, n):  unit = 2^-24 * S_mn,  S_mn = |alpha| sum_k |a||b| (+ |C0_mn| when accumulating).  The
error of a result is max_mn |got - ref| / unit_mn -- per element, so a fault confined to one row or tile edge is not diluted by a
large value elsewhere.  Where S_mn = 0 (an all-zero row of A) the result has to be exactly zero.

Twins.  Written from the kernels' stated arithmetic, never fitted to a GPU output:
  exact routes (gemm_kernel, v_mfma_f32_32x32x2_f32): a k-ordered fp32 fma chain (gemm_core.hpp), then alpha * acc and, when
      accumulating, C0 + that -- as two roundings and as one fma (the compiler may contract `*o + alpha * acc`); the worse counts.
  split and record routes (gemm_core_split.hpp, gemm_rec.hpp): hi = bf16_rne(x), lo = bf16_rne(x - hi); per 16-k block (32-k on
      the 16x16x32 route: one instruction per record) the three products a_lo b_hi, a_hi b_lo, a_hi b_hi in that order, fp32
      accumulation.  How the matrix unit sums the 16 products of one instruction is not stated, so the twin takes the worse of
      (a) a sequential fp32 sum inside the block and (b) the block summed exactly and rounded once.  Split-K: every split's
      partial from zero, alpha * partial added to C (zero or C0) in split order, each add rounded.
  limit(case) = 4 x the twin's error on that case's own data.  The twin's error on the split routes is dominated by the dropped
  a_lo b_lo product and the rounding of lo (2^-16 .. 2^-17 per product: hundreds of units at small K, tens at K = 640), which the
  kernels share bit for bit; the summation order is worth a few units.

Cases.  CASES[entry] lists Case records (frozen dataclasses, hashable: build / limit are cached per case).  build(case) lays the
operands out in flat buffers exactly as the entry will see them: NaN pattern (0x7FC0FFEE) in every pitch pad and batch gap,
a neighbouring column slice filled with other finite numbers, outputs pre-filled with the pattern or with C0.  Row M - 2 of A
(for M >= 3) is all zero in every case.  The `range` family scales A's output rows by 2^+-30 and B's output columns by 2^-+20.

Mutants.  MUTANTS maps a name to a function of a built case that returns the corrupted result (or None where the case cannot
show it): dropped k, wrong rows or operands, wrong scaling, the split arithmetic with a term missing, split-K partials lost or
doubled, a listed tile skipped, the 16-column halves of a 32-column block swapped.  test_gemmref.py: every mutant is at least
4 x limit(case) on at least one case (16 x the twin's own error)."""
import functools
import zlib
from dataclasses import dataclass, replace

import torch

from _gmaref import records_decode, records_encode

U24 = 2.0 ** -24
PATTERN = 0x7FC0FFEE
REC_LIST_MAX = 2048


def pattern(n):
    return torch.full((n,), PATTERN, dtype=torch.int32).view(torch.float32)


def ceil32(x):
    return (x + 31) // 32 * 32


def rec_pitch(C):
    """ops.rec_pitch restated (whole records, an odd number of them); test_gemm_kernels.py checks the two agree."""
    return 32 * (((C + 31) // 32) | 1)


# ------------------------------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    entry: str                  # f32 | tn_split | rec_nt | rec_tn | rec_nt_list | rec_tn_list
    name: str
    M: int
    N: int
    K: int
    batch: int = 1
    trans_b: int = 1            # f32 only
    split: int = 1              # f32 only: fsraft_set_gemm_split
    mfma16: int = 0             # rec_nt only: fsraft_set_rec_mfma16
    alpha: float = 1.0
    acc: int = 0
    ksplit: int = 1
    lda: int = 0                # 0: dense (the natural column count of the operand's container)
    ldb: int = 0
    ldc: int = 0
    gapA: int = 0               # floats between the batch entries
    gapB: int = 0
    gapC: int = 0
    sB0: bool = False           # one B matrix shared by the batch (batch stride 0)
    offA: int = 0               # floats the payload is moved off its 16-byte alignment by
    offB: int = 0
    cslice: bool = False        # C is the second column slice of a [M][2N] matrix
    bslice: bool = False        # B is the second column slice of a [K][2N] matrix (tn_split)
    shared: bool = False        # rec_nt: A and B are the two record slices of one [rows][2K] tensor
    rng: bool = False           # the range family
    lists: tuple = ()           # _list entries: per (batch, tile of the sparse operand) the listed k-tiles
    by_n: int = 0
    kl_stride: int = 0

    @property
    def id(self):
        return f"{self.entry}-{self.name}"

    @property
    def rec(self):
        return self.entry.startswith("rec")

    @property
    def tn(self):
        return self.entry in ("tn_split", "rec_tn", "rec_tn_list")


def _with(base, name, **kw):
    return replace(base, name=name, **kw)


def _cross(base, extra=()):
    """The shared cross-cutting cases on a base shape."""
    c = [_with(base, "batch3_gaps", batch=3, gapA=32 if base.rec else 8, gapC=5),
         _with(base, "alpha-0.37", alpha=-0.37),
         _with(base, "accumulate", acc=1, alpha=-0.37),
         _with(base, "accumulate_alpha1", acc=1),
         _with(base, "ldc+3", ldc=base.N + 3),
         _with(base, "cslice", cslice=True),
         _with(base, "cslice_accumulate", cslice=True, acc=1, alpha=-0.37),
         _with(base, "range", rng=True)]
    return c + list(extra)


def _f32_cases(mode):
    kw = dict(nt_split=dict(trans_b=1, split=1), nt_plain=dict(trans_b=1, split=0), nn=dict(trans_b=0, split=1))[mode]
    mk = lambda name, M, N, K, **k: Case("f32_" + mode, name, M, N, K, **kw, **k)
    out = []
    for K in (36, 100):
        for M, N in ((1, 1), (127, 129), (128, 128), (129, 127), (132, 260)):
            out.append(mk(f"{M}x{N}x{K}", M, N, K))
    for K in (1, 3, 4, 28, 32, 68, 132):
        out.append(mk(f"129x127x{K}", 129, 127, K))
    base = mk("base", 129, 127, 36)
    if mode == "nn":
        out += [mk("lda+1", 129, 127, 36, lda=37), mk("ldb+4_N%4", 129, 127, 36, ldb=128),      # A scalar | B scalar (N % 4), ldb % 4 == 0
                mk("N%4=0_ldb%4=0", 129, 128, 36), mk("N%4=0_ldb+1", 129, 128, 36, ldb=129)]       # B vector | B scalar
    else:
        out += [mk("lda+1_ldb+4", 129, 127, 36, lda=37, ldb=40), mk("lda+4_ldb+1", 129, 127, 36, lda=40, ldb=37),
                mk("lda+4_ldb+4", 129, 127, 36, lda=40, ldb=40)]
    out += [mk("misaligned_A", 129, 128, 36, offA=1), mk("misaligned_B", 129, 128, 36, offB=1),
            mk("misaligned_batch_stride", 129, 128, 36, batch=2, gapA=2, gapB=1)]
    out += _cross(base, [_with(base, "sB=0", batch=3, sB0=True), _with(base, "sB=0_aligned", batch=3, sB0=True, M=128, N=128, gapA=4)])
    return out


def _tn_split_cases():
    mk = lambda name, M, N, K, **k: Case("tn_split", name, M, N, K, **k)
    out = [mk(f"{M}x{N}x65", M, N, 65) for M, N in ((4, 4), (124, 132), (128, 128), (132, 124), (260, 8))]
    out += [mk(f"132x124x{K}", 132, 124, K) for K in (1, 2, 31, 32, 33, 64, 97)]
    base = mk("base", 132, 124, 65)
    out += [_with(base, "lda+4_ldb+8", lda=136, ldb=132), _with(base, "bslice_cslice", bslice=True, cslice=True),
            _with(base, "bslice_cslice_accumulate", bslice=True, cslice=True, acc=1, alpha=-0.37)]
    return out + _cross(base)


def _rec_nt_cases(mfma16):
    e = "rec_nt16" if mfma16 else "rec_nt"
    mk = lambda name, M, N, K, **k: Case(e, name, M, N, K, mfma16=mfma16, **k)
    out = [mk(f"{M}x{N}x96", M, N, 96) for M, N in ((1, 1), (255, 129), (256, 128), (257, 127), (300, 260))]
    out += [mk(f"257x127x{K}", 257, 127, K) for K in (32, 64, 160)]
    out += [mk(f"K160_ksplit{s}", 257, 127, 160, ksplit=s) for s in (2, 3, 4, 7)]
    out += [mk("K32_ksplit4", 257, 127, 32, ksplit=4)]
    base = mk("base", 257, 127, 96)
    out += [_with(base, "accumulate_ksplit3", acc=1, alpha=-0.37, ksplit=3),
            _with(base, "lda_rec_pitch", K=64, lda=rec_pitch(64), ldb=rec_pitch(64) + 32),
            _with(base, "shared_slices", shared=True), _with(base, "shared_slices_batch2", shared=True, batch=2, gapA=64),
            _with(base, "ldc+3_dense_sC_ksplit1", ldc=130, batch=2), _with(base, "ldc+3_dense_sC_ksplit3", ldc=130, batch=2, ksplit=3),
            _with(base, "sC_gap_ksplit1", batch=2, gapC=7), _with(base, "sC_gap_ksplit3", batch=2, gapC=7, ksplit=3),
            _with(base, "cslice_ksplit3", cslice=True, ksplit=3)]
    return out + _cross(base)


def _rec_tn_cases():
    mk = lambda name, M, N, K, **k: Case("rec_tn", name, M, N, K, **k)
    out = [mk(f"{M}x{N}x77", M, N, 77) for M, N in ((1, 1), (255, 129), (256, 128), (257, 127))]
    out += [mk(f"257x127x{K}", 257, 127, K) for K in (1, 31, 32, 33, 129, 160)]
    out += [mk(f"K{K}_ksplit{s}", 257, 127, K, ksplit=s) for K in (129, 160) for s in (3, 4)]
    base = mk("base", 257, 127, 77)
    out += [_with(base, "ld_one_record_wider", lda=ceil32(257) + 32, ldb=ceil32(127) + 32),
            _with(base, "accumulate_ksplit3", acc=1, alpha=-0.37, ksplit=3),
            _with(base, "ldc+3_ksplit3", ldc=130, batch=2, ksplit=3), _with(base, "sC_gap_ksplit3", batch=2, gapC=7, ksplit=3)]
    return out + _cross(base)


def _list_cases(tn):
    e = "rec_tn_list" if tn else "rec_nt_list"
    K = 129 if tn else 160                                   # five k-tiles; the k-major entry with a one-row last tile
    mk = lambda name, **k: Case(e, name, 257, 127, K, **k)   # two M tiles (256 + 1 rows), one N tile
    full = tuple(range(5))
    return [mk("full_by_n", lists=(full,), by_n=1), mk("full_by_m", lists=(full, full), by_n=0),
            mk("sparse_by_n", lists=((0, 2, 3),), by_n=1),
            mk("sparse_by_m_batch2", lists=((1, 2, 4), (0, 3), (4,), (0, 1, 2, 3)), by_n=0, batch=2),
            mk("empty_tile", lists=((0, 1, 3), ()), by_n=0),
            mk("stride_gt_count", lists=((1, 3, 4),), by_n=1, kl_stride=8),
            mk("ksplit2", lists=((0, 2, 4), (1, 3)), by_n=0, ksplit=2),
            mk("ksplit2_accumulate", lists=((0, 1, 2, 4),), by_n=1, ksplit=2, acc=1, alpha=-0.37),
            mk("sparse_by_n_accumulate_ksplit1", lists=((2, 4),), by_n=1, acc=1)]


CASES = {"f32_nt_split": _f32_cases("nt_split"), "f32_nt_plain": _f32_cases("nt_plain"), "f32_nn": _f32_cases("nn"),
         "tn_split": _tn_split_cases(), "rec_nt": _rec_nt_cases(0), "rec_nt16": _rec_nt_cases(1), "rec_tn": _rec_tn_cases(),
         "rec_nt_list": _list_cases(False), "rec_tn_list": _list_cases(True)}
ALL_CASES = [c for v in CASES.values() for c in v]
assert len({c.id for c in ALL_CASES}) == len(ALL_CASES)

TO_RECORDS_K = (1, 7, 8, 9, 31, 32, 33, 77, 96)
TO_RECORDS_ROWS = (1, 50)
TO_RECORDS_BIG = (8200, 4096)            # the smallest rows x K with rows * KR * 4 > 16384 * 256: the grid-stride second trip


def kind(c):
    """f32 | tn_split | rec_nt | rec_tn: the entry family (the case-table keys also carry the switch settings)."""
    return "f32" if c.entry.startswith("f32") else c.entry.replace("_list", "").replace("16", "")


def is_list(c):
    return c.entry.endswith("_list")


# ------------------------------------------------------------------------------------------------------------------ layout
def layout(c):
    """Per operand X in A, B, C: rows, cols of its container, ld, s (floats), off (floats from the start of its buffer to the
    pointer the entry gets), buf (A and B may share one), size of that buffer in floats."""
    k = kind(c)
    M, N, K = c.M, c.N, c.K
    dims = {"f32": ((M, K), (N, K) if c.trans_b else (K, N)), "tn_split": ((K, M), (K, N)), "rec_nt": ((M, K), (N, K)),
            "rec_tn": ((K, ceil32(M)), (K, ceil32(N)))}[k]
    L = {}
    for X, (rows, cols), ld, gap in (("A", dims[0], c.lda, c.gapA), ("B", dims[1], c.ldb, c.gapB)):
        ld = ld or cols
        nb = 1 if (X == "B" and c.sB0) else c.batch
        L[X] = dict(rows=rows, cols=cols, ld=ld, s=rows * ld + gap, off=0, buf=X, nb=nb)
    if c.bslice:
        L["B"].update(ld=2 * N, off=N, s=K * 2 * N + c.gapB)
    if c.shared:
        rows = max(M, N)
        for X, off in (("A", 0), ("B", K)):
            L[X].update(ld=2 * K, off=off, s=rows * 2 * K + c.gapA, buf="A")
    for X in "AB":
        d = L[X]
        d["size"] = (d["nb"] - 1) * d["s"] + (d["rows"] - 1) * d["ld"] + d["cols"] + d["off"]
    if c.shared:
        L["A"]["size"] = L["B"]["size"] = (c.batch - 1) * L["A"]["s"] + max(M, N) * 2 * K
    if c.sB0:
        L["B"]["s"] = 0
    ldc = 2 * N if c.cslice else (c.ldc or N)
    L["C"] = dict(rows=M, cols=N, ld=ldc, s=M * ldc + c.gapC, off=N if c.cslice else 0, buf="C", nb=c.batch)
    L["C"]["size"] = (c.batch - 1) * L["C"]["s"] + M * ldc if c.cslice else (c.batch - 1) * L["C"]["s"] + (M - 1) * ldc + N
    return L


def _index(d, nb=None, rows=None, cols=None, ld=None):
    nb, rows, cols, ld = nb or d["nb"], rows or d["rows"], cols or d["cols"], ld or d["ld"]
    ar = torch.arange
    return ar(nb)[:, None, None] * d["s"] + ar(rows)[None, :, None] * ld + ar(cols)[None, None, :]


def take(flat, s, ld, nb, rows, cols):
    """[nb][rows][cols] gathered from a flat buffer: element (b, r, c) at b * s + r * ld + c."""
    ar = torch.arange
    return flat[ar(nb)[:, None, None] * s + ar(rows)[None, :, None] * ld + ar(cols)[None, None, :]]


@dataclass
class Problem:
    case: Case
    a: torch.Tensor             # logical fp32 operands, k last: a [batch][M][K], b [batch or 1][N][K]
    b: torch.Tensor
    c0: torch.Tensor            # [batch][M][N]: what C holds before the call (used when accumulating)
    bufs: dict                  # name -> flat fp32 buffer as the device will hold it
    lay: dict
    cidx: torch.Tensor          # flat indices of the [batch][M][N] outputs inside bufs["C"]


def _gen(c):
    return torch.Generator().manual_seed(zlib.crc32(c.id.encode()))


@functools.lru_cache(maxsize=None)
def build(c):
    g = _gen(c)
    k = kind(c)
    M, N, K, nbB = c.M, c.N, c.K, (1 if c.sB0 else c.batch)
    a = torch.randn(c.batch, M, K, generator=g)
    b = torch.randn(nbB, N, K, generator=g)
    c0 = torch.randn(c.batch, M, N, generator=g) * 3.0
    if M >= 3:
        a[:, M - 2] = 0.0
    if c.rng:
        a *= (2.0 ** (30.0 * (1 - 2 * (torch.arange(M) % 2)))).float()[None, :, None]
        b *= (2.0 ** (-20.0 * (1 - 2 * (torch.arange(N) % 2)))).float()[None, :, None]
    if c.lists:                                              # zero records exactly where the sparse operand's lists say so
        tile, x = (128, b) if c.by_n else (256, a)
        nt = (x.shape[1] + tile - 1) // tile
        KT = (K + 31) // 32
        for bi in range(c.batch):
            for t in range(nt):
                for kt in set(range(KT)) - set(c.lists[bi * nt + t]):
                    x[bi, t * tile:(t + 1) * tile, kt * 32:(kt + 1) * 32] = 0.0
    L = layout(c)

    def container(x, X):
        if k == "f32":
            return x if (X == "A" or c.trans_b) else x.transpose(1, 2)
        if k == "tn_split":
            return x.transpose(1, 2)
        if k == "rec_nt":
            return records_encode(x.reshape(-1, K)).reshape(x.shape)
        xt = torch.zeros(x.shape[0], K, ceil32(x.shape[1]))
        xt[:, :, :x.shape[1]] = x.transpose(1, 2)
        return records_encode(xt.reshape(-1, xt.shape[2])).reshape(xt.shape)

    bufs = {}
    for X, x in (("A", a), ("B", b)):
        d = L[X]
        if d["buf"] not in bufs:
            bufs[d["buf"]] = pattern(d["size"])
        if c.bslice and X == "B":                            # the neighbouring slice: other finite numbers
            bufs["B"][d["off"] - N + _index(d)] = torch.randn(nbB, K, N, generator=g)
        bufs[d["buf"]][d["off"] + _index(d)] = container(x, X)
    dC = L["C"]
    C = pattern(dC["size"])
    cidx = dC["off"] + _index(dC)
    if c.cslice:
        C[cidx - N] = torch.randn(c.batch, M, N, generator=g)
    if c.acc:
        C[cidx] = c0
    bufs["C"] = C
    return Problem(c, a, b, c0, bufs, L, cidx)


def entry_args(c, L=None):
    """(lda, sA, ldb, sB, ldc, sC) as the C entry takes them: the record entries' operand batch strides in bytes."""
    L = L or layout(c)
    m = 4 if c.rec else 1
    return L["A"]["ld"], L["A"]["s"] * m, L["B"]["ld"], L["B"]["s"] * m, L["C"]["ld"], L["C"]["s"]


def list_arrays(c):
    """(klist int32 [tiles][kl_stride], kcount int32 [tiles]) of a _list case; slots beyond kcount name tile 0 (a kernel that
    read one would count that tile twice)."""
    stride = c.kl_stride or max(1, max(len(l) for l in c.lists))
    kl = torch.zeros(len(c.lists), stride, dtype=torch.int32)
    for i, l in enumerate(c.lists):
        kl[i, :len(l)] = torch.tensor(l, dtype=torch.int32)
    return kl, torch.tensor([len(l) for l in c.lists], dtype=torch.int32), stride


# ------------------------------------------------------------------------------------------------------------ restatements
def _contract(a, b, alpha, c0=None):
    """alpha * sum_k a[.., m, k] b[.., n, k] (+ c0), float64, a loop over k."""
    a, b = a.double(), b.double()
    out = torch.zeros(max(a.shape[0], b.shape[0]), a.shape[1], b.shape[1], dtype=torch.float64)
    for k in range(a.shape[2]):
        out += a[:, :, k, None] * b[:, None, :, k]
    out *= float(alpha)
    return out if c0 is None else out + c0.double()


def _decode(t):
    return records_decode(t.reshape(-1, t.shape[-1])).reshape(t.shape)


def ref_gemm_f32(A, lda, sA, Bm, ldb, sB, C0, ldc, sC, batch, M, N, K, trans_b, alpha, accumulate):
    a = take(A, sA, lda, batch, M, K)
    b = take(Bm, sB, ldb, batch, N, K) if trans_b else take(Bm, sB, ldb, batch, K, N).transpose(1, 2)
    return _contract(a, b, alpha, take(C0, sC, ldc, batch, M, N) if accumulate else None)


def ref_gemm_tn_split(A, lda, sA, Bm, ldb, sB, C0, ldc, sC, batch, M, N, K, alpha, accumulate):
    a = take(A, sA, lda, batch, K, M).transpose(1, 2)
    b = take(Bm, sB, ldb, batch, K, N).transpose(1, 2)
    return _contract(a, b, alpha, take(C0, sC, ldc, batch, M, N) if accumulate else None)


def _rec_operands(tn, A, lda, sA, Bm, ldb, sB, batch, M, N, K):
    assert sA % 4 == 0 and sB % 4 == 0
    if not tn:
        return _decode(take(A, sA // 4, lda, batch, M, K)), _decode(take(Bm, sB // 4, ldb, batch, N, K))
    a = _decode(take(A, sA // 4, lda, batch, K, ceil32(M)))[:, :, :M].transpose(1, 2)
    b = _decode(take(Bm, sB // 4, ldb, batch, K, ceil32(N)))[:, :, :N].transpose(1, 2)
    return a, b


def ref_gemm_rec_nt(A, lda, sA, Bm, ldb, sB, C0, ldc, sC, batch, M, N, K, alpha, accumulate):
    a, b = _rec_operands(False, A, lda, sA, Bm, ldb, sB, batch, M, N, K)
    return _contract(a, b, alpha, take(C0, sC, ldc, batch, M, N) if accumulate else None)


def ref_gemm_rec_tn(A, lda, sA, Bm, ldb, sB, C0, ldc, sC, batch, M, N, K, alpha, accumulate):
    a, b = _rec_operands(True, A, lda, sA, Bm, ldb, sB, batch, M, N, K)
    return _contract(a, b, alpha, take(C0, sC, ldc, batch, M, N) if accumulate else None)


def _listed(a, b, klist, kcount, kl_stride, by_n, fn):
    """fn(a_block, b_block, [k-tile numbers]) -> [1][m][n] for every (batch entry, tile of the sparse operand), assembled."""
    batch, M, N = a.shape[0], a.shape[1], b.shape[1]
    tile, ext = (128, N) if by_n else (256, M)
    nt = (ext + tile - 1) // tile
    kl = klist.reshape(-1)
    rows = []
    for bi in range(batch):
        parts = []
        for t in range(nt):
            lt = bi * nt + t
            tiles = [int(kl[lt * kl_stride + i]) for i in range(int(kcount[lt]))]
            sl = slice(t * tile, (t + 1) * tile)
            parts.append(fn(a[bi:bi + 1], b[bi:bi + 1, sl], tiles) if by_n else fn(a[bi:bi + 1, sl], b[bi:bi + 1], tiles))
        rows.append(torch.cat(parts, 2 if by_n else 1))
    return torch.cat(rows, 0)


def _ref_list(tn, A, lda, sA, Bm, ldb, sB, C0, ldc, sC, batch, M, N, K, alpha, accumulate, klist, kcount, kl_stride, kl_by_n):
    a, b = _rec_operands(tn, A, lda, sA, Bm, ldb, sB, batch, M, N, K)

    def fn(x, y, tiles):
        ks = [k for t in tiles for k in range(32 * t, min(32 * t + 32, K))]
        return _contract(x[:, :, ks], y[:, :, ks], alpha)
    out = _listed(a, b, klist, kcount, kl_stride, kl_by_n, fn)
    return out + take(C0, sC, ldc, batch, M, N).double() if accumulate else out


def ref_gemm_rec_nt_list(*args):
    """Arguments of ref_gemm_rec_nt, then klist, kcount, kl_stride, kl_by_n: the sum over the listed k-tiles only."""
    return _ref_list(False, *args)


def ref_gemm_rec_tn_list(*args):
    return _ref_list(True, *args)


def flat_args(p):
    """The pointer-level arguments of the case's entry on the CPU buffers: (A, lda, sA, B, ldb, sB, C, ldc, sC, batch, M, N, K)."""
    c, L = p.case, p.lay
    lda, sA, ldb, sB, ldc, sC = entry_args(c, L)
    A = p.bufs[L["A"]["buf"]][L["A"]["off"]:]
    Bm = p.bufs[L["B"]["buf"]][L["B"]["off"]:]
    return A, lda, sA, Bm, ldb, sB, p.bufs["C"][L["C"]["off"]:], ldc, sC, c.batch, c.M, c.N, c.K


def reference(p):
    """The case's restatement on its own buffers, [batch][M][N] float64."""
    c = p.case
    f = flat_args(p)
    k = kind(c)
    if k == "f32":
        return ref_gemm_f32(*f, c.trans_b, c.alpha, c.acc)
    if k == "tn_split":
        return ref_gemm_tn_split(*f, c.alpha, c.acc)
    if is_list(c):
        kl, kc, stride = list_arrays(c)
        return _ref_list(k == "rec_tn", *f, c.alpha, c.acc, kl, kc, stride, c.by_n)
    return (ref_gemm_rec_tn if k == "rec_tn" else ref_gemm_rec_nt)(*f, c.alpha, c.acc)


def operands64(p):
    """The values the entry multiplies, k last, float64: the fp32 operands, or the decoded records."""
    c = p.case
    A, lda, sA, Bm, ldb, sB = flat_args(p)[:6]
    nbB = 1 if c.sB0 else c.batch
    if c.rec:
        a, b = _rec_operands(c.tn, A, lda, sA, Bm, ldb, sB, c.batch, c.M, c.N, c.K)
        return a.double(), b.double()
    return p.a.double(), p.b.double()[:nbB]


def unit(p):
    """2^-24 S_mn, [batch][M][N] float64."""
    a, b = operands64(p)
    # (_list cases: the unlisted tiles are zero records, so the full sum is the listed sum)
    return U24 * _contract(a.abs(), b.abs(), abs(p.case.alpha), p.c0.abs() if p.case.acc else None)


def error(got, ref, un):
    """max_mn |got - ref| / unit_mn; where the unit is zero the result must be exact; NaN counts as infinite."""
    d = (got.double() - ref).abs()
    inf = torch.full_like(d, float("inf"))
    e = torch.where(un > 0, d / un, torch.where(d == 0, torch.zeros_like(d), inf))
    return float(torch.where(torch.isnan(e), inf, e).max())


@functools.lru_cache(maxsize=None)
def ref_and_unit(c):
    p = build(c)
    return reference(p), unit(p)


# -------------------------------------------------------------------------------------------------------------------- routes
def route(c):
    """The kernel the host code sends the case to (gemm.hip / gemm_rec.hip), with the loaders gemm_kernel picks."""
    k = kind(c)
    if k != "f32":
        r = {"tn_split": "gemm_split_tn_kernel", "rec_nt": "gemm_rec_nt_kernel<mfma16>" if c.mfma16 else "gemm_rec_nt_kernel",
             "rec_tn": "gemm_rec_tn_kernel"}[k] + ("<list>" if is_list(c) else "")
        KT = (c.K + 31) // 32
        ks = min(c.ksplit, KT)
        if c.rec and (ks > 1 or c.acc):
            r += f" atomic ksplit={ks}" + (" zero=" + ("dense" if zero_dense(c) else "pitched") if not c.acc else "")
        return r
    L = layout(c)
    lda, sA, ldb, sB = L["A"]["ld"], L["A"]["s"], L["B"]["ld"], L["B"]["s"]
    a16, b16 = c.offA % 4 == 0 and sA % 4 == 0, c.offB % 4 == 0 and sB % 4 == 0
    aligned = lda % 4 == 0 and ldb % 4 == 0 and c.K % 4 == 0 and a16 and b16
    if c.trans_b and c.split and aligned:
        return "gemm_split_nt_kernel"
    va = lda % 4 == 0 and c.K % 4 == 0 and a16
    vb = ldb % 4 == 0 and (c.K if c.trans_b else c.N) % 4 == 0 and b16
    return f"gemm_kernel<{'NT' if c.trans_b else 'NN'}> A={'vec' if va else 'scalar'} B={'vec' if vb else 'scalar'}"


def zero_dense(c):
    L = layout(c)["C"]
    return L["ld"] == c.N and L["s"] == c.M * c.N


def is_split_route(c):
    return not route(c).startswith("gemm_kernel<")


def is_atomic(c):
    return c.rec and (min(c.ksplit, (c.K + 31) // 32) > 1 or bool(c.acc))


# --------------------------------------------------------------------------------------------------------------------- twins
def bf16_split(x):
    """hi = bf16_rne(x), lo = bf16_rne(x - hi), both as fp32 (split4 / rec_split4)."""
    x = x.float()
    hi = x.bfloat16().float()
    return hi, (x - hi).bfloat16().float()


def _fma32(acc, x, y):
    """fl32(acc + x y): the product of two fp32 values is exact in float64."""
    return (acc.double() + x.double() * y.double()).float()


def _epilogues(c, parts, c0):
    """Every way the stated arithmetic may finish: parts = fp32 accumulators of the K splits (one unless split-K)."""
    al = torch.tensor(c.alpha, dtype=torch.float32)
    if is_atomic(c):
        out = c0.clone() if c.acc else torch.zeros_like(parts[0])
        for q in parts:
            out = out + al * q
        return [out]
    v = al * parts[0]
    if not c.acc:
        return [v]
    return [c0 + v, (c0.double() + al.double() * parts[0].double()).float()]


def _exact_parts(a, b):
    acc = torch.zeros(a.shape[0], b.shape[0], dtype=torch.float32)
    for k in range(a.shape[1]):
        acc = _fma32(acc, a[:, k, None], b[None, :, k])
    return [acc]


def _split_parts(a, b, tiles, ksplit, block, mode):
    """fp32 accumulators of the K splits over the listed 32-k tiles: a [m][K], b [n][K] fp32."""
    Kp = 32 * (max(tiles) + 1) if tiles else 32
    pad = lambda x: torch.cat([x[:, :Kp], torch.zeros(x.shape[0], max(0, Kp - x.shape[1]))], 1)
    (ah, al), (bh, bl) = bf16_split(pad(a)), bf16_split(pad(b))
    per = (len(tiles) + ksplit - 1) // ksplit
    parts = []
    for ks in range(ksplit):
        acc = torch.zeros(a.shape[0], b.shape[0], dtype=torch.float32)
        for t in tiles[ks * per:ks * per + per] if per else []:
            for k0 in range(32 * t, 32 * t + 32, block):
                sl = slice(k0, k0 + block)
                for x, y in ((al, bh), (ah, bl), (ah, bh)):
                    if mode == "sequential":
                        for k in range(k0, k0 + block):
                            acc = acc + x[:, k, None] * y[None, :, k]          # a product of two bf16 values is exact in fp32
                    else:
                        acc = (acc.double() + x[:, sl].double() @ y[:, sl].double().T).float()
        parts.append(acc)
    return parts


@functools.lru_cache(maxsize=None)
def twin_results(c):
    """{variant name: [batch][M][N] fp32} -- every variant of the case's twin."""
    p = build(c)
    KT = (c.K + 31) // 32
    ks = min(c.ksplit, KT) if c.rec else 1
    out = {}
    modes = [("exact", None)] if not is_split_route(c) else [("sequential", 32 if c.mfma16 else 16), ("once", 32 if c.mfma16 else 16)]
    for mode, block in modes:
        per_batch = []
        for bi in range(c.batch):
            a, b, c0 = p.a[bi], p.b[0 if c.sB0 else bi], p.c0[bi]
            if mode == "exact":
                res = _epilogues(c, _exact_parts(a, b), c0)
            elif is_list(c):
                kl, kc, stride = list_arrays(c)
                nt = len(c.lists) // c.batch
                fn = lambda x, y, tiles: torch.stack(_split_parts(x[0], y[0], tiles, ks, block, mode), -1)[None]
                parts = _listed(a[None], b[None], kl[bi * nt:(bi + 1) * nt], kc[bi * nt:(bi + 1) * nt], stride, c.by_n, fn)
                res = _epilogues(c, [parts[0, :, :, i] for i in range(ks)], c0)          # parts: [1][m][n][split]
            else:
                res = _epilogues(c, _split_parts(a, b, list(range(KT)), ks, block, mode), c0)
            per_batch.append(res)
        for i in range(len(per_batch[0])):
            out[f"{mode}{'/fma' if i else ''}"] = torch.stack([r[i] for r in per_batch])
    return out


@functools.lru_cache(maxsize=None)
def twin_error(c):
    ref, un = ref_and_unit(c)
    return max(error(t, ref, un) for t in twin_results(c).values())


def limit(c):
    """4 x the twin's error on the case's own data."""
    return 4.0 * twin_error(c)


# ------------------------------------------------------------------------------------------------------------------- mutants
def _ref_with(p, a=None, b=None, alpha=None, acc=None):
    c = p.case
    a0, b0 = operands64(p)
    a, b = a0 if a is None else a, b0 if b is None else b
    acc = c.acc if acc is None else acc
    return _contract(a, b, c.alpha if alpha is None else alpha, p.c0 if acc else None)


def _zero_k(p, k_from):
    a, _ = operands64(p)
    a = a.clone()
    a[:, :, k_from:] = 0.0
    return _ref_with(p, a=a)


def m_last_k_dropped(p):
    return _zero_k(p, p.case.K - 1)


def m_last_ktile_dropped(p):
    return _zero_k(p, 32 * ((p.case.K - 1) // 32))


def m_k4_tail_dropped(p):
    return _zero_k(p, p.case.K - p.case.K % 4) if p.case.K % 4 else None


def m_tile_row_as_row0(p):
    r = 256 if p.case.rec else 128
    if p.case.M <= r:
        return None
    out = reference(p).clone()
    out[:, r] = out[:, 0]
    return out


def m_batch_reads_batch0(p):
    if p.case.batch < 2:
        return None
    a, _ = operands64(p)
    return _ref_with(p, a=a[:1].expand_as(a))


def m_sB0_advancing(p):
    c = p.case
    if not c.sB0 or c.batch < 2:
        return None
    _, b = operands64(p)
    other = torch.randn(c.batch - 1, c.N, c.K, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    return _ref_with(p, b=torch.cat([b, other]))


def m_pitch_taken_as_k(p):
    c, d = p.case, p.lay["A"]
    if kind(c) != "f32" or d["ld"] == d["cols"]:
        return None
    A = flat_args(p)[0]
    return _ref_with(p, a=take(A, d["s"], d["cols"], c.batch, c.M, c.K).double())          # reads the NaN pads


def m_alpha_dropped(p):
    return _ref_with(p, alpha=1.0) if p.case.alpha != 1.0 else None


def m_alpha_on_c0(p):
    c = p.case
    return c.alpha * _ref_with(p, alpha=1.0) if (c.acc and c.alpha != 1.0) else None


def m_accumulate_ignored(p):
    return _ref_with(p, acc=0) if p.case.acc else None


def _terms(p, terms):
    """alpha * sum over the named hi / lo products (+ C0): the split arithmetic with terms missing or misplaced."""
    c = p.case
    if not is_split_route(c):
        return None
    (ah, al), (bh, bl) = bf16_split(p.a), bf16_split(p.b)
    h = dict(ah=ah, al=al, bh=bh, bl=bl)
    out = sum(_contract(h[x], h[y], c.alpha) for x, y in terms)
    return out + p.c0.double() if c.acc else out


def m_alo_bhi_dropped(p):
    return _terms(p, (("ah", "bl"), ("ah", "bh")))


def m_ahi_blo_dropped(p):
    return _terms(p, (("al", "bh"), ("ah", "bh")))


def m_record_halves_swapped(p):
    """A's records with hi and lo exchanged: the kernel then drops a_hi b_lo instead of a_lo b_lo."""
    return _terms(p, (("ah", "bh"), ("al", "bl"), ("al", "bh"))) if p.case.rec else None


def m_pure_bf16(p):
    return _terms(p, (("ah", "bh"),))


def _ksplit_weights(p, w):
    """The plain record entries with the partial of K split 1 weighted by w instead of 1."""
    c = p.case
    KT = (c.K + 31) // 32
    ks = min(c.ksplit, KT)
    if not c.rec or is_list(c) or ks < 2:
        return None
    per = (KT + ks - 1) // ks
    a, _ = operands64(p)
    a = a.clone()
    a[:, :, 32 * per:32 * 2 * per] *= w
    return _ref_with(p, a=a)


def m_ksplit_partial_missing(p):
    return _ksplit_weights(p, 0.0)


def m_ksplit_partial_twice(p):
    return _ksplit_weights(p, 2.0)


def m_listed_tile_skipped(p):
    c = p.case
    if not is_list(c) or not c.lists[0]:
        return None
    kl, kc, stride = list_arrays(replace(c, lists=(c.lists[0][:-1],) + c.lists[1:]))
    return _ref_list(kind(c) == "rec_tn", *flat_args(p), c.alpha, c.acc, kl, kc, stride, c.by_n)


def m_halves16_swapped(p):
    c = p.case
    if not c.mfma16 or c.N < 32:
        return None
    out = reference(p).clone()
    n = torch.arange(c.N)
    src = torch.where((n ^ 16) < c.N, n ^ 16, n)
    return out[:, :, src]


MUTANTS = {f.__name__[2:]: f for f in (
    m_last_k_dropped, m_last_ktile_dropped, m_k4_tail_dropped, m_tile_row_as_row0, m_batch_reads_batch0, m_sB0_advancing,
    m_pitch_taken_as_k, m_alpha_dropped, m_alpha_on_c0, m_accumulate_ignored, m_alo_bhi_dropped, m_ahi_blo_dropped,
    m_record_halves_swapped, m_pure_bf16, m_ksplit_partial_missing, m_ksplit_partial_twice, m_listed_tile_skipped,
    m_halves16_swapped)}


# ---------------------------------------------------------------------------------------------------------------- to_records
def halfway_values():
    """fp32 values exactly halfway between two bf16 neighbours, the lower neighbour's last bit 0 and 1 (RNE goes down / up), both
    signs, several exponents, and the carry into the exponent (1.1111111|1)."""
    v = []
    for e in (-20, -1, 0, 1, 30):
        for m in (0, 1, 2, 3, 126, 127):
            x = (1.0 + (2 * m + 1) * 2.0 ** -8) * 2.0 ** e
            v += [x, -x]
    return torch.tensor(v, dtype=torch.float32)


def rne_hi_bits(x):
    """The bf16 RNE of fp32 x as 16 integer bits, by integer arithmetic on the fp32 pattern (finite values)."""
    b = x.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF


def to_records_input(rows, K, seed=0):
    """Normal fp32 values and zeros, the halfway values among them."""
    g = torch.Generator().manual_seed(1000 * rows + K + seed)
    x = torch.randn(rows, K, generator=g) * (2.0 ** torch.randint(-12, 12, (rows, K), generator=g).float())
    x[torch.rand(rows, K, generator=g) < 0.1] = 0.0
    h = halfway_values()
    flat = x.reshape(-1)
    n = min(flat.numel() // 2 + 1, h.numel())
    flat[torch.randperm(flat.numel(), generator=g)[:n]] = h[:n]
    return flat.reshape(rows, K)


def ref_to_records(x, K):
    """[rows][ceil32(K)] container of x [rows][K]: records_encode of the zero-padded rows."""
    xp = torch.zeros(x.shape[0], ceil32(K), dtype=torch.float32, device=x.device)
    xp[:, :K] = x
    return records_encode(xp)
