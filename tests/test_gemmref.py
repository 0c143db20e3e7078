"""tests/_gemmref.py on the CPU: the restatements of the GEMM entries against torch.matmul in float64 on strided views of the same
buffers, records_encode on the halfway values, the case tables against the boundaries they are there for, and the proof of the
limits -- the twin passes every case, every mutant is at least 4 x the limit of at least one case."""
import pytest
import torch

import _gemmref as R
from _gmaref import records_decode, records_encode

GROUPS = sorted(R.CASES)


def _view(p, X, rows=None, cols=None):
    d = p.lay[X]
    s = d["s"]
    return torch.as_strided(p.bufs[d["buf"]], (p.case.batch, rows or d["rows"], cols or d["cols"]), (s, d["ld"], 1), d["off"])


def _decoded(v):
    return records_decode(v.reshape(-1, v.shape[-1])).reshape(v.shape)


def _matmul(p):
    c = p.case
    A, B = _view(p, "A"), _view(p, "B")
    if c.rec:
        A, B = _decoded(A), _decoded(B)
    A, B = A.double(), B.double()
    k = R.kind(c)
    if k == "f32":
        out = A @ (B.transpose(1, 2) if c.trans_b else B)
    elif k == "rec_nt":
        out = A @ B.transpose(1, 2)
    else:
        out = (A.transpose(1, 2) @ B)[:, :c.M, :c.N]
    out = c.alpha * out
    return out + _view(p, "C").double() if c.acc else out


@pytest.mark.parametrize("group", GROUPS)
def test_restatements_equal_matmul_on_strided_views(group):
    """(_list cases too: what their lists leave out is zero records, so the listed sum is the full product.)"""
    for c in R.CASES[group]:
        p = R.build(c)
        ref, un = R.ref_and_unit(c)
        want = _matmul(p)
        assert ref.shape == (c.batch, c.M, c.N) and torch.isfinite(ref).all(), c.id
        assert ((ref - want).abs() <= 1e-6 * un + 1e-300).all(), c.id            # 1e-6 units: float64 summation order only


@pytest.mark.parametrize("group", GROUPS)
def test_buffers_hold_the_pattern_everywhere_but_the_operands(group):
    for c in R.CASES[group]:
        p = R.build(c)
        for name, buf in p.bufs.items():
            n_pat = int((buf.view(torch.int32) == R.PATTERN).sum())
            L = p.lay
            if name == "C":
                live = c.batch * c.M * c.N * ((1 if c.acc else 0) + (1 if c.cslice else 0))
            else:
                live = sum(d["nb"] * d["rows"] * d["cols"] for X, d in L.items() if X != "C" and d["buf"] == name)
                live += L["B"]["nb"] * c.K * c.N if (c.bslice and name == "B") else 0
            assert n_pat == buf.numel() - live, (c.id, name)
        if c.M >= 3:
            assert not R.operands64(p)[0][:, c.M - 2].any(), c.id
        assert R.rec_pitch(64) == 96 and R.rec_pitch(96) == 96 and R.rec_pitch(100) == 160


def test_case_tables_cross_the_boundaries_they_name():
    routes = {R.route(c) for c in R.ALL_CASES}
    for ld in ("vec", "scalar"):
        for lb in ("vec", "scalar"):
            assert f"gemm_kernel<NT> A={ld} B={lb}" in routes and f"gemm_kernel<NN> A={ld} B={lb}" in routes, (ld, lb, sorted(routes))
    assert {"gemm_split_nt_kernel", "gemm_split_tn_kernel", "gemm_rec_nt_kernel", "gemm_rec_nt_kernel<mfma16>", "gemm_rec_tn_kernel",
            "gemm_rec_nt_kernel<list>", "gemm_rec_tn_kernel<list>"} <= routes
    assert any("zero=pitched" in r for r in routes) and any("zero=dense" in r for r in routes)
    # the misaligned base with every pitch aligned goes to the scalar loads of the plain kernel, also with the split switch on
    by_id = {c.id: c for c in R.ALL_CASES}
    assert R.route(by_id["f32_nt_split-misaligned_A"]) == "gemm_kernel<NT> A=scalar B=vec"
    assert R.route(by_id["f32_nn-misaligned_B"]) == "gemm_kernel<NN> A=vec B=scalar"
    assert R.route(by_id["f32_nt_plain-misaligned_batch_stride"]) == "gemm_kernel<NT> A=scalar B=scalar"
    assert R.route(by_id["f32_nt_split-sB=0_aligned"]) == "gemm_split_nt_kernel"
    # KT = 5 over 4 splits: two tiles each, the fourth workgroup's range starts past the end (kt = -1)
    c = by_id["rec_nt-K160_ksplit4"]
    KT, per = c.K // 32, (c.K // 32 + 3) // 4
    assert (KT, per, min(per, KT - 3 * per)) == (5, 2, -1)
    assert {(c.K + 31) // 32 for c in R.CASES["f32_nt_split"] if R.route(c) == "gemm_split_nt_kernel"} >= {1, 2, 3, 4, 5}
    assert {(c.K + 31) // 32 for c in R.CASES["tn_split"]} >= {1, 2, 3, 4}
    rows, K = R.TO_RECORDS_BIG
    assert rows * (K // 32) * 4 > 16384 * 256 >= (rows - 8) * (K // 32) * 4


def test_records_encode_on_halfway_values():
    """hi is the RNE bf16 of x by integer arithmetic on the bits (ties to the even neighbour, both parities, the carry into the
    exponent), lo the RNE bf16 of the exact remainder; and the twin's bf16_split is what the containers hold."""
    h = R.halfway_values()
    x = torch.cat([h, torch.zeros(64 - h.numel() % 64)]).reshape(-1, 32)
    t = records_encode(x).view(torch.int16).reshape(-1, 2, 32).to(torch.int32) & 0xFFFF
    hi_bits, lo_bits = t[:, 0].reshape(-1), t[:, 1].reshape(-1)
    assert torch.equal(hi_bits.long(), R.rne_hi_bits(x.reshape(-1)))
    w = hi_bits.long() << 16
    hi = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32).view(torch.float32)
    assert torch.equal(lo_bits.long(), R.rne_hi_bits(x.reshape(-1) - hi))
    n = h.numel()
    lower_even = (R.rne_hi_bits(h) == ((h.view(torch.int32).long() & 0xFFFFFFFF) >> 16))          # rounded down: the kept pattern
    assert 0 < int(lower_even.sum()) < n                                                        # both directions occur
    assert (hi[:n] != h).all()
    th, tl = R.bf16_split(x)
    bits = lambda v: (v.reshape(-1).view(torch.int32) >> 16) & 0xFFFF
    assert torch.equal(bits(th), hi_bits) and torch.equal(bits(tl), lo_bits)
    assert torch.equal(records_decode(records_encode(x)), th.double() + tl.double())
    for rows, K in ((1, 1), (50, 33), (3, 96)):
        xin = R.to_records_input(rows, K)
        assert torch.isfinite(xin).all() and ((xin == 0) | (xin.abs() >= 2.0 ** -126)).all()
        r = R.ref_to_records(xin, K)
        assert r.shape == (rows, R.ceil32(K))
        assert torch.equal(records_decode(r)[:, :K], sum(R.bf16_split(xin)).double()) and not records_decode(r)[:, K:].any()


@pytest.mark.parametrize("group", GROUPS)
def test_twin_passes_every_case(group):
    worst = {}
    for c in R.CASES[group]:
        e, lim = R.twin_error(c), R.limit(c)
        assert 0.0 < e < float("inf") and e <= lim == 4.0 * e, c.id
        worst[R.route(c).split(" atomic")[0]] = max(worst.get(R.route(c).split(" atomic")[0], 0.0), e)
    for r, e in worst.items():
        # orientation: a few units on the exact routes, the dropped lo * lo product (<= 2^-16 S: 256 units) and rounding beyond
        assert e < (8.0 if r.startswith("gemm_kernel<") else 512.0), (r, e)


@pytest.mark.parametrize("name", sorted(R.MUTANTS))
def test_every_mutant_is_rejected(name):
    """At least one case shows the mutant at 4 x its limit or more (16 x the twin's error)."""
    best, shown = 0.0, 0
    for c in R.ALL_CASES:
        got = R.MUTANTS[name](R.build(c))
        if got is None:
            continue
        ref, un = R.ref_and_unit(c)
        ratio = R.error(got, ref, un) / R.limit(c)
        shown += ratio >= 4.0
        best = max(best, ratio)
    assert shown >= 1 and best >= 4.0, (name, best, shown)


def test_mutants_are_rejected_on_every_route_they_apply_to():
    """The split-arithmetic mutants on each split route, the K-split mutants on both record entries: the gap holds per route, not
    only somewhere."""
    seen = {}
    for c in R.ALL_CASES:
        r = R.route(c).split(" ")[0]
        for name in ("alo_bhi_dropped", "ahi_blo_dropped", "pure_bf16", "record_halves_swapped", "ksplit_partial_missing",
                     "ksplit_partial_twice", "last_k_dropped", "tile_row_as_row0"):
            got = R.MUTANTS[name](R.build(c))
            if got is None:
                continue
            ref, un = R.ref_and_unit(c)
            seen[(r, name)] = max(seen.get((r, name), 0.0), R.error(got, ref, un) / R.limit(c))
    assert len(seen) >= 40
    assert all(v >= 4.0 for v in seen.values()), {k: v for k, v in seen.items() if v < 4.0}
