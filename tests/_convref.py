"""fp64 reference of the implicit-GEMM convolutions (fsraft_conv_forward / fsraft_conv_wgrad[_multi]) and a comparator whose
detection power every case proves on two mutants.  Device-agnostic: the CPU suite runs it on small shapes, the GPU suite on
the kernels' own inputs (tests/test_conv_routes.py).

Operation (one GEMM per call): Y[m, n] = sum_{s, tap, c} X_s[pixel m shifted by tap, c] * Wt[n, s, c, tap], m = (b, y, x),
taps (ky, kx) with top / left padding (PH, PW), zero outside the image.  The epilogues restate conv_epilogue_lds /
conv_finish_kernel.  Arithmetic twins, all computed in fp64 from the same fp32 inputs:
  bf16x1  -- bf16(a) * bf16(w)
  bf16x3  -- hi*hi + hi*lo + lo*hi, hi = bf16(x), lo = bf16(x - hi)     (the split-bf16 MFMA core)
  fp32    -- the same GEMM in torch float32 (accumulation error only)
"""
import math

import torch

U32 = 2.0 ** -24
GAMMA_PROD = {"fp32": 0.0, "bf16x3": 2.0 ** -16}     # per-product relative error bound of the arithmetic (|a w| units)
CHUNK_BYTES = 1 << 30                                # fp64 im2col rows per chunk: at most ~1 GB


def bf16_hi_lo(x):
    hi = x.to(torch.bfloat16).to(x.dtype)
    lo = (x - hi).to(torch.bfloat16).to(x.dtype)
    return hi, lo


def wmat(w):
    """OIHW weight [N, Cin, KH, KW] -> [KH*KW*Cin, N] in the im2col order of `columns` (tap-major, then channel)."""
    N, Cin, KH, KW = w.shape
    return w.permute(2, 3, 1, 0).reshape(KH * KW * Cin, N)


def columns(xs, B, H, W, KH, KW, pad, rows):
    """im2col of the concatenated sources at output pixels `rows` (int64 indices into B*H*W): [len(rows), KH*KW*Cin],
    dtype of xs.  xs: list of [B, H, W, C_s] tensors (the channels each source contributes)."""
    PH, PW = pad
    x = torch.cat(xs, -1) if len(xs) > 1 else xs[0]
    C = x.shape[-1]
    xp = x.new_zeros(B, H + KH - 1, W + KW - 1, C)
    xp[:, PH:PH + H, PW:PW + W] = x
    xp = xp.reshape(-1, C)
    b = rows // (H * W)
    yx = rows % (H * W)
    y, xq = yx // W, yx % W
    Hp, Wp = H + KH - 1, W + KW - 1
    base = (b * Hp + y) * Wp + xq
    cols = []
    for ky in range(KH):
        for kx in range(KW):
            cols.append(xp[base + ky * Wp + kx])
    return torch.cat(cols, 1)


def conv_gemm(xs, w, B, H, W, pad, rows, mode="fp64"):
    """Pre-epilogue GEMM at `rows`: [len(rows), N] in fp64.  mode: fp64 | abs (|X| |W|: the bound's scale) | fp32 | bf16x1 | bf16x3."""
    N, Cin, KH, KW = w.shape
    K = KH * KW * Cin
    step = max(1, CHUNK_BYTES // (8 * K * 3))
    out = []
    wm = wmat(w.double())
    if mode == "bf16x1":
        wm1 = bf16_hi_lo(wm)[0]
    elif mode == "bf16x3":
        whi, wlo = bf16_hi_lo(wm)
    for i in range(0, rows.numel(), step):
        r = rows[i:i + step]
        if mode == "fp32":
            out.append((columns([x.float() for x in xs], B, H, W, KH, KW, pad, r) @ wmat(w.float())).double())
            continue
        a = columns([x.double() for x in xs], B, H, W, KH, KW, pad, r)
        if mode == "fp64":
            out.append(a @ wm)
        elif mode == "abs":
            out.append(a.abs() @ wm.abs())
        elif mode == "bf16x1":
            out.append(bf16_hi_lo(a)[0] @ wm1)
        elif mode == "bf16x3":
            ahi, alo = bf16_hi_lo(a)
            out.append((ahi + alo) @ (whi + wlo) - alo @ wlo)
        else:
            raise ValueError(mode)
    return torch.cat(out, 0)


def chunk_contribution(xs, w, B, H, W, pad, rows, src, tap, c0):
    """The share of one 32-channel chunk (source `src`, channels c0..c0+31, one tap) in the GEMM at `rows`: mutant (a) removes it."""
    N, Cin, KH, KW = w.shape
    off = sum(x.shape[-1] for x in xs[:src])
    C = xs[src].shape[-1]
    c1 = min(C, c0 + 32)
    ky, kx = divmod(tap, KW)
    a = columns([xs[src][..., c0:c1].double()], B, H, W, KH, KW, pad, rows)
    ws = w[:, off + c0:off + c1].double()
    sel = torch.zeros(KH, KW, dtype=torch.bool)
    sel[ky, kx] = True
    wsel = ws * sel.to(ws.device)
    return a @ wmat(wsel)


def dgrad_weight(w):
    """The forward weight [Cout, Cin, KH, KW] as the data-gradient convolution sees it (packs of modes 1 / 11): [Cin, Cout, KH, KW],
    taps flipped; with forward padding (PH, PW) the data gradient pads (KH - 1 - PH, KW - 1 - PW)."""
    return w.flip(2, 3).transpose(0, 1).contiguous()


def wgrad_gemm(dys, xss, B, H, W, KH, KW, mode="fp64", pad=None):
    """Weight gradient sum_seg dY_seg^T im2col(X_seg) as OIHW [Cout, Cin, KH, KW] in fp64 (mode as conv_gemm, on the same
    products), padding (KH // 2, KW // 2) as the weight-gradient kernels use.  dys: [B, H, W, Cout] per segment; xss: list of
    source lists per segment."""
    pad = (KH // 2, KW // 2) if pad is None else pad
    Cout = dys[0].shape[-1]
    Cin = sum(x.shape[-1] for x in xss[0])
    M = B * H * W
    rows = torch.arange(M, device=dys[0].device)
    K = KH * KW * Cin
    step = max(1, CHUNK_BYTES // (8 * K * 3))
    acc = torch.zeros(K, Cout, dtype=torch.float64, device=dys[0].device)
    for dy, xs in zip(dys, xss):
        d = dy.reshape(M, Cout)
        for i in range(0, M, step):
            r = rows[i:i + step]
            if mode == "fp32":
                acc += (columns([x.float() for x in xs], B, H, W, KH, KW, pad, r).t() @ d[i:i + step].float()).double()
                continue
            a = columns([x.double() for x in xs], B, H, W, KH, KW, pad, r)
            g = d[i:i + step].double()
            if mode == "fp64":
                acc += a.t() @ g
            elif mode == "abs":
                acc += a.abs().t() @ g.abs()
            elif mode == "bf16x1":
                acc += bf16_hi_lo(a)[0].t() @ bf16_hi_lo(g)[0]
            elif mode == "bf16x3":
                ahi, alo = bf16_hi_lo(a)
                ghi, glo = bf16_hi_lo(g)
                acc += (ahi + alo).t() @ (ghi + glo) - alo.t() @ glo
            else:
                raise ValueError(mode)
    return acc.reshape(KH, KW, Cin, Cout).permute(3, 2, 0, 1).contiguous()


def packed_k_index(srcC, KH, KW):
    """Column of the packed [Cout, Ktot] matrix (forward packs, weight gradients) that holds input channel c (of the
    concatenated sources) at tap t: per source, taps x 32-padded channels (conv_ktot, build_ktab, wgrad_patch.inc).
    Returns (index [KH*KW, Cin] int64, Ktot)."""
    taps = KH * KW
    idx = torch.empty(taps, sum(srcC), dtype=torch.int64)
    k0, c0 = 0, 0
    for C in srcC:
        cpad = (C + 31) // 32 * 32
        for t in range(taps):
            idx[t, c0:c0 + C] = k0 + t * cpad + torch.arange(C)
        k0 += taps * cpad
        c0 += C
    return idx, k0


def unpack_ref(wpk, srcC, KH, KW):
    """Packed [Cout, Ktot] -> OIHW [Cout, Cin, KH, KW] by packed_k_index (exact: a gather)."""
    idx, ktot = packed_k_index(srcC, KH, KW)
    assert wpk.shape[1] == ktot
    g = wpk[:, idx.to(wpk.device).reshape(-1)].reshape(wpk.shape[0], KH * KW, -1)
    return g.permute(0, 2, 1).reshape(wpk.shape[0], -1, KH, KW).contiguous()


def pack_ref(w, srcC):
    """OIHW -> packed [Cout, Ktot] (zeros in the channel padding): the inverse of unpack_ref."""
    Cout, Cin, KH, KW = w.shape
    idx, ktot = packed_k_index(srcC, KH, KW)
    out = w.new_zeros(Cout, ktot)
    out[:, idx.to(w.device).reshape(-1)] = w.permute(0, 2, 3, 1).reshape(Cout, -1)
    return out


# ---------------------------------------------------------------------------------------------------------------- epilogues
class Epi:
    """What the kernel does with the GEMM result G [rows, N] (fp64 restatement of conv_epilogue_lds / conv_finish_kernel).
    kind 0 (plain): per destination d (GEMM columns [n0_d, n0_{d+1})): v = (G + bias) * alpha, ReLU, + old destination value
    if it accumulates, zeroed where the destination's mask (a [rows, maskc] tensor) is <= 0 on columns < maskc.
    kind 2 (EPI_ZR): s = sigmoid(G + bias + pre): columns < hid -> z, the rest -> r and r * h.
    kind 3 (EPI_Q):  q = tanh(G + bias + pre); h' = (1 - z) h + z q.
    `apply(G, e)` returns {output name: (value, bound)} with the bound propagated from |G error| <= e."""

    def __init__(self, kind=0, N=None, bias=None, alpha=1.0, relu=False, dsts=((0, None, None),), pre=None, h=None, z=None,
                 hid=0):
        self.kind, self.N, self.bias, self.alpha, self.relu = kind, N, bias, alpha, relu
        self.dsts = dsts              # plain: ((n0, old value [rows, width] or None, mask [rows, maskc] or None), ...)
        self.pre, self.h, self.z, self.hid = pre, h, z, hid

    def apply(self, G, e):
        N = G.shape[1]
        v = G if self.bias is None else G + self.bias.double()
        out = {}
        if self.kind == 0:
            v = v * self.alpha
            e = e * abs(self.alpha)
            if self.relu:
                v = v.clamp_min(0)
            bounds = list(self.dsts) + [(N, None, None)]
            for i, (n0, old, mask) in enumerate(self.dsts):
                n1 = bounds[i + 1][0]
                r, ee = v[:, n0:n1], e[:, n0:n1]
                if old is not None:
                    r = r + old.double()[:, :n1 - n0]
                    ee = ee + U32 * r.abs()
                if mask is not None:
                    mc = mask.shape[1]
                    keep = torch.ones_like(r, dtype=torch.bool)
                    keep[:, :mc] = mask.double()[:, :min(mc, n1 - n0)] > 0
                    r = torch.where(keep, r, torch.zeros_like(r))
                    ee = torch.where(keep, ee, torch.zeros_like(ee))
                out[f"dst{i}"] = (r, ee + 3 * U32 * r.abs())
            return out
        if self.pre is not None:
            v = v + self.pre.double()[:, :N]
        if self.kind == 2:
            s = torch.sigmoid(v)
            es = e / 4 + 4 * U32
            hid = self.hid
            h = self.h.double()[:, :hid]
            out["z"] = (s[:, :hid], es[:, :hid])
            out["r"] = (s[:, hid:], es[:, hid:])
            rh = s[:, hid:] * h
            out["rh"] = (rh, es[:, hid:] * h.abs() + 2 * U32 * rh.abs())
            return out
        q = torch.tanh(v)
        eq = e + 4 * U32
        h, z = self.h.double()[:, :N], self.z.double()[:, :N]
        hn = (1 - z) * h + z * q
        out["q"] = (q, eq)
        out["hn"] = (hn, z.abs() * eq + 4 * U32 * ((1 - z).abs() * h.abs() + (z * q).abs() + hn.abs()))
        return out


def gamma(arith, K):
    """Relative bound of the GEMM error per unit of sum|a||w|: the arithmetic's product error plus fp32 accumulation
    (probabilistic form, lambda = 8, of the sqrt(K) u bound; K u would be the worst case)."""
    return GAMMA_PROD[arith] + (8.0 * math.sqrt(K) + 2.0) * U32


# --------------------------------------------------------------------------------------------------------------- comparator
def elementwise_ok(got, ref, bound, tau=0.0):
    """(ok, worst used share, index of the worst element)."""
    err = (got.double() - ref).abs()
    lim = bound + tau
    used = err / lim.clamp_min(1e-300)
    used = torch.where(err == 0, torch.zeros_like(used), used)
    i = int(used.argmax())
    return bool((err <= lim).all()), float(used.reshape(-1)[i]), i


def frob(a, b):
    return float((a.double() - b.double()).norm())


def judge(got, ref, bound, twins, arith, tau=0.0):
    """Both criteria on one output.  twins: {"fp32" | "bf16x3" | "bf16x1": the output recomputed from that twin's GEMM}.
    Returns (ok, report dict)."""
    ok_e, used_e, _ = elementwise_ok(got, ref, bound, tau)
    eg = frob(got, ref)
    floor = U32 * float(ref.norm()) + 1e-30
    tw = "fp32" if arith == "fp32" else "bf16x3"
    e_tw = frob(twins[tw], ref)
    e_b1 = frob(twins["bf16x1"], ref)
    r_tw = eg / (4 * e_tw + floor)
    r_b1 = eg / (e_b1 / 16 + 1e-300)
    rep = dict(elem=used_e, twin=tw, ratio_twin=eg / max(e_tw, 1e-300), ratio_b1=eg / max(e_b1, 1e-300),
               ratio_fp32=eg / max(frob(twins["fp32"], ref), 1e-300) if "fp32" in twins else float("nan"),
               ratio_b3=eg / max(frob(twins["bf16x3"], ref), 1e-300) if "bf16x3" in twins else float("nan"))
    return ok_e and r_tw <= 1.0 and r_b1 <= 1.0, rep


def last_tile_rows(rows, M, tile=64):
    """Positions in `rows` of the pixels in the last (ragged when M % tile != 0) M tile."""
    lo = (M - 1) // tile * tile
    return (rows >= lo).nonzero().flatten()


def sample_rows(B, H, W, cap, gen_seed=0, tile=64, device="cpu"):
    """Output pixels a forward check looks at: all of them when B*H*W <= cap, else every border pixel, both sides of every
    `tile`-pixel M-tile edge, the first and the last 256 pixels and random fill up to `cap`."""
    M = B * H * W
    if M <= cap:
        return torch.arange(M, device=device)
    y = torch.arange(H, device=device)
    x = torch.arange(W, device=device)
    b = torch.arange(B, device=device)
    border = torch.cat([(b[:, None] * H * W + y[None, :] * W).flatten(), (b[:, None] * H * W + y[None, :] * W + W - 1).flatten(),
                        (b[:, None] * H * W + x[None, :]).flatten(), (b[:, None] * H * W + (H - 1) * W + x[None, :]).flatten()])
    edges = torch.arange(tile, M, tile, device=device)
    g = torch.Generator(device="cpu").manual_seed(gen_seed)
    rnd = torch.randint(0, M, (cap,), generator=g).to(device)
    rows = torch.cat([border, edges, edges - 1, torch.arange(256, device=device), torch.arange(M - 256, M, device=device), rnd])
    return torch.unique(rows)


def verdict(got, epi, G, S, K, arith, twins_g, mutant_g, log=None, what=""):
    """The whole comparison of one case.  got: {output name: the kernel's values [rows, width]}; G / S: fp64 GEMM and |.| GEMM
    at the same rows; twins_g: {"fp32", "bf16x3", "bf16x1": twin GEMMs}; mutant_g: G with one 32-channel chunk of one tap
    removed in the last M tile.  Returns (ok, mutants_rejected, {output: report}).  `log(what, err, lim, detail)`: margin sink."""
    if epi.bias is not None:
        S = S + epi.bias.double().abs()
    e = gamma(arith, K) * S
    ref = epi.apply(G, e)
    tw = {k: epi.apply(v, e) for k, v in twins_g.items()}
    mut = epi.apply(mutant_g, e)
    ok, rej_a, rej_b, reports = True, False, False, {}
    for name, (r, bound) in ref.items():
        twins = {k: tw[k][name][0] for k in tw}
        o, rep = judge(got[name], r, bound, twins, arith)
        ok = ok and o
        reports[name] = rep
        rej_a = rej_a or not judge(mut[name][0], r, bound, twins, arith)[0]
        rej_b = rej_b or not judge(twins["bf16x1"], r, bound, twins, arith)[0]
        if log is not None:
            log(f"{what} {name} elementwise", rep["elem"], 1.0, f"|got-ref| / (gamma_{arith} S + tau), K {K}")
            log(f"{what} {name} frobenius vs {rep['twin']} twin", rep["ratio_twin"], 4.0,
                f"||got-ref|| / ||twin-ref||; bf16x1 ratio {rep['ratio_b1']:.3e} (limit 1/16)")
    return ok, rej_a and rej_b, reports
