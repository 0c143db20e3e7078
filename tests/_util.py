import json
import os

import numpy as np
import torch

G = os.path.join(os.path.dirname(__file__), "golden")

# fsraft_get_tuning(key) of a freshly loaded library, as the knobs stood before they became one struct (csrc/conv_common.hpp
# ConvKnobs).  Keys 3 / 4 are the arithmetic mode (fsraft_set_arithmetic: 1 / 2 in the default mode, 0 / 0 in the exact one).
TUNING_DEFAULTS = {0: 0, 1: 0, 2: 512, 5: 1, 7: 0, 8: 1, 9: 0, 10: 1, 11: 2048, 12: 1, 13: 1, 14: 64, 15: 0, 16: 1, 17: 1024, 18: 1,
                   19: 65536, 20: 1, 21: 65536, 22: 1, 26: 1, 27: 1, 28: 1, 29: 8192, 31: 8192, 32: -1}


def load(name):
    return dict(np.load(os.path.join(G, name + ".npz")))


def shapes(name):
    return json.load(open(os.path.join(G, name + "_shapes.json")))


def T(a):
    return torch.from_numpy(np.asarray(a))


def close(a, b, atol, rtol=2e-5, what=""):
    a = (a if isinstance(a, torch.Tensor) else T(a)).detach().float().cpu()
    b = (b if isinstance(b, torch.Tensor) else T(b)).detach().float().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.isfinite(a).all(), f"{what}: non-finite values"
    err = (a - b).abs().max().item()
    ref = b.abs().max().item()
    lim = atol + rtol * ref
    log = os.environ.get("FSRAFT_PARITY_LOG")         # margins of every comparison, for profiles/*parity_margins*
    if log:
        test = os.environ.get("PYTEST_CURRENT_TEST", "").split("::")[-1].split(" ")[0]
        with open(log, "a") as f:
            f.write(f"{test}\t{what}\terr {err:.3e}\tlimit {lim:.3e} (atol {atol:g} + {rtol:g} * max|ref| {ref:.3g})\tused {err / lim if lim else 0:.3f}\n")
    assert err <= lim, f"{what}: max abs err {err:.3e} > {lim:.3e}"
    return err


def _log_margin(what, err, lim, detail):
    log = os.environ.get("FSRAFT_PARITY_LOG")
    if log:
        test = os.environ.get("PYTEST_CURRENT_TEST", "").split("::")[-1].split(" ")[0]
        with open(log, "a") as f:
            f.write(f"{test}\t{what}\terr {err:.3e}\tlimit {lim:.3e} ({detail})\tused {err / lim if lim else 0:.3f}\n")


def grad_digest_check(named_params, g, tol, prefix="gnorm.", hprefix="ghead.", skip=(), atol_norm=1e-5):
    """Every parameter-gradient norm (and, where the fixture has it, the first 32 elements) against a reference-generated
    digest.  tol: dict(gnorm, ghead, gnorm_fnet, ghead_fnet) -- the feature encoder's gradients pass through InstanceNorm
    and the volume backward and carry ~1e-3 of summation-order noise in the REFERENCE itself (measured in round 2, docs/history),
    so `fnet.*` has its own, wider pair of limits; everything else (update blocks, context encoder, GMA attention) is held
    to the tighter pair.  norm: |ours - ref| <= rtol * ref + atol_norm (atol: biases in front of InstanceNorm have a zero
    gradient in exact arithmetic and ~1e-6 of rounding noise in the reference); head: max abs error <= rtol_head *
    max|head| + the share of rtol * ref one element carries.  The worst margin of each group goes to the parity log.
    Returns the offenders."""
    import math
    bad = []
    worst = {}
    for k, p in named_params:
        if any(t in k for t in skip) or prefix + k not in g:
            continue
        grp = "fnet" if k.startswith("fnet.") else "rest"
        rn, rh = (tol["gnorm_fnet"], tol["ghead_fnet"]) if grp == "fnet" else (tol["gnorm"], tol["ghead"])
        ref = float(g[prefix + k])
        gn = 0.0 if p.grad is None else p.grad.norm().item()
        lim = rn * max(ref, 1e-6) + atol_norm
        err = abs(gn - ref)
        if err / lim >= worst.get(("n", grp), (-1.0,))[0]:
            worst[("n", grp)] = (err / lim, rn, f"{k}: {gn:.6g} vs {ref:.6g}")
        if not err <= lim:
            bad.append((k, "norm", gn, ref))
        if hprefix and hprefix + k in g and p.grad is not None and ref > 1e-4:
            head = T(g[hprefix + k]).float()
            herr = (p.grad.reshape(-1)[:32].cpu() - head).abs().max().item()
            hlim = rh * head.abs().max().item() + rn * ref / math.sqrt(p.numel()) + 1e-7
            if herr / hlim >= worst.get(("h", grp), (-1.0,))[0]:
                worst[("h", grp)] = (herr / hlim, rh, k)
            if not herr <= hlim:
                bad.append((k, "head", herr, head.abs().max().item()))
    for (kind, grp), (used, r, what) in sorted(worst.items()):
        _log_margin(f"{prefix if kind == 'n' else hprefix}* worst of {grp} ({what})", used * r, r,
                    "relative to the reference norm" if kind == "n" else "relative to max|head|")
    return bad


def rel_check(value, ref, rtol, what):
    """|value - ref| <= rtol * |ref| for scalars (losses), logged like close()."""
    err, lim = abs(float(value) - float(ref)), rtol * abs(float(ref))
    _log_margin(what, err, lim, f"{rtol:g} * |ref| {abs(float(ref)):.6g}")
    assert err <= lim, f"{what}: {float(value)!r} vs reference {float(ref)!r} (rel {err / max(abs(float(ref)), 1e-30):.2e} > {rtol:g})"


PATTERN = 0x7FC0FFEE            # guard rows and unwritten outputs: a NaN, so a read of one shows as well
GUARD = 64                      # floats per guard row (256 bytes: the payload keeps the allocation's alignment)


class Buf:
    """A flat fp32 device buffer of n floats between two guard rows.  src: a CPU tensor to hold (an input); otherwise the payload
    is PATTERN (an output) or zero.  offset: floats the payload is moved off its 16-byte alignment by."""

    def __init__(self, src=None, n=None, zero=False, offset=0):
        self.n = src.numel() if src is not None else n
        self.off = GUARD + offset
        self.whole = torch.empty(self.n + 2 * GUARD + offset, device="cuda", dtype=torch.float32)
        self.whole.view(torch.int32).fill_(PATTERN)
        self.mid = self.whole[self.off:self.off + self.n]
        assert self.mid.data_ptr() % 16 == 4 * (offset % 4)
        if src is not None:
            self.mid.copy_(src.reshape(-1).float())
        elif zero:
            self.mid.zero_()

    def cpu(self):
        return self.mid.cpu()

    def intact(self):
        w = self.whole.view(torch.int32)
        assert bool((w[:self.off] == PATTERN).all()) and bool((w[self.off + self.n:] == PATTERN).all()), "a guard row was written"

    def written(self, upto=None):
        """Guards intact and no pattern left in the payload (in its first `upto` floats; the rest still all pattern)."""
        self.intact()
        m = self.mid.view(torch.int32)
        upto = self.n if upto is None else upto
        assert not bool((m[:upto] == PATTERN).any()), "an output element was not written"
        assert bool((m[upto:] == PATTERN).all()), "an output that was not asked for was written"

    def untouched(self):
        assert bool((self.whole.view(torch.int32) == PATTERN).all()), "a refused call wrote an output"
