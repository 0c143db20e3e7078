"""Launch-sequence recorder: one ordered log of every libfsraft call and every ATen operator of a run, forward and backward.

For refactors of the Python above the kernels: run it on the old tree and on the new one and `diff -r` the two directories; an
identical log means the same library calls with the same integer / float arguments and the same null pointers, between the same
framework operators with the same output shapes, in the same order.  Nothing here synchronises, and nothing else imports this.

    python scripts/call_log.py OUT_DIR [scenario ...]        (GPU box; no names = every scenario; one OUT_DIR/<scenario>.log each)

Library calls are caught by putting a proxy in front of the loaded handle (`_lib._lib`); ATen operators by a TorchDispatchMode,
which the autograd engine carries into its backward threads.  Pointer VALUES never reach the log (they differ run to run), only
whether a pointer is null; integer fields of structures passed by reference are logged, arrays of ints by value.
"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from torch.utils._python_dispatch import TorchDispatchMode  # noqa: E402
from torch.utils._pytree import tree_leaves  # noqa: E402

from flow_supervisor_amd import _lib  # noqa: E402

DEV = "cuda"
LOG = []
_NUM = (ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double)


def _num(v):
    v = getattr(v, "value", v)
    return f"{v:.9g}" if isinstance(v, float) else str(v)


def _null(v):
    return "null" if not getattr(v, "value", v) else "ptr"


def _fields(s):
    out = []
    for name, typ in s._fields_:
        v = getattr(s, name)
        if typ is ctypes.c_void_p:
            out.append(f"{name}={_null(v)}")
        elif typ in _NUM:
            out.append(f"{name}={_num(v)}")
        elif issubclass(typ, ctypes.Array):
            out.append(f"{name}=[{','.join(_null(x) if typ._type_ is ctypes.c_void_p else _num(x) for x in v)}]")
    return "{" + " ".join(out) + "}"


def _arg(a, typ):
    if typ is ctypes.c_void_p:
        return _null(a)
    if typ in _NUM or isinstance(a, (int, float)):       # (a symbol without a signature: plain numbers still by value)
        return _num(a)
    obj = getattr(a, "_obj", a)                     # byref(x) -> x
    if isinstance(obj, ctypes.Structure):
        return _fields(obj)
    if isinstance(obj, ctypes.Array):
        if isinstance(obj[0] if len(obj) else 0, ctypes.Structure):
            return "[" + " ".join(_fields(x) for x in obj) + "]"
        if obj._type_ in _NUM:
            return "[" + ",".join(_num(x) for x in obj) + "]"
        return f"[{len(obj)} ptrs]"
    return "null" if not a else "ref"                # a cast pointer to an array built elsewhere


class _Handle:
    """In front of the ctypes handle: every fsraft_* call goes to LOG before it runs."""

    def __init__(self, lib):
        self._real = lib

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("fsraft_"):
            return fn
        types = _lib.SIGNATURES.get(name) or [None] * 64

        def logged(*args):
            LOG.append(f"lib  {name}(" + ", ".join(_arg(a, t) for a, t in zip(args, types)) + ")")
            return fn(*args)
        self.__dict__[name] = logged
        return logged


class _Aten(TorchDispatchMode):
    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        shapes = [tuple(t.shape) for t in tree_leaves(out) if isinstance(t, torch.Tensor)]
        LOG.append(f"aten {func} -> {shapes}")
        return out


# ----------------------------------------------------------------------------- scenarios
def _ns(**kw):
    return argparse.Namespace(**{**dict(small=False, mixed_precision=False, alternate_corr=False, dropout=0), **kw})


def _gma_ns():
    return _ns(num_heads=1, position_only=False, position_and_content=False)


def _pair(B, H, W):
    return torch.rand(B, 3, H, W, device=DEV) * 255, torch.rand(B, 3, H, W, device=DEV) * 255


def _crops(B, ox, oy, H=128, W=192, h=96, w=128):
    c1, c2 = _pair(B, H, W)
    xs, ys = (ox if isinstance(ox, list) else [ox] * B), (oy if isinstance(oy, list) else [oy] * B)
    cut = lambda c: torch.cat([c[i:i + 1, :, ys[i]:ys[i] + h, xs[i]:xs[i] + w] for i in range(B)]).contiguous()
    return cut(c1), cut(c2), c1, c2, ox, oy


def _train(model, call, sup_k=None):
    from flow_supervisor_amd.train import raft_sequence_loss
    model = model.to(DEV).train()
    model.freeze_bn()

    def run():
        preds = call(model)
        if sup_k is None:
            loss = raft_sequence_loss(preds)
        else:       # the promise behind sup_grad_samples: the supervisor's predictions of the samples behind k get no gradient
            half = len(preds) // 2
            loss = raft_sequence_loss(preds[:half]) + raft_sequence_loss([p[:sup_k] for p in preds[half:]])
        loss.backward()
    return run


def _test(model, call):
    model = model.to(DEV).eval()

    def run():
        with torch.no_grad():
            call(model)
    return run


def _block(alt, fmap_grad):
    """A bare block looked up both ways (flow, channels-last; coordinates, NCHW) with coordinates that require grad: the
    coordinate gradient with and without the feature maps' (the second lookup's stash entry changes convention)."""
    from flow_supervisor_amd.core.corr import AlternateCorrBlock, CorrBlock
    from flow_supervisor_amd.core.utils.utils import coords_grid
    f1, f2 = (torch.randn(2, 256, 16, 24, device=DEV).requires_grad_(fmap_grad) for _ in range(2))
    flow = (torch.randn(2, 2, 16, 24, device=DEV) * 2).requires_grad_()
    grid = coords_grid(2, 16, 24, device=DEV)

    def run():
        blk = AlternateCorrBlock(f1, f2, coords_grad=True) if alt else CorrBlock(f1, f2)
        (blk(flow, channels_last=True, is_flow=True).sum() + blk(flow + grid).sum()).backward()
    return run


def scenarios():
    from flow_supervisor_amd.core.gma_l2l import GMAL2L
    from flow_supervisor_amd.core.gma_network import RAFTGMA
    from flow_supervisor_amd.core.l2l import L2L
    from flow_supervisor_amd.core.raft import RAFT
    from flow_supervisor_amd.core.raft_dropin import ReferenceShapedRAFT
    S = {}
    one = lambda m: m(*_pair(1, 128, 192), iters=3)
    for overlap in (True, False):
        sfx = "" if overlap else "_one_stream"
        S["raft" + sfx] = (overlap, lambda: _train(RAFT(_ns()), one))
        S["l2l" + sfx] = (overlap, lambda: _train(L2L(_ns()), lambda m: m(*_crops(2, 16, 8), iters=5)))
        S["gma_l2l" + sfx] = (overlap, lambda: _train(GMAL2L(_gma_ns()), lambda m: m(*_crops(2, 16, 8), iters=5)))
    S["raft_small"] = (True, lambda: _train(RAFT(_ns(small=True)), one))
    S["raft_alt"] = (True, lambda: _train(RAFT(_ns(alternate_corr=True)), one))
    S["raft_alt_coords_grad"] = (True, lambda: _train(RAFT(_ns(alternate_corr=True, alt_coords_grad=True)), one))
    S["gma"] = (True, lambda: _train(RAFTGMA(_gma_ns()), one))
    S["gma_alternate_corr_flag"] = (True, lambda: _train(RAFTGMA(argparse.Namespace(**{**vars(_gma_ns()), "alternate_corr": True})), one))   # (the GMA networks ignore the flag)
    S["dropin"] = (True, lambda: _train(ReferenceShapedRAFT(_ns()), one))
    for name, cls, ns in (("l2l", L2L, _ns), ("gma_l2l", GMAL2L, _gma_ns)):
        S[name + "_no_supervisor_grad"] = (True, lambda cls=cls, ns=ns: _train(
            cls(ns()), lambda m: m(*_crops(2, 16, 8), iters=5, supervisor_grad=False)))
        S[name + "_sup_grad_samples"] = (True, lambda cls=cls, ns=ns: _train(
            cls(ns()), lambda m: m(*_crops(2, 16, 8), iters=5, sup_grad_samples=1), sup_k=1))
        S[name + "_iters1"] = (True, lambda cls=cls, ns=ns: _train(cls(ns()), lambda m: m(*_crops(2, 16, 8), iters=1)))
        S[name + "_test_mode"] = (True, lambda cls=cls, ns=ns: _test(cls(ns()), lambda m: m(*_pair(1, 128, 192), iters=3, test_mode=True)))
    S["l2l_offsets_per_sample"] = (True, lambda: _train(L2L(_ns()), lambda m: m(*_crops(2, [0, 24], [16, 8]), iters=5)))
    S["raft_test_mode"] = (True, lambda: _test(RAFT(_ns()), lambda m: m(*_pair(1, 128, 192), iters=3, test_mode=True)))
    S["raft_test_mode_flow_init"] = (True, lambda: _test(RAFT(_ns()), lambda m: m(
        *_pair(1, 128, 192), iters=3, test_mode=True, flow_init=torch.randn(1, 2, 16, 24, device=DEV))))
    S["gma_test_mode"] = (True, lambda: _test(RAFTGMA(_gma_ns()), lambda m: m(*_pair(1, 128, 192), iters=3, test_mode=True)))
    for alt in (False, True):
        S[("altcorr" if alt else "corr") + "_coords_grad_only"] = (True, lambda alt=alt: _block(alt, False))
        S[("altcorr" if alt else "corr") + "_coords_and_fmap_grad"] = (True, lambda alt=alt: _block(alt, True))
    return S


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("out_dir")
    ap.add_argument("names", nargs="*")
    a = ap.parse_args()
    from flow_supervisor_amd.core import streams
    _lib._lib = _Handle(_lib.load())
    os.makedirs(a.out_dir, exist_ok=True)
    S = scenarios()
    for name in a.names or list(S):
        overlap, make = S[name]
        streams.OVERLAP = overlap
        torch.manual_seed(7)
        run = make()                    # (model construction and input generation stay out of the log)
        del LOG[:]
        with _Aten():
            run()
        with open(os.path.join(a.out_dir, name + ".log"), "w") as f:
            f.write("\n".join(LOG) + "\n")
        print(f"{name}: {len(LOG)} lines", flush=True)


if __name__ == "__main__":
    main()
