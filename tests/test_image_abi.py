"""The argument checks of csrc/image_ops.hip, on the CPU: every entry answers FSRAFT_ERR_ARG (1) -- before any HIP call, so this
runs without a GPU -- for null pointers, a list length outside 1..32, non-positive sizes and a window outside its frame.  The
device pointers are made-up numbers: a refused call never reads through them."""
import ctypes

import pytest

ERR_ARG = 1
FAKE = 0x7F0000001000          # 16-byte aligned, never dereferenced


@pytest.fixture(scope="module")
def L():
    from flow_supervisor_amd import _lib
    _lib.load()
    return _lib


def table(n, null_at=None):
    arr = (ctypes.c_void_p * max(n, 1))(*[None if i == null_at else FAKE + 4096 * i for i in range(max(n, 1))])
    return ctypes.cast(arr, ctypes.POINTER(ctypes.c_void_p)), arr


NHWC = lambda H, W, C: (H * W * C, 1, W * C, C)       # noqa: E731


def box(L, src="ok", dst="ok", n=2, place=0, B=2, C=2, Hf=8, Wf=10, H=4, W=5, yx=(0, 0, 4, 5)):
    s, k1 = table(n, 0 if src == "entry" else None)
    d, k2 = table(n, n - 1 if dst == "entry" else None)
    offs = (ctypes.c_int * len(yx))(*yx) if yx is not None else None
    return L.load().fsraft_box_copy(None if src is None else s, None if dst is None else d, n, place, B, C, Hf, Wf, H, W, offs,
                                    *NHWC(Hf, Wf, C), *NHWC(H, W, C), None)


def resize(L, fn, src="ok", dst="ok", n=2, B=2, C=2, Hi=5, Wi=7, Ho=8, Wo=8, fac=None):
    s, k1 = table(n, 0 if src == "entry" else None)
    d, k2 = table(n, n - 1 if dst == "entry" else None)
    f = (ctypes.c_float * len(fac))(*fac) if fac is not None else None
    return getattr(L.load(), fn)(None if src is None else s, None if dst is None else d, n, B, C, Hi, Wi, Ho, Wo,
                                 *NHWC(Hi, Wi, C), *NHWC(Ho, Wo, C), f, None)


def pad(L, src="ok", dst="ok", n=2, B=2, C=2, H=5, W=9, pads=(1, 2, 3, 4)):
    s, k1 = table(n, 0 if src == "entry" else None)
    d, k2 = table(n, n - 1 if dst == "entry" else None)
    t, b, l, r = pads
    return L.load().fsraft_pad_edge(None if src is None else s, None if dst is None else d, n, B, C, H, W, t, b, l, r,
                                    *NHWC(H, W, C), *NHWC(H + t + b, W + l + r, C), None)


RESIZES = ("fsraft_resize_bilinear_fwd", "fsraft_resize_bilinear_bwd")


@pytest.mark.parametrize("place", (0, 1))
def test_box_copy_refuses(L, place):
    for kw in (dict(src=None), dict(dst=None), dict(src="entry"), dict(dst="entry"), dict(yx=None),
               dict(n=0), dict(n=33), dict(n=-1),
               dict(B=0), dict(C=0), dict(H=0), dict(W=0), dict(Hf=0), dict(Wf=0), dict(H=-4), dict(C=-1),
               dict(H=9), dict(W=11),                                   # a window larger than the frame
               dict(yx=(0, 0, 5, 5)), dict(yx=(0, 0, 4, 6)),            # one row / one column past the bottom-right corner
               dict(yx=(-1, 0, 0, 0)), dict(yx=(0, -1, 0, 0)),
               dict(C=2 ** 16, Hf=2 ** 8, Wf=2 ** 8)):                  # C * Hf * Wf = 2^32
        assert box(L, place=place, **kw) == ERR_ARG, kw


@pytest.mark.parametrize("fn", RESIZES)
def test_resize_refuses(L, fn):
    for kw in (dict(src=None), dict(dst=None), dict(src="entry"), dict(dst="entry"),
               dict(n=0), dict(n=33), dict(n=-1),
               dict(B=0), dict(B=65536), dict(C=0), dict(Hi=0), dict(Wi=0), dict(Ho=0), dict(Wo=0), dict(Ho=-8),
               dict(C=9, fac=[1.0] * 9),
               dict(C=2 ** 16, Ho=2 ** 8, Wo=2 ** 8)):
        assert resize(L, fn, **kw) == ERR_ARG, kw


def test_pad_edge_refuses(L):
    for kw in (dict(src=None), dict(dst=None), dict(src="entry"), dict(dst="entry"),
               dict(n=0), dict(n=33), dict(n=-1),
               dict(B=0), dict(B=65536), dict(C=0), dict(H=0), dict(W=0), dict(W=-9),
               dict(pads=(-1, 0, 0, 0)), dict(pads=(0, -1, 0, 0)), dict(pads=(0, 0, -1, 0)), dict(pads=(0, 0, 0, -1)),
               dict(pads=(2 ** 31 - 1, 0, 0, 0)), dict(C=2 ** 10, H=2 ** 10, W=2 ** 10, pads=(2 ** 10, 0, 0, 0))):
        assert pad(L, **kw) == ERR_ARG, kw
