"""float64 restatement of the image plumbing of the reference's TensorFlow tree -- util/image.py:6-49 crop_bboxes / pad_bboxes,
raft/__init__.py:199-222 get_proc_size / resize / resize_flow (tf.image.resize's default: bilinear, half-pixel centres, no
antialias), util/pad.py pad_edge and util/validate.py:301-325 pad_inputs / unpad_inputs -- in the form csrc/image_ops.hip computes
them, with the inputs the GPU tests use, an fp32 twin and analytic error scales (tests/test_imageref.py on the CPU,
tests/test_image_kernels.py and tests/test_image_ops_gpu.py against the kernels).  Plain torch on the CPU; tensors are [B,H,W,C].
TensorFlow is not installed anywhere here: test_imageref.py holds the restatement to independent formulations (F.interpolate and
its autograd gradient, the literal op sequence of resize_flow, slicing, F.pad, np.pad); parity with TensorFlow itself is unpinned.

Resize, per axis, the index arithmetic in float32 as TensorFlow's kernel does it and the rest in float64 (the convention of
_supaugref):
  scale = f32(n_in) / f32(n_out);  in = (f32(o) + 0.5) * scale - 0.5, the product and the difference rounded separately
  lo = max(floor(in), 0), hi = min(ceil(in), n_in - 1), lerp = in - floor(in)
  value = top + (bottom - top) * lerp_y, top = tl + (tr - tl) * lerp_x;  times factor[c] where factors are given
  (resize_flow: factor = (f32(W_out) / f32(W_in), f32(H_out) / f32(H_in)) on (x, y))
  backward = the transpose: source i receives (1 - lerp) from the destinations whose lo is i and lerp from those whose hi is i (1
  where lo == hi: the forward value is then tl itself); a source no tap reaches receives +0.0

Comparator: _tailref.need(got, ref, scale, slack) <= LIMITS[key], u = 2^-24, every scale elementwise:
  rs_val   u * |factor| * (the lerp form over |x| with every difference a - b counted as |a| + |b|): a + (b - a) * l rounds b - a
           relative to |a| + |b| and the sum relative to its operands, whatever weight 1 - l the corner a ends up with, so the
           weighted mean of |x| (which goes to 0 with 1 - l) is not the magnitude TensorFlow's own float32 kernel errs by
  rs_grad  u * |factor| * (the same transpose of |g|); 0 where no tap reaches, so anything but 0 there is an excess over scale 0
Box copies and edge padding are exact (no limit): they move bits.

LIMITS are 4 x the worst value the fp32 TWIN (the value: the lerp form with every operation rounded to fp32, along y first and then
along x, which is not the kernel's order; the gradient: separable matrices holding 1 - lerp and lerp, applied as two fp32 matrix
products) reaches against float64 over ALL_RUNS -- the very inputs the two GPU files launch -- rounded up to one significant digit
(_tailref.limit_from_twin).  The kernels' own worst values are in profiles/image_ops_margins.txt; they do not set the limits.
"""
import itertools

import torch

from _tailref import U24, _gen, limit_from_twin, need  # noqa: F401

LAYOUTS = ("nhwc", "nchw")
B = 2
# Hi, Wi, Ho, Wo: one pixel up; the get_proc_size case and back; 17 x 9 -> 4 x 3 skips sources; the workgroup edge at 255 / 256 /
# 257 source columns (the backward) into 256; equal sizes
RESIZE_CASES = ((1, 1, 3, 5), (5, 7, 8, 8), (8, 8, 5, 7), (17, 9, 4, 3), (2, 255, 3, 256), (2, 256, 3, 256), (2, 257, 3, 256), (5, 7, 5, 7))
CHANNELS = (1, 2, 3)
LIST_N = (1, 32)
SURFACE = (3, 16, 24, 2, 20, 40)          # B, Hi, Wi, C, Ho, Wo of tests/test_image_ops_gpu.py

TWIN_WORST = dict(rs_val=2.20, rs_grad=3.01)
LIMITS = dict(rs_val=9.0, rs_grad=20.0)


# ----------------------------------------------------------------------------------------------------------------------- resize
def taps(n_in, n_out):
    """(lo int64, hi int64, lerp float32) of every destination index, the arithmetic in float32."""
    o = torch.arange(n_out, dtype=torch.float32)
    scale = torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32)
    pos = (o + 0.5) * scale
    pos = pos - 0.5
    fl = torch.floor(pos)
    return fl.clamp_min(0).long(), torch.ceil(pos).clamp_max(n_in - 1).long(), pos - fl


def flow_factors(hi, wi, ho, wo):
    """(W_out / W_in, H_out / H_in) in float32 (raft/__init__.py:218-219), as python floats."""
    f = torch.tensor([float(wo), float(ho)], dtype=torch.float32) / torch.tensor([float(wi), float(hi)], dtype=torch.float32)
    return [float(f[0]), float(f[1])]


def _corners(x, size, dtype):
    x = x.to(dtype)
    ylo, yhi, ly = taps(x.shape[1], size[0])
    xlo, xhi, lx = taps(x.shape[2], size[1])
    ly, lx = ly.to(dtype)[None, :, None, None], lx.to(dtype)[None, None, :, None]
    return x[:, ylo][:, :, xlo], x[:, ylo][:, :, xhi], x[:, yhi][:, :, xlo], x[:, yhi][:, :, xhi], ly, lx


def resize_ref(x, size, factors=None, dtype=torch.float64, rows_first=False):
    """[B,Hi,Wi,C] -> [B,Ho,Wo,C], the lerp form as TensorFlow writes it: along x, then along y.  rows_first: along y, then along
    x (the twin's order)."""
    tl, tr, bl, br, ly, lx = _corners(x, size, dtype)
    if rows_first:
        left, right = tl + (bl - tl) * ly, tr + (br - tr) * ly
        v = left + (right - left) * lx
    else:
        top, bot = tl + (tr - tl) * lx, bl + (br - bl) * lx
        v = top + (bot - top) * ly
    return v * torch.tensor(factors, dtype=dtype) if factors is not None else v


def resize_mag(x, size, factors=None):
    """The magnitude of the terms of the lerp form, float64: every difference a - b counted as |a| + |b|.  a + (b - a) * l rounds
    b - a relative to |a| + |b| and the sum relative to its operands, whatever the weight 1 - l that a ends up with."""
    tl, tr, bl, br, ly, lx = _corners(x.abs(), size, torch.float64)
    top, bot = tl + (tr + tl) * lx, bl + (br + bl) * lx
    v = top + (bot + top) * ly
    return v * torch.tensor([abs(f) for f in factors], dtype=torch.float64) if factors is not None else v


def interp_matrix(n_in, n_out, dtype=torch.float64):
    """[n_out, n_in]: row o holds 1 - lerp at lo(o) and lerp at hi(o), 1 where they meet."""
    lo, hi, lerp = taps(n_in, n_out)
    lerp = lerp.to(dtype)
    A = torch.zeros(n_out, n_in, dtype=dtype)
    r = torch.arange(n_out)
    same = lo == hi
    A[r, lo] = torch.where(same, torch.ones_like(lerp), 1 - lerp)
    A[r[~same], hi[~same]] = lerp[~same]
    return A


def resize_matrix(x, size, factors=None, dtype=torch.float64):
    """The same function as two matrix products (the twin's form in fp32; in float64 the scale's form)."""
    Ay, Ax = interp_matrix(x.shape[1], size[0], dtype), interp_matrix(x.shape[2], size[1], dtype)
    v = torch.einsum("oy,byxc->boxc", Ay, x.to(dtype))
    v = torch.einsum("px,boxc->bopc", Ax, v)
    return v * torch.tensor(factors, dtype=dtype) if factors is not None else v


def resize_bwd_ref(g, size, factors=None, dtype=torch.float64):
    """[B,Ho,Wo,C] upstream -> [B,Hi,Wi,C]: the transpose."""
    Ay, Ax = interp_matrix(size[0], g.shape[1], dtype), interp_matrix(size[1], g.shape[2], dtype)
    g = g.to(dtype)
    if factors is not None:
        g = g * torch.tensor(factors, dtype=dtype)
    v = torch.einsum("oy,boxc->byxc", Ay, g)
    return torch.einsum("px,bypc->byxc", Ax, v)


def reached(n_in, n_out):
    """bool [n_in]: the sources some destination tap reaches."""
    lo, hi, _ = taps(n_in, n_out)
    m = torch.zeros(n_in, dtype=torch.bool)
    m[lo] = True
    m[hi] = True
    return m


def resize_inputs(case, C, i=0):
    """(x [B,Hi,Wi,C], upstream g [B,Ho,Wo,C]) fp32 of list member i."""
    hi, wi, ho, wo = case
    gen = _gen(23, hi, wi, ho, wo, C, i)
    return 3.0 * torch.randn(B, hi, wi, C, generator=gen), torch.randn(B, ho, wo, C, generator=gen)


def resize_expect(x, g, size, factors=None):
    """(value entry, gradient entry), each (ref, scale, slack, key)."""
    af = [abs(f) for f in factors] if factors is not None else None
    v = resize_ref(x, size, factors)
    d = resize_bwd_ref(g, x.shape[1:3], factors)
    return ((v, U24 * resize_mag(x, size, factors), 0.0, "rs_val"),
            (d, U24 * resize_bwd_ref(g.abs(), x.shape[1:3], af), 0.0, "rs_grad"))


def twin_needs(x, g, size, factors=None):
    ev, eg = resize_expect(x, g, size, factors)
    tv = resize_ref(x, size, factors, torch.float32, rows_first=True)
    tg = resize_bwd_ref(g, x.shape[1:3], factors, torch.float32)
    return dict(rs_val=need(tv, *ev[:3])[0], rs_grad=need(tg, *eg[:3])[0])


def resize_variants():
    """(case, C, with factors) of the kernel tests; the flow factors go with two channels."""
    return [(case, C, fac) for case, C in itertools.product(RESIZE_CASES, CHANNELS) for fac in ((False, True) if C == 2 else (False,))]


def case_factors(case, fac):
    return flow_factors(*case) if fac else None


def surface_inputs():
    b, hi, wi, c, ho, wo = SURFACE
    gen = _gen(29, *SURFACE)
    return [3.0 * torch.randn(b, hi, wi, c, generator=gen) for _ in range(3)], [torch.randn(b, ho, wo, c, generator=gen) for _ in range(3)]


def all_runs():
    """(x, g, size, factors) of every resize launch the GPU tests compare."""
    runs = []
    for case, C, fac in resize_variants():
        for i in range(max(LIST_N)):
            x, g = resize_inputs(case, C, i)
            runs.append((x, g, case[2:], case_factors(case, fac)))
    xs, gs = surface_inputs()
    b, hi, wi, c, ho, wo = SURFACE
    for x, g in zip(xs, gs):
        runs.append((x, g, (ho, wo), None))
        runs.append((x, g, (ho, wo), flow_factors(hi, wi, ho, wo)))
    return runs


def resize_flow_literal(flow, size, scaling=True):
    """raft/__init__.py:213-222 op for op (torch for tf) over resize_ref, in the dtype of `flow`."""
    flow_size = torch.tensor([float(flow.shape[-3]), float(flow.shape[-2])], dtype=torch.float32)
    out = resize_ref(flow, size, None, flow.dtype) if tuple(flow.shape[1:3]) != tuple(size) else flow
    if scaling:
        scale = torch.tensor([float(size[0]), float(size[1])], dtype=torch.float32) / flow_size
        scale = torch.stack([scale[1], scale[0]]).reshape(1, 1, 1, 2)
        out = out * scale.to(flow.dtype)
    return out


# ------------------------------------------------------------------------------------------------------ box copies, edge padding
def crop_ref(x, yx, size):
    """util/image.py:6-25: [B,Hf,Wf,C] -> [B,h,w,C]."""
    h, w = size
    out = torch.empty(x.shape[0], h, w, x.shape[3], dtype=x.dtype)
    for b, (y0, x0) in enumerate(yx):
        for y in range(h):
            out[b, y] = x[b, y0 + y, x0:x0 + w]
    return out


def pad_ref(x, yx, size):
    """util/image.py:28-49: [B,h,w,C] -> [B,Hf,Wf,C], +0.0 outside the window."""
    out = torch.zeros(x.shape[0], size[0], size[1], x.shape[3], dtype=x.dtype)
    for b, (y0, x0) in enumerate(yx):
        for y in range(x.shape[1]):
            out[b, y0 + y, x0:x0 + x.shape[2]] = x[b, y]
    return out


def pad_edge_ref(x, pads):
    """np.pad(x, ((0,0), (top, bottom), (left, right), (0,0)), 'edge') as an index clamp."""
    top, bottom, left, right = pads
    ys = (torch.arange(x.shape[1] + top + bottom) - top).clamp(0, x.shape[1] - 1)
    xs = (torch.arange(x.shape[2] + left + right) - left).clamp(0, x.shape[2] - 1)
    return x[:, ys][:, :, xs]


def input_padding_ref(ht, wd, mode=None):
    """util/validate.py:302-309."""
    pad_ht = (((ht // 8) + 1) * 8 - ht) % 8
    pad_wd = (((wd // 8) + 1) * 8 - wd) % 8
    if mode == 'sintel':
        return [[0, 0], [pad_ht // 2, pad_ht - pad_ht // 2], [pad_wd // 2, pad_wd - pad_wd // 2], [0, 0]]
    return [[0, 0], [0, pad_ht], [pad_wd // 2, pad_wd - pad_wd // 2], [0, 0]]


def box_values(B_, H, W, C, i=0):
    """[B,H,W,C] fp32, every element a distinct non-zero value with every byte in use (a bit-exact copy is then told from any
    other element, and from the +0.0 fill)."""
    n = B_ * H * W * C
    v = (torch.arange(n, dtype=torch.float64) + 1.0 + 7919.0 * i) * 1.000123 + 0.37
    return v.float().view(B_, H, W, C)
