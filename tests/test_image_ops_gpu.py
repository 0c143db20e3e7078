"""raft_tf.image (crop_bboxes, pad_bboxes, resize, resize_flow, pad_edge, pad_inputs, unpad_inputs) under autograd against
tests/_imageref.py, its refusals, and the BOX_OPS switch of core/l2l.py: _pad_state and _crop_back give the same bits, forward and
backward, with the switch on and off (function level: other kernels of a whole step sum through atomics)."""
import pytest
import torch

import _imageref as R
from _util import _log_margin

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _leave_no_cached_segments():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def image():
    from flow_supervisor_amd import raft_tf
    return raft_tf.image


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _lay(t, layout):
    """A canonical [B,H,W,C] CPU tensor as a device tensor of `layout`."""
    return (t if layout == "nhwc" else t.permute(0, 3, 1, 2).contiguous()).cuda()


def _canon(t, layout):
    return (t if layout == "nhwc" else t.permute(0, 2, 3, 1)).detach().cpu()


YX = [(0, 0), (4, 6), (2, 3)]            # B = 3: 5 x 6 windows of 9 x 12 frames


def _nodes(outs):
    return {o.grad_fn for o in outs}


@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_crop_and_pad_lists_are_one_node_each_and_unused_members_get_zeros(image, layout):
    frames = [R.box_values(3, 9, 12, 2, i) for i in range(3)]
    dev = [_lay(f, layout).requires_grad_(True) for f in frames]
    crops = image.crop_bboxes(dev, YX, (5, 6), layout)
    assert isinstance(crops, list) and len(crops) == 3 and len(_nodes(crops)) == 1
    for c, f in zip(crops, frames):
        assert _same_bits(_canon(c, layout), R.crop_ref(f, YX, (5, 6)))
    up = [R.box_values(3, 5, 6, 2, 10 + i) for i in range(3)]
    (crops[0] * _lay(up[0], layout)).sum().add((crops[2] * _lay(up[2], layout)).sum()).backward()
    for i in (0, 2):
        assert _same_bits(_canon(dev[i].grad, layout), R.pad_ref(up[i], YX, (9, 12)))
    assert dev[1].grad is not None and bool((_bits(dev[1].grad) == 0).all())
    # pad_bboxes: a single tensor comes back as a tensor, its backward is the crop
    w = _lay(up[0], layout).requires_grad_(True)
    padded = image.pad_bboxes(w, torch.tensor(YX), torch.tensor((9, 12)), layout)
    assert isinstance(padded, torch.Tensor) and _same_bits(_canon(padded, layout), R.pad_ref(up[0], YX, (9, 12)))
    padded.backward(_lay(frames[0], layout))
    assert _same_bits(_canon(w.grad, layout), R.crop_ref(frames[0], YX, (5, 6)))
    _log_margin(f"crop_bboxes / pad_bboxes under autograd {layout}", 0.0, 0.0, "exact")


def test_a_list_over_32_is_split(image):
    frames = [R.box_values(3, 9, 12, 1, i).cuda().requires_grad_(True) for i in range(33)]
    crops = image.crop_bboxes(frames, YX, (5, 6))
    assert len(crops) == 33 and len(_nodes(crops)) == 2
    for i in (0, 31, 32):
        assert _same_bits(crops[i].cpu(), R.crop_ref(frames[i].detach().cpu(), YX, (5, 6)))


@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_resize_and_resize_flow_under_autograd(image, layout):
    b, hi, wi, c, ho, wo = R.SURFACE
    xs, gs = R.surface_inputs()
    for scaling in (False, True):
        fac = R.flow_factors(hi, wi, ho, wo) if scaling else None
        dev = [_lay(x, layout).requires_grad_(True) for x in xs]
        outs = image.resize_flow(dev, (ho, wo), True, layout) if scaling else image.resize(dev, (ho, wo), layout)
        assert isinstance(outs, list) and len(_nodes(outs)) == 1
        torch.autograd.backward([outs[0], outs[2]], [_lay(gs[0], layout), _lay(gs[2], layout)])
        for i in range(3):
            ev, eg = R.resize_expect(xs[i], gs[i], (ho, wo), fac)
            w = R.need(_canon(outs[i], layout), *ev[:3])[0]
            _log_margin(f"resize{'_flow' if scaling else ''} value member {i} {layout}", w, R.LIMITS["rs_val"], "worst |got - ref| / scale")
            assert w <= R.LIMITS["rs_val"], (i, w)
            if i == 1:
                assert bool((_bits(dev[1].grad) == 0).all())
                continue
            w = R.need(_canon(dev[i].grad, layout), *eg[:3])[0]
            _log_margin(f"resize{'_flow' if scaling else ''} gradient member {i} {layout}", w, R.LIMITS["rs_grad"], "worst |got - ref| / scale")
            assert w <= R.LIMITS["rs_grad"], (i, w)
    single = image.resize_flow(_lay(xs[0], layout), torch.tensor((ho, wo)), True, layout)
    assert isinstance(single, torch.Tensor) and _same_bits(single, image.resize_flow([_lay(xs[0], layout)], (ho, wo), True, layout)[0])


def test_identity_resize_returns_the_same_object(image):
    x = torch.randn(2, 8, 16, 2, device="cuda", requires_grad=True)
    assert image.resize(x, (8, 16)) is x and image.resize_flow(x, (8, 16)) is x
    assert image.resize(x, image.get_proc_size((5, 9))) is x
    lst = [x, x.detach()]
    assert image.resize(lst, (8, 16)) is lst
    p = x.detach().permute(0, 3, 1, 2)
    assert image.resize(p, (8, 16), "nchw") is p
    assert image.get_proc_size((436, 1024)) == (440, 1024) and image.get_proc_size((5, 9), 4) == (8, 12)


@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("mode", ("sintel", None))
def test_unpad_of_pad_inputs_is_the_input_bit_for_bit(image, mode, layout):
    im1, im2, flow = R.box_values(2, 5, 9, 3), R.box_values(2, 5, 9, 3, 1), R.box_values(2, 5, 9, 2, 2)
    dev = [_lay(t, layout) for t in (im1, im2, flow)]
    out, pad = image.pad_inputs(*dev, mode=mode, layout=layout)
    assert pad == R.input_padding_ref(5, 9, mode)
    pads = (pad[1][0], pad[1][1], pad[2][0], pad[2][1])
    for o, t in zip(out, (im1, im2, flow)):
        assert _same_bits(_canon(o, layout), R.pad_edge_ref(t, pads)) and not o.requires_grad
    back = image.unpad_inputs(*out, pad=pad, layout=layout)
    for v, o, d in zip(back, out, dev):
        assert _same_bits(v, d) and v.data_ptr() >= o.data_ptr() and v._base is not None
    assert _same_bits(_canon(image.pad_edge(dev[2], pad, layout), layout), R.pad_edge_ref(flow, pads))
    _log_margin(f"pad_inputs / unpad_inputs mode {mode} {layout}", 0.0, 0.0, "exact")


def test_refusals(image):
    x = torch.randn(3, 9, 12, 2)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        image.crop_bboxes(x, YX, (5, 6))
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        image.resize(x, (8, 8))
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        image.pad_inputs(x)
    d = x.cuda()
    with pytest.raises(RuntimeError, match="crop_yx is read on the host"):
        image.crop_bboxes(d, torch.tensor(YX).cuda(), (5, 6))
    with pytest.raises(RuntimeError, match="crop_yx is read on the host"):
        image.pad_bboxes(d, torch.tensor(YX).cuda(), (20, 20))
    with pytest.raises(ValueError, match="does not fit"):
        image.crop_bboxes(d, [(0, 0), (5, 6), (2, 3)], (5, 6))              # one row past the bottom
    with pytest.raises(ValueError, match="does not fit"):
        image.pad_bboxes(d, [(0, 0), (0, 0), (0, 1)], (9, 12))              # one column past the right edge
    with pytest.raises(ValueError, match="does not fit"):
        image.crop_bboxes(d, [(0, 0), (-1, 0), (2, 3)], (5, 6))
    with pytest.raises(ValueError, match="share one shape"):
        image.crop_bboxes([d, d[:, :8]], YX, (5, 6))
    with pytest.raises(ValueError, match="share one shape"):
        image.resize([d, d[..., :1]], (8, 8))
    with pytest.raises(ValueError, match="layout"):
        image.resize(d, (8, 8), layout="hwc")
    with pytest.raises(RuntimeError):
        image.crop_bboxes(d, YX[:2], (5, 6))                                # two offsets for three samples


# ------------------------------------------------------------------------------------------------- the BOX_OPS switch of core/l2l.py
CROP, FRAME, N_PRED = (16, 24), (32, 40), 12
PER_SAMPLE = ([8, 16, 0], [0, 16, 8])          # ox, oy: three distinct windows
EQUAL = ([8, 8, 8], [16, 16, 16])


def _l2l_run(l2l, on, ox, oy):
    l2l_was = l2l.BOX_OPS
    l2l.BOX_OPS = on
    try:
        g = torch.Generator().manual_seed(5)
        net = torch.randn(3, CROP[0] // 8, CROP[1] // 8, 128, generator=g).cuda().requires_grad_(True)
        flow = torch.randn(3, 2, CROP[0] // 8, CROP[1] // 8, generator=g).cuda().requires_grad_(True)
        pn, pf = l2l._pad_state(net, flow, ox, oy, CROP, FRAME)
        torch.autograd.backward([pn, pf], [torch.randn(pn.shape, generator=g).cuda(), torch.randn(pf.shape, generator=g).cuda()])
        preds = [torch.randn(3, 2, *FRAME, generator=g).cuda().requires_grad_(True) for _ in range(N_PRED)]
        crops = l2l._crop_back(preds, ox, oy, CROP)
        ups = [torch.randn(3, 2, *CROP, generator=g).cuda() for _ in range(N_PRED)]
        torch.autograd.backward(crops[:-1], ups[:-1])         # the last prediction's window is not used
        return dict(values=[pn, pf] + list(crops), grads=[net.grad, flow.grad] + [p.grad for p in preds[:-1]], last=preds[-1].grad,
                    nodes=len({c.grad_fn for c in crops}))
    finally:
        l2l.BOX_OPS = l2l_was


@pytest.mark.parametrize("offsets", (PER_SAMPLE, EQUAL), ids=("per_sample", "equal"))
def test_l2l_pad_state_and_crop_back_same_bits_with_box_ops_on_and_off(offsets):
    from flow_supervisor_amd.core import l2l
    assert l2l.BOX_OPS in (True, False)
    ox, oy = offsets
    on, off = _l2l_run(l2l, True, ox, oy), _l2l_run(l2l, False, ox, oy)
    assert tuple(on["values"][0].shape) == (3, FRAME[0] // 8, FRAME[1] // 8, 128) and tuple(on["values"][1].shape) == (3, 2, FRAME[0] // 8, FRAME[1] // 8)
    for k in ("values", "grads"):
        assert len(on[k]) == len(off[k])
        for a, b in zip(on[k], off[k]):
            assert _same_bits(a, b), k
    for r in (on, off):
        assert r["last"] is None or bool((_bits(r["last"]) == 0).all())
    if offsets is PER_SAMPLE:
        assert on["nodes"] == 1 and off["nodes"] == N_PRED
    _log_margin(f"l2l._pad_state / _crop_back BOX_OPS on against off, {'per-sample' if offsets is PER_SAMPLE else 'equal'} offsets", 0.0, 0.0,
                "exact, forward and backward")
