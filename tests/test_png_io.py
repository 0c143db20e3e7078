"""frame_utils.writePNG / readPNG (zlib and struct only) and the KITTI functions on top of them where OpenCV is missing:
round trips, chunk CRCs, the five row filters (files written by PIL, which filters adaptively) and PIL reading what
writePNG wrote.  Host only."""
import struct
import sys
import zlib

import numpy as np
import pytest

from flow_supervisor_amd.raft_utils import frame_utils as FU

SIZES = ((1, 1), (3, 5), (37, 61))


def picture(dtype, shape, seed):
    """Smooth ramps plus noise: PIL's adaptive filter picks among all five row filters on such rows."""
    rng = np.random.default_rng(seed)
    h, w = shape[:2]
    top = np.iinfo(dtype).max
    ramp = np.add.outer(np.arange(h) * 3.0, np.arange(w) * 5.0) / max(1.0, 3.0 * h + 5.0 * w) * top
    a = ramp[..., None] * np.array([1.0, 0.6, 0.3]) + rng.integers(0, top // 16 + 1, (h, w, 1))
    a = np.clip(a, 0, top).astype(dtype)
    a[rng.random((h, w)) < 0.2] = rng.integers(0, top, endpoint=True)
    return a if len(shape) > 2 else a[..., 0]


def chunks(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, out = 8, []
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        out.append((kind, body, crc))
        pos += 12 + n
    return out


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("colour", [False, True])
@pytest.mark.parametrize("size", SIZES)
def test_round_trip_and_crcs(tmp_path, dtype, colour, size):
    x = picture(dtype, size + ((3,) if colour else ()), 11)
    path = str(tmp_path / "x.png")
    FU.writePNG(path, x)
    back = FU.readPNG(path)
    assert back.dtype == x.dtype and back.shape == x.shape and np.array_equal(back, x)
    cs = chunks(path)
    assert [k for k, _, _ in cs][0] == b"IHDR" and cs[-1][0] == b"IEND"
    for kind, body, crc in cs:
        assert crc == zlib.crc32(kind + body) & 0xFFFFFFFF, kind
    w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", cs[0][1])
    assert (w, h, depth, ctype, comp, filt, lace) == (size[1], size[0], 8 * x.dtype.itemsize, 2 if colour else 0, 0, 0, 0)
    if dtype == np.uint16:                                  # samples are big-endian in the file
        raw = zlib.decompress(b"".join(b for k, b, _ in cs if k == b"IDAT"))
        first = x.reshape(-1)[0]
        assert raw[1:3] == bytes([first >> 8, first & 255])


def test_bad_input_is_refused(tmp_path):
    path = str(tmp_path / "x.png")
    for bad in (np.zeros((3, 4), np.float32), np.zeros((3, 4, 2), np.uint8), np.zeros((0, 4), np.uint8), np.zeros(4, np.uint8)):
        with pytest.raises(ValueError):
            FU.writePNG(path, bad)
    FU.writePNG(path, np.zeros((2, 2), np.uint8))
    data = bytearray(open(path, "rb").read())
    data[20] ^= 1                                           # a bit of the IHDR body: its CRC no longer holds
    open(path, "wb").write(bytes(data))
    with pytest.raises(ValueError, match="CRC"):
        FU.readPNG(path)


def test_reads_what_pil_writes_and_pil_reads_what_this_writes(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    rgb = picture(np.uint8, (37, 61, 3), 5)
    p = str(tmp_path / "rgb.png")
    Image.fromarray(rgb).save(p)
    raw = zlib.decompress(b"".join(b for k, b, _ in chunks(p) if k == b"IDAT"))
    filters = {raw[y * (1 + 61 * 3)] for y in range(37)}
    print("row filters PIL chose for the 8-bit RGB file:", sorted(filters))
    assert np.array_equal(FU.readPNG(p), rgb)
    grey = picture(np.uint16, (37, 61), 6)
    p = str(tmp_path / "grey16.png")
    Image.fromarray(grey.astype(np.int32)).convert("I;16").save(p)
    assert struct.unpack(">IIBBBBB", chunks(p)[0][1])[2:4] == (16, 0)
    back = FU.readPNG(p)
    assert back.dtype == np.uint16 and np.array_equal(back, grey)
    rgba = np.concatenate([rgb, 255 - rgb[..., :1]], -1)
    p = str(tmp_path / "rgba.png")
    Image.fromarray(rgba).save(p)
    assert np.array_equal(FU.readPNG(p), rgba)
    for x in (rgb, rgb[..., 0]):
        p = str(tmp_path / "ours.png")
        FU.writePNG(p, x)
        assert np.array_equal(np.array(Image.open(p)), x)


def filtered_png(path, x, ftype):
    """Write uint8 [H,W,3] with every row under filter `ftype` (the forward filters of the PNG specification, restated here
    so that all five are exercised whatever an encoder would pick)."""
    h, w, _ = x.shape
    bpp, rows, prev = 3, [], np.zeros(w * 3, np.int64)
    for y in range(h):
        cur = x[y].reshape(-1).astype(np.int64)
        a = np.concatenate([np.zeros(bpp, np.int64), cur[:-bpp]])
        c = np.concatenate([np.zeros(bpp, np.int64), prev[:-bpp]])
        b = prev
        if ftype == 0:
            pred = 0
        elif ftype == 1:
            pred = a
        elif ftype == 2:
            pred = b
        elif ftype == 3:
            pred = (a + b) // 2
        else:
            p = a + b - c
            pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        rows.append(bytes([ftype]) + ((cur - pred) & 255).astype(np.uint8).tobytes())
        prev = cur
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n")
        f.write(FU._png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)))
        data = zlib.compress(b"".join(rows))
        f.write(FU._png_chunk(b"IDAT", data[:40]))          # the stream may be split over several IDAT chunks
        f.write(FU._png_chunk(b"IDAT", data[40:]))
        f.write(FU._png_chunk(b"IEND", b""))


@pytest.mark.parametrize("ftype", [0, 1, 2, 3, 4])
def test_every_row_filter_is_undone(tmp_path, ftype):
    x = picture(np.uint8, (9, 13, 3), 20 + ftype)
    p = str(tmp_path / "f.png")
    filtered_png(p, x, ftype)
    assert np.array_equal(FU.readPNG(p), x)


def test_kitti_files_without_opencv(tmp_path, monkeypatch):
    monkeypatch.setitem(sys.modules, "cv2", None)           # `import cv2` raises ImportError
    assert FU._cv2() is None
    rng = np.random.default_rng(9)
    flow = (rng.standard_normal((37, 61, 2)) * 40).astype(np.float32)
    p = str(tmp_path / "000000_10.png")
    FU.writeFlowKITTI(p, flow)
    back, valid = FU.readFlowKITTI(p)
    assert back.dtype == np.float32 and back.shape == flow.shape
    want = (np.trunc(64.0 * flow + 2 ** 15) - 2 ** 15) / 64.0          # flow rounded to 1/64, towards -2^9 as the uint16 cast does
    assert np.array_equal(back, want.astype(np.float32)) and np.abs(back - flow).max() < 1 / 64
    assert valid.shape == (37, 61) and np.all(valid == 1)
    raw = FU.readPNG(p)
    assert raw.dtype == np.uint16 and raw.shape == (37, 61, 3)
    # the device-encoded array goes to the same file
    FU.writeFlowKITTI16(str(tmp_path / "b.png"), raw.view(np.int16))
    assert open(str(tmp_path / "b.png"), "rb").read() == open(p, "rb").read()
    # disparity: a 16-bit grey file
    disp16 = rng.integers(0, 65535, (5, 7), endpoint=True).astype(np.uint16)
    FU.writePNG(str(tmp_path / "d.png"), disp16)
    d, ok = FU.readDispKITTI(str(tmp_path / "d.png"))
    assert np.array_equal(d[..., 0], -(disp16 / 256.0)) and not d[..., 1].any() and np.array_equal(ok, disp16 > 0)
