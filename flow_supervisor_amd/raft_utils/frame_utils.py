"""Flow file IO with the reference's names (pytorch/raft_utils/frame_utils.py): host-side data formats either side of the
path.  Pure numpy; nothing here touches the device.

  readFlow / writeFlow      Middlebury .flo (frame_utils.py:14-33, 74-103): float32 tag 202021.25, int32 width, int32
                            height, then height x width interleaved (u, v) float32, all little-endian
  readPFM                   frame_utils.py:36-71
  readFlowKITTI / writeFlowKITTI / readDispKITTI   16-bit PNG triplets (frame_utils.py:106-125) through OpenCV, which the
                            reference imports at module level -- here it is imported on first use, and where it is not
                            installed the files go through writePNG / readPNG below
  writePNG / readPNG        8- and 16-bit grey / RGB PNG files with zlib and struct only (no reference counterpart)
  writeFlowKITTI16          the KITTI file from the array fsraft_flow_kitti16 encoded on the device
  read_gen                 dispatch on the file extension (frame_utils.py:128-142)
"""
import re
import struct
import zlib
from os.path import splitext

import numpy as np

TAG_FLOAT = 202021.25
TAG_CHAR = np.array([TAG_FLOAT], np.float32)


def readFlow(fn):
    """[H,W,2] float32, or None (with the reference's message) when the tag is wrong."""
    with open(fn, "rb") as f:
        magic = np.frombuffer(f.read(4), "<f4")
        if magic.size != 1 or magic[0] != np.float32(TAG_FLOAT):
            print("Magic number incorrect. Invalid .flo file")
            return None
        w, h = (int(v) for v in np.frombuffer(f.read(8), "<i4"))
        data = np.frombuffer(f.read(8 * w * h), "<f4")
    return np.resize(data, (h, w, 2))


def writeFlow(filename, uv, v=None):
    """uv: [H,W,2], or the u plane with v given separately."""
    if v is None:
        uv = np.asarray(uv)
        assert uv.ndim == 3 and uv.shape[2] == 2
        u, v = uv[:, :, 0], uv[:, :, 1]
    else:
        u, v = np.asarray(uv), np.asarray(v)
    assert u.shape == v.shape
    h, w = u.shape
    with open(filename, "wb") as f:
        f.write(TAG_CHAR.astype("<f4").tobytes())
        f.write(np.array([w, h], "<i4").tobytes())
        f.write(np.stack([u, v], axis=-1).astype("<f4").tobytes())


def readPFM(file):
    with open(file, "rb") as f:
        header = f.readline().rstrip()
        if header == b"PF":
            color = True
        elif header == b"Pf":
            color = False
        else:
            raise Exception("Not a PFM file.")
        m = re.match(rb"^(\d+)\s(\d+)\s$", f.readline())
        if not m:
            raise Exception("Malformed PFM header.")
        width, height = int(m.group(1)), int(m.group(2))
        scale = float(f.readline().rstrip())
        endian = "<" if scale < 0 else ">"
        data = np.fromfile(f, endian + "f")
    return np.flipud(np.reshape(data, (height, width, 3) if color else (height, width)))


def _cv2():
    """OpenCV, or None where it is not installed (the KITTI functions then go through writePNG / readPNG)."""
    try:
        import cv2
    except ImportError:
        return None
    cv2.setNumThreads(0)
    cv2.ocl.setUseOpenCL(False)
    return cv2


_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"


def _png_chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def writePNG(filename, array):
    """array: uint8 or uint16, [H,W] (grey) or [H,W,3] (RGB) -> a non-interlaced PNG of bit depth 8 / 16 with big-endian
    samples, every row unfiltered (filter type 0)."""
    a = np.asarray(array)
    if a.dtype not in (np.uint8, np.uint16) or not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)) or 0 in a.shape:
        raise ValueError(f"writePNG: uint8 / uint16 [H,W] or [H,W,3] expected, got {a.dtype} {a.shape}")
    h, w = a.shape[:2]
    rows = np.ascontiguousarray(a.astype(">u2" if a.dtype == np.uint16 else np.uint8)).view(np.uint8).reshape(h, -1)
    raw = np.concatenate([np.zeros((h, 1), np.uint8), rows], axis=1).tobytes()
    with open(filename, "wb") as f:
        f.write(_PNG_MAGIC)
        f.write(_png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8 * a.dtype.itemsize, 0 if a.ndim == 2 else 2, 0, 0, 0)))
        f.write(_png_chunk(b"IDAT", zlib.compress(raw, 6)))
        f.write(_png_chunk(b"IEND", b""))


def _png_unfilter(data, h, stride, bpp):
    """Undo the five row filters of the PNG specification (none, sub, up, average, Paeth).  bpp: bytes per whole pixel."""
    out = np.zeros((h, stride), np.uint8)
    prev = np.zeros(stride, np.int64)
    pos = 0
    for y in range(h):
        ft = data[pos]
        line = np.frombuffer(data, np.uint8, stride, pos + 1).astype(np.int64)
        pos += 1 + stride
        if ft == 0:
            cur = line
        elif ft == 2:
            cur = (line + prev) & 255
        elif ft == 1:                    # sub: a running sum along each byte lane of the pixel
            cur = (np.cumsum(line.reshape(-1, bpp), axis=0) & 255).reshape(-1)
        elif ft in (3, 4):               # average, Paeth: the byte bpp to the left is an output, one running pass per row
            ln, up, res = line.tolist(), prev.tolist(), [0] * stride
            for i in range(stride):
                a = res[i - bpp] if i >= bpp else 0
                b = up[i]
                if ft == 3:
                    pred = (a + b) >> 1
                else:
                    c = up[i - bpp] if i >= bpp else 0
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                res[i] = (ln[i] + pred) & 255
            cur = np.array(res, np.int64)
        else:
            raise ValueError(f"readPNG: unknown row filter {ft}")
        out[y] = cur
        prev = cur
    return out


def readPNG(filename):
    """A non-interlaced PNG of bit depth 8 or 16 and colour type 0 (grey), 2 (RGB) or 6 (RGBA) -> uint8 / uint16 [H,W],
    [H,W,3] or [H,W,4].  Chunk CRCs are verified; palette and interlaced files are refused."""
    with open(filename, "rb") as f:
        data = f.read()
    if data[:8] != _PNG_MAGIC:
        raise ValueError(f"readPNG: {filename} is not a PNG file")
    pos, header, idat = 8, None, []
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] != zlib.crc32(kind + body) & 0xFFFFFFFF:
            raise ValueError(f"readPNG: {filename}: CRC mismatch in chunk {kind!r}")
        pos += 12 + n
        if kind == b"IHDR":
            header = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            break
    if header is None:
        raise ValueError(f"readPNG: {filename}: no IHDR chunk")
    w, h, depth, ctype, _, _, interlace = header
    if depth not in (8, 16) or ctype not in (0, 2, 6) or interlace:
        raise ValueError(f"readPNG: {filename}: bit depth {depth}, colour type {ctype}, interlace {interlace} is not supported")
    ch = {0: 1, 2: 3, 6: 4}[ctype]
    bpp = ch * depth // 8
    px = _png_unfilter(zlib.decompress(b"".join(idat)), h, w * bpp, bpp)
    img = px.view(">u2").astype(np.uint16) if depth == 16 else px
    return img.reshape(h, w) if ch == 1 else img.reshape(h, w, ch)


def readFlowKITTI(filename):
    cv2 = _cv2()
    if cv2 is None:
        raw = readPNG(filename)[:, :, :3].astype(np.float32)
    else:
        raw = cv2.imread(filename, cv2.IMREAD_ANYDEPTH | cv2.IMREAD_COLOR)[:, :, ::-1].astype(np.float32)
    return (raw[:, :, :2] - 2 ** 15) / 64.0, raw[:, :, 2]


def readDispKITTI(filename):
    cv2 = _cv2()
    if cv2 is None:
        raw = readPNG(filename)
        disp = (raw if raw.ndim == 2 else raw[:, :, 0]) / 256.0
    else:
        disp = cv2.imread(filename, cv2.IMREAD_ANYDEPTH) / 256.0
    return np.stack([-disp, np.zeros_like(disp)], -1), disp > 0.0


def writeFlowKITTI(filename, uv):
    cv2 = _cv2()
    uv = 64.0 * uv + 2 ** 15
    out = np.concatenate([uv, np.ones([uv.shape[0], uv.shape[1], 1])], axis=-1).astype(np.uint16)
    if cv2 is None:
        writePNG(filename, out)
    else:
        cv2.imwrite(filename, out[..., ::-1])


def writeFlowKITTI16(filename, rgb16):
    """rgb16: uint16 [H,W,3] = (64 u + 2^15, 64 v + 2^15, valid), what fsraft_flow_kitti16 encodes on the device (ops.flow_kitti16;
    an int16 array of the same bits is taken as such) -> the 16-bit PNG writeFlowKITTI would have written."""
    a = np.asarray(rgb16)
    if a.dtype == np.int16:
        a = a.view(np.uint16)
    if a.dtype != np.uint16 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"writeFlowKITTI16: uint16 [H,W,3] expected, got {a.dtype} {a.shape}")
    cv2 = _cv2()
    if cv2 is None:
        writePNG(filename, a)
    else:
        cv2.imwrite(filename, a[..., ::-1])


def read_gen(file_name, pil=False):
    ext = splitext(file_name)[-1]
    if ext in (".png", ".jpeg", ".ppm", ".jpg"):
        from PIL import Image
        return Image.open(file_name)
    if ext in (".bin", ".raw"):
        return np.load(file_name)
    if ext == ".flo":
        return readFlow(file_name).astype(np.float32)
    if ext == ".pfm":
        flow = readPFM(file_name).astype(np.float32)
        return flow if flow.ndim == 2 else flow[:, :, :-1]
    return []
