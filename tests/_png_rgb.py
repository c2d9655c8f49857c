"""Host restatement of the RGB half of the PNG stage (include/tce_rvos_vis.h): the per-row filter choice of
tce_png_filter_rgb_u8 and the stream of tce_png_deflate_rows_u8.  The filters are written from section 9 of the PNG specification,
one byte at a time; the blocks are tests/_png_dyn.py's (strip_block takes a strip's bytes as they are).  It shares nothing with the
kernel or with tce_rvos_amd/png.py."""
import zlib

import numpy as np

import _png as R
import _png_dyn as D

BPP = 3


def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    if pa <= pb and pa <= pc:
        return a
    return b if pb <= pc else c


def filter_row(t, cur, up):
    """bytes of a row filtered with type t; cur, up: the raw bytes of the row and of the row above (zeros for the first row)"""
    out = bytearray(len(cur))
    for i, x in enumerate(cur):
        a = cur[i - BPP] if i >= BPP else 0
        b = up[i]
        c = up[i - BPP] if i >= BPP else 0
        pred = (0, a, b, (a + b) // 2, paeth(a, b, c))[t]
        out[i] = (x - pred) & 255
    return bytes(out)


def cost(data):
    """the sum of the absolute values of the bytes read as signed 8-bit"""
    return sum(v if v < 128 else 256 - v for v in data)


def filtered_rows(img):
    """uint8 [H,W,3] -> uint8 [H,1+3W]: per row the type with the least cost (a tie: the lowest type) and the row filtered with it"""
    img = np.asarray(img, dtype=np.uint8)
    H, W, _ = img.shape
    flat = [bytes(r) for r in img.reshape(H, 3 * W)]
    rows = np.zeros((H, 1 + 3 * W), np.uint8)
    for y in range(H):
        up = flat[y - 1] if y else bytes(3 * W)
        cands = [filter_row(t, flat[y], up) for t in range(5)]
        costs = [cost(c) for c in cands]
        t = costs.index(min(costs))
        rows[y, 0] = t
        rows[y, 1:] = np.frombuffer(cands[t], np.uint8)
    return rows


def unfilter(rows, W):
    """the inverse: filtered rows [H,1+3W] (bytes or array) -> uint8 [H,W,3]"""
    rows = np.frombuffer(bytes(rows), np.uint8).reshape(-1, 1 + 3 * W) if not isinstance(rows, np.ndarray) else rows
    H = rows.shape[0]
    out = np.zeros((H, 3 * W), np.int64)
    for y in range(H):
        t = int(rows[y, 0])
        assert 0 <= t <= 4, t
        for i in range(3 * W):
            a = out[y, i - BPP] if i >= BPP else 0
            b = out[y - 1, i] if y else 0
            c = out[y - 1, i - BPP] if (y and i >= BPP) else 0
            pred = (0, a, b, (a + b) // 2, paeth(a, b, c))[t]
            out[y, i] = (int(rows[y, 1 + i]) + pred) & 255
    return out.astype(np.uint8).reshape(H, W, 3)


def rows_stream(rows, rows_per_strip):
    """the complete zlib stream of filtered rows [H,R], the bytes as they are -> (bytes, one info per strip)"""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    out, pair, infos = b"\x78\x01", (1, 0), []
    for y in range(0, rows.shape[0], rows_per_strip):
        data = rows[y:y + rows_per_strip].tobytes()
        block, info = D.strip_block(data)
        out += block
        infos.append(info)
        pair = R.adler_combine(pair, R.adler32(data), len(data))
    a, b = pair
    return out + b"\x03\x00" + bytes([b >> 8, b & 255, a >> 8, a & 255]), infos


def fixed_cost(rows, rows_per_strip):
    """bytes of the stream with every strip's block written with the fixed code"""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    return 2 + sum(len(R.strip_bytes(rows[y:y + rows_per_strip].tobytes())) for y in range(0, rows.shape[0], rows_per_strip)) + 6


def decode_file(blob):
    """A PNG file of colour type 2, bit depth 8 -> uint8 [H,W,3], by its chunks, zlib and un-filtering"""
    import struct
    assert blob[:8] == b"\x89PNG\r\n\x1a\n"
    at, idat, size = 8, b"", None
    while at < len(blob):
        n, kind = struct.unpack(">I4s", blob[at:at + 8])
        data = blob[at + 8:at + 8 + n]
        assert struct.unpack(">I", blob[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + data) & 0xFFFFFFFF
        if kind == b"IHDR":
            w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", data)
            assert (depth, ctype, comp, filt, lace) == (8, 2, 0, 0, 0)
            size = (h, w)
        elif kind == b"IDAT":
            idat += data
        at += 12 + n
    H, W = size
    raw = zlib.decompress(idat)
    assert len(raw) == H * (1 + 3 * W)
    return unfilter(raw, W)


# ---------------------------------------------------------------------------------------------------------------- images
def images(H, W, seed):
    """constant, ramp + seeded noise, uniform random bytes: uint8 [3,H,W,3]"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    ramp = np.stack([3 * x + y, 2 * y + 40, x + 2 * y + 90], -1) + rng.integers(-2, 3, (H, W, 3))
    return np.stack([np.full((H, W, 3), 77, np.uint8), np.clip(ramp, 0, 255).astype(np.uint8),
                     rng.integers(0, 256, (H, W, 3), dtype=np.uint8)])
