"""Host restatement of the PNG-file stage (include/tce_rvos_pngfile.h): THE FILE around a zlib stream, built from png.chunk, and the
register-level pieces of the header's two identities -- raw (the CRC register from a zero start, no final xor), mul (the product in
GF(2)[x] mod G) and X (x^k mod G), all in the reflected representation -- in plain Python, with the combination the two launches
make (segment_raw, combined_crc) restated from them."""
import struct

POLY = 0xEDB88320
ONE = 0x80000000   # x^0: bit 31 is the coefficient of x^0
IEND = bytes([0, 0, 0, 0, 0x49, 0x45, 0x4E, 0x44, 0xAE, 0x42, 0x60, 0x82])

_TABLE = []
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ (POLY if _c & 1 else 0)
    _TABLE.append(_c)


def file_bytes(head, data):
    """head, the IDAT chunk of data, the IEND chunk"""
    from tce_rvos_amd import png
    return bytes(head) + png.chunk(b"IDAT", bytes(data)) + png.chunk(b"IEND", b"")


def raw(data, start=0):
    """the register after `data` from `start` (0: the zero start of the identities), without the final xor"""
    c = start
    for b in bytes(data):
        c = (c >> 8) ^ _TABLE[(c ^ b) & 255]
    return c


def mul(a, b):
    p = 0
    for _ in range(32):
        if a & 0x80000000:
            p ^= b
        a = (a << 1) & 0xFFFFFFFF
        b = (b >> 1) ^ (POLY if b & 1 else 0)
    return p


def X(k):
    """x^k mod G by square and multiply"""
    r, base = ONE, 0x40000000
    while k:
        if k & 1:
            r = mul(r, base)
        base = mul(base, base)
        k >>= 1
    return r


def combine(raw_a, raw_b, len_b):
    """raw(A || B) from raw(A), raw(B) and len(B)"""
    return mul(raw_a, X(8 * len_b)) ^ raw_b


def crc32_from_raw(raw_m, len_m, init_term=True):
    """crc32(M) from raw(M); init_term=False leaves the initial-value term out (the wrong formula the zero strings tell apart)"""
    return (mul(0xFFFFFFFF, X(8 * len_m)) if init_term else 0) ^ raw_m ^ 0xFFFFFFFF


def segment_raw(data, piece, segment):
    """raw of one segment's bytes the way the first launch takes it: segment // piece pieces laid from the segment's END (only the
    first piece in use can be short), every piece multiplied by the constant shift for the whole pieces behind it, the xor of all"""
    data = bytes(data)
    lanes, pad = segment // piece, segment - len(data)
    assert 0 < len(data) <= segment
    out = 0
    for q in range(lanes):
        e = (q + 1) * piece - pad
        if e > 0:
            out ^= mul(raw(data[max(0, e - piece):e]), X(8 * piece * (lanes - 1 - q)))
    return out


def combined_crc(data, piece, segment):
    """the IDAT chunk's CRC-32 the way the two launches make it: K = the register after "IDAT" from the initial value, the full
    segments in front of the last one a constant shift apart, the last segment behind x^(8 * its length), the final xor"""
    data = bytes(data)
    n = len(data)
    acc = raw(b"IDAT", 0xFFFFFFFF)
    if n == 0:
        return acc ^ 0xFFFFFFFF
    F = (n - 1) // segment
    xseg = X(8 * segment)
    for s in range(F):
        acc = mul(acc, xseg) ^ segment_raw(data[s * segment:(s + 1) * segment], piece, segment)
    last = data[F * segment:]
    return mul(acc, X(8 * len(last))) ^ segment_raw(last, piece, segment) ^ 0xFFFFFFFF


def be32(v):
    return struct.pack(">I", v & 0xFFFFFFFF)
