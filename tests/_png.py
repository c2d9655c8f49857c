"""Plain numpy / Python restatement of the device's PNG stream (include/tce_rvos_png.h): RLE-only deflate
with the fixed Huffman code of RFC 1951, PNG filter type 0 on every row, strips of rows_per_strip rows that are independent of
each other, and the Adler-32 of the filtered bytes.  Written from the rule's text, one token at a time into a list of bits; it
shares nothing with the kernel or with tce_rvos_amd/png.py."""
import numpy as np

LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
ADLER = 65521


def value_map(plane, nonzero_value):
    plane = np.asarray(plane, dtype=np.uint8)
    return plane if nonzero_value == 0 else np.where(plane != 0, nonzero_value, 0).astype(np.uint8)


def filtered_rows(plane, nonzero_value):
    """[H,W] -> [H,W+1]: filter type 0 in front of every row of value-mapped bytes"""
    m = value_map(plane, nonzero_value)
    return np.concatenate([np.zeros((m.shape[0], 1), np.uint8), m], axis=1)


def filtered_bytes(plane, nonzero_value):
    return filtered_rows(plane, nonzero_value).tobytes()


class Bits:
    """bits fill bytes from the least significant bit"""

    def __init__(self):
        self.bits = []

    def huffman(self, code, n):      # most significant bit first
        self.bits.extend((code >> (n - 1 - k)) & 1 for k in range(n))

    def extra(self, value, n):       # least significant bit first
        self.bits.extend((value >> k) & 1 for k in range(n))

    def pad(self):
        self.bits.extend([0] * (-len(self.bits) % 8))

    def symbol(self, x):
        if x < 144:
            self.huffman(0x30 + x, 8)
        elif x < 256:
            self.huffman(0x190 + (x - 144), 9)
        elif x < 280:
            self.huffman(x - 256, 7)
        else:
            self.huffman(0xC0 + (x - 280), 8)

    def match(self, length):
        i = max(k for k in range(len(LENGTH_BASE)) if LENGTH_BASE[k] <= length)
        if length == 258:
            i = 28
        self.symbol(257 + i)
        self.extra(length - LENGTH_BASE[i], LENGTH_EXTRA[i])
        self.huffman(0, 5)           # distance 1: code 0, no extra bits

    def tobytes(self):
        assert len(self.bits) % 8 == 0
        return np.packbits(np.array(self.bits, np.uint8), bitorder="little").tobytes() if self.bits else b""


def run_tokens(out, b, L):
    out.symbol(b)
    r = L - 1
    while r >= 261 or r == 258:
        out.match(258)
        r -= 258
    if r in (259, 260):
        out.match(r - 3)
        r = 3
    if r >= 3:
        out.match(r)
    else:
        for _ in range(r):
            out.symbol(b)


def runs_of(data):
    """maximal runs (value, length) of a byte string"""
    a = np.frombuffer(data, np.uint8)
    starts = np.flatnonzero(np.concatenate([[True], a[1:] != a[:-1]]))
    ends = np.concatenate([starts[1:], [a.size]])
    return [(int(a[s]), int(e - s)) for s, e in zip(starts, ends)]


def strip_bytes(data):
    """one strip's block: fixed block, tokens, end of block, stored-block header, zero bits to the byte boundary, 00 00 FF FF"""
    out = Bits()
    out.extra(0, 1)                  # BFINAL = 0
    out.extra(1, 2)                  # BTYPE = 01
    for b, L in runs_of(data):
        run_tokens(out, b, L)
    out.symbol(256)
    out.extra(0, 1)
    out.extra(0, 2)
    out.pad()
    return out.tobytes() + b"\x00\x00\xff\xff"


def adler32(data):
    a, b = 1, 0
    for x in data:
        a = (a + x) % ADLER
        b = (b + a) % ADLER
    return a, b


def adler_combine(p1, p2, len2):
    (a1, b1), (a2, b2) = p1, p2
    return (a1 + a2 - 1) % ADLER, (b1 + b2 + len2 * (a1 - 1)) % ADLER


def stream(plane, rows_per_strip, nonzero_value):
    """the complete zlib stream of one [H,W] plane"""
    rows = filtered_rows(plane, nonzero_value)
    out, pair = b"\x78\x01", (1, 0)
    for y in range(0, rows.shape[0], rows_per_strip):
        data = rows[y:y + rows_per_strip].tobytes()
        out += strip_bytes(data)
        pair = adler_combine(pair, adler32(data), len(data))
    last = Bits()
    last.extra(1, 1)
    last.extra(1, 2)
    last.symbol(256)
    last.pad()
    a, b = pair
    return out + last.tobytes() + bytes([b >> 8, b & 255, a >> 8, a & 255])


def strip_bound(n):
    return (9 * n + 13 + 7) // 8 + 4


def stream_bound(H, W, S):
    full, rest = divmod(H, S)
    return 2 + full * strip_bound(S * (W + 1)) + (strip_bound(rest * (W + 1)) if rest else 0) + 2 + 4


def blob(H, W, seed=0):
    """a rectangular blob with a ragged edge: what a mask looks like"""
    rng = np.random.default_rng(seed)
    m = np.zeros((H, W), np.uint8)
    y0, y1, x0, x1 = H // 4, max(H // 4 + 1, 3 * H // 4), W // 5, max(W // 5 + 1, 4 * W // 5)
    for y in range(y0, y1):
        m[y, max(0, x0 - int(rng.integers(0, 3))):min(W, x1 + int(rng.integers(0, 3)))] = 1
    return m


def all_run_lengths(W, lo=1, hi=264):
    """rows of W bytes that hold a run of every length lo .. hi (alternating 0 and a value), one after the other: -> [H,W]"""
    data = np.concatenate([np.full(L, (k & 1) * (7 + k % 200), np.uint8) for k, L in enumerate(range(lo, hi + 1))])
    H = -(-data.size // W)
    return np.concatenate([data, np.full(H * W - data.size, 201, np.uint8)]).reshape(H, W)
