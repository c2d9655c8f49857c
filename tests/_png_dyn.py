"""Plain Python restatement of the device's PNG stream with codes = "dynamic" (include/tce_rvos_png.h):
the stream of tests/_png.py in which every strip's block is written either with the fixed Huffman code or with a code of its own
(BTYPE = 10), whichever takes fewer bits.  Written from the rule's text: the tree is a list of symbol groups that are merged, a
symbol's code length is the number of merges it took part in.  It shares the token rule, the bit writer and the Adler pair with
_png.py and nothing with the kernel or with tce_rvos_amd/png.py."""
from collections import deque

import _png as R

CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
NLITLEN = 286
FIXED_LEN = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 6


def code_lengths(counts, limit):
    """Code lengths of the symbols with a non-zero count -> (lengths, how often the counts had to be halved).  Huffman's algorithm
    with two queues over the symbols sorted by (count, symbol): of two equal weights a leaf goes before a merged node, merged nodes
    stay in the order they were made.  Too deep: every count c becomes (c + 1) >> 1, and again."""
    w, halved = list(counts), 0
    while True:
        leaves = deque((c, [s]) for c, s in sorted((c, s) for s, c in enumerate(w) if c > 0))
        merged = deque()
        lens = [0] * len(w)
        if len(leaves) == 1:                     # (no stream has such a code)
            lens[leaves[0][1][0]] = 1
            return lens, halved

        def take():
            if leaves and (not merged or leaves[0][0] <= merged[0][0]):
                return leaves.popleft()
            return merged.popleft()

        while len(leaves) + len(merged) > 1:
            (wa, sa), (wb, sb) = take(), take()
            for s in sa + sb:
                lens[s] += 1
            merged.append((wa + wb, sa + sb))
        if max(lens) <= limit:
            return lens, halved
        w = [(c + 1) >> 1 for c in w]
        halved += 1


def canonical(lens):
    """RFC 1951 section 3.2.2: codes in order of (length, symbol)"""
    codes, code, prev = [0] * len(lens), 0, 0
    for n, s in sorted((n, s) for s, n in enumerate(lens) if n):
        code <<= n - prev
        codes[s], prev = code, n
        code += 1
    return codes


def length_sequence_symbols(seq):
    """The code lengths seq as symbols of the code-length alphabet, (symbol, extra value, extra bits), greedily from the left.  A run
    of zeros: 18 for the longest piece of 11 .. 138 while at least 11 are left, then 17 for 3 .. 10, else single zeros.  A run of a
    length v > 0: v once, then 16 for the longest piece of 3 .. 6 while at least 3 are left, then single v."""
    out, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        r = j - i
        if v == 0:
            while r >= 11:
                t = min(r, 138)
                out.append((18, t - 11, 7))
                r -= t
            if r >= 3:
                out.append((17, r - 3, 3))
                r = 0
        else:
            out.append((v, 0, 0))
            r -= 1
            while r >= 3:
                t = min(r, 6)
                out.append((16, t - 3, 2))
                r -= t
        out.extend([(v, 0, 0)] * r)
        i = j
    return out


class Tokens:
    """takes the tokens of _png.run_tokens: (literal/length symbol, extra value, extra bits)"""

    def __init__(self):
        self.tokens = []

    def symbol(self, x):
        self.tokens.append((x, 0, 0))

    def match(self, length):
        i = 28 if length == 258 else max(k for k in range(29) if R.LENGTH_BASE[k] <= length)
        self.tokens.append((257 + i, length - R.LENGTH_BASE[i], R.LENGTH_EXTRA[i]))


def strip_block(data):
    """one strip -> (its bytes, what was decided and built on the way)"""
    toks = Tokens()
    for b, L in R.runs_of(data):
        R.run_tokens(toks, b, L)
    toks.symbol(256)
    counts = [0] * NLITLEN
    for s, _, _ in toks.tokens:
        counts[s] += 1
    extra = sum(e for _, _, e in toks.tokens)
    matches = sum(1 for s, _, _ in toks.tokens if s > 256)
    fixed_bits = 3 + sum(c * n for c, n in zip(counts, FIXED_LEN)) + extra + 5 * matches

    lens, halved = code_lengths(counts, 15)
    nlit = max(s for s in range(NLITLEN) if counts[s]) + 1
    seq_syms = length_sequence_symbols(lens[:nlit] + [1])        # the distance code: symbol 0 alone, one bit
    cl_counts = [0] * 19
    for s, _, _ in seq_syms:
        cl_counts[s] += 1
    cl_lens, cl_halved = code_lengths(cl_counts, 7)
    ncl = max(4, 1 + max(k for k in range(19) if cl_lens[CL_ORDER[k]]))
    dyn_bits = (3 + 5 + 5 + 4 + 3 * ncl + sum(cl_lens[s] + e for s, _, e in seq_syms)
                + sum(c * n for c, n in zip(counts, lens)) + extra + matches)
    info = {"kind": "dynamic" if dyn_bits < fixed_bits else "fixed", "fixed_bits": fixed_bits, "dynamic_bits": dyn_bits,
            "counts": counts, "lens": lens, "halved": halved, "nlit": nlit, "cl_lens": cl_lens, "cl_halved": cl_halved, "ncl": ncl,
            "cl_symbols": sorted({s for s, _, _ in seq_syms})}
    if info["kind"] == "fixed":
        block = R.strip_bytes(data)
        assert 8 * (len(block) - 4) - 7 <= fixed_bits + 3 <= 8 * (len(block) - 4)
        return block, info

    out = R.Bits()
    out.extra(0, 1)                  # BFINAL = 0
    out.extra(2, 2)                  # BTYPE = 10
    out.extra(nlit - 257, 5)         # HLIT
    out.extra(0, 5)                  # HDIST: one distance code
    out.extra(ncl - 4, 4)            # HCLEN
    for k in range(ncl):
        out.extra(cl_lens[CL_ORDER[k]], 3)
    cl_codes = canonical(cl_lens)
    for s, x, e in seq_syms:
        out.huffman(cl_codes[s], cl_lens[s])
        out.extra(x, e)
    codes = canonical(lens)
    for s, x, e in toks.tokens:      # ends with symbol 256
        out.huffman(codes[s], lens[s])
        out.extra(x, e)
        if s > 256:
            out.huffman(0, 1)        # distance 1: symbol 0 of the one-bit code
    assert len(out.bits) == dyn_bits
    out.extra(0, 1)                  # the stored block behind every strip
    out.extra(0, 2)
    out.pad()
    return out.tobytes() + b"\x00\x00\xff\xff", info


def stream(plane, rows_per_strip, nonzero_value):
    """the complete zlib stream of one [H,W] plane -> (bytes, one info per strip)"""
    rows = R.filtered_rows(plane, nonzero_value)
    out, pair, infos = b"\x78\x01", (1, 0), []
    for y in range(0, rows.shape[0], rows_per_strip):
        data = rows[y:y + rows_per_strip].tobytes()
        block, info = strip_block(data)
        out += block
        infos.append(info)
        pair = R.adler_combine(pair, R.adler32(data), len(data))
    a, b = pair
    return out + b"\x03\x00" + bytes([b >> 8, b & 255, a >> 8, a & 255]), infos


def kinds(infos):
    return [i["kind"] for i in infos]


# ------------------------------------------------------------------------------------------------- planes that take the hard paths
def spread(counts):
    """bytes with the given count per value, no two equal neighbours (the most frequent value fills every other place first)"""
    import numpy as np
    vals = [v for v, c in sorted(counts.items(), key=lambda kv: (-kv[1], kv[0])) for _ in range(c)]
    out = np.zeros(len(vals), np.uint8)
    half = (len(vals) + 1) // 2
    out[0::2], out[1::2] = vals[:half], vals[half:]
    assert (out[1:] != out[:-1]).all()
    return out


def fibonacci_plane(k=17):
    """one row whose literals 1 .. k have the counts 2, 3, 5, 8, ...: with the filter byte and symbol 256, once each, the counts
    are Fibonacci's and the Huffman tree is a chain k + 1 deep"""
    fib = [2, 3]
    while len(fib) < k:
        fib.append(fib[-1] + fib[-2])
    return spread({v + 1: c for v, c in enumerate(fib)})[None]


def skewed_lengths_plane():
    """one row of 1022 bytes over the values 1 .. 83 with counts 2^(10 - l): with the filter byte and symbol 256 (once each,
    l = 10) the code has 1, 3, 13, 8, 5, 21, 34 symbols of the lengths l = 2, 4, 5, 7, 8, 9, 10.  Those are the counts of seven
    symbols of the header's code-length code; length 1 (the distance code) comes once and 18 twice (the 172 zeros of 84 .. 255):
    1, 1, 2, 3, 5, 8, 13, 21, 34, a tree 8 deep.  No two neighbouring values get the same length (no symbol 16)."""
    per_length = {2: 1, 4: 3, 8: 5, 7: 8, 5: 13, 9: 21, 10: 32}
    lens = [int(l) for l in spread(per_length)]
    return spread({v + 1: 1 << (10 - l) for v, l in enumerate(lens)})[None]


def every_symbol_plane():
    """all 256 literals and all 29 length symbols in one strip of 300-byte rows: all_run_lengths(300), then every byte value, then
    rows of two alternating values that make a code of its own worth its 286-entry header"""
    import numpy as np
    every = np.concatenate([np.arange(256, dtype=np.uint8), np.arange(44, dtype=np.uint8)])[None]
    two = np.tile(np.array([3, 9], np.uint8), 150)[None].repeat(12, 0)
    return np.concatenate([R.all_run_lengths(300), every, two])


def mixed_plane():
    """rows of 40 bytes, one strip each: rows of unequal random bytes (a code of its own does not pay: fixed) between rows of two
    alternating values (dynamic)"""
    import numpy as np
    rng = np.random.default_rng(5)
    rows = []
    for y in range(8):
        if y % 2:
            rows.append(np.tile(np.array([0, 255], np.uint8), 20))
        else:
            rows.append(rng.permutation(200)[:40].astype(np.uint8) + 1)
    return np.stack(rows)
