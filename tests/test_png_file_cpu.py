"""CPU: the two CRC identities of include/tce_rvos_pngfile.h and the combination the launches make (tests/_png_file.py) against
zlib.crc32; the header's macros and the values of its two queries; the access model's ranges; the framing argument's errors;
the head that goes in front of the IDAT against png.frame / png.frame_rgb."""
import os
import re
import zlib

import numpy as np
import pytest

import _png_file as F

HERE = os.path.dirname(os.path.abspath(__file__))
LENGTHS = [0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 70001]


def _strings(n, rng):
    return {"random": rng.integers(0, 256, n, dtype=np.uint8).tobytes(), "zero": bytes(n), "ff": b"\xff" * n}


@pytest.mark.parametrize("n", LENGTHS)
def test_identities_equal_zlib(n):
    rng = np.random.default_rng(1000 + n)
    for kind, m in _strings(n, rng).items():
        cut = int(rng.integers(0, n + 1))
        a, b = m[:cut], m[cut:]
        ra, rb, rm = F.raw(a), F.raw(b), F.raw(m)
        assert F.combine(ra, rb, len(b)) == rm, (kind, n, cut)
        assert F.crc32_from_raw(rm, n) == zlib.crc32(m), (kind, n)
        assert F.crc32_from_raw(F.combine(ra, rb, len(b)), n) == zlib.crc32(m), (kind, n, cut)
        if kind == "zero":  # raw of zeros is 0 at every length: only the initial-value term tells the lengths apart
            assert rm == 0 and F.crc32_from_raw(rm, n, init_term=False) != zlib.crc32(m), n
    assert F.raw(bytes(7) + b"abc") == F.raw(b"abc")                 # zero bytes in front change nothing


def test_the_launches_combination_equals_zlib():
    """segment_raw / combined_crc restate what the two launches compute, with the library's own piece and segment sizes"""
    from tce_rvos_amd import ops
    P_, S_ = ops.PNG_FILE_PIECE, ops.PNG_FILE_SEGMENT
    assert S_ == 256 * P_
    rng = np.random.default_rng(5)
    big = rng.integers(0, 256, 3 * S_ + 7, dtype=np.uint8).tobytes()
    for n in [0, 1, 3, 4, P_ - 1, P_, P_ + 1, 2 * P_ + 5, S_ - 1, S_, S_ + 1, 2 * S_ - 1, 2 * S_ + 1, 3 * S_ + 7]:
        for m in (big[:n], bytes(n), b"\xff" * n):
            assert F.combined_crc(m, P_, S_) == zlib.crc32(b"IDAT" + m), n
    for n in (1, P_ + 3, S_):
        assert F.segment_raw(big[:n], P_, S_) == F.raw(big[:n]), n
    blob = F.file_bytes(b"12345678", big[:100])
    assert blob[:8] == b"12345678" and blob[8:16] == F.be32(100) + b"IDAT" and blob[16:116] == big[:100]
    assert blob[116:120] == F.be32(zlib.crc32(b"IDAT" + big[:100])) and blob[120:] == F.IEND and len(blob) == 8 + 24 + 100


def test_file_header_symbols_bound_exported_and_modelled():
    """What is the PNG-file stage's own about include/tce_rvos_pngfile.h: its macros against the ops constants, and the values of its
    two queries.  Its symbols, bindings and access models are held by tests/test_host_cpu.py, with every other header's."""
    from tce_rvos_amd import _lib, ops
    from tce_rvos_amd import build as b
    b.build(verbose=False)
    assert _lib.HEADERS["tce_rvos_pngfile.h"] is _lib.PNGFILE_SIGNATURES
    text = open(os.path.join(HERE, "..", "include", "tce_rvos_pngfile.h")).read()
    bound = _lib.lib()
    macros = {k: int(v) for k, v in re.findall(r"#define\s+(TCE_PNG_FILE_[A-Z_]+)\s+(\d+)", text)}
    assert macros == {"TCE_PNG_FILE_PIECE": ops.PNG_FILE_PIECE, "TCE_PNG_FILE_SEGMENT": ops.PNG_FILE_SEGMENT,
                      "TCE_PNG_FILE_MIN_HEAD": ops.PNG_FILE_MIN_HEAD, "TCE_PNG_FILE_MAX_HEAD": ops.PNG_FILE_MAX_HEAD}
    # the two queries launch nothing and need no GPU
    assert bound.tce_png_file_bound(33, 1000) == 33 + 24 + 1000 and bound.tce_png_file_bound(7, 1000) < 0
    assert bound.tce_png_file_bound(1025, 1000) < 0 and bound.tce_png_file_bound(33, 0) < 0 and bound.tce_png_file_bound(33, 2 ** 31) < 0
    seg = ops.PNG_FILE_SEGMENT
    assert bound.tce_png_file_ws_bytes(3, seg) == 16 and bound.tce_png_file_ws_bytes(3, seg + 1) == 24
    assert bound.tce_png_file_ws_bytes(0, seg) < 0 and bound.tce_png_file_ws_bytes(65536, seg) < 0 and bound.tce_png_file_ws_bytes(1, 0) < 0


def test_the_access_model_names_whole_rows():
    from tce_rvos_amd import hazard
    from tce_rvos_amd import build as b
    b.build(verbose=False)                                           # the model asks the library's two queries
    P, ss, hb = 3, 1001, 45
    bound = hb + 24 + ss
    a = (0x100000, 0x200000, 0x300000, hb, 0x400000, 0x500000, 0x600000, P, ss, bound, 0)
    rd, wr = hazard.MODELS["tce_png_file_u8"](a)
    rd, wr = hazard.union(*rd), hazard.union(*wr)
    assert rd.tolist() == [[0x100000, 0x100000 + P * ss], [0x200000, 0x200000 + 4 * P], [0x300000, 0x300000 + hb], [0x600000, 0x600000 + 16]]
    assert wr.tolist()[0] == [0x400000, 0x400000 + P * bound]        # rows that touch merge
    a = a[:9] + (bound + 5, 0)
    wr = hazard.union(*hazard.MODELS["tce_png_file_u8"](a)[1])
    assert wr.tolist() == [[0x400000 + p * (bound + 5), 0x400000 + p * (bound + 5) + bound] for p in range(P)] + \
        [[0x500000, 0x500000 + 4 * P], [0x600000, 0x600000 + 16]]


def test_framing_argument_errors_need_no_gpu():
    import torch
    from tce_rvos_amd import ops, png
    planes = torch.zeros(1, 4, 5, dtype=torch.uint8)
    for bad in ("gpu", None, "Device", 1):
        with pytest.raises(ValueError, match="framing"):
            png.encode(planes, "L", framing=bad)
        with pytest.raises(ValueError, match="framing"):
            png.mask_pngs(planes, framing=bad)
        with pytest.raises(ValueError, match="framing"):
            png.label_pngs(planes, [0, 0, 0], framing=bad)
        with pytest.raises(ValueError, match="framing"):
            png.rgb_pngs(torch.zeros(1, 4, 5, 3, dtype=torch.uint8), framing=bad)
    assert png.FRAMINGS == ("host", "device")
    with pytest.raises(ValueError, match="png_file"):                # on the CPU: no fall-back
        ops.png_file(torch.zeros(1, 64, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32), png.head(5, 4, "L"))


def test_heads_are_the_prefix_of_the_framed_file():
    from tce_rvos_amd import png
    stream = zlib.compress(bytes(6 * 4))
    h = png.head(5, 4, "L")
    assert len(h) == 33 and png.frame(stream, 5, 4, "L") == h + png.chunk(b"IDAT", stream) + png.chunk(b"IEND", b"") == F.file_bytes(h, stream)
    for entries, size in ((1, 48), (2, 51), (256, 813)):
        pal = bytes(range(256)) * 3
        pal = pal[:3 * entries]
        h = png.head(5, 4, "P", pal)
        assert len(h) == size and png.frame(stream, 5, 4, "P", pal) == F.file_bytes(h, stream)
        assert h[33:41] == F.be32(3 * entries) + b"PLTE" and h[41:41 + 3 * entries] == pal
    h = png.head_rgb(5, 4)
    assert len(h) == 33 and png.frame_rgb(zlib.compress(bytes(16 * 4)), 5, 4) == F.file_bytes(h, zlib.compress(bytes(16 * 4)))
    assert h[25] == 2 and png.head(5, 4, "L")[25] == 0 and png.head(5, 4, "P", [1, 2, 3])[25] == 3    # the colour type
    for bad in (lambda: png.head(5, 4, "RGB"), lambda: png.head(5, 4, "P"), lambda: png.head(5, 4, "L", [1, 2, 3]),
                lambda: png.head(0, 4, "L"), lambda: png.head_rgb(5, 0)):
        with pytest.raises(ValueError):
            bad()
