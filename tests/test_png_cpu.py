"""CPU: the PNG stage without a GPU -- the restatement of the stream (tests/_png.py) against zlib and Pillow, the host framing of
tce_rvos_amd/png.py against Pillow and against the reference's own save lines (inference_ytvos.py:354-363,
inference_davis.py:308-311, run through Pillow on the same arrays), the access model on a hand-made block, the two queries against
the bound's formula, and the extents the entries reject before anything is launched."""
import io
import os
import re
import zlib

import numpy as np
import pytest
from PIL import Image

import _png as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHING = ("tce_png_deflate_u8",)
QUERIES = ("tce_png_stream_bound", "tce_png_ws_bytes")
SHAPES = [(1, 1, 1), (3, 5, 1), (7, 259, 2), (9, 260, 8), (5, 262, 3), (4, 517, 4), (33, 854, 8), (6, 300, 16)]


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as g  # noqa: F401
    from tce_rvos_amd import build as b
    return b.build(verbose=False)


def planes_of(H, W, seed):
    rng = np.random.default_rng(seed)
    return {"empty": np.zeros((H, W), np.uint8),
            "random": (rng.integers(0, 256, (H, W)) * (rng.random((H, W)) < 0.4)).astype(np.uint8),
            "blob": R.blob(H, W, seed)}


# ------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("H,W,S", SHAPES)
def test_restatement_streams_decompress_to_the_filtered_bytes(H, W, S):
    for kind, plane in planes_of(H, W, H * 1000 + W).items():
        for v in (0, 255):
            s = R.stream(plane, S, v)
            assert s[:2] == b"\x78\x01" and zlib.decompress(s) == R.filtered_bytes(plane, v), (kind, v)
            assert len(s) <= R.stream_bound(H, W, S), (kind, v)
            assert int.from_bytes(s[-4:], "big") == zlib.adler32(R.filtered_bytes(plane, v))


def test_every_run_length_and_the_adler_combine_rule():
    plane = R.all_run_lengths(300)
    assert zlib.decompress(R.stream(plane, 200, 0)) == R.filtered_bytes(plane, 0)
    for L in list(range(1, 300)) + [515, 516, 517, 518, 519, 520, 775, 1000]:     # each branch of the run rule, alone
        out = R.Bits()
        out.extra(1, 1)
        out.extra(1, 2)
        R.run_tokens(out, 200, L)
        out.symbol(256)
        out.pad()
        assert zlib.decompress(out.tobytes(), wbits=-15) == bytes([200]) * L, L
    rng = np.random.default_rng(3)
    for _ in range(200):
        data = rng.integers(0, 256, int(rng.integers(2, 4000)), dtype=np.uint8).tobytes()
        k = int(rng.integers(0, len(data) + 1))
        a, b = R.adler_combine(R.adler32(data[:k]), R.adler32(data[k:]), len(data) - k)
        assert (b << 16) | a == zlib.adler32(data)


def test_the_bound_is_reached_only_by_unequal_bytes_of_nine_bits():
    rng = np.random.default_rng(9)
    for H, W, S in [(3, 5, 1), (5, 333, 2), (4, 40, 8)]:
        plane = rng.integers(144, 256, (H, W), dtype=np.uint8)
        plane[:, 1:][plane[:, 1:] == plane[:, :-1]] ^= 1                          # no two equal neighbours (144 .. 255 is closed under ^ 1)
        assert (plane[:, 1:] != plane[:, :-1]).all() and plane.min() >= 144
        n = len(R.stream(plane, S, 0))
        # every byte is a literal; a filter byte costs 8 bits, not 9: one bit of slack per row is all there is
        want = 2 + sum((9 * r * (W + 1) - r + 13 + 7) // 8 + 4 for r in [min(S, H - y) for y in range(0, H, S)]) + 6
        assert n == want <= R.stream_bound(H, W, S) <= want + -(-H // 8) + -(-H // S), (H, W, S, n)


# ----------------------------------------------------------------------------------------------------------------- the framing
@pytest.mark.parametrize("H,W,S", SHAPES)
def test_framed_masks_decode_in_pillow_to_what_the_reference_saves(H, W, S):
    from tce_rvos_amd import png
    for kind, plane in planes_of(H, W, 7 * H + W).items():
        m = (plane != 0).astype(np.uint8)                                          # run_video(...)["masks"]: 0/1
        blob = png.frame(R.stream(m, S, 255), W, H, "L")
        im = Image.open(io.BytesIO(blob))
        im.load()
        assert im.mode == "L" and im.size == (W, H), kind
        assert np.array_equal(np.asarray(im), m * 255), kind
        buf = io.BytesIO()                                                         # inference_ytvos.py:354-363, its own lines
        Image.fromarray(m.astype(np.float32) * 255).convert("L").save(buf, format="PNG")
        ref = Image.open(io.BytesIO(buf.getvalue()))
        assert ref.mode == im.mode and ref.size == im.size and np.array_equal(np.asarray(ref), np.asarray(im)), kind


@pytest.mark.parametrize("H,W,S", SHAPES)
def test_framed_label_maps_decode_in_pillow_with_the_palette_as_given(H, W, S):
    from tce_rvos_amd import png
    rng = np.random.default_rng(H + W)
    palette = rng.integers(0, 256, 768, dtype=np.uint8).tobytes()
    labels = (planes_of(H, W, 5)["blob"] * rng.integers(1, 17, (H, W))).astype(np.uint8)
    for pal in (palette, palette[:17 * 3], list(palette)):
        blob = png.frame(R.stream(labels, S, 0), W, H, "P", palette=pal)
        im = Image.open(io.BytesIO(blob))
        im.load()
        assert im.mode == "P" and im.size == (W, H)
        assert np.array_equal(np.asarray(im), labels)
        assert bytes(im.getpalette())[:len(bytes(pal))] == bytes(pal)
        ref_im = Image.fromarray(labels)                                           # inference_davis.py:308-311, its own lines
        ref_im.putpalette(bytes(pal))
        buf = io.BytesIO()
        ref_im.save(buf, format="PNG")
        ref = Image.open(io.BytesIO(buf.getvalue()))
        assert ref.mode == "P" and ref.size == im.size and np.array_equal(np.asarray(ref), np.asarray(im))
        assert np.array_equal(np.asarray(ref.convert("RGB")), np.asarray(im.convert("RGB")))


def test_frame_layout_and_errors(tmp_path):
    from tce_rvos_amd import png
    s = R.stream(np.zeros((2, 3), np.uint8), 8, 0)
    blob = png.frame(s, 3, 2, "L")
    assert blob[:8] == b"\x89PNG\r\n\x1a\n" and blob[12:16] == b"IHDR" and blob[16:29] == bytes([0, 0, 0, 3, 0, 0, 0, 2, 8, 0, 0, 0, 0])
    kinds = re.findall(rb"IHDR|PLTE|IDAT|IEND", png.frame(s, 3, 2, "P", palette=bytes(6)))
    assert kinds == [b"IHDR", b"PLTE", b"IDAT", b"IEND"] and blob.count(b"IDAT") == 1
    assert blob[-12:] == png.chunk(b"IEND", b"") == bytes.fromhex("0000000049454e44ae426082")
    for bad in (lambda: png.frame(s, 3, 2, "RGB"), lambda: png.frame(s, 3, 2, "P"), lambda: png.frame(s, 3, 2, "L", palette=bytes(3)),
                lambda: png.frame(s, 0, 2, "L"), lambda: png.frame(s, 3, 2, "P", palette=bytes(4)),
                lambda: png.frame(s, 3, 2, "P", palette=bytes(771)), lambda: png.write_files(["a"], [])):
        with pytest.raises(ValueError):
            bad()
    paths = [str(tmp_path / f"{k:05d}.png") for k in range(2)]
    png.write_files(paths, [blob, blob])
    assert open(paths[1], "rb").read() == blob


# -------------------------------------------------------------------------------------------- the header and the access model
# (symbols, binding table, exports, argtypes, models / launch-free names of include/tce_rvos_png.h: tests/test_host_cpu.py)
def test_the_header_says_which_entries_launch_nothing_and_png_is_the_last_source():
    from tce_rvos_amd import build as b
    text = open(os.path.join(ROOT, "include", "tce_rvos_png.h")).read()
    for q in QUERIES:
        assert re.search(rf"{q}\([^;]*;\s*/\*[^*]*launches nothing", text), q
    assert b.SOURCES[-1] == "png.hip"


# P = 2, H = 5, W = 7, S = 2: three strips a plane (16, 16 and 8 filtered bytes: at most 24, 24 and 15 stream bytes), planes and
# streams on odd addresses; every row of streams is named in full
BLOCK = (0x100001, 0x200003, 0x300000, 0x400000, 2, 5, 7, 2, 255, 0)
BLOCK_READS = [[0x100001, 0x100047], [0x400000, 0x4000D8]]
BLOCK_WRITES = [[0x200003, 0x200091], [0x300000, 0x300008], [0x400000, 0x4000D8]]


def test_access_model_on_a_hand_made_block(built_lib):
    from tce_rvos_amd import _lib, hazard
    l = _lib.lib()
    assert l.tce_png_stream_bound(5, 7, 2) == 71 and l.tce_png_ws_bytes(2, 5, 7, 2) == 216
    rd, wr = hazard.MODELS["tce_png_deflate_u8"](BLOCK)
    assert hazard.union(*rd).tolist() == BLOCK_READS and hazard.union(*wr).tolist() == BLOCK_WRITES


class _StandIn:
    """Stands where the CDLL stands under a dry hazard._LibProxy: every entry answers with its own name."""

    def __getattr__(self, name):
        return lambda *a: name


def test_recording_proxy_records_the_launching_entry_and_passes_the_queries_through(built_lib):
    from tce_rvos_amd import hazard
    rec = hazard.Recorder()
    proxy = hazard._LibProxy(_StandIn(), rec, dry=True)
    assert proxy.tce_png_deflate_u8(*BLOCK) == 0
    assert [x.name for x in rec.launches] == list(LAUNCHING)
    assert rec.launches[0].reads.tolist() == BLOCK_READS and rec.launches[0].writes.tolist() == BLOCK_WRITES
    for q in QUERIES:  # passed through, not recorded
        assert getattr(proxy, q)(5, 7, 2) == q
    assert len(rec.launches) == 1


# ----------------------------------------------------------------------------------------------------------------- the queries
def test_stream_bound_equals_the_formula_and_holds_the_restatement(built_lib):
    from tce_rvos_amd import _lib
    l = _lib.lib()
    for H, W, S in SHAPES + [(720, 1280, 8), (720, 1280, 1), (480, 854, 32), (5, 7, 100), (10, 3, 3), (11, 3, 3)]:
        assert l.tce_png_stream_bound(H, W, S) == R.stream_bound(H, W, S), (H, W, S)
        for P in (1, 3):
            ws = l.tce_png_ws_bytes(P, H, W, S)
            assert ws > 0 and ws % 8 == 0 and ws >= P * (R.stream_bound(H, W, S) - 8), (P, H, W, S)
    assert R.stream_bound(720, 1280, 8) == 2 + 90 * ((9 * 8 * 1281 + 13 + 7) // 8 + 4) + 6
    rng = np.random.default_rng(1)
    worst = rng.integers(144, 256, (5, 333), dtype=np.uint8)
    worst[:, 1:][worst[:, 1:] == worst[:, :-1]] ^= 1
    for S in (1, 2, 5, 9):
        assert len(R.stream(worst, S, 0)) <= l.tce_png_stream_bound(5, 333, S)


def test_extents_are_rejected_before_anything_is_launched(built_lib):
    from tce_rvos_amd import _lib
    l = _lib.lib()
    for H, W, S in ((0, 6, 1), (4, 0, 1), (4, 6, 0), (-1, 6, 1), (4, 6, -3), (1 << 16, 1 << 15, 8), (32768, 65536, 8)):
        assert l.tce_png_stream_bound(H, W, S) < 0, (H, W, S)
        assert l.tce_png_ws_bytes(1, H, W, S) < 0, (H, W, S)
    for P in (0, -1, 65536):
        assert l.tce_png_ws_bytes(P, 4, 6, 1) < 0, P
    assert l.tce_png_ws_bytes(65535, 4, 6, 1) > 0 and l.tce_png_stream_bound(1 << 15, (1 << 15) - 1, 1 << 30) > 0
    # null pointers, with good and with bad extents: rejected on the host with the entry's name (nothing is launched)
    assert l.tce_png_deflate_u8(None, None, None, None, 1, 4, 6, 8, 0, None) != 0 and b"tce_png_deflate_u8: null" in l.tce_last_error()
    for P, H, W, S, v in ((0, 4, 6, 8, 0), (65536, 4, 6, 8, 0), (1, 0, 6, 8, 0), (1, 4, 0, 8, 0), (1, 4, 6, 0, 0), (1, 4, 6, 8, 256),
                          (1, 4, 6, 8, -1), (1, 1 << 16, 1 << 15, 8, 0)):
        assert l.tce_png_deflate_u8(None, None, None, None, P, H, W, S, v, None) != 0, (P, H, W, S, v)
        assert b"tce_png_deflate_u8" in l.tce_last_error() and b"null" not in l.tce_last_error(), (P, H, W, S, v)
        assert l.tce_png_deflate_u8(8, 8, 8, 8, P, H, W, S, v, None) != 0, (P, H, W, S, v)
    assert l.tce_png_deflate_u8(8, 8, 8, 12, 1, 4, 6, 8, 0, None) != 0 and b"aligned" in l.tce_last_error()    # ws off its 8-byte boundary
    assert l.tce_png_deflate_u8(8, 8, 6, 8, 1, 4, 6, 8, 0, None) != 0 and b"aligned" in l.tce_last_error()     # nbytes off its 4-byte boundary


def test_ops_png_deflate_rejects_what_is_not_a_gpu_plane_stack():
    import torch
    from tce_rvos_amd import ops, png
    with pytest.raises(ValueError, match="png_deflate"):
        ops.png_deflate(torch.zeros(2, 3, 4, dtype=torch.uint8))                  # on the CPU: no fall-back
    with pytest.raises(ValueError, match="png_deflate"):
        ops.png_deflate(torch.zeros(3, 4, dtype=torch.uint8))
    with pytest.raises(ValueError):
        png.encode(torch.zeros(2, 3, 4, dtype=torch.uint8), "P")                  # no palette
