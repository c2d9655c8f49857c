"""CPU: the PNG stage's dynamic encoding without a GPU -- the restatement of the stream (tests/_png_dyn.py) against zlib, Pillow and
the fixed stream's length and bound; the codes it builds (complete, within 15 / 7 bits); inputs that take the hard paths of the
rule, each asserted to take them and to end in a dynamic block; the sizes at the two shapes of DESIGN.md section 3.16 beside
Pillow's; the entry's signature and its access model on a hand-made block; what the new entry and ops.png_deflate reject before anything is launched."""
import io
import os
import zlib
from fractions import Fraction

import numpy as np
import pytest
from PIL import Image

import _png as R
import _png_dyn as D
from test_png_cpu import SHAPES, planes_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "tce_png_deflate_dyn_u8"


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as g  # noqa: F401
    from tce_rvos_amd import build as b
    return b.build(verbose=False)


def kraft(lens):
    return sum(Fraction(1, 2 ** n) for n in lens if n)


def one_strip(plane, v=0):
    """the plane as one strip -> (stream, its info), checked against zlib"""
    s, infos = D.stream(plane, plane.shape[0], v)
    assert len(infos) == 1 and zlib.decompress(s) == R.filtered_bytes(plane, v)
    return s, infos[0]


# ------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("H,W,S", SHAPES)
def test_restatement_streams_decompress_and_are_no_longer_than_the_fixed_ones(H, W, S):
    for kind, plane in planes_of(H, W, H * 1000 + W).items():
        for v in (0, 255):
            s, infos = D.stream(plane, S, v)
            assert s[:2] == b"\x78\x01" and zlib.decompress(s) == R.filtered_bytes(plane, v), (kind, v)
            assert int.from_bytes(s[-4:], "big") == zlib.adler32(R.filtered_bytes(plane, v))
            assert len(s) <= len(R.stream(plane, S, v)) <= R.stream_bound(H, W, S), (kind, v)
            assert len(infos) == -(-H // S)
            for i in infos:
                assert (i["kind"] == "dynamic") == (i["dynamic_bits"] < i["fixed_bits"])
                assert kraft(i["lens"]) == 1 and max(i["lens"]) <= 15 and kraft(i["cl_lens"]) == 1 and max(i["cl_lens"]) <= 7


@pytest.mark.parametrize("H,W,S", SHAPES)
def test_framed_files_decode_in_pillow_to_what_the_reference_saves(H, W, S):
    from tce_rvos_amd import png
    rng = np.random.default_rng(H + W)
    palette = rng.integers(0, 256, 768, dtype=np.uint8).tobytes()
    for kind, plane in planes_of(H, W, 7 * H + W).items():
        m = (plane != 0).astype(np.uint8)
        im = Image.open(io.BytesIO(png.frame(D.stream(m, S, 255)[0], W, H, "L")))
        buf = io.BytesIO()                                                         # inference_ytvos.py:354-363, its own lines
        Image.fromarray(m.astype(np.float32) * 255).convert("L").save(buf, format="PNG")
        ref = Image.open(io.BytesIO(buf.getvalue()))
        assert ref.mode == im.mode == "L" and ref.size == im.size and np.array_equal(np.asarray(ref), np.asarray(im)), kind
        labels = (m * rng.integers(1, 17, (H, W))).astype(np.uint8)
        im = Image.open(io.BytesIO(png.frame(D.stream(labels, S, 0)[0], W, H, "P", palette=palette)))
        ref_im = Image.fromarray(labels)                                           # inference_davis.py:308-311, its own lines
        ref_im.putpalette(palette)
        buf = io.BytesIO()
        ref_im.save(buf, format="PNG")
        ref = Image.open(io.BytesIO(buf.getvalue()))
        assert im.mode == ref.mode == "P" and np.array_equal(np.asarray(ref), np.asarray(im)) and np.array_equal(np.asarray(im), labels)
        assert bytes(im.getpalette()) == palette
        assert np.array_equal(np.asarray(ref.convert("RGB")), np.asarray(im.convert("RGB")))


def test_every_code_is_complete_and_within_its_limit():
    rng = np.random.default_rng(11)
    for trial in range(300):
        for nsym, limit in ((286, 15), (19, 7)):
            used = int(rng.integers(2, nsym + 1))
            counts = np.zeros(nsym, np.int64)
            scale = [3, 50, 10 ** 6, 2 ** 30][trial % 4]
            counts[rng.permutation(nsym)[:used]] = np.maximum(1, (rng.random(used) ** 8 * scale).astype(np.int64))
            lens, _ = D.code_lengths([int(c) for c in counts], limit)
            assert kraft(lens) == 1 and max(lens) <= limit, (trial, nsym)
            assert [n > 0 for n in lens] == [c > 0 for c in counts]
            codes = D.canonical(lens)
            words = sorted(format(c, "b").zfill(n) for c, n in zip(codes, lens) if n)
            assert all(not b.startswith(a) for a, b in zip(words, words[1:])), (trial, nsym)   # prefix-free
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    for k, limit in ((19, 15), (40, 15), (9, 7), (19, 7)):
        lens, halved = D.code_lengths(fib[:k], limit)
        assert halved >= 1 and kraft(lens) == 1 and max(lens) <= limit, (k, limit)
    assert D.code_lengths([5, 0, 5], 15) == ([1, 0, 1], 0)
    assert D.code_lengths([1, 1, 2], 15)[0] == [2, 2, 1]                           # of two equal weights the leaf goes first
    assert D.code_lengths([1, 1, 2, 2], 15)[0] == [2, 2, 2, 2]


def test_the_length_sequence_rule():
    seq = [0] * 139 + [3] * 8 + [0] * 10 + [5] + [0, 0] + [4] * 4
    assert D.length_sequence_symbols(seq) == [(18, 127, 7), (0, 0, 0), (3, 0, 0), (16, 3, 2), (3, 0, 0), (17, 7, 3), (5, 0, 0),
                                              (0, 0, 0), (0, 0, 0), (4, 0, 0), (16, 0, 2)]
    assert D.length_sequence_symbols([0] * 149) == [(18, 127, 7), (18, 0, 7)]
    assert D.length_sequence_symbols([7] * 3) == [(7, 0, 0)] * 3


# -------------------------------------------------------------------------------------------------------------- the hard paths
def test_a_fibonacci_strip_halves_the_literal_counts():
    _, i = one_strip(D.fibonacci_plane())
    assert i["kind"] == "dynamic" and i["halved"] >= 1 and max(i["lens"]) <= 15 and kraft(i["lens"]) == 1
    assert D.code_lengths(i["counts"], 999)[0] != i["lens"] and max(D.code_lengths(i["counts"], 999)[0]) > 15


def test_a_skewed_strip_halves_the_code_length_counts():
    _, i = one_strip(D.skewed_lengths_plane())
    assert i["kind"] == "dynamic" and i["cl_halved"] >= 1 and max(i["cl_lens"]) <= 7 and kraft(i["cl_lens"]) == 1
    assert len([n for n in i["cl_lens"] if n]) == 9 and 16 not in i["cl_symbols"]


def test_every_length_symbol_every_literal_and_the_three_run_length_symbols():
    _, i = one_strip(R.all_run_lengths(300))
    assert i["kind"] == "dynamic" and all(i["counts"][257:286]) and i["nlit"] == 286
    assert {16, 17, 18} <= set(i["cl_symbols"])                                    # all three in one header
    _, i = one_strip(D.every_symbol_plane())
    assert i["kind"] == "dynamic" and all(i["counts"]) and i["nlit"] == 286        # HLIT = 29, nothing unused


def test_an_all_zero_strip_longer_than_a_pass_and_mixed_choices():
    s, i = one_strip(np.zeros((40, 300), np.uint8))
    assert i["kind"] == "dynamic" and 40 * 301 > 2048 and i["counts"][285] == 46 and len(s) < len(R.stream(np.zeros((40, 300), np.uint8), 40, 0))
    z = np.zeros((300, 2000), np.uint8)
    z[299, 1999] = 5
    _, i = one_strip(z)
    assert i["kind"] == "dynamic" and i["counts"][285] > 256 * 4
    plane = D.mixed_plane()
    s, infos = D.stream(plane, 1, 0)
    assert D.kinds(infos) == ["fixed", "dynamic"] * 4 and zlib.decompress(s) == R.filtered_bytes(plane, 0)
    assert len(s) < len(R.stream(plane, 1, 0))
    rng = np.random.default_rng(9)                                                 # the fixed stream's worst case: 112 values, 7 bits each
    worst = rng.integers(144, 256, (5, 333), dtype=np.uint8)
    worst[:, 1:][worst[:, 1:] == worst[:, :-1]] ^= 1
    for S in (1, 2, 5):
        s, infos = D.stream(worst, S, 0)
        assert set(D.kinds(infos)) == {"dynamic"} and len(s) < len(R.stream(worst, S, 0)) <= R.stream_bound(5, 333, S)


@pytest.mark.parametrize("H,W", [(720, 1280), (480, 854)])
def test_the_default_strip_height_makes_smaller_files_than_the_fixed_default(H, W, capsys):
    from tce_rvos_amd import png
    m = R.blob(H, W)
    fixed = R.stream(m, png.FIXED_ROWS_PER_STRIP, 255)
    assert png.FIXED_ROWS_PER_STRIP == 8 and png.DYNAMIC_ROWS_PER_STRIP in (16, 32, 64)
    dyn, infos = D.stream(m, png.DYNAMIC_ROWS_PER_STRIP, 255)
    assert zlib.decompress(dyn) == R.filtered_bytes(m, 255) and len(dyn) < len(fixed)
    buf = io.BytesIO()
    Image.fromarray(m.astype(np.float32) * 255).convert("L").save(buf, format="PNG")
    a, b, c = len(png.frame(dyn, W, H, "L")), len(png.frame(fixed, W, H, "L")), len(buf.getvalue())
    with capsys.disabled():
        print(f"\n[png dynamic] blob {H} x {W}: dynamic S={png.DYNAMIC_ROWS_PER_STRIP} {a} bytes, fixed S=8 {b} bytes, Pillow {c} bytes, "
              f"dynamic / Pillow = {a / c:.2f}")


# -------------------------------------------------------------------------------------------- the entry and its access model
# (symbols, binding table, exports, argtypes, models / launch-free names of include/tce_rvos_png.h: tests/test_host_cpu.py)
def test_the_dynamic_entry_has_the_fixed_entrys_signature_and_png_is_the_last_source(built_lib):
    from tce_rvos_amd import _lib
    from tce_rvos_amd import build as b
    assert _lib.PNG_SIGNATURES[ENTRY] == _lib.PNG_SIGNATURES["tce_png_deflate_u8"]
    fn, fixed = getattr(_lib.lib(), ENTRY), _lib.lib().tce_png_deflate_u8
    assert fn.restype is fixed.restype and list(fn.argtypes) == list(fixed.argtypes)
    assert b.SOURCES[-1] == "png.hip"


def test_access_model_on_a_hand_made_block_and_under_the_recording_proxy(built_lib):
    """P = 1, H = 3, W = 1500, S = 2: strips of 3002 and 1501 filtered bytes (at most 3383 and 1695 stream bytes), the plane and the
    stream row on odd addresses; the row is named in full, as for the fixed entry."""
    from tce_rvos_amd import _lib, hazard
    l = _lib.lib()
    assert l.tce_png_stream_bound(3, 1500, 2) == 5086 and l.tce_png_ws_bytes(1, 3, 1500, 2) == 6792
    block = (0x100003, 0x200001, 0x300000, 0x400000, 1, 3, 1500, 2, 0, 0)
    reads = [[0x100003, 0x100003 + 4500], [0x400000, 0x400000 + 6792]]
    writes = [[0x200001, 0x200001 + 5086], [0x300000, 0x300004], [0x400000, 0x400000 + 6792]]
    rd, wr = hazard.MODELS[ENTRY](block)
    assert hazard.union(*rd).tolist() == reads and hazard.union(*wr).tolist() == writes

    class StandIn:
        def __getattr__(self, name):
            return lambda *a: name
    rec = hazard.Recorder()
    proxy = hazard._LibProxy(StandIn(), rec, dry=True)
    assert getattr(proxy, ENTRY)(*block) == 0
    assert [x.name for x in rec.launches] == [ENTRY]
    assert rec.launches[0].reads.tolist() == reads and rec.launches[0].writes.tolist() == writes
    assert proxy.tce_png_ws_bytes(1, 3, 1500, 2) == "tce_png_ws_bytes" and len(rec.launches) == 1  # a query: passed through


def test_bad_calls_are_rejected_before_anything_is_launched(built_lib):
    from tce_rvos_amd import _lib
    l = _lib.lib()
    f = getattr(l, ENTRY)
    assert f(None, None, None, None, 1, 4, 6, 8, 0, None) != 0 and (ENTRY + ": null").encode() in l.tce_last_error()
    for P, H, W, S, v in ((0, 4, 6, 8, 0), (65536, 4, 6, 8, 0), (1, 0, 6, 8, 0), (1, 4, 0, 8, 0), (1, 4, 6, 0, 0), (1, 4, 6, 8, 256),
                          (1, 4, 6, 8, -1), (1, 1 << 16, 1 << 15, 8, 0)):
        assert f(None, None, None, None, P, H, W, S, v, None) != 0, (P, H, W, S, v)
        assert ENTRY.encode() in l.tce_last_error() and b"null" not in l.tce_last_error(), (P, H, W, S, v)
        assert f(8, 8, 8, 8, P, H, W, S, v, None) != 0, (P, H, W, S, v)
    assert f(8, 8, 8, 12, 1, 4, 6, 8, 0, None) != 0 and b"aligned" in l.tce_last_error() and ENTRY.encode() in l.tce_last_error()
    assert f(8, 8, 6, 8, 1, 4, 6, 8, 0, None) != 0 and b"aligned" in l.tce_last_error()


def test_ops_and_png_reject_unknown_codes():
    import torch
    from tce_rvos_amd import ops, png
    t = torch.zeros(2, 3, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="codes"):
        ops.png_deflate(t, codes="huffman")
    with pytest.raises(ValueError, match="png_deflate"):
        ops.png_deflate(t, codes="dynamic")                                        # on the CPU: no fall-back
    for bad in (lambda: png.encode(t, "L", codes="huffman"), lambda: png.mask_pngs(t, codes=None),
                lambda: png.label_pngs(t, bytes(6), codes="Dynamic")):
        with pytest.raises(ValueError, match="codes"):
            bad()
