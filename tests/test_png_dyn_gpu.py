"""PNG stage with codes="dynamic" on the GPU: tce_png_deflate_dyn_u8 (include/tce_rvos_png.h) byte for byte against the
restatement of the stream (tests/_png_dyn.py), every stream through zlib, never longer than the fixed stream; the hard paths of the
code build (both depth limits, every length symbol, HLIT at its maximum, the three run-length symbols of the header, strips longer
than a pass and than a sub-pass of matches, planes whose strips choose differently), each with the block kind the restatement
reports asserted; planes and streams off every alignment; png.mask_pngs / png.label_pngs against their codes="fixed" files; the access
model against the bytes the launches touch (the cases of test_png_gpu.py through this entry)."""
import io
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import _png as R
import _png_dyn as D
from test_png_gpu import FOOTPRINT_CASES, check_footprint, recorded_equals_unrecorded, slab  # noqa: F401  (slab: the fixture)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 5, 1), (7, 259, 2), (9, 260, 8), (5, 262, 3), (4, 517, 4), (33, 854, 8), (6, 300, 16)]


def _deflate(planes, S, v, codes="dynamic", **kw):
    from tce_rvos_amd import ops
    t = planes if torch.is_tensor(planes) else torch.from_numpy(np.ascontiguousarray(planes)).cuda()
    streams, nbytes = ops.png_deflate(t, rows_per_strip=S, nonzero_value=v, codes=codes, **kw)
    torch.cuda.synchronize()
    P, H, W = (int(s) for s in t.shape)
    assert streams.dtype == torch.uint8 and tuple(streams.shape) == (P, R.stream_bound(H, W, S)) and streams.is_cuda
    assert nbytes.dtype == torch.int32 and tuple(nbytes.shape) == (P,)
    n, rows = nbytes.cpu().tolist(), streams.cpu().numpy()
    return [rows[p, :n[p]].tobytes() for p in range(P)], streams, nbytes


def _check(planes, S, v, **kw):
    """byte equality with the restatement, zlib, the fixed stream's length -> the block kinds of every plane's strips"""
    planes = np.ascontiguousarray(planes)
    got, _, _ = _deflate(planes, S, v, **kw)
    kinds = []
    for p, plane in enumerate(planes):
        want, infos = D.stream(plane, S, v)
        assert len(got[p]) == len(want), (p, len(got[p]), len(want), D.kinds(infos))
        assert got[p] == want, (p, next(k for k in range(len(want)) if got[p][k] != want[k]), D.kinds(infos))
        assert zlib.decompress(got[p]) == R.filtered_bytes(plane, v), p
        assert len(got[p]) <= len(R.stream(plane, S, v)), p
        kinds.append(D.kinds(infos))
    return kinds


def _planes(H, W, seed):
    rng = np.random.default_rng(seed)
    return np.stack([np.zeros((H, W), np.uint8), (rng.integers(0, 256, (H, W)) * (rng.random((H, W)) < 0.4)).astype(np.uint8),
                     R.blob(H, W, seed)])


@pytest.mark.parametrize("H,W,S", SHAPES)
def test_streams_equal_the_restatement(H, W, S):
    planes = _planes(H, W, 31 * H + W)                                              # P = 3 different planes in one call
    _check(planes, S, 0)
    _check(planes, S, 255)


def test_the_literal_code_is_limited_to_15_bits():
    plane = D.fibonacci_plane()
    _, infos = D.stream(plane, 1, 0)
    assert infos[0]["halved"] >= 1 and max(infos[0]["lens"]) <= 15
    assert _check(plane[None], 1, 0) == [["dynamic"]]


def test_the_code_length_code_is_limited_to_7_bits():
    plane = D.skewed_lengths_plane()
    _, infos = D.stream(plane, 1, 0)
    assert infos[0]["cl_halved"] >= 1 and max(infos[0]["cl_lens"]) <= 7
    assert _check(plane[None], 1, 0) == [["dynamic"]]


def test_every_length_symbol_and_every_literal():
    """all_run_lengths(300) in one strip: the 29 length symbols; every_symbol_plane: the 256 literals too, HLIT = 29; between them
    the headers use 16, 17 and 18"""
    assert _check(R.all_run_lengths(300)[None], 200, 0) == [["dynamic"]]
    assert _check(D.every_symbol_plane()[None], 1000, 0) == [["dynamic"]]
    _check(R.all_run_lengths(2047)[None], 3, 0)
    _check(R.all_run_lengths(97, lo=250, hi=270)[None], 1000, 0)


def test_strips_longer_than_a_pass_and_than_a_sub_pass_of_matches():
    assert _check(np.zeros((1, 40, 300), np.uint8), 40, 0) == [["dynamic"]]         # 12040 bytes: six passes, one run
    z = np.zeros((2, 300, 2000), np.uint8)                                          # 2326 matches of 258: three sub-passes
    z[1, 299, 1999] = 5
    assert _check(z, 300, 0) == [["dynamic"], ["dynamic"]]


def test_strips_of_one_plane_choose_differently():
    kinds = _check(D.mixed_plane()[None], 1, 0)
    assert kinds == [["fixed", "dynamic"] * 4]


def test_checkerboard_row_and_a_shorter_last_strip():
    row = (np.arange(300) & 1).astype(np.uint8)
    _check(np.stack([row[None].repeat(3, 0), (1 - row)[None].repeat(3, 0)]), 2, 255)
    _check(np.stack([row[None].repeat(3, 0)]) * 200, 3, 0)
    rng = np.random.default_rng(4)
    planes = (rng.random((2, 11, 37)) < 0.3).astype(np.uint8)
    for S in (3, 4, 10, 11, 12):
        _check(planes, S, 255)


def test_the_worst_case_of_the_fixed_stream():
    rng = np.random.default_rng(9)
    plane = rng.integers(144, 256, (5, 333), dtype=np.uint8)
    plane[:, 1:][plane[:, 1:] == plane[:, :-1]] ^= 1
    for S in (1, 2, 5):
        _check(plane[None], S, 0)


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_planes_and_streams_at_any_address_and_sentinels_untouched(offset):
    P, H, W, S = 3, 7, 11, 3
    rng = np.random.default_rng(offset)
    host = rng.integers(0, 3, (P, H, W), dtype=np.uint8)
    bound = R.stream_bound(H, W, S)
    inbuf = torch.full((P * H * W + 8,), 0xAB, dtype=torch.uint8, device="cuda")
    inbuf[offset:offset + P * H * W] = torch.from_numpy(host).cuda().reshape(-1)
    planes = inbuf[offset:offset + P * H * W].view(P, H, W)
    outbuf = torch.full((P * bound + 16,), 0xCD, dtype=torch.uint8, device="cuda")
    streams = outbuf[offset:offset + P * bound].view(P, bound)
    nbuf = torch.full((P + 2,), -7, dtype=torch.int32, device="cuda")
    assert planes.data_ptr() % 4 == offset and streams.data_ptr() % 4 == offset
    got, s2, n2 = _deflate(planes, S, 0, streams=streams, nbytes=nbuf[1:1 + P])
    assert s2.data_ptr() == streams.data_ptr() and n2.data_ptr() == nbuf[1:].data_ptr()
    out = outbuf.cpu().numpy()
    assert (out[:offset] == 0xCD).all() and (out[offset + P * bound:] == 0xCD).all()
    kinds = set()
    for p in range(P):
        want, infos = D.stream(host[p], S, 0)
        kinds |= set(D.kinds(infos))
        assert got[p] == want, p
        assert (out[offset + p * bound + len(want):offset + (p + 1) * bound] == 0xCD).all(), p     # behind nbytes[p]: not written
    assert "dynamic" in kinds
    assert nbuf.cpu().tolist()[0] == -7 and nbuf.cpu().tolist()[-1] == -7
    assert (inbuf.cpu().numpy()[:offset] == 0xAB).all() and np.array_equal(planes.cpu().numpy(), host)


def test_workspace_content_is_irrelevant_and_calls_repeat():
    from tce_rvos_amd import _lib
    planes = _planes(33, 854, 2)
    P, H, W, S = 3, 33, 854, 8
    first, _, _ = _deflate(planes, S, 255)
    assert first[2] == D.stream(planes[2], S, 255)[0]
    need = _lib.lib_raw().tce_png_ws_bytes(P, H, W, S)
    ws = torch.full((need // 8,), -1, dtype=torch.int64, device="cuda")             # every byte 0xFF
    t = torch.from_numpy(planes).cuda()
    again, _, _ = _deflate(t, S, 255, ws=ws)
    third, _, _ = _deflate(t, S, 255, ws=ws)                                         # the workspace as the call before left it
    assert first == again == third


def test_mask_pngs_and_label_pngs_decode_like_the_fixed_files_and_are_no_longer():
    from tce_rvos_amd import png
    rng = np.random.default_rng(21)
    masks = np.stack([R.blob(48, 85, k) for k in range(4)] + [np.zeros((48, 85), np.uint8)])
    t = torch.from_numpy(masks).cuda()
    fixed, dyn = png.mask_pngs(t), png.mask_pngs(t, codes="dynamic")
    same_strips = png.mask_pngs(t, codes="fixed", rows_per_strip=png.DYNAMIC_ROWS_PER_STRIP)
    for m, a, b, c in zip(masks, fixed, dyn, same_strips):
        ia, ib = Image.open(io.BytesIO(a)), Image.open(io.BytesIO(b))
        assert ia.mode == ib.mode == "L" and np.array_equal(np.asarray(ia), np.asarray(ib)) and np.array_equal(np.asarray(ib), m * 255)
        assert len(b) <= len(a) and len(b) <= len(c)
    labels = (np.stack([R.blob(48, 85, k) for k in range(3)]) * rng.integers(1, 17, (3, 48, 85))).astype(np.uint8)
    palette = rng.integers(0, 256, 768, dtype=np.uint8).tobytes()
    t = torch.from_numpy(labels).cuda()
    for S in (None, 5):
        fixed = png.label_pngs(t, palette, rows_per_strip=S)
        dyn = png.label_pngs(t, palette, rows_per_strip=S, codes="dynamic")
        for l, a, b in zip(labels, fixed, dyn):
            ia, ib = Image.open(io.BytesIO(a)), Image.open(io.BytesIO(b))
            assert ib.mode == "P" and np.array_equal(np.asarray(ib), l) and np.array_equal(np.asarray(ia), l)
            assert bytes(ib.getpalette()) == palette
            assert len(b) <= len(a)                                                    # at the defaults too: 32 rows against 8
    with pytest.raises(ValueError):
        png.mask_pngs(t, codes="huffman")


def test_the_fixed_encoding_is_what_it_was():
    from tce_rvos_amd import ops
    planes = _planes(33, 854, 7)
    explicit, _, _ = _deflate(planes, 8, 255, codes="fixed")
    t = torch.from_numpy(planes).cuda()
    streams, nbytes = ops.png_deflate(t, rows_per_strip=8, nonzero_value=255)          # the default
    torch.cuda.synchronize()
    for p in range(3):
        want = R.stream(planes[p], 8, 255)
        assert explicit[p] == want and streams[p, :int(nbytes[p])].cpu().numpy().tobytes() == want, p
    with pytest.raises(ValueError):
        ops.png_deflate(t, codes="huffman")


# --------------------------------------------------------------------------------------------- the recorder and the footprint
def test_hazard_recording_lists_the_one_entry():
    recorded_equals_unrecorded("dynamic")


@pytest.mark.parametrize("tag,kw", FOOTPRINT_CASES, ids=[c[0] for c in FOOTPRINT_CASES])
def test_png_deflate_dyn_footprint(slab, tag, kw):
    check_footprint(slab, "tce_png_deflate_dyn_u8", tag, kw, lambda plane, S, v: D.stream(plane, S, v)[0])
