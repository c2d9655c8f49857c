"""PNG stage on the GPU: tce_png_deflate_u8 (include/tce_rvos_png.h) byte for byte against the restatement of the stream
(tests/_png.py), every stream through zlib and every framed file through Pillow back to the value-mapped input; png.mask_pngs and
png.label_pngs on synthetic device tensors; the access model against the bytes the launches touch (tests/_footprint.py).  Small shapes: each puts the kernel on another path (the branches of the run rule
through all-zero strips of S * (W + 1) bytes, runs across passes of 2048 bytes, more boundaries than threads, a shorter last
strip, planes and streams off every alignment)."""
import io
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import _footprint as fp
import _png as R
from tce_rvos_amd import _lib, hazard

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 5, 1), (7, 259, 2), (9, 260, 8), (5, 262, 3), (4, 517, 4), (33, 854, 8), (6, 300, 16)]


def _deflate(planes, S, v, **kw):
    """ops.png_deflate of host planes [P,H,W] -> (list of the P streams' used bytes, the streams tensor, the nbytes tensor)"""
    from tce_rvos_amd import ops
    t = planes if torch.is_tensor(planes) else torch.from_numpy(np.ascontiguousarray(planes)).cuda()
    streams, nbytes = ops.png_deflate(t, rows_per_strip=S, nonzero_value=v, **kw)
    torch.cuda.synchronize()
    P, H, W = (int(s) for s in t.shape)
    assert streams.dtype == torch.uint8 and tuple(streams.shape) == (P, R.stream_bound(H, W, S)) and streams.is_cuda
    assert nbytes.dtype == torch.int32 and tuple(nbytes.shape) == (P,)
    n, rows = nbytes.cpu().tolist(), streams.cpu().numpy()
    return [rows[p, :n[p]].tobytes() for p in range(P)], streams, nbytes


def _check(planes, S, v, mode="L", palette=None, **kw):
    """the three things every case checks"""
    from tce_rvos_amd import png
    planes = np.ascontiguousarray(planes)
    got, _, _ = _deflate(planes, S, v, **kw)
    H, W = planes.shape[1:]
    for p, plane in enumerate(planes):
        want = R.stream(plane, S, v)
        assert len(got[p]) == len(want), (p, len(got[p]), len(want))
        assert got[p] == want, (p, next(k for k in range(len(want)) if got[p][k] != want[k]))
        assert zlib.decompress(got[p]) == R.filtered_bytes(plane, v), p
        im = Image.open(io.BytesIO(png.frame(got[p], W, H, mode, palette)))
        im.load()
        assert im.mode == mode and im.size == (W, H) and np.array_equal(np.asarray(im), R.value_map(plane, v)), p
    return got


def _planes(H, W, seed):
    rng = np.random.default_rng(seed)
    return np.stack([np.zeros((H, W), np.uint8), (rng.integers(0, 256, (H, W)) * (rng.random((H, W)) < 0.4)).astype(np.uint8),
                     R.blob(H, W, seed)])


@pytest.mark.parametrize("H,W,S", SHAPES)
def test_streams_equal_the_restatement(H, W, S):
    """empty, random and blob planes: the all-zero strips are runs of S * (W + 1) = 2, 6, 520, 2088, 789, 2072, 6840 and 1806 bytes,
    which between them take every branch of the run rule, inside one pass of 2048 bytes and across two and four"""
    planes = _planes(H, W, 31 * H + W)
    _check(planes, S, 0)
    _check(planes, S, 255)


def test_every_run_length_inside_a_pass_and_across_passes():
    """runs of every length 1 .. 264, one after the other: every length symbol, every extra-bit count, 258, 259 and 260 and the two
    literals behind a run of 1 or 2; at W = 2047 rows of 2048 filtered bytes put them at other places of a pass"""
    _check(R.all_run_lengths(300)[None], 200, 0)
    _check(R.all_run_lengths(2047)[None], 3, 0)
    _check(R.all_run_lengths(97, lo=250, hi=270)[None], 1000, 0)


def test_checkerboard_row_has_more_runs_than_a_wavefront_pass():
    row = (np.arange(300) & 1).astype(np.uint8)
    _check(np.stack([row[None].repeat(3, 0), (1 - row)[None].repeat(3, 0)]), 2, 255)      # S = 2 of H = 3: a shorter last strip too
    _check(np.stack([row[None].repeat(3, 0)]) * 200, 3, 0)                                # nine-bit literals


def test_last_strip_is_shorter():
    rng = np.random.default_rng(4)
    planes = (rng.random((2, 11, 37)) < 0.3).astype(np.uint8)
    for S in (3, 4, 10, 11, 12):
        _check(planes, S, 255)


def test_worst_case_stays_inside_the_bound():
    rng = np.random.default_rng(9)
    plane = rng.integers(144, 256, (5, 333), dtype=np.uint8)
    plane[:, 1:][plane[:, 1:] == plane[:, :-1]] ^= 1
    for S in (1, 2, 5):
        got = _check(plane[None], S, 0)
        assert R.stream_bound(5, 333, S) - 8 <= len(got[0]) <= R.stream_bound(5, 333, S)


def test_a_long_run_goes_out_in_sub_passes():
    """an all-zero strip of 300 * 2001 bytes: 2326 matches of length 258 = three sub-passes of the long-run path, then a tail; and
    the same with one pixel set at the very end"""
    z = np.zeros((2, 300, 2000), np.uint8)
    z[1, 299, 1999] = 5
    _check(z, 300, 0)


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_planes_and_streams_at_any_address_and_sentinels_untouched(offset):
    from tce_rvos_amd import ops
    P, H, W, S = 3, 7, 11, 3                                                       # H*W = 77: every plane starts on another alignment
    rng = np.random.default_rng(offset)
    host = rng.integers(0, 17, (P, H, W), dtype=np.uint8)
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
    for p in range(P):
        want = R.stream(host[p], S, 0)
        assert got[p] == want, p
        assert zlib.decompress(got[p]) == R.filtered_bytes(host[p], 0)
        assert (out[offset + p * bound + len(want):offset + (p + 1) * bound] == 0xCD).all(), p     # behind nbytes[p]: not written
    assert nbuf.cpu().tolist()[0] == -7 and nbuf.cpu().tolist()[-1] == -7
    assert (inbuf.cpu().numpy()[:offset] == 0xAB).all() and np.array_equal(planes.cpu().numpy(), host)


def test_value_map_on_masks_and_labels():
    rng = np.random.default_rng(12)
    masks = (rng.random((2, 13, 29)) < 0.5).astype(np.uint8)
    got = _check(masks, 4, 255)
    assert zlib.decompress(got[0]) == R.filtered_bytes(masks[0] * 255, 0)
    labels = rng.integers(0, 17, (2, 13, 29), dtype=np.uint8)
    _check(labels, 4, 0, mode="P", palette=bytes(range(256)) * 3)
    _check(labels, 4, 7)                                                            # any value 1 .. 255


def test_workspace_content_is_irrelevant_and_calls_repeat():
    from tce_rvos_amd import _lib
    planes = _planes(33, 854, 2)
    P, H, W, S = 3, 33, 854, 8
    first = _check(planes, S, 255)
    need = _lib.lib_raw().tce_png_ws_bytes(P, H, W, S)
    ws = torch.full((need // 8,), -1, dtype=torch.int64, device="cuda")             # every byte 0xFF
    t = torch.from_numpy(planes).cuda()
    again, _, _ = _deflate(t, S, 255, ws=ws)
    third, _, _ = _deflate(t, S, 255, ws=ws)                                         # the workspace as the call before left it
    assert first == again == third


# --------------------------------------------------------------------------------------------- the recorder and the footprint
def recorded_equals_unrecorded(codes):
    """ops.png_deflate under hazard.recording(): its one entry, no conflict, the bytes of the unrecorded call"""
    from tce_rvos_amd import ops
    t = torch.from_numpy(_planes(9, 260, 5)).cuda()
    want_s, want_n = ops.png_deflate(t, rows_per_strip=4, nonzero_value=255, codes=codes)
    with hazard.recording() as rec:
        got_s, got_n = ops.png_deflate(t, rows_per_strip=4, nonzero_value=255, codes=codes)
    torch.cuda.synchronize()
    assert [x.name for x in rec.launches] == ["tce_png_deflate_u8" if codes == "fixed" else "tce_png_deflate_dyn_u8"]
    assert rec.analyse().clean and torch.equal(got_n, want_n)
    for p, n in enumerate(want_n.tolist()):
        assert n > 0 and torch.equal(got_s[p, :n], want_s[p, :n]), p


def test_hazard_recording_lists_the_one_entry():
    recorded_equals_unrecorded("fixed")


@pytest.fixture(scope="module")
def slab():
    s = fp.Slab(64 << 20, device="cuda")
    yield s
    del s
    torch.cuda.empty_cache()


TAIL = 0xEE  # what the cases write behind nbytes[p]


def footprint_planes(tag):
    if tag.startswith("masks"):
        return (np.random.default_rng(61).random((2, 5, 7)) < 0.5).astype(np.uint8)
    return ((np.arange(1500)[None] // 37 + np.arange(3)[:, None]) % 4).astype(np.uint8)[None]  # labels 0 .. 3 in runs of 37


# both entries take these (test_png_dyn_gpu.py runs them through the dynamic one)
FOOTPRINT_CASES = [
    # three strips a plane, the last one of a single row; 0/1 masks written as 0/255
    ("masks_2x5x7_strips_of_2_rows_value_255_addresses_1_and_3", dict(S=2, v=255, shift_p=1, shift_s=3)),
    # a strip of 3002 filtered bytes: more than one pass of 2048
    ("labels_1x3x1500_strips_of_2_rows_value_0_addresses_3_and_1", dict(S=2, v=0, shift_p=3, shift_s=1)),
]


def footprint_case(slab_, entry, planes, S, v, shift_p, shift_s):
    """Every buffer of the call in the slab, planes and streams `shift` bytes into their buffers.  By contract the bytes of a row of
    streams behind nbytes[p] are not written, while the model names whole rows (how much is written is device data): the case
    follows the launch with a fill of each row's tail, made on the device from nbytes on the same stream, so bytes [0, nbytes[p])
    are held to the canary and compared under R as they are, and no row needs an exemption."""
    P, H, W = planes.shape
    total, bound = P * H * W, R.stream_bound(H, W, S)
    host = np.zeros(shift_p + total + 3, np.uint8)
    host[shift_p:shift_p + total] = planes.reshape(-1)
    raw_p = slab_.put("planes", host)
    raw_s = slab_.alloc("streams", (shift_s + P * bound + 3,), dtype=torch.uint8)
    nbytes = slab_.alloc("nbytes", (P,), dtype=torch.int32)
    ws = slab_.alloc("ws", (_lib.lib_raw().tce_png_ws_bytes(P, H, W, S) // 8,), dtype=torch.int64)
    rows = raw_s[shift_s:shift_s + P * bound].view(P, bound)
    col = torch.arange(bound, dtype=torch.int32, device=slab_.device)[None]
    src, dst = raw_p.data_ptr() + shift_p, raw_s.data_ptr() + shift_s

    def fn():
        _lib.check(getattr(_lib.lib(), entry)(src, dst, nbytes.data_ptr(), ws.data_ptr(), P, H, W, S, v,
                                              torch.cuda.current_stream().cuda_stream), entry)
        rows.masked_fill_(col >= nbytes[:, None], TAIL)
    fn.check = lambda: (rows, nbytes)
    return fn


def check_footprint(slab_, entry, tag, kw, restatement):
    """W, O and R of tests/_footprint.py: nothing outside streams, nbytes and ws is written, every byte of a stream and every word
    of nbytes is written, and the result depends on no byte outside the planes -- the bytes around them included -- nor on what ws
    held (scratch: R fills it before the run).  ws is exempt from O: a strip's slot is written as far as its bits go."""
    planes = footprint_planes(tag)
    P, H, W = planes.shape
    build = lambda s: footprint_case(s, entry, planes, **kw)  # noqa: E731
    info = fp.check_case(slab_, build, fp.recorder(entry), exempt=("ws",), scratch=("ws",), props="WOR", sync=torch.cuda.synchronize,
                         label=f"{entry} {tag}")
    print(f"{entry} {tag}: read {info['read_bytes']} written {info['written_bytes']} guard {info['guard_bytes']} "
          f"untouched-in-buffers {info['pad_bytes']}")
    assert (info["W"], info["O"], info["R"]) == (2, 2, 3) and info["exempt"] == ["ws"]
    wsb = _lib.lib_raw().tce_png_ws_bytes(P, H, W, kw["S"])
    assert info["read_bytes"] == P * H * W + wsb and info["written_bytes"] == P * R.stream_bound(H, W, kw["S"]) + 4 * P + wsb
    slab_.begin(0)
    fn = build(slab_)
    fn()
    torch.cuda.synchronize()
    rows, nbytes = fn.check()
    rows, n = rows.cpu().numpy(), nbytes.cpu().tolist()
    for p in range(P):
        want = restatement(planes[p], kw["S"], kw["v"])
        assert rows[p, :n[p]].tobytes() == want and (rows[p, n[p]:] == TAIL).all(), p


@pytest.mark.parametrize("tag,kw", FOOTPRINT_CASES, ids=[c[0] for c in FOOTPRINT_CASES])
def test_png_deflate_footprint(slab, tag, kw):
    check_footprint(slab, "tce_png_deflate_u8", tag, kw, R.stream)


def test_mask_pngs_and_label_pngs_on_device_tensors(tmp_path):
    from tce_rvos_amd import png
    rng = np.random.default_rng(21)
    masks = np.stack([R.blob(48, 85, k) for k in range(4)] + [np.zeros((48, 85), np.uint8)])    # run_video(...)["masks"]: 0/1
    blobs = png.mask_pngs(torch.from_numpy(masks).cuda())
    assert len(blobs) == 5 and all(isinstance(b, bytes) for b in blobs)
    for m, blob in zip(masks, blobs):
        im = Image.open(io.BytesIO(blob))
        buf = io.BytesIO()
        Image.fromarray(m.astype(np.float32) * 255).convert("L").save(buf, format="PNG")        # inference_ytvos.py:354-363
        ref = Image.open(io.BytesIO(buf.getvalue()))
        assert im.mode == ref.mode == "L" and im.size == ref.size and np.array_equal(np.asarray(im), np.asarray(ref))
    labels = (np.stack([R.blob(48, 85, k) for k in range(3)]) * rng.integers(1, 17, (3, 48, 85))).astype(np.uint8)
    palette = rng.integers(0, 256, 768, dtype=np.uint8).tobytes()
    blobs = png.label_pngs(torch.from_numpy(labels).cuda(), palette, rows_per_strip=5)
    paths = [str(tmp_path / f"{k:05d}.png") for k in range(3)]
    png.write_files(paths, blobs)
    for l, path in zip(labels, paths):
        im = Image.open(path)
        ref = Image.fromarray(l)                                                                  # inference_davis.py:308-311
        ref.putpalette(palette)
        assert im.mode == "P" and np.array_equal(np.asarray(im), l) and bytes(im.getpalette()) == palette
        assert np.array_equal(np.asarray(im.convert("RGB")), np.asarray(ref.convert("RGB")))


def test_ops_rejects_bad_arguments():
    from tce_rvos_amd import ops
    t = torch.zeros(2, 5, 6, dtype=torch.uint8, device="cuda")
    for bad in (lambda: ops.png_deflate(t, rows_per_strip=0), lambda: ops.png_deflate(t, nonzero_value=256),
                lambda: ops.png_deflate(t.float()), lambda: ops.png_deflate(t[:, :, :3]),
                lambda: ops.png_deflate(t, streams=torch.zeros(2, 5, dtype=torch.uint8, device="cuda"))):
        with pytest.raises(ValueError):
            bad()
