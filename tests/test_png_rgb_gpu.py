"""RGB half of the PNG stage on the GPU: tce_png_filter_rgb_u8 and tce_png_deflate_rows_u8 (include/tce_rvos_vis.h) byte for byte
against their restatement (tests/_png_rgb.py, the blocks of tests/_png_dyn.py); the all-literal case inside the stream bound, no
stream above its fixed-code cost; every file decoded by zlib and un-filtering; images encoded together equal images encoded
alone; images and rows off every alignment; rejected arguments; the access models against the bytes the launches touch."""
import io
import zlib

import numpy as np
import pytest
import torch

import _footprint as fp
import _png as R
import _png_rgb as G
from tce_rvos_amd import _lib, hazard

pytestmark = pytest.mark.gpu

# H, W, rows_per_strip: 33 x 21 has rows of 64 bytes (whole dwords), 37 x 53 of 160; H one more and one less than a multiple of the
# strip; strips of 1 and of 32 rows
SHAPES = [(1, 1, 32), (1, 7, 1), (5, 1, 32), (33, 21, 32), (33, 21, 1), (37, 53, 32), (37, 53, 4), (35, 53, 4), (9, 12, 8), (7, 12, 8)]


@pytest.fixture(scope="module")
def reference():
    """per shape (H, W): the images, their filtered rows; per (H, W, S) the streams -- computed once, never changed"""
    imgs, rows, streams = {}, {}, {}
    for H, W, S in SHAPES:
        if (H, W) not in imgs:
            imgs[(H, W)] = G.images(H, W, 17 * H + W)
            rows[(H, W)] = np.stack([G.filtered_rows(im) for im in imgs[(H, W)]])
        streams[(H, W, S)] = [G.rows_stream(r, S) for r in rows[(H, W)]]
    return imgs, rows, streams


def _filter(images):
    from tce_rvos_amd import ops
    t = images if torch.is_tensor(images) else torch.from_numpy(np.ascontiguousarray(images)).cuda()
    rows = ops.png_filter_rgb(t)
    torch.cuda.synchronize()
    P, H, W, _ = t.shape
    assert rows.dtype == torch.uint8 and tuple(rows.shape) == (P, H, 1 + 3 * W) and rows.is_cuda
    return rows


def _deflate(rows, S, **kw):
    from tce_rvos_amd import ops
    t = rows if torch.is_tensor(rows) else torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    streams, nbytes = ops.png_deflate_rows(t, rows_per_strip=S, **kw)
    torch.cuda.synchronize()
    P, H, Rw = (int(s) for s in t.shape)
    assert tuple(streams.shape) == (P, R.stream_bound(H, Rw - 1, S)) and nbytes.dtype == torch.int32 and tuple(nbytes.shape) == (P,)
    n, flat = nbytes.cpu().tolist(), streams.cpu().numpy()
    return [flat[p, :n[p]].tobytes() for p in range(P)]


@pytest.mark.parametrize("H,W,S", SHAPES)
def test_rows_and_streams_equal_the_restatement(reference, H, W, S):
    imgs, rows, streams = reference
    got_rows = _filter(imgs[(H, W)])
    host = got_rows.cpu().numpy()
    for p in range(3):
        assert np.array_equal(host[p, :, 0], rows[(H, W)][p, :, 0]), (p, host[p, :, 0], rows[(H, W)][p, :, 0])
        assert np.array_equal(host[p], rows[(H, W)][p]), p
    got = _deflate(got_rows, S)
    bound = R.stream_bound(H, 3 * W, S)
    for p in range(3):
        want, infos = streams[(H, W, S)][p]
        assert len(got[p]) == len(want), (p, len(got[p]), len(want))
        assert got[p] == want, (p, next(k for k in range(len(want)) if got[p][k] != want[k]))
        # conditions of the stream, not measurements: inside the bound, never above the fixed-code cost of the same rows
        assert len(got[p]) <= bound and len(got[p]) <= G.fixed_cost(rows[(H, W)][p], S), p
        assert zlib.decompress(got[p]) == rows[(H, W)][p].tobytes(), p
        assert np.array_equal(G.unfilter(zlib.decompress(got[p]), W), imgs[(H, W)][p]), p


def test_uniform_random_bytes_stay_inside_the_bound_with_the_fixed_block(reference):
    """the all-literal case: no run, every byte value about equally often -- a code of its own cannot pay for its header in a strip
    of one short row, so the fixed block must win there, and the stream stays inside tce_png_stream_bound"""
    imgs, rows, streams = reference
    H, W, S = 33, 21, 1
    _, infos = streams[(H, W, S)][2]
    assert D_kinds(infos).count("fixed") >= H // 2
    got = _deflate(rows[(H, W)][2:3], S)
    assert got[0] == streams[(H, W, S)][2][0]
    assert len(got[0]) <= _lib.lib_raw().tce_png_stream_bound(H, 3 * W, S) == R.stream_bound(H, 3 * W, S)
    rng = np.random.default_rng(2)
    noise = rng.integers(0, 256, (1, 40, 64), dtype=np.uint8)                       # rows as they are: any bytes, any first byte
    for S in (1, 3, 40):
        got = _deflate(noise, S)
        want, _ = G.rows_stream(noise[0], S)
        assert got[0] == want and len(got[0]) <= R.stream_bound(40, 63, S) and len(got[0]) <= G.fixed_cost(noise[0], S)
        assert zlib.decompress(got[0]) == noise[0].tobytes()


def D_kinds(infos):
    return [i["kind"] for i in infos]


def test_rows_longer_than_a_chunk_and_strips_longer_than_a_pass():
    """W = 1500: a row of 4500 bytes is two chunks of the filter kernel (4096) and three passes of the strip kernel (2048)"""
    H, W, S = 3, 1500, 2
    rng = np.random.default_rng(8)
    x = np.arange(W)
    img = np.stack([np.stack([(x // 3) % 256, (x // 5 + 7 * y) % 256, (x * y) % 256], -1) for y in range(H)]).astype(np.uint8)
    img[1, 1360:1380] = rng.integers(0, 256, (20, 3))                              # around the chunk boundary (byte 4096 = pixel 1365)
    want_rows = G.filtered_rows(img)
    rows = _filter(img[None])
    assert np.array_equal(rows.cpu().numpy()[0], want_rows)
    got = _deflate(rows, S)
    assert got[0] == G.rows_stream(want_rows, S)[0]
    assert np.array_equal(G.unfilter(zlib.decompress(got[0]), W), img)


def test_every_filter_type_is_chosen_somewhere():
    H, W = 12, 40
    rng = np.random.default_rng(4)
    y, x = np.mgrid[0:H, 0:W]
    img = np.stack([4 * x + 3 * y, 2 * x + 5 * y + 20, 3 * x + 3 * y + 9], -1).astype(np.int64)
    img[0:2] = 0                                                                     # type 0
    img[2] = np.stack([5 * x[2], 5 * x[2] + 1, 3 * x[2]], -1)                        # a ramp over zeros: Sub
    img[3] = img[2]                                                                  # the row above again: Up
    img[6:8] = rng.integers(0, 256, (2, W, 3))
    img = np.clip(img, 0, 255).astype(np.uint8)
    want = G.filtered_rows(img)
    assert {0, 1, 2} <= set(want[:, 0].tolist()) and len(set(want[:, 0].tolist())) >= 4
    assert np.array_equal(_filter(img[None]).cpu().numpy()[0], want)


def test_images_encoded_together_equal_images_encoded_alone_and_pillow_opens_them(reference):
    from tce_rvos_amd import png
    imgs = reference[0][(37, 53)]
    t = torch.from_numpy(imgs).cuda()
    together = png.rgb_pngs(t)
    for p in range(3):
        alone = png.rgb_pngs(t[p:p + 1])
        assert alone[0] == together[p], p
        assert np.array_equal(G.decode_file(together[p]), imgs[p]), p
    for S in (1, 5):
        for p, blob in enumerate(png.rgb_pngs(t, rows_per_strip=S)):
            assert np.array_equal(G.decode_file(blob), imgs[p]), (S, p)
    from PIL import Image
    for p in range(3):
        im = Image.open(io.BytesIO(together[p]))
        assert im.mode == "RGB" and np.array_equal(np.asarray(im), imgs[p])
    with pytest.raises(ValueError):
        png.encode(t, "RGB")                                                          # encode and frame keep to 'L' and 'P'


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_images_rows_and_streams_at_any_address_and_sentinels_untouched(offset):
    from tce_rvos_amd import ops
    P, H, W, S = 2, 6, 11, 4                                                         # rows of 34 bytes: no two start alike
    img = G.images(H, W, offset)[1:3]
    n_img, n_rows = P * H * W * 3, P * H * (1 + 3 * W)
    inbuf = torch.full((n_img + 8,), 0xAB, dtype=torch.uint8, device="cuda")
    inbuf[offset:offset + n_img] = torch.from_numpy(img).cuda().reshape(-1)
    rowbuf = torch.full((n_rows + 8,), 0xCD, dtype=torch.uint8, device="cuda")
    images = inbuf[offset:offset + n_img].view(P, H, W, 3)
    rows = rowbuf[offset:offset + n_rows].view(P, H, 1 + 3 * W)
    assert images.data_ptr() % 4 == offset and rows.data_ptr() % 4 == offset
    ret = ops.png_filter_rgb(images, rows=rows)
    torch.cuda.synchronize()
    assert ret.data_ptr() == rows.data_ptr()
    want = np.stack([G.filtered_rows(im) for im in img])
    host = rowbuf.cpu().numpy()
    assert np.array_equal(host[offset:offset + n_rows].reshape(P, H, -1), want)
    assert (host[:offset] == 0xCD).all() and (host[offset + n_rows:] == 0xCD).all()
    bound = R.stream_bound(H, 3 * W, S)
    outbuf = torch.full((P * bound + 16,), 0xEF, dtype=torch.uint8, device="cuda")
    streams = outbuf[offset:offset + P * bound].view(P, bound)
    got = _deflate(rows, S, streams=streams)
    out = outbuf.cpu().numpy()
    assert (out[:offset] == 0xEF).all() and (out[offset + P * bound:] == 0xEF).all()
    for p in range(P):
        w = G.rows_stream(want[p], S)[0]
        assert got[p] == w, p
        assert (out[offset + p * bound + len(w):offset + (p + 1) * bound] == 0xEF).all(), p
    assert np.array_equal(images.cpu().numpy(), img) and (inbuf.cpu().numpy()[:offset] == 0xAB).all()


def test_rejected_arguments_launch_nothing():
    l = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    buf = torch.full((4096,), 0x5A, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(4096, dtype=torch.int64, device="cuda")
    nb = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    a, b = buf.data_ptr(), buf.data_ptr() + 2048
    assert l.tce_png_filter_rgb_u8(a, b, 0, 4, 4, s) < 0 and b"tce_png_filter_rgb_u8" in l.tce_last_error()
    assert l.tce_png_filter_rgb_u8(a, b, 1, 4, 0, s) < 0
    assert l.tce_png_filter_rgb_u8(None, b, 1, 4, 4, s) < 0
    assert l.tce_png_filter_rgb_u8(a, b, 1, 30000, 30000, s) < 0
    assert l.tce_png_deflate_rows_u8(a, b, nb.data_ptr(), ws.data_ptr(), 1, 4, 1, 4, s) < 0 and b"tce_png_deflate_rows_u8" in l.tce_last_error()
    assert l.tce_png_deflate_rows_u8(a, b, nb.data_ptr(), ws.data_ptr(), 1, 4, 8, 0, s) < 0
    assert l.tce_png_deflate_rows_u8(a, b, nb.data_ptr(), ws.data_ptr() + 4, 1, 4, 8, 4, s) < 0
    assert l.tce_png_deflate_rows_u8(a, None, nb.data_ptr(), ws.data_ptr(), 1, 4, 8, 4, s) < 0
    torch.cuda.synchronize()
    assert bool((buf == 0x5A).all()) and nb.cpu().tolist() == [-7] * 4


# ----------------------------------------------------------------------------------------------- the recorder and the footprint
@pytest.fixture(scope="module")
def slab():
    s = fp.Slab(16 << 20, device="cuda")
    yield s
    del s
    torch.cuda.empty_cache()


def test_png_filter_rgb_footprint(slab):
    P, H, W, shift_i, shift_r = 2, 5, 9, 3, 1
    img = G.images(H, W, 3)[1:3]
    n_img, n_rows = P * H * W * 3, P * H * (1 + 3 * W)

    def build(s):
        host = np.zeros(shift_i + n_img + 3, np.uint8)
        host[shift_i:shift_i + n_img] = img.reshape(-1)
        raw_i = s.put("img", host)
        raw_r = s.alloc("rows", (shift_r + n_rows + 3,), dtype=torch.uint8)

        def fn():
            _lib.check(_lib.lib().tce_png_filter_rgb_u8(raw_i.data_ptr() + shift_i, raw_r.data_ptr() + shift_r, P, H, W,
                                                        torch.cuda.current_stream().cuda_stream), "tce_png_filter_rgb_u8")
        fn.check = lambda: raw_r[shift_r:shift_r + n_rows]
        return fn

    info = fp.check_case(slab, build, fp.recorder("tce_png_filter_rgb_u8"), props="WOR", sync=torch.cuda.synchronize,
                         label="tce_png_filter_rgb_u8")
    assert (info["W"], info["O"], info["R"]) == (2, 2, 3) and info["read_bytes"] == n_img and info["written_bytes"] == n_rows
    slab.begin(0)
    fn = build(slab)
    fn()
    torch.cuda.synchronize()
    assert np.array_equal(fn.check().cpu().numpy().reshape(P, H, -1), np.stack([G.filtered_rows(im) for im in img]))


TAIL = 0xEE


def test_png_deflate_rows_footprint(slab):
    """as test_png_gpu.check_footprint: the model names whole rows of streams, so the case fills each row's tail behind nbytes[p] on
    the device; ws is exempt from O and scratch under R"""
    P, H, Rw, S, shift_r, shift_s = 2, 5, 700, 4, 1, 3                               # a strip of 2800 bytes: more than one pass
    rng = np.random.default_rng(12)
    rows = (rng.integers(0, 6, (P, H, Rw)) * (rng.random((P, H, Rw)) < 0.5)).astype(np.uint8)
    n_rows, bound = P * H * Rw, R.stream_bound(H, Rw - 1, S)
    wsb = _lib.lib_raw().tce_png_ws_bytes(P, H, Rw - 1, S)

    def build(s):
        host = np.zeros(shift_r + n_rows + 3, np.uint8)
        host[shift_r:shift_r + n_rows] = rows.reshape(-1)
        raw_r = s.put("rows", host)
        raw_s = s.alloc("streams", (shift_s + P * bound + 3,), dtype=torch.uint8)
        nbytes = s.alloc("nbytes", (P,), dtype=torch.int32)
        ws = s.alloc("ws", (wsb // 8,), dtype=torch.int64)
        view = raw_s[shift_s:shift_s + P * bound].view(P, bound)
        col = torch.arange(bound, dtype=torch.int32, device=s.device)[None]

        def fn():
            _lib.check(_lib.lib().tce_png_deflate_rows_u8(raw_r.data_ptr() + shift_r, raw_s.data_ptr() + shift_s, nbytes.data_ptr(),
                                                          ws.data_ptr(), P, H, Rw, S, torch.cuda.current_stream().cuda_stream),
                       "tce_png_deflate_rows_u8")
            view.masked_fill_(col >= nbytes[:, None], TAIL)
        fn.check = lambda: (view, nbytes)
        return fn

    info = fp.check_case(slab, build, fp.recorder("tce_png_deflate_rows_u8"), exempt=("ws",), scratch=("ws",), props="WOR",
                         sync=torch.cuda.synchronize, label="tce_png_deflate_rows_u8")
    assert (info["W"], info["O"], info["R"]) == (2, 2, 3) and info["exempt"] == ["ws"]
    assert info["read_bytes"] == n_rows + wsb and info["written_bytes"] == P * bound + 4 * P + wsb
    slab.begin(0)
    fn = build(slab)
    fn()
    torch.cuda.synchronize()
    view, nbytes = fn.check()
    view, n = view.cpu().numpy(), nbytes.cpu().tolist()
    for p in range(P):
        want = G.rows_stream(rows[p], S)[0]
        assert view[p, :n[p]].tobytes() == want and (view[p, n[p]:] == TAIL).all(), p


def test_hazard_recording_lists_the_two_entries(reference):
    from tce_rvos_amd import ops
    t = torch.from_numpy(reference[0][(9, 12)]).cuda()
    want_s, want_n = ops.png_deflate_rows(ops.png_filter_rgb(t), rows_per_strip=8)
    with hazard.recording() as rec:
        got_s, got_n = ops.png_deflate_rows(ops.png_filter_rgb(t), rows_per_strip=8)
    torch.cuda.synchronize()
    assert [x.name for x in rec.launches] == ["tce_png_filter_rgb_u8", "tce_png_deflate_rows_u8"]
    assert rec.analyse().clean and torch.equal(got_n, want_n)
    for p, n in enumerate(want_n.tolist()):
        assert n > 0 and torch.equal(got_s[p, :n], want_s[p, :n]), p
