"""PNG-file stage on the GPU: tce_png_file_u8 (include/tce_rvos_pngfile.h) byte for byte against its restatement (tests/_png_file.py)
at every length around a piece and a segment, with random, all-zero and all-0xFF data, streams and files off every alignment, one
long row; png.mask_pngs / label_pngs / rgb_pngs with framing="device" against framing="host" and Pillow; the access model against
the bytes the launches touch; rejected arguments; the call replayed from a graph."""
import io

import numpy as np
import pytest
import torch

import _footprint as fp
import _png_file as F
import _png_rgb as G
from tce_rvos_amd import _lib, hazard, ops, png

pytestmark = pytest.mark.gpu

PIECE, SEG = ops.PNG_FILE_PIECE, ops.PNG_FILE_SEGMENT
LENGTHS = list(range(0, 2 * PIECE + 6)) + [SEG - 1, SEG, SEG + 1, 2 * SEG - 1, 2 * SEG + 1, 3 * SEG + 7]
STRIDE = 3 * SEG + 7                                                 # odd; the longest length is n == stream_stride
FILL, TAIL_A, TAIL_B, GUARD = 0xA5, 0x3C, 0xD2, 512
HEAD_L = png.head(53, 37, "L")


@pytest.fixture(scope="module")
def data():
    """the three kinds of stream bytes, STRIDE of each -- made once, never changed"""
    rng = np.random.default_rng(23)
    return {"random": rng.integers(0, 256, STRIDE, dtype=np.uint8), "zero": np.zeros(STRIDE, np.uint8), "ff": np.full(STRIDE, 255, np.uint8)}


def _heads():
    pal = bytes((91 * k + 7) % 256 for k in range(768))
    heads = [HEAD_L, png.head(53, 37, "P", pal[:3]), png.head(53, 37, "P", pal[:6]), png.head(53, 37, "P", pal)]
    assert [len(h) for h in heads] == [33, 48, 51, 813]
    # the data starts head + 8 bytes into its row: 1, 0, 3, 1 modulo 4, and with rows that start 1, 2 and 3 bytes off, every offset
    assert {(len(h) + 8 + off) % 4 for h in heads for off in (1, 2, 3)} == {0, 1, 2, 3}
    return heads


def _run(rows, head, stride=None, s_off=0, s_pad=0, f_off=0, f_pad=0):
    """ops.png_file on rows (a list of P byte strings) laid into stream rows `stride` apart that start s_off bytes into their tensor
    (s_pad > 0: the tensor handed over is a view of rows stride - s_pad wide), files likewise; every check of the direct case"""
    P = len(rows)
    width = (max(len(r) for r in rows) if stride is None else stride - s_pad) or 1
    stride = width + s_pad
    want = [F.file_bytes(head, r) for r in rows]
    bound = len(head) + 24 + stride
    fstride = bound + f_pad
    outs = []
    for tail in (TAIL_A, TAIL_B):                                   # what lies behind n in a stream row is no input
        host = np.full(s_off + P * stride + 8, tail, np.uint8)
        for p, r in enumerate(rows):
            host[s_off + p * stride:s_off + p * stride + len(r)] = np.frombuffer(r, np.uint8)
        sbuf = torch.from_numpy(host).cuda()
        streams = sbuf[s_off:s_off + P * stride].view(P, stride)[:, :width]
        nbytes = torch.tensor([len(r) for r in rows], dtype=torch.int32, device="cuda")
        fbuf = torch.full((GUARD + f_off + P * fstride + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        files = fbuf[GUARD + f_off:GUARD + f_off + P * fstride].view(P, fstride)[:, :bound]
        assert streams.data_ptr() % 4 == (sbuf.data_ptr() + s_off) % 4 and files.data_ptr() % 4 == (fbuf.data_ptr() + GUARD + f_off) % 4
        ret, fb = ops.png_file(streams, nbytes, head, files=files if (f_off or f_pad) else None)
        torch.cuda.synchronize()
        assert tuple(ret.shape) == (P, bound) and ret.dtype == torch.uint8 and fb.dtype == torch.int32 and tuple(fb.shape) == (P,)
        assert fb.cpu().tolist() == [len(w) for w in want] == [len(head) + 24 + len(r) for r in rows]
        if f_off or f_pad:
            assert ret.data_ptr() == files.data_ptr()
            out = fbuf.cpu().numpy()
            assert (out[:GUARD + f_off] == FILL).all() and (out[GUARD + f_off + P * fstride:] == FILL).all()   # the guard band
            got = out[GUARD + f_off:GUARD + f_off + P * fstride].reshape(P, fstride)
            for p, w in enumerate(want):
                assert got[p, :len(w)].tobytes() == w, (p, len(rows[p]))
                assert (got[p, len(w):] == FILL).all(), (p, len(rows[p]))     # behind file_bytes[p], pad columns included
        else:
            got = ret.cpu().numpy()
            for p, w in enumerate(want):
                assert got[p, :len(w)].tobytes() == w, (p, len(rows[p]))
        assert np.array_equal(sbuf.cpu().numpy(), host)             # the inputs are inputs
        outs.append([got[p, :len(w)].tobytes() for p, w in enumerate(want)])
    assert outs[0] == outs[1]


@pytest.mark.parametrize("kind", ["random", "zero", "ff"])
def test_single_files_at_every_length_equal_the_restatement(data, kind):
    d = data[kind]
    for n in LENGTHS:
        # files in a guard band with a fill behind them; the longest row fills its stream row (n == stream_stride)
        _run([d[:n].tobytes()], HEAD_L, stride=STRIDE if n > 2 * PIECE + 5 else 2 * PIECE + 8, f_pad=3)


@pytest.mark.parametrize("kind", ["random", "zero", "ff"])
def test_five_files_of_different_lengths_equal_the_restatement(data, kind):
    d = data[kind]
    small = [n for n in LENGTHS if n <= 2 * PIECE + 5]
    for k in range(0, len(small), 5):
        rows = [d[7 * p:7 * p + n].tobytes() for p, n in enumerate(small[k:k + 5])]
        _run(rows + [b""] * (5 - len(rows)), HEAD_L, stride=2 * PIECE + 40, f_pad=1)
    _run([d[:n].tobytes() for n in (SEG - 1, 3 * SEG + 7, 0, SEG + 1, 2 * SEG + 1)], HEAD_L, stride=STRIDE, f_pad=2)
    _run([d[:n].tobytes() for n in (2 * SEG - 1, SEG, 5, 3 * SEG + 7, PIECE)], HEAD_L, stride=STRIDE)


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_streams_and_files_at_any_address(data, offset):
    """heads of 33, 48, 51 and 813 bytes in file rows that start 1, 2 and 3 bytes into a larger tensor put the data at every offset
    modulo 4; streams likewise are views that start 1, 2 and 3 bytes into a larger tensor; both with an odd stride"""
    d = data["random"]
    rows = [d[:SEG + 5].tobytes(), d[100:231].tobytes(), b"", d[3:3 + 2 * PIECE + 1].tobytes()]
    for head in _heads():
        for f_off in (1, 2, 3):
            stride = SEG + 10 + (0 if (SEG + 10) % 2 else 1)
            assert stride % 2 == 1
            _run(rows, head, stride=stride, s_off=offset, s_pad=2, f_off=f_off, f_pad=2 if (len(head) + 24 + stride) % 2 else 3)


def test_one_long_row_beside_a_short_one():
    rng = np.random.default_rng(31)
    long = rng.integers(0, 256, 2_100_001, dtype=np.uint8).tobytes()
    _run([long, long[:1000]], HEAD_L, f_pad=1)


# ------------------------------------------------------------------------------------------------------------------- end to end
def _pillow(blob):
    from PIL import Image
    im = Image.open(io.BytesIO(blob))
    im.load()                                                        # verifies every chunk's CRC
    return im


@pytest.mark.parametrize("codes", ["fixed", "dynamic"])
@pytest.mark.parametrize("H,W", [(37, 53), (1, 1)])
def test_mask_and_label_files_equal_host_framing_and_decode(codes, H, W):
    rng = np.random.default_rng(H * 100 + W)
    masks = (rng.random((3, H, W)) < 0.4).astype(np.uint8)
    t = torch.from_numpy(masks).cuda()
    host, dev = png.mask_pngs(t, codes=codes), png.mask_pngs(t, codes=codes, framing="device")
    assert isinstance(dev, list) and all(isinstance(b, bytes) for b in dev) and dev == host
    for p, blob in enumerate(dev):
        im = _pillow(blob)
        assert im.mode == "L" and np.array_equal(np.asarray(im), masks[p] * 255), p
    for entries in (2, 256):
        pal = bytes((53 * k + 11) % 256 for k in range(3 * entries))
        labels = rng.integers(0, entries, (3, H, W), dtype=np.uint8)
        t = torch.from_numpy(labels).cuda()
        host, dev = png.label_pngs(t, pal, codes=codes), png.label_pngs(t, pal, codes=codes, framing="device")
        assert dev == host, entries
        for p, blob in enumerate(dev):
            im = _pillow(blob)
            assert im.mode == "P" and np.array_equal(np.asarray(im), labels[p]) and bytes(im.getpalette()[:3 * entries]) == pal, (entries, p)


def test_rgb_files_equal_host_framing_and_decode():
    imgs = G.images(19, 23, 5)
    t = torch.from_numpy(imgs).cuda()
    for S in (None, 4):
        host, dev = png.rgb_pngs(t, rows_per_strip=S), png.rgb_pngs(t, rows_per_strip=S, framing="device")
        assert len(dev) == 3 and dev == host
        for p, blob in enumerate(dev):
            im = _pillow(blob)
            assert im.mode == "RGB" and np.array_equal(np.asarray(im), imgs[p]), (S, p)


# ------------------------------------------------------------------------------------------------ the recorder and the footprint
@pytest.fixture(scope="module")
def slab():
    s = fp.Slab(16 << 20, device="cuda")
    yield s
    del s
    torch.cuda.empty_cache()


TAIL = 0xEE


@pytest.mark.parametrize("case", ["segments", "palette_head"])
def test_png_file_footprint(slab, data, case):
    """as the deflate entries' cases: the model names whole rows of files, so the case fills each row's tail behind file_bytes[p] on
    the device; ws is exempt from O and scratch under R"""
    d = data["random"]
    if case == "segments":
        head, ss, shift_s, shift_f, lens = HEAD_L, 2 * SEG + 3, 1, 3, [2 * SEG + 3, SEG - 1]
    else:
        head, ss, shift_s, shift_f, lens = _heads()[3], 301, 3, 2, [0, 300, 2 * PIECE + 1]
    P, hb = len(lens), len(head)
    bound = hb + 24 + ss
    wsb = _lib.lib_raw().tce_png_file_ws_bytes(P, ss)
    assert bound == _lib.lib_raw().tce_png_file_bound(hb, ss)

    def build(s):
        host = np.full(shift_s + P * ss + 3, 0x77, np.uint8)
        for p, n in enumerate(lens):
            host[shift_s + p * ss:shift_s + p * ss + n] = d[p:p + n]
        raw_s = s.put("streams", host)
        nbytes = s.put("nbytes", np.array(lens, np.int32))
        hd = s.put("head", np.frombuffer(head, np.uint8).copy())
        raw_f = s.alloc("files", (shift_f + P * bound + 3,), dtype=torch.uint8)
        fb = s.alloc("file_bytes", (P,), dtype=torch.int32)
        ws = s.alloc("ws", (wsb // 8,), dtype=torch.int64)
        view = raw_f[shift_f:shift_f + P * bound].view(P, bound)
        col = torch.arange(bound, dtype=torch.int32, device=s.device)[None]

        def fn():
            _lib.check(_lib.lib().tce_png_file_u8(raw_s.data_ptr() + shift_s, nbytes.data_ptr(), hd.data_ptr(), hb, raw_f.data_ptr() + shift_f,
                                                  fb.data_ptr(), ws.data_ptr(), P, ss, bound, torch.cuda.current_stream().cuda_stream),
                       "tce_png_file_u8")
            view.masked_fill_(col >= fb[:, None], TAIL)
        fn.check = lambda: (view, fb)
        return fn

    info = fp.check_case(slab, build, fp.recorder("tce_png_file_u8"), exempt=("ws",), scratch=("ws",), props="WOR",
                         sync=torch.cuda.synchronize, label=f"tce_png_file_u8[{case}]")
    assert (info["W"], info["O"], info["R"]) == (2, 2, 3) and info["exempt"] == ["ws"]
    assert info["read_bytes"] == P * ss + 4 * P + hb + wsb and info["written_bytes"] == P * bound + 4 * P + wsb
    slab.begin(0)
    fn = build(slab)
    fn()
    torch.cuda.synchronize()
    view, fb = fn.check()
    view, n = view.cpu().numpy(), fb.cpu().tolist()
    for p in range(P):
        want = F.file_bytes(head, d[p:p + lens[p]].tobytes())
        assert n[p] == len(want) and view[p, :n[p]].tobytes() == want and (view[p, n[p]:] == TAIL).all(), p


def test_hazard_recording_of_device_framing_is_race_free():
    imgs = G.images(9, 12, 2)
    t = torch.from_numpy(imgs).cuda()
    want = png.rgb_pngs(t)
    with hazard.recording() as rec:
        got = png.rgb_pngs(t, framing="device")
    torch.cuda.synchronize()
    assert [x.name for x in rec.launches] == ["tce_png_filter_rgb_u8", "tce_png_deflate_rows_u8", "tce_png_file_u8"]
    assert rec.analyse().clean and got == want
    with hazard.recording() as rec:                                  # the default framing launches what it launched before
        assert png.rgb_pngs(t) == want
    assert [x.name for x in rec.launches] == ["tce_png_filter_rgb_u8", "tce_png_deflate_rows_u8"]


# -------------------------------------------------------------------------------------------------------------- rejected arguments
def test_rejected_arguments_raise_and_launch_nothing():
    P, n = 2, 200
    buf = torch.full((8192,), 0x5A, dtype=torch.uint8, device="cuda")
    streams = buf[:P * n].view(P, n)
    nbytes = torch.full((P,), n, dtype=torch.int32, device="cuda")
    bound = len(HEAD_L) + 24 + n
    files = torch.full((P, bound), 0x6B, dtype=torch.uint8, device="cuda")
    fb = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    short = torch.as_strided(torch.full((P * bound,), 0x6B, dtype=torch.uint8, device="cuda"), (P, bound), (bound - 1, 1))
    cases = {
        "P = 0": lambda: ops.png_file(streams[:0], nbytes[:0], HEAD_L),
        "head of 7 bytes": lambda: ops.png_file(streams, nbytes, HEAD_L[:7], files=None, file_bytes=fb),
        "head of 1025 bytes": lambda: ops.png_file(streams, nbytes, bytes(1025), file_bytes=fb),
        "file_stride one short": lambda: ops.png_file(streams, nbytes, HEAD_L, files=short, file_bytes=fb),
        "files of another bound": lambda: ops.png_file(streams, nbytes, HEAD_L, files=files[:, :bound - 1], file_bytes=fb),
        "files over streams": lambda: ops.png_file(streams, nbytes, HEAD_L, files=buf[n:n + P * bound].view(P, bound), file_bytes=fb),
        "nbytes int64": lambda: ops.png_file(streams, nbytes.long(), HEAD_L, files=files, file_bytes=fb),
        "nbytes of another length": lambda: ops.png_file(streams, nbytes[:1], HEAD_L, files=files, file_bytes=fb),
        "streams int8": lambda: ops.png_file(streams.view(torch.int8), nbytes, HEAD_L, files=files, file_bytes=fb),
        "ws too small": lambda: ops.png_file(streams, nbytes, HEAD_L, files=files, file_bytes=fb, ws=torch.zeros(1, dtype=torch.int32, device="cuda")),
    }
    for what, call in cases.items():
        with pytest.raises(ValueError, match="png_file"):
            call()
        assert isinstance(what, str)
    # the entry itself: each rejected with a message, before anything is launched
    l, s = _lib.lib(), torch.cuda.current_stream().cuda_stream
    hd = torch.frombuffer(bytearray(HEAD_L), dtype=torch.uint8).cuda()
    ws = torch.zeros(64, dtype=torch.int64, device="cuda")
    a = dict(streams=streams.data_ptr(), nbytes=nbytes.data_ptr(), head=hd.data_ptr(), hb=len(HEAD_L), files=files.data_ptr(), fb=fb.data_ptr(),
             ws=ws.data_ptr(), P=P, ss=n, fs=bound)

    def entry(**kw):
        b = dict(a, **kw)
        return l.tce_png_file_u8(b["streams"], b["nbytes"], b["head"], b["hb"], b["files"], b["fb"], b["ws"], b["P"], b["ss"], b["fs"], s)

    for kw in (dict(P=0), dict(P=65536), dict(hb=7), dict(hb=1025), dict(ss=0), dict(fs=bound - 1), dict(fs=2 ** 31 - 4096), dict(files=None),
               dict(ws=ws.data_ptr() + 4), dict(nbytes=nbytes.data_ptr() + 2), dict(fb=fb.data_ptr() + 1), dict(files=streams.data_ptr() + n),
               dict(files=buf.data_ptr() + 4096, head=buf.data_ptr() + 4096 + bound)):
        assert entry(**kw) < 0 and b"tce_png_file_u8" in l.tce_last_error(), kw
    torch.cuda.synchronize()
    assert bool((files == 0x6B).all()) and bool((short == 0x6B).all()) and bool((buf == 0x5A).all()) and fb.cpu().tolist() == [-7] * P
    assert bool((ws == 0).all())


# --------------------------------------------------------------------------------------------------------------------------- replay
def test_the_call_replays_from_a_graph_with_new_stream_content(data):
    P, stride = 3, SEG + 77
    streams = torch.zeros(P, stride, dtype=torch.uint8, device="cuda")
    nbytes = torch.zeros(P, dtype=torch.int32, device="cuda")
    head = torch.frombuffer(bytearray(HEAD_L), dtype=torch.uint8).cuda()
    bound = len(HEAD_L) + 24 + stride
    files = torch.full((P, bound), FILL, dtype=torch.uint8, device="cuda")
    fb = torch.zeros(P, dtype=torch.int32, device="cuda")
    ws = torch.zeros(_lib.lib_raw().tce_png_file_ws_bytes(P, stride) // 8, dtype=torch.int64, device="cuda")
    ops.png_file(streams, nbytes, head, files=files, file_bytes=fb, ws=ws)       # the kernels are loaded before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.png_file(streams, nbytes, head, files=files, file_bytes=fb, ws=ws)
    rng = np.random.default_rng(41)
    for lens in ([SEG + 77, 5, 0], [PIECE, SEG + 1, 300]):
        rows = [rng.integers(0, 256, n, dtype=np.uint8) for n in lens]
        host = np.full((P, stride), 0x11, np.uint8)
        for p, r in enumerate(rows):
            host[p, :len(r)] = r
        streams.copy_(torch.from_numpy(host).cuda())
        nbytes.copy_(torch.tensor(lens, dtype=torch.int32))
        files.fill_(FILL)
        ws.fill_(-1)                                                 # workspace content is irrelevant before a call
        g.replay()
        torch.cuda.synchronize()
        out, n = files.cpu().numpy(), fb.cpu().tolist()
        for p, r in enumerate(rows):
            want = F.file_bytes(HEAD_L, r.tobytes())
            assert n[p] == len(want) and out[p, :n[p]].tobytes() == want and (out[p, n[p]:] == FILL).all(), (lens, p)
