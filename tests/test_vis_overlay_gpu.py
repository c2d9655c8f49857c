"""Overlay stage on the GPU: tce_vis_overlay_u8 (include/tce_rvos_vis.h) byte for byte against the Pillow-rendered fixture
(tests/golden/vis_overlay_cases.npz) and against the rule's restatement (tests/_vis.py) where Pillow is not the rule (thin boxes);
every optional pointer NULL in turn; frames and out off every alignment, W0 = 1 and H0 = 1; rejected arguments; vis.py's two
functions; the access model against the bytes the launch touches."""
import os

import numpy as np
import pytest
import torch

import _footprint as fp
import _vis as V
from tce_rvos_amd import _lib, hazard

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(HERE, "golden", "vis_overlay_cases.npz")))


def _cuda(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _run(frames, colors, masks=None, boxes=None, points=None, **kw):
    from tce_rvos_amd import ops
    out = ops.vis_overlay(_cuda(frames), _cuda(colors), masks=_cuda(masks), boxes=_cuda(boxes, np.float32),
                          points=_cuda(points, np.float32), **kw)
    torch.cuda.synchronize()
    assert out.dtype == torch.uint8 and tuple(out.shape) == tuple(frames.shape)
    return out.cpu().numpy()


def _first_diff(got, want):
    bad = np.argwhere(got != want)
    return None if not len(bad) else (tuple(bad[0]), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]), len(bad))


@pytest.mark.parametrize("tag", ["s", "m"])
def test_kernel_equals_the_pillow_fixture(golden, tag):
    g = {k[2:]: v for k, v in golden.items() if k.startswith(tag + "_")}
    f = g["frames"]
    got = _run(f, g["a_colors"], g["a_masks"], g["a_boxes"], g["a_points"])              # L = 1: mask + box + point
    assert _first_diff(got, g["a_out"]) is None, _first_diff(got, g["a_out"])
    got = _run(f, g["b_colors"], None, g["b_boxes"], None)                                # L = 3: boxes only
    assert _first_diff(got, g["b_out"]) is None, _first_diff(got, g["b_out"])
    got = _run(f, g["a_colors"], g["c_masks"], None, g["c_points"])
    assert _first_diff(got, g["c_out"]) is None, _first_diff(got, g["c_out"])
    got = _run(f, g["a_colors"], None, None, g["d_points"])
    assert _first_diff(got, g["d_out"]) is None, _first_diff(got, g["d_out"])


def test_every_optional_pointer_null_in_turn(golden):
    g = {k[2:]: v for k, v in golden.items() if k.startswith("s_")}
    f, col = g["frames"], g["a_colors"]
    parts = {"masks": g["a_masks"], "boxes": g["a_boxes"], "points": g["a_points"]}
    seen = []
    for drop in ("masks", "boxes", "points", None):
        kw = {k: v for k, v in parts.items() if k != drop}
        got = _run(f, col, **kw)
        want = V.overlay(f, col, **kw)
        assert _first_diff(got, want) is None, (drop, _first_diff(got, want))
        seen.append(got)
    assert all(not np.array_equal(seen[k], seen[3]) for k in range(3))                    # each part draws something
    assert np.array_equal(_run(f, col), f)                                                # nothing given: a copy


def test_thin_and_degenerate_boxes_equal_the_restatement():
    H, W, N = 23, 31, 4
    rng = np.random.default_rng(11)
    frames = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)

    def box(x0, y0, x1, y1):
        return [(x0 + x1) / 2 / W, (y0 + y1) / 2 / H, (x1 - x0) / W, (y1 - y0) / H]

    boxes = np.array([[box(5.25, 4.25, 6.75, 12.75), box(5.25, 4.25, 5.75, 4.75), box(8.5, 4.5, 3.5, 9.5), box(-4.5, 3.5, -3.75, 9.5)],
                      [box(-0.75, 2.25, 0.75, 9.25), box(3.25, 3.25, 5.75, 5.75), box(2.0, 20.5, 40.0, 21.5), box(29.5, -3.0, 30.9, 40.0)],
                      [box(0, 0, 0, 0), box(0, 0, W, H), box(4.0, 9.0, 20.0, 3.0), box(-50.0, -50.0, 90.0, 90.0)]], dtype=np.float32)
    thin = [not V.is_regular(b, H, W) for b in boxes.reshape(-1, 4)]
    assert sum(thin) >= 8
    col = np.array([[255, 0, 0], [0, 255, 0], [1, 2, 3]], np.uint8)
    got, want = _run(frames, col, boxes=boxes), V.overlay(frames, col, boxes=boxes)
    assert _first_diff(got, want) is None, _first_diff(got, want)
    assert not np.array_equal(got, frames)
    # random boxes of both classes, sixteen layers
    L = 16
    boxes = rng.uniform(-0.2, 1.2, (L, N, 4)).astype(np.float32)
    boxes[..., 2:] = rng.uniform(-0.05, 0.3, (L, N, 2))
    points = rng.uniform(-0.1, 1.1, (L, N, 2)).astype(np.float32)
    masks = (rng.random((L, N, H, W)) < 0.2).astype(np.uint8) * rng.integers(1, 256, (L, N, H, W), dtype=np.uint8)
    col = rng.integers(0, 256, (L, 3), dtype=np.uint8)
    got, want = _run(frames, col, masks, boxes, points), V.overlay(frames, col, masks, boxes, points)
    assert _first_diff(got, want) is None, _first_diff(got, want)


@pytest.mark.parametrize("H,W", [(1, 1), (1, 9), (7, 1), (5, 6), (33, 70)])
@pytest.mark.parametrize("off_in,off_out", [(0, 0), (1, 3), (2, 1), (3, 2)])
def test_any_address_and_single_rows_and_columns(H, W, off_in, off_out):
    """(33, 70): several workgroups per frame (6930 bytes > 4 * 256 * 4).  The bytes around frames and out keep their sentinels."""
    from tce_rvos_amd import ops
    N, L = 3, 2
    rng = np.random.default_rng(H * 100 + W + off_in)
    frames = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    boxes = np.array([[[0.5, 0.5, 0.6, 0.6]] * N, [[0.2, 0.3, 0.5, 0.9]] * N], np.float32)
    points = rng.uniform(0, 1, (L, N, 2)).astype(np.float32)
    masks = (rng.random((L, N, H, W)) < 0.5).astype(np.uint8)
    col = np.array([[200, 100, 50], [10, 250, 30]], np.uint8)
    total = N * H * W * 3
    inbuf = torch.full((total + 8,), 0xAB, dtype=torch.uint8, device="cuda")
    inbuf[off_in:off_in + total] = torch.from_numpy(frames).cuda().reshape(-1)
    outbuf = torch.full((total + 8,), 0xCD, dtype=torch.uint8, device="cuda")
    f = inbuf[off_in:off_in + total].view(N, H, W, 3)
    o = outbuf[off_out:off_out + total].view(N, H, W, 3)
    assert f.data_ptr() % 4 == off_in and o.data_ptr() % 4 == off_out
    ret = ops.vis_overlay(f, _cuda(col), masks=_cuda(masks), boxes=_cuda(boxes), points=_cuda(points), out=o)
    torch.cuda.synchronize()
    assert ret.data_ptr() == o.data_ptr()
    want = V.overlay(frames, col, masks, boxes, points)
    got = outbuf.cpu().numpy()
    assert _first_diff(got[off_out:off_out + total].reshape(N, H, W, 3), want) is None
    assert (got[:off_out] == 0xCD).all() and (got[off_out + total:] == 0xCD).all()
    assert np.array_equal(f.cpu().numpy(), frames) and (inbuf.cpu().numpy()[:off_in] == 0xAB).all()


def test_rejected_arguments_launch_nothing():
    l = _lib.lib()
    N, H, W = 2, 4, 5
    total = N * H * W * 3
    buf = torch.full((2 * total,), 0x5A, dtype=torch.uint8, device="cuda")
    col = torch.zeros(17, 3, dtype=torch.uint8, device="cuda")
    f, o = buf.data_ptr(), buf.data_ptr() + total
    s = torch.cuda.current_stream().cuda_stream
    for L, fr, out, what in ((0, f, o, b"L = 0"), (17, f, o, b"L = 17"), (1, f, f, b"overlap"), (1, f, f + total - 1, b"overlap"),
                             (1, f + 1, f, b"overlap"), (1, None, o, b"null"), (1, f, o, None)):
        if what is None:
            assert l.tce_vis_overlay_u8(fr, out, None, None, None, None, L, N, H, W, s) < 0                # colors NULL
        else:
            assert l.tce_vis_overlay_u8(fr, out, None, None, None, col.data_ptr(), L, N, H, W, s) < 0, what
            assert what in l.tce_last_error() and b"tce_vis_overlay_u8" in l.tce_last_error(), l.tce_last_error()
    assert l.tce_vis_overlay_u8(f, o, None, None, None, col.data_ptr(), 1, 0, H, W, s) < 0
    assert l.tce_vis_overlay_u8(f, o, None, None, None, col.data_ptr(), 1, N, 30000, 30000, s) < 0         # 2.7e9 bytes a frame
    torch.cuda.synchronize()
    assert bool((buf == 0x5A).all())
    from tce_rvos_amd import ops
    fr = buf[:total].view(N, H, W, 3)
    with pytest.raises(ValueError):
        ops.vis_overlay(fr, col)                                                                           # 17 layers
    with pytest.raises(_lib.TceError, match="overlap"):
        ops.vis_overlay(fr, col[:1], out=fr)
    with pytest.raises(ValueError):
        ops.vis_overlay(fr, col[:1], boxes=torch.zeros(1, N, 4, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        ops.vis_overlay(fr, col[:1], masks=torch.zeros(1, N, H, W + 1, dtype=torch.uint8, device="cuda"))


def test_overlay_expression_and_overlay_objects(golden):
    from tce_rvos_amd import vis
    g = {k[2:]: v for k, v in golden.items() if k.startswith("m_")}
    f = _cuda(g["frames"])
    result = {"masks": _cuda(g["a_masks"][0]), "pred_boxes": _cuda(g["a_boxes"][0]), "reference_points": _cuda(g["a_points"][0]),
              "best_query": None}
    got = vis.overlay_expression(f, result, [int(v) for v in g["a_colors"][0]])
    assert np.array_equal(got.cpu().numpy(), g["a_out"])
    del result["reference_points"]                                                         # run_video's default dict: no cross
    got = vis.overlay_expression(f, result, g["a_colors"][0])
    assert np.array_equal(got.cpu().numpy(), V.overlay(g["frames"], g["a_colors"], g["a_masks"], g["a_boxes"], None))
    got = vis.overlay_objects(f, _cuda(g["b_boxes"]), g["b_colors"].tolist())
    assert np.array_equal(got.cpu().numpy(), g["b_out"])
    with pytest.raises(ValueError):
        vis.overlay_objects(f, _cuda(g["b_boxes"]), [[1, 2, 3]])
    with pytest.raises(ValueError):
        vis.overlay_expression(f, result, [300, 0, 0])


# ----------------------------------------------------------------------------------------------- the recorder and the footprint
@pytest.fixture(scope="module")
def slab():
    s = fp.Slab(16 << 20, device="cuda")
    yield s
    del s
    torch.cuda.empty_cache()


@pytest.mark.parametrize("parts,shift_in,shift_out", [("mbp", 1, 3), ("b", 2, 0), ("m", 0, 1)], ids=["all_1_3", "boxes_2_0", "masks_0_1"])
def test_vis_overlay_footprint(slab, parts, shift_in, shift_out):
    """W, O and R of tests/_footprint.py: nothing outside out is written, every byte of out is written, and the result depends on no
    byte outside the modelled reads -- the bytes around the frames included."""
    N, H, W, L = 2, 13, 21, 2
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    masks = (rng.random((L, N, H, W)) < 0.4).astype(np.uint8)
    boxes = np.array([[[0.5, 0.5, 0.5, 0.5]] * N, [[0.1, 0.8, 0.4, 0.6]] * N], np.float32)
    points = rng.uniform(0, 1, (L, N, 2)).astype(np.float32)
    col = np.array([[200, 100, 50], [10, 250, 30]], np.uint8)
    total = N * H * W * 3

    def build(s):
        host = np.zeros(shift_in + total + 3, np.uint8)
        host[shift_in:shift_in + total] = frames.reshape(-1)
        raw_f = s.put("frames", host)
        raw_o = s.alloc("out", (shift_out + total + 3,), dtype=torch.uint8)
        m = s.put("masks", masks.reshape(-1)) if "m" in parts else None
        b = s.put("boxes", boxes) if "b" in parts else None
        p = s.put("points", points) if "p" in parts else None
        c = s.put("colors", col)
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731

        def fn():
            _lib.check(_lib.lib().tce_vis_overlay_u8(raw_f.data_ptr() + shift_in, raw_o.data_ptr() + shift_out, ptr(m), ptr(b), ptr(p),
                                                     c.data_ptr(), L, N, H, W, torch.cuda.current_stream().cuda_stream), "tce_vis_overlay_u8")
        fn.check = lambda: raw_o[shift_out:shift_out + total]
        return fn

    info = fp.check_case(slab, build, fp.recorder("tce_vis_overlay_u8"), props="WOR", sync=torch.cuda.synchronize,
                         label=f"tce_vis_overlay_u8 {parts}")
    assert (info["W"], info["O"], info["R"]) == (2, 2, 3)
    assert info["written_bytes"] == total
    assert info["read_bytes"] == total + L * 3 + ("m" in parts) * L * N * H * W + ("b" in parts) * L * N * 16 + ("p" in parts) * L * N * 8
    slab.begin(0)
    fn = build(slab)
    fn()
    torch.cuda.synchronize()
    want = V.overlay(frames, col, masks if "m" in parts else None, boxes if "b" in parts else None, points if "p" in parts else None)
    assert np.array_equal(fn.check().cpu().numpy().reshape(N, H, W, 3), want)


def test_hazard_recording_lists_the_one_entry(golden):
    from tce_rvos_amd import ops
    g = {k[2:]: v for k, v in golden.items() if k.startswith("s_")}
    f, c, b = _cuda(g["frames"]), _cuda(g["b_colors"]), _cuda(g["b_boxes"])
    with hazard.recording() as rec:
        got = ops.vis_overlay(f, c, boxes=b)
    torch.cuda.synchronize()
    assert [x.name for x in rec.launches] == ["tce_vis_overlay_u8"] and rec.analyse().clean
    assert np.array_equal(got.cpu().numpy(), g["b_out"])
