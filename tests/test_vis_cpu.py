"""CPU: the overlay rule's numpy restatement (tests/_vis.py) against Pillow on the fixture's cases and on random regular boxes and
points; thin boxes against the stated rule; the RGB framing of png.py (frame_rgb) round trip; the filter restatement's choices;
the stage's header against its binding table, the built library and its access models."""
import io
import os
import zlib

import numpy as np
import pytest

import _png_rgb as G
import _vis as V

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "vis_overlay_cases.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(FIXTURE))


@pytest.mark.parametrize("tag", ["s", "m"])
def test_restatement_equals_the_fixture(golden, tag):
    g = {k[2:]: v for k, v in golden.items() if k.startswith(tag + "_")}
    f = g["frames"]
    assert f.shape in ((3, 37, 53, 3), (3, 48, 64, 3))
    assert np.array_equal(V.overlay(f, g["a_colors"], g["a_masks"], g["a_boxes"], g["a_points"]), g["a_out"])
    assert np.array_equal(V.overlay(f, g["b_colors"], None, g["b_boxes"], None), g["b_out"])
    assert np.array_equal(V.overlay(f, g["a_colors"], g["c_masks"], None, g["c_points"]), g["c_out"])
    assert np.array_equal(V.overlay(f, g["a_colors"], None, None, g["d_points"]), g["d_out"])
    for k in ("a_out", "b_out", "c_out", "d_out"):
        assert not np.array_equal(g[k], f), k                      # something was drawn
    for b in list(g["a_boxes"].reshape(-1, 4)) + list(g["b_boxes"].reshape(-1, 4)):
        assert V.is_regular(b, f.shape[1], f.shape[2])


def test_fixture_is_what_pillow_renders(golden):
    pytest.importorskip("PIL")
    g = {k[2:]: v for k, v in golden.items() if k.startswith("s_")}
    assert np.array_equal(V.pillow_overlay(g["frames"], g["a_colors"], g["a_masks"], g["a_boxes"], g["a_points"]), g["a_out"])
    assert np.array_equal(V.pillow_overlay(g["frames"], g["b_colors"], None, g["b_boxes"], None), g["b_out"])


def test_restatement_equals_pillow_on_random_regular_cases():
    pytest.importorskip("PIL")
    rng = np.random.default_rng(7)
    for H, W in ((37, 53), (48, 64), (9, 11)):
        n = 100
        frames = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
        boxes = V.regular_boxes(rng, n, H, W)[None]
        points = rng.uniform(-0.1, 1.1, (1, n, 2)).astype(np.float32)
        points[0, :8] = [[0, 0], [1, 1], [0, 1], [1, 0], [0.5, 0], [0, 0.5], [1, 0.5], [0.5, 1]]
        masks = (rng.random((1, n, H, W)) < 0.5).astype(np.uint8)
        col = rng.integers(0, 256, (1, 3), dtype=np.uint8)
        want = V.pillow_overlay(frames, col, masks, boxes, points)
        got = V.overlay(frames, col, masks, boxes, points)
        bad = [k for k in range(n) if not np.array_equal(got[k], want[k])]
        assert not bad, (H, W, bad[:5], boxes[0, bad[0]], points[0, bad[0]])


def test_thin_and_degenerate_boxes_follow_the_stated_rule():
    H, W = 20, 30
    frames = np.zeros((1, H, W, 3), np.uint8)
    col = np.array([[9, 8, 7]], np.uint8)

    def drawn(x0, y0, x1, y1):
        b = np.array([[[(x0 + x1) / 2 / W, (y0 + y1) / 2 / H, (x1 - x0) / W, (y1 - y0) / H]]], np.float32)
        assert not V.is_regular(b[0, 0], H, W) or (x1 - x0 >= 2 and y1 - y0 >= 2)
        return V.box_corners(b[0, 0], H, W), (V.overlay(frames, col, None, b, None)[0] == col[0]).all(-1)

    (X0, Y0, X1, Y1), m = drawn(5.25, 4.25, 6.75, 12.75)           # one pixel wide in x: filled
    assert (X0, Y0, X1, Y1) == (5, 4, 6, 12) and m.sum() == 2 * 9 and m[4:13, 5:7].all()
    (X0, Y0, X1, Y1), m = drawn(5.25, 4.25, 5.75, 4.75)            # a single pixel
    assert (X0, Y0, X1, Y1) == (5, 4, 5, 4) and m.sum() == 1 and m[4, 5]
    _, m = drawn(8.5, 4.5, 3.5, 9.5)                               # negative width: nothing
    assert m.sum() == 0
    _, m = drawn(-4.5, 3.5, -3.75, 9.5)                            # thin and outside: nothing
    assert m.sum() == 0
    (X0, Y0, X1, Y1), m = drawn(-0.75, 2.25, 0.75, 9.25)           # truncation toward zero: -0.75 -> 0, thin, column 0
    assert (X0, X1) == (0, 0) and m.sum() == 8 and m[2:10, 0].all()
    (X0, Y0, X1, Y1), m = drawn(3.25, 3.25, 5.75, 5.75)            # the smallest regular box: all nine pixels are within 2 of a side
    assert (X0, Y0, X1, Y1) == (3, 3, 5, 5) and m.sum() == 9
    (X0, Y0, X1, Y1), m = drawn(3.25, 3.25, 9.75, 9.75)            # a ring two pixels wide
    assert m.sum() == 49 - 9 and not m[5:8, 5:8].any()


def test_rgb_framing_round_trips():
    from tce_rvos_amd import png
    rng = np.random.default_rng(3)
    for H, W in ((1, 1), (5, 7), (12, 9)):
        img = G.images(H, W, H)[1]
        rows = G.filtered_rows(img)
        blob = png.frame_rgb(zlib.compress(rows.tobytes()), W, H)
        assert np.array_equal(G.decode_file(blob), img)
        stream, _ = G.rows_stream(rows, 4)
        blob2 = png.frame_rgb(stream, W, H)
        assert zlib.decompress(stream) == rows.tobytes() and np.array_equal(G.decode_file(blob2), img)
        try:
            from PIL import Image
        except ImportError:
            continue
        for b in (blob, blob2):
            im = Image.open(io.BytesIO(b))
            assert im.mode == "RGB" and im.size == (W, H) and np.array_equal(np.asarray(im), img)
    with pytest.raises(ValueError):
        png.frame_rgb(b"", 0, 2)
    with pytest.raises(ValueError):
        png.frame(b"", 3, 2, "RGB")                                  # frame keeps to 'L' and 'P'
    assert blob[8:33] == png.chunk(b"IHDR", bytes([0, 0, 0, 9, 0, 0, 0, 12, 8, 2, 0, 0, 0]))   # 9 x 12, depth 8, colour type 2


def test_filter_restatement_choices():
    zero = np.zeros((4, 6, 3), np.uint8)
    assert (G.filtered_rows(zero) == 0).all()                       # every type costs 0: the lowest wins
    x = np.arange(40, dtype=np.uint8)
    ramp = np.stack([5 * x, 5 * x + 1, 5 * x + 2], -1)[None].repeat(3, 0)   # a horizontal ramp: Sub leaves fives, Up zeros below
    rows = G.filtered_rows(ramp)
    assert rows[0, 0] == 1 and (rows[1:, 0] == 2).all() and (rows[1:, 1:] == 0).all()
    assert (rows[0, 4:] == 5).all() and rows[0, 1:4].tolist() == [0, 1, 2]
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (6, 5, 3), dtype=np.uint8)
    assert np.array_equal(G.unfilter(G.filtered_rows(img), 5), img)
    for t in range(5):                                               # each filter inverts, whatever the choice
        up, cur = bytes(img[2].reshape(-1)), bytes(img[3].reshape(-1))
        rows = np.zeros((2, 16), np.uint8)
        rows[0, 1:] = np.frombuffer(up, np.uint8)
        rows[1, 0], rows[1, 1:] = t, np.frombuffer(G.filter_row(t, cur, up), np.uint8)
        assert np.array_equal(G.unfilter(rows, 5)[1], img[3])


def test_vis_ops_reject_what_is_not_on_the_gpu():
    import torch
    from tce_rvos_amd import ops, vis
    f = torch.zeros(1, 4, 5, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="vis_overlay"):
        ops.vis_overlay(f, torch.zeros(1, 3, dtype=torch.uint8))     # on the CPU: no fall-back
    with pytest.raises(ValueError, match="png_filter_rgb"):
        ops.png_filter_rgb(f)
    with pytest.raises(ValueError, match="png_deflate_rows"):
        ops.png_deflate_rows(torch.zeros(1, 4, 16, dtype=torch.uint8))
    with pytest.raises(ValueError):
        vis.overlay_objects(f, torch.zeros(2, 4), [[1, 2, 3]])

