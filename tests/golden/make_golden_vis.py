"""Writes tests/golden/vis_overlay_cases.npz: inputs of the overlay stage and what Pillow renders for them (tests/_vis.py,
pillow_overlay: ImageDraw.rectangle(width=2), ImageDraw.line(width=4), the numpy blend -- made with Pillow 12.2.0).

    python tests/golden/make_golden_vis.py

Two frame sizes, 37 x 53 and 48 x 64, N = 3 frames each.  Per size: case A has L = 1 (mask + box + point), case B has L = 3 (boxes
only).  Every box is of the regular class (integer extents of at least 2 both ways; asserted here), so the fixture is Pillow-exact by
construction: boxes crossing every image border, wholly outside, and with negative corners.  Points lie in the interior, on every
border and in the corners.  Masks are empty, full, and blobs that cross the box ring and the cross."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _vis as V  # noqa: E402


def frames_of(rng, N, H, W):
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([(x * 255 // max(W - 1, 1)), (y * 255 // max(H - 1, 1)), ((x + y) * 255 // max(H + W - 2, 1))], -1)
    noise = rng.integers(-20, 21, (N, H, W, 3))
    return np.clip(base[None] + noise, 0, 255).astype(np.uint8)


def xyxy(H, W, x0, y0, x1, y1):
    """cx, cy, w, h of a box whose corners are about the given pixel coordinates"""
    return np.array([(x0 + x1) / 2 / W, (y0 + y1) / 2 / H, (x1 - x0) / W, (y1 - y0) / H], dtype=np.float32)


def cases(H, W, seed):
    rng = np.random.default_rng(seed)
    N = 3
    frames = frames_of(rng, N, H, W)
    # A: one layer, everything
    boxes_a = np.stack([xyxy(H, W, 5.5, 4.25, W - 7.5, H - 6.5),          # interior
                        xyxy(H, W, -6.5, -3.5, W * 0.6, H + 4.5),          # crosses the left, top and bottom borders, negative corners
                        xyxy(H, W, W * 0.5, H * 0.4, W + 9.0, H * 0.9)])[None]   # crosses the right border
    points_a = np.array([[[0.5, 0.5], [0.0, 0.0], [1.0, 1.0]]], dtype=np.float32)  # interior, two corners
    masks_a = np.stack([V.blob(H, W, H * 0.45, W * 0.5, H * 0.3, W * 0.42),  # crosses ring and cross
                        np.ones((H, W), np.uint8), np.zeros((H, W), np.uint8)])[None]
    col_a = np.array([[236, 95, 17]], dtype=np.uint8)
    # B: three layers of boxes
    boxes_b = np.stack([np.stack([xyxy(H, W, -30.0, -20.0, -4.0, -2.0),     # wholly outside, negative corners
                                  xyxy(H, W, 2.0, 3.0, 4.9, 5.9),            # the smallest regular box
                                  xyxy(H, W, -3.0, 6.0, W + 3.0, H - 4.0)]),  # crosses left and right
                        np.stack([xyxy(H, W, 8.0, -5.0, W - 9.0, H + 5.0),   # crosses top and bottom
                                  xyxy(H, W, W - 2.5, H - 2.5, W + 6.0, H + 6.0),  # the bottom-right corner
                                  xyxy(H, W, W + 2.0, 1.0, W + 20.0, H - 1.0)]),   # wholly outside on the right
                        V.regular_boxes(rng, 3, H, W)])
    col_b = np.array([[0, 114, 189], [217, 83, 25], [119, 172, 48]], dtype=np.uint8)
    # C: points on every border and in the other corners, with a blob over the cross
    points_c = np.array([[[0.5, 0.0], [0.0, 0.5], [1.0, 0.37]]], dtype=np.float32)
    points_d = np.array([[[0.41, 1.0], [1.0, 0.0], [0.0, 1.0]]], dtype=np.float32)
    masks_c = np.stack([V.blob(H, W, 2.0, W * 0.5, H * 0.2, W * 0.3), V.blob(H, W, H * 0.5, 1.0, H * 0.3, W * 0.2),
                        V.blob(H, W, H * 0.37, W - 2.0, H * 0.25, W * 0.25)])[None]
    for b in list(boxes_a.reshape(-1, 4)) + list(boxes_b.reshape(-1, 4)):
        assert V.is_regular(b, H, W), b
    out = {"frames": frames, "a_boxes": boxes_a, "a_points": points_a, "a_masks": masks_a, "a_colors": col_a,
           "b_boxes": boxes_b, "b_colors": col_b, "c_points": points_c, "c_masks": masks_c, "d_points": points_d}
    out["a_out"] = V.pillow_overlay(frames, col_a, masks_a, boxes_a, points_a)
    out["b_out"] = V.pillow_overlay(frames, col_b, None, boxes_b, None)
    out["c_out"] = V.pillow_overlay(frames, col_a, masks_c, None, points_c)
    out["d_out"] = V.pillow_overlay(frames, col_a, None, None, points_d)
    return out


if __name__ == "__main__":
    blob = {}
    for tag, (H, W) in (("s", (37, 53)), ("m", (48, 64))):
        for k, v in cases(H, W, 100 + H).items():
            blob[f"{tag}_{k}"] = v
    path = os.path.join(HERE, "vis_overlay_cases.npz")
    np.savez_compressed(path, **blob)
    print(path, os.path.getsize(path), "bytes")
