"""Host restatement of the overlay rule of tce_vis_overlay_u8 (include/tce_rvos_vis.h) in numpy, and the same layers rendered
with Pillow the way the reference's --visualize block draws them (ImageDraw.rectangle(width=2), two ImageDraw.line(width=4), the
numpy blend).  Written from the rule's text; it shares nothing with the kernel or with tce_rvos_amd/vis.py."""
import numpy as np

LIM = float(2 ** 30)


def box_corners(box, H0, W0):
    """(X0, Y0, X1, Y1): fp32 arithmetic, one rounding per operation, truncated toward zero"""
    f = np.float32
    cx, cy, w, h = (f(v) for v in box)
    hw, hh = f(0.5) * w, f(0.5) * h
    vals = [(cx - hw) * f(W0), (cy - hh) * f(H0), (cx + hw) * f(W0), (cy + hh) * f(H0)]
    assert all(v.dtype == np.float32 for v in vals)
    return tuple(int(np.trunc(np.clip(v, -LIM, LIM))) for v in vals)


def is_regular(box, H0, W0):
    X0, Y0, X1, Y1 = box_corners(box, H0, W0)
    return X1 - X0 >= 2 and Y1 - Y0 >= 2


def box_pixels(box, H0, W0):
    """bool [H0,W0]: the pixels a layer's box sets"""
    X0, Y0, X1, Y1 = box_corners(box, H0, W0)
    y, x = np.mgrid[0:H0, 0:W0]
    inside = (x >= X0) & (x <= X1) & (y >= Y0) & (y <= Y1)
    if X1 - X0 >= 2 and Y1 - Y0 >= 2:
        return inside & ((x - X0 < 2) | (X1 - x < 2) | (y - Y0 < 2) | (Y1 - y < 2))
    return inside  # a thin box: filled; empty when X1 < X0 or Y1 < Y0


def point_pixels(pt, H0, W0):
    """bool [H0,W0]: the cross of a layer's reference point (double arithmetic)"""
    x, y = W0 * float(np.float32(pt[0])), H0 * float(np.float32(pt[1]))
    t = lambda v: int(np.trunc(v))
    yy, xx = np.mgrid[0:H0, 0:W0]
    bar_h = (yy >= t(y) - 1) & (yy <= t(y) + 2) & (xx >= t(x - 10)) & (xx <= t(x + 10))
    bar_v = (xx >= t(x) - 1) & (xx <= t(x) + 2) & (yy >= t(y - 10)) & (yy <= t(y + 10))
    return bar_h | bar_v


def overlay(frames, colors, masks=None, boxes=None, points=None):
    """frames uint8 [N,H0,W0,3]; per layer: masks [L,N,H0,W0], boxes [L,N,4], points [L,N,2], colors [L,3] -> uint8 [N,H0,W0,3]"""
    out = np.array(frames, dtype=np.uint8, copy=True)
    N, H0, W0, _ = out.shape
    for l, c in enumerate(np.asarray(colors, dtype=np.uint8)):
        for n in range(N):
            if boxes is not None:
                out[n][box_pixels(boxes[l][n], H0, W0)] = c
            if points is not None:
                out[n][point_pixels(points[l][n], H0, W0)] = c
            if masks is not None:
                m = np.asarray(masks[l][n]) != 0
                out[n][m] = ((out[n][m].astype(np.int32) + c.astype(np.int32)) >> 1).astype(np.uint8)
    return out


def pillow_overlay(frames, colors, masks=None, boxes=None, points=None):
    """The same layers through Pillow, per frame and layer in the reference's order: an RGBA image of the frame, the rectangle of the
    rescaled box (a CPU float32 tensor's arithmetic, its values as Python floats), the two lines, then the blend
    image * 0.5 + colour * 0.5 stored into a uint8 array where the mask is set."""
    import torch
    from PIL import Image, ImageDraw
    out = np.array(frames, dtype=np.uint8, copy=True)
    N, H0, W0, _ = out.shape
    for l, c in enumerate(np.asarray(colors, dtype=np.uint8)):
        col = tuple(int(v) for v in c)
        for n in range(N):
            img = Image.fromarray(out[n]).convert("RGBA")
            draw = ImageDraw.Draw(img)
            if boxes is not None:
                b = torch.as_tensor(np.asarray(boxes[l][n], dtype=np.float32))[None]
                xc, yc, w, h = b.unbind(1)
                xyxy = torch.stack([xc - 0.5 * w, yc - 0.5 * h, xc + 0.5 * w, yc + 0.5 * h], 1)
                x0, y0, x1, y1 = (xyxy * torch.tensor([W0, H0, W0, H0], dtype=torch.float32)).tolist()[0]
                draw.rectangle(((x0, y0), (x1, y1)), outline=col, width=2)
            if points is not None:
                px, py = torch.as_tensor(np.asarray(points[l][n], dtype=np.float32)).tolist()
                x, y = W0 * px, H0 * py
                draw.line((x - 10, y, x + 10, y), col, width=4)
                draw.line((x, y - 10, x, y + 10), col, width=4)
            rgb = np.asarray(img.convert("RGB")).copy()
            if masks is not None:
                m = np.asarray(masks[l][n]).astype("uint8") != 0
                rgb[m] = rgb[m] * 0.5 + np.array(col) * 0.5
            out[n] = rgb
    return out


# ------------------------------------------------------------------------------------------------------------------ cases
def blob(H, W, cy, cx, ry, rx):
    y, x = np.mgrid[0:H, 0:W]
    return ((((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2) <= 1.0).astype(np.uint8)


def regular_boxes(rng, count, H0, W0):
    """random cx, cy, w, h whose integer extents are at least 2 both ways: partly or wholly outside the image and with negative
    corners included"""
    out = []
    while len(out) < count:
        x0, x1 = np.sort(rng.uniform(-0.6, 1.6, 2))
        y0, y1 = np.sort(rng.uniform(-0.6, 1.6, 2))
        b = np.array([(x0 + x1) / 2, (y0 + y1) / 2, x1 - x0, y1 - y0], dtype=np.float32)
        if is_regular(b, H0, W0):
            out.append(b)
    return np.stack(out)
