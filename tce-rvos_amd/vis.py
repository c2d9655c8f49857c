"""The --visualize images of the reference's drivers, drawn on the GPU: the decoded frame with the predicted box, the decoder's
reference point and the mask tint on it.

    inference_ytvos.py:325-351, inference_mevis.py (the same block)   -> overlay_expression(frames_u8, result, color)
    inference_davis.py:269-291                                        -> overlay_objects(frames_u8, boxes, colors)

One launch per call (ops.vis_overlay; include/tce_rvos_vis.h states the per-pixel rule, which is Pillow's
ImageDraw.rectangle(width=2) and ImageDraw.line(width=4) and the reference's numpy blend, byte for byte, except for boxes thinner
than 2 pixels, which are drawn as the filled rectangle of their integer corners).  png.rgb_pngs turns the result into files without
the pixels leaving the device.

The colours are the caller's: the reference takes them from its own table (`color_list` at the top of each inference script,
indexed by the expression's position modulo its length); that table is the reference's program text and is not repeated here.
"""
import torch

from . import ops


def _colors(colors, n, dev):
    c = torch.as_tensor(colors)
    if c.dtype != torch.uint8:
        if c.numel() and (int(c.min()) < 0 or int(c.max()) > 255):
            raise ValueError("vis: colours are R, G, B values in 0 .. 255")
        c = c.to(torch.uint8)
    c = c.reshape(-1, 3)
    if int(c.shape[0]) != n:
        raise ValueError(f"vis: {n} layers need {n} colours, got {int(c.shape[0])}")
    return c.to(dev).contiguous()


def overlay_expression(frames_u8, result, color, out=None):
    """The Ref-YouTube-VOS / MeViS image of ONE expression: frames_u8 uint8 [N,H0,W0,3] on the GPU (the decoded frames, e.g.
    infer.run_split's raw buffer), result a driver's dict (video.run_video(..., ref_points=True), run_video_expressions(...,
    ref_points=True) or run_video_windows) with masks uint8 [N,H0,W0], pred_boxes [N,4] and, if present, reference_points [N,2];
    color: one R, G, B triple.  Box outline, then the point's cross, then the mask tint, as the reference draws them.
    -> uint8 [N,H0,W0,3]."""
    dev = frames_u8.device
    masks = result.get("masks")
    boxes = result.get("pred_boxes")
    points = result.get("reference_points")
    return ops.vis_overlay(frames_u8, _colors(color, 1, dev),
                           masks=None if masks is None else masks.unsqueeze(0).contiguous(),
                           boxes=None if boxes is None else boxes.float().unsqueeze(0).contiguous(),
                           points=None if points is None else points.float().unsqueeze(0).contiguous(), out=out)


def overlay_objects(frames_u8, boxes, colors, out=None):
    """The Ref-DAVIS image of one annotator: frames_u8 uint8 [N,H0,W0,3] on the GPU, boxes float32 [L,N,4] (cx, cy, w, h normalised:
    run_video_objects(...)[i]["pred_boxes"]), colors [L,3]; one box outline per object, in order, 1 <= L <= 16.
    -> uint8 [N,H0,W0,3]."""
    if not torch.is_tensor(boxes) or boxes.dim() != 3:
        raise ValueError("overlay_objects: boxes must be [L,N,4]")
    return ops.vis_overlay(frames_u8, _colors(colors, int(boxes.shape[0]), frames_u8.device), boxes=boxes.float().contiguous(), out=out)
