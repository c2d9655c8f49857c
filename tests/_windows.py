"""The reference's context-frame window loop (inference_ytvos.py:194-277, inference_mevis.py:196-214) restated as plain loops, and
its per-window output stage on the CPU with torch.  What tce_rvos_amd.video.plan_windows and ops.select_window_masks are held to."""
import torch
import torch.nn.functional as F


def reference_windows(N, n, e, last="short"):
    """Per video frame the (window number, clip position, clip ids) of its FIRST stored entry: the driver keeps a list of masks per
    frame, every window appends the masks of its clip positions 0 .. m-1 to frames start .. start+m-1, and the frame's mask is
    entry [0] of its list."""
    stored = {}
    number = 0
    for begin in range(0, N, n):
        start = begin
        if last == "shifted":
            if start + n > N:
                start = N - n
            end = start + n
        else:
            end = min(start + n, N)
        if start < 0:
            raise ValueError("the reference indexes frames[-k] here")
        ids = list(range(start, end))
        for _ in range(e):
            head, tail = ids[0], ids[-1]
            ids = [max(0, head - 1)] + ids
            ids = ids + [min(N - 1, tail + 1)]
        kept = len(ids) - 2 * e
        for pos in range(kept):
            stored.setdefault(pos + start, []).append((number, pos, tuple(ids)))
        number += 1
    return [stored[f][0] for f in range(N)]


def reference_window_masks(logits, masks, size, first, count, thr):
    """logits [T,Q,K], masks [T,Q,h,w] (CPU float32) -> (up-sampled logits [count,H0,W0] of the best query's planes at clip positions
    first .. first+count-1, the 0/1 masks sigmoid(.) > thr, the best query): mean over ALL T frames, max over classes, arg-max."""
    score = logits.sigmoid().mean(0).max(-1)[0]
    best = int(score.argmax())
    planes = masks[first:first + count, best][None]
    up = F.interpolate(planes, size=tuple(size), mode="bilinear", align_corners=False)[0]
    return up, (up.sigmoid() > thr).to(torch.uint8), best
