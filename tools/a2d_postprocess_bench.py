"""A2D-Sentences / JHMDB-Sentences post-processor: postprocess.A2DSentencesPostProcess against the reference class's own sequence
of PyTorch operations on the same GPU (postprocessors.py:38-49: F.interpolate bilinear x4 -> sigmoid -> > 0.5 -> crop -> float ->
F.interpolate nearest -> .cpu() -> a Fortran-order numpy copy per query), followed by a vectorised numpy run-length pass where the
reference calls pycocotools' C encoder (absent here; both sides pack their run lengths with the same rle_to_string).

  shape       N = 5 queries, masks 80 x 120, size (320, 475), orig (240, 320): an A2D frame at the reference's 320-pixel evaluation
              size; smooth synthetic logits (a coarse random grid up-sampled: a few hundred runs per mask, like real masks).
  device      device-event time of the GPU work alone (ours: sigmoid + masks + run lengths; reference: its torch operations).
  wall        host time from the outputs to the finished Python result (scores, masks, rle_masks), device idle before and after.
  Interleaved A/B rounds in one process; one JSON line per measurement.

  python tools/a2d_postprocess_bench.py [--reps N] [--rounds R]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tce_rvos_amd import ops  # noqa: E402
from tce_rvos_amd.postprocess import A2DSentencesPostProcess, rle_to_string  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("a2d_postprocess_bench: needs the GPU (a time taken elsewhere says nothing)")

N, h, w, size, orig = 5, 80, 120, (320, 475), (240, 320)
g = torch.Generator().manual_seed(60)
logits = torch.randn(1, 1, N, 1, generator=g).cuda()
masks = (F.interpolate(torch.randn(N, 1, 5, 7, generator=g), size=(h, w), mode="bicubic", align_corners=True)[:, 0] * 8).view(1, 1, N, h, w).cuda()
outputs = {"pred_logits": logits, "pred_masks": masks}
orig_t, size_t = torch.tensor([orig]).cuda(), torch.tensor([size]).cuda()
post = A2DSentencesPostProcess()


def ours_device():
    ops.sigmoid(logits[0, 0, :, 0].contiguous())
    return ops.rle_counts(ops.a2d_masks(masks[0, 0], size, orig))


def reference_device():
    """postprocessors.py:34-47 for the one sample"""
    out_logits = outputs["pred_logits"][:, 0, :, 0]
    out_masks = outputs["pred_masks"][:, 0, :, :, :]
    out_h, out_w = out_masks.shape[-2:]
    scores = out_logits.sigmoid()
    pred_masks = F.interpolate(out_masks, size=(out_h * 4, out_w * 4), mode="bilinear", align_corners=False)
    pred_masks = (pred_masks.sigmoid() > 0.5)
    f_pred_masks_no_pad = pred_masks[0][:, :size[0], :size[1]].unsqueeze(1)
    return scores, F.interpolate(f_pred_masks_no_pad.float(), size=orig, mode="nearest")


def numpy_rle(fortran_mask):
    """run lengths of one Fortran-order [H,W,1] uint8 mask, vectorised (stands where mask_util.encode stands)"""
    flat = fortran_mask.reshape(-1, order="F")
    q = np.flatnonzero(np.diff(flat, prepend=np.uint8(0)))
    counts = np.diff(np.concatenate([[0], q, [flat.size]])) if q.size else np.asarray([flat.size])
    return {"size": [int(fortran_mask.shape[0]), int(fortran_mask.shape[1])], "counts": rle_to_string(counts)}


def reference_full():
    scores, processed = reference_device()
    rle = [numpy_rle(np.array(mask[0, :, :, np.newaxis], dtype=np.uint8, order="F")) for mask in processed.cpu()]  # :48-49
    return [{"scores": scores[0], "masks": processed, "rle_masks": rle}]


def ours_full():
    return post(outputs, orig_t, size_t)


def device_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def wall_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


for fn in (ours_device, reference_device, ours_full, reference_full):  # warm-up: code objects, the allocator's blocks
    for _ in range(5):
        fn()
torch.cuda.synchronize()
a, b = ours_full()[0], reference_full()[0]
differ = float((a["masks"] != b["masks"].to(torch.uint8)).float().mean())
same = sum(x["counts"] == y["counts"] for x, y in zip(a["rle_masks"], b["rle_masks"]))
runs = [len(x["counts"]) for x in a["rle_masks"]]
moved_ours = N * h * w * 4 + 2 * N * orig[0] * orig[1] + N * (orig[0] * orig[1] + 1) * 4
moved_ref = N * h * w * 4 + N * 16 * h * w * (4 + 4 + 1 + 1) + N * size[0] * size[1] * (1 + 4) + 3 * N * orig[0] * orig[1] * 4
print(json.dumps({"measure": "agreement", "shape": f"N={N} {h}x{w} size={size} orig={orig}", "masks_differ_share": differ,
                  "rle_strings_equal": f"{same}/{N}", "string_bytes_per_mask": runs,
                  "device_bytes_moved_ours": moved_ours, "device_bytes_moved_reference_at_least": moved_ref}), flush=True)
dev = {"ours": [], "reference": []}
wall = {"ours": [], "reference": []}
for _ in range(args.rounds):  # interleaved A/B
    dev["ours"].append(round(device_ms(ours_device, args.reps), 4))
    dev["reference"].append(round(device_ms(reference_device, args.reps), 4))
    wall["ours"].append(round(wall_ms(ours_full, args.reps), 4))
    wall["reference"].append(round(wall_ms(reference_full, args.reps), 4))
print(json.dumps({"measure": "device", "reps": args.reps, "ms_per_call": dev,
                  "reference_over_ours": round(min(dev["reference"]) / min(dev["ours"]), 2)}), flush=True)
print(json.dumps({"measure": "wall", "reps": args.reps, "ms_per_call": wall,
                  "reference_over_ours": round(min(wall["reference"]) / min(wall["ours"]), 2),
                  "ours_faster": max(wall["ours"]) < min(wall["reference"])}), flush=True)
