"""Ref-DAVIS J&F of one chunk: score.score_video on label maps that are already on the GPU, against the reference's scoring
arithmetic (davis2017/metrics.py) run two ways on the same maps.

  shape       32 frames of 480 x 854 with three objects (radius 8): synthetic discs, the prediction a jittered copy of the ground
              truth (tests/_jf.py's "sparse" maker), so boundaries are a fraction of a percent of a frame, as in real maps.
  ours        score_video: tce_jf_counts_i32 (two launches), one read-back of [3,32,6] counts, J / F / statistics on the host.
  numpy       the device-to-host copy of both stacks, then the NumPy restatement of db_eval_iou / _seg2bmap / f_measure per
              (object, frame) (tests/_jf.py: the dilation is the OR of 197 shifted copies where the reference calls cv2.dilate; cv2
              and skimage are absent here), then the same J / F arithmetic.
  torch       the reference's arithmetic kept on the GPU with PyTorch: boundary maps by shifted slices, the dilation as
              torch.nn.functional.conv2d with the disk as kernel, sums, one read-back.  Skipped with a note if conv2d refuses.
  device      device-event time of the GPU work alone (ours, torch).     wall: maps on the device -> J and F on the host, device
              idle before and after.  Interleaved rounds in one process; one JSON line per measurement.

  python tools/davis_score_bench.py [--reps N] [--rounds R]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _jf  # noqa: E402
from tce_rvos_amd import ops, score  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("davis_score_bench: needs the GPU (a time taken elsewhere says nothing)")

T, n, H, W = 32, 3, 480, 854
radius = score.boundary_radius(H, W)
pred_h, gt_h = _jf.make_case(("bench", 90, T, n, H, W, radius, "sparse"))
pred, gt = torch.from_numpy(pred_h).cuda(), torch.from_numpy(gt_h).cuda()


def ours_device():
    return ops.jf_counts(pred, gt, n, radius)


def ours_full():
    r = score.score_video(pred, gt, n=n, drop_first_last=False)
    return r["counts"], r["J"], r["F"]


def numpy_full():
    p, g = pred.cpu().numpy(), gt.cpu().numpy()
    return _jf.reference(p, g, n, radius)


def _bmap(s):
    """_seg2bmap at equal size on a bool stack [T,H,W]"""
    e, so, se = torch.zeros_like(s), torch.zeros_like(s), torch.zeros_like(s)
    e[:, :, :-1] = s[:, :, 1:]
    so[:, :-1, :] = s[:, 1:, :]
    se[:, :-1, :-1] = s[:, 1:, 1:]
    b = (s ^ e) | (s ^ so) | (s ^ se)
    b[:, -1, :] = s[:, -1, :] ^ e[:, -1, :]
    b[:, :, -1] = s[:, :, -1] ^ so[:, :, -1]
    b[:, -1, -1] = False
    return b


DISK = torch.from_numpy(_jf.disk(radius)).float().cuda()[None, None]


def torch_device():
    out = []
    for k in range(n):
        seg, ann = pred == k + 1, gt == k + 1
        bs, ba = _bmap(seg), _bmap(ann)
        ds = F.conv2d(bs[:, None].float(), DISK, padding=radius)[:, 0] > 0.5
        da = F.conv2d(ba[:, None].float(), DISK, padding=radius)[:, 0] > 0.5
        out.append(torch.stack([(seg & ann).sum((1, 2)), (seg | ann).sum((1, 2)), bs.sum((1, 2)), ba.sum((1, 2)),
                                (bs & da).sum((1, 2)), (ba & ds).sum((1, 2))], 1))
    return torch.stack(out)


def torch_full():
    c = torch_device().cpu().numpy()
    return (c,) + score.jf_from_counts(c)


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


torch_note = None
try:
    for _ in range(2):
        torch_full()
    torch.cuda.synchronize()
except Exception as e:  # noqa: BLE001  (a library that refuses the 17 x 17 kernel is a finding, not a failure of this tool)
    torch_note = f"not measured: {type(e).__name__}: {str(e)[:120]}"
for _ in range(3):  # warm-up: code objects, the allocator's blocks
    ours_full()
torch.cuda.synchronize()

c_ours, j_ours, f_ours = ours_full()
c_np, j_np, f_np = numpy_full()
same = bool(np.array_equal(c_ours, c_np))
same_jf = bool(np.array_equal(j_ours.view(np.uint64), j_np.view(np.uint64)) and np.array_equal(f_ours.view(np.uint64), f_np.view(np.uint64)))
same_torch = None if torch_note else bool(np.array_equal(torch_full()[0], c_np))
tiles = -(-H // 32) * -(-W // 64)
res = score.score_video(pred, gt, n=n, drop_first_last=False)
print(f"# python tools/davis_score_bench.py   (MI355X, one process, interleaved rounds, {args.rounds} rounds; ours and torch {args.reps} calls per figure, numpy 1)")
print(f"# one chunk: T={T} frames {H}x{W}, n={n} objects, disk radius {radius} ({int(_jf.disk(radius).sum())} taps); synthetic discs, boundary pixels "
      f"{100.0 * c_np[..., 2:4].sum() / (2 * n * T * H * W):.2f} % of a plane")
print("# ours   = score.score_video on device-resident maps: tce_jf_counts_i32 (2 launches), one read-back of the counts, J / F on the host")
print("# numpy  = .cpu() of both stacks + the NumPy restatement of metrics.py per (object, frame) (OR of shifted copies for cv2.dilate)")
print("# torch  = the reference's arithmetic on the same GPU: shifted slices, torch.nn.functional.conv2d with the disk, sums, one read-back")
print("# device: device-event time over the GPU work alone; wall: maps on the device -> J and F on the host, device idle before and after")
print(json.dumps({"measure": "agreement", "counts equal": "yes" if same else "no", "J and F bit-equal": "yes" if same_jf else "no",
                  "torch counts equal": torch_note or ("yes" if same_torch else "no"),
                  "J&F-Mean": round(score.summarize([res])["J&F-Mean"], 5),
                  "device_bytes_read_ours_at_least": 2 * T * H * W, "ws_bytes_written_and_read": n * T * tiles * 24,
                  "bytes_read_back_ours": n * T * 24, "bytes_copied_to_host_numpy": 2 * T * H * W,
                  "device_bytes_moved_torch_at_least": n * 2 * T * H * W * (1 + 4 + 4 + 1)}), flush=True)
dev = {"ours": [], "torch": []}
wall = {"ours": [], "numpy": [], "torch": []}
for _ in range(args.rounds):  # interleaved
    dev["ours"].append(round(device_ms(ours_device, args.reps), 4))
    wall["ours"].append(round(wall_ms(ours_full, args.reps), 4))
    wall["numpy"].append(round(wall_ms(numpy_full, 1), 1))
    if not torch_note:
        dev["torch"].append(round(device_ms(torch_device, args.reps), 4))
        wall["torch"].append(round(wall_ms(torch_full, args.reps), 4))
line = {"measure": "device", "reps": args.reps, "ms_per_chunk": dev}
if not torch_note:
    line["torch_over_ours"] = round(min(dev["torch"]) / min(dev["ours"]), 1)
print(json.dumps(line), flush=True)
line = {"measure": "wall", "reps": {"ours": args.reps, "torch": args.reps, "numpy": 1}, "ms_per_chunk": wall,
        "numpy_over_ours": round(min(wall["numpy"]) / min(wall["ours"]), 1), "ours_faster_than_numpy": max(wall["ours"]) < min(wall["numpy"]),
        "numpy_ms_per_frame_object": round(min(wall["numpy"]) / (n * T), 2)}
if not torch_note:
    line["torch_over_ours"] = round(min(wall["torch"]) / min(wall["ours"]), 1)
    line["ours_faster_than_torch"] = max(wall["ours"]) < min(wall["torch"])
print(json.dumps(line), flush=True)
