"""PNG files of one chunk of output masks: png.encode (the zlib streams made on the GPU, two small read-backs, host framing) against
the path a caller has without it, on the same GPU in the same process.

  A  existing   masks.cpu(), then per mask the reference's own lines (inference_ytvos.py:354-363) saved to memory:
                Image.fromarray(mask.astype(float32) * 255).convert('L').save(buffer, 'PNG')  -- Pillow's zlib at its default level
  B  png.encode png.mask_pngs(masks, rows_per_strip=S) for S = 1, 8, 32: three launches, the byte counts, the used bytes, the framing
  shapes        720 x 1280 and 480 x 854, one chunk of 32 planes of blob-like masks (an ellipse with a wavy edge per plane)
  wall          host time from the device tensor to the list of finished files, device idle before and after, per mask
  device        device-event time of ops.png_deflate alone (the three launches), per mask
  bytes         the mean file size of each path
  Interleaved rounds in one process; one JSON line per measurement, to stdout and to --out (default profiles/r14_png.txt).

  python tools/png_bench.py [--reps N] [--reps-a N] [--rounds R] [--out PATH]"""
import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tce_rvos_amd import ops, png  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--reps-a", type=int, default=2)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_png.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("png_bench: needs the GPU (a time taken elsewhere says nothing)")

P, STRIPS = 32, (1, 8, 32)
lines = []


def emit(obj):
    lines.append(json.dumps(obj))
    print(lines[-1], flush=True)


def blob_masks(P, H, W, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    out = np.zeros((P, H, W), np.uint8)
    for p in range(P):
        cy, cx = rng.uniform(0.3, 0.7) * H, rng.uniform(0.3, 0.7) * W
        ry, rx = rng.uniform(0.1, 0.3) * H, rng.uniform(0.1, 0.3) * W
        ang = np.arctan2(y - cy, x - cx)
        edge = 1.0 + 0.08 * np.sin(rng.integers(3, 9) * ang + rng.uniform(0, 6)) + 0.03 * np.sin(rng.integers(15, 40) * ang)
        out[p] = (((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 < edge ** 2).astype(np.uint8)
    return out


def path_a(masks):
    host = masks.cpu().numpy()
    files = []
    for m in host:
        buf = io.BytesIO()
        Image.fromarray(m.astype(np.float32) * 255).convert("L").save(buf, format="PNG")
        files.append(buf.getvalue())
    return files


def wall_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def device_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


emit({"measure": "setup", "device": torch.cuda.get_device_name(0), "planes_per_chunk": P, "reps_b": args.reps, "reps_a": args.reps_a,
      "rounds": args.rounds, "kernel_times_from_a_profiler": "none taken"})
for H, W in ((720, 1280), (480, 854)):
    host = blob_masks(P, H, W, H)
    masks = torch.from_numpy(host).cuda()
    shape = f"{P} x {H} x {W}"
    # agreement first: every file of both paths decodes to the same pixels
    files = {"A": path_a(masks)}
    for S in STRIPS:
        files[f"B{S}"] = png.mask_pngs(masks, rows_per_strip=S)
    for key, fs in files.items():
        for m, f in zip(host, fs):
            im = Image.open(io.BytesIO(f))
            assert im.mode == "L" and np.array_equal(np.asarray(im), m * 255), key
    emit({"measure": "bytes_per_file", "shape": shape, "foreground_share": round(float(host.mean()), 4),
          **{key: round(sum(len(f) for f in fs) / P) for key, fs in files.items()},
          "plane_bytes": H * W, "B8_over_A": round(sum(len(f) for f in files["B8"]) / sum(len(f) for f in files["A"]), 2)})
    for _ in range(3):                                    # warm-up: code objects, the allocator's blocks
        for S in STRIPS:
            png.mask_pngs(masks, rows_per_strip=S)
    wall = {"A": []}
    wall.update({f"B{S}": [] for S in STRIPS})
    dev = {f"B{S}": [] for S in STRIPS}
    for _ in range(args.rounds):                          # interleaved
        wall["A"].append(round(wall_ms(lambda: path_a(masks), args.reps_a) / P, 4))
        for S in STRIPS:
            wall[f"B{S}"].append(round(wall_ms(lambda: png.mask_pngs(masks, rows_per_strip=S), args.reps) / P, 4))
            dev[f"B{S}"].append(round(device_ms(lambda: ops.png_deflate(masks, rows_per_strip=S, nonzero_value=255), args.reps) / P, 5))
    emit({"measure": "wall_ms_per_mask", "shape": shape, **wall,
          "A_over_B8": round(min(wall["A"]) / min(wall["B8"]), 2), "B8_faster": max(wall["B8"]) < min(wall["A"])})
    emit({"measure": "device_event_ms_per_mask (ops.png_deflate alone, allocations included)", "shape": shape, **dev})
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
