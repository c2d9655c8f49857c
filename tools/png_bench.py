"""PNG files of one chunk of output masks: png.encode (the zlib streams made on the GPU, two small read-backs, host framing) against
the path a caller has without it, on the same GPU in the same process.

  A  existing   masks.cpu(), then per mask the reference's own lines (inference_ytvos.py:354-363) saved to memory:
                Image.fromarray(mask.astype(float32) * 255).convert('L').save(buffer, 'PNG')  -- Pillow's zlib at its default level
  F<S>          png.mask_pngs(masks, rows_per_strip=S, codes="fixed") for S = 8, 32: three launches, the byte counts, the used bytes,
                the framing
  D<S>          the same with codes="dynamic" for S = 16, 32, 64 (a Huffman code per strip where it is cheaper than the fixed one)
  shapes        720 x 1280 and 480 x 854, one chunk of 32 planes of blob-like masks (an ellipse with a wavy edge per plane)
  wall          host time from the device tensor to the list of finished files, device idle before and after, per mask
  device        device-event time of ops.png_deflate alone (the three launches), per mask
  bytes         the mean file size of each path
  default       the strip height for dynamic codes: the smallest files among the D<S> whose fastest round stays within the spread F8
                shows between its own rounds (max / min); if none does, the fastest D<S>
  Interleaved rounds in one process; one JSON line per measurement, to stdout and to --out (default profiles/r15_png_dyn.txt).

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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_png_dyn.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("png_bench: needs the GPU (a time taken elsewhere says nothing)")

P = 32
CONFIGS = (("F8", "fixed", 8), ("F32", "fixed", 32), ("D16", "dynamic", 16), ("D32", "dynamic", 32), ("D64", "dynamic", 64))
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
    # agreement first: every file of every path decodes to the same pixels
    files = {"A": path_a(masks)}
    for key, codes, S in CONFIGS:
        files[key] = png.mask_pngs(masks, rows_per_strip=S, codes=codes)
    for key, fs in files.items():
        for m, f in zip(host, fs):
            im = Image.open(io.BytesIO(f))
            assert im.mode == "L" and np.array_equal(np.asarray(im), m * 255), key
    size = {key: sum(len(f) for f in fs) / P for key, fs in files.items()}
    emit({"measure": "bytes_per_file", "shape": shape, "foreground_share": round(float(host.mean()), 4),
          **{key: round(b) for key, b in size.items()}, "plane_bytes": H * W,
          **{f"{key}_over_A": round(size[key] / size["A"], 2) for key, _, _ in CONFIGS}})
    for _ in range(3):                                    # warm-up: code objects, the allocator's blocks
        for key, codes, S in CONFIGS:
            png.mask_pngs(masks, rows_per_strip=S, codes=codes)
    wall = {"A": []}
    wall.update({key: [] for key, _, _ in CONFIGS})
    dev = {key: [] for key, _, _ in CONFIGS}
    for _ in range(args.rounds):                          # interleaved
        wall["A"].append(round(wall_ms(lambda: path_a(masks), args.reps_a) / P, 4))
        for key, codes, S in CONFIGS:
            wall[key].append(round(wall_ms(lambda: png.mask_pngs(masks, rows_per_strip=S, codes=codes), args.reps) / P, 4))
            dev[key].append(round(device_ms(lambda: ops.png_deflate(masks, rows_per_strip=S, nonzero_value=255, codes=codes), args.reps) / P, 5))
    emit({"measure": "wall_ms_per_mask", "shape": shape, **wall,
          "A_over_F8": round(min(wall["A"]) / min(wall["F8"]), 2), "F8_faster": max(wall["F8"]) < min(wall["A"]),
          **{f"{key}_over_F8": round(min(wall[key]) / min(wall["F8"]), 2) for key in ("D16", "D32", "D64")}})
    emit({"measure": "device_event_ms_per_mask (ops.png_deflate alone, allocations included)", "shape": shape, **dev})
    spread = max(wall["F8"]) / min(wall["F8"])
    within = [key for key in ("D16", "D32", "D64") if min(wall[key]) <= min(wall["F8"]) * spread]
    pick = min(within, key=lambda k: size[k]) if within else min(("D16", "D32", "D64"), key=lambda k: min(wall[k]))
    emit({"measure": "default strip height for dynamic codes", "shape": shape, "F8_spread_max_over_min": round(spread, 3),
          "within_the_spread": within, "pick": pick, "rule": "smallest files within the spread" if within else "none within: the fastest"})
# the one mask the CPU test of the sizes uses (tests/test_png_dyn_cpu.py, tests/_png.blob), at the defaults of png.py
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _png import blob  # noqa: E402
for H, W in ((720, 1280), (480, 854)):
    m = torch.from_numpy(blob(H, W)[None]).cuda()
    a, f, d = len(path_a(m)[0]), len(png.mask_pngs(m)[0]), len(png.mask_pngs(m, codes="dynamic")[0])
    emit({"measure": "bytes of tests/_png.blob at the defaults", "shape": f"{H} x {W}", "A": a, "fixed": f, "dynamic": d,
          "dynamic_rows_per_strip": png.DYNAMIC_ROWS_PER_STRIP, "dynamic_over_A": round(d / a, 2), "dynamic_over_fixed": round(d / f, 2)})
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
