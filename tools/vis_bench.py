"""The --visualize images of one chunk of frames: vis.overlay_expression + png.rgb_pngs (drawn, filtered and deflated on the GPU, two
small read-backs, host framing) against the loop a caller writes without them, on the same GPU in the same process.

  frames    one chunk of 32 frames at 720 x 1280 and at 480 x 854, generated the way tools/split_bench.py generates its split (smooth
            noise plus moving blobs plus a little grain), saved as JPEG (quality 90, 4:2:0) and decoded again with Pillow: the
            content of photographs, not flat colour
  layer     per frame an elliptic mask with a wavy edge, its bounding box, a reference point at its centre, one colour
  A  host   masks / boxes / points .cpu(), then per frame the reference's own lines (inference_ytvos.py:325-351) saved to memory:
            Image.fromarray(frame).convert('RGBA'), ImageDraw.rectangle(width=2), two ImageDraw.line(width=4), the numpy blend,
            Image.save(buffer, 'PNG') -- Pillow's zlib at its default level
  B  device vis.overlay_expression + png.rgb_pngs(rows_per_strip=S) for S = 16, 32, 64
  wall      host time from the device tensors to the list of finished files, device idle before and after, per image
  device    device-event time of each stage alone, per image: ops.vis_overlay, ops.png_filter_rgb, ops.png_deflate_rows (S = 32)
  bytes     the mean file size of each path, the raw size of an image, the rows per filter type, the block type of the first strip
  pixels    every file of both paths decodes to the same pixels (the boxes are of the regular class, where the rule is Pillow's)
  Interleaved rounds in one process; one JSON line per measurement, to stdout and to --out (default profiles/r22_vis_overlays.txt).

  python tools/vis_bench.py [--reps N] [--reps-a N] [--rounds R] [--out PATH]"""
import argparse
import io
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import PIL
import torch
from PIL import Image, ImageDraw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tce_rvos_amd import ops, png, vis  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--reps-a", type=int, default=1)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_vis_overlays.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("vis_bench: needs the GPU (a time taken elsewhere says nothing)")

P = 32
STRIPS = (16, 32, 64)
COLOR = (236, 95, 17)
lines = []


def emit(obj):
    lines.append(json.dumps(obj))
    print(lines[-1], flush=True)


def jpeg_frames(root, H, W, seed):
    """split_bench.make_split's recipe for one video of P frames -> (uint8 [P,H,W,3] as Pillow decodes the files, bytes per file)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    ground = Image.fromarray(rng.integers(0, 256, (H // 16, W // 16, 3), dtype=np.uint8)).resize((W, H), Image.BICUBIC)
    ground = np.asarray(ground).astype(np.float32)
    blobs = [(rng.uniform(0.2, 0.8) * H, rng.uniform(0.2, 0.8) * W, rng.uniform(0.05, 0.2) * H, rng.uniform(-6, 6),
              rng.uniform(-9, 9), rng.uniform(0, 255, 3)) for _ in range(4)]
    out, nbytes = [], 0
    for k in range(P):
        img = ground.copy()
        for cy, cx, r, vy, vx, colour in blobs:
            img[(y - cy - vy * k) ** 2 + (x - cx - vx * k) ** 2 < r * r] = colour
        img += rng.normal(0, 4, (H, W, 1)).astype(np.float32)
        path = os.path.join(root, "%dx%d_%05d.jpg" % (H, W, k))
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(path, quality=90, subsampling="4:2:0")
        nbytes += os.path.getsize(path)
        out.append(np.asarray(Image.open(path).convert("RGB")))
    return np.stack(out), nbytes / P


def layer(H, W, seed):
    """masks uint8 [P,H,W], boxes [P,4] (the masks' bounding boxes, a pixel inside), points [P,2]"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    masks, boxes, points = np.zeros((P, H, W), np.uint8), np.zeros((P, 4), np.float32), np.zeros((P, 2), np.float32)
    for p in range(P):
        cy, cx = rng.uniform(0.3, 0.7) * H, rng.uniform(0.3, 0.7) * W
        ry, rx = rng.uniform(0.1, 0.3) * H, rng.uniform(0.1, 0.3) * W
        ang = np.arctan2(y - cy, x - cx)
        edge = 1.0 + 0.08 * np.sin(rng.integers(3, 9) * ang + rng.uniform(0, 6)) + 0.03 * np.sin(rng.integers(15, 40) * ang)
        masks[p] = (((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 < edge ** 2).astype(np.uint8)
        ys, xs = np.nonzero(masks[p])
        x0, x1, y0, y1 = xs.min() + 0.5, xs.max() + 0.5, ys.min() + 0.5, ys.max() + 0.5
        boxes[p] = [(x0 + x1) / 2 / W, (y0 + y1) / 2 / H, (x1 - x0) / W, (y1 - y0) / H]
        points[p] = [cx / W, cy / H]
    return masks, boxes, points


def path_a(frames, result):
    """(files, the drawn pixels): the reference's block per frame, from device tensors"""
    host = frames.cpu().numpy()
    masks, boxes, points = result["masks"].cpu().numpy(), result["pred_boxes"].cpu(), result["reference_points"].cpu().tolist()
    Hh, Ww = host.shape[1:3]
    files, pixels = [], []
    for t in range(host.shape[0]):
        img = Image.fromarray(host[t]).convert("RGBA")
        draw = ImageDraw.Draw(img)
        xc, yc, w, h = boxes[t][None].unbind(1)
        b = torch.stack([xc - 0.5 * w, yc - 0.5 * h, xc + 0.5 * w, yc + 0.5 * h], 1) * torch.tensor([Ww, Hh, Ww, Hh], dtype=torch.float32)
        x0, y0, x1, y1 = b.tolist()[0]
        draw.rectangle(((x0, y0), (x1, y1)), outline=COLOR, width=2)
        px, py = Ww * points[t][0], Hh * points[t][1]
        draw.line((px - 10, py, px + 10, py), COLOR, width=4)
        draw.line((px, py - 10, px, py + 10), COLOR, width=4)
        rgb = np.asarray(img.convert("RGB")).copy()
        m = masks[t].astype("uint8") > 0
        rgb[m] = rgb[m] * 0.5 + np.array(COLOR) * 0.5
        buf = io.BytesIO()
        Image.fromarray(rgb).save(buf, format="PNG")
        files.append(buf.getvalue())
        pixels.append(rgb)
    return files, np.stack(pixels)


def path_b(frames, result, S):
    return png.rgb_pngs(vis.overlay_expression(frames, result, COLOR), rows_per_strip=S)


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


def first_block(blob):
    """the block type of a file's first strip: the IDAT data starts at byte 41 (signature, IHDR, the chunk's length and type), the
    zlib header takes two bytes, BTYPE is bits 1 and 2 of the next"""
    return {1: "fixed", 2: "dynamic"}.get((blob[43] >> 1) & 3, "?")


work = tempfile.mkdtemp(prefix="vis_bench_")
try:
    emit({"measure": "setup", "device": torch.cuda.get_device_name(0), "images_per_chunk": P, "reps_b": args.reps, "reps_a": args.reps_a,
          "rounds": args.rounds, "pillow": PIL.__version__,
          "kernel_times_from_a_profiler": "none taken", "not_measured": "the split driver with overlays= end to end; L > 1 layers; "
          "the write to disk; sizes other than the two below"})
    for H, W in ((720, 1280), (480, 854)):
        host, jpeg_bytes = jpeg_frames(work, H, W, H)
        m, b, pt = layer(H, W, H + 1)
        frames = torch.from_numpy(host).cuda()
        result = {"masks": torch.from_numpy(m).cuda(), "pred_boxes": torch.from_numpy(b).cuda(), "reference_points": torch.from_numpy(pt).cuda()}
        shape = f"{P} x {H} x {W} x 3"
        # agreement first: every file of every path decodes to the same pixels
        files_a, pixels = path_a(frames, result)
        drawn = vis.overlay_expression(frames, result, COLOR).cpu().numpy()
        same = bool(np.array_equal(drawn, pixels))
        files = {"A": files_a}
        for S in STRIPS:
            files[f"B{S}"] = path_b(frames, result, S)
        for key, fs in files.items():
            for k, f in enumerate(fs):
                im = Image.open(io.BytesIO(f))
                assert im.mode == "RGB" and np.array_equal(np.asarray(im), drawn[k] if key != "A" else pixels[k]), (key, k)
        size = {key: sum(len(f) for f in fs) / P for key, fs in files.items()}
        rows = ops.png_filter_rgb(torch.from_numpy(drawn).cuda())
        types = np.bincount(rows[:, :, 0].cpu().numpy().reshape(-1), minlength=5)
        emit({"measure": "pixels", "shape": shape, "device_overlay_equals_the_pillow_drawing": same,
              "pixels_that_differ": int((drawn != pixels).any(-1).sum()), "every_file_decodes_to_its_pixels": True,
              "jpeg_bytes_per_frame": round(jpeg_bytes)})
        emit({"measure": "bytes_per_file", "shape": shape, "raw_bytes": H * W * 3, **{key: round(v) for key, v in size.items()},
              **{f"B{S}_over_A": round(size[f"B{S}"] / size["A"], 2) for S in STRIPS},
              **{f"B{S}_over_raw": round(size[f"B{S}"] / (H * W * 3), 3) for S in STRIPS},
              "rows_per_filter_type_0_to_4": [int(v) for v in types], "first_block_of_image_0": first_block(files["B32"][0])})
        img = torch.from_numpy(drawn).cuda()
        col = torch.tensor([COLOR], dtype=torch.uint8).cuda()
        l1 = {k: v.unsqueeze(0).contiguous() for k, v in result.items()}
        for _ in range(2):  # warm-up: code objects, the allocator's blocks
            for S in STRIPS:
                path_b(frames, result, S)
        wall = {"A": []}
        wall.update({f"B{S}": [] for S in STRIPS})
        dev = {"overlay": [], "filter": [], "deflate_rows_S32": [], "all_three_S32": []}
        for _ in range(args.rounds):  # interleaved
            wall["A"].append(round(wall_ms(lambda: path_a(frames, result), args.reps_a) / P, 3))
            for S in STRIPS:
                wall[f"B{S}"].append(round(wall_ms(lambda: path_b(frames, result, S), args.reps) / P, 4))
            over = lambda: ops.vis_overlay(frames, col, masks=l1["masks"], boxes=l1["pred_boxes"], points=l1["reference_points"])  # noqa: E731
            dev["overlay"].append(round(device_ms(over, args.reps) / P, 5))
            dev["filter"].append(round(device_ms(lambda: ops.png_filter_rgb(img), args.reps) / P, 5))
            dev["deflate_rows_S32"].append(round(device_ms(lambda: ops.png_deflate_rows(rows, rows_per_strip=32), args.reps) / P, 5))
            dev["all_three_S32"].append(round(device_ms(lambda: ops.png_deflate_rows(ops.png_filter_rgb(over()), rows_per_strip=32),
                                                        args.reps) / P, 5))
        emit({"measure": "wall_ms_per_image (device tensors -> finished files)", "shape": shape, **wall,
              **{f"A_over_B{S}": round(min(wall["A"]) / min(wall[f"B{S}"]), 1) for S in STRIPS},
              "B32_faster_in_every_round": max(wall["B32"]) < min(wall["A"])})
        gb = H * W * (3 + 1 + 3) / 1e9
        emit({"measure": "device_event_ms_per_image (each stage alone, allocations included)", "shape": shape, **dev,
              "overlay_GB_per_s (7 bytes a pixel)": round(gb / (min(dev["overlay"]) * 1e-3), 1)})
finally:
    shutil.rmtree(work, ignore_errors=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
