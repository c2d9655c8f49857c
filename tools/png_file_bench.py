"""PNG files with the chunk framing and the IDAT's CRC-32 made by the host (framing="host": zlib.crc32 over every IDAT, the join)
against the same files with both made on the device (framing="device": ops.png_file, include/tce_rvos_pngfile.h), on the same GPU in the
same process.  The comparison is host framing against device framing, never the code under test against itself.

  frames    one chunk of 32 frames at 720 x 1280 and at 480 x 854, tools/vis_bench.py's recipe: smooth noise plus moving blobs plus a
            little grain, saved as JPEG (quality 90, 4:2:0) and decoded again with Pillow -- the content of photographs
  rgb       the --visualize images: vis.overlay_expression of those frames (an elliptic mask with a wavy edge, its box, a point),
            png.rgb_pngs
  masks     the same blob masks, png.mask_pngs(codes="dynamic")
  labels    label maps of three such blobs, png.label_pngs(codes="dynamic") with a 256-entry palette
  wall      host time from the device tensors to the list of finished `bytes`, device idle before and after, per file, for both
            framings, interleaved, --rounds rounds of --reps calls; "device" counts as faster only if it is in every round
  device    device-event time of ops.png_file alone (its two launches, outputs allocated before), per file
  crc32     the host's bare zlib.crc32 over one IDAT of each kind
  equal     both framings return the same files, byte for byte
  split     with --split-videos V: infer.run_split with overlays on over V generated videos of 32 frames at 720 x 1280 with 3
            expressions each (Swin-T, synthetic weights, Resize(360)), under both framings, interleaved after a warm-up pass of
            each: frames/s, the busy table, the encode stage's share of the wall time; the two trees of files are compared
  One JSON line per measurement, to stdout and to --out (default profiles/r23_png_file.txt).

  python tools/png_file_bench.py [--reps N] [--rounds R] [--split-videos V] [--out PATH]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
import zlib

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tce_rvos_amd import ops, png, vis  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--split-videos", type=int, default=0, help="> 0: also one run_split pass with overlays under both framings")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_png_file.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("png_file_bench: needs the GPU (a time taken elsewhere says nothing)")

P = 32
COLOR = (236, 95, 17)
PALETTE = bytes((37 * k + 11 * c) % 256 for k in range(256) for c in range(3))
lines = []


def emit(obj):
    lines.append(json.dumps(obj))
    print(lines[-1], flush=True)


def jpeg_frames(root, H, W, seed):
    """tools/vis_bench.py's generator: one video of P frames -> uint8 [P,H,W,3] as Pillow decodes the files"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    ground = Image.fromarray(rng.integers(0, 256, (H // 16, W // 16, 3), dtype=np.uint8)).resize((W, H), Image.BICUBIC)
    ground = np.asarray(ground).astype(np.float32)
    blobs = [(rng.uniform(0.2, 0.8) * H, rng.uniform(0.2, 0.8) * W, rng.uniform(0.05, 0.2) * H, rng.uniform(-6, 6),
              rng.uniform(-9, 9), rng.uniform(0, 255, 3)) for _ in range(4)]
    out = []
    for k in range(P):
        img = ground.copy()
        for cy, cx, r, vy, vx, colour in blobs:
            img[(y - cy - vy * k) ** 2 + (x - cx - vx * k) ** 2 < r * r] = colour
        img += rng.normal(0, 4, (H, W, 1)).astype(np.float32)
        path = os.path.join(root, "%dx%d_%05d.jpg" % (H, W, k))
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(path, quality=90, subsampling="4:2:0")
        out.append(np.asarray(Image.open(path).convert("RGB")))
    return np.stack(out)


def layer(H, W, seed):
    """tools/vis_bench.py's layer: masks uint8 [P,H,W], boxes [P,4] (the masks' bounding boxes), points [P,2]"""
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


def host_crc_ms(blob, head_bytes, reps=20):
    """zlib.crc32 over type + data of the file's IDAT, the way png.chunk runs it"""
    n = int.from_bytes(blob[head_bytes:head_bytes + 4], "big")
    body = blob[head_bytes + 4:head_bytes + 8 + n]
    assert body[:4] == b"IDAT" and zlib.crc32(body) == int.from_bytes(blob[head_bytes + 8 + n:head_bytes + 12 + n], "big")
    t0 = time.perf_counter()
    for _ in range(reps):
        zlib.crc32(body)
    return (time.perf_counter() - t0) / reps * 1e3, n


def split_pass(root):
    """tools/split_bench.py's split (--split-videos videos of 32 JPEG frames at 720 x 1280, 3 expressions, Swin-T with synthetic
    weights, Resize(360)) through infer.run_split with overlays on, under both framings: a warm-up pass of each, then interleaved
    rounds; wall seconds, frames/s, the busy table and the encode stage's share of the wall time"""
    import hashlib
    from tce_rvos_amd import build_model, infer, load_synth_weights
    from tce_rvos_amd.frontend import ClipFrontEnd
    H, W = 720, 1280
    captions = ("a person", "the person that walks to the left of the frame",
                "a small dog which runs behind the person and then jumps over the bench near the tree at the end")
    videos = {}
    for v in range(args.split_videos):
        name = "video%02d" % v
        d = os.path.join(root, "JPEGImages", name)
        os.makedirs(d)
        jpeg_frames(d, H, W, 100 + v)                                # P frames as 720x1280_%05d.jpg
        frames = ["%dx%d_%05d" % (H, W, k) for k in range(P)]
        videos[name] = {"frames": frames, "expressions": {str(i): {"exp": c} for i, c in enumerate(captions)}}
    meta = os.path.join(root, "meta_expressions.json")
    with open(meta, "w") as fh:
        json.dump({"videos": videos}, fh)
    jobs = infer.jobs_from_meta(meta, os.path.join(root, "JPEGImages"))
    total = sum(len(j.frame_paths) for j in jobs)
    model, _, _ = build_model(argparse.Namespace(backbone="swin_t_p4w7", with_box_refine=True, binary=True, freeze_text_encoder=True,
                                                 f_token=8, qtrans=True, num_feature_levels=4))
    model = model.cuda().eval()
    load_synth_weights(model, 31)
    model.repack()
    fe = ClipFrontEnd()
    colors = torch.tensor([[236, 95, 17], [17, 95, 236], [95, 236, 17]], dtype=torch.uint8)

    def digest(*dirs):
        h, n = hashlib.sha256(), 0
        for top in dirs:
            for d, sub, fs in os.walk(top):
                sub.sort()
                for f in sorted(fs):
                    h.update(os.path.relpath(os.path.join(d, f), top).encode())
                    with open(os.path.join(d, f), "rb") as fh:
                        h.update(fh.read())
                    n += 1
        return n, h.hexdigest()

    def one(framing):
        out, ov = os.path.join(root, "out_" + framing), os.path.join(root, "ov_" + framing)
        torch.cuda.synchronize()
        res = infer.run_split(model, jobs, out, mode="video", frontend=fe, driver_kwargs={"mixed_lengths": True}, workers=8, depth=2,
                              overlays=dict(dir=ov, colors=colors), framing=framing)
        torch.cuda.synchronize()
        dg = digest(out, ov)
        shutil.rmtree(out)
        shutil.rmtree(ov)
        return res, dg

    want = None
    for framing in ("host", "device"):  # warm-up: code objects, graph captures, the page cache; and the agreement of the files
        res, dg = one(framing)
        want = want or dg
        emit({"measure": "run_split with overlays, warm-up pass", "framing": framing, "seconds": round(res["seconds"], 3), "files": dg[0],
              "files_equal_host_framing_s": dg == want})
    rows = {"host": [], "device": []}
    for r in range(args.rounds):  # interleaved
        for framing in ("host", "device"):
            res, dg = one(framing)
            sec = res["seconds"]
            rows[framing].append(sec)
            emit({"measure": "run_split with overlays, pass", "round": r, "framing": framing, "videos": len(jobs), "frames": total,
                  "files": res["files"], "files_equal_host_framing_s": dg == want, "seconds": round(sec, 3),
                  "frames_per_s": round(total / sec, 1), "busy": {s: round(v, 3) for s, v in res["busy"].items()},
                  "encode_busy_over_wall": round(res["busy"]["encode"] / sec, 3), "forward_busy_over_wall": round(res["busy"]["forward"] / sec, 3)})
    emit({"measure": "run_split with overlays, summary (fastest pass)", "frames_per_s": {k: round(total / min(v), 1) for k, v in rows.items()},
          "device_rate_over_host": round(min(rows["host"]) / min(rows["device"]), 2),
          "device_faster_in_every_round": all(d < h for h, d in zip(rows["host"], rows["device"]))})


work = tempfile.mkdtemp(prefix="png_file_bench_")
try:
    emit({"measure": "setup", "device": torch.cuda.get_device_name(0), "files_per_chunk": P, "reps": args.reps, "rounds": args.rounds,
          "zlib": zlib.ZLIB_RUNTIME_VERSION, "segment_bytes": ops.PNG_FILE_SEGMENT, "piece_bytes": ops.PNG_FILE_PIECE,
          "kernel_times_from_a_profiler": "none taken",
          "not_measured": ("" if args.split_videos > 0 else "the split driver with overlays= end to end under either framing; ") +
          "the write to disk alone; sizes other than the two below; real checkpoints; several overlay layers"})
    for H, W in ((720, 1280), (480, 854)):
        frames = torch.from_numpy(jpeg_frames(work, H, W, H)).cuda()
        m, b, pt = layer(H, W, H + 1)
        result = {"masks": torch.from_numpy(m).cuda(), "pred_boxes": torch.from_numpy(b).cuda(), "reference_points": torch.from_numpy(pt).cuda()}
        images = vis.overlay_expression(frames, result, COLOR)
        lab = m.astype(np.uint8) + 2 * np.roll(m, (H // 5, W // 7), (1, 2)) * (1 - m) + 3 * np.roll(m, (-H // 6, -W // 5), (1, 2)) * (1 - m)
        labels = torch.from_numpy(np.minimum(lab, 5).astype(np.uint8)).cuda()
        kinds = {
            "rgb": (lambda f: png.rgb_pngs(images, framing=f), len(png.head_rgb(W, H)),
                    lambda: ops.png_deflate_rows(ops.png_filter_rgb(images), rows_per_strip=png.DYNAMIC_ROWS_PER_STRIP)),
            "masks": (lambda f: png.mask_pngs(result["masks"], codes="dynamic", framing=f), len(png.head(W, H, "L")),
                      lambda: ops.png_deflate(result["masks"], rows_per_strip=png.DYNAMIC_ROWS_PER_STRIP, nonzero_value=255, codes="dynamic")),
            "labels": (lambda f: png.label_pngs(labels, PALETTE, codes="dynamic", framing=f), len(png.head(W, H, "P", PALETTE)),
                       lambda: ops.png_deflate(labels, rows_per_strip=png.DYNAMIC_ROWS_PER_STRIP, codes="dynamic")),
        }
        for kind, (encode, head_bytes, streams_of) in kinds.items():
            shape = f"{P} x {H} x {W}" + (" x 3" if kind == "rgb" else "")
            host_files, dev_files = encode("host"), encode("device")
            equal = host_files == dev_files
            for _ in range(2):  # warm-up: code objects, the allocator's blocks
                encode("host"), encode("device")
            wall = {"host": [], "device": []}
            for _ in range(args.rounds):  # interleaved
                for f in ("host", "device"):
                    wall[f].append(round(wall_ms(lambda: encode(f), args.reps) / P, 4))
            streams, nbytes = streams_of()
            head = torch.frombuffer(bytearray(host_files[0][:head_bytes]), dtype=torch.uint8).cuda()
            files, fb = ops.png_file(streams, nbytes, head)
            ws = torch.empty(max(1, int(streams.shape[0]) * (int(streams.shape[1]) // ops.PNG_FILE_SEGMENT + 1)), dtype=torch.int64, device="cuda")
            two = [round(device_ms(lambda: ops.png_file(streams, nbytes, head, files=files, file_bytes=fb, ws=ws), args.reps) / P, 5)
                   for _ in range(args.rounds)]
            crc_ms, idat = host_crc_ms(host_files[0], head_bytes)
            faster = [d < h for h, d in zip(wall["host"], wall["device"])]
            emit({"measure": "wall_ms_per_file (device tensors -> finished bytes)", "kind": kind, "shape": shape,
                  "files_equal_byte_for_byte": equal, "mean_file_bytes": round(sum(len(x) for x in host_files) / P),
                  "host": wall["host"], "device": wall["device"], "host_over_device": round(min(wall["host"]) / min(wall["device"]), 2),
                  "device_faster_in_every_round": all(faster), "device_faster_in_no_round": not any(faster),
                  "png_file_device_event_ms_per_file (two launches)": two,
                  "host_zlib_crc32_ms_over_the_IDAT_of_file_0": round(crc_ms, 4), "IDAT_bytes_of_file_0": idat,
                  "extra_device_bytes_per_call": int(files.numel())})
    if args.split_videos > 0:
        split_pass(work)
finally:
    shutil.rmtree(work, ignore_errors=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
