"""A dataset split from JPEG files to PNG files: infer.run_split against the loop a caller writes by hand, in one process.

  split     generated into a temporary directory: 8 videos of 40 JPEG frames at 720 x 1280 (quality 90, 4:2:0; smooth noise plus
            moving blobs plus a little grain, so the files have the size of photographs), 3 expressions of different token length
            per video; BASELINE config 2 (Swin-T, Resize(360) -> 360 x 640) with synthetic weights
  hand      (a) per video: every frame through Pillow, .cuda(), the front-end, run_video_expressions(mixed_lengths=True) with all
            captions, png.mask_pngs per expression, makedirs + png.write_files -- one stage after the other
  split_wN  (b) infer.run_split(mode="video", driver_kwargs={"mixed_lengths": True}, workers=N, depth=2) for N = 1, 4, 8
  per_exp   (c) the reference's shape of loop (inference_ytvos.py:186-363): the frames are decoded AGAIN for every expression and
            each expression is a forward of its own.  Context only.
  rows      interleaved rounds after one warm-up pass of every loop (code objects, graph captures, the page cache); per row the wall
            seconds of the pass, frames/s (distinct frames of the split), pairs/s (video x expression), the busy table (seconds
            summed per stage; decode is summed over the worker threads) and forward busy over wall: the fraction of the pass in
            which the GPU program was the active stage
  files     the warm-up pass of every loop is compared file by file with the hand loop's

  python tools/split_bench.py [--rounds R] [--videos V] [--frames N] [--out PATH]     one JSON line per measurement"""
import argparse
import hashlib
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tce_rvos_amd import build_model, infer, load_synth_weights, png  # noqa: E402
from tce_rvos_amd.frontend import ClipFrontEnd  # noqa: E402
from tce_rvos_amd.video import run_video_expressions  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--videos", type=int, default=8)
ap.add_argument("--frames", type=int, default=40)
ap.add_argument("--height", type=int, default=720)
ap.add_argument("--width", type=int, default=1280)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_split_driver.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("split_bench: needs the GPU (a time taken elsewhere says nothing)")

CAPTIONS = ("a person", "the person that walks to the left of the frame",
            "a small dog which runs behind the person and then jumps over the bench near the tree at the end")
lines = []


def emit(obj):
    lines.append(json.dumps(obj))
    print(lines[-1], flush=True)


def make_split(root):
    H, W = args.height, args.width
    rng = np.random.default_rng(21)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    videos, nbytes = {}, 0
    for v in range(args.videos):
        name = "video%02d" % v
        os.makedirs(os.path.join(root, "JPEGImages", name))
        ground = Image.fromarray(rng.integers(0, 256, (H // 16, W // 16, 3), dtype=np.uint8)).resize((W, H), Image.BICUBIC)
        ground = np.asarray(ground).astype(np.float32)
        blobs = [(rng.uniform(0.2, 0.8) * H, rng.uniform(0.2, 0.8) * W, rng.uniform(0.05, 0.2) * H, rng.uniform(-6, 6),
                  rng.uniform(-9, 9), rng.uniform(0, 255, 3)) for _ in range(4)]
        frames = []
        for k in range(args.frames):
            img = ground.copy()
            for cy, cx, r, vy, vx, colour in blobs:
                img[(y - cy - vy * k) ** 2 + (x - cx - vx * k) ** 2 < r * r] = colour
            img += rng.normal(0, 4, (H, W, 1)).astype(np.float32)
            f = "%05d" % (5 * k)
            path = os.path.join(root, "JPEGImages", name, f + ".jpg")
            Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(path, quality=90, subsampling="4:2:0")
            nbytes += os.path.getsize(path)
            frames.append(f)
        videos[name] = {"frames": frames, "expressions": {str(i): {"exp": c} for i, c in enumerate(CAPTIONS)}}
    meta = os.path.join(root, "meta_expressions.json")
    with open(meta, "w") as fh:
        json.dump({"videos": videos}, fh)
    return meta, nbytes


def hand_loop(model, fe, jobs, out, per_expression=False):
    """(a), and with per_expression=True (c): the same calls, one after the other"""
    busy = {s: 0.0 for s in infer.STAGES}
    clock = time.perf_counter
    t_start = clock()
    for job in jobs:
        groups = [[e] for e in job.expressions] if per_expression else [list(job.expressions)]
        for exp_ids in groups:
            t0 = clock()
            u8 = np.stack([np.asarray(Image.open(p).convert("RGB")) for p in job.frame_paths])
            t1 = clock()
            dev = torch.from_numpy(u8).cuda()
            torch.cuda.synchronize()
            t2 = clock()
            res = run_video_expressions(model, fe(dev), [job.expressions[e] for e in exp_ids], u8.shape[1:3], mixed_lengths=True)
            t3 = clock()
            files = [png.mask_pngs(r["masks"]) for r in res]
            t4 = clock()
            for e, blobs in zip(exp_ids, files):
                d = os.path.join(out, job.name, e)
                os.makedirs(d, exist_ok=True)
                png.write_files([os.path.join(d, f + ".png") for f in job.frame_names], blobs)
            t5 = clock()
            for s, dt in zip(infer.STAGES, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4)):
                busy[s] += dt
    return {"seconds": clock() - t_start, "busy": busy}


def tree_digest(root):
    h, n = hashlib.sha256(), 0
    for d, dirs, fs in os.walk(root):
        dirs.sort()
        for f in sorted(fs):
            h.update(os.path.relpath(os.path.join(d, f), root).encode())
            with open(os.path.join(d, f), "rb") as fh:
                h.update(fh.read())
            n += 1
    return n, h.hexdigest()


work = tempfile.mkdtemp(prefix="split_bench_")
try:
    t0 = time.perf_counter()
    meta, jpeg_bytes = make_split(work)
    jobs = infer.jobs_from_meta(meta, os.path.join(work, "JPEGImages"))
    n_frames = sum(len(j.frame_paths) for j in jobs)
    n_pairs = sum(len(j.expressions) for j in jobs)
    model, _, _ = build_model(argparse.Namespace(backbone="swin_t_p4w7", with_box_refine=True, binary=True, freeze_text_encoder=True,
                                                 f_token=8, qtrans=True, num_feature_levels=4))
    model = model.cuda().eval()
    load_synth_weights(model, 31)
    model.repack()
    fe = ClipFrontEnd()
    emit({"measure": "setup", "device": torch.cuda.get_device_name(0), "videos": len(jobs), "frames": n_frames, "pairs": n_pairs,
          "frame": f"{args.height} x {args.width}", "jpeg_bytes_per_frame": round(jpeg_bytes / n_frames),
          "caption_tokens": [int(model._tokenise([c], "cpu")[0].shape[1]) for c in CAPTIONS], "model": "swin_t_p4w7, synthetic weights",
          "rounds": args.rounds, "setup_seconds": round(time.perf_counter() - t0, 1), "kernel_times_from_a_profiler": "none taken"})

    loops = {"hand": lambda out: hand_loop(model, fe, jobs, out)}
    for n in (1, 4, 8):
        loops[f"split_w{n}"] = lambda out, n=n: infer.run_split(model, jobs, out, mode="video", frontend=fe,
                                                                driver_kwargs={"mixed_lengths": True}, workers=n, depth=2)
    loops["per_exp"] = lambda out: hand_loop(model, fe, jobs, out, per_expression=True)

    def one_pass(key):
        out = os.path.join(work, "out_" + key)
        torch.cuda.synchronize()
        res = loops[key](out)
        torch.cuda.synchronize()
        digest = tree_digest(out)
        shutil.rmtree(out)
        return res, digest

    want = None
    for key in loops:  # warm-up: code objects, graph captures, the page cache; and the agreement of the files
        res, digest = one_pass(key)
        want = want or digest
        # (c) runs every expression as a forward of its own: another group shape, equal masks only to the round-off between them
        emit({"measure": "warm-up pass", "loop": key, "seconds": round(res["seconds"], 3), "files": digest[0],
              "files_equal_the_hand_loop_s": digest == want})
        assert digest == want or key == "per_exp", key
    rows = {key: [] for key in loops}
    for r in range(args.rounds):  # interleaved
        for key in loops:
            res, digest = one_pass(key)
            assert digest == want or key == "per_exp", key
            sec = res["seconds"]
            row = {"measure": "pass", "round": r, "loop": key, "seconds": round(sec, 3), "frames_per_s": round(n_frames / sec, 1),
                   "pairs_per_s": round(n_pairs / sec, 2), "busy": {s: round(v, 3) for s, v in res["busy"].items()},
                   "forward_busy_over_wall": round(res["busy"]["forward"] / sec, 3)}
            rows[key].append(row)
            emit(row)
    best = {key: min(r["seconds"] for r in rs) for key, rs in rows.items()}
    worst = {key: max(r["seconds"] for r in rs) for key, rs in rows.items()}
    emit({"measure": "summary (fastest pass of each loop)", "seconds": {k: round(v, 3) for k, v in best.items()},
          "slowest_pass_seconds": {k: round(v, 3) for k, v in worst.items()},
          "frames_per_s": {k: round(n_frames / v, 1) for k, v in best.items()},
          **{f"{k}_rate_over_hand": round(best["hand"] / best[k], 2) for k in best if k != "hand"},
          "split_w8_faster_than_hand_in_every_round": worst["split_w8"] < best["hand"]})
finally:
    shutil.rmtree(work, ignore_errors=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
