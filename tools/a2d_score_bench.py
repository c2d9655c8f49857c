"""A2D-Sentences / JHMDB-Sentences scoring: a2d_score.A2DScorer.update on device-resident masks (one upload of the ground truth's
run lengths, tce_rle_decode_u8, tce_mask_overlap_i32, one copy of the scores; no read-back) and its one state() read-back, beside
the host restatement of what the reference's scorer does with the same samples (numpy decode of every run-length string and
numpy overlap counts; the reference decodes with pycocotools' C code, absent here, and counts with torch on the CPU).

  shapes      N = 5 queries at 240 x 320 (A2D) and 320 x 426; smooth synthetic masks (ellipses, tens of runs per column-major mask).
  update      wall time per update() over the stream: K updates issued back to back, one synchronise at the end; and the
              device-event time of the same window.  Both include the host work of update (string -> counts, the upload).
  state       wall time of the one read-back of K images' counts and scores, device idle before.
  numpy       wall time per sample of the host restatement: .cpu() of the N masks, decode of the ground-truth string, counts.
  Interleaved rounds in one process; one JSON line per measurement.

  python tools/a2d_score_bench.py [--images K] [--rounds R]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tce_rvos_amd.a2d_score import A2DScorer, rle_from_string  # noqa: E402
from tce_rvos_amd.postprocess import rle_to_string  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=200)
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("a2d_score_bench: needs the GPU (a time taken elsewhere says nothing)")
N, K = 5, args.images


def ellipse(rng, H, W):
    cy, cx, ry, rx = rng.uniform(0.2 * H, 0.8 * H), rng.uniform(0.2 * W, 0.8 * W), rng.uniform(0.1 * H, 0.4 * H), rng.uniform(0.1 * W, 0.4 * W)
    y, x = np.mgrid[0:H, 0:W]
    return (((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0).astype(np.uint8)


def numpy_counts(mask):
    flat = mask.T.reshape(-1)
    q = np.flatnonzero(np.diff(flat, prepend=np.uint8(0)))
    return np.diff(np.concatenate([[0], q, [flat.size]])) if q.size else np.asarray([flat.size])


def numpy_decode(counts, H, W):
    return np.repeat((np.arange(len(counts)) & 1).astype(np.uint8), counts).reshape(W, H).T


def numpy_sample(masks_gpu, string, H, W):
    pred = masks_gpu.cpu().numpy() != 0
    gt = numpy_decode(rle_from_string(string), H, W) != 0
    return np.stack([(pred & gt[None]).sum((1, 2)), pred.sum((1, 2)), np.full(N, gt.sum())], axis=1)


for H, W in ((240, 320), (320, 426)):
    rng = np.random.default_rng(H)
    gts = [ellipse(rng, H, W) for _ in range(8)]
    strings = [rle_to_string(numpy_counts(g)) for g in gts]
    preds = [torch.from_numpy(np.stack([ellipse(rng, H, W) for _ in range(N)])).cuda().unsqueeze(1) for _ in range(8)]
    scores = [torch.rand(N, device="cuda") for _ in range(8)]
    gt = {k: {"size": [H, W], "counts": strings[k % 8]} for k in range(K)}
    processed = [{"scores": scores[k % 8], "masks": preds[k % 8]} for k in range(K)]

    def run_updates():
        sc = A2DScorer(gt)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for k in range(K):
            sc.update([k], [processed[k]])
        e1.record()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / K * 1e6
        t0 = time.perf_counter()
        st = sc.state()
        return sc, st, wall, e0.elapsed_time(e1) / K * 1e3, (time.perf_counter() - t0) * 1e6

    def run_numpy():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = [numpy_sample(preds[k % 8][:, 0], strings[k % 8], H, W) for k in range(K)]
        return out, (time.perf_counter() - t0) / K * 1e6

    run_updates()  # warm-up: code objects, the allocator's blocks
    run_numpy()
    upd, dev, state, host = [], [], [], []
    for _ in range(args.rounds):
        sc, st, w, d, s = run_updates()
        want, h = run_numpy()
        upd.append(round(w, 1)); dev.append(round(d, 1)); state.append(round(s, 1)); host.append(round(h, 1))
    equal = all(st["counts"][k] == want[k].tolist() for k in range(K))
    runs = [len(rle_from_string(s)) for s in strings]
    print(json.dumps({"shape": f"N={N} {H}x{W}", "images": K, "rounds": args.rounds, "counts_equal_numpy": equal,
                      "runs_per_ground_truth": [min(runs), max(runs)],
                      "us_per_update_wall": upd, "us_per_update_device_events": dev, "us_state_readback_of_all_images": state,
                      "us_per_sample_numpy_restatement": host, "numpy_over_update": round(min(host) / min(upd), 1)}), flush=True)
