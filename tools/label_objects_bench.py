"""Ref-DAVIS label maps: tce_label_objects_u8 against the same computation composed from the reference caller's own PyTorch
primitives on the GPU, in one process (inference_davis.py:239-248, 293-298: F.interpolate -> sigmoid -> threshold -> cat -> argmax
-> uint8), and video.run_video_objects with the four annotator sets against run_video_expressions plus that composition.

  kernel      n = 3 and 5 objects, T = 32, 120 x 214 -> 480 x 854 (a 32-frame DAVIS chunk): device-event time per call, interleaved
              rounds, the algorithmic bytes (n best-query planes read + 1 byte per pixel written) over that time, and the share of
              pixels on which the two disagree (rounding at the threshold / between near-equal scores: tests/_davis.py).
  driver      config-2 frames (Swin-T, T = 5, 360 x 640, one clip), 8 expressions = 2 objects x 4 annotators, label maps at 480 x 854:
              expressions/s of run_video_objects(object_sets=davis_annotator_sets(8)) against run_video_expressions (whose raw
              forward outputs are kept) followed by the composition per annotator.  The baseline's time includes the 8
              tce_select_masks_u8 launches run_video_expressions makes; a caller that only wants label maps would not need them.

  python tools/label_objects_bench.py [--reps N] [--skip-driver]        prints one JSON line per measurement"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tce_rvos_amd import build_model, load_synth_weights, ops  # noqa: E402
from tce_rvos_amd.video import davis_annotator_sets, run_video_expressions, run_video_objects  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--skip-driver", action="store_true")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("label_objects_bench: needs the GPU (a time taken elsewhere says nothing)")


def composition(logits, masks, size, threshold=0.5, background=0.1):
    """The reference caller's lines on the GPU, per object then per annotator."""
    anno_masks = []
    for pred_logits, pred_masks in zip(logits, masks):
        clip_len = pred_logits.shape[0]
        pred_scores = pred_logits.sigmoid().mean(0)
        max_scores, _ = pred_scores.max(-1)
        _, max_ind = max_scores.max(-1)
        max_inds = max_ind.repeat(clip_len)
        pm = pred_masks[range(clip_len), max_inds, ...].unsqueeze(0)
        pm = F.interpolate(pm, size=size, mode="bilinear", align_corners=False)
        anno_masks.append(pm.sigmoid()[0])
    anno_masks = torch.stack(anno_masks)
    t, h, w = anno_masks.shape[-3:]
    anno_masks[anno_masks < threshold] = 0.0
    bg = background * torch.ones(1, t, h, w, device=anno_masks.device)
    anno_masks = torch.cat([bg, anno_masks], dim=0)
    return torch.argmax(anno_masks, dim=0).to(torch.uint8)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps  # ms per call


T, Q, h, w, H0, W0 = 32, 5, 120, 214, 480, 854
for n in (3, 5):
    g = torch.Generator().manual_seed(40 + n)
    lg = [torch.randn(T, Q, 1, generator=g).cuda() for _ in range(n)]
    pm = [(torch.randn(T, Q, h, w, generator=g) * 3).cuda() for _ in range(n)]
    out = torch.empty(T, H0, W0, dtype=torch.uint8, device="cuda")
    best = torch.empty(n, dtype=torch.int32, device="cuda")
    run = {"kernel": lambda: ops.label_objects(lg, pm, (H0, W0), out=out, best_out=best),
           "composition": lambda: composition(lg, pm, (H0, W0))}
    for fn in run.values():  # warm-up: code objects, the allocator's blocks
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    differ = float((run["kernel"]()[0] != run["composition"]()).float().mean())
    ms = {k: [] for k in run}
    for _ in range(args.rounds):  # interleaved A/B
        for k, fn in run.items():
            ms[k].append(round(timed(fn, args.reps), 4))
    nbytes = n * T * h * w * 4 + T * H0 * W0
    km, cm = min(ms["kernel"]), min(ms["composition"])
    print(json.dumps({"measure": "kernel", "n": n, "shape": f"T={T} {h}x{w}->{H0}x{W0}", "reps": args.reps,
                      "ms_per_call": ms, "kernel_algorithmic_GB_per_s": round(nbytes / km / 1e6, 1),
                      "composition_over_kernel": round(cm / km, 2), "kernel_faster": km < cm,
                      "labels_differ_share": differ}), flush=True)
    assert max(ms["kernel"]) < min(ms["composition"]), "the kernel is not faster than the composition in this run"

if not args.skip_driver:
    model, _, _ = build_model(argparse.Namespace(backbone="swin_t_p4w7", with_box_refine=True, binary=True, freeze_text_encoder=True,
                                                 f_token=8, qtrans=True, num_feature_levels=4))
    model = model.cuda().eval()
    load_synth_weights(model, 31)
    model.repack()
    Tc, H, W = 5, 360, 640
    g = torch.Generator().manual_seed(0)
    frames = torch.randn(Tc, 3, H, W, generator=g).cuda()
    caps = []
    for ln in (9, 9, 9, 9, 12, 12, 12, 12):  # object-major, 4 annotators each (two token lengths: two forwards per clip)
        ids = torch.randint(3, 50000, (1, ln), generator=g)
        ids[0, 0], ids[0, -1] = 0, 2
        caps.append(ids)
    sets = davis_annotator_sets(len(caps))
    raw = []
    orig = model.forward_group

    def keeping(*a, **k):
        outs = orig(*a, **k)
        raw.extend(outs)
        return outs

    def ours():
        return [r["labels"] for r in run_video_objects(model, frames, caps, (H0, W0), clip_size=None, object_sets=sets, max_group=4)]

    def baseline():
        raw.clear()
        model.forward_group = keeping
        try:
            run_video_expressions(model, frames, caps, (H0, W0), clip_size=None, max_group=4)
        finally:
            del model.forward_group
        # plan_expression_groups with one bucket per length, in order: raw[i] is caption i's forward
        return [composition([raw[i]["pred_logits"][0] for i in s], [raw[i]["pred_masks"][0] for i in s], (H0, W0)) for s in sets]

    run = {"run_video_objects": ours, "run_video_expressions+composition": baseline}
    for fn in run.values():  # eager sightings + graph captures
        for _ in range(4):
            fn()
    torch.cuda.synchronize()
    a, b = ours(), baseline()
    differ = max(float((x != y).float().mean()) for x, y in zip(a, b))
    reps = max(5, args.reps // 3)
    res = {k: {"expressions_per_s": [], "ms_per_video": []} for k in run}
    for _ in range(args.rounds):
        for k, fn in run.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / reps
            res[k]["expressions_per_s"].append(round(len(caps) / dt, 1))
            res[k]["ms_per_video"].append(round(dt * 1e3, 2))
    print(json.dumps({"measure": "driver", "config": f"swin_t_p4w7 T={Tc} {H}x{W} -> labels {H0}x{W0}", "expressions": len(caps),
                      "sets": sets, "reps": reps, **res, "labels_differ_share_max": differ}), flush=True)
