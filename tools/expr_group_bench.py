"""Expressions of one video at mixed token lengths: run_video_expressions bucketed by length (the default) against
mixed_lengths=True (forward_group(..., ragged=True): one group per `max_group` expressions, right-padded to the longest).
Config-2 frames (Swin-T, T = 5, 360 x 640, one clip), five expressions of 6 / 9 / 12 / 14 / 20 tokens, graph replay after
warm-up.  Prints pairs/s and forward_group calls per video for each mode.   python tools/expr_group_bench.py [--reps N]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tce_rvos_amd import build_model, load_synth_weights  # noqa: E402
from tce_rvos_amd.video import run_video_expressions  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--lens", default="6,9,12,14,20")
ap.add_argument("--max-group", type=int, default=4)
args = ap.parse_args()

model, _, _ = build_model(argparse.Namespace(backbone="swin_t_p4w7", with_box_refine=True, binary=True, freeze_text_encoder=True,
                                             f_token=8, qtrans=True, num_feature_levels=4))
model = model.cuda().eval()
load_synth_weights(model, 31)
model.repack()
T, H, W = 5, 360, 640
g = torch.Generator().manual_seed(0)
frames = torch.randn(T, 3, H, W, generator=g).cuda()
lens = [int(x) for x in args.lens.split(",")]
caps = []
for n in lens:
    ids = torch.randint(3, 50000, (1, n), generator=g)
    ids[0, 0], ids[0, -1] = 0, 2
    caps.append(ids)

calls = []
orig = model.forward_group


def counting(*a, **k):
    calls.append(1)
    return orig(*a, **k)


model.forward_group = counting
res = {}
for mixed in (False, True, False, True):  # interleaved A/B
    name = "mixed" if mixed else "bucketed"
    for _ in range(3):  # eager sightings + captures
        run_video_expressions(model, frames, caps, (H, W), clip_size=None, max_group=args.max_group, mixed_lengths=mixed)
    torch.cuda.synchronize()
    calls.clear()
    t0 = time.perf_counter()
    for _ in range(args.reps):
        run_video_expressions(model, frames, caps, (H, W), clip_size=None, max_group=args.max_group, mixed_lengths=mixed)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.reps
    r = res.setdefault(name, {"pairs_per_s": [], "ms_per_video": [], "forward_group_calls_per_video": len(calls) / args.reps})
    r["pairs_per_s"].append(round(len(caps) / dt, 1))
    r["ms_per_video"].append(round(dt * 1e3, 2))
del model.forward_group
line = {"config": "swin_t_p4w7 T=5 360x640", "lens": lens, "max_group": args.max_group, "reps": args.reps, **res}
print(json.dumps(line))
