"""A2D-Sentences / JHMDB-Sentences evaluation, samples/s: the solo loop (forward with valid_indices + the per-sample post-processor,
one sample at a time -- the only path before clip groups took valid_indices) against video.run_annotated_frames with
A2DSentencesPostProcess(grouped=True) at G = 1, 2, 4, 8 samples per forward_group call.  8 samples per pass (distinct clips, one
annotated-frame index, captions of one token length), run lengths and read-backs included on both sides, graph replay after warm-up,
the modes interleaved round by round in ONE process; wall clock around passes that end in a device synchronise.
    python tools/a2d_group_bench.py [--reps N] [--rounds R] [--backbones a,b] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tce_rvos_amd import build_model, load_synth_weights  # noqa: E402
from tce_rvos_amd.postprocess import A2DSentencesPostProcess  # noqa: E402
from tce_rvos_amd.video import run_annotated_frames  # noqa: E402

SHAPES = {"a2d T=5 320x576 -> 240x432": (5, 320, 576, (240, 432)), "jhmdb T=5 240x320 -> 240x320": (5, 240, 320, (240, 320))}
GROUPS = (1, 2, 4, 8)
NSAMPLES = 8

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=8, help="passes of 8 samples per figure")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--backbones", default="resnet50,swin_t_p4w7")
ap.add_argument("--shapes", default=",".join(SHAPES))
ap.add_argument("--tokens", type=int, default=9)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("a2d_group_bench: needs the GPU (no timing is taken anywhere else)")

lines = [f"# python tools/a2d_group_bench.py --reps {args.reps} --rounds {args.rounds}   (one MI355X, one process, modes interleaved per round)",
         f"# solo    = for each sample: model([clip], ids, [{{size, valid_indices}}]) + A2DSentencesPostProcess() on its output",
         f"# group G = video.run_annotated_frames(model, samples, A2DSentencesPostProcess(grouped=True), max_group=G)",
         f"# {NSAMPLES} samples per pass, {args.tokens} caption tokens, text encoder inside every forward, run lengths + read-backs on both sides;",
         f"# samples/s per round = {NSAMPLES} * reps / wall seconds (host clock, device synchronised before and after); ratio = median / median"]


def emit(obj):
    s = obj if isinstance(obj, str) else json.dumps(obj)
    print(s, flush=True)
    lines.append(s)


for s in lines:
    print(s, flush=True)
for backbone in args.backbones.split(","):
    model, _, _ = build_model(argparse.Namespace(backbone=backbone, with_box_refine=True, binary=True, freeze_text_encoder=True,
                                                 f_token=8, qtrans=True, num_feature_levels=4))
    model = model.cuda().eval()
    load_synth_weights(model, 31)
    model.repack()
    for shape in args.shapes.split(","):
        T, H, W, orig = SHAPES[shape]
        g = torch.Generator().manual_seed(0)
        samples = []
        for i in range(NSAMPLES):
            ids = torch.randint(3, 50000, (1, args.tokens), generator=g)
            ids[0, 0], ids[0, -1] = 0, 2
            samples.append({"clip": torch.randn(T, 3, H, W, generator=g).cuda(), "caption": ids.cuda(), "valid_index": T // 2,
                            "orig_size": orig})
        solo_post, group_post = A2DSentencesPostProcess(), A2DSentencesPostProcess(grouped=True)

        def solo():
            res = []
            for s in samples:
                tgt = [{"size": torch.tensor([H, W]), "valid_indices": s["valid_index"]}]
                res.extend(solo_post(model([s["clip"]], s["caption"], tgt), [s["orig_size"]], [(H, W)]))
            return res

        modes = {"solo": solo}
        for G in GROUPS:
            modes[f"group{G}"] = (lambda G=G: run_annotated_frames(model, samples, group_post, max_group=G))
        first = {}
        for name, fn in modes.items():  # eager sighting, capture, replay
            for _ in range(3):
                first[name] = fn()
            torch.cuda.synchronize()
        # the results the timed passes produce: a group's masks against the solo loop's
        differ = {name: max(float((a["masks"] != b["masks"]).float().mean()) for a, b in zip(first[name], first["solo"]))
                  for name in modes if name != "solo"}
        rates = {name: [] for name in modes}
        for _ in range(args.rounds):
            for name, fn in modes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    fn()
                torch.cuda.synchronize()
                rates[name].append(round(NSAMPLES * args.reps / (time.perf_counter() - t0), 1))
        med = {name: statistics.median(v) for name, v in rates.items()}
        emit({"backbone": backbone, "shape": shape, "reps": args.reps, "samples_per_s": rates,
              "group_over_solo": {name: round(med[name] / med["solo"], 2) for name in modes if name != "solo"},
              "masks_differ_share_vs_solo_max": differ})
    del model
    torch.cuda.empty_cache()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
