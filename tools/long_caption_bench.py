"""What a long caption costs: one clip of BASELINE config 2 frames (Swin-T, T = 5, 360 x 640, twelve RoBERTa layers, synthetic
weights) under one caption of L = 32 / 128 / 129 / 256 / 512 tokens, in one process.

  clips/s   model.forward as a graph replay (eager sighting, capture and a replay first), host clock around `reps` forwards that
            end in a device synchronise; the lengths are timed twice, alternating, so the two columns show the spread.
  text us   RoBERTa alone (text_encoder.TextPlan.forward: embeddings, twelve layers, pooler) captured into a graph of its own and
            replayed `reps` times between two device events: the time of one replay.  The resizer and the key / value projections
            of the five text cross-attention sites are NOT in it; they are in clips/s.

Up to 128 rows the dense layers are weight streams and the attention kernel holds the sentence in LDS; from 129 rows the dense
layers are tiled GEMMs and the attention kernel walks key tiles; from 33 tokens the five cross-attention sites are un-fused.
   python tools/long_caption_bench.py [--reps N] [--out profiles/FILE]"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tce_rvos_amd import build_model, load_synth_weights, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--lengths", default="32,128,129,256,512")
ap.add_argument("--thw", default="5,360,640")
ap.add_argument("--out", default=None)
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("long_caption_bench: needs the GPU (nothing is measured without one)")
model, _, _ = build_model(argparse.Namespace(backbone="swin_t_p4w7", with_box_refine=True, binary=True, freeze_text_encoder=True,
                                             f_token=8, qtrans=True, num_feature_levels=4))
model = model.cuda().eval()
load_synth_weights(model, 31)
model.repack()
T, H, W = (int(v) for v in args.thw.split(","))
LENGTHS = [int(v) for v in args.lengths.split(",")]
g = torch.Generator().manual_seed(0)
frames = torch.randn(T, 3, H, W, generator=g).cuda()
TARGET = [{"size": torch.tensor([H, W])}]


def caption(n):
    ids = torch.randint(3, 50000, (1, n), generator=g)
    ids[0, 0], ids[0, -1] = 0, 2
    return ids.cuda()


def clips_per_s(ids):
    for _ in range(3):  # eager sighting, capture, replay
        model([frames], ids, TARGET)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.reps):
        model([frames], ids, TARGET)
    torch.cuda.synchronize()
    ops.check_range(frames.device)
    return args.reps / (time.perf_counter() - t0)


def text_us(ids):
    plan = model._text_plan()
    arena = ops.Arena("cuda", 256 << 20)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad(), model.arith("text"):
        plan.forward(ids, arena.alloc)  # lazy initialisations happen here, not in the capture
        side.synchronize()
        arena.reset()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            plan.forward(ids, arena.alloc)
        for _ in range(3):
            graph.replay()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            graph.replay()
        b.record()
        b.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    return a.elapsed_time(b) * 1e3 / args.reps


caps = {n: caption(n) for n in LENGTHS}
rate = {n: [] for n in LENGTHS}
for _ in range(2):  # alternate the lengths: the second pass shows the spread
    for n in LENGTHS:
        rate[n].append(clips_per_s(caps[n]))
text = {n: [text_us(caps[n]) for _ in range(2)] for n in LENGTHS}
lines = [f"long_caption_bench: swin_t_p4w7 T {T} {H}x{W}, 12 RoBERTa layers, reps {args.reps}, {torch.cuda.get_device_name(0)}",
         "clips/s: model.forward as graph replays, host clock around a synchronise, two alternating passes; text us: one replay of",
         "RoBERTa alone (TextPlan.forward in a graph of its own), device events, two passes; graphs captured: " +
         f"{sum(1 for k in model._graphs if k[0] == 'clip')} of {len(LENGTHS)} lengths",
         "   L    clips/s  clips/s    ms/clip    text us  text us"]
for n in LENGTHS:
    mean = sum(rate[n]) / 2
    lines.append(f"{n:4d}   {rate[n][0]:8.2f} {rate[n][1]:8.2f}   {1e3 / mean:8.3f}   {text[n][0]:8.1f} {text[n][1]:8.1f}")
print("\n".join(lines), flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
