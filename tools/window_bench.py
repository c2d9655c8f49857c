"""Context-frame windows over one video: video.run_video_windows at windows_per_forward 1 / 4 / 8 against the loop a caller would
write by hand with what existed before the driver -- per (caption, window) one model([frames[ids]], ...) on the widened clip,
ops.select_masks over the WHOLE clip, a slice of the kept planes.  Config-2 frames (Swin-T, 360 x 640, origin 720 x 1280), a 40-frame
video, num_frames 5, f_extra 0 / 1 / 2, one caption of 9 tokens and five captions of 6 / 9 / 9 / 14 / 14 tokens (two shared pairs and
one caption alone).  Every variant is warmed (eager sighting, capture, replay) right before it is timed, because the graph cache
holds fewer shapes than the table has; the variants of a row are timed twice, alternating, inside this one process.  Host clock
around a synchronise; no profiler.  The share="frames" driver (model.forward_indexed over each forward's pool of distinct frames,
DESIGN 3.19) runs at max_pairs 4 / 8 beside them; its rows are judged against "driver wpf=4" (the default plan): faster only if the
ratio of means exceeds 1.05 and the two passes of the two variants do not overlap.  Per variant and video: the graph shapes one
video asks for, and the graphs captured DURING the timed videos (all shapes were warm: a capture there is an eviction inside a video).
   python tools/window_bench.py [--reps N] [--out FILE] [--only NAME,NAME]"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tce_rvos_amd import build_model, load_synth_weights, ops  # noqa: E402
from tce_rvos_amd.video import plan_windows, run_video_windows  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--frames", type=int, default=40)
ap.add_argument("--hw", default="360,640")
ap.add_argument("--origin", default="720,1280")
ap.add_argument("--out", default=None)
ap.add_argument("--only", default=None, help="comma list of variant names (the hand loop always runs: it is the reference)")
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("window_bench: needs the GPU (nothing is measured without one)")
model, _, _ = build_model(argparse.Namespace(backbone="swin_t_p4w7", with_box_refine=True, binary=True, freeze_text_encoder=True,
                                             f_token=8, qtrans=True, num_feature_levels=4))
model = model.cuda().eval()
load_synth_weights(model, 31)
model.repack()
N, NF = args.frames, 5
H, W = (int(v) for v in args.hw.split(","))
ORIGIN = tuple(int(v) for v in args.origin.split(","))
g = torch.Generator().manual_seed(0)
frames = torch.randn(N, 3, H, W, generator=g).cuda()
TARGET = [{"size": torch.tensor([H, W])}]


def captions(lens):
    caps = []
    for n in lens:
        ids = torch.randint(3, 50000, (1, n), generator=g)
        ids[0, 0], ids[0, -1] = 0, 2
        caps.append(ids)
    return caps


def hand_loop(caps, e):
    """what exists without the driver: a forward per (caption, window), the whole widened clip rendered, the kept planes sliced"""
    plan = plan_windows(N, NF, e)
    idx = [torch.tensor(w[0], device="cuda") for w in plan]
    res = []
    for cap in caps:
        parts = []
        for (ids, first, count, lo), ix in zip(plan, idx):
            out = model([frames.index_select(0, ix)], cap, TARGET)
            m, _ = ops.select_masks(out["pred_logits"][0], out["pred_masks"][0], ORIGIN)
            parts.append(m[first:first + count])
        res.append(torch.cat(parts, 0))
    ops.check_range(frames.device)
    return res


def driver(wpf):
    def run(caps, e):
        return [r["masks"] for r in run_video_windows(model, frames, caps, ORIGIN, NF, e, windows_per_forward=wpf)]
    return run


def frames_driver(mp):
    def run(caps, e):
        return [r["masks"] for r in run_video_windows(model, frames, caps, ORIGIN, NF, e, share="frames", max_pairs=mp)]
    return run


VARIANTS = [("hand loop", hand_loop), ("driver wpf=1", driver(1)), ("driver wpf=4", driver(4)), ("driver wpf=8", driver(8)),
            ("frames mp=4", frames_driver(4)), ("frames mp=8", frames_driver(8))]
if args.only:
    VARIANTS = [v for v in VARIANTS if v[0] == "hand loop" or v[0] in args.only.split(",")]
BASE = "driver wpf=4"  # the default plan: what share="frames" is judged against
# graph shapes a video asks for / graphs captured while it is timed
shapes, captured = set(), [0]
_want, _capture = model._want_graph, model._capture
model._want_graph = lambda key: (shapes.add(key), _want(key))[1]
model._capture = lambda *a, **k: (captured.__setitem__(0, captured[0] + 1), _capture(*a, **k))[1]
lines = [f"window_bench: swin_t_p4w7 {H}x{W} -> {ORIGIN[0]}x{ORIGIN[1]}, {N} frames, num_frames {NF}, reps {args.reps}, "
         f"{torch.cuda.get_device_name(0)}",
         "frames/s = video frames that got a mask, per second, summed over the captions; two alternating passes per variant"]
for lens in ([9], [6, 9, 9, 14, 14]):
    caps = captions(lens)
    for e in (0, 1, 2):
        ref, fps, graphs = None, {name: [] for name, _ in VARIANTS}, {}
        for _ in range(2):  # alternate the variants: the second pass shows the spread
            for name, fn in VARIANTS:
                try:
                    for _ in range(3):  # eager sighting, capture, replay
                        got = fn(caps, e)
                    torch.cuda.synchronize()
                    if ref is None:
                        ref = got
                    same = sum(int((a != b).sum()) for a, b in zip(got, ref))  # pixels that differ from the hand loop's
                    shapes.clear()
                    captured[0] = 0
                    t0 = time.perf_counter()
                    for _ in range(args.reps):
                        fn(caps, e)
                    torch.cuda.synchronize()
                    dt = (time.perf_counter() - t0) / args.reps
                    graphs[name] = (len(shapes), max(captured[0], graphs.get(name, (0, 0))[1]))
                    fps[name].append((N * len(caps) / dt, same))
                except torch.cuda.OutOfMemoryError as err:  # a group too large for the card's free memory: reported, not timed
                    fps[name].append((float("nan"), -1))
                    print(f"{name}: out of memory ({str(err)[:80]})", flush=True)
        base = sum(v for v, _ in fps["hand loop"]) / 2
        lines.append(f"captions {lens} f_extra {e} (clips of {NF + 2 * e}):")
        for name, _ in VARIANTS:
            mean = sum(v for v, _ in fps[name]) / 2
            lines.append(f"  {name:13s} {fps[name][0][0]:8.1f} {fps[name][1][0]:8.1f} frames/s   x{mean / base:5.3f} of the hand loop   "
                         f"{max(s for _, s in fps[name])} of {N * len(caps) * ORIGIN[0] * ORIGIN[1]} mask pixels differ from the hand loop's")
            if name in graphs:
                lines[-1] += f"   {graphs[name][0]} graph shapes per video, {graphs[name][1]} captured while timed"
            if name.startswith("frames") and BASE in fps:
                mine, theirs = [v for v, _ in fps[name]], [v for v, _ in fps[BASE]]
                ratio = mean / (sum(theirs) / 2)
                faster = ratio > 1.05 and min(mine) > max(theirs)
                lines[-1] += f"   x{ratio:5.3f} of {BASE}: {'faster' if faster else 'NOT faster'}"
        print("\n".join(lines[-(1 + len(VARIANTS)):]), flush=True)
        if args.out:  # after every row: a later failure keeps what was measured
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
