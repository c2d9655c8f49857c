"""RefCOCO evaluation of BASELINE config 1 (ResNet-50, one frame of 360 x 640), images/s: the loop a caller could write before
this stage existed -- forward / forward_group, then the torch operations of the reference's PostProcess and PostProcessSegm on
the device tensors, with its `.cpu()` of the x4 planes, its crop and nearest resize on the host, and the generalised IoU of
RefExpEvaluator on the host -- against refexp.run_images (ops.refexp_group, RefExpScorer) at max_group 1, 2, 4, 8.
8 images per pass (one shape, captions of one token length), synthetic weights, graph replay after warm-up, read-backs included on
both sides (the torch loop's are inside it; run_images' one is RefExpScorer.state() at the end of the pass), the modes interleaved
round by round in ONE process; wall clock around passes that end in a device synchronise.
    python tools/refexp_bench.py [--reps N] [--rounds R] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tce_rvos_amd import build_model, build_refexp_postprocessors, load_synth_weights, ops  # noqa: E402
from tce_rvos_amd.refexp import plan_image_groups, run_images  # noqa: E402
from tce_rvos_amd.refexp_score import RefExpScorer  # noqa: E402

H, W, ORIG = 360, 640, (480, 853)
GROUPS = (1, 2, 4, 8)
NIMAGES = 8

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=6, help="passes of 8 images per figure")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--tokens", type=int, default=9)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("refexp_bench: needs the GPU (no timing is taken anywhere else)")

lines = [f"# python tools/refexp_bench.py --reps {args.reps} --rounds {args.rounds}   (one MI355X, one process, modes interleaved per round)",
         f"# config 1: resnet50, T = 1, {H} x {W} -> {ORIG[0]} x {ORIG[1]}, {NIMAGES} images per pass, {args.tokens} caption tokens, text encoder inside",
         "# forward G  = the forwards alone (model.forward_group, G images per call), nothing behind them",
         "# torch G    = the same forwards, then per image the torch operations of postprocessors.py:72-154 on the device tensors (topk,",
         "#              gather, x4 bilinear, sigmoid > threshold, .cpu(), crop, nearest resize on the host) and generalized_box_iou on the host",
         "# images G   = refexp.run_images(max_group=G) with a RefExpScorer, its state() read back at the end of the pass",
         "# +masks / boxes: with and without the 'segm' post-processor (the torch loop: with and without lines 128-152)",
         f"# images/s per round = {NIMAGES} * reps / wall seconds (host clock, device synchronised before and after); share = 1 - rate / forward rate"]


def emit(obj):
    s = obj if isinstance(obj, str) else json.dumps(obj)
    print(s, flush=True)
    lines.append(s)


for s in lines:
    print(s, flush=True)
model, _, _ = build_model(argparse.Namespace(backbone="resnet50", with_box_refine=True, binary=True, freeze_text_encoder=True, f_token=8,
                                             qtrans=True, num_feature_levels=4))
model = model.cuda().eval()
load_synth_weights(model, 31)
model.repack()
g = torch.Generator().manual_seed(0)
samples = []
for i in range(NIMAGES):
    ids = torch.randint(3, 50000, (1, args.tokens), generator=g)
    ids[0, 0], ids[0, -1] = 0, 2
    samples.append({"image": torch.randn(3, H, W, generator=g).cuda(), "caption": ids.cuda(), "size": (H, W), "orig_size": ORIG,
                    "image_id": i, "target": {"bbox": [100.0 + 10 * i, 80.0, 300.0, 250.0], "dataset_name": "refcoco"}})
post = {True: build_refexp_postprocessors(argparse.Namespace(masks=True, threshold=0.5)),
        False: build_refexp_postprocessors(argparse.Namespace(masks=False))}


def forwards(G):
    """[(sample indices, forward_group's outputs)] of one pass"""
    out = []
    for grp in plan_image_groups([tuple(s["image"].shape) for s in samples], [args.tokens] * NIMAGES, G):
        tok = torch.cat([samples[i]["caption"] for i in grp], 0)
        out.append((grp, model.forward_group([samples[i]["image"][None] for i in grp], tok, [{"size": torch.tensor([H, W])}])))
    return out


def torch_post(o, masks, i):
    """One image through the operations of postprocessors.py:72-100 and, with masks, :128-152; engine.py's RefExpEvaluator part
    (refexp_eval.py:53-68) behind it.  Returns (result dict, hits)."""
    logits, boxes = o["pred_logits"].flatten(1, 2), o["pred_boxes"].flatten(1, 2)
    Q, K = logits.shape[1], logits.shape[2]
    vals, idx = torch.topk(logits.sigmoid().view(1, -1), k=Q, dim=1, sorted=True)
    cx, cy, w, h = boxes.unbind(-1)
    xyxy = torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)
    xyxy = torch.gather(xyxy, 1, (idx // K).unsqueeze(-1).repeat(1, 1, 4))
    xyxy = xyxy * torch.tensor([ORIG[1], ORIG[0], ORIG[1], ORIG[0]], device=xyxy.device)[None, None]
    res = {"scores": vals[0], "labels": torch.ones_like(idx[0]), "boxes": xyxy[0]}
    if masks:
        pm = o["pred_masks"].flatten(1, 2)[0][idx[0] // K][None]
        up = F.interpolate(pm, size=(pm.shape[-2] * 4, pm.shape[-1] * 4), mode="bilinear", align_corners=False)
        up = (up.sigmoid() > 0.5).cpu()
        res["masks"] = F.interpolate(up[0][:, :H, :W].unsqueeze(1).float(), size=ORIG, mode="nearest").byte()
    # the evaluator: scores and boxes to the host, the generalised IoU there
    pairs = sorted(zip(res["scores"].tolist(), res["boxes"].tolist()), reverse=True)
    b1 = torch.tensor([p[1] for p in pairs])
    t = samples[i]["target"]["bbox"]
    b2 = torch.tensor([[t[0], t[1], t[0] + t[2], t[1] + t[3]]])
    area1, area2 = (b1[:, 2] - b1[:, 0]) * (b1[:, 3] - b1[:, 1]), (b2[:, 2] - b2[:, 0]) * (b2[:, 3] - b2[:, 1])
    wh = (torch.min(b1[:, None, 2:], b2[:, 2:]) - torch.max(b1[:, None, :2], b2[:, :2])).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    union = area1[:, None] + area2 - inter
    wh = (torch.max(b1[:, None, 2:], b2[:, 2:]) - torch.min(b1[:, None, :2], b2[:, :2])).clamp(min=0)
    area = wh[:, :, 0] * wh[:, :, 1]
    giou = (inter + 1e-6) / (union + 1e-6) - ((area - union) + 1e-6) / (area + 1e-6)
    return res, [bool(max(giou[:k]) >= 0.5) for k in (1, 5, 10)]


def torch_loop(G, masks):
    return [torch_post(o, masks, i) for grp, outs in forwards(G) for i, o in zip(grp, outs)]


def images(G, masks):
    scorer = RefExpScorer()
    res = run_images(model, samples, post[masks], max_group=G, scorer=scorer)
    return res, scorer.state()


modes = {}
for G in (1, 8):
    modes[f"forward{G}"] = (lambda G=G: forwards(G))
for masks, tag in ((True, "+masks"), (False, " boxes")):
    for G in (1, 8):
        modes[f"torch{G}{tag}"] = (lambda G=G, masks=masks: torch_loop(G, masks))
    for G in GROUPS:
        modes[f"images{G}{tag}"] = (lambda G=G, masks=masks: images(G, masks))
first = {}
for name, fn in modes.items():  # eager sighting, capture, replay
    for _ in range(3):
        first[name] = fn()
    torch.cuda.synchronize()
# what the timed passes produce: run_images against the torch loop at the same group size
mine, theirs = first["images8+masks"][0], first["torch8+masks"]
agree = {"masks_differ_share_max": max(float((mine[i]["masks"].cpu() != theirs[i][0]["masks"]).float().mean()) for i in range(NIMAGES)),
         "scores_max_abs_diff": max(float((mine[i]["scores"] - theirs[i][0]["scores"]).abs().max()) for i in range(NIMAGES)),
         "boxes_max_abs_diff": max(float((mine[i]["boxes"] - theirs[i][0]["boxes"]).abs().max()) for i in range(NIMAGES))}
rates = {name: [] for name in modes}
for _ in range(args.rounds):
    for name, fn in modes.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        torch.cuda.synchronize()
        rates[name].append(round(NIMAGES * args.reps / (time.perf_counter() - t0), 1))
med = {name: statistics.median(v) for name, v in rates.items()}
emit({"images_per_s": rates})
emit({"median_images_per_s": med})
share = {}
for name in modes:
    G = "".join(ch for ch in name if ch.isdigit())
    if not name.startswith("forward") and f"forward{G}" in med:
        share[name] = round(1 - med[name] / med[f"forward{G}"], 3)
emit({"output_stage_share_of_wall": share})
emit({"images_over_torch": {f"G{G}{tag}": round(med[f"images{G}{tag}"] / med[f"torch{G}{tag}"], 2) for tag in ("+masks", " boxes") for G in (1, 8)}})
emit({"agreement_of_the_timed_results_at_G8": agree})

# the stage's own launches: N back-to-back ops.refexp_group calls on one group of 8 between two device events (launch overhead
# included: the figure is a call's time on a busy stream, not a kernel time)
outs = [o for _, group in forwards(8) for o in group]
lg = [o["pred_logits"][0].flatten(0, 1).contiguous() for o in outs]
bx = [o["pred_boxes"][0].flatten(0, 1).contiguous() for o in outs]
pm = [o["pred_masks"][0].flatten(0, 1).contiguous() for o in outs]
N = 200
own = {}
for tag, call in (("rank launch, 8 images", lambda: ops.refexp_group(lg, bx, None, None, [ORIG] * 8)),
                  ("rank + masks launches, 8 images", lambda: ops.refexp_group(lg, bx, pm, [(H, W)] * 8, [ORIG] * 8))):
    for _ in range(10):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(N):
        call()
    e1.record()
    torch.cuda.synchronize()
    own[tag] = round(e0.elapsed_time(e1) / N * 1e3, 1)
emit({"microseconds_per_call_device_events_200_calls": own,
      "mask_bytes_written_per_call": 8 * int(lg[0].shape[0]) * ORIG[0] * ORIG[1]})
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
