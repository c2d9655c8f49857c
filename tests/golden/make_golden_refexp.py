"""Generates tests/golden/refexp_cases.npz: the reference's own PostProcess and PostProcessSegm (models/postprocessors.py:58-155)
run on the CPU on the cases of tests/_refexp.py, util/box_ops.generalized_box_iou on generated ground-truth boxes, and
RefExpEvaluator.summarize (datasets/refexp_eval.py) over all of the fixture's images with a small stand-in for the COCO object
(imgs, getAnnIds, loadImgs, loadAnns) -- build machine only; the reference is imported through ref_harness.  The evaluator's module
is loaded from its file (its package's __init__ imports the video datasets, which need OpenCV); it imports under the harness that
way, so the summary is the evaluator's own and the hits recorded from generalized_box_iou are checked against it.

Run from the repository root:  python tests/golden/make_golden_refexp.py
The file it writes is data.  Per case X of tests/_refexp.py CASES (c1 .. c4), B samples each:
  X_logits [B,T,N,K], X_boxes [B,T,N,4], X_masks [B,T,N,h,w] f32      inputs (torch.Generator(seed))
  X_scores [B,Q] f32, X_order [B,Q] i64, X_boxes_out [B,Q,4] f32      PostProcess' scores and boxes, and the topk_indexes behind them
  X_ref<b>, X_contested<b>                                            np.packbits of PostProcessSegm's masks [Q,H0,W0] of sample b, and
                                                                      of the pixels whose bit hangs on rounding (_a2d.contested)
  X_gt [B,4] f64 xywh, X_dataset [B], X_giou [B,Q] f32, X_hits [B,3]  the ground truth, generalized_box_iou, the hits at k = 1, 5, 10
syn_boxes [M,Q,4], syn_scores [M,Q], syn_gt [M,4], syn_dataset [M], syn_giou [M,Q], syn_hits [M,3]: a set of generated boxes.
summary [3,3]: RefExpEvaluator.summarize over all images above, rows in the order refcoco, refcoco+, refcocog.

Conditions asserted here, so that the reference alone stays inside them: neighbouring sorted sigmoid values of a sample differ by
more than SCORE_GAP; the contested share of a sample is at most _a2d.MAX_SHARE, and exactly 0 in c1 and c3; no giou and no running
maximum lies within GIOU_MARGIN of 0.5.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import _a2d  # noqa: E402
import _refexp as R  # noqa: E402
import ref_harness  # noqa: E402


class _Coco:
    """What RefExpEvaluator reads of a pycocotools COCO object: one annotation per image"""

    def __init__(self, targets):
        self.targets = targets
        self.imgs = {i: {"id": i, "dataset_name": t["dataset_name"]} for i, t in targets.items()}

    def getAnnIds(self, imgIds):
        return [imgIds]

    def loadImgs(self, image_id):
        return [self.imgs[image_id]]

    def loadAnns(self, ann_id):
        return [{"bbox": list(self.targets[ann_id]["bbox"])}]


def _giou_record(box_ops, boxes, gt_xywh):
    """generalized_box_iou as the evaluator calls it (:57-65) -> (giou [Q], hits at K_AT)"""
    conv = [gt_xywh[0], gt_xywh[1], gt_xywh[2] + gt_xywh[0], gt_xywh[3] + gt_xywh[1]]
    giou = box_ops.generalized_box_iou(boxes, torch.as_tensor(conv).view(-1, 4))[:, 0]
    best = torch.cummax(giou, 0).values
    for v in (giou, best):
        assert float((v - 0.5).abs().min()) > R.GIOU_MARGIN, "a giou within the margin of the threshold"
    return giou, [bool(max(giou[:k]) >= 0.5) for k in R.K_AT]


def main():
    ref_harness.import_reference()
    from models.postprocessors import PostProcess, PostProcessSegm
    from util import box_ops
    import importlib.util
    spec = importlib.util.spec_from_file_location("refexp_eval", os.path.join(ref_harness.REF_ROOT, "datasets", "refexp_eval.py"))
    refexp_eval = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(refexp_eval)
    RefExpEvaluator = refexp_eval.RefExpEvaluator
    out, targets, predictions = {}, {}, {}
    image_id = 0
    for name, seed, B, T, N, K, hw, sizes, origs, kind, scale, thr in R.CASES:
        Q = T * N
        logits, boxes, masks = R.make_inputs(seed, B, T, N, K, hw, kind, scale)
        outputs = {"pred_logits": logits, "pred_boxes": boxes, "pred_masks": masks}
        orig_t, size_t = torch.tensor(origs), torch.tensor(sizes)
        res = PostProcess()(outputs, orig_t)
        res = PostProcessSegm(threshold=thr)(res, outputs, orig_t, size_t)
        prob = logits.flatten(1, 2).sigmoid().view(B, -1)
        topv, topi = torch.topk(prob, k=Q, dim=1, sorted=True)                    # postprocessors.py:83
        out[f"{name}_logits"], out[f"{name}_boxes"], out[f"{name}_masks"] = logits.numpy(), boxes.numpy(), masks.numpy()
        out[f"{name}_order"] = topi.numpy()
        gts, dss, gious, hits = [], [], [], []
        for b in range(B):
            assert torch.equal(res[b]["scores"], topv[b]) and bool((res[b]["labels"] == 1).all())
            srt = prob[b].sort(descending=True).values
            assert float((srt[:-1] - srt[1:]).min()) > R.SCORE_GAP, "two scores too close: the ranking would hang on rounding"
            ref = res[b]["masks"][:, 0]
            assert ref.dtype == torch.uint8 and tuple(ref.shape) == (Q,) + tuple(origs[b])
            planes = masks[b].flatten(0, 1)[topi[b] // K]
            mine, v = _a2d.reference_post(planes, sizes[b], origs[b], threshold=thr)
            assert torch.equal(mine, ref), "the restatement is not the class"
            cont = _a2d.contested(v, thr)
            share = float(cont.float().mean())
            assert share <= _a2d.MAX_SHARE and (name not in R.EXACT or share == 0.0), (name, share)
            out[f"{name}_ref{b}"], out[f"{name}_contested{b}"] = np.packbits(ref.numpy()), np.packbits(cont.numpy())
            gt = R.make_gt(seed * 7 + b, res[b]["boxes"])
            ds = R.DATASETS[image_id % 3]
            giou, h = _giou_record(box_ops, res[b]["boxes"], gt)
            gts.append(gt), dss.append(ds), gious.append(giou.numpy()), hits.append(h)
            targets[image_id] = {"bbox": gt, "dataset_name": ds}
            predictions[image_id] = {"scores": res[b]["scores"], "boxes": res[b]["boxes"]}
            image_id += 1
            print(f"{name}[{b}]: Q={Q} K={K} order {topi[b].tolist()} contested share {share:.3e} ones {float(ref.float().mean()):.3f} "
                  f"giou {[round(float(x), 3) for x in giou]} hits {h}")
        out[f"{name}_scores"] = torch.stack([r["scores"] for r in res]).numpy()
        out[f"{name}_boxes_out"] = torch.stack([r["boxes"] for r in res]).numpy()
        out[f"{name}_gt"], out[f"{name}_dataset"] = np.asarray(gts, dtype=np.float64), np.asarray(dss)
        out[f"{name}_giou"], out[f"{name}_hits"] = np.stack(gious), np.asarray(hits)
    # the synthetic set: M images of Q boxes in a 150 x 100 image, scores descending and distinct
    M, Q = R.SYN
    g = torch.Generator().manual_seed(77)
    xy = torch.rand(M, Q, 2, generator=g) * torch.tensor([90.0, 60.0])
    wh = torch.rand(M, Q, 2, generator=g) * torch.tensor([55.0, 35.0]) + 4.0
    sboxes = torch.cat([xy, xy + wh], -1).contiguous()
    sscores = torch.rand(M, Q, generator=g).sort(1, descending=True).values
    sgt, sds, sgiou, shits = [], [], [], []
    for m in range(M):
        gt = R.make_gt(500 + m, sboxes[m])
        ds = R.DATASETS[(m * 2 + m // 5) % 3]
        giou, h = _giou_record(box_ops, sboxes[m], gt)
        sgt.append(gt), sds.append(ds), sgiou.append(giou.numpy()), shits.append(h)
        targets[image_id] = {"bbox": gt, "dataset_name": ds}
        predictions[image_id] = {"scores": sscores[m], "boxes": sboxes[m]}
        image_id += 1
    out["syn_boxes"], out["syn_scores"], out["syn_gt"] = sboxes.numpy(), sscores.numpy(), np.asarray(sgt, dtype=np.float64)
    out["syn_dataset"], out["syn_giou"], out["syn_hits"] = np.asarray(sds), np.stack(sgiou), np.asarray(shits)
    ev = RefExpEvaluator(_Coco(targets), ("bbox",), k=R.K_AT, thresh_iou=0.5)
    ev.update(predictions)
    summary = ev.summarize()
    # the evaluator's own counts against the hits recorded above
    for i, d in enumerate(R.DATASETS):
        mine = [[h for t, h in zip(targets.values(), [hh for c in R.CASES for hh in out[f"{c[0]}_hits"].tolist()] + shits)
                 if t["dataset_name"] == d]]
        want = sorted(np.mean(np.asarray(mine[0], dtype=np.float64), 0).tolist())
        assert np.allclose(summary[d], want, rtol=0, atol=1e-12), (d, summary[d], want)
    out["summary"] = np.asarray([summary[d] for d in R.DATASETS], dtype=np.float64)
    print("summary", summary, "synthetic hits per k", np.asarray(shits).sum(0).tolist(), "of", M)
    path = os.path.join(HERE, "refexp_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
