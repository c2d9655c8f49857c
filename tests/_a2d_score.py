"""A2D-Sentences / JHMDB-Sentences scoring restated for the tests: the synthetic cases of tests/golden/a2d_score_cases.npz, the
fixture's reader, numpy's overlap counts, and COCOeval's mask AP (iouType='segm', useCats=0, maxDets=100; one non-crowd ground
truth per image) as plain loops over images, thresholds and detections.

The AP loops follow the published algorithm (cocoeval.py: evaluateImg, accumulate, summarize) step by step and share no code with
tce_rvos_amd.a2d_score.  They are NOT pycocotools: pycocotools is on no machine this project can use, so no AP number here or in
the fixture was ever compared with pycocotools' own output.  Pure numpy; nothing here touches the library under test."""
import math

import numpy as np

import _a2d

P_AT = (0.5, 0.6, 0.7, 0.8, 0.9)


# ----------------------------------------------------------------------------------------------------------------- the cases
def _rect(H, W, y0, y1, x0, x1):
    m = np.zeros((H, W), np.uint8)
    m[y0:y1, x0:x1] = 1
    return m


def _blob(rng, H, W):
    """a random ellipse, possibly cut by the border, with a little noise on it"""
    cy, cx, ry, rx = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(1, H / 2 + 1), rng.uniform(1, W / 2 + 1)
    y, x = np.mgrid[0:H, 0:W]
    m = (((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0)
    return (m ^ (rng.random((H, W)) < 0.03)).astype(np.uint8)


def make_cases():
    """name -> list of images {'image_id', 'size', 'gt' [H,W], 'preds' [N,H,W], 'scores' [N], 'area' or None}.  Image ids are not in
    ascending order (the precision loop goes in the ground truth's order, the AP loop in ascending id order)."""
    cases = {}
    # hand-made: a tie of the two best scores (the later one, which is NOT the better mask, must be chosen); an IoU between two of
    # the five thresholds; an empty prediction with the best score; a prediction that equals the ground truth; four sizes
    g0 = _rect(12, 17, 2, 9, 3, 12)
    g1 = _rect(9, 9, 0, 5, 0, 6)                      # 30 pixels
    p1 = _rect(9, 9, 0, 5, 0, 4)                      # 20 of them: IoU 2/3, between 0.6 and 0.7
    g2 = _rect(20, 15, 5, 15, 5, 10)
    g3 = _rect(7, 30, 1, 6, 0, 30)
    cases["hand"] = [
        {"image_id": 70, "size": (12, 17), "gt": g0, "preds": np.stack([g0, _rect(12, 17, 4, 11, 3, 12), np.zeros_like(g0)]),
         "scores": [0.9, 0.9, 0.1], "area": None},
        {"image_id": 3, "size": (9, 9), "gt": g1, "preds": np.stack([_rect(9, 9, 4, 9, 4, 9), p1, _rect(9, 9, 0, 9, 0, 9)]),
         "scores": [0.2, 0.8, 0.5], "area": None},
        {"image_id": 41, "size": (20, 15), "gt": g2, "preds": np.stack([g2, _rect(20, 15, 0, 20, 0, 15), np.zeros_like(g2)]),
         "scores": [0.3, 0.6, 0.95], "area": None},
        {"image_id": 8, "size": (7, 30), "gt": g3, "preds": np.stack([_rect(7, 30, 0, 7, 2, 30), g3, _rect(7, 30, 1, 6, 0, 29)]),
         "scores": [0.5, 0.75, 0.7], "area": None},
    ]
    rng = np.random.default_rng(20)
    ims = []
    for k, (H, W) in enumerate([(31, 44), (16, 16), (40, 30), (5, 63), (27, 27), (33, 18)]):
        gt = _blob(rng, H, W)
        if not gt.any():
            gt[H // 2, W // 2] = 1
        preds = np.stack([gt ^ (rng.random((H, W)) < f).astype(np.uint8) for f in (0.02, 0.1, 0.25)] + [_blob(rng, H, W), _blob(rng, H, W)])
        scores = np.round(rng.random(5), 2)                     # two decimals: ties across images
        ims.append({"image_id": 100 - 7 * k, "size": (H, W), "gt": gt, "preds": preds, "scores": scores.tolist(),
                    "area": [None, 900.0, 5000.0, None, 1024.0, 20000.0][k]})   # annotation areas put ground truths into S, M and L
    cases["random"] = ims
    one = _rect(3, 5, 1, 2, 1, 4)
    cases["single"] = [{"image_id": 1, "size": (3, 5), "gt": one, "preds": one[None].copy(), "scores": [0.4], "area": None}]
    return cases


def encode(mask):
    return _a2d.rle_string(_a2d.rle_counts(mask))


def load_cases(path):
    """The committed fixture -> name -> {'images': [{'image_id', 'size', 'gt' bytes, 'preds' [N bytes], 'scores', 'area'}],
    'precision' [5], 'overall_iou', 'mean_iou'} (the three as the reference's own function returned them)."""
    fx = np.load(path)
    out = {}
    for name in [str(s) for s in fx["names"]]:
        ids, sizes, areas, scores = fx[f"{name}_image_ids"], fx[f"{name}_sizes"], fx[f"{name}_areas"], fx[f"{name}_scores"]
        gb, ge = fx[f"{name}_gt"].tobytes(), fx[f"{name}_gt_ends"].tolist()
        pb, pe = fx[f"{name}_pred"].tobytes(), fx[f"{name}_pred_ends"].tolist()
        gts = [gb[a:b] for a, b in zip([0] + ge[:-1], ge)]
        prs = [pb[a:b] for a, b in zip([0] + pe[:-1], pe)]
        N = scores.shape[1]
        ims = [{"image_id": int(ids[k]), "size": [int(sizes[k, 0]), int(sizes[k, 1])], "gt": gts[k], "preds": prs[k * N:(k + 1) * N],
                "scores": [float(v) for v in scores[k]], "area": None if math.isnan(areas[k]) else float(areas[k])} for k in range(len(ids))]
        out[name] = {"images": ims, "precision": fx[f"{name}_precision"].astype(np.float64), "overall_iou": float(fx[f"{name}_overall_iou"]),
                     "mean_iou": float(fx[f"{name}_mean_iou"])}
    return out


def gt_dict(images):
    """a case's images -> the ground-truth mapping A2DScorer takes"""
    return {im["image_id"]: {"size": list(im["size"]), "counts": im["gt"], **({"area": im["area"]} if im["area"] is not None else {})}
            for im in images}


def predictions(images):
    """a case's images -> the list evaluate_a2d builds (engine.py:314-319)"""
    return [{"image_id": im["image_id"], "category_id": 1, "segmentation": {"size": list(im["size"]), "counts": c}, "score": s}
            for im in images for c, s in zip(im["preds"], im["scores"])]


def overlap_counts(pred, gt):
    """numpy's counts of [N,H,W] against [H,W]: (intersection, prediction area, ground-truth area) per prediction, int64 [N,3]"""
    p, g = np.asarray(pred) != 0, np.asarray(gt) != 0
    return np.stack([(p & g[None]).sum((1, 2)), p.sum((1, 2)), np.full(p.shape[0], g.sum())], axis=1).astype(np.int64)


def per_image_of(images):
    """a case's images (strings) -> the host functions' input, counted with numpy on planes decoded by tests/_a2d.py"""
    out = []
    for im in images:
        H, W = im["size"]
        gt = _a2d.rle_decode(_a2d.rle_from_string(im["gt"]), H, W)
        preds = np.stack([_a2d.rle_decode(_a2d.rle_from_string(c), H, W) for c in im["preds"]])
        out.append({"image_id": im["image_id"], "scores": list(im["scores"]), "counts": overlap_counts(preds, gt).tolist(), "area": im["area"]})
    return out


# ------------------------------------------------------------------------------------------------ mask AP, as plain loops
def _stable_desc(scores):
    """indices by descending score, equal scores in input order (np.argsort(-s, kind='mergesort')), as a loop-free python sort"""
    return sorted(range(len(scores)), key=lambda d: -scores[d])   # python's sort is stable


def coco_mask_ap_loops(per_image):
    """-> [mAP, AP.5, AP.75, AP small, AP medium, AP large].  per_image: dicts with 'image_id', 'scores', 'counts' [N][3], 'area'."""
    iou_thrs = [float(v) for v in np.linspace(.5, 0.95, 10)]
    rec_thrs = [float(v) for v in np.linspace(.0, 1.0, 101)]
    ranges = [(0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10)]
    images = sorted(per_image, key=lambda im: im["image_id"])
    ap = [[None] * len(ranges) for _ in iou_thrs]
    for r, (lo, hi) in enumerate(ranges):
        # evaluateImg, image by image
        evals = []
        for im in images:
            counts, scores = im["counts"], [float(s) for s in im["scores"]]
            order = _stable_desc(scores)[:100]
            g = counts[0][2] if len(counts) else 0
            g_area = im["area"] if im.get("area") is not None else g
            g_ignore = g_area < lo or g_area > hi
            ious = []
            for d in order:
                i, a = counts[d][0], counts[d][1]
                union = a + g - i
                ious.append(i / union if union != 0 else 0.0)
            dtm = [[False] * len(order) for _ in iou_thrs]
            dtig = [[False] * len(order) for _ in iou_thrs]
            for t, thr in enumerate(iou_thrs):
                taken = False
                for dind in range(len(order)):
                    iou = min(thr, 1 - 1e-10)
                    if taken:                   # the only ground truth is matched already
                        continue
                    if ious[dind] < iou:
                        continue
                    taken = True
                    dtm[t][dind] = True
                    dtig[t][dind] = g_ignore
                for dind, d in enumerate(order):
                    a = counts[d][1]
                    if not dtm[t][dind] and (a < lo or a > hi):
                        dtig[t][dind] = True
            evals.append({"scores": [scores[d] for d in order], "dtm": dtm, "dtig": dtig, "g_ignore": g_ignore})
        # accumulate
        all_scores = [s for e in evals for s in e["scores"]]
        inds = _stable_desc(all_scores)
        npig = sum(1 for e in evals if not e["g_ignore"])
        for t in range(len(iou_thrs)):
            if npig == 0:
                ap[t][r] = -1.0
                continue
            dtm = [m for e in evals for m in e["dtm"][t]]
            dtig = [g for e in evals for g in e["dtig"][t]]
            tp, fp, tp_sum, fp_sum = [], [], 0.0, 0.0
            for d in inds:
                tp_sum += 1.0 if (dtm[d] and not dtig[d]) else 0.0
                fp_sum += 1.0 if (not dtm[d] and not dtig[d]) else 0.0
                tp.append(tp_sum)
                fp.append(fp_sum)
            nd = len(tp)
            rc = [tp[k] / npig for k in range(nd)]
            pr = [tp[k] / (fp[k] + tp[k] + float(np.spacing(1))) for k in range(nd)]
            for k in range(nd - 1, 0, -1):
                if pr[k] > pr[k - 1]:
                    pr[k - 1] = pr[k]
            q = []
            for rt in rec_thrs:
                k = 0
                while k < nd and rc[k] < rt:      # searchsorted(rc, rt, side='left')
                    k += 1
                q.append(pr[k] if k < nd else 0.0)
            ap[t][r] = sum(q) / len(q)

    def over_t(r):
        vals = [ap[t][r] for t in range(len(iou_thrs)) if ap[t][r] > -1]
        return sum(vals) / len(vals) if vals else -1.0
    return [over_t(0), ap[0][0], ap[5][0], over_t(1), over_t(2), over_t(3)]
