"""A2D-Sentences / JHMDB-Sentences scoring of masks that stay on the GPU: what the reference does after its post-processor
(engine.py:321-353: COCOeval with iouType='segm', useCats=0, and datasets/a2d_eval.py) -- P@0.5 .. P@0.9, overall IoU, mean IoU and
mask AP -- without pycocotools and without decoding a run-length string on the host.

The pixel work is two library calls per image (include/tce_rvos_score.h): ops.rle_decode turns the ground truth's run lengths
(and, for saved prediction files, the predictions') into planes, ops.mask_overlap counts per prediction the intersection, its own
area and the ground truth's.  Three integers per prediction and its score wait in device slabs; state() reads them back, once.
Everything after the counts is host arithmetic on integers, restated from the reference operation by operation:
precision_iou_metrics is a2d_eval.py:20-45, coco_mask_ap is COCOeval specialised to one non-crowd ground truth per image.

What is NOT verified: pycocotools exists on no machine this project can use, so coco_mask_ap is held to a plain-loop restatement
of the published algorithm (tests/_a2d_score.py) and to cases derived by hand, not to pycocotools' own output.
precision_iou_metrics is held to the reference's own function (tests/golden/a2d_score_cases.npz).

Limits and deviations: every image takes the same number N of predictions (the model's queries; the reference takes any number);
each image_id has exactly one non-crowd annotation (a2d_eval.py:26 assumes the same); planes stay below 2^24 pixels for
bit-identical IoUs (the reference sums 0/1 pixels in float32, exact only up to there); scores wait as float64, so float32 scores
and the Python floats of a saved file both keep their order and ties."""
import json

import numpy as np
import torch

from . import ops

AP_LABELS = ("mAP 0.5:0.95", "AP 0.5", "AP 0.75", "AP 0.5:0.95 S", "AP 0.5:0.95 M", "AP 0.5:0.95 L")  # engine.py:346
P_AT = (0.5, 0.6, 0.7, 0.8, 0.9)                                                                      # a2d_eval.py:22
AREA_RANGES = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))            # all, S, M, L
MAX_DETS = 100


def rle_from_string(s):
    """cocoapi rleFrString: bytes or str -> int64 array of run lengths; the inverse of postprocess.rle_to_string.

    A character is c = byte - 48: five value bits (c & 0x1f, low group first), bit 5 = another group follows; when the last group of
    a value has bit 4 set the value is sign-extended; value i > 2 is a difference against counts[i-2].  Vectorised like its twin: the
    groups of a value are gathered with one reduceat, the differences undone with one cumulative sum per parity."""
    b = np.frombuffer(s.encode("ascii") if isinstance(s, str) else bytes(s), dtype=np.uint8).astype(np.int64) - 48
    if b.size == 0:
        return np.zeros(0, dtype=np.int64)
    if (b < 0).any() or (b > 63).any():
        raise ValueError("rle_from_string: not a COCO run-length string")
    last = (b & 0x20) == 0                                    # the last group of its value
    if not last[-1]:
        raise ValueError("rle_from_string: the string ends inside a value")
    start = np.flatnonzero(np.concatenate(([True], last[:-1])))     # the first group of every value
    k = np.arange(b.size) - np.repeat(start, np.diff(np.append(start, b.size)))  # the group's rank in its value
    if int(k.max()) > 12:
        raise ValueError("rle_from_string: a value of more than 13 groups")
    x = np.bitwise_or.reduceat((b & 0x1f) << (5 * k), start)
    end = np.flatnonzero(last)
    neg = (b[end] & 0x10) != 0
    x = np.where(neg, x | (np.int64(-1) << (5 * (k[end] + 1))), x)
    x[1::2] = np.cumsum(x[1::2])                               # counts[1], counts[3] = x[3] + counts[1], ...
    x[2::2] = np.cumsum(x[2::2])                               # counts[2], counts[4] = x[4] + counts[2], ...; counts[0] stands alone
    return x


def _chosen(scores):
    """sorted(preds, key=score)[-1] (a2d_eval.py:30): a stable ascending sort, so of several maxima the LAST in input order"""
    s = np.asarray(scores, dtype=np.float64)
    return int(s.size - 1 - np.argmax(s[::-1]))


def precision_iou_metrics(per_image):
    """a2d_eval.py:20-45 on integer counts.  per_image: one dict per image, in the order of the ground truth's images, with
    'scores' [N] and 'counts' [N,3] = (intersection, prediction area, ground-truth area) per prediction
    -> (precision_at_k float64 [5], overall_iou, mean_iou).
    The prediction of an image is the last of its score maxima; iou = (float32(I) + float32(1e-6)) / (float32(U) + float32(1e-6))
    in float32 with U = a + g - I (compute_iou :12-17; bit-identical for planes below 2^24 pixels, where float32 holds the sums
    exactly); `iou > k` is strict; totals and the mean are Python floats in image order."""
    counters = {k: 0 for k in P_AT}
    total_i, total_u, ious = 0.0, 0.0, []
    eps = np.float32(1e-6)
    for im in per_image:
        c = np.asarray(im["counts"], dtype=np.int64).reshape(-1, 3)
        i, a, g = (int(v) for v in c[_chosen(im["scores"])])
        u = a + g - i
        iou = float((np.float32(i) + eps) / (np.float32(u) + eps))
        for k in counters:
            if iou > k:
                counters[k] += 1
        total_i += float(i)
        total_u += float(u)
        ious.append(iou)
    if not ious:
        raise ValueError("precision_iou_metrics: no image")
    precision_at_k = np.array(list(counters.values())) / len(ious)
    return precision_at_k, total_i / total_u, float(np.mean(ious))


def coco_mask_ap(per_image):
    """COCOeval (iouType='segm', useCats=0, maxDets=100) specialised to one non-crowd ground truth per image, on integer counts.
    per_image: as precision_iou_metrics, each dict with 'image_id' and optionally 'area' (the annotation's; else the ground
    truth's pixel count) -> float64 [6]: mAP 0.5:0.95, AP 0.5, AP 0.75, and AP 0.5:0.95 of the small, medium and large ranges
    (-1 for a range no ground truth lies in).

    Per image (ascending image_id): u_d = I / (a_d + g - I) in double (0 for an empty union); detections by descending score
    (stable), the first 100.  At threshold t a detection matches when the ground truth is still free and u_d >= min(t, 1 - 1e-10),
    so the first such detection takes it.  A matched detection is ignored when the ground truth is (its area outside the range), an
    unmatched one when its own area is.  Per (t, range): all kept detections by descending score (stable), tp / fp cumulated in
    float64, recall = tp / #ground truths not ignored, precision = tp / (tp + fp + spacing(1)) made non-increasing from the
    right and sampled at the first recall >= each of linspace(0, 1, 101), 0 beyond the last; AP = the mean of the samples."""
    ims = sorted(per_image, key=lambda im: im["image_id"])
    thr = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
    rec = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
    T, R = len(thr), len(AREA_RANGES)
    scores, matched, ignored = [], [], []
    npig = np.zeros(R, dtype=np.int64)
    for im in ims:
        c = np.asarray(im["counts"], dtype=np.int64).reshape(-1, 3)
        s = np.asarray(im["scores"], dtype=np.float64).reshape(-1)
        order = np.argsort(-s, kind="mergesort")[:MAX_DETS]
        i, a = c[order, 0].astype(np.float64), c[order, 1].astype(np.float64)
        g = float(c[0, 2]) if len(c) else 0.0
        union = a + g - i
        u = np.divide(i, union, out=np.zeros_like(i), where=union != 0)
        ok = u[None, :] >= np.minimum(thr, 1 - 1e-10)[:, None]                     # [T,D]
        m = np.zeros((T, len(order)), dtype=bool)
        if len(order):
            m[np.arange(T), ok.argmax(1)] = ok.any(1)                                # the first detection that reaches t
        garea = float(im["area"]) if im.get("area") is not None else g
        ig = np.zeros((R, T, len(order)), dtype=bool)
        for r, (lo, hi) in enumerate(AREA_RANGES):
            gig = garea < lo or garea > hi
            npig[r] += not gig
            ig[r] = np.where(m, gig, ((a < lo) | (a > hi))[None, :])
        scores.append(s[order])
        matched.append(m)
        ignored.append(ig)
    if not ims:
        raise ValueError("coco_mask_ap: no image")
    scores, matched, ignored = np.concatenate(scores), np.concatenate(matched, axis=1), np.concatenate(ignored, axis=2)
    inds = np.argsort(-scores, kind="mergesort")
    matched, ignored = matched[:, inds], ignored[:, :, inds]
    ap = -np.ones((T, R))
    for r in range(R):
        if npig[r] == 0:
            continue
        tps = np.cumsum(matched & ~ignored[r], axis=1).astype(np.float64)
        fps = np.cumsum(~matched & ~ignored[r], axis=1).astype(np.float64)
        for t in range(T):
            tp, fp = tps[t], fps[t]
            rc = tp / npig[r]
            pr = tp / (fp + tp + np.spacing(1))
            pr = np.maximum.accumulate(pr[::-1])[::-1]
            at = np.searchsorted(rc, rec, side="left")
            q = np.zeros(len(rec))
            q[at < len(pr)] = pr[at[at < len(pr)]]
            ap[t, r] = q.mean()

    def over_t(r):
        return float(ap[:, r].mean()) if npig[r] else -1.0
    return np.array([over_t(0), ap[0, 0], ap[5, 0], over_t(1), over_t(2), over_t(3)], dtype=np.float64)


def _annotation(image_id, entry):
    """One image's ground truth -> (H, W, counts source, area or None); exactly one non-crowd run-length annotation"""
    anns = list(entry) if isinstance(entry, (list, tuple)) else [entry]
    if len(anns) != 1:
        raise ValueError(f"A2DScorer: image {image_id!r} has {len(anns)} annotations, exactly one is expected (a2d_eval.py:26)")
    ann = anns[0]
    if int(ann.get("iscrowd", 0) or 0) != 0:
        raise ValueError(f"A2DScorer: image {image_id!r}: crowd annotations are not supported")
    seg = ann["segmentation"] if "segmentation" in ann else ann
    if not isinstance(seg, dict) or "size" not in seg or "counts" not in seg:
        raise ValueError(f"A2DScorer: image {image_id!r}: the annotation must be a run-length mask {{'size', 'counts'}}")
    return int(seg["size"][0]), int(seg["size"][1]), seg["counts"], ann.get("area")


def _counts_of(counts):
    """'counts' of a run-length dict (the compressed string, or the uncompressed list of integers) -> uint32-ranged int64 array"""
    c = rle_from_string(counts) if isinstance(counts, (bytes, bytearray, str)) else np.asarray(counts, dtype=np.int64).reshape(-1)
    if c.size and (int(c.min()) < 0 or int(c.max()) >= 2 ** 32):
        raise ValueError("A2DScorer: a run length outside 32 bits")
    return c


def _host_id(image_id):
    if torch.is_tensor(image_id):
        if image_id.is_cuda:
            raise ValueError("A2DScorer: image ids must be host values (reading one back would synchronise)")
        return image_id.item()
    return image_id


class A2DScorer:
    """Collects the counts and scores of one evaluation; see the module docstring.
    gt: image_id -> {'size': [H,W], 'counts': bytes|str} with optional 'area' (or a COCO annotation dict holding these under
    'segmentation', or a list of one such).  The order of gt is the reference's image order (coco_gt.imgs)."""

    def __init__(self, gt, device="cuda"):
        self.gt = {}
        for image_id, entry in gt.items():
            self.gt[image_id] = _annotation(image_id, entry)
        self.device = torch.device(device)
        self.N, self._ids, self._seen = None, [], set()
        self._counts = self._scores = None          # device slabs int32 [capacity,N,3] and float64 [capacity,N]
        self._merged = None

    @classmethod
    def from_coco_json(cls, path, device="cuda"):
        """The *_annotations_in_coco_format.json the reference loads (engine.py:333-337)"""
        with open(path) as f:
            data = json.load(f)
        gt = {im["id"]: [] for im in data.get("images", [])}
        for ann in data["annotations"]:
            gt.setdefault(ann["image_id"], []).append(ann)
        return cls(gt, device=device)

    # ------------------------------------------------------------------------------------------------------------ collecting
    def _slot(self, image_id, N, size):
        """Checks of one image, and its row of the slabs (grown by doubling: device copies, no read-back)"""
        if image_id not in self.gt:
            raise ValueError(f"A2DScorer: unknown image_id {image_id!r}")
        if image_id in self._seen:
            raise ValueError(f"A2DScorer: image_id {image_id!r} was scored already")
        H, W = self.gt[image_id][:2]
        if (int(size[0]), int(size[1])) != (H, W):
            raise ValueError(f"A2DScorer: image {image_id!r}: masks of size {tuple(int(v) for v in size)}, ground truth of {(H, W)}")
        if self.N is None:
            self.N = N
            self._counts = torch.empty(16, N, 3, dtype=torch.int32, device=self.device)
            self._scores = torch.empty(16, N, dtype=torch.float64, device=self.device)
        if N != self.N:
            raise ValueError(f"A2DScorer: image {image_id!r} has {N} predictions, earlier images had {self.N}")
        k = len(self._ids)
        if k == self._counts.shape[0]:
            counts, scores = self._counts.new_empty(2 * k, N, 3), self._scores.new_empty(2 * k, N)
            counts[:k].copy_(self._counts)
            scores[:k].copy_(self._scores)
            self._counts, self._scores = counts, scores
        return k

    def _upload_runs(self, rows):
        """Run lengths of several masks as ONE upload: int32 [P + P*stride] = nruns, then the rows padded to the longest"""
        stride = max(1, max(len(r) for r in rows))
        buf = np.zeros(len(rows) + len(rows) * stride, dtype=np.uint32)
        for p, r in enumerate(rows):
            buf[p] = len(r)
            buf[len(rows) + p * stride:len(rows) + p * stride + len(r)] = r
        dev = torch.from_numpy(buf.view(np.int32)).to(self.device)
        return dev[len(rows):].view(len(rows), stride), dev[:len(rows)]

    def _commit(self, image_id, k):
        self._ids.append(image_id)
        self._seen.add(image_id)
        self._merged = None

    @torch.no_grad()
    def update(self, image_ids, processed):
        """image_ids and what A2DSentencesPostProcess.forward returned for them ('scores' [N], 'masks' uint8 [N,1,H,W] on the
        GPU; 'rle_masks' is not looked at, so rle=False serves).  Per sample one small upload (the ground truth's run lengths), one
        rle_decode, one mask_overlap into the slab, one copy of the scores beside it: no read-back, no synchronisation."""
        image_ids, processed = list(image_ids), list(processed)
        if len(image_ids) != len(processed):
            raise ValueError(f"A2DScorer.update: {len(image_ids)} image ids, {len(processed)} results")
        for image_id, p in zip(image_ids, processed):
            image_id = _host_id(image_id)
            masks, scores = p["masks"], p["scores"]
            if masks.dim() != 4 or masks.shape[1] != 1 or masks.dtype != torch.uint8 or not masks.is_cuda:
                raise ValueError("A2DScorer.update: 'masks' must be uint8 [N,1,H,W] on the GPU")
            pred = masks[:, 0]
            N = int(pred.shape[0])
            if tuple(scores.shape) != (N,):
                raise ValueError(f"A2DScorer.update: 'scores' must be [{N}], got {tuple(scores.shape)}")
            k = self._slot(image_id, N, pred.shape[1:])
            H, W, src, _ = self.gt[image_id]
            counts, nruns = self._upload_runs([_counts_of(src)])
            plane = ops.rle_decode(counts, nruns, (H, W))
            ops.mask_overlap(pred.contiguous(), plane[0], counts=self._counts[k])
            self._scores[k].copy_(scores)
            self._commit(image_id, k)

    @torch.no_grad()
    def update_rle(self, predictions):
        """predictions: the list of {'image_id', 'segmentation': {'size', 'counts'}, 'score'} dicts evaluate_a2d builds
        (engine.py:314-319), e.g. a saved predictions file.  Grouped by image in order of appearance; per image ONE rle_decode
        over its N prediction strings and the ground truth's (P = N + 1), then as update."""
        groups = {}
        for pr in predictions:
            groups.setdefault(_host_id(pr["image_id"]), []).append(pr)
        for image_id, prs in groups.items():
            N = len(prs)
            sizes = {(int(pr["segmentation"]["size"][0]), int(pr["segmentation"]["size"][1])) for pr in prs}
            if len(sizes) != 1:
                raise ValueError(f"A2DScorer.update_rle: image {image_id!r}: predictions of sizes {sorted(sizes)}")
            k = self._slot(image_id, N, next(iter(sizes)))
            H, W, src, _ = self.gt[image_id]
            counts, nruns = self._upload_runs([_counts_of(pr["segmentation"]["counts"]) for pr in prs] + [_counts_of(src)])
            planes = ops.rle_decode(counts, nruns, (H, W))
            ops.mask_overlap(planes[:N], planes[N], counts=self._counts[k])
            self._scores[k].copy_(torch.tensor([float(pr["score"]) for pr in prs], dtype=torch.float64))
            self._commit(image_id, k)

    # ------------------------------------------------------------------------------------------------------------- reporting
    def state(self):
        """The one read-back: {'image_ids', 'scores' [K][N], 'counts' [K][N][3]} of what this scorer collected, plain Python
        (picklable; what a rank hands to all_gather)."""
        K = len(self._ids)
        if K == 0:
            return {"image_ids": [], "scores": [], "counts": []}
        both = torch.cat([self._scores[:K].unsqueeze(-1), self._counts[:K].to(torch.float64)], dim=-1).cpu().numpy()
        return {"image_ids": list(self._ids), "scores": both[..., 0].tolist(), "counts": both[..., 1:].astype(np.int64).tolist()}

    def merge(self, states):
        """Combines the states of several ranks (the job of utils.all_gather at engine.py:322) into the one summarize() reports;
        returns it (image_ids in the order of gt, whatever the order of the states).  An image in several states -- a sampler's
        padding -- is kept once if its scores and counts are identical, otherwise ValueError."""
        got = {}
        for st in states:
            for image_id, s, c in zip(st["image_ids"], st["scores"], st["counts"]):
                if image_id not in self.gt:
                    raise ValueError(f"A2DScorer.merge: unknown image_id {image_id!r}")
                s, c = [float(v) for v in s], [[int(v) for v in row] for row in c]
                if image_id in got and got[image_id] != (s, c):
                    raise ValueError(f"A2DScorer.merge: image_id {image_id!r} comes with different results from two states")
                got[image_id] = (s, c)
        ids = [i for i in self.gt if i in got]
        self._merged = {"image_ids": ids, "scores": [got[i][0] for i in ids], "counts": [got[i][1] for i in ids]}
        return self._merged

    def per_image(self):
        """The host functions' input, in the order of gt: merge()'s result if there is one, else this scorer's own state()"""
        st = self._merged if self._merged is not None else self.state()
        at = {image_id: k for k, image_id in enumerate(st["image_ids"])}
        missing = [i for i in self.gt if i not in at]
        if missing:
            raise ValueError(f"A2DScorer: {len(missing)} images of the ground truth have no predictions (first: {missing[0]!r})")
        return [{"image_id": i, "scores": st["scores"][at[i]], "counts": st["counts"][at[i]], "area": self.gt[i][3]} for i in self.gt]

    def summarize(self):
        """The dict of engine.py:346-352, same keys"""
        per_image = self.per_image()
        res = {label: float(v) for label, v in zip(AP_LABELS, coco_mask_ap(per_image))}
        precision_at_k, overall_iou, mean_iou = precision_iou_metrics(per_image)
        res.update({f"P@{k}": float(m) for k, m in zip(P_AT, precision_at_k)})
        res.update({"overall_iou": overall_iou, "mean_iou": mean_iou})
        return res
