"""RefCOCO / RefCOCO+ / RefCOCOg precision@k of boxes that stay on the GPU: what the reference's RefExpEvaluator does with the
results of PostProcess (datasets/refexp_eval.py:37-82, fed by engine.py:122-126).

Per update call one launch (ops.refexp_giou, include/tce_rvos_refexp.h): the generalised IoU of every predicted box of every image of
the call against the image's one ground-truth box, and its running maximum over the boxes in score order.  The running maxima
`best [Q]` of every image wait in a device slab (one slab per box count Q: a model's queries give one); state() reads a slab
back once.  What follows is host arithmetic on those floats:
an image is a hit at k when best[min(k, Q) - 1] >= thresh_iou (refexp_eval.py:66-68: max(giou[:k]) >= thresh_iou), compared in
float32 as torch compares a float32 tensor with a Python number; a dataset's precision is hits / images; summarize() returns per
dataset the values sorted ascending, as the reference does (:79), zeros for a dataset without an image.

Deviations from the reference:
  * exact score ties keep the post-processor's order (ties there go to the lower candidate index); the reference re-sorts
    (score, box) tuples, so among equal scores the box with the larger coordinates comes first;
  * a ground-truth box of negative width or height is a ValueError at update; the reference asserts inside generalized_box_iou.
Results that did not come from postprocess.PostProcess are put in descending score order first (a stable sort on the device)."""
import numpy as np
import torch

from . import ops

DATASETS = ("refcoco", "refcoco+", "refcocog")  # refexp_eval.py:39-43


def _host_id(image_id):
    if torch.is_tensor(image_id):
        if image_id.is_cuda:
            raise ValueError("RefExpScorer: image ids must be host values (reading one back would synchronise)")
        return image_id.item()
    return image_id


def _target(image_id, entry):
    """One image's ground truth -> (dataset name, [x0, y0, x1, y1] as the reference converts it at :59-64)"""
    anns = list(entry) if isinstance(entry, (list, tuple)) else [entry]
    if len(anns) != 1:
        raise ValueError(f"RefExpScorer: image {image_id!r} has {len(anns)} targets, exactly one is expected (refexp_eval.py:47)")
    t = anns[0]
    if "bbox" not in t or "dataset_name" not in t:
        raise ValueError(f"RefExpScorer: image {image_id!r}: a target is {{'bbox': [x, y, w, h], 'dataset_name': ...}}")
    name = t["dataset_name"]
    if name not in DATASETS:
        raise ValueError(f"RefExpScorer: image {image_id!r}: dataset_name {name!r} is none of {DATASETS}")
    bb = t["bbox"].tolist() if hasattr(t["bbox"], "tolist") else list(t["bbox"])
    if len(bb) != 4:
        raise ValueError(f"RefExpScorer: image {image_id!r}: bbox must be [x, y, w, h]")
    x, y, w, h = (float(v) for v in bb)
    if not (w >= 0 and h >= 0):
        raise ValueError(f"RefExpScorer: image {image_id!r}: ground-truth box of width {w} and height {h}")
    return name, [x, y, w + x, h + y]


def hits(best, k, thresh_iou):
    """best: one image's running maxima [Q] -> the hit (bool) at every k of `k`"""
    b = np.asarray(best, dtype=np.float32).reshape(-1)
    return [bool(b[min(int(kk), b.size) - 1] >= np.float32(thresh_iou)) for kk in k]


class RefExpScorer:
    """Collects the running maxima of one evaluation; see the module docstring."""

    def __init__(self, k=(1, 5, 10), thresh_iou=0.5, device="cuda"):
        if not isinstance(k, (list, tuple)) or not k or any(int(v) < 1 for v in k):
            raise ValueError("RefExpScorer: k must be a non-empty list or tuple of positive integers")
        self.k, self.thresh_iou = tuple(int(v) for v in k), float(thresh_iou)
        self.device = torch.device(device)
        self._ids, self._names, self._seen = [], [], set()
        self._at = []       # per image (Q, its row of the slab of Q)
        self._best = {}     # Q -> [device slab float32 [capacity,Q], rows in use]
        self._merged = None

    # ------------------------------------------------------------------------------------------------------------ collecting
    def _room(self, Q, M):
        """Rows k .. k+M of the slab of Q (grown by doubling: a device copy, no read-back)"""
        ent = self._best.setdefault(Q, [torch.empty(max(16, M), Q, dtype=torch.float32, device=self.device), 0])
        k = ent[1]
        if k + M > ent[0].shape[0]:
            grown = ent[0].new_empty(max(2 * ent[0].shape[0], k + M), Q)
            grown[:k].copy_(ent[0][:k])
            ent[0] = grown
        ent[1] = k + M
        return ent[0][k:k + M], k

    @torch.no_grad()
    def update(self, results_by_image_id, targets_by_image_id):
        """results_by_image_id: image_id -> what PostProcess.forward returned for it ('scores' [Q], 'boxes' [Q,4] on the GPU);
        targets_by_image_id: image_id -> {'bbox': [x, y, w, h], 'dataset_name': ...} (or a list of one such).  One small upload
        (the ground-truth boxes of the call), one launch into the slab per box count Q among the call's images (one for a model's
        queries): no read-back, no synchronisation."""
        ids, gts, names = [], [], []
        for image_id in results_by_image_id:
            hid = _host_id(image_id)
            if image_id not in targets_by_image_id:
                raise ValueError(f"RefExpScorer.update: image {hid!r} has no target")
            if hid in self._seen or hid in ids:
                raise ValueError(f"RefExpScorer.update: image_id {hid!r} was scored already")
            name, box = _target(hid, targets_by_image_id[image_id])
            ids.append(hid)
            gts.append(box)
            names.append(name)
        if not ids:
            return
        boxes = []
        for image_id in results_by_image_id:
            r = results_by_image_id[image_id]
            sc, bx = r["scores"], r["boxes"]
            if not torch.is_tensor(bx) or bx.dim() != 2 or int(bx.shape[1]) != 4 or tuple(sc.shape) != (int(bx.shape[0]),):
                raise ValueError("RefExpScorer.update: 'boxes' must be [Q,4] and 'scores' [Q]")
            if not bx.is_cuda or not sc.is_cuda:
                raise ValueError("RefExpScorer.update: 'scores' and 'boxes' must be on the GPU")
            if int(bx.shape[0]) < 1 or int(bx.shape[0]) > 1024:
                raise ValueError(f"RefExpScorer.update: 1..1024 boxes per image, got {int(bx.shape[0])}")
            if getattr(r, "_refexp", None) is None:   # not PostProcess' own result: put it in descending score order
                bx = bx[torch.sort(sc, descending=True, stable=True).indices]
            boxes.append(bx.to(torch.float32))
        gt = torch.tensor(gts, dtype=torch.float64).to(torch.float32).to(self.device)   # the sums above in double, as the reference's
        at = [None] * len(ids)
        for Q in sorted({int(b.shape[0]) for b in boxes}):
            sel = [i for i, b in enumerate(boxes) if int(b.shape[0]) == Q]
            rows, k = self._room(Q, len(sel))
            ops.refexp_giou(torch.stack([boxes[i] for i in sel]).contiguous(), gt if len(sel) == len(ids) else gt[sel].contiguous(),
                            best=rows)
            for j, i in enumerate(sel):
                at[i] = (Q, k + j)
        self._at += at
        self._ids += ids
        self._names += names
        self._seen.update(ids)
        self._merged = None

    # ------------------------------------------------------------------------------------------------------------- reporting
    def state(self):
        """The read-back (one per slab): {'image_ids', 'datasets', 'best' [M][Q]} of what this scorer collected, plain Python
        (picklable; what a rank hands to all_gather)."""
        host = {Q: ent[0][:ent[1]].cpu().numpy().tolist() for Q, ent in self._best.items()}
        return {"image_ids": list(self._ids), "datasets": list(self._names), "best": [host[Q][row] for Q, row in self._at]}

    def merge(self, states):
        """Combines the states of several ranks (utils.all_gather at refexp_eval.py:31) into the one summarize() reports; returns
        it.  An image in several states -- a sampler's padding -- is kept once if its values are identical, otherwise ValueError."""
        got, ids = {}, []
        for st in states:
            if not len(st["image_ids"]) == len(st["datasets"]) == len(st["best"]):
                raise ValueError("RefExpScorer.merge: a state's lists differ in length")
            for image_id, name, best in zip(st["image_ids"], st["datasets"], st["best"]):
                if name not in DATASETS:
                    raise ValueError(f"RefExpScorer.merge: dataset_name {name!r} is none of {DATASETS}")
                v = (name, [float(x) for x in best])
                if image_id in got:
                    if got[image_id] != v:
                        raise ValueError(f"RefExpScorer.merge: image_id {image_id!r} comes with different results from two states")
                    continue
                got[image_id] = v
                ids.append(image_id)
        self._merged = {"image_ids": ids, "datasets": [got[i][0] for i in ids], "best": [got[i][1] for i in ids]}
        return self._merged

    def summarize(self):
        """refexp_eval.py:37-82: {'refcoco': [..], 'refcoco+': [..], 'refcocog': [..]}, per dataset the precisions at self.k sorted
        ascending (as the reference returns them), zeros for a dataset without an image"""
        st = self._merged if self._merged is not None else self.state()
        score = {d: [0.0] * len(self.k) for d in DATASETS}
        count = {d: 0 for d in DATASETS}
        for name, best in zip(st["datasets"], st["best"]):
            for i, hit in enumerate(hits(best, self.k, self.thresh_iou)):
                score[name][i] += 1.0 if hit else 0.0
            count[name] += 1
        return {d: sorted(v / count[d] if count[d] else v for v in score[d]) for d in DATASETS}
