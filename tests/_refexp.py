"""The RefCOCO fixture's case table and loader (tests/golden/refexp_cases.npz, written by tests/golden/make_golden_refexp.py with
the reference's own PostProcess, PostProcessSegm, generalized_box_iou and RefExpEvaluator), shared by the maker and the tests.
Pure torch / numpy; nothing here touches the library under test."""
import numpy as np
import torch

import _a2d

DATASETS = ("refcoco", "refcoco+", "refcocog")
K_AT = (1, 5, 10)
SCORE_GAP = 4e-6   # neighbouring sorted sigmoid values of a case differ by more than this: the ranking does not hang on rounding
GIOU_MARGIN = 1e-5  # no giou or running maximum of the fixture lies this close to the 0.5 threshold

# case, seed, B, T, N, K, (h, w), sizes, origs, kind, scale, threshold
CASES = (("c1", 141, 1, 1, 5, 1, (18, 25), ((72, 100),), ((111, 150),), "smooth", 6.0, 0.5),     # _a2d case A's geometry
         ("c2", 142, 1, 2, 3, 2, (23, 40), ((90, 157),), ((87, 145),), "noise", 3.0, 0.5),       # K > 1: // K; crop; down-sampling
         ("c3", 143, 1, 1, 5, 1, (3, 4), ((9, 13),), ((5, 7),), "noise", 1.0, 0.35),              # tiny extents, another threshold
         ("c4", 144, 2, 1, 4, 1, (12, 17), ((48, 68), (40, 60)), ((50, 70), (33, 81)), "noise", 3.0, 0.5))  # a batch of two
EXACT = ("c1", "c3")   # no contested pixel: compared byte for byte
SYN = (12, 7)          # the synthetic GIoU set: images, boxes per image


def make_inputs(seed, B, T, N, K, hw, kind, scale):
    """pred_logits [B,T,N,K], pred_boxes [B,T,N,4] cxcywh, pred_masks [B,T,N,h,w] of a case, from torch.Generator(seed)"""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, T, N, K, generator=g) * 2.0
    cxcy = torch.rand(B, T, N, 2, generator=g) * 0.4 + 0.3
    wh = torch.rand(B, T, N, 2, generator=g) * 0.4 + 0.1
    masks = torch.stack([_a2d.make_inputs(seed * 10 + b, T * N, hw, kind, scale)[1].view(T, N, *hw) for b in range(B)])
    return logits, torch.cat([cxcy, wh], -1).contiguous(), masks.contiguous()


def make_gt(seed, boxes_xyxy):
    """A ground-truth [x, y, w, h] (Python floats, three decimals as COCO's) near one of the predicted boxes [Q,4]"""
    g = torch.Generator().manual_seed(seed)
    j = int(torch.randint(0, boxes_xyxy.shape[0], (1,), generator=g))
    x0, y0, x1, y1 = (float(v) for v in boxes_xyxy[j])
    r = torch.rand(4, generator=g).tolist()
    w, h = (x1 - x0) * (0.6 + 0.8 * r[0]), (y1 - y0) * (0.6 + 0.8 * r[1])
    return [round(x0 + (r[2] - 0.5) * 0.3 * w, 3), round(y0 + (r[3] - 0.5) * 0.3 * h, 3), round(w, 3), round(h, 3)]


def load_cases(path):
    """The committed fixture -> (cases, syn, summary): cases a list of dicts of CPU tensors -- name, B, T, N, K, threshold, logits,
    boxes, masks, sizes, origs, and per sample lists: scores [Q], order [Q] int64, boxes_out [Q,4], ref uint8 [Q,H0,W0], contested
    bool, gt [4] float64 xywh, dataset, giou [Q], hits [3]; syn the synthetic GIoU set; summary {dataset: [3]}."""
    fx = np.load(path)
    cases = []
    for name, seed, B, T, N, K, hw, sizes, origs, kind, scale, thr in CASES:
        Q = T * N
        c = {"name": name, "B": B, "T": T, "N": N, "K": K, "threshold": thr, "sizes": sizes, "origs": origs,
             "logits": torch.from_numpy(fx[f"{name}_logits"]), "boxes": torch.from_numpy(fx[f"{name}_boxes"]),
             "masks": torch.from_numpy(fx[f"{name}_masks"]), "scores": [], "order": [], "boxes_out": [], "ref": [], "contested": [],
             "gt": [], "dataset": [], "giou": [], "hits": []}
        for b in range(B):
            shape = (Q,) + tuple(origs[b])
            n = int(np.prod(shape))
            c["scores"].append(torch.from_numpy(fx[f"{name}_scores"][b]))
            c["order"].append(torch.from_numpy(fx[f"{name}_order"][b]))
            c["boxes_out"].append(torch.from_numpy(fx[f"{name}_boxes_out"][b]))
            c["ref"].append(torch.from_numpy(np.unpackbits(fx[f"{name}_ref{b}"])[:n].reshape(shape)))
            c["contested"].append(torch.from_numpy(np.unpackbits(fx[f"{name}_contested{b}"])[:n].reshape(shape).astype(bool)))
            c["gt"].append(fx[f"{name}_gt"][b].tolist())
            c["dataset"].append(str(fx[f"{name}_dataset"][b]))
            c["giou"].append(torch.from_numpy(fx[f"{name}_giou"][b]))
            c["hits"].append(fx[f"{name}_hits"][b].astype(bool).tolist())
        cases.append(c)
    syn = {"boxes": torch.from_numpy(fx["syn_boxes"]), "scores": torch.from_numpy(fx["syn_scores"]), "gt": fx["syn_gt"].tolist(),
           "dataset": [str(s) for s in fx["syn_dataset"]], "giou": torch.from_numpy(fx["syn_giou"]),
           "hits": fx["syn_hits"].astype(bool).tolist()}
    summary = {d: fx["summary"][i].tolist() for i, d in enumerate(DATASETS)}
    return cases, syn, summary
