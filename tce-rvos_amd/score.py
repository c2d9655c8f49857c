"""Ref-DAVIS J&F of label maps that stay on the GPU: what the reference's eval_davis.py does with the PNGs its driver wrote
(davis2017/evaluation.py:83-104 for the semi-supervised task, metrics.py, utils.py:135-161), without the PNGs.

The pixel work -- per (object, frame) the intersection, the union, the two boundary maps of _seg2bmap and their matches within
the disk -- is one call of ops.jf_counts (tce_jf_counts_i32, include/tce_rvos_score.h) over the whole video: six integers per
pair come back in one read-back.  Everything after the counts is the reference's float64 arithmetic on [n,T] numbers, restated
here operation by operation on the host, so J and F carry the reference's bits.

Not here: void masks (the reference's semi-supervised path passes None, evaluation.py:90), the unsupervised task (Hungarian
assignment), PNG reading and writing."""
import warnings

import numpy as np
import torch

from . import ops

G_MEASURES = ("J&F-Mean", "J-Mean", "J-Recall", "J-Decay", "F-Mean", "F-Recall", "F-Decay")  # eval_davis.py:43


def boundary_radius(H, W, bound_th=0.008):
    """metrics.py:77-78: the disk radius of f_measure for an [H,W] mask -- bound_th itself when it is >= 1, otherwise
    ceil(bound_th * |(H, W)|) in float64."""
    if bound_th >= 1:
        return bound_th
    return int(np.ceil(bound_th * np.linalg.norm((H, W))))


def jf_from_counts(counts):
    """counts [n,T,6] (ops.jf_counts; a tensor or an array) -> (J, F), float64 [n,T], with the operations of metrics.py:32-36 and
    :100-117 in their order: J = inters / union, 1 where the union is 0; precision = fg_match / n_fg and recall = gt_match / n_gt
    with the three empty-boundary cases (1, 0), (0, 1), (1, 1); F = 2 * precision * recall / (precision + recall), 0 where the
    sum is 0."""
    c = counts.detach().cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts)
    if c.ndim != 3 or c.shape[-1] != 6:
        raise ValueError(f"jf_from_counts: counts must be [n,T,6], got {tuple(c.shape)}")
    c = c.astype(np.int64)
    inters, union, n_fg, n_gt, fg_match, gt_match = (c[..., i] for i in range(6))
    with np.errstate(divide="ignore", invalid="ignore"):
        j = inters / union
        j[np.isclose(union, 0)] = 1
        precision = fg_match / n_fg.astype(np.float64)
        recall = gt_match / n_gt.astype(np.float64)
        no_fg, no_gt = n_fg == 0, n_gt == 0
        precision = np.where(no_fg, 1.0, np.where(no_gt, 0.0, precision))   # (no_fg, gt): 1; (fg, no_gt): 0; (neither): 1
        recall = np.where(no_gt, 1.0, np.where(no_fg, 0.0, recall))         # (no_fg, gt): 0; (fg, no_gt): 1; (neither): 1
        f = 2 * precision * recall / (precision + recall)
        f[precision + recall == 0] = 0
    return j, f


def db_statistics(per_frame_values):
    """utils.py:135-161: (mean, recall, decay) of one object's per-frame values -- nanmean; the share of frames above 0.5; the
    nanmean of the first of four bins minus that of the last.  The bin edges go through the reference's ids.astype(np.uint8)
    (:153), which WRAPS beyond 256 frames: this restates that, it does not mend it."""
    v = np.asarray(per_frame_values)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        M = np.nanmean(v)
        O = np.nanmean(v > 0.5)
    N_bins = 4
    ids = np.round(np.linspace(1, len(v), N_bins + 1) + 1e-10) - 1
    ids = ids.astype(np.int64).astype(np.uint8)  # the wrap of a float -> uint8 cast, spelled out: the cast itself is undefined past 255
    D_bins = [v[ids[i]:ids[i + 1] + 1] for i in range(0, 4)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        D = np.nanmean(D_bins[0]) - np.nanmean(D_bins[3])
    return M, O, D


def score_video(pred_labels, gt_labels, n=None, bound_th=0.008, drop_first_last=True):
    """J and F of one video.  pred_labels / gt_labels: uint8 [N,H,W] label maps on the GPU (0 = background, k = object k, 255 = void
    in the ground truth); video.run_video_objects(...)[i]["labels"] goes in as it is.  n: the number of objects, or None to read
    int(max(gt_labels[0])) back as davis.py:90-94 does (255 counting as 0).  drop_first_last: frames 1:-1 only, as
    evaluation.py:85.  Returns a dict: J, F float64 [n,N']; JM, JR, JD, FM, FR, FD float64 [n] (db_statistics per object);
    counts int64 [n,N',6]; n; radius."""
    for name, t in (("pred_labels", pred_labels), ("gt_labels", gt_labels)):
        if not torch.is_tensor(t) or t.dim() != 3 or t.dtype != torch.uint8:
            raise ValueError(f"score_video: {name} must be a uint8 [N,H,W] tensor")
    if tuple(pred_labels.shape) != tuple(gt_labels.shape):
        raise ValueError(f"score_video: pred_labels {tuple(pred_labels.shape)} and gt_labels {tuple(gt_labels.shape)} differ in shape")
    if n is None:
        g0 = gt_labels[0]
        n = int(torch.where(g0 == 255, torch.zeros_like(g0), g0).max())
    n = int(n)
    if drop_first_last:
        pred_labels, gt_labels = pred_labels[1:-1], gt_labels[1:-1]
    N, H, W = (int(s) for s in gt_labels.shape)
    if N < 1:
        raise ValueError("score_video: no frame left to score")
    radius = boundary_radius(H, W, bound_th)
    if radius != int(radius):
        raise ValueError(f"score_video: bound_th = {bound_th} is no whole number of pixels")
    radius = int(radius)
    if n == 0:  # no object in the first frame: the reference's loops run zero times
        counts = np.zeros((0, N, 6), dtype=np.int64)
    else:
        counts = ops.jf_counts(pred_labels.contiguous(), gt_labels.contiguous(), n, radius).cpu().numpy().astype(np.int64)
    J, F = jf_from_counts(counts)
    stats = np.array([db_statistics(J[k]) + db_statistics(F[k]) for k in range(n)], dtype=np.float64).reshape(n, 6)
    res = {"J": J, "F": F, "counts": counts, "n": n, "radius": radius}
    for i, key in enumerate(("JM", "JR", "JD", "FM", "FR", "FD")):
        res[key] = stats[:, i].copy()
    return res


def summarize(results):
    """The seven global numbers of eval_davis.py:43-46 over a list of score_video results (several videos, or one video's four
    annotator maps): every object of every result is one entry of the reference's J["M"], J["R"], ... lists."""
    if isinstance(results, dict):
        results = [results]
    cat = {k: np.concatenate([np.asarray(r[k], dtype=np.float64).reshape(-1) for r in results]) if len(results) else np.zeros(0)
           for k in ("JM", "JR", "JD", "FM", "FR", "FD")}
    if not cat["JM"].size:
        raise ValueError("summarize: no object to average over")
    final_mean = (np.mean(cat["JM"]) + np.mean(cat["FM"])) / 2.
    g_res = [final_mean, np.mean(cat["JM"]), np.mean(cat["JR"]), np.mean(cat["JD"]), np.mean(cat["FM"]), np.mean(cat["FR"]),
             np.mean(cat["FD"])]
    return {k: float(v) for k, v in zip(G_MEASURES, g_res)}
