"""The stage an A2D-Sentences / JHMDB-Sentences caller runs directly after the forward (models/postprocessors.py:14-54, called by
engine.py:308-319): dataset-size binary masks and their COCO run-length strings.

The masks and the run lengths are computed on the GPU (ops.a2d_masks, ops.rle_counts: include/tce_rvos_eval.h); the host sees the
run counts and the used prefix of the run lengths only, and packs them into the strings pycocotools' encoder returns
(rle_to_string).

The reference's image-setting post-processors, which its RefCOCO / RefCOCO+ / RefCOCOg evaluation calls (postprocessors.py:58-155,
engine.py:113-120), are PostProcess and PostProcessSegm below, on ops.refexp_group (include/tce_rvos_refexp.h); they are reached through
build_refexp_postprocessors.  build_postprocessors is unchanged and still hands out a stub for everything but A2D / JHMDB.
"""
import numpy as np
import torch
from torch import nn

from . import ops


def rle_to_string(counts):
    """cocoapi rleToString for one mask's run lengths -> bytes (what mask_util.encode returns under 'counts').

    Run i is stored as x = counts[i] (i <= 2) or counts[i] - counts[i-2] (i > 2), in 5-bit groups, low group first: c = x & 0x1f,
    x >>= 5 (arithmetic); more = (x != -1) if c & 0x10 else (x != 0); c |= 0x20 if more; the character is chr(c + 48).
    Vectorised over the runs: the only loop is over the at most 7 groups of a 32-bit value."""
    x = np.asarray(counts, dtype=np.int64).reshape(-1).copy()
    if x.size == 0:
        return b""
    x[3:] -= np.asarray(counts, dtype=np.int64).reshape(-1)[1:-2]
    chars = np.empty((x.size, 7), dtype=np.uint8)
    emit = np.zeros((x.size, 7), dtype=bool)
    alive = np.ones(x.size, dtype=bool)
    for k in range(7):
        c = x & 0x1f
        x = x >> 5
        more = np.where((c & 0x10) != 0, x != -1, x != 0)
        chars[:, k] = (c | np.where(more, 0x20, 0)) + 48
        emit[:, k] = alive
        alive = alive & more
        if not alive.any():
            break
    assert not alive.any(), "a run length beyond 32 bits"
    return chars[emit].tobytes()  # boolean indexing walks row by row: run after run, group after group


def _samples(outputs):
    """outputs (one dict with a batch axis, or a list of such dicts, as forward_group returns them) -> (logits [N], masks [N,h,w])
    per sample: frame 0 of every sample (there is only one valid frame, postprocessors.py:33-35)."""
    outs = [outputs] if isinstance(outputs, dict) else list(outputs)
    res = []
    for o in outs:
        lg, pm = o["pred_logits"], o["pred_masks"]
        if lg.dim() != 4 or pm.dim() != 5 or lg.shape[0] != pm.shape[0] or lg.shape[2] != pm.shape[2]:
            raise ValueError(f"A2DSentencesPostProcess: pred_logits must be [B,T,N,K] and pred_masks [B,T,N,h,w], got "
                             f"{tuple(lg.shape)} and {tuple(pm.shape)}")
        for b in range(lg.shape[0]):
            res.append((lg[b, 0, :, 0], pm[b, 0]))
    return res


def _sizes(x):
    """[B,2] tensor (one read-back if it lives on the GPU) or a sequence of (h, w) pairs -> list of [h, w] python ints"""
    if torch.is_tensor(x):
        return [[int(v) for v in s] for s in x.tolist()]
    return [[int(v) for v in (s.tolist() if torch.is_tensor(s) else s)] for s in x]


class A2DSentencesPostProcess(nn.Module):
    """models/postprocessors.py:14-54 on the GPU.  forward(outputs, orig_target_sizes, max_target_sizes) -> one dict per sample:
      scores     fp32 [N] on the GPU: sigmoid(pred_logits[b,0,:,0])
      masks      uint8 [N,1,H0,W0] on the GPU, values 0/1 (the reference returns float32 planes of 0/1: the one deviation)
      rle_masks  N dicts {'size': [H0,W0], 'counts': bytes}: what mask_util.encode(...)[0] returns per query
    Like the reference class it binarises at 0.5 whatever `threshold` it was built with (postprocessors.py:40 hard-codes 0.5);
    the attribute is kept because callers set and read it.
    Per sample one masks launch and one run-length call over the N queries; per call one read-back of the run counts, then one of
    the used run lengths.  The float masks never leave the GPU.
    rle=False: no run-length launches, no read-back and no 'rle_masks' key -- for a caller that scores `masks` on the device
    (a2d_score.A2DScorer.update) and needs no strings.
    grouped=True (opt-in): the samples of a call that share (N, h, w) -- a clip group's (model.forward_group with valid_indices) --
    get their scores and masks from ONE launch per ops.A2D_GROUP_MAX samples (ops.a2d_group_masks) instead of a sigmoid and a masks
    launch each; same bytes, same scores.  The run-length calls and the two read-backs stay as they are."""

    def __init__(self, threshold=0.5, rle=True, grouped=False):
        super().__init__()
        self.threshold = threshold
        self.rle = rle
        self.grouped = grouped

    def _held_grouped(self, samples, size, orig):
        """(scores, masks, counts, nruns) per sample, the samples of one (N, h, w) served by one group launch"""
        held = [None] * len(samples)
        buckets = {}
        for b, (_, pm) in enumerate(samples):
            buckets.setdefault((tuple(pm.shape), pm.device), []).append(b)
        for members in buckets.values():
            masks, scores = ops.a2d_group_masks([samples[b][1].to(torch.float32).contiguous() for b in members],
                                                [samples[b][0].to(torch.float32) for b in members],
                                                [size[b] for b in members], [orig[b] for b in members], threshold=0.5)
            for b, m, sc in zip(members, masks, scores):
                counts, nruns = ops.rle_counts(m) if self.rle else (None, None)
                held[b] = (sc, m, counts, nruns)
        return held

    @torch.no_grad()
    def forward(self, outputs, orig_target_sizes, max_target_sizes):
        samples = _samples(outputs)
        orig, size = _sizes(orig_target_sizes), _sizes(max_target_sizes)
        if not len(orig) == len(size) == len(samples):
            raise ValueError(f"A2DSentencesPostProcess: {len(samples)} samples, {len(orig)} original sizes, {len(size)} sizes")
        if self.grouped:
            held = self._held_grouped(samples, size, orig)
        else:
            held = []
            for (lg, pm), sz, og in zip(samples, size, orig):
                scores = ops.sigmoid(lg.to(torch.float32).contiguous())
                masks = ops.a2d_masks(pm.to(torch.float32).contiguous(), sz, og, threshold=0.5)
                counts, nruns = ops.rle_counts(masks) if self.rle else (None, None)
                held.append((scores, masks, counts, nruns))
        if not self.rle:
            return [{"scores": scores, "masks": masks.unsqueeze(1)} for scores, masks, _, _ in held]
        nruns = torch.cat([h[3] for h in held]).cpu().tolist()               # read-back 1: B*N integers
        k, used = 0, []
        for _, _, counts, nr in held:
            for n in range(counts.shape[0]):
                used.append(counts[n, :nruns[k]])
                k += 1
        flat = torch.cat(used).cpu().numpy()                                  # read-back 2: the run lengths in use
        res, k, at = [], 0, 0
        for (scores, masks, _, _), og in zip(held, orig):
            rle = []
            for n in range(masks.shape[0]):
                rle.append({"size": [int(og[0]), int(og[1])], "counts": rle_to_string(flat[at:at + nruns[k]])})
                at += nruns[k]
                k += 1
            res.append({"scores": scores, "masks": masks.unsqueeze(1), "rle_masks": rle})
        return res


def build_postprocessors(args, dataset_name):
    """models/postprocessors.py:158-166: the A2D / JHMDB post-processor for those two datasets; for anything else the reference
    returns its COCO-pretraining post-processors, which are stubs here."""
    if dataset_name == "a2d" or dataset_name == "jhmdb":
        return A2DSentencesPostProcess(threshold=getattr(args, "threshold", 0.5))
    from .model import _Stub
    return {"segm": _Stub("PostProcessSegm")}


# ------------------------------------------------------------------------------------------ RefCOCO / RefCOCO+ / RefCOCOg
class _Result(dict):
    """A result dict of PostProcess with a private marker beside its keys: the flattened logits it was ranked from and the ranking,
    so that PostProcessSegm on the same outputs does not rank again"""
    _refexp = None


def _refexp_samples(outputs, need_masks):
    """outputs (one dict with a batch axis, or a list of such dicts, as forward_group returns them) -> per sample (logits [Q,K],
    boxes [Q,4], masks [Q,h,w] | None) with Q = T*N: the reference's flatten(1, 2) (postprocessors.py:78-79, 128-129)"""
    outs = [outputs] if isinstance(outputs, dict) else list(outputs)
    res = []
    for o in outs:
        lg, bx = o["pred_logits"], o["pred_boxes"]
        if lg.dim() != 4 or bx.dim() != 4 or tuple(bx.shape) != tuple(lg.shape[:3]) + (4,):
            raise ValueError(f"PostProcess: pred_logits must be [B,T,N,K] and pred_boxes [B,T,N,4], got {tuple(lg.shape)} and "
                             f"{tuple(bx.shape)}")
        pm = o["pred_masks"] if need_masks else None
        if pm is not None and (pm.dim() != 5 or tuple(pm.shape[:3]) != tuple(lg.shape[:3])):
            raise ValueError(f"PostProcessSegm: pred_masks must be [B,T,N,h,w] beside pred_logits {tuple(lg.shape)}, got "
                             f"{tuple(pm.shape)}")
        K = int(lg.shape[3])
        for b in range(lg.shape[0]):
            res.append((lg[b].reshape(-1, K).to(torch.float32).contiguous(), bx[b].reshape(-1, 4).to(torch.float32).contiguous(),
                        None if pm is None else pm[b].reshape((-1,) + tuple(pm.shape[3:])).to(torch.float32).contiguous()))
    return res


def _buckets(samples):
    """sample indices by what one ops.refexp_group call shares: (Q, K), the mask plane, the device"""
    buckets = {}
    for b, (lg, _, pm) in enumerate(samples):
        buckets.setdefault((tuple(lg.shape), None if pm is None else tuple(pm.shape[1:]), lg.device), []).append(b)
    return list(buckets.values())


def _same_logits(marker, lg):
    """Was `marker` left by a ranking of exactly these logits (same memory, same shape, not written since)?"""
    t = None if marker is None else marker[0]
    return t is not None and t.data_ptr() == lg.data_ptr() and tuple(t.shape) == tuple(lg.shape) and t.device == lg.device \
        and marker[2] == lg._version


def _refexp_results(samples, orig, size, threshold):
    """One ops.refexp_group call per bucket for boxes and (where the samples carry masks) masks: the _Result per sample"""
    results = [None] * len(samples)
    for members in _buckets(samples):
        with_masks = samples[members[0]][2] is not None
        scores, order, boxes, masks = ops.refexp_group([samples[b][0] for b in members], [samples[b][1] for b in members],
                                                       [samples[b][2] for b in members] if with_masks else None,
                                                       [size[b] for b in members] if with_masks else None,
                                                       [orig[b] for b in members], threshold=threshold)
        labels = torch.ones(len(members), scores[0].shape[0], dtype=torch.int64, device=scores[0].device)
        for k, b in enumerate(members):
            r = _Result(scores=scores[k], labels=labels[k], boxes=boxes[k])
            if with_masks:
                r["masks"] = masks[k].unsqueeze(1)
            r._refexp = (samples[b][0], order[k], samples[b][0]._version)
            results[b] = r
    return results


class PostProcess(nn.Module):
    """models/postprocessors.py:58-100 on the GPU.  forward(outputs, target_sizes) -> one dict per sample, all on the GPU:
      scores  fp32 [Q]    the Q = T*N largest of the Q*K sigmoid scores, descending (torch.topk, sorted)
      labels  int64 [Q]   ones (:98, "binary for the pretraining")
      boxes   fp32 [Q,4]  x0,y0,x1,y1 in pixels of target_sizes: the ranked candidates' boxes, bit for bit the reference's
    outputs: one dict with a batch axis, or a list of such dicts (what model.forward_group returns).  One launch per
    ops.REFEXP_GROUP_MAX samples that share (Q, K).  Deviation: equal scores are ordered by their flat candidate index (topk
    leaves their order unspecified)."""

    @torch.no_grad()
    def forward(self, outputs, target_sizes):
        samples = _refexp_samples(outputs, need_masks=False)
        orig = _sizes(target_sizes)
        if len(orig) != len(samples):
            raise ValueError(f"PostProcess: {len(samples)} samples, {len(orig)} target sizes")
        return _refexp_results(samples, orig, None, 0.5)


class PostProcessSegm(nn.Module):
    """models/postprocessors.py:103-154 on the GPU.  forward(results, outputs, orig_target_sizes, max_target_sizes) adds to every
    result 'masks' uint8 [Q,1,H0,W0] of 0/1 on the GPU (the reference's dtype, on the host there): plane r is the mask of the
    r-th ranked candidate, up-sampled x4, binarised at `threshold` (used, unlike the A2D class's), cropped to max_target_sizes and
    resized (nearest) to orig_target_sizes -- the bytes of ops.a2d_masks for that plane.
    When `results` came from this module's PostProcess on the same outputs (a private marker says so), its ranking is used and only
    the masks launch runs; any other results take the full call (ranking and masks; their other keys are left as they are).
    with_boxes(outputs, orig_target_sizes, max_target_sizes) is both classes in ONE ops.refexp_group call per group: what
    refexp.run_images uses."""

    def __init__(self, threshold=0.5):
        super().__init__()
        self.threshold = threshold

    @staticmethod
    def _checked(outputs, orig_target_sizes, max_target_sizes):
        samples = _refexp_samples(outputs, need_masks=True)
        orig, size = _sizes(orig_target_sizes), _sizes(max_target_sizes)
        if not len(orig) == len(size) == len(samples):
            raise ValueError(f"PostProcessSegm: {len(samples)} samples, {len(orig)} original sizes, {len(size)} sizes")
        return samples, orig, size

    @torch.no_grad()
    def with_boxes(self, outputs, orig_target_sizes, max_target_sizes):
        samples, orig, size = self._checked(outputs, orig_target_sizes, max_target_sizes)
        return _refexp_results(samples, orig, size, self.threshold)

    @torch.no_grad()
    def forward(self, results, outputs, orig_target_sizes, max_target_sizes):
        samples, orig, size = self._checked(outputs, orig_target_sizes, max_target_sizes)
        if len(results) != len(samples):
            raise ValueError(f"PostProcessSegm: {len(samples)} samples, {len(results)} results")
        for members in _buckets(samples):
            ranked = all(_same_logits(getattr(results[b], "_refexp", None), samples[b][0]) for b in members)
            _, _, _, masks = ops.refexp_group([samples[b][0] for b in members], [samples[b][1] for b in members],
                                              [samples[b][2] for b in members], [size[b] for b in members],
                                              [orig[b] for b in members], threshold=self.threshold,
                                              order=[results[b]._refexp[1] for b in members] if ranked else None)
            for k, b in enumerate(members):
                results[b]["masks"] = masks[k].unsqueeze(1)
        return results


def build_refexp_postprocessors(args):
    """What models/postprocessors.py:162-166 returns for the image setting: {'bbox': PostProcess()} and, with args.masks,
    'segm': PostProcessSegm(threshold=args.threshold).  A builder of its own: build_postprocessors keeps returning what it
    returned (INTEGRATION.md has the swap in main.py's RefCOCO branch)."""
    post = {"bbox": PostProcess()}
    if getattr(args, "masks", False):
        post["segm"] = PostProcessSegm(threshold=getattr(args, "threshold", 0.5))
    return post
