"""The stage an A2D-Sentences / JHMDB-Sentences caller runs directly after the forward (models/postprocessors.py:14-54, called by
engine.py:308-319): dataset-size binary masks and their COCO run-length strings.

The masks and the run lengths are computed on the GPU (ops.a2d_masks, ops.rle_counts: include/tce_rvos_eval.h); the host sees the
run counts and the used prefix of the run lengths only, and packs them into the strings pycocotools' encoder returns
(rle_to_string).  The COCO-pretraining post-processors (PostProcess, PostProcessSegm) stay stubs: the reference itself does not
use them for RVOS.
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
