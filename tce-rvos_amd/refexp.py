"""The RefCOCO / RefCOCO+ / RefCOCOg evaluation loop of the reference's image setting (engine.py:105-132, without data loader and
criterion): images run as T = 1 clips through model.forward_group, then through the image post-processors in their grouped form
(postprocess.PostProcess / PostProcessSegm: one ops.refexp_group call per group for boxes and masks), and -- where the samples
carry targets -- into the scorers: refexp_score.RefExpScorer for precision@k of the boxes, a2d_score.A2DScorer for the masks (one
annotation per image is that scorer's own limit and RefCOCO's rule, so it is the coco_eval_masks analogue as it stands).

Nothing in the loop waits for the GPU: results stay on the device, the scorers read back once, in their state().
Out of scope: CocoEvaluator's box AP, the dataset classes and transforms, images of different shapes in one group (they are
grouped by exact shape instead of padded: every result is the image's own B = 1 forward)."""
import torch

from . import ops
from .video import plan_single_frame_groups


def plan_image_groups(shapes, lengths, max_group: int = 8, mixed_lengths: bool = False):
    """The forwards of run_images: lists of sample indices, one list per forward_group call.  Samples are bucketed by (shape, caption
    token length; mixed_lengths=True: whatever their lengths), buckets in order of first sighting, `max_group` samples at a time;
    every sample appears exactly once.  `shapes`: per sample whatever its group must share -- run_images passes the image's shape
    and its un-padded size.  video.plan_single_frame_groups with one annotated-frame index for all (an image is its own frame)."""
    if len(shapes) != len(lengths):
        raise ValueError(f"plan_image_groups: {len(shapes)} shapes, {len(lengths)} lengths")
    return plan_single_frame_groups(shapes, [0] * len(shapes), lengths, max_group, mixed_lengths)


def _pair(x):
    return tuple(int(v) for v in (x.tolist() if torch.is_tensor(x) else x))


@torch.no_grad()
def run_images(model, samples, postprocessors, max_group: int = 8, mixed_lengths: bool = False, scorer=None, mask_scorer=None):
    """samples: a list of dicts with `image` [3,H,W] float32 on the GPU (resized + normalised), `caption` (str or LongTensor [1,L]),
    `size` (the un-padded model-input size; default the image's (H, W)), `orig_size`, `image_id` (a host value) and optionally
    `target` ({'bbox': [x, y, w, h], 'dataset_name': ...}: read when `scorer` is given).
    postprocessors: what postprocess.build_refexp_postprocessors returns ({'bbox': PostProcess} and optionally 'segm').
    Returns {image_id: result} in input order; a result is PostProcess' dict, with 'masks' where 'segm' is there.
    scorer (refexp_score.RefExpScorer) is updated with every group's results and targets; mask_scorer (a2d_score.A2DScorer built
    over the images' ground-truth masks) with the group's 'masks' / 'scores' as they are."""
    if "bbox" not in postprocessors:
        raise ValueError("run_images: postprocessors must hold 'bbox' (postprocess.build_refexp_postprocessors)")
    if mask_scorer is not None and "segm" not in postprocessors:
        raise ValueError("run_images: a mask_scorer needs the 'segm' post-processor")
    if not samples:
        return {}
    for s in samples:
        if not torch.is_tensor(s["image"]) or s["image"].dim() != 3 or s["image"].shape[0] != 3:
            raise ValueError("run_images: `image` must be [3,H,W]")
        if scorer is not None and s.get("target") is None:
            raise ValueError(f"run_images: a scorer is given but image {s['image_id']!r} has no target")
    image_ids = [s["image_id"] for s in samples]
    if len(set(image_ids)) != len(image_ids):
        raise ValueError("run_images: image ids repeat")
    dev = samples[0]["image"].device
    ids = [s["caption"] if torch.is_tensor(s["caption"]) else model._tokenise([s["caption"]], dev)[0] for s in samples]
    sizes = [_pair(s["size"]) if s.get("size") is not None else (int(s["image"].shape[-2]), int(s["image"].shape[-1])) for s in samples]
    origs = [_pair(s["orig_size"]) for s in samples]
    plan = plan_image_groups([tuple(s["image"].shape) + sz for s, sz in zip(samples, sizes)], [int(t.shape[1]) for t in ids],
                             max_group, mixed_lengths)
    res = [None] * len(samples)
    for grp in plan:
        if mixed_lengths:  # right-padded on the host (validated there), lengths derived again on the device
            from .model import pad_captions
            tok = pad_captions([ids[i] for i in grp], model._pad_id())[0].to(dev)
        else:
            tok = torch.cat([ids[i].to(dev) for i in grp], 0)
        outs = model.forward_group([samples[i]["image"][None] for i in grp], tok, [{"size": torch.tensor(sizes[grp[0]])}],
                                   **({"ragged": True} if mixed_lengths else {}))
        orig, size = [origs[i] for i in grp], [sizes[i] for i in grp]
        if "segm" in postprocessors:
            results = postprocessors["segm"].with_boxes(outs, orig, size)
        else:
            results = postprocessors["bbox"](outs, orig)
        if scorer is not None:
            scorer.update({image_ids[i]: r for i, r in zip(grp, results)}, {image_ids[i]: samples[i]["target"] for i in grp})
        if mask_scorer is not None:
            mask_scorer.update([image_ids[i] for i in grp], results)
        for i, r in zip(grp, results):
            res[i] = r
    ops.check_range(dev)
    return {image_ids[i]: res[i] for i in range(len(samples))}
