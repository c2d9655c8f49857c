"""Whole-video drivers around the per-clip forward.

Two loops of the reference's callers, with the model call and the caller harness H on the GPU kernels:

* `run_video(..., clip_size=32)`  -- inference_davis.py:209-256: the video is cut into consecutive chunks of `clip_size`
  frames (the last one shorter), each chunk is one B=1 forward, the best query is chosen PER CHUNK from that chunk's
  mean class score, its masks are resized to the original size, and the per-chunk results are concatenated.
* `run_video(..., clip_size=None)` -- inference_ytvos.py:278-321 (the non-`keep_fps` branch): the whole video is one
  clip, whatever its length.  (The `keep_fps` branch is run_video_windows, below.)

* `run_video_expressions(...)` -- the loop AROUND those two in the reference's drivers (inference_ytvos.py:96-113,
  inference_davis.py:150-208: every expression of a video is run over the same frames): expressions whose captions tokenise to
  one length go through `model.forward_group` with the SAME clip tensor, so the backbone runs once per chunk and the rest of the
  program is shared by the group; each expression's result is what `run_video` returns for it.

* `run_video_objects(...)` -- the Ref-DAVIS driver's end (inference_davis.py:185-199 and 293-298): the expressions of a video are
  run ONCE per chunk (clip groups, as above), and each annotator's objects are combined into one uint8 label map per chunk by one
  launch (ops.label_objects: best query, up-sampling, sigmoid, threshold, background plane and arg-max over the objects).

* `run_annotated_frames(...)` -- the A2D-Sentences / JHMDB-Sentences evaluation loop (engine.py:301-319 without the data loader): one
  annotated frame per clip (`valid_indices`); samples of one clip shape and index go through `model.forward_group` together and
  through the post-processor's group launch.

* `run_video_windows(...)` -- the `keep_fps` branch of the Ref-YouTube-VOS driver (inference_ytvos.py:194-277; forced on when
  `args.f_extra != 0`, :136-137) and the live part of the MeViS driver (inference_mevis.py:196-214, `last="shifted"`): the video is
  cut into windows of `num_frames` frames, each widened by `f_extra` context frames on both sides (clamped at the video's ends), the
  best query is chosen over the WIDENED window and only the window's own frames get a mask (ops.select_window_masks: a context
  frame costs no output plane).  `plan_windows` is the rule, `plan_window_forwards` the forwards: the expressions of a video share
  the backbone per window, a lone expression runs several windows per forward.  `share="frames"` (opt-in) mixes
  captions and windows in one forward over a pool of the windows' distinct frames (model.forward_indexed).

A video's chunks share the caption, so with `model.text_cache_size > 0` RoBERTa runs once per expression instead of
once per chunk (the reference recomputes it inside every forward).  Chunks of one length share a captured hipGraph
(model._graphs is an LRU over shapes); a last, shorter chunk runs eagerly unless its shape comes back.
"""
from typing import Optional

import torch

from . import ops


@torch.no_grad()
def run_video(model, frames: torch.Tensor, caption, origin_hw, clip_size: Optional[int] = 32, threshold: float = 0.5,
              ref_points: bool = False):
    """frames [N,3,H,W] float32 on the GPU (already resized + normalised: frontend.py); caption: str or LongTensor
    [1,L] of token ids; origin_hw = (H0, W0) of the decoded video.
    Returns dict(masks uint8 [N,H0,W0] (1 = object), best_query int32 [n_chunks], pred_logits [N,K], pred_boxes [N,4]).
    ref_points=True (opt-in: what vis.overlay_expression draws the cross from): also reference_points [N,2], the best query's
    rows of the forward's reference_points, gathered like pred_boxes."""
    if frames.dim() != 4 or frames.shape[1] != 3:
        raise ValueError("run_video: frames must be [N,3,H,W]")
    n = frames.shape[0]
    if n == 0:
        raise ValueError("run_video: empty video")
    H, W = int(frames.shape[-2]), int(frames.shape[-1])
    target = [{"size": torch.tensor([H, W])}]
    cap = [caption] if isinstance(caption, str) else caption
    step = n if not clip_size else int(clip_size)
    masks, best, logits, boxes, points = [], [], [], [], []
    for lo in range(0, n, step):
        clip = frames[lo:lo + step]
        out = model([clip], cap, target)
        pl, pm = out["pred_logits"][0], out["pred_masks"][0]
        m, b = ops.select_masks(pl, pm, origin_hw, threshold)  # harness H: query choice + resize + sigmoid + threshold
        masks.append(m)
        best.append(b)
        idx = b.long().expand(pl.shape[0])
        ar = torch.arange(pl.shape[0], device=pl.device)
        logits.append(pl[ar, idx])
        boxes.append(out["pred_boxes"][0][ar, idx])
        if ref_points:
            points.append(out["reference_points"][0][ar, idx])
    ops.check_range(frames.device)  # the driver synchronises here anyway: surface a tripped range flag now
    res = {"masks": torch.cat(masks, 0), "best_query": torch.cat(best, 0), "pred_logits": torch.cat(logits, 0),
           "pred_boxes": torch.cat(boxes, 0)}
    if ref_points:
        res["reference_points"] = torch.cat(points, 0)
    return res


def _collect(out, origin_hw, threshold, acc):
    pl, pm = out["pred_logits"][0], out["pred_masks"][0]
    m, b = ops.select_masks(pl, pm, origin_hw, threshold)  # harness H: query choice + resize + sigmoid + threshold
    idx = b.long().expand(pl.shape[0])
    ar = torch.arange(pl.shape[0], device=pl.device)
    acc["masks"].append(m)
    acc["best_query"].append(b)
    acc["pred_logits"].append(pl[ar, idx])
    acc["pred_boxes"].append(out["pred_boxes"][0][ar, idx])
    if "reference_points" in acc:
        acc["reference_points"].append(out["reference_points"][0][ar, idx])


def plan_expression_groups(lengths, max_group: int = 4, mixed_lengths: bool = False):
    """The forwards of run_video_expressions: lists of expression indices, one list per forward_group call (per chunk).
    mixed_lengths=False: expressions of one token length are grouped, `max_group` at a time (buckets in order of first sighting).
    mixed_lengths=True: in input order, `max_group` at a time, whatever their lengths (forward_group(..., ragged=True))."""
    mg = max(1, int(max_group))
    if mixed_lengths:
        idx = list(range(len(lengths)))
        return [idx[g0:g0 + mg] for g0 in range(0, len(idx), mg)]
    buckets = {}
    for i, n in enumerate(lengths):
        buckets.setdefault(int(n), []).append(i)
    return [members[g0:g0 + mg] for members in buckets.values() for g0 in range(0, len(members), mg)]


@torch.no_grad()
def run_video_expressions(model, frames: torch.Tensor, captions, origin_hw, clip_size: Optional[int] = 32,
                          threshold: float = 0.5, max_group: int = 4, mixed_lengths: bool = False, ref_points: bool = False):
    """Every expression of ONE video.  frames as in run_video; captions: list of str (or of LongTensor [1,L]).  Returns a list with
    one run_video-style dict per caption, in order.  Captions of equal token length are grouped (at most `max_group` per forward);
    mixed_lengths=True groups them in input order whatever their lengths, right-padded to the group's longest
    (forward_group(..., ragged=True): fewer forwards per chunk, the pad rows cost some text work).  ref_points=True: every dict also
    carries reference_points [N,2], as run_video's."""
    if frames.dim() != 4 or frames.shape[1] != 3 or frames.shape[0] == 0:
        raise ValueError("run_video_expressions: frames must be a non-empty [N,3,H,W]")
    n = frames.shape[0]
    H, W = int(frames.shape[-2]), int(frames.shape[-1])
    target = [{"size": torch.tensor([H, W])}]
    ids = [c if torch.is_tensor(c) else model._tokenise([c], frames.device)[0] for c in captions]
    step = n if not clip_size else int(clip_size)
    accs = [{"masks": [], "best_query": [], "pred_logits": [], "pred_boxes": [], **({"reference_points": []} if ref_points else {})}
            for _ in captions]
    for grp in plan_expression_groups([int(t.shape[1]) for t in ids], max_group, mixed_lengths):
        if mixed_lengths:  # right-padded on the host (validated there), lengths derived again on the device
            from .model import pad_captions
            tok = pad_captions([ids[i] for i in grp], model._pad_id())[0].to(frames.device)
        else:
            tok = torch.cat([ids[i].to(frames.device) for i in grp], 0)
        for lo in range(0, n, step):
            clip = frames[lo:lo + step]
            # one tensor, len(grp) captions: shared backbone
            outs = model.forward_group([clip] * len(grp), tok, target, **({"ragged": True} if mixed_lengths else {}))
            for i, out in zip(grp, outs):
                _collect(out, origin_hw, threshold, accs[i])
    ops.check_range(frames.device)
    return [{k: torch.cat(v, 0) for k, v in a.items()} for a in accs]


def davis_annotator_sets(num_expressions: int):
    """inference_davis.py:185-194: a Ref-DAVIS video lists its expressions object-major with 4 annotators per object
    (expression obj * 4 + anno); annotator `anno`'s label map holds object `obj` as label obj + 1.  Returns the 4 index lists."""
    num_obj = int(num_expressions) // 4
    return [[obj * 4 + anno for obj in range(num_obj)] for anno in range(4)]


def plan_object_forwards(lengths, n_frames, clip_size=32, object_sets=None, max_group: int = 4, mixed_lengths: bool = False):
    """The forwards of run_video_objects, in order: (sets, [(lo, hi, [caption indices of one forward_group call]), ...]).  The chunk
    loop is the outer one; inside a chunk every caption that some set names runs exactly once, however many sets name it, grouped
    by plan_expression_groups.  sets = object_sets checked (default: one set of all captions, in order)."""
    ncap = len(lengths)
    sets = [list(range(ncap))] if object_sets is None else [[int(i) for i in s] for s in object_sets]
    for s in sets:
        if not 1 <= len(s) <= ops.LABEL_MAX_OBJS:
            raise ValueError(f"run_video_objects: a label map holds 1..{ops.LABEL_MAX_OBJS} objects, a set has {len(s)}")
        if any(i < 0 or i >= ncap for i in s) or len(set(s)) != len(s):
            raise ValueError(f"run_video_objects: set {s} must name distinct captions out of {ncap}")
    used = sorted({i for s in sets for i in s})
    groups = [[used[j] for j in g] for g in plan_expression_groups([lengths[i] for i in used], max_group, mixed_lengths)]
    step = int(n_frames) if not clip_size else int(clip_size)
    return sets, [(lo, min(lo + step, int(n_frames)), g) for lo in range(0, int(n_frames), step) for g in groups]


@torch.no_grad()
def run_video_objects(model, frames: torch.Tensor, captions, origin_hw, clip_size: Optional[int] = 32, object_sets=None,
                      max_group: int = 4, mixed_lengths: bool = False, threshold: float = 0.5, background: float = 0.1):
    """The label maps of ONE video (inference_davis.py:185-298 without the PNG writing).  frames, captions, clip_size, max_group and
    mixed_lengths as in run_video_expressions; object_sets: lists of caption indices, one list per label map (default: one map of
    all captions in order; davis_annotator_sets gives the driver's four).  Label k + 1 of a map is the k-th caption of its set, 0
    is background (no object's score reaches `threshold`; `background` is the driver's 0.1 plane).
    Returns one dict per set: labels uint8 [N,H0,W0], best_query int32 [n, n_chunks], pred_logits [n,N,K], pred_boxes [n,N,4]
    (per object what run_video_expressions returns for its caption).

    A caption runs once per chunk whatever the number of sets that name it.  The chunk's forwards all finish (are issued) before its
    label launches, so the outputs of several forward_group calls are read afterwards.  They stay valid: forward / forward_group hand
    back FRESH tensors from every call -- the eager program clones its outputs out of the arena (pipeline.run_clip, clone_outputs),
    a graph replay copies them out of the graph's static buffers into a new allocation (model._replay, ops.CopyPlan.clone) -- so a
    later forward writes none of them, and this function holds them until the chunk's last label launch has been issued on the same
    stream.  Each clip's pred_logits[0] / pred_masks[0] is a contiguous slice of such a tensor; its address goes into the launch's table."""
    if frames.dim() != 4 or frames.shape[1] != 3 or frames.shape[0] == 0:
        raise ValueError("run_video_objects: frames must be a non-empty [N,3,H,W]")
    n = int(frames.shape[0])
    H, W = int(frames.shape[-2]), int(frames.shape[-1])
    H0, W0 = int(origin_hw[0]), int(origin_hw[1])
    dev = frames.device
    target = [{"size": torch.tensor([H, W])}]
    ids = [c if torch.is_tensor(c) else model._tokenise([c], dev)[0] for c in captions]
    sets, plan = plan_object_forwards([int(t.shape[1]) for t in ids], n, clip_size, object_sets, max_group, mixed_lengths)
    toks = {}
    for _, _, grp in plan:
        if tuple(grp) not in toks:
            if mixed_lengths:  # right-padded on the host (validated there), lengths derived again on the device
                from .model import pad_captions
                toks[tuple(grp)] = pad_captions([ids[i] for i in grp], model._pad_id())[0].to(dev)
            else:
                toks[tuple(grp)] = torch.cat([ids[i].to(dev) for i in grp], 0)
    starts = sorted({lo for lo, _, _ in plan})
    res = [{"labels": torch.empty(n, H0, W0, dtype=torch.uint8, device=dev),
            "best_query": torch.empty(len(starts), len(s), dtype=torch.int32, device=dev), "pred_logits": [], "pred_boxes": []} for s in sets]
    for c, lo in enumerate(starts):
        hi, held = lo, {}
        for plo, phi, grp in plan:
            if plo != lo:
                continue
            hi = phi
            clip = frames[lo:hi]
            # one tensor, len(grp) captions: shared backbone
            outs = model.forward_group([clip] * len(grp), toks[tuple(grp)], target, **({"ragged": True} if mixed_lengths else {}))
            for i, out in zip(grp, outs):
                held[i] = (out["pred_logits"][0], out["pred_masks"][0], out["pred_boxes"][0])
        ar = torch.arange(hi - lo, device=dev)
        for s, r in zip(sets, res):
            _, best = ops.label_objects([held[i][0] for i in s], [held[i][1] for i in s], (H0, W0), threshold, background,
                                        out=r["labels"][lo:hi], best_out=r["best_query"][c])
            idx = best.long()
            r["pred_logits"].append(torch.stack([held[i][0][ar, idx[k].expand(hi - lo)] for k, i in enumerate(s)], 0))
            r["pred_boxes"].append(torch.stack([held[i][2][ar, idx[k].expand(hi - lo)] for k, i in enumerate(s)], 0))
    ops.check_range(dev)
    return [{"labels": r["labels"], "best_query": r["best_query"].t().contiguous(), "pred_logits": torch.cat(r["pred_logits"], 1),
             "pred_boxes": torch.cat(r["pred_boxes"], 1)} for r in res]


def plan_single_frame_groups(shapes, indices, lengths, max_group: int = 8, mixed_lengths: bool = False):
    """The forwards of run_annotated_frames: lists of sample indices, one list per forward_group call.  Samples are bucketed by
    (clip shape, annotated-frame index, caption token length; mixed_lengths=True: whatever their lengths), buckets in order of first
    sighting, `max_group` samples at a time; every sample appears exactly once.  Bucketing by index keeps the graph keys few: a
    captured group graph belongs to one index tuple (model.forward_group)."""
    if not len(shapes) == len(indices) == len(lengths):
        raise ValueError(f"plan_single_frame_groups: {len(shapes)} shapes, {len(indices)} indices, {len(lengths)} lengths")
    mg = max(1, int(max_group))
    buckets = {}
    for i, (shp, idx, n) in enumerate(zip(shapes, indices, lengths)):
        key = (tuple(shp), int(idx)) + (() if mixed_lengths else (int(n),))
        buckets.setdefault(key, []).append(i)
    return [members[g0:g0 + mg] for members in buckets.values() for g0 in range(0, len(members), mg)]


@torch.no_grad()
def run_annotated_frames(model, samples, postprocessor=None, max_group: int = 8, mixed_lengths: bool = False):
    """The A2D-Sentences / JHMDB-Sentences evaluation loop (engine.py:301-319 without the data loader).  samples: a list of dicts
    with `clip` [T,3,H,W] float32 on the GPU (resized + normalised), `caption` (str or LongTensor [1,L]), `valid_index` (the annotated
    frame), `orig_size` (the dataset's frame size) and optionally `size` (the model-input size; default the clip's (H, W)).  Returns,
    in input order, the post-processor's dict per sample (postprocess.A2DSentencesPostProcess; grouped=True serves a group's samples
    from one launch), or the forward's raw output dict when `postprocessor` is None.

    The clips are UN-PADDED: samples are grouped by exact clip shape (plan_single_frame_groups), which replaces the reference's
    padding of a batch to its largest clip, so each sample's result is its own B = 1 forward's -- forward([clip], caption,
    [{'size', 'valid_indices'}]) -- and does not depend on what else the batch holds.  Samples that name the SAME clip tensor
    (several expressions of one clip) share the backbone inside their group."""
    if not samples:
        return []
    dev = samples[0]["clip"].device
    ids = [s["caption"] if torch.is_tensor(s["caption"]) else model._tokenise([s["caption"]], dev)[0] for s in samples]
    sizes = [tuple(int(v) for v in s["size"]) if s.get("size") is not None else (int(s["clip"].shape[-2]), int(s["clip"].shape[-1]))
             for s in samples]
    plan = plan_single_frame_groups([tuple(s["clip"].shape) + sz for s, sz in zip(samples, sizes)],
                                    [int(s["valid_index"]) for s in samples], [int(t.shape[1]) for t in ids], max_group, mixed_lengths)
    res = [None] * len(samples)
    for grp in plan:
        if mixed_lengths:  # right-padded on the host (validated there), lengths derived again on the device
            from .model import pad_captions
            tok = pad_captions([ids[i] for i in grp], model._pad_id())[0].to(dev)
        else:
            tok = torch.cat([ids[i].to(dev) for i in grp], 0)
        targets = [{"size": torch.tensor(sizes[i]), "valid_indices": int(samples[i]["valid_index"])} for i in grp]
        outs = model.forward_group([samples[i]["clip"] for i in grp], tok, targets, **({"ragged": True} if mixed_lengths else {}))
        if postprocessor is not None:
            outs = postprocessor(outs, [samples[i]["orig_size"] for i in grp], [sizes[i] for i in grp])
        for i, o in zip(grp, outs):
            res[i] = o
    ops.check_range(dev)
    return res


def window_args(args):
    """dict(num_frames, f_extra) of the reference's argparse namespace, for plan_windows / run_video_windows.  The reference's
    drivers take the window loop when `args.keep_fps` is set and force it on when `args.f_extra != 0` (inference_ytvos.py:136-137):
    a caller that follows them runs run_video_windows in exactly those cases and run_video(clip_size=None) otherwise.  `f_extra` is
    an attribute some of the reference's own entry points forget to define: missing means 0.  num_frames defaults to 5 (opts.py)."""
    return {"num_frames": int(getattr(args, "num_frames", 5)), "f_extra": int(getattr(args, "f_extra", 0) or 0)}


def plan_windows(n_frames: int, num_frames: int, f_extra: int = 0, last: str = "short", take: str = "leading"):
    """The windows of run_video_windows, in order: a list of (ids, first, count, lo).  ids: the clip's frame indices (a tuple);
    the masks of clip positions first .. first+count-1 are written to video frames lo .. lo+count-1.  Every video frame is written
    exactly once, in increasing order.  Pure host arithmetic.

    Window w has the core frames [s, min(s + num_frames, N)), s = w * num_frames; its clip is the core with f_extra frames put in
    front (each max(0, first - 1)) and f_extra appended (each min(N - 1, last + 1)): frames repeat at the video's ends
    (inference_ytvos.py:198-212).  last="shifted" (inference_mevis.py:206-207): a window with s + num_frames > N starts at
    N - num_frames instead; the frames it shares with the window before keep their FIRST entry, so it writes only the frames from
    `covered` on (N < num_frames has negative indices in the reference: ValueError here).
    take="leading" is what the reference stores: core frame s + j gets the mask of clip position j (:243, range(m) of the
    widened clip), which with f_extra > 0 is frame clamp(s - f_extra + j).  take="centre" is the aligned variant: position
    f_extra + j, the frame itself."""
    N, n, e = int(n_frames), int(num_frames), int(f_extra)
    if N < 1:
        raise ValueError("plan_windows: empty video")
    if n < 1:
        raise ValueError(f"plan_windows: num_frames must be >= 1, got {n}")
    if e < 0:
        raise ValueError(f"plan_windows: f_extra must be >= 0, got {e}")
    if last not in ("short", "shifted"):
        raise ValueError(f"plan_windows: last must be 'short' or 'shifted', got {last!r}")
    if take not in ("leading", "centre"):
        raise ValueError(f"plan_windows: take must be 'leading' or 'centre', got {take!r}")
    if last == "shifted" and N < n:
        raise ValueError(f"plan_windows: last='shifted' needs a video of at least num_frames = {n} frames, got {N}")
    plan, covered = [], 0
    for s in range(0, N, n):
        if last == "shifted" and s + n > N:
            s = N - n
        hi = min(s + n, N)
        ids = [max(0, s - k) for k in range(e, 0, -1)] + list(range(s, hi)) + [min(N - 1, hi - 1 + k) for k in range(1, e + 1)]
        first = covered - s + (e if take == "centre" else 0)
        plan.append((tuple(ids), first, hi - covered, covered))
        covered = hi
    return plan


def _window_runs(windows, wpf):
    """consecutive windows of one clip length, at most wpf of them"""
    runs = []
    for w, win in enumerate(windows):
        if runs and len(runs[-1]) < wpf and len(windows[runs[-1][0]][0]) == len(win[0]):
            runs[-1].append(w)
        else:
            runs.append([w])
    return runs


def plan_window_forwards(lengths, windows, max_group: int = 4, windows_per_forward: int = 4, mixed_lengths: bool = False,
                         share: str = "clips", max_pairs: int = 8):
    """The forwards of run_video_windows, in order: a list of (captions, windows), both lists of indices; every (caption, window)
    pair appears exactly once.  `windows`: plan_windows' list.

    share="clips" (the default): model.forward_group shares the backbone only when ALL clips of a group are one tensor, so there
    are two kinds of forward: an expression bucket (plan_expression_groups) of two or more captions runs one SHARED group per window
    ([i, j, ...], [w]); a bucket of one caption runs its windows `windows_per_forward` at a time as distinct clips ([i], [w, ...]).
    Only consecutive windows of one clip length go together, so a short last window goes alone.  (max_pairs is not read.)

    share="frames" (opt-in; model.forward_indexed): a forward mixes captions and windows -- every bucket of c captions takes
    max(1, max_pairs // c) consecutive windows of one clip length per forward, a lone caption included (windows_per_forward is not
    read), so a forward has at most max_pairs (caption, window) slots unless the bucket alone is larger.  Its frames are a pool, the
    sorted distinct frames of its windows (window_pool): each runs through the backbone once, however many slots read it.

    Graph shapes per video with share="frames": the index tuples are relative to the forward's pool, so all interior forwards of a
    bucket are ONE shape; the first forward (f_extra > 0: frame 0 repeated), the last one (the last frame repeated, or fewer
    windows) and a short last window differ -- at most 4 shapes per bucket, 1 at f_extra = 0 when the windows divide evenly.  The
    graph cache holds 6 entries and 96 GB by default (model.max_graphs, model.max_graph_bytes; a graph owns arenas for all its
    slots' frames): a video of three buckets with f_extra > 0 asks for 8 shapes at max_pairs=4, and then evicts inside every video,
    which was measured at HALF the default plan's rate -- use share="frames" where a video's shapes fit the cache."""
    if share not in ("clips", "frames"):
        raise ValueError(f"plan_window_forwards: share must be 'clips' or 'frames', got {share!r}")
    out = []
    if share == "frames":
        mp = max(1, int(max_pairs))
        for grp in plan_expression_groups(lengths, max_group, mixed_lengths):
            out += [(list(grp), list(r)) for r in _window_runs(windows, max(1, mp // len(grp)))]
        return out
    runs = _window_runs(windows, max(1, int(windows_per_forward)))
    for grp in plan_expression_groups(lengths, max_group, mixed_lengths):
        if len(grp) >= 2:
            out += [(list(grp), [w]) for w in range(len(windows))]
        else:
            out += [(list(grp), list(r)) for r in runs]
    return out


def window_pool(windows, wins, n_captions: int = 1):
    """The frame pool of one share="frames" forward: (pool, index).  pool: the sorted distinct video frames of windows `wins` of
    plan_windows' list; index: n_captions * len(wins) tuples of positions in `pool`, caption-major (slot c * len(wins) + k is window
    wins[k] under the forward's c-th caption), so that [pool[p] for p in index[slot]] are that window's frame ids."""
    pool = sorted({f for w in wins for f in windows[w][0]})
    at = {f: k for k, f in enumerate(pool)}
    rel = [tuple(at[f] for f in windows[w][0]) for w in wins]
    return pool, [t for _ in range(int(n_captions)) for t in rel]


@torch.no_grad()
def run_video_windows(model, frames: torch.Tensor, captions, origin_hw, num_frames: int = 5, f_extra: int = 0, last: str = "short",
                      take: str = "leading", threshold: float = 0.5, max_group: int = 4, windows_per_forward: int = 4,
                      mixed_lengths: bool = False, share: str = "clips", max_pairs: int = 8):
    """The context-frame window loop over ONE video (see plan_windows for the rule and the module docstring for the citations).
    frames and origin_hw as in run_video; captions: a str, a LongTensor [1,L], or a list of either (a list returns a list).
    Returns per caption dict(masks uint8 [N,H0,W0], best_query int32 [n_windows], pred_logits [N,K], pred_boxes [N,4],
    reference_points [N,2] -- the best query's rows at the KEPT clip positions, as the reference indexes them --, windows: the plan).

    Each window's clip is frames.index_select(0, ids) on the device (the indices of all windows go up in one copy before the loop);
    `masks` is allocated once and every window's output stage writes its own slice of it.  Nothing inside the loop waits for the GPU.
    With take="leading" (the default: what the reference's published numbers were made with) and f_extra > 0 a frame's mask comes
    from a frame up to f_extra earlier; take="centre" aligns them.

    share="frames" (opt-in; plan_window_forwards has the rule): a forward holds up to max_pairs (caption, window) slots over a pool
    of its windows' distinct frames (model.forward_indexed), so the context frames that neighbouring windows repeat, the frames
    clamped at the video's ends and the windows that several captions read each pass the backbone once per forward.  The pool is one
    index_select into the video (the pool indices of all forwards go up in one copy before the loop); outputs are as above, to the
    round-off between one group shape and another."""
    if frames.dim() != 4 or frames.shape[1] != 3 or frames.shape[0] == 0:
        raise ValueError("run_video_windows: frames must be a non-empty [N,3,H,W]")
    single = isinstance(captions, str) or torch.is_tensor(captions)
    caps = [captions] if single else list(captions)
    if not caps:
        return []
    n = int(frames.shape[0])
    H, W = int(frames.shape[-2]), int(frames.shape[-1])
    H0, W0 = int(origin_hw[0]), int(origin_hw[1])
    dev = frames.device
    target = [{"size": torch.tensor([H, W])}]
    plan = plan_windows(n, num_frames, f_extra, last, take)
    ids = [c if torch.is_tensor(c) else model._tokenise([c], dev)[0] for c in caps]
    forwards = plan_window_forwards([int(t.shape[1]) for t in ids], plan, max_group, windows_per_forward, mixed_lengths, share,
                                    max_pairs)
    if share == "frames":
        return _run_window_pools(model, frames, caps, ids, plan, forwards, (H0, W0), target, threshold, mixed_lengths, single)
    flat = torch.tensor([i for win in plan for i in win[0]], dtype=torch.int64).to(dev)  # every window's indices: one copy
    offs = [0]
    for win in plan:
        offs.append(offs[-1] + len(win[0]))
    toks = {}
    for grp, wins in forwards:
        key = (tuple(grp), len(wins) if len(grp) == 1 else 1)
        if key in toks:
            continue
        if len(grp) == 1:  # one caption, len(wins) distinct clips (one window: the host ids, as run_video passes them)
            toks[key] = ids[grp[0]] if len(wins) == 1 else ids[grp[0]].to(dev).expand(len(wins), -1).contiguous()
        elif mixed_lengths:  # right-padded on the host (validated there), lengths derived again on the device
            from .model import pad_captions
            toks[key] = pad_captions([ids[i] for i in grp], model._pad_id())[0].to(dev)
        else:
            toks[key] = torch.cat([ids[i].to(dev) for i in grp], 0)
    res = [{"masks": torch.empty(n, H0, W0, dtype=torch.uint8, device=dev),
            "best_query": torch.empty(len(plan), dtype=torch.int32, device=dev),
            "pred_logits": [None] * len(plan), "pred_boxes": [None] * len(plan), "reference_points": [None] * len(plan)} for _ in caps]
    for grp, wins in forwards:
        clips = [frames.index_select(0, flat[offs[w]:offs[w + 1]]) for w in wins]
        if len(grp) == 1:
            outs = model.forward_group(clips, toks[(tuple(grp), len(wins))], target)
            pairs = [(grp[0], w) for w in wins]
        else:  # one tensor, len(grp) captions: shared backbone
            outs = model.forward_group(clips * len(grp), toks[(tuple(grp), 1)], target, **({"ragged": True} if mixed_lengths else {}))
            pairs = [(i, wins[0]) for i in grp]
        _store_windows(res, plan, pairs, outs, (H0, W0), threshold, dev)
    return _window_results(res, plan, single, dev)


def _store_windows(res, plan, pairs, outs, origin_hw, threshold, dev):
    """harness H of every (caption, window) pair of one forward: the query over the widened clip, the kept planes straight into the
    video's masks"""
    for (i, w), out in zip(pairs, outs):
        _, first, count, lo = plan[w]
        r = res[i]
        pl = out["pred_logits"][0]
        _, b = ops.select_window_masks(pl, out["pred_masks"][0], origin_hw, first, count, threshold,
                                       out=r["masks"][lo:lo + count], best_out=r["best_query"][w:w + 1])
        idx = b.long().expand(count)
        ar = torch.arange(first, first + count, device=dev)
        r["pred_logits"][w] = pl[ar, idx]
        r["pred_boxes"][w] = out["pred_boxes"][0][ar, idx]
        r["reference_points"][w] = out["reference_points"][0][ar, idx]


def _window_results(res, plan, single, dev):
    ops.check_range(dev)
    ret = [{"masks": r["masks"], "best_query": r["best_query"], "pred_logits": torch.cat(r["pred_logits"], 0),
            "pred_boxes": torch.cat(r["pred_boxes"], 0), "reference_points": torch.cat(r["reference_points"], 0), "windows": plan}
           for r in res]
    return ret[0] if single else ret


def _run_window_pools(model, frames, caps, ids, plan, forwards, origin_hw, target, threshold, mixed_lengths, single):
    """run_video_windows(share="frames"): every planned forward is one model.forward_indexed over the pool of its windows' frames."""
    n, dev = int(frames.shape[0]), frames.device
    pools = [window_pool(plan, wins, len(grp)) for grp, wins in forwards]
    flat = torch.tensor([f for pool, _ in pools for f in pool], dtype=torch.int64).to(dev)  # every forward's pool: one copy
    offs = [0]
    for pool, _ in pools:
        offs.append(offs[-1] + len(pool))
    toks = {}
    for grp, wins in forwards:
        key = (tuple(grp), len(wins))
        if key in toks:
            continue
        rows = [ids[i] for i in grp for _ in wins]  # caption-major: a caption's windows are neighbours
        if len(rows) == 1:  # one caption, one window: the host ids, as run_video passes them
            toks[key] = rows[0]
        elif mixed_lengths:  # right-padded on the host (validated there), lengths derived again on the device
            from .model import pad_captions
            toks[key] = pad_captions(rows, model._pad_id())[0].to(dev)
        else:
            toks[key] = torch.cat([r.to(dev) for r in rows], 0)
    res = [{"masks": torch.empty((n,) + tuple(origin_hw), dtype=torch.uint8, device=dev),
            "best_query": torch.empty(len(plan), dtype=torch.int32, device=dev),
            "pred_logits": [None] * len(plan), "pred_boxes": [None] * len(plan), "reference_points": [None] * len(plan)} for _ in caps]
    for k, (grp, wins) in enumerate(forwards):
        pool = frames.index_select(0, flat[offs[k]:offs[k + 1]])
        outs = model.forward_indexed(pool, pools[k][1], toks[(tuple(grp), len(wins))], target,
                                     **({"ragged": True} if mixed_lengths and len(grp) * len(wins) > 1 else {}))
        _store_windows(res, plan, [(i, w) for i in grp for w in wins], outs, origin_hw, threshold, dev)
    return _window_results(res, plan, single, dev)
