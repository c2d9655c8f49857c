"""The drivers' output stages over the C ABI: what the inference and evaluation drivers do with the outputs of forwards (masks of
the best query, label maps, dataset-size masks and run lengths, scoring counts, PNG streams and files, overlays), each a wrapper
of the entry points of include/tce_rvos_{video,eval,score,png,vis,pngfile,refexp}.h and of tce_select_masks_u8.  They share
nothing with the model's hot-path ops; ops re-exports every public name here, and callers use ops.<name>.  No fallback."""
import torch

from ._lib import A2D_GROUP_MAX, REFEXP_GROUP_MAX, REFEXP_MAX_CAND, A2dGroupSample, LabelObj, RefexpSample, check, lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _chk(t, name):
    if t.dtype != torch.float32 or not t.is_cuda:
        raise TypeError(f"{name}: expected a CUDA float32 tensor, got {t.dtype} on {t.device}")


def _gpu_tensor(t, op, name, dtype, dims=None, device=None):
    """An input whose address goes to a launch as it is: a contiguous `dtype` tensor on the GPU -- of the rank of dims ("P,H,W")
    where given, on `device` where given (the tensors of one launch table share a device)."""
    if dims is not None and (not torch.is_tensor(t) or t.dim() != len(dims.split(","))):
        raise ValueError(f"{op}: {name} must be [{dims}]")
    if t.dtype != dtype or not t.is_cuda or not t.is_contiguous() or (device is not None and t.device != device):
        raise ValueError(f"{op}: {name} must be a contiguous {str(dtype)[6:]} tensor on the GPU{'' if device is None else ' (one device)'}, "
                         f"got {t.dtype} on {t.device}, contiguous={t.is_contiguous()}")
    return t


def _out_tensor(t, what, dtype, shape, dev):
    """A caller-supplied output of an output stage (`what` = "op: name ... [dims]", for the message), or a new one."""
    if t is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.device != dev:
        raise ValueError(f"{what} must be a contiguous {str(dtype)[6:]} {list(shape)} on the inputs' device")
    return t


def _workspace(t, op, nbytes, dev):
    """A caller-supplied workspace of an output stage, or a new one: nbytes on an 8-byte boundary."""
    if t is None:
        return torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
    if t.numel() * t.element_size() < nbytes or t.data_ptr() % 8 or t.device != dev:
        raise ValueError(f"{op}: ws must hold {nbytes} bytes on an 8-byte boundary on the inputs' device")
    return t


def select_masks(pred_logits, pred_masks, out_hw, threshold=0.5, out=None, best_out=None):
    """Caller harness H (inference_ytvos.py:238-250) on the GPU: pred_logits [T,Q,K], pred_masks [T,Q,h,w]
    -> (uint8 masks [T,H0,W0], best-query index tensor [1] int32).
    out / best_out: write into these (e.g. a chunk's slice of a video's masks, at any address) instead of new tensors."""
    _chk(pred_logits, "pred_logits")
    _chk(pred_masks, "pred_masks")
    T, Q, K = pred_logits.shape
    _, _, h, w = pred_masks.shape
    H0, W0 = int(out_hw[0]), int(out_hw[1])
    out = _out_tensor(out, "select_masks: out [T,H0,W0]", torch.uint8, (T, H0, W0), pred_masks.device)
    best = _out_tensor(best_out, "select_masks: best_out [1]", torch.int32, (1,), pred_masks.device)
    check(lib().tce_select_masks_u8(pred_logits.contiguous().data_ptr(), pred_masks.contiguous().data_ptr(),
                                    out.data_ptr(), best.data_ptr(), T, Q, K, h, w, H0, W0, float(threshold), _stream()),
          "tce_select_masks_u8")
    return out, best


def select_window_masks(pred_logits, pred_masks, out_hw, first, count, threshold=0.5, out=None, best_out=None):
    """The harness H of one context-frame window (inference_ytvos.py:238-264 under keep_fps): pred_logits [T,Q,K] and pred_masks
    [T,Q,h,w] of the WIDENED clip -> (uint8 masks [count,H0,W0] of clip positions first .. first+count-1, best-query index [1] int32).
    The best query is chosen over all T frames; only the kept positions are resampled, so a context frame costs no output plane.
    Three launches that exist, no read-back in between: tce_select_masks_u8 at a 1x1 output writes the index (and T scratch
    bytes); index_select gathers the kept planes of that query on the device; tce_select_masks_u8 on those [count,1,h,w] planes
    (Q = K = 1: its own index is 0, not stored) renders them -- the operations of the whole-window launch on the same planes,
    hence its bits (tests/test_output_stage_gpu.py holds the Q = 1 form to that).  out / best_out as in select_masks."""
    _chk(pred_logits, "pred_logits")
    _chk(pred_masks, "pred_masks")
    if pred_logits.dim() != 3 or pred_masks.dim() != 4 or pred_masks.shape[:2] != pred_logits.shape[:2]:
        raise ValueError("select_window_masks: pred_logits must be [T,Q,K] and pred_masks [T,Q,h,w]")
    T, Q, K = (int(v) for v in pred_logits.shape)
    h, w = int(pred_masks.shape[2]), int(pred_masks.shape[3])
    H0, W0 = int(out_hw[0]), int(out_hw[1])
    first, count = int(first), int(count)
    if first < 0 or count < 1 or first + count > T:
        raise ValueError(f"select_window_masks: positions {first} .. {first + count - 1} are not inside a window of {T} frames")
    dev = pred_masks.device
    out = _out_tensor(out, "select_window_masks: out [count,H0,W0]", torch.uint8, (count, H0, W0), dev)
    best = _out_tensor(best_out, "select_window_masks: best_out [1]", torch.int32, (1,), dev)
    lg, pm = pred_logits.contiguous(), pred_masks.contiguous()
    scratch = torch.empty(T, dtype=torch.uint8, device=dev)  # the 1x1 "masks" of the index launch: written, never read
    check(lib().tce_select_masks_u8(lg.data_ptr(), pm.data_ptr(), scratch.data_ptr(), best.data_ptr(), T, Q, K, h, w, 1, 1,
                                    float(threshold), _stream()), "tce_select_masks_u8")
    planes = pm[first:first + count].index_select(1, best.long())  # [count,1,h,w], the index stays on the device
    # the render launch scores its one query from `count` floats of lg (T*Q*K >= count of them) and stores no index
    check(lib().tce_select_masks_u8(lg.data_ptr(), planes.data_ptr(), out.data_ptr(), None, count, 1, 1, h, w, H0, W0,
                                    float(threshold), _stream()), "tce_select_masks_u8")
    return out, best


LABEL_MAX_OBJS = 16  # TCE_LABEL_MAX_OBJS (include/tce_rvos_video.h)


def label_objects(pred_logits, pred_masks, out_hw, threshold=0.5, background=0.1, out=None, best_out=None):
    """Ref-DAVIS label map of one chunk (inference_davis.py:239-248, 293-298) on the GPU: the n objects of a label map, each with
    its own forward's pred_logits [T,Q,K] and pred_masks [T,Q,h,w] (lists of n tensors, or stacked [n,T,Q,K] / [n,T,Q,h,w])
    -> (labels uint8 [T,H0,W0]: 0 = background, k + 1 = object k; best-query indices int32 [n]).
    The tensors' addresses go into the launch's table as they are: no stacked copy of the masks is made, so every tensor must be
    contiguous float32 on the GPU.  out / best_out: write into these (e.g. a chunk's slice of a video's label map) instead of new tensors."""
    lg = list(pred_logits.unbind(0)) if torch.is_tensor(pred_logits) else list(pred_logits)
    pm = list(pred_masks.unbind(0)) if torch.is_tensor(pred_masks) else list(pred_masks)
    n = len(lg)
    if n < 1 or n > LABEL_MAX_OBJS:
        raise ValueError(f"label_objects: 1..{LABEL_MAX_OBJS} objects per label map, got {n}")
    if len(pm) != n:
        raise ValueError(f"label_objects: {n} pred_logits but {len(pm)} pred_masks")
    if lg[0].dim() != 3 or pm[0].dim() != 4:
        raise ValueError("label_objects: pred_logits must be [T,Q,K] and pred_masks [T,Q,h,w] per object")
    T, Q, K = (int(s) for s in lg[0].shape)
    h, w = int(pm[0].shape[2]), int(pm[0].shape[3])
    H0, W0 = int(out_hw[0]), int(out_hw[1])
    for k in range(n):
        if tuple(lg[k].shape) != (T, Q, K) or tuple(pm[k].shape) != (T, Q, h, w):
            raise ValueError(f"label_objects: object {k} has pred_logits {tuple(lg[k].shape)} / pred_masks {tuple(pm[k].shape)}, "
                             f"object 0 has {(T, Q, K)} / {(T, Q, h, w)}")
    for k in range(n):
        for t, name in ((lg[k], "pred_logits"), (pm[k], "pred_masks")):
            _gpu_tensor(t, "label_objects", f"{name}[{k}]", torch.float32, device=pm[0].device)
    if min(T, Q, K, h, w, H0, W0) < 1:
        raise ValueError("label_objects: empty extent")
    dev = pm[0].device
    out = _out_tensor(out, "label_objects: out [T,H0,W0]", torch.uint8, (T, H0, W0), dev)
    best_out = _out_tensor(best_out, "label_objects: best_out [n]", torch.int32, (n,), dev)
    table = (LabelObj * n)()  # read by the entry point on the host, at this call
    for k in range(n):
        table[k].logits, table[k].masks = lg[k].data_ptr(), pm[k].data_ptr()
    check(lib().tce_label_objects_u8(table, n, out.data_ptr(), best_out.data_ptr(), T, Q, K, h, w, H0, W0, float(threshold),
                                     float(background), _stream()), "tce_label_objects_u8")
    return out, best_out


def a2d_masks(pred_masks, size, orig_size, threshold=0.5, out=None):
    """Dataset-size binary masks of one A2D-Sentences / JHMDB-Sentences sample (postprocessors.py:39-47) on the GPU, one launch:
    pred_masks [N,h,w] (outputs['pred_masks'][b,0]), size = the un-padded model-input size (targets['size']), orig_size = the
    dataset's frame size -> uint8 [N,H0,W0] of 0/1.  The view's address goes to the launch as it is, so it must be contiguous
    float32 on the GPU.  out: write into this (any address) instead of a new tensor."""
    t = pred_masks
    if not torch.is_tensor(t) or t.dim() != 3:
        raise ValueError("a2d_masks: pred_masks must be one sample's [N,h,w] tensor")
    _gpu_tensor(t, "a2d_masks", "pred_masks", torch.float32)
    N, h, w = (int(s) for s in t.shape)
    fh, fw = int(size[0]), int(size[1])
    H0, W0 = int(orig_size[0]), int(orig_size[1])
    if min(N, h, w, fh, fw, H0, W0) < 1:
        raise ValueError("a2d_masks: empty extent")
    if fh > 4 * h or fw > 4 * w:
        raise ValueError(f"a2d_masks: size {(fh, fw)} exceeds 4x the mask plane {(h, w)}")
    if N * H0 * W0 >= 2 ** 31 - 4096:
        raise ValueError("a2d_masks: the output must stay below 2^31 elements")
    out = _out_tensor(out, "a2d_masks: out [N,H0,W0]", torch.uint8, (N, H0, W0), t.device)
    check(lib().tce_a2d_masks_u8(t.data_ptr(), out.data_ptr(), N, h, w, fh, fw, H0, W0, float(threshold), _stream()),
          "tce_a2d_masks_u8")
    return out


def a2d_group_masks(pred_masks_list, logits_list, sizes, orig_sizes, threshold=0.5, outs=None):
    """ops.a2d_masks and ops.sigmoid for the B samples of a group in ONE launch per A2D_GROUP_MAX samples
    (include/tce_rvos_eval.h).  pred_masks_list: B tensors [N,h,w] of one shape (each sample's outputs['pred_masks'][b,0]);
    logits_list: B tensors [N] (outputs['pred_logits'][b,0,:,0]: a strided view is taken as it is); sizes / orig_sizes: B pairs
    (the un-padded model-input size, the dataset's frame size) -> (masks: B uint8 [N,H0_b,W0_b] of 0/1, scores: B float32 [N]).
    Every output byte is ops.a2d_masks', every score ops.sigmoid's.  The tensors' addresses go into the launch's table as they are,
    so the masks must be contiguous float32 on the GPU.  outs: B tensors to write the masks into (any address) instead of new ones."""
    pm, lg = list(pred_masks_list), list(logits_list)
    B = len(pm)
    if B < 1:
        raise ValueError("a2d_group_masks: at least one sample")
    if not (len(lg) == len(sizes) == len(orig_sizes) == B) or (outs is not None and len(outs) != B):
        raise ValueError(f"a2d_group_masks: {B} pred_masks but {len(lg)} logits, {len(sizes)} sizes, {len(orig_sizes)} original sizes"
                         + ("" if outs is None else f", {len(outs)} outs"))
    t0 = pm[0]
    if not torch.is_tensor(t0) or t0.dim() != 3:
        raise ValueError("a2d_group_masks: pred_masks must be one [N,h,w] tensor per sample")
    N, h, w = (int(s) for s in t0.shape)
    dev = t0.device
    geo = []
    for b in range(B):
        t, l = pm[b], lg[b]
        if not torch.is_tensor(t) or tuple(t.shape) != (N, h, w):
            raise ValueError(f"a2d_group_masks: sample {b} has pred_masks {tuple(getattr(t, 'shape', ()))}, sample 0 has {(N, h, w)}")
        _gpu_tensor(t, "a2d_group_masks", f"pred_masks[{b}]", torch.float32, device=dev)
        if not torch.is_tensor(l) or l.dim() != 1 or int(l.shape[0]) != N or l.dtype != torch.float32 or l.device != dev:
            raise ValueError(f"a2d_group_masks: logits[{b}] must be a float32 [N = {N}] tensor on the masks' device")
        fh, fw = int(sizes[b][0]), int(sizes[b][1])
        H0, W0 = int(orig_sizes[b][0]), int(orig_sizes[b][1])
        if min(N, h, w, fh, fw, H0, W0) < 1:
            raise ValueError("a2d_group_masks: empty extent")
        if fh > 4 * h or fw > 4 * w:
            raise ValueError(f"a2d_group_masks: size {(fh, fw)} of sample {b} exceeds 4x the mask plane {(h, w)}")
        if N * H0 * W0 >= 2 ** 31 - 4096:
            raise ValueError("a2d_group_masks: an output must stay below 2^31 elements")
        geo.append((fh, fw, H0, W0))
    res = [_out_tensor(None if outs is None else outs[b], f"a2d_group_masks: outs[{b}] [N,H0,W0]", torch.uint8, (N, g[2], g[3]), dev)
           for b, g in enumerate(geo)]
    scores = torch.empty(B, N, dtype=torch.float32, device=dev)
    st = _stream()
    for lo in range(0, B, A2D_GROUP_MAX):
        n = min(A2D_GROUP_MAX, B - lo)
        table = (A2dGroupSample * n)()  # read by the entry point on the host, at this call
        for k in range(n):
            b, e = lo + k, table[k]
            e.masks, e.logits, e.out, e.scores = pm[b].data_ptr(), lg[b].data_ptr(), res[b].data_ptr(), scores[b].data_ptr()
            e.fh, e.fw, e.H0, e.W0 = geo[b]
            e.logit_stride = max(1, int(lg[b].stride(0)))
        check(lib().tce_a2d_group_masks_u8(table, n, N, h, w, float(threshold), st), "tce_a2d_group_masks_u8")
    return res, list(scores.unbind(0))


def refexp_group(logits_list, boxes_list, masks_list, sizes, orig_sizes, threshold=0.5, outs=None, order=None):
    """The reference's PostProcess and PostProcessSegm (postprocessors.py:72-100, 128-152) for B samples on the GPU, at most two
    launches per REFEXP_GROUP_MAX samples (include/tce_rvos_refexp.h).  logits_list: B tensors [Q,K] (outputs['pred_logits'][b]
    flattened over frames and queries); boxes_list: B tensors [Q,4] cxcywh; masks_list: B tensors [Q,h,w] of one shape, or None for
    a box-only call (sizes may be None then); sizes / orig_sizes: B pairs (the un-padded model-input size, the original image size)
    -> (scores, order, boxes, masks), each a list of B tensors: float32 [Q] descending, int32 [Q] flat candidate indices
    (topk_indexes; ties go to the lower index), float32 [Q,4] xyxy in pixels of the original image, uint8 [Q,H0_b,W0_b] of 0/1
    (masks is None for a box-only call).  The tensors' addresses go into the launch's table as they are, so every input must be
    contiguous float32 on the GPU.  outs: B tensors to write the masks into (any address) instead of new ones.
    order: B int32 [Q] tensors that an earlier (box-only) call on the same logits returned -- a ranked call: the ranking is not
    launched again, masks are required, and scores, order and boxes come back as None, the given order and None."""
    lg, bx = list(logits_list), list(boxes_list)
    pm = None if masks_list is None else list(masks_list)
    B = len(lg)
    if B < 1:
        raise ValueError("refexp_group: at least one sample")
    if not (len(bx) == len(orig_sizes) == B) or (pm is not None and (len(pm) != B or sizes is None or len(sizes) != B)) \
            or (outs is not None and len(outs) != B):
        raise ValueError(f"refexp_group: {B} logits but {len(bx)} boxes, {len(orig_sizes)} original sizes"
                         + ("" if pm is None else f", {len(pm)} masks, {0 if sizes is None else len(sizes)} sizes")
                         + ("" if outs is None else f", {len(outs)} outs"))
    if outs is not None and pm is None:
        raise ValueError("refexp_group: outs without masks (a box-only call writes no masks)")
    if order is not None and (pm is None or len(order) != B):
        raise ValueError("refexp_group: a ranked call (order given) takes masks and one order per sample")
    t0 = lg[0]
    if not torch.is_tensor(t0) or t0.dim() != 2:
        raise ValueError("refexp_group: logits must be one [Q,K] tensor per sample")
    Q, K = (int(s) for s in t0.shape)
    if Q < 1 or K < 1 or Q * K > REFEXP_MAX_CAND:
        raise ValueError(f"refexp_group: 1..{REFEXP_MAX_CAND} candidates (Q*K) per sample, got {Q} x {K}")
    dev = t0.device
    h = w = 0
    if pm is not None:
        if not torch.is_tensor(pm[0]) or pm[0].dim() != 3:
            raise ValueError("refexp_group: masks must be one [Q,h,w] tensor per sample")
        h, w = int(pm[0].shape[1]), int(pm[0].shape[2])
    geo = []
    named = [[(lg[b], "logits", (Q, K)), (bx[b], "boxes", (Q, 4))] + ([] if pm is None else [(pm[b], "masks", (Q, h, w))])
             for b in range(B)]
    for b in range(B):  # the shapes of all samples before anything else is looked at
        for t, name, shape in named[b]:
            if not torch.is_tensor(t) or tuple(t.shape) != shape:
                raise ValueError(f"refexp_group: {name}[{b}] has shape {tuple(getattr(t, 'shape', ()))}, expected {shape}")
    for b in range(B):
        for t, name, shape in named[b]:
            _gpu_tensor(t, "refexp_group", f"{name}[{b}]", torch.float32, device=dev)
        H0, W0 = int(orig_sizes[b][0]), int(orig_sizes[b][1])
        fh, fw = (0, 0) if pm is None else (int(sizes[b][0]), int(sizes[b][1]))
        if min(H0, W0) < 1 or (pm is not None and min(h, w, fh, fw) < 1):
            raise ValueError("refexp_group: empty extent")
        if pm is not None and (fh > 4 * h or fw > 4 * w):
            raise ValueError(f"refexp_group: size {(fh, fw)} of sample {b} exceeds 4x the mask plane {(h, w)}")
        if pm is not None and Q * H0 * W0 >= 2 ** 31 - 4096:
            raise ValueError("refexp_group: an output must stay below 2^31 elements")
        geo.append((fh, fw, H0, W0))
    res = None if pm is None else [_out_tensor(None if outs is None else outs[b], f"refexp_group: outs[{b}] [Q,H0,W0]", torch.uint8,
                                               (Q, g[2], g[3]), dev) for b, g in enumerate(geo)]
    ranked = order is not None
    if ranked:
        order = list(order)
        for b, t in enumerate(order):
            if not torch.is_tensor(t) or tuple(t.shape) != (Q,) or t.dtype != torch.int32 or not t.is_contiguous() or t.device != dev:
                raise ValueError(f"refexp_group: order[{b}] must be a contiguous int32 [Q = {Q}] tensor on the inputs' device")
        scores = boxes = None
    else:
        scores = torch.empty(B, Q, dtype=torch.float32, device=dev)
        order = torch.empty(B, Q, dtype=torch.int32, device=dev)
        boxes = torch.empty(B, Q, 4, dtype=torch.float32, device=dev)
    st = _stream()
    for lo in range(0, B, REFEXP_GROUP_MAX):
        n = min(REFEXP_GROUP_MAX, B - lo)
        table = (RefexpSample * n)()  # read by the entry point on the host, at this call
        for k in range(n):
            b, e = lo + k, table[k]
            e.order = order[b].data_ptr()
            if not ranked:
                e.logits, e.boxes_in, e.scores, e.boxes_out = lg[b].data_ptr(), bx[b].data_ptr(), scores[b].data_ptr(), boxes[b].data_ptr()
            if pm is not None:
                e.masks, e.out = pm[b].data_ptr(), res[b].data_ptr()
            e.fh, e.fw, e.H0, e.W0 = geo[b]
        check(lib().tce_refexp_group_u8(table, n, Q, K, h, w, float(threshold), st), "tce_refexp_group_u8")
    if ranked:
        return None, order, None, res
    return list(scores.unbind(0)), list(order.unbind(0)), list(boxes.unbind(0)), res


def refexp_giou(boxes, gt, giou=None, best=None):
    """Generalised IoU (util/box_ops.py:44-81 in fp32, operation for operation) of boxes [M,Q,4] against the one ground-truth box
    gt [M,4] of each image, all xyxy, and its running maximum over the Q boxes in their order -> (giou [M,Q], best [M,Q]) float32:
    best[m, k-1] >= thresh_iou is the hit of refexp_eval.py:67 at k.  One launch; M <= 65535, Q <= 1024."""
    for t, name, dims in ((boxes, "boxes [M,Q,4]", 3), (gt, "gt [M,4]", 2)):
        if not torch.is_tensor(t) or t.dim() != dims or int(t.shape[-1]) != 4:
            raise ValueError(f"refexp_giou: {name} expected, got {tuple(getattr(t, 'shape', ()))}")
    for t, name in ((boxes, "boxes [M,Q,4]"), (gt, "gt [M,4]")):
        _gpu_tensor(t, "refexp_giou", name, torch.float32, device=boxes.device)
    M, Q = int(boxes.shape[0]), int(boxes.shape[1])
    if int(gt.shape[0]) != M:
        raise ValueError(f"refexp_giou: {M} images of boxes but {int(gt.shape[0])} ground-truth boxes")
    if not (1 <= M <= 65535 and 1 <= Q <= 1024):
        raise ValueError(f"refexp_giou: 1..65535 images of 1..1024 boxes per call, got {M} x {Q}")
    giou = _out_tensor(giou, "refexp_giou: giou [M,Q]", torch.float32, (M, Q), boxes.device)
    best = _out_tensor(best, "refexp_giou: best [M,Q]", torch.float32, (M, Q), boxes.device)
    check(lib().tce_refexp_giou_f32(boxes.data_ptr(), gt.data_ptr(), giou.data_ptr(), best.data_ptr(), M, Q, _stream()),
          "tce_refexp_giou_f32")
    return giou, best


def rle_counts(masks, counts=None, nruns=None, ws=None):
    """Uncompressed COCO run lengths (cocoapi rleEncode, column-major) of uint8 masks [P,H,W] on the GPU -> (counts uint32-valued
    int32 [P,H*W+1], nruns int32 [P]): row p holds its nruns[p] counts, zeros behind them.  Two launches, no host read-back."""
    t = _gpu_tensor(masks, "rle_counts", "masks", torch.uint8, "P,H,W")
    P, H, W = (int(s) for s in t.shape)
    nbytes = lib().tce_rle_ws_bytes(P, H, W) if min(P, H, W) >= 1 and P <= 65535 else -1
    if nbytes < 0:
        raise ValueError(f"rle_counts: unsupported extents {(P, H, W)}")
    dev = t.device
    counts = _out_tensor(counts, "rle_counts: counts [P,H*W+1]", torch.int32, (P, H * W + 1), dev)  # no uint32 arithmetic in torch
    nruns = _out_tensor(nruns, "rle_counts: nruns [P]", torch.int32, (P,), dev)
    ws = _workspace(ws, "rle_counts", nbytes, dev)
    check(lib().tce_rle_counts_u32(t.data_ptr(), counts.data_ptr(), nruns.data_ptr(), ws.data_ptr(), P, H, W, _stream()),
          "tce_rle_counts_u32")
    return counts, nruns


def jf_counts(pred, gt, n, radius, counts=None, ws=None):
    """The six counts behind Ref-DAVIS J&F (include/tce_rvos_score.h) of every (object, frame) pair of two uint8 label-map stacks
    [T,H,W] on the GPU -> int32 [n,T,6]: intersection, union, the two boundary sizes, fg_match, gt_match.  Two launches, no host
    read-back.  The views' addresses go to the launch as they are (any address), so both must be contiguous."""
    for name, t in (("pred", pred), ("gt", gt)):
        _gpu_tensor(t, "jf_counts", name, torch.uint8, "T,H,W")
    if tuple(pred.shape) != tuple(gt.shape) or pred.device != gt.device:
        raise ValueError(f"jf_counts: pred {tuple(pred.shape)} on {pred.device} and gt {tuple(gt.shape)} on {gt.device} must have "
                         f"the same shape and device")
    T, H, W = (int(s) for s in pred.shape)
    n, radius = int(n), int(radius)
    nbytes = lib().tce_jf_ws_bytes(T, n, H, W, radius) if min(T, H, W) >= 1 and T * H * W < 2 ** 31 else -1
    if nbytes < 0:
        raise ValueError(f"jf_counts: unsupported extents {(T, H, W)}, n = {n} (1 .. 16) or radius = {radius} (0 .. 40)")
    dev = pred.device
    counts = _out_tensor(counts, "jf_counts: counts [n,T,6]", torch.int32, (n, T, 6), dev)
    ws = _workspace(ws, "jf_counts", nbytes, dev)
    check(lib().tce_jf_counts_i32(pred.data_ptr(), gt.data_ptr(), counts.data_ptr(), ws.data_ptr(), T, n, H, W, radius, _stream()),
          "tce_jf_counts_i32")
    return counts


def rle_decode(counts, nruns, hw, out=None, ws=None):
    """Planes of P run-length masks on the GPU (include/tce_rvos_score.h: cocoapi rleDecode, the inverse of rle_counts):
    counts int32 [P,stride] (uint32-valued, as rle_counts leaves them; any stride >= 1), nruns int32 [P], hw = (H, W) -> uint8
    [P,H,W] of 0/1.  Three launches, no host read-back: nruns is read on the device.  out: write into this (any address, e.g. a
    slice of a slab) instead of a new tensor."""
    for name, t, dims in (("counts", counts, "P,stride"), ("nruns", nruns, "P")):
        _gpu_tensor(t, "rle_decode", name, torch.int32, dims)
    P, stride = (int(s) for s in counts.shape)
    if int(nruns.shape[0]) != P or nruns.device != counts.device:
        raise ValueError(f"rle_decode: counts {tuple(counts.shape)} on {counts.device} and nruns {tuple(nruns.shape)} on "
                         f"{nruns.device} must agree in P and device")
    H, W = int(hw[0]), int(hw[1])
    nbytes = lib().tce_rle_decode_ws_bytes(P, H, W, stride) if min(P, H, W, stride) >= 1 and H * W < 2 ** 31 else -1
    if nbytes < 0:
        raise ValueError(f"rle_decode: unsupported extents P = {P} (1 .. 65535), (H, W) = {(H, W)} (below 2^31 - 4096 pixels), "
                         f"stride = {stride}")
    dev = counts.device
    out = _out_tensor(out, "rle_decode: out [P,H,W]", torch.uint8, (P, H, W), dev)
    ws = _workspace(ws, "rle_decode", nbytes, dev)
    check(lib().tce_rle_decode_u8(counts.data_ptr(), nruns.data_ptr(), out.data_ptr(), ws.data_ptr(), P, H, W, stride, _stream()),
          "tce_rle_decode_u8")
    return out


def mask_overlap(pred, gt, counts=None, ws=None):
    """Overlap counts of N uint8 prediction planes [N,H,W] against one ground-truth plane [H,W] on the GPU
    (include/tce_rvos_score.h) -> int32 [N,3]: per prediction (intersection, prediction area, ground-truth area), any nonzero
    byte counting as set.  Two launches, no host read-back.  The views' addresses go to the launch as they are (any address), so
    both must be contiguous.  counts: write into this (e.g. a slice of a slab) instead of a new tensor."""
    for name, t, dims in (("pred", pred, "N,H,W"), ("gt", gt, "H,W")):
        _gpu_tensor(t, "mask_overlap", name, torch.uint8, dims)
    if tuple(pred.shape[1:]) != tuple(gt.shape) or pred.device != gt.device:
        raise ValueError(f"mask_overlap: pred {tuple(pred.shape)} on {pred.device} and gt {tuple(gt.shape)} on {gt.device} must "
                         f"have the same plane and device")
    N, H, W = (int(s) for s in pred.shape)
    nbytes = lib().tce_mask_overlap_ws_bytes(N, H, W) if min(N, H, W) >= 1 and H * W < 2 ** 31 else -1
    if nbytes < 0:
        raise ValueError(f"mask_overlap: unsupported extents N = {N} (1 .. 65535), (H, W) = {(H, W)} (below 2^31 - 4096 pixels)")
    dev = pred.device
    counts = _out_tensor(counts, "mask_overlap: counts [N,3]", torch.int32, (N, 3), dev)
    ws = _workspace(ws, "mask_overlap", nbytes, dev)
    check(lib().tce_mask_overlap_i32(pred.data_ptr(), gt.data_ptr(), counts.data_ptr(), ws.data_ptr(), N, H, W, _stream()),
          "tce_mask_overlap_i32")
    return counts


def png_deflate(planes, rows_per_strip=8, nonzero_value=0, streams=None, nbytes=None, ws=None, codes="fixed"):
    """The zlib stream of every uint8 plane [P,H,W] on the GPU (include/tce_rvos_png.h: PNG filter type 0 on every row, RLE-only
    deflate with the fixed Huffman code in strips of rows_per_strip rows, Adler-32) -> (streams uint8 [P,bound], nbytes int32 [P]):
    row p holds its nbytes[p] bytes; what lies behind them is not written.  nonzero_value = v in 1..255: every nonzero byte is
    encoded as v (0/1 masks as 0/255); 0: bytes as they are (label maps).  Three launches, no host read-back.  The planes' address
    goes to the launch as it is (any address), so they must be contiguous.  codes = "dynamic": every strip's block with the cheaper
    of the fixed code and a Huffman code of its own (tce_png_deflate_dyn_u8); the same sizes of streams and ws, never more bytes."""
    if codes not in ("fixed", "dynamic"):
        raise ValueError(f"png_deflate: codes must be 'fixed' or 'dynamic', got {codes!r}")
    entry = "tce_png_deflate_u8" if codes == "fixed" else "tce_png_deflate_dyn_u8"
    t = _gpu_tensor(planes, "png_deflate", "planes", torch.uint8, "P,H,W")
    P, H, W = (int(s) for s in t.shape)
    S, v = int(rows_per_strip), int(nonzero_value)
    if not 0 <= v <= 255:
        raise ValueError(f"png_deflate: nonzero_value = {v} outside 0 .. 255")
    ok = min(P, H, W, S) >= 1 and H * W < 2 ** 31 and S < 2 ** 31
    bound = lib().tce_png_stream_bound(H, W, S) if ok else -1
    need = lib().tce_png_ws_bytes(P, H, W, S) if ok else -1
    if bound < 0 or need < 0:
        raise ValueError(f"png_deflate: unsupported extents P = {P} (1 .. 65535), (H, W) = {(H, W)} (below 2^31 pixels, the stream "
                         f"bound below 2^31 bytes), rows_per_strip = {S} (>= 1, at most 2^22 strips)")
    dev = t.device
    streams = _out_tensor(streams, "png_deflate: streams [P,bound]", torch.uint8, (P, bound), dev)
    nbytes = _out_tensor(nbytes, "png_deflate: nbytes [P]", torch.int32, (P,), dev)
    ws = _workspace(ws, "png_deflate", need, dev)
    check(getattr(lib(), entry)(t.data_ptr(), streams.data_ptr(), nbytes.data_ptr(), ws.data_ptr(), P, H, W, S, v, _stream()), entry)
    return streams, nbytes


def png_filter_rgb(images, rows=None):
    """The filtered rows of uint8 RGB images [P,H,W,3] on the GPU (tce_png_filter_rgb_u8) -> rows uint8 [P,H,1+3W]: per row its PNG
    filter type (the one with the least sum of absolute signed filtered bytes, ties to the lowest) and its bytes filtered with it.
    One launch, no host read-back."""
    t = _gpu_tensor(images, "png_filter_rgb", "images", torch.uint8, "P,H,W,3")
    P, H, W, C = (int(s) for s in t.shape)
    if C != 3 or min(P, H, W) < 1 or P > 65535 or W > 2 ** 24 or H * (3 * W + 1) >= 2 ** 31 - 4096:
        raise ValueError(f"png_filter_rgb: unsupported extents {tuple(t.shape)} (P in 1 .. 65535, 3 channels, W <= 2^24, "
                         f"H * (3W + 1) < 2^31 - 4096)")
    rows = _out_tensor(rows, "png_filter_rgb: rows [P,H,1+3W]", torch.uint8, (P, H, 1 + 3 * W), t.device)
    check(lib().tce_png_filter_rgb_u8(t.data_ptr(), rows.data_ptr(), P, H, W, _stream()), "tce_png_filter_rgb_u8")
    return rows


def png_deflate_rows(rows, rows_per_strip=32, streams=None, nbytes=None, ws=None):
    """The zlib stream of filtered rows uint8 [P,H,R] on the GPU (tce_png_deflate_rows_u8: png_deflate's dynamic stream over bytes
    that are filtered already, filter byte included) -> (streams uint8 [P,bound], nbytes int32 [P]), bound and the workspace those
    of png_deflate for planes [P,H,R-1].  Three launches, no host read-back."""
    t = _gpu_tensor(rows, "png_deflate_rows", "rows", torch.uint8, "P,H,R")
    P, H, R = (int(s) for s in t.shape)
    S = int(rows_per_strip)
    ok = min(P, H, S) >= 1 and R >= 2 and H * (R - 1) < 2 ** 31 and S < 2 ** 31
    bound = lib().tce_png_stream_bound(H, R - 1, S) if ok else -1
    need = lib().tce_png_ws_bytes(P, H, R - 1, S) if ok else -1
    if bound < 0 or need < 0:
        raise ValueError(f"png_deflate_rows: unsupported extents P = {P} (1 .. 65535), (H, R) = {(H, R)} (R >= 2, below 2^31 bytes, "
                         f"the stream bound below 2^31 bytes), rows_per_strip = {S} (>= 1, at most 2^22 strips)")
    dev = t.device
    streams = _out_tensor(streams, "png_deflate_rows: streams [P,bound]", torch.uint8, (P, bound), dev)
    nbytes = _out_tensor(nbytes, "png_deflate_rows: nbytes [P]", torch.int32, (P,), dev)
    ws = _workspace(ws, "png_deflate_rows", need, dev)
    check(lib().tce_png_deflate_rows_u8(t.data_ptr(), streams.data_ptr(), nbytes.data_ptr(), ws.data_ptr(), P, H, R, S, _stream()),
          "tce_png_deflate_rows_u8")
    return streams, nbytes


PNG_FILE_PIECE = 64       # TCE_PNG_FILE_PIECE (include/tce_rvos_pngfile.h)
PNG_FILE_SEGMENT = 16384  # TCE_PNG_FILE_SEGMENT
PNG_FILE_MIN_HEAD, PNG_FILE_MAX_HEAD = 8, 1024  # TCE_PNG_FILE_MIN_HEAD, TCE_PNG_FILE_MAX_HEAD


def _rows_u8(t, op, name):
    """A uint8 [P,n] tensor on the GPU whose rows are contiguous -> (P, n, row stride); the stride may exceed n (a view)"""
    if not torch.is_tensor(t) or t.dim() != 2 or t.dtype != torch.uint8 or not t.is_cuda:
        raise ValueError(f"{op}: {name} must be a uint8 [P,n] tensor on the GPU")
    P, n = (int(s) for s in t.shape)
    stride = n if P <= 1 else int(t.stride(0))
    if n > 1 and int(t.stride(1)) != 1 or stride < n:
        raise ValueError(f"{op}: the rows of {name} must be contiguous and must not overlap, got strides {tuple(t.stride())}")
    return P, n, stride


def png_file(streams, nbytes, head, files=None, file_bytes=None, ws=None):
    """The finished PNG file around every zlib stream on the GPU (tce_png_file_u8, include/tce_rvos_pngfile.h has the layout): head,
    the IDAT chunk of streams[p, :nbytes[p]] with its length and CRC-32, IEND -> (files uint8 [P,file_bound], file_bytes int32 [P]);
    row p holds its file_bytes[p] = len(head) + 24 + nbytes[p] bytes, what lies behind them is not written.  streams: the [P,bound]
    tensor of png_deflate / png_deflate_rows, or a view of one whose rows are contiguous and lie further apart (the row stride is
    passed on, and file_bound = len(head) + 24 + that stride); nbytes int32 [P].  head: bytes, the same for every file (signature,
    IHDR, PLTE for mode 'P': png.head / png.head_rgb), 8 .. 1024 of them; it goes to the device in a small uint8 tensor (a uint8
    tensor on the GPU is taken as it is: inside a graph capture no host memory can be copied).  files may be a view with a larger
    row stride too and must overlap none of the inputs.  Two launches, no host read-back."""
    P, n, sstride = _rows_u8(streams, "png_file", "streams")
    dev = streams.device
    if not torch.is_tensor(nbytes) or nbytes.dtype != torch.int32 or tuple(nbytes.shape) != (P,) or not nbytes.is_contiguous() or nbytes.device != dev:
        raise ValueError(f"png_file: nbytes must be a contiguous int32 [{P}] on the streams' device")
    if torch.is_tensor(head):
        if head.dtype != torch.uint8 or head.dim() != 1 or not head.is_contiguous() or head.device != dev:
            raise ValueError("png_file: head as a tensor must be a contiguous uint8 [head_bytes] on the streams' device")
        hb = int(head.numel())
    else:
        head = bytes(head)
        hb = len(head)
    if not 1 <= P <= 65535:
        raise ValueError(f"png_file: P = {P} outside 1 .. 65535")
    if not PNG_FILE_MIN_HEAD <= hb <= PNG_FILE_MAX_HEAD:
        raise ValueError(f"png_file: head holds {hb} bytes, outside {PNG_FILE_MIN_HEAD} .. {PNG_FILE_MAX_HEAD}")
    bound = lib().tce_png_file_bound(hb, sstride) if n >= 1 else -1
    need = lib().tce_png_file_ws_bytes(P, sstride) if n >= 1 else -1
    if bound < 0 or need < 0:
        raise ValueError(f"png_file: unsupported extents: rows of {n} bytes, {sstride} apart (at least 1, head + 24 + stride below 2^31 - 4096)")
    if files is None:
        files = torch.empty((P, bound), dtype=torch.uint8, device=dev)
    fP, fn, fstride = _rows_u8(files, "png_file", "files")
    if (fP, fn) != (P, bound) or files.device != dev:
        raise ValueError(f"png_file: files must be {[P, bound]} on the streams' device (tce_png_file_bound), got {list(files.shape)}")
    if fstride >= 2 ** 31 - 4096:
        raise ValueError(f"png_file: the rows of files lie {fstride} bytes apart, not below 2^31 - 4096")
    file_bytes = _out_tensor(file_bytes, "png_file: file_bytes [P]", torch.int32, (P,), dev)
    ws = _workspace(ws, "png_file", need, dev)
    if not torch.is_tensor(head):
        head = torch.frombuffer(bytearray(head), dtype=torch.uint8).to(dev)
    lo, hi = files.data_ptr(), files.data_ptr() + (P - 1) * fstride + bound
    for t, name, nb in ((streams, "streams", P * sstride), (nbytes, "nbytes", 4 * P), (head, "head", hb),
                        (file_bytes, "file_bytes", 4 * P), (ws, "ws", need)):
        if t.data_ptr() < hi and lo < t.data_ptr() + nb:
            raise ValueError(f"png_file: files overlaps {name}")
    check(lib().tce_png_file_u8(streams.data_ptr(), nbytes.data_ptr(), head.data_ptr(), hb, files.data_ptr(), file_bytes.data_ptr(),
                                ws.data_ptr(), P, sstride, fstride, _stream()), "tce_png_file_u8")
    return files, file_bytes


VIS_MAX_LAYERS = 16  # TCE_VIS_MAX_LAYERS (include/tce_rvos_vis.h)


def vis_overlay(frames, colors, masks=None, boxes=None, points=None, out=None):
    """The --visualize image of the reference's drivers on the GPU (tce_vis_overlay_u8, include/tce_rvos_vis.h has the per-pixel
    rule): frames uint8 [N,H0,W0,3] with L layers drawn on them in order -> out uint8 [N,H0,W0,3] (a new tensor, or `out`, which
    must not overlap frames).  Per layer l, each optional: masks uint8 [L,N,H0,W0] (nonzero = tinted), boxes float32 [L,N,4]
    (cx, cy, w, h, normalised), points float32 [L,N,2] (x, y, normalised); colors uint8 [L,3].  One launch, no host read-back."""
    f = _gpu_tensor(frames, "vis_overlay", "frames", torch.uint8, "N,H0,W0,3")
    N, H0, W0, C = (int(s) for s in f.shape)
    dev = f.device
    c = _gpu_tensor(colors, "vis_overlay", "colors", torch.uint8, "L,3")
    L = int(c.shape[0])
    if C != 3 or int(c.shape[1]) != 3 or c.device != dev:
        raise ValueError("vis_overlay: frames must be [N,H0,W0,3] and colors [L,3] on one device")
    if not 1 <= L <= VIS_MAX_LAYERS:
        raise ValueError(f"vis_overlay: 1..{VIS_MAX_LAYERS} layers, got {L}")
    if min(N, H0, W0) < 1 or N > 65535 or H0 * W0 * 3 >= 2 ** 31 - 2048:
        raise ValueError(f"vis_overlay: unsupported extents {tuple(f.shape)} (N in 1 .. 65535, a frame below 2^31 bytes)")
    if masks is not None:
        masks = _gpu_tensor(masks, "vis_overlay", "masks", torch.uint8, "L,N,H0,W0")
        if tuple(masks.shape) != (L, N, H0, W0) or masks.device != dev:
            raise ValueError(f"vis_overlay: masks must be {[L, N, H0, W0]} on the frames' device, got {list(masks.shape)}")
    for t, name, k in ((boxes, "boxes", 4), (points, "points", 2)):
        if t is not None and (not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != (L, N, k) or not t.is_contiguous()
                              or t.device != dev):
            raise ValueError(f"vis_overlay: {name} must be a contiguous float32 {[L, N, k]} on the frames' device")
    out = _out_tensor(out, "vis_overlay: out [N,H0,W0,3]", torch.uint8, (N, H0, W0, 3), dev)
    p = lambda t: None if t is None else t.data_ptr()
    check(lib().tce_vis_overlay_u8(f.data_ptr(), out.data_ptr(), p(masks), p(boxes), p(points), c.data_ptr(), L, N, H0, W0, _stream()),
          "tce_vis_overlay_u8")
    return out
