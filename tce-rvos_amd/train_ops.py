"""Thin tensor plumbing over libtce_rvos_train.so (train/tce_rvos_train.h): the criterion's entry points, forward and backward.  torch owns device
memory and streams, the arithmetic is HIP.  Every rejection here is a ValueError raised before anything is launched.  No fallback."""
import torch

from ._train_lib import MAX_B, MAX_ELEMS, MAX_K, MAX_Q, MAX_T, CriterionConsts, check, lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ceil32(n):
    return (n + 31) // 32 * 32


def _dev(t, op, name, dtype, shape=None, device=None):
    """t: a contiguous GPU tensor of `dtype` (and `shape`, on `device`) that takes no part in autograd"""
    if not torch.is_tensor(t):
        raise ValueError(f"{op}: {name} must be a tensor")
    if not t.is_cuda:
        raise ValueError(f"{op}: {name} is a CPU tensor; the criterion runs on the GPU")
    if t.requires_grad:
        raise ValueError(f"{op}: {name} requires grad; the entry points take no part in autograd and would silently cut the "
                         f"graph (SetCriterion with grad = True is the differentiable form)")
    if t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"{op}: {name} must be a contiguous {dtype} tensor, got {t.dtype}"
                         + ("" if t.is_contiguous() else " (not contiguous)"))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{op}: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    if device is not None and t.device != device:
        raise ValueError(f"{op}: {name} is on {t.device}, expected {device}")
    return t


def _limits(op, B, T, Q, K=1):
    if not (1 <= B <= MAX_B and 1 <= T <= MAX_T and 1 <= Q <= MAX_Q and 1 <= K <= MAX_K):
        raise ValueError(f"{op}: limits exceeded: 1..{MAX_B} clips of 1..{MAX_T} frames, 1..{MAX_Q} queries, 1..{MAX_K} class logits; "
                         f"got B={B} T={T} Q={Q} K={K}")


def check_mask_shape(op, h, w, H, W):
    if 4 * h != _ceil32(H) or 4 * w != _ceil32(W):
        raise ValueError(f"{op}: the mask plane {h} x {w} is not a quarter of the target masks' {H} x {W} padded to a multiple of 32 "
                         f"(expected {_ceil32(H) // 4} x {_ceil32(W) // 4})")


def criterion_mask_sums(pred_masks, masks, alpha=0.25, ws=None):
    """The three sums per query behind the matcher's mask costs and behind loss_mask / loss_dice (matcher.py:15-42,
    segmentation.py:467-510), and the target count: pred_masks [B,T,Q,h,w] float32 in the model's layout, masks [B,T,H,W] uint8 0/1
    un-padded -> (sums [B,3,Q] float64 = S_f, S_p, S_pt; st [B] float64 = S_t).  Two launches, one read of pred_masks."""
    op = "criterion_mask_sums"
    if not torch.is_tensor(pred_masks) or pred_masks.dim() != 5:
        raise ValueError(f"{op}: pred_masks [B,T,Q,h,w] expected, got {tuple(getattr(pred_masks, 'shape', ()))}")
    B, T, Q, h, w = (int(s) for s in pred_masks.shape)
    _dev(pred_masks, op, "pred_masks", torch.float32)
    if not torch.is_tensor(masks) or masks.dim() != 4 or int(masks.shape[0]) != B or int(masks.shape[1]) != T:
        raise ValueError(f"{op}: masks [B,T,H,W] = [{B},{T},H,W] expected, got {tuple(getattr(masks, 'shape', ()))}")
    _dev(masks, op, "masks", torch.uint8, device=pred_masks.device)
    H, W = int(masks.shape[2]), int(masks.shape[3])
    _limits(op, B, T, Q)
    if min(h, w, H, W) < 1 or T * h * w >= MAX_ELEMS:
        raise ValueError(f"{op}: limits exceeded: 1 <= T*h*w < 2^30, got {T} x {h} x {w}")
    check_mask_shape(op, h, w, H, W)
    l = lib()
    need = int(l.tce_criterion_mask_sums_ws_bytes(B, T, Q, h, w))
    if ws is None:
        ws = torch.empty(need // 8, dtype=torch.float64, device=pred_masks.device)
    elif _dev(ws, op, "ws", torch.float64, device=pred_masks.device).numel() * 8 < need:
        raise ValueError(f"{op}: ws holds {ws.numel() * 8} bytes, {need} needed")
    sums = torch.empty(B, 3, Q, dtype=torch.float64, device=pred_masks.device)
    st = torch.empty(B, dtype=torch.float64, device=pred_masks.device)
    check(l.tce_criterion_mask_sums_f64(pred_masks.data_ptr(), masks.data_ptr(), sums.data_ptr(), st.data_ptr(), ws.data_ptr(),
                                        B, T, Q, h, w, H, W, float(alpha), _stream()), "tce_criterion_mask_sums_f64")
    return sums, st


def criterion_match_losses(pred_logits, pred_boxes, labels, boxes, valid, num_boxes, pred_visible=None, sums=None, st=None, hw=None,
                           cost_class=2.0, cost_bbox=5.0, cost_giou=2.0, cost_mask=2.0, cost_dice=5.0, cost_vis=2.0,
                           focal_alpha=0.25):
    """The matcher's cost column (matcher.py:141-231), the match (ties to the lower index) and the losses of criterion.py:41-192 for B
    clips: pred_logits [B,T,Q,K], pred_boxes [B,T,Q,4], pred_visible [B,T,Q,1] or None, sums / st of criterion_mask_sums with hw =
    (h, w) or None, labels [B,T] int64, boxes [B,T,4] cxcywh, valid [B,T] int32, num_boxes: a one-element float32 device tensor
    -> (cost [B,Q] float32, index [B] int32, parts [B,6] float64, losses [6] float32 in the order loss_ce, loss_bbox, loss_giou,
    loss_mask, loss_dice, loss_vis).  Two launches."""
    op = "criterion_match_losses"
    if not torch.is_tensor(pred_logits) or pred_logits.dim() != 4:
        raise ValueError(f"{op}: pred_logits [B,T,Q,K] expected, got {tuple(getattr(pred_logits, 'shape', ()))}")
    B, T, Q, K = (int(s) for s in pred_logits.shape)
    dev = pred_logits.device
    _dev(pred_logits, op, "pred_logits", torch.float32)
    _dev(pred_boxes, op, "pred_boxes", torch.float32, (B, T, Q, 4), dev)
    if pred_visible is not None:
        _dev(pred_visible, op, "pred_visible", torch.float32, (B, T, Q, 1), dev)
    _dev(labels, op, "labels", torch.int64, (B, T), dev)
    _dev(boxes, op, "boxes", torch.float32, (B, T, 4), dev)
    _dev(valid, op, "valid", torch.int32, (B, T), dev)
    _dev(num_boxes, op, "num_boxes", torch.float32, device=dev)
    if num_boxes.numel() != 1:
        raise ValueError(f"{op}: num_boxes must hold one element")
    _limits(op, B, T, Q, K)
    if (sums is None) != (st is None) or (sums is not None and hw is None):
        raise ValueError(f"{op}: sums, st and hw come together or not at all")
    h = w = 0
    if sums is not None:
        h, w = int(hw[0]), int(hw[1])
        _dev(sums, op, "sums", torch.float64, (B, 3, Q), dev)
        _dev(st, op, "st", torch.float64, (B,), dev)
        if min(h, w) < 1 or T * h * w >= MAX_ELEMS:
            raise ValueError(f"{op}: limits exceeded: 1 <= T*h*w < 2^30, got {T} x {h} x {w}")
    consts = CriterionConsts(float(cost_class), float(cost_bbox), float(cost_giou), float(cost_mask), float(cost_dice), float(cost_vis),
                             float(focal_alpha))
    cost = torch.empty(B, Q, dtype=torch.float32, device=dev)
    index = torch.empty(B, dtype=torch.int32, device=dev)
    parts = torch.empty(B, 6, dtype=torch.float64, device=dev)
    losses = torch.empty(6, dtype=torch.float32, device=dev)
    check(lib().tce_criterion_match_losses_f32(
        pred_logits.data_ptr(), pred_boxes.data_ptr(), None if pred_visible is None else pred_visible.data_ptr(),
        None if sums is None else sums.data_ptr(), None if st is None else st.data_ptr(), labels.data_ptr(), boxes.data_ptr(),
        valid.data_ptr(), num_boxes.data_ptr(), cost.data_ptr(), index.data_ptr(), parts.data_ptr(), losses.data_ptr(),
        B, T, Q, K, h, w, consts, _stream()), "tce_criterion_match_losses_f32")
    return cost, index, parts, losses


def _out(out, op, name, shape, dev):
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=dev)
    return _dev(out, op, name, torch.float32, shape, dev)


def _gl(op, num_boxes, gl, dev):
    _dev(num_boxes, op, "num_boxes", torch.float32, device=dev)
    if num_boxes.numel() != 1:
        raise ValueError(f"{op}: num_boxes must hold one element")
    _dev(gl, op, "gl", torch.float32, (6,), dev)


def criterion_mask_grad(pred_masks, masks, sums, st, index, num_boxes, gl, alpha=0.25, out=None):
    """d L / d pred_masks of loss_mask and loss_dice (train/tce_rvos_train.h (c)): pred_masks [B,T,Q,h,w] float32, masks [B,T,H,W]
    uint8, sums [B,3,Q] / st [B] float64 of criterion_mask_sums, index [B] int32 of criterion_match_losses, num_boxes a one-element
    float32 device tensor, gl [6] float32 = dL/d losses on the device -> grad [B,T,Q,h,w] float32 (`out` if given).  One launch;
    the planes of the unmatched queries are +0.0."""
    op = "criterion_mask_grad"
    if not torch.is_tensor(pred_masks) or pred_masks.dim() != 5:
        raise ValueError(f"{op}: pred_masks [B,T,Q,h,w] expected, got {tuple(getattr(pred_masks, 'shape', ()))}")
    B, T, Q, h, w = (int(s) for s in pred_masks.shape)
    dev = pred_masks.device
    _dev(pred_masks, op, "pred_masks", torch.float32)
    if not torch.is_tensor(masks) or masks.dim() != 4 or int(masks.shape[0]) != B or int(masks.shape[1]) != T:
        raise ValueError(f"{op}: masks [B,T,H,W] = [{B},{T},H,W] expected, got {tuple(getattr(masks, 'shape', ()))}")
    _dev(masks, op, "masks", torch.uint8, device=dev)
    H, W = int(masks.shape[2]), int(masks.shape[3])
    _limits(op, B, T, Q)
    if min(h, w, H, W) < 1 or T * h * w >= MAX_ELEMS:
        raise ValueError(f"{op}: limits exceeded: 1 <= T*h*w < 2^30, got {T} x {h} x {w}")
    check_mask_shape(op, h, w, H, W)
    _dev(sums, op, "sums", torch.float64, (B, 3, Q), dev)
    _dev(st, op, "st", torch.float64, (B,), dev)
    _dev(index, op, "index", torch.int32, (B,), dev)
    _gl(op, num_boxes, gl, dev)
    grad = _out(out, op, "out", (B, T, Q, h, w), dev)
    check(lib().tce_criterion_mask_grad_f32(pred_masks.data_ptr(), masks.data_ptr(), sums.data_ptr(), st.data_ptr(), index.data_ptr(),
                                            num_boxes.data_ptr(), gl.data_ptr(), grad.data_ptr(), B, T, Q, h, w, H, W, float(alpha),
                                            _stream()), "tce_criterion_mask_grad_f32")
    return grad


def criterion_head_grads(pred_logits, pred_boxes, labels, boxes, valid, index, num_boxes, gl, pred_visible=None, focal_alpha=0.25,
                         want=(True, True, False), out=(None, None, None)):
    """d L / d (pred_logits, pred_boxes, pred_visible) of loss_ce, loss_bbox + loss_giou, loss_vis (train/tce_rvos_train.h (d)).
    Inputs as criterion_match_losses, index [B] int32 of it, gl [6] float32 on the device.  want: which of the three gradients to
    compute; out: tensors to write them to -> (g_logits [B,T,Q,K], g_boxes [B,T,Q,4], g_visible [B,T,Q,1]), None where not wanted.
    One launch."""
    op = "criterion_head_grads"
    if not torch.is_tensor(pred_logits) or pred_logits.dim() != 4:
        raise ValueError(f"{op}: pred_logits [B,T,Q,K] expected, got {tuple(getattr(pred_logits, 'shape', ()))}")
    B, T, Q, K = (int(s) for s in pred_logits.shape)
    dev = pred_logits.device
    _dev(pred_logits, op, "pred_logits", torch.float32)
    _dev(pred_boxes, op, "pred_boxes", torch.float32, (B, T, Q, 4), dev)
    if pred_visible is not None:
        _dev(pred_visible, op, "pred_visible", torch.float32, (B, T, Q, 1), dev)
    _dev(labels, op, "labels", torch.int64, (B, T), dev)
    _dev(boxes, op, "boxes", torch.float32, (B, T, 4), dev)
    _dev(valid, op, "valid", torch.int32, (B, T), dev)
    _dev(index, op, "index", torch.int32, (B,), dev)
    _gl(op, num_boxes, gl, dev)
    _limits(op, B, T, Q, K)
    want = tuple(bool(x) for x in want)
    if len(want) != 3 or len(out) != 3 or not any(want):
        raise ValueError(f"{op}: want and out name the three gradients (logits, boxes, visible), one at least wanted")
    if want[2] and pred_visible is None:
        raise ValueError(f"{op}: the gradient of pred_visible without pred_visible")
    shapes = ((B, T, Q, K), (B, T, Q, 4), (B, T, Q, 1))
    g = [(_out(o, op, f"out[{i}]", s, dev) if wd else None) for i, (wd, o, s) in enumerate(zip(want, out, shapes))]
    consts = CriterionConsts(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, float(focal_alpha))
    check(lib().tce_criterion_head_grads_f32(
        pred_logits.data_ptr(), pred_boxes.data_ptr(), None if pred_visible is None else pred_visible.data_ptr(), labels.data_ptr(),
        boxes.data_ptr(), valid.data_ptr(), index.data_ptr(), num_boxes.data_ptr(), gl.data_ptr(),
        *(None if t is None else t.data_ptr() for t in g), B, T, Q, K, consts, _stream()), "tce_criterion_head_grads_f32")
    return tuple(g)
