"""The reference's SetCriterion (models/criterion.py) and the one-target matcher it calls (models/matcher.py) on the GPU: two entry
points of libtce_rvos_train.so per decoder layer (train/tce_rvos_train.h).  Forward values only by default: an input
that requires grad is rejected.  With `grad = True` the losses are differentiable with respect to the model's outputs, through two
more entry points per layer.  Importing this module loads no library."""
import torch
from torch import nn

from . import train_ops
from ._train_lib import MAX_B, MAX_ELEMS, MAX_K, MAX_Q, MAX_T

_KEYS = ("pred_logits", "pred_boxes", "pred_masks", "pred_visible")
_LOSS_KEYS = {"labels": ("loss_ce",), "boxes": ("loss_bbox", "loss_giou"), "masks": ("loss_mask", "loss_dice"),
              "visible": ("loss_vis",)}
_SLOT = {"loss_ce": 0, "loss_bbox": 1, "loss_giou": 2, "loss_mask": 3, "loss_dice": 4, "loss_vis": 5}  # of the kernel's losses[6]


class _LayerLosses(torch.autograd.Function):
    """losses [6] of one decoder layer as a differentiable function of (pred_logits, pred_boxes, pred_masks | None, pred_visible |
    None).  Forward: the two forward entry points; backward: entry (c) if pred_masks needs a gradient, entry (d) for the others."""

    @staticmethod
    def forward(ctx, crit, tg, hw, num_boxes, logits, boxes, masks, visible):
        out = {"pred_logits": logits.detach(), "pred_boxes": boxes.detach()}
        if masks is not None:
            out["pred_masks"] = masks.detach()
        if visible is not None:
            out["pred_visible"] = visible.detach()
        vals = crit._layer(out, tg, hw, num_boxes)
        ctx.alpha = crit.focal_alpha
        ctx.save_for_backward(logits, boxes, masks, visible, vals["index"], vals["sums"], vals["st"], num_boxes, tg["labels"],
                              tg["boxes"], tg["valid"], tg.get("masks"))
        return vals["losses"]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gl):
        logits, boxes, masks, visible, index, sums, st, num_boxes, labels, tboxes, valid, tmasks = ctx.saved_tensors
        need = ctx.needs_input_grad[4:8]
        gl = gl.detach().to(torch.float32).contiguous()
        g_masks = None
        if need[2]:
            g_masks = train_ops.criterion_mask_grad(masks.detach(), tmasks, sums, st, index, num_boxes, gl, alpha=ctx.alpha)
        g_logits = g_boxes = g_vis = None
        if need[0] or need[1] or need[3]:
            g_logits, g_boxes, g_vis = train_ops.criterion_head_grads(
                logits.detach(), boxes.detach(), labels, tboxes, valid, index, num_boxes, gl,
                pred_visible=None if visible is None else visible.detach(), focal_alpha=ctx.alpha, want=(need[0], need[1], need[3]))
        return None, None, None, None, g_logits, g_boxes, g_masks, g_vis


def _stack_outputs(outputs):
    """A list of per-clip output dicts ([1,T,Q,..] each, what forward_group returns) as one dict of [B,T,Q,..] tensors"""
    if isinstance(outputs, dict):
        return outputs
    if not isinstance(outputs, (list, tuple)) or not outputs or not all(isinstance(o, dict) for o in outputs):
        raise ValueError("SetCriterion: outputs must be the model's output dict or a non-empty list of per-clip output dicts")
    out = {k: torch.cat([o[k] for o in outputs], 0) for k in _KEYS if all(k in o for o in outputs)}
    if all("aux_outputs" in o for o in outputs):
        n = len(outputs[0]["aux_outputs"])
        if any(len(o["aux_outputs"]) != n for o in outputs):
            raise ValueError("SetCriterion: the clips' aux_outputs differ in length")
        out["aux_outputs"] = [_stack_outputs([o["aux_outputs"][i] for o in outputs]) for i in range(n)]
    return out


class SetCriterion(nn.Module):
    """criterion(outputs, targets) -> the loss dict of criterion.py:216-262 (same keys, aux layers as suffix _{i}), every value a
    0-dim float32 device tensor; criterion.matcher(outputs, targets) -> the reference's [(src_idx, tgt_idx)] list.

    outputs: the model's dict ([B,T,Q,..] tensors) or a list of per-clip dicts.  targets: B dicts with masks [T,H,W] (bool / uint8 /
    float 0-1), boxes [T,4] cxcywh, labels [T], valid [T], all on the GPU; all clips of a call share one shape.

    grad (a plain attribute, False by default): when True, the outputs may require grad and every value of the loss dict carries a
    grad_fn back to pred_logits, pred_boxes, pred_masks and pred_visible; the targets still may not require grad, and matcher() and
    layer_values() stay forward only."""

    def __init__(self, num_classes, weight_dict, losses, focal_alpha=0.25, eos_coef=0.1, cost_class=2.0, cost_bbox=5.0, cost_giou=2.0,
                 cost_mask=2.0, cost_dice=5.0, cost_vis=2.0, masks=True, vis=False, grad=False):
        super().__init__()
        self.grad = bool(grad)
        for name in losses:
            if name not in _LOSS_KEYS:
                raise ValueError(f"SetCriterion: do you really want to compute {name} loss?")  # criterion.py:213
        self.num_classes, self.weight_dict, self.losses = num_classes, weight_dict, list(losses)
        self.focal_alpha, self.eos_coef = focal_alpha, eos_coef
        self.cost_class, self.cost_bbox, self.cost_giou = cost_class, cost_bbox, cost_giou
        self.cost_mask, self.cost_dice, self.cost_vis = cost_mask, cost_dice, cost_vis
        self.masks, self.vis = bool(masks), bool(vis)
        self.mask_out_stride = 4
        empty_weight = torch.ones(num_classes + 1)  # criterion.py:35-37: a buffer of the reference's state dict, read by no loss
        empty_weight[-1] = eos_coef
        self.register_buffer("empty_weight", empty_weight)

    # ---- checks that precede device work, then the plumbing: stacking and dtype conversion, no arithmetic on values
    def _layer_inputs(self, out, targets, what):
        for k in ("pred_logits", "pred_boxes"):
            if k not in out:
                raise ValueError(f"SetCriterion: {what} has no {k}")
        need_masks = self.masks or "masks" in self.losses
        need_vis = self.vis or "visible" in self.losses
        if need_masks and "pred_masks" not in out:
            raise ValueError(f"SetCriterion: 'masks' in losses (or the matcher's mask cost) without pred_masks in {what}")
        if need_vis and "pred_visible" not in out:
            raise ValueError(f"SetCriterion: the visible loss (or the matcher's visibility cost) without pred_visible in {what}")
        lg = out["pred_logits"]
        if not torch.is_tensor(lg) or lg.dim() != 4:
            raise ValueError(f"SetCriterion: {what} pred_logits [B,T,Q,K] expected, got {tuple(getattr(lg, 'shape', ()))}")
        B, T, Q, K = (int(s) for s in lg.shape)
        if len(targets) != B:
            raise ValueError(f"SetCriterion: {B} clips of outputs but {len(targets)} targets")
        if need_vis and B > 1:
            raise ValueError("SetCriterion: the visible loss takes one clip per call (the reference's own scatter_ fails at B > 1)")
        if not (1 <= B <= MAX_B and 1 <= T <= MAX_T and 1 <= Q <= MAX_Q and 1 <= K <= MAX_K):
            raise ValueError(f"SetCriterion: limits exceeded: 1..{MAX_B} clips of 1..{MAX_T} frames, 1..{MAX_Q} queries, 1..{MAX_K} "
                             f"class logits; got B={B} T={T} Q={Q} K={K}")
        use = [("pred_logits", (B, T, Q, K)), ("pred_boxes", (B, T, Q, 4))]
        if need_vis:
            use.append(("pred_visible", (B, T, Q, 1)))
        hw = None
        if need_masks:
            pm = out["pred_masks"]
            if not torch.is_tensor(pm) or pm.dim() != 5 or tuple(pm.shape[:3]) != (B, T, Q):
                raise ValueError(f"SetCriterion: {what} pred_masks [{B},{T},{Q},h,w] expected, got {tuple(getattr(pm, 'shape', ()))}")
            hw = (int(pm.shape[3]), int(pm.shape[4]))
            if min(hw) < 1 or T * hw[0] * hw[1] >= MAX_ELEMS:
                raise ValueError(f"SetCriterion: limits exceeded: 1 <= T*h*w < 2^30, got {T} x {hw[0]} x {hw[1]}")
            use.append(("pred_masks", (B, T, Q) + hw))
        for k, shape in use:
            t = out[k]
            if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != torch.float32:
                raise ValueError(f"SetCriterion: {what} {k} must be float32 {shape}, got {getattr(t, 'dtype', None)} "
                                 f"{tuple(getattr(t, 'shape', ()))}")
        return (B, T, Q, K), hw, [k for k, _ in use]

    def _targets(self, targets, B, T, hw):
        shapes = {"boxes": (T, 4), "labels": (T,), "valid": (T,)}
        for b, t in enumerate(targets):
            for k, shape in shapes.items():
                if k not in t or not torch.is_tensor(t[k]) or tuple(t[k].shape) != shape:
                    raise ValueError(f"SetCriterion: targets[{b}]['{k}'] {shape} expected, got "
                                     f"{tuple(getattr(t.get(k), 'shape', ()))}")
            if hw is not None:
                m = t.get("masks")
                if not torch.is_tensor(m) or m.dim() != 3 or int(m.shape[0]) != T or tuple(m.shape) != tuple(targets[0]["masks"].shape):
                    raise ValueError(f"SetCriterion: targets[{b}]['masks'] [T,H,W] of one shape for all clips expected, got "
                                     f"{tuple(getattr(m, 'shape', ()))}")
        if hw is not None:
            H, W = (int(s) for s in targets[0]["masks"].shape[1:])
            train_ops.check_mask_shape("SetCriterion", hw[0], hw[1], H, W)

    @staticmethod
    def _no_grad_on_gpu(named, differentiable=False):
        for name, t in named:  # grad first: it is a property of the call, the device one of the machine
            if t.requires_grad and differentiable and name.startswith("targets"):
                raise ValueError(f"SetCriterion: {name} requires grad; the losses are differentiable with respect to the model's "
                                 f"outputs only")
            if t.requires_grad and not differentiable:
                raise ValueError(f"SetCriterion: {name} requires grad; the criterion is forward only unless its grad attribute "
                                 f"is set, and the result would silently cut the graph")
        for name, t in named:
            if not t.is_cuda:
                raise ValueError(f"SetCriterion: {name} is a CPU tensor; the criterion runs on the GPU")

    def _prepare(self, outputs, targets, differentiable=False):
        outputs = _stack_outputs(outputs)
        if not isinstance(targets, (list, tuple)) or not targets or not all(isinstance(t, dict) for t in targets):
            raise ValueError("SetCriterion: targets must be a non-empty list of dicts")
        layers = [("outputs", outputs)] + [(f"aux_outputs[{i}]", a) for i, a in enumerate(outputs.get("aux_outputs", []))]
        dims, hw, named = None, None, []
        for what, out in layers:
            d, l_hw, keys = self._layer_inputs(out, targets, what)
            if dims is not None and (d, l_hw) != (dims, hw):
                raise ValueError(f"SetCriterion: {what} differs in shape from outputs")
            dims, hw = d, l_hw
            named += [(f"{what}['{k}']", out[k]) for k in keys]
        B, T = dims[0], dims[1]
        self._targets(targets, B, T, hw)
        named += [(f"targets[{b}]['{k}']", t[k]) for b, t in enumerate(targets)
                  for k in ("boxes", "labels", "valid") + (("masks",) if hw is not None else ())]
        self._no_grad_on_gpu(named, differentiable)
        dev = outputs["pred_logits"].device
        tg = {"labels": torch.stack([t["labels"] for t in targets]).to(device=dev, dtype=torch.int64).contiguous(),
              "boxes": torch.stack([t["boxes"] for t in targets]).to(device=dev, dtype=torch.float32).contiguous(),
              "valid": (torch.stack([t["valid"] for t in targets]) != 0).to(device=dev, dtype=torch.int32).contiguous()}
        if hw is not None:
            m = torch.stack([t["masks"] for t in targets])
            tg["masks"] = (m if m.dtype in (torch.bool, torch.uint8) else m != 0).to(device=dev, dtype=torch.uint8).contiguous()
        return [out for _, out in layers], tg, hw

    def _num_boxes(self, targets, dev):
        """criterion.py:231-237 with torch ops on the device: no read-back, no synchronisation"""
        n = torch.stack([t["valid"] for t in targets]).sum().to(device=dev, dtype=torch.float32).reshape(1)
        world = 1
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            torch.distributed.all_reduce(n)
            world = torch.distributed.get_world_size()
        return torch.clamp(n / world, min=1)

    def _layer(self, out, tg, hw, num_boxes):
        """One decoder layer, the two entry points -> dict: sums [B,3,Q] / st [B] float64 (None without masks), cost [B,Q], index [B]
        int32, parts [B,6] float64, losses [6]"""
        sums = st = None
        if hw is not None:
            sums, st = train_ops.criterion_mask_sums(out["pred_masks"].contiguous(), tg["masks"], alpha=self.focal_alpha)
        vis = out["pred_visible"].contiguous() if (self.vis or "visible" in self.losses) else None
        cost, index, parts, losses = train_ops.criterion_match_losses(
            out["pred_logits"].contiguous(), out["pred_boxes"].contiguous(), tg["labels"], tg["boxes"], tg["valid"], num_boxes,
            pred_visible=vis, sums=sums, st=st, hw=hw, cost_class=self.cost_class, cost_bbox=self.cost_bbox, cost_giou=self.cost_giou,
            cost_mask=self.cost_mask if self.masks else 0.0, cost_dice=self.cost_dice if self.masks else 0.0,
            cost_vis=self.cost_vis if self.vis else 0.0, focal_alpha=self.focal_alpha)
        return {"sums": sums, "st": st, "cost": cost, "index": index, "parts": parts, "losses": losses}

    @torch.no_grad()
    def layer_values(self, outputs, targets):
        """Everything the kernels leave, per layer (the last decoder layer first, then the aux layers): what forward() and
        matcher() are made of, for tools and tests"""
        layers, tg, hw = self._prepare(outputs, targets)
        num_boxes = self._num_boxes(targets, layers[0]["pred_logits"].device)
        return [self._layer(out, tg, hw, num_boxes) for out in layers]

    @torch.no_grad()
    def matcher(self, outputs, targets):
        """matcher.py:79-240 on the last layer's outputs: B tuples (src_idx [1], tgt_idx [1]) of int64 device tensors; ties in the cost
        go to the lower query index"""
        layers, tg, hw = self._prepare({k: v for k, v in _stack_outputs(outputs).items() if k != "aux_outputs"}, targets)
        dev = layers[0]["pred_logits"].device
        idx = self._layer(layers[0], tg, hw, torch.ones(1, dtype=torch.float32, device=dev))["index"].to(torch.int64)
        return [(idx[b:b + 1], torch.zeros(1, dtype=torch.int64, device=dev)) for b in range(idx.shape[0])]

    def forward(self, outputs, targets):
        if not self.grad:
            with torch.no_grad():
                return self._forward(outputs, targets, False)
        return self._forward(outputs, targets, True)

    def _forward(self, outputs, targets, differentiable):
        layers, tg, hw = self._prepare(outputs, targets, differentiable)
        num_boxes = self._num_boxes(targets, layers[0]["pred_logits"].device)
        need_vis = self.vis or "visible" in self.losses
        losses = {}
        for i, out in enumerate(layers):
            if differentiable:
                vals = _LayerLosses.apply(self, tg, hw, num_boxes, out["pred_logits"].contiguous(), out["pred_boxes"].contiguous(),
                                          out["pred_masks"].contiguous() if hw is not None else None,
                                          out["pred_visible"].contiguous() if need_vis else None)
            else:
                vals = self._layer(out, tg, hw, num_boxes)["losses"]
            suffix = "" if i == 0 else f"_{i - 1}"
            for name in self.losses:
                for key in _LOSS_KEYS[name]:
                    losses[key + suffix] = vals[_SLOT[key]]
        return losses


def build_criterion(args):
    """tce_rvos.py:686-715 and matcher.py:243-263, with the defaults of opts.py for what a sparse namespace leaves out"""
    def g(name, default):
        return getattr(args, name, default)
    if g("binary", False):
        num_classes = 1
    else:
        num_classes = {"ytvos": 65, "davis": 78, "a2d": 1, "jhmdb": 1}.get(g("dataset_file", "ytvos"), 91)
    masks, vis_loss = bool(g("masks", True)), bool(g("vis_loss", False))
    weight_dict = {"loss_ce": g("cls_loss_coef", 2), "loss_bbox": g("bbox_loss_coef", 5), "loss_giou": g("giou_loss_coef", 2)}
    if vis_loss:
        weight_dict["loss_vis"] = g("vis_loss_coef", 2)
    if masks:
        weight_dict["loss_mask"] = g("mask_loss_coef", 2)
        weight_dict["loss_dice"] = g("dice_loss_coef", 5)
    if g("aux_loss", True):
        aux = {}
        for i in range(g("dec_layers", 4) - 1):
            aux.update({k + f"_{i}": v for k, v in weight_dict.items()})
        weight_dict.update(aux)
    losses = ["labels", "boxes"] + (["masks"] if masks else []) + (["visible"] if vis_loss else [])
    return SetCriterion(num_classes, weight_dict, losses, focal_alpha=g("focal_alpha", 0.25), eos_coef=g("eos_coef", 0.1),
                        cost_class=g("set_cost_class", 2), cost_bbox=g("set_cost_bbox", 5), cost_giou=g("set_cost_giou", 2),
                        cost_mask=g("set_cost_mask", 2), cost_dice=g("set_cost_dice", 5), cost_vis=g("set_cost_vis", 2),
                        masks=masks, vis=vis_loss)
