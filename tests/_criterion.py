"""Shared by the criterion tests, the fixture generator and tools/criterion_bench.py: the case table, the input builders
(torch.Generator(seed)), the reference's formulas as torch operations (`torch_form`, any dtype and device), the fp64 restatement
with the error bound of every output derived from the kernels' op chain (`restate`).

THE BOUNDS (u = 2^-24, the unit round-off of fp32; nothing here was tuned to a GPU run).

Per element of the mask walk and of the focal losses (train/tce_rvos_train.h (a)):
  e = expf(-|v|)            library error taken as 2 ulp                         relative 4u
  1 + e                     one rounding; the error of e arrives scaled e/(1+e) <= 1/2   2u + u
  r = 1/(1+e)               one rounding                                          4u
  e*r                       4u (e) + 4u (r) + u                                   9u      -> s = sigmoid(v):  REL_S = 10u
  log1pf(e)                 2 ulp = 4u, and the error of e arrives with factor e/((1+e) log(1+e)) <= 1     8u
  ce = max(z,0) + log1pf(e) both terms >= 0, one rounding                         9u
  m*m                       2 * 9u + u                                            19u
  ce*(m*m), times alpha_t   9u + 19u + u, then u (1 - alpha in fp32) + u          31u     -> f:               REL_F = 32u
Where e falls below the normal range (|v| > 87) a result may be flushed: an absolute ABS_ELEM = 2^-100 per element covers it.
All terms are >= 0 and are accumulated in fp64 (relative N * 2^-53, covered by REL_ACC = 2^-40), so a sum's error is the sum of
the per-element errors: |dS| <= (REL + REL_ACC) * S + N * ABS_ELEM, no cancellation growth.  S_t is exact.

The matcher's class / visibility term cls(x) (header (b)): p = 1/(1+expf(-x)) has absolute error <= 4u and so has 1 - p
(x >= 0: 1+E in [1,2) rounds within u, the quotient in [0.5,1) within u/2, E's 4u relative arrives as <= u, and 1 - p is exact;
x < 0: p <= 1/2 with relative 6u, 1 - p rounds within u/2): DELTA = 4u.  The logs take a + 1e-8 whose argument a may be as small as
1e-8, so their error is NOT a multiple of u: |d log| <= log((a + D)/max(a - D, 1e-8(1-u))) + 4u|log|, D = DELTA + u*a.  The squares:
2*q*DELTA + DELTA^2 + u*q^2.  Products and the final difference add u per operation on the magnitudes.  A mean over n frames adds
(n + 1)u on the summed magnitudes.
L1: exact inputs, |a-b| one rounding, three additions: 4u * L1 per box.
gIoU (box_ops.py:44-81), S = max(1, max |coordinate|): a corner within u*S, a width within 3u*S, an area (and the intersection and
the enclosing area) within EA = 7u*S^2, the union within EU = 27u*S^2; a quotient (n + 1e-6)/(d + 1e-6) within
(En + u)/(D) + q*(Ed + u)/D + u*q with D = d + 1e-6 - Ed > 0 (a degenerate box has no bound; the generator asserts there is none).
The cost column is an fp32 accumulator over at most five terms: the weighted term bounds plus 8u on the summed magnitudes.
The losses: sums of >= 0 fp32 terms in fp64 (relative bounds above), the quotient by num_boxes in fp64, one rounding to fp32.
"""
import math

import torch

U = 2.0 ** -24
REL_S, REL_F, REL_ACC, ABS_ELEM = 10 * U, 32 * U, 2.0 ** -40, 2.0 ** -100
DELTA = 4 * U

CONSTS = dict(cost_class=2.0, cost_bbox=5.0, cost_giou=2.0, cost_mask=2.0, cost_dice=5.0, cost_vis=2.0, focal_alpha=0.25)
LOSS_ORDER = ("loss_ce", "loss_bbox", "loss_giou", "loss_mask", "loss_dice", "loss_vis")

# name, seed, B, T, Q, K, (H, W), valid rows [B][T], vis, aux layers
CASES = [
    ("c1", 101, 1, 1, 1, 1, (32, 32), [[1]], False, 0),                       # smallest everything
    ("c2", 102, 1, 3, 5, 1, (90, 150), [[1, 1, 1]], False, 0),                # bottom rows / right columns are padding samples
    ("c3", 103, 1, 2, 7, 1, (36, 44), [[1, 0]], False, 0),                    # w = 16 over a 44-pixel row, odd Q, one invalid frame
    ("c4", 104, 1, 2, 5, 65, (64, 96), [[1, 1]], False, 0),                   # multi-class path
    ("c5", 105, 1, 3, 5, 1, (90, 150), [[0, 0, 0]], False, 0),                # all frames invalid: mask-only cost, num_boxes clamped
    ("c6", 106, 3, 3, 5, 1, (90, 150), [[1, 1, 1], [1, 0, 1], [0, 1, 0]], False, 0),  # batch normalisation
    ("c7", 107, 1, 3, 5, 1, (90, 150), [[1, 0, 1]], True, 0),                 # visibility cost and loss
    ("c8", 108, 1, 3, 5, 1, (90, 150), [[1, 1, 0]], False, 2),                # suffixed aux losses
    ("c9", 109, 1, 5, 5, 1, (360, 640), [[1, 1, 1, 0, 1]], False, 0),         # config 2's padded size, h x w = 96 x 160
    # c10: the unaligned-base path.  The shape precondition 4w == ceil32(W) makes w a multiple of 8, so w % 4 != 0 cannot reach the
    # kernel; the scalar walk is reached through a base that is 4- but not 16-byte aligned (the GPU test builds that view)
    ("c10", 110, 1, 2, 3, 1, (30, 30), [[1, 1]], False, 0),
]
UNALIGNED = {"c10"}


def ceil32(n):
    return (n + 31) // 32 * 32


def _layer_inputs(g, B, T, Q, K, h, w, vis):
    out = {"pred_logits": torch.randn(B, T, Q, K, generator=g) * 1.5,
           "pred_boxes": torch.cat([0.3 + 0.4 * torch.rand(B, T, Q, 2, generator=g), 0.1 + 0.4 * torch.rand(B, T, Q, 2, generator=g)], -1),
           "pred_masks": torch.randn(B, T, Q, h, w, generator=g) * 3.0}
    if vis:
        out["pred_visible"] = torch.randn(B, T, Q, 1, generator=g) * 1.5
    return out


def make_case(case):
    """-> (outputs dict of float32 CPU tensors [B,T,Q,..] with aux_outputs if any, targets: B dicts)"""
    name, seed, B, T, Q, K, (H, W), valid, vis, n_aux = case
    g = torch.Generator().manual_seed(seed)
    h, w = ceil32(H) // 4, ceil32(W) // 4
    outputs = _layer_inputs(g, B, T, Q, K, h, w, vis)
    if n_aux:
        outputs["aux_outputs"] = [_layer_inputs(g, B, T, Q, K, h, w, vis) for _ in range(n_aux)]
    targets = []
    for b in range(B):
        v = torch.tensor(valid[b], dtype=torch.int64)
        boxes = torch.cat([0.3 + 0.4 * torch.rand(T, 2, generator=g), 0.15 + 0.35 * torch.rand(T, 2, generator=g)], -1)
        boxes = boxes * v[:, None].float()  # the datasets zero the box of a frame without the object
        ys, xs = torch.arange(H)[None, :, None] / H, torch.arange(W)[None, None, :] / W
        inside = ((ys - boxes[:, 1, None, None]).abs() < boxes[:, 3, None, None] / 2) & \
                 ((xs - boxes[:, 0, None, None]).abs() < boxes[:, 2, None, None] / 2)
        speck = torch.rand(T, H, W, generator=g) < 0.02
        masks = ((inside ^ speck) & (v[:, None, None] > 0)).to(torch.uint8)
        labels = torch.randint(0, K, (T,), generator=g) if K > 1 else torch.zeros(T, dtype=torch.int64)
        targets.append({"masks": masks, "boxes": boxes, "labels": labels, "valid": v})
    return outputs, targets


def sample_targets(masks, dtype):
    """[B,T,H,W] 0/1 -> [B,T,h,w]: zero-padded to a multiple of 32, then [2::4, 2::4] (matcher.py:110-122)"""
    B, T, H, W = masks.shape
    pad = torch.zeros(B, T, ceil32(H), ceil32(W), dtype=dtype, device=masks.device)
    pad[:, :, :H, :W] = masks.to(dtype)
    return pad[:, :, 2::4, 2::4]


# ---- the reference's formulas as torch operations, in the dtype and on the device of the inputs ------------------------------
def _xyxy(b):
    cx, cy, w, h = b.unbind(-1)
    return torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)


def _giou(a, b):
    """box_ops.generalized_box_iou, pairwise [N,4] x [M,4] -> [N,M]"""
    area1, area2 = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]), (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    wh = (torch.min(a[:, None, 2:], b[:, 2:]) - torch.max(a[:, None, :2], b[:, :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    union = area1[:, None] + area2 - inter
    iou = (inter + 1e-6) / (union + 1e-6)
    wh = (torch.max(a[:, None, 2:], b[:, 2:]) - torch.min(a[:, None, :2], b[:, :2])).clamp(min=0)
    area = wh[..., 0] * wh[..., 1]
    return iou - ((area - union) + 1e-6) / (area + 1e-6)


def _focal(x, t, alpha):
    prob = x.sigmoid()
    ce = torch.nn.functional.binary_cross_entropy_with_logits(x, t, reduction="none")
    p_t = prob * t + (1 - prob) * (1 - t)
    return (alpha * t + (1 - alpha) * (1 - t)) * (ce * (1 - p_t) ** 2)


def _cls(p):
    neg = 0.75 * p ** 2 * (-(1 - p + 1e-8).log())
    pos = 0.25 * (1 - p) ** 2 * (-(p + 1e-8).log())
    return pos - neg


def torch_layer(out, tg, num_boxes, c, masks=True, vis=False):
    """One decoder layer: the matcher's cost columns and the losses, as the loop a caller writes today.  tg: stacked targets with
    `tmask` already sampled [B,T,h,w].  -> (cost [B,Q], index [B], losses dict)"""
    lg, bx = out["pred_logits"], out["pred_boxes"]
    B, T, Q, K = lg.shape
    costs, idxs = [], []
    for b in range(B):
        C = torch.zeros(Q, dtype=lg.dtype, device=lg.device)
        vt = [t for t in range(T) if tg["valid"][b, t] != 0]
        if vt:
            p = lg[b].sigmoid()
            C = C + c["cost_class"] * torch.stack([_cls(p[t])[:, 0 if K == 1 else tg["labels"][b, t]] for t in vt]).mean(0)
            C = C + c["cost_bbox"] * torch.stack([torch.cdist(bx[b, t], tg["boxes"][b, t][None], p=1)[:, 0] for t in vt]).mean(0)
            C = C + c["cost_giou"] * torch.stack([-_giou(_xyxy(bx[b, t]), _xyxy(tg["boxes"][b, t][None]))[:, 0] for t in vt]).mean(0)
        if vis:
            C = C + c["cost_vis"] * _cls(out["pred_visible"][b].sigmoid())[..., 0].mean(0)
        if masks:
            x = out["pred_masks"][b].transpose(0, 1).flatten(1)     # [Q, T*h*w]
            t = tg["tmask"][b].flatten()[None].expand_as(x)
            s = x.sigmoid()
            dice = (2 * (s * t).sum(1) + 1) / (s.sum(1) + t.sum(1) + 1)
            C = C + (c["cost_mask"] * _focal(x, t, 0.25).mean(1) + c["cost_dice"] * -dice)
        costs.append(C)
        idxs.append(torch.min(C, 0)[1])
    idx = torch.stack(idxs)
    losses = {}
    onehot = torch.zeros_like(lg)
    for b in range(B):
        for t in range(T):
            if tg["valid"][b, t] != 0:
                onehot[b, t, idx[b], 0 if K == 1 else tg["labels"][b, t]] = 1
    losses["loss_ce"] = _focal(lg, onehot, c["focal_alpha"]).sum() / num_boxes
    src = torch.stack([bx[b, :, idx[b]] for b in range(B)]).flatten(0, 1)  # [B*T, 4]
    tb = tg["boxes"].flatten(0, 1)
    losses["loss_bbox"] = (src - tb).abs().sum() / num_boxes
    losses["loss_giou"] = (1 - torch.diag(_giou(_xyxy(src), _xyxy(tb)))).sum() / num_boxes
    if masks:
        x = torch.stack([out["pred_masks"][b, :, idx[b]] for b in range(B)]).flatten(1)
        t = tg["tmask"].flatten(1)
        s = x.sigmoid()
        losses["loss_mask"] = _focal(x, t, 0.25).mean(1).sum() / num_boxes  # criterion.py:189 leaves alpha at its default
        losses["loss_dice"] = (1 - (2 * (s * t).sum(1) + 1) / (s.sum(1) + t.sum(1) + 1)).sum() / num_boxes
    if vis:
        x = out["pred_visible"][0, :, idx[0], 0]
        f = _focal(x, (tg["valid"][0] != 0).to(x.dtype), c["focal_alpha"])
        losses["loss_vis"] = f.mean() / T * (T * Q)
    return torch.stack(costs), idx, losses


def torch_form(outputs, targets, c=CONSTS, masks=True, vis=False):
    """The whole criterion as torch operations (criterion.py:216-262), its .item() included -> (loss dict, [(cost, index)] per layer)"""
    lg = outputs["pred_logits"]
    tg = {"labels": torch.stack([t["labels"] for t in targets]), "boxes": torch.stack([t["boxes"] for t in targets]).to(lg.dtype),
          "valid": torch.stack([t["valid"] for t in targets])}
    if masks:
        tg["tmask"] = sample_targets(torch.stack([t["masks"] for t in targets]), lg.dtype)
    num_boxes = max(float(tg["valid"].sum().item()), 1.0)
    losses, match = {}, []
    for i, out in enumerate([outputs] + list(outputs.get("aux_outputs", []))):
        cost, idx, l = torch_layer(out, tg, num_boxes, c, masks, vis)
        match.append((cost, idx))
        losses.update({k + ("" if i == 0 else f"_{i - 1}"): v for k, v in l.items()})
    return losses, match


# ---- the fp64 restatement with bounds -----------------------------------------------------------------------------------------
def _sum_bound(S, n, rel):
    return (rel + REL_ACC) * S + n * ABS_ELEM


def _cls_bound(x):
    """cls(x) in fp64 -> (value, bound, magnitude), elementwise"""
    p = torch.sigmoid(x)
    q = torch.sigmoid(-x)
    val, bound, mag = 0, 0, 0
    for coef, sq, a, sign in ((0.25, q, p, 1.0), (0.75, p, q, -1.0)):
        arg = a + 1e-8
        L = -torch.log(arg)
        D = DELTA + U * arg
        EL = torch.log((arg + D) / torch.clamp(arg - D, min=1e-8 * (1 - U))) + 4 * U * L.abs()
        Esq = 2 * sq * DELTA + DELTA ** 2 + U * sq ** 2
        term = coef * sq ** 2 * L
        bound = bound + coef * (Esq * (L.abs() + EL) + sq ** 2 * EL) + 3 * U * term.abs()
        val = val + sign * term
        mag = mag + term.abs()
    return val, bound + U * mag, mag


def _giou_bound(a, b):
    """giou of cxcywh pairs [..,4] in fp64 -> (value, bound)"""
    S = max(1.0, float(_xyxy(a).abs().max()), float(_xyxy(b).abs().max()))
    EA, EU = 7 * U * S * S, 27 * U * S * S
    a, b = _xyxy(a), _xyxy(b)
    area1, area2 = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1]), (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    wh = (torch.min(a[..., 2:], b[..., 2:]) - torch.max(a[..., :2], b[..., :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    union = area1 + area2 - inter
    iou = (inter + 1e-6) / (union + 1e-6)
    wh = (torch.max(a[..., 2:], b[..., 2:]) - torch.min(a[..., :2], b[..., :2])).clamp(min=0)
    area = wh[..., 0] * wh[..., 1]
    r2 = ((area - union) + 1e-6) / (area + 1e-6)
    Du, Da = union + 1e-6 - EU, area + 1e-6 - EA
    assert bool((Du > 0).all()) and bool((Da > 0).all()), "a degenerate box: the gIoU has no bound"
    e = (EA + U) / Du + iou * (EU + U) / Du + U * iou + (EA + EU + 2 * U) / Da + r2.abs() * (EA + U) / Da + U * r2.abs()
    v = iou - r2
    return v, e + U * v.abs(), float(torch.min(Du.min(), Da.min()))


def _focal64(x, t, alpha):
    """The header's per-element f and s in fp64 (alpha and 1 - alpha as the fp32 values the kernel holds)"""
    a32 = torch.tensor(alpha, dtype=torch.float32)
    al, oma = float(a32), float(torch.tensor(1.0, dtype=torch.float32) - a32)
    z = torch.where(t > 0, -x, x)
    ce = z.clamp(min=0) + torch.log1p(torch.exp(-x.abs()))
    return torch.where(t > 0, al, oma) * (ce * torch.sigmoid(z) ** 2), torch.sigmoid(x)


def restate_layer(out, tg, num_boxes, c, masks=True, vis=False):
    """fp64 values and bounds of one layer.  out: float32 (or float64) CPU tensors; tg: stacked targets, `tmask` [B,T,h,w].
    -> dict: sums [B,3,Q], st [B], cost [B,Q], index [B], parts [B,6], losses [6], and e_<name> bounds of the same shapes"""
    lg, bx = out["pred_logits"].double(), out["pred_boxes"].double()
    B, T, Q, K = lg.shape
    tb = tg["boxes"].double()
    valid = tg["valid"] != 0
    r = {}
    if masks:
        x = out["pred_masks"].double().transpose(1, 2).flatten(2)   # [B,Q,N]
        N = x.shape[2]
        t = tg["tmask"].double().flatten(1)[:, None].expand_as(x)
        f, s = _focal64(x, t, c.get("mask_alpha", c["focal_alpha"]))
        r["sums"] = torch.stack([f.sum(2), s.sum(2), (s * t).sum(2)], 1)
        r["st"] = tg["tmask"].double().flatten(1).sum(1)
        r["e_sums"] = torch.stack([_sum_bound(r["sums"][:, 0], N, REL_F), _sum_bound(r["sums"][:, 1], N, REL_S),
                                   _sum_bound(r["sums"][:, 2], N, REL_S)], 1)
        den = r["sums"][:, 1] + r["st"][:, None] + 1
        dice = (2 * r["sums"][:, 2] + 1) / den
        e_dice = (2 * r["e_sums"][:, 2] + dice * r["e_sums"][:, 1]) / (den - r["e_sums"][:, 1]) + 2.0 ** -50
        fm = r["sums"][:, 0] / N
        e_fm = r["e_sums"][:, 0] / N
    cost, e_cost = torch.zeros(B, Q, dtype=torch.float64), torch.zeros(B, Q, dtype=torch.float64)
    mag = torch.zeros(B, Q, dtype=torch.float64)
    min_den = math.inf
    for b in range(B):
        vt = [t for t in range(T) if valid[b, t]]
        n = len(vt)
        if n:
            col = [0 if K == 1 else int(tg["labels"][b, t]) for t in vt]
            v, e, m = _cls_bound(torch.stack([lg[b, t, :, k] for t, k in zip(vt, col)]))
            cost[b] += c["cost_class"] * v.mean(0)
            e_cost[b] += c["cost_class"] * (e.mean(0) + (n + 1) * U * m.mean(0))
            mag[b] += c["cost_class"] * m.mean(0)
            l1 = (bx[b, vt] - tb[b, vt][:, None]).abs().sum(-1).mean(0)
            cost[b] += c["cost_bbox"] * l1
            e_cost[b] += c["cost_bbox"] * (n + 6) * U * l1
            mag[b] += c["cost_bbox"] * l1
            gv, ge, d = _giou_bound(bx[b, vt], tb[b, vt][:, None].expand(-1, Q, -1))
            min_den = min(min_den, d)
            cost[b] += c["cost_giou"] * (-gv).mean(0)
            e_cost[b] += c["cost_giou"] * (ge.mean(0) + (n + 1) * U * gv.abs().mean(0))
            mag[b] += c["cost_giou"] * gv.abs().mean(0)
        if vis:
            v, e, m = _cls_bound(out["pred_visible"].double()[b, :, :, 0])
            cost[b] += c["cost_vis"] * v.mean(0)
            e_cost[b] += c["cost_vis"] * (e.mean(0) + (T + 1) * U * m.mean(0))
            mag[b] += c["cost_vis"] * m.mean(0)
        if masks:
            cost[b] += c["cost_mask"] * fm[b] - c["cost_dice"] * dice[b]
            e_cost[b] += c["cost_mask"] * (e_fm[b] + 2 * U * fm[b]) + c["cost_dice"] * (e_dice[b] + 2 * U * dice[b])
            mag[b] += c["cost_mask"] * fm[b] + c["cost_dice"] * dice[b]
    e_cost += 8 * U * mag
    r["cost"], r["e_cost"] = cost, e_cost
    r["index"] = torch.stack([torch.min(cost[b], 0)[1] for b in range(B)])
    parts, e_parts = torch.zeros(B, 6, dtype=torch.float64), torch.zeros(B, 6, dtype=torch.float64)
    for b in range(B):
        i = int(r["index"][b])
        onehot = torch.zeros(T, Q, K, dtype=torch.float64)
        for t in range(T):
            if valid[b, t]:
                onehot[t, i, 0 if K == 1 else int(tg["labels"][b, t])] = 1
        parts[b, 0] = _focal64(lg[b], onehot, c["focal_alpha"])[0].sum()
        e_parts[b, 0] = _sum_bound(parts[b, 0], T * Q * K, REL_F)
        parts[b, 1] = (bx[b, :, i] - tb[b]).abs().sum()
        e_parts[b, 1] = 4 * U * parts[b, 1]
        gv, ge, d = _giou_bound(bx[b, :, i], tb[b])
        min_den = min(min_den, d)
        parts[b, 2] = (1 - gv).sum()
        e_parts[b, 2] = (ge + U * (1 - gv).abs()).sum()
        if masks:
            parts[b, 3], e_parts[b, 3] = fm[b, i], e_fm[b, i]
            parts[b, 4], e_parts[b, 4] = 1 - dice[b, i], e_dice[b, i]
        if vis:
            s = _focal64(out["pred_visible"].double()[b, :, i, 0], valid[b].double(), c["focal_alpha"])[0].sum()
            parts[b, 5] = s / T / T * (T * Q)
            e_parts[b, 5] = _sum_bound(s, T, REL_F) / T / T * (T * Q)
    r["parts"], r["e_parts"] = parts, e_parts
    div = torch.tensor([num_boxes] * 5 + [1.0], dtype=torch.float64)
    r["losses"] = parts.sum(0) / div
    r["e_losses"] = e_parts.sum(0) / div + 2 * U * r["losses"].abs()
    r["min_den"] = min_den
    return r


def stack_targets(targets, masks=True):
    tg = {"labels": torch.stack([t["labels"] for t in targets]), "boxes": torch.stack([t["boxes"] for t in targets]),
          "valid": torch.stack([t["valid"] for t in targets])}
    if masks:
        tg["tmask"] = sample_targets(torch.stack([t["masks"] for t in targets]), torch.float64)
    return tg


def restate(outputs, targets, c=CONSTS, masks=True, vis=False):
    """-> [restate_layer(..) of the last layer and of every aux layer], num_boxes"""
    tg = stack_targets(targets, masks)
    num_boxes = max(float(tg["valid"].sum()), 1.0)
    layers = [outputs] + list(outputs.get("aux_outputs", []))
    return [restate_layer(o, tg, num_boxes, c, masks, vis) for o in layers], num_boxes


def loss_names(masks=True, vis=False):
    return ["loss_ce", "loss_bbox", "loss_giou"] + (["loss_mask", "loss_dice"] if masks else []) + (["loss_vis"] if vis else [])


def ref_sum_bound(n):
    """What an fp32 sum of n terms of one sign may lose against the exact sum, relative, in ANY order: (n - 1) u.  The reference sums
    in fp32; the CPU test allows it this much on top of the derived bound where the fixture's recorded margin is not at hand."""
    return max(n - 1, 1) * U
