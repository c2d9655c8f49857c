"""Shared by the criterion-gradient tests, the fixture generator and tools/criterion_grad_bench.py: the fp64 closed form of the two
backward entry points of train/tce_rvos_train.h, (c) and (d), with a per-element error bound derived from the kernels' op chain
(`grad_layer`), on the cases and with the constants of tests/_criterion.py (R).

THE BOUNDS (u = R.U = 2^-24; nothing here was tuned to a GPU run).  From R's docstring: s, m and their complements sc, mc (each is r
or e*r) are within REL_S = 10u, ce within REL_CE = 9u, and an element whose e leaves the normal range gets ABS_ELEM absolute.

d f / d v = alpha_t * ((m*m) * (m + 2*(ce*mc))):
  m*m                          2 REL_S + u                                   21u
  ce*mc                        REL_CE + REL_S + u                            20u     (times 2: exact)
  m + 2*(ce*mc)                both terms >= 0: the larger relative + u      21u
  (m*m) * (..)                 21u + 21u + u                                 43u
  times alpha_t                u (1 - alpha formed in fp32) + u              45u     -> REL_DF = 45u;  f itself is R.REL_F = 32u
s*sc                           2 REL_S + u                                   21u     -> REL_DS = 21u
(c) grad = Gm*dfs + Gd*(s*sc).  Gm = gl[3]/n/N is an fp64 quotient rounded once: u.  Gd comes from the kernel's OWN sums, which differ
from the exact ones by at most R's e_sums (E_p for S_p, E_pt for S_pt): with A = 2 S_pt + 1 and D = S_p + S_t + 1,
  |d (A/D^2)| <= (2 E_pt + (A/D^2) (2 D E_p + E_p^2)) / (D - E_p)^2,   |d (2/D)| <= 2 E_p / (D (D - E_p)),
fp64 roundings REL_ACC on the magnitudes A/D^2 + 2/D (they may cancel in Gd1; the bound is on the magnitudes), times |gl[4]|/n, then u
for the rounding to fp32: E_Gd.  The two products add u each, the final sum u on the two MAGNITUDES (the focal and the dice term may
cancel; the bound is not on their sum):
  |d grad| <= |Gm dfs| (REL_DF + 2u) + (|Gd| (REL_DS + 2u) + E_Gd) s sc + u (|Gm dfs| + |Gd| s sc) + ABS_ELEM (|Gm| + |Gd| + E_Gd)
(d) g_logits, g_visible = c * dfs with c an fp64 quotient rounded once:  |c dfs| (REL_DF + 2u) + ABS_ELEM |c|.
g_boxes = c1 * sign(p - g) + c2 * dg.  sign is exact (the sign of an fp32 difference is the sign of the exact one).  dg is the reverse
chain of the header, bounded by running the chain itself in (value, bound) arithmetic (`_V`): every fp32 operation adds u on its
result, a product |a| Eb + |b| Ea + Ea Eb, a quotient (Ea + |q| Eb)/(|b| - Eb).  The forward quantities enter with the bounds of R's
docstring, S = max(1, max |coordinate|): a corner u S, a width 3u S, an area, the intersection and the enclosing area EA = 7u S^2, the
union EU = 27u S^2; the quotients' denominators are R._giou_bound's (union + 1e-6 - EU and area + 1e-6 - EA, asserted > 0).  The
selections (which argument a min / max took, whether a clamp was active) are taken from the fp64 values: the fixture generator asserts
every such comparison is decided by more than 1e-4, four orders above any rounding here.  Then u for c1, 2u on |c2 dg|, u on the
magnitudes of the final sum.
All bounds are first order with their second-order terms covered by the factor (1 + 2^-16).

THE REFERENCE'S ALLOWANCE (`a_*`, used by the generator's self-check only; the GPU test uses the recorded margin).  The reference
(torch autograd of models/criterion.py in fp32) (i) sums S_p, S_pt, S_t in fp32: relative R.ref_sum_bound(N) on A and D, reaching the
dice term as ref_sum_bound(N) * |gl[4]|/n * (3 A/D^2 + 2/D) * s sc; (ii) forms 1 - p_t, 1 - sigmoid and sigmoid - t by subtraction:
an absolute 4u in m or s, reaching the gradient through |d df/d m| <= alpha_t (3 m^2 + 4 ce m) and d (s sc) <= s; (iii) runs the
gIoU chain in reverse in another association of the same operations: once more the chain's own bound.
"""
import torch

import _criterion as R

U = R.U
REL_CE = 9 * U
REL_DF = 2 * (2 * R.REL_S + U) + U + 2 * U  # 45u, the table above
REL_DS = 2 * R.REL_S + U
SLACK = 1 + 2.0 ** -16
WEIGHTS = dict(loss_ce=2.0, loss_bbox=5.0, loss_giou=2.0, loss_mask=2.0, loss_dice=5.0, loss_vis=2.0)  # the reference's weight_dict
KINK = 1e-4
assert abs(REL_DF - 45 * U) < 1e-20


def gl_of(weights=WEIGHTS, vis=False):
    """The upstream gradient of losses[6] that sum(w_k * loss_k).backward() produces"""
    g = [float(weights[k]) for k in R.LOSS_ORDER]
    if not vis:
        g[5] = 0.0
    return g


class _V:
    """(value, absolute bound) of an fp32 computation, fp64 tensors"""

    def __init__(self, v, e=None):
        self.v = v
        self.e = torch.zeros_like(v) if e is None else e + torch.zeros_like(v)

    @staticmethod
    def _rounded(v, e):
        return _V(v, e + U * (v.abs() + e))

    def __add__(self, o):
        return _V._rounded(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        return _V._rounded(self.v - o.v, self.e + o.e)

    def __neg__(self):
        return _V(-self.v, self.e)

    def __mul__(self, o):
        return _V._rounded(self.v * o.v, self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e)

    def __truediv__(self, o):
        den = o.v.abs() - o.e
        assert bool((den > 0).all()), "a quotient without a bound"
        q = self.v / o.v
        return _V._rounded(q, (self.e + q.abs() * o.e) / den)

    def half(self):
        return _V(0.5 * self.v, 0.5 * self.e)

    def where(self, cond):
        return _V(torch.where(cond, self.v, torch.zeros_like(self.v)), torch.where(cond, self.e, torch.zeros_like(self.e)))


def giou_loss_grad(p, g):
    """d(1 - giou)/dp of cxcywh pairs [..,4] (fp64) by the header's reverse chain -> (value [..,4], bound [..,4], the smallest
    distance from a kink: min/max arguments, non-clamped extents)"""
    S = max(1.0, float(R._xyxy(p).abs().max()), float(R._xyxy(g).abs().max()))
    EW, EA, EU = 3 * U * S, 7 * U * S * S, 27 * U * S * S
    a, b = R._xyxy(p), R._xyxy(g)
    x0, y0, x1, y1 = a.unbind(-1)
    gx0, gy0, gx1, gy1 = b.unbind(-1)
    wp, hp = x1 - x0, y1 - y0
    ax, ay = torch.min(x1, gx1) - torch.max(x0, gx0), torch.min(y1, gy1) - torch.max(y0, gy0)
    iw, ih = ax.clamp(min=0), ay.clamp(min=0)
    inter = iw * ih
    uni = wp * hp + (gx1 - gx0) * (gy1 - gy0) - inter
    cx, cy = torch.max(x1, gx1) - torch.min(x0, gx0), torch.max(y1, gy1) - torch.min(y0, gy0)
    ew, eh = cx.clamp(min=0), cy.clamp(min=0)
    area = ew * eh
    assert bool((uni + 1e-6 - EU > 0).all()) and bool((area + 1e-6 - EA > 0).all()), "a degenerate box: the gIoU has no bound"
    kink = torch.stack([(x1 - gx1).abs(), (x0 - gx0).abs(), (y1 - gy1).abs(), (y0 - gy0).abs(),
                        torch.where(ax > 0, ax, ax.abs() + 1), torch.where(ay > 0, ay, ay.abs() + 1),
                        torch.where(cx > 0, cx, cx.abs() + 1), torch.where(cy > 0, cy, cy.abs() + 1)])
    eps, one = _V(torch.full_like(uni, 1e-6), 1e-6 * U), _V(torch.ones_like(uni))
    Vwp, Vhp, Viw, Vih, Vew, Veh = (_V(t, EW) for t in (wp, hp, iw, ih, ew, eh))
    Vinter, Vuni, Varea = _V(inter, EA), _V(uni, EU), _V(area, EA)
    du, da = Vuni + eps, Varea + eps
    iou = (Vinter + eps) / du
    r2 = ((Varea - Vuni) + eps) / da
    d_area = (one - r2) / da
    d_uni = iou / du - one / da
    d_inter = (-(one / du)) - d_uni
    d_iw, d_ih, d_ew, d_eh = d_inter * Vih, d_inter * Viw, d_area * Veh, d_area * Vew
    d_wp, d_hp = d_uni * Vhp, d_uni * Vwp
    out = []
    for (lo, hi, glo, ghi, act_i, act_e, d_i, d_e, d_w) in ((x0, x1, gx0, gx1, ax > 0, cx > 0, d_iw, d_ew, d_wp),
                                                           (y0, y1, gy0, gy1, ay > 0, cy > 0, d_ih, d_eh, d_hp)):
        d_hi = d_w + d_i.where(act_i & (hi <= ghi))
        d_hi = d_hi + d_e.where(act_e & (hi >= ghi))
        d_lo = (-d_w) - d_i.where(act_i & (lo >= glo))
        d_lo = d_lo - d_e.where(act_e & (lo <= glo))
        out.append((d_lo + d_hi, (d_hi - d_lo).half()))
    vals = [out[0][0], out[1][0], out[0][1], out[1][1]]
    return torch.stack([t.v for t in vals], -1), torch.stack([t.e for t in vals], -1), float(kink.min())


def focal_grad64(x, t, alpha):
    """The header's dfs and s*sc in fp64, with the pieces the bounds need -> (dfs, |df|, s*sc, alpha_t*(3m^2 + 4 ce m), s)"""
    a32 = torch.tensor(alpha, dtype=torch.float32)
    al, oma = float(a32), float(torch.tensor(1.0, dtype=torch.float32) - a32)
    z = torch.where(t > 0, -x, x)
    m, mc = torch.sigmoid(z), torch.sigmoid(-z)
    ce = z.clamp(min=0) + torch.log1p(torch.exp(-x.abs()))
    at = torch.where(t > 0, al, oma)
    df = at * ((m * m) * (m + 2 * (ce * mc)))
    s = torch.sigmoid(x)
    return torch.where(t > 0, -df, df), df, s * torch.sigmoid(-x), at * (3 * m * m + 4 * ce * m), s


def grad_layer(out, tg, r, num_boxes, gl, c=R.CONSTS, masks=True, vis=False):
    """fp64 gradients, bounds (e_*) and the reference's allowance (a_*) of one layer.  out: CPU tensors; tg: R.stack_targets(..);
    r: R.restate_layer(..) of the same inputs (index, sums, e_sums, st); gl: six floats.  -> dict: g_logits [B,T,Q,K], g_boxes
    [B,T,Q,4], g_masks [B,T,h,w] (the matched query's planes; all others are 0), g_visible [B,T,Q,1], min_kink"""
    lg, bx = out["pred_logits"].double(), out["pred_boxes"].double()
    B, T, Q, K = lg.shape
    n = float(num_boxes)
    valid = tg["valid"] != 0
    tb = tg["boxes"].double()
    res = {}
    onehot = torch.zeros(B, T, Q, K, dtype=torch.float64)
    for b in range(B):
        for t in range(T):
            if valid[b, t]:
                onehot[b, t, int(r["index"][b]), 0 if K == 1 else int(tg["labels"][b, t])] = 1
    c0 = gl[0] / n
    dfs, df, _, slope, _ = focal_grad64(lg, onehot, c["focal_alpha"])
    res["g_logits"] = c0 * dfs
    res["e_logits"] = (abs(c0) * df * (REL_DF + 2 * U) + R.ABS_ELEM * abs(c0)) * SLACK
    res["a_logits"] = 4 * U * abs(c0) * slope
    g_boxes, e_boxes = torch.zeros(B, T, Q, 4, dtype=torch.float64), torch.zeros(B, T, Q, 4, dtype=torch.float64)
    c1, c2 = gl[1] / n, gl[2] / n
    kink = float("inf")
    for b in range(B):
        i = int(r["index"][b])
        dg, e_dg, k = giou_loss_grad(bx[b, :, i], tb[b])
        diff = bx[b, :, i] - tb[b]
        kink = min(kink, k, float(diff.abs().min()))
        l1 = c1 * torch.sign(diff)
        g_boxes[b, :, i] = l1 + c2 * dg
        e_boxes[b, :, i] = (U * l1.abs() + abs(c2) * e_dg + 2 * U * (c2 * dg).abs() + U * (l1.abs() + (c2 * dg).abs())) * SLACK
    res["g_boxes"], res["e_boxes"], res["a_boxes"], res["min_kink"] = g_boxes, e_boxes, e_boxes.clone(), kink
    if vis:
        x = out["pred_visible"].double()
        c5 = gl[5] * Q / T
        sel = torch.zeros(B, T, Q, 1, dtype=torch.float64)
        for b in range(B):
            sel[b, :, int(r["index"][b])] = 1
        dfs, df, _, slope, _ = focal_grad64(x, valid.double()[:, :, None, None].expand_as(x), c["focal_alpha"])
        res["g_visible"] = c5 * dfs * sel
        res["e_visible"] = (abs(c5) * df * (REL_DF + 2 * U) + R.ABS_ELEM * abs(c5)) * SLACK * sel
        res["a_visible"] = 4 * U * abs(c5) * slope * sel
    if masks:
        pm = out["pred_masks"].double()
        N = T * pm.shape[3] * pm.shape[4]
        g, e, a = [], [], []
        for b in range(B):
            i = int(r["index"][b])
            x, t = pm[b, :, i], tg["tmask"][b].double()
            dfs, df, ds, slope, s = focal_grad64(x, t, c.get("mask_alpha", c["focal_alpha"]))
            Sp, Spt, St = float(r["sums"][b, 1, i]), float(r["sums"][b, 2, i]), float(r["st"][b])
            Ep, Ept = float(r["e_sums"][b, 1, i]), float(r["e_sums"][b, 2, i])
            A, D = 2 * Spt + 1, Sp + St + 1
            num, gd, Gm = A / D ** 2, gl[4] / n, gl[3] / n / N
            Gd = gd * (num - t * (2 / D))
            e_num = (2 * Ept + num * (2 * D * Ep + Ep * Ep)) / (D - Ep) ** 2
            e_inv = 2 * Ep / (D * (D - Ep))
            E_Gd = abs(gd) * (e_num + t * e_inv + R.REL_ACC * (num + 2 / D)) + U * Gd.abs()
            t1, t2 = abs(Gm) * df, Gd.abs() * ds
            g.append(Gm * dfs + Gd * ds)
            e.append((t1 * (REL_DF + 2 * U) + (Gd.abs() * (REL_DS + 2 * U) + E_Gd) * ds + U * (t1 + t2)
                      + R.ABS_ELEM * (abs(Gm) + Gd.abs() + E_Gd)) * SLACK)
            a.append(R.ref_sum_bound(N) * abs(gd) * (3 * num + 2 / D) * ds + 4 * U * (abs(Gm) * slope + Gd.abs() * s))
        res["g_masks"], res["e_masks"], res["a_masks"] = torch.stack(g), torch.stack(e), torch.stack(a)
    return res


def grads(outputs, targets, gl=None, c=R.CONSTS, masks=True, vis=False):
    """-> ([grad_layer(..) per layer, the last decoder layer first], [restate_layer(..) per layer], num_boxes)"""
    gl = gl_of(vis=vis) if gl is None else gl
    tg = R.stack_targets(targets, masks)
    layers, num_boxes = R.restate(outputs, targets, c, masks, vis)
    outs = [outputs] + list(outputs.get("aux_outputs", []))
    return [grad_layer(o, tg, r, num_boxes, gl, c, masks, vis) for o, r in zip(outs, layers)], layers, num_boxes


GRAD_KEYS = (("logits", "pred_logits"), ("boxes", "pred_boxes"), ("masks", "pred_masks"), ("visible", "pred_visible"))


def matched_planes(t, index):
    """[B,T,Q,h,w] -> [B,T,h,w] of the matched queries"""
    return torch.stack([t[b, :, int(index[b])] for b in range(t.shape[0])])


def off_query_mask(shape, index):
    """bool [B,T,Q,1..] that is True off the matched query"""
    m = torch.ones(shape[:3], dtype=torch.bool)
    for b in range(shape[0]):
        m[b, :, int(index[b])] = False
    return m
