/* tce_rvos_train.h -- entry points of libtce_rvos_train.so, the training-side sibling of libtce_rvos.so: the forward values of the
 * reference's SetCriterion (models/criterion.py) and of the matcher it calls (models/matcher.py), and the gradients of its losses
 * with respect to the model's outputs ((c), (d) at the end), csrc_train/criterion.hip.
 *
 * The library is separate from the inference one: its own version, its own last-error string, its own binding table
 * (tce_rvos_amd/_train_lib.py TRAIN_SIGNATURES); no name here occurs in a header of include/.
 *
 * Conventions of include/tce_rvos_eval.h: device pointers to contiguous memory, the caller owns all of it, every launching entry
 * takes the hipStream_t to launch on, is asynchronous, allocates nothing, never synchronises (legal inside hipGraph capture),
 * returns 0 = launched / <0 = rejected before anything is launched, with a message behind tce_train_last_error.  No atomics, every
 * output word written, results deterministic (fixed reduction trees, launches ordered by the stream only).
 *
 * In this fork every clip has ONE target, so the matcher is the minimum of a [Q,1] cost column (matcher.py:234-237), and its mask
 * costs and the mask losses are functions of the same three sums per query.
 */
#ifndef TCE_RVOS_TRAIN_H
#define TCE_RVOS_TRAIN_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* tceStream; /* hipStream_t */

#define TCE_TRAIN_ABI_VERSION 1
#define TCE_CRIT_MAX_B 64   /* clips per call */
#define TCE_CRIT_MAX_T 64   /* frames per clip */
#define TCE_CRIT_MAX_Q 1024 /* queries */
#define TCE_CRIT_MAX_K 128  /* class logits per query */
#define TCE_CRIT_CHUNK 4096 /* elements of one query's T*h*w that one workgroup of the mask walk owns */

int32_t tce_train_abi_version(void);      /* TCE_TRAIN_ABI_VERSION */
const char* tce_train_last_error(void);   /* of the calling thread */

/* ---- (a) Mask sums of B clips of one shape: one walk of pred [B,T,Q,h,w] (the model's own layout) against the stride-4 samples of
 * the un-padded target masks tgt [B,T,H,W] uint8 (non-zero = 1).  The target of element (t, y, x) is
 *   tv = (4y+2 < H && 4x+2 < W) ? tgt[t, 4y+2, 4x+2] != 0 : 0
 * which is nested_tensor_from_tensor_list(size_divisibility=32) followed by [2::4, 2::4] (matcher.py:110-122, criterion.py:169-179)
 * with no padded tensor.  Rejected unless 4h == ceil32(H) and 4w == ceil32(W) (the reference's two asserts).
 *
 * Per element, fp32, in this order (v = pred value, z = tv ? -v : v; fp contraction off):
 *   e  = expf(-|v|)                                   r = 1 / (1 + e)
 *   s  = v >= 0 ? r : e * r                           = sigmoid(v)
 *   m  = z >= 0 ? r : e * r                           = sigmoid(z) = 1 - p_t, NOT formed by subtraction
 *   ce = max(z, 0) + log1pf(e)                        = binary_cross_entropy_with_logits(v, tv), the stable form
 *   f  = (tv ? alpha : 1 - alpha) * (ce * (m * m))    the order of segmentation.py:504-508 with gamma = 2
 * Deviations from the reference's order: it forms 1 - p_t as 1 - (prob*t + (1-prob)*(1-t)), which cancels where prob -> 1; m above
 * is the same quantity without the cancellation.  1 - alpha is one fp32 subtraction on the host.
 * Sums over all T*h*w elements of query q, every term converted to fp64 before it is added (per-thread fp64 partials, a wavefront
 * shuffle tree, an LDS tree over the four wavefronts, then a second launch that adds the workgroup partials of ws in index order):
 *   sums[b,0,q] = S_f = sum f     sums[b,1,q] = S_p = sum s     sums[b,2,q] = S_pt = sum s*tv     st[b] = S_t = sum tv
 * Two launches: grid (ceil(T*h*w / TCE_CRIT_CHUNK), Q, B) then grid B.  pred is read once, with 16-byte loads when pred is 16-byte
 * aligned and w % 4 == 0, else one float at a time (any 4-byte aligned base); a target byte is fetched per element, rows are not
 * staged.  ws: tce_criterion_mask_sums_ws_bytes bytes, 8-byte aligned, content irrelevant before and after.
 * 1 <= B <= 64, T <= 64, Q <= 1024, T*h*w < 2^30. */
int64_t tce_criterion_mask_sums_ws_bytes(int32_t B, int32_t T, int32_t Q, int32_t h, int32_t w); /* < 0: bad extents */
int tce_criterion_mask_sums_f64(const float* pred /* [B,T,Q,h,w] */, const uint8_t* tgt /* [B,T,H,W] */, double* sums /* [B,3,Q] */,
                                double* st /* [B] */, void* ws, int32_t B, int32_t T, int32_t Q, int32_t h, int32_t w, int32_t H,
                                int32_t W, float alpha, tceStream stream);

/* The host scalars of (b). */
typedef struct {
  float cost_class, cost_bbox, cost_giou, cost_mask, cost_dice, cost_vis; /* matcher.py:53-76 */
  float focal_alpha; /* of loss_ce and loss_vis (criterion.py:89,120); the matcher's class / visibility costs use its own 0.25 */
} tceCriterionConsts;

/* ---- (b) Per-clip cost column, match and loss parts, then the batch's losses.  Two launches: grid B (a workgroup per clip), then
 * one workgroup.  All arithmetic on values is fp32 in the reference's order unless stated; sums over frames or logits of loss parts
 * are fp64 sums of fp32 terms.
 *
 * cost[b,q] (matcher.py:141-231), an fp32 accumulator C = 0 to which the present terms are added in this order:
 *   class (if any frame is valid):  cost_class * (sum over valid t of cls(logits[t,q,c_t])) / nvalid, c_t = 0 when K == 1 else
 *       labels[t] (clamped into [0,K-1]);  cls(x): p = 1/(1+expf(-x)); pos = (0.25*((1-p)*(1-p))) * (-logf(p + 1e-8f));
 *       neg = (0.75*(p*p)) * (-logf((1-p) + 1e-8f)); cls = pos - neg
 *   L1    (if any frame is valid):  cost_bbox * (sum over valid t of sum_j |pred_boxes[t,q,j] - boxes[t,j]|) / nvalid
 *   gIoU  (if any frame is valid):  cost_giou * (sum over valid t of -giou(xyxy(pred_boxes[t,q]), xyxy(boxes[t]))) / nvalid
 *       xyxy(c) = (cx - 0.5*w, cy - 0.5*h, cx + 0.5*w, cy + 0.5*h); giou is util/box_ops.py:44-81 operation for operation with this
 *       fork's 1e-6 terms: iou = (inter + 1e-6)/(union + 1e-6); giou = iou - ((area - union) + 1e-6)/(area + 1e-6)
 *   visibility (if visible != NULL): cost_vis * (sum over ALL t of cls(visible[t,q])) / T
 *   mask  (if sums != NULL):        cost_mask * (float)(S_f[q]/(T*h*w)) + cost_dice * -(float)((2*S_pt[q] + 1)/(S_p[q] + S_t + 1)),
 *       the two quotients in fp64
 * index[b] = the q of the smallest cost; TIES GO TO THE LOWER INDEX (torch.min leaves the order open; a NaN never wins, all-NaN
 * gives 0).
 *
 * parts[b,0..5], fp64, with idx = index[b] and focal() the per-element f of (a) with alpha = focal_alpha:
 *   0 loss_ce    sum over all (t,q,k) of focal(logits[t,q,k], valid[t] && q == idx && k == c_t)          (criterion.py:60-89)
 *   1 loss_bbox  sum over ALL t, j of |pred_boxes[t,idx,j] - boxes[t,j]|                                 (:126-147)
 *   2 loss_giou  sum over ALL t of 1 - giou(xyxy(pred_boxes[t,idx]), xyxy(boxes[t]))                     (:149-152)
 *   3 loss_mask  S_f[idx] / (T*h*w)                             (0 when sums == NULL)                    (:189)
 *   4 loss_dice  1 - (2*S_pt[idx] + 1)/(S_p[idx] + S_t + 1)     (0 when sums == NULL)                    (:190)
 *   5 loss_vis   (sum over t of focal(visible[t,idx], valid[t] != 0)) / T / T * (T*Q)  (0 when visible == NULL)  (:97-123)
 * losses[j] = (float)((sum over b of parts[b,j]) / num_boxes[0]) for j < 5; losses[5] = (float)(sum over b of parts[b,5]) (the
 * reference divides loss_vis by the frame count, not by num_boxes).  num_boxes is one device float, read by the second launch.
 *
 * logits [B,T,Q,K], pred_boxes [B,T,Q,4], visible [B,T,Q] or NULL, sums [B,3,Q] and st [B] of (a) or both NULL (then h, w are
 * ignored), labels [B,T] int64, boxes [B,T,4] cxcywh, valid [B,T] int32 (non-zero = valid).
 * 1 <= B <= 64, T <= 64, Q <= 1024, K <= 128. */
int tce_criterion_match_losses_f32(const float* logits, const float* pred_boxes, const float* visible, const double* sums,
                                   const double* st, const int64_t* labels, const float* boxes, const int32_t* valid,
                                   const float* num_boxes, float* cost /* [B,Q] */, int32_t* index /* [B] */,
                                   double* parts /* [B,6] */, float* losses /* [6] */, int32_t B, int32_t T, int32_t Q, int32_t K,
                                   int32_t h, int32_t w, const tceCriterionConsts* consts /* host */, tceStream stream);

/* ==== The backward of the losses with respect to the model's outputs.  Additions to version 1: nothing above changes.  Both entries
 * read num_boxes[0] = n and the upstream gradients gl[6] = dL/d losses[j] (the order of losses[6]) from the device; both are one
 * launch.  index, sums and st are what (a) and (b) left for the same inputs. */

/* ---- (c) d L / d pred of loss_mask and loss_dice, grad [B,T,Q,h,w] fp32, every word written.  Grid (ceil(T*h*w / TCE_CRIT_CHUNK),
 * Q, B) as (a).  A workgroup with q != index[b] stores +0.0 and reads nothing but index[b].  A workgroup of the matched query reads
 * pred once and fetches tv as (a) defines it.  With idx = index[b], N = T*h*w, in fp64 and then rounded once to fp32:
 *   D = S_p[idx] + S_t + 1        Gm  = gl[3] / n / N
 *   Gd0 = gl[4]/n * (2*S_pt[idx] + 1)/D^2            Gd1 = gl[4]/n * ((2*S_pt[idx] + 1)/D^2 - 2/D)
 * Per element, fp32, contraction off, with e, r, er = e*r, s, m, ce, z of (a):
 *   mc = z >= 0 ? er : r                              = 1 - m, NOT formed by subtraction
 *   sc = v >= 0 ? er : r                              = 1 - s, NOT formed by subtraction
 *   df = (tv ? alpha : 1 - alpha) * ((m*m) * (m + 2*(ce*mc)))          dfs = tv ? -df : df       = d f / d v
 *   grad = Gm * dfs + (tv ? Gd1 : Gd0) * (s*sc)
 * Where e underflows (|v| > 87) the terms are 0 or the saturated slope, never NaN.  pred is read with 16-byte loads when its base is
 * 16-byte aligned, grad is written with 16-byte stores when its base is; either falls back to one float at a time on its own (any
 * 4-byte aligned base), with the same bits.  Extents and the shape precondition are those of (a). */
int tce_criterion_mask_grad_f32(const float* pred /* [B,T,Q,h,w] */, const uint8_t* tgt /* [B,T,H,W] */, const double* sums /* [B,3,Q] */,
                                const double* st /* [B] */, const int32_t* index /* [B] */, const float* num_boxes, const float* gl /* [6] */,
                                float* grad /* [B,T,Q,h,w] */, int32_t B, int32_t T, int32_t Q, int32_t h, int32_t w, int32_t H,
                                int32_t W, float alpha, tceStream stream);

/* ---- (d) d L / d logits, pred_boxes, visible.  Grid (ceil(T*Q*K / 256), B).  An output pointer that is NULL is skipped; one at
 * least is given; g_visible needs visible.  dfs(v, tv, alpha) is (c)'s, alpha = consts->focal_alpha (the other fields are not read).
 *   g_logits[b,t,q,k]  = (float)(gl[0]/n) * dfs(logits[b,t,q,k], valid[t] && q == idx && k == c_t)       at every (t,q,k)
 *   g_visible[b,t,q]   = q == idx ? (float)(gl[5]*Q/T) * dfs(visible[t,idx], valid[t] != 0) : +0.0        for ALL t
 *   g_boxes[b,t,q,j]   = q == idx ? (float)(gl[1]/n) * sign(p_j - g_j) + (float)(gl[2]/n) * dg_j : +0.0   for ALL t, sign(0) = 0
 * dg = d(1 - giou)/dp, fp32, the chain of (b)'s giou in reverse (p the predicted box, g the target's, both cxcywh):
 *   x0 = p0 - 0.5*p2, x1 = p0 + 0.5*p2, y0 = p1 - 0.5*p3, y1 = p1 + 0.5*p3; gx0 .. gy1 the same of g
 *   wp = x1 - x0, hp = y1 - y0, area_p = wp*hp, area_g = (gx1 - gx0)*(gy1 - gy0)
 *   ax = min(x1,gx1) - max(x0,gx0), ay likewise; iw = max(ax,0), ih = max(ay,0); inter = iw*ih
 *   uni = (area_p + area_g) - inter; du = uni + 1e-6; iou = (inter + 1e-6)/du
 *   cx = max(x1,gx1) - min(x0,gx0), cy likewise; ew = max(cx,0), eh = max(cy,0); area = ew*eh; da = area + 1e-6
 *   r2 = ((area - uni) + 1e-6)/da
 *   d_area = (1 - r2)/da;  d_uni = iou/du - 1/da;  d_inter = (-1/du) - d_uni
 *   d_iw = d_inter*ih, d_ih = d_inter*iw, d_ew = d_area*eh, d_eh = d_area*ew, d_wp = d_uni*hp, d_hp = d_uni*wp
 *   d_x0 = -d_wp, d_x1 = d_wp; if ax > 0: { if x1 <= gx1: d_x1 += d_iw;  if x0 >= gx0: d_x0 -= d_iw }
 *                              if cx > 0: { if x1 >= gx1: d_x1 += d_ew;  if x0 <= gx0: d_x0 -= d_ew }      (y likewise)
 *   dg = (d_x0 + d_x1, d_y0 + d_y1, 0.5*(d_x1 - d_x0), 0.5*(d_y1 - d_y0))
 * The sub-gradients at the kinks, where torch splits or picks otherwise: min / max of EQUAL arguments hand the whole gradient to the
 * predicted box's corner (torch halves it); a clamp whose argument is exactly 0 (or negative) passes nothing (torch passes it at 0);
 * sign(0) = 0 as torch.  Extents as (b). */
int tce_criterion_head_grads_f32(const float* logits, const float* pred_boxes, const float* visible, const int64_t* labels,
                                 const float* boxes, const int32_t* valid, const int32_t* index, const float* num_boxes,
                                 const float* gl /* [6] */, float* g_logits /* [B,T,Q,K] | NULL */, float* g_boxes /* [B,T,Q,4] | NULL */,
                                 float* g_visible /* [B,T,Q] | NULL */, int32_t B, int32_t T, int32_t Q, int32_t K,
                                 const tceCriterionConsts* consts /* host */, tceStream stream);

#ifdef __cplusplus
}
#endif
#endif
