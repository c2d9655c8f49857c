/* tce_rvos_refexp.h -- RefCOCO / RefCOCO+ / RefCOCOg evaluation-stage entry points of libtce_rvos.so: what the reference's image
 * evaluation (engine.py:97-161) does with the outputs of a forward -- the box and mask post-processors (models/postprocessors.py:
 * 58-155) for a group of samples, and the generalised IoU behind precision@k (datasets/refexp_eval.py:37-82, util/box_ops.py:44-81).
 *
 * The stage's host-side tests are in tests/test_refexp_cpu.py.
 *
 * Conventions of include/tce_rvos_eval.h: device pointers to contiguous memory, the caller owns all of it, every entry takes the
 * hipStream_t to launch on, is asynchronous, allocates nothing, never synchronises (legal inside hipGraph capture), returns
 * 0 = launched / <0 = rejected with a message behind the library's last-error string, before anything is launched.  No atomics,
 * every output byte written, launches ordered by the stream alone: the results are deterministic.
 */
#ifndef TCE_RVOS_REFEXP_H
#define TCE_RVOS_REFEXP_H
#include <stdint.h>

#include "tce_rvos.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TCE_REFEXP_GROUP_MAX 16   /* samples per call: the table is passed to the kernels by value (1152 bytes of kernel arguments) */
#define TCE_REFEXP_MAX_CAND 1024  /* Q*K candidates per sample: one workgroup ranks them in LDS */

/* One sample of the group.  The table is read on the HOST at the call. */
typedef struct {
  const float* logits;   /* [Q,K] class logits (outputs['pred_logits'][b].flatten(0,1)), contiguous, 4-byte aligned; NULL: a ranked
                            sample, whose order is an INPUT */
  const float* boxes_in; /* [Q,4] cx,cy,w,h normalised (outputs['pred_boxes'][b].flatten(0,1)), 4-byte aligned */
  const float* masks;    /* [Q,h,w] mask logits (outputs['pred_masks'][b].flatten(0,1)), 4-byte aligned; NULL: a box-only sample */
  float* scores;         /* [Q] the Q largest sigmoid values, descending, 4-byte aligned */
  int32_t* order;        /* [Q] their flat candidate indices into [Q*K] (topk_indexes), 4-byte aligned */
  float* boxes_out;      /* [Q,4] x0,y0,x1,y1 in pixels of the (H0, W0) image, 4-byte aligned */
  uint8_t* out;          /* [Q,H0,W0] 0/1, ANY address; NULL: a box-only sample */
  int32_t fh, fw;        /* the un-padded model-input size (max_target_sizes); fh <= 4h, fw <= 4w (not read for a box-only sample) */
  int32_t H0, W0;        /* the original image size (target_sizes / orig_target_sizes); Q*H0*W0 < 2^31 - 4096 */
} tceRefexpSample;

/* PostProcess + PostProcessSegm (postprocessors.py:72-100, 128-152) for B samples, 1 <= B <= TCE_REFEXP_GROUP_MAX, that share
 * Q = T*N (the reference's flatten(1, 2)), the class count K (1 with --binary) and the mask plane (h, w); 1 <= Q*K <=
 * TCE_REFEXP_MAX_CAND.  Per sample:
 *   scores   p[i] = 1 / (1 + expf(-logits[i])) over the Q*K flat candidates (the sigmoid of the A2D group entry, bit for bit).
 *   ranking  candidate i has rank r(i) = #{j : p[j] > p[i] or (p[j] == p[i] and j < i)}; for r < Q: scores[r] = p[i], order[r] = i.
 *            This is torch.topk(prob.view(bs, -1), k=num_queries, sorted=True) (:83).  The values ranked are the sigmoids, not the
 *            logits, so saturated logits tie as they do in the reference.  TIES GO TO THE LOWER FLAT INDEX: topk leaves the order
 *            of equal values unspecified, this is the project's rule.  A NaN ranks before every number (as topk places it), NaNs
 *            among themselves by index, so the ranks are a permutation whatever the input and every output word is written.
 *   boxes    with q = order[r] / K and (cx, cy, w, h) = boxes_in[q], in fp32, every operation rounded on its own:
 *            boxes_out[r] = ((cx - 0.5f*w) * W0, (cy - 0.5f*h) * H0, (cx + 0.5f*w) * W0, (cy + 0.5f*h) * H0)
 *            (:88-94, box_ops.py:29-33; 0.5f*w is exact, the bits are the reference's on a CPU tensor).
 *   masks    out[r] = byte for byte what the per-sample masks entry of include/tce_rvos_eval.h writes for the plane
 *            masks[order[r] / K] with (h, w, fh, fw, H0, W0, threshold) (:138-152): the x4 bilinear plane, the crop to (fh, fw),
 *            the nearest resize to (H0, W0), sigmoid > threshold -- on the shared rules of csrc/mask_planes.h.  The threshold
 *            given is used.
 * A sample is box-only when its masks or its out is NULL; the samples of one call are all box-only or none is (a mixture is
 * rejected), and for a box-only call h, w, fh, fw and threshold are not looked at and nothing is written through out.
 * A sample is ranked when its logits are NULL: its order is what an earlier call on the same logits left (the box-only call of
 * PostProcess, followed by PostProcessSegm), the rank launch is left out and boxes_in, scores and boxes_out are not used (NULL, or
 * 4-byte aligned like the rest).  Again all samples of a call or none; a ranked call has masks.  Every order[r] is clamped to
 * 0 .. Q*K-1 where the masks launch reads it.
 * At most two launches, ordered by the stream only: one workgroup per sample ranks its candidates in LDS by counting and writes
 * scores, order and boxes_out; then (unless box-only) grid (x, B) as the A2D group entry's, a byte quad per thread, reading order.
 * The output ranges of one call (scores, order, boxes_out, out of every sample) must not overlap each other: checked, rejected. */
int tce_refexp_group_u8(const tceRefexpSample* samples, int32_t B, int32_t Q, int32_t K, int32_t h, int32_t w, float threshold,
                        tceStream stream);

/* Generalised IoU of Q predicted boxes against the one ground-truth box of each of M images, and its running maximum: what
 * RefExpEvaluator.summarize compares with its threshold (refexp_eval.py:65-67).  All boxes x0,y0,x1,y1.  util/box_ops.py:44-81
 * operation for operation in fp32, none fused, with p = boxes[m,q] and g = gt[m]:
 *   area_p = (p.x1 - p.x0) * (p.y1 - p.y0), area_g likewise;
 *   inter  = max(min(p.x1, g.x1) - max(p.x0, g.x0), 0) * max(min(p.y1, g.y1) - max(p.y0, g.y0), 0);
 *   union  = (area_p + area_g) - inter;   iou = (inter + 1e-6f) / (union + 1e-6f);
 *   area   = max(max(p.x1, g.x1) - min(p.x0, g.x0), 0) * max(max(p.y1, g.y1) - min(p.y0, g.y0), 0);
 *   giou[m,q] = iou - ((area - union) + 1e-6f) / (area + 1e-6f);   best[m,q] = max(giou[m,0], .., giou[m,q])  (fmaxf).
 * The reference asserts x1 >= x0 and y1 >= y0 for both; here that is the caller's to hold (refexp_score.RefExpScorer checks the
 * ground truth on the host).  One launch, a workgroup per image.  1 <= M <= 65535, 1 <= Q <= 1024. */
int tce_refexp_giou_f32(const float* boxes /* [M,Q,4] */, const float* gt /* [M,4] */, float* giou /* [M,Q] */,
                        float* best /* [M,Q] */, int32_t M, int32_t Q, tceStream stream);

#ifdef __cplusplus
}
#endif
#endif
