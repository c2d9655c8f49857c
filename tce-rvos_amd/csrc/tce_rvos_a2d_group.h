/* tce_rvos_a2d_group.h -- the A2D-Sentences / JHMDB-Sentences post-processor's output stage for a GROUP of samples: what B calls
 * of the per-sample masks entry of include/tce_rvos_eval.h and B sigmoid launches do (models/postprocessors.py:38-47), in one launch.
 * The samples of a clip group (model.forward_group with valid_indices) share the query count and the mask plane; everything else is
 * per sample and travels in a table.
 *
 * STAGED like csrc/tce_rvos_a2d_score.h and for the same reasons (its top comment): exported from the same library, declared
 * beside its translation unit (csrc/a2d_group.hip), bound from _lib.A2D_GROUP_SIGNATURES (applied by lib() after the other staged
 * tables), without an access model in hazard.MODELS -- hazard._LibProxy refuses the name, so it is launched outside the clip's
 * launch program only.  The ABI version stays 5: the change only adds.  tests/test_single_frame_groups_cpu.py holds the table to
 * this header.
 *
 * Conventions: those of the stage headers of include/ (device pointers, the caller owns all memory, asynchronous on the given
 * stream, allocates nothing, never synchronises, legal inside hipGraph capture, 0 = launched / <0 = rejected with a message behind
 * the last-error call before anything is launched, no atomics, every byte of every output written).
 */
#ifndef TCE_RVOS_A2D_GROUP_H
#define TCE_RVOS_A2D_GROUP_H
#include <stdint.h>

#include "../../include/tce_rvos.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TCE_A2D_GROUP_MAX 16 /* samples per launch: the table is passed to the kernel by value (896 bytes of kernel arguments) */

/* One sample of the group.  The table is read on the HOST at the call. */
typedef struct {
  const float* masks;   /* [N,h,w] mask logits (outputs['pred_masks'][b,0]), contiguous, 4-byte aligned */
  const float* logits;  /* N class logits, logit_stride floats apart (outputs['pred_logits'][b,0,:,0]) */
  uint8_t* out;         /* [N,H0,W0] 0/1, ANY address */
  float* scores;        /* [N] sigmoid(logits), 4-byte aligned */
  int32_t fh, fw;       /* the un-padded model-input size (targets['size']); fh <= 4h, fw <= 4w */
  int32_t H0, W0;       /* the dataset's frame size; N*H0*W0 < 2^31 - 4096 */
  int32_t logit_stride; /* >= 1 */
  int32_t reserved;     /* 0 */
} tceA2dGroupSample;

/* For each of the B samples (1 <= B <= TCE_A2D_GROUP_MAX): out = the bytes the per-sample masks entry writes for (masks, N, h, w,
 * fh, fw, H0, W0, threshold) -- the resampling rule and the byte-quad store of csrc/mask_planes.h, so equal byte for byte at any
 * output address -- and scores[n] = 1 / (1 + expf(-logits[n * logit_stride])), the bits of the sigmoid entry of include/tce_rvos.h.
 * One launch: grid (x, B); sample b's workgroups own 1024 output bytes each (a byte quad per thread) and those past its own
 * N*H0*W0 exit; workgroup 0 of a sample also writes its N scores.  Outputs of different samples must not overlap. */
int tce_a2d_group_masks_u8(const tceA2dGroupSample* samples, int32_t B, int32_t N, int32_t h, int32_t w, float threshold,
                           tceStream stream);

#ifdef __cplusplus
}
#endif
#endif
