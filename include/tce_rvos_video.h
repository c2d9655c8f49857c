/* tce_rvos_video.h -- driver-stage entry points of libtce_rvos.so: what the reference's inference drivers do with the
 * outputs of several forwards (one per referred object) AFTER the per-clip forward of include/tce_rvos.h.
 *
 * Same conventions as tce_rvos.h: device pointers to contiguous fp32 unless stated, the caller owns all memory, every
 * entry takes the hipStream_t to launch on, is asynchronous, allocates nothing, never synchronises (legal inside hipGraph
 * capture), returns 0 = launched / <0 = rejected with a message behind tce_last_error.  Tables of pointers are HOST arrays
 * read at launch time (as tce_copy_segments reads its segments).
 *
 * Each entry cites the reference code whose arithmetic it replaces.
 */
#ifndef TCE_RVOS_VIDEO_H
#define TCE_RVOS_VIDEO_H
#include <stdint.h>

#include "tce_rvos.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Ref-DAVIS label map of one chunk (inference_davis.py:239-248 per object, :293-298 per annotator): all objects of a
 * label map combined in one pass, 1 byte written per output pixel and no full-size fp32 plane in between.
 *   per object k < n:  best_query[k] = argmax_q max_k' mean_t sigmoid(logits_k[t,q,k'])   (first maximum wins, as
 *                      tce_select_masks_u8);
 *                      v_k = bilinear(align_corners=False) up-sampling of masks_k[t, best_query[k]] [h,w] to [H0,W0];
 *                      s_k = sigmoid(v_k), set to 0 where s_k < threshold           (:248, :294)
 *   labels[t,y,x]    = index of the first maximum of [background, s_0, .., s_{n-1}]  (:295-297; 0 = background, k + 1 =
 *                      object k).  The comparison is made on the fp32 SCORES: objects that both saturate to 1.0f tie and
 *                      the lower index wins, as torch.argmax does.
 * Two launches: the n best queries (one wavefront per object), then the pixels (whole dwords of labels wherever four
 * consecutive bytes of the plane are one aligned word, whatever W0; `labels` itself needs no alignment).
 * 1 <= n <= TCE_LABEL_MAX_OBJS; best_query [n] int32 is required (the pixel launch reads it). */
#define TCE_LABEL_MAX_OBJS 16
typedef struct tceLabelObj {
  const float* logits; /* [T,Q,K] */
  const float* masks;  /* [T,Q,h,w] */
} tceLabelObj;
int tce_label_objects_u8(const tceLabelObj* objs /* HOST [n] */, int32_t n, uint8_t* labels /* [T,H0,W0] */,
                         int32_t* best_query /* [n] */, int32_t T, int32_t Q, int32_t K, int32_t h, int32_t w, int32_t H0,
                         int32_t W0, float threshold /* 0.5 */, float background /* 0.1 */, tceStream stream);

#ifdef __cplusplus
}
#endif
#endif
