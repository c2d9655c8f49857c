/* tce_rvos_eval.h -- evaluation-stage entry points of libtce_rvos.so: what the reference's A2D-Sentences / JHMDB-Sentences
 * post-processor (models/postprocessors.py:14-54, called by engine.py:308-319) does with the outputs of one forward
 * (csrc/eval.hip), and its output stage for a GROUP of samples in one launch (csrc/a2d_group.hip).
 *
 * Same conventions as tce_rvos_video.h: device pointers to contiguous memory, the caller owns all of it, every launching entry
 * takes the hipStream_t to launch on, is asynchronous, allocates nothing, never synchronises (legal inside hipGraph capture),
 * returns 0 = launched / <0 = rejected with a message behind tce_last_error.
 *
 * Each entry cites the reference code whose arithmetic it replaces.
 */
#ifndef TCE_RVOS_EVAL_H
#define TCE_RVOS_EVAL_H
#include <stdint.h>

#include "tce_rvos.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Dataset-size binary masks of one sample (postprocessors.py:39-47), one launch, 1 byte written per output pixel and no
 * intermediate plane: per output pixel (n, yo, xo) of out [N,H0,W0]
 *   ys  = min((int)floorf(yo * ((float)fh / (float)H0)), fh - 1), xs likewise from fw, W0   (:47, F.interpolate "nearest" with
 *         size=: ONE fp32 multiply, as ATen; the integer formula (yo*fh)/H0 differs at some indices)
 *   v   = value at (ys, xs) of the x4 bilinear (align_corners=False) up-sampling of masks[n] [h,w]   (:39; the crop of :45 is
 *         the restriction ys < fh, xs < fw, so fh <= 4h and fw <= 4w)
 *   out = 1/(1+expf(-v)) > threshold ? 1 : 0                                                 (:40, where threshold is 0.5)
 * masks is fp32 [N,h,w] (outputs['pred_masks'][b,0]); (fh, fw) = targets['size'], the un-padded model input; (H0, W0) =
 * orig_size.  `out` needs no alignment: whole dwords are written wherever four consecutive bytes of the flat plane are one
 * aligned word, whatever W0, bytes at the two ends. */
int tce_a2d_masks_u8(const float* masks /* [N,h,w] */, uint8_t* out /* [N,H0,W0] */, int32_t N, int32_t h, int32_t w,
                     int32_t fh, int32_t fw, int32_t H0, int32_t W0, float threshold, tceStream stream);

/* Uncompressed COCO run lengths of P masks (cocoapi rleEncode on the column-major mask, which postprocessors.py:48 reaches
 * through mask_util.encode of a Fortran-order copy): with position p = x*H + y, bit(p) = masks[y,x] != 0, bit(-1) = 0 and
 * q_0 < .. < q_{m-1} the positions where bit(p) != bit(p-1),
 *   counts[0..m] = q_0, q_1 - q_0, .., H*W - q_{m-1}   ([H*W] when m = 0);   nruns = m + 1.
 * The first count is a run of zeros (0 when the mask starts with a 1); the counts sum to H*W.  counts is [P, H*W+1]: row p
 * holds its nruns[p] counts and zeros behind them (every word of the row is written, so the whole buffer is a function of
 * the masks alone).
 * Two launches over segments of TCE_RLE_SEGMENT consecutive positions, ordered by the stream only: the first leaves each
 * segment's boundary count and last boundary position in ws, the second places every count.  No atomics, no flags, no waiting:
 * the result is deterministic.  ws: tce_rle_ws_bytes(P,H,W) bytes, 8-byte aligned, content irrelevant before and after.
 * H*W < 2^31, P <= 65535. */
#define TCE_RLE_SEGMENT 1024
int64_t tce_rle_ws_bytes(int32_t P, int32_t H, int32_t W); /* < 0: bad extents */
int tce_rle_counts_u32(const uint8_t* masks /* [P,H,W] */, uint32_t* counts /* [P,H*W+1] */, int32_t* nruns /* [P] */,
                       void* ws, int32_t P, int32_t H, int32_t W, tceStream stream);

/* ---- The output stage for a group of samples: what B calls of tce_a2d_masks_u8 and B sigmoid launches do
 * (models/postprocessors.py:38-47), in one launch.  The samples of a clip group (model.forward_group with valid_indices) share the
 * query count and the mask plane; everything else is per sample and travels in a table.  No atomics, every byte of every output
 * written. */
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
