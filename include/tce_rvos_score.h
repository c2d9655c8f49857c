/* tce_rvos_score.h -- scoring-stage entry points of libtce_rvos.so: the integer counting behind the J&F score every Ref-DAVIS
 * user reports (davis2017/metrics.py: db_eval_iou :29-30, f_measure :81-97 with _seg2bmap :154-165), on label maps that stay on
 * the device.
 *
 * Same conventions as tce_rvos_video.h / tce_rvos_eval.h: device pointers to contiguous memory, the caller owns all of it, every
 * launching entry takes the hipStream_t to launch on, is asynchronous, allocates nothing, never synchronises (legal inside hipGraph
 * capture), returns 0 = launched / <0 = rejected with a message behind tce_last_error, before anything is launched.
 */
#ifndef TCE_RVOS_SCORE_H
#define TCE_RVOS_SCORE_H
#include <stdint.h>

#include "tce_rvos.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TCE_JF_MAX_OBJS   16     /* = TCE_LABEL_MAX_OBJS */
#define TCE_JF_MAX_RADIUS 40     /* 3840x2160 needs 36 */
#define TCE_JF_COUNTS     6

/* The six counts of every (object, frame) pair of two label-map stacks.  For object k < n and frame t, seg = (pred[t] == k+1) and
 * ann = (gt[t] == k+1); any other byte value belongs to no object (the 255 void label of the DAVIS PNGs, which davis.py:90-91
 * zeroes; prediction labels above n).  counts[k,t,:] =
 *   0  sum(seg & ann)                  metrics.py:29
 *   1  sum(seg | ann)                  metrics.py:30
 *   2  n_fg = sum(B(seg))              :96
 *   3  n_gt = sum(B(ann))              :97
 *   4  sum(B(seg) & dil(B(ann)))       the fg_match of :93
 *   5  sum(B(ann) & dil(B(seg)))       the gt_match of :92
 * B is _seg2bmap at equal size (:154-165), reads beyond the plane counting as 0: for y < H-1, x < W-1
 *   b = s[y,x]^s[y,x+1] | s[y,x]^s[y+1,x] | s[y,x]^s[y+1,x+1];  last row: b = s^s[y,x+1];  last column: b = s^s[y+1,x];
 *   b[H-1,W-1] = 0.
 * dil is the dilation by skimage's disk(radius) -- the offsets with dx*dx + dy*dy <= radius*radius -- with nothing beyond the plane
 * (cv2.dilate's default border adds nothing to a dilation).  No dilated plane is formed: a boundary pixel matches when one of the
 * 2*radius+1 rows of the other boundary map, kept as bit rows, has a bit within isqrt(radius^2 - dy^2) columns of it.
 *
 * Two launches ordered by the stream alone: one workgroup per (frame, 32 x 64 tile) leaves its six partial sums per object in ws,
 * one small launch adds them.  No atomics, no flags: every word of counts is written, the result is a function of pred and gt
 * alone, and the order in which workgroups finish does not matter.  ws: tce_jf_ws_bytes(...) bytes, 8-byte aligned, content
 * irrelevant before and after; counts 4-byte aligned; pred and gt at any address.
 * 0 <= radius <= TCE_JF_MAX_RADIUS, 1 <= n <= TCE_JF_MAX_OBJS, T*H*W < 2^31. */
int64_t tce_jf_ws_bytes(int32_t T, int32_t n, int32_t H, int32_t W, int32_t radius);   /* < 0: bad extents */
int tce_jf_counts_i32(const uint8_t* pred /* [T,H,W] */, const uint8_t* gt /* [T,H,W] */, int32_t* counts /* [n,T,6] */,
                      void* ws, int32_t T, int32_t n, int32_t H, int32_t W, int32_t radius, tceStream stream);

#ifdef __cplusplus
}
#endif
#endif
