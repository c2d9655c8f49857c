/* tce_rvos_score.h -- scoring-stage entry points of libtce_rvos.so, on planes that stay on the device.  Ref-DAVIS (csrc/score.hip):
 * the integer counting behind the J&F score every Ref-DAVIS user reports (davis2017/metrics.py: db_eval_iou :29-30, f_measure
 * :81-97 with _seg2bmap :154-165), on label maps.  A2D-Sentences / JHMDB-Sentences (csrc/a2d_score.hip): what the reference's
 * scorer (datasets/a2d_eval.py:12-45, and the mask IoU under COCOeval) does with run-length masks: run lengths back to planes, and
 * the overlap counts of N prediction planes against one ground-truth plane.
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

/* ---- A2D-Sentences / JHMDB-Sentences scoring.  Beyond the conventions above: launches are ordered by the stream alone; no
 * atomics, no flags; every word of every output is written; workspace content is irrelevant before and after.  The two *_ws_bytes
 * queries launch nothing. */

/* Planes of P run-length masks: the inverse of tce_rle_counts_u32: cocoapi rleDecode on the column-major plane.
 * counts is uint32 [P,stride], nruns int32 [P] (read on the device): the layout tce_rle_counts_u32 leaves with stride = H*W+1,
 * but any stride >= 1 is legal.  With m = min(max(nruns[p],0), stride), c_i = counts[p,i] and e_i = min(c_0 + .. + c_i, H*W)
 * (summed without 32-bit wrap), position q = x*H + y lies in run i(q) = the number of i < m with e_i <= q, and
 *   out[p,y,x] = i(q) < m ? (i(q) & 1) : 0.
 * So zero-length runs flip parity as in cocoapi, positions behind the last run decode to 0, counts running past the plane are
 * clipped, and no content of counts or nruns can make a launch read outside counts[p, 0..m) or write outside out.
 * Three launches: the clipped sum of every segment of TCE_RLE_SEGMENT counts (of the segments below m) into ws; every e_i, i < m,
 * into ws (a segment adds the sums of the segments before it to the scan of its own counts); then one thread per ALIGNED dword of
 * a plane of out finds the run of each of its four positions by bisection over e_0 .. e_{m-1} and stores the dword: whole dwords
 * along rows although the runs go down columns, bytes at the two ends of a plane.  out [P,H,W] row-major at any address.
 * ws: tce_rle_decode_ws_bytes(...) bytes, 8-byte aligned; counts and nruns 4-byte aligned.
 * H*W < 2^31 - 4096 (the byte-quad arithmetic is 32-bit, as in tce_a2d_masks_u8), 1 <= P <= 65535, stride >= 1. */
#ifndef TCE_RLE_SEGMENT
#define TCE_RLE_SEGMENT 1024
#endif
int64_t tce_rle_decode_ws_bytes(int32_t P, int32_t H, int32_t W, int32_t stride); /* < 0: bad extents; launches nothing */
int tce_rle_decode_u8(const uint32_t* counts /* [P,stride] */, const int32_t* nruns /* [P] */, uint8_t* out /* [P,H,W] */,
                      void* ws, int32_t P, int32_t H, int32_t W, int32_t stride, tceStream stream);

/* Overlap counts of N prediction planes against one ground-truth plane; any nonzero byte counts as set:
 *   counts[n] = (sum(pred[n] != 0 & gt != 0), sum(pred[n] != 0), sum(gt != 0))
 * -- what a2d_eval.compute_iou (:12-17) and maskUtils.iou need, the union being counts[n][1] + counts[n][2] - counts[n][0].
 * Two launches: a workgroup per tile of TCE_OVERLAP_TILE consecutive bytes of the plane reads its piece of gt ONCE, walks the N
 * predictions over it and leaves per-tile partial sums in ws; one small launch adds them.  pred [N,H,W] and gt [H,W] at any
 * address (aligned dwords are fetched wherever four bytes of a plane are one aligned word); counts int32 [N,3], 4-byte aligned;
 * ws: tce_mask_overlap_ws_bytes(...) bytes, 8-byte aligned.  H*W < 2^31 - 4096, 1 <= N <= 65535. */
#define TCE_OVERLAP_TILE 1024
int64_t tce_mask_overlap_ws_bytes(int32_t N, int32_t H, int32_t W); /* < 0: bad extents; launches nothing */
int tce_mask_overlap_i32(const uint8_t* pred /* [N,H,W] */, const uint8_t* gt /* [H,W] */, int32_t* counts /* [N,3] */, void* ws,
                         int32_t N, int32_t H, int32_t W, tceStream stream);

#ifdef __cplusplus
}
#endif
#endif
