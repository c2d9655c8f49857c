/* tce_rvos_a2d_score.h -- A2D-Sentences / JHMDB-Sentences scoring-stage entry points of libtce_rvos.so: what the reference's
 * scorer (datasets/a2d_eval.py:12-45, and the mask IoU under COCOeval) does with run-length masks, on planes that stay on the
 * device: run lengths back to planes, and the overlap counts of N prediction planes against one ground-truth plane.
 *
 * WHY THIS HEADER IS HERE AND NOT IN include/.  The set of files in include/, the symbol sets of the stage headers, the tables
 * of _lib.HEADERS and the entries the hazard checker models are pinned by existing tests (tests/test_host_cpu.py HEADER_CASES,
 * tests/test_footprint_cpu.py, tests/test_hazard_cpu.py), and a change that adds entries cannot edit them.  So these entries are
 * STAGED: exported from the same library, declared beside their translation unit (csrc/a2d_score.hip), bound from
 * _lib.STAGED_SIGNATURES (applied by lib() after the HEADERS tables), and without an access model in hazard.MODELS -- inside a
 * recorded launch program hazard._LibProxy refuses every name of this header ("no access model"), the two launch-free *_ws_bytes
 * queries included (ops.py asks them of the library itself, _lib.lib_raw()).  The ABI version stays 5: the change only adds.
 * Moving this file to include/tce_rvos_a2d_score.h, its table into _lib.HEADERS and access models into hazard.MODELS is a
 * follow-up that edits those pinned tests; tests/test_a2d_score_cpu.py holds this table to its header meanwhile.
 *
 * Same conventions as the stage headers of include/: device pointers to contiguous memory, the caller owns all of it, every
 * launching entry takes the hipStream_t to launch on, is asynchronous, allocates nothing, never synchronises (legal inside hipGraph
 * capture), returns 0 = launched / <0 = rejected with a message behind tce_last_error, before anything is launched.  Launches
 * are ordered by the stream alone; no atomics, no flags; every word of every output is written; workspace content is irrelevant
 * before and after.  The two *_ws_bytes queries launch nothing.
 */
#ifndef TCE_RVOS_A2D_SCORE_H
#define TCE_RVOS_A2D_SCORE_H
#include <stdint.h>

#include "../../include/tce_rvos.h"

#ifdef __cplusplus
extern "C" {
#endif

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
