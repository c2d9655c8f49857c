/* tce_rvos_vis.h -- visualisation-stage entry points of libtce_rvos.so: the --visualize images of the reference's inference drivers
 * (the decoded frame with box, reference point and mask tint drawn on it) made on the device, and their RGB PNG streams.
 *
 * The stage's host-side tests are in tests/test_vis_cpu.py.
 *
 * Conventions of the other stage headers: device pointers, the caller owns all memory, every entry takes the hipStream_t to launch
 * on, is asynchronous, allocates nothing, never synchronises (legal inside hipGraph capture), returns 0 = launched / <0 = rejected
 * with a message behind the library's last-error string, before anything is launched.  Launches are ordered by the stream alone.
 */
#ifndef TCE_RVOS_VIS_H
#define TCE_RVOS_VIS_H
#include <stdint.h>

#include "tce_rvos.h"
#include "tce_rvos_png.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The --visualize image of the reference's drivers (inference_ytvos.py:325-351, inference_davis.py:269-291, the same block in
 * inference_mevis.py): the decoded frame with the predicted box, the decoder's reference point and the mask tint drawn on it, in
 * one pass over the pixels (csrc/vis.hip).  THE RULE is exact, so that a host restatement (tests/_vis.py) and the kernel are
 * compared byte for byte.  out[n,y,x] starts as frames[n,y,x]; layers l = 0 .. L-1 are applied in order, with c = colors[l]:
 *   box    (boxes given)  in fp32, every operation rounded on its own (no fused multiply-add), as rescale_bboxes computes on a CPU
 *          tensor:  xmin = (cx - 0.5f*w) * W0, ymin = (cy - 0.5f*h) * H0, xmax = (cx + 0.5f*w) * W0, ymax = (cy + 0.5f*h) * H0;
 *          X0, Y0, X1, Y1 = these truncated toward zero (clamped to +-2^30 first; a NaN counts as -2^30).
 *          X1 - X0 >= 2 and Y1 - Y0 >= 2: the pixel becomes c where X0 <= x <= X1, Y0 <= y <= Y1 and x - X0 < 2 or X1 - x < 2 or
 *          y - Y0 < 2 or Y1 - y < 2: ImageDraw.rectangle(..., width=2) of Pillow 12.2.0, clipped to the image.
 *          Otherwise (a THIN box) the filled rectangle [X0..X1] x [Y0..Y1] clipped to the image, nothing if X1 < X0 or Y1 < Y0.
 *          A stated deviation: Pillow's outline loop overshoots such a box by up to two pixels.
 *   point  (points given) in double: x = W0 * (double)px, y = H0 * (double)py.  The pixel becomes c in rows trunc(y)-1 .. trunc(y)+2,
 *          columns trunc(x-10) .. trunc(x+10), and in columns trunc(x)-1 .. trunc(x)+2, rows trunc(y-10) .. trunc(y+10): the two
 *          draw.line(..., width=4) calls of draw_reference_points.
 *   mask   (masks given, masks[l,n,y,x] != 0)  every channel p becomes (p + c) >> 1: vis_add_mask's origin*0.5 + color*0.5 stored
 *          into a uint8 array.
 * masks, boxes and points may each be NULL (that part is not drawn).  The colours are the caller's.  One launch, a workgroup's
 * threads each own one ALIGNED dword of a frame of out (first and last dword of a frame byte by byte), so W0*3 needs no alignment
 * and frames / out may start at any address; a frame's layer geometry is computed once per workgroup.  3 + L bytes are read and 3
 * written per pixel.  out must not overlap frames.  1 <= L <= TCE_VIS_MAX_LAYERS, 1 <= N <= 65535, H0*W0*3 < 2^31. */
#define TCE_VIS_MAX_LAYERS 16
int tce_vis_overlay_u8(const uint8_t* frames /* [N,H0,W0,3] */, uint8_t* out /* [N,H0,W0,3] */,
                       const uint8_t* masks /* [L,N,H0,W0] 0 / nonzero, or NULL */,
                       const float* boxes /* [L,N,4] cx,cy,w,h normalised, or NULL */,
                       const float* points /* [L,N,2] x,y normalised, or NULL */, const uint8_t* colors /* [L,3] */, int32_t L,
                       int32_t N, int32_t H0, int32_t W0, tceStream stream);

/* RGB: the --visualize images of the reference's drivers are photographs with a few things drawn on them (tce_vis_overlay_u8 above
 * makes them).  Filter type 0 and run-length matches alone would leave such an image at its raw size, so an RGB
 * image takes two calls: a row filter chosen per row, then the dynamic stream over the filtered rows as they are.
 *
 * tce_png_filter_rgb_u8: rows[p,y,0] = the row's PNG filter type t in 0 .. 4; rows[p,y,1 .. 3W] = the row's 3W bytes filtered with
 * type t at 3 bytes per pixel (PNG specification section 9: None, Sub, Up, Average, Paeth; the prior row of y = 0 is all zero).  The
 * filters read the RAW bytes of the row above, so rows are independent of each other.  t is the type whose filtered bytes, read as
 * signed 8-bit values, have the least sum of absolute values; a tie goes to the lowest type.  The rule is exact (tests/_png_rgb.py
 * restates it).  One launch, a workgroup per row: five sums, one reduction, then the chosen row; whole dwords are loaded and stored
 * wherever four bytes are one aligned word, img and rows at any address.  1 <= P <= 65535, W <= 2^24, H * (3W + 1) < 2^31 - 4096. */
int tce_png_filter_rgb_u8(const uint8_t* img /* [P,H,W,3] */, uint8_t* rows /* [P,H,1+3W] */, int32_t P, int32_t H, int32_t W,
                          tceStream stream);

/* THE DYNAMIC STREAM over rows that are filtered already: the filtered bytes of row y are rows[p,y,0 .. R) as they are -- no filter
 * byte is put in front and no value map is applied.  Everything else is the dynamic entry's of include/tce_rvos_png.h: the strips, the tokens, the
 * choice between the fixed and the dynamic block, the flush behind every strip, the trailer, the Adler-32, TCE_PNG_STRIP_BOUND, the
 * three launches and the workspace layout (the strip kernel's byte source has a second compile-time form; nothing else differs).
 * streams rows and ws are sized by the two queries called with W = R - 1.  R >= 2; the other limits as above with W = R - 1.
 * There are no distance matches, so a photograph's file is larger than zlib's (DESIGN.md section 3.22 has the measured sizes). */
int tce_png_deflate_rows_u8(const uint8_t* rows /* [P,H,R] */, uint8_t* streams /* [P,bound] */, int32_t* nbytes /* [P] */, void* ws,
                            int32_t P, int32_t H, int32_t R, int32_t rows_per_strip, tceStream stream);

#ifdef __cplusplus
}
#endif
#endif
