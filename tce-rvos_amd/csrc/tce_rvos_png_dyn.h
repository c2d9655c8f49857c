/* tce_rvos_png_dyn.h -- the second encoding of the PNG-writing stage (csrc/tce_rvos_png.h): the same zlib stream in which every
 * strip's block is written with the fixed Huffman code or with a code of the strip's own (a dynamic block), whichever takes fewer
 * bits.  png.py reaches it as codes="dynamic"; the default stays the fixed stream of tce_rvos_png.h, byte for byte as it was.
 *
 * STAGED like tce_rvos_png.h and for the same reasons (its top comment): exported from the same library, declared beside its
 * translation unit (csrc/png.hip), bound from _lib.PNG_DYN_SIGNATURES (applied by lib() after PNG_SIGNATURES), without an access
 * model in hazard.MODELS -- hazard._LibProxy refuses the name.  A header and a table of its own because tests pin the three names of
 * tce_rvos_png.h.  The ABI version stays 5: the change only adds.
 *
 * THE STREAM is one exact encoding, so that a host restatement (tests/_png_dyn.py) and the kernel are compared byte for byte.
 * Unchanged from tce_rvos_png.h: the value map, filter type 0, the strips, the tokens of a run, 78 01, the stored-block header and
 * 00 00 FF FF behind every strip, the final 03 00, the Adler-32.  What changes is the strip's block:
 *   counts          c[s] = how many of the strip's tokens use literal/length symbol s = 0 .. 285 (a literal: its byte; a match: its
 *                   length symbol; end-of-block: c[256] = 1); X = the sum of the matches' extra bits; M = the number of matches.
 *   code lengths    of an alphabet with counts c and a limit: (1) the used symbols are those with c > 0; (2) sorted by (count,
 *                   symbol) ascending they are the leaves; Huffman's algorithm with two queues, the leaves and the merged nodes in
 *                   the order they are made; the lighter head is taken, of two equal weights the leaf; a symbol's length is its
 *                   leaf's depth; (3) if a length exceeds the limit, every used count becomes (c + 1) >> 1 and (2) is done again;
 *                   (4) codes are assigned as in RFC 1951 section 3.2.2.  (A single used symbol would get length 1: no stream has
 *                   such an alphabet -- a strip has a literal and symbol 256, a header a zero run or two different lengths.)
 *   literal/length  lengths l[s] from c with limit 15.  HLIT = nlit - 257, nlit = the highest used symbol + 1.
 *   distance        one code, symbol 0 with length 1: HDIST = 0, every match ends with one zero bit.
 *   length sequence l[0 .. nlit) followed by the distance length 1, as symbols of the code-length alphabet, greedily from the left.
 *                   A maximal run of r zeros: while r >= 11, symbol 18 for t = min(r, 138) (7 extra bits, t - 11), r -= t; then if
 *                   r >= 3, symbol 17 (3 extra bits, r - 3); else r single zeros.  A maximal run of r lengths v > 0: v once, r -= 1;
 *                   while r >= 3, symbol 16 for t = min(r, 6) (2 extra bits, t - 3), r -= t; then r single v.
 *   code-length     lengths from the counts of those symbols with limit 7.  HCLEN = ncl - 4, ncl = max(4, the last position in
 *                   the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15 with a non-zero length, + 1).
 *   the choice      fixed   = 3 + sum c[s] * (the fixed code's length of s) + X + 5 M
 *                   dynamic = 3 + 14 + 3 ncl + the bits of the length sequence + sum c[s] * l[s] + X + M
 *                   both exact, from the true counts; the block is dynamic if dynamic < fixed, else exactly the fixed block.
 *   a dynamic block BFINAL = 0, BTYPE = 10, HLIT (5 bits), HDIST (5), HCLEN (4), ncl three-bit lengths in the order above, the
 *                   length sequence, the tokens (a match: length code, extra bits, one zero bit), symbol 256.
 * Every strip costs at most its fixed block, so TCE_PNG_STRIP_BOUND, the two queries of tce_rvos_png.h and the workspace layout hold
 * for this entry as they are, and a stream is never longer than the fixed stream of the same plane and rows_per_strip.  A code pays
 * for its header (a few dozen bytes) per strip: strips of 32 or 64 rows make smaller files than strips of 8.
 *
 * Conventions: those of tce_rvos_png.h (device pointers, asynchronous, allocates nothing, legal inside hipGraph capture, rejected
 * with a message behind tce_last_error before anything is launched, deterministic, workspace content irrelevant).
 */
#ifndef TCE_RVOS_PNG_DYN_H
#define TCE_RVOS_PNG_DYN_H
#include <stdint.h>

#include "tce_rvos_png.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The arguments, alignment rules and limits of the fixed entry of tce_rvos_png.h; streams rows and ws are sized by its two queries.
 * Three launches: (1) a workgroup of 256 threads per (plane, strip) walks the strip's filtered bytes twice.  The first walk finds
 * the runs as the fixed kernel does and counts their tokens into a histogram in LDS (integer atomics).  Then the workgroup sorts
 * the used symbols (a rank count per symbol), one lane merges them and takes the depths, builds the code-length code the same way,
 * sums both bit totals, chooses, and writes the block header into the bit window.  The second walk writes the tokens through the
 * chosen table (the fixed code's table if that won).  (2) and (3) are the launches of the fixed entry. */
int tce_png_deflate_dyn_u8(const uint8_t* planes /* [P,H,W] */, uint8_t* streams /* [P,bound] */, int32_t* nbytes /* [P] */,
                           void* ws, int32_t P, int32_t H, int32_t W, int32_t rows_per_strip, int32_t nonzero_value, tceStream stream);

#ifdef __cplusplus
}
#endif
#endif
