/* tce_rvos_png.h -- PNG-writing stage entry points of libtce_rvos.so: the zlib stream (row filter bytes, deflate, Adler-32) of every
 * uint8 output plane, made on the device, so that the host reads back a few KB per mask instead of the plane and only adds the PNG
 * chunk framing (tce_rvos_amd/png.py).  What the reference's drivers end with: inference_ytvos.py:354-363 (binary masks, mode 'L')
 * and inference_davis.py:300-311 (palettised label maps, mode 'P').  Two encodings of the same stream (csrc/png.hip): every strip's
 * block with the fixed Huffman code (tce_png_deflate_u8, the default of png.py), or with the cheaper of the fixed code and a code
 * of the strip's own (tce_png_deflate_dyn_u8, codes="dynamic"; "THE DYNAMIC STREAM" below).
 *
 * THE STREAM is one exact encoding, so that a host restatement (tests/_png.py) and the kernel are compared byte for byte: RLE-only
 * deflate with the fixed Huffman code of RFC 1951, PNG filter type 0 on every row, strips that are independent of each other.
 * For a plane [H,W] of bytes and S = rows_per_strip:
 *   value map       nonzero_value = v in 1..255: every nonzero byte is encoded as v (0/1 masks -> 0/255); v = 0: bytes as they are.
 *   filtered bytes  each row is one byte 0 followed by its W mapped bytes; a strip is the concatenation of the filtered bytes of its
 *                   S rows (the last strip may have fewer).  Runs may cross row ends inside a strip, never a strip's end.
 *   stream          78 01; per strip, in order: a block with BFINAL = 0, BTYPE = 01, its tokens, end-of-block (symbol 256), a
 *                   stored-block header (3 bits 0,00), zero bits to the byte boundary, 00 00 FF FF -- so every strip starts and
 *                   ends on a byte boundary; then a final empty fixed block (03 00); then the Adler-32 of all filtered bytes,
 *                   big-endian.
 *   tokens of a maximal run of L equal bytes b:  literal b; r = L - 1; while r >= 261 or r == 258: a match of length 258, r -= 258;
 *                   if r is 259 or 260: a match of length r - 3, r = 3; if r >= 3: a match of length r, else r more literals b.
 *                   Every match has distance 1 (distance code 0: five zero bits).
 *   codes           RFC 1951 section 3.2.6; bits fill bytes from the least significant bit, Huffman codes most-significant-bit
 *                   first, extra bits least-significant first; a length uses the largest base <= it, 258 is always symbol 285.
 * A strip of n filtered bytes costs at most 9n + 13 bits, rounded up to a byte, plus 4 bytes (TCE_PNG_STRIP_BOUND); a plane costs
 * 2 bytes + its strips + 2 + 4 = tce_png_stream_bound.  The file is several times the size of zlib's at its default level (fixed
 * codes, matches of at most 258 bytes, a 5-byte flush per strip): the price of a stream whose strips are made independently.
 *
 * Conventions of the other stage headers: device pointers, the caller owns all memory, the launching entry takes the
 * hipStream_t to launch on, is asynchronous, allocates nothing, never synchronises (legal inside hipGraph capture), returns 0 =
 * launched / <0 = rejected with a message behind tce_last_error, before anything is launched.  Launches are ordered by the stream
 * alone; no atomics between workgroups, no flags; workspace content is irrelevant before and after; the result is deterministic.
 */
#ifndef TCE_RVOS_PNG_H
#define TCE_RVOS_PNG_H
#include <stdint.h>

#include "tce_rvos.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of a strip of n filtered bytes, at most */
#define TCE_PNG_STRIP_BOUND(n) ((9ll * (n) + 13 + 7) / 8 + 4)

/* The row length of streams: the most bytes the stream of one [H,W] plane can take.  H, W, rows_per_strip >= 1, H*W < 2^31; the
 * bound itself must stay below 2^31 - 4096 (nbytes is int32), which holds for every H*W + H <= 1.9e9; and a plane has at most
 * TCE_PNG_MAX_STRIPS strips (a launch has a workgroup per strip). */
#define TCE_PNG_MAX_STRIPS (1 << 22)
int64_t tce_png_stream_bound(int32_t H, int32_t W, int32_t rows_per_strip);        /* launches nothing; < 0: bad extents */
int64_t tce_png_ws_bytes(int32_t P, int32_t H, int32_t W, int32_t rows_per_strip); /* launches nothing; < 0: bad extents */

/* streams[p, 0 .. nbytes[p]) = the zlib stream of planes[p]; bytes of a row of streams behind nbytes[p] are not written.
 * Three launches: (1) a workgroup per (plane, strip) walks the strip's filtered bytes in passes of TCE_PNG_PASS bytes: it finds the
 * run boundaries, takes the prefix sum of the runs' bit counts, packs the bits (in LDS, whole dwords to the workspace) and sums the
 * strip's Adler pair; (2) a workgroup per plane scans the strips' byte counts into offsets, combines the Adler pairs in strip
 * order, writes the header, the final block, the trailer and nbytes[p]; (3) a workgroup per (plane, strip) copies the strip to its
 * offset.  planes [P,H,W] and streams [P,bound] (bound = tce_png_stream_bound) at any address: whole dwords are loaded and stored
 * wherever four bytes are one aligned word.  nbytes int32 [P], 4-byte aligned.  ws: tce_png_ws_bytes(...) bytes, 8-byte aligned.
 * 1 <= P <= 65535, 1 <= rows_per_strip, 0 <= nonzero_value <= 255. */
#define TCE_PNG_PASS 2048
int tce_png_deflate_u8(const uint8_t* planes /* [P,H,W] */, uint8_t* streams /* [P,bound] */, int32_t* nbytes /* [P] */,
                       void* ws, int32_t P, int32_t H, int32_t W, int32_t rows_per_strip, int32_t nonzero_value, tceStream stream);

/* THE DYNAMIC STREAM (tce_png_deflate_dyn_u8) is one exact encoding too, so that a host restatement (tests/_png_dyn.py) and the
 * kernel are compared byte for byte.  Unchanged from the fixed stream: the value map, filter type 0, the strips, the tokens of a
 * run, 78 01, the stored-block header and 00 00 FF FF behind every strip, the final 03 00, the Adler-32.  What changes is the
 * strip's block:
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
 * Every strip costs at most its fixed block, so TCE_PNG_STRIP_BOUND, the two queries and the workspace layout hold for this entry
 * as they are, and a stream is never longer than the fixed stream of the same plane and rows_per_strip.  A code pays for its header
 * (a few dozen bytes) per strip: strips of 32 or 64 rows make smaller files than strips of 8. */

/* The arguments, alignment rules and limits of the fixed entry; streams rows and ws are sized by its two queries.
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
