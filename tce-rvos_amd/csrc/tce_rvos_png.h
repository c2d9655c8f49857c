/* tce_rvos_png.h -- PNG-writing stage entry points of libtce_rvos.so: the zlib stream (row filter bytes, deflate, Adler-32) of every
 * uint8 output plane, made on the device, so that the host reads back a few KB per mask instead of the plane and only adds the PNG
 * chunk framing (tce_rvos_amd/png.py).  What the reference's drivers end with: inference_ytvos.py:354-363 (binary masks, mode 'L')
 * and inference_davis.py:300-311 (palettised label maps, mode 'P').
 *
 * WHY THIS HEADER IS HERE AND NOT IN include/: the same reasons as csrc/tce_rvos_a2d_score.h (its top comment; DESIGN.md section
 * 3.15).  These entries are STAGED: exported from the same library, declared beside their translation unit (csrc/png.hip), bound
 * from _lib.PNG_SIGNATURES (applied by lib() after the staged table), without an access model in hazard.MODELS -- inside a recorded
 * launch program hazard._LibProxy refuses every name of this header, the two launch-free queries included (ops.py asks them of the
 * library itself, _lib.lib_raw()).  The ABI version stays 5: the change only adds.
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
 * Conventions of the stage headers of include/: device pointers, the caller owns all memory, the launching entry takes the
 * hipStream_t to launch on, is asynchronous, allocates nothing, never synchronises (legal inside hipGraph capture), returns 0 =
 * launched / <0 = rejected with a message behind tce_last_error, before anything is launched.  Launches are ordered by the stream
 * alone; no atomics between workgroups, no flags; workspace content is irrelevant before and after; the result is deterministic.
 */
#ifndef TCE_RVOS_PNG_H
#define TCE_RVOS_PNG_H
#include <stdint.h>

#include "../../include/tce_rvos.h"

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

#ifdef __cplusplus
}
#endif
#endif
