/* tce_rvos_pngfile.h -- PNG-file stage entry points of libtce_rvos.so: the finished PNG file around every zlib stream that the
 * PNG-writing stage made on the device (include/tce_rvos_png.h, include/tce_rvos_vis.h): the IDAT chunk's CRC-32 and the chunk framing,
 * so that what the host reads back is the file and no zlib.crc32 runs over the IDAT (tce_rvos_amd/png.py, framing="device").
 *
 * The stage's host-side tests are in tests/test_png_file_cpu.py.
 *
 * THE FILE is one exact layout, so that a host restatement (tests/_png_file.py) and the kernel are compared byte for byte.  With
 * n = nbytes[p] clamped to [0, stream_stride], files[p, 0 .. file_bytes[p]) is, in order:
 *   head                                      head_bytes bytes, the same for every file of a call: signature, IHDR and, for mode 'P',
 *                                             PLTE, each chunk with its own CRC, made on the host (png.chunk); at most 813 bytes
 *   BE32(n)                                   the IDAT chunk's length, big-endian
 *   "IDAT"
 *   streams[p, 0 .. n)
 *   BE32(crc)                                 crc = the PNG / zlib CRC-32 of the 4 type bytes followed by the n data bytes: reflected
 *                                             polynomial 0xEDB88320, initial value and final xor 0xFFFFFFFF
 *   00 00 00 00 49 45 4E 44 AE 42 60 82       the IEND chunk
 * file_bytes[p] = head_bytes + 24 + n; tce_png_file_bound = head_bytes + 24 + stream_stride.  Bytes of a row of files behind
 * file_bytes[p] are not written.
 *
 * THE COMPUTATION.  raw(M) is the CRC register after the bytes M from a zero start, without the final xor; mul is the product in
 * GF(2)[x] mod G and X(k) = x^k mod G, both in the reflected representation (bit 31 is the coefficient of x^0).  Then
 *   raw(A || B) = mul(raw(A), X(8 * len(B))) ^ raw(B)          and          raw(0^k || M) = raw(M)
 *   crc32(M)    = mul(0xFFFFFFFF, X(8 * len(M))) ^ raw(M) ^ 0xFFFFFFFF
 * Two launches (csrc/pngfile.hip).
 * (1) A workgroup of 256 threads per (file, segment), a segment being TCE_PNG_FILE_SEGMENT bytes of the stream; the grid is sized
 *     by stream_stride and a workgroup whose segment starts at or behind n returns.  One pass over the segment's len bytes: they are
 *     loaded into LDS, stored to their place in the file, and their raw value is taken.  Every lane covers a contiguous piece of
 *     TCE_PNG_FILE_PIECE bytes through four 256-entry tables held in LDS (a dword a step).  The pieces are laid from the segment's
 *     END: lane q covers bytes (q + 1 - 256) * PIECE + len - PIECE .. of the segment, clipped at byte 0, so that only the first
 *     piece in use can be short and zero bytes in front of it change nothing.  Behind piece q lie exactly (255 - q) * PIECE bytes:
 *     every lane's shift is a constant, raw(segment) = the xor over q of mul(raw(piece q), X(8 * PIECE * (255 - q))), which is the
 *     in-order combination written as a sum.  The value goes to ws[p, segment].
 * (2) A workgroup of 256 threads per file.  With F = the number of segments in front of the last one in use, the values
 *     K, raw(segment 0), .., raw(segment F - 1) -- K = the register after "IDAT" from the initial value, which carries the
 *     initial-value term -- are combined in order with the constant shift X(8 * SEGMENT) (a contiguous run per thread, then each
 *     thread's value by the power for what lies behind its run); the last segment, of 1 .. SEGMENT bytes, needs x^k for a length
 *     read on the device, by square and multiply; then the final xor.  The workgroup writes head, length, type, CRC, IEND and
 *     file_bytes[p].
 * No atomics between workgroups, no flags: the result is deterministic and workspace content is irrelevant before and after.
 *
 * ADDRESSES.  Stream rows start at any address (stream_stride is the deflate bound, often odd); the data lands at head_bytes + 8 in
 * a row of any stride, so source and destination disagree modulo 4.  Whole dwords are loaded and stored wherever four bytes are
 * one aligned word (the first and last dword of a segment, of the head and the 16 bytes behind the data go byte by byte).
 *
 * Conventions of the other stage headers: device pointers, the caller owns all memory, the launching entry takes the
 * hipStream_t to launch on, is asynchronous, allocates nothing, never synchronises (legal inside hipGraph capture), returns 0 =
 * launched / <0 = rejected with a message behind tce_last_error, before anything is launched.  Launches are ordered by the stream
 * alone.
 */
#ifndef TCE_RVOS_PNGFILE_H
#define TCE_RVOS_PNGFILE_H
#include <stdint.h>

#include "tce_rvos.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TCE_PNG_FILE_PIECE 64      /* bytes of a stream that one lane takes the CRC of */
#define TCE_PNG_FILE_SEGMENT 16384 /* bytes of a stream that one workgroup copies and takes the CRC of: 256 pieces */
#define TCE_PNG_FILE_MIN_HEAD 8
#define TCE_PNG_FILE_MAX_HEAD 1024

/* The row length of files that holds every file of streams of stream_stride bytes: head_bytes + 24 + stream_stride.
 * TCE_PNG_FILE_MIN_HEAD <= head_bytes <= TCE_PNG_FILE_MAX_HEAD, 1 <= stream_stride, the bound itself below 2^31 - 4096. */
int64_t tce_png_file_bound(int32_t head_bytes, int64_t stream_stride); /* launches nothing; < 0: bad extents */

/* Bytes of ws: one 32-bit value per (file, segment), rounded up to 8.  1 <= P <= 65535, 1 <= stream_stride < 2^31. */
int64_t tce_png_file_ws_bytes(int32_t P, int64_t stream_stride); /* launches nothing; < 0: bad extents */

/* files[p, 0 .. file_bytes[p]) = THE FILE of streams[p, 0 .. nbytes[p]); two launches (above).  streams [P,stream_stride], head
 * [head_bytes] and files [P,file_stride] at any address; nbytes and file_bytes int32 [P], 4-byte aligned; ws:
 * tce_png_file_ws_bytes(P, stream_stride) bytes, 8-byte aligned.  1 <= P <= 65535, 8 <= head_bytes <= 1024, 1 <= stream_stride,
 * tce_png_file_bound(head_bytes, stream_stride) <= file_stride < 2^31 - 4096.  files (its P rows, bound bytes of each) overlaps
 * none of streams, nbytes, head, file_bytes and ws. */
int tce_png_file_u8(const uint8_t* streams /* [P,stream_stride] */, const int32_t* nbytes /* [P] */,
                    const uint8_t* head /* [head_bytes] */, int32_t head_bytes, uint8_t* files /* [P,file_stride] */,
                    int32_t* file_bytes /* [P] */, void* ws, int32_t P, int64_t stream_stride, int64_t file_stride, tceStream stream);

#ifdef __cplusplus
}
#endif
#endif
