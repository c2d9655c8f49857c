"""PNG files of output planes that stay on the GPU: what the reference's inference drivers end with.

    inference_ytvos.py:354-363   Image.fromarray(mask * 255).convert('L').save(...)       -> mask_pngs(run_video(...)["masks"])
    inference_davis.py:300-311   Image.fromarray(labels), putpalette(palette), save(...)  -> label_pngs(run_video_objects(...)[i]["labels"], palette)
    the --visualize images       Image.fromarray(frame with box, point, mask).save(...)    -> rgb_pngs(vis.overlay_expression(...))

The device makes each plane's complete zlib stream (ops.png_deflate, include/tce_rvos_png.h: filter bytes, deflate, Adler-32); the host
reads back the byte counts and then only the bytes in use -- a few KB per mask instead of the plane -- and adds the chunk framing
below.  The files decode to the same pixels as the reference's.  With codes="fixed" (the default: the stream as it always was) they
are several times LARGER than Pillow's (fixed Huffman codes, run-length matches only, a flush per strip of 8 rows).  With
codes="dynamic" every strip's block takes the cheaper of the fixed code and a Huffman code of its own (tce_png_deflate_dyn_u8) and
the strips are DYNAMIC_ROWS_PER_STRIP rows: files about the size of Pillow's (DESIGN.md section 3.16 has the measured sizes and
times), never longer than the fixed stream of the same strips.  RGB images (rgb_pngs, frame_rgb) take a row filter chosen per
row on the device and then the dynamic stream over the filtered rows (ops.png_filter_rgb, ops.png_deflate_rows); with no distance
matches a photograph's file is larger than Pillow's.  The framing functions need neither the GPU nor the
shared library.
"""
import struct
import zlib

SIGNATURE = b"\x89PNG\r\n\x1a\n"
COLOUR_TYPE = {"L": 0, "P": 3}
FIXED_ROWS_PER_STRIP = 8
# of 16, 32 and 64 (tools/png_bench.py, profiles/r15_png_dyn.txt): none is as fast as the fixed code; 32 is the fastest at 720 x 1280,
# 9 % behind 16 at 480 x 854 with files 16 % smaller; 64 is the slowest at both for 8 % smaller files
DYNAMIC_ROWS_PER_STRIP = 32


def chunk(kind, data):
    """length, type, data, CRC-32 of type and data"""
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def palette_bytes(palette):
    """The PLTE data of a palette given the way Image.putpalette takes it: bytes, or a flat sequence of R, G, B values; 1 .. 256 entries"""
    data = bytes(palette)
    if len(data) == 0 or len(data) % 3 or len(data) > 768:
        raise ValueError(f"png: a palette holds 1 .. 256 RGB triples, got {len(data)} bytes")
    return data


FRAMINGS = ("host", "device")


def head(width, height, mode, palette=None):
    """What stands in front of the IDAT chunk of frame(): signature, IHDR and, for mode 'P', PLTE, each chunk with its own CRC.  33
    bytes for 'L', 45 + 3 per palette entry for 'P' (at most 813).  The same for every file of one encode call."""
    if mode not in COLOUR_TYPE:
        raise ValueError(f"png: mode must be 'L' or 'P', got {mode!r}")
    if (palette is None) != (mode == "L"):
        raise ValueError("png: mode 'P' needs a palette and mode 'L' takes none")
    width, height = int(width), int(height)
    if not (0 < width < 2 ** 31 and 0 < height < 2 ** 31):
        raise ValueError(f"png: bad size {(width, height)}")
    out = [SIGNATURE, chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, 8, COLOUR_TYPE[mode], 0, 0, 0))]
    if mode == "P":
        out.append(chunk(b"PLTE", palette_bytes(palette)))
    return b"".join(out)


def head_rgb(width, height):
    """What stands in front of the IDAT chunk of frame_rgb(): signature and IHDR (colour type 2), 33 bytes"""
    width, height = int(width), int(height)
    if not (0 < width < 2 ** 31 and 0 < height < 2 ** 31):
        raise ValueError(f"png: bad size {(width, height)}")
    return SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, 8, 2, 0, 0, 0))


def _check_framing(framing):
    if framing not in FRAMINGS:
        raise ValueError(f"png: framing must be 'host' or 'device', got {framing!r}")


def _device_files(streams, nbytes, head_bytes):
    """framing="device": the chunk framing and the IDAT's CRC-32 on the device (ops.png_file), then the two read-backs -- the P file
    lengths, the rows' prefix in use -- and the rows sliced: no zlib.crc32, no chunk(), no join over the IDAT."""
    from . import ops
    files, file_bytes = ops.png_file(streams, nbytes, head_bytes)
    used = file_bytes.cpu().tolist()                               # read-back 1: P integers
    flat = files[:, :max(used)].cpu().numpy()                      # read-back 2: the bytes in use
    return [flat[p, :n].tobytes() for p, n in enumerate(used)]


def frame(stream, width, height, mode, palette=None):
    """One complete PNG file around a zlib stream of the height * (width + 1) filtered bytes of an 8-bit image: signature, IHDR
    (bit depth 8, colour type 0 for 'L' and 3 for 'P', no interlace), PLTE for 'P', one IDAT, IEND.  (RGB images: frame_rgb.)"""
    return b"".join([head(width, height, mode, palette), chunk(b"IDAT", bytes(stream)), chunk(b"IEND", b"")])


def encode(planes, mode, palette=None, nonzero_value=0, rows_per_strip=None, codes="fixed", framing="host"):
    """One complete PNG file (bytes) per plane of a uint8 [P,H,W] tensor on the GPU.  One device call (three launches), one
    read-back of the P byte counts, one read-back of the streams' prefixes in use, then the framing.  codes: "fixed" or "dynamic";
    rows_per_strip = None: 8 for the fixed code, DYNAMIC_ROWS_PER_STRIP for dynamic codes.  (RGB images: rgb_pngs.)
    framing="device": the framing and the IDAT chunk's CRC-32 are made on the device too (ops.png_file: two more launches, one more
    [P, bound + head + 24] buffer); the two read-backs are then of the file lengths and of the files.  The same bytes either way."""
    from . import ops
    _check_framing(framing)
    if codes not in ("fixed", "dynamic"):
        raise ValueError(f"png: codes must be 'fixed' or 'dynamic', got {codes!r}")
    if rows_per_strip is None:
        rows_per_strip = FIXED_ROWS_PER_STRIP if codes == "fixed" else DYNAMIC_ROWS_PER_STRIP
    if mode not in COLOUR_TYPE or (palette is None) != (mode == "L"):
        frame(b"", 1, 1, mode, palette)  # raises with the message
    if mode == "P":
        palette = palette_bytes(palette)
    streams, nbytes = ops.png_deflate(planes, rows_per_strip=rows_per_strip, nonzero_value=nonzero_value, codes=codes)
    if framing == "device":
        return _device_files(streams, nbytes, head(int(planes.shape[2]), int(planes.shape[1]), mode, palette))
    used = nbytes.cpu().tolist()                                   # read-back 1: P integers
    flat = streams[:, :max(used)].cpu().numpy()                    # read-back 2: the bytes in use (the longest stream's prefix of every row)
    H, W = int(planes.shape[1]), int(planes.shape[2])
    return [frame(flat[p, :n].tobytes(), W, H, mode, palette) for p, n in enumerate(used)]


def mask_pngs(masks, rows_per_strip=None, codes="fixed", framing="host"):
    """The files inference_ytvos.py:354-363 writes, from run_video(...)["masks"] (uint8 [N,H0,W0] of 0/1 on the GPU): mode 'L',
    0 and 255."""
    return encode(masks, "L", nonzero_value=255, rows_per_strip=rows_per_strip, codes=codes, framing=framing)


def label_pngs(labels, palette, rows_per_strip=None, codes="fixed", framing="host"):
    """The files inference_davis.py:308-311 writes, from run_video_objects(...)[i]["labels"] (uint8 [T,H0,W0] on the GPU): mode
    'P' with the caller's palette bytes (what Image.putpalette takes), the labels as they are."""
    return encode(labels, "P", palette=palette, rows_per_strip=rows_per_strip, codes=codes, framing=framing)


def frame_rgb(stream, width, height):
    """One complete PNG file around a zlib stream of the height * (3 * width + 1) filtered bytes of an 8-bit RGB image: signature,
    IHDR (bit depth 8, colour type 2, no interlace), one IDAT, IEND.  A function of its own: frame() keeps to the modes 'L' and
    'P' of 8-bit planes and rejects every other mode, as it always did."""
    return b"".join([head_rgb(width, height), chunk(b"IDAT", bytes(stream)), chunk(b"IEND", b"")])


def rgb_pngs(images, rows_per_strip=None, framing="host"):
    """One complete PNG file (bytes) per image of a uint8 [P,H,W,3] tensor on the GPU, colour type 2: the --visualize images of the
    reference's drivers (vis.overlay_expression / vis.overlay_objects make the pixels).  Two device calls (the row filter: one
    launch; the dynamic stream over the filtered rows: three), then the same two read-backs as the other modes and the framing.
    rows_per_strip = None: DYNAMIC_ROWS_PER_STRIP.  framing: as encode -- "device" is where it pays: an overlay's IDAT is megabytes
    and the host's CRC-32 over it is nearly all of the host's share.  The Ref-DAVIS reference saves these
    images as RGBA with a constant alpha of 255 (inference_davis.py:291); the files here are RGB, which decode to the same colours."""
    from . import ops
    _check_framing(framing)
    if rows_per_strip is None:
        rows_per_strip = DYNAMIC_ROWS_PER_STRIP
    rows = ops.png_filter_rgb(images)
    streams, nbytes = ops.png_deflate_rows(rows, rows_per_strip=rows_per_strip)
    if framing == "device":
        return _device_files(streams, nbytes, head_rgb(int(images.shape[2]), int(images.shape[1])))
    used = nbytes.cpu().tolist()                                   # read-back 1: P integers
    flat = streams[:, :max(used)].cpu().numpy()                    # read-back 2: the bytes in use
    H, W = int(images.shape[1]), int(images.shape[2])
    return [frame_rgb(flat[p, :n].tobytes(), W, H) for p, n in enumerate(used)]


def write_files(paths, blobs):
    """blobs[k] -> paths[k].  Directory layout and file names are the caller's business; the directories must exist."""
    paths, blobs = list(paths), list(blobs)
    if len(paths) != len(blobs):
        raise ValueError(f"png: {len(paths)} paths for {len(blobs)} files")
    for path, blob in zip(paths, blobs):
        with open(path, "wb") as f:
            f.write(blob)
