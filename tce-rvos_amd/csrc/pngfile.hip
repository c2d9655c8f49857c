// PNG-file stage kernels (csrc/tce_rvos_pngfile.h): the finished PNG file around every zlib stream -- the stream's bytes copied to
// their place, the IDAT chunk's CRC-32, head, length, type and IEND -- in two launches.  Byte and table kernels: bound by LDS traffic
// and by the streams' bytes going through once, not by arithmetic.
#include "common.h"
#include "../../include/tce_rvos_pngfile.h"

namespace {

constexpr int FT = 256, FWAVES = FT / 64;
constexpr int PIECE = TCE_PNG_FILE_PIECE, SEG = TCE_PNG_FILE_SEGMENT;
static_assert(PIECE % 4 == 0 && PIECE * FT == SEG, "a segment is one piece per lane");
constexpr uint32_t POLY = 0xEDB88320u;
constexpr uint32_t ONE = 0x80000000u;  // x^0 in the reflected representation

// the product in GF(2)[x] mod G, reflected: bit 31 of a is its coefficient of x^0
__host__ __device__ constexpr uint32_t mul(uint32_t a, uint32_t b) {
  uint32_t p = 0u;
  for (int i = 0; i < 32; ++i) {
    p ^= (a & 0x80000000u) ? b : 0u;
    a <<= 1;
    b = (b >> 1) ^ ((b & 1u) ? POLY : 0u);
  }
  return p;
}

// base^e
__host__ __device__ constexpr uint32_t power(uint32_t base, unsigned long long e) {
  uint32_t r = ONE;
  while (e) {
    if (e & 1ull) r = mul(r, base);
    base = mul(base, base);
    e >>= 1;
  }
  return r;
}

constexpr uint32_t X1 = 0x40000000u;                      // x
constexpr uint32_t XPIECE = power(X1, 8ull * PIECE);      // x^(8 PIECE)
constexpr uint32_t XSEG = power(X1, 8ull * SEG);          // x^(8 SEGMENT)

// the register after one byte from a zero start
__host__ __device__ constexpr uint32_t byte_step(uint32_t c) {
  for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? POLY : 0u);
  return c;
}

// K: the register after "IDAT" from the initial value 0xFFFFFFFF (no final xor)
__host__ __device__ constexpr uint32_t idat_state() {
  uint32_t c = 0xFFFFFFFFu;
  const uint32_t t[4] = {0x49u, 0x44u, 0x41u, 0x54u};
  for (int i = 0; i < 4; ++i) c = (c >> 8) ^ byte_step((c ^ t[i]) & 255u);
  return c;
}
constexpr uint32_t KIDAT = idat_state();
static_assert((KIDAT ^ 0xFFFFFFFFu) == 0x35AF061Eu, "CRC-32 of \"IDAT\"");

// SHIFT.v[j] = x^(8 PIECE j): what a piece with j pieces behind it is multiplied by
struct PieceShift {
  uint32_t v[FT];
};
constexpr PieceShift piece_shift() {
  PieceShift s{};
  uint32_t x = ONE;
  for (int j = 0; j < FT; ++j) {
    s.v[j] = x;
    x = mul(x, XPIECE);
  }
  return s;
}
__constant__ const PieceShift SHIFT = piece_shift();

// The segment's bytes in LDS as the aligned dwords of the source that hold them, one pad dword behind every 16: lane q's piece starts
// 16 q dwords in, so its dwords fall into different banks.
constexpr int RAW_DW = SEG / 4 + 2;
__device__ __forceinline__ int phys(const int d) { return d + (d >> 4); }
constexpr int RAW_PHYS = RAW_DW + (RAW_DW >> 4) + 1;

// bytes B .. B+3 of the staged bytes (B >= 0, any alignment)
__device__ __forceinline__ uint32_t lds_dword(const uint32_t* raw, const int B) {
  const int d = B >> 2, sh = (B & 3) * 8;
  const uint32_t lo = raw[phys(d)];
  if (sh == 0) return lo;
  return (lo >> sh) | (raw[phys(d + 1)] << (32 - sh));
}

__device__ __forceinline__ uint32_t lds_byte(const uint32_t* raw, const int B) { return (raw[phys(B >> 2)] >> ((B & 3) * 8)) & 255u; }

__device__ __forceinline__ uint32_t wg_xor(uint32_t v, uint32_t* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v ^= (uint32_t)__shfl_xor((int)v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] ^ red[1] ^ red[2] ^ red[3];
}

__device__ __forceinline__ int clamp_n(const int n, const long long stride) {
  return n < 0 ? 0 : ((long long)n > stride ? (int)stride : n);
}

// First launch: a workgroup per (file, segment).
__global__ void __launch_bounds__(FT) png_file_segment_kernel(const uint8_t* __restrict__ streams, const int* __restrict__ nbytes,
                                                              uint8_t* __restrict__ files, uint32_t* __restrict__ ws, const int head_bytes,
                                                              const long long stream_stride, const long long file_stride, const int nseg) {
  __shared__ uint32_t raw[RAW_PHYS];
  __shared__ uint32_t tab[4][256];
  __shared__ uint32_t red[FWAVES];
  const int tid = threadIdx.x, seg = blockIdx.x, p = blockIdx.y;
  const int n = clamp_n(nbytes[p], stream_stride);
  const long long s0 = (long long)seg * SEG;
  if (s0 >= n) return;  // the whole workgroup
  const int len = (int)min((long long)SEG, n - s0);
  const uint8_t* __restrict__ src = streams + (long long)p * stream_stride + s0;
  uint8_t* __restrict__ dst = files + (long long)p * file_stride + head_bytes + 8 + s0;

  // tab[k][i]: the register after byte i and k zero bytes, from a zero start
  {
    uint32_t c = (uint32_t)tid;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      c = byte_step(c);
      tab[k][tid] = c;
    }
  }
  // the segment's bytes: staged byte k of the segment is byte lead + k of raw
  const int lead = (int)(reinterpret_cast<uintptr_t>(src) & 3u);
  for (int j = tid; 4 * j < lead + len; j += FT) {
    const int f = 4 * j - lead;  // the segment's byte in the dword's lowest byte
    uint32_t d = 0u;
    if (f >= 0 && f + 4 <= len) {
      d = *reinterpret_cast<const uint32_t*>(src + f);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (f + q >= 0 && f + q < len) d |= (uint32_t)src[f + q] << (8 * q);
    }
    raw[phys(j)] = d;
  }
  if (tid == 0) raw[phys((lead + len + 3) >> 2)] = 0u;  // lds_dword's second word behind the last byte
  __syncthreads();

  // to their place in the file: a thread owns an aligned dword of the destination
  const int shift = (int)(reinterpret_cast<uintptr_t>(dst) & 3u);
  for (int g = tid; 4 * g - shift < len; g += FT) {
    const int k0 = 4 * g - shift;
    if (k0 >= 0 && k0 + 4 <= len) {
      *reinterpret_cast<uint32_t*>(dst + k0) = lds_dword(raw, lead + k0);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = k0 + q;
        if (k >= 0 && k < len) dst[k] = (uint8_t)lds_byte(raw, lead + k);
      }
    }
  }

  // the lane's piece, laid from the segment's end: bytes a .. e-1, none if e <= 0
  const int e = (tid + 1) * PIECE - (SEG - len);
  const int a = max(0, e - PIECE);
  uint32_t c = 0u;
  if (e > 0) {
    int k = a;
    for (; k + 4 <= e; k += 4) {
      c ^= lds_dword(raw, lead + k);
      c = tab[3][c & 255u] ^ tab[2][(c >> 8) & 255u] ^ tab[1][(c >> 16) & 255u] ^ tab[0][c >> 24];
    }
    for (; k < e; ++k) c = (c >> 8) ^ tab[0][(c ^ lds_byte(raw, lead + k)) & 255u];
    c = mul(c, SHIFT.v[FT - 1 - tid]);
  }
  c = wg_xor(c, red);
  if (tid == 0) ws[(long long)p * nseg + seg] = c;
}

// Second launch: a workgroup per file.
__global__ void __launch_bounds__(FT) png_file_frame_kernel(const uint32_t* __restrict__ ws, const int* __restrict__ nbytes,
                                                            const uint8_t* __restrict__ head, uint8_t* __restrict__ files,
                                                            int* __restrict__ file_bytes, const int head_bytes, const long long stream_stride,
                                                            const long long file_stride, const int nseg) {
  __shared__ uint32_t pre[(TCE_PNG_FILE_MAX_HEAD + 8) / 4 + 1];
  __shared__ uint32_t red[FWAVES];
  const int tid = threadIdx.x, p = blockIdx.x;
  const int n = clamp_n(nbytes[p], stream_stride);
  const uint32_t* __restrict__ val = ws + (long long)p * nseg;
  uint8_t* __restrict__ row = files + (long long)p * file_stride;

  // head, BE32(n), "IDAT": through LDS, then a thread per aligned dword of the row
  uint8_t* preb = reinterpret_cast<uint8_t*>(pre);
  const int npre = head_bytes + 8;
  for (int i = tid; i < npre; i += FT) {
    const int k = i - head_bytes;
    preb[i] = k < 0 ? head[i] : k < 4 ? (uint8_t)((uint32_t)n >> (24 - 8 * k)) : (uint8_t)(0x54414449u >> (8 * (k - 4)));  // "IDAT"
  }

  // K and the F segments in front of the last one in use: V = F + 1 values a full segment apart, a contiguous run per thread
  const int F = n > 0 ? (n - 1) / SEG : 0;
  const int V = F + 1, per = (V + FT - 1) / FT;
  const int v0 = min(V, tid * per), v1 = min(V, v0 + per);
  uint32_t acc = 0u;
  for (int v = v0; v < v1; ++v) acc = mul(acc, XSEG) ^ (v == 0 ? KIDAT : val[v - 1]);
  if (v1 > v0) acc = mul(acc, power(XSEG, (unsigned long long)(V - v1)));
  acc = wg_xor(acc, red);  // (its barrier: pre is in)

  const int shift = (int)(reinterpret_cast<uintptr_t>(row) & 3u);
  for (int g = tid; 4 * g - shift < npre; g += FT) {
    const int k0 = 4 * g - shift;
    if (k0 >= 0 && k0 + 4 <= npre) {
      uint32_t d = 0u;
#pragma unroll
      for (int q = 0; q < 4; ++q) d |= (uint32_t)preb[k0 + q] << (8 * q);
      *reinterpret_cast<uint32_t*>(row + k0) = d;
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (k0 + q >= 0 && k0 + q < npre) row[k0 + q] = preb[k0 + q];
    }
  }

  if (tid < 16) {
    uint32_t crc = acc;
    if (n > 0) crc = mul(acc, power(X1, 8ull * (unsigned long long)(n - F * SEG))) ^ val[F];
    crc ^= 0xFFFFFFFFu;
    const uint32_t iend = tid < 8 ? 0x00000000u : tid < 12 ? 0x444E4549u : 0x826042AEu;  // 00 00 00 00 "IEND" AE 42 60 82, little-endian dwords
    const uint32_t b = tid < 4 ? crc >> (24 - 8 * tid) : iend >> (8 * (tid & 3));
    row[npre + n + tid] = (uint8_t)b;
    if (tid == 0) file_bytes[p] = head_bytes + 24 + n;
  }
}

int64_t file_bound(const int32_t head_bytes, const int64_t stream_stride) {
  if (head_bytes < TCE_PNG_FILE_MIN_HEAD || head_bytes > TCE_PNG_FILE_MAX_HEAD || stream_stride < 1 || stream_stride >= (1ll << 31))
    return -1;
  const int64_t b = (int64_t)head_bytes + 24 + stream_stride;
  return b < (1ll << 31) - 4096 ? b : -1;
}

bool disjoint(const void* a, const int64_t na, const void* b, const int64_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x + (uintptr_t)na <= y || y + (uintptr_t)nb <= x;
}

}  // namespace

extern "C" int64_t tce_png_file_bound(int32_t head_bytes, int64_t stream_stride) { return file_bound(head_bytes, stream_stride); }

extern "C" int64_t tce_png_file_ws_bytes(int32_t P, int64_t stream_stride) {
  if (P < 1 || P > 65535 || stream_stride < 1 || stream_stride >= (1ll << 31)) return -1;
  const int64_t nseg = (stream_stride + SEG - 1) / SEG;
  return ((int64_t)P * nseg * 4 + 7) & ~(int64_t)7;
}

extern "C" int tce_png_file_u8(const uint8_t* streams, const int32_t* nbytes, const uint8_t* head, int32_t head_bytes, uint8_t* files,
                               int32_t* file_bytes, void* ws, int32_t P, int64_t stream_stride, int64_t file_stride, tceStream stream) {
  TCE_CHECK_ARG(P >= 1 && P <= 65535, "tce_png_file_u8: P = %d outside 1 .. 65535", P);
  TCE_CHECK_ARG(head_bytes >= TCE_PNG_FILE_MIN_HEAD && head_bytes <= TCE_PNG_FILE_MAX_HEAD, "tce_png_file_u8: head_bytes = %d outside %d .. %d",
                head_bytes, TCE_PNG_FILE_MIN_HEAD, TCE_PNG_FILE_MAX_HEAD);
  const int64_t bound = file_bound(head_bytes, stream_stride);
  TCE_CHECK_ARG(bound > 0, "tce_png_file_u8: stream_stride must be at least 1 and head_bytes + 24 + stream_stride below 2^31 - 4096");
  TCE_CHECK_ARG(file_stride >= bound && file_stride < (1ll << 31) - 4096,
                "tce_png_file_u8: file_stride = %lld outside tce_png_file_bound = %lld .. 2^31 - 4096", (long long)file_stride, (long long)bound);
  TCE_CHECK_ARG(streams && nbytes && head && files && file_bytes && ws, "tce_png_file_u8: null pointer");
  TCE_CHECK_ARG(((uintptr_t)ws & 7u) == 0 && ((uintptr_t)nbytes & 3u) == 0 && ((uintptr_t)file_bytes & 3u) == 0,
                "tce_png_file_u8: ws must be 8-byte aligned, nbytes and file_bytes 4-byte aligned");
  const int64_t wsb = tce_png_file_ws_bytes(P, stream_stride), span = (int64_t)(P - 1) * file_stride + bound;
  TCE_CHECK_ARG(disjoint(files, span, streams, (int64_t)P * stream_stride) && disjoint(files, span, nbytes, 4ll * P) &&
                    disjoint(files, span, head, head_bytes) && disjoint(files, span, file_bytes, 4ll * P) && disjoint(files, span, ws, wsb),
                "tce_png_file_u8: files overlaps streams, nbytes, head, file_bytes or ws");
  const int nseg = (int)((stream_stride + SEG - 1) / SEG);
  hipLaunchKernelGGL(png_file_segment_kernel, dim3(nseg, P), dim3(FT), 0, (hipStream_t)stream, streams, nbytes, files, (uint32_t*)ws, head_bytes,
                     (long long)stream_stride, (long long)file_stride, nseg);
  hipLaunchKernelGGL(png_file_frame_kernel, dim3(P), dim3(FT), 0, (hipStream_t)stream, (const uint32_t*)ws, nbytes, head, files, file_bytes,
                     head_bytes, (long long)stream_stride, (long long)file_stride, nseg);
  TCE_CHECK_LAUNCH("tce_png_file_u8");
  return TCE_OK;
}
