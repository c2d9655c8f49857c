// A2D-Sentences / JHMDB-Sentences scoring-stage kernels (csrc/tce_rvos_a2d_score.h): run lengths back to planes, and the overlap
// counts of N prediction planes against one ground-truth plane.  Byte kernels, bound by memory latency at dataset sizes.
#include "common.h"
#include "mask_planes.h"
#include "../../include/tce_rvos_score.h"

namespace {

// ------------------------------------------------------------------------------------------------------------ run lengths
constexpr int DEC_THREADS = 256, DEC_PER = 4, DEC_WAVES = DEC_THREADS / 64;  // a thread owns DEC_PER consecutive counts of its segment
static_assert(DEC_THREADS * DEC_PER == TCE_RLE_SEGMENT, "segment length");

// a + b held at cap.  a, b <= cap < 2^31, so the sum fits 32 bits; min(. , cap) of sums of non-negative numbers is associative, so
// every partial sum below may be held at cap = H*W: e_i = min(c_0 + .. + c_i, H*W) comes out exactly, with no 64-bit arithmetic.
__device__ __forceinline__ uint32_t sat_add(const uint32_t a, const uint32_t b, const uint32_t cap) { return min(a + b, cap); }

// the number of counts of mask p in use
__device__ __forceinline__ int rle_used(const int* __restrict__ nruns, const int p, const int stride) {
  return min(max(nruns[p], 0), stride);
}

// the running sums (held at cap) of the thread's DEC_PER counts i0 .. i0+3 of a row; a count at or behind m is 0
__device__ __forceinline__ void dec_running(const uint32_t* __restrict__ row, const long long i0, const int m, const uint32_t cap,
                                            uint32_t l[DEC_PER]) {
  uint32_t run = 0u;
#pragma unroll
  for (int j = 0; j < DEC_PER; ++j) {
    if (i0 + j < m) run = sat_add(run, min(row[i0 + j], cap), cap);
    l[j] = run;
  }
}

// the sum (held at cap) of v over the workgroup, returned to every thread (red: DEC_WAVES words of LDS; may be reused after the call)
__device__ __forceinline__ uint32_t dec_block_sum(uint32_t v, uint32_t* red, const uint32_t cap) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = sat_add(v, (uint32_t)__shfl_xor((int)v, o, 64), cap);
  __syncthreads();  // earlier readers of red are done
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return sat_add(sat_add(red[0], red[1], cap), sat_add(red[2], red[3], cap), cap);
}

// first launch: the sum of every segment that holds a count in use (the others are never read)
__global__ void __launch_bounds__(DEC_THREADS) rle_segment_sum_kernel(const uint32_t* __restrict__ counts, const int* __restrict__ nruns,
                                                                      uint32_t* __restrict__ seg_sum, const int HW, const int stride,
                                                                      const int nseg) {
  __shared__ uint32_t red[DEC_WAVES];
  const int p = blockIdx.y, seg = blockIdx.x, m = rle_used(nruns, p, stride);
  if ((long long)seg * TCE_RLE_SEGMENT >= m) return;  // the whole workgroup
  uint32_t l[DEC_PER];
  dec_running(counts + (long long)p * stride, (long long)seg * TCE_RLE_SEGMENT + threadIdx.x * DEC_PER, m, (uint32_t)HW, l);
  const uint32_t s = dec_block_sum(l[DEC_PER - 1], red, (uint32_t)HW);
  if (threadIdx.x == 0) seg_sum[(long long)p * nseg + seg] = s;
}

// second launch: e_i of every count in use = the sums of the segments before its own + the scan of its own segment
__global__ void __launch_bounds__(DEC_THREADS) rle_prefix_kernel(const uint32_t* __restrict__ counts, const int* __restrict__ nruns,
                                                                 const uint32_t* __restrict__ seg_sum, uint32_t* __restrict__ ends,
                                                                 const int HW, const int stride, const int nseg) {
  __shared__ uint32_t red[2 * DEC_WAVES];
  const int p = blockIdx.y, seg = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = rle_used(nruns, p, stride);
  if ((long long)seg * TCE_RLE_SEGMENT >= m) return;
  const uint32_t cap = (uint32_t)HW;
  uint32_t before = 0u;
  for (int s = tid; s < seg; s += DEC_THREADS) before = sat_add(before, seg_sum[(long long)p * nseg + s], cap);
  before = dec_block_sum(before, red, cap);

  const long long i0 = (long long)seg * TCE_RLE_SEGMENT + tid * DEC_PER;
  uint32_t l[DEC_PER];
  dec_running(counts + (long long)p * stride, i0, m, cap, l);
  uint32_t sc = l[DEC_PER - 1];  // inclusive scan over the wavefront
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t a = (uint32_t)__shfl_up((int)sc, o, 64);
    if (lane >= o) sc = sat_add(sc, a, cap);
  }
  uint32_t ex = (uint32_t)__shfl_up((int)sc, 1, 64);
  if (lane == 0) ex = 0u;
  if (lane == 63) red[DEC_WAVES + wave] = sc;  // (dec_block_sum used red[0 .. DEC_WAVES) only)
  __syncthreads();
  uint32_t base = before;
  for (int k = 0; k < wave; ++k) base = sat_add(base, red[DEC_WAVES + k], cap);
  base = sat_add(base, ex, cap);
  uint32_t* __restrict__ row = ends + (long long)p * stride;
#pragma unroll
  for (int j = 0; j < DEC_PER; ++j)
    if (i0 + j < m) row[i0 + j] = sat_add(base, l[j], cap);
}

// third launch, pixel-stationary: a thread owns one aligned dword of plane p of out (mask_planes.h; the plane starts at any
// address, so the shift is the plane's own).  Byte r = y*W + x of the plane is position q = x*H + y of the column-major walk; its
// run is the number of e_i <= q, found by bisection over e_0 .. e_{m-1} (non-decreasing), the four positions in step.
__global__ void __launch_bounds__(QUAD_THREADS) rle_decode_kernel(const uint32_t* __restrict__ ends, const int* __restrict__ nruns,
                                                                  uint8_t* __restrict__ out, const int H, const int W, const int HW,
                                                                  const int stride) {
  const int p = blockIdx.y;
  uint8_t* __restrict__ plane = out + (long long)p * HW;
  const int p0 = byte_quad_p0((int)(reinterpret_cast<uintptr_t>(plane) & 3u));
  if (p0 >= HW) return;
  const uint32_t m = (uint32_t)rle_used(nruns, p, stride);
  const uint32_t* __restrict__ e = ends + (long long)p * stride;
  QuadPixel px[4];
  byte_quad_pixels(p0, HW, H, W, px);  // one plane: px[j].plane = 0
  uint32_t q[4], lo[4], hi[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    q[j] = (uint32_t)(px[j].x * H + px[j].y);
    lo[j] = 0u;
    hi[j] = m;
  }
  const int steps = m ? 32 - __clz(m) : 0;  // a range of m candidates + "none" halves to one in bit-length(m) steps
  for (int it = 0; it < steps; ++it) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (lo[j] < hi[j]) {
        const uint32_t mid = (lo[j] + hi[j]) >> 1;  // < m <= stride: inside the row; lo + hi < 2^32
        if (e[mid] <= q[j]) lo[j] = mid + 1u;
        else hi[j] = mid;
      }
    }
  }
  uint32_t bit[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) bit[j] = lo[j] < m ? (lo[j] & 1u) : 0u;
  byte_quad_store(plane, p0, HW, bit);
}

bool plane_ok(const int H, const int W) { return H > 0 && W > 0 && (long long)H * W < (1ll << 31) - 4096; }

// ------------------------------------------------------------------------------------------------------------ overlap counts
constexpr int OV_THREADS = 256, OV_WAVES = OV_THREADS / 64;

// bytes f .. f+3 of a plane of HW bytes at b, (b + f) on a 4-byte boundary: one dword where all four are inside the plane, byte by
// byte (0 for those outside) at the plane's two ends
__device__ __forceinline__ uint32_t plane_dword(const uint8_t* __restrict__ b, const int f, const int HW) {
  if (f >= 0 && f + 4 <= HW) return *reinterpret_cast<const uint32_t*>(b + f);
  uint32_t d = 0u;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (f + q >= 0 && f + q < HW) d |= (uint32_t)b[f + q] << (8 * q);
  return d;
}

// A workgroup owns bytes t0 .. t0+len-1 of the plane.  Its piece of gt goes into LDS as 0/1 bytes, once; then every prediction's
// piece is fetched as the aligned dwords that hold it (the planes sit at any address and H*W is any number, so the alignment is
// each plane's own) and counted against it.  ws: part [N][tiles][2] = (intersection, prediction area), then gsum [tiles].
__global__ void __launch_bounds__(OV_THREADS) overlap_tile_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt,
                                                                  int* __restrict__ ws, const int N, const int HW, const int tiles) {
  __shared__ uint8_t g[TCE_OVERLAP_TILE];
  __shared__ uint32_t red[2][OV_WAVES];
  const int tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t0 = tile * TCE_OVERLAP_TILE, len = min(TCE_OVERLAP_TILE, HW - t0);
  {
    const int lead = (int)((reinterpret_cast<uintptr_t>(gt) + (uintptr_t)t0) & 3u);
    uint32_t cnt = 0u;
    for (int j = tid; 4 * j < lead + len; j += OV_THREADS) {
      const int k0 = 4 * j - lead;
      const uint32_t d = plane_dword(gt, t0 + k0, HW);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = k0 + q;
        if (k >= 0 && k < len) {
          const uint32_t b = ((d >> (8 * q)) & 0xFFu) != 0u;
          g[k] = (uint8_t)b;
          cnt += b;
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += (uint32_t)__shfl_xor((int)cnt, o, 64);
    if (lane == 0) red[1][wave] = cnt;
    __syncthreads();  // ... and g is complete
    if (tid == 0) ws[(long long)N * tiles * 2 + tile] = (int)(red[1][0] + red[1][1] + red[1][2] + red[1][3]);
  }
  for (int n = 0; n < N; ++n) {
    const uint8_t* __restrict__ pl = pred + (long long)n * HW;
    const int lead = (int)((reinterpret_cast<uintptr_t>(pl) + (uintptr_t)t0) & 3u);
    uint32_t acc = 0u;  // intersection | area << 16: a tile's sums are at most TCE_OVERLAP_TILE
    for (int j = tid; 4 * j < lead + len; j += OV_THREADS) {
      const int k0 = 4 * j - lead;
      const uint32_t d = plane_dword(pl, t0 + k0, HW);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = k0 + q;
        if (k >= 0 && k < len) {
          const uint32_t b = ((d >> (8 * q)) & 0xFFu) != 0u;
          acc += (b & g[k]) | (b << 16);
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += (uint32_t)__shfl_xor((int)acc, o, 64);
    // red[n & 1]: its readers of two rounds ago passed the barrier of the round before this one
    if (lane == 0) red[n & 1][wave] = acc;
    __syncthreads();
    if (tid == 0) {
      const uint32_t s = red[n & 1][0] + red[n & 1][1] + red[n & 1][2] + red[n & 1][3];
      int* __restrict__ dst = ws + ((long long)n * tiles + tile) * 2;
      dst[0] = (int)(s & 0xFFFFu);
      dst[1] = (int)(s >> 16);
    }
  }
}
static_assert(TCE_OVERLAP_TILE < (1 << 16), "two sums of a tile share a word");

// counts[n,:] = the sums of the tiles' partial sums: a wavefront per prediction
__global__ void __launch_bounds__(64) overlap_reduce_kernel(const int* __restrict__ ws, int* __restrict__ counts, const int N,
                                                            const int tiles) {
  const int n = blockIdx.x;
  const int* __restrict__ part = ws + (long long)n * tiles * 2;
  const int* __restrict__ gsum = ws + (long long)N * tiles * 2;
  int a0 = 0, a1 = 0, a2 = 0;
  for (int i = threadIdx.x; i < tiles; i += 64) {
    a0 += part[2 * (long long)i];
    a1 += part[2 * (long long)i + 1];
    a2 += gsum[i];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a0 += __shfl_xor(a0, o, 64);
    a1 += __shfl_xor(a1, o, 64);
    a2 += __shfl_xor(a2, o, 64);
  }
  if (threadIdx.x == 0) {
    counts[3 * (long long)n] = a0;
    counts[3 * (long long)n + 1] = a1;
    counts[3 * (long long)n + 2] = a2;
  }
}

}  // namespace

extern "C" int64_t tce_rle_decode_ws_bytes(int32_t P, int32_t H, int32_t W, int32_t stride) {
  if (P <= 0 || P > 65535 || stride <= 0 || !plane_ok(H, W)) return -1;
  const int64_t words = (int64_t)P * stride + (int64_t)P * tce_cdiv(stride, TCE_RLE_SEGMENT);  // every e_i, then the segment sums
  return (words * 4 + 7) & ~(int64_t)7;
}

extern "C" int tce_rle_decode_u8(const uint32_t* counts, const int32_t* nruns, uint8_t* out, void* ws, int32_t P, int32_t H,
                                 int32_t W, int32_t stride, tceStream stream) {
  TCE_CHECK_ARG(counts && nruns && out && ws, "tce_rle_decode_u8: null pointer");
  TCE_CHECK_ARG(P > 0 && H > 0 && W > 0 && stride > 0, "tce_rle_decode_u8: non-positive extent");
  TCE_CHECK_ARG(plane_ok(H, W) && P <= 65535, "tce_rle_decode_u8: a mask must stay below 2^31 - 4096 elements and P at or below 65535");
  TCE_CHECK_ARG(((uintptr_t)ws & 7u) == 0 && ((uintptr_t)counts & 3u) == 0 && ((uintptr_t)nruns & 3u) == 0,
                "tce_rle_decode_u8: ws must be 8-byte aligned, counts and nruns 4-byte aligned");
  const int HW = H * W, nseg = tce_cdiv(stride, TCE_RLE_SEGMENT);
  uint32_t* ends = (uint32_t*)ws;
  uint32_t* seg_sum = ends + (long long)P * stride;
  hipLaunchKernelGGL(rle_segment_sum_kernel, dim3(nseg, P), dim3(DEC_THREADS), 0, (hipStream_t)stream, counts, nruns, seg_sum, HW, stride,
                     nseg);
  hipLaunchKernelGGL(rle_prefix_kernel, dim3(nseg, P), dim3(DEC_THREADS), 0, (hipStream_t)stream, counts, nruns,
                     (const uint32_t*)seg_sum, ends, HW, stride, nseg);
  // a plane's shift is at most 3: HW + 3 bytes cover every dword that holds one of its bytes
  hipLaunchKernelGGL(rle_decode_kernel, dim3(tce_cdiv(tce_cdiv((long long)HW + 3, 4), QUAD_THREADS), P), dim3(QUAD_THREADS), 0,
                     (hipStream_t)stream, (const uint32_t*)ends, nruns, out, H, W, HW, stride);
  TCE_CHECK_LAUNCH("tce_rle_decode_u8");
  return TCE_OK;
}

extern "C" int64_t tce_mask_overlap_ws_bytes(int32_t N, int32_t H, int32_t W) {
  if (N <= 0 || N > 65535 || !plane_ok(H, W)) return -1;
  const int64_t tiles = tce_cdiv((long long)H * W, TCE_OVERLAP_TILE);
  return (((int64_t)N * tiles * 2 + tiles) * 4 + 7) & ~(int64_t)7;
}

extern "C" int tce_mask_overlap_i32(const uint8_t* pred, const uint8_t* gt, int32_t* counts, void* ws, int32_t N, int32_t H, int32_t W,
                                    tceStream stream) {
  TCE_CHECK_ARG(pred && gt && counts && ws, "tce_mask_overlap_i32: null pointer");
  TCE_CHECK_ARG(N > 0 && H > 0 && W > 0, "tce_mask_overlap_i32: non-positive extent");
  TCE_CHECK_ARG(plane_ok(H, W) && N <= 65535, "tce_mask_overlap_i32: a plane must stay below 2^31 - 4096 elements and N at or below 65535");
  TCE_CHECK_ARG(((uintptr_t)ws & 7u) == 0 && ((uintptr_t)counts & 3u) == 0,
                "tce_mask_overlap_i32: ws must be 8-byte aligned, counts 4-byte aligned");
  const int HW = H * W, tiles = tce_cdiv(HW, TCE_OVERLAP_TILE);
  hipLaunchKernelGGL(overlap_tile_kernel, dim3(tiles), dim3(OV_THREADS), 0, (hipStream_t)stream, pred, gt, (int*)ws, N, HW, tiles);
  hipLaunchKernelGGL(overlap_reduce_kernel, dim3(N), dim3(64), 0, (hipStream_t)stream, (const int*)ws, counts, N, tiles);
  TCE_CHECK_LAUNCH("tce_mask_overlap_i32");
  return TCE_OK;
}
