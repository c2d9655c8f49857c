// Evaluation-stage kernels (include/tce_rvos_eval.h): the A2D-Sentences / JHMDB-Sentences post-processor's dataset-size masks and
// their uncompressed COCO run lengths.
#include "common.h"
#include "mask_planes.h"
#include "../../include/tce_rvos_eval.h"

namespace {

// postprocessors.py:39-47 per output pixel, a byte quad of the [N*H0*W0] output per thread (mask_planes.h).  The nearest source
// index is ATen's (one fp32 multiply, floorf, clamp); the value there is the resampling rule's at scale 0.25 (weights are multiples
// of 1/8).
__global__ void __launch_bounds__(QUAD_THREADS) a2d_masks_kernel(const float* __restrict__ masks, uint8_t* __restrict__ out, const int h,
                                                                 const int w, const int fh, const int fw, const int H0, const int W0,
                                                                 const int total, const int shift, const float threshold) {
  const int p0 = byte_quad_p0(shift);
  if (p0 >= total) return;
  const float sy = (float)fh / (float)H0, sx = (float)fw / (float)W0;
  QuadPixel px[4];
  byte_quad_pixels(p0, total, H0, W0, px);
  uint32_t bit[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ys = min((int)floorf((float)px[j].y * sy), fh - 1), xs = min((int)floorf((float)px[j].x * sx), fw - 1);
    const float v = mask_tap_value(masks + (long long)px[j].plane * h * w, mask_tap(ys, xs, h, w, 0.25f, 0.25f));
    bit[j] = mask_sigmoid(v) > threshold ? 1u : 0u;
  }
  byte_quad_store(out, p0, total, bit);
}

// ---------------------------------------------------------------------------------------------------------------- run lengths
constexpr int RLE_THREADS = 256, RLE_PER = 4;  // a thread owns RLE_PER consecutive positions of its segment
static_assert(RLE_THREADS * RLE_PER == TCE_RLE_SEGMENT, "segment length");

// Boundary flags of positions p0 .. p0+3 of the column-major walk (p = x*H + y) over a row-major [H,W] mask: bit j set where
// bit(p0+j) != bit(p0+j-1), bit(-1) = 0.  Positions >= HW have no flag.
__device__ __forceinline__ uint32_t rle_flags(const uint8_t* __restrict__ m, const int p0, const int H, const int W, const int HW) {
  if (p0 >= HW) return 0u;
  int x = p0 / H, y = p0 - x * H;
  uint32_t prev = 0u;
  if (p0 > 0) prev = (y > 0 ? m[(y - 1) * W + x] : m[(H - 1) * W + x - 1]) != 0;
  uint32_t f = 0u;
#pragma unroll
  for (int j = 0; j < RLE_PER; ++j) {
    if (p0 + j < HW) {
      const uint32_t cur = m[y * W + x] != 0;
      f |= (cur ^ prev) << j;
      prev = cur;
      if (++y == H) {
        y = 0;
        ++x;
      }
    }
  }
  return f;
}

// sum of a, maximum of b over the workgroup, returned to every thread (red: 2 * 4 ints of LDS; may be reused after the call)
__device__ __forceinline__ void rle_block_sum_max(int& a, int& b, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o, 64);
    b = max(b, __shfl_xor(b, o, 64));
  }
  const int wave = threadIdx.x >> 6;
  __syncthreads();  // earlier readers of red are done
  if ((threadIdx.x & 63) == 0) {
    red[wave] = a;
    red[4 + wave] = b;
  }
  __syncthreads();
  a = red[0] + red[1] + red[2] + red[3];
  b = max(max(red[4], red[5]), max(red[6], red[7]));
}

// first launch: the record of every segment = (number of boundaries, position of the last one or -1)
__global__ void __launch_bounds__(RLE_THREADS) rle_count_kernel(const uint8_t* __restrict__ masks, int2* __restrict__ ws, const int H,
                                                                const int W, const int HW, const int nseg) {
  __shared__ int red[8];
  const uint8_t* __restrict__ m = masks + (long long)blockIdx.y * HW;
  const int p0 = blockIdx.x * TCE_RLE_SEGMENT + threadIdx.x * RLE_PER;
  const uint32_t f = rle_flags(m, p0, H, W, HW);
  int cnt = __popc(f), last = f ? p0 + 31 - __clz(f) : -1;
  rle_block_sum_max(cnt, last, red);
  if (threadIdx.x == 0) ws[(long long)blockIdx.y * nseg + blockIdx.x] = make_int2(cnt, last);
}

// second launch: a segment finds its place from the records of its mask (boundaries before it, the last boundary before it, the
// mask's total m and its last boundary), scans its own flags and writes one word per position: a boundary of rank r writes
// counts[r] = its distance to the boundary before it (to 0 for r = 0); the k-th position that is no boundary writes the zero at
// counts[m + 1 + k].  The last segment adds counts[m] = H*W - (last boundary) and nruns.
__global__ void __launch_bounds__(RLE_THREADS) rle_place_kernel(const uint8_t* __restrict__ masks, uint32_t* __restrict__ counts,
                                                                int* __restrict__ nruns, const int2* __restrict__ ws, const int H,
                                                                const int W, const int HW, const int nseg) {
  __shared__ int red[8];
  const int seg = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int2* __restrict__ rec = ws + (long long)blockIdx.y * nseg;
  int before = 0, total = 0, prev_last = -1, all_last = -1;
  for (int s = tid; s < nseg; s += RLE_THREADS) {
    const int2 r = rec[s];
    total += r.x;
    all_last = max(all_last, r.y);
    if (s < seg) {
      before += r.x;
      prev_last = max(prev_last, r.y);
    }
  }
  rle_block_sum_max(total, all_last, red);
  rle_block_sum_max(before, prev_last, red);

  const uint8_t* __restrict__ m = masks + (long long)blockIdx.y * HW;
  const int p0 = seg * TCE_RLE_SEGMENT + tid * RLE_PER;
  const uint32_t f = rle_flags(m, p0, H, W, HW);
  const int cnt = __popc(f), last = f ? p0 + 31 - __clz(f) : -1;
  int sc = cnt, ml = last;  // inclusive scans over the wavefront
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int a = __shfl_up(sc, o, 64), b = __shfl_up(ml, o, 64);
    if (lane >= o) {
      sc += a;
      ml = max(ml, b);
    }
  }
  int ex_l = __shfl_up(ml, 1, 64);
  if (lane == 0) ex_l = -1;
  __syncthreads();
  if (lane == 63) {
    red[wave] = sc;
    red[4 + wave] = ml;
  }
  __syncthreads();
  int rank = before + sc - cnt, prev = max(prev_last, ex_l);
  for (int k = 0; k < wave; ++k) {
    rank += red[k];
    prev = max(prev, red[4 + k]);
  }
  prev = max(prev, 0);  // no boundary yet: the first count is measured from position 0

  uint32_t* __restrict__ row = counts + (long long)blockIdx.y * ((long long)HW + 1);
#pragma unroll
  for (int j = 0; j < RLE_PER; ++j) {
    const int p = p0 + j;
    if (p < HW) {
      if ((f >> j) & 1u) {
        row[rank] = (uint32_t)(p - prev);
        prev = p;
        ++rank;
      } else {
        row[total + 1 + (p - rank)] = 0u;
      }
    }
  }
  if (seg == nseg - 1 && tid == 0) {
    row[total] = (uint32_t)(HW - max(all_last, 0));
    nruns[blockIdx.y] = total + 1;
  }
}

}  // namespace

extern "C" int tce_a2d_masks_u8(const float* masks, uint8_t* out, int32_t N, int32_t h, int32_t w, int32_t fh, int32_t fw,
                                int32_t H0, int32_t W0, float threshold, tceStream stream) {
  TCE_CHECK_ARG(masks && out, "tce_a2d_masks_u8: null pointer");
  TCE_CHECK_ARG(N > 0 && h > 0 && w > 0 && fh > 0 && fw > 0 && H0 > 0 && W0 > 0, "tce_a2d_masks_u8: non-positive extent");
  TCE_CHECK_ARG((long long)fh <= 4ll * h && (long long)fw <= 4ll * w,
                "tce_a2d_masks_u8: the un-padded size (%d, %d) exceeds 4x the mask plane (%d, %d)", fh, fw, h, w);
  const long long total = (long long)N * H0 * W0;
  TCE_CHECK_ARG(total < (1ll << 31) - 4096 && (long long)N * h * w < (1ll << 31),
                "tce_a2d_masks_u8: the output and the mask planes must stay below 2^31 elements");
  const ByteQuadLaunch ql = byte_quad_launch(out, total);
  hipLaunchKernelGGL(a2d_masks_kernel, dim3(ql.blocks), dim3(QUAD_THREADS), 0, (hipStream_t)stream, masks, out, h, w, fh, fw, H0, W0,
                     (int)total, ql.shift, threshold);
  TCE_CHECK_LAUNCH("tce_a2d_masks_u8");
  return TCE_OK;
}

extern "C" int64_t tce_rle_ws_bytes(int32_t P, int32_t H, int32_t W) {
  if (P <= 0 || H <= 0 || W <= 0 || (long long)H * W >= (1ll << 31) - TCE_RLE_SEGMENT) return -1;
  return (int64_t)P * tce_cdiv((long long)H * W, TCE_RLE_SEGMENT) * (int64_t)sizeof(int2);
}

extern "C" int tce_rle_counts_u32(const uint8_t* masks, uint32_t* counts, int32_t* nruns, void* ws, int32_t P, int32_t H, int32_t W,
                                  tceStream stream) {
  TCE_CHECK_ARG(masks && counts && nruns && ws, "tce_rle_counts_u32: null pointer");
  TCE_CHECK_ARG(P > 0 && H > 0 && W > 0, "tce_rle_counts_u32: non-positive extent");
  TCE_CHECK_ARG((long long)H * W < (1ll << 31) - TCE_RLE_SEGMENT && P <= 65535,
                "tce_rle_counts_u32: a mask must stay below 2^31 elements and P at or below 65535");
  TCE_CHECK_ARG(((uintptr_t)ws & 7u) == 0 && ((uintptr_t)counts & 3u) == 0 && ((uintptr_t)nruns & 3u) == 0,
                "tce_rle_counts_u32: ws must be 8-byte aligned, counts and nruns 4-byte aligned");
  const int HW = H * W, nseg = tce_cdiv(HW, TCE_RLE_SEGMENT);
  hipLaunchKernelGGL(rle_count_kernel, dim3(nseg, P), dim3(RLE_THREADS), 0, (hipStream_t)stream, masks, (int2*)ws, H, W, HW, nseg);
  hipLaunchKernelGGL(rle_place_kernel, dim3(nseg, P), dim3(RLE_THREADS), 0, (hipStream_t)stream, masks, counts, nruns,
                     (const int2*)ws, H, W, HW, nseg);
  TCE_CHECK_LAUNCH("tce_rle_counts_u32");
  return TCE_OK;
}
