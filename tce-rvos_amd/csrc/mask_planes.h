// What every output stage behind the forward pass shares (harness_kernel in misc.hip, label.hip, eval.hip): the mask-resampling
// rule, the best-query score, and the byte-quad rule of a flat uint8 output plane.  Each is written ONCE here, with its
// floating-point operation sequence fixed (no contraction left to the compiler), so the kernels that use it give the same bits by
// construction (tests/test_output_stage_gpu.py holds them to exact equality).
#pragma once
#include "common.h"

// ------------------------------------------------------------------------------------------------------------- resampling
// the four taps and two weights of output pixel (yo, xo) of F.interpolate(mode="bilinear", align_corners=False) from an [h,w] plane
// at scales (sy, sx) = (h / H0, w / W0); which plane (frame, query) is the caller's business
struct MaskTap {
  int o00, o01, o10, o11;  // offsets into the [h,w] plane
  float lx, ly;
};

__device__ __forceinline__ MaskTap mask_tap(const int yo, const int xo, const int h, const int w, const float sy, const float sx) {
#pragma clang fp contract(off)
  const float fy = fmaxf(__builtin_fmaf(sy, (float)yo + 0.5f, -0.5f), 0.f);
  const float fx = fmaxf(__builtin_fmaf(sx, (float)xo + 0.5f, -0.5f), 0.f);
  const int y0 = min((int)fy, h - 1), x0 = min((int)fx, w - 1);
  const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
  return {y0 * w + x0, y0 * w + x1, y1 * w + x0, y1 * w + x1, fx - (float)x0, fy - (float)y0};
}

// the blended logit: each row blend is one rounded product and one fma, the column blend two rounded products and an add
__device__ __forceinline__ float mask_tap_value(const float* __restrict__ plane, const MaskTap& p) {
#pragma clang fp contract(off)
  const float hx = 1.f - p.lx, hy = 1.f - p.ly;
  const float top = __builtin_fmaf(p.lx, plane[p.o01], hx * plane[p.o00]);
  const float bot = __builtin_fmaf(hx, plane[p.o10], p.lx * plane[p.o11]);
  return hy * top + p.ly * bot;
}

// (nothing in the sigmoid or in the score below is a product feeding a sum: there is nothing to contract)
__device__ __forceinline__ float mask_sigmoid(const float v) { return 1.f / (1.f + expf(-v)); }

// pred_scores = sigmoid(logits).mean(frames), max over classes, of query q of logits [T,Q,K]: each (query, class) mean is summed
// over the frames in order.  The callers take the arg-max over queries with `>` (the first maximum wins; -1 to start, so query 0
// when every score is NaN).
__device__ __forceinline__ float mask_query_score(const float* __restrict__ logits, const int q, const int T, const int Q, const int K) {
  float mx = -1.f;
  for (int k = 0; k < K; ++k) {
    float sum = 0.f;
    for (int t = 0; t < T; ++t) sum += mask_sigmoid(logits[((long long)t * Q + q) * K + k]);
    mx = fmaxf(mx, sum / (float)T);
  }
  return mx;
}

// -------------------------------------------------------------------------------------------------------------- byte quads
// A thread owns the four bytes of one ALIGNED dword of a [planes*H0*W0] uint8 output taken as a flat byte string that may start
// at any address: thread g has bytes p0 .. p0 + 3, p0 = 4g - shift, shift = the output's address mod 4.  A row length such as 854
// costs nothing: only the first and the last dword of the whole output can be partial, and those go out byte by byte.
constexpr int QUAD_THREADS = 256;

struct ByteQuadLaunch {
  int shift, blocks;
};
static inline ByteQuadLaunch byte_quad_launch(const void* out, const long long total) {
  const int shift = (int)((uintptr_t)out & 3u);
  return {shift, tce_cdiv(tce_cdiv(total + shift, 4), QUAD_THREADS)};
}

// p0 may be negative (first dword) and p0 + 3 may pass total (last dword); p0 >= total: the thread has nothing to do
__device__ __forceinline__ int byte_quad_p0(const int shift) { return (blockIdx.x * QUAD_THREADS + threadIdx.x) * 4 - shift; }

// (plane, y, x) of the four bytes: two divisions for the first, then a step per byte.  A byte outside [0, total) takes the
// coordinates of the nearest real one, so every load stays inside the planes; it is not stored.
struct QuadPixel {
  int plane, y, x;
};
__device__ __forceinline__ void byte_quad_pixels(const int p0, const int total, const int H0, const int W0, QuadPixel px[4]) {
  int c = min(max(p0, 0), total - 1);
  const int r = c / W0;
  px[0] = {r / H0, r % H0, c % W0};
#pragma unroll
  for (int j = 1; j < 4; ++j) {
    const int cj = min(max(p0 + j, 0), total - 1);
    px[j] = px[j - 1];
    if (cj != c && ++px[j].x == W0) {  // one pixel on
      px[j].x = 0;
      if (++px[j].y == H0) {
        px[j].y = 0;
        ++px[j].plane;
      }
    }
    c = cj;
  }
}

__device__ __forceinline__ void byte_quad_store(uint8_t* __restrict__ out, const int p0, const int total, const uint32_t b[4]) {
  if (p0 >= 0 && p0 + 4 <= total) {
    *reinterpret_cast<uint32_t*>(out + p0) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (p0 + j >= 0 && p0 + j < total) out[p0 + j] = (uint8_t)b[j];
}

// ------------------------------------------------------------------------------------------------------- dataset-size bits
// The four bits of a byte quad of a dataset-size output [planes,H0,W0] (the group kernels of a2d_group.hip and refexp.hip): per
// byte the nearest source pixel (ONE fp32 multiply, as ATen) of the (fh, fw) crop of the x4 bilinear plane, its blended logit,
// sigmoid > threshold -- a2d_masks_kernel's operation sequence (eval.hip).  plane_of(n) = the [h,w] plane behind output plane n.
template <class PlaneOf>
__device__ __forceinline__ void mask_quad_bits(const QuadPixel px[4], const int h, const int w, const int fh, const int fw, const int H0,
                                               const int W0, const float threshold, PlaneOf plane_of, uint32_t bit[4]) {
  const float sy = (float)fh / (float)H0, sx = (float)fw / (float)W0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ys = min((int)floorf((float)px[j].y * sy), fh - 1), xs = min((int)floorf((float)px[j].x * sx), fw - 1);
    const float v = mask_tap_value(plane_of(px[j].plane), mask_tap(ys, xs, h, w, 0.25f, 0.25f));
    bit[j] = mask_sigmoid(v) > threshold ? 1u : 0u;
  }
}
