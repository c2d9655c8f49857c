// Visualisation overlay (csrc/tce_rvos_vis.h, tce_vis_overlay_u8): the decoded frame with box outline, reference cross and mask
// tint of up to 16 layers, one pass over the pixels.  Memory-bound: 3 + L bytes read, 3 written per pixel.
#include "common.h"
#include "../../include/tce_rvos_vis.h"

namespace {

constexpr int VT = 256;

// what a layer draws on one frame, computed once per workgroup.  An empty rectangle has x1 < x0.
struct VisGeom {
  int bx0, by0, bx1, by1, ring;  // the box; ring = 1: only the pixels within 2 of a side
  int hx0, hx1, hy0, hy1;        // the cross's horizontal bar
  int vx0, vx1, vy0, vy1;        // its vertical bar
};

__device__ __forceinline__ int trunc_f(const float v) { return (int)fminf(fmaxf(v, -1073741824.f), 1073741824.f); }
__device__ __forceinline__ int trunc_d(const double v) { return (int)fmin(fmax(v, -1073741824.0), 1073741824.0); }

__device__ __forceinline__ VisGeom vis_geom(const float* __restrict__ box, const float* __restrict__ pt, const int H0, const int W0) {
#pragma clang fp contract(off)
  VisGeom g;
  g.bx0 = g.by0 = g.hx0 = g.hy0 = g.vx0 = g.vy0 = 0;
  g.bx1 = g.by1 = g.hx1 = g.hy1 = g.vx1 = g.vy1 = -1;
  g.ring = 0;
  if (box) {
    const float cx = box[0], cy = box[1], hw = 0.5f * box[2], hh = 0.5f * box[3];
    g.bx0 = trunc_f((cx - hw) * (float)W0);
    g.by0 = trunc_f((cy - hh) * (float)H0);
    g.bx1 = trunc_f((cx + hw) * (float)W0);
    g.by1 = trunc_f((cy + hh) * (float)H0);
    g.ring = (g.bx1 - g.bx0 >= 2 && g.by1 - g.by0 >= 2) ? 1 : 0;
    if (g.by1 < g.by0) g.bx1 = g.bx0 - 1;  // nothing: one test per pixel
  }
  if (pt) {
    const double x = (double)W0 * (double)pt[0], y = (double)H0 * (double)pt[1];
    const int tx = trunc_d(x), ty = trunc_d(y);
    g.hx0 = trunc_d(x - 10.0);
    g.hx1 = trunc_d(x + 10.0);
    g.hy0 = ty - 1;
    g.hy1 = ty + 2;
    g.vx0 = tx - 1;
    g.vx1 = tx + 2;
    g.vy0 = trunc_d(y - 10.0);
    g.vy1 = trunc_d(y + 10.0);
  }
  return g;
}

// 4 bytes at t[off .. off+3] of a tensor of `total` bytes at any address; bytes outside [0, total) read as 0.  The two aligned dwords
// that hold them where both lie inside the tensor, byte loads at its two ends.
__device__ __forceinline__ uint32_t load4(const uint8_t* __restrict__ t, const long long off, const long long total) {
  const int mis = (int)(reinterpret_cast<uintptr_t>(t + off) & 3u);
  const long long a0 = off - mis;
  if (a0 >= 0 && a0 + (mis ? 8 : 4) <= total) {
    const uint32_t* __restrict__ w = reinterpret_cast<const uint32_t*>(t + a0);
    uint32_t d = w[0];
    if (mis) d = (d >> (8 * mis)) | (w[1] << (32 - 8 * mis));
    return d;
  }
  uint32_t d = 0u;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (off + q >= 0 && off + q < total) d |= (uint32_t)t[off + q] << (8 * q);
  return d;
}

// grid (dwords of a frame / VT, N).  Thread g of frame n owns bytes p0 .. p0+3 of the frame, p0 = 4g - (address of the frame in out) mod 4.
__global__ void __launch_bounds__(VT) vis_overlay_kernel(const uint8_t* __restrict__ frames, uint8_t* __restrict__ out, const uint8_t* __restrict__ masks,
                                                         const float* __restrict__ boxes, const float* __restrict__ points,
                                                         const uint8_t* __restrict__ colors, const int L, const int H0, const int W0) {
  __shared__ VisGeom geom[TCE_VIS_MAX_LAYERS];
  __shared__ uint32_t col[TCE_VIS_MAX_LAYERS];
  const int n = blockIdx.y, N = gridDim.y;
  const int HW = H0 * W0, FB = HW * 3;
  if ((int)threadIdx.x < L) {
    const int l = threadIdx.x;
    const long long ln = (long long)l * N + n;
    geom[l] = vis_geom(boxes ? boxes + ln * 4 : nullptr, points ? points + ln * 2 : nullptr, H0, W0);
    col[l] = (uint32_t)colors[3 * l] | ((uint32_t)colors[3 * l + 1] << 8) | ((uint32_t)colors[3 * l + 2] << 16);
  }
  __syncthreads();
  uint8_t* __restrict__ fo = out + (long long)n * FB;
  const int shift = (int)(reinterpret_cast<uintptr_t>(fo) & 3u);
  const int p0 = (blockIdx.x * VT + threadIdx.x) * 4 - shift;  // (grid: 4 * threads < FB + 3 + 4 * VT: no overflow)
  if (p0 >= FB) return;
  const uint32_t src = load4(frames, (long long)n * FB + p0, (long long)N * FB);

  // pixel and channel of the first byte that exists, then a step per byte
  const int pf = max(p0, 0);
  int pix = pf / 3, ch = pf - 3 * pix;
  int y = pix / W0, x = pix - y * W0;
  uint32_t res = 0u;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int p = p0 + q;
    if (p < 0 || p >= FB) continue;
    uint32_t v = (src >> (8 * q)) & 255u;
    for (int l = 0; l < L; ++l) {
      const VisGeom& g = geom[l];
      const uint32_t c = (col[l] >> (8 * ch)) & 255u;
      if (x >= g.bx0 && x <= g.bx1 && y >= g.by0 && y <= g.by1 &&
          (!g.ring || x - g.bx0 < 2 || g.bx1 - x < 2 || y - g.by0 < 2 || g.by1 - y < 2))
        v = c;
      if ((x >= g.hx0 && x <= g.hx1 && y >= g.hy0 && y <= g.hy1) || (x >= g.vx0 && x <= g.vx1 && y >= g.vy0 && y <= g.vy1)) v = c;
      if (masks && masks[((long long)l * N + n) * HW + pix]) v = (v + c) >> 1;
    }
    res |= v << (8 * q);
    if (++ch == 3) {
      ch = 0;
      ++pix;
      if (++x == W0) {
        x = 0;
        ++y;
      }
    }
  }
  if (p0 >= 0 && p0 + 4 <= FB) {
    *reinterpret_cast<uint32_t*>(fo + p0) = res;
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (p0 + q >= 0 && p0 + q < FB) fo[p0 + q] = (uint8_t)(res >> (8 * q));
  }
}

}  // namespace

extern "C" int tce_vis_overlay_u8(const uint8_t* frames, uint8_t* out, const uint8_t* masks, const float* boxes, const float* points,
                                  const uint8_t* colors, int32_t L, int32_t N, int32_t H0, int32_t W0, tceStream stream) {
  TCE_CHECK_ARG(L >= 1 && L <= TCE_VIS_MAX_LAYERS, "tce_vis_overlay_u8: L = %d outside 1 .. %d", L, TCE_VIS_MAX_LAYERS);
  TCE_CHECK_ARG(N >= 1 && N <= 65535 && H0 >= 1 && W0 >= 1, "tce_vis_overlay_u8: N = %d outside 1 .. 65535 or a non-positive extent", N);
  TCE_CHECK_ARG((long long)H0 * W0 * 3 < (1ll << 31) - 4 * VT - 8, "tce_vis_overlay_u8: a frame must stay below 2^31 bytes");
  TCE_CHECK_ARG(frames && out && colors, "tce_vis_overlay_u8: null pointer");
  TCE_CHECK_ARG(((uintptr_t)boxes & 3u) == 0 && ((uintptr_t)points & 3u) == 0, "tce_vis_overlay_u8: boxes and points must be 4-byte aligned");
  const long long total = (long long)N * H0 * W0 * 3;
  TCE_CHECK_ARG(out + total <= frames || frames + total <= out, "tce_vis_overlay_u8: out must not overlap frames");
  const int fb = H0 * W0 * 3;
  hipLaunchKernelGGL(vis_overlay_kernel, dim3(tce_cdiv(tce_cdiv((long long)fb + 3, 4), VT), N), dim3(VT), 0, (hipStream_t)stream, frames,
                     out, masks, boxes, points, colors, L, H0, W0);
  TCE_CHECK_LAUNCH("tce_vis_overlay_u8");
  return TCE_OK;
}
