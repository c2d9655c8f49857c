// Driver-stage kernels (include/tce_rvos_video.h): the Ref-DAVIS label map of one chunk, all objects of an annotator combined.
#include "common.h"
#include "../../include/tce_rvos_video.h"

namespace {

// the host table, by value in the kernel arguments (as copy_segments_kernel takes its segments): 256 bytes, read with scalar loads
struct LabelObjs {
  const float* logits[TCE_LABEL_MAX_OBJS];
  const float* masks[TCE_LABEL_MAX_OBJS];
};

// inference_davis.py:239-243 per object: pred_scores = sigmoid(logits).mean(frames); max over classes; argmax over queries, first
// maximum wins.  One wavefront per object, a lane per query (strided); each (query, class) mean is summed over the frames in order,
// the same operations in the same order as harness_kernel, so the index is the one tce_select_masks_u8 reports.
__global__ void __launch_bounds__(64) label_best_kernel(const LabelObjs objs, int* __restrict__ best_out, const int T, const int Q,
                                                        const int K) {
  const float* __restrict__ logits = objs.logits[blockIdx.x];
  const int none = 0x7fffffff;
  float best = -1.f;
  int bq = none;
  for (int q = threadIdx.x; q < Q; q += 64) {
    float mx = -1.f;
    for (int k = 0; k < K; ++k) {
      float sum = 0.f;
      for (int t = 0; t < T; ++t) sum += 1.f / (1.f + expf(-logits[((long long)t * Q + q) * K + k]));
      mx = fmaxf(mx, sum / (float)T);
    }
    if (mx > best) {
      best = mx;
      bq = q;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oq = __shfl_xor(bq, o, 64);
    if (ob > best || (ob == best && oq < bq)) {
      best = ob;
      bq = oq;
    }
  }
  if (threadIdx.x == 0) best_out[blockIdx.x] = bq == none ? 0 : bq;  // nothing above -1 (NaN scores): query 0, as harness_kernel
}

// the four taps and two weights of one output pixel of F.interpolate(mode="bilinear", align_corners=False), as harness_kernel
struct LabelTap {
  int o00, o01, o10, o11;  // offsets into a [h,w] plane
  int tq;                  // t * Q: the pixel's frame, in planes
  float lx, ly;
};

__device__ __forceinline__ LabelTap label_tap(const int t, const int yo, const int xo, const int Q, const int h, const int w,
                                              const float sy, const float sx) {
  const float fy = fmaxf(sy * ((float)yo + 0.5f) - 0.5f, 0.f);
  const float fx = fmaxf(sx * ((float)xo + 0.5f) - 0.5f, 0.f);
  const int y0 = min((int)fy, h - 1), x0 = min((int)fx, w - 1);
  const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
  LabelTap p;
  p.o00 = y0 * w + x0;
  p.o01 = y0 * w + x1;
  p.o10 = y1 * w + x0;
  p.o11 = y1 * w + x1;
  p.tq = t * Q;
  p.ly = fy - (float)y0;
  p.lx = fx - (float)x0;
  return p;
}

// inference_davis.py:245-248 and :293-298 per output pixel.  A thread owns the four label bytes of one ALIGNED dword of the
// [T*H0*W0] plane taken as a flat byte string (thread g: bytes 4g - shift .. 4g - shift + 3, shift = the plane's address mod 4), so a
// row length such as 854 costs nothing: only the first and the last dword of the whole plane can be partial, and those go out
// byte by byte.  The objects are walked per pixel with a running maximum of the fp32 score; `>` keeps the first maximum, the
// background's 0.1 included.
__global__ void __launch_bounds__(256) label_pixels_kernel(const LabelObjs objs, const int* __restrict__ best,
                                                           uint8_t* __restrict__ labels, const int n, const int Q, const int h,
                                                           const int w, const int H0, const int W0, const int total,
                                                           const int shift, const float threshold, const float background) {
  const int p0 = (blockIdx.x * 256 + threadIdx.x) * 4 - shift;
  if (p0 >= total) return;
  const float sy = (float)h / (float)H0, sx = (float)w / (float)W0;
  // pixels outside [0, total) (head of the first dword, tail of the last) take the coordinates of the nearest real one: every
  // load stays inside the planes, and their bytes are not stored
  int c = min(max(p0, 0), total - 1);
  int xo = c % W0, r = c / W0;
  int yo = r % H0, t = r / H0;
  LabelTap tap[4];
  tap[0] = label_tap(t, yo, xo, Q, h, w, sy, sx);
#pragma unroll
  for (int j = 1; j < 4; ++j) {
    const int cj = min(max(p0 + j, 0), total - 1);
    if (cj != c) {  // one pixel on
      c = cj;
      if (++xo == W0) {
        xo = 0;
        if (++yo == H0) {
          yo = 0;
          ++t;
        }
      }
    }
    tap[j] = label_tap(t, yo, xo, Q, h, w, sy, sx);
  }
  float top[4] = {background, background, background, background};
  uint32_t lab[4] = {0u, 0u, 0u, 0u};
  const long long hw = (long long)h * w;
  for (int k = 0; k < n; ++k) {
    const int bq = best[k];
    const float* __restrict__ m = objs.masks[k];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float* __restrict__ mp = m + (long long)(tap[j].tq + bq) * hw;
      const float lx = tap[j].lx, ly = tap[j].ly, hx = 1.f - lx, hy = 1.f - ly;
      const float v = hy * (hx * mp[tap[j].o00] + lx * mp[tap[j].o01]) + ly * (hx * mp[tap[j].o10] + lx * mp[tap[j].o11]);
      float s = 1.f / (1.f + expf(-v));
      s = s < threshold ? 0.f : s;
      if (s > top[j]) {
        top[j] = s;
        lab[j] = (uint32_t)(k + 1);
      }
    }
  }
  if (p0 >= 0 && p0 + 4 <= total) {
    *reinterpret_cast<uint32_t*>(labels + p0) = lab[0] | (lab[1] << 8) | (lab[2] << 16) | (lab[3] << 24);
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (p0 + j >= 0 && p0 + j < total) labels[p0 + j] = (uint8_t)lab[j];
}

}  // namespace

extern "C" int tce_label_objects_u8(const tceLabelObj* objs, int32_t n, uint8_t* labels, int32_t* best_query, int32_t T,
                                    int32_t Q, int32_t K, int32_t h, int32_t w, int32_t H0, int32_t W0, float threshold,
                                    float background, tceStream stream) {
  TCE_CHECK_ARG(objs && n >= 1 && n <= TCE_LABEL_MAX_OBJS, "tce_label_objects_u8: 1..TCE_LABEL_MAX_OBJS objects");
  TCE_CHECK_ARG(labels && best_query && T > 0 && Q > 0 && K > 0 && h > 0 && w > 0 && H0 > 0 && W0 > 0,
                "tce_label_objects_u8: bad arguments (best_query is required)");
  const long long total = (long long)T * H0 * W0;
  TCE_CHECK_ARG(total < (1ll << 31) - 4096 && (long long)T * Q * h * w < (1ll << 31),
                "tce_label_objects_u8: the label map and each object's mask planes must stay below 2^31 elements");
  LabelObjs pack;
  for (int i = 0; i < TCE_LABEL_MAX_OBJS; ++i) {
    const tceLabelObj& o = objs[i < n ? i : 0];  // unused slots repeat object 0: never read, never a stray pointer
    TCE_CHECK_ARG(o.logits && o.masks, "tce_label_objects_u8: null object pointers");
    pack.logits[i] = o.logits;
    pack.masks[i] = o.masks;
  }
  const int shift = (int)((uintptr_t)labels & 3u);
  hipLaunchKernelGGL(label_best_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, pack, best_query, T, Q, K);
  hipLaunchKernelGGL(label_pixels_kernel, dim3(tce_cdiv(tce_cdiv(total + shift, 4), 256)), dim3(256), 0, (hipStream_t)stream,
                     pack, best_query, labels, n, Q, h, w, H0, W0, (int)total, shift, threshold, background);
  TCE_CHECK_LAUNCH("tce_label_objects_u8");
  return TCE_OK;
}
