// Driver-stage kernels (include/tce_rvos_video.h): the Ref-DAVIS label map of one chunk, all objects of an annotator combined.
#include "common.h"
#include "mask_planes.h"
#include "../../include/tce_rvos_video.h"

namespace {

// the host table, by value in the kernel arguments (as copy_segments_kernel takes its segments): 256 bytes, read with scalar loads
struct LabelObjs {
  const float* logits[TCE_LABEL_MAX_OBJS];
  const float* masks[TCE_LABEL_MAX_OBJS];
};

// inference_davis.py:239-243 per object: the arg-max over queries of mask_query_score, first maximum wins.  One wavefront per
// object, a lane per query (strided); the score is the function harness_kernel calls, so the index is the one tce_select_masks_u8 reports.
__global__ void __launch_bounds__(64) label_best_kernel(const LabelObjs objs, int* __restrict__ best_out, const int T, const int Q,
                                                        const int K) {
  const float* __restrict__ logits = objs.logits[blockIdx.x];
  const int none = 0x7fffffff;
  float best = -1.f;
  int bq = none;
  for (int q = threadIdx.x; q < Q; q += 64) {
    const float s = mask_query_score(logits, q, T, Q, K);
    if (s > best) {
      best = s;
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

// inference_davis.py:245-248 and :293-298 per output pixel, a byte quad of the [T*H0*W0] label map per thread (mask_planes.h).
// The objects are walked per pixel with a running maximum of the fp32 score; `>` keeps the first maximum, the background's 0.1
// included.
__global__ void __launch_bounds__(QUAD_THREADS) label_pixels_kernel(const LabelObjs objs, const int* __restrict__ best,
                                                                    uint8_t* __restrict__ labels, const int n, const int Q, const int h,
                                                                    const int w, const int H0, const int W0, const int total,
                                                                    const int shift, const float threshold, const float background) {
  const int p0 = byte_quad_p0(shift);
  if (p0 >= total) return;
  const float sy = (float)h / (float)H0, sx = (float)w / (float)W0;
  QuadPixel px[4];
  byte_quad_pixels(p0, total, H0, W0, px);
  MaskTap tap[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) tap[j] = mask_tap(px[j].y, px[j].x, h, w, sy, sx);
  float top[4] = {background, background, background, background};
  uint32_t lab[4] = {0u, 0u, 0u, 0u};
  const long long hw = (long long)h * w;
  for (int k = 0; k < n; ++k) {
    const int bq = best[k];
    const float* __restrict__ m = objs.masks[k];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float s = mask_sigmoid(mask_tap_value(m + (long long)(px[j].plane * Q + bq) * hw, tap[j]));
      s = s < threshold ? 0.f : s;
      if (s > top[j]) {
        top[j] = s;
        lab[j] = (uint32_t)(k + 1);
      }
    }
  }
  byte_quad_store(labels, p0, total, lab);
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
  const ByteQuadLaunch ql = byte_quad_launch(labels, total);
  hipLaunchKernelGGL(label_best_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, pack, best_query, T, Q, K);
  hipLaunchKernelGGL(label_pixels_kernel, dim3(ql.blocks), dim3(QUAD_THREADS), 0, (hipStream_t)stream, pack, best_query, labels, n, Q,
                     h, w, H0, W0, (int)total, ql.shift, threshold, background);
  TCE_CHECK_LAUNCH("tce_label_objects_u8");
  return TCE_OK;
}
