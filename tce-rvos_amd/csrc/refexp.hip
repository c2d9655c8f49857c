// The RefCOCO / RefCOCO+ / RefCOCOg evaluation stage (csrc/tce_rvos_refexp.h): the reference's PostProcess and PostProcessSegm
// (models/postprocessors.py:58-155) for a group of samples -- a counting rank of each sample's Q*K sigmoid scores in LDS, the
// gathered and rescaled boxes, then the dataset-size masks of the ranked planes on the shared rules of mask_planes.h -- and the
// generalised IoU with its running maximum behind precision@k (util/box_ops.py:44-81, datasets/refexp_eval.py:65-67).
#include "common.h"
#include "mask_planes.h"
#include "../../include/tce_rvos_refexp.h"

namespace {

// the host table, by value in the kernel arguments (as a2d_group.hip takes its own): indexed by the workgroup, so a workgroup's
// entry arrives through scalar loads
struct RefexpTable {
  tceRefexpSample s[TCE_REFEXP_GROUP_MAX];
};

constexpr int RANK_THREADS = 256;

// does a stand before b in the descending order?  A NaN stands before every number, two NaNs tie (the index decides)
__device__ __forceinline__ bool rank_before(const float a, const float b) { return a > b || (a != a && b == b); }
__device__ __forceinline__ bool rank_tie(const float a, const float b) { return a == b || (a != a && b != b); }

// blockIdx.x = the sample.  Every candidate counts the candidates that stand before it: its rank, a permutation of 0 .. Q*K-1;
// the Q first ranks are the sample's outputs.
__global__ void __launch_bounds__(RANK_THREADS) refexp_rank_kernel(const RefexpTable tab, const int Q, const int K) {
#pragma clang fp contract(off)
  __shared__ float p[TCE_REFEXP_MAX_CAND];
  const tceRefexpSample s = tab.s[blockIdx.x];
  const int n = Q * K;
  for (int i = threadIdx.x; i < n; i += RANK_THREADS) p[i] = mask_sigmoid(s.logits[i]);
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += RANK_THREADS) {
    const float pi = p[i];
    int r = 0;
    for (int j = 0; j < n; ++j) {
      const float pj = p[j];
      r += (rank_before(pj, pi) || (rank_tie(pj, pi) && j < i)) ? 1 : 0;
    }
    if (r >= Q) continue;
    s.scores[r] = pi;
    s.order[r] = i;
    const float* b = s.boxes_in + (long long)(i / K) * 4;
    const float cx = b[0], cy = b[1], hw = 0.5f * b[2], hh = 0.5f * b[3];
    const float W0 = (float)s.W0, H0 = (float)s.H0;
    float* o = s.boxes_out + (long long)r * 4;
    o[0] = (cx - hw) * W0;
    o[1] = (cy - hh) * H0;
    o[2] = (cx + hw) * W0;
    o[3] = (cy + hh) * H0;
  }
}

// blockIdx.y = the sample, blockIdx.x = the 1024-byte piece of ITS [Q*H0*W0] output, as a2d_group_masks_kernel; output plane r is
// made from mask plane order[r] / K, which the rank launch in front of this one left in the sample's order (or the caller, in a
// ranked call: so the index is clamped to the candidates, and a foreign order can select a wrong plane but never leave the planes)
__global__ void __launch_bounds__(QUAD_THREADS) refexp_masks_kernel(const RefexpTable tab, const int Q, const int K, const int h,
                                                                    const int w, const float threshold) {
  const tceRefexpSample s = tab.s[blockIdx.y];
  const int total = Q * s.H0 * s.W0;  // < 2^31 - 4096 (checked on the host)
  const int shift = (int)((uintptr_t)s.out & 3u);
  const int p0 = byte_quad_p0(shift);
  if (p0 >= total) return;
  QuadPixel px[4];
  byte_quad_pixels(p0, total, s.H0, s.W0, px);
  uint32_t bit[4];
  mask_quad_bits(px, h, w, s.fh, s.fw, s.H0, s.W0, threshold,
                 [&](const int r) { return s.masks + (long long)(min(max(s.order[r], 0), Q * K - 1) / K) * h * w; }, bit);
  byte_quad_store(s.out, p0, total, bit);
}

// blockIdx.x = the image: its Q values, then their running maximum out of LDS
__global__ void __launch_bounds__(RANK_THREADS) refexp_giou_kernel(const float* __restrict__ boxes, const float* __restrict__ gt,
                                                                   float* __restrict__ giou, float* __restrict__ best, const int Q) {
#pragma clang fp contract(off)
  __shared__ float g[1024];
  const long long m = blockIdx.x;
  const float gx0 = gt[m * 4], gy0 = gt[m * 4 + 1], gx1 = gt[m * 4 + 2], gy1 = gt[m * 4 + 3];
  const float area_g = (gx1 - gx0) * (gy1 - gy0);
  for (int q = threadIdx.x; q < Q; q += RANK_THREADS) {
    const float* b = boxes + (m * Q + q) * 4;
    const float x0 = b[0], y0 = b[1], x1 = b[2], y1 = b[3];
    const float area_p = (x1 - x0) * (y1 - y0);
    const float inter = fmaxf(fminf(x1, gx1) - fmaxf(x0, gx0), 0.f) * fmaxf(fminf(y1, gy1) - fmaxf(y0, gy0), 0.f);
    const float uni = (area_p + area_g) - inter;
    const float iou = (inter + 1e-6f) / (uni + 1e-6f);
    const float area = fmaxf(fmaxf(x1, gx1) - fminf(x0, gx0), 0.f) * fmaxf(fmaxf(y1, gy1) - fminf(y0, gy0), 0.f);
    const float v = iou - ((area - uni) + 1e-6f) / (area + 1e-6f);
    g[q] = v;
    giou[m * Q + q] = v;
  }
  __syncthreads();
  for (int q = threadIdx.x; q < Q; q += RANK_THREADS) {
    float mx = g[0];
    for (int j = 1; j <= q; ++j) mx = fmaxf(mx, g[j]);
    best[m * Q + q] = mx;
  }
}

struct Range {
  uintptr_t lo, hi;
};

}  // namespace

extern "C" int tce_refexp_group_u8(const tceRefexpSample* samples, int32_t B, int32_t Q, int32_t K, int32_t h, int32_t w,
                                   float threshold, tceStream stream) {
  TCE_CHECK_ARG(samples, "tce_refexp_group_u8: null pointer");
  TCE_CHECK_ARG(B >= 1 && B <= TCE_REFEXP_GROUP_MAX, "tce_refexp_group_u8: 1..%d samples per call, got %d", TCE_REFEXP_GROUP_MAX, B);
  TCE_CHECK_ARG(Q > 0 && K > 0, "tce_refexp_group_u8: non-positive extent");
  TCE_CHECK_ARG((long long)Q * K <= TCE_REFEXP_MAX_CAND, "tce_refexp_group_u8: at most %d candidates (Q*K) per sample, got %lld",
                TCE_REFEXP_MAX_CAND, (long long)Q * K);
  const bool box_only = !(samples[0].masks && samples[0].out), ranked = !samples[0].logits;
  TCE_CHECK_ARG(!(box_only && ranked), "tce_refexp_group_u8: a ranked call (logits NULL) needs masks and out: nothing to do");
  if (!box_only) {
    TCE_CHECK_ARG(h > 0 && w > 0, "tce_refexp_group_u8: non-positive extent");
    TCE_CHECK_ARG((long long)Q * h * w < (1ll << 31), "tce_refexp_group_u8: the mask planes must stay below 2^31 elements");
  }
  RefexpTable pack;
  Range rg[4 * TCE_REFEXP_GROUP_MAX];
  int blocks = 0, nr = 0;
  for (int i = 0; i < TCE_REFEXP_GROUP_MAX; ++i) {
    const tceRefexpSample& s = samples[i < B ? i : 0];  // unused slots repeat sample 0: never read (the grids have B rows)
    if (i < B) {
      TCE_CHECK_ARG(!s.logits == ranked, "tce_refexp_group_u8: sample %d %s logits, sample 0 %s (a call is ranked for all samples or for none)",
                    i, ranked ? "has" : "lacks", ranked ? "lacks them" : "has them");
      TCE_CHECK_ARG(s.order && (ranked || (s.boxes_in && s.scores && s.boxes_out)), "tce_refexp_group_u8: null pointer in sample %d", i);
      TCE_CHECK_ARG(s.H0 > 0 && s.W0 > 0, "tce_refexp_group_u8: non-positive extent in sample %d", i);
      TCE_CHECK_ARG(!(s.masks && s.out) == box_only,
                    "tce_refexp_group_u8: sample %d %s masks and out, sample 0 %s (a call is box-only for all samples or for none)", i,
                    box_only ? "has" : "lacks", box_only ? "lacks them" : "has them");
      TCE_CHECK_ARG((((uintptr_t)s.logits | (uintptr_t)s.boxes_in | (uintptr_t)s.masks | (uintptr_t)s.scores | (uintptr_t)s.order |
                      (uintptr_t)s.boxes_out) & 3u) == 0,
                    "tce_refexp_group_u8: logits, boxes_in, masks, scores, order and boxes_out of sample %d must be 4-byte aligned", i);
      if (!ranked) {
        rg[nr++] = {(uintptr_t)s.scores, (uintptr_t)s.scores + (size_t)Q * 4};
        rg[nr++] = {(uintptr_t)s.order, (uintptr_t)s.order + (size_t)Q * 4};
        rg[nr++] = {(uintptr_t)s.boxes_out, (uintptr_t)s.boxes_out + (size_t)Q * 16};
      }
      if (!box_only) {
        TCE_CHECK_ARG(s.fh > 0 && s.fw > 0, "tce_refexp_group_u8: non-positive extent in sample %d", i);
        TCE_CHECK_ARG((long long)s.fh <= 4ll * h && (long long)s.fw <= 4ll * w,
                      "tce_refexp_group_u8: the un-padded size (%d, %d) of sample %d exceeds 4x the mask plane (%d, %d)", s.fh, s.fw, i, h,
                      w);
        const long long total = (long long)Q * s.H0 * s.W0;
        TCE_CHECK_ARG(total < (1ll << 31) - 4096, "tce_refexp_group_u8: the output of sample %d must stay below 2^31 elements", i);
        blocks = std::max(blocks, byte_quad_launch(s.out, total).blocks);
        rg[nr++] = {(uintptr_t)s.out, (uintptr_t)s.out + (size_t)total};
      }
    }
    pack.s[i] = s;
  }
  for (int a = 0; a < nr; ++a)
    for (int b = a + 1; b < nr; ++b)
      TCE_CHECK_ARG(rg[a].hi <= rg[b].lo || rg[b].hi <= rg[a].lo, "tce_refexp_group_u8: two output ranges of the call overlap");
  if (!ranked) {
    hipLaunchKernelGGL(refexp_rank_kernel, dim3(B), dim3(RANK_THREADS), 0, (hipStream_t)stream, pack, Q, K);
    TCE_CHECK_LAUNCH("tce_refexp_group_u8");
  }
  if (!box_only) {
    hipLaunchKernelGGL(refexp_masks_kernel, dim3(blocks, B), dim3(QUAD_THREADS), 0, (hipStream_t)stream, pack, Q, K, h, w, threshold);
    TCE_CHECK_LAUNCH("tce_refexp_group_u8");
  }
  return TCE_OK;
}

extern "C" int tce_refexp_giou_f32(const float* boxes, const float* gt, float* giou, float* best, int32_t M, int32_t Q,
                                   tceStream stream) {
  TCE_CHECK_ARG(boxes && gt && giou && best, "tce_refexp_giou_f32: null pointer");
  TCE_CHECK_ARG(M >= 1 && M <= 65535, "tce_refexp_giou_f32: 1..65535 images per call, got %d", M);
  TCE_CHECK_ARG(Q >= 1 && Q <= 1024, "tce_refexp_giou_f32: 1..1024 boxes per image, got %d", Q);
  TCE_CHECK_ARG((((uintptr_t)boxes | (uintptr_t)gt | (uintptr_t)giou | (uintptr_t)best) & 3u) == 0,
                "tce_refexp_giou_f32: the pointers must be 4-byte aligned");
  hipLaunchKernelGGL(refexp_giou_kernel, dim3(M), dim3(RANK_THREADS), 0, (hipStream_t)stream, boxes, gt, giou, best, Q);
  TCE_CHECK_LAUNCH("tce_refexp_giou_f32");
  return TCE_OK;
}
