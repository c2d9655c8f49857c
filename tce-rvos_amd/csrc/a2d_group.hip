// The A2D-Sentences / JHMDB-Sentences post-processor's output stage for a group of samples (csrc/tce_rvos_a2d_group.h): the
// dataset-size masks and the query scores of up to TCE_A2D_GROUP_MAX samples from one launch.  A byte kernel like a2d_masks_kernel
// (eval.hip), whose per-pixel body it takes from mask_planes.h (mask_quad_bits, shared with refexp.hip); what it saves is launches, not bytes.
#include "common.h"
#include "mask_planes.h"
#include "../../include/tce_rvos_eval.h"

namespace {

// the host table, by value in the kernel arguments (as label.hip and copy_segments_kernel take theirs): indexed by blockIdx.y, so
// a workgroup's entry arrives through scalar loads
struct A2dGroupTable {
  tceA2dGroupSample s[TCE_A2D_GROUP_MAX];
};

// blockIdx.y = the sample, blockIdx.x = the 1024-byte piece of ITS [N*H0*W0] output (the grid's x extent is the largest sample's:
// the workgroups of a smaller sample past its own end exit at once).  Per output byte exactly a2d_masks_kernel's operation sequence.
__global__ void __launch_bounds__(QUAD_THREADS) a2d_group_masks_kernel(const A2dGroupTable tab, const int N, const int h, const int w,
                                                                       const float threshold) {
  const tceA2dGroupSample s = tab.s[blockIdx.y];
  if (blockIdx.x == 0)  // the sample's scores: sigmoid_kernel's expression (misc.hip)
    for (int n = threadIdx.x; n < N; n += QUAD_THREADS) s.scores[n] = 1.f / (1.f + expf(-s.logits[(long long)n * s.logit_stride]));
  const int total = N * s.H0 * s.W0;  // < 2^31 - 4096 (checked on the host)
  const int shift = (int)((uintptr_t)s.out & 3u);
  const int p0 = byte_quad_p0(shift);
  if (p0 >= total) return;
  QuadPixel px[4];
  byte_quad_pixels(p0, total, s.H0, s.W0, px);
  uint32_t bit[4];
  mask_quad_bits(px, h, w, s.fh, s.fw, s.H0, s.W0, threshold, [&](const int n) { return s.masks + (long long)n * h * w; }, bit);
  byte_quad_store(s.out, p0, total, bit);
}

}  // namespace

extern "C" int tce_a2d_group_masks_u8(const tceA2dGroupSample* samples, int32_t B, int32_t N, int32_t h, int32_t w, float threshold,
                                      tceStream stream) {
  TCE_CHECK_ARG(samples, "tce_a2d_group_masks_u8: null pointer");
  TCE_CHECK_ARG(B >= 1 && B <= TCE_A2D_GROUP_MAX, "tce_a2d_group_masks_u8: 1..%d samples per launch, got %d", TCE_A2D_GROUP_MAX, B);
  TCE_CHECK_ARG(N > 0 && h > 0 && w > 0, "tce_a2d_group_masks_u8: non-positive extent");
  TCE_CHECK_ARG((long long)N * h * w < (1ll << 31), "tce_a2d_group_masks_u8: the mask planes must stay below 2^31 elements");
  A2dGroupTable pack;
  int blocks = 0;
  for (int i = 0; i < TCE_A2D_GROUP_MAX; ++i) {
    const tceA2dGroupSample& s = samples[i < B ? i : 0];  // unused slots repeat sample 0: never read (the grid has B rows)
    if (i < B) {
      TCE_CHECK_ARG(s.masks && s.logits && s.out && s.scores, "tce_a2d_group_masks_u8: null pointer in sample %d", i);
      TCE_CHECK_ARG(s.fh > 0 && s.fw > 0 && s.H0 > 0 && s.W0 > 0 && s.logit_stride >= 1,
                    "tce_a2d_group_masks_u8: non-positive extent in sample %d", i);
      TCE_CHECK_ARG((long long)s.fh <= 4ll * h && (long long)s.fw <= 4ll * w,
                    "tce_a2d_group_masks_u8: the un-padded size (%d, %d) of sample %d exceeds 4x the mask plane (%d, %d)", s.fh, s.fw, i, h, w);
      const long long total = (long long)N * s.H0 * s.W0;
      TCE_CHECK_ARG(total < (1ll << 31) - 4096, "tce_a2d_group_masks_u8: the output of sample %d must stay below 2^31 elements", i);
      TCE_CHECK_ARG((((uintptr_t)s.masks | (uintptr_t)s.logits | (uintptr_t)s.scores) & 3u) == 0,
                    "tce_a2d_group_masks_u8: masks, logits and scores of sample %d must be 4-byte aligned", i);
      blocks = std::max(blocks, byte_quad_launch(s.out, total).blocks);
    }
    pack.s[i] = s;
  }
  hipLaunchKernelGGL(a2d_group_masks_kernel, dim3(blocks, B), dim3(QUAD_THREADS), 0, (hipStream_t)stream, pack, N, h, w, threshold);
  TCE_CHECK_LAUNCH("tce_a2d_group_masks_u8");
  return TCE_OK;
}
