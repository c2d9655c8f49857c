// Per-wave tile helpers shared by the token-stationary kernel families (ffn.hip, rowlin.hip, conv3x3.hip, patch_embed.hip):
// the x operand as fp16 hi/lo B fragments, residual / bias tiles, the full-line tile store through the wave's LDS staging
// tile, the row LayerNorm on accumulator tiles; static_for (also swinattn.hip) and the CU count the launch plans use.
#pragma once
#include <type_traits>

#include "common.h"
#include "gemm_epilogue.h"
#include "frag.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// Per-wave staging tile in LDS: 32 rows x 32 floats, 144-byte pitch.  Global memory is touched only in full 128-byte
// lines (one instruction = 8 rows x 128 B: lane l -> row 8i + (l>>3), 16-byte piece l&7), the MFMA side reads / writes
// row-per-lane; with the 144-byte pitch both patterns are bank-conflict free.  A wave's LDS operations execute in
// order, so its private tile needs no workgroup barrier -- only the compiler must not reorder (wave_barrier).
// ---------------------------------------------------------------------------------------------------------------

// x[32 tokens, K] (+ a2, LayerNorm) -> fp16 hi/lo B fragments (lane (r, hf) holds k = 16s + 8hf + 0..7 of token r).
// a2: optional addend with row pitch lda2; a2_rows > 0: its row index is (token % a2_rows) (a position map shared by
// all frames).  g_in / be_in: optional LayerNorm over K applied to (x + a2).
template <int K, bool HAS_A2 = true>
__device__ __forceinline__ void load_x_frags(const float* __restrict__ x, const long long ldx,
                                             const float* __restrict__ a2, const long long lda2, const int a2_rows,
                                             const int m0, const int M, float* __restrict__ wt, const int lane,
                                             const float* __restrict__ g_in, const float* __restrict__ be_in,
                                             const float eps, h16x8 (&xh)[K / 16], h16x8 (&xl)[K / 16],
                                             const int single = 0) {
  constexpr int NP = K / 32;
  const int cr = lane >> 3, cp = (lane & 7) * 4;
  const int r = lane & 31, hf = lane >> 5;
  f32x4 v[NP][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = min(m0 + 8 * i + cr, M - 1);
    const float* px = x + (long long)row * ldx + cp;
#pragma unroll
    for (int q = 0; q < NP; ++q) v[q][i] = *reinterpret_cast<const f32x4*>(px + 32 * q);
    if (HAS_A2 && a2) {
      const float* pa = a2 + (long long)(a2_rows > 0 ? row % a2_rows : row) * lda2 + cp;
#pragma unroll
      for (int q = 0; q < NP; ++q) v[q][i] += *reinterpret_cast<const f32x4*>(pa + 32 * q);
    }
  }
  if (g_in) {
    float mean[4], rstd[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float sum = 0.f;
#pragma unroll
      for (int q = 0; q < NP; ++q) sum += (v[q][i][0] + v[q][i][1]) + (v[q][i][2] + v[q][i][3]);
      sum += __shfl_xor(sum, 1, 64);
      sum += __shfl_xor(sum, 2, 64);
      sum += __shfl_xor(sum, 4, 64);
      mean[i] = sum * (1.f / K);
      float sq = 0.f;
#pragma unroll
      for (int q = 0; q < NP; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = v[q][i][e] - mean[i];
          sq = fmaf(d, d, sq);
        }
      sq += __shfl_xor(sq, 1, 64);
      sq += __shfl_xor(sq, 2, 64);
      sq += __shfl_xor(sq, 4, 64);
      rstd[i] = rsqrtf(sq * (1.f / K) + eps);
    }
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      const f32x4 g = *reinterpret_cast<const f32x4*>(g_in + 32 * q + cp);
      const f32x4 b = *reinterpret_cast<const f32x4*>(be_in + 32 * q + cp);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) v[q][i][e] = (v[q][i][e] - mean[i]) * rstd[i] * g[e] + b[e];
    }
  }
#pragma unroll
  for (int q = 0; q < NP; ++q) {
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(wt + (8 * i + cr) * WT_PITCH + cp) = v[q][i];
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float* pr = wt + r * WT_PITCH + 16 * h + 8 * hf;
      const f32x4 a = *reinterpret_cast<const f32x4*>(pr);
      const f32x4 b = *reinterpret_cast<const f32x4*>(pr + 4);
      const float f[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
      const HL sp = split8(f, single);
      xh[2 * q + h] = sp.hi;
      xl[2 * q + h] = sp.lo;
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// residual tile res[32 tokens, col0 .. col0+31] as four full-line loads per lane (issue them for ALL tiles first: a
// load -> LDS -> registers chain per tile would pay one memory round trip per tile)
struct ResTile {
  f32x4 v[4];
};
__device__ __forceinline__ ResTile tile_res_load(const float* __restrict__ res, const long long ldres, const int m0,
                                                 const int M, const int col0, const int lane) {
  const int cr = lane >> 3, cp = (lane & 7) * 4;
  ResTile t;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = min(m0 + 8 * i + cr, M - 1);
    t.v[i] = *reinterpret_cast<const f32x4*>(res + (long long)row * ldres + col0 + cp);
  }
  return t;
}

// bias[col0 .. col0+31] in accumulator order (4 x float4 per lane); loaded ahead of use like the residual tile
struct BiasTile {
  f32x4 v[4];
};
__device__ __forceinline__ BiasTile tile_bias_load(const float* __restrict__ bias, const int col0, const int lane) {
  BiasTile b;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    b.v[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (bias) b.v[g] = *reinterpret_cast<const f32x4*>(bias + col0 + 8 * g + 4 * (lane >> 5));
  }
  return b;
}

// acc (32 channels col0.. of 32 tokens, lane = token) = (acc + bias tile) (+ / *) residual tile
template <int RES>  // 0 none, 1 add, 2 multiply
__device__ __forceinline__ void tile_bias_res(f32x16& acc, const BiasTile& bt, const ResTile& rt,
                                              float* __restrict__ wt, const int lane) {
  const int cr = lane >> 3, cp = (lane & 7) * 4;
  const int r = lane & 31, hf = lane >> 5;
  if (RES != 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(wt + (8 * i + cr) * WT_PITCH + cp) = rt.v[i];
    __builtin_amdgcn_wave_barrier();
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const f32x4 bv = bt.v[g];
    if (RES != 0) {
      const f32x4 rv = *reinterpret_cast<const f32x4*>(wt + r * WT_PITCH + 8 * g + 4 * hf);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (RES == 1) acc[4 * g + c] = acc[4 * g + c] + bv[c] + rv[c];
        else acc[4 * g + c] = (acc[4 * g + c] + bv[c]) * rv[c];
      }
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[4 * g + c] += bv[c];
    }
  }
  if (RES != 0) __builtin_amdgcn_wave_barrier();
}

// stores acc (32 channels of 32 tokens) in full 128-byte lines
__device__ __forceinline__ void tile_store(const f32x16& acc, float* __restrict__ out, const long long ldo, const int m0,
                                           const int M, const int col0, float* __restrict__ wt, const int lane,
                                           tce_amax_t& amax) {
  const int cr = lane >> 3, cp = (lane & 7) * 4;
  const int r = lane & 31, hf = lane >> 5;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const f32x4 o = {acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
    amax = tce_amax4(amax, o);
    *reinterpret_cast<f32x4*>(wt + r * WT_PITCH + 8 * g + 4 * hf) = o;
  }
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = m0 + 8 * i + cr;
    const f32x4 o = *reinterpret_cast<const f32x4*>(wt + (8 * i + cr) * WT_PITCH + cp);
    if (row < M) *reinterpret_cast<f32x4*>(out + (long long)row * ldo + col0 + cp) = o;
  }
  __builtin_amdgcn_wave_barrier();
}

// LayerNorm over the N = 32 * NT channels a lane pair (l, l^32) holds in acc[NT] (registers 4g..4g+3 of tile t =
// channels 32t + 8g + 4hf + 0..3)
template <int NT>
__device__ __forceinline__ void rows_layernorm(f32x16 (&acc)[NT], const float* __restrict__ gamma,
                                               const float* __restrict__ beta, const float eps, const int hf) {
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) sum += acc[t][i];
  sum += __shfl_xor(sum, 32, 64);
  const float mean = sum * (1.f / (32 * NT));
  float sq = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float d = acc[t][i] - mean;
      sq = fmaf(d, d, sq);
    }
  sq += __shfl_xor(sq, 32, 64);
  const float rstd = rsqrtf(sq * (1.f / (32 * NT)) + eps);
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 gv = *reinterpret_cast<const f32x4*>(gamma + 32 * t + 8 * g + 4 * hf);
      const f32x4 bv = *reinterpret_cast<const f32x4*>(beta + 32 * t + 8 * g + 4 * hf);
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[t][4 * g + c] = (acc[t][4 * g + c] - mean) * rstd * gv[c] + bv[c];
    }
}

// compile-time loop: f(integral_constant<int, I>) for I = 0 .. N-1 (every per-step decision inside -- register arrays, ring
// offsets, wait counts -- is then a compile-time one)
template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

// Compute units of the current device, read once per device; 256 (MI355X) when there is no device (CPU-side planning).
inline int tce_cu_count() {
  static int cache[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
    (void)hipGetLastError();
    return 256;
  }
  if (!cache[dev]) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
      (void)hipGetLastError();
      n = 256;
    }
    cache[dev] = n;
  }
  return cache[dev];
}

}  // namespace
