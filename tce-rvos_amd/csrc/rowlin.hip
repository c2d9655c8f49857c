// ---------------------------------------------------------------------------------------------------------------
// Token-stationary linear layer ("rowlin"):  out[M,N] = LN_out?( epi( LN_in?(x + a2) W^T + bias ) )   K = 96..256
// Same machinery as the fused FFN: x (32 tokens per wave, K/2 registers) is loaded once in full lines and stays in
// registers as fp16 hi/lo B fragments; W [N,K] is pre-split / pre-ordered into 1 KiB A fragments, one block of
// 2*K/16 pieces per 32 output channels, streamed L2 -> LDS by DMA through a two-stage ring; each 32-channel
// accumulator tile is finished (bias, activation, residual add / multiply) and stored in full lines through the
// wave's staging tile while the next tile's weights are in flight.  ROW mode (N = 256) keeps all 8 tiles in registers
// and applies a LayerNorm over the row before storing: out_proj + residual + LayerNorm of the post-norm transformer
// blocks in one launch.  Replaces the K <= 256 nn.Linear / 1x1 conv call sites with many rows
// (tce_deformable_transformer.py:439-489,535-548; ops/modules/ms_deform_attn.py:94-101,115; segmentation.py:187,330-372;
// swin_transformer.py:133,151; tce_rvos.py:260).
// ---------------------------------------------------------------------------------------------------------------
#include "common.h"
#include "gemm_epilogue.h"
#include "frag.h"
#include "tiles.h"
#include "../../include/tce_rvos.h"

namespace {

// Diagnostic stamps: THIS unit's copy of the pointer that tce_debug_ffn_set_stamp_buffer (ffn.hip) sets through
// tce_rowlin_set_stamps below.  Lane 0 of wave 0 of the first 1024 workgroups records, slots 0..6: {s_memtime at entry, before
// the loop, at exit (twice), s_memrealtime at entry, at exit, s_memtime after the x load}.
static __device__ long long* g_ffn_stamps = nullptr;

struct LinArgs {
  const float *x, *a2;
  const unsigned char* wpk;
  const float *bias, *res;
  float* out;
  const float *g_in, *be_in, *g_out, *be_out;
  long long ldx, lda2, ldres, ldo;
  long long sX, sA2, sRes, sOut;  // batch strides in floats (grid.y)
  int M, N, a2_rows, act, res_mode;
  float eps_in, eps_out;
  int* range_flag;
  int single;
};

// K = 384 (round 4: Swin-T's third stage, 4600 rows at config 2: norm1 -> qkv, proj + residual, norm2 -> fc1 + GELU): the x
// fragments take 192 registers -> one workgroup per CU (90 KB of LDS); with the output tiles split over gridDim.z the 36 row
// blocks become ~290 workgroups of 4-6 tiles each, against the tiled GEMM's 12 short K slices per tile (32 us per launch there).
// K = 96 (Swin-T stage 0) is compiled for THREE workgroups per CU (168 registers, 43 KB of LDS): at config 2 the stage has
// 72000 rows = 563 row blocks, one more than two per CU hold (512) -- a second, nearly empty round.  47.7 -> 38.5 us for the
// norm1 -> qkv launch (profiles/r03_rowlin_occupancy.txt).
template <int K, bool ROW, bool SINGLE>  // SINGLE: compile-time arithmetic mode, see ffn_fused_kernel
__global__ void __launch_bounds__(256, (ROW || K > 256) ? 1 : (K <= 96 ? 3 : 2)) rowlin_kernel(const LinArgs p) {
  // The ring holds HALF blocks (the first / second K/32 k-steps of a 32-channel tile, hi and lo pieces interleaved,
  // padded to a multiple of 4 pieces so that every wave issues the same number of DMAs): three half-stages, the DMA of
  // half h+2 is issued while half h is multiplied.  3 x 16 KiB + staging tiles = 66 KiB at K = 256: two workgroups
  // per CU in streaming mode (<= 256 registers), so one workgroup's tile epilogue hides under the other's MFMAs.
  constexpr int WAVES = 4, KS = K / 16, KH = KS / 2;
  constexpr int HP = (2 * KH + WAVES - 1) / WAVES * WAVES;  // pieces per half block
  constexpr int SLOTS = HP / WAVES;
  constexpr int HSTAGE = HP * PIECE;
  constexpr int NTR = 8;  // ROW mode: N = 256
  static_assert(KS % 2 == 0 && SLOTS <= KH, "piece count");
  __shared__ __attribute__((aligned(16))) unsigned char smem[3 * HSTAGE + WAVES * WT_BYTES];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hf = lane >> 5;
  const int bz = blockIdx.y;
  const int m0 = blockIdx.x * (32 * WAVES) + wave * 32;
  if (p.M < 0) reinterpret_cast<u32x4*>(smem)[tid] = u32x4{0u, 0u, 0u, 0u};  // see ffn_fused_kernel

  const float* const x = p.x + bz * p.sX;
  const float* const a2 = p.a2 ? p.a2 + bz * p.sA2 : nullptr;
  const float* const res = p.res ? p.res + bz * p.sRes : nullptr;
  float* const out = p.out + bz * p.sOut;
  // streaming mode: the 32-channel tiles may be split over gridDim.z workgroups (each re-reads x: a few MB against a
  // much shorter serial chain of tiles per workgroup, which is what bounds launches with few rows)
  const int ntiles = p.N / 32;
  const int t_begin = ROW ? 0 : (int)((long long)blockIdx.z * ntiles / gridDim.z);
  const int t_end = ROW ? ntiles : (int)((long long)(blockIdx.z + 1) * ntiles / gridDim.z);

  long long* const stamps = (g_ffn_stamps && blockIdx.x < 1024 && bz == 0 && blockIdx.z == 0 && tid == 0) ? g_ffn_stamps + blockIdx.x * 8 : nullptr;
  if (stamps) {
    stamps[0] = (long long)__builtin_amdgcn_s_memtime();
    stamps[4] = (long long)__builtin_amdgcn_s_memrealtime();
  }
  const unsigned char* wp = p.wpk + ((long long)2 * t_begin * HP + wave) * PIECE;
  const unsigned voff = lane * 16;
  const unsigned wbase = wave * PIECE;
  int dstage = 0;  // ring slot the next half block goes to
  auto dma_half = [&](int q) { glds16(wp + (long long)q * WAVES * PIECE, voff, wbase + (unsigned)(dstage * HSTAGE + q * WAVES * PIECE)); };
  auto dma_next = [&]() {
    wp += HP * PIECE;
    dstage = dstage == 2 ? 0 : dstage + 1;
  };
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int q = 0; q < SLOTS; ++q) dma_half(q);
    dma_next();
  }

  float* const wt = reinterpret_cast<float*>(smem + 3 * HSTAGE + wave * WT_BYTES);
  h16x8 xh[KS], xl[KS];
  load_x_frags<K>(x, p.ldx, a2, p.lda2, p.a2_rows, m0, p.M, wt, lane, p.g_in, p.be_in, p.eps_in, xh, xl, SINGLE);
  constexpr int single = SINGLE;
  tce_amax_t amax = 0;
  if (stamps) stamps[6] = (long long)__builtin_amdgcn_s_memtime();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (stamps) stamps[1] = (long long)__builtin_amdgcn_s_memtime();

  int cstage = 0;  // ring slot of the half block being multiplied
  // one half of a 32-channel tile: acc += W[tile, k-steps of this half] x^T; issues the DMA of the half after next.
  // Fragments are fetched TWO k-steps ahead of their MFMAs (LDS latency under load is longer than one step's three
  // MFMAs); sched_barrier pins each step, otherwise the compiler sinks the reads behind the MFMAs they should overlap.
  auto half_mma = [&](auto half_c, f32x16& acc) {
    constexpr int S0 = decltype(half_c)::value * KH;
    const unsigned char* const st = smem + cstage * HSTAGE + lane * 16;
    h16x8 fh[3], fl[3];
#pragma unroll
    for (int q = 0; q < 2; ++q)
      if (q < KH) {
        fh[q] = *reinterpret_cast<const h16x8*>(st + (2 * q) * PIECE);
        fl[q] = *reinterpret_cast<const h16x8*>(st + (2 * q + 1) * PIECE);
      }
#pragma unroll
    for (int s = 0; s < KH; ++s) {
      if (s + 2 < KH) {
        fh[(s + 2) % 3] = *reinterpret_cast<const h16x8*>(st + (2 * s + 4) * PIECE);
        fl[(s + 2) % 3] = *reinterpret_cast<const h16x8*>(st + (2 * s + 5) * PIECE);
      }
      if (s < SLOTS) dma_half(s);
      __builtin_amdgcn_sched_barrier(0);
      if (!single) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fh[s % 3], xl[S0 + s], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fl[s % 3], xh[S0 + s], acc, 0, 0, 0);
      }
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fh[s % 3], xh[S0 + s], acc, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    dma_next();
    cstage = cstage == 2 ? 0 : cstage + 1;
  };
  auto act_tile = [&](f32x16& acc) {
    if (p.act == 1) {
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = fmaxf(acc[i], 0.f);
    } else if (p.act == 2) {
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = tce_gelu(acc[i]);
    }
  };
  // bias, activation, residual (activation sits between bias and residual, as in tce_gemm_f32)
  auto finish_tile = [&](f32x16& acc, const BiasTile& bt, const ResTile& rt) {
    const ResTile none = {};
    const BiasTile nob = {};
    if (p.res_mode == 0 || p.act != 0) {
      tile_bias_res<0>(acc, bt, none, wt, lane);
      act_tile(acc);
      if (p.res_mode == 1) tile_bias_res<1>(acc, nob, rt, wt, lane);
      else if (p.res_mode == 2) tile_bias_res<2>(acc, nob, rt, wt, lane);
    } else if (p.res_mode == 1) {
      tile_bias_res<1>(acc, bt, rt, wt, lane);
    } else {
      tile_bias_res<2>(acc, bt, rt, wt, lane);
    }
  };
  // the half just multiplied may be overwritten and the next one must have landed: only this wave's DMAs of the half
  // after next (SLOTS of them) may stay in flight
  auto tile_mma = [&](f32x16& acc, const bool stores_follow) {
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    half_mma(std::integral_constant<int, 0>{}, acc);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(SLOTS) : "memory");
    __syncthreads();
    half_mma(std::integral_constant<int, 1>{}, acc);
    (void)stores_follow;
  };

  if (ROW) {
    f32x16 oacc[NTR];
#pragma unroll
    for (int t = 0; t < NTR; ++t) {
      tile_mma(oacc[t], false);
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(SLOTS) : "memory");
      __syncthreads();
    }
    {
      ResTile rt[NTR];
      if (p.res_mode != 0) {
#pragma unroll
        for (int t = 0; t < NTR; ++t) rt[t] = tile_res_load(res, p.ldres, m0, p.M, 32 * t, lane);
      }
#pragma unroll
      for (int t = 0; t < NTR; ++t) finish_tile(oacc[t], tile_bias_load(p.bias, 32 * t, lane), rt[t]);
    }
    if (p.g_out) rows_layernorm<NTR>(oacc, p.g_out, p.be_out, p.eps_out, hf);
#pragma unroll
    for (int t = 0; t < NTR; ++t) tile_store(oacc[t], out, p.ldo, m0, p.M, 32 * t, wt, lane, amax);
  } else {
    for (int t = t_begin; t < t_end; ++t) {
      ResTile rt = {};
      if (p.res_mode != 0) rt = tile_res_load(res, p.ldres, m0, p.M, 32 * t, lane);  // both land under the MFMAs
      const BiasTile bt = tile_bias_load(p.bias, 32 * t, lane);
      f32x16 acc;
      tile_mma(acc, true);
      // Only the DMAs of the half after next are younger than what must have landed, and DMAs retire in issue order
      // among themselves -- so this count is exact.  The wait sits BEFORE the tile's stores on purpose: loads and
      // stores do not retire in order relative to each other, and with the stores in front of it a count of
      // SLOTS + 4 could be satisfied by early store acknowledgements while a needed DMA was still in flight.
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(SLOTS) : "memory");
      __syncthreads();
      finish_tile(acc, bt, rt);
      tile_store(acc, out, p.ldo, m0, p.M, 32 * t, wt, lane, amax);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // no DMA may outlive the workgroup's LDS allocation
  tce_range_report(p.range_flag, amax);
  if (stamps) {
    stamps[2] = (long long)__builtin_amdgcn_s_memtime();
    stamps[3] = (long long)__builtin_amdgcn_s_memtime();
    stamps[5] = (long long)__builtin_amdgcn_s_memrealtime();
  }
}

// W [N, K] (row pitch ldw) -> per 32 output channels two HALF blocks of HP pieces (HP = 2 * K/32 rounded up to a
// multiple of 4): piece 2j (+1) of half h = hi (lo) fragment of k-step s = h*K/32 + j: lane (r, hf) holds
// W[32t + r][16s + 8hf + 0..7]; padding pieces are zero.  Two trailing half blocks of zeros (the prefetch runs two
// halves ahead).
__global__ void __launch_bounds__(256) rowlin_pack_kernel(const float* __restrict__ W, unsigned char* __restrict__ out,
                                                          const int N, const int K, const long long ldw,
                                                          const long long units, const int single) {
  const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
  if (u >= units) return;
  const int KH = K / 32, HP = (2 * KH + 3) / 4 * 4;
  const int lane = (int)(u & 63);
  const long long pg = u >> 6;
  const int piece = (int)(pg % HP);
  const long long hb = pg / HP;  // half-block index = 2 * tile + half
  const int t = (int)(hb >> 1), h = (int)(hb & 1);
  const int r = lane & 31, hf = lane >> 5, s = h * KH + (piece >> 1);
  u32x4 o = {0u, 0u, 0u, 0u};
  const int n = 32 * t + r;
  if (piece < 2 * KH && n < N) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = W[(long long)n * ldw + 16 * s + 8 * hf + j];
    const HL f = split8(v, single);
    o = __builtin_bit_cast(u32x4, (piece & 1) ? f.lo : f.hi);
  }
  reinterpret_cast<u32x4*>(out)[u] = o;
}

inline bool rowlin_shape_ok(int N, int K) {
  return (K == 96 || K == 128 || K == 192 || K == 256 || K == 384 || K == 512) && N > 0 && N % 32 == 0;
}
inline long long rowlin_units(int N, int K) {
  const int HP = (2 * (K / 32) + 3) / 4 * 4;
  return (long long)(2 * (N / 32) + 2) * HP * 64;
}

template <int K>
void rowlin_launch(const LinArgs& a, int batch, bool row, hipStream_t s) {
  // aim at >= ~3 workgroups per CU-pair slot: split the output tiles when the row blocks alone leave the chip idle
  const int rb = tce_cdiv(a.M, 128) * batch, ntiles = a.N / 32;
  int nz = 1;
  if (!row && K > 256) {
    // one workgroup per CU (x alone takes 192 registers): exactly ONE round of <= 256 workgroups, at least two tiles each
    // (36 row blocks x 8 splits = 288 workgroups ran a second, nearly empty round: slower than the tiled GEMM)
    nz = 256 / (rb > 0 ? rb : 1);
    if (nz > ntiles / 2) nz = ntiles / 2;
    if (nz < 1) nz = 1;
  } else if (!row) {
    while (nz < ntiles && rb * nz < 160 && ntiles / (nz * 2) >= 2) nz *= 2;  // only launches with few row blocks
  }
  const dim3 grid(tce_cdiv(a.M, 128), batch, nz), block(256);
  if constexpr (K <= 384) {  // (row mode keeps 8 accumulator tiles beside x: no room at K = 512; the entry point rejects it)
    if (row) {
      if (a.single) hipLaunchKernelGGL((rowlin_kernel<K, true, true>), grid, block, 0, s, a);
      else hipLaunchKernelGGL((rowlin_kernel<K, true, false>), grid, block, 0, s, a);
      return;
    }
  }
  if (a.single) hipLaunchKernelGGL((rowlin_kernel<K, false, true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((rowlin_kernel<K, false, false>), grid, block, 0, s, a);
}

}  // namespace

int tce_rowlin_set_stamps(long long* dev_buf) {
  return hipMemcpyToSymbol(HIP_SYMBOL(g_ffn_stamps), &dev_buf, sizeof(dev_buf)) == hipSuccess ? 0 : -1;
}

extern "C" int64_t tce_rowlin_packed_bytes(int32_t N, int32_t K) { return rowlin_shape_ok(N, K) ? rowlin_units(N, K) * 16 : -1; }

extern "C" int tce_rowlin_pack_f32(const float* W, int64_t ldw, void* packed, int32_t N, int32_t K, tceStream stream) {
  TCE_CHECK_ARG(rowlin_shape_ok(N, K), "tce_rowlin_pack_f32: unsupported shape N=%d K=%d (K in 96/128/192/256/384/512, N %% 32 == 0)", N, K);
  TCE_CHECK_ARG(W && packed && tce_aligned16(packed) && ldw >= K, "tce_rowlin_pack_f32: null / misaligned pointer or ldw < K");
  const long long units = rowlin_units(N, K);
  hipLaunchKernelGGL(rowlin_pack_kernel, dim3(tce_cdiv(units, 256)), dim3(256), 0, (hipStream_t)stream, W,
                     (unsigned char*)packed, N, K, (long long)ldw, units, tce_gemm_single_pass());
  TCE_CHECK_LAUNCH("tce_rowlin_pack_f32");
  return TCE_OK;
}

extern "C" int tce_rowlin_f32(const tceRowLinArgs* args, tceStream stream) {
  TCE_CHECK_ARG(args != nullptr, "tce_rowlin_f32: null args");
  const tceRowLinArgs& q = *args;
  TCE_CHECK_ARG(rowlin_shape_ok(q.N, q.K), "tce_rowlin_f32: unsupported shape N=%d K=%d", q.N, q.K);
  TCE_CHECK_ARG(q.M > 0 && q.x && q.packed && q.out, "tce_rowlin_f32: null pointer or M <= 0");
  TCE_CHECK_ARG(q.act >= 0 && q.act <= 2 && q.res_mode >= 0 && q.res_mode <= 2, "tce_rowlin_f32: bad act / res_mode");
  TCE_CHECK_ARG(q.res_mode == 0 || q.res, "tce_rowlin_f32: res_mode set without res");
  TCE_CHECK_ARG(q.ldx >= q.K && q.ldx % 4 == 0 && q.ldo >= q.N && q.ldo % 4 == 0 && (!q.res || (q.ldres >= q.N && q.ldres % 4 == 0)) &&
                    (!q.a2 || (q.lda2 >= q.K && q.lda2 % 4 == 0)),
                "tce_rowlin_f32: bad row pitch");
  TCE_CHECK_ARG(q.sX % 4 == 0 && q.sA2 % 4 == 0 && q.sRes % 4 == 0 && q.sOut % 4 == 0, "tce_rowlin_f32: batch strides must be multiples of 4 floats");
  TCE_CHECK_ARG(tce_aligned16(q.x) && tce_aligned16(q.out) && tce_aligned16(q.packed) && (!q.a2 || tce_aligned16(q.a2)) &&
                    (!q.res || tce_aligned16(q.res)) && (!q.bias || tce_aligned16(q.bias)),
                "tce_rowlin_f32: pointers must be 16-byte aligned");
  TCE_CHECK_ARG((!q.g_in || (q.be_in && tce_aligned16(q.g_in) && tce_aligned16(q.be_in))) &&
                    (!q.g_out || (q.be_out && tce_aligned16(q.g_out) && tce_aligned16(q.be_out))),
                "tce_rowlin_f32: LayerNorm gamma/beta must come in pairs, 16-byte aligned");
  TCE_CHECK_ARG(!q.g_out || (q.N == 256 && q.K <= 384), "tce_rowlin_f32: the output LayerNorm is built for N = 256, K <= 384");
  LinArgs a;
  a.x = q.x; a.a2 = q.a2; a.wpk = (const unsigned char*)q.packed; a.bias = q.bias; a.res = q.res; a.out = q.out;
  a.g_in = q.g_in; a.be_in = q.be_in; a.g_out = q.g_out; a.be_out = q.be_out;
  a.ldx = q.ldx; a.lda2 = q.lda2; a.ldres = q.ldres; a.ldo = q.ldo;
  a.sX = q.sX; a.sA2 = q.sA2; a.sRes = q.sRes; a.sOut = q.sOut;
  a.M = q.M; a.N = q.N; a.a2_rows = q.a2_rows; a.act = q.act; a.res_mode = q.res_mode;
  a.eps_in = q.eps_in; a.eps_out = q.eps_out; a.range_flag = tce_range_flag(); a.single = tce_gemm_single_pass();
  const int batch = q.batch > 0 ? q.batch : 1;
  const bool row = q.g_out != nullptr;
  hipStream_t s = (hipStream_t)stream;
  if (q.K == 512) rowlin_launch<512>(a, batch, row, s);  // Swin-B stage 3 (C = 512): x = 256 registers, one workgroup per CU
  else if (q.K == 384) rowlin_launch<384>(a, batch, row, s);  // Swin stage 3 (C = 384): x = 192 registers, one workgroup per CU
  else if (q.K == 256) rowlin_launch<256>(a, batch, row, s);
  else if (q.K == 192) rowlin_launch<192>(a, batch, row, s);
  else if (q.K == 128) rowlin_launch<128>(a, batch, row, s);
  else rowlin_launch<96>(a, batch, row, s);
  TCE_CHECK_LAUNCH("tce_rowlin_f32");
  return TCE_OK;
}
