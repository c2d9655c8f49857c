// ---------------------------------------------------------------------------------------------------------------
// 3x3 convolution, stride 1, zero padding 1, CIN -> 256 channels, channels-last (the pixel decoder's output
// convolutions, segmentation.py:186-204,253-283).  Pixel-stationary: a wave owns 32 pixels (the MFMA columns) and all
// 256 output channels (8 accumulator tiles); K = 9 taps x CIN runs in 16-wide steps, ordered (vertical tap, channel
// chunk, horizontal tap) so that the three horizontal neighbours of a chunk are read in consecutive steps.
//   * The pixel's own operand -- 16 input channels of the tap's neighbour -- goes from global memory straight into
//     registers LX steps ahead (32 contiguous bytes per lane; out-of-image taps read a block of zeros instead) and is
//     split into fp16 hi/lo between the previous step's MFMAs: the activations never pass through LDS.
//   * The weight fragments of a step (8 channel tiles x hi/lo = 16 pieces of 1 KiB, pre-split and pre-ordered by
//     tce_conv3x3_pack_f32) are requested LW steps ahead into registers, each wave a quarter of the stage, written into
//     a 4-stage LDS ring two steps before use and read back by all waves as A fragments.
//   * One barrier per step, placed after tile 5: by then every fragment of the stage is in registers (the stage can be
//     refilled), and tiles 6 and 7 are issued behind the barrier so the LDS latency of the next step's first
//     fragments hides under them.
//   * All loads of the loop are issued by hand in a fixed order (per mid-step: the lane's two operand loads, then the
//     wave's four weight loads), which makes the counted vmcnt at a mid-step exact.  They are all REGISTER loads on
//     purpose: a first version streamed the weights with LDS-DMA (global_load_lds) next to register loads of the
//     operand, and on real (not L2-resident) activations the counted wait let operand registers be read before their
//     data had arrived -- register loads and LDS-DMA loads do not retire in issue order relative to each other, so one
//     vmcnt cannot cover both.  (The FFN / row-linear kernels, ffn.hip / rowlin.hip, count only DMA against DMA.)
// Ablations (tools/conv3_ablate.py, profiles/r02_conv3x3.txt): MFMA + LDS alone run at 1.4 PFLOP/s issued; the loads
// cost as much again because the L2 -> CU traffic (every workgroup streams the 2.4 MB of weights, every tap re-reads
// its pixels) is throughput-bound at the clock the MFMAs leave.
// ---------------------------------------------------------------------------------------------------------------
#include "common.h"
#include "gemm_epilogue.h"
#include "frag.h"
#include "tiles.h"
#include "../../include/tce_rvos.h"
#include "../../include/tce_rvos_debug.h"

namespace {

constexpr int CONV_PAD_STAGES = 6;  // = the kernel's weight lead LW

struct ConvArgs {
  const float* x;
  const unsigned char* wpk;
  const float* bias;
  float* out;
  long long ldx, ldo;
  int H, W, M;
  int* range_flag;
  int single;
  int m_off;  // first pixel of this launch (a launch may cover a row range [m_off, ...) of the map: the mixed form below)
  // split form only: workgroup = (piece, block) piece-major over nb blocks; piece s walks iterations conv3x3_piece_iter(pieces, s) ..
  // conv3x3_piece_iter(pieces, s+1) and stores its fp32 partial sums (no bias) to ws + s * (M - m_off) * 256, rows m - m_off
  int nb, pieces;
  float* ws;
};

// The K walk is 3 * CIN/64 iterations of 12 k-steps (vertical tap, group of 4 channel chunks); a split piece is a contiguous run of whole
// iterations (the unrolled body and its compile-time ring positions stay as they are).  Piece s of p starts at iteration s * ITERS / p:
// the p pieces cover every iteration exactly once (tce_conv3x3_split_kstep exports it for the CPU test).
constexpr int CONV_ITERS = 12;  // CIN = 256
__host__ __device__ constexpr int conv3x3_piece_iter(const int pieces, const int s) { return s * CONV_ITERS / pieces; }

// Ablation builds (tools/conv3_ablate.py, -DCONV_ABL=n; results are then wrong): bit 0: one workgroup per CU; bit 1: no
// barrier inside the loop; bit 2: no MFMA (fragments kept live); bit 3: no weight DMA inside the loop; bit 4: no operand
// loads inside the loop.
#ifndef CONV_ABL
#define CONV_ABL 0
#endif

template <int BYTE_OFF>
__device__ __forceinline__ void gload16(f32x4& dst, const float* ptr) {
  asm volatile("global_load_dwordx4 %0, %1, off offset:%2" : "=v"(dst) : "v"(ptr), "n"(BYTE_OFF) : "memory");
}

// WAVES = 8 (round 5, A/B): 256 pixels per workgroup, two waves per SIMD sharing ONE weight ring -- half the weight bytes per pixel
// through L2 -> CU, which is what bounds the kernel; each wave then moves 2 of a stage's 16 pieces and keeps shorter register rings
// (XS 4, NW 3) to stay inside 256 registers.
// SPLIT: one piece of the K walk per workgroup (see ConvArgs); partial sums out, conv3x3_reduce_kernel adds them and the bias.
template <int CIN, bool SINGLE, int WAVES = 4, bool SPLIT = false>
__global__ void __launch_bounds__(64 * WAVES, WAVES / 4) conv3x3_kernel(const ConvArgs p) {
  constexpr int NTL = 8;
  constexpr int PW = 16 / WAVES;          // weight pieces a wave moves per stage
  constexpr int STAGE = 2 * NTL * PIECE;  // one k-step of weights: 16 KiB
  constexpr int R = 4;                    // LDS ring stages
  constexpr int XS = WAVES == 4 ? 6 : 4, LX = XS + 1;  // operand ring slots (registers); the operand of step q is requested at mid-step q-LX
  constexpr int NW = WAVES == 4 ? CONV_PAD_STAGES - 2 : 3, LW = NW + 2;  // weight stages in flight (registers); those of step s are requested at mid-step s-LW
  constexpr int INFLIGHT = (2 + PW) * (LW - 3);  // loads younger than the weights a mid-step waits for (2 operand + PW weight per mid-step)
  static_assert(LW <= CONV_PAD_STAGES, "the packed stream's zero padding covers the weight lead");
  constexpr int BODY = 12;                // unrolled steps: 4 channel chunks x 3 horizontal taps (lcm of 3 and R)
  constexpr int ITERS = 3 * (CIN / 64);   // (vertical tap, group of 4 chunks)
  constexpr int KS = BODY * ITERS;
  static_assert(CIN % 64 == 0, "channel chunks come in groups of four");
  static_assert(BODY % R == 0 && BODY % XS == 0 && BODY % NW == 0 && LX >= LW, "ring positions are compile-time");
  static_assert(WAVES * WT_BYTES <= R * STAGE, "the epilogue's staging tiles alias the ring");
  static_assert(!SPLIT || (ITERS == CONV_ITERS && WAVES == 4 && !SINGLE), "split pieces: CIN = 256, 128-pixel workgroups, split fp16");
  __shared__ __attribute__((aligned(16))) unsigned char smem[R * STAGE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hf = lane >> 5;
  const int blk = SPLIT ? (int)blockIdx.x % p.nb : (int)blockIdx.x;
  const int piece = SPLIT ? (int)blockIdx.x / p.nb : 0;
  const int i0 = SPLIT ? conv3x3_piece_iter(p.pieces, piece) : 0;  // iterations [i0, i1) of the K walk
  const int i1 = SPLIT ? conv3x3_piece_iter(p.pieces, piece + 1) : ITERS;
  const int m0 = p.m_off + blk * (32 * WAVES) + wave * 32;

  // this lane's pixel; per (vertical tap, chunk group) the addresses of its three horizontal neighbours' channels, or
  // of the zero block behind the weights for taps outside the image
  const int m = m0 + (lane & 31);
  const int px = m % p.W, py = (m / p.W) % p.H;
  const float* const zeros = reinterpret_cast<const float*>(p.wpk + (long long)(KS + CONV_PAD_STAGES) * STAGE) + 8 * hf;
  const float* const xme = p.x + (long long)min(m, p.M - 1) * p.ldx + 8 * hf;
  auto iter_ptrs = [&](const int it, const float* (&q)[3]) {
    const int dy = it / (CIN / 64) - 1, cq = it % (CIN / 64);
    const bool row_ok = it < i1 && m < p.M && (unsigned)(py + dy) < (unsigned)p.H;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const bool ok = row_ok && (unsigned)(px + d - 1) < (unsigned)p.W;
      q[d] = (ok ? xme + (long long)(dy * p.W + d - 1) * p.ldx : zeros) + 64 * cq;
    }
  };

  // weights: this wave moves pieces PW*wave .. PW*wave+PW-1 of every stage (one float4 per lane and piece) through
  // registers into the ring
  const float* wp = reinterpret_cast<const float*>(p.wpk + ((long long)i0 * BODY * STAGE) + (long long)(PW * wave) * PIECE + lane * 16);
  unsigned char* const wdst = smem + (PW * wave) * PIECE + lane * 16;
  f32x4 wr[NW][PW];
  auto wload = [&](f32x4 (&dst)[PW]) {
    if (!(CONV_ABL & 8)) {
      gload16<0>(dst[0], wp);
      gload16<PIECE>(dst[1], wp);
      if constexpr (PW == 4) {
        gload16<2 * PIECE>(dst[2], wp);
        gload16<3 * PIECE>(dst[3], wp);
      }
    }
    wp += STAGE / 4;
  };
  auto wstore = [&](const f32x4 (&src)[PW], const int stage) {
#pragma unroll
    for (int q = 0; q < PW; ++q) *reinterpret_cast<f32x4*>(wdst + stage * STAGE + q * PIECE) = src[q];
  };

  f32x4 xr[XS][2];
  const float* cur[3];
  const float* nxt[3];
  iter_ptrs(i0, cur);
  iter_ptrs(i0 + 1, nxt);
  // operand of body step JJ (>= BODY: of the next iteration) -> ring slot
  auto xload = [&](auto jjc, f32x4 (&dst)[2]) {
    constexpr int JJ = decltype(jjc)::value;
    constexpr int J = JJ % BODY;
    const float* const src = JJ < BODY ? cur[J % 3] : nxt[J % 3];
    if (CONV_ABL & 16) return;
    gload16<64 * (J / 3)>(dst[0], src);
    gload16<64 * (J / 3) + 16>(dst[1], src);
  };
  // "every load up to n operations ago has landed"; the register tuples named here are what the following code reads
  auto wait_loads = [&](auto nc, f32x4 (&xs)[2], f32x4 (&ws)[PW]) {
    constexpr int N = (CONV_ABL & 24) ? 0 : decltype(nc)::value;
    if constexpr (PW == 4) {
      asm volatile("s_waitcnt vmcnt(%6)"
                   : "+v"(xs[0]), "+v"(xs[1]), "+v"(ws[0]), "+v"(ws[1]), "+v"(ws[2]), "+v"(ws[3])
                   : "n"(N)
                   : "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(%4)" : "+v"(xs[0]), "+v"(xs[1]), "+v"(ws[0]), "+v"(ws[1]) : "n"(N) : "memory");
    }
  };
  using nfl = std::integral_constant<int, INFLIGHT>;

  // prologue = mid-steps -LX .. -1 in the loop's own order (wait + ring write of step m+2, then the requests)
  f32x16 acc[NTL];
#pragma unroll
  for (int t = 0; t < NTL; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
  h16x8 bh, bl;
  static_for<0, LX>([&](auto mc) {
    constexpr int m = decltype(mc)::value - LX;
    if constexpr (m + 2 >= 0) {
      wait_loads(nfl{}, xr[(m + 2) % XS], wr[(m + 2) % NW]);
      wstore(wr[(m + 2) % NW], (m + 2) % R);
      if constexpr (m + 2 == 0) {  // operand 0 (two mid-steps older than these weights) feeds step 0 directly
        const float f[8] = {xr[0][0][0], xr[0][0][1], xr[0][0][2], xr[0][0][3], xr[0][1][0], xr[0][1][1], xr[0][1][2], xr[0][1][3]};
        const HL b = split8(f, SINGLE ? 1 : 0);
        bh = b.hi;
        bl = b.lo;
        asm volatile("" : "+v"(bh), "+v"(bl));  // the split reads xr[0] before a later request reuses it
      }
    }
    if constexpr (m + LX >= 0) xload(std::integral_constant<int, m + LX>{}, xr[(m + LX) % XS]);
    if constexpr (m + LW >= 0) wload(wr[(m + LW) % NW]);
  });
  __syncthreads();
  h16x8 fh[4], fl[4];
  {
    const unsigned char* const st = smem + lane * 16;
    fh[0] = *reinterpret_cast<const h16x8*>(st);
    fl[0] = *reinterpret_cast<const h16x8*>(st + PIECE);
    fh[1] = *reinterpret_cast<const h16x8*>(st + 2 * PIECE);
    fl[1] = *reinterpret_cast<const h16x8*>(st + 3 * PIECE);
  }

  for (int it = i0; it < i1; ++it) {
    static_for<0, BODY>([&](auto jc) {
      constexpr int j = decltype(jc)::value;
      constexpr int nslot = (j + 1) % XS;  // operand of the next step: split under this step's first four tiles
      const unsigned char* const st = smem + (j % R) * STAGE + lane * 16;
      unsigned nh[4], nl[4];
      auto tile = [&](auto tc) {
        constexpr int t = decltype(tc)::value;
#if CONV_ABL & 4
        const h16x8 k0 = fh[t % 4], k1 = fl[t % 4], k2 = bh, k3 = bl;
        asm volatile("" : : "v"(k0), "v"(k1), "v"(k2), "v"(k3));
#else
        if constexpr (!SINGLE) {
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fh[t % 4], bl, acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fl[t % 4], bh, acc[t], 0, 0, 0);
        }
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fh[t % 4], bh, acc[t], 0, 0, 0);
#endif
      };
      // tiles 0..5, the fragments two tiles ahead of their MFMAs (tiles 0 and 1 were fetched by the previous step)
      static_for<0, 6>([&](auto tc) {
        constexpr int t = decltype(tc)::value;
        fh[(t + 2) % 4] = *reinterpret_cast<const h16x8*>(st + (2 * t + 4) * PIECE);
        fl[(t + 2) % 4] = *reinterpret_cast<const h16x8*>(st + (2 * t + 5) * PIECE);
        __builtin_amdgcn_sched_barrier(0);
        tile(tc);
        if constexpr (t < 4) {
          const float a = xr[nslot][t >> 1][2 * (t & 1)], b = xr[nslot][t >> 1][2 * (t & 1) + 1];
          if constexpr (SINGLE) {
            nh[t] = __builtin_bit_cast(unsigned, fp16x2_t{(__fp16)a, (__fp16)b});
            nl[t] = 0u;
          } else {
            const fp16x2_t h = __builtin_amdgcn_cvt_pkrtz(a, b);
            nh[t] = __builtin_bit_cast(unsigned, h);
            nl[t] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(a - (float)h[0], b - (float)h[1]));
          }
          asm volatile("" : "+v"(nh[t]), "+v"(nl[t]));  // keeps the split here (it is only consumed by the next step)
        }
        __builtin_amdgcn_sched_barrier(0);
      });
      // Mid-step: every fragment of this stage is in registers.  The weights of step j+2 (requested LW-2 mid-steps ago)
      // go into their stage -- free since the barrier of mid-step j-2 -- and the barrier publishes the stage written
      // one mid-step ago and releases this one.  Tiles 6 and 7 are issued AFTER the barrier so that the LDS latency
      // of the next step's first fragments hides under them.
      wait_loads(nfl{}, xr[(j + 2) % XS], wr[(j + 2) % NW]);
      wstore(wr[(j + 2) % NW], (j + 2) % R);
      if (!(CONV_ABL & 2)) __syncthreads();
      xload(std::integral_constant<int, j + LX>{}, xr[(j + LX) % XS]);
      wload(wr[(j + LW) % NW]);
      {
        const unsigned char* const sn = smem + ((j + 1) % R) * STAGE + lane * 16;
        fh[0] = *reinterpret_cast<const h16x8*>(sn);
        fl[0] = *reinterpret_cast<const h16x8*>(sn + PIECE);
        fh[1] = *reinterpret_cast<const h16x8*>(sn + 2 * PIECE);
        fl[1] = *reinterpret_cast<const h16x8*>(sn + 3 * PIECE);
      }
      __builtin_amdgcn_sched_barrier(0);
      tile(std::integral_constant<int, 6>{});
      tile(std::integral_constant<int, 7>{});
      __builtin_amdgcn_sched_barrier(0);
      bh = __builtin_bit_cast(h16x8, u32x4{nh[0], nh[1], nh[2], nh[3]});
      bl = __builtin_bit_cast(h16x8, u32x4{nl[0], nl[1], nl[2], nl[3]});
    });
#pragma unroll
    for (int d = 0; d < 3; ++d) cur[d] = nxt[d];
    iter_ptrs(it + 2, nxt);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the trailing (padding) loads
  __syncthreads();

  float* const wt = reinterpret_cast<float*>(smem + wave * WT_BYTES);
  tce_amax_t amax = 0;
  if constexpr (SPLIT) {  // partial sums; the range guard runs on the reduced output
    float* const part = p.ws + (long long)piece * (p.M - p.m_off) * 256;
#pragma unroll
    for (int t = 0; t < NTL; ++t) tile_store(acc[t], part, 256, m0 - p.m_off, p.M - p.m_off, 32 * t, wt, lane, amax);
    return;
  }
  const ResTile none = {};
#pragma unroll
  for (int t = 0; t < NTL; ++t) {
    tile_bias_res<0>(acc[t], tile_bias_load(p.bias, 32 * t, lane), none, wt, lane);
    tile_store(acc[t], p.out, p.ldo, m0, p.M, 32 * t, wt, lane, amax);
  }
  tce_range_report(p.range_flag, amax);
}

// out[m_off + r][c] = bias[c] + part_0[r][c] + part_1[r][c] + ... in piece order (deterministic whatever order the pieces ran in);
// r < rows = M - m_off, one float4 per thread and step
__global__ void __launch_bounds__(256) conv3x3_reduce_kernel(const float* __restrict__ ws, const int pieces, const int rows,
                                                             const float* __restrict__ bias, float* __restrict__ out,
                                                             const long long ldo, const int m_off, int* range_flag) {
  const long long n4 = (long long)rows * 64, stride = (long long)gridDim.x * 256;
  tce_amax_t amax = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    const f32x4* src = reinterpret_cast<const f32x4*>(ws) + i;
    f32x4 v = src[0];
    for (int s = 1; s < pieces; ++s) v += src[(long long)s * n4];
    const int c4 = (int)(i & 63);
    if (bias) v += reinterpret_cast<const f32x4*>(bias)[c4];
    amax = tce_amax4(amax, v);
    *reinterpret_cast<f32x4*>(out + (m_off + (i >> 6)) * ldo + 4 * c4) = v;
  }
  tce_range_report(range_flag, amax);
}

// w [256, 9*CIN] (k = tap*CIN + c) -> 9*CIN/16 + 4 stages of 16 pieces in the kernel's K order: stage s = 12*it + j is
// vertical tap dy = it / (CIN/64), channel chunk cc = 4*(it % (CIN/64)) + j/3, horizontal tap dx = j % 3 (the three
// horizontal neighbours of a chunk in consecutive steps: they share cache lines).  Piece 2t (+1) = hi (lo) fragment of
// channel tile t: lane (r, hf) holds w[32t + r][(3dy+dx)*CIN + 16cc + 8hf + 0..7].  CONV_PAD_STAGES trailing stages of
// zeros (the weight requests run that many steps ahead) and 2 KiB of zeros that out-of-image taps read as their operand.
__global__ void __launch_bounds__(256) conv3x3_pack_kernel(const float* __restrict__ w, unsigned char* __restrict__ out,
                                                           const int CIN, const long long units, const int single) {
  const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
  if (u >= units) return;
  const int lane = (int)(u & 63);
  const long long pg = u >> 6;
  const int piece = (int)(pg & 15);
  const long long s = pg >> 4;
  const int r = lane & 31, hf = lane >> 5, t = piece >> 1;
  u32x4 o = {0u, 0u, 0u, 0u};
  if (s < 9 * CIN / 16) {
    const int it = (int)(s / 12), j = (int)(s % 12);
    const int dy = it / (CIN / 64), cc = 4 * (it % (CIN / 64)) + j / 3, dx = j % 3;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = w[(long long)(32 * t + r) * (9 * CIN) + (3 * dy + dx) * CIN + 16 * cc + 8 * hf + e];
    const HL f = split8(v, single);
    o = __builtin_bit_cast(u32x4, (piece & 1) ? f.lo : f.hi);
  }
  reinterpret_cast<u32x4*>(out)[u] = o;
}

inline bool conv3x3_shape_ok(int Cin, int N) { return Cin == 256 && N == 256; }
inline long long conv3x3_units(int Cin) { return (long long)(9 * Cin / 16 + CONV_PAD_STAGES) * 16 * 64 + 128; }

}  // namespace

extern "C" int64_t tce_conv3x3_packed_bytes(int32_t Cin, int32_t N) { return conv3x3_shape_ok(Cin, N) ? conv3x3_units(Cin) * 16 : -1; }

extern "C" int tce_conv3x3_pack_f32(const float* w, void* packed, int32_t Cin, int32_t N, tceStream stream) {
  TCE_CHECK_ARG(conv3x3_shape_ok(Cin, N), "tce_conv3x3_pack_f32: unsupported shape Cin=%d N=%d (256 -> 256)", Cin, N);
  TCE_CHECK_ARG(w && packed && tce_aligned16(packed), "tce_conv3x3_pack_f32: null / misaligned pointer");
  const long long units = conv3x3_units(Cin);
  hipLaunchKernelGGL(conv3x3_pack_kernel, dim3(tce_cdiv(units, 256)), dim3(256), 0, (hipStream_t)stream, w,
                     (unsigned char*)packed, Cin, units, tce_gemm_single_pass());
  TCE_CHECK_LAUNCH("tce_conv3x3_pack_f32");
  return TCE_OK;
}

static int g_conv3_waves = 0;
extern "C" int tce_debug_conv3x3_set_waves(int32_t waves) {
  TCE_CHECK_ARG(waves == 0 || waves == 4 || waves == 8, "tce_debug_conv3x3_set_waves: 0 (automatic), 4 or 8");
  g_conv3_waves = waves;
  return TCE_OK;
}

// Launch plan of the 3x3 convolution (pure: tce_conv3x3_split_ws_floats / _pieces export it).  Forms, in units of a narrow round x 4:
// 256-pixel (8-wave) workgroups halve the weight bytes per pixel; a round of them takes 1.75 x a round of 128-pixel workgroups
// (measured, tools/conv3_bench.py: 128400 px 508 -> 444 us, 72000 px 333 -> 337, 18000 px 100 -> 142): taken when the rounds of
// 256 workgroups that way cost less -- config 5 and clip groups, not the single config-2 clip.  Mixed form (round 5): full rounds of
// 256-pixel workgroups, then the REMAINDER as 128-pixel workgroups (they run one wave per SIMD: a round of them costs 1 against 1.75).
// 72000 px: 256 wide workgroups + 51 narrow ones = 1.75 + 1 rounds against 3 narrow rounds (or 2 x 1.75 wide ones).
// Split (round 6, tce_conv3x3_split_f32 only): a narrow launch that fills less than one round -- the mixed form's remainder, or a
// single sub-round launch such as 18000 px -- walks the same 144 k-steps per workgroup whatever its size, so it is issued as `pieces`
// workgroups per block, each a contiguous run of the K walk (conv3x3_piece_iter), and a reduce pass adds the fp32 partials and the bias.
struct Conv3Plan {
  int wide = 4;          // form of the un-split part: 8 = 256-pixel workgroups, 4 = 128-pixel ones
  int full8 = 0;         // mixed form: workgroups of the wide launch over pixels [0, 65536 * full8 / 256)
  int m_narrow = 0;      // first pixel of the narrow launch (mixed form), else 0
  int nb = 0;            // 128-pixel blocks of the narrow launch
  int pieces = 1;        // > 1: the narrow launch is split
  long long ws_floats = 0;
};
inline Conv3Plan conv3x3_plan(const int M, const int cus, const int single, const int force_waves, const int split, const int force_pieces) {
  Conv3Plan pl;
  const int r4 = tce_cdiv(tce_cdiv(M, 128), cus), r8 = tce_cdiv(tce_cdiv(M, 256), cus);
  const int full8 = tce_cdiv(M, 256) / cus;  // complete rounds of wide workgroups
  const int rem_px = M - full8 * 256 * cus;
  const int mixed4 = 7 * full8 + 4 * tce_cdiv(tce_cdiv(rem_px, 128), cus);
  if (!force_waves && !single && full8 >= 1 && rem_px > 0 && mixed4 < 4 * r4 && mixed4 < 7 * r8) {
    pl.full8 = full8 * cus;
    pl.m_narrow = full8 * 256 * cus;
  } else {
    pl.wide = force_waves ? force_waves : (4 * r4 > 7 * r8 ? 8 : 4);
    if (single) pl.wide = 4;
    if (pl.wide == 8) return pl;
  }
  pl.nb = tce_cdiv(M - pl.m_narrow, 128);
  if (!split || single || pl.nb >= cus) return pl;
  // cost in iterations of one workgroup's walk (12 for an un-split block): rounds x (longest piece + OVH), plus the reduce pass --
  // its fp32 traffic ((pieces + 1) x 1 KiB per pixel) at RED_BPI bytes per iteration-time, and LAUNCH for the extra launch.
  // Pieces are capped at two rounds of workgroups (this bounds the workspace: tce_conv3x3_split_ws_floats).
  const double OVH = 0.5, LAUNCH = 0.3, RED_BPI = 8.0 * (3u << 20);  // ~3.3 TB/s over one iteration (~7.5 us)
  const long long px = M - pl.m_narrow;
  auto cost = [&](int p) {
    const double walk = (double)tce_cdiv((long long)pl.nb * p, cus) * (tce_cdiv(CONV_ITERS, p) + OVH);
    return p == 1 ? walk : walk + LAUNCH + (double)(p + 1) * px * 1024.0 / RED_BPI;
  };
  int best = 1;
  for (int p = 2; p <= 6; ++p)
    if ((long long)pl.nb * p <= 2ll * cus && cost(p) < cost(best)) best = p;
  if (force_pieces > 0) best = force_pieces;
  if (best > 1) {
    pl.pieces = best;
    pl.ws_floats = (long long)best * px * 256;
  }
  return pl;
}

static int g_conv3_pieces = 0;
extern "C" int tce_debug_conv3x3_set_pieces(int32_t pieces) {
  TCE_CHECK_ARG(pieces >= 0 && pieces <= CONV_ITERS, "tce_debug_conv3x3_set_pieces: 0 (automatic) .. 12");
  g_conv3_pieces = pieces;
  return TCE_OK;
}

static int conv3_force_waves() {
  static const int env_force = []() { const char* e = getenv("TCE_CONV3_WAVES"); return e ? atoi(e) : 0; }();
  return g_conv3_waves ? g_conv3_waves : env_force;
}

static Conv3Plan conv3x3_plan_for(const int M, const bool split) {
  return conv3x3_plan(M, tce_cu_count(), tce_gemm_single_pass(), conv3_force_waves(), split, g_conv3_pieces);
}

// Workspace of tce_conv3x3_split_f32 (floats; 0 = that call splits nothing and needs none) and its piece count.
extern "C" int64_t tce_conv3x3_split_ws_floats(int32_t M, int32_t Cin, int32_t N) {
  return conv3x3_shape_ok(Cin, N) && M > 0 ? conv3x3_plan_for(M, true).ws_floats : 0;
}
extern "C" int32_t tce_conv3x3_split_pieces(int32_t M, int32_t Cin, int32_t N) {
  return conv3x3_shape_ok(Cin, N) && M > 0 ? conv3x3_plan_for(M, true).pieces : 0;
}
// First k-step of piece s of `pieces` (s = pieces: the end of the walk, 9 * 256 / 16 = 144).
extern "C" int32_t tce_conv3x3_split_kstep(int32_t pieces, int32_t s) {
  return pieces >= 1 && pieces <= CONV_ITERS && s >= 0 && s <= pieces ? 12 * conv3x3_piece_iter(pieces, s) : -1;
}

static int conv3x3_launch(const float* x, int64_t ldx, const void* packed, const float* bias, float* out, int64_t ldo, int32_t T,
                          int32_t H, int32_t W, int32_t Cin, int32_t N, float* ws, int64_t ws_floats, const bool split, tceStream stream,
                          const char* name) {
  TCE_CHECK_ARG(conv3x3_shape_ok(Cin, N), "%s: unsupported shape Cin=%d N=%d (256 -> 256)", name, Cin, N);
  TCE_CHECK_ARG(x && packed && out && T > 0 && H > 0 && W > 0 && (long long)T * H * W < (1ll << 31),
                "%s: null pointer or bad sizes", name);
  TCE_CHECK_ARG(ldx >= Cin && ldx % 4 == 0 && ldo >= N && ldo % 4 == 0, "%s: bad row pitch", name);
  TCE_CHECK_ARG(tce_aligned16(x) && tce_aligned16(out) && tce_aligned16(packed) && (!bias || tce_aligned16(bias)),
                "%s: pointers must be 16-byte aligned", name);
  ConvArgs a;
  a.x = x; a.wpk = (const unsigned char*)packed; a.bias = bias; a.out = out;
  a.ldx = ldx; a.ldo = ldo; a.H = H; a.W = W; a.M = T * H * W;
  a.range_flag = tce_range_flag(); a.single = tce_gemm_single_pass();
  a.m_off = 0; a.nb = 0; a.pieces = 1; a.ws = nullptr;
  hipStream_t s = (hipStream_t)stream;
  const Conv3Plan pl = conv3x3_plan_for(a.M, split);
  if (pl.pieces > 1)
    TCE_CHECK_ARG(ws && tce_aligned16(ws) && ws_floats >= pl.ws_floats,
                  "%s: workspace of %lld floats needed (tce_conv3x3_split_ws_floats), %lld given", name, pl.ws_floats, (long long)ws_floats);
  if (pl.full8) hipLaunchKernelGGL((conv3x3_kernel<256, false, 8>), dim3(pl.full8), dim3(512), 0, s, a);
  a.m_off = pl.m_narrow;
  if (pl.wide == 8) hipLaunchKernelGGL((conv3x3_kernel<256, false, 8>), dim3(tce_cdiv(a.M, 256)), dim3(512), 0, s, a);
  else if (a.single) hipLaunchKernelGGL((conv3x3_kernel<256, true>), dim3(pl.nb), dim3(256), 0, s, a);
  else if (pl.pieces == 1) hipLaunchKernelGGL((conv3x3_kernel<256, false>), dim3(pl.nb), dim3(256), 0, s, a);
  else {
    a.nb = pl.nb; a.pieces = pl.pieces; a.ws = ws;
    hipLaunchKernelGGL((conv3x3_kernel<256, false, 4, true>), dim3(pl.nb * pl.pieces), dim3(256), 0, s, a);
    const int rows = a.M - a.m_off;
    hipLaunchKernelGGL(conv3x3_reduce_kernel, dim3(std::min(tce_cdiv((long long)rows * 64, 256), 8 * tce_cu_count())), dim3(256), 0, s,
                       (const float*)ws, pl.pieces, rows, bias, out, ldo, a.m_off, a.range_flag);
  }
  TCE_CHECK_LAUNCH(name);
  return TCE_OK;
}

// TCE_CONV3_WAVES=4|8 / tce_debug_conv3x3_set_waves force one form.
extern "C" int tce_conv3x3_f32(const float* x, int64_t ldx, const void* packed, const float* bias, float* out, int64_t ldo,
                               int32_t T, int32_t H, int32_t W, int32_t Cin, int32_t N, tceStream stream) {
  return conv3x3_launch(x, ldx, packed, bias, out, ldo, T, H, W, Cin, N, nullptr, 0, false, stream, "tce_conv3x3_f32");
}

// As tce_conv3x3_f32, with a sub-round narrow launch split over the K walk: ws = tce_conv3x3_split_ws_floats(M) floats (16-byte
// aligned; unused when that is 0), not shared with a launch that may run concurrently.  Bit-identical run to run.
extern "C" int tce_conv3x3_split_f32(const float* x, int64_t ldx, const void* packed, const float* bias, float* out, int64_t ldo,
                                     int32_t T, int32_t H, int32_t W, int32_t Cin, int32_t N, float* ws, int64_t ws_floats,
                                     tceStream stream) {
  return conv3x3_launch(x, ldx, packed, bias, out, ldo, T, H, W, Cin, N, ws, ws_floats, true, stream, "tce_conv3x3_split_f32");
}
