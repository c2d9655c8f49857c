// Scoring-stage kernels (include/tce_rvos_score.h): the six integer counts per (object, frame) behind Ref-DAVIS J&F.
#include "common.h"
#include "../../include/tce_rvos_score.h"

namespace {

// A workgroup owns a tile of JF_TH rows x 64 columns of one frame: the tile's columns are ONE 64-bit word of a bit row.  Around
// it, a halo of `radius` rows above and below and of one word (64 >= TCE_JF_MAX_RADIUS columns) to the left and to the right, so a
// bit row of the workgroup is three words: word 0 = columns x0-64 .. x0-1, word 1 = the tile, word 2 = x0+64 .. x0+127.
constexpr int JF_TH = 32, JF_THREADS = 256, JF_WAVES = JF_THREADS / 64, JF_ROW = 192;
static_assert(TCE_JF_MAX_RADIUS < 64, "the halo is one word wide");

// LDS of a workgroup at `radius` (RB = JF_TH + 2*radius rows of boundary bits, RL = RB + 1 rows of labels and object bits: the
// boundary of a row needs the row below it): S [2][RL][3] and B [2][RB][3] 64-bit words, the half-widths [radius+1], the per-wave
// label sets [JF_WAVES] and the per-wave sums [JF_WAVES][6] as ints, the label bytes [2][RL][JF_ROW].  54.5 KB at radius 40.
__host__ __device__ inline int jf_hw_ints(int R) { return (R + 2) & ~1; }
inline size_t jf_lds_bytes(int R) {
  const int RB = JF_TH + 2 * R, RL = RB + 1;
  return (size_t)(2 * RL * 3 + 2 * RB * 3) * 8 + (size_t)(jf_hw_ints(R) + JF_WAVES + JF_WAVES * TCE_JF_COUNTS) * 4 + (size_t)2 * RL * JF_ROW;
}

// bits a .. b of a word (clipped to 0 .. 63; none when the range is empty)
__device__ __forceinline__ uint64_t jf_bits(int a, int b) {
  a = max(a, 0);
  b = min(b, 63);
  return a > b ? 0ull : (~0ull >> (63 - (b - a))) << a;
}

// The matches of one tile row, both ways in one walk: how many boundary pixels of the prediction (bp, word 1 of bit row ry of Bp)
// have a boundary pixel of the annotation (Ba) within the disk, and the reverse.  Lane p is pixel p of the word.  Rows ry - dy and
// ry + dy share their half-width, so their words are OR-ed and the walk is over |dy| = 0 .. R, ending once every pixel of both
// words is matched.  Bp / Ba are B [RB][3]; rows ry - R .. ry + R exist for every tile row (ry = R + r).
__device__ __forceinline__ void jf_match(const uint64_t bp, const uint64_t ba, const uint64_t* __restrict__ Bp,
                                         const uint64_t* __restrict__ Ba, const int ry, const int R, const int* __restrict__ hwt,
                                         const int lane, int& fg_match, int& gt_match) {
  if ((bp | ba) == 0ull) return;
  const bool wp = (bp >> lane) & 1ull, wa = (ba >> lane) & 1ull;
  bool fp = false, fa = false;
  for (int ady = 0; ady <= R; ++ady) {
    if (!__any((wp && !fp) || (wa && !fa))) break;
    const uint64_t* __restrict__ pu = Bp + (ry - ady) * 3;
    const uint64_t* __restrict__ pd = Bp + (ry + ady) * 3;
    const uint64_t* __restrict__ au = Ba + (ry - ady) * 3;
    const uint64_t* __restrict__ ad = Ba + (ry + ady) * 3;
    const uint64_t p0 = pu[0] | pd[0], p1 = pu[1] | pd[1], p2 = pu[2] | pd[2];
    const uint64_t a0 = au[0] | ad[0], a1 = au[1] | ad[1], a2 = au[2] | ad[2];
    const int hw = hwt[ady], lo = 64 + lane - hw, hi = 64 + lane + hw;
    const uint64_t m0 = jf_bits(lo, hi), m1 = jf_bits(lo - 64, hi - 64), m2 = jf_bits(lo - 128, hi - 128);
    fp = fp || ((a0 & m0) | (a1 & m1) | (a2 & m2)) != 0ull;
    fa = fa || ((p0 & m0) | (p1 & m1) | (p2 & m2)) != 0ull;
  }
  fg_match += __popcll(__ballot(wp && fp));
  gt_match += __popcll(__ballot(wa && fa));
}

// which of the 4 bytes of d equal the byte repeated in pat: bits 0 .. 3 (exact per byte: no carry crosses a byte)
__device__ __forceinline__ uint32_t jf_eq4(const uint32_t d, const uint32_t pat) {
  const uint32_t x = d ^ pat, t = ((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x;  // bit 7 of a byte of t is 0 iff that byte of x is 0
  return ((((~t & 0x80808080u) >> 7) * 0x01020408u) >> 24) & 0xFu;
}

__global__ void __launch_bounds__(JF_THREADS) jf_tile_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt,
                                                             int* __restrict__ ws, const int T, const int n, const int H, const int W,
                                                             const int R, const int tilesX, const int tiles) {
  extern __shared__ uint64_t jf_lds[];
  const int RB = JF_TH + 2 * R, RL = RB + 1;
  uint64_t* S = jf_lds;                // [2][RL][3]: bit = the pixel carries the label of the object in hand
  uint64_t* B = S + 2 * RL * 3;        // [2][RB][3]: bit = boundary pixel (_seg2bmap), 0 beyond the plane
  int* hwt = reinterpret_cast<int*>(B + 2 * RB * 3);
  int* seen = hwt + jf_hw_ints(R);
  int* red = seen + JF_WAVES;
  uint8_t* lab = reinterpret_cast<uint8_t*>(red + JF_WAVES * TCE_JF_COUNTS);  // [2][RL][JF_ROW], 0 beyond the plane
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t = blockIdx.x / tiles, tile = blockIdx.x - t * tiles;
  const int ty = tile / tilesX, tx = tile - ty * tilesX;
  const int x0 = tx * 64, y0 = ty * JF_TH;

  // labels: row ry <-> y = y0 - R + ry, column c <-> x = x0 - 64 + c.  Only columns 64 - R .. 129 + R can reach a count (a window
  // ends R columns from the tile, and a boundary bit looks one column to the right); everything else stays 0.
  for (int i = tid; i < 2 * RL * (JF_ROW / 8); i += JF_THREADS) reinterpret_cast<uint64_t*>(lab)[i] = 0ull;
  __syncthreads();
  // A row's bytes are fetched as the ALIGNED dwords that hold them, a dword per lane (the planes sit at any address and W is any
  // number, so the alignment differs from row to row); a dword that is not wholly inside the stack -- only the first and the last
  // one of the whole [T,H,W] stack can be -- is fetched byte by byte.  Up to (66 + 2R + 6) / 4 dwords per row: two rows per
  // wavefront pass while that is at most 32 (R <= 28), one otherwise.
  const long long total = (long long)T * H * W, plane = (long long)t * H * W;
  const int xa = max(0, x0 - R), xb = min(W, x0 + 66 + R);  // the row's columns xa .. xb - 1
  const int two = R <= 28, j = two ? (lane & 31) : lane, sub = two ? (lane >> 5) : 0;
  unsigned labels = 0u;  // bit k: label k + 1 occurs among the bytes this lane loaded
  for (int i0 = wave * (1 + two); i0 < 2 * RL; i0 += JF_WAVES * (1 + two)) {
    const int i = i0 + sub, p = i >= RL, ry = i - p * RL, y = y0 - R + ry;
    if (i >= 2 * RL || y < 0 || y >= H) continue;
    const uint8_t* __restrict__ base = p ? gt : pred;
    const long long f0 = plane + (long long)y * W + xa;            // the row's first byte, as an index of the stack
    const int lead = (int)((reinterpret_cast<uintptr_t>(base) + (uintptr_t)f0) & 3u);
    if (4 * j >= lead + (xb - xa)) continue;
    const long long f = f0 - lead + 4 * j;                         // this lane's dword: bytes f .. f + 3 of the stack
    uint32_t d = 0u;
    if (f >= 0 && f + 4 <= total) {
      d = *reinterpret_cast<const uint32_t*>(base + f);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (f + q >= 0 && f + q < total) d |= (uint32_t)base[f + q] << (8 * q);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int x = xa - lead + 4 * j + q;
      if (x >= xa && x < xb) {
        const uint32_t v = (d >> (8 * q)) & 0xFFu;
        lab[i * JF_ROW + (x - x0 + 64)] = (uint8_t)v;
        if (v >= 1u && v <= (uint32_t)TCE_JF_MAX_OBJS) labels |= 1u << (v - 1u);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) labels |= (unsigned)__shfl_xor((int)labels, o, 64);
  if (lane == 0) seen[wave] = (int)labels;
  if (tid <= R) {  // isqrt(R^2 - dy^2)
    const int v = R * R - tid * tid;
    int h = (int)sqrtf((float)v);
    while (h * h > v) --h;
    while ((h + 1) * (h + 1) <= v) ++h;
    hwt[tid] = h;
  }
  __syncthreads();
  labels = 0u;
#pragma unroll
  for (int v = 0; v < JF_WAVES; ++v) labels |= (unsigned)seen[v];

  for (int k = 0; k < n; ++k) {
    if (!((labels >> k) & 1u)) {  // the object is in neither map anywhere near this tile (most tiles of most objects): six zeros
      if (tid < TCE_JF_COUNTS) ws[(((long long)k * T + t) * tiles + tile) * TCE_JF_COUNTS + tid] = 0;
      continue;
    }
    // object bits: a thread per word, 8 labels per LDS read (word i is bytes 64 i .. 64 i + 63 of lab); the reads of neighbouring
    // threads are 64 bytes apart, so each starts at another of its word's eight 8-byte pieces
    const uint32_t pat = 0x01010101u * (uint32_t)(k + 1);
    for (int i = tid; i < 2 * RL * 3; i += JF_THREADS) {
      const uint2* __restrict__ src = reinterpret_cast<const uint2*>(lab + i * 64);
      uint64_t word = 0ull;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int piece = (q + (tid >> 2)) & 7;
        const uint2 d = src[piece];
        word |= (uint64_t)(jf_eq4(d.x, pat) | (jf_eq4(d.y, pat) << 4)) << (8 * piece);
      }
      S[i] = word;
    }
    __syncthreads();
    // boundary bits: a thread per word
    for (int i = tid; i < 2 * RB * 3; i += JF_THREADS) {
      const int p = i >= RB * 3, rem = i - p * RB * 3, ry = rem / 3, w = rem - ry * 3, y = y0 - R + ry;
      uint64_t b = 0ull;
      if (y >= 0 && y < H) {
        const uint64_t* __restrict__ s0 = S + (p * RL + ry) * 3;
        const uint64_t* __restrict__ s1 = s0 + 3;
        const uint64_t s = s0[w], e = (s >> 1) | (w < 2 ? s0[w + 1] << 63 : 0ull);
        const uint64_t sd = s1[w], se = (sd >> 1) | (w < 2 ? s1[w + 1] << 63 : 0ull);
        const bool last = y == H - 1;
        b = last ? (s ^ e) : ((s ^ e) | (s ^ sd) | (s ^ se));
        const int xs = x0 - 64 + 64 * w, lc = W - 1 - xs;  // lc: the bit of the plane's last column
        if (lc >= 0 && lc < 64) {
          const uint64_t lb = 1ull << lc;
          b = (b & ~lb) | (last ? 0ull : ((s ^ sd) & lb));
        }
        b &= jf_bits(-xs, lc);
      }
      B[i] = b;
    }
    __syncthreads();
    // counts: a wavefront per tile row; every lane holds the same sums
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0, c5 = 0;
    for (int r = wave; r < JF_TH && y0 + r < H; r += JF_WAVES) {
      const int ry = r + R;
      const uint64_t sp = S[ry * 3 + 1], sa = S[(RL + ry) * 3 + 1];
      const uint64_t bp = B[ry * 3 + 1], ba = B[(RB + ry) * 3 + 1];
      c0 += __popcll(sp & sa);
      c1 += __popcll(sp | sa);
      c2 += __popcll(bp);
      c3 += __popcll(ba);
      jf_match(bp, ba, B, B + RB * 3, ry, R, hwt, lane, c4, c5);
    }
    if (lane == 0) {
      int* q = red + wave * TCE_JF_COUNTS;
      q[0] = c0, q[1] = c1, q[2] = c2, q[3] = c3, q[4] = c4, q[5] = c5;
    }
    __syncthreads();  // ... and every wavefront is done with S and B of this object
    if (tid < TCE_JF_COUNTS) {
      int s = 0;
#pragma unroll
      for (int v = 0; v < JF_WAVES; ++v) s += red[v * TCE_JF_COUNTS + tid];
      ws[(((long long)k * T + t) * tiles + tile) * TCE_JF_COUNTS + tid] = s;
    }
  }
}

// counts[k,t,:] = the sum of the tiles' partial sums: a wavefront per (object, frame)
__global__ void __launch_bounds__(64) jf_reduce_kernel(const int* __restrict__ ws, int* __restrict__ counts, const int T, const int tiles) {
  const long long kt = (long long)blockIdx.y * T + blockIdx.x;
  const int* __restrict__ src = ws + kt * tiles * TCE_JF_COUNTS;
  int acc[TCE_JF_COUNTS] = {0, 0, 0, 0, 0, 0};
  for (int i = threadIdx.x; i < tiles; i += 64)
#pragma unroll
    for (int j = 0; j < TCE_JF_COUNTS; ++j) acc[j] += src[(long long)i * TCE_JF_COUNTS + j];
#pragma unroll
  for (int j = 0; j < TCE_JF_COUNTS; ++j)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc[j] += __shfl_xor(acc[j], o, 64);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < TCE_JF_COUNTS; ++j) counts[kt * TCE_JF_COUNTS + j] = acc[j];
  }
}

bool jf_extents_ok(int T, int n, int H, int W, int radius) {
  return T > 0 && H > 0 && W > 0 && n >= 1 && n <= TCE_JF_MAX_OBJS && radius >= 0 && radius <= TCE_JF_MAX_RADIUS &&
         (long long)T * H * W < (1ll << 31);
}

}  // namespace

extern "C" int64_t tce_jf_ws_bytes(int32_t T, int32_t n, int32_t H, int32_t W, int32_t radius) {
  if (!jf_extents_ok(T, n, H, W, radius)) return -1;
  const int64_t tiles = (int64_t)tce_cdiv(W, 64) * tce_cdiv(H, JF_TH);
  return (int64_t)n * T * tiles * TCE_JF_COUNTS * (int64_t)sizeof(int32_t);
}

extern "C" int tce_jf_counts_i32(const uint8_t* pred, const uint8_t* gt, int32_t* counts, void* ws, int32_t T, int32_t n, int32_t H,
                                 int32_t W, int32_t radius, tceStream stream) {
  TCE_CHECK_ARG(pred && gt && counts && ws, "tce_jf_counts_i32: null pointer");
  TCE_CHECK_ARG(T > 0 && H > 0 && W > 0, "tce_jf_counts_i32: non-positive extent");
  TCE_CHECK_ARG(n >= 1 && n <= TCE_JF_MAX_OBJS, "tce_jf_counts_i32: n = %d objects, 1 .. %d are supported", n, TCE_JF_MAX_OBJS);
  TCE_CHECK_ARG(radius >= 0 && radius <= TCE_JF_MAX_RADIUS, "tce_jf_counts_i32: radius %d, 0 .. %d are supported", radius,
                TCE_JF_MAX_RADIUS);
  TCE_CHECK_ARG((long long)T * H * W < (1ll << 31), "tce_jf_counts_i32: the label maps must stay below 2^31 elements");
  TCE_CHECK_ARG(((uintptr_t)ws & 7u) == 0 && ((uintptr_t)counts & 3u) == 0,
                "tce_jf_counts_i32: ws must be 8-byte aligned, counts 4-byte aligned");
  const int tilesX = tce_cdiv(W, 64), tiles = tilesX * tce_cdiv(H, JF_TH);  // T * tiles <= T*H*W < 2^31
  hipLaunchKernelGGL(jf_tile_kernel, dim3((unsigned)((long long)T * tiles)), dim3(JF_THREADS), jf_lds_bytes(radius), (hipStream_t)stream,
                     pred, gt, (int*)ws, T, n, H, W, radius, tilesX, tiles);
  hipLaunchKernelGGL(jf_reduce_kernel, dim3(T, n), dim3(64), 0, (hipStream_t)stream, (const int*)ws, counts, T, tiles);
  TCE_CHECK_LAUNCH("tce_jf_counts_i32");
  return TCE_OK;
}
