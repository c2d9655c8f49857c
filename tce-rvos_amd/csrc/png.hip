// PNG-writing stage kernels (csrc/tce_rvos_png.h, csrc/tce_rvos_png_dyn.h): the zlib stream of every uint8 output plane -- filter
// bytes, RLE-only deflate with the fixed Huffman code or, behind the second entry, with the cheaper of the fixed code and a code of
// the strip's own, Adler-32 -- in three launches.  Byte and bit kernels: bound by LDS traffic and barriers, not by arithmetic.
// RGB images (at the end of the file): a row filter chosen per row, then the second encoding over rows that are filtered already.
#include "common.h"
#include "../../include/tce_rvos_png.h"
#include "../../include/tce_rvos_vis.h"

namespace {

constexpr int PT = 256, PWAVES = PT / 64, PER = 8;  // a thread owns PER consecutive filtered bytes of a pass
static_assert(PT * PER == TCE_PNG_PASS, "pass length");
constexpr int REP = 4;                 // matches of length 258 per thread and sub-pass of a long run
constexpr int MATCH258_BITS = 13;      // symbol 285 (8 bits, 0xC5 -> 0xA3 least significant bit first) + distance code 0 (5 bits)
constexpr uint32_t MATCH258 = 0xA3u;
// The bit window.  It holds the bits behind the last whole dword flushed: at most 31 of them, the block header (3), head and tail of
// a carried run (9 + 36), and then EITHER the runs that lie inside a pass (at most 9 bits a byte: 18432) OR a sub-pass of
// PT * REP matches of length 258 (13312) OR the strip's end (7 + 3 + 7 + 32): below 18600 bits = 582 dwords.
constexpr int WIN_DW = 640;
static_assert(31 + 3 + 45 + 9 * TCE_PNG_PASS + 64 < 32 * (WIN_DW - 1) && 31 + 45 + PT * REP * MATCH258_BITS + 64 < 32 * (WIN_DW - 1), "window");
constexpr uint32_t ADLER = 65521u;

struct Tok {
  uint32_t v;  // the bits, first bit of the stream in bit 0
  int n;
};

// a Huffman code goes in most significant bit first
__device__ __forceinline__ uint32_t huff(const uint32_t code, const int n) { return __brev(code) >> (32 - n); }

__device__ __forceinline__ Tok lit_tok(const uint32_t b) {
  return b < 144u ? Tok{huff(0x30u + b, 8), 8} : Tok{huff(0x190u + (b - 144u), 9), 9};
}

// a match of length 3 .. 258 at distance 1: length symbol 257 + i of the largest base <= len (258: always i = 28), its extra bits
// least significant first, five zero bits of distance code 0.  Bases: 3 .. 10 one apart; from 11 on, four codes per extra-bit count
// e >= 1, spaced 2^e: with l = len - 3 >= 8, e = floor(log2 l) - 2 and the code within its group of four is (l >> e) & 3.
__device__ __forceinline__ Tok match_tok(const int len) {
  int i, e = 0;
  uint32_t x = 0u;
  if (len == 258) {
    i = 28;
  } else if (len < 11) {
    i = len - 3;
  } else {
    const int l = len - 3;
    e = 29 - __clz(l);
    i = 4 * e + 4 + ((l >> e) & 3);
    x = (uint32_t)l & ((1u << e) - 1u);
  }
  const int n = i < 23 ? 7 : 8;  // symbols 256 .. 279: 7 bits, x - 256; 280 .. 287: 8 bits, 0xC0 + (x - 280)
  const uint32_t code = i < 23 ? (uint32_t)(i + 1) : 0xC0u + (uint32_t)(i - 23);
  return Tok{huff(code, n) | (x << n), n + e + 5};
}

// what follows the matches of length 258 of a run of byte b: r < 261, r != 258 more bytes
template <class F>
__device__ __forceinline__ void run_tail(const uint32_t b, int r, F&& f) {
  if (r == 259 || r == 260) {
    f(match_tok(r - 3));
    r = 3;
  }
  if (r >= 3) {
    f(match_tok(r));
  } else {
    for (int k = 0; k < r; ++k) f(lit_tok(b));
  }
}

// every token of a run of L >= 1 bytes b (a run inside a pass: L <= TCE_PNG_PASS, a handful of tokens)
template <class F>
__device__ __forceinline__ void run_tokens(const uint32_t b, const int L, F&& f) {
  f(lit_tok(b));
  int r = L - 1;
  while (r >= 261 || r == 258) {
    f(Tok{MATCH258, MATCH258_BITS});
    r -= 258;
  }
  run_tail(b, r, f);
}

// ORs a token into the window at bit `at`: LDS atomics, so tokens of different threads may share a dword
__device__ __forceinline__ void put(uint32_t* win, const int at, const Tok t) {
  const unsigned long long v = (unsigned long long)t.v << (at & 31);
  if ((uint32_t)v) atomicOr(&win[at >> 5], (uint32_t)v);
  if ((uint32_t)(v >> 32)) atomicOr(&win[(at >> 5) + 1], (uint32_t)(v >> 32));
}

// the window's whole dwords go to the strip's workspace, the bits behind them (wb & 31) to the window's start.  Every thread calls it.
__device__ __forceinline__ void flush(uint32_t* win, uint32_t* __restrict__ out, long long& flushed, int& wb) {
  __syncthreads();  // every token is in
  const int nfull = wb >> 5;
  for (int i = threadIdx.x; i < nfull; i += PT) out[flushed + i] = win[i];
  const uint32_t part = win[nfull];
  __syncthreads();
  for (int i = threadIdx.x; i <= nfull; i += PT) win[i] = i == 0 ? part : 0u;
  __syncthreads();
  flushed += nfull;
  wb &= 31;
}

// A run that began in an earlier pass (or the strip's last run), of any length: the whole workgroup writes it.  b, L, wb, flushed
// are the same in every thread.  Thread 0 puts the literal and the tail; the matches of length 258 between them, one 13-bit
// pattern M times, go in sub-passes of PT * REP, the window flushed after each.
__device__ __forceinline__ void long_run(uint32_t* win, uint32_t* __restrict__ out, long long& flushed, int& wb, const uint32_t b,
                                         const int L) {
  const int r0 = L - 1;
  int M = 0, r = r0;
  if (r0 >= 258) {  // the loop "while r >= 261 or r == 258" in closed form: its last step leaves r0 % 258, legal unless that is 1 or 2
    const int q = r0 / 258, m = r0 - q * 258;
    M = (m == 0 || m >= 3) ? q : q - 1;
    r = r0 - 258 * M;
  }
  const Tok head = lit_tok(b);
  if (threadIdx.x == 0) put(win, wb, head);
  wb += head.n;
  for (int done = 0; done < M; done += PT * REP) {
    const int cnt = min(PT * REP, M - done);
#pragma unroll
    for (int k = 0; k < REP; ++k) {
      const int idx = threadIdx.x + k * PT;
      if (idx < cnt) put(win, wb + MATCH258_BITS * idx, Tok{MATCH258, MATCH258_BITS});
    }
    wb += MATCH258_BITS * cnt;
    flush(win, out, flushed, wb);
  }
  int at = wb;
  const bool t0 = threadIdx.x == 0;
  run_tail(b, r, [&](const Tok t) {
    if (t0) put(win, at, t);
    at += t.n;
  });
  wb = at;
}

// bytes f .. f+3 of the strip's ns plane bytes at b, (b + f) on a 4-byte boundary: one dword where all four are inside the strip,
// byte by byte (0 for those outside) at its two ends
__device__ __forceinline__ uint32_t strip_dword(const uint8_t* __restrict__ b, const int f, const int ns) {
  if (f >= 0 && f + 4 <= ns) return *reinterpret_cast<const uint32_t*>(b + f);
  uint32_t d = 0u;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (f + q >= 0 && f + q < ns) d |= (uint32_t)b[f + q] << (8 * q);
  return d;
}

// ws: meta [P*nstrips][2] = (bytes of the strip, Adler a | b << 16), offs [P*nstrips], then the strips' bytes, stride_dw dwords each
//
// First launch: a workgroup per (plane, strip).  The strip's filtered bytes f = 0 .. n-1 are walked in passes of TCE_PNG_PASS.  A run
// is written when its end is seen: at a BOUNDARY f (byte f differs from byte f-1), by the thread that owns byte f, and at the
// strip's end.  Carried from pass to pass, the same in every thread: open_start (the last boundary so far), open_val (the last byte
// so far), the window's bit count wb and the dwords flushed.
__global__ void __launch_bounds__(PT) png_strip_kernel(const uint8_t* __restrict__ planes, uint32_t* __restrict__ ws, const int H, const int W,
                                                       const int S, const int nstrips, const long long stride_dw, const int nonzero) {
  __shared__ uint32_t win[WIN_DW];
  __shared__ uint32_t raw[TCE_PNG_PASS / 4 + 4];  // the pass's plane bytes as the aligned dwords that hold them
  __shared__ int sc_max[PWAVES], sc_min[PWAVES], sc_sum[PWAVES];
  __shared__ uint32_t last_val;
  __shared__ uint32_t red[2][PWAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int strip = blockIdx.x, p = blockIdx.y;
  const long long sidx = (long long)p * nstrips + strip, nstr = (long long)gridDim.y * nstrips;
  const int row0 = strip * S, rows = min(S, H - row0), W1 = W + 1;
  const int n = rows * W1, ns = rows * W;  // filtered bytes, plane bytes
  const uint8_t* __restrict__ pl = planes + ((long long)p * H + row0) * W;
  uint32_t* __restrict__ out = ws + nstr * 3 + sidx * stride_dw;
  const uint8_t* rawb = reinterpret_cast<const uint8_t*>(raw);

  for (int i = tid; i < WIN_DW; i += PT) win[i] = 0u;
  __syncthreads();
  if (tid == 0) put(win, 0, Tok{2u, 3});  // BFINAL = 0, BTYPE = 01 (least significant bit first)
  int wb = 3, open_start = 0;
  long long flushed = 0;
  uint32_t open_val = 0u;
  unsigned long long sa = 0ull, sb = 0ull;  // sum of bytes; sum of byte * (n - f): both fit (n < 2^31, a thread owns n / PT bytes)

  for (int f0 = 0; f0 < n; f0 += TCE_PNG_PASS) {
    const int len = min(TCE_PNG_PASS, n - f0);
    // the pass's plane bytes q0 .. q1-1 (strip-relative): filtered byte f of row r = f / W1, column c = f % W1 > 0 is plane byte f - r - 1
    const int r0 = f0 / W1, c0 = f0 - r0 * W1, fe = f0 + len - 1, re = fe / W1;
    const int q0 = f0 - r0 - (c0 ? 1 : 0), q1 = fe - re;  // q1 - 1 = the last plane byte at or before fe
    const int lead = (int)((reinterpret_cast<uintptr_t>(pl) + (uintptr_t)q0) & 3u);
    for (int j = tid; 4 * j < lead + (q1 - q0); j += PT) raw[j] = strip_dword(pl, q0 - lead + 4 * j, ns);
    __syncthreads();

    // the thread's bytes, its boundaries, its share of the Adler sums
    const int f = f0 + tid * PER;
    uint32_t v[PER + 1];  // v[0]: the byte before the thread's own, v[j + 1]: its byte j
    uint32_t bmask = 0u;
    v[0] = open_val;
    if (f < f0 + len) {
      int r = f / W1, c = f - r * W1;
      auto fbyte = [&](const int ff, const int rr, const int cc) -> uint32_t {
        if (cc == 0) return 0u;
        const uint32_t x = rawb[lead + (ff - rr - 1 - q0)];
        return nonzero ? (x ? (uint32_t)nonzero : 0u) : x;
      };
      if (tid > 0) v[0] = c > 0 ? fbyte(f - 1, r, c - 1) : fbyte(f - 1, r - 1, W);  // (tid > 0: f - 1 >= f0 is in this pass)
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        v[j + 1] = 0u;
        if (f + j < f0 + len) {
          v[j + 1] = fbyte(f + j, r, c);
          if (f + j > 0 && v[j + 1] != v[j]) bmask |= 1u << j;
          sa += v[j + 1];
          sb += (unsigned long long)v[j + 1] * (unsigned)(n - (f + j));
          if (f + j == fe) last_val = v[j + 1];
          if (++c == W1) {
            c = 0;
            ++r;
          }
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < PER; ++j) v[j + 1] = 0u;
    }
    const int lastb = bmask ? f + (31 - __clz(bmask)) : -1, firstb = bmask ? f + (__ffs(bmask) - 1) : 0x7fffffff;

    // the boundary before the thread's bytes (exclusive max-scan, starting from open_start) and the pass's first boundary
    int sm = lastb, mn = firstb;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int a = __shfl_up(sm, o, 64);
      if (lane >= o) sm = max(sm, a);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mn = min(mn, __shfl_xor(mn, o, 64));
    if (lane == 63) sc_max[wave] = sm;
    if (lane == 0) sc_min[wave] = mn;
    __syncthreads();
    int s_in = __shfl_up(sm, 1, 64);
    if (lane == 0) s_in = -1;
    s_in = max(s_in, open_start);
    for (int k = 0; k < wave; ++k) s_in = max(s_in, sc_max[k]);
    int new_open = open_start;
    for (int k = 0; k < PWAVES; ++k) new_open = max(new_open, sc_max[k]);
    const int first = min(min(sc_min[0], sc_min[1]), min(sc_min[2], sc_min[3]));

    // the run carried into this pass ends at the pass's first boundary
    if (f0 > 0 && first != 0x7fffffff) long_run(win, out, flushed, wb, open_val, first - open_start);

    // the runs inside the pass: bit counts, their prefix sum, the bits
    int bits = 0;
    {
      int s = s_in;
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        if (bmask & (1u << j)) {
          if (s >= f0) run_tokens(v[j], f + j - s, [&](const Tok t) { bits += t.n; });
          s = f + j;
        }
      }
    }
    int sum = bits;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int a = __shfl_up(sum, o, 64);
      if (lane >= o) sum += a;
    }
    if (lane == 63) sc_sum[wave] = sum;
    __syncthreads();  // (also: last_val is in)
    int at = wb + sum - bits, total = 0;
    for (int k = 0; k < PWAVES; ++k) {
      if (k < wave) at += sc_sum[k];
      total += sc_sum[k];
    }
    {
      int s = s_in;
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        if (bmask & (1u << j)) {
          if (s >= f0)
            run_tokens(v[j], f + j - s, [&](const Tok t) {
              put(win, at, t);
              at += t.n;
            });
          s = f + j;
        }
      }
    }
    wb += total;
    open_start = new_open;
    open_val = last_val;
    flush(win, out, flushed, wb);  // its barriers also protect raw, last_val and the scan words for the next pass
  }

  // the last run, end of block, a stored-block header, zero bits to the byte boundary, 00 00 FF FF
  long_run(win, out, flushed, wb, open_val, n - open_start);
  wb = (wb + 7 + 3 + 7) & ~7;
  if (tid == 0) put(win, wb + 16, Tok{0xFFFFu, 16});
  wb += 32;
  __syncthreads();
  const int ndw = (wb + 31) >> 5;
  for (int i = tid; i < ndw; i += PT) out[flushed + i] = win[i];

  // Adler pair of the strip's filtered bytes: a = 1 + sum of bytes, b = n + sum of byte_f * (n - f), mod 65521
  uint32_t ra = (uint32_t)(sa % ADLER), rb = (uint32_t)(sb % ADLER);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ra += (uint32_t)__shfl_xor((int)ra, o, 64);  // 64 * 65520 < 2^32
    rb += (uint32_t)__shfl_xor((int)rb, o, 64);
  }
  if (lane == 0) {
    red[0][wave] = ra;
    red[1][wave] = rb;
  }
  __syncthreads();
  if (tid == 0) {
    const uint32_t a = (1u + red[0][0] + red[0][1] + red[0][2] + red[0][3]) % ADLER;
    const uint32_t b = ((uint32_t)(n % (int)ADLER) + red[1][0] + red[1][1] + red[1][2] + red[1][3]) % ADLER;
    ws[sidx * 2] = (uint32_t)(flushed * 4 + (wb >> 3));
    ws[sidx * 2 + 1] = a | (b << 16);
  }
}

// Second launch: a workgroup per plane.  Offsets of the strips (2 + the exclusive scan of their byte counts), the Adler pair of the
// whole plane, the header, the final block, the trailer, nbytes[p].  The pairs combine in strip order as
//   a = 1 + sum_s (a_s - 1),  b = sum_s b_s + sum_s (a_s - 1) * (filtered bytes behind strip s)      (mod 65521)
// which is the rule (a1 + a2 - 1, b1 + b2 + len(B) * (a1 - 1)) applied from the left: a sum, so no scan is needed for it.
__global__ void __launch_bounds__(PT) png_plane_kernel(uint32_t* __restrict__ ws, uint8_t* __restrict__ streams, int* __restrict__ nbytes,
                                                       const int H, const int W, const int S, const int nstrips, const long long bound) {
  __shared__ uint32_t sc[PWAVES];
  __shared__ uint32_t red[2][PWAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p = blockIdx.x;
  const long long nstr = (long long)gridDim.x * nstrips, base = (long long)p * nstrips;
  const uint32_t* __restrict__ meta = ws + base * 2;
  uint32_t* __restrict__ offs = ws + nstr * 2 + base;
  const long long ntot = (long long)H * (W + 1);
  uint32_t carry = 2u;                // bytes in front of the strip: below 2^31 (tce_png_stream_bound)
  unsigned long long sa = 0ull, sb = 0ull;  // at most nstrips / PT terms below 2^17: no overflow
  for (int s0 = 0; s0 < nstrips; s0 += PT) {
    const int s = s0 + tid;
    uint32_t nb = 0u;
    if (s < nstrips) {
      nb = meta[2 * (long long)s];
      const uint32_t ad = meta[2 * (long long)s + 1];
      const uint32_t a1 = ((ad & 0xFFFFu) + ADLER - 1u) % ADLER;  // a_s - 1
      const long long end = min((long long)(s + 1) * S, (long long)H) * (W + 1);
      sa += a1;
      sb += (ad >> 16) + (a1 * (uint32_t)((ntot - end) % ADLER)) % ADLER;  // 65520^2 < 2^32
    }
    uint32_t sum = nb;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t a = (uint32_t)__shfl_up((int)sum, o, 64);
      if (lane >= o) sum += a;
    }
    __syncthreads();  // the readers of sc of the pass before are done
    if (lane == 63) sc[wave] = sum;
    __syncthreads();
    uint32_t at = carry + sum - nb;
    for (int k = 0; k < wave; ++k) at += sc[k];
    if (s < nstrips) offs[s] = at;
    carry += sc[0] + sc[1] + sc[2] + sc[3];
  }
  uint32_t ra = (uint32_t)(sa % ADLER), rb = (uint32_t)(sb % ADLER);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ra += (uint32_t)__shfl_xor((int)ra, o, 64);
    rb += (uint32_t)__shfl_xor((int)rb, o, 64);
  }
  if (lane == 0) {
    red[0][wave] = ra;
    red[1][wave] = rb;
  }
  __syncthreads();
  if (tid == 0) {
    const uint32_t a = (1u + red[0][0] + red[0][1] + red[0][2] + red[0][3]) % ADLER;
    const uint32_t b = (red[1][0] + red[1][1] + red[1][2] + red[1][3]) % ADLER;
    uint8_t* __restrict__ row = streams + (long long)p * bound;
    row[0] = 0x78;
    row[1] = 0x01;
    uint8_t* __restrict__ t = row + carry;
    t[0] = 0x03;  // BFINAL = 1, BTYPE = 01, symbol 256 (seven zero bits), zero bits to the byte boundary
    t[1] = 0x00;
    t[2] = (uint8_t)(b >> 8);
    t[3] = (uint8_t)b;
    t[4] = (uint8_t)(a >> 8);
    t[5] = (uint8_t)a;
    nbytes[p] = (int)(carry + 6u);
  }
}

// Third launch: a workgroup per (plane, strip) copies the strip's bytes to their place.  A thread owns an ALIGNED dword of the
// destination (the row of streams starts at any address, the offset is any number); its four bytes come out of the two workspace
// dwords that hold them.  The strip's first and last dword go byte by byte.
__global__ void __launch_bounds__(PT) png_copy_kernel(const uint32_t* __restrict__ ws, uint8_t* __restrict__ streams, const int nstrips,
                                                      const long long stride_dw, const long long bound) {
  const int strip = blockIdx.x, p = blockIdx.y;
  const long long sidx = (long long)p * nstrips + strip, nstr = (long long)gridDim.y * nstrips;
  const int nb = (int)ws[sidx * 2];
  const uint32_t* __restrict__ src = ws + nstr * 3 + sidx * stride_dw;
  uint8_t* __restrict__ dst = streams + (long long)p * bound + ws[nstr * 2 + sidx];
  const int shift = (int)(reinterpret_cast<uintptr_t>(dst) & 3u);
  for (int g = threadIdx.x; 4 * g - shift < nb; g += PT) {
    const int k0 = 4 * g - shift;
    if (k0 >= 0 && k0 + 4 <= nb) {
      const int a = k0 >> 2, sh = (k0 & 3) * 8;
      uint32_t d = src[a];
      if (sh) d = (d >> sh) | (src[a + 1] << (32 - sh));  // byte 4 (a + 1) <= k0 + 3 < nb: inside the strip
      *reinterpret_cast<uint32_t*>(dst + k0) = d;
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = k0 + q;
        if (k >= 0 && k < nb) dst[k] = (uint8_t)(src[k >> 2] >> ((k & 3) * 8));
      }
    }
  }
}

// ---------------------------------------------------------------------------------------- codes = "dynamic" (csrc/tce_rvos_png_dyn.h)
// The same strips, tokens, window and workspace; the strip's block is written with the fixed code or with a code of its own,
// whichever takes fewer bits.  A workgroup walks its strip twice: (a) counts the tokens, (b) builds the code and decides, (c) emits.
constexpr int NLL = 286, NTAB = 288, NCL = 19;  // literal/length symbols in use; entries of the table (the fixed code has 288); code-length symbols
constexpr int DYN_CODE = 15;                    // bits of a literal/length code, at most
constexpr int DYN_MATCH = DYN_CODE + 5 + 5;     // of a match, at most: its length code, five extra bits, the distance code (1 or 5 bits)
constexpr int DYN_HEADER = 3 + 14 + 3 * NCL + 7 * (NLL + 1);  // BTYPE, HLIT/HDIST/HCLEN, the code-length code, a 7-bit symbol per length at most
// The bit window of this kernel.  Behind the at most 31 bits of the last flush it holds EITHER the block header (flushed at once)
// OR head and tail of a carried run and the runs inside a pass (15 bits a byte) OR a sub-pass of PT * REP matches of length 258
// OR the last run's head and tail, end-of-block and the strip's end.
constexpr int DWIN_DW = 1024;
static_assert(31 + DYN_HEADER < 32 * (DWIN_DW - 1) && 31 + DYN_CODE + 2 * DYN_MATCH + DYN_CODE * TCE_PNG_PASS < 32 * (DWIN_DW - 1) &&
                  31 + DYN_CODE + PT * REP * DYN_MATCH < 32 * (DWIN_DW - 1) && 31 + DYN_CODE + 2 * DYN_MATCH + DYN_CODE + 3 + 7 + 32 < 32 * (DWIN_DW - 1),
              "window of the dynamic kernel");
__constant__ uint8_t CL_ORDER[NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct DynShared {
  uint32_t win[DWIN_DW];
  uint32_t raw[TCE_PNG_PASS / 4 + 4];
  int sc_max[PWAVES], sc_min[PWAVES], sc_sum[PWAVES];
  uint32_t last_val;
  uint32_t red[2][PWAVES];
  uint32_t cnt[NTAB];            // tokens of the strip per literal/length symbol
  uint32_t extra, matches;       // their extra bits, their matches
  uint32_t tab[NTAB];            // the chosen code: bits << 16 | the code with the stream's first bit in bit 0
  int dbits, hbits, dynamic;     // bits of distance code 0; bits of the block header in the window; the choice
  // the code build
  uint32_t w[NTAB];              // the counts as halved so far
  uint32_t wgt[2 * NTAB];        // nodes: the leaves in sorted order, then the merged nodes in the order they are made
  uint16_t par[2 * NTAB], dep[2 * NTAB], order[NTAB];
  int nused, over, nlit;         // nlit: literal/length codes in the header (the highest symbol in use + 1)
  uint8_t len[NTAB], cllen[NCL + 1];
  uint32_t clcnt[NCL], cltab[NCL], clextra;
  uint32_t next[16];
};

struct Sym {
  int s;       // literal/length symbol
  uint32_t x;  // extra bits
  int e;
};

// match_tok's symbol
__device__ __forceinline__ Sym match_sym(const int len) {
  int i, e = 0;
  uint32_t x = 0u;
  if (len == 258) {
    i = 28;
  } else if (len < 11) {
    i = len - 3;
  } else {
    const int l = len - 3;
    e = 29 - __clz(l);
    i = 4 * e + 4 + ((l >> e) & 3);
    x = (uint32_t)l & ((1u << e) - 1u);
  }
  return Sym{257 + i, x, e};
}

template <class F>
__device__ __forceinline__ void run_tail_syms(const uint32_t b, int r, F&& f) {
  if (r == 259 || r == 260) {
    f(match_sym(r - 3));
    r = 3;
  }
  if (r >= 3) {
    f(match_sym(r));
  } else {
    for (int k = 0; k < r; ++k) f(Sym{(int)b, 0u, 0});
  }
}

template <class F>
__device__ __forceinline__ void run_syms(const uint32_t b, const int L, F&& f) {
  f(Sym{(int)b, 0u, 0});
  int r = L - 1;
  while (r >= 261 || r == 258) {
    f(Sym{285, 0u, 0});
    r -= 258;
  }
  run_tail_syms(b, r, f);
}

// a run of L bytes = a literal, M matches of length 258, a tail of r < 261, r != 258 bytes (long_run's closed form)
__device__ __forceinline__ void long_split(const int L, int& M, int& r) {
  const int r0 = L - 1;
  M = 0;
  r = r0;
  if (r0 >= 258) {
    const int q = r0 / 258, m = r0 - q * 258;
    M = (m == 0 || m >= 3) ? q : q - 1;
    r = r0 - 258 * M;
  }
}

__device__ __forceinline__ Tok sym_tok(const uint32_t* tab, const int dbits, const Sym y) {
  const uint32_t ent = tab[y.s];
  const int n = (int)(ent >> 16);
  return Tok{(ent & 0xFFFFu) | (y.x << n), n + y.e + (y.s > 256 ? dbits : 0)};  // the distance code is zero bits in either code
}

// long_run through the table
__device__ __forceinline__ void dyn_long_run(DynShared& S, uint32_t* __restrict__ out, long long& flushed, int& wb, const uint32_t b, const int L) {
  int M, r;
  long_split(L, M, r);
  const int dbits = S.dbits;
  const bool t0 = threadIdx.x == 0;
  const Tok head = sym_tok(S.tab, dbits, Sym{(int)b, 0u, 0});
  if (t0) put(S.win, wb, head);
  wb += head.n;
  const Tok m258 = sym_tok(S.tab, dbits, Sym{285, 0u, 0});  // (read only where M > 0: then symbol 285 has a code)
  for (int done = 0; done < M; done += PT * REP) {
    const int cnt = min(PT * REP, M - done);
#pragma unroll
    for (int k = 0; k < REP; ++k) {
      const int idx = threadIdx.x + k * PT;
      if (idx < cnt) put(S.win, wb + m258.n * idx, m258);
    }
    wb += m258.n * cnt;
    flush(S.win, out, flushed, wb);
  }
  int at = wb;
  run_tail_syms(b, r, [&](const Sym y) {
    const Tok t = sym_tok(S.tab, dbits, y);
    if (t0) put(S.win, at, t);
    at += t.n;
  });
  wb = at;
}

// One walk of the strip's n filtered bytes, png_strip_kernel's: EMIT = false counts every token into S.cnt / S.extra / S.matches
// (integer LDS atomics: the sums do not depend on their order), EMIT = true writes them through S.tab and sums the Adler pair.
// The byte source has two forms.  ROWS = false: pl is the strip's plane bytes, W1 - 1 a row; a row's filtered bytes are a zero and
// its mapped plane bytes.  ROWS = true (tce_png_deflate_rows_u8): pl is the strip's filtered bytes themselves, W1 a row, ns = n.
template <bool EMIT, bool ROWS>
__device__ __forceinline__ void dyn_walk(DynShared& S, const uint8_t* __restrict__ pl, const int n, const int ns, const int W1, const int nonzero,
                                         uint32_t* __restrict__ out, long long& flushed, int& wb, unsigned long long& sa, unsigned long long& sb) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint8_t* rawb = reinterpret_cast<const uint8_t*>(S.raw);
  const int dbits = EMIT ? S.dbits : 0;
  int open_start = 0;
  uint32_t open_val = 0u, my_extra = 0u, my_matches = 0u;
  auto count = [&](const Sym y) {
    atomicAdd(&S.cnt[y.s], 1u);
    my_extra += (uint32_t)y.e;
    my_matches += y.s > 256 ? 1u : 0u;
  };
  auto count_long = [&](const uint32_t b, const int L) {  // thread 0
    int M, r;
    long_split(L, M, r);
    atomicAdd(&S.cnt[b], 1u);
    if (M) atomicAdd(&S.cnt[285], (uint32_t)M);
    my_matches += (uint32_t)M;
    run_tail_syms(b, r, count);
  };

  for (int f0 = 0; f0 < n; f0 += TCE_PNG_PASS) {
    const int len = min(TCE_PNG_PASS, n - f0);
    const int r0 = f0 / W1, c0 = f0 - r0 * W1, fe = f0 + len - 1, re = fe / W1;
    const int q0 = ROWS ? f0 : f0 - r0 - (c0 ? 1 : 0), q1 = ROWS ? fe + 1 : fe - re;
    const int lead = (int)((reinterpret_cast<uintptr_t>(pl) + (uintptr_t)q0) & 3u);
    for (int j = tid; 4 * j < lead + (q1 - q0); j += PT) S.raw[j] = strip_dword(pl, q0 - lead + 4 * j, ns);
    __syncthreads();

    const int f = f0 + tid * PER;
    uint32_t v[PER + 1];
    uint32_t bmask = 0u;
    v[0] = open_val;
    if (f < f0 + len) {
      int r = f / W1, c = f - r * W1;
      auto fbyte = [&](const int ff, const int rr, const int cc) -> uint32_t {
        if (ROWS) return rawb[lead + (ff - q0)];
        if (cc == 0) return 0u;
        const uint32_t x = rawb[lead + (ff - rr - 1 - q0)];
        return nonzero ? (x ? (uint32_t)nonzero : 0u) : x;
      };
      if (tid > 0) v[0] = c > 0 ? fbyte(f - 1, r, c - 1) : fbyte(f - 1, r - 1, W1 - 1);
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        v[j + 1] = 0u;
        if (f + j < f0 + len) {
          v[j + 1] = fbyte(f + j, r, c);
          if (f + j > 0 && v[j + 1] != v[j]) bmask |= 1u << j;
          if (EMIT) {
            sa += v[j + 1];
            sb += (unsigned long long)v[j + 1] * (unsigned)(n - (f + j));
          }
          if (f + j == fe) S.last_val = v[j + 1];
          if (++c == W1) {
            c = 0;
            ++r;
          }
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < PER; ++j) v[j + 1] = 0u;
    }
    const int lastb = bmask ? f + (31 - __clz(bmask)) : -1, firstb = bmask ? f + (__ffs(bmask) - 1) : 0x7fffffff;

    int sm = lastb, mn = firstb;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int a = __shfl_up(sm, o, 64);
      if (lane >= o) sm = max(sm, a);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mn = min(mn, __shfl_xor(mn, o, 64));
    if (lane == 63) S.sc_max[wave] = sm;
    if (lane == 0) S.sc_min[wave] = mn;
    __syncthreads();  // (also: last_val is in)
    int s_in = __shfl_up(sm, 1, 64);
    if (lane == 0) s_in = -1;
    s_in = max(s_in, open_start);
    for (int k = 0; k < wave; ++k) s_in = max(s_in, S.sc_max[k]);
    int new_open = open_start;
    for (int k = 0; k < PWAVES; ++k) new_open = max(new_open, S.sc_max[k]);
    const int first = min(min(S.sc_min[0], S.sc_min[1]), min(S.sc_min[2], S.sc_min[3]));

    if (!EMIT) {
      if (tid == 0 && f0 > 0 && first != 0x7fffffff) count_long(open_val, first - open_start);
      int s = s_in;
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        if (bmask & (1u << j)) {
          if (s >= f0) run_syms(v[j], f + j - s, count);
          s = f + j;
        }
      }
      open_start = new_open;
      open_val = S.last_val;
      __syncthreads();  // raw, last_val and the scan words are free for the next pass
    } else {
      if (f0 > 0 && first != 0x7fffffff) dyn_long_run(S, out, flushed, wb, open_val, first - open_start);
      int bits = 0;
      {
        int s = s_in;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
          if (bmask & (1u << j)) {
            if (s >= f0) run_syms(v[j], f + j - s, [&](const Sym y) { bits += sym_tok(S.tab, dbits, y).n; });
            s = f + j;
          }
        }
      }
      int sum = bits;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int a = __shfl_up(sum, o, 64);
        if (lane >= o) sum += a;
      }
      if (lane == 63) S.sc_sum[wave] = sum;
      __syncthreads();
      int at = wb + sum - bits, total = 0;
      for (int k = 0; k < PWAVES; ++k) {
        if (k < wave) at += S.sc_sum[k];
        total += S.sc_sum[k];
      }
      {
        int s = s_in;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
          if (bmask & (1u << j)) {
            if (s >= f0)
              run_syms(v[j], f + j - s, [&](const Sym y) {
                const Tok t = sym_tok(S.tab, dbits, y);
                put(S.win, at, t);
                at += t.n;
              });
            s = f + j;
          }
        }
      }
      wb += total;
      open_start = new_open;
      open_val = S.last_val;
      flush(S.win, out, flushed, wb);  // its barriers also protect raw, last_val and the scan words for the next pass
    }
  }

  // the last run
  if (!EMIT) {
    if (tid == 0) {
      count_long(open_val, n - open_start);
      atomicAdd(&S.cnt[256], 1u);
    }
    if (my_extra) atomicAdd(&S.extra, my_extra);
    if (my_matches) atomicAdd(&S.matches, my_matches);
  } else {
    dyn_long_run(S, out, flushed, wb, open_val, n - open_start);
  }
}

// Code lengths of the symbols with a non-zero count (tce_rvos_png_dyn.h, "code lengths").  Every thread calls it; len[0 .. nsym) is
// ready behind its last barrier.  The sort is a rank count per symbol; the merge and the depths are one lane's serial work.
__device__ __forceinline__ void huff_lengths(DynShared& S, const uint32_t* cnt, const int nsym, const int limit, uint8_t* len) {
  const int tid = threadIdx.x;
  for (int s = tid; s < nsym; s += PT) S.w[s] = cnt[s];
  __syncthreads();
  for (;;) {  // ends: halved often enough every count is 1, and the tree of nsym <= 286 equal weights is 9 deep (19: 5)
    for (int s = tid; s < nsym; s += PT) {
      const uint32_t c = S.w[s];
      int rank = 0, used = 0;
      for (int t = 0; t < nsym; ++t) {
        const uint32_t d = S.w[t];
        if (d) {
          ++used;
          if (d < c || (d == c && t < s)) ++rank;
        }
      }
      if (c) {
        S.order[rank] = (uint16_t)s;
        S.wgt[rank] = c;
      }
      if (s == 0) S.nused = used;
    }
    __syncthreads();
    if (tid == 0) {
      const int n = S.nused;
      int maxd = 1;
      if (n > 1) {
        int li = 0, ii = n;  // heads of the two queues: leaves li .. n-1, merged nodes ii .. nx-1
        for (int nx = n; nx < 2 * n - 1; ++nx) {
          const int a = (li < n && (ii >= nx || S.wgt[li] <= S.wgt[ii])) ? li++ : ii++;
          const int b = (li < n && (ii >= nx || S.wgt[li] <= S.wgt[ii])) ? li++ : ii++;
          S.wgt[nx] = S.wgt[a] + S.wgt[b];
          S.par[a] = S.par[b] = (uint16_t)nx;
        }
        S.dep[2 * n - 2] = 0;
        int deepest = 0;
        for (int k = 2 * n - 3; k >= n; --k) {  // a node's parent was made after it
          const int d = S.dep[S.par[k]] + 1;
          S.dep[k] = (uint16_t)d;
          deepest = max(deepest, d);
        }
        maxd = deepest + 1;  // the deepest merged node has two leaves
      }
      S.over = maxd > limit;
    }
    __syncthreads();
    if (!S.over) break;
    for (int s = tid; s < nsym; s += PT) {
      const uint32_t c = S.w[s];
      if (c) S.w[s] = (c + 1u) >> 1;
    }
    __syncthreads();
  }
  for (int s = tid; s < nsym; s += PT) len[s] = 0;
  __syncthreads();
  const int n = S.nused;
  for (int i = tid; i < n; i += PT) len[S.order[i]] = (uint8_t)(n > 1 ? S.dep[S.par[i]] + 1 : 1);
  __syncthreads();
}

// canonical codes (RFC 1951 section 3.2.2) of lengths below 16 -> table entries; one lane
__device__ __forceinline__ void canonical(DynShared& S, const uint8_t* len, const int nsym, uint32_t* tab) {
  for (int b = 0; b < 16; ++b) S.next[b] = 0u;
  for (int s = 0; s < nsym; ++s) ++S.next[len[s]];
  uint32_t code = 0u, before = 0u;  // next[b]: from the count of length b to its first code
  for (int b = 1; b < 16; ++b) {
    code = (code + before) << 1;
    before = S.next[b];
    S.next[b] = code;
  }
  for (int s = 0; s < nsym; ++s) {
    const int l = len[s];
    tab[s] = l ? (huff(S.next[l]++, l) | ((uint32_t)l << 16)) : 0u;
  }
}

// the literal/length code lengths 0 .. nlit-1 and the distance code's one length 1 as symbols of the code-length alphabet: f(symbol,
// extra value, extra bits), greedily from the left (tce_rvos_png_dyn.h, "length sequence")
template <class F>
__device__ __forceinline__ void length_sequence(const uint8_t* len, const int nlit, F&& f) {
  auto at = [&](const int i) -> int { return i < nlit ? len[i] : 1; };
  const int n = nlit + 1;
  int i = 0;
  while (i < n) {
    const int v = at(i);
    int j = i + 1;
    while (j < n && at(j) == v) ++j;
    int r = j - i;
    if (v == 0) {
      while (r >= 11) {
        const int t = min(r, 138);
        f(18, (uint32_t)(t - 11), 7);
        r -= t;
      }
      if (r >= 3) {
        f(17, (uint32_t)(r - 3), 3);
        r = 0;
      }
    } else {
      f(v, 0u, 0);
      --r;
      while (r >= 3) {
        const int t = min(r, 6);
        f(16, (uint32_t)(t - 3), 2);
        r -= t;
      }
    }
    for (; r > 0; --r) f(v, 0u, 0);
    i = j;
  }
}

__device__ __forceinline__ int fixed_len(const int s) { return s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8; }

// From the counts to the code: S.tab, S.dbits, S.dynamic, and the block header in the (empty) window, S.hbits bits.  Every thread calls it.
__device__ __forceinline__ void dyn_build(DynShared& S) {
  const int tid = threadIdx.x;
  huff_lengths(S, S.cnt, NLL, DYN_CODE, S.len);
  if (tid == 0) {
    int nlit = NLL;
    while (nlit > 257 && S.len[nlit - 1] == 0) --nlit;
    S.nlit = nlit;
    for (int c = 0; c < NCL; ++c) S.clcnt[c] = 0u;
    uint32_t x = 0u;
    length_sequence(S.len, nlit, [&](const int c, const uint32_t, const int e) {
      ++S.clcnt[c];
      x += (uint32_t)e;
    });
    S.clextra = x;
  }
  __syncthreads();
  huff_lengths(S, S.clcnt, NCL, 7, S.cllen);
  if (tid == 0) {
    const int nlit = S.nlit;
    int ncl = NCL;
    while (ncl > 4 && S.cllen[CL_ORDER[ncl - 1]] == 0) --ncl;
    unsigned long long dyn = 3ull + 14ull + 3ull * (unsigned)ncl + S.clextra, fix = 3ull;
    for (int c = 0; c < NCL; ++c) dyn += (unsigned long long)S.clcnt[c] * S.cllen[c];
    for (int s = 0; s < NLL; ++s) {
      const unsigned long long c = S.cnt[s];
      dyn += c * S.len[s];
      fix += c * (unsigned)fixed_len(s);
    }
    dyn += (unsigned long long)S.extra + S.matches;
    fix += (unsigned long long)S.extra + 5ull * S.matches;
    const int dynamic = dyn < fix;  // a tie goes to the fixed code
    S.dynamic = dynamic;
    S.dbits = dynamic ? 1 : 5;
    int at = 0;
    auto w = [&](const uint32_t v, const int nb) {
      put(S.win, at, Tok{v, nb});
      at += nb;
    };
    if (dynamic) {
      canonical(S, S.len, NLL, S.tab);
      canonical(S, S.cllen, NCL, S.cltab);
      w(4u, 3);  // BFINAL = 0, BTYPE = 10
      w((uint32_t)(nlit - 257), 5);
      w(0u, 5);
      w((uint32_t)(ncl - 4), 4);
      for (int k = 0; k < ncl; ++k) w(S.cllen[CL_ORDER[k]], 3);
      length_sequence(S.len, nlit, [&](const int c, const uint32_t x, const int e) {
        const uint32_t ent = S.cltab[c];
        const int nb = (int)(ent >> 16);
        w((ent & 0xFFFFu) | (x << nb), nb + e);
      });
    } else {
      w(2u, 3);  // BFINAL = 0, BTYPE = 01
    }
    S.hbits = at;
  }
  __syncthreads();
  if (!S.dynamic) {
    for (int s = tid; s < NTAB; s += PT) {
      const int l = fixed_len(s);
      const uint32_t code = s < 144 ? 0x30u + s : s < 256 ? 0x190u + (s - 144) : s < 280 ? (uint32_t)(s - 256) : 0xC0u + (s - 280);
      S.tab[s] = huff(code, l) | ((uint32_t)l << 16);
    }
  }
  __syncthreads();
}

// First launch of the dynamic encoding, in png_strip_kernel's place: the same workspace layout, the same meta words.  ROWS = true:
// `planes` is rows [P,H,W+1], the filtered bytes as they are (dyn_walk).
template <bool ROWS>
__global__ void __launch_bounds__(PT) png_strip_dyn_kernel(const uint8_t* __restrict__ planes, uint32_t* __restrict__ ws, const int H, const int W,
                                                           const int S_rows, const int nstrips, const long long stride_dw, const int nonzero) {
  __shared__ DynShared S;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int strip = blockIdx.x, p = blockIdx.y;
  const long long sidx = (long long)p * nstrips + strip, nstr = (long long)gridDim.y * nstrips;
  const int row0 = strip * S_rows, rows = min(S_rows, H - row0), W1 = W + 1;
  const int n = rows * W1, ns = ROWS ? n : rows * W;
  const uint8_t* __restrict__ pl = planes + ((long long)p * H + row0) * (ROWS ? W1 : W);
  uint32_t* __restrict__ out = ws + nstr * 3 + sidx * stride_dw;

  for (int i = tid; i < DWIN_DW; i += PT) S.win[i] = 0u;
  for (int i = tid; i < NTAB; i += PT) S.cnt[i] = 0u;
  if (tid == 0) S.extra = S.matches = 0u;
  __syncthreads();
  int wb = 0;
  long long flushed = 0;
  unsigned long long sa = 0ull, sb = 0ull;
  dyn_walk<false, ROWS>(S, pl, n, ns, W1, nonzero, out, flushed, wb, sa, sb);
  __syncthreads();
  dyn_build(S);
  wb = S.hbits;
  flush(S.win, out, flushed, wb);
  dyn_walk<true, ROWS>(S, pl, n, ns, W1, nonzero, out, flushed, wb, sa, sb);

  // end of block, a stored-block header, zero bits to the byte boundary, 00 00 FF FF
  const Tok eob = sym_tok(S.tab, 0, Sym{256, 0u, 0});
  if (tid == 0) put(S.win, wb, eob);
  wb = (wb + eob.n + 3 + 7) & ~7;
  if (tid == 0) put(S.win, wb + 16, Tok{0xFFFFu, 16});
  wb += 32;
  __syncthreads();
  const int ndw = (wb + 31) >> 5;
  for (int i = tid; i < ndw; i += PT) out[flushed + i] = S.win[i];

  uint32_t ra = (uint32_t)(sa % ADLER), rb = (uint32_t)(sb % ADLER);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ra += (uint32_t)__shfl_xor((int)ra, o, 64);
    rb += (uint32_t)__shfl_xor((int)rb, o, 64);
  }
  if (lane == 0) {
    S.red[0][wave] = ra;
    S.red[1][wave] = rb;
  }
  __syncthreads();
  if (tid == 0) {
    const uint32_t a = (1u + S.red[0][0] + S.red[0][1] + S.red[0][2] + S.red[0][3]) % ADLER;
    const uint32_t b = ((uint32_t)(n % (int)ADLER) + S.red[1][0] + S.red[1][1] + S.red[1][2] + S.red[1][3]) % ADLER;
    ws[sidx * 2] = (uint32_t)(flushed * 4 + (wb >> 3));
    ws[sidx * 2 + 1] = a | (b << 16);
  }
}

struct PngPlan {
  long long bound, stride_dw;
  int nstrips;
};

// false: bad extents
bool png_plan(const int H, const int W, const int S, PngPlan* pl) {
  if (H <= 0 || W <= 0 || S <= 0 || (long long)H * W >= (1ll << 31)) return false;
  const long long rows = S < H ? S : H, W1 = (long long)W + 1, full = H / rows, rest = H % rows;
  const long long sb = TCE_PNG_STRIP_BOUND(rows * W1);
  pl->bound = 2 + full * sb + (rest ? TCE_PNG_STRIP_BOUND(rest * W1) : 0) + 2 + 4;
  pl->stride_dw = (sb + 3) / 4;
  pl->nstrips = (int)(full + (rest ? 1 : 0));
  // nbytes is int32, and byte offsets of a plane's stream stay ints with room for a workgroup's stride; a grid holds nstrips * 256 threads
  return pl->bound < (1ll << 31) - 4096 && pl->nstrips <= TCE_PNG_MAX_STRIPS;
}

}  // namespace

extern "C" int64_t tce_png_stream_bound(int32_t H, int32_t W, int32_t rows_per_strip) {
  PngPlan pl;
  return png_plan(H, W, rows_per_strip, &pl) ? pl.bound : -1;
}

extern "C" int64_t tce_png_ws_bytes(int32_t P, int32_t H, int32_t W, int32_t rows_per_strip) {
  PngPlan pl;
  if (P <= 0 || P > 65535 || !png_plan(H, W, rows_per_strip, &pl)) return -1;
  const int64_t dwords = (int64_t)P * pl.nstrips * (3 + pl.stride_dw);
  return (dwords * 4 + 7) & ~(int64_t)7;
}

extern "C" int tce_png_deflate_u8(const uint8_t* planes, uint8_t* streams, int32_t* nbytes, void* ws, int32_t P, int32_t H, int32_t W,
                                  int32_t rows_per_strip, int32_t nonzero_value, tceStream stream) {
  PngPlan pl;
  TCE_CHECK_ARG(P > 0 && H > 0 && W > 0 && rows_per_strip > 0, "tce_png_deflate_u8: non-positive extent");
  TCE_CHECK_ARG(P <= 65535 && png_plan(H, W, rows_per_strip, &pl),
                "tce_png_deflate_u8: a plane must stay below 2^31 elements, its stream bound below 2^31 - 4096 bytes, its strips at or below 2^22 and P at or below 65535");
  TCE_CHECK_ARG(nonzero_value >= 0 && nonzero_value <= 255, "tce_png_deflate_u8: nonzero_value %d outside 0 .. 255", nonzero_value);
  TCE_CHECK_ARG(planes && streams && nbytes && ws, "tce_png_deflate_u8: null pointer");
  TCE_CHECK_ARG(((uintptr_t)ws & 7u) == 0 && ((uintptr_t)nbytes & 3u) == 0,
                "tce_png_deflate_u8: ws must be 8-byte aligned, nbytes 4-byte aligned");
  const int S = rows_per_strip < H ? rows_per_strip : H;  // the same strips, and s * S stays an int
  hipLaunchKernelGGL(png_strip_kernel, dim3(pl.nstrips, P), dim3(PT), 0, (hipStream_t)stream, planes, (uint32_t*)ws, H, W, S, pl.nstrips,
                     pl.stride_dw, nonzero_value);
  hipLaunchKernelGGL(png_plane_kernel, dim3(P), dim3(PT), 0, (hipStream_t)stream, (uint32_t*)ws, streams, nbytes, H, W, S, pl.nstrips,
                     pl.bound);
  hipLaunchKernelGGL(png_copy_kernel, dim3(pl.nstrips, P), dim3(PT), 0, (hipStream_t)stream, (const uint32_t*)ws, streams, pl.nstrips,
                     pl.stride_dw, pl.bound);
  TCE_CHECK_LAUNCH("tce_png_deflate_u8");
  return TCE_OK;
}

extern "C" int tce_png_deflate_dyn_u8(const uint8_t* planes, uint8_t* streams, int32_t* nbytes, void* ws, int32_t P, int32_t H, int32_t W,
                                      int32_t rows_per_strip, int32_t nonzero_value, tceStream stream) {
  PngPlan pl;
  TCE_CHECK_ARG(P > 0 && H > 0 && W > 0 && rows_per_strip > 0, "tce_png_deflate_dyn_u8: non-positive extent");
  TCE_CHECK_ARG(P <= 65535 && png_plan(H, W, rows_per_strip, &pl),
                "tce_png_deflate_dyn_u8: a plane must stay below 2^31 elements, its stream bound below 2^31 - 4096 bytes, its strips at or below 2^22 and P at or below 65535");
  TCE_CHECK_ARG(nonzero_value >= 0 && nonzero_value <= 255, "tce_png_deflate_dyn_u8: nonzero_value %d outside 0 .. 255", nonzero_value);
  TCE_CHECK_ARG(planes && streams && nbytes && ws, "tce_png_deflate_dyn_u8: null pointer");
  TCE_CHECK_ARG(((uintptr_t)ws & 7u) == 0 && ((uintptr_t)nbytes & 3u) == 0,
                "tce_png_deflate_dyn_u8: ws must be 8-byte aligned, nbytes 4-byte aligned");
  const int S = rows_per_strip < H ? rows_per_strip : H;
  hipLaunchKernelGGL(png_strip_dyn_kernel<false>, dim3(pl.nstrips, P), dim3(PT), 0, (hipStream_t)stream, planes, (uint32_t*)ws, H, W, S, pl.nstrips,
                     pl.stride_dw, nonzero_value);
  hipLaunchKernelGGL(png_plane_kernel, dim3(P), dim3(PT), 0, (hipStream_t)stream, (uint32_t*)ws, streams, nbytes, H, W, S, pl.nstrips,
                     pl.bound);
  hipLaunchKernelGGL(png_copy_kernel, dim3(pl.nstrips, P), dim3(PT), 0, (hipStream_t)stream, (const uint32_t*)ws, streams, pl.nstrips,
                     pl.stride_dw, pl.bound);
  TCE_CHECK_LAUNCH("tce_png_deflate_dyn_u8");
  return TCE_OK;
}

// ------------------------------------------------------------------------------------------------ RGB images (csrc/tce_rvos_vis.h)
namespace {

constexpr int FCH = 4096;  // filtered bytes of a row staged at a time, with the 3 bytes in front of them

__device__ __forceinline__ int paeth(const int a, const int b, const int c) {
  const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// byte i of the row filtered with type t: cs / us hold bytes i0-3 .. of the row and of the row above
__device__ __forceinline__ uint32_t filt_byte(const uint8_t* cs, const uint8_t* us, const int k, const int i, const bool top, const int t) {
  const int x = cs[k + 3], a = i >= 3 ? cs[k] : 0, b = top ? 0 : us[k + 3], c = (top || i < 3) ? 0 : us[k];
  const int pred = t == 0 ? 0 : t == 1 ? a : t == 2 ? b : t == 3 ? ((a + b) >> 1) : paeth(a, b, c);
  return (uint32_t)(x - pred) & 255u;
}

// A workgroup per image row.  Pass 1: the five sums of |filtered byte as int8| over the row, in chunks staged in LDS (whole dwords
// of the image wherever four bytes are one aligned word), one reduction, the choice.  Pass 2: the chosen row, a thread per
// aligned dword of rows.
__global__ void __launch_bounds__(PT) png_filter_rgb_kernel(const uint8_t* __restrict__ img, uint8_t* __restrict__ rows, const int H, const int W) {
  __shared__ uint32_t craw[FCH / 4 + 4], uraw[FCH / 4 + 4];
  __shared__ uint32_t part[5][PWAVES];
  __shared__ int chosen;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int y = blockIdx.x, p = blockIdx.y, n = 3 * W, ns = H * n;
  const bool top = y == 0;
  const uint8_t* __restrict__ im = img + (long long)p * ns;
  uint8_t* __restrict__ dst = rows + ((long long)p * H + y) * (n + 1);
  const uint8_t* cs = reinterpret_cast<const uint8_t*>(craw);
  const uint8_t* us = reinterpret_cast<const uint8_t*>(uraw);
  int clead = 0, ulead = 0;
  auto stage = [&](const int i0, const int len) {  // bytes i0-3 .. i0+len-1 of the row and of the row above; outside the image: 0
    const int s = y * n + i0 - 3, u = s - n;
    clead = (int)((reinterpret_cast<uintptr_t>(im) + (uintptr_t)(intptr_t)s) & 3u);
    ulead = (int)((reinterpret_cast<uintptr_t>(im) + (uintptr_t)(intptr_t)u) & 3u);
    for (int j = tid; 4 * j < clead + len + 3; j += PT) craw[j] = strip_dword(im, s - clead + 4 * j, ns);
    if (!top)
      for (int j = tid; 4 * j < ulead + len + 3; j += PT) uraw[j] = strip_dword(im, u - ulead + 4 * j, ns);
    __syncthreads();
  };

  uint32_t sum[5] = {0u, 0u, 0u, 0u, 0u};  // a wave's share: at most 128 * 3W / 4 < 2^32 (W <= 2^24)
  for (int i0 = 0; i0 < n; i0 += FCH) {
    const int len = min(FCH, n - i0);
    stage(i0, len);
    for (int k = tid; k < len; k += PT) {
#pragma unroll
      for (int t = 0; t < 5; ++t) {
        const int f = (int)(int8_t)filt_byte(cs + clead, us + ulead, k, i0 + k, top, t);
        sum[t] += (uint32_t)abs(f);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int t = 0; t < 5; ++t) {
    uint32_t v = sum[t];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    if (lane == 0) part[t][wave] = v;
  }
  __syncthreads();
  if (tid == 0) {
    int best = 0;
    unsigned long long bs = ~0ull;
    for (int t = 0; t < 5; ++t) {
      unsigned long long v = 0ull;
      for (int k = 0; k < PWAVES; ++k) v += part[t][k];
      if (v < bs) {  // a tie goes to the lowest type
        bs = v;
        best = t;
      }
    }
    chosen = best;
  }
  __syncthreads();
  const int t = chosen;

  for (int i0 = 0; i0 < n; i0 += FCH) {
    const int len = min(FCH, n - i0);
    stage(i0, len);
    // bytes k_lo .. k_hi-1 of the output row: byte 0 is the type, byte k the filtered byte k - 1
    const int k_lo = i0 ? i0 + 1 : 0, k_hi = i0 + len + 1;
    const int shift = (int)(reinterpret_cast<uintptr_t>(dst + k_lo) & 3u);
    for (int g = tid; 4 * g - shift < k_hi - k_lo; g += PT) {
      const int kk = k_lo + 4 * g - shift;
      uint32_t d = 0u;
      bool whole = true;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = kk + q;
        if (k >= k_lo && k < k_hi) {
          const uint32_t b = k == 0 ? (uint32_t)t : filt_byte(cs + clead, us + ulead, k - 1 - i0, k - 1, top, t);
          d |= b << (8 * q);
        } else {
          whole = false;
        }
      }
      if (whole) {
        *reinterpret_cast<uint32_t*>(dst + kk) = d;
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (kk + q >= k_lo && kk + q < k_hi) dst[kk + q] = (uint8_t)(d >> (8 * q));
      }
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" int tce_png_filter_rgb_u8(const uint8_t* img, uint8_t* rows, int32_t P, int32_t H, int32_t W, tceStream stream) {
  TCE_CHECK_ARG(P > 0 && H > 0 && W > 0, "tce_png_filter_rgb_u8: non-positive extent");
  TCE_CHECK_ARG(P <= 65535 && W <= (1 << 24) && (long long)H * (3ll * W + 1) < (1ll << 31) - 4096,
                "tce_png_filter_rgb_u8: an image's rows must stay below 2^31 - 4096 bytes, W at or below 2^24 and P at or below 65535");
  TCE_CHECK_ARG(img && rows, "tce_png_filter_rgb_u8: null pointer");
  hipLaunchKernelGGL(png_filter_rgb_kernel, dim3(H, P), dim3(PT), 0, (hipStream_t)stream, img, rows, H, W);
  TCE_CHECK_LAUNCH("tce_png_filter_rgb_u8");
  return TCE_OK;
}

extern "C" int tce_png_deflate_rows_u8(const uint8_t* rows, uint8_t* streams, int32_t* nbytes, void* ws, int32_t P, int32_t H, int32_t R,
                                       int32_t rows_per_strip, tceStream stream) {
  PngPlan pl;
  TCE_CHECK_ARG(P > 0 && H > 0 && R > 1 && rows_per_strip > 0, "tce_png_deflate_rows_u8: non-positive extent (R must be at least 2)");
  TCE_CHECK_ARG(P <= 65535 && png_plan(H, R - 1, rows_per_strip, &pl),
                "tce_png_deflate_rows_u8: H * (R - 1) must stay below 2^31, the stream bound below 2^31 - 4096 bytes, the strips at or below 2^22 and P at or below 65535");
  TCE_CHECK_ARG(rows && streams && nbytes && ws, "tce_png_deflate_rows_u8: null pointer");
  TCE_CHECK_ARG(((uintptr_t)ws & 7u) == 0 && ((uintptr_t)nbytes & 3u) == 0,
                "tce_png_deflate_rows_u8: ws must be 8-byte aligned, nbytes 4-byte aligned");
  const int S = rows_per_strip < H ? rows_per_strip : H;
  hipLaunchKernelGGL(png_strip_dyn_kernel<true>, dim3(pl.nstrips, P), dim3(PT), 0, (hipStream_t)stream, rows, (uint32_t*)ws, H, R - 1, S,
                     pl.nstrips, pl.stride_dw, 0);
  hipLaunchKernelGGL(png_plane_kernel, dim3(P), dim3(PT), 0, (hipStream_t)stream, (uint32_t*)ws, streams, nbytes, H, R - 1, S, pl.nstrips,
                     pl.bound);
  hipLaunchKernelGGL(png_copy_kernel, dim3(pl.nstrips, P), dim3(PT), 0, (hipStream_t)stream, (const uint32_t*)ws, streams, pl.nstrips,
                     pl.stride_dw, pl.bound);
  TCE_CHECK_LAUNCH("tce_png_deflate_rows_u8");
  return TCE_OK;
}
