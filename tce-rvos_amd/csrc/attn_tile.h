// What the attention kernels of attn.hip share: the Q / K / V fragment loads, the score and PV products, the online-softmax tile
// step (one per arithmetic: base e, and the 3-D window kernel's base 2), the KSPLIT merge, the accumulator store and the window
// geometry.  Every function is inlined and every mode (SINGLE, NW) is a compile-time parameter: as run-time flags they put uniform
// branches around the splits and in front of the lo-term MFMAs, and the basic-block boundaries kept the scheduler from overlapping
// the softmax arithmetic with the MFMAs (see ffn_fused_kernel).  A helper adds no branch that its callers did not have.
//
// Layout all of it rests on (attn.hip, mha_mfma_kernel): scores are computed TRANSPOSED, S^T = K Q^T, so a lane (query = lane & 31,
// half lhi = lane >> 5) holds the scores of ITS query against the 16 keys crow(r, lhi) of a 32-key tile in accumulator registers
// r = 0..15, and those registers are the B operand of O^T = V^T P^T.
#pragma once
#include "frag.h"

namespace {

constexpr int HD = 32;  // head dim

// ---------------------------------------------------------------------------------------------------
// Q
// ---------------------------------------------------------------------------------------------------
// fp16 forms.  B operand of S^T = K Q^T: the lane holds Q[q][16s + 8*lhi + 0..7] * scale, split, for the two k-steps s; p = the query's row
template <bool SINGLE>
__device__ __forceinline__ void load_q_split(const float* p, const float scale, const int lhi, h16x8 (&qh)[2], h16x8 (&ql)[2]) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p + 16 * s + 8 * lhi);
    const f32x4 c = *reinterpret_cast<const f32x4*>(p + 16 * s + 8 * lhi + 4);
    unsigned hw[4], lw[4];
    split2(a[0] * scale, a[1] * scale, hw[0], lw[0], SINGLE);
    split2(a[2] * scale, a[3] * scale, hw[1], lw[1], SINGLE);
    split2(c[0] * scale, c[1] * scale, hw[2], lw[2], SINGLE);
    split2(c[2] * scale, c[3] * scale, hw[3], lw[3], SINGLE);
    qh[s] = __builtin_bit_cast(h16x8, u32x4{hw[0], hw[1], hw[2], hw[3]});
    ql[s] = __builtin_bit_cast(h16x8, u32x4{lw[0], lw[1], lw[2], lw[3]});
  }
}

// fp32 forms: the query's 32 channels, scaled, one row per lane.  The VALU kernels use it as is; the exact-MFMA kernels pick their B
// operand Q[q][d = 2s + lhi] out of it themselves: with that select in here the compiler keeps the row in registers, and their
// 144 bytes/lane of scratch go -- a code-generation change, which a move of code is not the place for
__device__ __forceinline__ void load_q_row(const float* p, const float scale, float (&q)[HD]) {
#pragma unroll
  for (int d4 = 0; d4 < 8; ++d4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p + d4 * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) q[d4 * 4 + j] = v[j] * scale;
  }
}

// ---------------------------------------------------------------------------------------------------
// K / V of one token (4 channels at `off` = h * HD + 4 * d4), or the qkv bias when the token is padding (!real; row unread)
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ void load_kv(const float* qkv, const float* qkv_bias, const bool real, const long long row, const int C,
                                        const int off, f32x4& kv, f32x4& vv) {
  if (real) {
    const float* p = qkv + row * (3 * C) + off;
    kv = *reinterpret_cast<const f32x4*>(p + C);
    vv = *reinterpret_cast<const f32x4*>(p + 2 * C);
  } else {
    kv = *reinterpret_cast<const f32x4*>(qkv_bias + C + off);
    vv = *reinterpret_cast<const f32x4*>(qkv_bias + 2 * C + off);
  }
}

// V transposed into fp16 planes Vt[d][key] (pitch in halfs): the four channels 4 d4 .. + 3 of `key`, (h0, h1) / (l0, l1) from split2
__device__ __forceinline__ void scatter_vt(void* plane_hi, void* plane_lo, const int pitch_halfs, const int key, const int d4,
                                           const unsigned h0, const unsigned h1, const unsigned l0, const unsigned l1) {
  unsigned short* const vh = reinterpret_cast<unsigned short*>(plane_hi) + (d4 * 4) * pitch_halfs + key;
  unsigned short* const vl = reinterpret_cast<unsigned short*>(plane_lo) + (d4 * 4) * pitch_halfs + key;
  vh[0] = (unsigned short)(h0 & 0xffffu);
  vh[pitch_halfs] = (unsigned short)(h0 >> 16);
  vh[2 * pitch_halfs] = (unsigned short)(h1 & 0xffffu);
  vh[3 * pitch_halfs] = (unsigned short)(h1 >> 16);
  vl[0] = (unsigned short)(l0 & 0xffffu);
  vl[pitch_halfs] = (unsigned short)(l0 >> 16);
  vl[2 * pitch_halfs] = (unsigned short)(l1 & 0xffffu);
  vl[3 * pitch_halfs] = (unsigned short)(l1 >> 16);
}

// ---------------------------------------------------------------------------------------------------
// Fragments of one 32-key tile out of fp16 planes (LDS or global)
// ---------------------------------------------------------------------------------------------------
// A operand of S^T: K[key = lane & 31][16s + 8*lhi + 0..7]; rowh / rowl = the key's row (32 halfs) in the hi / lo plane
__device__ __forceinline__ void load_k_frags(const unsigned char* rowh, const unsigned char* rowl, const int lhi, h16x8 (&kh)[2],
                                             h16x8 (&kl)[2]) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    kh[s] = *reinterpret_cast<const h16x8*>(rowh + (16 * s + 8 * lhi) * 2);
    kl[s] = *reinterpret_cast<const h16x8*>(rowl + (16 * s + 8 * lhi) * 2);
  }
}

// A operand of O^T, k-step s: V^T[d = lane & 31][key]; element j <-> accumulator register 8s + j <-> key crow(8s + j, lhi), i.e.
// elements 0..3 are keys 16s + 4*lhi + 0..3 and elements 4..7 those + 8: two 8-byte reads.  row = channel d's keys of this tile
__device__ __forceinline__ h16x8 load_vt_frag(const unsigned char* row, const int s, const int lhi) {
  const int kb = (16 * s + 4 * lhi) * 2;
  const u32x2 a = *reinterpret_cast<const u32x2*>(row + kb);
  const u32x2 b = *reinterpret_cast<const u32x2*>(row + kb + 16);
  return __builtin_bit_cast(h16x8, u32x4{a[0], a[1], b[0], b[1]});
}

// ---------------------------------------------------------------------------------------------------
// Scores of one tile, S^T[key][q]
// ---------------------------------------------------------------------------------------------------
template <bool SINGLE>
__device__ __forceinline__ void scores_split(const h16x8 (&kh)[2], const h16x8 (&kl)[2], const h16x8 (&qh)[2], const h16x8 (&ql)[2],
                                             f32x16& st) {
#pragma unroll
  for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
  for (int s = 0; s < 2; ++s) mma3(st, kh[s], kl[s], qh[s], ql[s], SINGLE);
}

// exact fp32 (v_mfma_f32_32x32x2_f32): A = K[key = lane & 31][d = 2s + lhi], krow = &K[lane & 31][lhi] in LDS; B = qreg[s]
__device__ __forceinline__ void scores_f32(const float* krow, const float (&qreg)[16], f32x16& st) {
#pragma unroll
  for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
  for (int s2 = 0; s2 < 16; ++s2) st = __builtin_amdgcn_mfma_f32_32x32x2f32(krow[2 * s2], qreg[s2], st, 0, 0, 0);
}

// ---------------------------------------------------------------------------------------------------
// Online softmax, one tile.  In: st = the tile's raw scores; mask(r, s) = the kernel's own mask path (they differ by kernel and
// stay there): it returns -3.0e38 for a key that is ignored or does not exist and min(s, 3.0e38) otherwise.  It is applied in
// the pass that takes the tile maximum, as every kernel had it: as a pass of its own before the call it cost the
// staged split-fp16 kernels up to 8 VGPRs.
// Out: st = the probabilities relative to the new running maximum m; l (this lane half's partial sum) and o rescaled.
// A sentinel is a select, not arithmetic: p = 0 whatever m is, so a tile (or a whole row) of ignored keys leaves (m, l, o) alone.
// ---------------------------------------------------------------------------------------------------
template <class Mask>
__device__ __forceinline__ void online_update(f32x16& st, float& m, float& l, f32x16& o, const Mask mask) {
  float tmax = -3.0e38f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    st[r] = mask(r, st[r]);
    tmax = fmaxf(tmax, st[r]);
  }
  tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
  const float mnew = fmaxf(m, tmax);
  const float corr = __expf(m - mnew);
  l *= corr;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    o[r] *= corr;
    const float pj = (st[r] > -1.0e38f) ? __expf(st[r] - mnew) : 0.f;
    st[r] = pj;
    l += pj;
  }
  m = mnew;
}

// The 3-D window kernel's step: DIFFERENT arithmetic, not a mode of the one above.  Scores are in base 2 (scale and bias table
// carry log2(e); v_exp_f32 IS 2^x), every query has at least one real key so no select guards the exponential
// (exp2(-3e38 - m) = 0 for the keys that do not exist), and the rescale is skipped when no query's maximum moved.
__device__ __forceinline__ void online_update_exp2(f32x16& st, float& m, float& l, f32x16& o) {
  float tmax = -3.0e38f;
#pragma unroll
  for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, st[r]);
  tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
  const float mnew = fmaxf(m, tmax);
  if (__builtin_amdgcn_ballot_w64(mnew > m) != 0) {  // the running maximum of some query moved: rescale (else corr = 1 for all)
    const float corr = __builtin_amdgcn_exp2f(m - mnew);
    l *= corr;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] *= corr;
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float pj = __builtin_amdgcn_exp2f(st[r] - mnew);
    st[r] = pj;
    l += pj;
  }
  m = mnew;
}

// ---------------------------------------------------------------------------------------------------
// O^T[d][q] += V^T[d][key] P^T[key][q]
// ---------------------------------------------------------------------------------------------------
// probabilities of accumulator registers 8s .. 8s + 7 -> the B fragment of k-step s; the product is then
// mma3(o, vh, vl, ph, pl, SINGLE) with vh / vl = load_vt_frag of the hi / lo plane, or the same fragments held in registers
template <bool SINGLE>
__device__ __forceinline__ void p_frag(const f32x16& st, const int s, h16x8& ph, h16x8& pl) {
  unsigned hw[4], lw[4];
#pragma unroll
  for (int q2 = 0; q2 < 4; ++q2) split2(st[8 * s + 2 * q2], st[8 * s + 2 * q2 + 1], hw[q2], lw[q2], SINGLE);
  ph = __builtin_bit_cast(h16x8, u32x4{hw[0], hw[1], hw[2], hw[3]});
  pl = __builtin_bit_cast(h16x8, u32x4{lw[0], lw[1], lw[2], lw[3]});
}

// exact fp32: k-step r pairs the keys crow(r, 0), crow(r, 1); vcol = &V[key 0 of the tile][d = lane & 31] in LDS, rows of HD floats
__device__ __forceinline__ void pv_f32(const float* vcol, const int lhi, const f32x16& st, f32x16& o) {
#pragma unroll
  for (int r = 0; r < 16; ++r) o = __builtin_amdgcn_mfma_f32_32x32x2f32(vcol[crow(r, lhi) * HD], st[r], o, 0, 0, 0);
}

// ---------------------------------------------------------------------------------------------------
// KSPLIT: the NW waves of a workgroup hold partial (m, l, O) of the SAME 32 queries over disjoint key ranges.  Merge through LDS:
// O = sum_w O_w e^(m_w - m*), l likewise; a wave that saw no kept key carries (sentinel, 0) and weighs e^(sentinel - m*) = 0,
// or 1 on zeros when every wave did.  Wave 0 returns true with the merged (l, o); the others return false and are done.
// ---------------------------------------------------------------------------------------------------
template <int NW>
__device__ __forceinline__ bool ksplit_merge(f32x16& o, const float m, float& l, const int wave, const int l31, const int lhi) {
  __shared__ float sO[NW][HD][33];
  __shared__ float sML[NW][2][32];
#pragma unroll
  for (int r = 0; r < 16; ++r) sO[wave][crow(r, lhi)][l31] = o[r];
  if (lhi == 0) {
    sML[wave][0][l31] = m;
    sML[wave][1][l31] = l;
  }
  __syncthreads();
  if (wave != 0) return false;
  float mstar = -3.0e38f;
#pragma unroll
  for (int w = 0; w < NW; ++w) mstar = fmaxf(mstar, sML[w][0][l31]);
  float f[NW];
  l = 0.f;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    f[w] = __expf(sML[w][0][l31] - mstar);
    l += sML[w][1][l31] * f[w];
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float acc = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) acc = fmaf(sO[w][crow(r, lhi)][l31], f[w], acc);
    o[r] = acc;
  }
  return true;
}

// ---------------------------------------------------------------------------------------------------
// Normalised store of a query's output row (32 floats at po)
// ---------------------------------------------------------------------------------------------------
// MFMA accumulator layout: registers 4g .. 4g + 3 are 4 consecutive d: d = 8g + 4*lhi + (0..3)
__device__ __forceinline__ void store_o(float* po, const f32x16& o, const float inv, const int lhi) {
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4) {
    f32x4 v = {o[4 * g4] * inv, o[4 * g4 + 1] * inv, o[4 * g4 + 2] * inv, o[4 * g4 + 3] * inv};
    *reinterpret_cast<f32x4*>(po + 8 * g4 + 4 * lhi) = v;
  }
}

// ---------------------------------------------------------------------------------------------------
// Window geometry.  The zero-padding to a multiple of the window, the cyclic shift, window partition / reverse and the final crop
// are index arithmetic; a padded token carries qkv = bias; the -100 mask separates region ids built on the padded, shifted grid.
// ---------------------------------------------------------------------------------------------------
struct Win2D {
  static constexpr int WS = 7;
  int wy, wx;   // the window
  int shift;    // 0 or 3
  int Hp, Wp;   // padded frame
  int H, W;     // frame
  // token j of the window -> source pixel (un-shifted, padded coordinates); false = padded token
  __device__ __forceinline__ bool src(const int j, int& ys, int& xs) const {
    const int yy = wy * WS + j / WS, xx = wx * WS + j % WS;  // shifted-frame coordinates
    ys = yy + shift;
    xs = xx + shift;
    if (ys >= Hp) ys -= Hp;
    if (xs >= Wp) xs -= Wp;
    return ys < H && xs < W;
  }
  // region id of the token at (jy, jx) of the window; callers test shift > 0 first (one region otherwise)
  __device__ __forceinline__ int region(const int jy, const int jx) const {
    const int y2 = wy * WS + jy, x2 = wx * WS + jx;
    const int ry = y2 < Hp - WS ? 0 : (y2 < Hp - shift ? 1 : 2);
    const int rx = x2 < Wp - WS ? 0 : (x2 < Wp - shift ? 1 : 2);
    return ry * 3 + rx;
  }
};

struct Win3D {
  int D, H, W;        // token grid (frames, rows, cols)
  int wd, wh, ww;     // effective window
  int sd, sh, sw;     // effective shift (0 if the block is not shifted)
  int Dp, Hp, Wp;     // padded grid
  int fd, fh, fw;     // nominal (full) window: 8,7,7
  // token n of window (bd, by, bx) -> src = its row of the token grid or -1 (padded), rid = its mask region id
  __device__ __forceinline__ void token(const int n, const int bd, const int by, const int bx, int& src, int& rid) const {
    const int x = n % ww, y = (n / ww) % wh, d = n / (ww * wh);
    const int dd = bd * wd + d, yy = by * wh + y, xx = bx * ww + x;  // shifted-grid coordinates
    int ds = dd + sd, ys = yy + sh, xs = xx + sw;
    if (ds >= Dp) ds -= Dp;
    if (ys >= Hp) ys -= Hp;
    if (xs >= Wp) xs -= Wp;
    src = (ds < D && ys < H && xs < W) ? (ds * H + ys) * W + xs : -1;
    const int rd = sd > 0 ? (dd < Dp - wd ? 0 : (dd < Dp - sd ? 1 : 2)) : 0;
    const int ry = sh > 0 ? (yy < Hp - wh ? 0 : (yy < Hp - sh ? 1 : 2)) : 0;
    const int rx = sw > 0 ? (xx < Wp - ww ? 0 : (xx < Wp - sw ? 1 : 2)) : 0;
    rid = (rd * 3 + ry) * 3 + rx;
  }
  // host: a (T, H, W) grid under the nominal window (full_d, 7, 7), rolled by (full_d / 2, shift, shift) when shift != 0.
  // shrink = the video backbone's get_window_size: a dim that fits in one window shrinks the window to it and is never shifted;
  // without it (2-D Swin, full_d = 1) rows and columns are padded up to the full window
  static Win3D make(const int T, const int H, const int W, const int full_d, const int shift, const bool shrink) {
    Win3D g;
    g.D = T; g.H = H; g.W = W;
    g.fd = full_d; g.fh = 7; g.fw = 7;
    const int size[3] = {T, H, W}, full[3] = {full_d, 7, 7}, roll[3] = {shift ? full_d / 2 : 0, shift, shift};
    int win[3], sh[3], pad[3];
    for (int i = 0; i < 3; ++i) {
      const bool fits = shrink && size[i] <= full[i];
      win[i] = fits ? size[i] : full[i];
      sh[i] = fits ? 0 : roll[i];
      pad[i] = (size[i] + win[i] - 1) / win[i] * win[i];
    }
    g.wd = win[0]; g.wh = win[1]; g.ww = win[2];
    g.sd = sh[0]; g.sh = sh[1]; g.sw = sh[2];
    g.Dp = pad[0]; g.Hp = pad[1]; g.Wp = pad[2];
    return g;
  }
};

}  // namespace
