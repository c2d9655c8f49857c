// RoBERTa text encoder pieces that the GEMM / LayerNorm kernels do not already cover
// (reference call site: models/tce_rvos.py:406-424; arithmetic: HuggingFace RobertaModel).
#include "common.h"
#include "../../include/tce_rvos.h"

namespace {

// embeddings: word[ids] + position[pos_ids] + token_type[0] -> LayerNorm.  One wavefront per token.
__global__ void __launch_bounds__(256) embed_ln_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ pos_ids,
                                                       const float* __restrict__ word, const float* __restrict__ pos,
                                                       const float* __restrict__ type0, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float* __restrict__ out, int L,
                                                       int C, float eps, int pad_id, int seq_len) {
  const int lane = threadIdx.x & 63;
  const int tok = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tok >= L) return;
  long long pid;
  if (pos_ids) {
    pid = pos_ids[tok];
  } else {
    // HF create_position_ids_from_input_ids: pad + (number of non-pad tokens up to and including this one), pad -> pad;
    // seq_len: the L tokens are L / seq_len captions of equal length, the count restarts at each caption
    int cnt = 0;
    for (int i = (tok / seq_len) * seq_len + lane; i <= tok; i += 64) cnt += ids[i] != pad_id;
    cnt = (int)wave_sum((float)cnt);
    pid = ids[tok] != pad_id ? pad_id + cnt : pad_id;
  }
  const f32x4* w4 = reinterpret_cast<const f32x4*>(word + ids[tok] * C);
  const f32x4* p4 = reinterpret_cast<const f32x4*>(pos + pid * C);
  const f32x4* t4 = reinterpret_cast<const f32x4*>(type0);
  const int n4 = C >> 2;
  float s = 0.f;
  for (int i = lane; i < n4; i += 64) {
    const f32x4 v = w4[i] + t4[i] + p4[i];
    s += (v[0] + v[1]) + (v[2] + v[3]);
  }
  const float mean = wave_sum(s) / (float)C;
  float q = 0.f;
  for (int i = lane; i < n4; i += 64) {
    const f32x4 v = w4[i] + t4[i] + p4[i];
    const float a = v[0] - mean, b = v[1] - mean, c = v[2] - mean, d = v[3] - mean;
    q += (a * a + b * b) + (c * c + d * d);
  }
  const float rstd = rsqrtf(wave_sum(q) / (float)C + eps);
  const f32x4* g4 = reinterpret_cast<const f32x4*>(gamma);
  const f32x4* b4 = reinterpret_cast<const f32x4*>(beta);
  f32x4* o4 = reinterpret_cast<f32x4*>(out + (long long)tok * C);
  for (int i = lane; i < n4; i += 64) {
    const f32x4 v = w4[i] + t4[i] + p4[i], g = g4[i], b = b4[i];
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (v[j] - mean) * rstd * g[j] + b[j];
    o4[i] = o;
  }
}

// The keys sK / sV[0 .. n) of one staged tile folded into a query quarter's running softmax (m, l, o[]), one key at a time.  Both
// attention kernels below walk their keys through this one body, so a key meets the same statements in the same order whether the
// sentence was staged whole or in tiles: the result of a row depends on its keys and their order only, not on the kernel.
template <int HDIM>
__device__ __forceinline__ void mha_fold_keys(const float* __restrict__ sK, const float* __restrict__ sV, int n, int part,
                                              const float (&q)[HDIM / 4], float& m, float& l, float (&o)[HDIM / 4]) {
  constexpr int QD = HDIM / 4;
  for (int j = 0; j < n; ++j) {
    const f32x4* kp = reinterpret_cast<const f32x4*>(&sK[j * HDIM + part * QD]);
    float a = 0.f;
#pragma unroll
    for (int d4 = 0; d4 < QD / 4; ++d4) {
      const f32x4 kv = kp[d4];
      a = fmaf(q[d4 * 4 + 0], kv[0], a);
      a = fmaf(q[d4 * 4 + 1], kv[1], a);
      a = fmaf(q[d4 * 4 + 2], kv[2], a);
      a = fmaf(q[d4 * 4 + 3], kv[3], a);
    }
    a += __shfl_xor(a, 1, 64);
    a += __shfl_xor(a, 2, 64);
    const float mnew = fmaxf(m, a);
    const float corr = __expf(m - mnew), pj = __expf(a - mnew);
    l = l * corr + pj;
    const f32x4* vp = reinterpret_cast<const f32x4*>(&sV[j * HDIM + part * QD]);
#pragma unroll
    for (int d4 = 0; d4 < QD / 4; ++d4) {
      const f32x4 vv = vp[d4];
#pragma unroll
      for (int c = 0; c < 4; ++c) o[d4 * 4 + c] = fmaf(pj, vv[c], o[d4 * 4 + c] * corr);
    }
    m = mnew;
  }
}

// Short-sequence self-attention with head_dim 64 (12 heads x 64 for RoBERTa-base).  One workgroup per (head, block of 32
// queries, sequence), four lanes per query.  Two kernels share this contract: mha_small_kernel keeps K and V of the whole
// sentence (L <= LMAX = 128 tokens) in LDS; mha_tiled_kernel below walks longer sentences (the launchers send it 129..512
// tokens, RoBERTa's position table) in tiles of TK keys.
// splits > 1 / bias: qkv is given as `splits` partial planes [L, 3E] (split-K partial sums, plane stride L*3E) + a bias [3E]:
// the reduction of the projection rides in this kernel's loads (no reduce launch between projection and attention).
// lens != NULL (right-padded captions of a ragged clip group): sequence z's keys stop at lens[z] (HF's attention_mask); every
// query row is still computed, pad rows included, each over the same keys in the same order as the un-padded sequence.
template <int HDIM, int LMAX>
__global__ void __launch_bounds__(256) mha_small_kernel(const float* __restrict__ qkv, float* __restrict__ out, int L,
                                                        int nheads, float scale, int splits, const float* __restrict__ bias,
                                                        const int* __restrict__ lens) {
  // gridDim.z sequences of L tokens stacked as rows: sequence z owns rows z*L .. z*L + L - 1 of every plane and of `out`
  __shared__ __attribute__((aligned(16))) float sK[LMAX * HDIM];
  __shared__ __attribute__((aligned(16))) float sV[LMAX * HDIM];
  const int h = blockIdx.x;
  const int E = nheads * HDIM;
  const int tid = threadIdx.x;
  const int Lk = lens ? min(max(lens[blockIdx.z], 1), L) : L;  // keys of this sequence
  const long long plane = (long long)L * gridDim.z * 3 * E;
  qkv += (long long)blockIdx.z * L * 3 * E;
  out += (long long)blockIdx.z * L * E;
  auto ld4 = [&](const float* p, int col) {  // sum of the partial planes (+ bias) at p
    f32x4 v = *reinterpret_cast<const f32x4*>(p);
    for (int s = 1; s < splits; ++s) v += *reinterpret_cast<const f32x4*>(p + s * plane);
    if (bias) v += *reinterpret_cast<const f32x4*>(bias + col);
    return v;
  };
  // 256 threads stage K / V (with partial planes that is three times the loads); the upper 128 leave after the barrier
  for (int i = tid; i < Lk * (HDIM / 4); i += 256) {
    const int j = i / (HDIM / 4), d4 = i % (HDIM / 4);
    const float* p = qkv + (long long)j * 3 * E + h * HDIM + d4 * 4;
    *reinterpret_cast<f32x4*>(&sK[j * HDIM + d4 * 4]) = ld4(p + E, E + h * HDIM + d4 * 4);
    *reinterpret_cast<f32x4*>(&sV[j * HDIM + d4 * 4]) = ld4(p + 2 * E, 2 * E + h * HDIM + d4 * 4);
  }
  __syncthreads();
  if (tid >= 128) return;
  // four lanes per query (a quarter of the head dim each): the score is a 16-term partial dot + two shuffles, the output
  // row is split the same way -- a thread per query walked the keys with 128 dependent FMAs each (19 us for 32 tokens)
  constexpr int QD = HDIM / 4;
  const int i = blockIdx.y * 32 + (tid >> 2), part = tid & 3;
  const int ic = min(i, L - 1);
  float q[QD];
  {
    const float* p = qkv + (long long)ic * 3 * E + h * HDIM + part * QD;
#pragma unroll
    for (int d4 = 0; d4 < QD / 4; ++d4) {
      const f32x4 v = ld4(p + d4 * 4, h * HDIM + part * QD + d4 * 4);
#pragma unroll
      for (int c = 0; c < 4; ++c) q[d4 * 4 + c] = v[c] * scale;
    }
  }
  float m = -3.0e38f, l = 0.f;
  float o[QD];
#pragma unroll
  for (int d = 0; d < QD; ++d) o[d] = 0.f;
  mha_fold_keys<HDIM>(sK, sV, Lk, part, q, m, l, o);  // online softmax, one key at a time (L is tiny)
  if (i >= L) return;
  const float inv = 1.f / l;
  float* po = out + (long long)i * E + h * HDIM + part * QD;
#pragma unroll
  for (int d4 = 0; d4 < QD / 4; ++d4) {
    f32x4 v = {o[d4 * 4] * inv, o[d4 * 4 + 1] * inv, o[d4 * 4 + 2] * inv, o[d4 * 4 + 3] * inv};
    *reinterpret_cast<f32x4*>(po + d4 * 4) = v;
  }
}

// The same attention for sentences that do not fit LDS whole: same arguments, same grid, same four lanes per query, but K and V
// pass through LDS in tiles of TK keys and (m, l, o[]) stay in registers from one tile to the next.  TK = 64 (2 x 16 KB of LDS): a
// workgroup alternates between staging and folding with nothing in flight across its barriers, so what covers a staging round
// trip is the other workgroups of the CU -- five of them at 32 KB against two at the 64 KB of a 128-key tile.
// Barriers: the trip count comes from Lk of blockIdx.z alone, so it is the same for all 256 threads, and every thread -- the upper
// 128 that only stage, and the idle queries i >= L of a last block -- runs every tile's two barriers; nothing returns before the
// loop ends and only the final store is predicated.  Tiles wholly past lens[z] are never entered.
template <int HDIM, int TK>
__global__ void __launch_bounds__(256) mha_tiled_kernel(const float* __restrict__ qkv, float* __restrict__ out, int L,
                                                        int nheads, float scale, int splits, const float* __restrict__ bias,
                                                        const int* __restrict__ lens) {
  __shared__ __attribute__((aligned(16))) float sK[TK * HDIM];
  __shared__ __attribute__((aligned(16))) float sV[TK * HDIM];
  const int h = blockIdx.x;
  const int E = nheads * HDIM;
  const int tid = threadIdx.x;
  const int Lk = lens ? min(max(lens[blockIdx.z], 1), L) : L;  // keys of this sequence: uniform over the workgroup
  const long long plane = (long long)L * gridDim.z * 3 * E;
  qkv += (long long)blockIdx.z * L * 3 * E;
  out += (long long)blockIdx.z * L * E;
  auto ld4 = [&](const float* p, int col) {  // sum of the partial planes (+ bias) at p
    f32x4 v = *reinterpret_cast<const f32x4*>(p);
    for (int s = 1; s < splits; ++s) v += *reinterpret_cast<const f32x4*>(p + s * plane);
    if (bias) v += *reinterpret_cast<const f32x4*>(bias + col);
    return v;
  };
  constexpr int QD = HDIM / 4;
  const bool folds = tid < 128;  // the upper 128 threads stage only
  const int i = blockIdx.y * 32 + ((tid & 127) >> 2), part = tid & 3;
  const int ic = min(i, L - 1);
  float q[QD];
#pragma unroll
  for (int d = 0; d < QD; ++d) q[d] = 0.f;
  if (folds) {
    const float* p = qkv + (long long)ic * 3 * E + h * HDIM + part * QD;
#pragma unroll
    for (int d4 = 0; d4 < QD / 4; ++d4) {
      const f32x4 v = ld4(p + d4 * 4, h * HDIM + part * QD + d4 * 4);
#pragma unroll
      for (int c = 0; c < 4; ++c) q[d4 * 4 + c] = v[c] * scale;
    }
  }
  float m = -3.0e38f, l = 0.f;
  float o[QD];
#pragma unroll
  for (int d = 0; d < QD; ++d) o[d] = 0.f;
  for (int k0 = 0; k0 < Lk; k0 += TK) {
    const int n = min(TK, Lk - k0);  // keys of this tile
    if (k0) __syncthreads();         // the previous tile has been folded by every query
    for (int e = tid; e < n * (HDIM / 4); e += 256) {
      const int j = e / (HDIM / 4), d4 = e % (HDIM / 4);
      const float* p = qkv + (long long)(k0 + j) * 3 * E + h * HDIM + d4 * 4;
      *reinterpret_cast<f32x4*>(&sK[j * HDIM + d4 * 4]) = ld4(p + E, E + h * HDIM + d4 * 4);
      *reinterpret_cast<f32x4*>(&sV[j * HDIM + d4 * 4]) = ld4(p + 2 * E, 2 * E + h * HDIM + d4 * 4);
    }
    __syncthreads();
    if (folds) mha_fold_keys<HDIM>(sK, sV, n, part, q, m, l, o);
  }
  if (!folds || i >= L) return;
  const float inv = 1.f / l;
  float* po = out + (long long)i * E + h * HDIM + part * QD;
#pragma unroll
  for (int d4 = 0; d4 < QD / 4; ++d4) {
    f32x4 v = {o[d4 * 4] * inv, o[d4 * 4 + 1] * inv, o[d4 * 4 + 2] * inv, o[d4 * 4 + 3] * inv};
    *reinterpret_cast<f32x4*>(po + d4 * 4) = v;
  }
}

// Caption lengths of right-padded ids [G, Lmax] (one workgroup per caption): lens[b] = index of the first pad id, Lmax if
// none, at least 1; kmask[b][j] = (j >= lens[b]); pos[b * Lmax + j][:] = PositionEmbeddingSine1D(normalize=True) with that
// mask (position_encoding.py:28-50): x = cumsum(not_mask) = min(j + 1, lens), x / (lens + 1e-6) * 2 pi, sin / cos interleaved.
__global__ void __launch_bounds__(256) caption_lens_kernel(const int64_t* __restrict__ ids, int Lmax, int pad_id, int D,
                                                           int* __restrict__ lens, unsigned char* __restrict__ kmask,
                                                           float* __restrict__ pos) {
  __shared__ int first;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) first = Lmax;
  __syncthreads();
  for (int j = tid; j < Lmax; j += 256)
    if (ids[(long long)b * Lmax + j] == pad_id) atomicMin(&first, j);
  __syncthreads();
  const int n = max(first, 1);
  if (tid == 0) lens[b] = n;
  for (int j = tid; j < Lmax; j += 256) kmask[(long long)b * Lmax + j] = j >= n;
  const float last = (float)n + 1e-6f;
  for (int e = tid; e < Lmax * D; e += 256) {
    const int j = e / D, c = e - j * D;
    const float x = (float)min(j + 1, n) / last * 6.28318530717958647692f;
    const float dim_t = powf(10000.0f, (float)(2 * (c >> 1)) / (float)D);
    const float a = x / dim_t;
    pos[(long long)b * Lmax * D + e] = (c & 1) ? cosf(a) : sinf(a);
  }
}

__global__ void __launch_bounds__(256) tanh_kernel(const float* __restrict__ x, float* __restrict__ out, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  // evaluated in double and rounded once: the device library's tanhf is 1.1 ulp off near |x| = 0.68 (tests/test_text_kernels_gpu.py
  // holds this to ~1 ulp, twice a host libm's error); the pooler's G * 768 elements make the cost nothing
  if (i < n) out[i] = (float)tanh((double)x[i]);
}

// The four tce_mha_small64_* entries share this dispatch: up to 128 tokens the whole-sentence kernel (the launch it has always
// been), 129 .. MHA_SMALL_LMAX the key-tiled one on the same grid.  The callers have checked 1 <= L <= MHA_SMALL_LMAX.
constexpr int MHA_SMALL_LMAX = 512;  // RoBERTa's position table (514 rows, ids from pad_id + 1)
void mha_small64_launch(dim3 grid, hipStream_t stream, const float* qkv, float* out, int L, int nheads, float scale, int splits,
                        const float* bias, const int* lens) {
  if (L <= 128)
    hipLaunchKernelGGL((mha_small_kernel<64, 128>), grid, dim3(256), 0, stream, qkv, out, L, nheads, scale, splits, bias, lens);
  else
    hipLaunchKernelGGL((mha_tiled_kernel<64, 64>), grid, dim3(256), 0, stream, qkv, out, L, nheads, scale, splits, bias, lens);
}

}  // namespace

extern "C" int tce_embed_ln_f32(const int64_t* ids, const int64_t* pos_ids, const float* word, const float* pos,
                                const float* type0, const float* gamma, const float* beta, float* out, int32_t L,
                                int32_t C, float eps, int32_t pad_id, tceStream stream) {
  TCE_CHECK_ARG(ids && word && pos && type0 && gamma && beta && out && L > 0 && C > 0 && C % 4 == 0,
                "tce_embed_ln_f32: bad arguments");
  hipLaunchKernelGGL(embed_ln_kernel, dim3(tce_cdiv(L, 4)), dim3(256), 0, (hipStream_t)stream, ids, pos_ids, word, pos,
                     type0, gamma, beta, out, L, C, eps, pad_id, L);
  TCE_CHECK_LAUNCH("tce_embed_ln_f32");
  return TCE_OK;
}

extern "C" int tce_embed_ln_seqs_f32(const int64_t* ids, const float* word, const float* pos, const float* type0, const float* gamma,
                                     const float* beta, float* out, int32_t nseq, int32_t seq_len, int32_t C, float eps, int32_t pad_id,
                                     tceStream stream) {
  TCE_CHECK_ARG(ids && word && pos && type0 && gamma && beta && out && nseq > 0 && seq_len > 0 && C > 0 && C % 4 == 0,
                "tce_embed_ln_seqs_f32: bad arguments");
  const int L = nseq * seq_len;
  hipLaunchKernelGGL(embed_ln_kernel, dim3(tce_cdiv(L, 4)), dim3(256), 0, (hipStream_t)stream, ids, (const int64_t*)nullptr, word, pos,
                     type0, gamma, beta, out, L, C, eps, pad_id, seq_len);
  TCE_CHECK_LAUNCH("tce_embed_ln_seqs_f32");
  return TCE_OK;
}

extern "C" int tce_mha_small64_f32(const float* qkv, float* out, int32_t L, int32_t nheads, float scale,
                                   tceStream stream) {
  TCE_CHECK_ARG(qkv && out && nheads > 0, "tce_mha_small64_f32: bad arguments");
  TCE_CHECK_ARG(L > 0 && L <= MHA_SMALL_LMAX, "tce_mha_small64_f32: sequence length %d outside 1..512", L);
  TCE_CHECK_ARG(tce_aligned16(qkv) && tce_aligned16(out), "tce_mha_small64_f32: pointers must be 16-byte aligned");
  mha_small64_launch(dim3(nheads, tce_cdiv(L, 32)), (hipStream_t)stream, qkv, out, L, nheads, scale, 1, (const float*)nullptr, (const int*)nullptr);
  TCE_CHECK_LAUNCH("tce_mha_small64_f32");
  return TCE_OK;
}

extern "C" int tce_mha_small64_splits_f32(const float* qkv_planes, int32_t splits, const float* bias, float* out, int32_t L,
                                          int32_t nheads, float scale, tceStream stream) {
  TCE_CHECK_ARG(qkv_planes && out && nheads > 0 && splits >= 1 && splits <= 64, "tce_mha_small64_splits_f32: bad arguments");
  TCE_CHECK_ARG(L > 0 && L <= MHA_SMALL_LMAX, "tce_mha_small64_splits_f32: sequence length %d outside 1..512", L);
  TCE_CHECK_ARG(tce_aligned16(qkv_planes) && tce_aligned16(out) && (!bias || tce_aligned16(bias)),
                "tce_mha_small64_splits_f32: pointers must be 16-byte aligned");
  mha_small64_launch(dim3(nheads, tce_cdiv(L, 32)), (hipStream_t)stream, qkv_planes, out, L, nheads, scale, splits, bias, (const int*)nullptr);
  TCE_CHECK_LAUNCH("tce_mha_small64_splits_f32");
  return TCE_OK;
}

extern "C" int tce_mha_small64_seqs_f32(const float* qkv_planes, int32_t splits, const float* bias, float* out, int32_t nseq, int32_t L,
                                        int32_t nheads, float scale, tceStream stream) {
  TCE_CHECK_ARG(qkv_planes && out && nheads > 0 && splits >= 1 && splits <= 64 && nseq > 0 && nseq <= 64, "tce_mha_small64_seqs_f32: bad arguments");
  TCE_CHECK_ARG(L > 0 && L <= MHA_SMALL_LMAX, "tce_mha_small64_seqs_f32: sequence length %d outside 1..512", L);
  TCE_CHECK_ARG(tce_aligned16(qkv_planes) && tce_aligned16(out) && (!bias || tce_aligned16(bias)),
                "tce_mha_small64_seqs_f32: pointers must be 16-byte aligned");
  mha_small64_launch(dim3(nheads, tce_cdiv(L, 32), nseq), (hipStream_t)stream, qkv_planes, out, L, nheads, scale, splits, bias, (const int*)nullptr);
  TCE_CHECK_LAUNCH("tce_mha_small64_seqs_f32");
  return TCE_OK;
}

extern "C" int tce_mha_small64_lens_f32(const float* qkv_planes, int32_t splits, const float* bias, float* out, int32_t nseq,
                                        int32_t L, int32_t nheads, float scale, const int32_t* lens, tceStream stream) {
  TCE_CHECK_ARG(qkv_planes && out && lens && nheads > 0 && splits >= 1 && splits <= 64 && nseq > 0 && nseq <= 64,
                "tce_mha_small64_lens_f32: bad arguments");
  TCE_CHECK_ARG(L > 0 && L <= MHA_SMALL_LMAX, "tce_mha_small64_lens_f32: sequence length %d outside 1..512", L);
  TCE_CHECK_ARG(tce_aligned16(qkv_planes) && tce_aligned16(out) && (!bias || tce_aligned16(bias)),
                "tce_mha_small64_lens_f32: pointers must be 16-byte aligned");
  mha_small64_launch(dim3(nheads, tce_cdiv(L, 32), nseq), (hipStream_t)stream, qkv_planes, out, L, nheads, scale, splits, bias, (const int*)lens);
  TCE_CHECK_LAUNCH("tce_mha_small64_lens_f32");
  return TCE_OK;
}

extern "C" int tce_caption_lens_f32(const int64_t* ids, int32_t nseq, int32_t Lmax, int32_t pad_id, int32_t D, int32_t* lens,
                                    uint8_t* kmask, float* pos, tceStream stream) {
  TCE_CHECK_ARG(ids && lens && kmask && pos && nseq > 0 && Lmax > 0 && D > 0 && D % 2 == 0, "tce_caption_lens_f32: bad arguments");
  hipLaunchKernelGGL(caption_lens_kernel, dim3(nseq), dim3(256), 0, (hipStream_t)stream, ids, Lmax, pad_id, D, (int*)lens,
                     (unsigned char*)kmask, pos);
  TCE_CHECK_LAUNCH("tce_caption_lens_f32");
  return TCE_OK;
}

extern "C" int tce_tanh_f32(const float* x, float* out, int64_t n, tceStream stream) {
  TCE_CHECK_ARG(x && out && n > 0, "tce_tanh_f32: bad arguments");
  hipLaunchKernelGGL(tanh_kernel, dim3(tce_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x, out, (long long)n);
  TCE_CHECK_LAUNCH("tce_tanh_f32");
  return TCE_OK;
}
