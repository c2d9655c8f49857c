// SetCriterion and its one-target matcher (train/tce_rvos_train.h).  Forward: a streaming walk of the mask logits that leaves three
// fp64 sums per query, and a workgroup per clip that turns them and the few hundred other numbers of a clip into the cost column,
// the match and the loss parts.  Backward: one launch that writes the gradient of the mask logits from those sums, one for the three
// heads.  This translation unit is the whole of libtce_rvos_train.so.
#define tce_set_error tce_train_set_error  // common.h's macros report into this library's own last-error string
#include "../csrc/common.h"

#include <stdarg.h>

#include "../../train/tce_rvos_train.h"

static thread_local char g_train_err[512] = "";

void tce_train_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_train_err, sizeof(g_train_err), fmt, ap);
  va_end(ap);
}

extern "C" int32_t tce_train_abi_version(void) { return TCE_TRAIN_ABI_VERSION; }
extern "C" const char* tce_train_last_error(void) { return g_train_err; }

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The sum of v over the workgroup, in every thread; red: WAVES doubles of LDS.  Fixed tree: the same bits on every run.
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
  v = wave_sum_f64(v);
  __syncthreads();  // red may still be read from an earlier call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int i = 1; i < WAVES; ++i) s += red[i];
  return s;
}

// The per-element terms of the header: f (focal) and s (sigmoid) of logit v against target tv
__device__ __forceinline__ void focal_terms(const float v, const bool tv, const float alpha, const float one_minus_alpha, float& f,
                                            float& s) {
#pragma clang fp contract(off)
  const float z = tv ? -v : v;
  const float e = expf(-fabsf(v));
  const float r = 1.f / (1.f + e);
  const float er = e * r;
  s = v >= 0.f ? r : er;
  const float m = z >= 0.f ? r : er;
  const float ce = fmaxf(z, 0.f) + log1pf(e);
  f = (tv ? alpha : one_minus_alpha) * (ce * (m * m));
}

struct SumsArgs {
  const float* pred;
  const uint8_t* tgt;
  double* ws;  // [B,Q,G,4]
  int T, Q, h, w, H, W, G, chunk;
  float alpha, one_minus_alpha;
};

// blockIdx = (chunk of the query's T*h*w elements, query, clip)
template <bool VEC>
__global__ void __launch_bounds__(THREADS) mask_sums_kernel(const SumsArgs a) {
  __shared__ double red[WAVES];
  const int g = blockIdx.x, q = blockIdx.y, b = blockIdx.z;
  const int hw = a.h * a.w, N = a.T * hw;
  const int lo = g * a.chunk, hi = min(N, lo + a.chunk);
  const float* __restrict__ pred = a.pred + ((long long)b * a.T * a.Q + q) * hw;  // + t*Q*hw + rem
  const uint8_t* __restrict__ tgt = a.tgt + (long long)b * a.T * a.H * a.W;
  const long long tstride = (long long)a.Q * hw;
  double sf = 0., sp = 0., spt = 0., stv = 0.;
  constexpr int STEP = VEC ? 4 : 1;
  for (int e = lo + (int)threadIdx.x * STEP; e < hi; e += THREADS * STEP) {
    const int t = e / hw, rem = e - t * hw, y = rem / a.w, x = rem - y * a.w;
    float v[STEP];
    if constexpr (VEC) {  // w % 4 == 0: the four elements lie in one row; N % 4 == 0: e + 3 < N
      const f32x4 q4 = *(const f32x4*)(pred + t * tstride + rem);
#pragma unroll
      for (int j = 0; j < STEP; ++j) v[j] = q4[j];
    } else {
      v[0] = pred[t * tstride + rem];
    }
    const int yy = 4 * y + 2;
    const uint8_t* row = tgt + ((long long)t * a.H + yy) * a.W;
#pragma unroll
    for (int j = 0; j < STEP; ++j) {
      const int xx = 4 * (x + j) + 2;
      const bool tv = (yy < a.H && xx < a.W) ? row[xx] != 0 : false;
      float f, s;
      focal_terms(v[j], tv, a.alpha, a.one_minus_alpha, f, s);
      sf += (double)f;
      sp += (double)s;
      if (tv) {
        spt += (double)s;
        stv += 1.;
      }
    }
  }
  sf = block_sum_f64(sf, red);
  sp = block_sum_f64(sp, red);
  spt = block_sum_f64(spt, red);
  stv = block_sum_f64(stv, red);
  if (threadIdx.x == 0) {
    double* o = a.ws + (((long long)b * a.Q + q) * a.G + g) * 4;
    o[0] = sf, o[1] = sp, o[2] = spt, o[3] = stv;
  }
}

// blockIdx.x = clip: the workgroup partials of ws added in index order
__global__ void __launch_bounds__(THREADS) mask_sums_reduce_kernel(const double* __restrict__ ws, double* __restrict__ sums,
                                                                   double* __restrict__ st, const int Q, const int G) {
  const int b = blockIdx.x;
  for (int i = threadIdx.x; i < 3 * Q + 1; i += THREADS) {
    const int k = i / Q, q = i - k * Q;  // i == 3Q: k = 3, q = 0 (S_t is the same from every query; query 0's is taken)
    const double* p = ws + ((long long)b * Q + q) * G * 4 + k;
    double s = 0.;
    for (int g = 0; g < G; ++g) s += p[g * 4];
    if (k < 3)
      sums[((long long)b * 3 + k) * Q + q] = s;
    else
      st[b] = s;
  }
}

struct MatchArgs {
  const float *logits, *pred_boxes, *visible;
  const double *sums, *st;
  const int64_t* labels;
  const float* boxes;
  const int32_t* valid;
  float* cost;
  int32_t* index;
  double* parts;
  int T, Q, K, N;  // N = T*h*w
  tceCriterionConsts c;
};

// matcher.py:154-159 / :210-214
__device__ __forceinline__ float cls_cost(const float x) {
#pragma clang fp contract(off)
  const float p = 1.f / (1.f + expf(-x));
  const float omp = 1.f - p;
  const float neg = (0.75f * (p * p)) * (-logf(omp + 1e-8f));
  const float pos = (0.25f * (omp * omp)) * (-logf(p + 1e-8f));
  return pos - neg;
}

// util/box_ops.py:29-33, 44-81 for one pair of cxcywh boxes
__device__ __forceinline__ float giou_cxcywh(const float* p, const float* g) {
#pragma clang fp contract(off)
  const float x0 = p[0] - 0.5f * p[2], y0 = p[1] - 0.5f * p[3], x1 = p[0] + 0.5f * p[2], y1 = p[1] + 0.5f * p[3];
  const float gx0 = g[0] - 0.5f * g[2], gy0 = g[1] - 0.5f * g[3], gx1 = g[0] + 0.5f * g[2], gy1 = g[1] + 0.5f * g[3];
  const float area_p = (x1 - x0) * (y1 - y0), area_g = (gx1 - gx0) * (gy1 - gy0);
  const float inter = fmaxf(fminf(x1, gx1) - fmaxf(x0, gx0), 0.f) * fmaxf(fminf(y1, gy1) - fmaxf(y0, gy0), 0.f);
  const float uni = (area_p + area_g) - inter;
  const float iou = (inter + 1e-6f) / (uni + 1e-6f);
  const float area = fmaxf(fmaxf(x1, gx1) - fminf(x0, gx0), 0.f) * fmaxf(fmaxf(y1, gy1) - fminf(y0, gy0), 0.f);
  return iou - ((area - uni) + 1e-6f) / (area + 1e-6f);
}

__device__ __forceinline__ float l1_4(const float* p, const float* g) {
#pragma clang fp contract(off)
  return ((fabsf(p[0] - g[0]) + fabsf(p[1] - g[1])) + fabsf(p[2] - g[2])) + fabsf(p[3] - g[3]);
}

// blockIdx.x = clip
__global__ void __launch_bounds__(THREADS) match_losses_kernel(const MatchArgs a) {
#pragma clang fp contract(off)
  __shared__ double red[WAVES];
  __shared__ float best_c[THREADS];
  __shared__ int best_i[THREADS];
  __shared__ int s_valid[TCE_CRIT_MAX_T], s_cls[TCE_CRIT_MAX_T];
  const int b = blockIdx.x, T = a.T, Q = a.Q, K = a.K, tid = threadIdx.x;
  const float* logits = a.logits + (long long)b * T * Q * K;
  const float* pboxes = a.pred_boxes + (long long)b * T * Q * 4;
  const float* vis = a.visible ? a.visible + (long long)b * T * Q : nullptr;
  const float* tboxes = a.boxes + (long long)b * T * 4;
  for (int t = tid; t < T; t += THREADS) {
    s_valid[t] = a.valid[b * T + t] != 0;
    const long long l = a.labels[b * T + t];
    s_cls[t] = K == 1 ? 0 : (int)(l < 0 ? 0 : (l > K - 1 ? K - 1 : l));
  }
  __syncthreads();
  int nvalid = 0;
  for (int t = 0; t < T; ++t) nvalid += s_valid[t];
  const double S_t = a.sums ? a.st[b] : 0.;

  float mine_c = INFINITY;
  int mine_i = 0x7fffffff;
  for (int q = tid; q < Q; q += THREADS) {
    float C = 0.f;
    if (nvalid > 0) {
      float acc = 0.f, accb = 0.f, accg = 0.f;
      for (int t = 0; t < T; ++t) {
        if (!s_valid[t]) continue;
        acc += cls_cost(logits[((long long)t * Q + q) * K + s_cls[t]]);
        accb += l1_4(pboxes + ((long long)t * Q + q) * 4, tboxes + t * 4);
        accg += -giou_cxcywh(pboxes + ((long long)t * Q + q) * 4, tboxes + t * 4);
      }
      C += a.c.cost_class * (acc / (float)nvalid);
      C += a.c.cost_bbox * (accb / (float)nvalid);
      C += a.c.cost_giou * (accg / (float)nvalid);
    }
    if (vis) {
      float acc = 0.f;
      for (int t = 0; t < T; ++t) acc += cls_cost(vis[t * Q + q]);
      C += a.c.cost_vis * (acc / (float)T);
    }
    if (a.sums) {
      const double* s = a.sums + (long long)b * 3 * Q;
      const float fm = (float)(s[q] / (double)a.N);
      const float dc = (float)((2. * s[2 * Q + q] + 1.) / (s[Q + q] + S_t + 1.));
      C += a.c.cost_mask * fm + a.c.cost_dice * (-dc);
    }
    a.cost[(long long)b * Q + q] = C;
    if (C < mine_c) mine_c = C, mine_i = q;  // q ascends within a thread: a tie keeps the lower index
  }
  best_c[tid] = mine_c, best_i[tid] = mine_i;
  __syncthreads();
  for (int o = THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) {
      const float c2 = best_c[tid + o];
      const int i2 = best_i[tid + o];
      if (c2 < best_c[tid] || (c2 == best_c[tid] && i2 < best_i[tid])) best_c[tid] = c2, best_i[tid] = i2;
    }
    __syncthreads();
  }
  const int idx = best_i[0] == 0x7fffffff ? 0 : best_i[0];

  // loss_ce: every logit against the one-hot of the matched query's valid frames
  const float alpha = a.c.focal_alpha, oma = 1.f - a.c.focal_alpha;
  double ce = 0.;
  const int QK = Q * K, TQK = T * QK;
  for (int i = tid; i < TQK; i += THREADS) {
    const int t = i / QK, r = i - t * QK, q = r / K, k = r - q * K;
    float f, s;
    focal_terms(logits[i], s_valid[t] && q == idx && k == s_cls[t], alpha, oma, f, s);
    ce += (double)f;
  }
  ce = block_sum_f64(ce, red);
  if (tid == 0) {
    double lb = 0., lg = 0., lv = 0.;
    for (int t = 0; t < T; ++t) {
      lb += (double)l1_4(pboxes + ((long long)t * Q + idx) * 4, tboxes + t * 4);
      lg += (double)(1.f - giou_cxcywh(pboxes + ((long long)t * Q + idx) * 4, tboxes + t * 4));
      if (vis) {
        float f, s;
        focal_terms(vis[t * Q + idx], s_valid[t] != 0, alpha, oma, f, s);
        lv += (double)f;
      }
    }
    double* o = a.parts + (long long)b * 6;
    o[0] = ce, o[1] = lb, o[2] = lg;
    if (a.sums) {
      const double* s = a.sums + (long long)b * 3 * Q;
      o[3] = s[idx] / (double)a.N;
      o[4] = 1. - (2. * s[2 * Q + idx] + 1.) / (s[Q + idx] + S_t + 1.);
    } else {
      o[3] = 0., o[4] = 0.;
    }
    o[5] = lv / (double)T / (double)T * (double)(T * Q);
    a.index[b] = idx;
  }
}

// one wavefront: the batch's six losses
__global__ void __launch_bounds__(64) losses_kernel(const double* __restrict__ parts, const float* __restrict__ num_boxes,
                                                    float* __restrict__ losses, const int B) {
  const int j = threadIdx.x;
  if (j >= 6) return;
  double s = 0.;
  for (int b = 0; b < B; ++b) s += parts[b * 6 + j];
  losses[j] = (float)(j < 5 ? s / (double)num_boxes[0] : s);
}

// ---- the backward of the losses (header (c), (d)) ---------------------------------------------------------------------------------
// d f / d v and s * (1 - s) of the header's per-element chain
__device__ __forceinline__ void focal_grad_terms(const float v, const bool tv, const float alpha, const float one_minus_alpha,
                                                 float& dfs, float& ds) {
#pragma clang fp contract(off)
  const float z = tv ? -v : v;
  const float e = expf(-fabsf(v));
  const float r = 1.f / (1.f + e);
  const float er = e * r;
  const float s = v >= 0.f ? r : er;
  const float sc = v >= 0.f ? er : r;
  const float m = z >= 0.f ? r : er;
  const float mc = z >= 0.f ? er : r;
  const float ce = fmaxf(z, 0.f) + log1pf(e);
  const float df = (tv ? alpha : one_minus_alpha) * ((m * m) * (m + 2.f * (ce * mc)));
  dfs = tv ? -df : df;
  ds = s * sc;
}

struct MaskGradArgs {
  const float* pred;
  const uint8_t* tgt;
  const double *sums, *st;
  const int32_t* index;
  const float *num_boxes, *gl;
  float* grad;
  int T, Q, h, w, H, W, chunk;
  float alpha, one_minus_alpha;
};

// blockIdx = (chunk of the query's T*h*w elements, query, clip); four consecutive elements of one row per thread and step
// (w % 4 == 0).  PV / GV: 16-byte loads of pred / stores of grad; the arithmetic is the same in all four forms.
template <bool PV, bool GV>
__global__ void __launch_bounds__(THREADS) mask_grad_kernel(const MaskGradArgs a) {
#pragma clang fp contract(off)
  const int g = blockIdx.x, q = blockIdx.y, b = blockIdx.z;
  const int hw = a.h * a.w, N = a.T * hw;
  const int lo = g * a.chunk, hi = min(N, lo + a.chunk);
  const long long base = ((long long)b * a.T * a.Q + q) * hw, tstride = (long long)a.Q * hw;
  float* __restrict__ grad = a.grad + base;
  const int idx = a.index[b];
  if (q != idx) {
    for (int e = lo + (int)threadIdx.x * 4; e < hi; e += THREADS * 4) {
      const int t = e / hw, rem = e - t * hw;
      float* o = grad + t * tstride + rem;
      if constexpr (GV) {
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        *(f32x4*)o = zero;
      } else {
        o[0] = 0.f, o[1] = 0.f, o[2] = 0.f, o[3] = 0.f;
      }
    }
    return;
  }
  // the block-uniform factors: fp64, rounded once
  const double* s = a.sums + (long long)b * 3 * a.Q;
  const double n = (double)a.num_boxes[0];
  const double D = s[a.Q + idx] + a.st[b] + 1.;
  const double num = (2. * s[2 * a.Q + idx] + 1.) / (D * D);
  const double gd = (double)a.gl[4] / n;
  const float Gm = (float)((double)a.gl[3] / n / (double)N);
  const float Gd0 = (float)(gd * num), Gd1 = (float)(gd * (num - 2. / D));
  const float* __restrict__ pred = a.pred + base;
  const uint8_t* __restrict__ tgt = a.tgt + (long long)b * a.T * a.H * a.W;
  for (int e = lo + (int)threadIdx.x * 4; e < hi; e += THREADS * 4) {
    const int t = e / hw, rem = e - t * hw, y = rem / a.w, x = rem - y * a.w;
    const float* p = pred + t * tstride + rem;
    float v[4], o4[4];
    if constexpr (PV) {
      const f32x4 q4 = *(const f32x4*)p;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = q4[j];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = p[j];
    }
    const int yy = 4 * y + 2;
    const uint8_t* row = tgt + ((long long)t * a.H + yy) * a.W;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int xx = 4 * (x + j) + 2;
      const bool tv = (yy < a.H && xx < a.W) ? row[xx] != 0 : false;
      float dfs, ds;
      focal_grad_terms(v[j], tv, a.alpha, a.one_minus_alpha, dfs, ds);
      o4[j] = Gm * dfs + (tv ? Gd1 : Gd0) * ds;
    }
    float* o = grad + t * tstride + rem;
    if constexpr (GV) {
      const f32x4 r4 = {o4[0], o4[1], o4[2], o4[3]};
      *(f32x4*)o = r4;
    } else {
      o[0] = o4[0], o[1] = o4[1], o[2] = o4[2], o[3] = o4[3];
    }
  }
}

struct HeadGradArgs {
  const float *logits, *pred_boxes, *visible;
  const int64_t* labels;
  const float* boxes;
  const int32_t *valid, *index;
  const float *num_boxes, *gl;
  float *g_logits, *g_boxes, *g_visible;
  int T, Q, K;
  float alpha;
};

// d(1 - giou)/d(cx, cy, w, h) of the predicted box: giou_cxcywh's chain in reverse (header (d))
__device__ __forceinline__ void giou_loss_grad(const float* p, const float* g, float* d) {
#pragma clang fp contract(off)
  const float x0 = p[0] - 0.5f * p[2], y0 = p[1] - 0.5f * p[3], x1 = p[0] + 0.5f * p[2], y1 = p[1] + 0.5f * p[3];
  const float gx0 = g[0] - 0.5f * g[2], gy0 = g[1] - 0.5f * g[3], gx1 = g[0] + 0.5f * g[2], gy1 = g[1] + 0.5f * g[3];
  const float wp = x1 - x0, hp = y1 - y0;
  const float area_p = wp * hp, area_g = (gx1 - gx0) * (gy1 - gy0);
  const float ax = fminf(x1, gx1) - fmaxf(x0, gx0), ay = fminf(y1, gy1) - fmaxf(y0, gy0);
  const float iw = fmaxf(ax, 0.f), ih = fmaxf(ay, 0.f);
  const float inter = iw * ih;
  const float uni = (area_p + area_g) - inter;
  const float du = uni + 1e-6f;
  const float iou = (inter + 1e-6f) / du;
  const float cx = fmaxf(x1, gx1) - fminf(x0, gx0), cy = fmaxf(y1, gy1) - fminf(y0, gy0);
  const float ew = fmaxf(cx, 0.f), eh = fmaxf(cy, 0.f);
  const float area = ew * eh;
  const float da = area + 1e-6f;
  const float r2 = ((area - uni) + 1e-6f) / da;
  // L = 1 - (iou - r2)
  const float d_area = (1.f - r2) / da;            // r2 = ((area - uni) + eps) / (area + eps)
  const float d_uni = iou / du - 1.f / da;         // through both quotients
  const float d_inter = (-1.f / du) - d_uni;       // directly, and through uni = (area_p + area_g) - inter
  const float d_iw = d_inter * ih, d_ih = d_inter * iw;
  const float d_ew = d_area * eh, d_eh = d_area * ew;
  const float d_wp = d_uni * hp, d_hp = d_uni * wp;  // d_area_p = d_uni
  float d_x0 = -d_wp, d_x1 = d_wp, d_y0 = -d_hp, d_y1 = d_hp;
  if (ax > 0.f) {  // a clamp at exactly 0 passes nothing; equal arguments: the predicted box's corner takes the whole gradient
    if (x1 <= gx1) d_x1 += d_iw;
    if (x0 >= gx0) d_x0 -= d_iw;
  }
  if (ay > 0.f) {
    if (y1 <= gy1) d_y1 += d_ih;
    if (y0 >= gy0) d_y0 -= d_ih;
  }
  if (cx > 0.f) {
    if (x1 >= gx1) d_x1 += d_ew;
    if (x0 <= gx0) d_x0 -= d_ew;
  }
  if (cy > 0.f) {
    if (y1 >= gy1) d_y1 += d_eh;
    if (y0 <= gy0) d_y0 -= d_eh;
  }
  d[0] = d_x0 + d_x1, d[1] = d_y0 + d_y1, d[2] = 0.5f * (d_x1 - d_x0), d[3] = 0.5f * (d_y1 - d_y0);
}

// blockIdx = (slice of the clip's T*Q*K logits, clip); the first T*Q threads of a clip also own a box and a visibility logit
__global__ void __launch_bounds__(THREADS) head_grads_kernel(const HeadGradArgs a) {
#pragma clang fp contract(off)
  const int b = blockIdx.y, T = a.T, Q = a.Q, K = a.K;
  const int i = blockIdx.x * THREADS + (int)threadIdx.x;
  const int idx = a.index[b];
  const double n = (double)a.num_boxes[0];
  const float oma = 1.f - a.alpha;
  if (a.g_logits && i < T * Q * K) {
    const int t = i / (Q * K), r = i - t * (Q * K), q = r / K, k = r - q * K;
    const long long l = a.labels[b * T + t];
    const int c = K == 1 ? 0 : (int)(l < 0 ? 0 : (l > K - 1 ? K - 1 : l));
    const long long at = (long long)b * T * Q * K + i;
    float dfs, ds;
    focal_grad_terms(a.logits[at], a.valid[b * T + t] != 0 && q == idx && k == c, a.alpha, oma, dfs, ds);
    a.g_logits[at] = (float)((double)a.gl[0] / n) * dfs;
  }
  if (i < T * Q) {
    const int t = i / Q, q = i - t * Q;
    const long long at = (long long)b * T * Q + i;
    if (a.g_visible) {
      float dfs = 0.f, ds;
      if (q == idx) {
        focal_grad_terms(a.visible[at], a.valid[b * T + t] != 0, a.alpha, oma, dfs, ds);
        dfs = (float)((double)a.gl[5] * (double)Q / (double)T) * dfs;
      }
      a.g_visible[at] = dfs;
    }
    if (a.g_boxes) {
      float o[4] = {0.f, 0.f, 0.f, 0.f};
      if (q == idx) {
        const float* p = a.pred_boxes + at * 4;
        const float* g = a.boxes + ((long long)b * T + t) * 4;
        const float c1 = (float)((double)a.gl[1] / n), c2 = (float)((double)a.gl[2] / n);
        float d[4];
        giou_loss_grad(p, g, d);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float df = p[j] - g[j];
          o[j] = c1 * (df > 0.f ? 1.f : (df < 0.f ? -1.f : 0.f)) + c2 * d[j];
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) a.g_boxes[at * 4 + j] = o[j];
    }
  }
}

int sums_groups(long long N) { return tce_cdiv(N, TCE_CRIT_CHUNK); }

}  // namespace

#define CRIT_CHECK_EXTENTS(name)                                                                                          \
  TCE_CHECK_ARG(B >= 1 && B <= TCE_CRIT_MAX_B, name ": 1..%d clips per call, got %d", TCE_CRIT_MAX_B, B);                 \
  TCE_CHECK_ARG(T >= 1 && T <= TCE_CRIT_MAX_T, name ": 1..%d frames per clip, got %d", TCE_CRIT_MAX_T, T);                \
  TCE_CHECK_ARG(Q >= 1 && Q <= TCE_CRIT_MAX_Q, name ": 1..%d queries, got %d", TCE_CRIT_MAX_Q, Q)

extern "C" int64_t tce_criterion_mask_sums_ws_bytes(int32_t B, int32_t T, int32_t Q, int32_t h, int32_t w) {
  if (B < 1 || B > TCE_CRIT_MAX_B || T < 1 || T > TCE_CRIT_MAX_T || Q < 1 || Q > TCE_CRIT_MAX_Q || h < 1 || w < 1 ||
      (long long)T * h * w >= (1ll << 30)) {
    tce_train_set_error("tce_criterion_mask_sums_ws_bytes: bad extents B=%d T=%d Q=%d h=%d w=%d", B, T, Q, h, w);
    return TCE_EINVAL;
  }
  return (int64_t)B * Q * sums_groups((long long)T * h * w) * 4 * (int64_t)sizeof(double);
}

extern "C" int tce_criterion_mask_sums_f64(const float* pred, const uint8_t* tgt, double* sums, double* st, void* ws, int32_t B,
                                           int32_t T, int32_t Q, int32_t h, int32_t w, int32_t H, int32_t W, float alpha,
                                           tceStream stream) {
  TCE_CHECK_ARG(pred && tgt && sums && st && ws, "tce_criterion_mask_sums_f64: null pointer");
  CRIT_CHECK_EXTENTS("tce_criterion_mask_sums_f64");
  TCE_CHECK_ARG(h >= 1 && w >= 1 && H >= 1 && W >= 1, "tce_criterion_mask_sums_f64: non-positive extent");
  TCE_CHECK_ARG((long long)T * h * w < (1ll << 30), "tce_criterion_mask_sums_f64: T*h*w must stay below 2^30");
  TCE_CHECK_ARG(4ll * h == ((long long)H + 31) / 32 * 32 && 4ll * w == ((long long)W + 31) / 32 * 32,
                "tce_criterion_mask_sums_f64: the mask plane %d x %d is not a quarter of the target %d x %d padded to a multiple of 32",
                h, w, H, W);
  TCE_CHECK_ARG((((uintptr_t)pred) & 3u) == 0 && ((((uintptr_t)sums) | ((uintptr_t)st) | ((uintptr_t)ws)) & 7u) == 0,
                "tce_criterion_mask_sums_f64: pred must be 4-byte, sums / st / ws 8-byte aligned");
  SumsArgs a;
  a.pred = pred, a.tgt = tgt, a.ws = (double*)ws;
  a.T = T, a.Q = Q, a.h = h, a.w = w, a.H = H, a.W = W;
  a.G = sums_groups((long long)T * h * w), a.chunk = TCE_CRIT_CHUNK;
  a.alpha = alpha, a.one_minus_alpha = 1.f - alpha;
  const dim3 grid(a.G, Q, B);
  if (tce_aligned16(pred) && w % 4 == 0)
    hipLaunchKernelGGL(mask_sums_kernel<true>, grid, dim3(THREADS), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(mask_sums_kernel<false>, grid, dim3(THREADS), 0, (hipStream_t)stream, a);
  TCE_CHECK_LAUNCH("tce_criterion_mask_sums_f64");
  hipLaunchKernelGGL(mask_sums_reduce_kernel, dim3(B), dim3(THREADS), 0, (hipStream_t)stream, (const double*)ws, sums, st, Q, a.G);
  TCE_CHECK_LAUNCH("tce_criterion_mask_sums_f64");
  return TCE_OK;
}

extern "C" int tce_criterion_match_losses_f32(const float* logits, const float* pred_boxes, const float* visible, const double* sums,
                                              const double* st, const int64_t* labels, const float* boxes, const int32_t* valid,
                                              const float* num_boxes, float* cost, int32_t* index, double* parts, float* losses,
                                              int32_t B, int32_t T, int32_t Q, int32_t K, int32_t h, int32_t w,
                                              const tceCriterionConsts* consts, tceStream stream) {
  TCE_CHECK_ARG(logits && pred_boxes && labels && boxes && valid && num_boxes && cost && index && parts && losses && consts,
                "tce_criterion_match_losses_f32: null pointer");
  CRIT_CHECK_EXTENTS("tce_criterion_match_losses_f32");
  TCE_CHECK_ARG(K >= 1 && K <= TCE_CRIT_MAX_K, "tce_criterion_match_losses_f32: 1..%d class logits, got %d", TCE_CRIT_MAX_K, K);
  TCE_CHECK_ARG((sums != nullptr) == (st != nullptr), "tce_criterion_match_losses_f32: sums and st come together or not at all");
  TCE_CHECK_ARG(!sums || (h >= 1 && w >= 1 && (long long)T * h * w < (1ll << 30)),
                "tce_criterion_match_losses_f32: bad mask plane %d x %d", h, w);
  TCE_CHECK_ARG(((((uintptr_t)logits) | ((uintptr_t)pred_boxes) | ((uintptr_t)visible) | ((uintptr_t)boxes) | ((uintptr_t)valid) |
                  ((uintptr_t)num_boxes) | ((uintptr_t)cost) | ((uintptr_t)index) | ((uintptr_t)losses)) & 3u) == 0 &&
                    ((((uintptr_t)sums) | ((uintptr_t)st) | ((uintptr_t)labels) | ((uintptr_t)parts)) & 7u) == 0,
                "tce_criterion_match_losses_f32: misaligned pointer (4 bytes for fp32 / int32, 8 for fp64 / int64)");
  MatchArgs a;
  a.logits = logits, a.pred_boxes = pred_boxes, a.visible = visible, a.sums = sums, a.st = st, a.labels = labels, a.boxes = boxes;
  a.valid = valid, a.cost = cost, a.index = index, a.parts = parts;
  a.T = T, a.Q = Q, a.K = K, a.N = sums ? T * h * w : 1;
  a.c = *consts;
  hipLaunchKernelGGL(match_losses_kernel, dim3(B), dim3(THREADS), 0, (hipStream_t)stream, a);
  TCE_CHECK_LAUNCH("tce_criterion_match_losses_f32");
  hipLaunchKernelGGL(losses_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)parts, num_boxes, losses, B);
  TCE_CHECK_LAUNCH("tce_criterion_match_losses_f32");
  return TCE_OK;
}

extern "C" int tce_criterion_mask_grad_f32(const float* pred, const uint8_t* tgt, const double* sums, const double* st,
                                           const int32_t* index, const float* num_boxes, const float* gl, float* grad, int32_t B,
                                           int32_t T, int32_t Q, int32_t h, int32_t w, int32_t H, int32_t W, float alpha,
                                           tceStream stream) {
  TCE_CHECK_ARG(pred && tgt && sums && st && index && num_boxes && gl && grad, "tce_criterion_mask_grad_f32: null pointer");
  CRIT_CHECK_EXTENTS("tce_criterion_mask_grad_f32");
  TCE_CHECK_ARG(h >= 1 && w >= 1 && H >= 1 && W >= 1, "tce_criterion_mask_grad_f32: non-positive extent");
  TCE_CHECK_ARG((long long)T * h * w < (1ll << 30), "tce_criterion_mask_grad_f32: T*h*w must stay below 2^30");
  TCE_CHECK_ARG(4ll * h == ((long long)H + 31) / 32 * 32 && 4ll * w == ((long long)W + 31) / 32 * 32,
                "tce_criterion_mask_grad_f32: the mask plane %d x %d is not a quarter of the target %d x %d padded to a multiple of 32",
                h, w, H, W);
  TCE_CHECK_ARG(((((uintptr_t)pred) | ((uintptr_t)grad) | ((uintptr_t)index) | ((uintptr_t)num_boxes) | ((uintptr_t)gl)) & 3u) == 0 &&
                    ((((uintptr_t)sums) | ((uintptr_t)st)) & 7u) == 0,
                "tce_criterion_mask_grad_f32: pred / grad / index / num_boxes / gl must be 4-byte, sums / st 8-byte aligned");
  MaskGradArgs a;
  a.pred = pred, a.tgt = tgt, a.sums = sums, a.st = st, a.index = index, a.num_boxes = num_boxes, a.gl = gl, a.grad = grad;
  a.T = T, a.Q = Q, a.h = h, a.w = w, a.H = H, a.W = W, a.chunk = TCE_CRIT_CHUNK;
  a.alpha = alpha, a.one_minus_alpha = 1.f - alpha;
  const dim3 grid(sums_groups((long long)T * h * w), Q, B), block(THREADS);
  const bool pv = tce_aligned16(pred), gv = tce_aligned16(grad);  // 4w == ceil32(W): w % 8 == 0, every row starts a 16-byte group
  if (pv && gv)
    hipLaunchKernelGGL((mask_grad_kernel<true, true>), grid, block, 0, (hipStream_t)stream, a);
  else if (pv)
    hipLaunchKernelGGL((mask_grad_kernel<true, false>), grid, block, 0, (hipStream_t)stream, a);
  else if (gv)
    hipLaunchKernelGGL((mask_grad_kernel<false, true>), grid, block, 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL((mask_grad_kernel<false, false>), grid, block, 0, (hipStream_t)stream, a);
  TCE_CHECK_LAUNCH("tce_criterion_mask_grad_f32");
  return TCE_OK;
}

extern "C" int tce_criterion_head_grads_f32(const float* logits, const float* pred_boxes, const float* visible, const int64_t* labels,
                                            const float* boxes, const int32_t* valid, const int32_t* index, const float* num_boxes,
                                            const float* gl, float* g_logits, float* g_boxes, float* g_visible, int32_t B, int32_t T,
                                            int32_t Q, int32_t K, const tceCriterionConsts* consts, tceStream stream) {
  TCE_CHECK_ARG(logits && pred_boxes && labels && boxes && valid && index && num_boxes && gl && consts,
                "tce_criterion_head_grads_f32: null pointer");
  TCE_CHECK_ARG(g_logits || g_boxes || g_visible, "tce_criterion_head_grads_f32: no output asked for");
  TCE_CHECK_ARG(!g_visible || visible, "tce_criterion_head_grads_f32: g_visible without visible");
  CRIT_CHECK_EXTENTS("tce_criterion_head_grads_f32");
  TCE_CHECK_ARG(K >= 1 && K <= TCE_CRIT_MAX_K, "tce_criterion_head_grads_f32: 1..%d class logits, got %d", TCE_CRIT_MAX_K, K);
  TCE_CHECK_ARG(((((uintptr_t)logits) | ((uintptr_t)pred_boxes) | ((uintptr_t)visible) | ((uintptr_t)boxes) | ((uintptr_t)valid) |
                  ((uintptr_t)index) | ((uintptr_t)num_boxes) | ((uintptr_t)gl) | ((uintptr_t)g_logits) | ((uintptr_t)g_boxes) |
                  ((uintptr_t)g_visible)) & 3u) == 0 && (((uintptr_t)labels) & 7u) == 0,
                "tce_criterion_head_grads_f32: misaligned pointer (4 bytes for fp32 / int32, 8 for int64)");
  HeadGradArgs a;
  a.logits = logits, a.pred_boxes = pred_boxes, a.visible = visible, a.labels = labels, a.boxes = boxes, a.valid = valid;
  a.index = index, a.num_boxes = num_boxes, a.gl = gl, a.g_logits = g_logits, a.g_boxes = g_boxes, a.g_visible = g_visible;
  a.T = T, a.Q = Q, a.K = K, a.alpha = consts->focal_alpha;
  const int items = g_logits ? T * Q * K : T * Q;  // <= 64 * 1024 * 128
  hipLaunchKernelGGL(head_grads_kernel, dim3(tce_cdiv(items, THREADS), B), dim3(THREADS), 0, (hipStream_t)stream, a);
  TCE_CHECK_LAUNCH("tce_criterion_head_grads_f32");
  return TCE_OK;
}
