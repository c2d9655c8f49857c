"""fp64 references, per-element first-order error bounds, input designs and fp32 CPU emulations (with planted defects) of the
normalisation, resampling, position-map, mask-head and contrastive launches of csrc/norm.hip and csrc/misc.hip.

Pure torch / numpy on the CPU.  Every bound is derived from the kernel's own operation order and the fp32 format (EPS = 2^-24 per
rounding); nothing is fitted to what a kernel returns.  Summation errors use the worst case n * EPS * sum|terms| with n the number of
additions on the longest path of that kernel's order (stated per kernel below with the lines of the source it is read from); a bound
composed of first-order terms is multiplied by 2 for the remainder, as everywhere in _arith.

Assumed accuracy of the device math functions (the HIP math accuracy table is not part of the ROCm installation this was written
against, so these are assumptions, each at least twice the figure the public HIP documentation gives): rsqrtf and sqrtf within 2 ulp,
powf within 4 ulp, sinf / cosf within 2 ulp (1 ulp = 2 EPS relative; 2 ulp of a sine <= 2 EPS absolute)."""
import math

import numpy as np
import torch

import _arith as A

F64 = torch.float64
F32 = torch.float32
EPS = A.EPS_F32
ULP = 2.0 * EPS
RSQRT_ERR = 2 * ULP      # rsqrtf / sqrtf, relative (assumption above)
POW_ERR = 4 * ULP        # powf, relative (assumption above)
SIN_ERR = 2 * EPS        # sinf / cosf, absolute (2 ulp of a value below 1)

FAMILIES = ("layernorm", "patch_merge_ln", "groupnorm", "groupnorm_up_add", "resize_nearest", "resize_bilinear", "resize_bilinear_ln",
            "pos_sine2d", "mask_head", "contrastive")


def gen(seed):
    return torch.Generator().manual_seed(int(seed))


def d64(x):
    return x.detach().cpu().to(F64)


def check(results, family, shape, design, out, ref, B):
    """Every element: |out - ref| <= B.  Appends (family, shape, design, max err / B) to results; an exact element is inside any
    bound (B = 0 included), NaN is outside every bound."""
    out, ref = d64(out).reshape(ref.shape), d64(ref)
    err = (out - ref).abs().nan_to_num(nan=float("inf"))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / B)
    i = int(ratio.argmax())
    rB = float(ratio.flatten()[i])
    results.append((family, shape, design, rB))
    if not bool((err <= B).all()):
        raise AssertionError(f"{family} {shape} [{design}]: {int((err > B).sum())} of {err.numel()} elements outside the bound; worst err/B = "
                             f"{rB:.3g} (out {float(out.flatten()[i]):.9e}, ref {float(ref.flatten()[i]):.9e}, B {float(B.flatten()[i]):.3e}) "
                             f"at flat index {i} of {tuple(ref.shape)}")
    return rB


def worst(out, ref, B):
    out, ref = d64(out).reshape(ref.shape), d64(ref)
    err = (out - ref).abs().nan_to_num(nan=float("inf"))
    return float(torch.where(err == 0, torch.zeros_like(err), err / B).max())


# =====================================================================================================================
# Row LayerNorm (tce_layernorm_f32) and the patch-merge LayerNorm
# =====================================================================================================================
LN_C = (4, 96, 128, 132, 192, 256, 260, 768, 3072)
LN_M = (1, 7, 9, 17, 1003)
LN_DESIGNS = ("unit", "offset", "decades", "epsprobe")
OFFSET_MU, OFFSET_SIGMA = 40.0, 0.05        # mu / sigma = 800
PROBE_SIGMA = 2.0 ** -8


def ln_n(C):
    """Additions on the longest path of a row sum.
    layernorm_reg_kernel<32> (C <= 128; norm.hip:70-72): the lane's quad (v0 + v1) + (v2 + v3) = 2 levels, then 5 xor-shuffle levels -> 7.
    layernorm_reg_kernel<64> (C <= 256; norm.hip:70-72): 2 + 6 -> 8.
    layernorm_kernel (norm.hip:25-30): per lane ceil(C / 256) serial `s +=` of a 2-level quad, then wave_sum's 6 levels."""
    if C <= 128:
        return 2 + 5
    if C <= 256:
        return 2 + 6
    return 2 + -(-C // 256) + 6


def pm_n(C):
    """patch_merge_ln_kernel (norm.hip:113-120): a row of 4C floats in layernorm_kernel's order."""
    return 2 + -(-4 * C // 256) + 6


def _design_rows(design, M, C, g):
    if design == "unit":
        return torch.randn(M, C, generator=g)
    if design == "offset":
        return OFFSET_MU + OFFSET_SIGMA * torch.randn(M, C, generator=g)
    if design == "decades":
        return torch.randn(M, C, generator=g) * torch.logspace(-2, 2, C)[None, :]
    if design == "epsprobe":   # exactly sigma = 2^-8 per row (to fp32 rounding), mean 0
        z = torch.randn(M, C, generator=g, dtype=F64)
        z = (z - z.mean(1, keepdim=True)) / z.std(1, unbiased=False, keepdim=True)
        return (z * PROBE_SIGMA).float()
    raise ValueError(design)


_R_SCALE = {"unit": 0.5, "offset": 0.4 * OFFSET_SIGMA, "decades": 0.5, "epsprobe": 0.25 * PROBE_SIGMA}


def ln_operands(design, M, C, seed, with_r):
    """(x, r or None, gamma, beta) as fp32: x + r follows the design (x = design row - r, so the residual takes part in the statistics)."""
    g = gen(seed)
    z = _design_rows(design, M, C, g)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    if not with_r:
        return z, None, gamma, beta
    r = torch.randn(M, C, generator=g) * _R_SCALE[design]
    if design == "decades":
        r = r * torch.logspace(-2, 2, C)[None, :]
    return z - r, r, gamma, beta


def ln_ref_bound(x, r, gamma, beta, eps, n):
    """fp64 LayerNorm of x (+ r) and the bound of its fp32 two-pass evaluation with row sums of path length n:
      mean:      |dm| <= EPS (n mean|z| + |mean|)                       (sum, then one division)
      variance:  relative EPS (3 + n + 2): d = z - m and d * d round three times per element, the sum of non-negative terms n times,
                 / C and + eps once each; the sum about the computed mean exceeds the centred one by dm^2 exactly -- second order, but
                 with |mean| / sigma = 800 not small against the rest, so it is carried
      rstd:      half the variance's relative error + rsqrtf
      apply:     d (1 rounding), d * rstd, * gamma (2), + beta (1 of |y|)
      residual:  z = fl(x + r) is off by EPS |z| per element, pushed through _arith.layernorm_bound.
    Returns (ref, B, sigma per row)."""
    z = d64(x) + (d64(r) if r is not None else 0.0)
    gamma, beta = d64(gamma), d64(beta)
    mu = z.mean(-1, keepdim=True)
    var = ((z - mu) ** 2).mean(-1, keepdim=True)
    sig = torch.sqrt(var + eps)
    y = (z - mu) / sig * gamma + beta
    dm = EPS * (n * z.abs().mean(-1, keepdim=True) + mu.abs())
    rel_var = EPS * (3 + n + 2) + dm ** 2 / (var + eps)
    rel = EPS * (1 + 2) + 0.5 * rel_var + RSQRT_ERR
    B = gamma.abs() / sig * dm + (y - beta).abs() * rel + EPS * y.abs()
    if r is not None:
        B = B + A.layernorm_bound(z, EPS * z.abs(), gamma, eps)
    return y, 2 * B, torch.sqrt(var).squeeze(-1)


LN_MUTANTS = ("one_pass_variance", "variance_over_c_minus_1", "eps_1e-5_for_1e-12", "eps_after_sqrt", "r_not_in_statistics")
PM_MUTANTS = ("one_pass_variance", "variance_over_c_minus_1", "eps_after_sqrt", "zero_quadrant_not_counted")


def ln_emulate(x, r, gamma, beta, eps, mutant=None, count=None):
    """The kernel's pass structure in torch fp32: z = x + r, mean, centred variance, rsqrt, apply.  count [M, 1]: the divisor of both
    statistics where it is not the row length (the patch-merge count defect)."""
    x, gamma, beta = x.float(), gamma.float(), beta.float()
    z = x + r.float() if r is not None else x
    C = z.shape[-1]
    n = torch.full((z.shape[0], 1), float(C)) if count is None else count.float()
    s = z if not (mutant == "r_not_in_statistics" and r is not None) else x
    mean = s.sum(-1, keepdim=True) / n
    if mutant == "one_pass_variance":
        var = (s * s).sum(-1, keepdim=True) / n - mean * mean
    else:
        d = s - mean
        var = (d * d).sum(-1, keepdim=True) / (n - 1 if mutant == "variance_over_c_minus_1" else n)
    e = torch.tensor(1e-5 if mutant == "eps_1e-5_for_1e-12" else eps, dtype=F32)
    rstd = 1.0 / (torch.sqrt(var) + e) if mutant == "eps_after_sqrt" else torch.rsqrt(var + e)
    return (z - mean) * rstd * gamma + beta


def pm_rows(x, T, H, W, C):
    """[T*H*W, C] -> ([T*H2*W2, 4C] rows of the four neighbours in the order (dy, dx) = (0,0), (1,0), (0,1), (1,1), zeros outside the
    map (norm.hip:104-110), number of floats of each row that lie inside the map)."""
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    xx = torch.zeros(T, 2 * H2, 2 * W2, C, dtype=x.dtype)
    xx[:, :H, :W] = x.view(T, H, W, C)
    inside = torch.zeros(1, 2 * H2, 2 * W2, 1, dtype=x.dtype)
    inside[:, :H, :W] = 1
    q = lambda t: torch.cat([t[:, 0::2, 0::2], t[:, 1::2, 0::2], t[:, 0::2, 1::2], t[:, 1::2, 1::2]], -1)
    cnt = q(inside).sum(-1).expand(T, H2, W2).reshape(T * H2 * W2, 1) * C
    return q(xx).reshape(T * H2 * W2, 4 * C), cnt


PM_SHAPES = ((2, 18, 25, 96), (1, 9, 13, 192), (1, 5, 7, 384), (1, 4, 4, 32), (1, 1, 1, 32))


def pm_operands(design, T, H, W, C, seed):
    g = gen(seed)
    x = _design_rows(design, T * H * W, C, g)
    return x, torch.randn(4 * C, generator=g), torch.randn(4 * C, generator=g)


def pm_emulate(x, gamma, beta, T, H, W, C, eps, mutant=None):
    rows, cnt = pm_rows(x.float(), T, H, W, C)
    if mutant == "zero_quadrant_not_counted":
        return ln_emulate(rows, None, gamma, beta, eps, count=cnt)
    return ln_emulate(rows, None, gamma, beta, eps, mutant)


# =====================================================================================================================
# GroupNorm on channels-last maps (tce_groupnorm_f32, tce_groupnorm_up_add_f32)
# =====================================================================================================================
GN_DESIGNS = ("unit", "offset", "distinct")
GN_ROWS_G = (8, 16, 32, 64)
GN_ROWS_HW = (7, 8, 9, 511, 512, 513, 3000, 4095, 4096, 4097)
GN_GENERIC = ((64, 8), (128, 32), (256, 4), (256, 1))
GN_GENERIC_HW = (63, 513, 3000)
GN_UP_SIZES = ((2, 6, 7, 13, 15), (1, 3, 3, 3, 3), (3, 12, 20, 23, 40), (1, 9, 16, 18, 32), (1, 13, 15, 6, 7))


def gn_rows_per(HW):
    return 128 if HW >= 4096 else (32 if HW >= 512 else 8)    # norm.hip:628


def gn_nsplit(HW):
    return -(-HW // gn_rows_per(HW))


def gn_is_rows_kernel(C, G):
    return C == 256 and G in (8, 16, 32, 64)                  # norm.hip:653


def gn_chunk_rows(HW, C, G):
    """Rows of a statistics chunk: the rows kernel takes groupnorm_rows_per (norm.hip:380), the generic kernel re-derives
    ceil(HW / nsplit) (norm.hip:338), which can be smaller (trailing chunks may then be empty)."""
    return gn_rows_per(HW) if gn_is_rows_kernel(C, G) else -(-HW // gn_nsplit(HW))


def gn_n_stats(HW, C, G):
    """Additions on the longest path of a chunk sum.
    groupnorm_stats_rows_kernel<R> (norm.hip:390-398): R = rows_per / 4 serial `s +=` of a 2-level quad, log2(64 / G) shuffle levels,
    2 levels over the four waves.
    groupnorm_stats_kernel (norm.hip:344-351): ceil(rows * C / G / 256) serial additions per thread, wave_sum's 6, 2 over the waves."""
    if gn_is_rows_kernel(C, G):
        return 2 + gn_rows_per(HW) // 4 + int(math.log2(64 // G)) + 2
    return -(-gn_chunk_rows(HW, C, G) * (C // G) // 256) + 6 + 2


def gn_levels(HW):
    """Chan merges on the longest path of groupnorm_scale_shift (norm.hip:446-463): a lane of 16 merges ceil(nsplit / 16) partials
    serially, then 4 butterfly steps; never fewer than the ceil(log2 nsplit) + 4 of a balanced tree."""
    ns = gn_nsplit(HW)
    return max(-(-ns // 16), math.ceil(math.log2(ns)) if ns > 1 else 0) + 4


def gn_operands(design, T, HW, C, G, seed):
    """x [T, HW, C], gamma, beta.  offset: mu / sigma = 800 per (frame, group), the pair scaled by 2^((t + g) % 3 - 1).
    distinct: frame t, group g gets scale 2^((t + g) % 5 - 2) and offset 3 ((2 t + g) % 7 - 3)."""
    g = gen(seed)
    cg = C // G
    x = torch.randn(T, HW, G, cg, generator=g)
    t, gg = torch.arange(T).view(T, 1, 1, 1), torch.arange(G).view(1, 1, G, 1)
    if design == "offset":
        k = 2.0 ** ((t + gg) % 3 - 1).float()
        x = k * (OFFSET_MU + OFFSET_SIGMA * x)
    elif design == "distinct":
        x = x * 2.0 ** ((t + gg) % 5 - 2).float() + 3.0 * ((2 * t + gg) % 7 - 3).float()
    elif design != "unit":
        raise ValueError(design)
    return x.reshape(T, HW, C).contiguous(), torch.randn(C, generator=g), torch.randn(C, generator=g)


def _chunk_stats(x, T, HW, C, G, rows):
    """Per chunk of `rows` rows: (count, sum, sum|x|) as [T, nchunk, G] in x's dtype."""
    cg = C // G
    nch = -(-HW // rows)
    pad = nch * rows - HW
    xx = x.view(T, HW, G, cg)
    s, a = xx.sum(3), xx.abs().sum(3)
    if pad:
        z = torch.zeros(T, pad, G, dtype=x.dtype)
        s, a = torch.cat([s, z], 1), torch.cat([a, z], 1)
    cnt = torch.full((nch,), float(rows * cg), dtype=x.dtype)
    cnt[-1] = (HW - (nch - 1) * rows) * cg
    return cnt.view(1, nch, 1).expand(T, nch, G), s.view(T, nch, rows, G).sum(2), a.view(T, nch, rows, G).sum(2)


def gn_ref_bound(x, gamma, beta, T, HW, C, G, eps):
    """fp64 GroupNorm (before the ReLU, which is 1-Lipschitz) and the bound of the kernel's evaluation:
      chunk mean  |dm_k| <= EPS (n mean_k|x| + |mean_k|), n = gn_n_stats
      merged mean + L levels of  mean += d * f:  EPS (|mean| + 3 |d f|) each, |d| <= 2 D, D = max_k |mean_k - mean|, |mean| <= Mx = max_k |mean_k|
      M2          every term is non-negative, so errors stay relative: EPS (3 + n) in a chunk (d, d * d, the sum), 8 per merge level
                  (d, d * d twice, f, n * f, the product, two additions), / n and + eps; the chunk means' errors enter the between-chunk
                  term as 2 D * 2 dm per element, and the sums about computed means carry dm^2
      apply       out = v * scale + shift, scale = rstd * gamma, shift = beta - mean * scale: the error of scale is common to both terms
                  -> |(v - mean) scale| (rel(rstd) + EPS);  |scale| dm;  EPS (|v scale| + 2 |mean scale| + |beta| + |out|) for the
                  products, the subtraction and the final addition."""
    cg = C // G
    n, L = gn_n_stats(HW, C, G), gn_levels(HW)
    xd = d64(x)
    xx = xd.view(T, HW, G, cg)
    mean = xx.mean((1, 3))                                           # [T, G]
    var = ((xx - mean.view(T, 1, G, 1)) ** 2).mean((1, 3))
    cnt, s, a = _chunk_stats(xd, T, HW, C, G, gn_chunk_rows(HW, C, G))
    mk, ak = s / cnt, a / cnt
    Mx = mk.abs().amax(1)
    D = (mk - mean.view(T, 1, G)).abs().amax(1)
    dm_k = EPS * (n * ak + mk.abs()).amax(1)
    dm = dm_k + L * EPS * (Mx + 6 * D)
    rel_var = EPS * (3 + n + 8 * L + 2) + (4 * D * dm_k + dm_k ** 2) / (var + eps)
    rel = 0.5 * rel_var + RSQRT_ERR + EPS
    ch = lambda v: v.repeat_interleave(cg, 1).view(T, 1, C)          # per (frame, group) -> per channel
    gamma, beta = d64(gamma).view(1, 1, C), d64(beta).view(1, 1, C)
    sc = gamma / torch.sqrt(ch(var) + eps)
    y = (xd - ch(mean)) * sc + beta
    B = (y - beta).abs() * ch(rel) + sc.abs() * ch(dm) + EPS * ((xd * sc).abs() + 2 * (ch(mean) * sc).abs() + beta.abs() + y.abs())
    return y, 2 * B, torch.sqrt(var)


GN_MUTANTS = ("one_pass_variance", "last_chunk_count_full", "chan_without_nb_over_nt", "partials_of_previous_frame", "group_index_c_over_c8")


def gn_emulate(x, gamma, beta, T, HW, C, G, eps, relu=False, mutant=None):
    """Partials (count, mean, M2 about that mean) per chunk, a serial Chan merge, scale / shift, apply -- torch fp32."""
    x, gamma, beta = x.float(), gamma.float(), beta.float()
    cg = C // G
    rows = gn_chunk_rows(HW, C, G)
    cnt, s, _ = _chunk_stats(x, T, HW, C, G, rows)
    nch = cnt.shape[1]
    if mutant == "last_chunk_count_full":
        cnt = torch.full_like(cnt, float(rows * cg))
    mk = s / cnt
    pad = nch * rows - HW
    xx = x.view(T, HW, G, cg)
    if mutant == "one_pass_variance":
        q = (xx * xx).sum(3)
    else:
        q = ((xx - mk.repeat_interleave(rows, 1)[:, :HW].unsqueeze(-1)) ** 2).sum(3)
    if pad:
        q = torch.cat([q, torch.zeros(T, pad, G)], 1)
    m2k = q.view(T, nch, rows, G).sum(2)
    if mutant == "one_pass_variance":
        m2k = m2k - cnt * mk * mk
    n, mean, m2 = cnt[:, 0].clone(), mk[:, 0].clone(), m2k[:, 0].clone()
    for k in range(1, nch):
        nb, mb, qb = cnt[:, k], mk[:, k], m2k[:, k]
        nt = n + nb
        d, f = mb - mean, nb / nt
        mean = mean + d * f
        m2 = m2 + (qb + d * d * (n if mutant == "chan_without_nb_over_nt" else n * f))
        n = nt
    rstd = torch.rsqrt(m2 / n + torch.tensor(eps, dtype=F32))
    if mutant == "partials_of_previous_frame":
        mean, rstd = mean.roll(1, 0), rstd.roll(1, 0)
    gi = torch.arange(C) // cg
    if mutant == "group_index_c_over_c8":
        gi = torch.arange(C) // (C // 8)
    sc = rstd[:, gi] * gamma[None]
    sh = beta[None] - mean[:, gi] * sc
    y = x * sc.view(T, 1, C) + sh.view(T, 1, C)
    return torch.relu(y) if relu else y


def gn_up_ref_bound(x, gamma, beta, add, T, h, w, ho, wo, C, G, eps, relu=True):
    """add + act(GN(x)) gathered by the fp32 nearest rule (groupnorm_apply_up_kernel, norm.hip:539-552): the GroupNorm bound of the
    gathered element plus one rounding of the addition."""
    y, B, sig = gn_ref_bound(x, gamma, beta, T, h * w, C, G, eps)
    y = (y.clamp_min(0) if relu else y).reshape(T * h * w, C)
    out = nearest_ref(y, T, h, w, ho, wo, C) + d64(add)
    return out, nearest_ref(B.reshape(T * h * w, C), T, h, w, ho, wo, C) + 2 * EPS * out.abs(), sig


def gn_up_emulate(x, gamma, beta, add, T, h, w, ho, wo, C, G, eps, relu=True, mutant=None):
    y = gn_emulate(x, gamma, beta, T, h * w, C, G, eps, relu).reshape(T * h * w, C)
    return nearest_ref(y, T, h, w, ho, wo, C, mutant) + add.float()


# =====================================================================================================================
# Resampling (tce_resize_nearest_f32, tce_resize_bilinear_f32, tce_resize_bilinear_ln_f32, the up-sampling GroupNorm apply)
# =====================================================================================================================
RESIZE_SIZES = ((1, 1, 1, 3, 2), (3, 5, 7, 11, 13), (2, 12, 20, 23, 40), (1, 12, 20, 45, 80), (1, 45, 80, 12, 20), (1, 7, 9, 7, 9),
                (1, 6, 10, 12, 20))
RESIZE_C = (4, 64, 256)
NEAREST_MUTANTS = ("round_not_floor", "inverted_scale")
BILINEAR_MUTANTS = ("align_corners", "no_half_pixel", "no_clamp_at_0")


def nearest_index(n, no, mutant=None):
    """PyTorch's fp32 rule min(floorf(o * (float) n / (float) no), n - 1) in numpy float32 (misc.hip:45-47, norm.hip:539-544)."""
    o = np.arange(no, dtype=np.float32)
    s = np.float32(n) / np.float32(no)
    if mutant == "inverted_scale":
        s = np.float32(no) / np.float32(n)
    f = (o * s).astype(np.float32)
    i = np.floor(f + np.float32(0.5)) if mutant == "round_not_floor" else np.floor(f)
    return torch.from_numpy(np.minimum(i, n - 1).astype(np.int64))


def nearest_ref(x, T, h, w, ho, wo, C, mutant=None):
    """Exact: a gather.  x [T*h*w, C] -> [T*ho*wo, C] in x's dtype."""
    yi, xi = nearest_index(h, ho, mutant), nearest_index(w, wo, mutant)
    return x.view(T, h, w, C)[:, yi][:, :, xi].reshape(T * ho * wo, C)


def _coords(n, no):
    """fp64 source coordinate max(s (o + 0.5) - 0.5, 0), s = n / no, and what the fp32 one may be off by: 3 EPS (f + 1) (s, the
    product and the subtraction round once each, on values below f + 1)."""
    o = torch.arange(no, dtype=F64)
    f = (n / no * (o + 0.5) - 0.5).clamp_min(0.0)
    return f, 3 * EPS * (f + 1)


def _axis_lin(V, f, delta, dim):
    """Linear interpolation of V along dim at coordinates f (misc.hip:62-65: i0 = min((int) f, n - 1), i1 = i0 + (i0 < n - 1), weight
    f - i0) -> (value, slope): slope = |V[i1] - V[i0]|, and where f is within delta of a cell border also the neighbouring cell's,
    since the fp32 coordinate may fall there (the weights are continuous across the border)."""
    n = V.shape[dim]
    i0 = f.floor().clamp(max=n - 1).long()
    i1 = (i0 + 1).clamp(max=n - 1)
    l = f - i0.double()
    shp = [1] * V.dim()
    shp[dim] = -1
    lv, dv = l.view(shp), delta.view(shp)
    sel = lambda i: V.index_select(dim, i)
    v0, v1 = sel(i0), sel(i1)
    slope = (v1 - v0).abs()
    lower = (v0 - sel((i0 - 1).clamp(min=0))).abs()
    upper = (sel((i1 + 1).clamp(max=n - 1)) - v1).abs()
    slope = torch.maximum(slope, torch.where(lv <= dv, lower, torch.zeros_like(lower)))
    slope = torch.maximum(slope, torch.where(lv >= 1 - dv, upper, torch.zeros_like(upper)))
    return (1 - lv) * v0 + lv * v1, slope, i0, i1


def bilinear_ref_bound(x, T, h, w, ho, wo, C, add=None):
    """fp64 F.interpolate(bilinear, align_corners=False) of x [T*h*w, C] (+ add) and its bound
    d_fy |bot - top| + d_fx max(|v01 - v00|, |v11 - v10|) + 3 EPS sum w_i |v_i|  (hx = 1 - lx, hx * v and the fma round once each on
    every path through misc.hip:72-73), + EPS |out| for the addition."""
    V = d64(x).view(T, h, w, C)
    fy, dy = _coords(h, ho)
    fx, dx = _coords(w, wo)
    Vx, Sx, _, _ = _axis_lin(V, fx, dx, 2)                 # [T, h, wo, C]
    val, Sy, y0, y1 = _axis_lin(Vx, fy, dy, 1)             # [T, ho, wo, C]
    Sxm = torch.maximum(Sx.index_select(1, y0), Sx.index_select(1, y1))
    Ax = _axis_lin(V.abs(), fx, dx, 2)[0]
    Wabs = _axis_lin(Ax, fy, dy, 1)[0]
    B = dy.view(1, ho, 1, 1) * Sy + dx.view(1, 1, wo, 1) * Sxm + 3 * EPS * Wabs
    val, B = val.reshape(T * ho * wo, C), B.reshape(T * ho * wo, C)
    if add is not None:
        val = val + d64(add)
        B = B + EPS * val.abs()
    return val, 2 * B


def bilinear_emulate(x, T, h, w, ho, wo, C, add=None, mutant=None):
    """misc.hip:59-74 in torch fp32."""
    V = x.float().view(T, h, w, C)

    def axis(n, no):
        o = torch.arange(no, dtype=F32)
        nf, nof = torch.tensor(float(n), dtype=F32), torch.tensor(float(no), dtype=F32)
        if mutant == "align_corners":
            f = o * ((nf - 1) / (nof - 1)) if no > 1 else torch.zeros(no)
        elif mutant == "no_half_pixel":
            f = o * (nf / nof)
        else:
            f = (nf / nof) * (o + 0.5) - 0.5
            if mutant != "no_clamp_at_0":
                f = f.clamp_min(0.0)
        i0 = f.trunc().clamp(max=n - 1).long()               # (int) truncates toward zero
        i1 = (i0 + 1).clamp(max=n - 1)
        l = f - i0.float()
        return i0, i1, l, 1.0 - l

    y0, y1, ly, hy = axis(h, ho)
    x0, x1, lx, hx = axis(w, wo)
    lx, hx, ly, hy = lx.view(1, 1, wo, 1), hx.view(1, 1, wo, 1), ly.view(1, ho, 1, 1), hy.view(1, ho, 1, 1)
    top = lx * V[:, y0][:, :, x1] + hx * V[:, y0][:, :, x0]
    bot = lx * V[:, y1][:, :, x1] + hx * V[:, y1][:, :, x0]
    o = (ly * bot + hy * top).reshape(T * ho * wo, C)
    return o + add.float() if add is not None else o


def resize_operands(T, h, w, ho, wo, C, seed, design="unit"):
    """(x [T*h*w, C], add [T*ho*wo, C], gamma, beta).  offset: add = 40 + 0.05 randn per row and x at 0.05, so the LayerNorm row of
    add + bilinear(x) keeps mu / sigma near 800."""
    g = gen(seed)
    x, add = torch.randn(T * h * w, C, generator=g), torch.randn(T * ho * wo, C, generator=g)
    if design == "offset":
        x, add = OFFSET_SIGMA * x, OFFSET_MU + OFFSET_SIGMA * add
    return x, add, torch.randn(C, generator=g), torch.randn(C, generator=g)


def bilinear_ln_ref_bound(x, T, h, w, ho, wo, C, add, gamma, beta, eps):
    """LayerNorm(add + bilinear(x)) (resize_bilinear_ln_kernel, misc.hip:110-127: layernorm_reg_kernel<64>'s order, n = 8): the row is
    off by B_bilinear + one rounding of the addition (bilinear_ref_bound carries both), pushed through _arith.layernorm_bound, plus the
    fp32 evaluation of the norm itself."""
    z, Bz = bilinear_ref_bound(x, T, h, w, ho, wo, C, add)
    y, By, sig = ln_ref_bound(z, None, gamma, beta, eps, 8)
    return y, 2 * A.layernorm_bound(z, Bz / 2, gamma, eps) + By, sig


# =====================================================================================================================
# Sine position maps (tce_pos_sine2d_valid_f32)
# =====================================================================================================================
POS_F = (64, 128)
POS_SIZES = ((2, 9, 13), (1, 45, 80))
POS_PADDED = ((12, 20, 12, 17), (9, 13, 7, 10), (6, 10, 6, 10))
# rounding steps on the way to the argument v (misc.hip:25-29): yl + 1e-6f, the division, * two_pi and the rounding of the constant
# itself, powf (its exponent 2 (i / 2) / F is exact for F a power of two), e / dim_t
POS_K = 1 + 1 + 2 + POW_ERR / EPS + 1
POS_MUTANTS = ("sin_cos_swapped", "y_plus_1_dropped", "no_1e-6", "padded_columns_not_zeroed")


def _pos_args(T, h, w, F, hv, wv, dtype, mutant=None):
    """The argument v [T, h, w, 2F] of the sine / cosine and the mask of cosine channels, in `dtype` arithmetic."""
    t = lambda v: torch.tensor(v, dtype=dtype)
    y, x = torch.arange(h).view(h, 1), torch.arange(w).view(1, w)
    shift = 0 if mutant == "y_plus_1_dropped" else 1
    col_ok = (x < wv) | (mutant == "padded_columns_not_zeroed")
    ye = torch.where(col_ok, (y + shift).clamp(max=hv), torch.zeros_like(y)).to(dtype).expand(h, w)
    yl = torch.where(col_ok, torch.tensor(hv), torch.tensor(0)).to(dtype).expand(h, w)
    xe = torch.where(y < hv, (x + 1).clamp(max=wv), torch.zeros_like(x)).to(dtype).expand(h, w)
    xl = torch.where(y < hv, torch.tensor(wv), torch.tensor(0)).to(dtype).expand(h, w)
    e6 = t(0.0 if mutant == "no_1e-6" else 1e-6)
    two_pi = t(6.283185307179586)
    emb = torch.stack([(ye - 0.5) / (yl + e6) * two_pi, (xe - 0.5) / (xl + e6) * two_pi], 2)     # [h, w, 2]
    i = torch.arange(F)
    dim_t = torch.pow(t(10000.0), (2 * (i // 2)).to(dtype) / t(float(F)))
    v = (emb.unsqueeze(-1) / dim_t).reshape(1, h, w, 2 * F).expand(T, h, w, 2 * F)
    cosine = ((i % 2) == 1).repeat(2)
    if mutant == "sin_cos_swapped":
        cosine = ~cosine
    return v, cosine


def pos_ref_bound(T, h, w, F, hv=None, wv=None, add=None):
    """fp64 map [T*h*w, 2F] and its bound POS_K EPS |v| + 2 EPS (the argument's roundings reach the value through |d sin| <= |dv|;
    sinf / cosf themselves) + EPS |out| for an added level embedding."""
    hv, wv = (h, w) if hv is None else (hv, wv)
    v, cosine = _pos_args(T, h, w, F, hv, wv, F64)
    out = torch.where(cosine, v.cos(), v.sin()).reshape(T * h * w, 2 * F)
    B = POS_K * EPS * v.abs().reshape(T * h * w, 2 * F) + SIN_ERR
    if add is not None:
        out = out + d64(add)
        B = B + EPS * out.abs()
    return out, B


def pos_emulate(T, h, w, F, hv=None, wv=None, add=None, mutant=None):
    hv, wv = (h, w) if hv is None else (hv, wv)
    v, cosine = _pos_args(T, h, w, F, hv, wv, F32, mutant)
    out = torch.where(cosine, v.cos(), v.sin()).reshape(T * h * w, 2 * F)
    return out + add.float() if add is not None else out


# =====================================================================================================================
# Dynamic mask head: mask_pack -> gemm_batched -> mask_tail
# =====================================================================================================================
MASK_SHAPES = ((3, 2, 5, 18, 25), (3, 2, 30, 9, 15), (1, 1, 1, 5, 131), (2, 1, 9, 1, 1))
MASK_CM = (16, 64)
MASK_STRIDES = (4,)        # every stride_px the pipeline passes (pipeline.py: its one mask_tail call; ops.mask_tail's default)
MASK_PARAM_SCALES = (0.2, 0.2 * 2.0 ** -4)
MASK_MUTANTS = ("px_without_half_stride", "relx_rely_swapped", "img_h_img_w_swapped", "w1_transposed", "no_relu_after_layer_1")
DC = 8


def mask_npar(Cm):
    return DC * (Cm + 2) + DC * DC + DC + DC + DC + 1


def mask_operands(nl, T, Q, h, w, Cm, scale, seed):
    """(feats [T, Cm, h, w], params [nl, T*Q, npar], refs [nl, T*Q, 4] with 0.0 and 1.0 among them, img (H, W) = (4h - 2, 4w - 1))."""
    g = gen(seed)
    feats = torch.randn(T, Cm, h, w, generator=g)
    params = torch.randn(nl, T * Q, mask_npar(Cm), generator=g) * scale
    refs = torch.rand(nl, T * Q, 4, generator=g)
    refs[0, 0, 0], refs[0, 0, 1] = 0.0, 1.0
    refs[-1, -1, 0], refs[-1, -1, 1] = 1.0, 0.0
    return feats, params, refs, (4 * h - 2, 4 * w - 1)


def _mask_split(params, Cm):
    """[..., npar] -> w0 [..., 8, Cm + 2], w1 [..., 8, 8], w2 [..., 8], b0 [..., 8], b1 [..., 8], b2 [...] (parse_dynamic_params: [w0 | w1 |
    w2 | b0 | b1 | b2], each weight [out][in])."""
    o1 = DC * (Cm + 2)
    o2, o3 = o1 + DC * DC, o1 + DC * DC + DC
    lead = params.shape[:-1]
    return (params[..., :o1].reshape(*lead, DC, Cm + 2), params[..., o1:o2].reshape(*lead, DC, DC), params[..., o2:o3],
            params[..., o3:o3 + DC], params[..., o3 + DC:o3 + 2 * DC], params[..., o3 + 2 * DC])


def _mask_geometry(refs, h, w, img, stride, dtype, mutant=None):
    """relx, rely [nl, T*Q, h, w] and ref * size [nl, T*Q, 1, 1] in `dtype` arithmetic (misc.hip:259, 271-272)."""
    img_h, img_w = (img[1], img[0]) if mutant == "img_h_img_w_swapped" else img
    half = 0 if mutant == "px_without_half_stride" else stride // 2
    px = (torch.arange(w) * stride + half).to(dtype).view(1, 1, 1, w)
    py = (torch.arange(h) * stride + half).to(dtype).view(1, 1, h, 1)
    rx = (refs[..., 0].to(dtype) * torch.tensor(float(img_w), dtype=dtype))[..., None, None]
    ry = (refs[..., 1].to(dtype) * torch.tensor(float(img_h), dtype=dtype))[..., None, None]
    relx, rely = (rx - px).expand(*refs.shape[:2], h, w), (ry - py).expand(*refs.shape[:2], h, w)
    if mutant == "relx_rely_swapped":
        relx, rely = rely, relx
    return relx, rely, rx, ry


def mask_ref(feats, params, refs, img, stride, Cm):
    """oracle.tce_oracle.dynamic_mask_head evaluated on fp64 tensors, per level -> [nl, T*Q, h, w]."""
    from oracle import tce_oracle as O
    cfg = O.OracleConfig(mask_dim=Cm)
    return torch.stack([O.dynamic_mask_head(cfg, d64(feats), d64(params[l]), d64(refs[l, :, :2]), img, stride) for l in range(params.shape[0])])


def mask_ref_bound(feats, params, refs, img, stride, Cm):
    """The head restated in fp64 with every intermediate kept (equal to mask_ref: tests/test_pointwise_bound_cpu.py) and its bound:
      G        the split-fp16 product of gemm_batched: _arith.bound_split with c = c_dense(Cm)
      layer 1  relx = fl(fl(ref * img_w) - px) is off by EPS (|ref img_w| + |relx|); s_c * relx and s_{8+c} * rely round once each;
               three additions of at most |G| + |s_c relx| + |s_{8+c} rely| + |b0| (misc.hip:277)
      layer 2  eight fmaf on b1 (misc.hip:282-284): n = 9 against |w1| |h0| + |b1|, plus the chained layer-1 bound
      layer 3  eight fmaf on b2 (misc.hip:279-285): n = 9 against |w2| relu(a) + |b2|, plus the chained layer-2 bound."""
    nl, TQ = params.shape[:2]
    T, _, h, w = feats.shape
    Q = TQ // T
    w0, w1, w2, b0, b1, b2 = (d64(v) for v in _mask_split(params, Cm))
    relx, rely, rx, ry = _mask_geometry(d64(refs), h, w, img, stride, F64)
    f = d64(feats).permute(0, 2, 3, 1).reshape(T, h * w, Cm)
    ref = torch.empty(nl, TQ, h * w, dtype=F64)
    B = torch.empty_like(ref)
    for lvl in range(nl):
        for t in range(T):
            it = slice(t * Q, (t + 1) * Q)
            wf = w0[lvl, it, :, :Cm].reshape(Q * DC, Cm)
            G = (f[t] @ wf.T).view(h * w, Q, DC).permute(1, 2, 0)                     # [Q, 8, hw]
            BG = A.bound_split(f[t], wf, A.c_dense(Cm)).view(h * w, Q, DC).permute(1, 2, 0)
            sx, sy = w0[lvl, it, :, Cm, None], w0[lvl, it, :, Cm + 1, None]           # [Q, 8, 1]
            X, Y = relx[lvl, it].reshape(Q, 1, h * w), rely[lvl, it].reshape(Q, 1, h * w)
            dX = EPS * (rx[lvl, it].abs().reshape(Q, 1, 1) + X.abs())
            dY = EPS * (ry[lvl, it].abs().reshape(Q, 1, 1) + Y.abs())
            bb0 = b0[lvl, it, :, None]
            pre = G + sx * X + sy * Y + bb0
            B1 = BG + sx.abs() * dX + sy.abs() * dY + EPS * ((sx * X).abs() + (sy * Y).abs()) \
                + 3 * EPS * (G.abs() + (sx * X).abs() + (sy * Y).abs() + bb0.abs())
            h0 = pre.clamp_min(0)
            W1, bb1 = w1[lvl, it], b1[lvl, it, :, None]
            a = W1 @ h0 + bb1
            B2 = W1.abs() @ B1 + 9 * EPS * (W1.abs() @ h0 + bb1.abs())
            a1 = a.clamp_min(0)
            W2 = w2[lvl, it].unsqueeze(1)                                             # [Q, 1, 8]
            bb2 = b2[lvl, it].view(Q, 1, 1)
            ref[lvl, it] = (W2 @ a1 + bb2).squeeze(1)
            B[lvl, it] = (W2.abs() @ B2 + 9 * EPS * (W2.abs() @ a1 + bb2.abs())).squeeze(1)
    return ref.view(nl, TQ, h, w), 2 * B.view(nl, TQ, h, w)


def mask_emulate(feats, params, refs, img, stride, Cm, mutant=None):
    """The three launches in torch fp32, the first layer's product through _arith.emulate_split."""
    nl, TQ = params.shape[:2]
    T, _, h, w = feats.shape
    Q = TQ // T
    w0, w1, w2, b0, b1, b2 = (v.float() for v in _mask_split(params, Cm))
    if mutant == "w1_transposed":
        w1 = w1.transpose(-1, -2)
    relx, rely, _, _ = _mask_geometry(refs.float(), h, w, img, stride, F32, mutant)
    f = feats.float().permute(0, 2, 3, 1).reshape(T, h * w, Cm)
    out = torch.empty(nl, TQ, h * w)
    for lvl in range(nl):
        for t in range(T):
            it = slice(t * Q, (t + 1) * Q)
            G = A.emulate_split(f[t], w0[lvl, it, :, :Cm].reshape(Q * DC, Cm)).view(h * w, Q, DC).permute(1, 2, 0)
            X, Y = relx[lvl, it].reshape(Q, 1, h * w), rely[lvl, it].reshape(Q, 1, h * w)
            pre = G + w0[lvl, it, :, Cm, None] * X + w0[lvl, it, :, Cm + 1, None] * Y + b0[lvl, it, :, None]
            h0 = pre if mutant == "no_relu_after_layer_1" else pre.clamp_min(0)
            a = (w1[lvl, it] @ h0 + b1[lvl, it, :, None]).clamp_min(0)
            out[lvl, it] = (w2[lvl, it].unsqueeze(1) @ a).squeeze(1) + b2[lvl, it].view(Q, 1)
    return out.view(nl, TQ, h, w)


# =====================================================================================================================
# Contrastive cosine (tce_contrastive_f32)
# =====================================================================================================================
CONTRASTIVE_CASES = ((3, 168, 256, 3), (8, 1000, 256, 2), (1, 7, 256, 1), (4, 50, 96, 2), (2, 33, 64, 1))
CONTRASTIVE_MUTANTS = ("norms_clamped_once", "mean_over_32_chunks")
COS_EPS = 1e-6


def contrastive_operands(T, S, C, fpc, seed):
    """memory [T, S, C] (randn + 0.3), sentence features [T / fpc, C]; the last clip's sentence scaled by 1e-9: its norm is far below
    the 1e-6 clamp, which then decides.  With more than one frame, frame 0's memory is scaled by 1e-8 as well: the cosine is free of the
    scale of the mean unless the MEAN's norm is the clamped one, so only there a wrong divisor of the mean shows."""
    g = gen(seed)
    mem = torch.randn(T, S, C, generator=g) + 0.3
    sent = torch.randn(T // fpc, C, generator=g)
    if T // fpc > 1:
        sent[-1] *= 1e-9
    if T > 1:
        mem[0] *= 1e-8
    return mem, sent


def contrastive_n_mean(S):
    """Additions on the longest path of a column sum (misc.hip:471-484, 493): ceil(S / 32) rows of a chunk as a serial chain over every
    fourth row plus up to 3 tail rows, 2 levels over the four accumulators, then the 32 chunk sums serially."""
    rows = -(-S // 32)
    return rows // 4 + 3 + 2 + 32


CONTRASTIVE_N_DOT = 1 + 6 + 2      # the product, wave_sum's 6 levels, 2 levels over the four waves (misc.hip:497-507)


def contrastive_ref_bound(mem, sent, fpc):
    mem, s = d64(mem), d64(sent).repeat_interleave(fpc, 0)
    S = mem.shape[1]
    m = mem.mean(1)
    dmc = EPS * (contrastive_n_mean(S) * mem.abs().mean(1) + m.abs())                # per column: the sum, then / S
    dot, mm, ss = (m * s).sum(1), (m * m).sum(1), (s * s).sum(1)
    n = CONTRASTIVE_N_DOT
    d_dot = (s.abs() * dmc).sum(1) + n * EPS * (m * s).abs().sum(1)
    d_mm = 2 * (m.abs() * dmc).sum(1) + n * EPS * mm
    d_ss = n * EPS * ss
    n1, n2 = mm.sqrt(), ss.sqrt()

    def clamped(nv, d_sq, sq):
        dn = nv * (0.5 * d_sq / sq.clamp_min(1e-300) + RSQRT_ERR)
        return nv.clamp_min(COS_EPS), torch.where(nv + 2 * dn < COS_EPS, torch.zeros_like(dn), dn)   # the clamp absorbs it

    N1, dN1 = clamped(n1, d_mm, mm)
    N2, dN2 = clamped(n2, d_ss, ss)
    ref = dot / (N1 * N2)
    B = d_dot / (N1 * N2) + ref.abs() * (dN1 / N1 + dN2 / N2 + 2 * EPS)
    return ref, 2 * B


def contrastive_emulate(mem, sent, fpc, mutant=None):
    """32 chunk sums per column, their sum / S, three dot products, each norm clamped -- torch fp32."""
    mem, s = mem.float(), sent.float().repeat_interleave(fpc, 0)
    T, S, C = mem.shape
    parts = [mem[:, p * S // 32:(p + 1) * S // 32].sum(1) for p in range(32)]
    m = torch.stack(parts, 0).sum(0) / (32.0 if mutant == "mean_over_32_chunks" else float(S))
    dot, n1, n2 = (m * s).sum(1), (m * m).sum(1).sqrt(), (s * s).sum(1).sqrt()
    e = torch.tensor(COS_EPS, dtype=F32)
    if mutant == "norms_clamped_once":
        return dot / torch.maximum(n1 * n2, e)
    return dot / (torch.maximum(n1, e) * torch.maximum(n2, e))
