"""Multi-scale deformable attention: an fp64 reference, a derived per-element bound, structural inputs and deliberate defects.

Pure torch on the CPU; imports the oracle and tests/_arith.py only.  A *case* is a dict of the fp32 tensors a kernel receives
(kind "plain": value, loc, weights; kind "fused": value, proj = offsets | logits, ref, valid_hw, ref_dim, ref_per_frame; kind "raw":
a fused case whose value is value_proj(src)) and `ref_and_bound(case)` returns the fp64 result from exactly those fp32 numbers and the
bound B below.

Bound B (per element, first order, times 2 for the remainder as everywhere in _arith.py; eps = 2^-24)
-----------------------------------------------------------------------------------------------------
out[d] = sum_k a_k * sample_k[d],  sample_k = sum_c cw_c v_c[d]  (4 corners, cw_c >= 0, sum_c cw_c <= 1, a dropped corner = a zero row).

Position.  The sample is the bilinear interpolation of the level's map extended by zeros (outside the level and on padding), which is
continuous in (w_im, h_im): every corner's coefficient goes to 0 where that corner is dropped, and at w_im = -1 / W the whole sample
is 0.  Its slope along either axis is at most the largest difference of two neighbouring rows of the extended map, <= G_l = 2 max|v|
over the level (per frame, head, channel).  So evaluating at a position that is off by (dw, dh) moves sample_k by <= (dw + dh) G_l
WHATEVER side of a border either position is on -- which is why the lattice below can sit exactly on the borders.
  dw, plain op: w_im = x * W - 0.5 is two roundings (or one, fused): eps (|x W| + |w_im|).
  dw, fused forms, ref_dim 2: px = rp * vr + ox / W rounds the product, the quotient (one rounding: the build has no fast-math flag)
  and the sum: eps (|rp vr| + |ox / W| + |px|), carried through * W, plus the two of w_im:
      dw = eps (W (|rp vr| + |ox / W| + |px|) + |px W| + |w_im|).
  ref_dim 4: px = rp0 * vr + ((ox / P) * (rp2 * vr)) * 0.5: the second term T carries three roundings (* 0.5 is exact):
      dw = eps (W (|rp0 vr| + 3 |T| + |px|) + |px W| + |w_im|).
  vr is the fp32 quotient float(wv) / float(W) on both sides (an input, no error).  dh likewise with H, y.

Weights (fused forms).  The logits s_k are inputs.  Score model of tests/test_arith_bound_gpu.py::attention_ref_and_bound, validated
there on these kernels' __expf: delta_k = eps (3 |s_k| + 2 |s_k - max s|), and 4 eps of p for exp and the normalisation.  First
order of the softmax: dp_k = p_k (delta_k' - sum_j p_j delta_j') with |delta'| <= delta, so |dp_k| <= p_k (delta_k + sum_j p_j delta_j);
this is A.softmax_v_bound's propagation per point instead of with the row's largest delta (with one logit 200 above the others the
row maximum of delta would put 1e-4 on a point whose own delta is 0).  Products are exact fp32 (no fp16 split anywhere in MSDA).
A weight that underflows in fp32 (exp(-200)) is below 2^-126: absolute term 2^-120 sum_k |sample_k|.

Accumulation.  1 - lh, the coefficient products, the four-term corner sum, the product with a_k and the L*P additions:
(L*P + 6) eps sum_k a_k sum_c cw_c |v_c|.

    B = 2 [ sum_k a_k (dw_k + dh_k) G_l(k)  +  sum_k a_k ((L*P + 6) eps + delta_k + sum_j p_j delta_j + 4 eps + 2^-120 / a_k) |v|-sample_k ]

tce_msda_fewq_raw_f32 samples the 256 raw channels (bound Bs as above, on src) and the map that is 1 on valid positions (bound Bw),
then applies a head's slice of value_proj in exact fp32 over K = 256:
    B = 2 [ Bs |W_h|^T + A.bound_f32(s, W_h) + |b| Bw + eps (|b w| + |out|) ].

Nothing here is fitted to what a kernel returns.  (Strictness of the range test, `> -1` against `>= -1` or `< H` against `<= H`, is
NOT among the defects below: at those positions every surviving coefficient is zero, so the two are the same function.)"""
import math

import torch

import _arith as A
from oracle import tce_oracle as O

F64 = torch.float64
EPS = A.EPS_F32
E = 2.0 ** -20
SHAPES_ODD = [(9, 13), (5, 7), (1, 4), (2, 1)]     # a level one pixel high, a level one pixel wide
SHAPES_POW2 = [(8, 16), (4, 8), (2, 4), (1, 2)]    # lattice nodes exactly representable: the exact borders are hit
VALID_ODD = [(7, 10), (4, 5), (1, 3), (1, 1)]
VALID_POW2 = [(6, 12), (3, 5), (2, 3), (1, 1)]
LOGIT_SCALES = (1.0, 30.0, 100.0)

MUTANTS = ("border_replicate", "trunc", "align_corners", "normaliser_swapped", "level_start_off_by_one", "points_i_i8_exchanged",
           "level_is_pj_mod_L", "valid_ratio_on_offset", "padded_corner_kept", "hv_wv_exchanged", "frame0_ref", "softmax_no_max",
           "head_plus_one")


def _d(x):
    return x.detach().to("cpu", F64)


def n_rows(shapes):
    return sum(h * w for h, w in shapes)


def pad_mask(shapes, valid):
    """[S] bool: True on padded positions (outside the top-left valid rectangle of each level)."""
    parts = []
    for (h, w), (hv, wv) in zip(shapes, valid):
        yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        parts.append(((yy >= hv) | (xx >= wv)).flatten())
    return torch.cat(parts)


def valid_ratios(shapes, valid):
    """fp32 quotients as the reference and the launcher compute them, as fp64: [L, 2] (x, y)."""
    valid = valid if valid is not None else shapes
    return torch.tensor([[(torch.tensor(float(wv), dtype=torch.float32) / torch.tensor(float(w), dtype=torch.float32)).item(),
                          (torch.tensor(float(hv), dtype=torch.float32) / torch.tensor(float(h), dtype=torch.float32)).item()]
                         for (h, w), (hv, wv) in zip(shapes, valid)], dtype=F64)


def nodes(n, nv=None):
    t = [-7.0, -1.5, -1.0, -1.0 + E, -0.5, -E, 0.0, E, 0.5, n - 1 - E, n - 1.0, n - 1 + E, n - 0.5, n - E, float(n), n + E, n + 3.25]
    if nv is not None:
        t += [nv - 1.0, nv - 1 + E, nv - 0.5, float(nv)]
    return t


# ---------------------------------------------------------------------------------------------------------------
# the rule, restated (mutants change a copy of it; ref_and_bound gathers with the oracle's own msda_core)
# ---------------------------------------------------------------------------------------------------------------
def core(value, shapes, loc, w, mutant=None):
    """O.msda_core restated with the switches of the gather's defects."""
    N, S, M, D = value.shape
    _, Lq, _, L, P, _ = loc.shape
    out = torch.zeros(N, Lq, M, D, dtype=value.dtype)
    start = 0
    n_idx = torch.arange(N).view(N, 1, 1, 1)
    m_idx = torch.arange(M).view(1, 1, M, 1)
    half = 0.0 if mutant == "align_corners" else 0.5
    for lvl, (H, W) in enumerate(shapes):
        st = min(start + 1, S - H * W) if mutant == "level_start_off_by_one" else start
        v = value[:, st:st + H * W]
        x = loc[:, :, :, lvl, :, 0] * W - half
        y = loc[:, :, :, lvl, :, 1] * H - half
        ok = (y > -1) & (x > -1) & (y < H) & (x < W)
        y0, x0 = (torch.trunc(y), torch.trunc(x)) if mutant == "trunc" else (torch.floor(y), torch.floor(x))
        ly, lx = y - y0, x - x0
        hy, hx = 1 - ly, 1 - lx
        y0, x0 = y0.long(), x0.long()
        acc = torch.zeros(N, Lq, M, P, D, dtype=value.dtype)
        for dy, dx, wgt in ((0, 0, hy * hx), (0, 1, hy * lx), (1, 0, ly * hx), (1, 1, ly * lx)):
            yy, xx = y0 + dy, x0 + dx
            inb = ok if mutant == "border_replicate" else ok & (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            idx = yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)
            acc = acc + v[n_idx, idx, m_idx] * (wgt * inb.to(value.dtype)).unsqueeze(-1)
        out = out + (acc * w[:, :, :, lvl, :].unsqueeze(-1)).sum(3)
        start += H * W
    return out.reshape(N, Lq, M * D)


def fused_terms(c, mutant=None, with_value=True):
    """(value64 with padded rows zeroed, loc, softmax weights, logits, dpos = dw + dh per point) of a fused / raw case in fp64."""
    N, Lq, M, L, P, rd = c["N"], c["Lq"], c["M"], c["L"], c["P"], c["ref_dim"]
    LP = L * P
    shapes, valid = c["shapes"], c["valid"]
    proj = _d(c["proj"]).view(N, Lq, M * LP * 3)
    off = proj[..., :M * LP * 2].reshape(N, Lq, M, LP, 2)
    s = proj[..., M * LP * 2:].reshape(N, Lq, M, LP)
    if mutant == "level_is_pj_mod_L":      # point pj belongs to level pj % L: the (l, p) grid read as (p, l)
        off = off.view(N, Lq, M, P, L, 2).transpose(3, 4).reshape(N, Lq, M, LP, 2)
        s = s.view(N, Lq, M, P, L).transpose(3, 4).reshape(N, Lq, M, LP)
    off = off.view(N, Lq, M, L, P, 2)
    ref = _d(c["ref"]).view(-1, Lq, rd)
    if mutant == "frame0_ref":
        ref = ref[:1]
    ref = ref.expand(N, Lq, rd)[:, :, None, None, None, :]
    use_valid = valid
    if mutant == "hv_wv_exchanged" and valid is not None:
        use_valid = [(min(wv, h), min(hv, w)) for (h, w), (hv, wv) in zip(shapes, valid)]
    vr = valid_ratios(shapes, use_valid).view(1, 1, 1, L, 1, 2)
    WH = torch.tensor([[w, h] for h, w in shapes], dtype=F64).view(1, 1, 1, L, 1, 2)
    if mutant == "normaliser_swapped":
        norm = torch.tensor([[h, w] for h, w in shapes], dtype=F64).view(1, 1, 1, L, 1, 2)
    else:
        norm = WH
    if rd == 2:
        t1, t2 = ref * vr, off / norm
        loc = (ref + off / norm) * vr if mutant == "valid_ratio_on_offset" else t1 + t2
        rel = t1.abs() + t2.abs() + loc.abs()
    else:
        t1 = ref[..., :2] * vr
        t2 = off / P * (ref[..., 2:] * vr) * 0.5
        loc = t1 + t2
        rel = t1.abs() + 3 * t2.abs() + loc.abs()
    pix = loc * WH
    dpos = (EPS * (WH * rel + pix.abs() + (pix - 0.5).abs())).sum(-1)
    if mutant == "softmax_no_max":
        e = torch.exp(s.float())
        a = (e / e.sum(-1, keepdim=True)).double()
    else:
        a = torch.softmax(s, -1)
    if mutant == "points_i_i8_exchanged" and LP == 16:
        a = torch.cat([a[..., 8:], a[..., :8]], -1)
    if not with_value:
        return None, loc, a.view(N, Lq, M, L, P), s, dpos
    value = _d(c["src"]) @ _d(c["wv"]).T + _d(c["bv"]) if c["kind"] == "raw" else _d(c["value"])
    value = value.reshape(N, n_rows(shapes), M, -1)
    if use_valid is not None and mutant != "padded_corner_kept":
        value = value.masked_fill(pad_mask(shapes, use_valid)[None, :, None, None], 0.0)
    if mutant == "head_plus_one":
        value = torch.roll(value, -1, 2)
    return value, loc, a.view(N, Lq, M, L, P), s, dpos


def sample_bound(value, shapes, loc, a, dpos, wrel):
    """Un-doubled bound of sum_k a_k sample_k: position term + sum_k a_k wrel_k |v|-sample_k.  value [N, S, M, D] (padding zeroed),
    loc [N, Lq, M, L, P, 2], a / dpos / wrel [N, Lq, M, L, P]."""
    N, S, M, D = value.shape
    Lq = loc.shape[1]
    pos = torch.zeros(N, Lq, M, D, dtype=F64)
    start = 0
    for lvl, (H, W) in enumerate(shapes):
        G = 2.0 * value[:, start:start + H * W].abs().amax(1)            # [N, M, D]
        pos = pos + (a[:, :, :, lvl] * dpos[:, :, :, lvl]).sum(-1)[..., None] * G[:, None]
        start += H * W
    return pos.reshape(N, Lq, M * D) + O.msda_core(value.abs(), shapes, loc, a * wrel + 2.0 ** -120)


def _softmax_rel(c, a, s):
    LP = c["L"] * c["P"]
    delta = EPS * (3 * s.abs() + 2 * (s - s.amax(-1, keepdim=True)).abs())
    af = a.reshape(s.shape)
    return ((LP + 6) * EPS + delta + (af * delta).sum(-1, keepdim=True) + 4 * EPS).view(a.shape)


def ref_and_bound(c):
    """(ref [N, Lq, M * D] fp64, B) of a case."""
    shapes = c["shapes"]
    if c["kind"] == "plain":
        value, loc, a = _d(c["value"]), _d(c["loc"]), _d(c["weights"])
        L, P = loc.shape[3], loc.shape[4]
        WH = torch.tensor([[w, h] for h, w in shapes], dtype=F64).view(1, 1, 1, L, 1, 2)
        pix = loc * WH
        dpos = (EPS * (pix.abs() + (pix - 0.5).abs())).sum(-1)
        ref = O.msda_core(value, shapes, loc, a)
        return ref, 2 * sample_bound(value, shapes, loc, a.abs(), dpos, torch.full_like(a, (L * P + 6) * EPS))
    value, loc, a, s, dpos = fused_terms(c)
    ref = O.msda_core(value, shapes, loc, a)
    wrel = _softmax_rel(c, a, s)
    if c["kind"] == "fused":
        return ref, 2 * sample_bound(value, shapes, loc, a, dpos, wrel)
    N, Lq, M = c["N"], c["Lq"], c["M"]
    S = n_rows(shapes)
    src = _d(c["src"]).view(N, S, 256)
    one = torch.ones(N, S, 1, dtype=F64)
    if c["valid"] is not None:
        pm = pad_mask(shapes, c["valid"])[None, :, None]
        src, one = src.masked_fill(pm, 0.0), one.masked_fill(pm, 0.0)
    raw = torch.cat([src, one], -1)[:, :, None, :].expand(N, S, M, 257)
    sm = O.msda_core(raw, shapes, loc, a).view(N, Lq, M, 257)
    Bsm = sample_bound(raw, shapes, loc, a, dpos, wrel).view(N, Lq, M, 257)
    wv, bv = _d(c["wv"]).view(M, 32, 256), _d(c["bv"]).view(M, 32)
    B = torch.einsum("nqmk,mdk->nqmd", Bsm[..., :256], wv.abs())
    B = B + 256 * EPS * torch.einsum("nqmk,mdk->nqmd", sm[..., :256].abs(), wv.abs())
    B = B + bv.abs() * Bsm[..., 256:] + EPS * (bv.abs() * sm[..., 256:].abs() + ref.view(N, Lq, M, 32).abs())
    return ref, 2 * B.reshape(N, Lq, M * 32)


def ref_and_bound_fn(c, value_fn, vmax, D=32):
    """ref_and_bound of an un-padded fused case whose value tensor is value_fn(flat index) (|.| <= vmax), evaluated only at the rows
    the reference gathers: for value tensors too large to hold twice."""
    shapes, N, Lq, M, P = c["shapes"], c["N"], c["Lq"], c["M"], c["P"]
    _, loc, a, s, dpos = fused_terms(c, with_value=False)
    wrel = _softmax_rel(c, a, s)
    S = n_rows(shapes)
    out = torch.zeros(N, Lq, M, D, dtype=F64)
    sab = torch.zeros(N, Lq, M, D, dtype=F64)
    n_idx = torch.arange(N).view(N, 1, 1, 1)
    m_idx = torch.arange(M).view(1, 1, M, 1)
    start = 0
    for lvl, (H, W) in enumerate(shapes):
        x = loc[:, :, :, lvl, :, 0] * W - 0.5
        y = loc[:, :, :, lvl, :, 1] * H - 0.5
        ok = (y > -1) & (x > -1) & (y < H) & (x < W)
        y0, x0 = torch.floor(y), torch.floor(x)
        ly, lx = y - y0, x - x0
        hy, hx = 1 - ly, 1 - lx
        y0, x0 = y0.long(), x0.long()
        for dy, dx, wgt in ((0, 0, hy * hx), (0, 1, hy * lx), (1, 0, ly * hx), (1, 1, ly * lx)):
            yy, xx = y0 + dy, x0 + dx
            inb = ok & (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            row = n_idx * S + start + yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)
            v = value_fn(((row * M + m_idx) * D)[..., None] + torch.arange(D)).double()
            cw = (wgt * inb.double())[..., None]
            out = out + (v * cw * a[:, :, :, lvl, :, None]).sum(3)
            sab = sab + (v.abs() * cw * (a * wrel + 2.0 ** -120)[:, :, :, lvl, :, None]).sum(3)
        start += H * W
    pos = 2.0 * vmax * (a * dpos).sum((-1, -2))[..., None]
    return out.reshape(N, Lq, M * D), 2 * (pos + sab).reshape(N, Lq, M * D)


def emulate(c, mutant=None):
    """The rule on the CPU in fp64 from the restatement above, optionally with one defect."""
    if c["kind"] == "plain":
        value, loc, a = _d(c["value"]), _d(c["loc"]), _d(c["weights"])
        if mutant == "head_plus_one":
            value = torch.roll(value, -1, 2)
        if mutant == "points_i_i8_exchanged" and a.shape[3] * a.shape[4] == 16:
            af = a.flatten(3)
            a = torch.cat([af[..., 8:], af[..., :8]], -1).view(a.shape)
        return core(value, c["shapes"], loc, a, mutant)
    value, loc, a, _, _ = fused_terms(c, mutant)
    return core(value, c["shapes"], loc, a, mutant)


def oracle_fp32(c):
    """O.msda_core on fp32 tensors with the formulas around it in fp32 too: a correct fp32 evaluation."""
    shapes = c["shapes"]
    if c["kind"] == "plain":
        return O.msda_core(c["value"], shapes, c["loc"], c["weights"])
    N, Lq, M, L, P, rd = c["N"], c["Lq"], c["M"], c["L"], c["P"], c["ref_dim"]
    LP = L * P
    proj = c["proj"].view(N, Lq, M * LP * 3)
    off = proj[..., :M * LP * 2].reshape(N, Lq, M, L, P, 2)
    a = torch.softmax(proj[..., M * LP * 2:].reshape(N, Lq, M, LP), -1).view(N, Lq, M, L, P)
    ref = c["ref"].view(-1, Lq, rd).expand(N, Lq, rd)[:, :, None, None, None, :]
    vr = valid_ratios(shapes, c["valid"]).float().view(1, 1, 1, L, 1, 2)
    WH = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float32).view(1, 1, 1, L, 1, 2)
    loc = ref * vr + off / WH if rd == 2 else ref[..., :2] * vr + off / P * (ref[..., 2:] * vr) * 0.5
    value = c["src"] @ c["wv"].T + c["bv"] if c["kind"] == "raw" else c["value"]
    value = value.reshape(N, n_rows(shapes), M, -1)
    if c["valid"] is not None:
        value = value.masked_fill(pad_mask(shapes, c["valid"])[None, :, None, None], 0.0)
    return O.msda_core(value, shapes, loc, a)


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
def _value(g, N, shapes, valid, M, D):
    """randn rows; rows on padding hold 1e4 * (1 + row index): finite, and any leak is enormous."""
    S = n_rows(shapes)
    v = torch.randn(N, S, M, D, generator=g)
    if valid is not None:
        pm = pad_mask(shapes, valid)
        fill = 1e4 * (1.0 + torch.arange(S, dtype=torch.float32))
        v = torch.where(pm[None, :, None, None], fill[None, :, None, None].expand_as(v), v)
    return v


def _pack(c, off, logits, ref, value=None, raw=None):
    """off [N, Lq, M, L, P, 2], logits [N, Lq, M, L*P], ref [Nr, Lq, rd] (fp64) -> the fp32 tensors of the ABI."""
    N, Lq, M, LP = c["N"], c["Lq"], c["M"], c["L"] * c["P"]
    c["proj"] = torch.cat([off.reshape(N * Lq, M * LP * 2), logits.reshape(N * Lq, M * LP)], 1).float().contiguous()
    c["ref"] = ref.float().contiguous()
    if raw is not None:
        c["kind"], (c["src"], c["wv"], c["bv"]) = "raw", raw
    else:
        c["kind"], c["value"] = "fused", value
    return c


def _raw_operands(g, N, shapes, valid):
    S = n_rows(shapes)
    src = _value(g, N, shapes, valid, 1, 256).view(N * S, 256)
    return src, torch.randn(256, 256, generator=g) / 16.0, torch.randn(256, generator=g)


def _lattice_targets(shapes, valid, L):
    """[nodes^2, L, 2] normalised (x, y): query (iy, ix) sits on node (tx[ix], ty[iy]) of EVERY level's own lattice."""
    per = []
    for l in range(L):
        (h, w), (hv, wv) = shapes[l], (valid[l] if valid is not None else (None, None))
        tx, ty = torch.tensor(nodes(w, wv), dtype=F64), torch.tensor(nodes(h, hv), dtype=F64)
        yy, xx = torch.meshgrid(ty, tx, indexing="ij")
        per.append(torch.stack([(xx.flatten() + 0.5) / w, (yy.flatten() + 0.5) / h], -1))
    return torch.stack(per, 1)


def lattice_plain(shapes, N, M, D, P, seed, reps=1):
    """Plain op: loc IS the lattice; weights the fp32 softmax of randn."""
    g = torch.Generator().manual_seed(int(seed))
    L = len(shapes)
    tgt = _lattice_targets(shapes, None, L).repeat(reps, 1, 1)
    Lq = tgt.shape[0]
    loc = tgt.float()[None, :, None, :, None, :].expand(N, Lq, M, L, P, 2).contiguous()
    w = torch.softmax(torch.randn(N, Lq, M, L * P, generator=g), -1).view(N, Lq, M, L, P)
    return dict(kind="plain", shapes=shapes, valid=None, N=N, Lq=Lq, M=M, L=L, P=P, value=_value(g, N, shapes, None, M, D), loc=loc,
                weights=w, note="lattice")


def lattice_fused(shapes, valid, N, M, L, P, mode, rd, rpf, seed, reps=1, raw=False, logit_scale=1.0):
    """mode "off": ref = 0 (ref_dim 4: (0, 0, 1, 1)) and the offsets carry every level's own lattice, Lq = nodes^2 * reps.
    mode "ref": offsets 0 and the reference point carries the lattice of ONE level (vr folded out), Lq = nodes^2 * L * reps: block
    q // nodes^2 % L aims at that level (the other levels sample wherever the same point falls); with ref_per_frame frame n's
    reference points are frame 0's rolled by 7 n queries."""
    g = torch.Generator().manual_seed(int(seed))
    shapes = shapes[:L]
    valid = valid[:L] if valid is not None else None
    tgt = _lattice_targets(shapes, valid, L)
    vr = valid_ratios(shapes, valid)
    nq = tgt.shape[0]
    if mode == "off":
        Lq = nq * reps
        t = tgt.repeat(reps, 1, 1)[None, :, None, :, None, :].expand(N, Lq, M, L, P, 2)
        if rd == 2:
            off = t * torch.tensor([[w, h] for h, w in shapes], dtype=F64).view(1, 1, 1, L, 1, 2)
            ref = torch.zeros(1, Lq, 2, dtype=F64)
        else:
            off = t * 2.0 * P / vr.view(1, 1, 1, L, 1, 2)
            ref = torch.tensor([0.0, 0.0, 1.0, 1.0], dtype=F64).expand(1, Lq, 4)
        ref = ref.expand(N if rpf else 1, Lq, rd)
    else:
        Lq = nq * L * reps
        xy = torch.cat([tgt[:, l] / vr[l] for l in range(L)], 0).repeat(reps, 1)
        r0 = xy if rd == 2 else torch.cat([xy, 0.1 + torch.rand(Lq, 2, generator=g).double()], 1)
        ref = torch.stack([torch.roll(r0, 7 * n, 0) for n in range(N)], 0) if rpf else r0[None]
        off = torch.zeros(N, Lq, M, L, P, 2, dtype=F64)
    logits = torch.randn(N, Lq, M, L * P, generator=g).double() * logit_scale
    c = dict(shapes=shapes, valid=valid, N=N, Lq=Lq, M=M, L=L, P=P, ref_dim=rd, ref_per_frame=int(bool(rpf)),
             note=f"lattice via {mode}")
    if raw:
        return _pack(c, off, logits, ref, raw=_raw_operands(g, N, shapes, valid))
    return _pack(c, off, logits, ref, value=_value(g, N, shapes, valid, M, 32))


def code_value(N, shapes, M, D):
    """value[n, s, m, d] = (((s + 31 n) % S) * M + m) * D + d: an exactly representable integer that names the row (rotated per frame,
    so a wrong frame is a wrong row), the head and the channel.  Kept small: the bound resolves max|v| * ~1e-5."""
    S = n_rows(shapes)
    n, s, m, d = torch.meshgrid(torch.arange(N), torch.arange(S), torch.arange(M), torch.arange(D), indexing="ij")
    return ((((s + 31 * n) % S) * M + m) * D + d).float()


def decode(x, M, D):
    """(row code (s + 31 n) % S, head, channel) nearest to an output value of a code_value tensor."""
    k = int(round(float(x)))
    return k // (M * D), (k // D) % M, k % D


def _interior(g, shapes, n):
    """n distinct interior pixel centres per level, normalised: [n, L, 2]; off-centre by a per-point fraction so that the four corners
    all carry weight at levels wider than a pixel."""
    per = []
    for h, w in shapes:
        fx, fy = torch.rand(n, generator=g).double() * 0.5 + 0.25, torch.rand(n, generator=g).double() * 0.5 + 0.25
        ix = torch.randint(0, max(w - 1, 1), (n,), generator=g).double()
        iy = torch.randint(0, max(h - 1, 1), (n,), generator=g).double()
        per.append(torch.stack([(ix + fx + 0.5) / w if w > 1 else torch.full((n,), 0.5, dtype=F64),
                                (iy + fy + 0.5) / h if h > 1 else torch.full((n,), 0.5, dtype=F64)], -1))
    return torch.stack(per, 1)


def dense_fused(shapes, valid, N, Lq, M, L, P, rd, rpf, seed, logit_scale=1.0, onehot=False, raw=False, code=False, value=True, edges=False):
    """Random reference points and offsets; logits randn * logit_scale, or one-hot: query q has logit 0 at slot q % (L*P) and -200
    elsewhere (an fp32 weight of exactly 0), every slot at its own interior location."""
    g = torch.Generator().manual_seed(int(seed))
    shapes = shapes[:L]
    valid = valid[:L] if valid is not None else None
    LP = L * P
    WH = torch.tensor([[w, h] for h, w in shapes], dtype=F64).view(1, 1, 1, L, 1, 2)
    vr = valid_ratios(shapes, valid).view(1, 1, 1, L, 1, 2)
    Nr = N if rpf else 1
    rxy = torch.rand(Nr, Lq, 2, generator=g).double() * 0.8 + 0.1
    if onehot:
        tgt = _interior(g, shapes, N * Lq * M * P).view(N, Lq, M, P, L, 2).transpose(3, 4)
        if valid is not None:   # keep the probed location on the valid part
            tgt = tgt * vr
        if edges:   # frame 0 probes the first two rows of the value tensor's first level, the last frame the last two of its last
            (h0, w0), (h1, w1) = shapes[0], shapes[-1]
            tgt = tgt.clone()
            tgt[0, :, :, 0, :, 1] = (torch.rand(Lq, M, P, generator=g).double() * 0.9 + 0.5) / h0
            tgt[-1, :, :, -1, :, 1] = (h1 - 2 + torch.rand(Lq, M, P, generator=g).double() * 0.9 + 0.5) / h1
    else:
        tgt = None
    if rd == 2:
        ref = rxy
        r = ref.expand(N, Lq, 2)[:, :, None, None, None, :]
        off = (tgt - r * vr) * WH if onehot else torch.randn(N, Lq, M, L, P, 2, generator=g).double() * 1.5
    else:
        ref = torch.cat([rxy, torch.rand(Nr, Lq, 2, generator=g).double() * 0.3 + 0.05], -1)
        r = ref.expand(N, Lq, 4)[:, :, None, None, None, :]
        off = (tgt - r[..., :2] * vr) * 2.0 * P / (r[..., 2:] * vr) if onehot else torch.randn(N, Lq, M, L, P, 2, generator=g).double() * 2.0
    if onehot:
        slot = (torch.arange(Lq)[None, :, None] + torch.arange(M)[None, None, :] + 3 * torch.arange(N)[:, None, None]) % LP
        logits = torch.full((N, Lq, M, LP), -200.0, dtype=F64).scatter_(3, slot[..., None], 0.0)
    else:
        logits = torch.randn(N, Lq, M, LP, generator=g).double() * logit_scale
    c = dict(shapes=shapes, valid=valid, N=N, Lq=Lq, M=M, L=L, P=P, ref_dim=rd, ref_per_frame=int(bool(rpf)),
             note="one-hot" if onehot else f"logits x {logit_scale:g}")
    if raw:
        return _pack(c, off, logits, ref, raw=_raw_operands(g, N, shapes, valid))
    if not value:   # the caller fills value on the device from a formula (ref_and_bound_fn)
        return _pack(c, off, logits, ref, value=None)
    value = code_value(N, shapes, M, 32) if code else _value(g, N, shapes, valid, M, 32)
    if code and valid is not None:
        pm = pad_mask(shapes, valid)
        value = torch.where(pm[None, :, None, None], 1e4 * (1.0 + torch.arange(value.shape[1]).float())[None, :, None, None].expand_as(value), value)
    return _pack(c, off, logits, ref, value=value)


def dense_plain(shapes, N, Lq, M, D, P, seed, logit_scale=1.0, onehot=False, code=False):
    """Plain op: random locations in [-0.1, 1.1]; weights the fp32 softmax of randn * logit_scale, or the one-hot probe."""
    g = torch.Generator().manual_seed(int(seed))
    L = len(shapes)
    LP = L * P
    if onehot:
        loc = _interior(g, shapes, N * Lq * M * P).view(N, Lq, M, P, L, 2).transpose(3, 4).float().contiguous()
        slot = (torch.arange(Lq)[None, :, None] + torch.arange(M)[None, None, :] + 3 * torch.arange(N)[:, None, None]) % LP
        w = torch.zeros(N, Lq, M, LP).scatter_(3, slot[..., None], 1.0)
    else:
        loc = torch.rand(N, Lq, M, L, P, 2, generator=g) * 1.2 - 0.1
        w = torch.softmax(torch.randn(N, Lq, M, LP, generator=g) * logit_scale, -1)
    value = code_value(N, shapes, M, D) if code else _value(g, N, shapes, None, M, D)
    return dict(kind="plain", shapes=shapes, valid=None, N=N, Lq=Lq, M=M, L=L, P=P, value=value, loc=loc, weights=w.view(N, Lq, M, L, P),
                note="one-hot" if onehot else f"logits x {logit_scale:g}")


def slot_of(c, n, q, m):
    return (q + m + 3 * n) % (c["L"] * c["P"])


def worst(out, ref, B):
    """(max err / B with an exact element counted as inside, flat index, max err / max|ref|)."""
    out, ref = _d(out).reshape(ref.shape), _d(ref)
    err = (out - ref).abs().nan_to_num(nan=float("inf"))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / B)
    i = int(ratio.argmax())
    return float(ratio.flatten()[i]), i, float(err.max() / ref.abs().max().clamp_min(1e-300))


def describe(c, i):
    """Where flat output element i sits: frame, query -> lattice node or point slot, head, channel."""
    D = 32 if c["kind"] != "plain" else c["value"].shape[-1]
    M, Lq = c["M"], c["Lq"]
    d, m = i % D, (i // D) % M
    q, n = (i // (D * M)) % Lq, i // (D * M * Lq)
    where = f"frame {n}, query {q}, head {m}, channel {d}"
    if c["note"].startswith("lattice"):
        k = int(round(math.sqrt(_lattice_targets(c["shapes"], c["valid"], c["L"]).shape[0])))
        node = q % (k * k)
        (h, w) = c["shapes"][0]
        v0 = c["valid"][0] if c["valid"] is not None else (None, None)
        where += f" -> lattice node (x {nodes(w, v0[1])[node % k]:g}, y {nodes(h, v0[0])[node // k]:g}) of level 0's numbering, block {q // (k * k)}"
    elif c["note"] == "one-hot":
        s = slot_of(c, n, q, m)
        where += f" -> point slot {s} (level {s // c['P']}, point {s % c['P']})"
    return where
