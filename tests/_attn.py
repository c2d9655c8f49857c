"""The generic attention core (tce_mha_f32 / tce_mha_ws_f32, csrc/attn.hip) as a test subject: which of its seven launch forms a
call selects, the smallest shapes that select each, key masks and score designs that put an online softmax into the states it gets
wrong, the memory layouts the pipeline really passes, the fp64 reference with its derived bound, and plain-torch emulations with one
planted defect each.  Pure torch; needs no GPU and loads no native library."""
import math

import torch

import _arith as A

KT = 32          # keys per tile, every kernel
NW = 4           # waves of a KSPLIT workgroup
SCALE = 32 ** -0.5
MODES = ("f32", "f16x3", "f16")
PRODUCT = {"f32": A.bound_split, "f16x3": A.bound_split, "f16": A.bound_f16}   # exact mode: bound_split contains the fp32 bound


def cdiv(a, b):
    return -(-a // b)


def mha_form(batch, nh, Lq, Lk, mode, ws):
    """F1..F7: the kernel a call of ops.mha_core launches.

    A RESTATEMENT of the dispatch, not a query: the library has no entry that reports which kernel ran.  It mirrors
    ops.mha_core (ops.py: the workspace form needs an allocator, Lk >= ops.MHA_WS_MIN_KEYS and a split mode), tce_mha_f32
    (attn.hip, the body of tce_mha_f32: tiles, nw, the Lk >= 256 split-mode branch, ksplit = tiles < 4096 && Lk >= 1024) and
    tce_mha_ws_f32 (attn.hip: tiles < 4096 picks the KSPLIT instantiation).  If the dispatcher changes, this changes with it.
        F1 mha_mfma_kernel<1>   F2 mha_mfma_kernel<4>   F3 mha_f16x3_kernel<1,false>   F4 mha_f16x3_kernel<4,false>
        F5 mha_f16x3_kernel<4,KSPLIT>   F6 mha_presplit_kernel<KSPLIT>   F7 mha_presplit_kernel<false>"""
    from tce_rvos_amd import ops
    tiles = cdiv(Lq, KT) * batch * nh
    if ws and Lk >= ops.MHA_WS_MIN_KEYS and mode != "f32":
        return "F6" if tiles < 4096 else "F7"
    if mode != "f32" and Lk >= 256:
        if tiles < 4096 and Lk >= 1024:
            return "F5"
        return "F4" if tiles >= 4096 else "F3"
    return "F2" if tiles >= 4096 else "F1"


SPLIT_MODES = ("f16x3", "f16")
# (name, batch, nh, Lq, Lk, workspace passed, modes).  The first entry of a form is its smallest shape; the others sit on a threshold.
CASES = (
    ("F1", 2, 3, 77, 40, False, MODES),
    ("F2", 16, 8, 1000, 33, False, MODES),            # 4096 tiles exactly, ragged last query tile, one partial key tile beside a full one
    ("F1 at 3968 tiles", 16, 8, 992, 33, False, MODES),
    ("F3", 2, 3, 77, 257, False, SPLIT_MODES),
    ("F1 at Lk=255", 2, 3, 77, 255, False, SPLIT_MODES),
    ("F3 at Lk=256", 2, 3, 77, 256, False, SPLIT_MODES),
    ("F4", 16, 8, 1000, 257, False, SPLIT_MODES),
    ("F5", 2, 3, 77, 1056, False, SPLIT_MODES),       # 33 key tiles: the four waves own tiles 0-8 / 8-16 / 16-24 / 24-33
    ("F3 at Lk=1023", 2, 3, 77, 1023, False, SPLIT_MODES),
    ("F5 at Lk=1024", 2, 3, 77, 1024, False, SPLIT_MODES),
    ("F6", 2, 3, 77, 1025, True, SPLIT_MODES),        # Lkp = 1056: 31 padding keys
    ("F7", 16, 8, 1000, 1025, True, SPLIT_MODES),
    ("F3 at Lk=1023 (workspace offered)", 2, 3, 77, 1023, True, SPLIT_MODES),
    ("F6 at Lk=1024", 2, 3, 77, 1024, True, SPLIT_MODES),
)
PRIMARY = tuple(c for c in CASES if c[0] in ("F1", "F2", "F3", "F4", "F5", "F6", "F7"))
BOUNDARY = tuple(c for c in CASES if c not in PRIMARY)


def case(name):
    return next(c for c in CASES if c[0] == name)


# ---------------------------------------------------------------------------------------------------------------
# Key masks: uint8 [batch, Lk], non-zero = ignore the key
# ---------------------------------------------------------------------------------------------------------------
def wave_tiles(Lk, w):
    """[t_begin, t_end) of KSPLIT wave w, the kernels' own formula (attn.hip: t_begin / t_end of mha_f16x3_kernel and mha_presplit_kernel)."""
    nt = cdiv(Lk, KT)
    return w * nt // NW, (w + 1) * nt // NW


def _rand(batch, Lk, p, seed):
    g = torch.Generator().manual_seed(int(seed))
    return (torch.rand(batch, Lk, generator=g) < p).to(torch.uint8)


def mask_m0(batch, Lk, seed=0):
    return None


def mask_m1(batch, Lk, seed=0):
    """The first key tile entirely masked: the running maximum leaves tile 0 at the sentinel."""
    m = torch.zeros(batch, Lk, dtype=torch.uint8)
    m[:, :KT] = 1
    return m


def interior_tile(Lk):
    nt = cdiv(Lk, KT)
    return nt // 2 if nt >= 3 else nt - 1   # fewer than three tiles: the last


def mask_m2(batch, Lk, seed=0):
    """Random 30 % and one interior tile entirely masked; key 0 kept."""
    m = _rand(batch, Lk, 0.3, 1000 + seed)
    t = interior_tile(Lk)
    m[:, t * KT:(t + 1) * KT] = 1
    m[:, 0] = 0
    return m


def m3_start(Lk, b=0):
    s = max(1, 3 * Lk // 4 - 3 * b)
    return s + 5 if s % KT == 0 else s


def mask_m3(batch, Lk, seed=0):
    """Everything from a key index that is no multiple of 32 to the end (ragged captions, padded clips); the index differs by entry."""
    m = torch.zeros(batch, Lk, dtype=torch.uint8)
    for b in range(batch):
        m[b, m3_start(Lk, b):] = 1
    return m


def mask_head(batch, Lk, seed=0):
    """An interior block near the start, keys 1 .. Lk/4: for scores that FALL with the key index, where a masked tail is blind."""
    m = torch.zeros(batch, Lk, dtype=torch.uint8)
    m[:, 1:max(2, Lk // 4) + 1] = 1
    return m


def mask_m4(waves):
    """Every key tile of the KSPLIT waves `waves`: such a wave carries (m, l) = (sentinel, 0) into the merge."""
    def build(batch, Lk, seed=0):
        m = torch.zeros(batch, Lk, dtype=torch.uint8)
        for w in waves:
            t0, t1 = wave_tiles(Lk, w)
            m[:, t0 * KT:t1 * KT] = 1
        return m
    return build


def m5_keys(batch, Lk):
    """The one kept key of each batch entry: the last key, a key of the last (ragged) tile, then keys spread over the rest."""
    last_tile = (cdiv(Lk, KT) - 1) * KT
    picks = [Lk - 1, last_tile, 0, KT - 1, KT, Lk // 2]
    return [picks[b] if b < len(picks) else (b * 37) % Lk for b in range(batch)]


def mask_m5(batch, Lk, seed=0):
    m = torch.ones(batch, Lk, dtype=torch.uint8)
    for b, j in enumerate(m5_keys(batch, Lk)):
        m[b, j] = 0
    return m


def mask_m6(batch, Lk, seed=0):
    """A different random half per batch entry, the same for every head: catches b against b * nheads + h indexing."""
    m = _rand(batch, Lk, 0.5, 2000 + seed)
    for b in range(batch):
        m[b, (7 * b) % Lk] = 0
    return m


def mask_m7(batch, Lk, seed=0):
    """Batch entry 1 entirely masked, the others random 30 %."""
    m = _rand(batch, Lk, 0.3, 3000 + seed)
    m[:, 0] = 0
    m[1] = 1
    return m


MASKS = {"M0": mask_m0, "M1": mask_m1, "M2": mask_m2, "M3": mask_m3, "M5": mask_m5, "M6": mask_m6}
MASKS_M4 = {"M4 wave 0": mask_m4((0,)), "M4 wave 3": mask_m4((3,)), "M4 waves 0,1,3": mask_m4((0, 1, 3))}


# ---------------------------------------------------------------------------------------------------------------
# Operands: (q [batch, Lq, E], k, v [batch, Lk, E]) fp32
# ---------------------------------------------------------------------------------------------------------------
def _unit(nh, g):
    u = torch.randn(nh, 32, generator=g)
    return u / u.norm(dim=1, keepdim=True)


def operands(design, batch, nh, Lq, Lk, seed=0, mask=None):
    """N: q, k, v ~ N(0, 1), |s| <= ~5.
    S1: keys along a fixed direction per head, s rises with the key index from 0 to 60..75 (by query): the running maximum rises in
        every tile.      S2: S1 reversed: the maximum is set by the first tile and corr = 1 ever after.
    S3: two keys far ahead, s ~ 115 and s ~ 230 (the others |s| <= ~5); the higher is batch entry b's FIRST MASKED key, the
        lower its first kept key that is not key 0: the row is one-hot on the lower, and e^-104 is below the smallest fp32 subnormal.
    S4: q = 0: all scores tie, the output is the mean of the kept V rows."""
    g = torch.Generator().manual_seed(int(seed) * 7919 + Lq * 31 + Lk)
    E = nh * 32
    q, k, v = (torch.randn(batch, L, E, generator=g) for L in (Lq, Lk, Lk))
    if design == "N":
        return q, k, v
    if design == "S4":
        return torch.zeros_like(q), k, v
    u = _unit(nh, g)                                                    # [nh, 32]
    q, k = 0.25 * q.view(batch, Lq, nh, 32), 0.25 * k.view(batch, Lk, nh, 32)
    # remove the noise's component along u, so that the designed part of a score is exact in the design
    q = q - (q * u).sum(-1, keepdim=True) * u
    k = k - (k * u).sum(-1, keepdim=True) * u
    if design in ("S1", "S2"):
        top = 60.0 + 15.0 * torch.rand(batch, Lq, nh, 1, generator=g)   # the row's largest score
        ramp = torch.linspace(0.0, 1.0, Lk).view(1, Lk, 1, 1)
        if design == "S2":
            ramp = ramp.flip(1)
        q = q + (top / (8.0 * SCALE)) * u                                # q . k * SCALE = top * ramp
        k = k + 8.0 * ramp * u
    elif design == "S3":
        assert mask is not None, "S3 places its keys by the mask"
        q = q + (20.0 / SCALE / 8.0) * u                                 # q . (c u) * SCALE = 2.5 c
        for b in range(batch):
            masked = torch.nonzero(mask[b]).flatten()
            kept = torch.nonzero(mask[b] == 0).flatten()
            k[b, int(masked[0])] += 92.0 * u                             # s ~ 230
            k[b, int(kept[kept > 0][0] if (kept > 0).any() else kept[0])] += 46.0 * u   # s ~ 115
    else:
        raise ValueError(design)
    return q.reshape(batch, Lq, E).contiguous(), k.reshape(batch, Lk, E).contiguous(), v


# (design, mask name): the mask under which the design's MASKED keys would carry visible probability
def design_mask(design, Lk):
    return ("head", mask_head) if design == "S2" else ("M3", mask_m3)


DESIGNS = ("S1", "S2", "S3", "S4")


# ---------------------------------------------------------------------------------------------------------------
# Reference and bound
# ---------------------------------------------------------------------------------------------------------------
def attention_ref_and_bound(q, k, v, scale, add=None, Bq=None, Bk=None, Bv=None, product=A.bound_split):
    """One head: q [Lq, 32], k / v [Lk, 32] -> softmax(scale q k^T + add) v and its bound (x 2).  The scores carry the product's
    error and the fp32 roundings of the scaled score, of the added bias / mask, of the subtraction of the row maximum and of its
    conversion to a base-2 exponent; exp and the normalisation a few ulp of p.  Bq / Bk / Bv: what the operands themselves are off by (fused kernels that project them).
    product: the bound of both matrix products (A.bound_split; A.bound_f16 in mode "f16")."""
    q64, k64, v64 = q.double() * scale, k.double(), v.double()
    s = q64 @ k64.T
    Bs = product(q64, k64, A.c_dense(32))
    if Bq is not None:
        Bs = Bs + scale * A.chain(Bq, k64) + A.chain(q64.abs(), Bk)
    if add is not None:
        s = s + add.double()
    Bs = Bs + A.EPS_F32 * (3 * s.abs() + 2 * (s - s.amax(1, keepdim=True)).abs())
    p = torch.softmax(s, -1)
    bs = Bs.amax(1, keepdim=True)
    S = p @ v64.abs()
    B = A.softmax_v_bound(p, v64, bs, A.c_dense(k.shape[0]), product) + 4 * A.EPS_F32 * S
    if Bv is not None:
        B = B + p @ Bv
    return p @ v64, 2 * B, S


def masked_ref_and_bound(q, k, v, mask, nh, scale=SCALE, product=A.bound_split, device="cpu"):
    """q [batch, Lq, E], k / v [batch, Lk, E], mask uint8 [batch, Lk] or None -> (ref, B, S) fp64 [batch, Lq, E] on `device`:
    attention_ref_and_bound per (batch, head) over the KEPT keys only.  An ignored key contributes exact zeros whatever its K row
    holds (an additive -inf would make the bound infinite); an entry with no kept key is exact zeros with bound 0.  No margin."""
    batch, Lq, E = q.shape
    with A.on(device):
        q, k, v = (t.to(device) for t in (q, k, v))
        ref, B, S = (torch.zeros(batch, Lq, E, dtype=torch.float64, device=device) for _ in range(3))
        for b in range(batch):
            keep = torch.ones(k.shape[1], dtype=torch.bool, device=device) if mask is None else (mask[b] == 0).to(device)
            if not bool(keep.any()):
                continue
            kb, vb = k[b][keep], v[b][keep]
            for h in range(nh):
                sl = slice(32 * h, 32 * h + 32)
                ref[b, :, sl], B[b, :, sl], S[b, :, sl] = attention_ref_and_bound(q[b, :, sl], kb[:, sl], vb[:, sl], scale, product=product)
    return ref, B, S


def ratio(out, ref, B):
    """err / B per element; an exact result is inside any bound (B = 0 included), NaN is infinitely outside."""
    err = (out.double() - ref).abs().nan_to_num(nan=float("inf"))
    return torch.where(err == 0, torch.zeros_like(err), err / B)


# ---------------------------------------------------------------------------------------------------------------
# Plain fp32 torch, and the same with one planted defect
# ---------------------------------------------------------------------------------------------------------------
def _heads(t, nh):
    b, L, E = t.shape
    return t.view(b, L, nh, 32).permute(0, 2, 1, 3)   # [batch, nh, L, 32]


def torch_f32(q, k, v, mask, nh, scale=SCALE):
    """scores, masked_fill, softmax, @ v in fp32 (an entry with no kept key: zeros, the kernels' rule)."""
    s = (_heads(q, nh) * scale) @ _heads(k, nh).transpose(-1, -2)
    if mask is not None:
        s = s.masked_fill(mask.bool()[:, None, None, :], float("-inf"))
    p = torch.softmax(s, -1).nan_to_num(nan=0.0)
    o = p @ _heads(v, nh)
    return o.permute(0, 2, 1, 3).reshape(q.shape)


def first_masked(mask):
    return [int(torch.nonzero(mask[b]).flatten()[0]) if bool(mask[b].any()) else None for b in range(mask.shape[0])]


def defect_leak(q, k, v, mask, nh):
    """One masked key let in: the lowest-indexed masked key of every batch entry."""
    m = mask.clone()
    for b, j in enumerate(first_masked(mask)):
        if j is not None:
            m[b, j] = 0
    return torch_f32(q, k, v, m, nh)


def defect_batch_shift(q, k, v, mask, nh):
    """The mask of batch entry b applied to entry b + 1."""
    return torch_f32(q, k, v, mask.roll(1, 0), nh)


def kept_tiles(mask, Lk, b=0):
    keep = torch.ones(Lk, dtype=torch.bool) if mask is None else mask[b] == 0
    return sorted(set((torch.nonzero(keep).flatten() // KT).tolist()))


def defect_drop_tile(which):
    """One key tile dropped: the first or the last tile in which batch entry 0 keeps a key."""
    def go(q, k, v, mask, nh):
        Lk = k.shape[1]
        t = kept_tiles(mask, Lk)[0 if which == "first" else -1]
        m = torch.zeros(q.shape[0], Lk, dtype=torch.uint8) if mask is None else mask.clone()
        m[:, t * KT:(t + 1) * KT] = 1
        return torch_f32(q, k, v, m, nh)
    return go


def ksplit_f32(q, k, v, mask, nh, bad_wave=None, scale=SCALE):
    """The KSPLIT forms' structure in fp32: each of the four waves reduces its own tiles to (m_w, l_w, O_w) from the sentinel
    -3e38, and the partials merge with the weights exp(m_w - m*).  bad_wave: that wave's partial merged with weight 1."""
    batch, Lq, E = q.shape
    Lk = k.shape[1]
    s = (_heads(q, nh) * scale) @ _heads(k, nh).transpose(-1, -2)
    if mask is not None:
        s = s.masked_fill(mask.bool()[:, None, None, :], -3.0e38)
    vh = _heads(v, nh)
    ms, ls, os_ = [], [], []
    for w in range(NW):
        t0, t1 = wave_tiles(Lk, w)
        sw = s[..., t0 * KT:min(t1 * KT, Lk)]
        m = sw.amax(-1, keepdim=True).clamp_min(-3.0e38) if sw.shape[-1] else torch.full_like(s[..., :1], -3.0e38)
        p = torch.where(sw > -1.0e38, torch.exp(sw - m), torch.zeros_like(sw))
        ms.append(m), ls.append(p.sum(-1, keepdim=True)), os_.append(p @ vh[:, :, t0 * KT:min(t1 * KT, Lk)])
    mstar = torch.stack(ms).amax(0)
    l, o = torch.zeros_like(ls[0]), torch.zeros_like(os_[0])
    for w in range(NW):
        f = torch.ones_like(mstar) if w == bad_wave else torch.exp(ms[w] - mstar)
        l, o = l + ls[w] * f, o + os_[w] * f
    o = torch.where(l > 0, o / l, torch.zeros_like(o))
    return o.permute(0, 2, 1, 3).reshape(q.shape)


def defect_merge_weight_one(bad_wave):
    def go(q, k, v, mask, nh):
        return ksplit_f32(q, k, v, mask, nh, bad_wave=bad_wave)
    return go
