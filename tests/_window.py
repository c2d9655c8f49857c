"""The Swin and Video-Swin window-attention kernels (tce_window_attn_f32, tce_window_attn3d_f32: csrc/attn.hip; tce_swin_attn_fused_f32:
csrc/swinattn.hip) as a test subject: which of their six launch forms a call selects, the smallest frame sizes that reach each edge of
the window geometry, operand designs that make the finite -100 shift mask, the padded tokens, the relative-position index and the
base-2 online softmax of the 3-D kernel decide the result, the fp64 reference built from the oracle's own geometry functions with the
derived bound of tests/_arith.py, and plain-torch fp32 emulations with one planted defect each.  Pure torch; needs no GPU and loads
no native library."""
import math

import torch
import torch.nn.functional as F

import _arith as A
from _attn import PRODUCT, attention_ref_and_bound, ratio  # noqa: F401  (ratio, PRODUCT: re-exported for the tests)

SCALE = 32 ** -0.5
MODES = ("f32", "f16x3", "f16")
SPLIT_MODES = ("f16x3", "f16")
FULL3D = (8, 7, 7)
FUSED_C = (96, 128, 192, 256)


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------
# Forms
# ---------------------------------------------------------------------------------------------------------------
FORMS = {
    "W1": "window_attn_kernel (VALU, 2-D)",
    "W2": "window_attn_mfma_kernel (fp32 MFMA, 2-D)",
    "W3": "window_attn3d_mfma_kernel<2,64,169,SINGLE> (2-D as a (1,7,7) window)",
    "W4": "window_attn3d_kernel (VALU, 3-D)",
    "W5": "window_attn3d_mfma_kernel<8,416,2535,SINGLE>",
    "W6": "swin_attn_fused_kernel<C,SINGLE>",
}


def window_form(entry, mode, dbg=1):
    """W1..W6: the kernel a call launches.  entry: "2d" (ops.window_attn), "3d" (ops.window_attn3d) or "fused" (ops.swin_attn_fused);
    mode: the arithmetic mode of the ops.arith context; dbg: the value last passed to tce_debug_window_attn_set_mfma (1 = default).

    A RESTATEMENT of the dispatch, not a query: the library has no entry that reports which kernel ran.  It mirrors
    tce_debug_window_attn_set_mfma (attn.hip: mfma = dbg != 0, split2d = dbg != 2), tce_window_attn_f32 (mfma && split2d && mode !=
    f32 -> the (1,7,7) form of the 3-D split kernel; else mfma -> the fp32 MFMA kernel; else the VALU kernel), tce_window_attn3d_f32
    (mfma && mode != f32 -> the split kernel; else the VALU kernel) and tce_swin_attn_fused_f32 (swinattn.hip: one kernel; it reads
    only tce_gemm_single_pass(), so mode f32 runs the three-product split arithmetic of f16x3).  If a dispatcher changes, this
    changes with it."""
    mfma, split2d = dbg != 0, dbg != 2
    if entry == "fused":
        return "W6"
    if entry == "2d":
        if mfma and split2d and mode != "f32":
            return "W3"
        return "W2" if mfma else "W1"
    if entry == "3d":
        return "W5" if (mfma and mode != "f32") else "W4"
    raise ValueError(entry)


# (form, entry, dbg, modes it is run in).  W1 / W4 under dbg = 0 ignore the mode (one run); W2 is what mode f32 runs, and what
# dbg = 2 runs in a split mode (the same kernel: the bit-identity claim of test_form_agreement)
FORM_RUNS = (
    ("W1", "2d", 0, ("f16x3",)),
    ("W2", "2d", 1, ("f32",)),
    ("W2", "2d", 2, ("f16x3",)),
    ("W3", "2d", 1, SPLIT_MODES),
    ("W4", "3d", 1, ("f32",)),
    ("W4", "3d", 0, ("f16x3",)),
    ("W5", "3d", 1, SPLIT_MODES),
    ("W6", "fused", 1, SPLIT_MODES),
)


# ---------------------------------------------------------------------------------------------------------------
# Geometry cases
# ---------------------------------------------------------------------------------------------------------------
# 2-D (T, H, W): each at shift 0 and shift 3
CASES_2D = (
    ((1, 7, 7), "one window"),
    ((1, 1, 1), "one real token in a padded window"),
    ((2, 5, 6), "both extents below the window, two frames"),
    ((1, 3, 25), "H <= shift: the rolled rows are all padding or all real"),
    ((1, 7, 15), "three windows: an odd count above one, for the two-window workgroups of W2 and W6"),
    ((1, 8, 15), "the last window row holds one real row"),
    ((3, 13, 10), "residues 6 and 3"),
    ((1, 14, 21), "exact multiples"),
)
# 3-D (T, H, W, shifted)
CASES_3D = (
    ((1, 3, 4, False), "N = 12: T = 1, one ragged key tile, seven of the eight waves idle"),
    ((1, 3, 4, True), "N = 12, shifted asked for and every dimension shrunken: no shift"),
    ((2, 2, 2, False), "N = 8"),
    ((2, 2, 2, True), "N = 8, shifted asked for"),
    ((8, 4, 4, False), "N = 128: an un-ragged last tile, unmasked"),
    ((16, 4, 4, True), "N = 128: an un-ragged last tile, masked (shift along D only)"),
    ((8, 7, 7, True), "N = 392: 12 tiles plus 8 keys; every dimension fits, so no shift"),
    ((4, 8, 6, True), "wd = 4, ww = 6: the [:N,:N] quirk with rows padded and shifted"),
    ((9, 7, 7, True), "temporal padding to 16, shift along D only"),
    ((17, 8, 6, True), "temporal padding to 24 and row padding to 14, ww = 6, shifts along D and H (the largest case)"),
    ((16, 14, 7, True), "exact multiples, shifts along D and H, the nominal window"),
)
# W6: each C at three 2-D cases, (1,7,15) and one with H < 7 among them
CASES_FUSED = {
    96: ((1, 7, 15), (2, 5, 6), (3, 13, 10)),
    128: ((1, 7, 15), (1, 3, 25), (1, 1, 1)),
    192: ((1, 7, 15), (2, 5, 6), (1, 8, 15)),
    256: ((1, 7, 15), (1, 3, 25), (1, 14, 21)),
}


def win3d(T, H, W, full_d, shift, shrink):
    """(window, shift, padded grid) of Win3D::make (attn_tile.h), restated: a dimension that fits in one nominal window shrinks the
    window to it and is never shifted (shrink: the video backbone; the 2-D entry pads instead)."""
    size, full, roll = (T, H, W), (full_d, 7, 7), ((full_d // 2 if shift else 0), shift, shift)
    win, sh, pad = [], [], []
    for i in range(3):
        fits = shrink and size[i] <= full[i]
        win.append(size[i] if fits else full[i])
        sh.append(0 if fits else roll[i])
        pad.append(cdiv(size[i], win[-1]) * win[-1])
    return tuple(win), tuple(sh), tuple(pad)


def key_tile_bodies(T, H, W, shifted, full_d=8, shrink=True):
    """The (MASKED, RAGGED) instantiations of key_tile that window_attn3d_mfma_kernel runs at this grid, restated from the kernel:
    NKP = N rounded up to 32; every tile but the last is (masked, False), the last (masked, NKP > N); masked = the window is the last
    one along a shifted dimension."""
    w, s, p = win3d(T, H, W, full_d, 3 if shifted else 0, shrink)
    N = w[0] * w[1] * w[2]
    nkt, ragged = cdiv(N, 32), cdiv(N, 32) * 32 > N
    bodies = set()
    for bd in range(p[0] // w[0]):
        for by in range(p[1] // w[1]):
            for bx in range(p[2] // w[2]):
                last = (bd == p[0] // w[0] - 1, by == p[1] // w[1] - 1, bx == p[2] // w[2] - 1)
                masked = any(s[i] > 0 and last[i] for i in range(3))
                if nkt > 1:
                    bodies.add((masked, False))
                bodies.add((masked, ragged))
    return bodies


def windows_2d(T, H, W):
    return T * cdiv(H, 7) * cdiv(W, 7)


def heads_2d(T, H, W):
    """One head where the window count is odd, so that W2's (window, head) items, two to a workgroup, come to an odd count too."""
    return 1 if windows_2d(T, H, W) % 2 else 2


# ---------------------------------------------------------------------------------------------------------------
# Windowing, built on the oracle's geometry functions (moved here from test_arith_bound_gpu.py)
# ---------------------------------------------------------------------------------------------------------------
def to_windows2d(g, T, H, W, shift, fill, sign=1):
    """[T*H*W, Cx] -> ([nW, 49, Cx] windows of the padded, shifted grid; pad positions hold `fill`), and the inverse map.
    sign = -1: the roll in the wrong direction (a planted defect)."""
    Cx = g.shape[-1]
    Hp, Wp = (H + 6) // 7 * 7, (W + 6) // 7 * 7
    grid = fill.to(g.dtype).expand(T, Hp, Wp, Cx).clone()
    grid[:, :H, :W] = g.view(T, H, W, Cx)
    if shift:
        grid = torch.roll(grid, shifts=(-sign * shift, -sign * shift), dims=(1, 2))
    win = grid.view(T, Hp // 7, 7, Wp // 7, 7, Cx).permute(0, 1, 3, 2, 4, 5).reshape(-1, 49, Cx)

    def back(y):
        C = y.shape[-1]
        y = y.view(T, Hp // 7, Wp // 7, 7, 7, C).permute(0, 1, 3, 2, 4, 5).reshape(T, Hp, Wp, C)
        if shift:
            y = torch.roll(y, shifts=(sign * shift, sign * shift), dims=(1, 2))
        return y[:, :H, :W].reshape(T * H * W, C)
    return win, back, (Hp, Wp)


def to_windows3d(g, T, H, W, shifted, fill, sign=1, force_sd=None):
    """[T*H*W, Cx] -> (windows [nW, N, Cx], back, mask [nW, N, N] or None, N) of the Video-Swin block: get_window_size_3d, padding
    with `fill`, roll, window_partition_3d, compute_mask_3d.  force_sd: a temporal shift applied whatever the window (a defect)."""
    from oracle import tce_oracle as O
    Cx = g.shape[-1]
    ws, ss = O.get_window_size_3d((T, H, W), FULL3D, tuple(i // 2 for i in FULL3D) if shifted else (0, 0, 0))
    if force_sd is not None and shifted:
        ss = (force_sd,) + tuple(ss[1:])
    Dp, Hp, Wp = (-(-n // w) * w for n, w in zip((T, H, W), ws))
    grid = fill.to(g.dtype).expand(1, Dp, Hp, Wp, Cx).clone()
    grid[0, :T, :H, :W] = g.view(T, H, W, Cx)
    mask = None
    rolled = any(i > 0 for i in ss)
    if rolled:
        grid = torch.roll(grid, shifts=(-sign * ss[0], -sign * ss[1], -sign * ss[2]), dims=(1, 2, 3))
        mask = O.compute_mask_3d(Dp, Hp, Wp, ws, ss)
    win = O.window_partition_3d(grid, ws)

    def back(y):
        y = O.window_reverse_3d(y, ws, 1, Dp, Hp, Wp)
        if rolled:
            y = torch.roll(y, shifts=(sign * ss[0], sign * ss[1], sign * ss[2]), dims=(1, 2, 3))
        return y[0, :T, :H, :W].reshape(T * H * W, y.shape[-1])
    return win, back, mask, win.shape[1]


def bias_2d(table, nh):
    from oracle import tce_oracle as O
    return table[O.rel_pos_index(7).view(-1)].view(49, 49, nh).permute(2, 0, 1)


def bias_3d(table, nh, N):
    """relative_position_index[:N, :N] of the NOMINAL window: the reference's quirk for a shrunken window."""
    from oracle import tce_oracle as O
    return table[O.rel_pos_index_3d(*FULL3D)[:N, :N].reshape(-1)].reshape(N, N, nh).permute(2, 0, 1)


def windows_ref_and_bound(qkv_w, nh, bias, mask, Bqkv=None, product=A.bound_split):
    """qkv_w [nW, N, 3C] (windows of q | k | v rows), bias [nh, N, N], mask [nWm, N, N] or None -> ([nW, N, C] ref, bound, S)."""
    nW, N, C3 = qkv_w.shape
    C = C3 // 3
    ref, B, S = (torch.zeros(nW, N, C, dtype=torch.float64) for _ in range(3))
    for w in range(nW):
        for h in range(nh):
            sl = [slice(j * C + 32 * h, j * C + 32 * h + 32) for j in range(3)]
            add = bias[h].double() + (mask[w % mask.shape[0]].double() if mask is not None else 0.0)
            eb = [Bqkv[w][:, s_] for s_ in sl] if Bqkv is not None else [None] * 3
            r, b, s_ = attention_ref_and_bound(qkv_w[w][:, sl[0]], qkv_w[w][:, sl[1]], qkv_w[w][:, sl[2]], 32 ** -0.5, add, *eb,
                                               product=product)
            ref[w][:, 32 * h:32 * h + 32], B[w][:, 32 * h:32 * h + 32], S[w][:, 32 * h:32 * h + 32] = r, b, s_
    return ref, B, S


class Layout:
    """What a case's windows hold, read off the oracle's windowing of an INDEX grid (no index arithmetic of the kernels restated):
    src [nW, N] the token row of window slot n or -1 (padded), reg [nW, N] a region label (the first slot of the same region under
    the shift mask), pos [ntok] the slot of a token in its window, win [ntok] its window."""

    def __init__(self, kind, T, H, W, shift):
        self.kind, self.T, self.H, self.W, self.shift = kind, T, H, W, shift
        self.ntok = T * H * W
        idx = torch.arange(self.ntok, dtype=torch.float64).view(-1, 1)
        fill = torch.full((1,), -1.0, dtype=torch.float64)
        if kind == "2d":
            from oracle import tce_oracle as O
            win, _, (Hp, Wp) = to_windows2d(idx, T, H, W, shift, fill)
            self.mask = O.shift_attn_mask(Hp, Wp, 7, 3) if shift else None
            self.N, self.NKP, self.rows = 49, 64, 169
        else:
            win, _, self.mask, self.N = to_windows3d(idx, T, H, W, bool(shift), fill)
            self.NKP, self.rows = cdiv(self.N, 32) * 32, 15 * 13 * 13
        self.src = win[..., 0].long()
        self.nW = self.src.shape[0]
        if self.mask is None:
            self.reg = torch.zeros_like(self.src)
        else:
            m = self.mask[torch.arange(self.nW) % self.mask.shape[0]]
            self.reg = (m == 0).float().argmax(-1)
        self.pos, self.win = torch.zeros(self.ntok, dtype=torch.long), torch.zeros(self.ntok, dtype=torch.long)
        real = self.src >= 0
        self.pos[self.src[real]] = torch.arange(self.N).expand(self.nW, self.N)[real]
        self.win[self.src[real]] = torch.arange(self.nW).view(-1, 1).expand(self.nW, self.N)[real]
        self.padded = bool((~real).any())
        self.two_regions = [w for w in range(self.nW) if len(set(self.reg[w][real[w]].tolist())) > 1]

    def windows(self, g, fill, **kw):
        if self.kind == "2d":
            win, back, _ = to_windows2d(g, self.T, self.H, self.W, self.shift, fill, **kw)
            return win, back
        win, back, _, _ = to_windows3d(g, self.T, self.H, self.W, bool(self.shift), fill, **kw)
        return win, back

    def bias(self, table, nh):
        return bias_2d(table, nh) if self.kind == "2d" else bias_3d(table, nh, self.N)


_LAYOUTS = {}


def layout(kind, T, H, W, shift):
    key = (kind, T, H, W, int(shift))
    if key not in _LAYOUTS:
        _LAYOUTS[key] = Layout(*key)
    return _LAYOUTS[key]


# ---------------------------------------------------------------------------------------------------------------
# Operand designs: (qkv [ntok, 3C], qkv_bias [3C], table [rows, nh]) fp32
# ---------------------------------------------------------------------------------------------------------------
DESIGNS = ("N", "G+", "G-", "R^", "Rv", "U")
CODED = ("G+", "G-")               # V's first channels carry the key's token row
CODE_BITS = 11                     # token rows < 2047; the padded tokens' V (the bias) carries 2047
# G-: 66, not 60: the planted "mask in base-2 units" defect (-69.3) must leave the masked key visible.  At a lead of 60 it would sit
# at e^-9.3 = 9e-5, below the split modes' bound on a score of this size (2^-20 * 60 per operand); at 66 it sits at e^-3.3 = 4 %,
# while the correct -100 keeps it at e^-34
LEAD = {"G+": 130.0, "G-": 66.0}
QCOEF = 8.0                        # the designed component of q; the key's is score / (QCOEF * SCALE)


def _code(idx):
    bits = (idx.view(-1, 1) >> torch.arange(CODE_BITS)) & 1
    return bits.float() * 2 - 1


def decode(row):
    """The token row whose V code dominates an output row [32] of a head (2047: a padded token)."""
    return int(((row[:CODE_BITS] > 0).long() << torch.arange(CODE_BITS)).sum())


def design_applies(design, lay):
    if design in LEAD:
        return len(lay.two_regions) > 0
    return True


# Where the designs run on the GPU: shifted cases with padding (both extents below the window; residues 6 and 3 over several
# windows), shrunken 3-D cases (rows padded and shifted; N = 128 masked along D, whose last window has two regions of REAL tokens),
# the largest case, the nominal window with shifts along D and H, and the nominal window's 13 unmasked key tiles for R^ / Rv.
# In (4,8,6) and (17,8,6) the second region of every shifted window holds padded tokens only, so G+ / G- do not apply there.
DESIGN_CASES = (("2d", 2, 5, 6, 3), ("2d", 3, 13, 10, 3), ("3d", 4, 8, 6, 1), ("3d", 16, 4, 4, 1), ("3d", 17, 8, 6, 1),
                ("3d", 16, 14, 7, 1), ("3d", 8, 7, 7, 1))


def design_runs():
    """(design, kind, T, H, W, shift) of every design other than N at every case of DESIGN_CASES where it applies."""
    return [(d,) + c for d in DESIGNS if d != "N" for c in DESIGN_CASES if design_applies(d, layout(*c))]


def design_coeffs(design, lay, nh, g):
    """a [ntok, nh, 2], b [ntok, nh, 2], table scale: the components of q rows and k rows along the two design directions; the
    designed part of the score of (query i, key j) is SCALE * (a_i . b_j), exact in the design."""
    a, b = torch.zeros(lay.ntok, nh, 2), torch.zeros(lay.ntok, nh, 2)
    if design in ("R^", "Rv"):
        top = 60.0 + 15.0 * torch.rand(lay.ntok, nh, generator=g)
        ramp = lay.pos.float() / max(lay.N - 1, 1)
        a[:, :, 0] = top / (QCOEF * SCALE)
        b[:, :, 0] = (QCOEF * (ramp if design == "R^" else 1 - ramp)).view(-1, 1)
        return a, b, 0.1      # a table of N(0,1) would undo the rise over the 8 keys of a nominal window's last tile
    if design in LEAD:
        # window with two regions: beacon 1 = the first real token (region r1), beacon 2 = the first real token of another region.
        # Queries of r1 look along direction 2, the others along direction 1: every real query's leader is a key it has masked.
        c = LEAD[design] / (QCOEF * SCALE)
        for w in lay.two_regions:
            real = torch.nonzero(lay.src[w] >= 0).flatten()
            n1 = int(real[0])
            r1 = int(lay.reg[w, n1])
            n2 = int(real[lay.reg[w][real] != r1][0])
            b[lay.src[w, n1], :, 0] = c
            b[lay.src[w, n2], :, 1] = c
            in_r1 = lay.reg[w][real] == r1
            a[lay.src[w][real[in_r1]], :, 1] = QCOEF
            a[lay.src[w][real[~in_r1]], :, 0] = QCOEF
        return a, b, 0.3
    raise ValueError(design)


def _directions(nh, g):
    u = torch.randn(nh, 2, 32, generator=g)
    u[:, 0] /= u[:, 0].norm(dim=-1, keepdim=True)
    u[:, 1] -= (u[:, 1] * u[:, 0]).sum(-1, keepdim=True) * u[:, 0]
    u[:, 1] /= u[:, 1].norm(dim=-1, keepdim=True)
    return u


def _off(t, u):
    """t [..., nh, 32] with its components along u[:, 0] and u[:, 1] removed."""
    for j in range(2):
        t = t - (t * u[:, j]).sum(-1, keepdim=True) * u[:, j]
    return t


def operands(design, lay, nh, seed=0):
    """N: qkv ~ N(0,1), bias ~ 0.3, table ~ N(0,1).
    G+ / G-: in every window with two regions one key of the OTHER region leads a query's best same-region key by ~130 / ~66
        (LEAD; 69 in the fused form).
    R^ / Rv: scores rise / fall with the key's slot in the window from 0 to 60..75 (by query).
    U: q = 0 (rows and bias), table = 0: every query is the mean of V over its same-region keys, padded ones included."""
    g = torch.Generator().manual_seed(int(seed) * 7919 + lay.ntok * 31 + lay.N + 1000 * DESIGNS.index(design))
    C = 32 * nh
    qkv, qb = torch.randn(lay.ntok, 3 * C, generator=g), 0.3 * torch.randn(3 * C, generator=g)
    table = torch.randn(lay.rows, nh, generator=g)
    if design == "U":
        qkv[:, :C], qb[:C] = 0.0, 0.0
        table = table * 0.0
    elif design != "N":
        u = _directions(nh, g)
        a, b, tscale = design_coeffs(design, lay, nh, g)
        q, k = _off(0.25 * qkv[:, :C].view(-1, nh, 32), u), _off(0.25 * qkv[:, C:2 * C].view(-1, nh, 32), u)
        q = q + a[..., 0:1] * u[:, 0] + a[..., 1:2] * u[:, 1]
        k = k + b[..., 0:1] * u[:, 0] + b[..., 1:2] * u[:, 1]
        qkv[:, :C], qkv[:, C:2 * C] = q.reshape(-1, C), k.reshape(-1, C)
        qb[:C] = _off(qb[:C].view(nh, 32), u).reshape(C)
        qb[C:2 * C] = _off(qb[C:2 * C].view(nh, 32), u).reshape(C)
        table = table * tscale
    if design in CODED:
        v = qkv[:, 2 * C:].view(-1, nh, 32)
        v[:, :, :CODE_BITS] = _code(torch.arange(lay.ntok)).view(-1, 1, CODE_BITS)
        qb[2 * C:].view(nh, 32)[:, :CODE_BITS] = 1.0
    return qkv.contiguous(), qb.contiguous(), table.contiguous()


# ---------------------------------------------------------------------------------------------------------------
# Reference and bound
# ---------------------------------------------------------------------------------------------------------------
def core_ref_and_bound(lay, qkv, qb, table, nh, mode):
    """The attention core on a given qkv tensor -> (ref, B, S) fp64 [ntok, C]; |out - ref| <= B element-wise, no margin.

    The base-2 softmax of window_attn3d_mfma_kernel needs no term of its own.  The model of attention_ref_and_bound charges every
    score 3 eps |s| + 2 eps |s - max| for the fp32 roundings of the scaled score, the added bias / mask, the subtraction of the
    maximum and the conversion to a base-2 exponent.  The base-2 kernel makes the
    conversion once per operand instead: scale * log2(e) is one constant (its rounding is a relative 2^-24 of the product, inside the
    product's bound), the table entry is rounded once more (eps |table| <= eps (|s| + |qk| + 100), and |qk| is charged by the product
    bound), and -144.2695 carries a relative 2^-24 of 100.  Each is a relative eps of a term whose magnitude the model already charges
    three times over.  tests/test_window_forms_cpu.py holds an fp32 base-2 emulation (emulate(base2=True)) to the unmodified bound."""
    win, back = lay.windows(qkv, qb)
    ref, B, S = windows_ref_and_bound(win, nh, lay.bias(table, nh), lay.mask, product=PRODUCT[mode])
    return back(ref), back(B), back(S)


def scores64(lay, qkv, qb, table, nh):
    """fp64 scores [nW, nh, N, N] without and with the mask (for the CPU test's claims about the designs)."""
    win, _ = lay.windows(qkv.double(), qb.double())
    C = 32 * nh
    q = win[..., :C].view(lay.nW, lay.N, nh, 32).permute(0, 2, 1, 3) * SCALE
    k = win[..., C:2 * C].view(lay.nW, lay.N, nh, 32).permute(0, 2, 1, 3)
    s = q @ k.transpose(-1, -2) + lay.bias(table.double(), nh)
    if lay.mask is None:
        return s, s
    return s, s + lay.mask[torch.arange(lay.nW) % lay.mask.shape[0]].double()[:, None]


FUSED_DESIGNS = ("N", "G+", "G-", "U")   # R^ / Rv are about a running maximum; the fused kernel's softmax holds all 49 scores in registers
FLAG = 5.0
CAMP = 0.5     # amplitude of the token-row code in x (channels 3 .. 3 + CODE_BITS of the coded designs)
# G- at 69: the fused bound is composed through LayerNorm and two projections, and the masked key must come closer to the planted
# -69.3 than in the cores to be seen through it (e^-0.3 against the correct e^-31)
LEAD_FUSED = {"G+": 130.0, "G-": 69.0}


def fused_operands(design, lay, C, seed=0):
    """x, norm1 (g1, b1), Wqkv, bqkv, table, Wproj, bproj for the fused half-block.  U: Wq = 0, bq = 0, table = 0.  G+ / G-: the
    beacons of design_coeffs through LayerNorm and the projection: channels 0, 1, 2 of x flag a token as beacon 1, beacon 2, query of
    region r1 (FLAG or 0; the other channels are scaled so that the row has mean 0 and variance 1), column 0 / 1 of Wk puts a flagged
    key on direction 1 / 2, and column 2 of Wq turns a query from direction 1 (the q bias) to direction 2.  The leads are those of
    the design to within the noise, which the CPU test measures in the fp64 scores.  The next CODE_BITS channels of x hold the
    token row as +-CAMP, and Wv / bv turn them into the first channels of every head's V: 3 or -1 by bit, 1 (row 2047) when padded."""
    nh = C // 32
    g = torch.Generator().manual_seed(int(seed) * 7919 + lay.ntok * 31 + C + 1000 * DESIGNS.index(design))
    x = torch.randn(lay.ntok, C, generator=g)
    g1, b1 = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    wqkv, bqkv = torch.randn(3 * C, C, generator=g) / math.sqrt(C), torch.randn(3 * C, generator=g) * 0.3
    table = torch.randn(169, nh, generator=g)
    wp, bp = torch.randn(C, C, generator=g) / math.sqrt(C), torch.randn(C, generator=g) * 0.2
    if design == "U":
        wqkv[:C], bqkv[:C] = 0.0, 0.0
        table = table * 0.0
    elif design in LEAD:
        u = _directions(nh, g)
        a, b, tscale = design_coeffs(design, lay, nh, g)
        flags = torch.stack([b[:, 0, 0] > 0, b[:, 0, 1] > 0, a[:, 0, 1] > 0], 1).double()
        fixed = torch.cat([flags * FLAG, _code(torch.arange(lay.ntok)).double() * CAMP], 1)
        nf = fixed.shape[1]
        # rows of mean 0 and variance 1 whose flag and code channels hold their values EXACTLY: norm1 (gamma 1, beta 0 there)
        # returns them as they are
        n = x[:, nf:].double()
        n = (n - n.mean(1, keepdim=True)) / n.std(1, unbiased=False, keepdim=True)
        beta = -fixed.sum(1, keepdim=True) / (C - nf)
        alpha = ((C - (fixed ** 2).sum(1, keepdim=True)) / (C - nf) - beta ** 2).sqrt()
        x = torch.cat([fixed, alpha * n + beta], 1).float()
        g1[:nf], b1[:nf] = 1.0, 0.0
        lit = FLAG
        wv = wqkv[2 * C:].view(nh, 32, C)
        wv[:, :CODE_BITS] = 0.0
        wv[:, torch.arange(CODE_BITS), 3 + torch.arange(CODE_BITS)] = 2.0 / CAMP
        bqkv[2 * C:].view(nh, 32)[:, :CODE_BITS] = 1.0
        wq, wk = (_off(0.25 * w.T.reshape(C, nh, 32), u) for w in (wqkv[:C], wqkv[C:2 * C]))   # [C in, nh, 32]: off both directions
        lead = LEAD_FUSED[design] / (QCOEF * SCALE)
        wk[0], wk[1] = (lead / lit) * u[:, 0], (lead / lit) * u[:, 1]
        wq[2] = (QCOEF / lit) * (u[:, 1] - u[:, 0])
        wqkv[:C], wqkv[C:2 * C] = wq.reshape(C, C).T, wk.reshape(C, C).T
        bqkv[:C] = (_off(bqkv[:C].view(nh, 32), u) + QCOEF * u[:, 0]).reshape(C)
        bqkv[C:2 * C] = _off(bqkv[C:2 * C].view(nh, 32), u).reshape(C)
        table = table * tscale
    elif design != "N":
        raise ValueError(f"the fused form has no design {design}")
    return tuple(t.contiguous() for t in (x, g1, b1, wqkv, bqkv, table, wp, bp))


def fused_qkv64(x, g1, b1, wqkv, bqkv):
    C = x.shape[1]
    return F.layer_norm(x.double(), (C,), g1.double(), b1.double(), 1e-5) @ wqkv.double().T + bqkv.double()


def fused_ref_and_bound(lay, x, g1, b1, wqkv, bqkv, table, wp, bp, mode):
    """x + proj(window_attention(LayerNorm(x))): LayerNorm evaluation -> qkv product -> attention (its operands off by the qkv
    product's bound) -> proj product -> bias and residual, composed to first order (x 2), exactly as
    test_arith_bound_gpu.py::test_swin_attn_fused; product: every matrix product's bound in `mode`."""
    C, nh, product = x.shape[1], x.shape[1] // 32, PRODUCT[mode]
    assert A.layernorm_sigma(x).min().item() > 1e-3
    y = F.layer_norm(x.double(), (C,), g1.double(), b1.double(), 1e-5)
    qkv = y @ wqkv.double().T + bqkv.double()
    Bqkv = product(y, wqkv, A.c_dense(C)) + A.chain(A.ln_eval_bound(x, g1, b1, 1e-5), wqkv) + A.bound_bias(qkv)
    win, back = lay.windows(qkv, bqkv.double())
    Bwin, _ = lay.windows(Bqkv, torch.zeros(3 * C, dtype=torch.float64))   # padding rows are the exact bias
    att, Batt, _ = windows_ref_and_bound(win, nh, bias_2d(table, nh), lay.mask, Bwin, product=product)
    att, Batt = back(att), back(Batt) / 2      # windows_ref_and_bound doubles; the factor 2 is applied once, at the end
    ref = x.double() + att @ wp.double().T + bp.double()
    B = 2 * (A.chain(Batt, wp) + product(att, wp, A.c_dense(C)) + 2 * A.bound_bias(ref))
    return ref, B, A.sum_abs(att, wp)


# ---------------------------------------------------------------------------------------------------------------
# Plain fp32 torch, and the same with one planted defect
# ---------------------------------------------------------------------------------------------------------------
DEFECTS = ("mask_inf", "mask_base2_units", "drop_padded_keys", "ragged_kept", "region_off_by_one", "bias_shrunken_coords",
           "bias_swapped", "roll_reversed", "temporal_shift_on_shrunken_d",
           # beyond the issue's nine: what only R^, Rv and U can see (softmax is shift-invariant, so a stale maximum is exact
           # until a probability leaves the fp16 range of the P fragments; N(0,1) scores are never exactly zero)
           "max_frozen_first_tile", "max_from_last_tile", "zero_score_is_absent")
ONLY_3D = ("bias_shrunken_coords", "temporal_shift_on_shrunken_d")


def _bias_shrunken(lay, table, nh):
    """The index a kernel WITHOUT the [:N,:N] quirk would use: true (d, y, x) offsets inside the shrunken window."""
    w, _, _ = win3d(lay.T, lay.H, lay.W, 8, 3 if lay.shift else 0, True)
    n = torch.arange(lay.N)
    c = torch.stack([n // (w[1] * w[2]), (n // w[2]) % w[1], n % w[2]])
    rel = c[:, :, None] - c[:, None, :]
    idx = ((rel[0] + 7) * 13 + (rel[1] + 6)) * 13 + (rel[2] + 6)
    return table[idx.reshape(-1)].reshape(lay.N, lay.N, nh).permute(2, 0, 1)


def core_f32(win, bias, mask, pad, nh, defect=None, extra=None, base2=False):
    """win [nW, N, 3C] fp32 -> [nW, N, C]: scores, + bias, + mask, softmax, @ v, all in fp32.  pad [nW, N]: padded slots.
    extra = (count, score [nh]): that many more key slots with zero V (ragged_kept).  base2: the 3-D split kernel's arithmetic
    order (scale and table pre-multiplied by log2(e), mask -144.2695, exp2)."""
    nW, N, C3 = win.shape
    C = C3 // 3
    L2E = 1.4426950408889634
    q = win[..., :C].view(nW, N, nh, 32).permute(0, 2, 1, 3)
    k = win[..., C:2 * C].view(nW, N, nh, 32).permute(0, 2, 1, 3)
    v = win[..., 2 * C:].view(nW, N, nh, 32).permute(0, 2, 1, 3)
    if defect == "bias_swapped":
        bias = bias.transpose(-1, -2)
    if base2:
        s = (q * torch.tensor(SCALE * L2E, dtype=torch.float32)) @ k.transpose(-1, -2) + bias * torch.tensor(L2E, dtype=torch.float32)
        mval = -144.26950408889634
    else:
        s = (q * SCALE) @ k.transpose(-1, -2) + bias
        mval = -100.0
    if mask is not None:
        m = mask[torch.arange(nW) % mask.shape[0]][:, None] != 0
        if defect == "mask_inf":
            mval = float("-inf")
        elif defect == "mask_base2_units":
            mval = mval * math.log(2.0)
        s = s + m.float() * mval if math.isfinite(mval) else s.masked_fill(m, mval)
    if defect == "drop_padded_keys":
        s = s.masked_fill(pad[:, None, None, :], float("-inf"))
    if extra is not None:
        cnt, sc = extra
        s = torch.cat([s, (sc * (L2E if base2 else 1.0)).view(1, nh, 1, 1).expand(nW, nh, N, cnt)], -1)
        v = torch.cat([v, torch.zeros(nW, nh, cnt, 32)], 2)
    if defect == "zero_score_is_absent":      # a ragged slot recognised by its zero K row's score instead of by its index
        s = s.masked_fill(s == 0, float("-inf"))
    if defect in ("max_frozen_first_tile", "max_from_last_tile"):   # probabilities against a stale maximum, through fp16 (<= 65504)
        t = s[..., :32] if defect == "max_frozen_first_tile" else s[..., (cdiv(s.shape[-1], 32) - 1) * 32:]
        e = torch.exp(s - t.amax(-1, keepdim=True)).clamp(max=65504.0)
        p = e / e.sum(-1, keepdim=True)
    elif base2:
        e = torch.exp2(s - s.amax(-1, keepdim=True))
        p = e / e.sum(-1, keepdim=True)
    else:
        p = torch.softmax(s, -1)
    return (p.nan_to_num(nan=0.0) @ v).permute(0, 2, 1, 3).reshape(nW, N, C)


def emulate(lay, qkv, qb, table, nh, defect=None, base2=False):
    """The attention core in fp32 torch on the oracle's windowing -> [ntok, C]; defect: one of DEFECTS (None: the correct op)."""
    from oracle import tce_oracle as O
    kw = {}
    if lay.kind == "2d" and defect in ONLY_3D:
        defect = None
    if defect == "roll_reversed":
        kw["sign"] = -1
    if defect == "temporal_shift_on_shrunken_d":
        kw["force_sd"] = 4
    mask = lay.mask
    if lay.kind == "2d":
        win, back, (Hp, Wp) = to_windows2d(qkv, lay.T, lay.H, lay.W, lay.shift, qb, **kw)
        if defect == "region_off_by_one" and lay.shift:
            mask = O.shift_attn_mask(Hp, Wp, 7, 4)       # the inner boundary at Hp - shift - 1
    else:
        win, back, mask, _ = to_windows3d(qkv, lay.T, lay.H, lay.W, bool(lay.shift), qb, **kw)
        if defect == "region_off_by_one" and mask is not None:
            ws, ss = O.get_window_size_3d((lay.T, lay.H, lay.W), FULL3D, (4, 3, 3))
            Dp, Hp, Wp = (cdiv(n, w) * w for n, w in zip((lay.T, lay.H, lay.W), ws))
            mask = O.compute_mask_3d(Dp, Hp, Wp, ws, tuple(s + 1 if s > 0 else 0 for s in ss))
    bias = lay.bias(table, nh)
    if defect == "bias_shrunken_coords" and lay.kind == "3d":
        bias = _bias_shrunken(lay, table, nh)
    idx = torch.arange(lay.ntok, dtype=torch.float32).view(-1, 1)
    pad = (lay.windows(idx, torch.full((1,), -1.0), **kw)[0][..., 0] < 0)
    extra = (lay.NKP - lay.N, table[0]) if (defect == "ragged_kept" and lay.NKP > lay.N) else None
    return back(core_f32(win, bias, mask, pad, nh, defect, extra, base2))


def fused_f32(lay, x, g1, b1, wqkv, bqkv, table, wp, bp, defect=None):
    """The fused half-block in fp32 torch; defect: planted in its attention core."""
    C, nh = x.shape[1], x.shape[1] // 32
    qkv = F.layer_norm(x, (C,), g1, b1, 1e-5) @ wqkv.T + bqkv
    return x + emulate(lay, qkv, bqkv, table, nh, defect) @ wp.T + bp


def fused_attention_of(out, x, wp, bp):
    """The attention rows behind an output of the fused half-block, (out - x - bproj) Wproj^-T in fp64: where decode() reads the key."""
    return torch.linalg.solve(wp.double(), (out.double() - x.double() - bp.double()).T).T
