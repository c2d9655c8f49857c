"""Everything wrapped around the product of tce_gemm_f32 / tce_gemm_splitk_f32 -- the A + A2 prologue, the tile epilogues of
csrc/gemm_epilogue.h, epi_fix_kernel, splitk_reduce_kernel and the two LayerNorm reduce kernels (csrc/gemm.hip) -- as designs, fp64
references, bounds and a matrix-level model with deliberate defects.  Pure torch on the CPU; imports nothing that needs a GPU.

Exact-product design: a, a2 in {-8..8} * 2^-3 and w in {-8..8} * 2^-s.  Every value and a + a2 is exact in fp16 (lo halves zero), every
partial sum is an integer below 2^24 times 2^-(3+s), so (a + a2) W^T is exact in modes f32, f16x3 and f16, in any summation order, on
every tile and at every split count: the wrapper's arithmetic is all the error there is.  Without GELU / LayerNorm every step of the
wrapper is ONE correctly rounded fp32 operation in a documented order (gemm_epilogue.h: x + bias, activation, + res or * res, trailing
ReLU), so the expectation is the same chain in float32 on the CPU and the comparison is bit equality.

Dense design: _arith.dense_operands at scale (1, 1), the wrapper composed to first order (x 2 for the remainder) like
test_arith_bound_gpu.test_rowlin_tails.

A Case is one launch; tests/test_gemm_epilogue_gpu.py holds the table of them, and tests/test_gemm_epilogue_cpu.py reads that table."""
import functools
import math
import zlib
from dataclasses import dataclass, replace  # noqa: F401  (replace: for the case tables)

import torch

import _arith as A

F32, F64 = torch.float32, torch.float64
ACT_NONE, ACT_RELU, ACT_GELU, ACT_RELU_AFTER_RES = 0, 1, 2, 3
RES_NONE, RES_ADD, RES_MUL = 0, 1, 2
COMBOS = tuple((a, r) for a in range(4) for r in range(3))
# gemm_epilogue.h TCE_EPI_DISPATCH / tce_epi_supported: the bodies a tile epilogue is specialised on
FUSED = ((0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (2, 0), (3, 1))
# gemm.hip tce_gemm_f32: act 3 without a residual is rewritten to act 1; the other four run the GEMM with the activation (act 3: none)
# and then epi_fix_kernel for the residual (and act 3's ReLU)
REWRITTEN = (3, 0)
FOLDED = ((1, 2), (2, 1), (2, 2), (3, 2))
TILE_BM = {6464: 64, 6465: 64, 12864: 128, 128128: 128, 256128: 256}
TILE_BN = {6464: 64, 6465: 64, 12864: 64, 128128: 128, 256128: 128}
PAD = 8            # floats of NaN in front of and behind every output / bias / residual extent (keeps 16-byte alignment)
LN_EPS = 1e-5
RANGE_LIMIT = 60000.0   # csrc/common.h TCE_RANGE_LIMIT


@dataclass(frozen=True)
class Case:
    group: str                 # which part of the GPU module runs it
    mode: str = "f16x3"        # arithmetic: f32 / f16x3 / f16
    tile: int = 0              # tce_gemm_force_tile (0 = the launcher's choice)
    epi: int = 1               # tce_debug_set_epilogue: 1 = LDS-staged (256128 tile only), 0 = direct stores
    M: int = 1
    N: int = 4
    K: int = 32
    a2: bool = False
    act: int = 0
    res_mode: int = 0
    batch: int = 1
    ldc: int = 0               # 0 = N
    ldres: int = 0             # 0 = N
    c_off: int = 0             # floats the C / bias / residual base is moved off its 16-byte aligned place
    b_off: int = 0
    r_off: int = 0
    inplace: bool = False      # res aliases C
    bias_pb: bool = False      # per-batch bias (sBias = N)
    res_shared: bool = False   # sRes = 0
    a2_shared: bool = False    # sA2 = 0
    gap: int = 0               # floats between one batch entry's C (and residual) extent and the next
    splits: int = 0            # 0 = tce_gemm_f32; >= 1 = the split-K entries (GEMM into planes, then a reduce kernel)
    ln: bool = False           # LayerNorm folded into the reduce
    conv: tuple = None         # (T, H, W, Cin, k, stride, pad): implicit-GEMM convolution, M / K follow
    handmade: bool = False     # tce_splitk_reduce_f32 alone on hand-made partial planes
    design: str = "exact"      # exact / dense

    @property
    def combo(self):
        return (self.act, self.res_mode)

    @property
    def path(self):
        """Which kernel applies the epilogue: "tile" (fused in the GEMM), "fix" (GEMM + epi_fix_kernel), "reduce", "ln"."""
        if self.ln:
            return "ln"
        if self.splits or self.handmade:
            return "reduce"
        return "tile" if (self.combo in FUSED or self.combo == REWRITTEN) else "fix"

    @property
    def form(self):
        """Store form of the tile epilogue: "lds" (tce_epi_store_lds) on the 8-wave tile unless switched off, else "direct"."""
        return "lds" if (self.mode != "f32" and self.tile == 256128 and self.epi == 1) else "direct"

    @property
    def instance(self):
        inst = f"mode {self.mode}"
        if self.handmade:
            return "tce_splitk_reduce_f32" + (" LayerNorm" if self.ln else "")
        if self.conv:
            inst += " conv"
        inst += f" tile {self.tile or 'auto'}"
        if self.tile == 256128 and self.mode != "f32":
            inst += " lds" if self.epi else " direct"
        if self.a2:
            inst += " +a2"
        if self.splits:
            inst += f" split-K {self.splits}" + (" LayerNorm" if self.ln else "")
        return inst

    @property
    def shape(self):
        s = f"{self.batch}x" if self.batch > 1 else ""
        if self.conv:
            T, H, W, Cin, k, st, p = self.conv
            return f"{T}x{H}x{W} {Cin}->{self.N} {k}x{k}/s{st}"
        return s + f"{self.M}x{self.N}x{self.K}"

    @property
    def variant(self):
        L = layout(self)
        v = []
        if L.ldc != self.N:
            v.append(f"ldc {L.ldc}")
        if self.res_mode and L.ldres != self.N and not self.inplace:
            v.append(f"ldres {L.ldres}")
        for name, off in (("C", self.c_off), ("bias", self.b_off), ("res", self.r_off)):
            if off:
                v.append(f"{name} +{4 * off} B")
        for flag, name in ((self.inplace, "in place"), (self.bias_pb, "per-batch bias"), (self.res_shared, "shared res"),
                           (self.a2_shared, "shared a2")):
            if flag:
                v.append(name)
        if self.gap:
            v.append(f"sC gap {self.gap}")
        if self.design != "exact":
            v.append(self.design)
        return ", ".join(v) or "aligned"

    @property
    def label(self):
        return f"{self.instance} | {self.shape} | act {self.act} res {self.res_mode} | {self.variant}"


def conv_case(**kw):
    T, H, W, Cin, k, st, p = kw["conv"]
    Ho, Wo = (H + 2 * p - k) // st + 1, (W + 2 * p - k) // st + 1
    return Case(M=T * Ho * Wo, K=k * k * Cin, **kw)


@dataclass(frozen=True)
class Layout:
    ldc: int
    ldres: int
    sC: int
    sRes: int
    sBias: int
    c_base: int
    r_base: int
    b_base: int
    c_size: int
    r_size: int
    b_size: int


def layout(c):
    """Where the outputs, the residual and the bias lie inside their NaN-filled buffers (all in floats)."""
    ldc = c.ldc or c.N
    ldres = ldc if c.inplace else (c.ldres or c.N)
    sC = c.M * ldc + c.gap if c.batch > 1 else 0
    sRes = sC if c.inplace else (0 if (c.res_shared or c.batch == 1) else c.M * ldres + c.gap)
    sBias = c.N if c.bias_pb else 0
    c_base, b_base = PAD + c.c_off, PAD + c.b_off
    r_base = c_base if c.inplace else PAD + c.r_off
    c_size = c_base + (c.batch - 1) * sC + c.M * ldc + PAD
    r_size = r_base + (0 if sRes == 0 else (c.batch - 1) * sRes) + c.M * ldres + PAD
    b_size = b_base + (c.batch - 1) * sBias + c.N + PAD
    return Layout(ldc, ldres, sC, sRes, sBias, c_base, r_base, b_base, c_size, r_size, b_size)


def out_index(c):
    """Flat positions of out[b, m, n] inside the C buffer, [batch, M, N]."""
    L = layout(c)
    b, m, n = torch.arange(c.batch)[:, None, None], torch.arange(c.M)[None, :, None], torch.arange(c.N)[None, None, :]
    return L.c_base + b * L.sC + m * L.ldc + n


def res_index(c, ld=None, batch0=False, row_cap=None):
    L = layout(c)
    b, m, n = torch.arange(c.batch)[:, None, None], torch.arange(c.M)[None, :, None], torch.arange(c.N)[None, None, :]
    if batch0:
        b = b * 0
    if row_cap is not None:
        m = m.clamp(max=row_cap)
    return L.r_base + b * L.sRes + m * (L.ldres if ld is None else ld) + n


# ---------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------
def exact_shift(K):
    """s of w = {-8..8} * 2^-s: a + a2 has variance 2 * 24 / 64 and w 24 * 4^-s, so the product's is 18 K 4^-s; s makes it <= 1 and
    keeps the GELU arguments (product + a bias of deviation 0.3) inside +-6 with room."""
    return max(0, math.ceil(math.log(18.0 * K, 4.0)))


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


def _ints(g, shape, scale):
    return torch.randint(-8, 9, shape, generator=g).to(F32) * scale


@dataclass
class Operands:
    a: torch.Tensor = None       # [batch, M, K]  (conv: the image [T*H*W, Cin])
    a2: torch.Tensor = None      # [batch or 1, M, K]
    w: torch.Tensor = None       # [N, K]
    planes: torch.Tensor = None  # hand-made [splits, M, N]
    asum: torch.Tensor = None    # fp64 [batch, M, K]: a + a2 (conv: the im2col rows)
    x64: torch.Tensor = None     # fp64 [batch, M, N]: the product
    bias: torch.Tensor = None    # [batch or 1, N]
    res: torch.Tensor = None     # [batch or 1, M, N]
    gamma: torch.Tensor = None
    beta: torch.Tensor = None
    shift: int = 0


@functools.lru_cache(maxsize=64)
def _product_operands(design, M, N, K, batch, a2, a2_shared, conv, handmade, splits):
    """The product's operands and its fp64 value: shared by every case of one (shape, design) -- computed once, never changed."""
    g = torch.Generator().manual_seed(_seed("product", design, M, N, K, batch, a2, a2_shared, conv, handmade, splits))
    o = Operands()
    if handmade:    # partial planes whose sums are exact in any order: {-64..64} * 2^-6
        o.planes = torch.randint(-64, 65, (splits, M, N), generator=g).to(F32) / 64
        o.x64 = o.planes.double().sum(0)[None]
        return o
    if design == "exact":
        o.shift = exact_shift(K)
        if conv:
            T, H, W, Cin, k, st, p = conv
            o.a = _ints(g, (T * H * W, Cin), 0.125)
            o.w = _ints(g, (N, K), 2.0 ** -o.shift)
            o.asum = A.im2col(o.a, T, H, W, Cin, k, st, p).double()[None]
        else:
            o.a = _ints(g, (batch, M, K), 0.125)
            o.w = _ints(g, (N, K), 2.0 ** -o.shift)
            o.asum = o.a.double()
            if a2:
                o.a2 = _ints(g, (1 if a2_shared else batch, M, K), 0.125)
                o.asum = o.asum + o.a2.double()
    else:
        assert not conv
        a, o.w = A.dense_operands(batch * M, N, K, 1.0, 1.0, _seed("dense", M, N, K))
        o.a = a.view(batch, M, K)
        o.asum = o.a.double()
        if a2:
            o.a2 = torch.randn(1 if a2_shared else batch, M, K, generator=g) * 0.25   # keeps the GELU arguments inside +-6
            o.asum = o.asum + o.a2.double()
    o.x64 = o.asum @ o.w.double().T
    return o


def operands(c):
    """CPU tensors of a case.  The product part is cached per shape; bias / residual / LayerNorm weights are random fp32 values,
    distinct per element, so that a wrong row, column or batch index is visible."""
    p = _product_operands(c.design, c.M, c.N, c.K, c.batch, c.a2, c.a2_shared, c.conv, c.handmade, c.splits if c.handmade else 0)
    g = torch.Generator().manual_seed(_seed("wrap", c.M, c.N, c.batch, c.bias_pb, c.res_shared))
    o = replace(p)
    o.bias = torch.randn(c.batch if c.bias_pb else 1, c.N, generator=g) * 0.3
    o.res = torch.randn(1 if (c.res_shared or c.batch == 1) else c.batch, c.M, c.N, generator=g)
    o.gamma, o.beta = torch.rand(c.N, generator=g) + 0.5, torch.randn(c.N, generator=g) * 0.2
    return o


def plane(c, o, s):
    """fp64 partial plane s of a split-K case (exact design: exact in fp32 too)."""
    if c.handmade:
        return o.planes[s].double()[None]
    kc = c.K // c.splits
    return o.asum[..., s * kc:(s + 1) * kc] @ o.w.double()[:, s * kc:(s + 1) * kc].T


def buffers(c, o):
    """(C buffer, residual buffer or None, bias buffer): NaN everywhere except the values a correct launch may read.  In place the
    residual lies in the C buffer."""
    L = layout(c)
    nan = float("nan")
    cbuf, bbuf = torch.full((L.c_size,), nan), torch.full((L.b_size,), nan)
    for b in range(o.bias.shape[0]):
        bbuf[L.b_base + b * L.sBias:L.b_base + b * L.sBias + c.N] = o.bias[b]
    rbuf = None
    if c.res_mode:
        if c.inplace:
            cbuf[out_index(c)] = o.res.expand(c.batch, c.M, c.N)
        else:
            rbuf = torch.full((L.r_size,), nan)
            nb = 1 if L.sRes == 0 else c.batch
            rbuf[res_index(c)[:nb]] = o.res[:nb]
    return cbuf, rbuf, bbuf


# ---------------------------------------------------------------------------------------------------------------------
# the matrix-level model
# ---------------------------------------------------------------------------------------------------------------------
def vec_ok(c, b):
    """tce_epi_vec_ok for batch entry b (gemm_epilogue.h:174-179); every buffer starts 16-byte aligned."""
    L = layout(c)
    ok = L.ldc % 4 == 0 and (L.c_base + b * L.sC) % 4 == 0 and (L.b_base + b * L.sBias) % 4 == 0
    if c.path == "tile" and c.res_mode:
        ok = ok and L.ldres % 4 == 0 and (L.r_base + b * L.sRes) % 4 == 0
    return ok


def scalar_cols(c, b):
    """[N] bool: the columns a tile epilogue stores through its scalar tail path.  Direct form (tce_epi_store_t): a lane's column base
    is n0 = 32 j + 4 (lane >> 5) and it stores float4s when vec_ok && n0 + 27 < N (gemm_epilogue.h:60); LDS form: 4 columns per lane,
    float4 when vec_ok && n + 3 < N (gemm_epilogue.h:125)."""
    n = torch.arange(c.N)
    if not vec_ok(c, b):
        return torch.ones(c.N, dtype=torch.bool)
    if c.form == "lds":
        return (n // 4) * 4 + 3 >= c.N
    return (n // 32) * 32 + 4 * ((n % 32) // 4 % 2) + 27 >= c.N


def hi_halfwave_cols(c):
    """Columns owned by lanes with lane >> 5 == 1 in the direct form."""
    n = torch.arange(c.N)
    return (n % 32) // 4 % 2 == 1


def gelu_tanh(z):
    return 0.5 * z * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (z + 0.044715 * z ** 3)))


# name -> what the planted defect is (the kinds of mistake this code can actually have)
DEFECTS = {
    "bias_dropped_on_tail": "bias dropped on the scalar-tail columns only",
    "bias_col_minus_4_hi_halfwave": "bias taken from column n - 4 on the half-wave with lane >> 5 == 1 (direct stores)",
    "res_row_clamped_early": "residual row clamped to M - 1 one row early",
    "res_pitch_ldc": "residual read with ldc in place of ldres",
    "act_after_res": "activation applied after the residual where it belongs before it",
    "relu3_before_res": "the trailing ReLU of act = 3 applied before the residual",
    "fix_res_batch0": "epi_fix using batch 0's residual for every batch",
    "sbias_ignored": "per-batch bias ignored (sBias treated as 0)",
    "fix_mul_as_add": "RES_MUL executed as RES_ADD on the folded path",
    "ln_plane_skipped": "one partial plane skipped when splits % 4 == 1 in the LayerNorm reduce (the wave-per-row kernel)",
    "gelu_tanh": "GELU replaced by its tanh approximation",
}


def model(c, o, defect=None):
    """What the launch stores, [batch, M, N], from the exact product, the bias / residual BUFFERS and the pitches.

    Without GELU / LayerNorm: float32, every step one fp32 operation in the kernels' order -- the bit-exact expectation.
    With GELU: the argument x + bias in float32 (one correctly rounded operation, as on the device), GELU and what follows in fp64.
    With LayerNorm: fp64 throughout (z = x + bias + res, then the LayerNorm), as test_gemm_splitk_layernorm_reduce composes it.
    The dense design is fp64 throughout."""
    assert defect is None or defect in DEFECTS
    L = layout(c)
    act, res_mode = c.act, c.res_mode
    exact = c.design == "exact"
    x = o.x64
    if defect == "ln_plane_skipped" and c.path == "ln" and c.M > 256 and c.splits % 4 == 1 and c.splits > 1:
        x = x - plane(c, o, c.splits - 1)
    x = x.expand(c.batch, c.M, c.N)
    x = x.to(F32) if (exact and not c.ln) else x
    dt = x.dtype
    _, rbuf, bbuf = buffers(c, o)
    # bias, [batch, 1 or M, N]
    tile = c.path in ("tile", "fix")
    bm = torch.stack([bbuf[L.b_base + (0 if defect == "sbias_ignored" else b) * L.sBias:][:c.N] for b in range(c.batch)])[:, None, :]
    if tile and defect == "bias_dropped_on_tail":
        bm = torch.where(torch.stack([scalar_cols(c, b) for b in range(c.batch)])[:, None, :], torch.zeros_like(bm), bm)
    if tile and defect == "bias_col_minus_4_hi_halfwave" and c.form == "direct":
        shifted = torch.stack([bbuf[L.b_base + b * L.sBias - 4:][:c.N] for b in range(c.batch)])[:, None, :].nan_to_num(0.0)
        bm = torch.where(hi_halfwave_cols(c)[None, None, :], shifted, bm)
    bm = bm.to(dt)
    # residual, [batch, M, N]
    rm = None
    if res_mode:
        src = buffers(c, o)[0] if c.inplace else rbuf
        idx = res_index(c, ld=L.ldc if defect == "res_pitch_ldc" else None, batch0=(defect == "fix_res_batch0" and c.path == "fix"),
                        row_cap=c.M - 2 if (defect == "res_row_clamped_early" and c.M > 1) else None)
        rm = src[idx.clamp(max=src.numel() - 1)].to(dt)
    if defect == "fix_mul_as_add" and c.path == "fix" and res_mode == RES_MUL:
        res_mode = RES_ADD
    if c.ln:
        z = x + bm
        if res_mode:
            z = z + rm
        return torch.nn.functional.layer_norm(z, (c.N,), o.gamma.double(), o.beta.double(), LN_EPS)

    def activation(v):
        if act == ACT_RELU:
            return torch.relu(v)
        if act == ACT_GELU:
            v = v.double()
            return gelu_tanh(v) if defect == "gelu_tanh" else torch.nn.functional.gelu(v)
        return v

    def residual(v):
        if res_mode == RES_ADD:
            return v + rm.to(v.dtype)
        if res_mode == RES_MUL:
            return v * rm.to(v.dtype)
        return v

    v = x + bm
    if defect == "act_after_res" and res_mode and act in (ACT_RELU, ACT_GELU):
        v = activation(residual(v))
    elif defect == "relu3_before_res" and act == ACT_RELU_AFTER_RES and res_mode:
        v = residual(torch.relu(v))
    else:
        v = residual(activation(v))
        if act == ACT_RELU_AFTER_RES:
            v = torch.relu(v)
    return v


def bit_exact(c):
    return c.design == "exact" and c.act != ACT_GELU and not c.ln


def product_bound(c, o):
    """[batch, M, N]: the dense design's product term and, with an addend, the fp32 rounding of a + a2 (gemm.hip:106 /
    gemm_f16x3_kernel.h:185) chained through |w|."""
    B = []
    for b in range(c.batch):
        a, w = o.asum[b], o.w
        P = {"f32": lambda: A.bound_f32(a, w), "f16": lambda: A.bound_f16(a, w, A.c_dense(c.K)),
             "f16x3": lambda: A.bound_split(a, w, A.c_dense(c.K) + max(c.splits, 0))}[c.mode]()
        if c.a2:
            P = P + A.chain(A.EPS_F32 * a.abs(), w)
        B.append(P)
    return torch.stack(B)


def ln_input_bound(c, o):
    """LayerNorm reduce kernels (gemm.hip:421-422 and 484-485): `a += bias` rounds x + bias, `a += res` rounds the sum."""
    x = o.x64.expand(c.batch, c.M, c.N)
    zb = x + o.bias.double()[:, None, :]
    Bz = A.bound_bias(zb)
    if c.res_mode:
        Bz = Bz + A.bound_bias(zb + o.res.double())
    return zb + (o.res.double() if c.res_mode else 0.0), Bz


def reference(c, o):
    """(ref, B): B is None for a bit-exact case (ref is float32 then), else the fp64 per-element bound."""
    ref = model(c, o)
    if bit_exact(c):
        assert ref.dtype == F32
        return ref, None
    exact = c.design == "exact"
    Bx = torch.zeros_like(o.x64.expand(c.batch, c.M, c.N)) if exact else product_bound(c, o)
    if c.ln:
        z, Bz = ln_input_bound(c, o)
        return ref, 2 * A.ln_tail(z, Bx + Bz, o.gamma, o.beta, LN_EPS)
    x = o.x64.expand(c.batch, c.M, c.N)
    z = x + o.bias.double()[:, None, :]
    # exact design: the GELU argument is the correctly rounded fp32 sum on both sides -- no bias term
    Bz = Bx if exact else Bx + A.bound_bias(z)
    if c.act == ACT_GELU:
        zz = (x.to(F32) + o.bias[:, None, :]).double() if exact else z
        Bv = (0.0 if exact else A.GELU_LIPSCHITZ * Bz) + A.gelu_eval_bound(zz)
    else:
        Bv = Bz
    if c.res_mode:
        r = o.res.double().expand(c.batch, c.M, c.N)
        Bv = (Bv * r.abs() if c.res_mode == RES_MUL else Bv) + A.bound_bias(ref)
    return ref, (Bv if exact else 2 * Bv)


def compare(c, out, ref, B):
    """("exact", 0.0) or ("bound", worst err / B); raises with the place of the worst element."""
    out = out.reshape(ref.shape)
    if B is None:
        if torch.equal(out, ref):
            return "exact", 0.0
        bad = torch.nonzero(~((out == ref) | (out.isnan() & ref.isnan())))
        b, m, n = bad[0].tolist()
        raise AssertionError(f"{c.label}: {bad.shape[0]} of {ref.numel()} elements differ from the fp32 chain; first at batch {b}, row {m}, "
                             f"column {n}: got {float(out[b, m, n])!r}, expected {float(ref[b, m, n])!r}")
    r, i = worst_ratio(out, ref, B)
    if r > 1.0:
        n = i % c.N
        m = i // c.N % c.M
        raise AssertionError(f"{c.label}: worst err/B = {r:.3g} at batch {i // (c.M * c.N)}, row {m}, column {n} "
                             f"(got {float(out.flatten()[i])!r}, ref {float(ref.flatten()[i])!r})")
    return "bound", r


def worst_ratio(out, ref, B):
    err = (out.double() - ref.double()).abs().nan_to_num(nan=float("inf"))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / B)
    i = int(ratio.argmax())
    return float(ratio.flatten()[i]), i


def defect_shows(c, o, defect):
    """True when the planted defect breaks bit equality, or is at least 4 x outside the bound, on this case."""
    ref, B = reference(c, o)
    bad = model(c, o, defect)
    if B is None:
        return not torch.equal(bad, ref)
    return worst_ratio(bad, ref, B)[0] >= 4.0


# ---------------------------------------------------------------------------------------------------------------------
# the range-guard probe
# ---------------------------------------------------------------------------------------------------------------------
def range_probe():
    """256128 tile, LDS-staged epilogue, M % 32 != 0, RES_MUL.  Column 0 of a and w makes every product -300 + O(1) (exact), the bias
    is +300, so every stored value is O(1) * res; the last valid row's residual is 300.  A row >= M of the last 32-row fragment has a
    zero accumulator, so tce_epi_store_lds evaluates (0 + 300) * 300 = 90000 >= TCE_RANGE_LIMIT there -- a value that is never stored."""
    M, N, K = 256 + 35, 128 + 29, 32
    c = Case("probe", tile=256128, epi=1, M=M, N=N, K=K, act=0, res_mode=RES_MUL, ldc=160, ldres=160)
    o = operands(c)
    o = replace(o, a=o.a.clone(), w=o.w.clone(), bias=torch.full((1, N), 300.0), res=o.res.clone())
    o.a[:, :, 0], o.w[:, 0] = 4.0, -75.0
    o.res[0, M - 1] = 300.0
    o.asum = o.a.double()
    o.x64 = o.asum @ o.w.double().T
    return c, o
