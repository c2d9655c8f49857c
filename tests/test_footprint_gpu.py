"""Every access model of hazard.MODELS held to what its kernel touches (W, O, R of tests/_footprint.py), then the whole
launch program: arena-content independence and program-level W on the capture topology.

The case table (CASES) is importable without a GPU: test_footprint_cpu.py checks that it covers exactly
set(hazard.MODELS) with at least two cases per entry point.  A case allocates EVERY buffer of its call in the slab
(weights, packed streams, integer tables, workspaces, counters included); only arguments the entry point dereferences on
the host stay outside (HOST_ARGS).  Shapes follow the parametrisations of tests/test_kernels_gpu.py, with row pitches,
batch strides and gaps added wherever the entry point takes one."""
import ctypes as C
import os
import time

import numpy as np
import pytest
import torch

import _footprint as fp
from tce_rvos_amd import _lib, hazard

F32, I32, I64, U8 = torch.float32, torch.int32, torch.int64, torch.uint8

# ---------------------------------------------------------------------------------------------------------------------
# The three lists.  W has no exemptions.
# ---------------------------------------------------------------------------------------------------------------------
# O: buffers that a launch need not write in full -- scratch whose content no later launch reads.  {entry: {argument: index in
# _lib.SIGNATURES[entry][1]}}; the key is also the slab name of the buffer in the cases below.
O_EXEMPT = {
    "tce_gemm_splitk_f32": {"workspace": 2},        # splits * M * N partial sums: scratch between the two passes of one entry
    "tce_gemm_splitk_ln_f32": {"workspace": 2},
    "tce_groupnorm_f32": {"ws": 4},                 # per-(frame, group) partial statistics
    "tce_groupnorm_up_add_f32": {"ws": 5},
    "tce_mha_ws_f32": {"ws": 4},                    # fp16 planes of K / V, padded to the key tile
    "tce_ffn_fused_split_f32": {"ws": 16, "counters": 18},   # partial sums of the cut blocks only; counters: zero before and after
    "tce_conv3x3_split_f32": {"ws": 11},            # planned for the split blocks only
}
# R: entry points that accumulate with float atomics are not bit-reproducible; finite + the tolerance of the entry point's own
# test (test_msda_backward_matches_reference_fixture: 1e-4 relative, 1e-5 * max|ref| absolute).
ATOMIC = {
    "tce_ms_deform_attn_backward_f32": {"grad_value": 6},    # csrc/msda.hip:676-688: atomicAdd(gvalue + p, w * top)
}
ATOMIC_TOL = (1e-4, 1e-5)
# arguments the entry point reads on the HOST at launch time: they stay outside the slab
HOST_ARGS = {
    "tce_msda_fused_f32": {"shapes_hw": 4},
    "tce_msda_fused_valid_f32": {"shapes_hw": 4, "valid_hw": 5},
    "tce_msda_fewq_raw_f32": {"shapes_hw": 6, "valid_hw": 7},
    "tce_copy_segments": {"segs": 0},
    "tce_gemm_f32": {"args": 0}, "tce_gemm_splitk_f32": {"args": 0}, "tce_gemm_splitk_ln_f32": {"args": 0},
    "tce_rowlin_f32": {"args": 0}, "tce_xattn_fused_f32": {"args": 0}, "tce_xattn_ffn_fused_f32": {"args": 0, "ffn": 1},
    "tce_fewrow_linear_f32": {"args": 0},
}


class Case:
    def __init__(self, entry, tag, build, mode=None):
        self.entry, self.tag, self.build, self.mode = entry, tag, build, mode
        self.id = f"{entry}-{tag}" + (f"-{mode}" if mode else "")
        self.exempt = tuple(O_EXEMPT.get(entry, {}))
        # R fills the workspaces too, whatever the model says about reading them; the split counters are a true input (zero)
        self.scratch = tuple(n for n in self.exempt if n != "counters")
        self.atomic = (tuple(ATOMIC[entry]),) + ATOMIC_TOL if entry in ATOMIC else None


CASES = []


def case(entry, tag, mode=None, **kw):
    def deco(fn):
        CASES.append(Case(entry, tag, (lambda S, fn=fn, kw=kw: fn(S, **kw)), mode))
        return fn
    return deco


def L():
    return _lib.lib()


def st():
    return torch.cuda.current_stream().cuda_stream


def P(t):
    return None if t is None else t.data_ptr()


def call(name, *a):
    _lib.check(getattr(L(), name)(*a, st()), name)


def ops():
    from tce_rvos_amd import ops as o
    return o


def pinned(setter, value, fn):
    """fn with a launch form pinned through the library's tuning switch for the duration of the call (0 = automatic again)."""
    def go():
        getattr(_lib.lib_raw(), setter)(value)
        try:
            fn()
        finally:
            getattr(_lib.lib_raw(), setter)(0)
    if getattr(fn, "post", None):
        go.post = fn.post
    return go


def ln(S, n, tag=""):
    return S.randn("gamma" + tag, (n,), scale=0.2, shift=1.0), S.randn("beta" + tag, (n,), scale=0.1)


# ---------------------------------------------------------------------------------------------------------------------
# matrix products
# ---------------------------------------------------------------------------------------------------------------------
def _gemm(S, M, N, K, batch=1, bias=True, a2=False, act=0, res_mode=0, splitk=1, lnorm=False, inplace=False, pad=4, tile=None):
    """tile: the output tile the launcher must choose for this shape in this arithmetic (asserted: the coverage of the tile
    kernels cannot shrink silently when a selection rule moves)."""
    o = ops()
    if tile is not None:
        got = _lib.lib_raw().tce_gemm_select_tile_ex(M, N, K, batch, 0)
        assert got == tile, f"gemm {M}x{N}x{K} batch {batch}: the launcher selects tile {got}, the case is meant for {tile}"
    lda, ldw, ldc, ldres = K + pad, K + pad, (N if lnorm else N + pad), N + 2 * pad
    sA, sW, sC, sRes = M * lda + 64, N * ldw + 32, M * ldc + 128, M * ldres + 64
    sh = (lambda r, c: (batch, r, c)) if batch > 1 else (lambda r, c: (r, c))
    kb = (lambda s: {"bstride": s}) if batch > 1 else (lambda s: {})
    A = S.randn("A", sh(M, K), pitch=lda, **kb(sA))
    A2 = S.randn("A2", (M, K), pitch=K + 2 * pad) if a2 else None  # shared by the batch (sA2 = 0)
    W = S.randn("W", sh(N, K), scale=K ** -0.5, pitch=ldw, **kb(sW))
    b = S.randn("bias", sh(1, N) if batch > 1 else (N,), **({"pitch": N, "bstride": N + 16} if batch > 1 else {})) if bias else None
    if inplace:
        Cc = S.randn("C", sh(M, N), pitch=ldc, **kb(sC))
        R, ldres, sRes = Cc, ldc, sC
    else:
        R = S.randn("res", sh(M, N), pitch=ldres, **kb(sRes)) if res_mode else None
        Cc = S.alloc("C", sh(M, N), pitch=ldc, **kb(sC))
    ws = S.alloc("workspace", (splitk * M * N,)) if splitk > 1 else None
    g = ln(S, N) if lnorm else None

    def fn():
        o.gemm_ex(A, W, Cc, M, N, K, lda, ldw, ldc, bias=b, a2=A2, lda2=K + 2 * pad, act=act, res=R, ldres=ldres, res_mode=res_mode,
                  batch=batch, sA=sA if batch > 1 else 0, sW=sW if batch > 1 else 0, sBias=N + 16 if (batch > 1 and bias) else 0,
                  sC=sC if batch > 1 else 0, sRes=sRes if batch > 1 else 0, splitk=splitk, ws=ws, ln=g if splitk > 1 else None)
    return fn


# every output tile of the launcher (csrc/gemm.hip select_tile_ex), each at a ragged M and N with pitched rows
case("tce_gemm_f32", "tile6464_1200x2048x256")(lambda S: _gemm(S, 1200, 2048, 256, tile=6464))
case("tce_gemm_f32", "tile6464_ragged_130x70x96_gelu_res_a2")(lambda S: _gemm(S, 130, 70, 96, a2=True, act=2, res_mode=1, tile=6464))
case("tce_gemm_f32", "tile6464_ragged_130x70x96_gelu_res_a2", mode="f32")(lambda S: _gemm(S, 130, 70, 96, a2=True, act=2, res_mode=1, tile=6464))
case("tce_gemm_f32", "tile6464_ragged_300x384x96_relu_mul", mode="f16")(lambda S: _gemm(S, 300, 384, 96, act=1, res_mode=2, tile=6464))
case("tce_gemm_f32", "tile6464_tiny_1x1x16_nobias")(lambda S: _gemm(S, 1, 1, 16, bias=False, tile=6464))
case("tce_gemm_f32", "tile6464_batched_3x333x160x256")(lambda S: _gemm(S, 333, 160, 256, batch=3, act=1, tile=6464))
case("tce_gemm_f32", "tile6464_relu_after_res_inplace_25x256x256")(lambda S: _gemm(S, 25, 256, 256, act=3, res_mode=1, inplace=True, tile=6464))
case("tce_gemm_f32", "tile12864_ragged_3333x1000x160_gelu_res_a2")(lambda S: _gemm(S, 3333, 1000, 160, a2=True, act=2, res_mode=1, tile=12864))
case("tce_gemm_f32", "tile12864_ragged_3333x1000x160_relu", mode="f32")(lambda S: _gemm(S, 3333, 1000, 160, act=1, tile=12864))
case("tce_gemm_f32", "tile12864_batched_5x4820x384x256")(lambda S: _gemm(S, 4820, 384, 256, batch=5, act=1, tile=12864))
case("tce_gemm_f32", "tile12864_ragged_33333x70x96_mul", mode="f16")(lambda S: _gemm(S, 33333, 70, 96, res_mode=2, tile=12864))
case("tce_gemm_f32", "tile256128_ragged_12345x1000x96_gelu_res")(lambda S: _gemm(S, 12345, 1000, 96, act=2, res_mode=1, tile=256128))
case("tce_gemm_f32", "tile256128_ragged_16333x250x1024_a2_relu")(lambda S: _gemm(S, 16333, 250, 1024, a2=True, act=1, tile=256128))
case("tce_gemm_f32", "tile256128_ragged_12345x1000x96_mul", mode="f16")(lambda S: _gemm(S, 12345, 1000, 96, res_mode=2, tile=256128))
case("tce_gemm_f32", "tile128128_ragged_12345x1000x96_gelu_res", mode="f32")(lambda S: _gemm(S, 12345, 1000, 96, act=2, res_mode=1, tile=128128))


@case("tce_gemm_f32", "conv3x3s1_2x9x13x32_48", T=2, H=9, W=13, Cin=32, N=48, k=3, s=1, p=1, tile=6464)
@case("tce_gemm_f32", "conv3x3s2_3x12x20x64_256_res", T=3, H=12, W=20, Cin=64, N=256, k=3, s=2, p=1, res=True, tile=6464)
@case("tce_gemm_f32", "conv3x3s1_tile128128_2x90x91x32_250", T=2, H=90, W=91, Cin=32, N=250, k=3, s=1, p=1, tile=128128)
@case("tce_gemm_f32", "conv3x3s1_tile128128_2x90x91x32_250_res", T=2, H=90, W=91, Cin=32, N=250, k=3, s=1, p=1, res=True, tile=128128, mode="f16")
@case("tce_gemm_splitk_f32", "conv_1x9x7x64_96_s3", T=1, H=9, W=7, Cin=64, N=96, k=3, s=1, p=1, splitk=3)
def _conv(S, T, H, W, Cin, N, k, s, p, res=False, splitk=1, tile=None):
    o = ops()
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    if tile is not None:
        got = _lib.lib_raw().tce_gemm_select_tile_ex(T * Ho * Wo, N, k * k * Cin, 1, 1)
        assert got == tile, f"conv {T}x{H}x{W}x{Cin}->{N}: the launcher selects tile {got}, the case is meant for {tile}"
    x = S.randn("A", (T * H * W, Cin))
    w = S.randn("W", (N, k * k * Cin), scale=(k * k * Cin) ** -0.5)
    b = S.randn("bias", (N,))
    R = S.randn("res", (T * Ho * Wo, N)) if res else None
    out = S.alloc("C", (T * Ho * Wo, N))
    ws = S.alloc("workspace", (splitk * T * Ho * Wo * N,)) if splitk > 1 else None
    return lambda: o.conv2d_cl(x, w, T, H, W, Cin, k, k, s, p, bias=b, act=3 if res else 0, out=out, res=R, res_mode=1 if res else 0,
                               splitk=splitk, ws=ws)


case("tce_gemm_splitk_f32", "32x2304x768_s4_gelu")(lambda S: _gemm(S, 32, 2304, 768, act=2, splitk=4))
case("tce_gemm_splitk_f32", "25x256x2048_s8_res")(lambda S: _gemm(S, 25, 256, 2048, res_mode=1, splitk=8))
case("tce_gemm_splitk_f32", "1x768x768_s2_nobias", mode="f32")(lambda S: _gemm(S, 1, 768, 768, bias=False, splitk=2))
case("tce_gemm_splitk_ln_f32", "32x768x3072_s16_res")(lambda S: _gemm(S, 32, 768, 3072, res_mode=1, splitk=16, lnorm=True))
case("tce_gemm_splitk_ln_f32", "25x256x2048_s8_res_inplace")(lambda S: _gemm(S, 25, 256, 2048, res_mode=1, splitk=8, lnorm=True, inplace=True))
case("tce_gemm_splitk_ln_f32", "1x768x768_s4")(lambda S: _gemm(S, 1, 768, 768, splitk=4, lnorm=True))


@case("tce_thin_partials_f32", "32x2304x768", M=32, N=2304, K=768)
@case("tce_thin_partials_f32", "7x768x768", M=7, N=768, K=768)
@case("tce_thin_partials_f32", "32x768x3072_from_planes_gelu", M=32, N=768, K=3072, xs=3)
@case("tce_thin_partials_f32", "1x32x256", M=1, N=32, K=256, mode="f16")
def _thin(S, M, N, K, xs=0):
    ldx, ldw = (K if xs else K + 8), K + 4
    x = S.randn("x", (xs * M, K)) if xs else S.randn("x", (M, K), pitch=ldx)
    bx = S.randn("bias_x", (K,)) if xs else None
    W = S.randn("W", (N, K), scale=K ** -0.5, pitch=ldw)
    ws = S.alloc("ws", ((K // 256) * M * N,))
    return lambda: call("tce_thin_partials_f32", P(x), ldx, xs, P(bx), 2 if xs else 0, P(W), ldw, P(ws), M, N, K)


@case("tce_splitk_reduce_f32", "3x32x768_res_ln", splits=3, M=32, N=768, res=True, lnorm=True)
@case("tce_splitk_reduce_f32", "2x7x768_gelu", splits=2, M=7, N=768, act=2)
@case("tce_splitk_reduce_f32", "12x100x3072_res_mul_nobias", splits=12, M=100, N=3072, res=True, res_mode=2, bias=False)
def _reduce(S, splits, M, N, res=False, res_mode=1, lnorm=False, act=0, bias=True):
    ws = S.randn("ws", (splits * M, N))
    b = S.randn("bias", (N,)) if bias else None
    ldres, ldc = N + 8, (N if lnorm else N + 4)
    R = S.randn("res", (M, N), pitch=ldres) if res else None
    out = S.alloc("C", (M, N), pitch=ldc)
    g = ln(S, N) if lnorm else (None, None)
    return lambda: call("tce_splitk_reduce_f32", P(ws), splits, M, N, P(b), act, P(R), ldres, res_mode if res else 0, P(out), ldc,
                        P(g[0]), P(g[1]), 1e-5)


@case("tce_fewrow_linear_f32", "40x256_three_segments_ln_in", R=40, K=256, nseg=3, full=True)
@case("tce_fewrow_linear_f32", "7x96_one_segment", R=7, K=96, nseg=1)
@case("tce_fewrow_linear_f32", "200x256_two_segments_a2", R=200, K=256, nseg=2, a2rows=50)
@case("tce_fewrow_linear_f32", "32x768_gelu", R=32, K=768, nseg=1, act=3)
def _fewrow(S, R, K, nseg, full=False, a2rows=0, act=0):
    o = ops()
    ldx = K + 4
    x = S.randn("x", (R, K), pitch=ldx)
    a2 = S.randn("a2", (a2rows or R, K), pitch=K + 8) if (full or a2rows) else None
    Ns = [256, 104, 32][:nseg]
    segs = []
    for i, N in enumerate(Ns):
        W = S.randn(f"W{i}", (N, K), scale=K ** -0.5, pitch=K + 4)
        b = S.randn(f"bias{i}", (N,)) if i != 1 else None
        out = S.alloc(f"out{i}", (R, N), pitch=N + 4)
        segs.append((W, b, out, N, N + 4, a2 is not None and i != 2, act if i == 0 else (2 if i == 1 else 1)))
    res = S.randn("res", (R, Ns[0]), pitch=Ns[0] + 12) if full else None
    g = ln(S, K) if full else None
    xn = S.alloc("xn_out", (R, K), pitch=K + 16) if full else None
    return lambda: o.fewrow_linear(x, R, K, segs, ldx=ldx, a2=a2, lda2=K + 8, a2_rows=a2rows, res=res, ldres=Ns[0] + 12, ln_in=g,
                                   xn_out=xn)


# ---------------------------------------------------------------------------------------------------------------------
# norms, resampling, element-wise
# ---------------------------------------------------------------------------------------------------------------------
@case("tce_layernorm_f32", "1000x256_res", M=1000, Cn=256, r=True)
@case("tce_layernorm_f32", "7x260", M=7, Cn=260)
@case("tce_layernorm_f32", "17x132_inplace", M=17, Cn=132, inplace=True)
@case("tce_layernorm_f32", "33x3072_res", M=33, Cn=3072, r=True)
@case("tce_layernorm_f32", "9x4", M=9, Cn=4)
def _layernorm(S, M, Cn, r=False, inplace=False):
    x = S.randn("x", (M, Cn))
    rr = S.randn("r", (M, Cn)) if r else None
    g, b = ln(S, Cn)
    out = x if inplace else S.alloc("out", (M, Cn))
    return lambda: call("tce_layernorm_f32", P(x), P(rr), P(g), P(b), P(out), M, Cn, 1e-5)


@case("tce_groupnorm_f32", "2x60x256_g32", T=2, HW=60, Cn=256, G=32, relu=0)
@case("tce_groupnorm_f32", "3x1300x256_g8_relu", T=3, HW=1300, Cn=256, G=8, relu=1)
@case("tce_groupnorm_f32", "1x14400x64_g8_relu", T=1, HW=14400, Cn=64, G=8, relu=1)
def _groupnorm(S, T, HW, Cn, G, relu):
    x = S.randn("x", (T * HW, Cn))
    g, b = ln(S, Cn)
    out = S.alloc("out", (T * HW, Cn))
    ws = S.alloc("ws", (T * G * (_lib.lib_raw().tce_groupnorm_nsplit(HW) * 3 + 2),))
    return lambda: call("tce_groupnorm_f32", P(x), P(g), P(b), P(out), P(ws), T, HW, Cn, G, 1e-5, relu)


@case("tce_groupnorm_up_add_f32", "5x23x40_to_45x80_g8", T=5, h=23, w=40, ho=45, wo=80, G=8)
@case("tce_groupnorm_up_add_f32", "2x6x7_to_13x15_g32_inplace", T=2, h=6, w=7, ho=13, wo=15, G=32, inplace=True)
def _gn_up(S, T, h, w, ho, wo, G, inplace=False, Cn=256):
    x = S.randn("x", (T * h * w, Cn))
    g, b = ln(S, Cn)
    add = S.randn("add", (T * ho * wo, Cn))
    out = add if inplace else S.alloc("out", (T * ho * wo, Cn))
    ws = S.alloc("ws", (T * G * (_lib.lib_raw().tce_groupnorm_nsplit(h * w) * 3 + 2),))
    return lambda: call("tce_groupnorm_up_add_f32", P(x), P(g), P(b), P(add), P(out), P(ws), T, h, w, ho, wo, Cn, G, 1e-5, 1)


@case("tce_resize_nearest_f32", "2x12x20_to_23x40_add", name="tce_resize_nearest_f32", T=2, h=12, w=20, ho=23, wo=40, Cn=256, add=True)
@case("tce_resize_nearest_f32", "3x5x7_to_11x13_c96", name="tce_resize_nearest_f32", T=3, h=5, w=7, ho=11, wo=13, Cn=96)
@case("tce_resize_bilinear_f32", "2x12x20_to_23x40_add", name="tce_resize_bilinear_f32", T=2, h=12, w=20, ho=23, wo=40, Cn=256, add=True)
@case("tce_resize_bilinear_f32", "3x11x13_to_5x7_c96_down", name="tce_resize_bilinear_f32", T=3, h=11, w=13, ho=5, wo=7, Cn=96)
@case("tce_resize_bilinear_f32", "1x1x1_to_3x2", name="tce_resize_bilinear_f32", T=1, h=1, w=1, ho=3, wo=2, Cn=256)
def _resize(S, name, T, h, w, ho, wo, Cn, add=False):
    x = S.randn("in", (T * h * w, Cn))
    a = S.randn("add", (T * ho * wo, Cn)) if add else None
    out = S.alloc("out", (T * ho * wo, Cn))
    return lambda: call(name, P(x), P(a), P(out), T, h, w, ho, wo, Cn)


@case("tce_resize_bilinear_ln_f32", "2x12x20_to_23x40", T=2, h=12, w=20, ho=23, wo=40)
@case("tce_resize_bilinear_ln_f32", "3x5x7_to_11x13_inplace", T=3, h=5, w=7, ho=11, wo=13, inplace=True)
@case("tce_resize_bilinear_ln_f32", "1x1x1_to_3x2", T=1, h=1, w=1, ho=3, wo=2)
def _resize_ln(S, T, h, w, ho, wo, inplace=False, Cn=256):
    x = S.randn("in", (T * h * w, Cn))
    a = S.randn("add", (T * ho * wo, Cn))
    g, b = ln(S, Cn)
    out = a if inplace else S.alloc("out", (T * ho * wo, Cn))
    return lambda: call("tce_resize_bilinear_ln_f32", P(x), P(a), P(g), P(b), 1e-5, P(out), T, h, w, ho, wo, Cn)


@case("tce_add_f32", "256000_plus_256", n=256000, nb=256)
@case("tce_add_f32", "77_plus_77", n=77, nb=77)
def _add(S, n, nb):
    a, b, out = S.randn("a", (n,)), S.randn("b", (nb,)), S.alloc("out", (n,))
    return lambda: call("tce_add_f32", P(a), P(b), P(out), n, nb)


@case("tce_tile_f32", "256x5", n=256, reps=5)
@case("tce_tile_f32", "7x3", n=7, reps=3)
def _tile(S, n, reps):
    a, out = S.randn("src", (n,)), S.alloc("out", (n * reps,))
    return lambda: call("tce_tile_f32", P(a), P(out), n, reps)


@case("tce_sigmoid_f32", "1000", name="tce_sigmoid_f32", n=1000)
@case("tce_sigmoid_f32", "13_inplace", name="tce_sigmoid_f32", n=13, inplace=True)
@case("tce_tanh_f32", "1536_inplace", name="tce_tanh_f32", n=1536, inplace=True)
@case("tce_tanh_f32", "13", name="tce_tanh_f32", n=13)
def _unary(S, name, n, inplace=False):
    x = S.randn("x", (n,))
    out = x if inplace else S.alloc("out", (n,))
    return lambda: call(name, P(x), P(out), n)


@case("tce_box_refine_f32", "25_ref2", n=25, rd=2)
@case("tce_box_refine_f32", "7_ref4", n=7, rd=4)
def _box(S, n, rd):
    tmp, ref, out = S.randn("tmp", (n, 4)), S.rand("ref", (n, rd), lo=0.05, hi=0.95), S.alloc("out", (n, 4))
    return lambda: call("tce_box_refine_f32", P(tmp), P(ref), P(out), n, rd)


@case("tce_copy_segments", "dense_and_gather", n=2)
@case("tce_copy_segments", "three_segments_odd_sizes", n=3)
def _copy(S, n):
    geo = [(1, 1000, 1000), (37, 25, 40), (3, 1, 7)][:n]  # (rows, row_words, src_pitch_words)
    segs = (_lib.CopySeg * n)()
    for i, (rows, rw, pitch) in enumerate(geo):
        src = S.randn(f"src{i}", (rows, rw), pitch=pitch)
        dst = S.alloc(f"dst{i}", (rows * rw,))
        segs[i].src, segs[i].dst, segs[i].rows, segs[i].row_words, segs[i].src_pitch_words = P(src), P(dst), rows, rw, pitch
    return lambda: call("tce_copy_segments", segs, n)


@case("tce_pos_sine2d_f32", "2x9x13_add", name="tce_pos_sine2d_f32", T=2, h=9, w=13, add=True)
@case("tce_pos_sine2d_f32", "1x6x10", name="tce_pos_sine2d_f32", T=1, h=6, w=10)
@case("tce_pos_sine2d_valid_f32", "2x9x13_valid_7x10_add", name="tce_pos_sine2d_valid_f32", T=2, h=9, w=13, valid=(7, 10), add=True)
@case("tce_pos_sine2d_valid_f32", "1x6x10_valid_5x10", name="tce_pos_sine2d_valid_f32", T=1, h=6, w=10, valid=(5, 10))
def _pos(S, name, T, h, w, add=False, valid=None, Fh=128):
    a = S.randn("add", (2 * Fh,)) if add else None
    out = S.alloc("out", (T * h * w, 2 * Fh))
    extra = tuple(valid) if valid else ()
    return lambda: call(name, P(out), P(a), T, h, w, Fh, *extra)


@case("tce_contrastive_f32", "3x168_fpc3", T=3, Sn=168, fpc=3)
@case("tce_contrastive_f32", "8x1000_fpc2", T=8, Sn=1000, fpc=2)
@case("tce_contrastive_f32", "1x7_fpc1", T=1, Sn=7, fpc=1)
def _contrastive(S, T, Sn, fpc, Cn=256):
    mem, sent = S.randn("memory", (T * Sn, Cn)), S.randn("sent", (T // fpc, Cn))
    out, ws = S.alloc("out", (T,)), S.alloc("ws", (T * 32 * Cn,))
    return lambda: call("tce_contrastive_f32", P(mem), P(sent), P(out), P(ws), T, Sn, Cn, fpc)


# ---------------------------------------------------------------------------------------------------------------------
# backbones and front-end
# ---------------------------------------------------------------------------------------------------------------------
@case("tce_resnet_stem_f32", "1x72x100", T=1, H=72, W=100)
@case("tce_resnet_stem_f32", "2x37x61", T=2, H=37, W=61)
def _stem(S, T, H, W):
    fr = S.randn("frames", (T * 3 * H, W))
    w, b = S.randn("w_k64", (147, 64), scale=0.1), S.randn("bias", (64,))
    out = S.alloc("out", (T * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1), 64))
    return lambda: call("tce_resnet_stem_f32", P(fr), P(w), P(b), P(out), T, H, W)


@case("tce_maxpool3x3s2_cl_f32", "1x36x50x64", T=1, H=36, W=50, Cn=64)
@case("tce_maxpool3x3s2_cl_f32", "2x19x31x64", T=2, H=19, W=31, Cn=64)
def _maxpool(S, T, H, W, Cn):
    x = S.randn("x", (T * H * W, Cn))
    out = S.alloc("out", (T * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1), Cn))
    return lambda: call("tce_maxpool3x3s2_cl_f32", P(x), P(out), T, H, W, Cn)


@case("tce_patch_embed_f32", "2x72x100_c96", T=2, H=72, W=100, Cn=96)
@case("tce_patch_embed_f32", "1x30x41_c128", T=1, H=30, W=41, Cn=128)
@case("tce_patch_embed_f32", "1x37x50_c192", T=1, H=37, W=50, Cn=192)
def _patch_embed(S, T, H, W, Cn):
    fr = S.randn("frames", (T * 3 * H, W))
    w, b = S.randn("w", (Cn, 48), scale=0.15), S.randn("b", (Cn,))
    g, be = ln(S, Cn)
    out = S.alloc("out", (T * ((H + 3) // 4) * ((W + 3) // 4), Cn))
    return lambda: call("tce_patch_embed_f32", P(fr), P(w), P(b), P(g), P(be), P(out), T, H, W, Cn, 1e-5)


@case("tce_window_attn_f32", "2x18x25_h3_shift3", name="tce_window_attn_f32", T=2, H=18, W=25, nH=3, shift=3, rows=169)
@case("tce_window_attn_f32", "2x18x25_h3_shift3", name="tce_window_attn_f32", T=2, H=18, W=25, nH=3, shift=3, rows=169, mode="f32")
@case("tce_window_attn_f32", "1x9x13_h6_noshift", name="tce_window_attn_f32", T=1, H=9, W=13, nH=6, shift=0, rows=169)
@case("tce_window_attn_f32", "1x7x7_h1_shift3", name="tce_window_attn_f32", T=1, H=7, W=7, nH=1, shift=3, rows=169, mode="f32")
@case("tce_window_attn3d_f32", "3x18x25_h3", name="tce_window_attn3d_f32", T=3, H=18, W=25, nH=3, shift=0, rows=15 * 169)
@case("tce_window_attn3d_f32", "9x9x13_h2_shifted", name="tce_window_attn3d_f32", T=9, H=9, W=13, nH=2, shift=1, rows=15 * 169)
def _win(S, name, T, H, W, nH, shift, rows):
    Cn = 32 * nH
    qkv, qb = S.randn("qkv", (T * H * W, 3 * Cn)), S.randn("qkv_bias", (3 * Cn,), scale=0.2)
    table = S.randn("bias_table", (rows, nH), scale=0.5)
    out = S.alloc("out", (T * H * W, Cn))
    return lambda: call(name, P(qkv), P(qb), P(table), P(out), T, H, W, Cn, nH, shift)


@case("tce_patch_merge_ln_f32", "2x18x25_c96", T=2, H=18, W=25, Cn=96)
@case("tce_patch_merge_ln_f32", "1x9x13_c192", T=1, H=9, W=13, Cn=192)
@case("tce_patch_merge_ln_f32", "1x4x4_c32", T=1, H=4, W=4, Cn=32)
def _merge(S, T, H, W, Cn):
    x = S.randn("x", (T * H * W, Cn))
    g, b = ln(S, 4 * Cn)
    out = S.alloc("out", (T * ((H + 1) // 2) * ((W + 1) // 2), 4 * Cn))
    return lambda: call("tce_patch_merge_ln_f32", P(x), P(g), P(b), P(out), T, H, W, Cn, 1e-5)


@case("tce_swin_attn_pack_f32", "c96", Cn=96)
@case("tce_swin_attn_pack_f32", "c192", Cn=192, mode="f16")
def _swin_pack(S, Cn):
    wq, wp = S.randn("Wqkv", (3 * Cn, Cn), scale=Cn ** -0.5), S.randn("Wproj", (Cn, Cn), scale=Cn ** -0.5)
    pk = S.alloc("packed", (_lib.lib_raw().tce_swin_attn_packed_bytes(Cn),), dtype=U8)
    return lambda: call("tce_swin_attn_pack_f32", P(wq), P(wp), P(pk), Cn)


@case("tce_swin_attn_fused_f32", "2x18x25_c96_shift3", T=2, H=18, W=25, Cn=96, shift=3)
@case("tce_swin_attn_fused_f32", "1x9x13_c192_inplace", T=1, H=9, W=13, Cn=192, shift=0, inplace=True)
@case("tce_swin_attn_fused_f32", "1x7x7_c256_shift3", T=1, H=7, W=7, Cn=256, shift=3, mode="f16")
def _swin_fused(S, T, H, W, Cn, shift, inplace=False):
    pk = _swin_pack(S, Cn)
    pk()  # the stream is an input of the launch under test
    pk = S.buf("packed").tensor
    ldx, ldo = Cn + 4, Cn + 8
    x = S.randn("x", (T * H * W, Cn), pitch=ldx)
    qb, pb = S.randn("qkv_bias", (3 * Cn,), scale=0.2), S.randn("proj_bias", (Cn,), scale=0.2)
    table = S.randn("bias_table", (169, Cn // 32), scale=0.5)
    g, b = ln(S, Cn)
    out, ldo = (x, ldx) if inplace else (S.alloc("out", (T * H * W, Cn), pitch=ldo), ldo)
    return lambda: call("tce_swin_attn_fused_f32", P(x), ldx, P(pk), P(qb), P(pb), P(table), P(g), P(b), 1e-5, P(out), ldo, T, H, W, Cn, shift)


def _coef(S, tag, n_in, n_out):
    from tce_rvos_amd.frontend import bilinear_coeffs
    c, b, k = bilinear_coeffs(n_in, n_out)
    return S.put("coef" + tag, torch.from_numpy(c)), S.put("bounds" + tag, torch.from_numpy(b)), k


@case("tce_resize_h_u8", "40x100_to_61", rows=40, Win=100, Wout=61)
@case("tce_resize_h_u8", "7x33_to_50_up", rows=7, Win=33, Wout=50)
def _resize_h(S, rows, Win, Wout):
    src = S.randint("in", (rows, Win * 3), 0, 256, dtype=U8)
    c, b, k = _coef(S, "", Win, Wout)
    tmp = S.alloc("tmp", (rows, Wout * 3), dtype=U8)
    return lambda: call("tce_resize_h_u8", P(src), P(c), P(b), P(tmp), rows, Win, Wout, k)


@case("tce_resize_v_norm_f32", "2x40x61_to_25", T=2, Hin=40, W=61, Hout=25)
@case("tce_resize_v_norm_f32", "1x7x50_to_11_up", T=1, Hin=7, W=50, Hout=11)
def _resize_v(S, T, Hin, W, Hout):
    from tce_rvos_amd.frontend import normalise_lut
    tmp = S.randint("tmp", (T * Hin, W * 3), 0, 256, dtype=U8)
    c, b, k = _coef(S, "", Hin, Hout)
    lut = S.put("lut", normalise_lut())
    out = S.alloc("out", (T * 3 * Hout, W))
    return lambda: call("tce_resize_v_norm_f32", P(tmp), P(c), P(b), P(lut), P(out), T, Hin, W, Hout, k)


# ---------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------
@case("tce_mha_f32", "5x8_700q_8k", name="tce_mha_f32", batch=5, nh=8, Lq=700, Lk=8)
@case("tce_mha_f32", "1x8_40q_40k_masked", name="tce_mha_f32", batch=1, nh=8, Lq=40, Lk=40, masked=True)
@case("tce_mha_f32", "2x8_33q_300k_masked", name="tce_mha_f32", batch=2, nh=8, Lq=33, Lk=300, masked=True, mode="f32")
@case("tce_mha_ws_f32", "1x8_1200q_1200k", name="tce_mha_ws_f32", batch=1, nh=8, Lq=1200, Lk=1200)
@case("tce_mha_ws_f32", "2x8_100q_1030k_masked", name="tce_mha_ws_f32", batch=2, nh=8, Lq=100, Lk=1030, masked=True)
@case("tce_mha_ws_f32", "1x8_25q_1500k", name="tce_mha_ws_f32", batch=1, nh=8, Lq=25, Lk=1500, mode="f16")
def _mha(S, name, batch, nh, Lq, Lk, masked=False):
    E = nh * 32
    ldq, ldk, ldv, ldo = E + 8, E + 4, E + 12, E + 16
    sQ, sK, sV, sO = Lq * ldq + 64, Lk * ldk + 32, Lk * ldv + 16, Lq * ldo + 128
    Q = S.randn("Q", (batch, Lq, E), pitch=ldq, bstride=sQ)
    K = S.randn("K", (batch, Lk, E), pitch=ldk, bstride=sK)
    V = S.randn("V", (batch, Lk, E), pitch=ldv, bstride=sV)
    O = S.alloc("O", (batch, Lq, E), pitch=ldo, bstride=sO)
    km = None
    if masked:
        m = torch.zeros(batch, Lk, dtype=U8)
        m[:, Lk - Lk // 3:] = 1
        m[0, 1] = 1
        km = S.put("kmask", m)
    ws = (S.alloc("ws", (_lib.lib_raw().tce_mha_ws_bytes(batch, nh, Lk),), dtype=U8),) if name == "tce_mha_ws_f32" else ()
    return lambda: call(name, P(Q), P(K), P(V), P(O), *[P(w) for w in ws], batch, nh, Lq, Lk, ldq, ldk, ldv, ldo, sQ, sK, sV, sO, P(km),
                        32 ** -0.5)


@case("tce_mha_small64_f32", "32x12", Ln=32, nh=12)
@case("tce_mha_small64_f32", "7x2", Ln=7, nh=2)
@case("tce_mha_small64_f32", "128x12", Ln=128, nh=12)
def _small64(S, Ln, nh):
    qkv, out = S.randn("qkv", (Ln, 3 * nh * 64)), S.alloc("out", (Ln, nh * 64))
    return lambda: call("tce_mha_small64_f32", P(qkv), P(out), Ln, nh, 0.125)


@case("tce_mha_small64_splits_f32", "3_planes_32x12_bias", kind="splits", splits=3, nseq=1, Ln=32, nh=12, bias=True)
@case("tce_mha_small64_splits_f32", "1_plane_5x2_nobias", kind="splits", splits=1, nseq=1, Ln=5, nh=2)
@case("tce_mha_small64_seqs_f32", "3_planes_2x11x12_bias", kind="seqs", splits=3, nseq=2, Ln=11, nh=12, bias=True)
@case("tce_mha_small64_seqs_f32", "1_plane_5x40x2_nobias", kind="seqs", splits=1, nseq=5, Ln=40, nh=2)
@case("tce_mha_small64_lens_f32", "1_plane_3x12x12", kind="lens", splits=1, nseq=3, Ln=12, nh=12, lens=(5, 12, 1))
@case("tce_mha_small64_lens_f32", "3_planes_2x33x2_bias", kind="lens", splits=3, nseq=2, Ln=33, nh=2, bias=True, lens=(33, 17))
def _small64_planes(S, kind, splits, nseq, Ln, nh, bias=False, lens=None):
    E = nh * 64
    planes = S.randn("qkv_planes", (splits * nseq * Ln, 3 * E), scale=0.6)
    b = S.randn("bias", (3 * E,), scale=0.2) if bias else None
    out = S.alloc("out", (nseq * Ln, E))
    if kind == "splits":
        return lambda: call("tce_mha_small64_splits_f32", P(planes), splits, P(b), P(out), Ln, nh, 0.125)
    if kind == "seqs":
        return lambda: call("tce_mha_small64_seqs_f32", P(planes), splits, P(b), P(out), nseq, Ln, nh, 0.125)
    ln_ = S.put("lens", torch.tensor(lens, dtype=I32))
    return lambda: call("tce_mha_small64_lens_f32", P(planes), splits, P(b), P(out), nseq, Ln, nh, 0.125, P(ln_))


LEVELS = ((12, 20), (6, 10), (3, 5), (2, 3))


def _levels(Lv):
    hw = LEVELS[:Lv]
    start = np.concatenate([[0], np.cumsum([h * w for h, w in hw])])
    return hw, start[:-1], int(start[-1])


@case("tce_ms_deform_attn_forward_f32", "2x17_m3_d30_l2_p3_generic", bwd=False, N=2, Lq=17, M=3, D=30, Lv=2, Pn=3)
@case("tce_ms_deform_attn_forward_f32", "1x300_m8_d32_l4_p4_rows16", bwd=False, N=1, Lq=300, M=8, D=32, Lv=4, Pn=4)
@case("tce_ms_deform_attn_forward_f32", "2x50_m8_d32_l4_p8_rows_dword", bwd=False, N=2, Lq=50, M=8, D=32, Lv=4, Pn=8)
@case("tce_ms_deform_attn_backward_f32", "2x17_m3_d30_l2_p3_generic", bwd=True, N=2, Lq=17, M=3, D=30, Lv=2, Pn=3)
@case("tce_ms_deform_attn_backward_f32", "1x300_m8_d32_l4_p4", bwd=True, N=1, Lq=300, M=8, D=32, Lv=4, Pn=4)
def _msda_ref(S, bwd, N, Lq, M, D, Lv, Pn):
    hw, start, Sn = _levels(Lv)
    value = S.randn("value", (N * Sn, M * D))
    shapes = S.put("spatial_shapes", torch.tensor(hw, dtype=I64))
    lsi = S.put("level_start_index", torch.tensor(start, dtype=I64))
    loc = S.rand("sampling_loc", (N * Lq * M, Lv * Pn * 2), lo=-0.1, hi=1.1)  # some samples fall outside the map
    aw = S.rand("attn_weight", (N * Lq * M, Lv * Pn), lo=0.0, hi=2.0 / (Lv * Pn))
    if not bwd:
        out = S.alloc("out", (N * Lq, M * D))
        return lambda: call("tce_ms_deform_attn_forward_f32", P(value), P(shapes), P(lsi), P(loc), P(aw), P(out), N, Sn, M, D, Lq, Lv, Pn)
    go = S.randn("grad_output", (N * Lq, M * D))
    gv, gl, ga = S.alloc("grad_value", (N * Sn, M * D)), S.alloc("grad_sampling_loc", (N * Lq * M, Lv * Pn * 2)), \
        S.alloc("grad_attn_weight", (N * Lq * M, Lv * Pn))
    return lambda: call("tce_ms_deform_attn_backward_f32", P(value), P(shapes), P(lsi), P(loc), P(aw), P(go), P(gv), P(gl), P(ga), N, Sn, M,
                        D, Lq, Lv, Pn)


@case("tce_msda_fused_f32", "2x300_ref2", kind="fused", N=2, Lq=300, rd=2)
@case("tce_msda_fused_f32", "3x5_ref4_per_frame_fewq", kind="fused", N=3, Lq=5, rd=4, rpf=1)
@case("tce_msda_fused_valid_f32", "2x300_ref2_padded", kind="valid", N=2, Lq=300, rd=2, padded=True)
@case("tce_msda_fused_valid_f32", "3x5_ref4_unpadded_per_frame", kind="valid", N=3, Lq=5, rd=4, rpf=1)
@case("tce_msda_fused_valid_f32", "2x700_ref2_padded", kind="valid", N=2, Lq=700, rd=2, padded=True)
@case("tce_msda_fewq_raw_f32", "5x8_ref2", kind="raw", N=5, Lq=8, rd=2)
@case("tce_msda_fewq_raw_f32", "2x8_ref2_padded", kind="raw", N=2, Lq=8, rd=2, padded=True)
@case("tce_msda_fewq_raw_f32", "1x1_ref4_padded_per_frame", kind="raw", N=1, Lq=1, rd=4, padded=True, rpf=1)
def _msda_fused(S, kind, N, Lq, rd, rpf=0, padded=False, M=8, Lv=4, Pn=4):
    hw, _, Sn = _levels(Lv)
    arr = (C.c_int32 * (2 * Lv))(*[v for p in hw for v in p])
    varr = (C.c_int32 * (2 * Lv))(*[v for h, w in hw for v in (max(1, h - h // 4), max(1, w - w // 5))]) if padded else None
    proj = S.randn("proj", (N * Lq, M * Lv * Pn * 3))
    ref = S.rand("ref", ((N if rpf else 1) * Lq, rd), lo=0.1, hi=0.9)
    out = S.alloc("out", (N * Lq, M * 32))
    if kind == "raw":
        src = S.randn("src", (N * Sn, 256))
        wv, bv = S.randn("wv", (256, 256), scale=1 / 16), S.randn("bv", (256,), scale=0.2)
        return lambda: call("tce_msda_fewq_raw_f32", P(src), P(wv), P(bv), P(proj), P(ref), P(out), arr, varr, N, Sn, M, Lq, Lv, Pn, rd, rpf)
    value = S.randn("value", (N * Sn, M * 32))
    if kind == "fused":
        return lambda: call("tce_msda_fused_f32", P(value), P(proj), P(ref), P(out), arr, N, Sn, M, Lq, Lv, Pn, rd, rpf)
    return lambda: call("tce_msda_fused_valid_f32", P(value), P(proj), P(ref), P(out), arr, varr, N, Sn, M, Lq, Lv, Pn, rd, rpf)


# ---------------------------------------------------------------------------------------------------------------------
# text encoder pieces
# ---------------------------------------------------------------------------------------------------------------------
@case("tce_embed_ln_f32", "32x768_derived_positions", Ln=32, Cn=768)
@case("tce_embed_ln_f32", "7x64_given_positions", Ln=7, Cn=64, given=True)
@case("tce_embed_ln_seqs_f32", "2x11x768", Ln=11, Cn=768, nseq=2)
@case("tce_embed_ln_seqs_f32", "3x5x64", Ln=5, Cn=64, nseq=3)
def _embed(S, Ln, Cn, nseq=0, given=False, vocab=50, pad_id=1):
    n = max(1, nseq) * Ln
    ids = torch.randint(2, vocab, (max(1, nseq), Ln), generator=torch.Generator().manual_seed(5))
    ids[:, Ln - Ln // 4:] = pad_id  # right-padded captions
    ids = S.put("ids", ids.reshape(-1))
    pos_ids = S.put("pos_ids", torch.arange(2, 2 + n, dtype=I64)) if given else None
    word, pos = S.randn("word", (vocab, Cn)), S.randn("pos", (pad_id + n + 2, Cn))
    type0 = S.randn("type0", (Cn,))
    g, b = ln(S, Cn)
    out = S.alloc("out", (n, Cn))
    if nseq:
        fn = lambda: call("tce_embed_ln_seqs_f32", P(ids), P(word), P(pos), P(type0), P(g), P(b), P(out), nseq, Ln, Cn, 1e-5, pad_id)  # noqa: E731
    else:
        fn = lambda: call("tce_embed_ln_f32", P(ids), P(pos_ids), P(word), P(pos), P(type0), P(g), P(b), P(out), Ln, Cn, 1e-5, pad_id)  # noqa: E731
    fn.tables = (word, pos)  # gathered by id: their extents are declared to the recording (hazard.recording(tables=...))
    return fn


@case("tce_caption_lens_f32", "3x12", nseq=3, Lmax=12, lens=(5, 12, 1))
@case("tce_caption_lens_f32", "1x40", nseq=1, Lmax=40, lens=(33,))
def _caption_lens(S, nseq, Lmax, lens, D=256, pad_id=1):
    ids = torch.randint(2, 50, (nseq, Lmax), generator=torch.Generator().manual_seed(6))
    for i, n in enumerate(lens):
        ids[i, n:] = pad_id
    ids = S.put("ids", ids.reshape(-1))
    ln_, km, pos = S.alloc("lens", (nseq,), dtype=I32), S.alloc("kmask", (nseq * Lmax,), dtype=U8), S.alloc("pos", (nseq * Lmax, D))
    return lambda: call("tce_caption_lens_f32", P(ids), nseq, Lmax, pad_id, D, P(ln_), P(km), P(pos))


# ---------------------------------------------------------------------------------------------------------------------
# fused FFN / token-stationary family (csrc/chain*.hip)
# ---------------------------------------------------------------------------------------------------------------------
@case("tce_ffn_pack_f32", "c256_h2048", name="tce_ffn_pack_f32", Cn=256, Hd=2048)
@case("tce_ffn_pack_f32", "c96_h384_nob1", name="tce_ffn_pack_f32", Cn=96, Hd=384, b1=False, mode="f16")
@case("tce_ffn_pack_chain_f32", "c256_h2048", name="tce_ffn_pack_chain_f32", Cn=256, Hd=2048)
@case("tce_ffn_pack_chain_f32", "c256_h1024_nob1", name="tce_ffn_pack_chain_f32", Cn=256, Hd=1024, b1=False)
@case("tce_ffn_pack_batched_f32", "c256_h64_b5", name="tce_ffn_pack_batched_f32", Cn=256, Hd=64, batch=5)
@case("tce_ffn_pack_batched_f32", "c256_h256_b2_nob1", name="tce_ffn_pack_batched_f32", Cn=256, Hd=256, batch=2, b1=False)
def _ffn_pack(S, name, Cn, Hd, batch=1, b1=True, tag=""):
    W1 = S.randn("W1" + tag, (batch * Hd, Cn), scale=Cn ** -0.5)
    bb = S.randn("b1" + tag, (batch * Hd,), scale=0.2) if b1 else None
    W2 = S.randn("W2" + tag, (batch * Cn, Hd), scale=Hd ** -0.5)
    pk = S.alloc("packed" + tag, (batch * _lib.lib_raw().tce_ffn_packed_bytes(Cn, Hd),), dtype=U8)
    extra = (batch,) if name == "tce_ffn_pack_batched_f32" else ()
    return lambda: call(name, P(W1), P(bb), P(W2), P(pk), Cn, Hd, *extra)


@case("tce_ffn_fused_f32", "3000x96_h384_gelu_ln_in", M=3000, Cn=96, Hd=384, act=2, lin=True)
@case("tce_ffn_fused_f32", "301x256_h2048_relu_ln_out_inplace", M=301, Cn=256, Hd=2048, act=1, lout=True, inplace=True)
@case("tce_ffn_fused_f32", "1003x128_h512_gelu_both", M=1003, Cn=128, Hd=512, act=2, lin=True, lout=True, mode="f16")
@case("tce_ffn_fused_f32", "50x192_h768_gelu_plain", M=50, Cn=192, Hd=768, act=2)
@case("tce_ffn_fused_f32", "3000x96_h384_gelu_ln_in_128row_workgroups", M=3000, Cn=96, Hd=384, act=2, lin=True, half=1)
@case("tce_ffn_fused_f32", "3000x96_h384_gelu_ln_in_256row_workgroups", M=3000, Cn=96, Hd=384, act=2, lin=True, half=-1)
@case("tce_ffn_fused_f32", "20001x128_h512_gelu_inplace_128row_workgroups", M=20001, Cn=128, Hd=512, act=2, lin=True, inplace=True, half=1)
@case("tce_ffn_fused_f32", "20001x128_h512_gelu_inplace_256row_workgroups", M=20001, Cn=128, Hd=512, act=2, lin=True, inplace=True, half=-1)
@case("tce_ffn_fused_split_f32", "18000x256_h2048_relu_ln_out", M=18000, Cn=256, Hd=2048, act=1, lout=True, split=True)
@case("tce_ffn_fused_split_f32", "17999x256_h2048_relu_plain_inplace", M=17999, Cn=256, Hd=2048, act=1, inplace=True, split=True)
@case("tce_ffn_fused_split_f32", "16000x256_h2048_relu_unsplit_plan", M=16000, Cn=256, Hd=2048, act=1, lout=True, split=True)
def _ffn(S, M, Cn, Hd, act, lin=False, lout=False, inplace=False, split=False, half=0):
    """half: the C <= 128 GELU kernel pinned to its 128-row (1) or 256-row (-1) workgroup form (tce_debug_ffn_set_half)."""
    _ffn_pack(S, "tce_ffn_pack_f32", Cn, Hd)()
    pk = S.buf("packed").tensor
    ldx, ldo = Cn + 4, Cn + 8
    x = S.randn("x", (M, Cn), pitch=ldx)
    b2 = S.randn("b2", (Cn,), scale=0.2)
    gi = ln(S, Cn, "_in") if lin else (None, None)
    go = ln(S, Cn, "_out") if lout else (None, None)
    out, ldo = (x, ldx) if inplace else (S.alloc("out", (M, Cn), pitch=ldo), ldo)
    if not split:
        fn = lambda: call("tce_ffn_fused_f32", P(x), ldx, P(pk), P(b2), P(gi[0]), P(gi[1]), 1e-5, P(go[0]), P(go[1]), 1e-5, P(out), ldo,  # noqa: E731
                          M, Cn, Hd, act)
        return pinned("tce_debug_ffn_set_half", half, fn) if half else fn
    raw = _lib.lib_raw()
    nws, ncnt = int(raw.tce_ffn_split_ws_floats(M, Cn, Hd, act)), int(raw.tce_ffn_split_counters(M, Cn, Hd, act))
    ws = S.alloc("ws", (max(nws, 4),))
    cnt = S.put("counters", torch.zeros(max(ncnt, 1), dtype=I32))  # the arena hands them out zeroed (ops.Arena.alloc_flags)

    def fn():
        call("tce_ffn_fused_split_f32", P(x), ldx, P(pk), P(b2), P(gi[0]), P(gi[1]), 1e-5, P(go[0]), P(go[1]), 1e-5, P(out), ldo, M, Cn, Hd,
             act, P(ws), nws, P(cnt), ncnt)

    def post():  # counter invariant: zero again when the launch ends
        assert int(cnt.abs().max()) == 0, f"split counters not zero after the launch: {cnt[cnt != 0][:8].tolist()}"
    fn.post = post
    return fn


@case("tce_rowlin_pack_f32", "384x256_pitched", N=384, K=256)
@case("tce_rowlin_pack_f32", "288x96", N=288, K=96, mode="f16")
def _rowlin_pack(S, N, K):
    ldw = K + 4
    W = S.randn("W", (N, K), scale=K ** -0.5, pitch=ldw)
    pk = S.alloc("packed", (_lib.lib_raw().tce_rowlin_packed_bytes(N, K),), dtype=U8)
    return lambda: call("tce_rowlin_pack_f32", P(W), ldw, P(pk), N, K)


@case("tce_rowlin_f32", "24100x256x256_ln_out", M=24100, N=256, K=256, variant="ln_out")
@case("tce_rowlin_f32", "1000x576x192_b2_plain", M=1000, N=576, K=192, batch=2, variant="plain")
@case("tce_rowlin_f32", "482x384x256_b5_a2_relu", M=482, N=384, K=256, batch=5, variant="a2_relu")
@case("tce_rowlin_f32", "1001x288x96_ln_in", M=1001, N=288, K=96, variant="ln_in")
@case("tce_rowlin_f32", "333x512x512_res_mul", M=333, N=512, K=512, variant="res_mul")
@case("tce_rowlin_f32", "777x384x384_gelu_res_inplace", M=777, N=384, K=384, variant="gelu_res", mode="f16")
@case("tce_rowlin_f32", "130x128x128_b3_a2_shared_rows", M=130, N=128, K=128, batch=3, variant="a2_mod")
def _rowlin(S, M, N, K, variant, batch=1):
    o = ops()
    _rowlin_pack(S, N, K)()
    pk = S.buf("packed").tensor
    ldx, ldo, ldres, lda2 = K + 4, N + 8, N + 12, K + 8
    sX, sOut, sRes, sA2 = M * ldx + 64, M * ldo + 128, M * ldres + 32, M * lda2 + 16
    sh = (lambda r, c: (batch, r, c)) if batch > 1 else (lambda r, c: (r, c))
    kb = (lambda s: {"bstride": s}) if batch > 1 else (lambda s: {})
    x = S.randn("x", sh(M, K), pitch=ldx, **kb(sX))
    bias = S.randn("bias", (N,), scale=0.2)
    kw = {}
    if variant == "a2_relu":
        kw = dict(a2=S.randn("a2", sh(M, K), pitch=lda2, **kb(sA2)), lda2=lda2, act=1, sA2=sA2 if batch > 1 else 0)
    elif variant == "a2_mod":
        kw = dict(a2=S.randn("a2", (40, K), pitch=lda2), lda2=lda2, a2_rows=40)
    elif variant == "res_mul":
        kw = dict(res=S.randn("res", sh(M, N), pitch=ldres, **kb(sRes)), ldres=ldres, res_mode=2, sRes=sRes if batch > 1 else 0)
    elif variant == "ln_in":
        kw = dict(ln_in=ln(S, K, "_in"))
    elif variant == "ln_out":
        kw = dict(ln_out=ln(S, N, "_out"), res=S.randn("res", sh(M, N), pitch=ldres, **kb(sRes)), ldres=ldres, res_mode=1)
    if variant == "gelu_res":  # out aliases res (in place on the residual stream)
        out = S.randn("out", sh(M, N), pitch=ldo, **kb(sOut))
        kw = dict(res=out, ldres=ldo, res_mode=1, act=2, sRes=sOut if batch > 1 else 0)
    else:
        out = S.alloc("out", sh(M, N), pitch=ldo, **kb(sOut))
    return lambda: o.rowlin(x, pk, out, M, N, K, ldx, ldo, bias=bias, batch=batch, sX=sX if batch > 1 else 0, sOut=sOut if batch > 1 else 0, **kw)


@case("tce_conv3x3_pack_f32", "256_256")
@case("tce_conv3x3_pack_f32", "256_256", mode="f16")
def _conv3_pack(S, Cin=256, N=256):
    w = S.randn("w", (N, 9 * Cin), scale=(9 * Cin) ** -0.5)
    pk = S.alloc("packed", (_lib.lib_raw().tce_conv3x3_packed_bytes(Cin, N),), dtype=U8)
    return lambda: call("tce_conv3x3_pack_f32", P(w), P(pk), Cin, N)


@case("tce_conv3x3_f32", "1x9x13_ragged", T=1, H=9, W=13)
@case("tce_conv3x3_f32", "2x32x40", T=2, H=32, W=40)
@case("tce_conv3x3_f32", "3x17x5_nobias", T=3, H=17, W=5, bias=False, mode="f16")
@case("tce_conv3x3_f32", "1x45x80_128px_workgroups", T=1, H=45, W=80, waves=4)
@case("tce_conv3x3_f32", "1x45x80_256px_workgroups", T=1, H=45, W=80, waves=8)
@case("tce_conv3x3_f32", "3x17x5_256px_workgroups_ragged", T=3, H=17, W=5, waves=8)
@case("tce_conv3x3_f32", "1x9x13_256px_workgroups_nobias", T=1, H=9, W=13, waves=8, bias=False)
@case("tce_conv3x3_f32", "5x90x160_mixed_256px_round_plus_128px_rest", T=5, H=90, W=160, mixed=True)
@case("tce_conv3x3_split_f32", "1x45x80_split", T=1, H=45, W=80, split=True, pieces=True)
@case("tce_conv3x3_split_f32", "3x17x5_split_ragged", T=3, H=17, W=5, split=True, pieces=True)
@case("tce_conv3x3_split_f32", "2x32x40_split_nobias", T=2, H=32, W=40, split=True, bias=False, mode="f16")
@case("tce_conv3x3_split_f32", "1x45x80_256px_workgroups_nothing_split", T=1, H=45, W=80, split=True, waves=8)
@case("tce_conv3x3_split_f32", "3x17x5_128px_workgroups_split", T=3, H=17, W=5, split=True, waves=4, pieces=True)
@case("tce_conv3x3_split_f32", "5x90x160_mixed_rest_split", T=5, H=90, W=160, split=True, mixed=True, pieces=True)
def _conv3(S, T, H, W, split=False, bias=True, Cin=256, N=256, waves=0, mixed=False, pieces=False):
    """waves: the workgroup form pinned (tce_debug_conv3x3_set_waves: 4 = 128-pixel, 8 = 256-pixel workgroups).  mixed: the
    launcher's own choice must be one full round of 256-pixel workgroups + the rest as 128-pixel ones (csrc/conv3x3.hip
    conv3x3_plan), read off the exported plan: the split workspace then covers exactly the pixels after that round.
    pieces: the split entry must really split (more than one piece)."""
    raw = _lib.lib_raw()
    _conv3_pack(S)()
    pk = S.buf("packed").tensor
    M = T * H * W
    raw.tce_debug_conv3x3_set_waves(waves)
    try:
        npieces = int(raw.tce_conv3x3_split_pieces(M, Cin, N))
        plan_ws = int(raw.tce_conv3x3_split_ws_floats(M, Cin, N))
    finally:
        raw.tce_debug_conv3x3_set_waves(0)
    if pieces:
        assert npieces > 1 and plan_ws == npieces * (M - (M // 65536 * 65536 if mixed else 0)) * 256, (M, npieces, plan_ws)
    if mixed:  # the remainder after the wide round(s) is what the plan splits: pixels [65536 * rounds, M)
        assert M > 65536 and npieces > 1 and plan_ws == npieces * (M % 65536) * 256, f"{M} px: not the mixed form (pieces {npieces}, ws {plan_ws})"
    if waves == 8:
        assert plan_ws == 0
    ldx, ldo = Cin + 4, N + 8
    x = S.randn("x", (M, Cin), pitch=ldx)
    b = S.randn("bias", (N,), scale=0.2) if bias else None
    out = S.alloc("out", (M, N), pitch=ldo)
    if not split:
        fn = lambda: call("tce_conv3x3_f32", P(x), ldx, P(pk), P(b), P(out), ldo, T, H, W, Cin, N)  # noqa: E731
    else:
        ws = S.alloc("ws", (max(plan_ws, 4),))
        fn = lambda: call("tce_conv3x3_split_f32", P(x), ldx, P(pk), P(b), P(out), ldo, T, H, W, Cin, N, P(ws), plan_ws)  # noqa: E731
    return pinned("tce_debug_conv3x3_set_waves", waves, fn) if waves else fn


def _xattn_kv(S, Lk, batch):
    k, v = S.randn("k", (batch * Lk, 256)), S.randn("v", (batch * Lk, 256))
    wq, wo = S.randn("wqT_ext", (257, 256), scale=1 / 64), S.randn("wo", (256, 256), scale=1 / 16)
    return k, v, wq, wo


@case("tce_xattn_prepare_f32", "l32_g32_b1", Lk=32, group=32, batch=1)
@case("tce_xattn_prepare_f32", "l5_g8_b2", Lk=5, group=8, batch=2)
@case("tce_xattn_prepare_lens_f32", "l12_g32_b3_lens", Lk=12, group=32, batch=3, lens=(5, 12, 1))
@case("tce_xattn_prepare_lens_f32", "l8_g8_b2_lens", Lk=8, group=8, batch=2, lens=(8, 3))
def _xattn_prepare(S, Lk, group, batch, lens=None):
    k, v, wq, wo = _xattn_kv(S, Lk, batch)
    Hd = 8 * group
    W1, b1, W2 = S.alloc("W1", (batch * Hd, 256)), S.alloc("b1", (batch * Hd,)), S.alloc("W2", (batch * 256, Hd))
    if lens is None:
        return lambda: call("tce_xattn_prepare_f32", P(k), P(v), P(wq), P(wo), P(W1), P(b1), P(W2), Lk, group, batch)
    ln_ = S.put("lens", torch.tensor(lens, dtype=I32))
    return lambda: call("tce_xattn_prepare_lens_f32", P(k), P(v), P(wq), P(wo), P(W1), P(b1), P(W2), Lk, group, batch, P(ln_))


@case("tce_xattn_pack_f32", "l32_g32_b1", Lk=32, group=32, batch=1)
@case("tce_xattn_pack_f32", "l9_g32_b1", Lk=9, group=32, batch=1)
@case("tce_xattn_pack_f32", "l5_g8_b2", Lk=5, group=8, batch=2)
@case("tce_xattn_pack_lens_f32", "l12_g32_b3_lens", Lk=12, group=32, batch=3, lens=(5, 12, 1))
@case("tce_xattn_pack_lens_f32", "l8_g8_b2_lens", Lk=8, group=8, batch=2, lens=(8, 3))
def _xattn_pack(S, Lk, group, batch, lens=None):
    k, v, wq, wo = _xattn_kv(S, Lk, batch)
    pk = S.alloc("packed", (batch, _lib.lib_raw().tce_ffn_packed_bytes(256, 8 * group)), dtype=U8)
    if lens is None:
        return lambda: call("tce_xattn_pack_f32", P(k), P(v), P(wq), P(wo), P(pk), Lk, group, batch)
    ln_ = S.put("lens", torch.tensor(lens, dtype=I32))
    return lambda: call("tce_xattn_pack_lens_f32", P(k), P(v), P(wq), P(wo), P(pk), Lk, group, batch, P(ln_))


@case("tce_xattn_fused_f32", "4600_l11_add_ln_a2", M=4600, Lk=11, mode_="add_ln")
@case("tce_xattn_fused_f32", "301_l32_mul", M=301, Lk=32, mode_="mul")
@case("tce_xattn_fused_f32", "720_l20_mul_batched_b5_shared_stream", M=720, Lk=20, mode_="mul", batch=5)
@case("tce_xattn_fused_f32", "130_l8_g8_b3_streams_per_frame_inplace", M=130, Lk=8, group=8, batch=3, per_batch=True, mode_="add_ln", inplace=True)
@case("tce_xattn_fused_f32", "301_l32_add_ln", M=301, Lk=32, mode_="add_ln", mode="f16")
@case("tce_xattn_ffn_fused_f32", "301_l11_g32_chain", M=301, Lk=11, mode_="add_ln", chain=True)
@case("tce_xattn_ffn_fused_f32", "130_l8_g8_b3_chain", M=130, Lk=8, group=8, batch=3, per_batch=True, mode_="add_ln", chain=True)
def _xattn(S, M, Lk, mode_, group=32, batch=1, per_batch=False, inplace=False, chain=False):
    o = ops()
    nstreams = batch if per_batch else 1
    _xattn_pack(S, Lk, group, nstreams)()
    pk = S.buf("packed").tensor
    ldx, ldo, ldres, lda2 = 260, 264, 268, 272
    sX, sOut, sRes = M * ldx + 64, M * ldo + 128, M * ldres + 32
    sh = (lambda r, c: (batch, r, c)) if batch > 1 else (lambda r, c: (r, c))
    kb = (lambda s: {"bstride": s}) if batch > 1 else (lambda s: {})
    x = S.randn("x", sh(M, 256), pitch=ldx, **kb(sX))
    bo = S.randn("bo", (256,), scale=0.2)
    kw = dict(res_mode=1 if mode_ == "add_ln" else 2)
    if mode_ == "add_ln":
        kw.update(a2=S.randn("a2", (40, 256), pitch=lda2), lda2=lda2, a2_rows=40, ln_out=ln(S, 256, "_out"))
    else:
        kw.update(res=S.randn("res", sh(M, 256), pitch=ldres, **kb(sRes)), ldres=ldres, sRes=sRes if batch > 1 else 0)
    if inplace:
        out, ldo, sOut = x, ldx, sX
    else:
        out = S.alloc("out", sh(M, 256), pitch=ldo, **kb(sOut))
    if chain:
        _ffn_pack(S, "tce_ffn_pack_chain_f32", 256, 1024, tag="_ffn")()
        mid = S.alloc("mid", sh(M, 256), **kb(M * 256 + 64))
        kw["ffn"] = (S.buf("packed_ffn").tensor, S.randn("b2", (256,), scale=0.2), 1024, ln(S, 256, "_ffn"), mid, M * 256 + 64 if batch > 1 else 0)
    return lambda: o.xattn_fused(x, pk, bo, M, out, batch=batch, sX=sX if batch > 1 else 0, sOut=sOut if batch > 1 else 0, ldx=ldx, ldo=ldo,
                                 group=group, per_batch_weights=per_batch, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# heads
# ---------------------------------------------------------------------------------------------------------------------
@case("tce_mask_pack_f32", "3x2x5", nl=3, T=2, Q=5)
@case("tce_mask_pack_f32", "1x1x1", nl=1, T=1, Q=1)
def _mask_pack(S, nl, T, Q, Cm=16):
    npar = 8 * (Cm + 2) + 64 + 8 + 8 + 8 + 1
    params = S.randn("params", (nl * T * Q, npar))
    w0f, tail = S.alloc("w0f", (T * nl * Q * 8, Cm)), S.alloc("tail", (nl * T * Q, 112))
    return lambda: call("tce_mask_pack_f32", P(params), P(w0f), P(tail), nl, T, Q, Cm)


@case("tce_mask_tail_f32", "3x2x5_18x25", nl=3, T=2, Q=5, h=18, w=25, ref_ld=4)
@case("tce_mask_tail_f32", "3x2x30_9x15", nl=3, T=2, Q=30, h=9, w=15, ref_ld=2)
@case("tce_mask_tail_f32", "1x1x1_5x131", nl=1, T=1, Q=1, h=5, w=131, ref_ld=2)
def _mask_tail(S, nl, T, Q, h, w, ref_ld):
    G = S.randn("G", (T * h * w, nl * Q * 8))
    tail = S.randn("tail", (nl * T * Q, 112))
    refs = S.rand("refs", (nl * T * Q, ref_ld), lo=0.1, hi=0.9)
    masks = S.alloc("masks", (nl * T * Q, h * w))
    return lambda: call("tce_mask_tail_f32", P(G), P(tail), P(refs), ref_ld, P(masks), nl, T, Q, h, w, float(h * 4), float(w * 4), 4)


@case("tce_select_masks_u8", "3x5x1_18x25_to_72x100", T=3, Q=5, K=1, h=18, w=25, H0=72, W0=100, best=True)
@case("tce_select_masks_u8", "2x3x2_9x13_to_37x50_no_index", T=2, Q=3, K=2, h=9, w=13, H0=37, W0=50, best=False)
def _select(S, T, Q, K, h, w, H0, W0, best):
    logits, masks = S.randn("logits", (T * Q, K)), S.randn("masks", (T * Q, h * w), scale=3.0)
    out = S.alloc("out", (T * H0 * W0,), dtype=U8)
    bq = S.alloc("best_query", (1,), dtype=I32) if best else None
    return lambda: call("tce_select_masks_u8", P(logits), P(masks), P(out), P(bq), T, Q, K, h, w, H0, W0, 0.5)


# ---------------------------------------------------------------------------------------------------------------------
# the per-entry tests
# ---------------------------------------------------------------------------------------------------------------------
SLAB_BYTES = 768 << 20
_RESULTS = {}
_T0 = [None]


@pytest.fixture(scope="module")
def slab():
    _T0[0] = time.time()
    s = fp.Slab(SLAB_BYTES, device="cuda")
    _range_tripped()  # the split-fp16 range guard is registered (as in the product) and clear before the first case
    yield s
    del s
    torch.cuda.empty_cache()


def _range_tripped():
    """Reads and clears the range guard's device flag (ops.check_range): True if a launch since the last call stored a value outside
    the fp16 range or a NaN.  Left set, it would raise in the next forward of any later test."""
    o = ops()
    try:
        o.check_range()
    except o.RangeError:
        return True
    return False


def gpu_record(fn, dry):
    """The model's own intervals for the real call: everything fn launches goes through hazard.recording()."""
    with hazard.recording(dry=dry, tables=getattr(fn, "tables", ())) as rec:
        fn()
    torch.cuda.synchronize()
    if not rec.launches:
        raise fp.FootprintError("the case launched nothing through the C ABI")
    if not dry and getattr(fn, "post", None):
        fn.post()
    return [x.reads for x in rec.launches], [x.writes for x in rec.launches], [x.name for x in rec.launches]


def run_case(slab, c, props="WOR"):
    o = ops()
    seen = []

    def record(fn, dry):
        rd, wr, names = gpu_record(fn, dry)
        seen.extend(names)
        return rd, wr
    with o.arith(c.mode):
        info = fp.check_case(slab, c.build, record, exempt=c.exempt, atomic=c.atomic, scratch=c.scratch, props=props, sync=torch.cuda.synchronize, label=c.id)
    assert set(seen) == {c.entry}, f"{c.id}: the case launched {sorted(set(seen))}, not its entry point alone"
    return info


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_footprint(slab, c):
    info = run_case(slab, c)
    info["mode"] = c.mode or "f16x3"
    info["range_guard"] = _range_tripped()
    assert not info["range_guard"], f"{c.id}: a case whose stored values are all finite and small tripped the fp16 range guard"
    _RESULTS[c.id] = (c, info)
    print(f"{c.id}: read {info['read_bytes']} written {info['written_bytes']} guard {info['guard_bytes']} untouched-in-buffers {info['pad_bytes']}")


# Controls that launch nothing wrong: the kernel runs unchanged on its real buffers, the MODEL is made to claim less.
@pytest.mark.gpu
def test_control_gemm_model_one_row_short_fails_w(slab, monkeypatch):
    c = next(c for c in CASES if c.id == "tce_gemm_f32-tile6464_ragged_130x70x96_gelu_res_a2")
    run_case(slab, c, props="W")
    real = hazard.MODELS["tce_gemm_f32"]

    def short(a):
        rd, wr = real(a)
        g = hazard._st(a[0])
        return rd, [hazard.strided(int(g.C), g.N * 4, (g.M - 1, g.ldc * 4))]
    monkeypatch.setitem(hazard.MODELS, "tce_gemm_f32", short)
    with pytest.raises(fp.FootprintError) as e:
        run_case(slab, c, props="W")
    print(e.value)
    assert "W violated" in str(e.value) and "C + " in str(e.value) and "(row 129, byte 0 " in str(e.value)
    _range_tripped()


@pytest.mark.gpu
def test_control_rowlin_model_without_bias_fails_r(slab, monkeypatch):
    c = next(c for c in CASES if c.id == "tce_rowlin_f32-1001x288x96_ln_in")
    run_case(slab, c, props="R")
    real = hazard.MODELS["tce_rowlin_f32"]

    def nobias(a):
        rd, wr = real(a)
        q = hazard._st(a[0])
        lo = int(q.bias)
        return [s for s in rd if not (len(s) and int(s[0, 0]) == lo)], wr
    monkeypatch.setitem(hazard.MODELS, "tce_rowlin_f32", nobias)
    with pytest.raises(fp.FootprintError) as e:
        run_case(slab, c, props="R")
    print(e.value)
    assert "R violated" in str(e.value) and "out + 0 bytes" in str(e.value)
    assert _range_tripped()  # the NaN bias reached the output: the guard saw it; cleared here so that later forwards start clean


# ---------------------------------------------------------------------------------------------------------------------
# The whole launch program on the capture topology
# ---------------------------------------------------------------------------------------------------------------------
OUT_KEYS = ("pred_logits", "pred_boxes", "pred_masks", "memory", "reference_points")
_PROGRAM = []


def _args(backbone):
    import argparse
    return argparse.Namespace(backbone=backbone, with_box_refine=True, binary=True, freeze_text_encoder=True, f_token=8,
                              qtrans=True, num_feature_levels=4, text_encoder_layers=1)


def _fresh_model(backbone, salt=5):
    from tce_rvos_amd import build_model, load_synth_weights
    m, _, _ = build_model(_args(backbone))
    m = m.cuda().eval()
    load_synth_weights(m, salt)
    m.repack()
    return m


def _frames(T, H, W, seed):
    from _util import synth_frames
    return synth_frames(T, H, W, seed).cuda()


def _ids(G, Ln, seed=3):
    return torch.randint(3, 50000, (G, Ln), generator=torch.Generator().manual_seed(seed)).cuda()


def _filled_arena(real, word):
    class Filled(real):
        """ops.Arena whose bytes hold `word` from construction on (a previous tenant's leftovers); the counters stay zero."""

        def __init__(self, device, nbytes):
            super().__init__(device, nbytes)
            n = self.buf.numel() // 4 * 4
            self.buf[:n].view(torch.int32).fill_(fp._i32(word))
            self.buf[n:].fill_(word & 0xFF)
    return Filled


# (tag, forward(model) -> list of output dicts); each is run three times: eager, capture, replay
def _single(T, H, W, Ln, valid=None):
    def go(model):
        from tce_rvos_amd import nested_tensor_from_videos_list
        ids = _ids(1, Ln)
        if valid is None:
            return [model([_frames(T, H, W, 11)], ids, [{"size": torch.tensor([H, W])}])]
        nt = nested_tensor_from_videos_list([_frames(T, valid[0], valid[1], 11)], size_divisibility=32)
        assert tuple(nt.tensors.shape[-2:]) == (H, W)
        return [model(nt, ids, [{"size": torch.tensor([H, W])}])]
    return go


def _group(G, T, H, W, lens, ragged):
    def go(model):
        clips = [_frames(T, H, W, 70 + i) for i in range(G)]
        ids = _ids(G, max(lens), seed=70)
        if ragged:
            for g, n in enumerate(lens):
                ids[g, n:] = model._pad_id()
        return model.forward_group(clips, ids, [{"size": torch.tensor([H, W])}], ragged=ragged)
    return go


PROGRAMS = {
    "swin_t_p4w7": [("small_3x96x132", _single(3, 96, 132, 9)),              # every un-fused form
                    ("config2_5x360x640", _single(5, 360, 640, 32)),         # BASELINE config 2: the fused forms
                    ("padded_3x96x160_valid_90x140", _single(3, 96, 160, 9, valid=(90, 140))),
                    ("caption_40_tokens_2x64x96", _single(2, 64, 96, 40)),   # un-folded text cross-attention
                    ("group2_3x96x132", _group(2, 3, 96, 132, (9, 9), False)),
                    ("group2_ragged_3x96x132", _group(2, 3, 96, 132, (9, 5), True))],
    "resnet50": [("small_1x96x128", _single(1, 96, 128, 9))],
    "video_swin_t_p4w7": [("small_4x96x128", _single(4, 96, 128, 9))],
}


@pytest.mark.gpu
@pytest.mark.parametrize("backbone", list(PROGRAMS))
def test_forward_does_not_depend_on_what_its_arenas_held(backbone, monkeypatch):
    """Arenas are torch.empty: a hole in an output, or a tile that reads rows not yet produced, shows as a dependence on the
    previous tenant's bytes.  Every arena of a freshly built model is filled with zero / quiet NaN / -1e38 at construction;
    eager pass, capture and replay of each program must give the same bits under all three."""
    from tce_rvos_amd import ops as o
    real = o.Arena
    ref = {}
    for fname, word in fp.FILLS:
        monkeypatch.setattr(o, "Arena", _filled_arena(real, word))
        model = _fresh_model(backbone)
        for tag, go in PROGRAMS[backbone]:
            graphs = len(model._graphs)
            for run in ("eager", "capture", "replay"):
                outs = go(model)
                torch.cuda.synchronize()
                got = [{k: out[k].clone() for k in OUT_KEYS} for out in outs]
                want = ref.setdefault(tag, got)
                for g, (a, b) in enumerate(zip(got, want)):
                    for k in OUT_KEYS:
                        assert a[k].shape == b[k].shape
                        same = torch.equal(a[k].view(torch.int32), b[k].view(torch.int32))
                        assert same, (f"{backbone} {tag} clip {g} {k}: '{fname}' fill / {run} differs from 'zero' fill / eager in "
                                      f"{int((a[k].view(torch.int32) != b[k].view(torch.int32)).sum())} of {a[k].numel()} words")
            assert len(model._graphs) > graphs, f"{tag}: no graph was captured for this program, the capture / replay legs ran eager"
            _PROGRAM.append(f"arena-content independence | {backbone} {tag} | fill {fname} | eager = capture = replay = zero-fill bits")
        monkeypatch.setattr(o, "Arena", real)
        del model
        torch.cuda.empty_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("tag,T,H,W,Ln", [("small_3x96x132", 3, 96, 132, 9), ("config2_5x360x640", 5, 360, 640, 32)])
def test_program_writes_stay_inside_the_recorded_writes(tag, T, H, W, Ln):
    """Program-level W: one pass recorded exactly as model.hazard_check records it, all five arenas filled with the canary
    after the warm-up pass.  Every arena byte outside the union of ALL recorded writes still holds the canary afterwards --
    so no kernel wrote outside its model, and no torch op outside the C ABI (which the checker cannot see) wrote arena memory
    -- and the split counters are all zero."""
    from tce_rvos_amd import ops as o
    model = _fresh_model("swin_t_p4w7")
    canary = fp.CANARIES[0]
    seen = {}

    def observe(phase, res, rec):
        arenas = [r for r in res if isinstance(r, o.Arena)]
        assert len(arenas) == 5
        if phase == "before":
            for a in arenas:
                n = a.buf.numel() // 4 * 4
                a.buf[:n].view(torch.int32).fill_(fp._i32(canary))
                assert int(a.flags.abs().max()) == 0
            return
        writes = hazard.union(*[x.writes for x in rec.launches])
        seen["launches"] = len(rec.launches)
        for i, a in enumerate(arenas):
            n = a.buf.numel() // 4 * 4
            base = a.buf.data_ptr()
            inside = np.clip(writes, base, base + n)
            seen[i] = (n, int((inside[:, 1] - inside[:, 0]).sum()))
            hit = fp.first_touched_outside(a.buf[:n], writes, canary)
            assert hit is None, (f"{tag}: arena {i}: {hit[1]} bytes outside every recorded write changed during the pass, first at "
                                 f"arena offset {hit[0]:#x}")
            assert int(a.flags.abs().max()) == 0, f"{tag}: arena {i}: split counters not zero after the pass"

    rep = model.hazard_check(_frames(T, H, W, 11), _ids(1, Ln), (H, W), observe=observe)
    assert rep.clean, str(rep)
    assert seen["launches"] > 200
    for i in range(5):
        _PROGRAM.append(f"program-level W | swin_t_p4w7 {tag} | arena {i}: {seen[i][0]} bytes, {seen[i][1]} inside recorded writes, "
                        f"the other {seen[i][0] - seen[i][1]} still canary; counters zero")


# ---------------------------------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "r08_footprint_by_entry.txt")


@pytest.mark.gpu
def test_zz_write_profile():
    """Writes the table of every case above (run the whole module)."""
    missing = [c.id for c in CASES if c.id not in _RESULTS]
    assert not missing, f"cases that did not run (or failed): {missing}"
    wall = time.time() - _T0[0]
    with open(PROFILE, "w") as f:
        f.write("# tests/test_footprint_gpu.py on an MI355X: every access model of hazard.MODELS against the bytes its kernel touches.\n"
                "# W: nothing outside the modelled writes changed (2 canaries); O: no canary left in a modelled output (workspaces /\n"
                "# counters listed under 'exempt' excepted); R: output bits equal with everything outside the modelled reads filled with\n"
                "# zero / quiet NaN / -1e38 ('atomic': finite and within 1e-4 rel + 1e-5 max|ref| instead).\n"
                "# 'untouched' = bytes inside the case's buffers that neither model covers (pad columns, batch gaps): checked by W and R.\n"
                f"# module wall time {wall:.0f} s ({len(CASES)} cases + whole-program tests); the rest of the GPU suite at the previous\n"
                "# commit: 154 s arithmetic bounds + 309 s everything else.\n"
                "# Found: no kernel failed W or O.  Models completed on the read side (R fails with the previous models of the first five):\n"
                "#   window attention 2-D / 3-D (relative position bias table), patch_embed (bias, gamma, beta), patch_merge_ln (gamma, beta),\n"
                "#   embed_ln / embed_ln_seqs (word, position, token-type tables), ms_deform_attn_backward (spatial shapes, level starts),\n"
                "#   resize_h_u8 / resize_v_norm (coefficient, bounds, LUT tables), ffn_fused_split (its counters must be zero: a read).\n"
                "#   Checked and left as they were: xattn's a2 (shared by the batch in the kernel), mha (32-wide heads are the ABI), mha_small64_*.\n"
                "# entry point | case | arithmetic | bytes read | bytes written | guard bytes | untouched | properties | exempt from O\n")
        for cid in sorted(_RESULTS):
            c, i = _RESULTS[cid]
            f.write(f"{c.entry} | {c.tag} | {i['mode']} | {i['read_bytes']} | {i['written_bytes']} | {i['guard_bytes']} | {i['pad_bytes']} | "
                    f"W x{i['W']} O x{i['O']} R x{i['R']}{' (atomic)' if c.atomic else ''} | {', '.join(i['exempt']) or '-'}"
                    f"{' | RANGE GUARD TRIPPED' if i['range_guard'] else ''}\n")
        f.write("# whole program\n")
        for line in _PROGRAM:
            f.write(line + "\n")
