"""GPU: every matrix-product kernel family against an fp64 reference on the CPU, element by element, under a bound that is derived from
the documented operand contract |x - hi - lo| <= max(2^-20 |x|, 2^-24) and the number formats (tests/_arith.py) -- not calibrated on
what the kernels return, and with no margin added.  Two input designs per family: a dense sweep over operand magnitudes, and a
K-block probe whose rows are non-zero in 8 consecutive k only, so that one wrong lo value at one k index, or one misplaced 8-half
fragment, is the whole of some output's error instead of 1/K of it.  tests/test_arith_bound_cpu.py shows on an emulation that the
correct arithmetic is inside these bounds on these inputs and each such defect is >= 4 x outside.

Every case appends (family, shape, scales, max err / sum|a||b|, max err / B) to a table the last test writes to
profiles/r07_arith_bound_by_family.txt."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

import _arith as A
from _attn import attention_ref_and_bound
from _window import bias_3d, to_windows2d, to_windows3d, windows_ref_and_bound

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "r07_arith_bound_by_family.txt")
RESULTS = []


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from tce_rvos_amd import ops as _ops
    return _ops


@pytest.fixture
def lib():
    from tce_rvos_amd._lib import lib as _lib
    return _lib()


@pytest.fixture(autouse=True)
def _range_flag_stays_clean(ops):
    ops.check_range()
    yield
    ops.check_range()   # no case may raise the range flag


def dev(t):
    return t.cuda().contiguous()


def tag(ws, as_):
    f = lambda v: "1" if v == 1 else f"2^{int(round(math.log2(v)))}"
    return f"w x {f(ws)}, a x {f(as_)}"


def check(family, shape, scales, out, ref, B, S, a=None, period=None, expect_outside=None):
    """Per-element |out - ref| <= B; records the case.  expect_outside: a second bound the result must EXCEED somewhere."""
    out, ref = out.detach().cpu().double().reshape(ref.shape), ref.double()
    err = (out - ref).abs().nan_to_num(nan=float("inf"))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / B)   # an exact result is inside any bound, B = 0 included
    rS = (err / S.clamp_min(1e-300)).max().item()
    i = int(ratio.argmax())
    rB = float(ratio.flatten()[i])
    RESULTS.append((family, shape, scales, rS, rB))
    if not bool((err <= B).all()):
        r, c = divmod(i, ref.shape[-1]) if ref.dim() == 2 else (i, 0)
        where = f"row {r}, column {c}"
        if period:
            where += f", row-in-tile {r % period}"
        if a is not None:
            nz = torch.nonzero(a.reshape(ref.shape[0], -1)[r])
            where += f", k-blocks of the row {sorted(set((nz.flatten() // 8).tolist()))[:12]}"
        n_bad = int((err > B).sum())
        raise AssertionError(f"{family} {shape} [{scales}]: {n_bad} of {err.numel()} elements outside the bound; worst err/B = {rB:.3g} "
                             f"(err {float(err.flatten()[i]):.3e}, ref {float(ref.flatten()[i]):.3e}) at {where}")
    if expect_outside is not None:
        assert bool((err > expect_outside).any()), f"{family} {shape} [{scales}]: single-pass mode is inside the three-product bound"
    return rB


def linear_cases(M, N, K, period, seed, probe=True, probe_rows=None, dense=True, scales=A.DENSE_SCALES, decades=True):
    """(kind, scales tag, a [rows, K], w [N, K], c) for one linear family at one shape."""
    if dense:
        for j, (ws, as_) in enumerate(scales):
            a, w = A.dense_operands(M, N, K, ws, as_, seed * 16 + j)
            yield "dense", tag(ws, as_), a, w, A.c_dense(K)
        if decades:
            a, w = A.decades_operands(M, N, K, seed * 16 + 9)
            yield "dense", "4 decades along K", a, w, A.c_dense(K)
    if probe and K % 8 == 0:
        Mp = A.probe_rows(K, period) if probe_rows is None else probe_rows
        for j, (ws, as_) in enumerate(A.PROBE_SCALES):
            a = A.kblock_probe(Mp, K, as_, period, seed * 16 + 10 + j)
            _, w = A.dense_operands(1, N, K, ws, 1.0, seed * 16 + 13 + j)
            yield "probe", tag(ws, as_), a, w, A.c_probe(a)


def run_linear(family, shape, fn, M, N, K, period, seed, f16=None, **kw):
    """fn(a, w) -> out [rows, N] on the device (any row count).  f16 = ops: the probe again in mode "f16".  shape(rows): the label
    of a case, from the row count it really runs (the probe's differs from the dense sweep's)."""
    label = shape
    for kind, sc, a, w, c in linear_cases(M, N, K, period, seed, **kw):
        shape = label(a.shape[0])
        ref, S = a.double() @ w.double().T, A.sum_abs(a, w)
        out = fn(a, w)
        torch.cuda.synchronize()
        check(f"{family} {kind}", shape, sc, out, ref, A.bound_split(a, w, c, S), S, a if kind == "probe" else None, period)
        if f16 is not None and kind == "probe":
            with f16.arith("f16"):
                out = fn(a, w)
                torch.cuda.synchronize()
            # the floor 2^-24 makes the two bounds meet where both operands' errors are floor-dominated; the switch must show at (1, 1)
            check(f"{family} probe mode f16", shape, sc, out, ref, A.bound_f16(a, w, c, S), S, a, period,
                  expect_outside=A.bound_split(a, w, c, S) if sc == tag(1, 1) else None)


def chunked(fn, rows):
    """Families with few rows by nature: a long probe is run as several launches of `rows` rows (the block shifts from launch to
    launch, see _arith.probe_blocks with period = rows)."""
    def go(a, w):
        return torch.cat([fn(a[i:i + rows], w) for i in range(0, a.shape[0], rows)], 0)
    return go


def few_row_probe_rows(M, K):
    return M * -(-(K // 8) // M)


# ---------------------------------------------------------------------------------------------------------------
# Tiled GEMM
# ---------------------------------------------------------------------------------------------------------------
GEMM_SHAPES = [(25, 256, 256), (130, 70, 96), (300, 384, 96), (1200, 2048, 256), (4097, 96, 384), (513, 2153, 256), (3333, 1000, 160),
               (24100, 256, 64), (1024, 512, 2048), (8192, 512, 1024), (12288, 1024, 384)]


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_tiled(ops, lib, M, N, K):
    """ops.gemm over the small tile and the persistent 128 / 256 tiles (single and split walk); the tile code the launcher picks is
    part of the recorded shape.  The probe runs in mode "f16" too: inside the single-pass bound and outside the three-product one."""
    fn = lambda a, w: ops.gemm(dev(a), dev(w))
    run_linear("gemm", lambda m: f"{m}x{N}x{K} tile {lib.tce_gemm_select_tile_ex(m, N, K, 1, 0)}", fn, M, N, K, 256, M + N + K, f16=ops,
               probe_rows=max(M, A.probe_rows(K, 256) + M % 256))


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_exact_fp32_validates_the_dense_accumulation_model(ops, M, N, K):
    """The dense c = sqrt(3 K) is a model, not a bound: the exact-fp32 MFMA kernel (mode "f32", the reference arithmetic, not a
    kernel under test here) must stay within bound_acc ALONE with a factor 2 of room on every dense case."""
    for kind, sc, a, w, c in linear_cases(M, N, K, 256, M + N + K, probe=False):
        with ops.arith("f32"):
            out = ops.gemm(dev(a), dev(w))
        ref = a.double() @ w.double().T
        r = check("gemm mode f32 (model validation)", f"{M}x{N}x{K}", sc, out, ref, A.bound_acc(a, w, c), A.sum_abs(a, w))
        assert r <= 0.5, f"exact fp32 at {r:.2f} of bound_acc: DENSE_C_FACTOR must be raised"


@pytest.mark.parametrize("batch,M,N,K", [(5, 3600, 256, 256), (3, 333, 160, 256)])
def test_gemm_ex_strided_batched(ops, batch, M, N, K):
    """gemm_ex: frames of a wider [batch, M + pad, 2K] buffer (row pitch 2K, A a column slice), output into a level slice."""
    def fn(a, w):
        rows = a.shape[0]
        m = rows // batch
        wide = torch.zeros(batch, m + 7, 2 * K)
        wide[:, :m, K:] = a.view(batch, m, K)
        dw, out = dev(wide), torch.zeros(batch, m + 50, N, device="cuda")
        ops.gemm_ex(dw[:, :, K:], dev(w), out[:, 50:], m, N, K, 2 * K, K, N, batch=batch, sA=(m + 7) * 2 * K, sC=(m + 50) * N)
        assert float(out[:, :50].abs().max()) == 0.0
        return out[:, 50:].reshape(rows, N)
    run_linear("gemm_ex strided", lambda m: f"{batch}x{m // batch}x{N}x{K}", fn, batch * M, N, K, 256, 3 + M, probe_rows=batch * (8192 // batch // 8 * 8))


@pytest.mark.parametrize("B,M,N,K", [(3, 333, 160, 256), (5, 4820, 384, 256)])
def test_gemm_batched(ops, B, M, N, K):
    for kind, sc, a, w, c in linear_cases(B * M, B * N, K, 256, B + M, probe_rows=B * M):
        a3, w3 = a.view(B, M, K), w.view(B, N, K)
        out = ops.gemm_batched(dev(a3), dev(w3), torch.empty(B, M, N, device="cuda")).cpu()
        for b in range(B):
            check(f"gemm_batched {kind}", f"{B}x{M}x{N}x{K}", sc, out[b], a3[b].double() @ w3[b].double().T,
                  A.bound_split(a3[b], w3[b], c[b * M:(b + 1) * M] if torch.is_tensor(c) else c), A.sum_abs(a3[b], w3[b]),
                  a3[b] if kind == "probe" else None, 256)


# ---------------------------------------------------------------------------------------------------------------
# Split-K GEMM + reduce
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,splits", [(32, 768, 3072, 16), (32, 2304, 768, 4), (25, 256, 2048, 8), (100, 2152, 512, 4)])
def test_gemm_splitk(ops, M, N, K, splits):
    """The reduce adds `splits` fp32 partial planes: `splits` more roundings against sum|a||b|, added to c."""
    def fn(a, w):
        m = a.shape[0]
        return ops.gemm_ex(dev(a), dev(w), torch.empty(m, N, device="cuda"), m, N, K, K, K, N, splitk=splits,
                           ws=torch.empty(splits * m * N, device="cuda"))
    for kind, sc, a, w, c in linear_cases(M, N, K, M, M + K, probe_rows=few_row_probe_rows(M, K)):
        out = chunked(fn, M)(a, w)
        check(f"gemm split-K {kind}", f"{M}x{N}x{K} / {splits}" + (f", {a.shape[0] // M} launches" if a.shape[0] > M else ""), sc, out, a.double() @ w.double().T, A.bound_split(a, w, c + splits),
              A.sum_abs(a, w), a if kind == "probe" else None, M)


@pytest.mark.parametrize("M,N,K,splits", [(32, 768, 3072, 16), (25, 256, 2048, 8), (40, 1024, 512, 2)])
def test_gemm_splitk_layernorm_reduce(ops, M, N, K, splits):
    g = torch.Generator().manual_seed(K)
    gam, bet = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 0.2
    b, res = torch.randn(N, generator=g) * 0.2, torch.randn(M, N, generator=g)
    for kind, sc, a, w, c in linear_cases(M, N, K, M, M + K + 1, probe=False):
        buf = dev(res).clone()
        ops.gemm_ex(dev(a), dev(w), buf, M, N, K, K, K, N, bias=dev(b), res=buf, ldres=N, res_mode=ops.RES_ADD, splitk=splits,
                    ws=torch.empty(splits * M * N, device="cuda"), ln=(dev(gam), dev(bet)), ln_eps=1e-12)
        z = a.double() @ w.double().T + b.double() + res.double()
        assert A.layernorm_sigma(z).min().item() > 1e-3
        Bz = A.bound_split(a, w, c + splits) + 2 * A.bound_bias(z)
        ref = F.layer_norm(z, (N,), gam.double(), bet.double(), 1e-12)
        check("gemm split-K + LayerNorm reduce", f"{M}x{N}x{K} / {splits}", sc, buf, ref, 2 * A.ln_tail(z, Bz, gam, bet, 1e-12),
              A.sum_abs(a, w))


# ---------------------------------------------------------------------------------------------------------------
# Implicit-GEMM convolution
# ---------------------------------------------------------------------------------------------------------------
def conv_cases(T, H, W, Cin, N, k, seed, probe_frames=None):
    for kind, ws, as_, Tn, x, w in A.conv_cases(T, H, W, Cin, N, k, seed, probe_frames):
        yield kind, ("4 decades along K" if ws is None else tag(ws, as_)), Tn, x, w, ("probe" if kind == "probe" else None)


im2col = A.im2col


@pytest.mark.parametrize("T,H,W,Cin,N,k,s,p,splits", [(2, 9, 13, 32, 48, 3, 1, 1, 1), (3, 12, 20, 64, 256, 3, 2, 1, 1), (2, 7, 5, 16, 33, 1, 1, 0, 1),
                                                     (2, 14, 10, 256, 512, 1, 2, 0, 1), (4, 45, 81, 64, 250, 3, 1, 1, 1), (5, 45, 80, 64, 256, 3, 1, 1, 1),
                                                     (5, 12, 20, 768, 256, 3, 2, 1, 8), (1, 9, 7, 64, 96, 3, 1, 1, 3)])
def test_conv_implicit_gemm(ops, T, H, W, Cin, N, k, s, p, splits):
    for kind, sc, Tn, x, w, pr in conv_cases(T, H, W, Cin, N, k, T + H + N):
        a = im2col(x, Tn, H, W, Cin, k, s, p)
        M = a.shape[0]
        ws_ = torch.empty(splits * M * N, device="cuda") if splits > 1 else None
        out, _, _ = ops.conv2d_cl(dev(x), dev(w), Tn, H, W, Cin, k, k, s, p, splitk=splits, ws=ws_)
        c = (A.c_probe(a) if pr else A.c_dense(k * k * Cin)) + (splits if splits > 1 else 0)
        check(f"conv2d_cl {kind}", f"{Tn}x{H}x{W} {Cin}->{N} {k}x{k}/s{s}" + (f" split-K {splits}" if splits > 1 else ""), sc, out,
              a.double() @ w.double().T, A.bound_split(a, w, c), A.sum_abs(a, w), a if pr else None, 128)


# ---------------------------------------------------------------------------------------------------------------
# rowlin
# ---------------------------------------------------------------------------------------------------------------
ROWLIN_SHAPES = [(7200, 288, 96), (129, 32, 96), (1000, 576, 192), (24100, 256, 256), (4600, 384, 384), (200, 256, 384), (16200, 512, 512),
                 (130, 256, 512)]


@pytest.mark.parametrize("M,N,K", ROWLIN_SHAPES)
def test_rowlin_plain(ops, M, N, K):
    def fn(a, w):
        pk = ops.rowlin_pack(dev(w))     # packed in the arithmetic mode under test
        return ops.rowlin(dev(a), pk, torch.empty(a.shape[0], N, device="cuda"), a.shape[0], N, K, K, N)
    # the probe also runs at the shape's own (possibly ragged) row count when that is the larger
    run_linear("rowlin", lambda m: f"{m}x{N}x{K}", fn, M, N, K, 256, M + N + K, f16=ops, probe_rows=max(M, A.probe_rows(K, 256) + M % 256))


ROWLIN_TAILS = [(M, N, K, v) for (M, N, K) in [(7200, 288, 96), (1000, 576, 192), (24100, 256, 256), (4600, 384, 384), (130, 256, 512),
                                               (1000, 256, 192), (333, 256, 96)]
                for v in ("ln_in", "gelu_res", "ln_out") if v != "ln_out" or (N == 256 and K != 512)]   # ln_out: built for N = 256, K < 512


@pytest.mark.parametrize("M,N,K,variant", ROWLIN_TAILS)
def test_rowlin_tails(ops, M, N, K, variant):
    """Composed first-order bounds (x 2 for the remainder).  gelu_res leaves out the (2^4, 2^4) point and the four-decade rows, whose
    GELU arguments (standard deviation 256 / 30) lie far beyond +-6."""
    g = torch.Generator().manual_seed(M + K)
    b, res = torch.randn(N, generator=g) * 0.3, torch.randn(M, N, generator=g)
    gi, bi = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.2
    go, bo = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 0.2
    scales = [s for s in A.DENSE_SCALES if not (variant == "gelu_res" and s[0] > 1)]
    for kind, sc, a, w, c in linear_cases(M, N, K, 256, M + N + K + 5, probe=False, scales=scales, decades=(variant != "gelu_res")):
        pk = ops.rowlin_pack(dev(w))
        out = torch.empty(M, N, device="cuda")
        kw = dict(bias=dev(b))
        a64, w64 = a.double(), w.double()
        if variant == "ln_in":
            assert A.layernorm_sigma(a).min().item() > 1e-3
            kw.update(ln_in=(dev(gi), dev(bi)))
            y = F.layer_norm(a64, (K,), gi.double(), bi.double(), 1e-5)
            ref = y @ w64.T + b.double()
            B = A.bound_split(y, w, c) + A.chain(A.ln_eval_bound(a, gi, bi, 1e-5), w) + A.bound_bias(ref)
            S = A.sum_abs(y, w)
        elif variant == "gelu_res":
            kw.update(act=ops.ACT_GELU, res=dev(res), ldres=N, res_mode=ops.RES_ADD)
            z = a64 @ w64.T + b.double()
            assert z.abs().max().item() < 6.0
            ref = F.gelu(z) + res.double()
            B = A.GELU_LIPSCHITZ * (A.bound_split(a, w, c) + A.bound_bias(z)) + A.gelu_eval_bound(z) + A.bound_bias(ref)
            S = A.sum_abs(a, w)
        else:
            kw.update(res=dev(res), ldres=N, res_mode=ops.RES_ADD, ln_out=(dev(go), dev(bo)))
            z = a64 @ w64.T + b.double() + res.double()
            assert A.layernorm_sigma(z).min().item() > 1e-3
            ref = F.layer_norm(z, (N,), go.double(), bo.double(), 1e-5)
            B = A.ln_tail(z, A.bound_split(a, w, c) + 2 * A.bound_bias(z), go, bo, 1e-5)
            S = A.sum_abs(a, w)
        ops.rowlin(dev(a), pk, out, M, N, K, K, N, **kw)
        check(f"rowlin {variant}", f"{M}x{N}x{K}", sc, out, ref, 2 * B, S)


# ---------------------------------------------------------------------------------------------------------------
# Fused FFN
# ---------------------------------------------------------------------------------------------------------------
def ffn_launch(ops, x, w1, b1, w2, b2, Hd, act, ln_in, ln_out, split=False):
    pk = ops.ffn_pack(dev(w1), dev(b1), dev(w2))
    xd = dev(x)
    out = torch.empty_like(xd)
    kw = dict(ln_in=(dev(ln_in[0]), dev(ln_in[1])) if ln_in else None, ln_out=(dev(ln_out[0]), dev(ln_out[1])) if ln_out else None)
    a = ops.ACT_RELU if act == "relu" else ops.ACT_GELU
    if split:
        nws, ncnt = ops.ffn_split_need(x.shape[0], x.shape[1], Hd, a)
        assert nws > 0, "no split planned at this shape"
        kw["split"] = (torch.empty(nws, device="cuda"), torch.zeros(ncnt, dtype=torch.int32, device="cuda"))
    ops.ffn_fused(xd, pk, dev(b2), Hd, a, out=out, **kw)
    torch.cuda.synchronize()
    return out


FFN_DENSE = [(4600, 96, 384, "gelu", "in", ""), (1201, 128, 512, "gelu", "in", ""), (4600, 192, 768, "gelu", "in", ""),
             (4100, 256, 2048, "relu", "out", ""), (333, 256, 64, "relu", "none", ""), (333, 256, 64, "gelu", "none", ""),
             (4100, 256, 2048, "relu", "none", ""), (4600, 256, 2048, "relu", "out", "split"), (3000, 96, 384, "gelu", "in", "half"),
             (3000, 128, 512, "gelu", "none", "half")]


@pytest.mark.parametrize("M,C,Hd,act,ln,form", FFN_DENSE)
def test_ffn_dense(ops, lib, M, C, Hd, act, ln, form):
    """GELU cases leave out the (2^4, 2^4) point and the four-decade rows (hidden arguments far beyond +-6)."""
    for j, (ws, as_) in enumerate(A.DENSE_SCALES + ((None, None),)):
        if act == "gelu" and (ws is None or ws > 1):
            continue
        g = torch.Generator().manual_seed(M + C + Hd + j)
        decades = ws is None
        if decades:   # four decades of range along the channels of x
            ws, as_ = 1.0, 1.0
        x = torch.randn(M, C, generator=g) * as_ * (torch.logspace(-2, 2, C)[None, :] if decades else 1.0)
        w1, b1 = torch.randn(Hd, C, generator=g) / math.sqrt(C) * ws, torch.randn(Hd, generator=g) * 0.2 * ws * as_
        w2, b2 = torch.randn(C, Hd, generator=g) / math.sqrt(Hd) * ws, torch.randn(C, generator=g) * 0.2 * as_
        gam, bet = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
        ln_in, ln_out = ((gam, bet) if ln == "in" else None), ((gam, bet) if ln == "out" else None)
        ref, B, S, h = A.ffn_ref_and_bound(x, w1, b1, w2, b2, act, ln_in, ln_out, A.c_dense(C), A.c_dense(Hd))
        if ln_in is not None:
            assert A.layernorm_sigma(x).min().item() > 1e-3
        if act == "gelu":
            assert h.abs().max().item() < 6.0
        if form == "half":
            lib.tce_debug_ffn_set_half(1)
        try:
            out = ffn_launch(ops, x, w1, b1, w2, b2, Hd, act, ln_in, ln_out, split=(form == "split"))
        finally:
            lib.tce_debug_ffn_set_half(0)
        check(f"ffn {act} ln={ln}" + (f" ({form})" if form else ""), f"{M}x{C}x{Hd}", "4 decades along K" if decades else tag(ws, as_), out, ref, B, S)


@pytest.mark.parametrize("C,Hd", [(96, 384), (128, 512), (192, 768), (256, 2048)])
@pytest.mark.parametrize("act", ["relu", "gelu"])
def test_ffn_dense_single_pass(ops, C, Hd, act):
    """Mode "f16" on dense rows, both activations, every width: every element inside the single-pass composed bound."""
    g = torch.Generator().manual_seed(C + Hd)
    M = 3000
    x = torch.randn(M, C, generator=g)
    w1, b1 = torch.randn(Hd, C, generator=g) / math.sqrt(C), torch.randn(Hd, generator=g) * 0.2
    w2, b2 = torch.randn(C, Hd, generator=g) / math.sqrt(Hd), torch.randn(C, generator=g) * 0.2
    ref, B, S, h = A.ffn_ref_and_bound(x, w1, b1, w2, b2, act, None, None, A.c_dense(C), A.c_dense(Hd), first=A.bound_f16, second=A.bound_f16)
    assert h.abs().max().item() < 6.0
    with ops.arith("f16"):
        out = ffn_launch(ops, x, w1, b1, w2, b2, Hd, act, None, None)
    check(f"ffn {act} mode f16", f"{M}x{C}x{Hd}", tag(1, 1), out, ref, B, S)


FFN_PROBE = [(96, 384, ""), (128, 512, ""), (192, 768, ""), (256, 2048, ""), (256, 64, ""), (256, 2048, "split"), (96, 384, "half")]


@pytest.mark.parametrize("C,Hd,form", FFN_PROBE)
@pytest.mark.parametrize("which", ["first", "second"])
def test_ffn_probe(ops, lib, C, Hd, form, which):
    """The operands of _arith.ffn_probe_operands: K-block rows into the first product (observed through a 0 / 1 selection as W2), or
    into the second (through a 0 / 1 selection as W1); one launch per C hidden units.  The plain form also runs in mode "f16"."""
    period = 256
    M = 4600 if form == "split" else A.probe_rows(C, period)
    launches = max(1, Hd // C)
    act = "gelu" if form == "half" else "relu"   # the half-workgroup form is the GELU MLP's; every hidden value is >= 0 and < 6
    for j, (ws, as_) in enumerate(A.PROBE_SCALES):
        for l in range(launches):
            x, w1, b1, w2, b2, c1, c2 = A.ffn_probe_operands(which, C, Hd, M, period, ws, as_, seed=C + Hd + j, launch=l)
            ref, B, S, h = A.ffn_ref_and_bound(x, w1, b1, w2, b2, act, None, None, c1, c2)
            assert 0.0 <= h.min().item() and h.max().item() < 6.0
            outs = {}
            for mode in ("f16x3", "f16") if form == "" else ("f16x3",):
                if form == "half":
                    lib.tce_debug_ffn_set_half(1)
                try:
                    with ops.arith(mode):
                        outs[mode] = ffn_launch(ops, x, w1, b1, w2, b2, Hd, act, None, None, split=(form == "split"))
                finally:
                    lib.tce_debug_ffn_set_half(0)
            name = f"ffn probe {which} product" + (f" ({form})" if form else "")
            check(name, f"{M}x{C}x{Hd}", tag(ws, as_), outs["f16x3"], ref, B, S, x, period)
            if "f16" in outs:
                _, B16, _, _ = A.ffn_ref_and_bound(x, w1, b1, w2, b2, "relu", None, None, c1, c2, first=A.bound_f16, second=A.bound_f16)
                check(name + " mode f16", f"{M}x{C}x{Hd}", tag(ws, as_), outs["f16"], ref, B16, S, x, period,
                      expect_outside=B if (ws, as_) == (1.0, 1.0) else None)


# ---------------------------------------------------------------------------------------------------------------
# 3x3 pixel-stationary convolution and its split entry
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture
def conv3_debug(lib):
    yield lib
    lib.tce_debug_conv3x3_set_pieces(0)
    lib.tce_debug_conv3x3_set_waves(0)


@pytest.mark.parametrize("waves,pieces", [(4, -1), (8, -1), (0, -1), (0, 0), (0, 5), (4, 2)])
@pytest.mark.parametrize("T,H,W", [(2, 32, 40), (3, 17, 5)])
def test_conv3x3(ops, conv3_debug, T, H, W, waves, pieces):
    """pieces = -1: tce_conv3x3_f32; otherwise tce_conv3x3_split_f32 at the plan's own (0) or a forced piece count.  The reduce adds
    the pieces' fp32 partials: as many more roundings.  Probe (on the small frame size): 32 frames, frame t holds channel block t only.
    The forced wave counts also run the probe in mode "f16"."""
    lib = conv3_debug
    for kind, sc, Tn, x, w, pr in conv_cases(T, H, W, 256, 256, 3, H + W + waves, probe_frames=32):
        if kind == "probe" and (H, W) != (17, 5):
            continue
        a = im2col(x, Tn, H, W, 256, 3, 1, 1)
        M = a.shape[0]
        ref, S = a.double() @ w.double().T, A.sum_abs(a, w)
        for mode in ("f16x3", "f16") if (pr and pieces == -1 and waves != 0) else ("f16x3",):
            with ops.arith(mode):
                pk = ops.conv3x3_pack(dev(w), 256)
                lib.tce_debug_conv3x3_set_waves(waves)
                lib.tce_debug_conv3x3_set_pieces(max(pieces, 0))
                xd, extra = dev(x), 0
                if pieces < 0:
                    out = ops.conv3x3(xd, pk, Tn, H, W, 256, 256)
                else:
                    extra = int(lib.tce_conv3x3_split_pieces(M, 256, 256))
                    assert pieces == 0 or extra == pieces
                    nws = max(1, int(lib.tce_conv3x3_split_ws_floats(M, 256, 256)))
                    wsb, out = torch.full((nws,), float("nan"), device="cuda"), torch.full((M, 256), float("nan"), device="cuda")
                    rc = lib.tce_conv3x3_split_f32(xd.data_ptr(), 256, pk.data_ptr(), None, out.data_ptr(), 256, Tn, H, W, 256, 256,
                                                   wsb.data_ptr(), nws, torch.cuda.current_stream().cuda_stream)
                    assert rc == 0
                torch.cuda.synchronize()
            c = (A.c_probe(a) if pr else A.c_dense(2304)) + extra
            name = f"conv3x3 {kind} waves={waves}" + (f" split pieces={pieces}" if pieces >= 0 else "")
            if mode == "f16x3":
                check(name, f"{Tn}x{H}x{W}", sc, out, ref, A.bound_split(a, w, c, S), S, a if pr else None, 128)
            else:
                check(name + " mode f16", f"{Tn}x{H}x{W}", sc, out, ref, A.bound_f16(a, w, c, S), S, a, 128,
                      expect_outside=A.bound_split(a, w, c, S) if sc == tag(1, 1) else None)


# ---------------------------------------------------------------------------------------------------------------
# Thin weight streams
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(32, 2304, 768), (32, 768, 3072), (7, 768, 768), (100, 3072, 768)])
def test_thin_stream(ops, M, N, K):
    """Partial planes finished by splitk_reduce (K / 256 more fp32 additions)."""
    splits = K // 256

    def fn(a, w):
        m = a.shape[0]
        assert ops.thin_splits(m, N, K) == splits
        ws = ops.thin_partials(dev(a), dev(w), torch.empty(splits, m, N, device="cuda"), m, N, K)
        return ops.splitk_reduce(ws, splits, m, N, torch.empty(m, N, device="cuda"))
    for kind, sc, a, w, c in linear_cases(M, N, K, M, M + K + 2, probe_rows=few_row_probe_rows(M, K)):
        out = chunked(fn, M)(a, w)
        check(f"thin stream {kind}", f"{M}x{N}x{K}" + (f", {a.shape[0] // M} launches" if a.shape[0] > M else ""), sc, out, a.double() @ w.double().T, A.bound_split(a, w, c + splits), A.sum_abs(a, w),
              a if kind == "probe" else None, M)


@pytest.mark.parametrize("M,N,K", [(32, 768, 768), (32, 3072, 768)])
def test_thin_stream_planes_as_next_x(ops, M, N, K):
    """y = GELU(x W^T + b) W2^T with the first layer's planes finished on load by the second launch."""
    N2 = 64
    for j, (ws_, as_) in enumerate(A.DENSE_SCALES[:4]):   # (2^4, 2^4): GELU arguments beyond +-6
        g = torch.Generator().manual_seed(N + j)
        x, w = A.dense_operands(M, N, K, ws_, as_, N + j)
        b = torch.randn(N, generator=g) * 0.3 * ws_ * as_
        w2 = torch.randn(N2, N, generator=g) / math.sqrt(N)
        s1, s2 = K // 256, N // 256
        ws1 = ops.thin_partials(dev(x), dev(w), torch.empty(s1, M, N, device="cuda"), M, N, K)
        ws2 = ops.thin_partials(ws1, dev(w2), torch.empty(s2, M, N2, device="cuda"), M, N2, N, xsplits=s1, bias_x=dev(b), act_x=ops.ACT_GELU)
        out = ops.splitk_reduce(ws2, s2, M, N2, torch.empty(M, N2, device="cuda"))
        z = x.double() @ w.double().T + b.double()
        assert z.abs().max().item() < 6.0
        h = F.gelu(z)
        Bh = A.GELU_LIPSCHITZ * (A.bound_split(x, w, A.c_dense(K) + s1) + A.bound_bias(z)) + A.gelu_eval_bound(z)
        B = 2 * (A.chain(Bh, w2) + A.bound_split(h, w2, A.c_dense(N) + s2))
        check("thin stream, planes as the next x", f"{M}x{N}x{K} -> {N2}", tag(ws_, as_), out, h @ w2.double().T, B, A.sum_abs(h, w2))


# ---------------------------------------------------------------------------------------------------------------
# Exact-fp32 VALU: fewrow_linear
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,N,K", [(40, 384, 256), (25, 300, 256), (1, 256, 256), (64, 256, 256), (32, 384, 768), (7, 300, 96)])
def test_fewrow_linear_exact_fp32(ops, R, N, K):
    def fn(a, w):
        out = torch.full((a.shape[0], N), float("nan"), device="cuda")
        ops.fewrow_linear(dev(a), a.shape[0], K, [(dev(w), None, out, N, N, False, ops.FR_NONE)])
        return out
    for kind, sc, a, w, c in linear_cases(R, N, K, R, R + K, probe_rows=few_row_probe_rows(R, K)):
        out = chunked(fn, R)(a, w)
        check(f"fewrow_linear {kind}", f"{R}x{N}x{K}" + (f", {a.shape[0] // R} launches" if a.shape[0] > R else ""), sc, out, a.double() @ w.double().T, A.bound_f32(a, w), A.sum_abs(a, w),
              a if kind == "probe" else None, R)


# ---------------------------------------------------------------------------------------------------------------
# Patch embedding
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,H,W,C", [(2, 72, 100, 96), (1, 30, 41, 128), (1, 37, 50, 192)])
def test_patch_embed(ops, T, H, W, C):
    """4x4 / stride 4 patches (K = 48) + bias + LayerNorm; ragged H / W are zero-padded."""
    for j, (ws, as_) in enumerate(A.DENSE_SCALES + ((None, None),)):
        g = torch.Generator().manual_seed(H + C + j)
        decades = ws is None
        if decades:
            ws, as_ = 1.0, 1.0
        x = torch.randn(T, 3, H, W, generator=g) * as_
        if decades:   # four decades along K = (channel, row in patch, column in patch)
            sc48 = torch.logspace(-2, 2, 48).view(3, 4, 4)
            x = x * sc48.repeat(1, (H + 3) // 4, (W + 3) // 4)[None, :, :H, :W]
        w, b = torch.randn(C, 3, 4, 4, generator=g) / math.sqrt(48) * ws, torch.randn(C, generator=g) * 0.2 * ws * as_
        ga, be = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
        xp = F.pad(x, (0, (4 - W % 4) % 4, 0, (4 - H % 4) % 4))
        a = F.unfold(xp, 4, stride=4).transpose(1, 2).reshape(-1, 48)      # column order (c, ky, kx) = the weight's flattening
        wm = w.reshape(C, 48)
        z = a.double() @ wm.double().T + b.double()
        assert A.layernorm_sigma(z).min().item() > 1e-3
        ref = F.layer_norm(z, (C,), ga.double(), be.double(), 1e-5)
        B = 2 * A.ln_tail(z, A.bound_split(a, wm, A.c_dense(48)) + A.bound_bias(z), ga, be, 1e-5)
        out, _, _ = ops.patch_embed(dev(x), dev(w), dev(b), dev(ga), dev(be))
        check("patch_embed", f"{T}x{H}x{W} -> {C}", "4 decades along K" if decades else tag(ws, as_), out, ref, B, A.sum_abs(a, wm))
        if (ws, as_) == (1.0, 1.0) and not decades:
            with ops.arith("f16"):
                out16, _, _ = ops.patch_embed(dev(x), dev(w), dev(b), dev(ga), dev(be))
            B16 = 2 * A.ln_tail(z, A.bound_f16(a, wm, A.c_dense(48)) + A.bound_bias(z), ga, be, 1e-5)
            check("patch_embed mode f16", f"{T}x{H}x{W} -> {C}", tag(ws, as_), out16, ref, B16, A.sum_abs(a, wm), expect_outside=B)


# ---------------------------------------------------------------------------------------------------------------
# Attention cores (unit scale, composed softmax bound)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,H,W,nH,shift", [(2, 18, 25, 3, 0), (2, 18, 25, 3, 3), (1, 9, 13, 6, 3), (1, 7, 7, 1, 3), (1, 14, 21, 2, 0)])
def test_window_attn(ops, T, H, W, nH, shift):
    """2-D window attention core on a given qkv tensor (padding rows hold the qkv bias), relative-position bias, -100 shift mask."""
    from oracle import tce_oracle as O
    g = torch.Generator().manual_seed(H * W + shift)
    C = nH * 32
    qkv, qb = torch.randn(T * H * W, 3 * C, generator=g), torch.randn(3 * C, generator=g) * 0.3
    table = torch.randn(169, nH, generator=g)
    win, back, (Hp, Wp) = to_windows2d(qkv, T, H, W, shift, qb)
    bias = table[O.rel_pos_index(7).view(-1)].view(49, 49, nH).permute(2, 0, 1)
    mask = O.shift_attn_mask(Hp, Wp, 7, 3) if shift else None
    ref, B, S = windows_ref_and_bound(win, nH, bias, mask)
    out = ops.window_attn(dev(qkv), dev(qb), dev(table), T, H, W, C, nH, shift)
    check("window_attn", f"{T}x{H}x{W} C={C} shift={shift}", tag(1, 1), out, back(ref), back(B), back(S))


@pytest.mark.parametrize("T,H,W,nH,shifted", [(3, 18, 25, 3, False), (3, 18, 25, 3, True), (9, 9, 13, 2, True), (8, 16, 23, 2, False),
                                               (8, 16, 23, 2, True), (16, 14, 7, 1, True)])
def test_window_attn3d(ops, T, H, W, nH, shifted):
    """3-D (8, 7, 7) window attention core on a given qkv tensor."""
    g = torch.Generator().manual_seed(T * H + W)
    C = nH * 32
    qkv, qb = torch.randn(T * H * W, 3 * C, generator=g), torch.randn(3 * C, generator=g) * 0.3
    table = torch.randn(15 * 13 * 13, nH, generator=g)
    win, back, mask, N = to_windows3d(qkv, T, H, W, shifted, qb)
    ref, B, S = windows_ref_and_bound(win, nH, bias_3d(table, nH, N), mask)
    out = ops.window_attn3d(dev(qkv), dev(qb), dev(table), T, H, W, C, nH, shifted)
    check("window_attn3d", f"{T}x{H}x{W} C={C} shifted={shifted}", tag(1, 1), out, back(ref), back(B), back(S))


@pytest.mark.parametrize("T,H,W,C,shift", [(2, 18, 25, 96, 0), (2, 18, 25, 96, 3), (1, 9, 13, 192, 3), (1, 7, 7, 128, 3), (1, 14, 21, 256, 0),
                                            (1, 23, 40, 256, 3)])
def test_swin_attn_fused(ops, T, H, W, C, shift):
    """x + proj(window_attention(LayerNorm(x))) in one launch: LayerNorm evaluation -> qkv product -> attention (its operands off by
    the qkv product's bound) -> proj product -> bias and residual, composed to first order (x 2)."""
    from oracle import tce_oracle as O
    g = torch.Generator().manual_seed(H * W + C + shift)
    nH = C // 32
    x = torch.randn(T * H * W, C, generator=g)
    g1, b1 = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    wqkv, bqkv = torch.randn(3 * C, C, generator=g) / math.sqrt(C), torch.randn(3 * C, generator=g) * 0.3
    table = torch.randn(169, nH, generator=g)
    wp, bp = torch.randn(C, C, generator=g) / math.sqrt(C), torch.randn(C, generator=g) * 0.2
    assert A.layernorm_sigma(x).min().item() > 1e-3
    y = F.layer_norm(x.double(), (C,), g1.double(), b1.double(), 1e-5)
    qkv = y @ wqkv.double().T + bqkv.double()
    Bqkv = A.bound_split(y, wqkv, A.c_dense(C)) + A.chain(A.ln_eval_bound(x, g1, b1, 1e-5), wqkv) + A.bound_bias(qkv)
    win, back, (Hp, Wp) = to_windows2d(qkv, T, H, W, shift, bqkv.double())
    Bwin, _, _ = to_windows2d(Bqkv, T, H, W, shift, torch.zeros(3 * C, dtype=torch.float64))   # padding rows are the exact bias
    bias = table[O.rel_pos_index(7).view(-1)].view(49, 49, nH).permute(2, 0, 1)
    mask = O.shift_attn_mask(Hp, Wp, 7, 3) if shift else None
    att, Batt, _ = windows_ref_and_bound(win, nH, bias, mask, Bwin)
    att, Batt = back(att), back(Batt) / 2      # windows_ref_and_bound doubles; the factor 2 is applied once, at the end
    ref = x.double() + att @ wp.double().T + bp.double()
    B = 2 * (A.chain(Batt, wp) + A.bound_split(att, wp, A.c_dense(C)) + 2 * A.bound_bias(ref))
    pk = ops.swin_attn_pack(dev(wqkv), dev(wp))
    out = torch.full((T * H * W, C), float("nan"), device="cuda")
    ops.swin_attn_fused(dev(x), pk, dev(bqkv), dev(bp), dev(table), dev(g1), dev(b1), T, H, W, C, shift, out=out)
    check("swin_attn_fused", f"{T}x{H}x{W} C={C} shift={shift}", tag(1, 1), out, ref, B, A.sum_abs(att, wp))


@pytest.mark.parametrize("batch,nh,Lq,Lk,pre_split", [(1, 8, 40, 40, False), (2, 8, 300, 700, False), (1, 8, 1200, 1200, False),
                                                      (1, 8, 1200, 1200, True), (2, 3, 77, 257, False)])
def test_mha_core(ops, batch, nh, Lq, Lk, pre_split):
    g = torch.Generator().manual_seed(Lq + Lk)
    E = nh * 32
    q, k, v = (torch.randn(batch, L, E, generator=g) for L in (Lq, Lk, Lk))
    out = torch.empty(batch, Lq, E, device="cuda")
    ops.mha_core(dev(q), dev(k), dev(v), batch, nh, Lq, Lk, E, E, E, Lq * E, Lk * E, Lk * E, out, E, Lq * E,
                 alloc=(lambda n: torch.empty(n, dtype=torch.float32, device="cuda")) if pre_split else None)
    out = out.cpu()
    for b in range(batch):
        for h in range(nh):
            sl = slice(32 * h, 32 * h + 32)
            ref, B, S = attention_ref_and_bound(q[b, :, sl], k[b, :, sl], v[b, :, sl], 32 ** -0.5)
            check("mha_core" + (" (pre-split planes)" if pre_split else ""), f"{batch}x{nh} Lq={Lq} Lk={Lk}", tag(1, 1), out[b, :, sl], ref, B, S)


def _fold(rows):
    """One line per (family, shape, scales): the worst of its launches / heads / batch entries."""
    best = {}
    for fam, shape, sc, rS, rB in rows:
        key = (fam, shape, sc)
        o = best.get(key, (0.0, 0.0))
        best[key] = (max(o[0], rS), max(o[1], rB))
    return [(k[0], k[1], k[2], v[0], v[1]) for k, v in best.items()]


# ---------------------------------------------------------------------------------------------------------------
# xattn (folded text cross-attention)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,L,mode", [(18000, 32, "add_ln"), (4600, 11, "add_ln"), (301, 32, "mul")])
def test_xattn(ops, M, L, mode):
    """x -> q-projection -> 8-head softmax over L <= 32 keys -> out-projection -> residual (-> LayerNorm), run as a fused FFN whose
    weights W1 = scale Wq^T k_h, b1 = scale bq k_h, W2 = Wo v_h are folded on the device in fp32 (K = 32 sums: worst-case c = 32
    each), whose activation is the per-head softmax.  Dense sweep over the five magnitudes and the four-decade rows."""
    Cn, nh, scale = 256, 8, 32 ** -0.5
    for j, (ws, as_) in enumerate(A.DENSE_SCALES + ((None, None),)):   # ws scales Wq / Wo and their biases, as_ the rows x
        g = torch.Generator().manual_seed(M + L + j)
        decades = ws is None
        if decades:   # four decades of range along the channels of x
            ws, as_ = 1.0, 1.0
        x = torch.randn(M, Cn, generator=g) * as_ * (torch.logspace(-2, 2, Cn)[None, :] if decades else 1.0)
        Wq, Wo = torch.randn(Cn, Cn, generator=g) * 0.06 * ws, torch.randn(Cn, Cn, generator=g) * 0.06 * ws
        bq, bo = torch.randn(Cn, generator=g) * 0.2 * ws * as_, torch.randn(Cn, generator=g) * 0.2 * ws
        k, v = torch.randn(L, Cn, generator=g), torch.randn(L, Cn, generator=g)
        gam, bet = torch.rand(Cn, generator=g) + 0.5, torch.randn(Cn, generator=g) * 0.2
        ar = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device="cuda")
        pk = ops.xattn_pack(dev(k), dev(v), ops.xattn_static(dev(Wq), dev(bq)), dev(Wo), L, ar)
        out = torch.empty(M, Cn, device="cuda")
        if mode == "add_ln":
            ops.xattn_fused(dev(x), pk, dev(bo), M, out, ln_out=(dev(gam), dev(bet)))
        else:
            ops.xattn_fused(dev(x), pk, dev(bo), M, out, res_mode=ops.RES_MUL)
        x64 = x.double()
        att, Batt, Satt = torch.zeros(M, Cn, dtype=torch.float64), torch.zeros(M, Cn, dtype=torch.float64), torch.zeros(M, Cn, dtype=torch.float64)
        for h in range(nh):
            sl = slice(32 * h, 32 * h + 32)
            W1 = scale * (k[:, sl].double() @ Wq[sl].double())                      # [L, 256]
            b1 = scale * (k[:, sl].double() @ bq[sl].double())                      # [L]
            E1 = A.EPS_F32 * 34 * scale * (k[:, sl].double().abs() @ Wq[sl].double().abs())   # fold in fp32: 32 terms + scale + store
            Eb1 = A.EPS_F32 * 34 * scale * (k[:, sl].double().abs() @ bq[sl].double().abs())
            s = x64 @ W1.T + b1
            Bs = (A.bound_split(x, W1, A.c_dense(Cn)) + A.chain(x64.abs(), E1) + Eb1
                  + A.EPS_F32 * (2 * s.abs() + (s - s.amax(1, keepdim=True)).abs()))
            p = torch.softmax(s, -1)
            W2 = Wo[:, sl].double() @ v[:, sl].double().T                           # [256, L]
            E2 = A.EPS_F32 * 33 * (Wo[:, sl].double().abs() @ v[:, sl].double().abs().T)
            dp = (2.0 * Bs.amax(1, keepdim=True) + 4 * A.EPS_F32) * p
            att += p @ W2.T
            Batt += A.chain(dp, W2) + A.bound_split(p, W2, A.c_dense(nh * L)) + A.chain(p, E2)
            Satt += A.sum_abs(p, W2)
        y = att + bo.double()
        if mode == "add_ln":
            z = x64 + y
            assert A.layernorm_sigma(z).min().item() > 1e-3
            ref = F.layer_norm(z, (Cn,), gam.double(), bet.double(), 1e-5)
            B = 2 * A.ln_tail(z, Batt + 2 * A.bound_bias(z), gam, bet, 1e-5)
        else:
            ref = x64 * y
            B = 2 * (x64.abs() * (Batt + A.bound_bias(y)) + A.bound_bias(ref))
        check(f"xattn {mode}", f"{M} rows, {L} keys", "4 decades along K" if decades else tag(ws, as_), out, ref, B, Satt)


# ---------------------------------------------------------------------------------------------------------------
def test_zz_write_profile(ops):
    """Writes the table of every case above (run the whole module: each family test appends its lines)."""
    rows = _fold(RESULTS)
    families = {r[0].split()[0] for r in rows}
    need = {"gemm", "gemm_ex", "gemm_batched", "conv2d_cl", "rowlin", "ffn", "conv3x3", "thin", "fewrow_linear", "patch_embed", "mha_core",
            "xattn", "window_attn", "window_attn3d", "swin_attn_fused"}
    assert need <= families, f"families that did not run: {sorted(need - families)}"
    with open(PROFILE, "w") as f:
        f.write("# tests/test_arith_bound_gpu.py on an MI355X: per case, the largest |out - fp64 ref| over the output as a fraction of\n"
                "# S = sum_k |a_k||w_k| (the product's error scale; for chained families the last product's) and of the derived bound B.\n"
                f"# dense accumulation model c = {A.DENSE_C_FACTOR:g} * sqrt(3 K), validated by the 'gemm mode f32' lines (<= 0.5 of bound_acc).\n"
                "# family | shape | scales | max err/S | max err/B\n")
        for fam, shape, sc, rS, rB in sorted(rows):
            f.write(f"{fam} | {shape} | {sc} | {rS:.3e} | {rB:.3f}\n")
