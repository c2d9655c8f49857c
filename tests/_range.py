"""The fp16 range guard of the split-mode arithmetic (include/tce_rvos.h, tce_set_range_flag) as a reference predicate and a table of
store sites.  Nothing here needs a GPU at import; the launches a case carries run only when the GPU module calls them.

    expected_flag(values)   the guard's rule on fp32 bit patterns; expected_flag_plain is the same rule in words
    SITES                   one entry per (store site, launch form): entry point, form, source file, output / intermediate, and a
                            builder make(target, cls, via) -> Case
    UNGUARDED               every other launching entry point, with the reason it carries no report

A case is an EXACT construction: operands are fp16 numbers, so products are exact in every mode.  A one-hot row a[r, k0] = 256
against w[c, k0] = 235 stores 60160 at (r, c); against 234 it stores 59904; everything else stays O(1) (or, in the LayerNorm
forms, well under 59000).  The same target is reached through the bias, through RES_ADD and RES_MUL, and -- in the split-K forms --
through the sum of two chunks of 30080 each.  LayerNorm forms make the pre-norm row one-hot at c0, which stores
sqrt(N - 1) * gamma[c0] there, and pick gamma[c0] on either side of the limit (ln_gammas).

Condition on every case (check_condition, asserted before any launch; a condition on the INPUTS, no result depends on it): the fp64
reference of every tensor the launch stores (or, for a consumer-side site, splits) has no |value| in [59000, 61000] other than the
constructed target -- which is exact, or known to +-1, and at least 64 away from the limit, so the reference decides it without
ambiguity -- and at most one offending element.  References are intervals [lo, hi] so that sites whose stored value has a bounded, unmodelled part (the
attention term of the fused Swin block, the folded cross-attention) state a bound instead of an exact value.
"""
import dataclasses
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

LIMIT = 60000.0
LIMIT_BITS = int(np.array([LIMIT], dtype=np.float32).view(np.uint32)[0])
BAND = (59000.0, 61000.0)   # no reference value but the constructed target may lie here
TARGET_MARGIN = 64.0        # the target keeps this distance from the limit (an fp32 ulp at 60000 is 2^-8: nothing rounds across it)
ACT_NONE, ACT_RELU, ACT_GELU, ACT_RELU_AFTER = 0, 1, 2, 3
RES_NONE, RES_ADD, RES_MUL = 0, 1, 2
ALL = ("over+", "over-", "under", "inf", "nan", "clean")
POS = ("over+", "under", "inf", "clean")     # forms that end in a ReLU: negative values and NaN do not survive it (fmaxf(NaN, 0) = 0)


def _f32(values):
    v = np.asarray(values)
    with np.errstate(over="ignore"):    # fp64 values beyond FLT_MAX become Inf, as a store would have them
        return v if v.dtype == np.float32 else v.astype(np.float64).astype(np.float32)


def expected_flag(values):
    """The guard's rule (csrc/gemm_epilogue.h, tce_absbits / tce_range_report) on the fp32 bit patterns of the stored values."""
    bits = np.ascontiguousarray(_f32(values)).view(np.uint32) & np.uint32(0x7FFFFFFF)
    return bool((bits >= np.uint32(LIMIT_BITS)).any())


def expected_flag_plain(values):
    """The same rule in words: a stored value that is not strictly inside (-60000, 60000) -- NaN included -- raises the flag."""
    v = _f32(values)
    with np.errstate(invalid="ignore"):
        return bool((~(np.abs(v) < np.float32(LIMIT))).any())


@dataclasses.dataclass
class Case:
    site: object
    target: tuple
    cls: str
    via: str
    tensors: list            # [(name, lo, hi)] fp64 reference intervals of every tensor the launch stores / splits under the guard
    launch: object           # (ops, lib, put) -> the output tensor on the device; put(name, cpu tensor) -> device tensor
    nan_rows: tuple = ()     # output rows that may hold non-finite values (every other row must come back finite)
    nan_cols: tuple = ()
    _expect: object = None

    @property
    def expect(self):
        """expected_flag over every guarded tensor of the case (on the elements that are not plainly below the band)."""
        if self._expect is None:
            self._expect = False
            for _, lo, hi in self.tensors:
                lo, hi = _not_plainly_clean(lo, hi)
                with np.errstate(over="ignore"):
                    self._expect = self._expect or expected_flag(lo.numpy()) or expected_flag(hi.numpy())
        return self._expect

    @property
    def label(self):
        return f"{self.site.entry} [{self.site.form}] {self.site.shape} target {self.target} {self.cls} via {self.via}"


def _not_plainly_clean(lo, hi):
    """The elements of an interval reference with |value| >= 59000 possible, or not finite: a handful, as flat vectors."""
    amax = lo.abs() if lo is hi else torch.maximum(lo.abs(), hi.abs())
    idx = torch.nonzero(~(amax < BAND[0]).reshape(-1)).flatten()
    return lo.reshape(-1)[idx], hi.reshape(-1)[idx]


def check_condition(case):
    """The condition of the module docstring.  Returns the number of offending elements (0 or 1; non-finite classes: >= 1)."""
    n_off = n_near = 0
    for name, lo, hi in case.tensors:
        lo, hi = _not_plainly_clean(lo, hi)          # every other element is finite and below the band
        fin = torch.isfinite(lo) & torch.isfinite(hi)
        if case.cls not in ("inf", "nan"):
            assert bool(fin.all()), f"{case.label}: non-finite reference in {name}"
        amin = torch.where((lo <= 0) & (hi >= 0), torch.zeros_like(lo), torch.minimum(lo.abs(), hi.abs()))
        amax = torch.maximum(lo.abs(), hi.abs())
        off = fin & (amin > BAND[1])
        near = fin & ~off                           # the constructed target alone (60160 / 59904 and the like)
        near_over, near_under = near & (amin >= LIMIT + TARGET_MARGIN), near & (amax <= LIMIT - TARGET_MARGIN)
        assert bool((near == (near_over | near_under)).all()), f"{case.label}: {name} has an undecided reference value near the limit"
        n_near += int(near.sum())
        n_off += int(off.sum()) + int(near_over.sum()) + int((~fin).sum())
    assert n_near <= 1, f"{case.label}: {n_near} reference values in [{BAND[0]:g}, {BAND[1]:g}] (the target alone may lie there)"
    if case.cls in ("over+", "over-"):
        assert n_off == 1, f"{case.label}: {n_off} offending elements, expected exactly one"
    elif case.cls in ("inf", "nan"):
        assert n_off >= 1, f"{case.label}: the non-finite value did not reach a guarded tensor"
    else:
        assert n_off == 0, f"{case.label}: {n_off} offending elements in a case that must stay clean"
    assert case.expect == (n_off > 0)
    return n_off


@dataclasses.dataclass
class Site:
    entry: str
    form: str
    source: str
    kind: str                # "output" | "intermediate"
    shape: str
    targets: list
    variants: list           # [(via, classes)]
    make: object             # (target, cls, via) -> Case
    modes: tuple = ("f16x3", "f16")

    @property
    def id(self):
        return f"{self.entry}-{self.form}-{self.shape}".replace(" ", "_")

    def cases(self):
        for via, classes in self.variants:
            for cls in classes:
                for t in (self.targets[:1] if cls == "clean" else self.targets):
                    c = self.make(t, cls, via)
                    c.site, c.target, c.cls, c.via = self, t, cls, via
                    yield c


def targets(M, N, row_slice=32, rows_per_wg=128):
    """(0, 0), (M - 1, N - 1), one row in each wave's slice of the (last, ragged) workgroup tile and one column in each 32-column tile,
    paired so that every row slice and every column tile occurs."""
    base = (M - 1) // rows_per_wg * rows_per_wg
    rows = sorted({min(M - 1, s + 5) for s in range(0, min(M, rows_per_wg), row_slice)} |
                  {min(M - 1, base + s + 3) for s in range(0, rows_per_wg, row_slice) if base + s < M})
    cols = [min(N - 1, 32 * t + (7 * t + 1) % 32) for t in range((N + 31) // 32)]
    n = max(len(rows), len(cols))
    out = [(0, 0), (M - 1, N - 1)] + [(rows[i % len(rows)], cols[i % len(cols)]) for i in range(n)]
    return list(dict.fromkeys(out))


def ln_gammas(N):
    """(over, under): fp16 numbers g with sqrt(N - 1) * g >= 62000 resp. <= 58000, as close to the limit as 3 mantissa bits allow."""
    s = math.sqrt(N - 1)
    cand = sorted(m / 8 * 2.0 ** e for e in range(4, 16) for m in range(8, 16))
    return min(g for g in cand if s * g >= 62000), max(g for g in cand if s * g <= 58000)


def relu_fmax(v):
    return torch.where(torch.isnan(v), torch.zeros_like(v), v.clamp_min(0))


def epilogue(z, bias, act, res, res_mode):
    """What every GEMM-like epilogue of the library computes, in fp64."""
    v = z if bias is None else z + bias.double()
    if act == ACT_RELU:
        v = relu_fmax(v)
    if act == ACT_GELU:
        v = torch.where(torch.isinf(v) & (v > 0), v, F.gelu(v))
    if res_mode == RES_ADD:
        v = v + res.double()
    if res_mode == RES_MUL:
        v = v * res.double()
    if act == ACT_RELU_AFTER:
        v = relu_fmax(v)
    return v


# ---------------------------------------------------------------------------------------------------------------------
# the exact construction for linear forms
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _base(M, N, K, seed, ln):
    g = torch.Generator().manual_seed(1000 + seed)
    a = (torch.randn(M, K, generator=g) * 0.5).half().float()
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).half().float()
    k0, k1 = 3, K - 5
    a[:, k0] = 0
    a[:, k1] = 0
    w[:, k0] = 0.0 if ln else 2.0 ** -8
    w[:, k1] = 0.0 if ln else 2.0 ** -8
    bias = (torch.randn(N, generator=g) * 0.25).half().float()
    res = (torch.randn(M, N, generator=g) * 0.5 + 1.5).half().float()
    return a, w, bias, res, a.double() @ w.double().T, k0, k1


def linear_operands(M, N, K, r, c, cls, via, act=ACT_NONE, res_mode=RES_NONE, seed=0, use_bias=True):
    """a [M, K], w [N, K], bias [N] or None, res [M, N] or None and the fp64 reference of epilogue(a w^T): the target value class
    `cls` at (r, c), reached by `via` in product | sum | bias | res_add | res_mul | input."""
    a, w, bias, res, z, k0, k1 = _base(M, N, K, seed, False)
    a, w = a.clone(), w.clone()
    bias = bias.clone() if use_bias else None
    res = res.clone() if res_mode else None
    over, sgn = cls in ("over+", "over-"), (-1.0 if cls == "over-" else 1.0)
    special = {"inf": float("inf"), "nan": float("nan")}.get(cls)
    a[r] = 0
    if bias is not None:
        bias[c] = 0
    if cls == "clean":
        a[r, k0] = 1.0
    elif special is not None:
        a[r, k0] = 1.0
        if via in ("res_add", "res_mul"):
            res[r, c] = special
        elif via == "bias":
            bias[c] = special
        else:
            a[r, k0] = special
    elif via == "product":
        a[r, k0], w[c, k0] = 256.0, sgn * (235.0 if over else 234.0)
    elif via == "sum":
        a[r, k0] = a[r, k1] = 256.0
        w[c, k0] = w[c, k1] = sgn * (117.5 if over else 117.0)
    elif via in ("bias", "res_add"):
        a[r, k0], w[c, k0] = 256.0, sgn * 117.5
        if via == "bias":
            bias[c] = sgn * (30080.0 if over else 29824.0)
        else:
            res[r, c] = sgn * (30080.0 if over else 29824.0)
    elif via == "res_mul":
        a[r, k0], w[c, k0], res[r, c] = 1.0, sgn * (235.0 if over else 234.0), 256.0
    else:
        raise ValueError(via)
    zr = a[r].double() @ w.double().T if special is None or via != "input" else _row_with_special(a[r], w)
    ref = epilogue(z, bias, act, res, res_mode)     # rows other than r: a[m, k0] = a[m, k1] = 0, so the changed weights do not reach them
    ref = ref.clone() if ref is z else ref
    ref[r] = epilogue(zr[None], bias, act, None if res is None else res[r:r + 1], res_mode)[0]
    return a, w, bias, res, ref


def _row_with_special(arow, w):
    """a row holding one Inf / NaN against w: Inf * 0 = NaN as the hardware has it."""
    return (arow.double()[None, :] * w.double()).sum(1)


def near_operands(M, N, K, seed=0):
    """False-positive case: EVERY output within +-[50000, 59000] (256 * (200 .. 230) plus an O(1) remainder), no bias, no residual."""
    a, w, _, _, z, k0, _ = (t.clone() if torch.is_tensor(t) else t for t in _base(M, N, K, seed, False))
    a[:, k0] = 256.0
    c = torch.arange(N)
    w[:, k0] = torch.where(c % 2 == 0, 1.0, -1.0) * (200.0 + (c % 31).float())
    return a, w, a.double() @ w.double().T


def ln_operands(M, N, K, r, c0, cls, seed=0, eps=1e-5, res_mode=RES_NONE):
    """LayerNorm-ended forms: row r of the pre-norm tensor is one-hot (256 at c0, through the product), gamma[c0] decides the class."""
    a, w, _, res, z, k0, _ = (t.clone() if torch.is_tensor(t) else t for t in _base(M, N, K, seed, True))
    res = res - 1.5 if res_mode else None     # zero-mean residual rows
    g = torch.Generator().manual_seed(77 + seed)
    gamma, beta = (torch.rand(N, generator=g) + 0.5).half().float(), (torch.randn(N, generator=g) * 0.2).half().float()
    g_over, g_under = ln_gammas(N)
    a[r] = 0
    a[r, k0] = 256.0
    w[c0, k0] = 1.0
    if res is not None:
        res[r] = 0
    if cls in ("over+", "over-"):
        gamma[c0] = g_over * (-1.0 if cls == "over-" else 1.0)
    elif cls == "under":
        gamma[c0] = g_under
    elif cls in ("inf", "nan"):
        if res is not None:
            res[r, c0] = float(cls)
        else:
            a[r, k0] = float(cls)
    z[r] = _row_with_special(a[r], w)
    zz = z if res is None else z + res.double()
    ref = F.layer_norm(zz, (N,), gamma.double(), beta.double(), eps)
    return a, w, res, gamma, beta, ref


def exact(name, ref):
    return (name, ref, ref)


def _finite_rows(t):
    return tuple(sorted(set(torch.nonzero(~torch.isfinite(t).all(1)).flatten().tolist())))


def _finite_cols(t):
    return tuple(sorted(set(torch.nonzero(~torch.isfinite(t).all(0)).flatten().tolist())))


def _out_case(ref, launch, name="out"):
    return Case(None, None, None, None, [exact(name, ref)], launch, nan_rows=_finite_rows(ref), nan_cols=_finite_cols(ref))


# ---------------------------------------------------------------------------------------------------------------------
# tce_gemm_f32: the tiled GEMM (csrc/gemm_f16x3_kernel.h) and the fix-up pass (csrc/gemm.hip, epi_fix_kernel)
# ---------------------------------------------------------------------------------------------------------------------
def gemm_site(M, N, K, tile, form, variants, act=ACT_NONE, res_mode=RES_NONE, batch=1, a2=False, source="gemm_f16x3_kernel.h",
              row_slice=32, rows_per_wg=128, seed=1, tg=None):
    rows = batch * M

    def make(t, cls, via):
        r, c = t
        rm = res_mode if via not in ("res_add", "res_mul") else {"res_add": RES_ADD, "res_mul": RES_MUL}[via]
        a, w, bias, res, ref = linear_operands(rows, N, K, r, c, cls, via, act, rm, seed)

        def launch(ops, lib, put):
            assert lib.tce_gemm_select_tile_ex(M, N, K, batch, 0) == tile, (lib.tce_gemm_select_tile_ex(M, N, K, batch, 0), tile)
            kw = dict(bias=put("bias", bias), act=act, res=put("res", res) if rm else None, res_mode=rm)
            if batch == 1 and not a2:
                return ops.gemm(put("a", a), put("w", w), out=put("out", torch.zeros(M, N)), **kw)
            gap = 3
            out = put("out", torch.zeros(batch, M + gap, N))
            extra = {}
            if a2:   # A + A2 = a, exactly: the target row's 256 is 128 + 128
                g = torch.Generator().manual_seed(5)
                p2 = (torch.randn(rows, K, generator=g) * 0.25).half().float()
                p2[r] = a[r] / 2
                extra = dict(a2=put("a2", p2), lda2=K, sA2=M * K)
                a1 = a - p2
            else:
                a1 = a
            ops.gemm_ex(put("a", a1), put("w", w), out, M, N, K, K, K, N, batch=batch, sA=M * K, sC=(M + gap) * N, sRes=M * N,
                        ldres=N, **extra, **kw)
            assert float(out[:, M:].abs().max()) == 0.0   # the gap between the batch entries' outputs is not written
            return out[:, :M].reshape(rows, N)
        return _out_case(ref, launch)
    return Site("tce_gemm_f32", form, source, "output", f"{batch}x{M}x{N}x{K}" if batch > 1 else f"{M}x{N}x{K}",
                tg or (targets(rows, N, row_slice, rows_per_wg) if batch == 1 else targets(rows, N, row_slice, rows_per_wg)[1:]),
                variants, make)


def conv_site(T, H, W, Cin, N, k, tile, form, variants, splits=1, entry="tce_gemm_f32", source="gemm_f16x3_kernel.h", seed=2):
    """Implicit-GEMM convolution, stride 1, pad k // 2: the one-hot row is one input pixel with one channel set; its centre tap
    carries the large weight, the same channel of every other tap 2^-8."""
    import _arith
    M, K, p = T * H * W, k * k * Cin, k // 2
    ctap = (k * k) // 2

    def make(t, cls, via):
        r, c = t
        g = torch.Generator().manual_seed(2000 + seed)
        x = (torch.randn(M, Cin, generator=g) * 0.5).half().float()
        w = (torch.randn(N, K, generator=g) / math.sqrt(K)).half().float()
        bias = (torch.randn(N, generator=g) * 0.25).half().float()
        c0 = 3
        x[:, c0] = 0
        x[r] = 0
        w[:, c0::Cin] = 2.0 ** -8
        bias[c] = 0
        over, sgn = cls in ("over+", "over-"), (-1.0 if cls == "over-" else 1.0)
        if cls == "clean":
            x[r, c0] = 1.0
        elif cls in ("inf", "nan"):
            x[r, c0] = 1.0
            if via == "bias":
                bias[c] = float(cls)
            else:
                x[r, c0] = float(cls)
        elif via == "product":
            x[r, c0], w[c, ctap * Cin + c0] = 256.0, sgn * (235.0 if over else 234.0)
        else:   # bias
            x[r, c0], w[c, ctap * Cin + c0], bias[c] = 256.0, sgn * 117.5, sgn * (30080.0 if over else 29824.0)
        a = _arith.im2col(x, T, H, W, Cin, k, 1, p)
        with np.errstate(all="ignore"):
            z = a.double() @ w.double().T
            if cls in ("inf", "nan") and via != "bias":   # Inf * 0 = NaN in every pixel whose window holds the input pixel
                bad = ~torch.isfinite(a).all(1)
                z[bad] = float("nan")
        ref = z + bias.double()

        def launch(ops, lib, put):
            if splits == 1:
                assert lib.tce_gemm_select_tile_ex(M, N, K, 1, 1) == tile
            ws = put("ws", torch.zeros(splits * M * N)) if splits > 1 else None
            out, _, _ = ops.conv2d_cl(put("x", x), put("w", w), T, H, W, Cin, k, k, 1, p, bias=put("bias", bias),
                                      out=put("out", torch.zeros(M, N)), splitk=splits, ws=ws)
            return out
        return _out_case(ref, launch)
    shape = f"{T}x{H}x{W} {Cin}->{N} {k}x{k}" + (f" / {splits}" if splits > 1 else "")
    return Site(entry, form, source, "output", shape, targets(M, N), variants, make)


# ---------------------------------------------------------------------------------------------------------------------
# split-K: the partial launches report on the partial planes, the reduce kernels (csrc/gemm.hip) on what they store
# ---------------------------------------------------------------------------------------------------------------------
def splitk_site(M, N, K, splits, variants, seed=3):
    def make(t, cls, via):
        r, c = t
        rm = {"res_add": RES_ADD, "res_mul": RES_MUL}.get(via, RES_NONE)
        a, w, bias, res, ref = linear_operands(M, N, K, r, c, cls, via, ACT_NONE, rm, seed)

        def launch(ops, lib, put):
            return ops.gemm_ex(put("a", a), put("w", w), put("out", torch.zeros(M, N)), M, N, K, K, K, N, bias=put("bias", bias),
                               res=put("res", res) if rm else None, ldres=N, res_mode=rm, splitk=splits,
                               ws=put("ws", torch.zeros(splits * M * N)))
        return _out_case(ref, launch)
    return Site("tce_gemm_splitk_f32", "splitk_reduce_kernel", "gemm.hip", "output", f"{M}x{N}x{K} / {splits}", targets(M, N),
                variants, make)


def splitk_ln_site(M, N, K, splits, kernel, seed=4):
    def make(t, cls, via):
        r, c = t
        rm = RES_ADD if via == "res_add" else RES_NONE
        a, w, res, gamma, beta, ref = ln_operands(M, N, K, r, c, cls, seed, eps=1e-12, res_mode=rm)

        def launch(ops, lib, put):
            buf = put("out", res if rm else torch.zeros(M, N))    # in place on the residual stream, as every caller runs it
            return ops.gemm_ex(put("a", a), put("w", w), buf, M, N, K, K, K, N, res=buf if rm else None, ldres=N, res_mode=rm,
                               splitk=splits, ws=put("ws", torch.zeros(splits * M * N)), ln=(put("gamma", gamma), put("beta", beta)),
                               ln_eps=1e-12)
        return _out_case(ref, launch)
    return Site("tce_gemm_splitk_ln_f32", kernel, "gemm.hip", "output", f"{M}x{N}x{K} / {splits}", targets(M, N),
                [("gamma", ALL), ("res_add", ("over+", "under", "nan"))], make)


# ---------------------------------------------------------------------------------------------------------------------
# thin weight streams (csrc/thin.hip): planes + splitk_reduce, and the planes-as-next-x chain (consumer-side report)
# ---------------------------------------------------------------------------------------------------------------------
def thin_reduce_site(M, N, K, variants, seed=5):
    splits = K // 256

    def make(t, cls, via):
        r, c = t
        rm = {"res_add": RES_ADD}.get(via, RES_NONE)
        a, w, bias, res, ref = linear_operands(M, N, K, r, c, cls, via, ACT_NONE, rm, seed)

        def launch(ops, lib, put):
            assert ops.thin_splits(M, N, K) == splits
            ws = ops.thin_partials(put("a", a), put("w", w), put("ws", torch.zeros(splits, M, N)), M, N, K)
            return ops.splitk_reduce(ws, splits, M, N, put("out", torch.zeros(M, N)), bias=put("bias", bias),
                                     res=put("res", res) if rm else None, ldres=N, res_mode=rm)
        return _out_case(ref, launch)
    return Site("tce_splitk_reduce_f32", "after thin_partials", "gemm.hip", "output", f"{M}x{N}x{K}", targets(M, N), variants, make)


def thin_chain_site(M, N, K, N2, seed=6):
    """y = GELU(x W^T + b) W2^T, the first layer's planes finished on load by the second launch: the finished hidden value is over
    the limit (sum of three planes + bias, then GELU) while W2 (scaled by 2^-10) keeps every stored output O(1)."""
    s1, s2 = K // 256, N // 256

    def make(t, cls, via):
        r, c = t
        a, w, bias, _, h = linear_operands(M, N, K, r, c, cls, via, ACT_GELU, RES_NONE, seed)
        g = torch.Generator().manual_seed(60 + seed)
        w2 = ((torch.randn(N2, N, generator=g) / math.sqrt(N)) * 2.0 ** -10).half().float()
        out = h @ w2.double().T
        if cls in ("inf", "nan"):
            bad = ~torch.isfinite(h).all(1)
            out[bad] = float("nan")

        def launch(ops, lib, put):
            ws1 = ops.thin_partials(put("a", a), put("w", w), put("ws1", torch.zeros(s1, M, N)), M, N, K)
            ws2 = ops.thin_partials(ws1, put("w2", w2), put("ws2", torch.zeros(s2, M, N2)), M, N2, N, xsplits=s1,
                                    bias_x=put("bias", bias), act_x=ACT_GELU)
            return ops.splitk_reduce(ws2, s2, M, N2, put("out", torch.zeros(M, N2)))
        return Case(None, None, None, None, [exact("finished x", h), exact("out", out)], launch, nan_rows=_finite_rows(out))
    return Site("tce_thin_partials_f32", "xsplits > 0 (planes as the next x)", "thin.hip", "intermediate", f"{M}x{N}x{K} -> {N2}",
                targets(M, N), [("sum", ("over+", "under", "clean")), ("bias", ("over+", "under", "inf", "nan"))], make)


# ---------------------------------------------------------------------------------------------------------------------
# rowlin (csrc/rowlin.hip)
# ---------------------------------------------------------------------------------------------------------------------
def rowlin_site(M, N, K, variant, batch=1, seed=7):
    rows = batch * M

    def make(t, cls, via):
        r, c = t
        kw, extra = {}, {}
        if variant == "ln_out":
            a, w, res, gamma, beta, ref = ln_operands(rows, N, K, r, c, cls, seed, res_mode=RES_ADD)
            bias = None
            extra = dict(res=res, ln_out=(gamma, beta))
            kw = dict(res_mode=RES_ADD, ldres=N, sRes=M * N)
        elif variant == "ln_in":
            a, w, bias, ref = _ln_in_operands(rows, N, K, r, c, cls, seed)
            extra = dict(ln_in=(torch.ones(K), torch.zeros(K)))
        else:
            act, rm = {"plain": (ACT_NONE, RES_NONE), "a2_relu": (ACT_RELU, RES_NONE), "res_mul": (ACT_NONE, RES_MUL),
                       "gelu_res": (ACT_GELU, RES_ADD)}[variant]
            a, w, bias, res, ref = linear_operands(rows, N, K, r, c, cls, via, act, rm, seed)
            kw = dict(act=act, res_mode=rm, ldres=N, sRes=M * N)
            if rm:
                extra["res"] = res
            if variant == "a2_relu":   # a position map shared by the batch entries (sA2 = 0): x = a - pos, exactly, row by row
                g = torch.Generator().manual_seed(8)
                pos = (torch.randn(M, K, generator=g) * 0.25).half().float()
                pos[r % M] = 0
                extra["a2"] = pos
                a = a - pos.repeat(batch, 1)
                kw.update(lda2=K, sA2=0)

        def launch(ops, lib, put):
            pk = ops.rowlin_pack(put("w", w))     # packed in the arithmetic mode under test
            k2 = dict(kw)
            for name, v in extra.items():
                k2[name] = tuple(put(f"{name}{i}", x) for i, x in enumerate(v)) if isinstance(v, tuple) else put(name, v)
            out = put("out", torch.zeros(rows, N))
            ops.rowlin(put("a", a), pk, out, M, N, K, K, N, bias=put("bias", bias) if bias is not None else None, batch=batch,
                       sX=M * K, sOut=M * N, **k2)
            return out
        return _out_case(ref, launch)
    variants = {"plain": [("product", ALL), ("bias", ("over+", "over-", "under", "inf"))],
                # no Inf through the input here: the split turns it into Inf (hi) and NaN (lo), and the ReLU then stores 0
                "a2_relu": [("product", ("over+", "under", "clean"))],
                "res_mul": [("res_mul", ALL)],
                "gelu_res": [("res_add", ("over+", "under", "inf", "nan", "clean"))],
                "ln_in": [("product", ("over+", "over-", "under", "nan", "clean"))],
                "ln_out": [("gamma", ALL)]}[variant]
    return Site("tce_rowlin_f32", variant + (f", batch {batch}" if batch > 1 else ""), "rowlin.hip", "output", f"{M}x{N}x{K}",
                targets(rows, N), variants, make)


def _ln_in_operands(M, N, K, r, c, cls, seed):
    """LayerNorm prologue (gamma 1, beta 0): the one-hot row normalises to sqrt(K - 1) at k0, the weight there decides the class."""
    a, w, bias, _, _, k0, _ = (t.clone() if torch.is_tensor(t) else t for t in _base(M, N, K, seed, False))
    s = math.sqrt(K - 1)
    a[r] = 0
    a[r, k0] = 256.0
    bias[c] = 0
    if cls in ("over+", "over-"):
        w[c, k0] = float(torch.tensor(63000.0 / s).half()) * (-1.0 if cls == "over-" else 1.0)
    elif cls == "under":
        w[c, k0] = float(torch.tensor(57000.0 / s).half())
    elif cls == "nan":
        a[r, k0] = float("nan")
    y = F.layer_norm(a.double(), (K,), None, None, 1e-5)
    ref = y @ w.double().T + bias.double()
    return a, w, bias, ref


# ---------------------------------------------------------------------------------------------------------------------
# fused FFN (csrc/ffn.hip): hidden values, final store; the folded cross-attention and its chain into an FFN
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _ffn_base(M, C, Hd, seed, site, act, ln, cols):
    """Operands shared by every case of a site, and the fp64 hidden / pre-norm tensors they give: a case changes row r only (plus, at
    most, one output column by a constant), so its reference is this one with that row computed again."""
    g = torch.Generator().manual_seed(3000 + seed)
    x = (torch.randn(M, C, generator=g) * 0.5).half().float()
    w1 = (torch.randn(Hd, C, generator=g) / math.sqrt(C)).half().float()
    b1 = (torch.randn(Hd, generator=g) * 0.2).half().float()
    w2 = (torch.randn(C, Hd, generator=g) / math.sqrt(Hd) * (2.0 ** -10 if site == "hidden" else 1.0)).half().float()
    b2 = (torch.randn(C, generator=g) * 0.2).half().float()
    gam, bet = (torch.rand(C, generator=g) + 0.5).half().float(), (torch.randn(C, generator=g) * 0.2).half().float()
    if site == "hidden":     # column k0 of x is zero outside the target row: W1[c, k0] then matters to that row alone
        x[:, 3] = 0
        w1[:, 3] = 2.0 ** -8
    else:                    # the target columns stay out of the hidden product and carry no bias
        w1[:, list(cols)] = 0
        b2[list(cols)] = 0
    if site == "ln_out":     # every hidden value of every row is switched off by the ReLU: the pre-norm tensor is x itself
        b1[:] = -8.0
        b2[:] = 0
    h, pre = ffn_rows(x, w1, b1, w2, b2, act, ln == "in")
    return x, w1, b1, w2, b2, gam, bet, h, pre


def ffn_rows(x, w1, b1, w2, b2, act, ln_in):
    """(hidden, x + W2 hidden + b2) in fp64; Inf / NaN propagate as IEEE has them (Inf * 0 = NaN)."""
    xs = x.double()
    y = F.layer_norm(xs, (xs.shape[1],), None, None, 1e-5) if ln_in else xs
    fin = bool(torch.isfinite(y).all())
    pre = (y @ w1.double().T if fin else (y[:, None, :] * w1.double()[None]).sum(2)) + b1.double()
    if act == ACT_RELU:      # the kernel's ReLU is an integer max on the bit pattern: +Inf and a positive NaN pass
        h = torch.where(torch.isnan(pre), pre, pre.clamp_min(0))
    else:
        h = torch.where(torch.isinf(pre) & (pre > 0), pre, F.gelu(pre))
    fin = bool(torch.isfinite(h).all())
    return h, xs + (h @ w2.double().T if fin else (h[:, None, :] * w2.double()[None]).sum(2)) + b2.double()


def ffn_site(M, C, Hd, act, ln, site, form="", seed=9, tg=None):
    """site = hidden: hidden[r, h0] is the target (x one-hot at k0, W1[h0, k0] large), W2 scaled by 2^-10 keeps the output O(1);
    site = out: out[r, c] through the residual x[r, c] (W1[:, c] = 0 keeps it out of the hidden product), or x plus b2;
    site = ln_out: the pre-norm row is the one-hot x row itself, gamma[c] decides."""
    act_c = ACT_RELU if act == "relu" else ACT_GELU
    tg = tg or targets(M, Hd if site == "hidden" else C)
    cols = tuple(sorted({c for _, c in tg}))

    def make(t, cls, via):
        r, c = t
        x, w1, b1, w2, b2, gam, bet, h, pre = _ffn_base(M, C, Hd, seed, site, act_c, ln, cols)
        x, w1, b2, gam = x.clone(), w1.clone(), b2.clone(), gam.clone()
        k0 = 3
        over, sgn = cls in ("over+", "over-"), (-1.0 if cls == "over-" else 1.0)
        special = {"inf": float("inf"), "nan": float("nan")}.get(cls)
        if site == "hidden":
            x[r] = 0
            s = math.sqrt(C - 1) if ln == "in" else 256.0
            x[r, k0] = 256.0 if special is None else special
            if cls == "clean":
                x[r, k0] = 1.0
            elif special is None:
                w1[c, k0] = float(torch.tensor((63000.0 if over else 57000.0) / s).half()) if ln == "in" else (235.0 if over else 234.0)
        elif site == "out":
            if special is not None:
                x[r, c] = special
            elif cls != "clean":
                if via == "res":
                    x[r, c] = sgn * (60160.0 if over else 58880.0)
                else:   # x + b2
                    x[r, c], b2[c] = sgn * 30080.0, sgn * (30080.0 if over else 28800.0)
        else:
            g_over, g_under = ln_gammas(C)
            x[r] = 0
            x[r, c] = 256.0 if special is None else special
            if over:
                gam[c] = sgn * g_over
            elif cls == "under":
                gam[c] = g_under
        hr, pr = ffn_rows(x[r:r + 1], w1, b1, w2, b2, act_c, ln == "in")
        h, pre = h.clone(), pre.clone()
        if site == "out" and via == "b2":
            pre[:, c] += b2[c].double()
        h[r], pre[r] = hr[0], pr[0]
        o = F.layer_norm(pre, (C,), gam.double(), bet.double(), 1e-5) if ln == "out" else pre
        ln_in = (torch.ones(C), torch.zeros(C)) if ln == "in" else None
        ln_out = (gam, bet) if ln == "out" else None

        def launch(ops, lib, put):
            pk = ops.ffn_pack(put("w1", w1), put("b1", b1), put("w2", w2))
            xd = put("x", x)
            out = put("out", torch.zeros(M, C))
            kw = dict(ln_in=(put("gi", ln_in[0]), put("bi", ln_in[1])) if ln_in else None,
                      ln_out=(put("go", ln_out[0]), put("bo", ln_out[1])) if ln_out else None)
            if form == "split":
                nws, ncnt = ops.ffn_split_need(M, C, Hd, act_c)
                assert nws > 0, "no split planned at this shape"
                kw["split"] = (put("ws", torch.zeros(nws)), torch.zeros(ncnt, dtype=torch.int32, device=xd.device))
            if form == "half":
                lib.tce_debug_ffn_set_half(1)
            try:
                ops.ffn_fused(xd, pk, put("b2", b2), Hd, act_c, out=out, **kw)
            finally:
                lib.tce_debug_ffn_set_half(0)
            return out
        return Case(None, None, None, None, [exact("hidden", h), exact("out", o)], launch, nan_rows=_finite_rows(o))
    variants = {"hidden": [("product", ("over+", "under", "inf", "nan", "clean"))],
                "out": [("res", ALL), ("b2", ("over+", "over-", "under"))],
                "ln_out": [("gamma", ALL)]}[site]
    name = {"hidden": "hidden", "out": "final store", "ln_out": "final store, ln_out"}[site]
    entry = "tce_ffn_fused_split_f32" if form == "split" else "tce_ffn_fused_f32"
    return Site(entry, f"{name}, {act}" + (", ln_in" if ln == "in" else "") + (f", {form}" if form else ""), "ffn.hip",
                "intermediate" if site == "hidden" else "output", f"{M}x{C}x{Hd}", tg, variants, make)


# ---------------------------------------------------------------------------------------------------------------------
# 3x3 pixel-stationary convolution (csrc/conv3x3.hip): tile store and the split entry's reduce
# ---------------------------------------------------------------------------------------------------------------------
def conv3x3_site(T, H, W, waves, pieces, variants, seed=10):
    import _arith
    Cin = N = 256
    M = T * H * W

    def make(t, cls, via):
        r, c = t
        g = torch.Generator().manual_seed(4000 + seed)
        x = (torch.randn(M, Cin, generator=g) * 0.5).half().float()
        w = (torch.randn(N, 9 * Cin, generator=g) / math.sqrt(9 * Cin)).half().float()
        bias = (torch.randn(N, generator=g) * 0.25).half().float()
        c0, c1 = 3, Cin - 5
        x[:, c0] = 0
        x[:, c1] = 0
        x[r] = 0
        w[:, c0::Cin] = 2.0 ** -8
        w[:, c1::Cin] = 2.0 ** -8
        bias[c] = 0
        over, sgn = cls in ("over+", "over-"), (-1.0 if cls == "over-" else 1.0)
        if cls == "clean":
            x[r, c0] = 1.0
        elif cls in ("inf", "nan"):
            x[r, c0] = 1.0
            if via == "bias":
                bias[c] = float(cls)
            else:
                x[r, c0] = float(cls)
        elif via == "product":
            x[r, c0], w[c, 4 * Cin + c0] = 256.0, sgn * (235.0 if over else 234.0)
        elif via == "sum":   # the K walk is cut along the channels: c0 and c1 lie in different pieces
            x[r, c0] = x[r, c1] = 256.0
            w[c, 4 * Cin + c0] = w[c, 4 * Cin + c1] = sgn * (117.5 if over else 117.0)
        else:
            x[r, c0], w[c, 4 * Cin + c0], bias[c] = 256.0, sgn * 117.5, sgn * (30080.0 if over else 29824.0)
        a = _arith.im2col(x, T, H, W, Cin, 3, 1, 1)
        z = a.double().nan_to_num(0.0, 0.0, 0.0) @ w.double().T
        if cls in ("inf", "nan") and via != "bias":
            z[~torch.isfinite(a).all(1)] = float("nan")
        ref = z + bias.double()

        def launch(ops, lib, put):
            pk = ops.conv3x3_pack(put("w", w), Cin)
            lib.tce_debug_conv3x3_set_waves(waves)
            lib.tce_debug_conv3x3_set_pieces(max(pieces, 0))
            try:
                xd, out = put("x", x), put("out", torch.zeros(M, N))
                if pieces < 0:
                    ops.conv3x3(xd, pk, T, H, W, Cin, N, bias=put("bias", bias), out=out)
                else:
                    assert int(lib.tce_conv3x3_split_pieces(M, Cin, N)) == pieces
                    nws = max(1, int(lib.tce_conv3x3_split_ws_floats(M, Cin, N)))
                    wsb = put("ws", torch.zeros(nws))
                    rc = lib.tce_conv3x3_split_f32(xd.data_ptr(), Cin, pk.data_ptr(), put("bias", bias).data_ptr(), out.data_ptr(), N,
                                                   T, H, W, Cin, N, wsb.data_ptr(), nws, torch.cuda.current_stream().cuda_stream)
                    assert rc == 0
            finally:
                lib.tce_debug_conv3x3_set_pieces(0)
                lib.tce_debug_conv3x3_set_waves(0)
            return out
        return _out_case(ref, launch)
    split = pieces >= 0
    return Site("tce_conv3x3_split_f32" if split else "tce_conv3x3_f32", (f"split reduce, {pieces} pieces" if split else "tile store") +
                f", {waves} waves", "conv3x3.hip", "output", f"{T}x{H}x{W} 256->256", targets(M, N), variants, make,
                modes=("f16x3",) if split else ("f16x3", "f16"))   # the split entry exists in the three-product mode only


# ---------------------------------------------------------------------------------------------------------------------
# patch embedding (csrc/patch_embed.hip): 4x4 / stride 4 patches + bias + LayerNorm, through gamma
# ---------------------------------------------------------------------------------------------------------------------
def patch_embed_site(T, H, W, C, seed=11):
    Hp, Wp = (H + 3) // 4, (W + 3) // 4
    M = T * Hp * Wp

    def make(t, cls, via):
        r, c = t
        g = torch.Generator().manual_seed(5000 + seed)
        x = (torch.randn(T, 3, H, W, generator=g) * 0.5).half().float()
        w = (torch.randn(C, 3, 4, 4, generator=g) / math.sqrt(48)).half().float()
        b = torch.zeros(C)
        gam, bet = (torch.rand(C, generator=g) + 0.5).half().float(), (torch.randn(C, generator=g) * 0.2).half().float()
        g_over, g_under = ln_gammas(C)
        # input element (channel 0, row 0, column 0 of every patch) is zero except in patch r; weight tap (0, 0, 0) is one-hot at c
        x[:, 0, 0::4, 0::4] = 0
        w[:, 0, 0, 0] = 0
        w[c, 0, 0, 0] = 1.0
        tt, py, px = r // (Hp * Wp), (r // Wp) % Hp, r % Wp
        x[tt, :, 4 * py:4 * py + 4, 4 * px:4 * px + 4] = 0
        x[tt, 0, 4 * py, 4 * px] = 256.0 if cls not in ("inf", "nan") else float(cls)
        if cls in ("over+", "over-"):
            gam[c] = g_over * (-1.0 if cls == "over-" else 1.0)
        elif cls == "under":
            gam[c] = g_under
        xp = F.pad(x, (0, (4 - W % 4) % 4, 0, (4 - H % 4) % 4))
        a = F.unfold(xp, 4, stride=4).transpose(1, 2).reshape(-1, 48)
        z = a.double().nan_to_num(0.0, 0.0, 0.0) @ w.reshape(C, 48).double().T + b.double()
        z[~torch.isfinite(a).all(1)] = float("nan")
        ref = F.layer_norm(z, (C,), gam.double(), bet.double(), 1e-5)

        def launch(ops, lib, put):
            out = put("out", torch.zeros(M, C))
            ops.patch_embed(put("x", x), put("w", w), put("b", b), put("gamma", gam), put("beta", bet), out=out)
            return out
        return _out_case(ref, launch)
    # widths outside 96 / 128 / 192 run the fp32 kernels of norm.hip in the split modes too (lane-per-token form: C % 8 == 0, C <= 120)
    mfma = C in (96, 128, 192)
    form = "LayerNorm output" + ("" if mfma else (", fp32 lane kernel" if C % 8 == 0 and C <= 120 else ", fp32 generic kernel"))
    return Site("tce_patch_embed_f32", form, "patch_embed.hip" if mfma else "norm.hip", "output", f"{T}x{H}x{W} -> {C}", targets(M, C),
                [("gamma", ALL)], make)


# ---------------------------------------------------------------------------------------------------------------------
# fused Swin attention half-block (csrc/swinattn.hip): qkv rows, attention output, final store
# ---------------------------------------------------------------------------------------------------------------------
def swin_site(T, H, W, C, shift, site, seed=12):
    """out = x + proj(window_attention(LayerNorm(x) Wqkv^T + bqkv)) + bproj.  The attention output is a convex combination of v rows
    (|att| <= max |v|), so the final store is x + bproj within +- max|v| * sum_j |Wproj[c, j]|: an interval reference.
    site = final: x[r, c] carries the target (LayerNorm makes that row one-hot-like: its qkv stays O(sqrt(C)));
    site = qkv:   qkv[r, j] carries it (x one-hot in row r, LayerNorm with gamma 1, Wqkv[j, c0] large); Wproj is scaled by 2^-10, so
                  the final store stays clean;
    site = att:   bounded by the v rows, so it cannot be isolated: a NaN in x reaches all three sites (recorded as such)."""
    M = T * H * W

    def make(t, cls, via):
        r, c = t
        g = torch.Generator().manual_seed(6000 + seed)
        nH = C // 32
        x = (torch.randn(M, C, generator=g) * 0.5).half().float()
        g1, b1 = torch.ones(C), torch.zeros(C)
        wqkv = (torch.randn(3 * C, C, generator=g) / math.sqrt(C)).half().float()
        bqkv = (torch.randn(3 * C, generator=g) * 0.25).half().float()
        table = torch.randn(169, nH, generator=g)
        wp = (torch.randn(C, C, generator=g) / math.sqrt(C) * 2.0 ** -10).half().float()
        bp = (torch.randn(C, generator=g) * 0.2).half().float()
        over, sgn = cls in ("over+", "over-"), (-1.0 if cls == "over-" else 1.0)
        special = {"inf": float("inf"), "nan": float("nan")}.get(cls)
        if site == "final":
            bp[c] = 0
            if special is not None:
                x[r, c] = special
            elif cls != "clean":
                x[r, c] = sgn * (60160.0 if over else 58880.0)
        elif site == "qkv":   # LayerNorm (gamma 1, beta 0) turns the one-hot row into sqrt(C - 1) at c0; Wqkv[c, c0] decides
            c0 = 3
            x[:, c0] = 0
            x[r] = 0
            x[r, c0] = 256.0
            wqkv[:, c0] = 2.0 ** -8
            if cls != "clean":
                wqkv[c, c0] = sgn * float(torch.tensor((63000.0 if over else 57000.0) / math.sqrt(C - 1)).half())
        else:
            x[r, c] = special
        xs = x.double().nan_to_num(0.0, 0.0, 0.0)
        y = F.layer_norm(xs, (C,), g1.double(), b1.double(), 1e-5)
        qkv = y @ wqkv.double().T + bqkv.double()
        bad_rows = ~torch.isfinite(x).all(1)
        qkv[bad_rows] = float("nan")
        vmax = max(qkv[:, 2 * C:][~bad_rows].abs().max(), bqkv[2 * C:].abs().max())     # pad tokens hold the qkv bias
        slack = vmax * wp.double().abs().sum(1)[None, :].expand(M, C)
        lo, hi = x.double() + bp.double() - slack, x.double() + bp.double() + slack
        if bool(bad_rows.any()):   # a NaN row poisons its whole window: any row may come back NaN
            lo = torch.full_like(lo, float("nan"))
            hi = lo
        tensors = [("qkv", qkv, qkv), ("out", lo, hi)]

        def launch(ops, lib, put):
            pk = ops.swin_attn_pack(put("wqkv", wqkv), put("wp", wp))
            out = put("out", torch.zeros(M, C))
            ops.swin_attn_fused(put("x", x), pk, put("bqkv", bqkv), put("bp", bp), put("table", table), put("g1", g1), put("b1", b1),
                                T, H, W, C, shift, out=out)
            return out
        nan_rows = tuple(range(M)) if bool(bad_rows.any()) else ()
        return Case(None, None, None, None, tensors, launch, nan_rows=nan_rows)
    if site == "qkv":
        # q, k and v columns (a v value over the limit may also pass the attention-output site: the expectation is the same)
        tg = [(0, 5), (M - 1, 3 * C - 1), (M // 2, C - 1), (5, C + 37), (M - 3, 2 * C - 1), (40, 2 * C + 33)]
        variants = [("product", ("over+", "over-", "under", "clean"))]
        kind, name = "intermediate", "qkv rows"
    elif site == "final":
        tg, variants, kind, name = targets(M, C, 32, 64), [("res", ALL)], "output", "final store"
    else:
        tg, variants, kind, name = [(0, 0), (M - 1, C - 1)], [("input", ("nan",))], "intermediate", "attention output (NaN only: bounded by v)"
    return Site("tce_swin_attn_fused_f32", name, "swinattn.hip", kind, f"{T}x{H}x{W} C={C} shift={shift}", tg, variants, make)


# ---------------------------------------------------------------------------------------------------------------------
# folded text cross-attention (tce_xattn_fused_f32) and its chain into an FFN (tce_xattn_ffn_fused_f32), csrc/ffn.hip
# ---------------------------------------------------------------------------------------------------------------------
def xattn_site(M, L, chain, seed=13):
    """out = x + att(x) + bo (xattn_fused, additive residual, no LayerNorm): the softmax weights are a convex combination per head, so
    |att[m, c]| <= sum_h max_l |(Wo_h v_h^T)[c, l]|: an interval reference; x[r, c] carries the target (Wq[:, c] = 0 keeps it out of
    the scores).  chain: Wo = 0 and bo = 0 make stage 1's pre-norm row x itself, one-hot in row r: `mid` stores sqrt(255) gamma[c]
    there, and the FFN stage's LayerNorm brings the final store back to O(1) (W1[:, c] = 0 keeps the 65408 out of its products)."""
    Cn, nh, Hd = 256, 8, 256

    def make(t, cls, via):
        r, c = t
        g = torch.Generator().manual_seed(7000 + seed)
        x = (torch.randn(M, Cn, generator=g) * 0.5).half().float()
        Wq, Wo = torch.randn(Cn, Cn, generator=g) * 0.06, torch.randn(Cn, Cn, generator=g) * 0.06
        bq, bo = torch.randn(Cn, generator=g) * 0.2, (torch.randn(Cn, generator=g) * 0.2).half().float()
        k, v = torch.randn(L, Cn, generator=g), torch.randn(L, Cn, generator=g)
        gam, bet = (torch.rand(Cn, generator=g) + 0.5).half().float(), (torch.randn(Cn, generator=g) * 0.2).half().float()
        W1, b1 = (torch.randn(Hd, Cn, generator=g) / 16).half().float(), (torch.randn(Hd, generator=g) * 0.2).half().float()
        W2, b2 = (torch.randn(Cn, Hd, generator=g) / 16).half().float(), (torch.randn(Cn, generator=g) * 0.2).half().float()
        g2, be2 = (torch.rand(Cn, generator=g) + 0.5).half().float(), (torch.randn(Cn, generator=g) * 0.2).half().float()
        over, sgn = cls in ("over+", "over-"), (-1.0 if cls == "over-" else 1.0)
        special = {"inf": float("inf"), "nan": float("nan")}.get(cls)
        Wq[:, c] = 0
        if not chain:
            bo[c] = 0
            if special is not None:
                x[r, c] = special
            elif cls != "clean":
                x[r, c] = sgn * (60160.0 if over else 58880.0)
            bound = sum((Wo[:, 32 * h:32 * h + 32].double() @ v[:, 32 * h:32 * h + 32].double().T).abs().amax(1) for h in range(nh))
            slack = bound[None, :].expand(M, Cn) * (1 + 1e-3)
            lo, hi = x.double() + bo.double() - slack, x.double() + bo.double() + slack
            tensors = [("out", lo, hi)]
            nan_rows = (r,) if special is not None else ()
        else:
            g_over, g_under = ln_gammas(Cn)
            Wo[:] = 0
            bo[:] = 0
            W1[:, c] = 0
            x[r] = 0
            x[r, c] = 256.0 if special is None else special
            if over:
                gam[c] = sgn * g_over
            elif cls == "under":
                gam[c] = g_under
            mid = F.layer_norm(x.double(), (Cn,), gam.double(), bet.double(), 1e-5)
            hdn = relu_fmax(mid.nan_to_num(0.0, 0.0, 0.0) @ W1.double().T + b1.double())
            pre = mid + hdn @ W2.double().T + b2.double()
            out = F.layer_norm(pre, (Cn,), g2.double(), be2.double(), 1e-5)
            tensors = [exact("mid", mid), exact("hidden", hdn), exact("out", out)]
            nan_rows = (r,) if special is not None else ()

        def launch(ops, lib, put):
            ar = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device="cuda")
            pk = ops.xattn_pack(put("k", k), put("v", v), ops.xattn_static(put("Wq", Wq), put("bq", bq)), put("Wo", Wo), L, ar)
            xd, out = put("x", x), put("out", torch.zeros(M, Cn))
            if not chain:
                ops.xattn_fused(xd, pk, put("bo", bo), M, out, res_mode=RES_ADD)
            else:
                midb = put("mid", torch.zeros(M, Cn))
                ops.xattn_fused(xd, pk, put("bo", bo), M, out, ln_out=(put("gam", gam), put("bet", bet)),
                                ffn=(ops.ffn_pack_chain(put("W1", W1), put("b1", b1), put("W2", W2)), put("b2", b2), Hd,
                                     (put("g2", g2), put("be2", be2)), midb, M * Cn))
            return out
        return Case(None, None, None, None, tensors, launch, nan_rows=nan_rows)
    if chain:
        return Site("tce_xattn_ffn_fused_f32", "chain mid", "ffn.hip", "intermediate", f"{M} rows, {L} keys", targets(M, Cn),
                    [("gamma", ("over+", "over-", "under", "nan", "clean"))], make)
    return Site("tce_xattn_fused_f32", "final store", "ffn.hip", "output", f"{M} rows, {L} keys", targets(M, Cn), [("res", ALL)], make)


# ---------------------------------------------------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------------------------------------------------
PLAIN = [("product", ALL), ("bias", ("over+", "over-", "under", "inf"))]
SITES = [
    # csrc/gemm_f16x3_kernel.h: one report, every tile
    gemm_site(130, 72, 64, 6464, "tile 6464", PLAIN + [("res_add", ALL), ("res_mul", ALL)], row_slice=32, rows_per_wg=64),
    gemm_site(130, 70, 64, 6464, "tile 6464, N % 4 != 0 (vec_ok false)", [("product", ALL), ("res_add", ("over+", "under", "nan"))],
              rows_per_wg=64),
    gemm_site(130, 72, 64, 6464, "tile 6464, GELU", [("product", ("over+", "under", "inf", "nan", "clean"))], act=ACT_GELU, rows_per_wg=64),
    gemm_site(130, 72, 64, 6464, "tile 6464, ReLU after RES_ADD", [("res_add", POS)], act=ACT_RELU_AFTER, rows_per_wg=64),
    gemm_site(6100, 512, 32, 12864, "tile 12864", [("product", ALL), ("res_add", ("over+", "under", "nan"))], rows_per_wg=128),
    gemm_site(49100, 256, 32, 256128, "tile 256128 (big_256_split / big_256_single by mode)",
              [("product", ("over+", "over-", "under", "nan", "clean")), ("res_add", ("over+", "under"))], row_slice=64, rows_per_wg=256),
    conv_site(1, 127, 129, 32, 256, 1, 128128, "conv tile 128128 (big_128_split / big_128_single by mode)",
              [("product", ("over+", "over-", "under", "nan", "clean")), ("bias", ("over+", "under"))]),
    gemm_site(67, 96, 64, 6464, "batch 2, strided output", [("product", ALL), ("res_add", ("over+", "under", "nan"))], batch=2, rows_per_wg=64),
    gemm_site(130, 72, 64, 6464, "a2 addend", [("product", ALL)], a2=True, rows_per_wg=64),
    conv_site(1, 9, 7, 64, 96, 3, 6464, "conv2d_cl 3x3", [("product", ALL), ("bias", ("over+", "under", "inf"))]),
    # csrc/gemm.hip: the fix-up pass and the three reduce kernels
    gemm_site(130, 72, 64, 6464, "epi_fix_kernel: GELU then RES_ADD", [("res_add", ("over+", "under", "inf", "nan", "clean"))],
              act=ACT_GELU, source="gemm.hip", rows_per_wg=64),
    gemm_site(130, 72, 64, 6464, "epi_fix_kernel: ReLU then RES_MUL", [("res_mul", ("over+", "under", "inf", "nan", "clean"))],
              act=ACT_RELU, source="gemm.hip", rows_per_wg=64),
    gemm_site(130, 72, 64, 6464, "epi_fix_kernel: RES_MUL then ReLU", [("res_mul", POS)], act=ACT_RELU_AFTER, source="gemm.hip",
              rows_per_wg=64),
    splitk_site(25, 256, 2048, 8, [("sum", ("over+", "over-", "under", "clean")), ("bias", ("over+", "over-", "under", "inf")),
                                   ("res_add", ALL), ("res_mul", ("over+", "under", "nan"))]),
    splitk_site(1, 768, 768, 2, [("sum", ("over+", "over-", "under", "clean")), ("bias", ("over+", "under", "inf")),
                                 ("res_add", ("over+", "under", "nan"))]),
    conv_site(1, 9, 7, 64, 96, 3, 6464, "conv2d_cl 3x3, split-K (splitk_reduce_kernel)", [("product", ("over+", "under", "nan", "clean")),
                                                                                        ("bias", ("over+", "over-", "under", "inf"))],
              splits=3, entry="tce_gemm_splitk_f32", source="gemm.hip"),
    splitk_ln_site(40, 1024, 512, 2, "splitk_reduce_ln_row_kernel"),
    splitk_ln_site(260, 256, 512, 2, "splitk_reduce_ln_kernel (M > 256)"),
    thin_reduce_site(7, 768, 768, [("sum", ("over+", "over-", "under", "clean")), ("bias", ("over+", "under", "inf")),
                                   ("res_add", ("over+", "under", "nan"))]),
    # csrc/thin.hip
    thin_chain_site(32, 768, 768, 64),
    # csrc/rowlin.hip
    *[rowlin_site(M, N, K, v) for (M, N, K) in [(129, 32, 96), (200, 256, 384), (130, 256, 512)]
      for v in ("plain", "a2_relu", "res_mul", "gelu_res", "ln_in", "ln_out")
      if v != "ln_out" or (N == 256 and K != 512)],          # the output LayerNorm is built for N = 256, K < 512
    rowlin_site(67, 32, 96, "res_mul", batch=2), rowlin_site(67, 32, 96, "a2_relu", batch=2),
    # csrc/ffn.hip
    ffn_site(333, 256, 64, "relu", "none", "hidden"), ffn_site(333, 256, 64, "relu", "none", "out"),
    ffn_site(333, 256, 64, "relu", "out", "ln_out"),
    ffn_site(300, 96, 384, "gelu", "in", "hidden"), ffn_site(300, 96, 384, "gelu", "in", "out"),
    ffn_site(300, 96, 384, "gelu", "in", "hidden", form="half"), ffn_site(300, 96, 384, "gelu", "in", "out", form="half"),
    ffn_site(4600, 256, 2048, "relu", "none", "hidden", form="split", tg=[(0, 0), (4599, 2047), (37, 1000), (4500, 1100)]),
    ffn_site(4600, 256, 2048, "relu", "none", "out", form="split", tg=[(0, 0), (4599, 255), (70, 100), (4550, 200)]),
    xattn_site(301, 11, chain=False), xattn_site(130, 8, chain=True),
    # csrc/conv3x3.hip
    conv3x3_site(1, 9, 13, 4, -1, [("product", ALL), ("bias", ("over+", "under", "inf"))]),
    conv3x3_site(3, 17, 5, 8, -1, [("product", ALL), ("bias", ("over+", "under", "inf"))]),
    conv3x3_site(3, 17, 5, 4, 2, [("sum", ("over+", "over-", "under", "clean")), ("bias", ("over+", "over-", "under", "inf")),
                                  ("product", ("nan",))]),
    # csrc/swinattn.hip
    swin_site(1, 7, 7, 128, 3, "final"), swin_site(1, 9, 13, 192, 3, "final"),
    swin_site(1, 7, 7, 128, 3, "qkv"), swin_site(1, 9, 13, 192, 3, "qkv"),
    swin_site(1, 7, 7, 128, 3, "att"),
    # csrc/patch_embed.hip
    patch_embed_site(1, 30, 41, 128), patch_embed_site(1, 8, 8, 32), patch_embed_site(1, 9, 10, 36),
]

R_EXACT = "exact fp32, no split operands"
R_CONVEX = "output is a convex combination of guarded values"
R_NOT = "not consumed by a split product"
R_OPEN = "consumed by a split product, not guarded"
UNGUARDED = {
    # packs and prepares: weights (checked on the host when packed, ops.check_weight_range) re-ordered or folded, no activations
    "tce_ffn_pack_f32": R_NOT, "tce_ffn_pack_batched_f32": R_NOT, "tce_ffn_pack_chain_f32": R_NOT, "tce_rowlin_pack_f32": R_NOT,
    "tce_conv3x3_pack_f32": R_NOT, "tce_swin_attn_pack_f32": R_NOT,
    "tce_xattn_prepare_f32": R_OPEN, "tce_xattn_pack_f32": R_OPEN, "tce_xattn_prepare_lens_f32": R_OPEN, "tce_xattn_pack_lens_f32": R_OPEN,
    # norms and resampling: fp32 arithmetic whose outputs feed split products
    "tce_layernorm_f32": R_OPEN, "tce_groupnorm_f32": R_OPEN, "tce_groupnorm_up_add_f32": R_OPEN, "tce_patch_merge_ln_f32": R_OPEN,
    "tce_resize_bilinear_ln_f32": R_OPEN, "tce_add_f32": R_OPEN, "tce_pos_sine2d_f32": R_OPEN, "tce_pos_sine2d_valid_f32": R_OPEN,
    "tce_embed_ln_f32": R_OPEN, "tce_embed_ln_seqs_f32": R_OPEN, "tce_resnet_stem_f32": R_OPEN, "tce_resize_v_norm_f32": R_OPEN,
    "tce_tanh_f32": R_OPEN,
    # selections / interpolations of guarded values
    "tce_maxpool3x3s2_cl_f32": R_CONVEX, "tce_resize_nearest_f32": R_CONVEX, "tce_resize_bilinear_f32": R_CONVEX, "tce_tile_f32": R_CONVEX,
    "tce_copy_segments": R_CONVEX,
    # attention cores and deformable attention
    "tce_window_attn_f32": R_CONVEX, "tce_window_attn3d_f32": R_CONVEX, "tce_mha_f32": R_CONVEX, "tce_mha_ws_f32": R_CONVEX,
    "tce_ms_deform_attn_forward_f32": R_CONVEX, "tce_msda_fused_f32": R_CONVEX, "tce_msda_fused_valid_f32": R_CONVEX,
    "tce_msda_fewq_raw_f32": R_CONVEX, "tce_mha_small64_f32": R_EXACT, "tce_mha_small64_seqs_f32": R_EXACT,
    "tce_mha_small64_lens_f32": R_EXACT, "tce_mha_small64_splits_f32": R_EXACT,
    "tce_fewrow_linear_f32": R_EXACT,
    # heads and output stages
    "tce_ms_deform_attn_backward_f32": R_NOT, "tce_resize_h_u8": R_NOT, "tce_contrastive_f32": R_NOT, "tce_sigmoid_f32": R_NOT,
    "tce_box_refine_f32": R_NOT, "tce_mask_pack_f32": R_NOT, "tce_mask_tail_f32": R_NOT, "tce_select_masks_u8": R_NOT,
    "tce_caption_lens_f32": R_NOT,
    "tce_vis_overlay_u8": R_NOT, "tce_png_filter_rgb_u8": R_NOT, "tce_png_deflate_rows_u8": R_NOT, "tce_png_file_u8": R_NOT,
    "tce_refexp_group_u8": R_NOT, "tce_refexp_giou_f32": R_NOT,
}
REASONS = (R_EXACT, R_CONVEX, R_NOT, R_OPEN)
