"""GPU: the launches of csrc/norm.hip and csrc/misc.hip that sit between the matrix products -- row LayerNorm (its three kernels, with
and without the residual, in place), the patch-merge LayerNorm, GroupNorm (both statistics kernels, every chunk size, the Chan merge
past 64 partials, the up-sampling apply), nearest / bilinear resampling (plain, + add, + add + LayerNorm), the sine position maps, the
dynamic mask head (mask_pack -> gemm_batched -> mask_tail) and the contrastive cosine -- against fp64 references, EVERY output
element under the per-element bound of tests/_pointwise.py (derived from each kernel's operation order; nothing fitted), on inputs
that make a wrong kernel's error large while the rows stay well conditioned (sigma asserted): a common offset of 800 sigma, four
decades along the channels, rows whose variance is comparable to eps, (frame, group) slots with statistics of their own.
tests/test_pointwise_bound_cpu.py shows that a correct fp32 evaluation is inside these bounds and each planted defect is outside.

Every case appends (family, shape, design, max err / B) to a table the last test writes to profiles/r28_pointwise_bound_by_family.txt."""
import os

import pytest
import torch

import _pointwise as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "r28_pointwise_bound_by_family.txt")
RESULTS = []
NSPLIT_OVER_64 = set()     # statistics kernels that ran with more than 64 partials per (frame, group)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from tce_rvos_amd import ops as _ops
    return _ops


@pytest.fixture(autouse=True)
def _range_flag_stays_clean(ops):
    ops.check_range()
    yield
    ops.check_range()   # no case may raise the range flag


def dev(t):
    return None if t is None else t.cuda().contiguous()


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def check(family, shape, design, out, ref, B):
    return P.check(RESULTS, family, shape, design, out, ref, B)


# ---------------------------------------------------------------------------------------------------------------
# 1. layernorm
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", P.LN_C)
def test_layernorm(ops, C):
    n = P.ln_n(C)
    for M in P.LN_M:
        for design in P.LN_DESIGNS:
            for eps in ((1e-5, 1e-12) if design == "epsprobe" else (1e-5,)):
                for with_r in (False, True):
                    x, r, g, b = P.ln_operands(design, M, C, 1000 * C + M, with_r)
                    ref, B, sig = P.ln_ref_bound(x, r, g, b, eps, n)
                    assert float(sig.min()) > 1e-3
                    dx, dr, dg, db = dev(x), dev(r), dev(g), dev(b)
                    out = ops.layernorm(dx, dg, db, eps, r=dr)
                    check("layernorm", f"{M}x{C}", f"{design}, eps {eps:g}" + (", +r" if with_r else ""), out, ref, B)
                    assert torch.equal(dx.cpu(), x), "the input was written"
                    xc = dx.clone()                                      # the pipeline's form: out = x
                    assert ops.layernorm(xc, dg, db, eps, r=dr, out=xc) is xc
                    assert same_bits(xc, out), f"layernorm {M}x{C} [{design}]: in place differs from out of place"


# ---------------------------------------------------------------------------------------------------------------
# 2. patch_merge_ln
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,H,W,C", P.PM_SHAPES)
def test_patch_merge_ln(ops, T, H, W, C):
    for design in ("unit", "offset"):
        x, g, b = P.pm_operands(design, T, H, W, C, 7 * H + W)
        rows, _ = P.pm_rows(P.d64(x), T, H, W, C)          # the zero quadrants of odd H / W are part of the row
        ref, B, sig = P.ln_ref_bound(rows, None, g, b, 1e-5, P.pm_n(C))
        assert float(sig.min()) > 1e-3
        out, H2, W2 = ops.patch_merge_ln(dev(x), dev(g), dev(b), T, H, W, C)
        assert (H2, W2) == ((H + 1) // 2, (W + 1) // 2)
        check("patch_merge_ln", f"{T}x{H}x{W}x{C}", design, out, ref, B)


# ---------------------------------------------------------------------------------------------------------------
# 3. groupnorm_cl
# ---------------------------------------------------------------------------------------------------------------
def _groupnorm_case(ops, T, HW, C, G, designs=P.GN_DESIGNS):
    from tce_rvos_amd._lib import lib
    ns = lib().tce_groupnorm_nsplit(HW)
    assert ns == P.gn_nsplit(HW)
    if ns > 64:
        NSPLIT_OVER_64.add("rows" if P.gn_is_rows_kernel(C, G) else "generic")
    for design in designs:
        x, g, b = P.gn_operands(design, T, HW, C, G, HW * 64 + G)
        ref, B, sig = P.gn_ref_bound(x, g, b, T, HW, C, G, 1e-5)
        assert float(sig.min()) > 1e-3
        dx, dg, db = dev(x.view(T * HW, C)), dev(g), dev(b)
        for relu in (False, True):
            out = ops.groupnorm_cl(dx, dg, db, T, HW, C, G, relu=relu)
            check("groupnorm", f"{T}x{HW}x{C}/{G}", design + (", relu" if relu else ""), out, (ref.clamp_min(0) if relu else ref).view(T * HW, C),
                  B.view(T * HW, C))


@pytest.mark.parametrize("HW", P.GN_ROWS_HW)
@pytest.mark.parametrize("G", P.GN_ROWS_G)
def test_groupnorm_rows_kernel(ops, G, HW):
    _groupnorm_case(ops, 3, HW, 256, G)


@pytest.mark.parametrize("HW", P.GN_GENERIC_HW)
@pytest.mark.parametrize("C,G", P.GN_GENERIC)
def test_groupnorm_generic_kernel(ops, C, G, HW):
    assert not P.gn_is_rows_kernel(C, G)
    _groupnorm_case(ops, 3, HW, C, G)


@pytest.mark.parametrize("C,G", [(256, 32), (64, 8)])
def test_groupnorm_113_partials(ops, C, G):
    """HW = 14400 (a 90 x 160 map): 113 chunks of 128 rows, the merge loop's second trip -- in the rows kernel and the generic one."""
    _groupnorm_case(ops, 1, 14400, C, G, designs=("distinct", "offset"))


# ---------------------------------------------------------------------------------------------------------------
# 4. groupnorm_up_add
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,h,w,ho,wo", P.GN_UP_SIZES)
@pytest.mark.parametrize("G", [8, 32])
def test_groupnorm_up_add(ops, G, T, h, w, ho, wo):
    C = 256
    x, g, b = P.gn_operands("distinct", T, h * w, C, G, h * 100 + wo)
    add = torch.randn(T * ho * wo, C, generator=P.gen(wo))
    ref, B, sig = P.gn_up_ref_bound(x, g, b, add, T, h, w, ho, wo, C, G, 1e-5)
    assert float(sig.min()) > 1e-3
    dx, dg, db, dadd = dev(x.view(T * h * w, C)), dev(g), dev(b), dev(add)
    out = ops.groupnorm_up_add(dx, dg, db, T, h, w, ho, wo, C, G, dadd, torch.empty_like(dadd))
    check("groupnorm_up_add", f"{T}x{h}x{w}->{ho}x{wo} /{G}", "distinct", out, ref, B)
    two = ops.resize_nearest(ops.groupnorm_cl(dx, dg, db, T, h * w, C, G, relu=True), T, h, w, ho, wo, C, add=dadd)
    assert same_bits(out, two), "the fused launch differs from groupnorm_cl + resize_nearest"
    alias = dadd.clone()
    ops.groupnorm_up_add(dx, dg, db, T, h, w, ho, wo, C, G, alias, alias)
    assert same_bits(alias, out), "out aliasing add differs"


# ---------------------------------------------------------------------------------------------------------------
# 5. resize_nearest, resize_bilinear, resize_bilinear(ln=...)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,h,w,ho,wo", P.RESIZE_SIZES)
@pytest.mark.parametrize("C", P.RESIZE_C)
def test_resize(ops, C, T, h, w, ho, wo):
    x, add, _, _ = P.resize_operands(T, h, w, ho, wo, C, h * 1000 + wo + C)
    dx, dadd = dev(x), dev(add)
    shape = f"{T}x{h}x{w}->{ho}x{wo} C={C}"
    # nearest: exact
    want = P.nearest_ref(x, T, h, w, ho, wo, C)
    out = ops.resize_nearest(dx, T, h, w, ho, wo, C)
    assert same_bits(out.cpu(), want), f"resize_nearest {shape}"
    check("resize_nearest", shape, "unit", out, want, torch.zeros_like(want, dtype=torch.float64))
    out = ops.resize_nearest(dx, T, h, w, ho, wo, C, add=dadd)
    assert same_bits(out.cpu(), want + add), f"resize_nearest {shape} + add"
    check("resize_nearest", shape, "unit, + add", out, want + add, torch.zeros_like(want, dtype=torch.float64))
    alias = dadd.clone()
    ops.resize_nearest(dx, T, h, w, ho, wo, C, add=alias, out=alias)
    assert same_bits(alias, out), "out aliasing add differs"
    # bilinear: under the bound
    for a, tag in ((None, "unit"), (dadd, "unit, + add")):
        ref, B = P.bilinear_ref_bound(x, T, h, w, ho, wo, C, None if a is None else add)
        out = ops.resize_bilinear(dx, T, h, w, ho, wo, C, add=a)
        check("resize_bilinear", shape, tag, out, ref, B)
    alias = dadd.clone()
    ops.resize_bilinear(dx, T, h, w, ho, wo, C, add=alias, out=alias)
    assert same_bits(alias, out), "out aliasing add differs"
    assert torch.equal(dx.cpu(), x)


@pytest.mark.parametrize("T,h,w,ho,wo", P.RESIZE_SIZES)
def test_resize_bilinear_ln(ops, T, h, w, ho, wo):
    C = 256
    assert ops.RESIZE_LN_FUSE, "the fused launch is what this test holds"
    for design in ("unit", "offset"):
        x, add, g, b = P.resize_operands(T, h, w, ho, wo, C, h * 1000 + wo, design)
        ref, B, sig = P.bilinear_ln_ref_bound(x, T, h, w, ho, wo, C, add, g, b, 1e-5)
        assert float(sig.min()) > 1e-3
        dx, dadd, dg, db = dev(x), dev(add), dev(g), dev(b)
        out = ops.resize_bilinear(dx, T, h, w, ho, wo, C, add=dadd, ln=(dg, db))
        check("resize_bilinear_ln", f"{T}x{h}x{w}->{ho}x{wo}", design, out, ref, B)
        alias = dadd.clone()
        ops.resize_bilinear(dx, T, h, w, ho, wo, C, add=alias, out=alias, ln=(dg, db))
        assert same_bits(alias, out), "out aliasing add differs"


# ---------------------------------------------------------------------------------------------------------------
# 6. pos_sine2d and its padded form
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", P.POS_F)
def test_pos_sine2d(ops, F):
    cases = [(T, h, w, None) for T, h, w in P.POS_SIZES] + [(2, h, w, (hv, wv)) for h, w, hv, wv in P.POS_PADDED]
    for T, h, w, valid in cases:
        for add in (None, torch.randn(2 * F, generator=P.gen(F + h))):
            hv, wv = valid or (h, w)
            ref, B = P.pos_ref_bound(T, h, w, F, hv, wv, add)
            out = ops.pos_sine2d(T, h, w, F, "cuda", add=dev(add), valid=valid)
            assert bool(torch.isfinite(out).all())
            check("pos_sine2d", f"{T}x{h}x{w} F={F}", ("all valid" if valid is None else f"valid {hv}x{wv}") + (", + add" if add is not None else ""),
                  out, ref, B)


# ---------------------------------------------------------------------------------------------------------------
# 7. mask head
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nl,T,Q,h,w", P.MASK_SHAPES)
@pytest.mark.parametrize("Cm", P.MASK_CM)
def test_mask_head(ops, Cm, nl, T, Q, h, w):
    for scale in P.MASK_PARAM_SCALES:
        for stride in P.MASK_STRIDES:
            feats, params, refs, img = P.mask_operands(nl, T, Q, h, w, Cm, scale, Q * 10 + Cm)
            assert 0.0 in refs[..., :2] and 1.0 in refs[..., :2]
            ref, B = P.mask_ref_bound(feats, params, refs, img, stride, Cm)
            o64 = P.mask_ref(feats, params, refs, img, stride, Cm)         # the oracle in fp64 is the reference; the restatement carries the bound
            assert float((o64 - ref).abs().max()) <= 1e-11 * max(1.0, float(ref.abs().max()))
            feats_cl = dev(feats.permute(0, 2, 3, 1).reshape(T, h * w, Cm))
            w0f = torch.empty(T, nl * Q * 8, Cm, device="cuda")
            tail = torch.empty(nl, T * Q, 112, device="cuda")
            ops.mask_pack(dev(params), nl, T, Q, Cm, w0f, tail)
            G = torch.empty(T, h * w, nl * Q * 8, device="cuda")
            ops.gemm_batched(feats_cl, w0f, G)
            masks = torch.empty(nl, T, Q, h, w, device="cuda")
            ops.mask_tail(G, tail, dev(refs), 4, masks, nl, T, Q, h, w, img[0], img[1], stride)
            check("mask_head", f"{nl}x{T}x{Q}x{h}x{w} Cm={Cm} stride {stride}", f"params x {scale:g}", masks.view(nl, T * Q, h, w), o64, B)


# ---------------------------------------------------------------------------------------------------------------
# 8. contrastive
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,S,C,fpc", P.CONTRASTIVE_CASES)
def test_contrastive(ops, T, S, C, fpc):
    mem, sent = P.contrastive_operands(T, S, C, fpc, T * S)
    ref, B = P.contrastive_ref_bound(mem, sent, fpc)
    out, ws = torch.empty(T, device="cuda"), torch.empty(T * 32 * C, device="cuda")
    ops.contrastive(dev(mem), dev(sent), T, S, C, fpc, out, ws)
    check("contrastive", f"{T}x{S}x{C}/{fpc}", "a clamped norm" if T > 1 else "plain", out, ref, B)


# ---------------------------------------------------------------------------------------------------------------
def test_zz_write_profile(ops):
    """Writes the table of every case above (run the whole module: each family test appends its lines)."""
    ran = {r[0] for r in RESULTS}
    assert set(P.FAMILIES) <= ran, f"families that did not run: {sorted(set(P.FAMILIES) - ran)}"
    assert NSPLIT_OVER_64 == {"rows", "generic"}, f"more than 64 partials reached only {sorted(NSPLIT_OVER_64)}"
    assert all(r[3] <= 1.0 for r in RESULTS)
    with open(PROFILE, "w") as f:
        f.write("# tests/test_pointwise_bound_gpu.py on an MI355X: per case, the largest |out - fp64 ref| / B over EVERY output element, B the\n"
                "# per-element bound of tests/_pointwise.py (0 for the exact comparisons of resize_nearest).\n"
                "# family | worst case of the family: shape | design | max err/B\n")
        for fam in P.FAMILIES:
            w = max((r for r in RESULTS if r[0] == fam), key=lambda r: r[3])
            f.write(f"{fam} | worst of {sum(r[0] == fam for r in RESULTS)} cases: {w[1]} | {w[2]} | {w[3]:.3f}\n")
        f.write("# family | shape | design | max err/B\n")
        for fam, shape, design, rB in RESULTS:
            f.write(f"{fam} | {shape} | {design} | {rB:.3f}\n")
