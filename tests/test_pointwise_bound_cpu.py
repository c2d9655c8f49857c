"""CPU: what makes the bounds of tests/_pointwise.py mean something, shown with no kernel involved.  Each stage is emulated in torch
fp32 in the kernel's pass structure (mean, centred variance, apply; chunk partials, then Chan's merge; the resampling rule; the three
mask-head launches) on the operands test_pointwise_bound_gpu.py uses, at the smaller shapes of each list:
  (a) the correct emulation is inside every bound at every element of every design;
  (b) every planted defect is outside the bound by at least 4x on at least one design -- the ratio test_arith_bound_cpu.py demands of
      its mutants -- or is listed as not observable, with the reason.
The last test writes the table (family, mutant, design that catches it, worst err / B) to profiles/r28_pointwise_mutants.txt."""
import os

import pytest
import torch

import _pointwise as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "r28_pointwise_mutants.txt")
CATCH = 4.0
MUT = {}        # (family, mutant) -> {design: worst err / B over the shapes}
INSIDE = {}     # family -> worst err / B of the correct emulation
NOT_OBSERVABLE = {
    ("pos_sine2d", "no_1e-6"): "on an all-valid map the normaliser h + 1e-6 rounds to h in fp32 (1e-6 / h is below one rounding of the "
                               "argument); only the padded form divides by the bare 1e-6, and there the defect is a NaN",
}


def note(family, mutant, design, ratio):
    d = MUT.setdefault((family, mutant), {})
    d[design] = max(d.get(design, 0.0), ratio)


def inside(family, tag, out, ref, B):
    r = P.worst(out, ref, B)
    INSIDE[family] = max(INSIDE.get(family, 0.0), r)
    assert r <= 1.0, f"{family} {tag}: the correct fp32 emulation is outside the bound (err / B = {r:.3g})"


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", P.LN_C)
def test_layernorm(C):
    for M in (1, 7, 9, 17):
        for design in P.LN_DESIGNS:
            for eps in ((1e-5, 1e-12) if design == "epsprobe" else (1e-5,)):
                for with_r in (False, True):
                    x, r, g, b = P.ln_operands(design, M, C, 1000 * C + M, with_r)
                    ref, B, sig = P.ln_ref_bound(x, r, g, b, eps, P.ln_n(C))
                    assert float(sig.min()) > 1e-3, "the designs are well conditioned"
                    tag = f"{design}, eps {eps:g}" + (", +r" if with_r else "")
                    inside("layernorm", f"{M}x{C} [{tag}]", P.ln_emulate(x, r, g, b, eps), ref, B)
                    for m in P.LN_MUTANTS:
                        if m == "r_not_in_statistics" and not with_r:
                            continue
                        note("layernorm", m, tag, P.worst(P.ln_emulate(x, r, g, b, eps, m), ref, B))


def test_layernorm_offset_rows_put_a_one_pass_variance_outside_the_bound():
    """The design's purpose, per width of each of the three kernels: E[x^2] - mean^2 in fp32 on rows with mean / sigma = 800."""
    for C in (96, 256, 768):
        x, r, g, b = P.ln_operands("offset", 17, C, 1000 * C + 17, False)
        ref, B, _ = P.ln_ref_bound(x, None, g, b, 1e-5, P.ln_n(C))
        assert P.worst(P.ln_emulate(x, None, g, b, 1e-5, "one_pass_variance"), ref, B) > CATCH, C


def test_eps_probe_rows_move_by_tens_of_percent():
    x, _, g, b = P.ln_operands("epsprobe", 9, 256, 5, False)
    lo, hi = P.ln_ref_bound(x, None, g, b, 1e-12, 8)[0], P.ln_ref_bound(x, None, g, b, 1e-5, 8)[0]
    rel = ((lo - hi).abs() / (lo - P.d64(b)).abs().clamp_min(1e-30)).median()
    assert 0.1 < float(rel) < 0.9


@pytest.mark.parametrize("T,H,W,C", P.PM_SHAPES)
def test_patch_merge_ln(T, H, W, C):
    for design in ("unit", "offset"):
        x, g, b = P.pm_operands(design, T, H, W, C, 7 * H + W)
        rows, cnt = P.pm_rows(P.d64(x), T, H, W, C)
        ref, B, sig = P.ln_ref_bound(rows, None, g, b, 1e-5, P.pm_n(C))
        assert float(sig.min()) > 1e-3
        inside("patch_merge_ln", f"{T}x{H}x{W}x{C} [{design}]", P.pm_emulate(x, g, b, T, H, W, C, 1e-5), ref, B)
        for m in P.PM_MUTANTS:
            note("patch_merge_ln", m, design, P.worst(P.pm_emulate(x, g, b, T, H, W, C, 1e-5, m), ref, B))


def test_patch_merge_rows_hold_zero_quadrants():
    rows, cnt = P.pm_rows(torch.ones(5 * 7, 4), 1, 5, 7, 4)
    assert rows.shape == (12, 16) and sorted(set(cnt.flatten().tolist())) == [4.0, 8.0, 16.0]
    assert torch.equal(rows.sum(1, keepdim=True), cnt)


# ---------------------------------------------------------------------------------------------------------------
GN_CPU = [(256, G, HW) for G in P.GN_ROWS_G for HW in (7, 9, 513)] + [(256, 32, 3000), (256, 8, 4097)] \
    + [(C, G, HW) for C, G in P.GN_GENERIC for HW in (63, 513)] + [(64, 8, 3000)]


@pytest.mark.parametrize("C,G,HW", GN_CPU)
def test_groupnorm(C, G, HW):
    T = 3
    for design in P.GN_DESIGNS:
        x, g, b = P.gn_operands(design, T, HW, C, G, HW * 64 + G)
        ref, B, sig = P.gn_ref_bound(x, g, b, T, HW, C, G, 1e-5)
        assert float(sig.min()) > 1e-3
        inside("groupnorm", f"{T}x{HW}x{C}/{G} [{design}]", P.gn_emulate(x, g, b, T, HW, C, G, 1e-5), ref, B)
        inside("groupnorm", f"{T}x{HW}x{C}/{G} [{design}, relu]", P.gn_emulate(x, g, b, T, HW, C, G, 1e-5, relu=True), ref.clamp_min(0), B)
        for m in P.GN_MUTANTS:
            if m == "group_index_c_over_c8" and G != 32:
                continue
            note("groupnorm", m, design, P.worst(P.gn_emulate(x, g, b, T, HW, C, G, 1e-5, mutant=m), ref, B))


def test_groupnorm_chunking_is_the_kernels():
    assert [P.gn_rows_per(v) for v in (511, 512, 4095, 4096)] == [8, 32, 32, 128]
    assert P.gn_nsplit(14400) == 113 and P.gn_nsplit(3000) == 94 and P.gn_nsplit(4097) == 33 and P.gn_nsplit(511) == 64 and P.gn_nsplit(513) == 17
    assert P.gn_chunk_rows(513, 256, 32) == 32 and P.gn_chunk_rows(513, 256, 4) == 31      # the generic kernel re-derives its rows
    assert not P.gn_is_rows_kernel(256, 4) and not P.gn_is_rows_kernel(128, 32) and P.gn_is_rows_kernel(256, 64)
    assert P.gn_levels(14400) == 8 + 4 and P.gn_levels(3000) == 7 + 4 and P.gn_levels(7) == 1 + 4


def test_groupnorm_distinct_design_gives_every_slot_its_own_statistics():
    x, _, _ = P.gn_operands("distinct", 3, 513, 256, 32, 0)
    xx = x.view(3, 513, 32, 8)
    mean, std = xx.mean((1, 3)), xx.std((1, 3))
    for t in range(3):
        for g in range(32):
            assert abs(float(mean[t, g]) - 3 * ((2 * t + g) % 7 - 3)) < 0.5 * float(std[t, g]) + 0.3
            assert 0.8 < float(std[t, g]) / 2.0 ** ((t + g) % 5 - 2) < 1.25


@pytest.mark.parametrize("T,h,w,ho,wo", P.GN_UP_SIZES)
def test_groupnorm_up_add(T, h, w, ho, wo):
    C, G = 256, 8
    x, g, b = P.gn_operands("distinct", T, h * w, C, G, h * 100 + wo)
    add = torch.randn(T * ho * wo, C, generator=P.gen(wo))
    ref, B, _ = P.gn_up_ref_bound(x, g, b, add, T, h, w, ho, wo, C, G, 1e-5)
    inside("groupnorm_up_add", f"{T}x{h}x{w}->{ho}x{wo}", P.gn_up_emulate(x, g, b, add, T, h, w, ho, wo, C, G, 1e-5), ref, B)
    for m in P.NEAREST_MUTANTS:
        note("groupnorm_up_add", "nearest_" + m, f"distinct {h}x{w}->{ho}x{wo}",
             P.worst(P.gn_up_emulate(x, g, b, add, T, h, w, ho, wo, C, G, 1e-5, mutant=m), ref, B))


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,h,w,ho,wo", P.RESIZE_SIZES)
def test_resize(T, h, w, ho, wo):
    size = f"{h}x{w}->{ho}x{wo}"
    for C in (4, 64):
        x, add, _, _ = P.resize_operands(T, h, w, ho, wo, C, h * 1000 + wo + C)
        # nearest: the float32 rule is F.interpolate's, exactly
        ref_n = torch.nn.functional.interpolate(x.view(T, h, w, C).permute(0, 3, 1, 2), size=(ho, wo), mode="nearest")
        assert torch.equal(P.nearest_ref(x, T, h, w, ho, wo, C), ref_n.permute(0, 2, 3, 1).reshape(T * ho * wo, C))
        inside("resize_nearest", size, P.nearest_ref(x, T, h, w, ho, wo, C), ref_n.permute(0, 2, 3, 1).reshape(T * ho * wo, C),
               torch.zeros(T * ho * wo, C, dtype=torch.float64))
        for m in P.NEAREST_MUTANTS:
            same =torch.equal(P.nearest_ref(x, T, h, w, ho, wo, C, m), P.nearest_ref(x, T, h, w, ho, wo, C))
            note("resize_nearest", m, size, 0.0 if same else float("inf"))
        for a in (None, add):
            ref, B = P.bilinear_ref_bound(x, T, h, w, ho, wo, C, a)
            inside("resize_bilinear", f"{size} C={C}", P.bilinear_emulate(x, T, h, w, ho, wo, C, a), ref, B)
            for m in P.BILINEAR_MUTANTS:
                note("resize_bilinear", m, size, P.worst(P.bilinear_emulate(x, T, h, w, ho, wo, C, a, m), ref, B))
        # and the fp64 restatement of the rule is F.interpolate's
        ref_b = torch.nn.functional.interpolate(x.double().view(T, h, w, C).permute(0, 3, 1, 2), size=(ho, wo), mode="bilinear", align_corners=False)
        got = P.bilinear_ref_bound(x, T, h, w, ho, wo, C)[0]
        assert float((got - ref_b.permute(0, 2, 3, 1).reshape(T * ho * wo, C)).abs().max()) < 1e-12


@pytest.mark.parametrize("T,h,w,ho,wo", P.RESIZE_SIZES)
def test_resize_bilinear_ln(T, h, w, ho, wo):
    C = 256
    for design in ("unit", "offset"):
        x, add, g, b = P.resize_operands(T, h, w, ho, wo, C, h * 1000 + wo, design)
        ref, B, sig = P.bilinear_ln_ref_bound(x, T, h, w, ho, wo, C, add, g, b, 1e-5)
        assert float(sig.min()) > 1e-3
        emu = lambda m_res=None, m_ln=None: P.ln_emulate(P.bilinear_emulate(x, T, h, w, ho, wo, C, add, m_res), None, g, b, 1e-5, m_ln)
        inside("resize_bilinear_ln", f"{h}x{w}->{ho}x{wo} [{design}]", emu(), ref, B)
        for m in P.BILINEAR_MUTANTS:
            note("resize_bilinear_ln", m, f"{design} {h}x{w}->{ho}x{wo}", P.worst(emu(m_res=m), ref, B))
        note("resize_bilinear_ln", "one_pass_variance", design, P.worst(emu(m_ln="one_pass_variance"), ref, B))


def test_nearest_rule_lands_on_integers():
    """o * n / no is an integer for some o in the 2x, identity and 3x3 -> 3x3 cases and in 13 -> 6 never; the float32 products decide."""
    assert P.nearest_index(6, 12).tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5]
    assert P.nearest_index(7, 7).tolist() == list(range(7))
    assert P.nearest_index(13, 6).tolist() == [0, 2, 4, 6, 8, 10]
    assert P.nearest_index(5, 11).tolist() == [0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4]


# ---------------------------------------------------------------------------------------------------------------
def _pos_cases():
    for F in P.POS_F:
        for T, h, w in P.POS_SIZES:
            yield F, T, h, w, h, w
        for h, w, hv, wv in P.POS_PADDED:
            yield F, 2, h, w, hv, wv


def test_pos_sine2d():
    for F, T, h, w, hv, wv in _pos_cases():
        padded = (hv, wv) != (h, w)
        for add in (None, torch.randn(2 * F, generator=P.gen(F + h))):
            ref, B = P.pos_ref_bound(T, h, w, F, hv, wv, add)
            tag = f"{T}x{h}x{w} valid {hv}x{wv} F={F}"
            inside("pos_sine2d", tag, P.pos_emulate(T, h, w, F, hv, wv, add), ref, B)
            for m in P.POS_MUTANTS:
                if m == "no_1e-6" and padded:
                    continue    # NaN there: see NOT_OBSERVABLE
                note("pos_sine2d", m, "padded" if padded else "all valid", P.worst(P.pos_emulate(T, h, w, F, hv, wv, add, m), ref, B))
    assert max(MUT[("pos_sine2d", "no_1e-6")].values()) <= 1.0, "the 1e-6 of the normaliser became observable: drop it from NOT_OBSERVABLE"


def test_pos_sine2d_restatement_is_the_oracles():
    from oracle import tce_oracle as O
    mask = torch.ones(2, 9, 13, dtype=torch.bool)
    mask[:, :7, :10] = False
    theirs = O.pos_sine_2d(mask, 128).permute(0, 2, 3, 1)
    ref, B = P.pos_ref_bound(2, 9, 13, 128, 7, 10)
    ours, B = ref.view(2, 9, 13, 256)[:, :7, :10], B.view(2, 9, 13, 256)[:, :7, :10]
    assert bool(((theirs[:, :7, :10].double() - ours).abs() <= B).all())
    assert P.POS_K == 13


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nl,T,Q,h,w", P.MASK_SHAPES)
def test_mask_head(nl, T, Q, h, w):
    for Cm in P.MASK_CM:
        for scale in P.MASK_PARAM_SCALES:
            for stride in P.MASK_STRIDES:
                feats, params, refs, img = P.mask_operands(nl, T, Q, h, w, Cm, scale, Q * 10 + Cm)
                assert 0.0 in refs[..., :2] and 1.0 in refs[..., :2]
                ref, B = P.mask_ref_bound(feats, params, refs, img, stride, Cm)
                design = f"params x {scale:g}"
                inside("mask_head", f"{nl}x{T}x{Q}x{h}x{w} Cm={Cm} [{design}]", P.mask_emulate(feats, params, refs, img, stride, Cm), ref, B)
                for m in P.MASK_MUTANTS:
                    note("mask_head", m, design, P.worst(P.mask_emulate(feats, params, refs, img, stride, Cm, m), ref, B))


def test_mask_head_restatement_is_the_oracles():
    from oracle import tce_oracle as O
    nl, T, Q, h, w, Cm = 3, 2, 5, 18, 25, 16
    feats, params, refs, img = P.mask_operands(nl, T, Q, h, w, Cm, 0.2, 3)
    ref, B = P.mask_ref_bound(feats, params, refs, img, 4, Cm)
    o64 = P.mask_ref(feats, params, refs, img, 4, Cm)
    assert o64.dtype == torch.float64 and float((o64 - ref).abs().max()) <= 1e-11 * float(ref.abs().max())
    o32 = torch.stack([O.dynamic_mask_head(O.OracleConfig(mask_dim=Cm), feats, params[l], refs[l, :, :2], img) for l in range(nl)])
    assert o32.dtype == torch.float32 and bool(((o32.double() - ref).abs() <= B).all())     # equal to fp32 rounding


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,S,C,fpc", P.CONTRASTIVE_CASES)
def test_contrastive(T, S, C, fpc):
    mem, sent = P.contrastive_operands(T, S, C, fpc, T * S)
    ref, B = P.contrastive_ref_bound(mem, sent, fpc)
    expect = torch.nn.functional.cosine_similarity(mem.double().mean(1), sent.double().repeat_interleave(fpc, 0), dim=1, eps=1e-6)
    assert float((ref - expect).abs().max()) <= 1e-12 * max(1.0, float(expect.abs().max()))
    clamp = T > 1
    inside("contrastive", f"{T}x{S}x{C}/{fpc}", P.contrastive_emulate(mem, sent, fpc), ref, B)
    for m in P.CONTRASTIVE_MUTANTS:
        note("contrastive", m, "a clamped norm" if clamp else "plain", P.worst(P.contrastive_emulate(mem, sent, fpc, m), ref, B))


# ---------------------------------------------------------------------------------------------------------------
def test_zz_every_mutant_is_caught_and_write_profile():
    want = {("layernorm", m) for m in P.LN_MUTANTS} | {("patch_merge_ln", m) for m in P.PM_MUTANTS} | {("groupnorm", m) for m in P.GN_MUTANTS} \
        | {("groupnorm_up_add", "nearest_" + m) for m in P.NEAREST_MUTANTS} | {("resize_nearest", m) for m in P.NEAREST_MUTANTS} \
        | {("resize_bilinear", m) for m in P.BILINEAR_MUTANTS} | {("resize_bilinear_ln", m) for m in P.BILINEAR_MUTANTS} \
        | {("pos_sine2d", m) for m in P.POS_MUTANTS} | {("mask_head", m) for m in P.MASK_MUTANTS} | {("contrastive", m) for m in P.CONTRASTIVE_MUTANTS}
    assert want <= set(MUT), f"run the whole module; missing {sorted(want - set(MUT))}"
    assert set(INSIDE) == set(P.FAMILIES), sorted(set(P.FAMILIES) ^ set(INSIDE))
    lines, missed = [], []
    for (fam, m), by in sorted(MUT.items()):
        design, r = max(by.items(), key=lambda kv: kv[1])
        if (fam, m) in NOT_OBSERVABLE:
            assert r <= 1.0, (fam, m, r)
            lines.append(f"{fam} | {m} | not observable: {NOT_OBSERVABLE[(fam, m)]} | {r:.3g}")
            continue
        if r < CATCH:
            missed.append((fam, m, design, r))
        seen = sorted(d for d, v in by.items() if v >= CATCH)
        lines.append(f"{fam} | {m} | {design} | {r:.3g} | caught at >= {CATCH:g}x by {len(seen)} of {len(by)} designs")
    assert not missed, f"no design puts these defects {CATCH:g}x outside the bound: {missed}"
    with open(PROFILE, "w") as f:
        f.write("# tests/test_pointwise_bound_cpu.py: planted defects of the fp32 CPU emulations against the bounds of tests/_pointwise.py.\n"
                "# family | mutant | design with the worst element | worst err/B there | designs that catch it\n"
                "# (inf: NaN, or a mismatch of an exact comparison)\n")
        f.write("\n".join(lines) + "\n")
        f.write("# correct emulation, worst err/B over every design and shape (must be <= 1)\n")
        for fam in P.FAMILIES:
            f.write(f"{fam} | correct | {INSIDE[fam]:.3g}\n")
