"""CPU: the designs, references and planted defects of tests/_window.py, proved on this machine before any GPU run.

  * plain fp32 torch -- in base e, and in the base-2 order of the 3-D split kernel -- is inside the derived bound of every
    (case, design) for both products' bounds (the split modes', which contains exact fp32's, and mode f16's): the designs are fair;
  * every planted defect is outside the bound at a named (case, design);
  * every design other than N has a defect that no other design catches;
  * the case table reaches the four key_tile bodies and the two-window-workgroup edge, the form table selects W1..W6;
  * G+ really leads by more than the mask's 100, G- by less, R^ really rises from key tile to key tile.

Two designs of the issue were built, measured and REMOVED under its own rule (a design that catches nothing new goes): T (q = 0,
table = 12 N(0,1): the relative-position index alone picks the winner) and P (the k bias large along u: padded keys lead every row
by ~40).  Against every planted defect each caught only what N already catches: the bound is tight enough (N's ratios for a wrong
index, a dropped padded key or a kept ragged slot are 4e3 .. 5e5) that any change of a probability by 1e-3 is far outside it.  T's
ratios were 20-30 x those of N on the index defects (bias_swapped 4.0e5 against 1.8e4, bias_shrunken_coords 5.4e5 against 1.6e4), P's
the same as N's on drop_padded_keys (6.3e4 against 5.2e5 at (1,1,1)): sharper, nothing new."""
import pytest
import torch

import _window as Wn

NH = 2
CASES = [("2d",) + c + (s,) for c, _ in Wn.CASES_2D for s in (0, 3)] + [("3d",) + c[:3] + (int(c[3]),) for c, _ in Wn.CASES_3D]
BOUND_MODES = ("f16x3", "f16")    # PRODUCT["f32"] is PRODUCT["f16x3"]

# the (case, design) at which each defect is held to ratio > 1 by name
NAMED = {
    "mask_inf": (("2d", 1, 7, 7, 3), "G+"),
    "mask_base2_units": (("2d", 2, 5, 6, 3), "G-"),
    "drop_padded_keys": (("2d", 1, 1, 1, 0), "U"),
    "ragged_kept": (("3d", 1, 3, 4, 0), "N"),
    "region_off_by_one": (("2d", 1, 3, 25, 3), "N"),
    "bias_shrunken_coords": (("3d", 4, 8, 6, 1), "N"),
    "bias_swapped": (("2d", 1, 7, 7, 0), "N"),
    "roll_reversed": (("3d", 9, 7, 7, 1), "N"),
    "temporal_shift_on_shrunken_d": (("3d", 8, 7, 7, 1), "N"),
    "max_frozen_first_tile": (("3d", 8, 7, 7, 1), "R^"),
    "max_from_last_tile": (("3d", 8, 7, 7, 1), "Rv"),
    "zero_score_is_absent": (("3d", 2, 2, 2, 0), "U"),
}
# the mask constants again on the 3-D path, in its own arithmetic order (emulate(base2=True): -144.2695 and its planted -100)
NAMED_3D = {
    "mask_inf": (("3d", 16, 14, 7, 1), "G+"),
    "mask_base2_units": (("3d", 16, 4, 4, 1), "G-"),
}
# design -> the defect that only it catches.  R^ / Rv: over the cases with neither a shift mask nor padded tokens -- a query whose
# whole first (last) tile is masked or padded has a stale maximum 100 (60..75) below its scores under ANY design
UNIQUE = {"G+": "mask_inf", "G-": "mask_base2_units", "U": "zero_score_is_absent", "R^": "max_frozen_first_tile",
          "Rv": "max_from_last_tile"}
PLAIN_ONLY = ("R^", "Rv")


@pytest.fixture(scope="module")
def matrix():
    """{(case, design): (operands, {mode: (ref, B)})} and {(defect, case, design): ratio under the split bound}."""
    refs, caught = {}, {}
    for c in CASES:
        lay = Wn.layout(*c)
        for d in Wn.DESIGNS:
            if not Wn.design_applies(d, lay):
                continue
            ops = Wn.operands(d, lay, NH)
            refs[(c, d)] = (ops, {m: Wn.core_ref_and_bound(lay, *ops, NH, m)[:2] for m in BOUND_MODES})
            ref, B = refs[(c, d)][1]["f16x3"]
            for df in Wn.DEFECTS:
                if c[0] == "2d" and df in Wn.ONLY_3D:
                    continue
                caught[(df, c, d)] = float(Wn.ratio(Wn.emulate(lay, *ops, NH, df), ref, B).max())
    return refs, caught


def test_form_table_selects_every_form():
    seen = set()
    for form, entry, dbg, modes in Wn.FORM_RUNS:
        for m in modes:
            assert Wn.window_form(entry, m, dbg) == form, (form, entry, dbg, m)
            seen.add(form)
    assert seen == set(Wn.FORMS)
    # the default switch: mode f32 stays on the exact kernels, the split modes leave them
    assert [Wn.window_form("2d", m) for m in Wn.MODES] == ["W2", "W3", "W3"]
    assert [Wn.window_form("3d", m) for m in Wn.MODES] == ["W4", "W5", "W5"]


def test_case_table_reaches_the_kernels_edges():
    bodies = set()
    for (T, H, W, sh), _ in Wn.CASES_3D:
        bodies |= Wn.key_tile_bodies(T, H, W, sh)
    assert bodies == {(False, False), (False, True), (True, False), (True, True)}
    assert Wn.key_tile_bodies(8, 4, 4, False) == {(False, False)}                       # N = 128: no ragged tile at all
    assert (True, False) in Wn.key_tile_bodies(16, 4, 4, True) and (True, True) not in Wn.key_tile_bodies(16, 4, 4, True)
    assert Wn.key_tile_bodies(1, 3, 4, False) == {(False, True)}                        # one tile, ragged
    # W3: a 2-D window is 49 keys in two tiles, the second ragged, masked in the last window row / column only
    assert Wn.key_tile_bodies(1, 14, 21, True, full_d=1, shrink=False) == {(False, False), (False, True), (True, False), (True, True)}
    # two windows (W6) / two (window, head) items (W2) per workgroup: an odd count above one, the last workgroup half empty
    assert Wn.windows_2d(1, 7, 15) == 3 and Wn.heads_2d(1, 7, 15) == 1
    for C in Wn.FUSED_C:
        cs = Wn.CASES_FUSED[C]
        assert len(cs) <= 3 and (1, 7, 15) in cs and any(H < 7 for _, H, _ in cs)
        assert all(any(c == k for k, _ in Wn.CASES_2D) for c in cs)
    pad = lambda T, H, W, sh: Wn.win3d(T, H, W, 8, 3 * sh, True)[2]
    assert max(pad(*c)[0] * pad(*c)[1] * pad(*c)[2] for c, _ in Wn.CASES_3D) == 24 * 14 * 6      # (17,8,6): the largest padded grid
    assert max(T * H * W for (T, H, W, _), _ in Wn.CASES_3D) < 2 ** Wn.CODE_BITS - 1
    # the [:N,:N] quirk is live only where a window is narrower than 7
    assert sum(1 for (T, H, W, sh), _ in Wn.CASES_3D if Wn.win3d(T, H, W, 8, 3 * sh, True)[0][2] < 7) >= 4


def test_fp32_is_inside_every_bound(matrix):
    """The fairness condition: the correct operation in fp32, in either arithmetic order, at ratio <= 1 everywhere."""
    refs, _ = matrix
    worst = 0.0
    for (c, d), (ops, by_mode) in refs.items():
        lay = Wn.layout(*c)
        for base2 in (False, True):
            out = Wn.emulate(lay, *ops, NH, base2=base2)
            for m, (ref, B) in by_mode.items():
                r = float(Wn.ratio(out, ref, B).max())
                worst = max(worst, r)
                assert r <= 1.0, f"{c} {d} [{m} bound] base2={base2}: fp32 torch at {r:.3g} of the bound"
    print(f"worst fp32 ratio over {len(refs)} (case, design): {worst:.3f}")


@pytest.mark.parametrize("C", Wn.FUSED_C)
def test_fused_fp32_is_inside_every_bound(C):
    for thw in Wn.CASES_FUSED[C]:
        for shift in (0, 3):
            lay = Wn.layout("2d", *thw, shift)
            for d in Wn.FUSED_DESIGNS:
                if not Wn.design_applies(d, lay):
                    continue
                ops = Wn.fused_operands(d, lay, C)
                out = Wn.fused_f32(lay, *ops)
                for m in BOUND_MODES:
                    ref, B, _ = Wn.fused_ref_and_bound(lay, *ops, m)
                    r = float(Wn.ratio(out, ref, B).max())
                    assert r <= 1.0, f"fused C={C} {thw} shift={shift} {d} [{m} bound]: fp32 torch at {r:.3g} of the bound"


def test_every_defect_is_caught_where_named(matrix):
    """Under the split modes' bound (which is exact fp32's too) every defect; under mode f16's every defect but the mask in
    base-2 units: a key at 4 % is inside what fp16 operands leave of a score of 66 (ratio 0.12).  The SINGLE template parameter of
    W3 / W5 changes the number of MFMAs per product, not the mask path, which the f16x3 run of the same template holds."""
    refs, caught = matrix
    assert set(NAMED) == set(Wn.DEFECTS)
    for df, (c, d) in NAMED.items():
        r = caught[(df, c, d)]
        ops, by_mode = refs[(c, d)]
        r16 = float(Wn.ratio(Wn.emulate(Wn.layout(*c), *ops, NH, df), *by_mode["f16"]).max())
        print(f"{df}: caught at {c} {d}, ratio {r:.3g} (f16 bound: {r16:.3g})")
        assert r > 1.0, f"{df} passes at {c} {d}: ratio {r:.3g}"
        assert r16 > 1.0 or df == "mask_base2_units", f"{df} passes the f16 bound at {c} {d}: ratio {r16:.3g}"


def test_mask_constants_are_held_on_the_3d_path(matrix):
    """The planted mask defects in the base-2 order of the 3-D split kernel are outside the bound at a named 3-D case, and the
    correct base-2 emulation is inside it there."""
    refs, _ = matrix
    for df, (c, d) in NAMED_3D.items():
        lay = Wn.layout(*c)
        ops, by_mode = refs[(c, d)]
        ref, B = by_mode["f16x3"]
        ok = float(Wn.ratio(Wn.emulate(lay, *ops, NH, base2=True), ref, B).max())
        bad = float(Wn.ratio(Wn.emulate(lay, *ops, NH, df, base2=True), ref, B).max())
        print(f"{df} (base 2): caught at {c} {d}, ratio {bad:.3g} (without the defect {ok:.3g})")
        assert ok <= 1.0 < bad, (df, c, d, ok, bad)


def test_every_design_runs_on_every_core_form():
    """The GPU module's forms x designs take their cases from here: no (2-D / 3-D, design) pair may be empty, and G+ / G- reach a
    3-D window with two regions of real tokens."""
    runs = Wn.design_runs()
    assert {(k, d) for d, k, *_ in runs} == {(k, d) for k in ("2d", "3d") for d in Wn.DESIGNS if d != "N"}
    for d in ("G+", "G-"):
        assert sum(1 for r in runs if r[0] == d and r[1] == "3d") >= 2
    assert all(c in CASES for c in Wn.DESIGN_CASES)


def test_every_design_has_a_defect_of_its_own(matrix):
    _, caught = matrix
    assert set(UNIQUE) == set(Wn.DESIGNS) - {"N"}
    for d, df in UNIQUE.items():
        def counts(c):
            lay = Wn.layout(*c)
            return not (d in PLAIN_ONLY and (lay.mask is not None or lay.padded))
        by = {dd for (f, c, dd), r in caught.items() if f == df and r > 1.0 and counts(c)}
        assert by == {d}, f"{df} is caught by {sorted(by)}, not by {d} alone"


def test_designs_do_what_they_say():
    for c in CASES:
        lay = Wn.layout(*c)
        real = lay.src >= 0
        for d in ("G+", "G-"):
            if not Wn.design_applies(d, lay):
                assert lay.mask is None or not lay.two_regions
                continue
            raw, _ = Wn.scores64(lay, *Wn.operands(d, lay, NH), NH)
            for w in lay.two_regions:
                same = (lay.reg[w][:, None] == lay.reg[w][None, :]) & real[w][None, :]
                other = ~(lay.reg[w][:, None] == lay.reg[w][None, :]) & real[w][None, :]
                lead = (raw[w].masked_fill(~other, -1e30).amax(-1) - raw[w].masked_fill(~same, -1e30).amax(-1))[:, real[w]]
                if d == "G+":
                    assert float(lead.min()) > 110.0, (c, w, float(lead.min()))      # the masked key wins by e^10 at least
                else:
                    assert 60.0 < float(lead.min()) and float(lead.max()) < 72.0, (c, w, float(lead.min()), float(lead.max()))
    # R^: the row maximum of every real query rises from every key tile to the next (13 tiles at N = 392); Rv: the first tile holds it
    lay = Wn.layout("3d", 8, 7, 7, 1)
    for d in ("R^", "Rv"):
        _, s = Wn.scores64(lay, *Wn.operands(d, lay, NH), NH)
        tmax = torch.stack([s[..., t * 32:(t + 1) * 32].amax(-1) for t in range(Wn.cdiv(lay.N, 32))], -1)
        assert tmax.shape[-1] == 13
        if d == "R^":
            assert bool((tmax[..., 1:] > tmax[..., :-1]).all()) and 59.0 < float(s.amax(-1).min()) and float(s.amax(-1).max()) < 80.0
        else:
            assert bool((tmax[..., 1:] < tmax[..., :1]).all())


def test_fused_mask_designs_keep_their_leads():
    for C in Wn.FUSED_C:
        for thw in Wn.CASES_FUSED[C]:
            lay = Wn.layout("2d", *thw, 3)
            if not lay.two_regions:
                continue
            nh = C // 32
            for d in ("G+", "G-"):
                x, g1, b1, wqkv, bqkv, table, _, _ = Wn.fused_operands(d, lay, C)
                raw, _ = Wn.scores64(lay, Wn.fused_qkv64(x, g1, b1, wqkv, bqkv), bqkv, table, nh)
                real = lay.src >= 0
                for w in lay.two_regions:
                    eq = lay.reg[w][:, None] == lay.reg[w][None, :]
                    other, same = ~eq & real[w][None, :], eq & real[w][None, :]
                    lead = (raw[w].masked_fill(~other, -1e30).amax(-1) - raw[w].masked_fill(~same, -1e30).amax(-1))[:, real[w]]
                    if d == "G+":
                        assert float(lead.min()) > 110.0, (C, thw, w, float(lead.min()))
                    else:
                        assert 64.0 < float(lead.min()) and float(lead.max()) < 75.0, (C, thw, w, float(lead.min()))


@pytest.mark.parametrize("C", Wn.FUSED_C)
def test_fused_bound_still_sees_the_mask_defects(C):
    """The fused form's bound is composed through LayerNorm and two projections and is looser on the attention core than the cores'
    own.  Under the split modes' bound it still separates -inf from -100 on G+, -100 in base-2 units on G-, and a dropped padded key
    on U.  Under mode f16's bound only U does, barely (measured: U 1.1 .. 2.8, G+ 0.2 .. 0.36, G- 0.03 .. 0.05; printed, not
    asserted): fp16 operands leave +-0.3 of a score of 130, and the bound of a one-hot row carries that in full.  The mask path of
    the kernel does not depend on SINGLE."""
    lay = Wn.layout("2d", 1, 7, 15, 3)
    for design, defect in (("G+", "mask_inf"), ("G-", "mask_base2_units"), ("U", "drop_padded_keys")):
        ops = Wn.fused_operands(design, lay, C)
        out = Wn.fused_f32(lay, *ops, defect=defect)
        r = {m: float(Wn.ratio(out, *Wn.fused_ref_and_bound(lay, *ops, m)[:2]).max()) for m in BOUND_MODES}
        print(f"fused C={C} {design} {defect}: ratio {r['f16x3']:.3g} (f16 bound: {r['f16']:.3g})")
        assert r["f16x3"] > 1.0, f"fused C={C}: {defect} passes on {design} (ratio {r['f16x3']:.3g})"
