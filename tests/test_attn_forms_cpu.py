"""CPU: the case table, masks, score designs and bound of tests/_attn.py do what test_attn_forms_gpu.py relies on, shown with no
kernel involved.  The case table reaches every launch form in every mode it has and both sides of every threshold; every mask has
its property; the reference equals fp64 softmax(masked_fill(-inf)) @ v; plain fp32 torch is inside the (margin-free) bound at every
element of every mask and score design; and each planted defect is outside it somewhere in every design that is listed as seeing it.
A (design, defect) pair that is NOT listed is a blind spot of that design, stated here instead of passing quietly:
  * a leaked key under S2 with a masked tail (the tail's probabilities are ~ e^-50): S2 runs with the head mask instead;
  * a leaked key other than the lowest-indexed masked one under S2 / S3 (far behind the leaders);
  * a dropped tile under S1 unless it is the last kept tile, under S2 unless the first, under S3 unless it holds the leader (not listed);
  * a merge weight of 1 under S4 (all maxima tie, the right weight IS 1), for the wave that holds the row maximum, or for a wave
    whose keys are all masked (its partial is zero)."""
import pytest
import torch

import _arith as A
import _attn as T

F1, F5 = T.case("F1"), T.case("F5")


def _worst(out, ref, B):
    return T.ratio(out, ref, B).max().item()


# ---------------------------------------------------------------------------------------------------------------
# The case table
# ---------------------------------------------------------------------------------------------------------------
def test_cases_reach_every_form_in_every_mode():
    want = {(f, m) for f in ("F1", "F2") for m in T.MODES} | {(f, m) for f in ("F3", "F4", "F5", "F6", "F7") for m in T.SPLIT_MODES}
    got = set()
    for name, batch, nh, Lq, Lk, ws, modes in T.CASES:
        for mode in modes:
            form = T.mha_form(batch, nh, Lq, Lk, mode, ws)
            assert name.startswith(form), (name, mode, form)     # a case runs the form it is named after, in every mode it lists
            got.add((form, mode))
    assert got == want, sorted(want ^ got)


def test_cases_sit_on_both_sides_of_every_threshold():
    from tce_rvos_amd import ops
    forms = {}
    for name, batch, nh, Lq, Lk, ws, modes in T.CASES:
        tiles = T.cdiv(Lq, 32) * batch * nh
        forms[(tiles, Lk, ws)] = T.mha_form(batch, nh, Lq, Lk, "f16x3", ws)
    assert forms[(3968, 33, False)] == "F1" and forms[(4096, 33, False)] == "F2"          # 4096 tiles
    assert forms[(18, 255, False)] == "F1" and forms[(18, 256, False)] == "F3"            # 256 keys
    assert forms[(18, 1023, False)] == "F3" and forms[(18, 1024, False)] == "F5"          # 1024 keys
    assert ops.MHA_WS_MIN_KEYS == 1024, "the table's workspace threshold cases assume the default"
    assert forms[(18, ops.MHA_WS_MIN_KEYS - 1, True)] == "F3" and forms[(18, ops.MHA_WS_MIN_KEYS, True)] == "F6"
    assert forms[(18, 1025, True)] == "F6" and forms[(4096, 1025, True)] == "F7"          # 4096 tiles, workspace form
    assert T.mha_form(2, 3, 77, 1025, "f32", True) == "F1"                                # exact mode never takes the workspace form


def test_f5_waves_own_the_tiles_the_table_says():
    assert [T.wave_tiles(1056, w) for w in range(4)] == [(0, 8), (8, 16), (16, 24), (24, 33)]
    assert [T.wave_tiles(1025, w) for w in range(4)] == [(0, 8), (8, 16), (16, 24), (24, 33)]   # F6: Lkp / 32 = 33 too


# ---------------------------------------------------------------------------------------------------------------
# Masks
# ---------------------------------------------------------------------------------------------------------------
SHAPES = sorted({(c[1], c[4]) for c in T.CASES})


@pytest.mark.parametrize("batch,Lk", SHAPES)
def test_mask_properties(batch, Lk):
    nt = T.cdiv(Lk, 32)
    every = dict(T.MASKS, M7=T.mask_m7, head=T.mask_head)
    for name, build in every.items():
        m = build(batch, Lk)
        if m is None:
            continue
        assert m.dtype == torch.uint8 and m.shape == (batch, Lk)
        kept = (m == 0).sum(1)
        if name == "M7":
            assert kept[1] == 0 and bool((kept[torch.arange(batch) != 1] > 0).all())
        else:
            assert bool((kept > 0).all()), name
    assert bool(T.mask_m1(batch, Lk)[:, :32].all()) and not bool(T.mask_m1(batch, Lk)[:, 32:].any())     # M1: exactly the first tile
    t = T.interior_tile(Lk)
    assert bool(T.mask_m2(batch, Lk)[:, t * 32:(t + 1) * 32].all()) and (0 < t < nt - 1 or nt < 3)
    m3 = T.mask_m3(batch, Lk)
    for b in range(batch):
        s = T.m3_start(Lk, b)
        assert s % 32 != 0 and 0 < s < Lk and bool(m3[b, s:].all()) and not bool(m3[b, :s].any())
    m5 = T.mask_m5(batch, Lk)
    keys = T.m5_keys(batch, Lk)
    assert bool(((m5 == 0).sum(1) == 1).all()) and all(m5[b, j] == 0 for b, j in enumerate(keys))         # M5: exactly one key kept
    assert keys[0] == Lk - 1 and keys[1] // 32 == nt - 1 and (batch < 3 or len(set(keys[:4])) >= 3)
    m6 = T.mask_m6(batch, Lk)
    assert len({tuple(r.tolist()) for r in m6}) == batch                                                   # M6: differs in every entry


@pytest.mark.parametrize("Lk", [1056, 1025, 1024])
def test_m4_empties_exactly_the_named_waves(Lk):
    for name, build in T.MASKS_M4.items():
        waves = [int(c) for c in name.split()[-1].split(",")]
        m = build(2, Lk)
        assert bool((m == 0).any(1).all())                       # at least one key survives
        for t in range(T.cdiv(Lk, 32)):
            owner = next(w for w in range(4) if T.wave_tiles(Lk, w)[0] <= t < T.wave_tiles(Lk, w)[1])
            tile = m[:, t * 32:(t + 1) * 32]
            assert bool(tile.all()) if owner in waves else not bool(tile.any()), (name, t)
    assert set(T.MASKS_M4) == {"M4 wave 0", "M4 wave 3", "M4 waves 0,1,3"}   # wave 0, wave 3, every wave except wave 2


# ---------------------------------------------------------------------------------------------------------------
# Score designs
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [F1, F5], ids=["F1", "F5"])
def test_score_designs(c):
    _, batch, nh, Lq, Lk, _, _ = c
    for d in T.DESIGNS:
        mname, build = T.design_mask(d, Lk)
        mask = build(batch, Lk)
        q, k, v = T.operands(d, batch, nh, Lq, Lk, mask=mask)
        s = (T._heads(q.double(), nh) * T.SCALE) @ T._heads(k.double(), nh).transpose(-1, -2)     # [batch, nh, Lq, Lk]
        if d in ("S1", "S2"):
            top = s.amax(-1)
            assert 59.0 < top.min().item() and top.max().item() < 76.0
            tile_max = torch.stack([s[..., t * 32:(t + 1) * 32].amax(-1) for t in range(T.cdiv(Lk, 32))], -1)
            steps = tile_max[..., 1:] - tile_max[..., :-1]
            assert bool((steps > 0).all()) if d == "S1" else bool((steps < 0).all())      # the maximum moves in every tile, one way
        elif d == "S3":
            sm = s.masked_fill(mask.bool()[:, None, None, :], float("-inf"))
            two = sm.topk(2, -1).values
            assert (two[..., 0] - two[..., 1]).min().item() > 104.0                        # one-hot in fp32
            assert (s.amax(-1) - sm.amax(-1)).min().item() > 104.0                        # and the masked leader would take it all
        else:
            assert float(s.abs().max()) == 0.0
        # the masked keys would carry visible probability: unmasked, they hold more than 10 % of some row
        p = torch.softmax(s, -1)
        assert (p * mask.bool()[:, None, None, :]).sum(-1).max().item() > 0.1, (d, mname)


# ---------------------------------------------------------------------------------------------------------------
# The reference
# ---------------------------------------------------------------------------------------------------------------
def test_reference_equals_fp64_masked_softmax():
    batch, nh, Lq, Lk = 2, 2, 19, 70
    q, k, v = T.operands("N", batch, nh, Lq, Lk, seed=3)
    mask = T.mask_m2(batch, Lk)
    ref, B, S = T.masked_ref_and_bound(q, k, v, mask, nh)
    s = (T._heads(q.double(), nh) * T.SCALE) @ T._heads(k.double(), nh).transpose(-1, -2)
    s = s.masked_fill(mask.bool()[:, None, None, :], float("-inf"))
    want = (torch.softmax(s, -1) @ T._heads(v.double(), nh)).permute(0, 2, 1, 3).reshape(batch, Lq, nh * 32)
    assert (ref - want).abs().max().item() <= 1e-12
    assert bool((B > 0).all()) and bool(torch.isfinite(B).all())
    # whatever the ignored keys' K rows hold
    k2 = k.clone()
    k2[mask.bool()] = float("nan")
    ref2, B2, _ = T.masked_ref_and_bound(q, k2, v, mask, nh)
    assert torch.equal(ref, ref2) and torch.equal(B, B2)
    # the single-pass bound is the wider one, an entry with no kept key is exact zeros
    _, B16, _ = T.masked_ref_and_bound(q, k, v, mask, nh, product=A.bound_f16)
    assert bool((B16 > B).all())
    r7, B7, _ = T.masked_ref_and_bound(q, k, v, T.mask_m7(batch, Lk), nh)
    assert float(r7[1].abs().max()) == 0.0 and float(B7[1].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------
# The reference alone is inside; planted defects are outside
# ---------------------------------------------------------------------------------------------------------------
def _families(c):
    """(label, design, mask name, mask) of every mask at N(0, 1) and every score design under its mask."""
    _, batch, nh, Lq, Lk, _, _ = c
    masks = dict(T.MASKS, M7=T.mask_m7)
    if Lk >= 1024:
        masks.update(T.MASKS_M4)
    for name, build in masks.items():
        yield f"N {name}", "N", name, build(batch, Lk)
    for d in T.DESIGNS:
        name, build = T.design_mask(d, Lk)
        yield f"{d} {name}", d, name, build(batch, Lk)


_REF = {}


def _ref(c, label, design, mask):
    """Computed once per (shape, family) and shared; never modified."""
    key = (c[0], label)
    if key not in _REF:
        _, batch, nh, Lq, Lk, _, _ = c
        q, k, v = T.operands(design, batch, nh, Lq, Lk, mask=mask)
        _REF[key] = (q, k, v) + T.masked_ref_and_bound(q, k, v, mask, nh)
    return _REF[key]


@pytest.mark.parametrize("c", [F1, F5], ids=["F1", "F5"])
def test_plain_fp32_torch_is_inside_the_bound(c):
    nh = c[2]
    for label, design, mname, mask in _families(c):
        q, k, v, ref, B, S = _ref(c, label, design, mask)
        r = _worst(T.torch_f32(q, k, v, mask, nh), ref, B)
        assert r <= 1.0, (c[0], label, r)
        if c is F5:     # and so is the KSPLIT structure (sentinel partials of fully masked waves included)
            r = _worst(T.ksplit_f32(q, k, v, mask, nh), ref, B)
            assert r <= 1.0, (c[0], label, "ksplit", r)


LEAK_SEEN_BY = ("N M1", "N M2", "N M3", "N M5", "N M6", "N M7", "N M4 wave 0", "N M4 wave 3", "N M4 waves 0,1,3",
                "S1 M3", "S2 head", "S3 M3", "S4 M3")
SHIFT_SEEN_BY = ("N M2", "N M3", "N M5", "N M6", "N M7", "S1 M3", "S3 M3", "S4 M3")    # masks that differ between batch entries
DROP_SEEN_BY = {"first": ("N M0", "N M1", "N M2", "N M3", "N M6", "S2 head", "S4 M3"),
                "last": ("N M0", "N M1", "N M2", "N M3", "N M6", "S1 M3", "S4 M3")}
MERGE_SEEN_BY = {0: ("N M0", "N M2", "N M3", "N M6", "N M4 wave 3", "S1 M3"), 1: ("N M4 wave 0",),       # under "M4 waves 0,1,3" wave 2 holds every maximum: blind
                 3: ("N M0", "N M2", "N M6", "S2 head")}


@pytest.mark.parametrize("c", [F1, F5], ids=["F1", "F5"])
def test_planted_defects_are_outside_the_bound(c):
    nh, Lk = c[2], c[4]
    fam = {label: (design, mask) for label, design, mname, mask in _families(c)}
    seen = []

    def outside(label, what, fn):
        design, mask = fam[label]
        q, k, v, ref, B, S = _ref(c, label, design, mask)
        r = _worst(fn(q, k, v, mask, nh), ref, B)
        assert r > 1.0, (c[0], label, what, r)
        seen.append(r)

    for label in LEAK_SEEN_BY:
        if label in fam:
            outside(label, "one masked key let in", T.defect_leak)
    for label in SHIFT_SEEN_BY:
        outside(label, "mask of entry b applied to b + 1", T.defect_batch_shift)
    for which, labels in DROP_SEEN_BY.items():
        for label in labels:
            outside(label, f"{which} kept key tile dropped", T.defect_drop_tile(which))
    if c is F5:
        for w, labels in MERGE_SEEN_BY.items():
            for label in labels:
                outside(label, f"wave {w} merged with weight 1", T.defect_merge_weight_one(w))
    assert min(seen) > 1.0
