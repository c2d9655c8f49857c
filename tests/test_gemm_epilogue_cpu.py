"""CPU: the designs and the model behind tests/test_gemm_epilogue_gpu.py, on that module's own case table.

* the exact-product design IS exact: for every (shape, scale) the GPU module runs, _arith.emulate_split, its single_pass form and a
  plain fp32 matmul equal the fp64 product bit for bit, a + a2 and every partial plane are exact and so is their fp32 sum;
* the GELU arguments stay inside +-6 and every LayerNorm row has sigma > 1e-3;
* each planted defect of _epilogue.DEFECTS breaks bit equality, or lies at least 4 x outside the bound, on at least one case of the
  table; the defects and the cases that catch them go to profiles/r29_gemm_epilogue_mutants.txt."""
import os

import pytest
import torch

import _arith as A
import _epilogue as E
import test_gemm_epilogue_gpu as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "r29_gemm_epilogue_mutants.txt")


def _distinct_products(design):
    seen, out = set(), []
    for c in G.CASES:
        key = (c.design, c.M, c.N, c.K, c.batch, c.a2, c.a2_shared, c.conv, c.handmade, c.splits)
        if c.design == design and key not in seen:
            seen.add(key)
            out.append(c)
    return out


def test_case_table_covers_what_the_issue_lists():
    inst = {(c.mode, c.tile, c.epi, c.a2) for c in G.cases("instance")}
    assert len(inst) == 2 * (len(G.SPLIT_INSTANCES) + len(G.F32_INSTANCES))
    for mode, tile, epi in G.SPLIT_INSTANCES + G.F32_INSTANCES:
        for a2 in (False, True):
            mine = G.cases("instance", mode=mode, tile=tile, epi=epi, a2=a2)
            BM, BN = E.TILE_BM[tile], E.TILE_BN[tile]
            assert {c.N for c in mine} >= {1, 3, 4, 28, 29, 31, 32, 33, 61, BN + 28, BN + 29, BN + 33}
            assert {c.K for c in mine} == {32, 64, 96, 160} and {c.M for c in mine} == {1, BM + 35}
            assert {c.combo for c in mine} == set(G.EIGHT)
            for N in (29, 31, 33, 61):   # scalar everywhere, and vector + scalar lanes in one wave
                assert {E.layout(c).ldc for c in mine if c.N == N and c.M > 1} == {N, G.pitch4(N)}
    for tile in (6464, 256128):
        assert {c.combo for c in G.cases("combo", tile=tile, inplace=False)} == set(E.COMBOS)
        assert {c.combo for c in G.cases("combo", tile=tile, inplace=True)} == {(0, 1), (0, 2), (1, 1), (3, 1)}
    assert {c.combo for c in G.cases("splitk")} == set(E.COMBOS) == {c.combo for c in G.cases("reduce", ln=False)}
    assert {(c.M, c.N, c.splits) for c in G.cases("ln")} == {(M, N, s) for M in (256, 257) for N in (4, 260, 1024) for s in (1, 4, 5, 9)}
    assert all(c.batch * ((c.M + 63) // 64) * ((c.N + 63) // 64) >= 512 for c in G.cases("ring"))
    assert len(set(G.CASES)) == len(G.CASES)


def test_exact_design_is_exact():
    n = 0
    for c in _distinct_products("exact"):
        o = E.operands(c)
        x32 = o.x64.float()
        assert torch.equal(x32.double(), o.x64), c.label
        if c.handmade:
            acc = o.planes[0].clone()
            for s in range(1, c.splits):
                acc += o.planes[s]
            assert torch.equal(acc.double()[None], o.x64), c.label
            continue
        asum = o.asum.float()
        assert torch.equal(asum.double(), o.asum) and torch.equal(asum.half().double(), o.asum), c.label   # lo halves are zero
        assert torch.equal(o.w.half().float(), o.w), c.label
        if o.a2 is not None:
            assert torch.equal((o.a + o.a2).double(), o.asum), c.label       # the prologue's fp32 sum
        for b in range(asum.shape[0]):
            for got in (A.emulate_split(asum[b], o.w), A.emulate_split(asum[b], o.w, mutant="single_pass"), asum[b] @ o.w.T):
                assert torch.equal(got, x32[b]), c.label
        if c.splits > 1:
            acc = E.plane(c, o, 0).float()
            for s in range(c.splits):
                p = E.plane(c, o, s)
                assert torch.equal(p.float().double(), p), c.label
                if s:
                    acc += p.float()
            assert torch.equal(acc.double(), o.x64), c.label
        n += 1
    assert n > 100


def test_gelu_arguments_and_layernorm_rows():
    for c in G.CASES:
        o = E.operands(c)
        if c.act == E.ACT_GELU:
            z = o.x64 + o.bias.double()[:, None, :]
            assert float(z.abs().max()) < 6.0, c.label
        if c.ln:
            z, _ = E.ln_input_bound(c, o)
            assert float(A.layernorm_sigma(z).min()) > 1e-3, c.label


def test_range_probe_is_what_it_says():
    c, o = E.range_probe()
    ref, B = E.reference(c, o)
    assert B is None and c.form == "lds" and c.M % 32 != 0 and c.res_mode == E.RES_MUL
    assert float(ref.abs().max()) < 3000.0 < E.RANGE_LIMIT
    assert float((o.bias[0] * o.res[0, c.M - 1]).abs().min()) >= E.RANGE_LIMIT
    assert float(o.a.abs().max()) < E.RANGE_LIMIT and float(o.w.abs().max()) < E.RANGE_LIMIT
    x32 = o.x64.float()
    assert torch.equal(x32.double(), o.x64) and torch.equal(A.emulate_split(o.a[0], o.w), x32[0])
    assert torch.equal(A.emulate_split(o.a[0], o.w, mutant="single_pass"), x32[0])


# cheap filters: the cases on which a defect can show at all (the scan stops at the third case that catches it)
APPLIES = {
    # only where some columns of the tile go through float4 stores and others through the scalar tail
    "bias_dropped_on_tail": lambda c: c.path in ("tile", "fix") and 0 < int(E.scalar_cols(c, 0).sum()) < c.N,
    "bias_col_minus_4_hi_halfwave": lambda c: c.path in ("tile", "fix") and c.form == "direct" and c.N > 4,
    "res_row_clamped_early": lambda c: c.res_mode and c.M > 1 and not c.ln,
    "res_pitch_ldc": lambda c: c.res_mode and E.layout(c).ldc != E.layout(c).ldres and c.M > 1 and not c.ln,
    "act_after_res": lambda c: c.res_mode and c.act in (1, 2),
    "relu3_before_res": lambda c: c.res_mode and c.act == 3,
    "fix_res_batch0": lambda c: c.path == "fix" and c.batch > 1 and not c.res_shared,
    "sbias_ignored": lambda c: c.bias_pb,
    "fix_mul_as_add": lambda c: c.path == "fix" and c.res_mode == E.RES_MUL,
    "ln_plane_skipped": lambda c: c.ln and c.M > 256 and c.splits % 4 == 1 and c.splits > 1 and c.N <= 260,
    "gelu_tanh": lambda c: c.act == E.ACT_GELU and c.design == "exact",
}
CAUGHT = {}


@pytest.mark.parametrize("defect", sorted(E.DEFECTS))
def test_planted_defect_is_caught(defect):
    assert set(APPLIES) == set(E.DEFECTS)
    caught = []
    for c in G.CASES:
        if APPLIES[defect](c) and E.defect_shows(c, E.operands(c), defect):
            caught.append(c)
            if len(caught) == 3:
                break
    CAUGHT[defect] = caught
    assert caught, f"no case of the GPU module shows: {E.DEFECTS[defect]}"


def test_defects_do_not_show_where_they_cannot():
    """The model without a defect is the reference, and a defect of the LDS form's / the folded path's kind leaves the other cases alone."""
    c = G.cases("combo", tile=256128, epi=1, act=1, res_mode=1, inplace=False)[0]
    o = E.operands(c)
    for defect in ("bias_col_minus_4_hi_halfwave", "fix_res_batch0", "fix_mul_as_add", "sbias_ignored", "ln_plane_skipped"):
        assert not E.defect_shows(c, o, defect), defect


def test_zz_write_mutant_table():
    assert set(CAUGHT) == set(E.DEFECTS), "run the whole module"
    with open(PROFILE, "w") as f:
        f.write("# tests/test_gemm_epilogue_cpu.py: every planted defect of tests/_epilogue.py's matrix-level model and the first cases of\n"
                "# tests/test_gemm_epilogue_gpu.py's table (up to three) on which it breaks bit equality or lies >= 4 x outside the bound.\n"
                "# defect | what it is | instance and tile | shape | combination | alignment variant\n")
        for defect in sorted(E.DEFECTS):
            for c in CAUGHT[defect]:
                f.write(f"{defect} | {E.DEFECTS[defect]} | {c.label}\n")
