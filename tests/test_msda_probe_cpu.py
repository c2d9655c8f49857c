"""CPU: the reference, bound and inputs of test_msda_probe_gpu.py (tests/_msda.py) discriminate, with no kernel involved.  ref64 is the
oracle's rule; a correct fp32 evaluation of it is inside the bound B on every input set; every defect of _msda.MUTANTS is at least 4 x
outside B on some input set.  The 4 x is a condition on the CHOICE OF INPUTS; the bound itself has no margin.  The table of (defect,
input set that catches it, worst err / B) is written to profiles/r16_msda_probe_mutants.txt."""
import os

import pytest
import torch

import _msda as K
from _util import load_npz
from oracle import tce_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "r16_msda_probe_mutants.txt")
MARGIN = 4.0

# name -> builder; every kind of input the GPU module runs, at M = 2 (the head count changes the launch geometry, not the rule)
SETS = {
    "plain lattice, odd shapes": lambda: K.lattice_plain(K.SHAPES_ODD, 2, 2, 32, 4, 1),
    "plain lattice, 2^k shapes": lambda: K.lattice_plain(K.SHAPES_POW2, 1, 2, 32, 4, 2),
    "plain one-hot": lambda: K.dense_plain(K.SHAPES_ODD, 2, 37, 2, 32, 4, 3, onehot=True, code=True),
    "plain logits x 100": lambda: K.dense_plain(K.SHAPES_ODD, 2, 37, 2, 32, 4, 4, logit_scale=100.0),
    "lattice via off, ref_dim 2, odd": lambda: K.lattice_fused(K.SHAPES_ODD, None, 2, 2, 4, 4, "off", 2, 0, 5),
    "lattice via off, ref_dim 4, 2^k": lambda: K.lattice_fused(K.SHAPES_POW2, None, 1, 2, 4, 4, "off", 4, 0, 6),
    "lattice via ref, ref_dim 2, per frame, 2^k": lambda: K.lattice_fused(K.SHAPES_POW2, None, 2, 2, 4, 4, "ref", 2, 1, 7),
    "lattice via ref, ref_dim 4, odd": lambda: K.lattice_fused(K.SHAPES_ODD, None, 1, 2, 4, 4, "ref", 4, 0, 8),
    "lattice via off, logits x 30, odd": lambda: K.lattice_fused(K.SHAPES_ODD, None, 1, 2, 4, 4, "off", 2, 0, 9, logit_scale=30.0),
    "padded lattice via off, ref_dim 2, odd": lambda: K.lattice_fused(K.SHAPES_ODD, K.VALID_ODD, 1, 2, 4, 4, "off", 2, 0, 10),
    "padded lattice via ref, ref_dim 2, 2^k": lambda: K.lattice_fused(K.SHAPES_POW2, K.VALID_POW2, 1, 2, 4, 4, "ref", 2, 0, 11),
    "padded lattice via off, ref_dim 4, 2^k": lambda: K.lattice_fused(K.SHAPES_POW2, K.VALID_POW2, 1, 2, 4, 4, "off", 4, 0, 12),
    "one-hot, ref_dim 2, per frame": lambda: K.dense_fused(K.SHAPES_ODD, None, 3, 37, 2, 4, 4, 2, 1, 13, onehot=True, code=True),
    "one-hot, ref_dim 4, padded": lambda: K.dense_fused(K.SHAPES_ODD, K.VALID_ODD, 2, 37, 2, 4, 4, 4, 0, 14, onehot=True, code=True),
    "one-hot, (L, P) = (4, 3)": lambda: K.dense_fused(K.SHAPES_ODD, None, 2, 37, 3, 4, 3, 2, 0, 15, onehot=True, code=True),
    "logits x 1": lambda: K.dense_fused(K.SHAPES_ODD, None, 2, 37, 2, 4, 4, 2, 0, 16, logit_scale=1.0),
    "logits x 30": lambda: K.dense_fused(K.SHAPES_ODD, None, 2, 37, 2, 4, 4, 2, 0, 16, logit_scale=30.0),
    "logits x 100": lambda: K.dense_fused(K.SHAPES_ODD, None, 2, 37, 2, 4, 4, 4, 1, 16, logit_scale=100.0),
    "raw padded lattice via off": lambda: K.lattice_fused(K.SHAPES_ODD, K.VALID_ODD, 1, 8, 4, 4, "off", 2, 0, 17, raw=True),
    "raw logits x 30, ref_dim 4": lambda: K.dense_fused(K.SHAPES_POW2, None, 2, 5, 8, 4, 4, 4, 1, 18, logit_scale=30.0, raw=True),
}
_CACHE = {}


def case(name):
    """(case, ref64, B), built once and left unchanged."""
    if name not in _CACHE:
        c = SETS[name]()
        _CACHE[name] = (c,) + K.ref_and_bound(c)
    return _CACHE[name]


def test_restated_rule_is_the_oracles_rule():
    c = K.dense_plain(K.SHAPES_ODD, 2, 19, 3, 7, 3, 21)
    v, loc, w = c["value"].double(), c["loc"].double(), c["weights"].double()
    assert torch.equal(K.core(v, c["shapes"], loc, w), O.msda_core(v, c["shapes"], loc, w))
    for name in SETS:
        c, ref, _ = case(name)
        assert torch.equal(K.emulate(c), ref), name


@pytest.mark.parametrize("rd", [2, 4])
def test_ref64_is_the_oracle_module_on_the_common_domain(rd):
    """O.msda_module (un-padded, fp64) with identity projections fed the case's own fp32 numbers: the formulas around the gather."""
    N, Lq, M, L, P = 2, 11, 8, 2, 2
    c = K.dense_fused(K.SHAPES_ODD, None, N, Lq, M, L, P, rd, 1, 30 + rd, logit_scale=30.0, raw=True)
    ref, _ = K.ref_and_bound(c)
    LP = L * P
    eye = torch.eye(256, dtype=torch.float64)
    sd = {"a.value_proj.weight": c["wv"].double(), "a.value_proj.bias": c["bv"].double(),
          "a.sampling_offsets.weight": eye[:M * LP * 2], "a.sampling_offsets.bias": torch.zeros(M * LP * 2, dtype=torch.float64),
          "a.attention_weights.weight": eye[M * LP * 2:M * LP * 3], "a.attention_weights.bias": torch.zeros(M * LP, dtype=torch.float64),
          "a.output_proj.weight": eye, "a.output_proj.bias": torch.zeros(256, dtype=torch.float64)}
    query = torch.zeros(N, Lq, 256, dtype=torch.float64)
    query[..., :M * LP * 3] = c["proj"].double().view(N, Lq, -1)
    refpts = c["ref"].double().view(N, Lq, 1, rd).expand(N, Lq, L, rd)     # valid ratios are 1: the module's per-level points
    out, _, _ = O.msda_module(sd, "a.", query, refpts, c["src"].double().view(N, -1, 256), c["shapes"], None, M, L, P)
    assert torch.allclose(out, ref, rtol=1e-12, atol=1e-12), (out - ref).abs().max()


def test_ref64_reproduces_the_reference_fixture():
    fx = load_npz("msda_cases.npz")
    for i in range(int(fx["n_cases"])):
        shapes = [tuple(int(v) for v in r) for r in fx[f"c{i}_shapes"]]
        c = dict(kind="plain", shapes=shapes, valid=None, value=torch.from_numpy(fx[f"c{i}_value"]), loc=torch.from_numpy(fx[f"c{i}_loc"]),
                 weights=torch.from_numpy(fx[f"c{i}_w"]))
        ref, B = K.ref_and_bound(c)
        want = torch.from_numpy(fx[f"c{i}_out"])
        assert torch.allclose(ref.float(), want, rtol=1e-4, atol=1e-6), (i, (ref.float() - want).abs().max())
        assert bool(torch.isfinite(B).all())


def test_formula_valued_reference_is_the_tensor_valued_one():
    """ref_and_bound_fn (value given as a function of the flat index, for the multi-gigabyte case of the GPU module) against
    ref_and_bound on the materialised tensor; its position term takes one max|v| for the whole tensor, so its bound is no smaller."""
    fn = lambda i: ((i * 48271) % 241).float()
    c = K.dense_fused(K.SHAPES_ODD, None, 3, 21, 2, 4, 4, 2, 1, 40, onehot=True, value=False, edges=True)
    ref_fn, B_fn = K.ref_and_bound_fn(c, fn, 240.0)
    c["value"] = fn(torch.arange(3 * K.n_rows(K.SHAPES_ODD) * 2 * 32)).view(3, -1, 2, 32)
    ref, B = K.ref_and_bound(c)
    assert torch.allclose(ref_fn, ref, rtol=1e-13, atol=1e-13)
    assert bool((B_fn >= B * (1 - 1e-12)).all())
    r, i, _ = K.worst(K.oracle_fp32(c), ref_fn, B_fn)
    assert r <= 1.0, (r, K.describe(c, i))


@pytest.mark.parametrize("name", list(SETS))
def test_correct_fp32_evaluation_is_inside_the_bound(name):
    c, ref, B = case(name)
    r, i, rel = K.worst(K.oracle_fp32(c), ref, B)
    print(f"{name}: fp32 oracle err / B = {r:.3f}, err / max|ref| = {rel:.2e}")
    assert r <= 1.0, f"{name}: fp32 oracle {r:.3g} x B at {K.describe(c, i)}"


def test_issue_figures_fp32_against_fp64_and_border_replicate():
    """The discrimination in plain figures, bound aside: first shape set, M = 2, logits 30 * randn: fp32 and fp64 differ by ~1e-6 of
    max|ref|, the border-replicate defect by O(max|ref|)."""
    c, ref, B = case("lattice via off, logits x 30, odd")
    _, _, rel = K.worst(K.oracle_fp32(c), ref, B)
    _, _, rel_mut = K.worst(K.emulate(c, "border_replicate"), ref, B)
    assert rel < 1e-5 and rel_mut > 0.1, (rel, rel_mut)


def test_every_defect_is_far_outside_the_bound_somewhere():
    rows = []
    for mut in K.MUTANTS:
        best = (0.0, None)
        for name in SETS:
            c, ref, B = case(name)
            r, _, _ = K.worst(K.emulate(c, mut), ref, B)
            if r > best[0]:
                best = (r, name)
        rows.append((mut, best[1], best[0]))
    with open(PROFILE, "w") as f:
        f.write("# tests/test_msda_probe_cpu.py: every defect of tests/_msda.py MUTANTS on every input set of the module (fp64 emulation, no kernel);\n"
                "# the set on which it is furthest outside the derived bound B, and how far.  Asserted >= 4 for every defect.\n"
                "# defect | input set | worst err / B\n")
        for mut, name, r in rows:
            f.write(f"{mut} | {name} | {r:.3g}\n")
    missed = [row for row in rows if not row[2] >= MARGIN]
    assert not missed, f"defects no input set sees at {MARGIN:g} x B: {missed}"
