"""CPU: the references, bounds and inputs of test_text_kernels_gpu.py (tests/_text.py) discriminate, with no kernel involved.  The
restated rules are HuggingFace's / the oracle's; the emulation of each kernel's order of operations equals the reference in fp64 and is
inside the bound B in fp32 on every input set; every defect of _text.MUTANTS is at least 4 x outside B on some input set.  The 4 x is a
condition on the CHOICE OF INPUTS; the bounds have no margin.  The table of (defect, input set that catches it, worst err / B, the
same on the kind of input the earlier tests ran, and the absolute error there) is written to profiles/r18_text_kernel_mutants.txt."""
import os

import numpy as np
import pytest
import torch

import _text as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "r18_text_kernel_mutants.txt")
GOLDEN = os.path.join(ROOT, "tests", "golden")
MARGIN = 4.0
F64 = torch.float64
# per kind, the input set that is what the earlier tests ran: near-uniform softmax rows / one un-padded caption with pad id 1 / one
# right-padded group; and the absolute tolerance those tests held the path to
BASELINE = {"mha": (K.NEAR_UNIFORM["mha"], 2e-4), "embed": ("embed single: nopad, C 768 nseq 1 L 7 pad 1", 2e-4),
            "lens": ("lens: Lmax 128 D 256 lens (128, 1, 64)", 2e-6)}
assert all(b[0] in K.SETS for b in BASELINE.values())


def by_kind(kind):
    return [n for n in K.SETS if n.split(":")[0].split(" ")[0] == kind]


# ---------------------------------------------------------------------------------------------------------------------
# the restated rules are the reference's
# ---------------------------------------------------------------------------------------------------------------------
def test_position_ids_are_huggingfaces():
    from transformers.models.roberta import modeling_roberta as R
    fn = getattr(R, "create_position_ids_from_input_ids", None) or R.RobertaEmbeddings.create_position_ids_from_input_ids
    for pad in (1, 5):
        for pattern in ("right", "inside", "allpad", "nopad"):
            ids = K.embed_ids(3, 70, pad, pattern, seed=pad)
            assert torch.equal(K.position_ids(ids, pad), fn(ids, pad)), (pad, pattern)


@pytest.mark.parametrize("pad,pattern", [(1, "right"), (5, "inside")])
def test_embedding_reference_is_huggingfaces_module(pad, pattern):
    import transformers
    c = K.embed_case(260, 3, 11, pad=pad, pattern=pattern, seed=50)
    ref, B, _ = K.ref_and_bound(c)
    cfg = transformers.RobertaConfig(vocab_size=64, hidden_size=260, max_position_embeddings=c["pos"].shape[0], type_vocab_size=1,
                                     pad_token_id=pad, layer_norm_eps=c["eps"], hidden_dropout_prob=0.0)
    emb = transformers.models.roberta.modeling_roberta.RobertaEmbeddings(cfg).double().eval()
    with torch.no_grad():
        emb.word_embeddings.weight.copy_(c["word"])
        emb.position_embeddings.weight.copy_(c["pos"])
        emb.token_type_embeddings.weight.copy_(c["type0"][None])
        emb.LayerNorm.weight.copy_(c["gamma"])
        emb.LayerNorm.bias.copy_(c["beta"])
        want = emb(input_ids=c["ids"]).reshape(-1, 260)
    assert torch.allclose(ref, want, rtol=1e-12, atol=1e-12), (ref - want).abs().max()
    assert bool(torch.isfinite(B).all() and (B > 0).all())


@pytest.mark.parametrize("scale", [0.125, 0.1])
def test_attention_reference_is_plain_softmax_attention(scale):
    c = K.mha_case("wide", 2, 33, nseq=2, splits=3, bias=True, scale=scale, lens=(20, 40), seed=51)
    ref, B, _ = K.ref_and_bound(c)
    E, L = 128, 33
    x = c["planes"].double().sum(0) + c["bias"].double()
    for z, n in enumerate((20, 33)):
        r = x[z * L:(z + 1) * L]
        q, k, v = (r[:, i * E:(i + 1) * E].view(L, 2, 64).transpose(0, 1) for i in range(3))
        want = torch.nn.functional.scaled_dot_product_attention(q, k[:, :n], v[:, :n], scale=scale).transpose(0, 1).reshape(L, E)
        assert torch.allclose(ref[z * L:(z + 1) * L], want, rtol=1e-12, atol=1e-13), (z, (ref[z * L:(z + 1) * L] - want).abs().max())
    assert bool(torch.isfinite(B).all() and (B > 0).all())


def test_caption_rule_is_the_suites_and_the_reference_fixture():
    from test_ragged_captions_cpu import text_pos_ragged
    fx = np.load(os.path.join(GOLDEN, "text_pos_ragged.npz"))
    lens, Lmax = fx["lens"].tolist(), fx["mask"].shape[1]
    c = K.lens_case(Lmax, 256, lens, seed=52)
    got_lens, kmask, pos, B, _ = K.lens_ref_and_bound(c)
    assert got_lens == lens and np.array_equal(kmask.numpy(), fx["mask"])
    assert float((pos - torch.from_numpy(fx["pos"]).double().reshape(pos.shape)).abs().max()) < 2e-6
    assert float((pos - text_pos_ragged(lens, Lmax).double().reshape(pos.shape)).abs().max()) < 2e-6
    assert float(B.max()) <= 2e-6
    # no pad -> Lmax; a leading pad -> 1; the first pad rules
    assert K.lens_rule(torch.tensor([[0, 5, 6, 2], [1, 1, 1, 1], [0, 2, 1, 1], [0, 1, 7, 1]]), 1) == [4, 1, 2, 1]


# ---------------------------------------------------------------------------------------------------------------------
# the emulation: the reference in fp64, inside the bound in fp32
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K.SETS))
def test_emulation_is_the_reference_in_fp64_and_inside_the_bound_in_fp32(name):
    c, want = K.case(name)
    r64 = K.ratio(c, K.emulate(c, None, F64), want)
    r32 = K.ratio(c, K.emulate(c, None, torch.float32), want)
    print(f"{name}: fp64 emulation err / B = {r64:.2e}, fp32 emulation err / B = {r32:.3f}")
    assert r64 <= 1e-6, (name, r64)
    assert r32 <= 1.0, (name, r32)


def test_tanh_bound_is_measured_on_the_grid_and_small():
    b = K.tanh_ulp_bound()
    print("tanh bound:", b, "ulp")
    assert 0.5 < b <= 8.0, b     # a libm worse than 4 ulp is no yardstick
    x = K.tanh_values(2304)
    assert float(x[12:].min()) == -10.0 and float(x[12:].max()) == 10.0 and torch.equal(x[:12], torch.tensor(K.TANH_SPECIAL))


# ---------------------------------------------------------------------------------------------------------------------
# every defect is far outside the bound somewhere
# ---------------------------------------------------------------------------------------------------------------------
def _abs_err(c, got, want):
    if c["kind"] == "lens":
        if K.worst_lens(got, want)[0] == float("inf"):
            return float("inf")
        return float((got[2].double() - want[2]).abs().max())
    n = want[0].shape[0]
    return float((got[:n].double() - want[0]).abs().nan_to_num(nan=float("inf")).max())


def test_every_defect_is_far_outside_the_bound_somewhere():
    rows = []
    for kind in ("mha", "embed", "lens"):
        base, tol = BASELINE[kind]
        for mut in K.MUTANTS[kind]:
            best = (0.0, None)
            for name in by_kind(kind):
                c, want = K.case(name)
                r = K.ratio(c, K.emulate(c, mut), want)
                if r > best[0]:
                    best = (r, name)
            c, want = K.case(base)
            got = K.emulate(c, mut)
            rows.append((kind, mut, best[1], best[0], K.ratio(c, got, want), _abs_err(c, got, want), tol))
    with open(PROFILE, "w") as f:
        f.write("# tests/test_text_kernels_cpu.py: every defect of tests/_text.py MUTANTS on every input set of its kernel (fp64 emulation, no\n"
                "# kernel); the set on which it is furthest outside the derived bound B and how far (asserted >= 4 for every defect); then\n"
                "# the same defect on the kind of input the earlier tests ran -- mha: near-uniform rows, " + BASELINE["mha"][0] + ";\n"
                "# embed: " + BASELINE["embed"][0] + "; lens: " + BASELINE["lens"][0] + " -- as err / B and as the absolute\n"
                "# error beside the absolute tolerance of those tests (seen: the old tolerance would have caught it on that input).\n"
                "# kernel | defect | input set | worst err / B | err / B on the earlier input | abs err there | old tolerance | seen\n")
        for kind, mut, name, r, rb, ab, tol in rows:
            f.write(f"{kind} | {mut} | {name} | {r:.3g} | {rb:.3g} | {ab:.3g} | {tol:g} | {'yes' if ab > tol else 'no'}\n")
    missed = [row[:4] for row in rows if not row[3] >= MARGIN]
    assert not missed, f"defects no input set sees at {MARGIN:g} x B: {missed}"
