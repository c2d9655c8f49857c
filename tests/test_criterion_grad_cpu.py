"""CPU: the closed form of the criterion's gradients (tests/_criterion_grad.py) against fp64 autograd of the torch form and against
the reference fixture; argument rejection of the two backward entry points (before any launch, so stand-in pointers are safe); the
`grad` attribute and the checks that precede device work."""
import argparse

import numpy as np
import pytest
import torch

import _criterion as R
import _criterion_grad as G
from _util import load_npz


@pytest.fixture(scope="module")
def fixture():
    return load_npz("criterion_grad_cases.npz")


@pytest.fixture(scope="module")
def train_lib():
    from tce_rvos_amd import _train_lib
    return _train_lib.lib()  # builds the library when its file is absent


@pytest.fixture(scope="module")
def closed():
    cache = {}

    def get(name):
        if name not in cache:
            case = {c[0]: c for c in R.CASES}[name]
            outputs, targets = R.make_case(case)
            cache[name] = (outputs, targets) + G.grads(outputs, targets, vis=case[8])
        return cache[name]
    return get


def _leaves64(o):
    return {k: v.double().requires_grad_(True) for k, v in o.items() if k != "aux_outputs"}


@pytest.mark.parametrize("name", [c[0] for c in R.CASES])
def test_closed_form_is_the_gradient_of_the_torch_form(closed, name):
    """fp64 autograd of R.torch_form, sum(w_k * loss_k).backward(): every gradient tensor within REL_ACC of its largest magnitude"""
    outputs, targets, mine, restated, _ = closed(name)
    vis = {c[0]: c for c in R.CASES}[name][8]
    o64 = _leaves64(outputs)
    if "aux_outputs" in outputs:
        o64["aux_outputs"] = [_leaves64(a) for a in outputs["aux_outputs"]]
    losses, match = R.torch_form(o64, targets, R.CONSTS, masks=True, vis=vis)
    sum(G.WEIGHTS["_".join(k.split("_")[:2])] * v for k, v in losses.items()).backward()
    for L, (g, o) in enumerate(zip(mine, [o64] + o64.get("aux_outputs", []))):
        index = restated[L]["index"]
        assert torch.equal(match[L][1], index)
        for short, key in G.GRAD_KEYS:
            if key not in o:
                assert "g_" + short not in g
                continue
            ref = o[key].grad
            if short == "masks":
                assert not bool((ref[G.off_query_mask(ref.shape, index)] != 0).any())
                ref = G.matched_planes(ref, index)
            d, top = float((ref - g["g_" + short]).abs().max()), float(ref.abs().max())
            print(f"{name} L{L} {short}: max |d| {d:.3e} of max |g| {top:.3e}")
            assert d <= R.REL_ACC * top
            if short in ("boxes", "visible"):  # nothing off the matched query
                assert not bool((g["g_" + short][G.off_query_mask(ref.shape, index)] != 0).any())


@pytest.mark.parametrize("name", [c[0] for c in R.CASES])
def test_reference_fixture_against_the_closed_form(fixture, closed, name):
    """The reference's own autograd gradients within the derived bound plus the recorded margin, and the margin is that distance"""
    outputs, targets, mine, restated, _ = closed(name)
    for L, g in enumerate(mine):
        assert g["min_kink"] > G.KINK
        for short, key in G.GRAD_KEYS:
            if "g_" + short not in g:
                assert f"{name}_g_{short}{L}" not in fixture
                continue
            ref, margin = fixture[f"{name}_g_{short}{L}"], fixture[f"{name}_margin_{short}{L}"]
            assert ref.dtype == np.float32 and ref.shape == tuple(g["g_" + short].shape)
            d = np.abs(ref.astype(np.float64) - g["g_" + short].numpy())
            assert (d <= margin.astype(np.float64)).all() and (margin.astype(np.float64) <= d * (1 + 2.0 ** -22) + 1e-45).all()
            assert (d <= (g["e_" + short] + g["a_" + short]).numpy()).all()
            assert (d <= g["e_" + short].numpy() + margin).all()


def test_bad_arguments_are_rejected_with_the_entry_name(train_lib):
    from tce_rvos_amd._train_lib import CriterionConsts
    l, p = train_lib, 4096  # p: a non-null, aligned stand-in address; every call below is rejected before it is used
    mg, hg = "tce_criterion_mask_grad_f32", "tce_criterion_head_grads_f32"

    def rejected(status, name):
        assert status < 0 and name.encode() in l.tce_train_last_error(), (status, l.tce_train_last_error())

    rejected(l.tce_criterion_mask_grad_f32(None, None, None, None, None, None, None, None, 1, 1, 1, 8, 8, 32, 32, 0.25, None), mg)
    rejected(l.tce_criterion_mask_grad_f32(p, p, p, p, p, p, None, p, 1, 1, 1, 8, 8, 32, 32, 0.25, None), mg)      # gl
    rejected(l.tce_criterion_mask_grad_f32(p, p, p, p, p, p, p, None, 1, 1, 1, 8, 8, 32, 32, 0.25, None), mg)      # grad
    rejected(l.tce_criterion_mask_grad_f32(p, p, p, p, p, p, p, p, 65, 1, 1, 8, 8, 32, 32, 0.25, None), mg)        # B > 64
    rejected(l.tce_criterion_mask_grad_f32(p, p, p, p, p, p, p, p, 1, 65, 1, 8, 8, 32, 32, 0.25, None), mg)        # T > 64
    rejected(l.tce_criterion_mask_grad_f32(p, p, p, p, p, p, p, p, 1, 1, 1025, 8, 8, 32, 32, 0.25, None), mg)      # Q > 1024
    rejected(l.tce_criterion_mask_grad_f32(p, p, p, p, p, p, p, p, 1, 1, 1, 8, 10, 32, 40, 0.25, None), mg)        # 4w != ceil32(W)
    rejected(l.tce_criterion_mask_grad_f32(p, p, p, p, p, p, p, p, 1, 64, 1, 4096, 4096, 16384, 16384, 0.25, None), mg)  # T*h*w >= 2^30
    rejected(l.tce_criterion_mask_grad_f32(p, p, p, p, p, p, p, p + 2, 1, 1, 1, 8, 8, 32, 32, 0.25, None), mg)     # misaligned grad
    rejected(l.tce_criterion_mask_grad_f32(p, p, p + 4, p, p, p, p, p, 1, 1, 1, 8, 8, 32, 32, 0.25, None), mg)     # misaligned sums
    c = CriterionConsts(2, 5, 2, 2, 5, 2, 0.25)
    rejected(l.tce_criterion_head_grads_f32(None, None, None, None, None, None, None, None, None, None, None, None, 1, 1, 1, 1, c, None), hg)
    rejected(l.tce_criterion_head_grads_f32(p, p, None, p, p, p, p, p, None, p, p, None, 1, 1, 1, 1, c, None), hg)   # gl
    rejected(l.tce_criterion_head_grads_f32(p, p, None, p, p, p, p, p, p, None, None, None, 1, 1, 1, 1, c, None), hg)  # no output
    rejected(l.tce_criterion_head_grads_f32(p, p, None, p, p, p, p, p, p, p, p, p, 1, 1, 1, 1, c, None), hg)       # g_visible, no visible
    rejected(l.tce_criterion_head_grads_f32(p, p, None, p, p, p, p, p, p, p, p, None, 1, 1, 1, 129, c, None), hg)  # K > 128
    rejected(l.tce_criterion_head_grads_f32(p, p, None, p, p, p, p, p, p, p, p, None, 65, 1, 1, 1, c, None), hg)   # B > 64
    rejected(l.tce_criterion_head_grads_f32(p, p, None, p, p, p, p, p, p, p, p, None, 1, 1, 1025, 1, c, None), hg)  # Q > 1024
    rejected(l.tce_criterion_head_grads_f32(p, p, None, p + 4, p, p, p, p, p, p, p, None, 1, 1, 1, 1, c, None), hg)  # int64 labels
    rejected(l.tce_criterion_head_grads_f32(p, p, None, p, p, p, p, p, p, p, p, None, 1, 1, 1, 1, None, None), hg)  # consts


def _small(T=2, Q=3, H=32, W=32):
    h, w = R.ceil32(H) // 4, R.ceil32(W) // 4
    out = {"pred_logits": torch.zeros(1, T, Q, 1), "pred_boxes": torch.full((1, T, Q, 4), 0.5), "pred_masks": torch.zeros(1, T, Q, h, w)}
    tg = [{"masks": torch.zeros(T, H, W, dtype=torch.uint8), "boxes": torch.full((T, 4), 0.5), "labels": torch.zeros(T, dtype=torch.int64),
           "valid": torch.ones(T, dtype=torch.int64)}]
    return out, tg


def test_grad_mode_checks_precede_device_work():
    from tce_rvos_amd import _train_lib, ops
    from tce_rvos_amd.criterion import SetCriterion
    loaded = _train_lib._LIB
    crit = SetCriterion(1, {}, ["labels", "boxes", "masks"], grad=True)
    assert crit.grad is True
    out, tg = _small()
    out["pred_masks"].requires_grad_(True)
    with pytest.raises(ValueError, match="CPU tensor"):  # requires grad is accepted; the device check still comes first
        crit(out, tg)
    with pytest.raises(ValueError, match="requires grad"):  # matcher() stays forward only
        crit.matcher(out, tg)
    with pytest.raises(ValueError, match="requires grad"):
        crit.layer_values(out, tg)
    out, tg = _small()
    tg[0]["boxes"].requires_grad_(True)
    with pytest.raises(ValueError, match="targets.*requires grad"):
        crit(out, tg)
    crit.grad = False
    out, tg = _small()
    out["pred_boxes"].requires_grad_(True)
    with pytest.raises(ValueError, match="requires grad"):
        crit(out, tg)
    z = torch.zeros
    with pytest.raises(ValueError, match="CPU tensor"):
        ops.criterion_mask_grad(z(1, 1, 1, 8, 8), z(1, 1, 32, 32, dtype=torch.uint8), z(1, 3, 1, dtype=torch.float64),
                                z(1, dtype=torch.float64), z(1, dtype=torch.int32), z(1), z(6))
    with pytest.raises(ValueError, match="CPU tensor"):
        ops.criterion_head_grads(z(1, 1, 1, 1), z(1, 1, 1, 4), z(1, 1, dtype=torch.int64), z(1, 1, 4), z(1, 1, dtype=torch.int32),
                                 z(1, dtype=torch.int32), z(1), z(6))
    with pytest.raises(ValueError, match=r"pred_masks \[B,T,Q,h,w\] expected"):
        ops.criterion_mask_grad(z(1, 8, 8), None, None, None, None, None, None)
    assert _train_lib._LIB is loaded  # none of the above loaded anything


def test_grad_defaults_to_false():
    from tce_rvos_amd import build_model
    from tce_rvos_amd.criterion import SetCriterion, build_criterion
    assert SetCriterion(1, {}, ["labels", "boxes", "masks"]).grad is False
    assert build_criterion(argparse.Namespace(binary=True)).grad is False
    _, crit, _ = build_model(argparse.Namespace(backbone="swin_t_p4w7", with_box_refine=True, binary=True, freeze_text_encoder=True,
                                                f_token=8, qtrans=True, num_feature_levels=4, text_encoder_layers=1))
    assert crit.grad is False
    crit.grad = True  # a plain attribute
    assert crit.grad is True
