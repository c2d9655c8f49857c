"""CPU: the criterion's restatement against the reference fixture, the train library's header against its binding table and
exported symbols, argument rejection (before any launch, so null pointers are safe), the build_model boundary, and the ValueError
cases whose checks precede device work."""
import argparse
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _criterion as R
from _util import load_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "train", "tce_rvos_train.h")


@pytest.fixture(scope="module")
def fixture():
    return load_npz("criterion_cases.npz")


@pytest.fixture(scope="module")
def train_lib():
    from tce_rvos_amd import _train_lib
    return _train_lib.lib()  # builds the library when its file is absent


def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"\b(tce_[a-z0-9_]+)\s*\(", text))


@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_restatement_matches_reference_fixture(fixture, case):
    """The fp64 restatement against the reference's own matcher and criterion: the same match, costs and losses within the derived
    bound plus what the reference's fp32 sums may lose in the worst case"""
    name, seed, B, T, Q, K, (H, W), valid, vis, n_aux = case
    outputs, targets = R.make_case(case)
    layers, num_boxes = R.restate(outputs, targets, R.CONSTS, masks=True, vis=vis)
    assert num_boxes == max(1.0, float(sum(sum(v) for v in valid)))
    N = T * (R.ceil32(H) // 4) * (R.ceil32(W) // 4)
    names = []
    for L, r in enumerate(layers):
        assert np.array_equal(fixture[f"{name}_index{L}"], r["index"].numpy())
        d = np.abs(fixture[f"{name}_cost{L}"].astype(np.float64) - r["cost"].numpy())
        allowed = r["e_cost"].numpy() + R.ref_sum_bound(N) * (R.CONSTS["cost_mask"] + R.CONSTS["cost_dice"]) * 2
        assert (d <= allowed).all(), (d.max(), allowed.min())
        assert np.array_equal(d, fixture[f"{name}_margin_cost{L}"])  # the recorded margin is this distance
        names += [k + ("" if L == 0 else f"_{L - 1}") for k in R.loss_names(True, vis)]
    assert list(fixture[f"{name}_loss_names"]) == names
    mine = np.asarray([float(layers[L]["losses"][R.LOSS_ORDER.index(k)]) for L in range(len(layers)) for k in R.loss_names(True, vis)])
    e = np.asarray([float(layers[L]["e_losses"][R.LOSS_ORDER.index(k)]) for L in range(len(layers)) for k in R.loss_names(True, vis)])
    d = np.abs(fixture[f"{name}_loss_values"].astype(np.float64) - mine)
    assert (d <= e + R.ref_sum_bound(max(N, T * Q * K)) * np.abs(mine)).all(), (d, e)
    # the torch form (the loop a caller writes today, tools/criterion_bench.py's baseline) is the same function
    tl, match = R.torch_form(outputs, targets, R.CONSTS, masks=True, vis=vis)
    assert list(tl) == names
    for L, (cost, idx) in enumerate(match):
        assert np.array_equal(idx.numpy(), fixture[f"{name}_index{L}"])
    assert np.allclose(np.asarray([float(tl[k]) for k in names]), fixture[f"{name}_loss_values"], rtol=1e-4, atol=1e-6)


def test_header_table_and_exported_symbols(train_lib):
    from tce_rvos_amd import _lib, _train_lib
    from tce_rvos_amd import build as b
    declared = _declared()
    assert declared == set(_train_lib.TRAIN_SIGNATURES), declared ^ set(_train_lib.TRAIN_SIGNATURES)
    raw = ctypes.CDLL(b.TRAIN_LIB)
    for name, (res, args) in _train_lib.TRAIN_SIGNATURES.items():
        assert hasattr(raw, name), name
        fn = getattr(train_lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert train_lib.tce_train_abi_version() == 1
    # the sibling library shares no name with the inference registry, and its header is not one of include/
    every = set().union(*_lib.HEADERS.values())
    assert not (declared & every)
    inc = os.path.join(ROOT, "include")
    assert "tce_rvos_train.h" not in os.listdir(inc)
    text = "".join(open(os.path.join(inc, f)).read() for f in os.listdir(inc))
    assert not [n for n in declared if n in text]
    # rebuilt when its source or train/*.h change; the inference library's lists are what they were
    deps = {os.path.realpath(d) for d in b.train_dependencies()}
    assert os.path.realpath(HEADER) in deps and b.TRAIN_SOURCES == ["criterion.hip"]
    assert "criterion.hip" not in b.SOURCES and os.path.realpath(HEADER) not in {os.path.realpath(d) for d in b.dependencies()}
    assert os.path.basename(b.LIB) == "libtce_rvos.so" and os.path.basename(b.TRAIN_LIB) == "libtce_rvos_train.so"


def test_bad_arguments_are_rejected_with_the_entry_name(train_lib):
    from tce_rvos_amd._train_lib import CriterionConsts
    l, p = train_lib, 4096  # p: a non-null, aligned stand-in address; every call below is rejected before it is used
    sums = "tce_criterion_mask_sums_f64"
    match = "tce_criterion_match_losses_f32"

    def rejected(status, name):
        assert status < 0 and name.encode() in l.tce_train_last_error(), (status, l.tce_train_last_error())

    rejected(l.tce_criterion_mask_sums_f64(None, None, None, None, None, 1, 1, 1, 8, 8, 32, 32, 0.25, None), sums)
    rejected(l.tce_criterion_mask_sums_f64(p, p, p, p, p, 65, 1, 1, 8, 8, 32, 32, 0.25, None), sums)      # B > 64
    rejected(l.tce_criterion_mask_sums_f64(p, p, p, p, p, 1, 65, 1, 8, 8, 32, 32, 0.25, None), sums)      # T > 64
    rejected(l.tce_criterion_mask_sums_f64(p, p, p, p, p, 1, 1, 1025, 8, 8, 32, 32, 0.25, None), sums)    # Q > 1024
    rejected(l.tce_criterion_mask_sums_f64(p, p, p, p, p, 1, 1, 1, 8, 10, 32, 40, 0.25, None), sums)      # 4w != ceil32(W)
    rejected(l.tce_criterion_mask_sums_f64(p, p, p, p, p, 1, 1, 1, 9, 8, 33, 32, 0.25, None), sums)       # 4h != ceil32(H)
    rejected(l.tce_criterion_mask_sums_f64(p + 2, p, p, p, p, 1, 1, 1, 8, 8, 32, 32, 0.25, None), sums)   # misaligned pred
    assert l.tce_criterion_mask_sums_ws_bytes(0, 1, 1, 8, 8) < 0 and b"tce_criterion_mask_sums_ws_bytes" in l.tce_train_last_error()
    assert l.tce_criterion_mask_sums_ws_bytes(1, 5, 5, 96, 160) == 5 * 19 * 4 * 8  # ceil(76800 / 4096) workgroups per query
    c = CriterionConsts(2, 5, 2, 2, 5, 2, 0.25)
    rejected(l.tce_criterion_match_losses_f32(None, None, None, None, None, None, None, None, None, None, None, None, None,
                                              1, 1, 1, 1, 8, 8, c, None), match)
    rejected(l.tce_criterion_match_losses_f32(p, p, None, p, p, p, p, p, p, p, p, p, p, 1, 1, 1, 129, 8, 8, c, None), match)  # K
    rejected(l.tce_criterion_match_losses_f32(p, p, None, p, None, p, p, p, p, p, p, p, p, 1, 1, 1, 1, 8, 8, c, None), match)  # st
    rejected(l.tce_criterion_match_losses_f32(p, p, None, p, p, p + 4, p, p, p, p, p, p, p, 1, 1, 1, 1, 8, 8, c, None), match)  # int64


def _args(**kw):
    return argparse.Namespace(backbone="swin_t_p4w7", with_box_refine=True, binary=True, freeze_text_encoder=True, f_token=8,
                              qtrans=True, num_feature_levels=4, text_encoder_layers=1, **kw)


@pytest.mark.parametrize("aux", [0, 1])
@pytest.mark.parametrize("vis", [0, 1])
def test_build_criterion_weight_dict_is_the_reference_s(fixture, aux, vis):
    from tce_rvos_amd.criterion import SetCriterion, build_criterion
    crit = build_criterion(argparse.Namespace(binary=True, aux_loss=bool(aux), vis_loss=bool(vis)))
    assert isinstance(crit, SetCriterion)
    assert list(crit.weight_dict) == list(fixture[f"weight_a{aux}_v{vis}_names"])
    assert [float(v) for v in crit.weight_dict.values()] == fixture[f"weight_a{aux}_v{vis}_values"].tolist()
    assert crit.losses == ["labels", "boxes", "masks"] + (["visible"] if vis else [])
    assert build_criterion(argparse.Namespace()).num_classes == 65 and build_criterion(argparse.Namespace(dataset_file="a2d")).num_classes == 1


def test_build_model_returns_a_criterion_and_loads_nothing():
    """In a fresh interpreter: import, build_model on a sparse namespace, no library loaded by either"""
    code = ("import argparse, sys; sys.path.insert(0, %r)\n"
            "import tce_rvos_amd\n"
            "from tce_rvos_amd import _lib, _train_lib\n"
            "m, c, p = tce_rvos_amd.build_model(argparse.Namespace(backbone='swin_t_p4w7', with_box_refine=True, binary=True, "
            "freeze_text_encoder=True, f_token=8, qtrans=True, num_feature_levels=4, text_encoder_layers=1))\n"
            "assert type(c).__name__ == 'SetCriterion' and isinstance(c, tce_rvos_amd.SetCriterion)\n"
            "assert set(c.weight_dict) >= {'loss_ce', 'loss_bbox', 'loss_giou', 'loss_mask', 'loss_dice', 'loss_dice_2'}\n"
            "assert _lib._LIB is None and _train_lib._LIB is None\n"
            "assert not [l for l in open('/proc/self/maps') if 'libtce_rvos' in l]\n"
            "print('ok')\n") % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]


def _small(T=2, Q=3, K=1, H=32, W=32, B=1, h=None, w=None, vis=False):
    h, w = h or R.ceil32(H) // 4, w or R.ceil32(W) // 4
    out = {"pred_logits": torch.zeros(B, T, Q, K), "pred_boxes": torch.full((B, T, Q, 4), 0.5), "pred_masks": torch.zeros(B, T, Q, h, w)}
    if vis:
        out["pred_visible"] = torch.zeros(B, T, Q, 1)
    tg = [{"masks": torch.zeros(T, H, W, dtype=torch.uint8), "boxes": torch.full((T, 4), 0.5), "labels": torch.zeros(T, dtype=torch.int64),
           "valid": torch.ones(T, dtype=torch.int64)} for _ in range(B)]
    return out, tg


def test_value_errors_precede_device_work():
    from tce_rvos_amd import _train_lib
    from tce_rvos_amd.criterion import SetCriterion
    loaded = _train_lib._LIB
    crit = SetCriterion(1, {}, ["labels", "boxes", "masks"])
    out, tg = _small()
    with pytest.raises(ValueError, match="CPU tensor"):
        crit(out, tg)
    with pytest.raises(ValueError, match="CPU tensor"):
        crit.matcher(out, tg)
    out, tg = _small()
    out["pred_masks"].requires_grad_(True)
    with pytest.raises(ValueError, match="requires grad"):
        crit(out, tg)
    out, tg = _small(h=8, w=10)
    with pytest.raises(ValueError, match="padded to a multiple of 32"):
        crit(out, tg)
    out, tg = _small(B=2, vis=True)
    with pytest.raises(ValueError, match="one clip per call"):
        SetCriterion(1, {}, ["labels", "boxes", "masks", "visible"], vis=True)(out, tg)
    out, tg = _small(T=65)
    with pytest.raises(ValueError, match="limits exceeded"):
        crit(out, tg)
    out, tg = _small(K=129)
    with pytest.raises(ValueError, match="limits exceeded"):
        crit(out, tg)
    out, tg = _small()
    del out["pred_masks"]
    with pytest.raises(ValueError, match="without pred_masks"):
        crit(out, tg)
    out, tg = _small()
    with pytest.raises(ValueError, match="CPU tensor"):  # the list-of-dicts form reaches the same checks
        crit([out, out], tg + tg)
    with pytest.raises(ValueError, match="do you really want"):
        SetCriterion(1, {}, ["cardinality"])
    assert _train_lib._LIB is loaded  # none of the above loaded anything
    from tce_rvos_amd import ops
    with pytest.raises(ValueError, match="CPU tensor"):
        ops.criterion_mask_sums(torch.zeros(1, 1, 1, 8, 8), torch.zeros(1, 1, 32, 32, dtype=torch.uint8))
