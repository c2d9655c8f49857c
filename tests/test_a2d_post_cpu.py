"""The A2D-Sentences / JHMDB-Sentences post-processor, the parts that need no GPU (the evaluation-stage header against its binding
table, the exported symbols and the access models: tests/test_host_cpu.py, with every other header): the two access models on
hand-made argument blocks; rle_to_string against the plain-loop restatement of cocoapi (tests/_a2d.py), the issue's check values
and the committed fixture; build_postprocessors; the argument checks of ops.a2d_masks / ops.rle_counts."""
import argparse
import os

import numpy as np
import pytest
import torch

import _a2d
from tce_rvos_amd import _lib, hazard
from tce_rvos_amd.postprocess import A2DSentencesPostProcess, build_postprocessors, rle_to_string

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "a2d_post_cases.npz")


def test_rle_ws_bytes_and_host_side_rejections_need_no_device():
    l = _lib.lib()
    seg = 1024  # TCE_RLE_SEGMENT
    assert f"#define TCE_RLE_SEGMENT {seg}" in open(os.path.join(ROOT, "include", "tce_rvos_eval.h")).read()
    assert l.tce_rle_ws_bytes(1, 1, 1) == 8 and l.tce_rle_ws_bytes(5, 240, 320) == 5 * 75 * 8
    assert l.tce_rle_ws_bytes(3, 32, 32) == 3 * 8 and l.tce_rle_ws_bytes(3, 32, 33) == 3 * 2 * 8
    assert l.tce_rle_ws_bytes(0, 4, 4) < 0 and l.tce_rle_ws_bytes(1, -1, 4) < 0 and l.tce_rle_ws_bytes(1, 1 << 16, 1 << 15) < 0
    # every rejection happens before anything is launched: null pointers, bad extents, the 4x rule, 2^31
    assert l.tce_a2d_masks_u8(None, 0x1000, 1, 2, 2, 8, 8, 4, 4, 0.5, None) != 0
    assert b"tce_a2d_masks_u8" in l.tce_last_error() and b"null" in l.tce_last_error()
    assert l.tce_a2d_masks_u8(0x1000, None, 1, 2, 2, 8, 8, 4, 4, 0.5, None) != 0
    for bad in ((0, 2, 2, 8, 8, 4, 4), (1, 0, 2, 8, 8, 4, 4), (1, 2, 2, 0, 8, 4, 4), (1, 2, 2, 8, 8, 4, -1)):
        assert l.tce_a2d_masks_u8(0x1000, 0x2000, *bad, 0.5, None) != 0 and b"extent" in l.tce_last_error(), bad
    assert l.tce_a2d_masks_u8(0x1000, 0x2000, 1, 2, 2, 9, 8, 4, 4, 0.5, None) != 0 and b"4x" in l.tce_last_error()
    assert l.tce_a2d_masks_u8(0x1000, 0x2000, 1, 2, 2, 8, 9, 4, 4, 0.5, None) != 0
    assert l.tce_a2d_masks_u8(0x1000, 0x2000, 2, 2, 2, 8, 8, 1 << 15, 1 << 15, 0.5, None) != 0 and b"2^31" in l.tce_last_error()
    assert l.tce_a2d_masks_u8(0x1000, 0x2000, 1 << 12, 1 << 10, 1 << 9, 8, 8, 4, 4, 0.5, None) != 0
    for args in ((None, 0x2000, 0x3000, 0x4000, 1, 4, 4), (0x1000, None, 0x3000, 0x4000, 1, 4, 4), (0x1000, 0x2000, None, 0x4000, 1, 4, 4),
                 (0x1000, 0x2000, 0x3000, None, 1, 4, 4), (0x1000, 0x2000, 0x3000, 0x4000, 0, 4, 4), (0x1000, 0x2000, 0x3000, 0x4000, 1, 4, 0),
                 (0x1000, 0x2000, 0x3000, 0x4000, 1, 1 << 16, 1 << 15), (0x1000, 0x2000, 0x3000, 0x4000, 1 << 16, 4, 4),
                 (0x1000, 0x2000, 0x3000, 0x4004, 1, 4, 4)):
        assert l.tce_rle_counts_u32(*args, None) != 0 and b"tce_rle_counts_u32" in l.tce_last_error(), args


def test_access_models_on_hand_made_blocks():
    N, h, w, fh, fw, H0, W0 = 5, 18, 25, 72, 100, 111, 151
    masks, out = 0x100000, 0x900003  # out on an odd address
    rd, wr = hazard.MODELS["tce_a2d_masks_u8"]((masks, out, N, h, w, fh, fw, H0, W0, 0.5, 0))
    assert hazard.union(*rd).tolist() == [[masks, masks + N * h * w * 4]]
    assert hazard.union(*wr).tolist() == [[out, out + N * H0 * W0]]
    P, H, W = 3, 87, 145
    m, counts, nruns, ws = 0x200001, 0x400000, 0x800000, 0xA00000  # masks on an odd address
    wsb = _lib.lib().tce_rle_ws_bytes(P, H, W)
    assert wsb == P * -(-H * W // 1024) * 8
    rd, wr = hazard.MODELS["tce_rle_counts_u32"]((m, counts, nruns, ws, P, H, W, 0))
    assert hazard.union(*rd).tolist() == [[m, m + P * H * W], [ws, ws + wsb]]
    assert hazard.union(*wr).tolist() == [[counts, counts + P * (H * W + 1) * 4], [nruns, nruns + 4 * P], [ws, ws + wsb]]


def test_recording_proxy_consults_the_eval_models_after_the_video_models():
    class Real:
        def __getattr__(self, name):
            return lambda *a: 0
    rec = hazard.Recorder()
    proxy = hazard._LibProxy(Real(), rec, dry=True)
    proxy.tce_a2d_masks_u8(0x1000, 0x9003, 2, 3, 3, 12, 12, 5, 7, 0.5, 0)
    proxy.tce_label_objects_u8((_lib.LabelObj * 1)(), 1, 0x9000, 0xA000, 1, 2, 1, 3, 3, 6, 6, 0.5, 0.1, 0)
    assert [x.name for x in rec.launches] == ["tce_a2d_masks_u8", "tce_label_objects_u8"]
    assert rec.launches[0].writes.tolist() == [[0x9003, 0x9003 + 70]] and rec.launches[0].reads.tolist() == [[0x1000, 0x1000 + 72]]
    assert proxy.tce_rle_ws_bytes(1, 2, 3) == 0 and len(rec.launches) == 2  # a query: passed through, not recorded
    with pytest.raises(RuntimeError):
        proxy.tce_not_modelled_anywhere


def test_rle_to_string_check_values():
    """The four values of the plain-loop restatement (not checked against pycocotools itself, which is absent here)."""
    for counts, want in (([4], b"4"), ([0, 4], b"04"), ([1, 2, 1], b"121"), ([100, 5, 3, 50, 2, 40], b"T353]1OF")):
        assert rle_to_string(counts) == want == _a2d.rle_string(counts), counts
        assert rle_to_string(np.asarray(counts, dtype=np.int32)) == want
        assert _a2d.rle_from_string(want) == counts
    assert rle_to_string([]) == b""


def test_rle_to_string_matches_the_loop_on_random_counts():
    rng = np.random.default_rng(7)
    seen_neg = seen_big = 0
    for trial in range(300):
        n = int(rng.integers(1, 60))
        hi = (40, 1 << 10, 1 << 15, 1 << 20, (1 << 31) - 1)[trial % 5]
        counts = rng.integers(0 if trial % 7 == 0 else 1, hi, size=n)
        if trial % 3 == 0:
            counts[rng.integers(0, n)] = (1 << 15) + int(rng.integers(0, 1 << 16))
        diffs = counts[3:] - counts[1:-2] if n > 3 else np.zeros(0)
        seen_neg += int((diffs < 0).sum())
        seen_big += int((counts >= 1 << 15).sum())
        s = rle_to_string(counts)
        assert s == _a2d.rle_string(counts.tolist()), counts.tolist()
        assert _a2d.rle_from_string(s) == counts.tolist()
    assert seen_neg > 500 and seen_big > 500, (seen_neg, seen_big)
    # the group boundaries of the sign rule: values whose top emitted group has bit 4 set / clear
    edge = [0, 15, 16, 31, 32, 511, 512, 1023, 1024, (1 << 15) - 1, 1 << 15, (1 << 31) - 1]
    for a in edge:
        for b in edge:
            c = [7, b, 3, a, 5, a]  # differences a - b, 5 - 3, a - a
            assert rle_to_string(c) == _a2d.rle_string(c), c


def test_fixture_strings_masks_and_contested_share():
    assert os.path.getsize(FIXTURE) < 1_000_000
    cases = _a2d.load_cases(FIXTURE)
    assert [c["name"] for c in cases] == [c[0] for c in _a2d.CASES] == ["A", "B", "C", "D"]
    for c, (name, seed, N, hw, size, orig, kind, scale) in zip(cases, _a2d.CASES):
        share = float(c["contested"].float().mean())
        print(f"case {name}: contested share {share:.3e}")
        assert share <= _a2d.MAX_SHARE and (name not in ("C", "D") or share == 0.0), (name, share)
        assert c["size"] == tuple(size) and c["orig"] == tuple(orig) and tuple(c["masks"].shape) == (N,) + tuple(hw)
        assert tuple(c["ref"].shape) == (N,) + tuple(orig) and len(c["rle"]) == N and tuple(c["scores"].shape) == (N,)
        assert size[0] <= 4 * hw[0] and size[1] <= 4 * hw[1]
        # the restatement run again here: the class's masks wherever neither run calls the pixel contested
        ref, v = _a2d.reference_post(c["masks"], size, orig)
        cont = _a2d.contested(v)
        assert not bool(((ref != c["ref"]) & ~(cont | c["contested"])).any())
        assert float((c["scores"] - c["logits"].sigmoid()).abs().max()) <= 1e-6
        for n in range(N):
            counts = _a2d.rle_from_string(c["rle"][n])
            assert counts == _a2d.rle_counts(c["ref"][n].numpy()), (name, n)
            assert rle_to_string(counts) == c["rle"][n] == _a2d.rle_string(counts), (name, n)
            assert np.array_equal(_a2d.rle_decode(counts, *orig), c["ref"][n].numpy())
    b_runs = [len(_a2d.rle_from_string(s)) for s in cases[1]["rle"]]
    assert min(b_runs) > 1000, b_runs  # case B is the many-runs case


def test_float_nearest_rows_differ_from_the_integer_formula_in_the_fixture_shapes():
    """Cases A and C hold output rows where ATen's fp32 nearest index is not (yo*fh)//H0 -- the rows an integer formula gets wrong."""
    for fh, H0 in ((72, 111), (72, 222), (90, 87)):
        yo = np.arange(H0)
        f = np.minimum(np.floor(yo.astype(np.float32) * (np.float32(fh) / np.float32(H0))).astype(np.int64), fh - 1)
        assert int((f != (yo * fh) // H0).sum()) > 0, (fh, H0)
        t = torch.nn.functional.interpolate(torch.arange(fh, dtype=torch.float32).view(1, 1, fh, 1), size=(H0, 1), mode="nearest")
        assert np.array_equal(t.view(-1).numpy().astype(np.int64), f), (fh, H0)  # ... and the formula of the header is ATen's


def test_build_postprocessors_and_build_model_third_value():
    from tce_rvos_amd import build_model
    from tce_rvos_amd.model import _Stub
    for ds in ("a2d", "jhmdb"):
        p = build_postprocessors(argparse.Namespace(threshold=0.3), ds)
        assert isinstance(p, A2DSentencesPostProcess) and isinstance(p, torch.nn.Module) and p.threshold == 0.3
        assert build_postprocessors(argparse.Namespace(), ds).threshold == 0.5
    for ds in ("ytvos", "davis", "refcoco", None):
        p = build_postprocessors(argparse.Namespace(threshold=0.3, masks=True), ds)
        assert isinstance(p, dict) and set(p) == {"segm"} and isinstance(p["segm"], _Stub)
        with pytest.raises(NotImplementedError):
            p["segm"]()
    kw = dict(backbone="swin_t_p4w7", with_box_refine=True, binary=True, freeze_text_encoder=True, f_token=8, qtrans=True,
              num_feature_levels=4, text_encoder_layers=1)
    _, _, post = build_model(argparse.Namespace(dataset_file="a2d", threshold=0.5, **kw))
    assert isinstance(post, A2DSentencesPostProcess)
    _, _, post = build_model(argparse.Namespace(**kw))
    assert isinstance(post, dict) and isinstance(post["segm"], _Stub)


def test_argument_checks_need_no_device():
    from tce_rvos_amd import ops
    pm = torch.zeros(2, 4, 5)
    with pytest.raises(ValueError, match="on the GPU"):
        ops.a2d_masks(pm, (16, 20), (8, 10))  # CPU tensor
    with pytest.raises(ValueError, match="contiguous"):
        ops.a2d_masks(torch.zeros(2, 5, 4).transpose(1, 2), (16, 20), (8, 10))
    with pytest.raises(ValueError):
        ops.a2d_masks(pm.double(), (16, 20), (8, 10))
    with pytest.raises(ValueError):
        ops.a2d_masks(pm[0], (16, 20), (8, 10))
    with pytest.raises(ValueError, match="on the GPU"):
        ops.rle_counts(torch.zeros(2, 4, 5, dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.rle_counts(torch.zeros(2, 4, 5))
    post = A2DSentencesPostProcess()
    with pytest.raises(ValueError, match="samples"):
        post({"pred_logits": torch.zeros(1, 1, 2, 1), "pred_masks": torch.zeros(1, 1, 2, 4, 5)}, torch.tensor([[8, 10], [8, 10]]),
             torch.tensor([[16, 20]]))
    with pytest.raises(ValueError, match="pred_logits"):
        post({"pred_logits": torch.zeros(1, 2, 1), "pred_masks": torch.zeros(1, 1, 2, 4, 5)}, torch.tensor([[8, 10]]), torch.tensor([[16, 20]]))
