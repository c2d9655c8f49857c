"""CPU: the RefCOCO evaluation stage's header (include/tce_rvos_refexp.h): its macros and struct against the Python constants;
its two access models on hand-made argument blocks; the builders (the new one, and the old ones unchanged); argument
errors that need no device; plan_image_groups; RefExpScorer.summarize / merge on injected running maxima against the hits and the
summary of the reference's evaluator (tests/golden/refexp_cases.npz)."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _refexp as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "refexp_cases.npz")


@pytest.fixture(scope="module")
def fixture():
    return R.load_cases(FIXTURE)


def test_refexp_header_symbols_bound_exported_and_modelled():
    """What is the stage's own about include/tce_rvos_refexp.h: its macros against the constants of ops and _lib, the size of the
    sample struct, the build order.  Its symbols, bindings and access models are held by tests/test_host_cpu.py, with every other
    header's."""
    from tce_rvos_amd import _lib, ops
    from tce_rvos_amd import build as b
    b.build(verbose=False)                                            # the tests below call the library
    assert _lib.HEADERS["tce_rvos_refexp.h"] is _lib.REFEXP_SIGNATURES
    text = open(os.path.join(HERE, "..", "include", "tce_rvos_refexp.h")).read()
    macros = {k: int(v) for k, v in re.findall(r"#define\s+(TCE_REFEXP_[A-Z_]+)\s+(\d+)", text)}
    assert macros == {"TCE_REFEXP_GROUP_MAX": ops.REFEXP_GROUP_MAX, "TCE_REFEXP_MAX_CAND": ops.REFEXP_MAX_CAND}
    assert (_lib.REFEXP_GROUP_MAX, _lib.REFEXP_MAX_CAND) == (16, 1024) and ctypes.sizeof(_lib.RefexpSample) == 72
    assert "refexp.hip" in b.SOURCES and b.SOURCES[-1] == "png.hip"


def test_rejected_calls_return_a_code_and_launch_nothing():
    """Host-side argument checks of the two entries: a return code and a message, with null streams and no device"""
    from tce_rvos_amd import _lib
    l = _lib.lib()
    t = (_lib.RefexpSample * 2)()
    assert l.tce_refexp_group_u8(None, 1, 5, 1, 3, 4, 0.5, None) < 0
    for B, Q, K in ((0, 5, 1), (17, 5, 1), (1, 0, 1), (1, 5, 0), (1, 1025, 1), (1, 205, 5), (1, 513, 2)):
        assert l.tce_refexp_group_u8(t, B, Q, K, 3, 4, 0.5, None) < 0, (B, Q, K)
        assert b"tce_refexp_group_u8" in l.tce_last_error()
    assert b"1025" in l.tce_last_error() or b"1026" in l.tce_last_error()
    assert l.tce_refexp_group_u8(t, 1, 5, 1, 3, 4, 0.5, None) < 0 and b"nothing to do" in l.tce_last_error()   # all pointers NULL
    e = t[0]
    e.logits, e.boxes_in, e.scores, e.order, e.boxes_out, e.H0, e.W0 = 0x1000, 0x2000, 0x3000, 0x4000, 0x5002, 5, 7
    assert l.tce_refexp_group_u8(t, 1, 5, 1, 3, 4, 0.5, None) < 0 and b"aligned" in l.tce_last_error()
    e.boxes_out = 0x3004                                              # inside scores [0x3000, 0x3014)
    assert l.tce_refexp_group_u8(t, 1, 5, 1, 3, 4, 0.5, None) < 0 and b"overlap" in l.tce_last_error()
    e.boxes_out, e.masks, e.out, e.fh, e.fw = 0x5000, 0x6000, 0x7001, 13, 16
    assert l.tce_refexp_group_u8(t, 1, 5, 1, 3, 4, 0.5, None) < 0 and b"4x" in l.tce_last_error()
    e.fh = 12
    t[1].logits, t[1].boxes_in, t[1].scores, t[1].order, t[1].boxes_out, t[1].H0, t[1].W0 = 0x11000, 0x12000, 0x13000, 0x14000, 0x15000, 5, 7
    assert l.tce_refexp_group_u8(t, 2, 5, 1, 3, 4, 0.5, None) < 0 and b"box-only" in l.tce_last_error()
    e.H0 = e.W0 = 40000
    assert l.tce_refexp_group_u8(t, 1, 5, 1, 3, 4, 0.5, None) < 0 and b"2^31" in l.tce_last_error()
    for M, Q in ((0, 5), (65536, 5), (3, 0), (3, 1025)):
        assert l.tce_refexp_giou_f32(0x1000, 0x2000, 0x3000, 0x4000, M, Q, None) < 0, (M, Q)
        assert b"tce_refexp_giou_f32" in l.tce_last_error()
    assert l.tce_refexp_giou_f32(0x1000, None, 0x3000, 0x4000, 3, 5, None) < 0
    assert l.tce_refexp_giou_f32(0x1002, 0x2000, 0x3000, 0x4000, 3, 5, None) < 0 and b"aligned" in l.tce_last_error()


def test_the_access_models_on_hand_made_argument_blocks():
    from tce_rvos_amd import _lib, hazard
    Q, K, h, w = 6, 2, 3, 4
    t = (_lib.RefexpSample * 2)()
    for b, base in enumerate((0x100000, 0x200000)):
        e = t[b]
        e.logits, e.boxes_in, e.masks, e.scores, e.order, e.boxes_out, e.out = (base + 0x1000 * k for k in range(1, 8))
        e.fh, e.fw, e.H0, e.W0 = 9, 13, 5 + b, 7
    e = t[1]
    e.out += 3                                                        # any address
    rd, wr = hazard.MODELS["tce_refexp_group_u8"]((t, 2, Q, K, h, w, 0.5, 0))
    rd, wr = hazard.union(*rd), hazard.union(*wr)
    assert rd.tolist() == [[0x101000, 0x101000 + Q * K * 4], [0x102000, 0x102000 + Q * 16], [0x103000, 0x103000 + Q * h * w * 4],
                           [0x201000, 0x201000 + Q * K * 4], [0x202000, 0x202000 + Q * 16], [0x203000, 0x203000 + Q * h * w * 4]]
    assert wr.tolist() == [[0x104000, 0x104000 + Q * 4], [0x105000, 0x105000 + Q * 4], [0x106000, 0x106000 + Q * 16],
                           [0x107000, 0x107000 + Q * 5 * 7], [0x204000, 0x204000 + Q * 4], [0x205000, 0x205000 + Q * 4],
                           [0x206000, 0x206000 + Q * 16], [0x207003, 0x207003 + Q * 6 * 7]]
    # a box-only call names no mask bytes, neither read nor written -- whether it is masks or out that is NULL
    for field in ("masks", "out"):
        saved = [getattr(t[b], field) for b in range(2)]
        for b in range(2):
            setattr(t[b], field, None)
        rd, wr = hazard.MODELS["tce_refexp_group_u8"]((t, 2, Q, K, h, w, 0.5, 0))
        rd, wr = hazard.union(*rd), hazard.union(*wr)
        assert len(rd) == 4 and len(wr) == 6
        assert not any(0x103000 <= lo < 0x104000 or 0x203000 <= lo < 0x204000 for lo, _ in rd.tolist())
        assert not any(0x107000 <= lo < 0x108000 or 0x207000 <= lo < 0x208000 for lo, _ in wr.tolist())
        for b in range(2):
            setattr(t[b], field, saved[b])
    # a ranked call reads the order it is given and writes the masks alone
    for b in range(2):
        t[b].logits = None
    rd, wr = hazard.MODELS["tce_refexp_group_u8"]((t, 2, Q, K, h, w, 0.5, 0))
    assert hazard.union(*rd).tolist() == [[0x103000, 0x103000 + Q * h * w * 4], [0x105000, 0x105000 + Q * 4],
                                          [0x203000, 0x203000 + Q * h * w * 4], [0x205000, 0x205000 + Q * 4]]
    assert hazard.union(*wr).tolist() == [[0x107000, 0x107000 + Q * 5 * 7], [0x207003, 0x207003 + Q * 6 * 7]]
    M = 3
    rd, wr = hazard.MODELS["tce_refexp_giou_f32"]((0x10000, 0x20000, 0x30000, 0x40000, M, Q, 0))
    assert hazard.union(*rd).tolist() == [[0x10000, 0x10000 + M * Q * 16], [0x20000, 0x20000 + M * 16]]
    assert hazard.union(*wr).tolist() == [[0x30000, 0x30000 + M * Q * 4], [0x40000, 0x40000 + M * Q * 4]]


def test_builders_the_new_one_and_the_old_ones_unchanged():
    import tce_rvos_amd
    from tce_rvos_amd import postprocess
    from tce_rvos_amd.model import _Stub
    assert tce_rvos_amd.PostProcess is postprocess.PostProcess and tce_rvos_amd.PostProcessSegm is postprocess.PostProcessSegm
    assert tce_rvos_amd.build_refexp_postprocessors is postprocess.build_refexp_postprocessors
    post = postprocess.build_refexp_postprocessors(argparse.Namespace(masks=True, threshold=0.35))
    assert list(post) == ["bbox", "segm"] and type(post["bbox"]) is postprocess.PostProcess
    assert type(post["segm"]) is postprocess.PostProcessSegm and post["segm"].threshold == 0.35
    post = postprocess.build_refexp_postprocessors(argparse.Namespace(masks=False, threshold=0.35))
    assert list(post) == ["bbox"]
    assert list(postprocess.build_refexp_postprocessors(argparse.Namespace())) == ["bbox"]
    assert postprocess.PostProcessSegm().threshold == 0.5
    for ds in ("ytvos", "davis", "refcoco", None):                   # build_postprocessors is what it was: still the stub
        old = postprocess.build_postprocessors(argparse.Namespace(masks=True, threshold=0.35), ds)
        assert list(old) == ["segm"] and isinstance(old["segm"], _Stub)
    assert isinstance(postprocess.build_postprocessors(argparse.Namespace(threshold=0.4), "a2d"), postprocess.A2DSentencesPostProcess)


def test_argument_errors_need_no_gpu():
    from tce_rvos_amd import ops
    from tce_rvos_amd.postprocess import PostProcess, PostProcessSegm
    from tce_rvos_amd.refexp_score import RefExpScorer
    lg, bx, pm = torch.zeros(5, 1), torch.zeros(5, 4), torch.zeros(5, 3, 4)
    with pytest.raises(ValueError, match="at least one"):
        ops.refexp_group([], [], None, None, [])
    with pytest.raises(ValueError, match="on the GPU"):                # on the CPU: no fall-back
        ops.refexp_group([lg], [bx], None, None, [(5, 7)])
    with pytest.raises(ValueError, match="on the GPU"):
        ops.refexp_group([lg], [bx], [pm], [(9, 13)], [(5, 7)])
    with pytest.raises(ValueError, match="candidates"):
        ops.refexp_group([torch.zeros(1025, 1)], [torch.zeros(1025, 4)], None, None, [(5, 7)])
    with pytest.raises(ValueError, match="candidates"):
        ops.refexp_group([torch.zeros(513, 2)], [torch.zeros(513, 4)], None, None, [(5, 7)])
    with pytest.raises(ValueError, match=r"boxes\[0\]"):
        ops.refexp_group([lg], [torch.zeros(4, 4)], None, None, [(5, 7)])
    with pytest.raises(ValueError, match=r"masks\[0\]"):
        ops.refexp_group([lg], [bx], [torch.zeros(4, 3, 4)], [(9, 13)], [(5, 7)])
    with pytest.raises(ValueError, match=r"logits\[1\]"):
        ops.refexp_group([lg, torch.zeros(6, 1)], [bx, bx], None, None, [(5, 7)] * 2)
    with pytest.raises(ValueError, match="sizes"):
        ops.refexp_group([lg], [bx], [pm], None, [(5, 7)])
    with pytest.raises(ValueError, match="original sizes"):
        ops.refexp_group([lg], [bx], None, None, [(5, 7)] * 2)
    with pytest.raises(ValueError, match="outs without masks"):
        ops.refexp_group([lg], [bx], None, None, [(5, 7)], outs=[torch.zeros(5, 5, 7, dtype=torch.uint8)])
    with pytest.raises(ValueError, match="ranked"):
        ops.refexp_group([lg], [bx], None, None, [(5, 7)], order=[torch.zeros(5, dtype=torch.int32)])
    with pytest.raises(ValueError, match="one \\[Q,K\\]"):
        ops.refexp_group([torch.zeros(5)], [bx], None, None, [(5, 7)])
    boxes, gt = torch.zeros(3, 5, 4), torch.zeros(3, 4)
    with pytest.raises(ValueError, match="on the GPU"):
        ops.refexp_giou(boxes, gt)
    with pytest.raises(ValueError, match="boxes"):
        ops.refexp_giou(torch.zeros(3, 5), gt)
    with pytest.raises(ValueError, match="gt"):
        ops.refexp_giou(boxes, torch.zeros(3, 5))
    with pytest.raises(ValueError, match="pred_boxes"):
        PostProcess()({"pred_logits": torch.zeros(1, 1, 5, 1), "pred_boxes": torch.zeros(1, 1, 4, 4)}, [(5, 7)])
    with pytest.raises(ValueError, match="target sizes"):
        PostProcess()({"pred_logits": torch.zeros(1, 1, 5, 1), "pred_boxes": torch.zeros(1, 1, 5, 4)}, [(5, 7), (5, 7)])
    with pytest.raises(ValueError, match="pred_masks"):
        PostProcessSegm()([{}], {"pred_logits": torch.zeros(1, 1, 5, 1), "pred_boxes": torch.zeros(1, 1, 5, 4),
                                 "pred_masks": torch.zeros(1, 1, 4, 3, 4)}, [(5, 7)], [(9, 13)])
    # the scorer: its constructor and the target checks of update touch no device
    with pytest.raises(ValueError, match="k must"):
        RefExpScorer(k=5)
    s = RefExpScorer()
    res = {7: {"scores": torch.zeros(5), "boxes": torch.zeros(5, 4)}}
    with pytest.raises(ValueError, match="no target"):
        s.update(res, {})
    with pytest.raises(ValueError, match="width -1.0"):               # the reference asserts inside generalized_box_iou
        s.update(res, {7: {"bbox": [1.0, 2.0, -1.0, 3.0], "dataset_name": "refcoco"}})
    with pytest.raises(ValueError, match="height -0.5"):
        s.update(res, {7: {"bbox": [1.0, 2.0, 1.0, -0.5], "dataset_name": "refcoco"}})
    with pytest.raises(ValueError, match="width nan"):
        s.update(res, {7: {"bbox": [1.0, 2.0, float("nan"), 3.0], "dataset_name": "refcoco"}})
    with pytest.raises(ValueError, match="2 targets"):
        s.update(res, {7: [{"bbox": [1, 2, 3, 4], "dataset_name": "refcoco"}] * 2})
    with pytest.raises(ValueError, match="dataset_name"):
        s.update(res, {7: {"bbox": [1, 2, 3, 4], "dataset_name": "coco"}})
    with pytest.raises(ValueError, match="dataset_name"):
        s.update(res, {7: {"bbox": [1, 2, 3, 4]}})
    with pytest.raises(ValueError, match="on the GPU"):
        s.update(res, {7: {"bbox": [1, 2, 3, 4], "dataset_name": "refcoco"}})
    assert s.state() == {"image_ids": [], "datasets": [], "best": []}
    assert s.summarize() == {d: [0.0, 0.0, 0.0] for d in R.DATASETS}  # a dataset with no image keeps zeros


def test_plan_image_groups():
    from tce_rvos_amd.refexp import plan_image_groups
    a, b = (3, 64, 96, 64, 96), (3, 64, 80, 64, 80)
    shapes = [a, b, a, a, b, a, a]
    lengths = [8, 8, 8, 9, 8, 8, 8]
    assert plan_image_groups(shapes, lengths, max_group=2) == [[0, 2], [5, 6], [1, 4], [3]]
    assert plan_image_groups(shapes, lengths, max_group=8) == [[0, 2, 5, 6], [1, 4], [3]]
    assert plan_image_groups(shapes, lengths, max_group=3, mixed_lengths=True) == [[0, 2, 3], [5, 6], [1, 4]]
    assert plan_image_groups(shapes, lengths, max_group=1) == [[0], [2], [5], [6], [1], [4], [3]]
    assert plan_image_groups(shapes, lengths, max_group=0) == plan_image_groups(shapes, lengths, max_group=1)
    assert plan_image_groups([], []) == []
    for plan in (plan_image_groups(shapes, lengths, 2), plan_image_groups(shapes, lengths, 3, True)):
        assert sorted(i for g in plan for i in g) == list(range(7))  # every sample exactly once
    with pytest.raises(ValueError):
        plan_image_groups(shapes, lengths[:-1])


def _images(fixture):
    """(image_id, dataset, running maxima, hits) of every image of the fixture: the cases' samples, then the synthetic set"""
    cases, syn, _ = fixture
    out, k = [], 0
    for c in cases:
        for b in range(c["B"]):
            out.append((k, c["dataset"][b], np.maximum.accumulate(c["giou"][b].numpy()).tolist(), c["hits"][b]))
            k += 1
    for m in range(len(syn["gt"])):
        out.append((k, syn["dataset"][m], np.maximum.accumulate(syn["giou"][m].numpy()).tolist(), syn["hits"][m]))
        k += 1
    return out


def test_scorer_summary_on_injected_running_maxima(fixture):
    """RefExpScorer.summarize / merge on the running maxima of the reference's own giou values against the hits recorded from
    generalized_box_iou and the summary RefExpEvaluator.summarize printed, and on a split over two ranks"""
    from tce_rvos_amd.refexp_score import RefExpScorer, hits
    ims = _images(fixture)
    summary = fixture[2]
    assert len(ims) == 5 + R.SYN[0] and {d for _, d, _, _ in ims} == set(R.DATASETS)
    for _, _, best, want in ims:
        assert hits(best, R.K_AT, 0.5) == want
    state = {"image_ids": [i for i, _, _, _ in ims], "datasets": [d for _, d, _, _ in ims], "best": [b for _, _, b, _ in ims]}
    s = RefExpScorer()
    merged = s.merge([state])
    assert merged["image_ids"] == state["image_ids"]
    got = s.summarize()
    assert list(got) == list(R.DATASETS)
    for d in R.DATASETS:
        assert got[d] == sorted(got[d]) and np.allclose(got[d], summary[d], rtol=0, atol=1e-12), (d, got[d], summary[d])
    assert any(v > 0 for d in R.DATASETS for v in got[d]) and any(v < 1 for d in R.DATASETS for v in got[d])

    def part(sel):
        return {k: [v[i] for i in sel] for k, v in state.items()}
    n = len(ims)
    two = RefExpScorer()
    two.merge([part(range(0, n, 2)), part(range(1, n, 2))])
    assert two.summarize() == got
    pad = RefExpScorer()                                              # a sampler's padding: an image in both states, identical
    pad.merge([part(range(0, n, 2)), part([0] + list(range(1, n, 2)))])
    assert pad.summarize() == got
    bad = part([0])
    bad["best"] = [[v + 0.25 for v in bad["best"][0]]]
    with pytest.raises(ValueError, match="different results"):
        RefExpScorer().merge([state, bad])
    with pytest.raises(ValueError, match="dataset_name"):
        RefExpScorer().merge([{"image_ids": [1], "datasets": ["coco"], "best": [[0.1]]}])
    # k beyond the number of boxes takes them all (giou[:k]); the threshold is compared as >=
    assert hits([0.1, 0.5, 0.5], (1, 2, 10), 0.5) == [False, True, True]
    assert hits([0.1, 0.49999997, 0.49999997], (3,), 0.5) == [False]
    one = RefExpScorer(k=(1, 2), thresh_iou=0.3)
    one.merge([{"image_ids": ["a", "b"], "datasets": ["refcocog", "refcocog"], "best": [[0.1, 0.3], [0.35, 0.35]]}])
    assert one.summarize() == {"refcoco": [0.0, 0.0], "refcoco+": [0.0, 0.0], "refcocog": [0.5, 1.0]}
