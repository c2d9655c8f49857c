"""CPU: the A2D scoring entries' access models on hand-made blocks (their header against its binding table, the exported symbols
and the checker's tables: tests/test_host_cpu.py, with every other header), the run-length string reader, and the host scoring functions on integer counts -- against the reference's own function through the
fixture (tests/golden/a2d_score_cases.npz), the plain-loop restatement of COCOeval (tests/_a2d_score.py) and cases derived by
hand.  No AP number here was compared with pycocotools' own output (it is on no machine this project can use)."""
import os
import pickle
import re

import numpy as np
import pytest

import _a2d
import _a2d_score as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "a2d_score_cases.npz")
LAUNCHING = ("tce_rle_decode_u8", "tce_mask_overlap_i32")
QUERIES = ("tce_rle_decode_ws_bytes", "tce_mask_overlap_ws_bytes")
AP_KEYS = ("mAP 0.5:0.95", "AP 0.5", "AP 0.75", "AP 0.5:0.95 S", "AP 0.5:0.95 M", "AP 0.5:0.95 L")


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as g  # noqa: F401
    from tce_rvos_amd import build as b
    return b.build(verbose=False)


@pytest.fixture(scope="module")
def cases():
    return S.load_cases(FIXTURE)


# ------------------------------------------------------------------------------------------- the header and the access models
# (symbols, binding table, exports, argtypes, models / launch-free names of include/tce_rvos_score.h: tests/test_host_cpu.py)
def test_the_header_says_which_entries_launch_nothing():
    text = open(os.path.join(ROOT, "include", "tce_rvos_score.h")).read()
    for q in QUERIES:
        assert re.search(rf"{q}\([^;]*;\s*/\*[^*]*launches nothing", text), q


def test_access_models_on_hand_made_blocks(built_lib):
    from tce_rvos_amd import _lib, hazard
    l = _lib.lib()
    # P = 3, H = 5, W = 7, stride = 36: 35-byte planes from an odd address; every e_i and one segment sum per row in ws
    assert l.tce_rle_decode_ws_bytes(3, 5, 7, 36) == 448
    rd, wr = hazard.MODELS["tce_rle_decode_u8"]((0x100000, 0x200000, 0x300001, 0x400000, 3, 5, 7, 36, 0))
    assert hazard.union(*rd).tolist() == [[0x100000, 0x1001B0], [0x200000, 0x20000C], [0x400000, 0x4001C0]]
    assert hazard.union(*wr).tolist() == [[0x300001, 0x30006A], [0x400000, 0x4001C0]]
    # N = 3, H = 5, W = 7: pred and gt on odd addresses, one tile
    assert l.tce_mask_overlap_ws_bytes(3, 5, 7) == 32
    rd, wr = hazard.MODELS["tce_mask_overlap_i32"]((0x500001, 0x600003, 0x700000, 0x800000, 3, 5, 7, 0))
    assert hazard.union(*rd).tolist() == [[0x500001, 0x50006A], [0x600003, 0x600026], [0x800000, 0x800020]]
    assert hazard.union(*wr).tolist() == [[0x700000, 0x700024], [0x800000, 0x800020]]


class _StandIn:
    """Stands where the CDLL stands under a dry hazard._LibProxy: every entry answers with its own name."""

    def __getattr__(self, name):
        return lambda *a: name


def test_recording_proxy_records_the_launching_entries_and_passes_the_queries_through(built_lib):
    from tce_rvos_amd import hazard
    rec = hazard.Recorder()
    proxy = hazard._LibProxy(_StandIn(), rec, dry=True)
    assert proxy.tce_rle_decode_u8(0x100000, 0x200000, 0x300001, 0x400000, 3, 5, 7, 36, 0) == 0
    assert proxy.tce_mask_overlap_i32(0x500001, 0x600003, 0x700000, 0x800000, 3, 5, 7, 0) == 0
    assert [x.name for x in rec.launches] == list(LAUNCHING)
    assert rec.launches[0].reads.tolist() == [[0x100000, 0x1001B0], [0x200000, 0x20000C], [0x400000, 0x4001C0]]
    assert rec.launches[0].writes.tolist() == [[0x300001, 0x30006A], [0x400000, 0x4001C0]]
    assert rec.launches[1].reads.tolist() == [[0x500001, 0x50006A], [0x600003, 0x600026], [0x800000, 0x800020]]
    assert rec.launches[1].writes.tolist() == [[0x700000, 0x700024], [0x800000, 0x800020]]
    for q in QUERIES:  # passed through, not recorded
        assert getattr(proxy, q)(3, 5, 7, 36) == q
    assert len(rec.launches) == 2


def test_extents_are_rejected_before_anything_is_launched(built_lib):
    from tce_rvos_amd import _lib
    l = _lib.lib()
    assert l.tce_rle_decode_ws_bytes(1, 4, 6, 25) == (25 + 1) * 4 and l.tce_mask_overlap_ws_bytes(2, 4, 6) == (2 * 2 + 1) * 4 + 4
    assert l.tce_rle_decode_ws_bytes(3, 40, 30, 1201) % 8 == 0 and l.tce_rle_decode_ws_bytes(3, 40, 30, 1201) >= (3 * 1201 + 3 * 2) * 4
    for P, H, W, stride in ((0, 4, 6, 25), (65536, 4, 6, 25), (1, 0, 6, 25), (1, 4, 0, 25), (1, 4, 6, 0), (1, 1 << 16, 1 << 15, 25),
                            (1, 32768, 65536, 25), (-1, 4, 6, 25)):
        assert l.tce_rle_decode_ws_bytes(P, H, W, stride) < 0, (P, H, W, stride)
    for N, H, W in ((0, 4, 6), (65536, 4, 6), (1, 0, 6), (1, 4, 0), (1, 1 << 16, 1 << 15), (1, 32768, 65536)):
        assert l.tce_mask_overlap_ws_bytes(N, H, W) < 0, (N, H, W)
    assert l.tce_rle_decode_ws_bytes(65535, 4, 6, 25) > 0 and l.tce_mask_overlap_ws_bytes(65535, 4, 6) > 0
    # null pointers: rejected on the host with the entry's name (nothing is launched: there is no GPU here)
    assert l.tce_rle_decode_u8(None, None, None, None, 1, 4, 6, 25, None) != 0 and b"tce_rle_decode_u8" in l.tce_last_error()
    assert l.tce_mask_overlap_i32(None, None, None, None, 1, 4, 6, None) != 0 and b"tce_mask_overlap_i32" in l.tce_last_error()
    assert l.tce_rle_decode_u8(8, 8, 8, 8, 65536, 4, 6, 25, None) != 0 and b"tce_rle_decode_u8" in l.tce_last_error()
    assert l.tce_mask_overlap_i32(8, 8, 8, 8, 1, 1 << 16, 1 << 15, None) != 0 and b"tce_mask_overlap_i32" in l.tce_last_error()
    assert l.tce_rle_decode_u8(8, 8, 8, 12, 1, 4, 6, 25, None) != 0 and b"aligned" in l.tce_last_error()   # ws off its 8-byte boundary


# ----------------------------------------------------------------------------------------------------------- the strings
@pytest.mark.parametrize("counts", [[0, 1, 2 ** 20, 3, 2 ** 20 + 5, 1], [240 * 320], [0, 76800], [5], [0], [3, 1, 1, 1, 1, 2 ** 31 - 9],
                                    [31, 32, 33, 1, 2 ** 25, 7, 1, 2 ** 25, 40000, 2], list(range(1, 200))])
def test_rle_string_round_trip(counts):
    """the difference coding against counts[i-2] (i > 2) with negative differences, values of one to seven groups, a single run"""
    from tce_rvos_amd.a2d_score import rle_from_string
    from tce_rvos_amd.postprocess import rle_to_string
    s = rle_to_string(counts)
    assert s == _a2d.rle_string(counts)
    got = rle_from_string(s)
    assert got.dtype == np.int64 and got.tolist() == counts == _a2d.rle_from_string(s)
    assert rle_from_string(s.decode("ascii")).tolist() == counts
    assert rle_from_string(b"").tolist() == [] and rle_from_string("").tolist() == []


def test_rle_from_string_agrees_with_the_loop_on_the_fixture(cases):
    from tce_rvos_amd.a2d_score import rle_from_string
    n = 0
    for c in cases.values():
        for im in c["images"]:
            for s in [im["gt"]] + list(im["preds"]):
                assert rle_from_string(s).tolist() == _a2d.rle_from_string(s)
                n += 1
    assert n == 4 * 4 + 6 * 6 + 2
    with pytest.raises(ValueError):
        rle_from_string(b"\x10abc")      # a byte below '0'
    with pytest.raises(ValueError):
        rle_from_string(b"0P")           # ends inside a value


# ------------------------------------------------------------------------------------------------- precision@K and the IoUs
@pytest.mark.parametrize("name", ["hand", "random", "single"])
def test_precision_iou_metrics_equal_the_reference_function(cases, name):
    from tce_rvos_amd.a2d_score import precision_iou_metrics
    c = cases[name]
    precision, overall_iou, mean_iou = precision_iou_metrics(S.per_image_of(c["images"]))
    print(f"{name}: P@K {precision.tolist()} (reference {c['precision'].tolist()}), overall {overall_iou!r} ({c['overall_iou']!r}), "
          f"mean {mean_iou!r} ({c['mean_iou']!r})")
    assert precision.tolist() == c["precision"].tolist()
    assert abs(overall_iou - c["overall_iou"]) <= 1e-12 and abs(mean_iou - c["mean_iou"]) <= 1e-12


def test_the_fixture_holds_the_cases_the_metrics_can_go_wrong_on(cases):
    per = S.per_image_of(cases["hand"]["images"])
    assert [im["image_id"] for im in per] == [70, 3, 41, 8]                       # not ascending
    assert len({tuple(im["size"]) for im in cases["hand"]["images"]}) == 4       # different sizes per image
    tie = per[0]
    assert tie["scores"][0] == tie["scores"][1] == max(tie["scores"])
    i0, a0, g0 = tie["counts"][0]
    assert i0 == a0 == g0                                                          # the first of the tie equals the ground truth ...
    i, a, g = per[1]["counts"][int(np.argmax(per[1]["scores"]))]
    assert 0.6 < i / (a + g - i) < 0.7                                             # between two thresholds
    assert per[2]["counts"][int(np.argmax(per[2]["scores"]))][:2] == [0, 0]        # an empty prediction with the best score
    assert any(c[0] == c[1] == c[2] for c in per[3]["counts"])


def test_a_tie_picks_the_last_maximum():
    """sorted(key=score)[-1] is a stable ascending sort: of equal best scores the LAST in input order"""
    from tce_rvos_amd.a2d_score import precision_iou_metrics
    im = {"image_id": 1, "scores": [0.9, 0.2, 0.9, 0.1], "counts": [[100, 100, 100], [0, 0, 100], [60, 100, 100], [100, 100, 100]]}
    precision, overall_iou, mean_iou = precision_iou_metrics([im])
    want = float((np.float32(60) + np.float32(1e-6)) / (np.float32(140) + np.float32(1e-6)))
    assert mean_iou == want and overall_iou == 60 / 140 and precision.tolist() == [0, 0, 0, 0, 0]
    # `iou > k` is strict: 50 / 100 in float32 with the epsilons is exactly 0.5
    half = {"image_id": 2, "scores": [1.0], "counts": [[50, 50, 100]]}
    assert float((np.float32(50) + np.float32(1e-6)) / (np.float32(100) + np.float32(1e-6))) == 0.5
    assert precision_iou_metrics([half])[0].tolist() == [0, 0, 0, 0, 0]


# -------------------------------------------------------------------------------------------------------------------- AP
def _random_count_set(rng):
    ims = []
    for k in range(int(rng.integers(1, 7))):
        n = int(rng.integers(1, 7))
        g = int(rng.integers(1, 30000))
        a = rng.integers(0, 30000, n)
        i = np.array([rng.integers(0, min(int(x), g) + 1) for x in a])
        if rng.random() < 0.3:
            i[0], a[0] = g, g                                                       # IoU exactly 1
        scores = np.round(rng.random(n), 1)                                         # one decimal: ties within and across images
        area = [None, float(rng.integers(1, 20000))][int(rng.random() < 0.5)]
        ims.append({"image_id": int(rng.integers(0, 1000)) * 10 + k, "scores": scores.tolist(),
                    "counts": np.stack([i, a, np.full(n, g)], 1).tolist(), "area": area})
    return ims


def test_coco_mask_ap_equals_the_plain_loops(cases):
    from tce_rvos_amd.a2d_score import coco_mask_ap
    sets = [(name, S.per_image_of(c["images"])) for name, c in cases.items()]
    rng = np.random.default_rng(77)
    sets += [(f"random {k}", _random_count_set(rng)) for k in range(20)]
    seen_minus_one, seen_positive = False, False
    for name, per in sets:
        got, want = coco_mask_ap(per), S.coco_mask_ap_loops(per)
        d = float(np.abs(got - np.asarray(want)).max())
        print(f"{name}: {np.round(got, 6).tolist()} max |diff| {d:.2e}")
        assert d <= 1e-12, (name, got.tolist(), want)
        seen_minus_one |= bool((got == -1).any())
        seen_positive |= bool((got[3:] > 0).any())
    assert seen_minus_one and seen_positive


def test_coco_mask_ap_more_than_100_detections_keeps_the_best_100():
    from tce_rvos_amd.a2d_score import coco_mask_ap
    rng = np.random.default_rng(5)
    n = 130
    scores = rng.permutation(n) / n
    counts = [[50, 100, 100]] * n
    best = int(np.argsort(-scores)[100])          # the 101st by score: the only good mask, cut off
    counts[best] = [100, 100, 100]
    per = [{"image_id": 1, "scores": scores.tolist(), "counts": counts, "area": None}]
    got = coco_mask_ap(per)
    assert np.abs(got - np.asarray(S.coco_mask_ap_loops(per))).max() <= 1e-12 and got[0] == 0.0


def test_ap_by_hand_all_perfect():
    """three images, one detection each, every IoU >= 0.95: tp = 1, 2, 3 and fp = 0 at every threshold, so every sample of the
    precision curve is 1 / (1 + spacing(1) / tp)"""
    from tce_rvos_amd.a2d_score import coco_mask_ap
    per = [{"image_id": k, "scores": [0.3 + 0.1 * k], "counts": [[i, a, 20000]]} for k, (i, a) in enumerate(((20000, 20000), (19500, 19600), (19900, 20700)))]
    assert min(i / (a + 20000 - i) for i, a in ((20000, 20000), (19500, 19600), (19900, 20700))) >= 0.95
    got = coco_mask_ap(per)
    assert np.abs(got[:3] - 1.0).max() <= 1e-9, got
    assert got[3] == -1 and got[4] == -1 and abs(got[5] - 1.0) <= 1e-9      # 20000 pixels: large


def test_ap_and_precision_by_hand_three_images():
    """g = 100; (I, a) = (84, 100) score .9, (57, 100) score .8, (98, 99) score .7: IoUs 0.724, 0.399, 0.970.
    At t = 0.5 (and up to 0.7): tp, fp, tp by descending score: precision 1, 1/2, 2/3 -> 1, 2/3, 2/3 from the right; recall 1/3,
    1/3, 2/3: the 34 recall samples 0 .. 0.33 take 1, the 33 samples 0.34 .. 0.66 take 2/3, the rest 0: AP = 56/101.
    At t = 0.75 .. 0.95: fp, fp, tp: precision 1/3 at recall 1/3, the 34 samples: 34/303.  mAP = (5 * 56/101 + 5 * 34/303) / 10 = 1/3."""
    from tce_rvos_amd.a2d_score import coco_mask_ap, precision_iou_metrics
    per = [{"image_id": k, "scores": [s], "counts": [[i, a, 100]], "area": 100.0}
           for k, (i, a, s) in enumerate(((84, 100, 0.9), (57, 100, 0.8), (98, 99, 0.7)))]
    got = coco_mask_ap(per)
    print(got.tolist())
    assert abs(got[1] - 56 / 101) <= 1e-9 and abs(got[2] - 34 / 303) <= 1e-9 and abs(got[0] - 1 / 3) <= 1e-9
    assert abs(got[3] - 1 / 3) <= 1e-9 and got[4] == -1 and got[5] == -1        # areas of 100: small; no medium or large ground truth
    assert precision_iou_metrics(per)[0].tolist() == [2 / 3, 2 / 3, 2 / 3, 1 / 3, 1 / 3]


# ----------------------------------------------------------------------------------------------- the scorer's host side
def _state(images, pick=None):
    per = S.per_image_of(images)
    per = per if pick is None else [per[k] for k in pick]
    return {"image_ids": [im["image_id"] for im in per], "scores": [im["scores"] for im in per], "counts": [im["counts"] for im in per]}


def test_merge_keeps_identical_repeats_once_and_is_independent_of_order(cases):
    from tce_rvos_amd.a2d_score import A2DScorer, coco_mask_ap, precision_iou_metrics
    images = cases["random"]["images"]
    whole = _state(images)
    parts = [_state(images, [0, 3, 4]), _state(images, [4, 1]), _state(images, [2, 5, 0])]      # 4 and 0 repeat, identical
    sums = []
    for order in ([0, 1, 2], [2, 1, 0], [1, 2, 0]):
        sc = A2DScorer(S.gt_dict(images))
        merged = sc.merge(pickle.loads(pickle.dumps([parts[k] for k in order])))               # plain Python: picklable
        assert merged["image_ids"] == whole["image_ids"] and merged["scores"] == whole["scores"] and merged["counts"] == whole["counts"]
        sums.append(sc.summarize())
    assert sums[0] == sums[1] == sums[2]
    res, per = sums[0], S.per_image_of(images)
    assert list(res) == list(AP_KEYS) + [f"P@{k}" for k in S.P_AT] + ["overall_iou", "mean_iou"]
    assert [res[k] for k in AP_KEYS] == coco_mask_ap(per).tolist()
    precision, overall_iou, mean_iou = precision_iou_metrics(per)
    assert [res[f"P@{k}"] for k in S.P_AT] == precision.tolist() and res["overall_iou"] == overall_iou and res["mean_iou"] == mean_iou
    assert [res[f"P@{k}"] for k in S.P_AT] == cases["random"]["precision"].tolist()
    bad = _state(images, [4])
    bad["counts"][0][2][0] += 1
    with pytest.raises(ValueError, match="different results"):
        A2DScorer(S.gt_dict(images)).merge(parts + [bad])
    bad = _state(images, [4])
    bad["scores"][0][1] += 1e-9
    with pytest.raises(ValueError, match="different results"):
        A2DScorer(S.gt_dict(images)).merge([bad] + parts)
    with pytest.raises(ValueError, match="unknown image_id"):
        A2DScorer(S.gt_dict(images[:3])).merge(parts)


def test_error_paths(cases, tmp_path):
    import json
    from tce_rvos_amd.a2d_score import A2DScorer
    images = cases["hand"]["images"]
    sc = A2DScorer(S.gt_dict(images))
    sc.merge([_state(images, [0, 1, 2])])
    with pytest.raises(ValueError, match="no predictions"):
        sc.summarize()
    with pytest.raises(ValueError, match="no predictions"):
        A2DScorer(S.gt_dict(images)).summarize()                       # nothing collected at all (no GPU is touched for that)
    one = {"size": [3, 5], "counts": images[0]["gt"]}
    with pytest.raises(ValueError, match="crowd"):
        A2DScorer({1: dict(one, iscrowd=1)})
    with pytest.raises(ValueError, match="2 annotations"):
        A2DScorer({1: [one, one]})
    with pytest.raises(ValueError, match="0 annotations"):
        A2DScorer({1: []})
    with pytest.raises(ValueError, match="run-length"):
        A2DScorer({1: {"segmentation": [[1.0, 2.0, 3.0, 4.0, 5.0, 6.0]]}})
    # the reference's ground-truth file: strings under 'segmentation', areas, image order of 'images'
    data = {"images": [{"id": im["image_id"]} for im in images], "categories": [{"id": 1}],
            "annotations": [{"id": k, "image_id": im["image_id"], "category_id": 1, "iscrowd": 0, "area": 77.0,
                             "segmentation": {"size": im["size"], "counts": im["gt"].decode("ascii")}} for k, im in enumerate(images)]}
    path = tmp_path / "gt.json"
    path.write_text(json.dumps(data))
    sc = A2DScorer.from_coco_json(str(path))
    assert list(sc.gt) == [70, 3, 41, 8] and sc.gt[3][:2] == (9, 9) and sc.gt[3][3] == 77.0
    sc.merge([_state(images)])
    assert [sc.summarize()[f"P@{k}"] for k in S.P_AT] == cases["hand"]["precision"].tolist()
    data["annotations"].append(dict(data["annotations"][0], id=99))
    path.write_text(json.dumps(data))
    with pytest.raises(ValueError, match="2 annotations"):
        A2DScorer.from_coco_json(str(path))
    data["annotations"] = data["annotations"][1:-1]
    path.write_text(json.dumps(data))
    with pytest.raises(ValueError, match="0 annotations"):
        A2DScorer.from_coco_json(str(path))


def test_postprocess_rle_flag_is_an_attribute_and_defaults_to_true():
    from tce_rvos_amd.postprocess import A2DSentencesPostProcess, build_postprocessors
    import argparse
    assert A2DSentencesPostProcess().rle is True and A2DSentencesPostProcess(0.5, rle=False).rle is False
    assert build_postprocessors(argparse.Namespace(), "a2d").rle is True
