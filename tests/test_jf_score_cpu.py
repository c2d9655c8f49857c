"""Ref-DAVIS J&F scoring, the parts that need no GPU (the scoring-stage header against its binding table, the exported symbols and
the access model: tests/test_host_cpu.py, with every other header): the header's limits and host-side rejections on fake
pointers; the access model on a hand-made block; score.boundary_radius, jf_from_counts (hand-made counts and the committed fixture, bit for bit), db_statistics, summarize; the argument checks of
ops.jf_counts."""
import os
import warnings

import numpy as np
import pytest
import torch

import _jf
from tce_rvos_amd import _lib, hazard, score

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "jf_cases.npz")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def test_jf_ws_bytes_and_host_side_rejections_need_no_device():
    l = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "tce_rvos_score.h")).read()
    for define in ("#define TCE_JF_MAX_OBJS   16", "#define TCE_JF_MAX_RADIUS 40", "#define TCE_JF_COUNTS     6"):
        assert define in hdr, define
    # one partial sum of six words per (object, frame, 32 x 64 tile)
    assert l.tce_jf_ws_bytes(1, 1, 1, 1, 0) == 24 and l.tce_jf_ws_bytes(3, 2, 7, 9, 1) == 3 * 2 * 24
    assert l.tce_jf_ws_bytes(2, 3, 33, 65, 2) == 2 * 3 * 2 * 2 * 24 and l.tce_jf_ws_bytes(32, 3, 480, 854, 8) == 32 * 3 * 15 * 14 * 24
    assert l.tce_jf_ws_bytes(2, 3, 480, 854, 8) % 8 == 0
    for bad in ((0, 1, 4, 4, 1), (1, 1, 0, 4, 1), (1, 1, 4, -1, 1), (1, 0, 4, 4, 1), (1, 17, 4, 4, 1), (1, 1, 4, 4, -1), (1, 1, 4, 4, 41),
                (2, 1, 1 << 15, 1 << 15, 1), (1 << 11, 1, 1 << 10, 1 << 10, 1)):
        assert l.tce_jf_ws_bytes(*bad) < 0, bad
    assert l.tce_jf_ws_bytes(1, 16, 4, 4, 40) > 0 and l.tce_jf_ws_bytes((1 << 11) - 1, 1, 1 << 10, 1 << 10, 1) > 0
    # every rejection happens before anything is launched: the pointers are fake
    P, G, C, WS = 0x1001, 0x2003, 0x3000, 0x4000
    ok = (1, 1, 4, 4, 1)
    for args, word in (((None, G, C, WS) + ok, b"null"), ((P, None, C, WS) + ok, b"null"), ((P, G, None, WS) + ok, b"null"),
                       ((P, G, C, None) + ok, b"null"),
                       ((P, G, C, WS, 1, 0, 4, 4, 1), b"objects"), ((P, G, C, WS, 1, 17, 4, 4, 1), b"objects"),
                       ((P, G, C, WS, 1, 1, 4, 4, -1), b"radius"), ((P, G, C, WS, 1, 1, 4, 4, 41), b"radius"),
                       ((P, G, C, WS, 0, 1, 4, 4, 1), b"extent"), ((P, G, C, WS, 1, 1, 0, 4, 1), b"extent"), ((P, G, C, WS, 1, 1, 4, 0, 1), b"extent"),
                       ((P, G, C, WS, 2, 1, 1 << 15, 1 << 15, 1), b"2^31"), ((P, G, C, WS, 1 << 11, 1, 1 << 10, 1 << 10, 1), b"2^31"),
                       ((P, G, C, WS + 4) + ok, b"aligned"), ((P, G, C + 2, WS) + ok, b"aligned")):
        assert l.tce_jf_counts_i32(*args, None) < 0, args
        assert b"tce_jf_counts_i32" in l.tce_last_error() and word in l.tce_last_error(), (args, l.tce_last_error())


def test_access_model_on_a_hand_made_block():
    T, n, H, W, radius = 5, 3, 87, 145, 2
    pred, gt, counts, ws = 0x100001, 0x200003, 0x400000, 0x800000  # the label planes on odd addresses
    wsb = _lib.lib().tce_jf_ws_bytes(T, n, H, W, radius)
    assert wsb == T * n * 3 * 3 * 24
    rd, wr = hazard.MODELS["tce_jf_counts_i32"]((pred, gt, counts, ws, T, n, H, W, radius, 0))
    assert hazard.union(*rd).tolist() == [[pred, pred + T * H * W], [gt, gt + T * H * W], [ws, ws + wsb]]
    assert hazard.union(*wr).tolist() == [[counts, counts + n * T * 6 * 4], [ws, ws + wsb]]


def test_recording_proxy_consults_the_score_models_after_the_eval_models():
    class Real:
        def __getattr__(self, name):
            return lambda *a: 0
    rec = hazard.Recorder()
    proxy = hazard._LibProxy(Real(), rec, dry=True)
    proxy.tce_jf_counts_i32(0x1001, 0x2003, 0x3000, 0x4000, 1, 1, 4, 4, 1, 0)
    proxy.tce_a2d_masks_u8(0x10000, 0x9003, 2, 3, 3, 12, 12, 5, 7, 0.5, 0)
    assert [x.name for x in rec.launches] == ["tce_jf_counts_i32", "tce_a2d_masks_u8"]
    assert rec.launches[0].reads.tolist() == [[0x1001, 0x1011], [0x2003, 0x2013], [0x4000, 0x4018]]
    assert rec.launches[0].writes.tolist() == [[0x3000, 0x3018], [0x4000, 0x4018]]
    assert proxy.tce_jf_ws_bytes(1, 1, 4, 4, 1) == 0 and len(rec.launches) == 2  # a query: passed through, not recorded


def test_boundary_radius():
    assert score.boundary_radius(480, 854) == 8
    assert score.boundary_radius(480, 910) == 9
    assert score.boundary_radius(1080, 1920) == 18
    assert score.boundary_radius(40, 56) == 1
    assert score.boundary_radius(2160, 3840) == 36  # TCE_JF_MAX_RADIUS covers it
    assert score.boundary_radius(480, 854, bound_th=3) == 3
    for hw in ((480, 854), (33, 65), (7, 9)):  # the reference's own expression (metrics.py:77-78)
        assert score.boundary_radius(*hw) == np.ceil(0.008 * np.linalg.norm(np.zeros(hw).shape))
        assert isinstance(score.boundary_radius(*hw), int)


def test_jf_from_counts_empty_and_non_empty_boundaries_and_empty_union():
    # inters, union, n_fg, n_gt, fg_match, gt_match
    c = np.array([[[30, 40, 10, 8, 7, 4],      # both boundaries non-empty
                   [0, 12, 0, 9, 0, 0],        # no predicted boundary: precision 1, recall 0
                   [0, 15, 11, 0, 0, 0],       # no annotated boundary: precision 0, recall 1
                   [0, 0, 0, 0, 0, 0],         # neither, and an empty union: J = 1, F = 1
                   [5, 9, 6, 6, 0, 0],         # both non-empty, nothing matches: P + R = 0 -> F = 0
                   [3, 7, 1, 3, 1, 1]]], dtype=np.int32)
    J, F = score.jf_from_counts(c)
    assert J.dtype == np.float64 and F.dtype == np.float64 and J.shape == (1, 6) and F.shape == (1, 6)
    p, r = 7 / float(10), 4 / float(8)
    p5, r5 = 1 / float(1), 1 / float(3)
    want_j = [30 / 40, 0 / 12, 0 / 15, 1.0, 5 / 9, 3 / 7]
    want_f = [2 * p * r / (p + r), 0.0, 0.0, 1.0, 0.0, 2 * p5 * r5 / (p5 + r5)]
    assert _bits(J[0]).tolist() == _bits(want_j).tolist()
    assert _bits(F[0]).tolist() == _bits(want_f).tolist()
    Jt, Ft = score.jf_from_counts(torch.from_numpy(c))  # a tensor goes in as well
    assert np.array_equal(_bits(Jt), _bits(J)) and np.array_equal(_bits(Ft), _bits(F))
    with pytest.raises(ValueError):
        score.jf_from_counts(np.zeros((3, 5)))


def test_jf_from_counts_is_bit_equal_to_the_fixture():
    assert os.path.getsize(FIXTURE) < 1_000_000
    cases = _jf.load_cases(FIXTURE)
    assert list(cases) == [c[0] for c in _jf.CASES] == ["A", "B", "C", "D", "E", "F", "G"]
    for case in _jf.CASES:
        name, seed, T, n, H, W, radius, kind = case
        c = cases[name]
        assert c["n"] == n and c["radius"] == radius and c["pred"].shape == (T, H, W) == c["gt"].shape and c["counts"].shape == (n, T, 6)
        pred, gt = _jf.make_case(case)  # the makers still make the committed maps
        assert np.array_equal(pred, c["pred"]) and np.array_equal(gt, c["gt"]), name
        J, F = score.jf_from_counts(c["counts"])
        assert np.array_equal(_bits(J), _bits(c["J"])) and np.array_equal(_bits(F), _bits(c["F"])), name
    # the restatement run again on the small cases: the fixture is what it computes
    for name in ("A", "C", "D", "E"):
        c = cases[name]
        counts, J, F = _jf.reference(c["pred"], c["gt"], c["n"], c["radius"])
        assert np.array_equal(counts, c["counts"]) and np.array_equal(_bits(J), _bits(c["J"])) and np.array_equal(_bits(F), _bits(c["F"]))
    # what the cases are there for
    assert (cases["C"]["gt"] == 255).any() and (cases["C"]["pred"] == 3).any() and cases["C"]["gt"][:, -1, -1].all()
    d = cases["D"]["counts"][0, 0]
    assert d.tolist() == [0, 36, 72, 72, 15, 15]  # 18 pixel pairs, 2x2 boundary blocks; (6,0) and (0,-6): 2 matches, (4,5): 1, the rest 0
    e = cases["E"]["counts"]
    assert not e[:, 0, 2].any() and e[:, 0, 3].all() and e[:, 1, 2].all() and not e[:, 1, 3].any() and not e[:, 2].any()
    assert np.array_equal(e[:, 3, 0], e[:, 3, 1]) and np.array_equal(e[:, 3, 2], e[:, 3, 4]) and np.array_equal(e[:, 3, 3], e[:, 3, 5])
    assert cases["E"]["J"][:, 2].tolist() == [1.0, 1.0] and cases["E"]["F"][:, 2].tolist() == [1.0, 1.0]
    assert cases["E"]["F"][:, 0].tolist() == [0.0, 0.0] and cases["E"]["J"][:, 3].tolist() == [1.0, 1.0]


def test_seg2bmap_last_row_last_column_and_corner_rules():
    """The three rules of the header on a plane that is set everywhere: only the inner boundary towards nothing would show, and the
    reference shows none of it (reads beyond the plane are never made: the last row and column use their own rule)."""
    assert not _jf.seg2bmap(np.ones((5, 7), dtype=bool)).any()
    m = np.zeros((5, 7), dtype=bool)
    m[4, 2:5] = True  # a run in the last row: b = s ^ s[y, x+1] there, and the row above sees it below and below-right
    b = _jf.seg2bmap(m)
    assert b[4].tolist() == [False, True, False, False, True, False, False]
    assert b[3].tolist() == [False, True, True, True, True, False, False]
    m = np.zeros((5, 7), dtype=bool)
    m[4, 6] = True  # the corner pixel itself
    b = _jf.seg2bmap(m)
    assert not b[4, 6] and b[4, 5] and b[3, 6] and b[3, 5] and int(b.sum()) == 3


def test_db_statistics_on_a_hand_computed_vector_with_a_nan():
    v = np.array([0.9, 0.8, np.nan, 0.6, 0.55, 0.5, 0.4, 0.7, 0.2, 0.1])
    M, O, D = score.db_statistics(v)
    # linspace(1, 10, 5) = [1, 3.25, 5.5, 7.75, 10]; + 1e-10 and rounded: [1, 3, 6, 8, 10]; - 1: the bin edges
    ids = (np.round(np.linspace(1, 10, 5) + 1e-10) - 1).astype(np.uint8)
    assert ids.tolist() == [0, 2, 5, 7, 9]
    assert M == np.nanmean(v) and abs(M - (0.9 + 0.8 + 0.6 + 0.55 + 0.5 + 0.4 + 0.7 + 0.2 + 0.1) / 9) < 1e-15
    assert O == 5 / 10  # NaN > 0.5 is False and still counts as a frame: 0.9, 0.8, 0.6, 0.55, 0.7 of ten
    first, last = (0.9 + 0.8) / 2, (0.7 + 0.2 + 0.1) / 3  # bins [0:3] (the NaN dropped) and [7:10]
    assert abs(D - (first - last)) < 1e-15 and D == np.nanmean(v[0:3]) - np.nanmean(v[7:10])
    # beyond 256 frames the reference's uint8 edges wrap; this restates that
    w = np.linspace(1.0, 0.0, 300)
    ids = (np.round(np.linspace(1, 300, 5) + 1e-10) - 1).astype(np.int64) % 256
    assert ids.tolist() == [0, 75, 150, 224, 43]  # the last bin, [224:44], is empty
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        want = np.nanmean(w[ids[0]:ids[1] + 1]) - np.nanmean(w[ids[3]:ids[4] + 1])
    got = score.db_statistics(w)[2]
    assert got == want or (np.isnan(got) and np.isnan(want))
    assert score.db_statistics(np.array([0.7]))[0] == 0.7


def test_summarize_on_two_small_results():
    a = {"JM": np.array([0.5, 0.7]), "JR": np.array([1.0, 0.5]), "JD": np.array([0.1, -0.1]),
         "FM": np.array([0.4, 0.6]), "FR": np.array([0.5, 0.5]), "FD": np.array([0.0, 0.2])}
    b = {"JM": np.array([0.9]), "JR": np.array([1.0]), "JD": np.array([0.3]), "FM": np.array([0.8]), "FR": np.array([1.0]), "FD": np.array([0.1])}
    s = score.summarize([a, b])
    assert tuple(s) == ("J&F-Mean", "J-Mean", "J-Recall", "J-Decay", "F-Mean", "F-Recall", "F-Decay")
    jm, fm = np.mean([0.5, 0.7, 0.9]), np.mean([0.4, 0.6, 0.8])
    assert s["J-Mean"] == jm and s["F-Mean"] == fm and s["J&F-Mean"] == (jm + fm) / 2.
    assert s["J-Recall"] == np.mean([1.0, 0.5, 1.0]) and s["J-Decay"] == np.mean([0.1, -0.1, 0.3])
    assert s["F-Recall"] == np.mean([0.5, 0.5, 1.0]) and s["F-Decay"] == np.mean([0.0, 0.2, 0.1])
    assert score.summarize(b) == score.summarize([b])
    with pytest.raises(ValueError):
        score.summarize([])


def test_argument_checks_need_no_device():
    from tce_rvos_amd import ops
    u8 = torch.zeros(2, 4, 5, dtype=torch.uint8)
    with pytest.raises(ValueError, match="on the GPU"):
        ops.jf_counts(u8, u8, 1, 1)  # CPU tensors
    with pytest.raises(ValueError, match="contiguous"):
        ops.jf_counts(torch.zeros(2, 5, 4, dtype=torch.uint8).transpose(1, 2), u8, 1, 1)
    with pytest.raises(ValueError, match="uint8"):
        ops.jf_counts(u8.float(), u8, 1, 1)
    with pytest.raises(ValueError, match="uint8"):
        ops.jf_counts(u8, u8.int(), 1, 1)
    with pytest.raises(ValueError):
        ops.jf_counts(u8[0], u8[0], 1, 1)
    with pytest.raises(ValueError):
        ops.jf_counts(u8.numpy(), u8, 1, 1)
    with pytest.raises(ValueError):
        score.score_video(u8.float(), u8)
    with pytest.raises(ValueError, match="shape"):
        score.score_video(u8, torch.zeros(2, 4, 6, dtype=torch.uint8))
    with pytest.raises(ValueError, match="no frame"):
        score.score_video(u8, u8, n=1)  # two frames, first and last dropped
