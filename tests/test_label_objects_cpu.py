"""Ref-DAVIS label maps, the parts that need no GPU (the driver-stage header against its binding table, the exported symbols and
the access models: tests/test_host_cpu.py, with every other header): the access model of tce_label_objects_u8 on a hand-made
argument block; the annotator sets and the forward plan of run_video_objects; the committed fixture's contested-share cap; the
argument checks of ops.label_objects."""
import os

import numpy as np
import pytest
import torch

import _davis
from tce_rvos_amd import _lib, hazard, video

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "davis_label_cases.npz")


def _table(ptrs):
    t = (_lib.LabelObj * len(ptrs))()
    for o, (lg, pm) in zip(t, ptrs):
        o.logits, o.masks = lg, pm
    return t


def test_label_objects_access_model_on_a_hand_made_block():
    n, T, Q, K, h, w, H0, W0 = 3, 4, 5, 2, 6, 7, 25, 31
    ptrs = [(0x100000 * (k + 1), 0x100000 * (k + 1) + 0x40000) for k in (2, 0, 1)]  # table order != address order
    labels, best = 0x900003, 0xA00000  # labels on an odd address
    rd, wr = hazard.MODELS["tce_label_objects_u8"]((_table(ptrs), n, labels, best, T, Q, K, h, w, H0, W0, 0.5, 0.1, 0))
    want_rd = sorted([[lg, lg + T * Q * K * 4] for lg, _ in ptrs] + [[pm, pm + T * Q * h * w * 4] for _, pm in ptrs])
    assert hazard.union(*rd).tolist() == want_rd
    assert hazard.union(*wr).tolist() == [[labels, labels + T * H0 * W0], [best, best + 4 * n]]
    assert len(rd) == 2 * n
    # n = 1: one logits and one masks block, 4 bytes of best_query
    rd, wr = hazard.MODELS["tce_label_objects_u8"]((_table(ptrs[:1]), 1, labels, best, T, Q, K, h, w, H0, W0, 0.5, 0.1, 0))
    assert len(rd) == 2 and hazard.union(*wr).tolist() == [[labels, labels + T * H0 * W0], [best, best + 4]]


def test_recording_proxy_consults_the_video_models_after_the_main_table():
    class Real:
        def __getattr__(self, name):
            return lambda *a: 0
    rec = hazard.Recorder()
    proxy = hazard._LibProxy(Real(), rec, dry=True)
    proxy.tce_label_objects_u8(_table([(0x1000, 0x2000)]), 1, 0x9000, 0xA000, 1, 2, 1, 3, 3, 6, 6, 0.5, 0.1, 0)
    assert [x.name for x in rec.launches] == ["tce_label_objects_u8"]
    assert rec.launches[0].writes.tolist() == [[0x9000, 0x9000 + 36], [0xA000, 0xA004]]
    with pytest.raises(RuntimeError):
        proxy.tce_not_modelled_anywhere


def test_davis_annotator_sets():
    assert video.davis_annotator_sets(12) == [[0, 4, 8], [1, 5, 9], [2, 6, 10], [3, 7, 11]]
    assert video.davis_annotator_sets(4) == [[0], [1], [2], [3]]
    num_expressions = 20  # inference_davis.py:185-194
    num_obj = num_expressions // 4
    ref = [[obj_id * 4 + anno_id for obj_id in range(num_obj)] for anno_id in range(4)]
    assert video.davis_annotator_sets(num_expressions) == ref
    assert sorted(i for s in ref for i in s) == list(range(num_expressions))


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("sets", [[[0, 1, 2, 3], [2, 0], [1]], None, [[3, 1], [1, 3], [1]]])
def test_forward_plan_runs_each_caption_once_per_chunk(mixed, sets):
    lens = [5, 7, 5, 7]
    got_sets, plan = video.plan_object_forwards(lens, 7, 4, sets, max_group=4, mixed_lengths=mixed)
    assert got_sets == ([[0, 1, 2, 3]] if sets is None else sets)
    used = sorted({i for s in got_sets for i in s})
    chunks = [(0, 4), (4, 7)]  # a shorter last chunk
    assert [(lo, hi) for lo, hi, _ in plan] == sorted((lo, hi) for lo, hi, _ in plan), "the chunk loop is the outer loop"
    for lo, hi in chunks:
        ran = [i for plo, phi, g in plan if (plo, phi) == (lo, hi) for i in g]
        assert sorted(ran) == used and len(ran) == len(set(ran)), (lo, hi, ran)
    assert {(lo, hi) for lo, hi, _ in plan} == set(chunks)
    for _, _, g in plan:
        assert 1 <= len(g) <= 4
        if not mixed:
            assert len({lens[i] for i in g}) == 1, "bucketed groups hold one token length"
    if sets is not None and sets[0] == [0, 1, 2, 3]:  # the groups are run_video_expressions' own
        assert [g for lo, _, g in plan if lo == 0] == video.plan_expression_groups(lens, 4, mixed)
    # whole video as one clip
    assert [(lo, hi) for lo, hi, _ in video.plan_object_forwards(lens, 7, None, sets, 4, mixed)[1]][0] == (0, 7)


def test_forward_plan_rejects_bad_sets():
    for bad in ([[0, 0]], [[4]], [[]], [list(range(17))], [[-1]]):
        with pytest.raises(ValueError):
            video.plan_object_forwards([5] * 17 if len(bad[0]) == 17 else [5, 5, 5, 5], 8, 4, bad)
    with pytest.raises(ValueError):
        video.plan_object_forwards([5] * 18, 8, 4, None)  # the default set would hold 18 objects


def test_fixture_contested_share_is_capped_and_ties_are_not_contested():
    assert os.path.getsize(FIXTURE) < 1_000_000
    cases = _davis.load_cases(FIXTURE)
    assert [c["name"] for c in cases] == [c[0] for c in _davis.CASES] == ["A", "B", "D", "E"]
    for c, (name, seed, n, T, Q, hw, size, scale) in zip(cases, _davis.CASES):
        share = float(c["contested"].float().mean())
        print(f"case {name}: contested share {share:.3e}")
        assert share <= _davis.MAX_SHARE, (name, share)
        assert tuple(c["labels"].shape) == (T,) + tuple(size) == tuple(c["contested"].shape) and c["size"] == tuple(size)
        assert int(c["labels"].max()) <= n == c["n"] and tuple(c["best"].shape) == (n,)
        logits, masks = _davis.make_inputs(name, seed, n, T, Q, hw, scale)
        assert torch.equal(logits, c["logits"]) and torch.equal(masks, c["masks"]), "the fixture holds the case table's inputs"
        # the restatement run again here: same query choice, same labels wherever neither run calls the pixel contested
        labels, best, contested = _davis.reference_labels(list(logits), list(masks), size)
        assert torch.equal(best, c["best"])
        assert not bool(((labels != c["labels"]) & ~(contested | c["contested"])).any())
        assert float(contested.float().mean()) <= _davis.MAX_SHARE
    # case D: the saturated ties (both blocks' objects at exactly 1.0f) are NOT contested and go to the lower index
    d = cases[2]
    import torch.nn.functional as F
    T = d["masks"].shape[1]
    v = [F.interpolate(d["masks"][k][range(T), int(d["best"][k])][None], size=d["size"], mode="bilinear", align_corners=False)[0] for k in (0, 1)]
    tie = (v[0] >= _davis.V_SAT) & (v[1] >= _davis.V_SAT)
    print(f"case D: {int(tie.sum())} saturated ties of {tie.numel()} pixels, {int((tie & d['contested']).sum())} of them contested")
    assert float(tie.float().mean()) > 0.05
    assert not bool((tie & d["contested"]).any())
    assert bool((d["labels"][tie] == 1).all())
    # ... and a comparison of LOGITS instead of scores is wrong on many of them (object 1's block is the larger logit)
    assert int(((v[1] > v[0]) & tie).sum()) > 1000


def test_label_objects_argument_checks_need_no_device():
    from tce_rvos_amd import ops
    lg, pm = torch.zeros(2, 3, 1), torch.zeros(2, 3, 4, 5)
    with pytest.raises(ValueError, match="1..16 objects"):
        ops.label_objects([lg] * 17, [pm] * 17, (8, 10))
    with pytest.raises(ValueError, match="1..16 objects"):
        ops.label_objects([], [], (8, 10))
    with pytest.raises(ValueError):
        ops.label_objects([lg, lg], [pm], (8, 10))
    with pytest.raises(ValueError, match="object 1"):
        ops.label_objects([lg, lg], [pm, torch.zeros(2, 3, 4, 6)], (8, 10))
    with pytest.raises(ValueError, match="object 1"):
        ops.label_objects([lg, torch.zeros(2, 4, 1)], [pm, pm], (8, 10))
    with pytest.raises(ValueError, match="on the GPU"):
        ops.label_objects([lg], [pm], (8, 10))  # CPU tensors
    with pytest.raises(ValueError, match="on the GPU"):
        ops.label_objects(torch.zeros(2, 2, 3, 1), torch.zeros(2, 2, 3, 4, 5), (8, 10))  # stacked, CPU
    with pytest.raises(ValueError):
        ops.label_objects([lg], [pm.transpose(2, 3)], (8, 10))  # shape of a transposed view differs; non-contiguous below
    with pytest.raises(ValueError, match="contiguous"):
        ops.label_objects([lg], [torch.zeros(2, 3, 5, 4).transpose(2, 3)], (8, 10))
    with pytest.raises(ValueError):
        ops.label_objects([lg.double()], [pm.double()], (8, 10))
