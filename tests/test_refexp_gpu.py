"""GPU: the RefCOCO evaluation stage (include/tce_rvos_refexp.h, ops.refexp_group / ops.refexp_giou, postprocess.PostProcess /
PostProcessSegm, refexp_score.RefExpScorer, refexp.run_images) against the reference's own classes (tests/golden/refexp_cases.npz),
the per-sample masks entry, the tie rule, the candidate cap, a group larger than a launch table, the access models
(tests/_footprint.py) and, end to end, the one-image path.

Bounds.  scores: 1e-6, what tests/test_a2d_post_gpu.py holds this sigmoid to.  boxes: equal bits.  order: equal (the fixture's
neighbouring scores differ by more than 4e-6).  masks: the rule of tests/_a2d.py.  giou: 2e-6 absolute -- about ten fp32 roundings
on quantities no larger than their denominators, result in [-2, 1]: under 1.3e-6.  End to end the group bound of
tests/test_single_frame_groups_gpu.py on the forward's outputs, carried through the stage (see _e2e_bounds)."""
import os

import numpy as np
import pytest
import torch

import _a2d
import _footprint as fp
import _refexp as R
from _util import synth_frames
from tce_rvos_amd import _lib, hazard

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refexp_cases.npz")


@pytest.fixture(scope="module")
def fixture():
    return R.load_cases(FIXTURE)


def _flat(c, b):
    """sample b of a case as ops.refexp_group takes it: logits [Q,K], boxes [Q,4], masks [Q,h,w] on the GPU"""
    return (c["logits"][b].flatten(0, 1).contiguous().cuda(), c["boxes"][b].flatten(0, 1).contiguous().cuda(),
            c["masks"][b].flatten(0, 1).contiguous().cuda())


@pytest.fixture(scope="module")
def ran(fixture):
    """Every case through one ops.refexp_group call: computed once, shared, never modified"""
    from tce_rvos_amd import ops
    out = {}
    for c in fixture[0]:
        flat = [_flat(c, b) for b in range(c["B"])]
        res = ops.refexp_group([f[0] for f in flat], [f[1] for f in flat], [f[2] for f in flat], c["sizes"], c["origs"],
                               threshold=c["threshold"])
        torch.cuda.synchronize()
        out[c["name"]] = (flat, res)
    return out


@pytest.mark.parametrize("name", [c[0] for c in R.CASES])
def test_fixture_cases_against_the_reference_classes(fixture, ran, name):
    c = next(c for c in fixture[0] if c["name"] == name)
    _, (scores, order, boxes, masks) = ran[name]
    Q = c["T"] * c["N"]
    for b in range(c["B"]):
        assert order[b].dtype == torch.int32 and scores[b].dtype == torch.float32 and boxes[b].dtype == torch.float32
        assert tuple(order[b].shape) == (Q,) and tuple(boxes[b].shape) == (Q, 4) and tuple(masks[b].shape) == (Q,) + tuple(c["origs"][b])
        err = float((scores[b].cpu() - c["scores"][b]).abs().max())
        print(f"{name}[{b}]: order {order[b].tolist()} max|score diff| {err:.3e}")
        assert order[b].cpu().tolist() == c["order"][b].tolist()     # topk_indexes, exactly
        assert err <= 1e-6
        assert torch.equal(boxes[b].cpu(), c["boxes_out"][b])         # bit-equal
        _a2d.check_masks(masks[b], c["ref"][b], c["contested"][b], f"{name}[{b}]")
        if name in R.EXACT:
            assert not bool(c["contested"][b].any()) and torch.equal(masks[b].cpu(), c["ref"][b])


def test_masks_equal_the_per_sample_entry_on_the_gathered_planes(fixture, ran):
    from tce_rvos_amd import ops
    for c in fixture[0]:
        flat, (_, order, _, masks) = ran[c["name"]]
        for b in range(c["B"]):
            planes = flat[b][2][(order[b] // c["K"]).long()].contiguous()
            want = ops.a2d_masks(planes, c["sizes"][b], c["origs"][b], threshold=c["threshold"])
            assert torch.equal(masks[b], want), (c["name"], b)
    c = fixture[0][2]                                                 # the threshold given is used: 0.35 is not 0.5
    flat, (_, order, _, masks) = ran[c["name"]]
    planes = flat[0][2][(order[0] // c["K"]).long()].contiguous()
    assert not torch.equal(masks[0], ops.a2d_masks(planes, c["sizes"][0], c["origs"][0], threshold=0.5))


def _table(rows):
    t = (_lib.RefexpSample * len(rows))()
    for e, r in zip(t, rows):
        for k, v in r.items():
            setattr(e, k, v)
    return t


def _call(t, B, Q, K, h, w, thr=0.5):
    return _lib.lib().tce_refexp_group_u8(t, B, Q, K, h, w, thr, torch.cuda.current_stream().cuda_stream)


def test_box_only_call_leaves_out_untouched(fixture, ran):
    from tce_rvos_amd import ops
    c = fixture[0][0]
    flat, (scores, order, boxes, masks) = ran[c["name"]]
    s2, o2, b2, m2 = ops.refexp_group([flat[0][0]], [flat[0][1]], None, None, c["origs"])
    torch.cuda.synchronize()
    assert m2 is None and torch.equal(s2[0], scores[0]) and torch.equal(o2[0], order[0]) and torch.equal(b2[0], boxes[0])
    # the table itself: masks = NULL beside a canary-filled out
    Q, (H0, W0) = 5, c["origs"][0]
    canary = torch.full((Q * H0 * W0,), 0xEE, dtype=torch.uint8, device="cuda")
    sc, od, bo = torch.empty(Q, device="cuda"), torch.empty(Q, dtype=torch.int32, device="cuda"), torch.empty(Q, 4, device="cuda")
    t = _table([dict(logits=flat[0][0].data_ptr(), boxes_in=flat[0][1].data_ptr(), masks=None, scores=sc.data_ptr(), order=od.data_ptr(),
                     boxes_out=bo.data_ptr(), out=canary.data_ptr(), fh=72, fw=100, H0=H0, W0=W0)])
    assert _call(t, 1, Q, 1, 18, 25) == 0
    torch.cuda.synchronize()
    assert bool((canary == 0xEE).all()) and torch.equal(sc, scores[0]) and torch.equal(od, order[0]) and torch.equal(bo, boxes[0])


def test_ties_go_to_the_lower_flat_index():
    from tce_rvos_amd import ops
    one = torch.tensor([0.5, 2.0, 0.5, -200.0, 2.0, 40.0, 45.0, 50.0, -3.0, -100.0]).view(-1, 1)    # K = 1
    bx = (torch.arange(40, dtype=torch.float32).view(10, 4) + 1) / 64
    s, o, b, _ = ops.refexp_group([one.cuda()], [bx.cuda()], None, None, [(64, 128)])
    torch.cuda.synchronize()
    want = [5, 6, 7, 1, 4, 0, 2, 8, 3, 9]      # 40, 45, 50 saturate to 1; equal logits; -200 and -100 both give 0
    assert o[0].tolist() == want
    sc = s[0].tolist()
    assert sc[:3] == [1.0, 1.0, 1.0] and sc[3] == sc[4] and sc[5] == sc[6] and sc[8:] == [0.0, 0.0] and sc == sorted(sc, reverse=True)
    cx, cy, w, h = bx[want].unbind(1)
    assert torch.equal(b[0].cpu(), torch.stack([(cx - 0.5 * w) * 128, (cy - 0.5 * h) * 64, (cx + 0.5 * w) * 128, (cy + 0.5 * h) * 64], 1))
    two = torch.tensor([[3.0, 3.0], [-40.0, -41.0], [3.0, 0.0], [40.0, 40.0]])                       # K = 2: [Q = 4, K]
    s, o, b, _ = ops.refexp_group([two.cuda()], [bx[:4].contiguous().cuda()], None, None, [(64, 128)])
    torch.cuda.synchronize()
    assert o[0].tolist() == [6, 7, 0, 1]
    cx, cy, w, h = bx[[3, 3, 0, 0]].unbind(1)   # the candidates' queries: flat index // K
    assert torch.equal(b[0].cpu(), torch.stack([(cx - 0.5 * w) * 128, (cy - 0.5 * h) * 64, (cx + 0.5 * w) * 128, (cy + 0.5 * h) * 64], 1))
    nan = torch.tensor([0.5, float("nan"), 2.0, float("nan")]).view(-1, 1)   # NaN first, by index: every rank is still written
    s, o, _, _ = ops.refexp_group([nan.cuda()], [bx[:4].contiguous().cuda()], None, None, [(64, 128)])
    assert o[0].tolist() == [1, 3, 2, 0]


@pytest.mark.parametrize("Q,K", [(1024, 1), (512, 2)])
def test_the_candidate_cap_runs(Q, K):
    from tce_rvos_amd import ops
    g = torch.Generator().manual_seed(Q + K)
    lg = torch.randn(Q, K, generator=g) * 3
    lg.view(-1)[[5, 900, 17]] = float(lg.view(-1)[3])                 # some exact ties among the candidates
    lg = lg.cuda()
    bx = (torch.rand(Q, 4, generator=g) * 0.5 + 0.1).cuda()
    pm = torch.randn(Q, 3, 4, generator=g).cuda()
    s, o, b, m = ops.refexp_group([lg], [bx], [pm], [(9, 13)], [(5, 7)])
    torch.cuda.synchronize()
    p = ops.sigmoid(lg.view(-1).contiguous()).cpu().numpy()
    want = np.lexsort((np.arange(Q * K), -p.astype(np.float64)))[:Q]  # descending value, then ascending index
    assert o[0].cpu().numpy().tolist() == want.tolist()
    assert np.array_equal(s[0].cpu().numpy(), p[want])
    assert torch.equal(m[0], ops.a2d_masks(pm[(o[0] // K).long()].contiguous(), (9, 13), (5, 7)))
    cx, cy, w, h = bx[(o[0] // K).long()].cpu().unbind(1)
    assert torch.equal(b[0].cpu(), torch.stack([(cx - 0.5 * w) * 7, (cy - 0.5 * h) * 5, (cx + 0.5 * w) * 7, (cy + 0.5 * h) * 5], 1))


def test_one_candidate_more_than_the_cap_is_rejected_and_nothing_is_launched():
    from tce_rvos_amd import ops
    Q = 1025
    lg, bx, pm = torch.zeros(Q, 1, device="cuda"), torch.zeros(Q, 4, device="cuda"), torch.zeros(Q, 3, 4, device="cuda")
    with pytest.raises(ValueError, match="candidates"):
        ops.refexp_group([lg], [bx], [pm], [(9, 13)], [(5, 7)])
    bufs = [torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda") for n in (Q * 4, Q * 4, Q * 16, Q * 35)]
    t = _table([dict(logits=lg.data_ptr(), boxes_in=bx.data_ptr(), masks=pm.data_ptr(), scores=bufs[0].data_ptr(),
                     order=bufs[1].data_ptr(), boxes_out=bufs[2].data_ptr(), out=bufs[3].data_ptr(), fh=9, fw=13, H0=5, W0=7)])
    assert _call(t, 1, Q, 1, 3, 4) < 0 and b"1025" in _lib.lib().tce_last_error()   # a return code, not a launch
    torch.cuda.synchronize()
    assert all(bool((x == 0xEE).all()) for x in bufs)


def test_seventeen_samples_equal_seventeen_single_calls():
    from tce_rvos_amd import ops
    B, Q, K, hw = ops.REFEXP_GROUP_MAX + 1, 3, 2, (3, 4)
    ins = [R.make_inputs(300 + b, 1, 1, Q, K, hw, "noise", 1.0) for b in range(B)]
    lg = [i[0][0, 0].contiguous().cuda() for i in ins]
    bx = [i[1][0, 0].contiguous().cuda() for i in ins]
    pm = [i[2][0, 0].contiguous().cuda() for i in ins]
    origs = [(5 + b % 3, 7 + b % 4) for b in range(B)]
    sizes = [(9 + b % 4, 13 + b % 3) for b in range(B)]
    n16 = Q * origs[16][0] * origs[16][1]
    raw = torch.full((n16 + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    shift = (3 - raw.data_ptr()) % 4
    odd = raw[shift:shift + n16].view(Q, *origs[16])
    assert odd.data_ptr() % 4 == 3
    s, o, bo, m = ops.refexp_group(lg, bx, pm, sizes, origs, outs=[None] * 16 + [odd])
    torch.cuda.synchronize()
    assert len(s) == len(o) == len(bo) == len(m) == B and m[16].data_ptr() == odd.data_ptr()
    for b in range(B):
        s1, o1, b1, m1 = ops.refexp_group([lg[b]], [bx[b]], [pm[b]], [sizes[b]], [origs[b]])
        assert torch.equal(s[b], s1[0]) and torch.equal(o[b], o1[0]) and torch.equal(bo[b], b1[0]) and torch.equal(m[b], m1[0]), b
    assert bool((raw[:shift] == 0xEE).all()) and bool((raw[shift + n16:] == 0xEE).all())


# ----------------------------------------------------------------------------------------------------------- the classes
def _outputs(c):
    return {"pred_logits": c["logits"].cuda(), "pred_boxes": c["boxes"].cuda(), "pred_masks": c["masks"].cuda()}


def test_post_processors_and_the_marker(fixture, ran):
    from tce_rvos_amd.postprocess import PostProcess, PostProcessSegm
    c = fixture[0][3]                                                 # the batch of two
    outputs = _outputs(c)
    _, (scores, order, boxes, masks) = ran[c["name"]]
    with hazard.recording() as rec1:
        results = PostProcess()(outputs, torch.tensor(c["origs"]))
    with hazard.recording() as rec2:
        results = PostProcessSegm(threshold=c["threshold"])(results, outputs, torch.tensor(c["origs"]), torch.tensor(c["sizes"]))
    torch.cuda.synchronize()
    assert [x.name for x in rec1.launches] == ["tce_refexp_group_u8"] == [x.name for x in rec2.launches]
    assert rec1.analyse().clean and rec2.analyse().clean
    Q = c["T"] * c["N"]
    assert len(results) == 2
    for b, r in enumerate(results):
        assert set(r) == {"scores", "labels", "boxes", "masks"}
        assert r["labels"].dtype == torch.int64 and r["labels"].tolist() == [1] * Q and r["labels"].is_cuda
        assert torch.equal(r["scores"], scores[b]) and torch.equal(r["boxes"], boxes[b])
        assert r["masks"].dtype == torch.uint8 and tuple(r["masks"].shape) == (Q, 1) + tuple(c["origs"][b])
        assert torch.equal(r["masks"][:, 0], masks[b])
        # the second call was the ranked one: it read this result's order and wrote no scores
        lo = r._refexp[1].data_ptr()
        assert hazard.overlap(rec2.launches[0].reads, hazard.dense(lo, Q * 4)) is not None
        assert hazard.overlap(rec2.launches[0].writes, hazard.dense(lo, Q * 4)) is None
        assert hazard.overlap(rec2.launches[0].writes, hazard.dense(r["scores"].data_ptr(), Q * 4)) is None
    # any other results take the full call (ranking and masks) and keep their keys
    plain = [{"scores": r["scores"], "labels": r["labels"], "boxes": r["boxes"], "mine": 7} for r in results]
    with hazard.recording() as rec3:
        plain = PostProcessSegm(threshold=c["threshold"])(plain, outputs, c["origs"], c["sizes"])
    torch.cuda.synchronize()
    assert [x.name for x in rec3.launches] == ["tce_refexp_group_u8"]
    assert len(rec3.launches[0].writes) > len(rec2.launches[0].writes)
    for b, r in enumerate(plain):
        assert set(r) == {"scores", "labels", "boxes", "masks", "mine"} and torch.equal(r["masks"][:, 0], masks[b])
    # a list of dicts (what forward_group returns), samples of other shapes in between; both classes in one call
    c1 = fixture[0][0]
    lst = [{k: v[:1] for k, v in outputs.items()}, _outputs(c1), {k: v[1:] for k, v in outputs.items()}]
    origs, sizes = [c["origs"][0], c1["origs"][0], c["origs"][1]], [c["sizes"][0], c1["sizes"][0], c["sizes"][1]]
    both = PostProcessSegm(threshold=0.5).with_boxes(lst, origs, sizes)
    torch.cuda.synchronize()
    assert torch.equal(both[0]["masks"][:, 0], masks[0]) and torch.equal(both[2]["masks"][:, 0], masks[1])
    assert torch.equal(both[1]["masks"][:, 0], ran["c1"][1][3][0]) and torch.equal(both[1]["boxes"], ran["c1"][1][2][0])
    assert torch.equal(both[2]["scores"], scores[1])


# ------------------------------------------------------------------------------------------------------------------ GIoU
def _xyxy(gt):
    return [gt[0], gt[1], gt[2] + gt[0], gt[3] + gt[1]]


def test_giou_and_hits_against_the_reference(fixture):
    from tce_rvos_amd import ops
    from tce_rvos_amd.refexp_score import RefExpScorer, hits
    cases, syn, summary = fixture
    boxes = syn["boxes"].cuda()
    gt = torch.tensor([_xyxy(g) for g in syn["gt"]], dtype=torch.float64).to(torch.float32).cuda()
    giou, best = ops.refexp_giou(boxes, gt)
    torch.cuda.synchronize()
    err = float((giou.cpu() - syn["giou"]).abs().max())
    print(f"synthetic set: max|giou diff| {err:.3e}")
    assert err <= 2e-6
    assert torch.equal(best.cpu(), torch.cummax(giou, 1).values.cpu())
    for m in range(len(syn["gt"])):
        assert hits(best[m].cpu().numpy(), R.K_AT, 0.5) == syn["hits"][m], m
    # the scorer over every image of the fixture: the cases' own boxes first, then the synthetic set
    scorer, k = RefExpScorer(), 0
    for c in cases:
        res, tg = {}, {}
        for b in range(c["B"]):
            res[k] = {"scores": c["scores"][b].cuda(), "boxes": c["boxes_out"][b].cuda()}
            tg[k] = {"bbox": c["gt"][b], "dataset_name": c["dataset"][b]}
            k += 1
        scorer.update(res, tg)
    res = {k + m: {"scores": syn["scores"][m].cuda(), "boxes": boxes[m]} for m in range(len(syn["gt"]))}
    tg = {k + m: [{"bbox": syn["gt"][m], "dataset_name": syn["dataset"][m]}] for m in range(len(syn["gt"]))}
    scorer.update(res, tg)
    with pytest.raises(ValueError, match="scored already"):
        scorer.update({0: res[k]}, {0: tg[k]})
    st = scorer.state()
    assert st["image_ids"] == list(range(k + len(syn["gt"]))) and len(st["best"]) == len(st["datasets"]) == len(st["image_ids"])
    at = 0
    for c in cases:
        for b in range(c["B"]):
            got = np.asarray(st["best"][at], dtype=np.float32)
            assert float(np.abs(got - np.maximum.accumulate(c["giou"][b].numpy())).max()) <= 2e-6
            assert hits(got, R.K_AT, 0.5) == c["hits"][b], (c["name"], b)
            at += 1
    got = scorer.summarize()
    for d in R.DATASETS:
        assert np.allclose(got[d], summary[d], rtol=0, atol=1e-12), (d, got[d], summary[d])
    # results that are not PostProcess' own are put in score order first
    perm = torch.tensor([3, 0, 6, 1, 5, 2, 4])
    other = RefExpScorer()
    other.update({0: {"scores": syn["scores"][0][perm].cuda(), "boxes": boxes[0][perm.cuda()]}}, {0: tg[k]})
    assert other.state()["best"][0] == st["best"][k]


# ------------------------------------------------------------------------------------------------------------- footprint
@pytest.fixture(scope="module")
def slab():
    s = fp.Slab(32 << 20, device="cuda")
    yield s
    del s
    torch.cuda.empty_cache()


def _group_case(S, Q, K, h, w, samples, ranked=False):
    """samples: per sample (fh, fw, H0, W0, the bytes `out` starts into its buffer).  Every device buffer of the call in the slab; the
    table is a host array, read by the entry point at the call: it stays outside the slab."""
    B = len(samples)
    rows = []
    for b, (fh, fw, H0, W0, shift) in enumerate(samples):
        pm = S.randn(f"masks{b}", (Q * h * w,), scale=3.0)
        raw = S.alloc(f"out{b}", (shift + Q * H0 * W0 + 3,), dtype=torch.uint8)
        row = dict(masks=pm.data_ptr(), out=raw.data_ptr() + shift, fh=fh, fw=fw, H0=H0, W0=W0)
        if ranked:
            g = torch.Generator().manual_seed(b)
            row["order"] = S.put(f"order{b}", torch.randperm(Q * K, generator=g)[:Q].to(torch.int32)).data_ptr()
        else:
            row.update(logits=S.randn(f"logits{b}", (Q * K,), scale=2.0).data_ptr(), boxes_in=S.rand(f"boxes{b}", (Q * 4,)).data_ptr(),
                       scores=S.alloc(f"scores{b}", (Q,)).data_ptr(), order=S.alloc(f"order{b}", (Q,), dtype=torch.int32).data_ptr(),
                       boxes_out=S.alloc(f"boxes_out{b}", (Q * 4,)).data_ptr())
        rows.append(row)
    table = _table(rows)

    def fn():
        _lib.check(_lib.lib().tce_refexp_group_u8(table, B, Q, K, h, w, 0.5, torch.cuda.current_stream().cuda_stream),
                   "tce_refexp_group_u8")
    return fn


GROUP_FOOTPRINT = [
    # the second sample's planes of 6 x 20 x 30 = 3600 bytes take more than one 1024-byte workgroup
    ("two_samples_6x2_candidates_addresses_1_and_2", dict(Q=6, K=2, h=4, w=6, samples=[(13, 20, 9, 11, 1), (16, 24, 20, 30, 2)])),
    ("ranked_two_samples_addresses_3_and_0", dict(Q=6, K=2, h=4, w=6, samples=[(13, 20, 9, 11, 3), (16, 24, 20, 30, 0)], ranked=True)),
]


@pytest.mark.parametrize("tag,kw", GROUP_FOOTPRINT, ids=[c[0] for c in GROUP_FOOTPRINT])
def test_refexp_group_footprint(slab, tag, kw):
    """W, O and R of tests/_footprint.py, no exemptions"""
    info = fp.check_case(slab, lambda S: _group_case(S, **kw), fp.recorder("tce_refexp_group_u8"), props="WOR",
                         sync=torch.cuda.synchronize, label=tag)
    print(f"{tag}: read {info['read_bytes']} written {info['written_bytes']} guard {info['guard_bytes']} untouched-in-buffers {info['pad_bytes']}")
    assert (info["W"], info["O"], info["R"]) == (2, 2, 3) and info["exempt"] == []
    Q, K, h, w, samples = kw["Q"], kw["K"], kw["h"], kw["w"], kw["samples"]
    per = Q * 4 if kw.get("ranked") else (Q * K + Q * 4) * 4
    assert info["read_bytes"] == len(samples) * (Q * h * w * 4 + per)
    assert info["written_bytes"] == sum(Q * s[2] * s[3] + (0 if kw.get("ranked") else Q * 24) for s in samples)


def test_refexp_giou_footprint(slab):
    M, Q = 3, 300                                                     # more boxes than a workgroup has threads

    def build(S):
        xy = S.rand("xy", (M * Q * 2,), 0.0, 50.0)
        wh = S.rand("wh", (M * Q * 2,), 1.0, 40.0)
        boxes = S.alloc("boxes", (M * Q, 4))
        boxes.copy_(torch.cat([xy.view(-1, 2), xy.view(-1, 2) + wh.view(-1, 2)], 1))
        gt = S.put("gt", torch.tensor([[10.0, 10.0, 40.0, 50.0], [0.0, 5.0, 80.0, 20.0], [30.0, 30.0, 31.0, 31.0]]).view(-1))
        giou, best = S.alloc("giou", (M * Q,)), S.alloc("best", (M * Q,))

        def fn():
            _lib.check(_lib.lib().tce_refexp_giou_f32(boxes.data_ptr(), gt.data_ptr(), giou.data_ptr(), best.data_ptr(), M, Q,
                                                      torch.cuda.current_stream().cuda_stream), "tce_refexp_giou_f32")
        return fn
    info = fp.check_case(slab, build, fp.recorder("tce_refexp_giou_f32"), props="WOR", sync=torch.cuda.synchronize, label="giou_3x300")
    assert (info["W"], info["O"], info["R"]) == (2, 2, 3) and info["exempt"] == []
    assert info["read_bytes"] == M * Q * 16 + M * 16 and info["written_bytes"] == 2 * M * Q * 4


# ------------------------------------------------------------------------------------------------------------- end to end
E2E_MAX_SHARE = 1e-2   # of pixels whose bit may hang on the group round-off: more and the rule could hide a failure


def _e2e_bounds(solo, H0, W0):
    """The group bound tol(ref) = 2e-5 * max|ref| + 1e-6 on the forward's outputs, carried through the stage: the sigmoid's slope
    is at most 1/4 (plus the 1e-6 its own evaluation is held to); a box coordinate is (c +- w/2) * extent: 1.5 tol times the extent
    plus an fp32 rounding of the result; a mask logit is a convex combination of plane values, so it moves by at most tol."""
    def tol(t):
        return 2e-5 * float(t.abs().max()) + 1e-6
    ext = float(max(H0, W0))
    return 0.25 * tol(solo["pred_logits"]) + 1e-6, 1.5 * tol(solo["pred_boxes"]) * ext + ext * 2.0 ** -22, tol(solo["pred_masks"])


def test_run_images_end_to_end():
    import argparse
    from tce_rvos_amd import build_model, build_refexp_postprocessors, load_synth_weights
    from tce_rvos_amd.a2d_score import A2DScorer
    from tce_rvos_amd.refexp import run_images
    from tce_rvos_amd.refexp_score import RefExpScorer
    model, _, _ = build_model(argparse.Namespace(backbone="resnet50", with_box_refine=True, binary=True, freeze_text_encoder=True,
                                                 f_token=8, qtrans=True, num_feature_levels=4, text_encoder_layers=1))
    model = model.cuda().eval()
    load_synth_weights(model, 31)
    model.repack()
    H, W, L, thr = 96, 128, 9, 0.5
    g = torch.Generator().manual_seed(70)
    ids = torch.randint(3, 50000, (3, L), generator=g)
    origs = [(120, 161), (77, 100), (96, 128)]
    samples = []
    for i in range(3):
        x0, y0 = 10.0 + 20 * i, 8.0 + 5 * i
        samples.append({"image": synth_frames(1, H, W, 70 + i)[0].cuda(), "caption": ids[i:i + 1], "size": (H, W), "orig_size": origs[i],
                        "image_id": 100 + i, "target": {"bbox": [x0, y0, 60.0, 50.0], "dataset_name": R.DATASETS[i]}})
    gt_masks = {}
    for i, (H0, W0) in enumerate(origs):
        m = np.zeros((H0, W0), dtype=np.uint8)
        m[8 + 5 * i:58 + 5 * i, 10 + 20 * i:70 + 20 * i] = 1
        gt_masks[100 + i] = {"size": [H0, W0], "counts": _a2d.rle_counts(m)}
    post = build_refexp_postprocessors(argparse.Namespace(masks=True, threshold=thr))
    # the one-image path: forward, then the two classes, per image
    solo, solo_out = [], []
    for s in samples:
        out = model([s["image"][None]], s["caption"], [{"size": torch.tensor([H, W])}])
        out = {k: out[k].clone() for k in ("pred_logits", "pred_boxes", "pred_masks")}
        r = post["bbox"](out, [s["orig_size"]])
        r = post["segm"](r, out, [s["orig_size"]], [s["size"]])
        solo.append(r[0])
        solo_out.append(out)
    runs = []
    for _ in range(3):                                                # eager, capture, replay
        scorer, mask_scorer = RefExpScorer(), A2DScorer(gt_masks)
        res = run_images(model, samples, post, max_group=2, scorer=scorer, mask_scorer=mask_scorer)
        torch.cuda.synchronize()
        runs.append((res, scorer, mask_scorer))
    res, scorer, mask_scorer = runs[0]
    assert list(res) == [100, 101, 102]
    for i, s in enumerate(samples):
        r, w, out = res[100 + i], solo[i], solo_out[i]
        H0, W0 = origs[i]
        Q = int(w["scores"].shape[0])
        b_s, b_b, b_m = _e2e_bounds(out, H0, W0)
        gap = float((w["scores"][:-1] - w["scores"][1:]).min())
        e_s, e_b = float((r["scores"] - w["scores"]).abs().max()), float((r["boxes"] - w["boxes"]).abs().max())
        print(f"image {i}: score gap {gap:.3e}; max|score diff| {e_s:.3e} (bound {b_s:.3e}); max|box diff| {e_b:.3e} (bound {b_b:.3e})")
        assert gap > 2 * b_s, "the synthetic scores are too close for the order to be compared"
        assert torch.equal(r._refexp[1], w._refexp[1])                # the same ranking
        assert e_s <= b_s and e_b <= b_b
        assert r["labels"].tolist() == [1] * Q and tuple(r["masks"].shape) == (Q, 1, H0, W0) and r["masks"].dtype == torch.uint8
        planes = out["pred_masks"][0].flatten(0, 1)[(w._refexp[1] // 1).long()].cpu()
        ref, v = _a2d.reference_post(planes, (H, W), (H0, W0), threshold=thr)
        cont = (v - _a2d.logit(thr)).abs() <= b_m + _a2d.V_EPS
        share = float(cont.float().mean())
        bad = (r["masks"][:, 0].cpu() != w["masks"][:, 0].cpu()) & ~cont
        print(f"image {i}: contested share {share:.3e} (mask logit bound {b_m:.3e}), mismatches outside {int(bad.sum())}")
        assert share <= E2E_MAX_SHARE and not bool(bad.any())
        for other in runs[1:]:                                        # capture and replay give the eager pass' results
            for k in ("scores", "boxes", "masks"):
                assert torch.equal(other[0][100 + i][k], r[k]), (i, k)
    # the scorers fed by run_images against the same results fed by hand
    hand, hand_masks = RefExpScorer(), A2DScorer(gt_masks)
    for s in samples:
        hand.update({s["image_id"]: res[s["image_id"]]}, {s["image_id"]: s["target"]})
        hand_masks.update([s["image_id"]], [res[s["image_id"]]])
    assert scorer.state() == hand.state() and scorer.summarize() == hand.summarize()
    assert mask_scorer.summarize() == hand_masks.summarize()
    assert set(scorer.summarize()) == set(R.DATASETS) and scorer.state()["image_ids"] == [100, 101, 102]
    # one more call, recorded (graph replays by now): no unordered conflicting pair
    sd = model._text_plan().sd
    with hazard.recording(tables=[sd["embeddings.word_embeddings.weight"], sd["embeddings.position_embeddings.weight"]]) as rec:
        again = run_images(model, samples, post, max_group=2, scorer=RefExpScorer(), mask_scorer=A2DScorer(gt_masks))
    torch.cuda.synchronize()
    rep = rec.analyse()
    names = [x.name for x in rec.launches]
    print(rep)
    assert rep.clean and names.count("tce_refexp_group_u8") == 2 and names.count("tce_refexp_giou_f32") == 2
    assert torch.equal(again[101]["masks"], res[101]["masks"])
